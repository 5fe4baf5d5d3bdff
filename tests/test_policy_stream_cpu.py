"""The float64 restatement of the fused policy's sampling stream (tests/policy_stream_ref.py), checked on the
CPU: against the Random123 known answers, against gr_rng.h through the oracle, and as a standard normal
stream (so the GPU tests that compare the kernels with it compare with something that is itself right).

Statistical limits, at seed 3, envs 0..65 552, counters 0..7 (N = 524 424 draws per action row): means within
5 / sqrt(N) and stds within 5 / sqrt(2 N) (5 standard errors), Kolmogorov-Smirnov p > 1e-3 per row, every
correlation (across rows, lag 1 over counters, lag 1 over envs) within 5 / sqrt(N) = 6.9e-3.  Measured:
KS p 0.61, 0.14, 0.34, 0.50; largest cross-row correlation 3.0e-3; lag-1 correlations <= 1.4e-3."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import oracle
from policy_stream_ref import TAG_POLICY, philox4x32_10, policy_normals, policy_words

SEED, ENVS, COUNTERS = 3, 65553, 8

# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, expected words)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]

# (seed-3, counter-0 env id, word index, top 24 bits): the ends of Box-Muller's radius, found by a scan of the
# env ids below 2^27.  u1 = (top + 1) / 2^24: top 0 is the largest radius sqrt(48 ln 2), top 0xFFFFFF radius 0.
EDGES = [(278116, 0, 0), (11769317, 2, 0), (71469791, 0, 0xFFFFFF), (20978160, 2, 0xFFFFFF)]


def test_known_answers():
    for ctr, key, want in KAT:
        assert tuple(int(v) for v in philox4x32_10(*ctr, *key)) == want
    # and vectorised, the three at once
    c = np.array([k[0] for k in KAT], np.uint64)
    k = np.array([k[1] for k in KAT], np.uint64)
    got = philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1])
    assert got.dtype == np.uint32 and got.tolist() == [list(k[2]) for k in KAT]


def test_matches_gr_rng_through_the_oracle():
    rng = np.random.default_rng(11)
    runs, n = 512, 8  # 4 096 blocks: 512 random (counter, key) pairs, 8 consecutive c0 each (c0 may wrap)
    v = rng.integers(0, 2**32, size=(runs, 6), dtype=np.uint64)
    v[0, 0] = 0xFFFFFFFC  # c0 + i wraps past 2^32 inside the run
    for r in range(runs):
        c0, c1, c2, c3, k0, k1 = (int(x) for x in v[r])
        want = oracle.test_philox(n, c0, c1, c2, c3, k0, k1)
        got = philox4x32_10((c0 + np.arange(n)) & 0xFFFFFFFF, c1, c2, c3, k0, k1)
        assert np.array_equal(got, want), r
    # the policy's own counter layout and key split
    seed = 0x9E3779B97F4A7C15
    want = oracle.test_philox(100, 5000, 7, TAG_POLICY, 0, seed & 0xFFFFFFFF, seed >> 32)
    assert np.array_equal(policy_words(seed, 5000 + np.arange(100), 7), want)


@pytest.fixture(scope="module")
def stream():
    z = policy_normals(SEED, np.arange(ENVS)[:, None], np.arange(COUNTERS)[None, :])  # [env, counter, row]
    assert z.shape == (ENVS, COUNTERS, 4) and z.dtype == np.float64
    z.setflags(write=False)
    return z


def _ks_p(x):
    """Kolmogorov-Smirnov against N(0, 1): the asymptotic p value (Stephens' small-sample correction)."""
    x = np.sort(x)
    n = x.size
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(x / math.sqrt(2.0))).numpy())
    i = np.arange(1, n + 1)
    d = max(float((i / n - cdf).max()), float((cdf - (i - 1) / n).max()))
    lam = (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)) * d
    return min(1.0, max(0.0, 2.0 * sum((-1) ** (k - 1) * math.exp(-2.0 * k * k * lam * lam) for k in range(1, 101))))


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def test_stream_moments_and_ks(stream):
    n = ENVS * COUNTERS
    for g in range(4):
        x = stream[:, :, g].ravel()
        mean, std, p = float(x.mean()), float(x.std()), _ks_p(x)
        print(f"row {g}: mean {mean:+.2e} std-1 {std - 1:+.2e} KS p {p:.2f}")
        assert abs(mean) < 5.0 / math.sqrt(n)
        assert abs(std - 1.0) < 5.0 / math.sqrt(2 * n)
        assert p > 1e-3
    assert np.isfinite(stream).all() and float(np.abs(stream).max()) <= math.sqrt(48.0 * math.log(2.0))


def test_stream_correlations(stream):
    tol = 5.0 / math.sqrt(ENVS * COUNTERS)
    cross = [abs(_corr(stream[:, :, a], stream[:, :, b])) for a in range(4) for b in range(a + 1, 4)]
    lag_t = [abs(_corr(stream[:, :-1, g], stream[:, 1:, g])) for g in range(4)]
    lag_e = [abs(_corr(stream[:-1, :, g], stream[1:, :, g])) for g in range(4)]
    # rows of a later call against other rows of this one, and of the next env: a pair reused across calls or envs
    lag_tx = [abs(_corr(stream[:, :-1, a], stream[:, 1:, b])) for a in range(4) for b in range(4) if a != b]
    lag_ex = [abs(_corr(stream[:-1, :, a], stream[1:, :, b])) for a in range(4) for b in range(4) if a != b]
    print(f"cross-row {max(cross):.1e} lag-1 counters {max(lag_t):.1e} envs {max(lag_e):.1e} "
          f"cross lag-1 counters {max(lag_tx):.1e} envs {max(lag_ex):.1e} (limit {tol:.1e})")
    assert max(cross) < tol
    assert max(lag_t) < tol and max(lag_e) < tol
    assert max(lag_tx) < tol and max(lag_ex) < tol


def test_edge_env_ids():
    for env, word, top in EDGES:
        w = policy_words(SEED, env, 0)
        assert int(w[word]) >> 8 == top, (env, word, hex(int(w[word])))
        z = policy_normals(SEED, env, 0)
        rows = z[word:word + 2]
        if top == 0:  # u1 = 2^-24: the largest radius
            assert abs(math.hypot(*rows) - math.sqrt(48.0 * math.log(2.0))) < 1e-12
        else:  # u1 = 1: both rows exactly zero
            assert np.all(rows == 0.0)
