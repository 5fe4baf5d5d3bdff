"""The fused rollout policy's sampling stream, restated in numpy / float64.

An independent statement of what `policy_kernel` (csrc/gr_policy.hip) and `policy_f32_kernel`
(csrc/gr_policy_f32.hip) draw: one Philox4x32-10 block (Salmon et al., SC'11) per env with counter
(global env id, call counter, tag "POL!", 0) and key (seed low word, seed high word); Box-Muller on words
(x, y) gives action rows 0 and 1 (cos, sin), on words (z, w) rows 2 and 3.  numpy only: nothing from the
product or the oracle is imported, so a test that compares with it compares two separate statements.
"""
from __future__ import annotations

import numpy as np

TAG_POLICY = 0x504F4C21
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counters (c0, c1, c2, c3) and keys (k0, k1), broadcast against each other
    -> uint32 [..., 4] (words x, y, z, w)."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) & _MASK
                                                   for v in (c0, c1, c2, c3, k0, k1)))
    for i in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64 bits: exact in uint64
        r0 = (k0 + np.uint64(i * _W0 & 0xFFFFFFFF)) & _MASK
        r1 = (k1 + np.uint64(i * _W1 & 0xFFFFFFFF)) & _MASK
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ r0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ r1, p0 & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def policy_words(seed, env_ids, counter):
    """The Philox block of global env ids `env_ids` at call counter `counter` -> uint32 [..., 4]."""
    seed = int(seed)
    return philox4x32_10(env_ids, counter, TAG_POLICY, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def policy_normals(seed, env_ids, counter):
    """The standard normals of action rows 0..3 -> float64 [..., 4]."""
    w = policy_words(seed, env_ids, counter)
    n = (w >> np.uint32(8)).astype(np.float64)
    z = np.empty(w.shape, np.float64)
    for pair in (0, 1):
        u1 = (n[..., 2 * pair] + 1.0) / 2.0**24  # (0, 1]
        u2 = n[..., 2 * pair + 1] / 2.0**24      # [0, 1)
        rad = np.sqrt(-2.0 * np.log(u1))
        z[..., 2 * pair] = rad * np.cos(2.0 * np.pi * u2)
        z[..., 2 * pair + 1] = rad * np.sin(2.0 * np.pi * u2)
    return z


def log_prob(z, std):
    """sum over the action rows of Normal(mean, std).log_prob(mean + std z), float64; z [..., k], std [k]."""
    z, std = np.asarray(z, np.float64), np.asarray(std, np.float64)
    return (-0.5 * z * z - np.log(std) - 0.5 * np.log(2.0 * np.pi)).sum(-1)
