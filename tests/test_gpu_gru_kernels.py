"""The fused GRU memory (gr_gru_step / gr_gru_seq_forward / gr_gru_seq_backward, csrc/gr_gru.hip; rsl_rl/fused_gru.py)
against the float64 restatement of the masked sequence (tests/recurrent_ref.py: torch.nn.GRU on the CPU, stepped with
the mask), fed the op's own inputs, upcast.

Bound: per case and per tensor, torch's own fp32 GRU (the same restatement in float32 on the CPU) is measured against
float64 at run time, and the fused op must stay within max(1e-5, 4 x that error) of the tensor's norm; the 4 covers
a different summation order and the non-libm tanh, nothing else.  The measured figures of an MI355X run are in
profiles/gru_error_budget.json.

Cases (T, B, R, D): a single step and row; a partial 16-env tile with D no multiple of 4; 48 envs = three workgroup
tiles (the env tile is 16); the recipe's size over 24 steps with a partial tile; the largest instantiation with the
widest input.  dones: the golden fixture's pattern scaled to T, row 0 never done, the last row done at every step.
x and dones are blocks of wider buffers (the storage's [T, N] layout), so the strides are exercised."""
import pytest
import torch

import recurrent_ref as rr
from generalizableracing_amd import _abi
from generalizableracing_amd.rsl_rl import fused_gru

gpu = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(1, 1, 64, 16), (5, 17, 64, 13), (5, 48, 192, 16), (24, 33, 192, 16), (3, 16, 256, 64)]
NAMES = ("gW_ih", "gW_hh", "gb_ih", "gb_hh")


def _inputs(T, B, R, D, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + 1000 * T + B + R + D)
    rnn = torch.nn.GRU(D, R)
    with torch.no_grad():
        for p in rnn.parameters():  # larger than the default init: the gates leave their linear range
            p.copy_(torch.randn(p.shape, generator=g) * (1.5 / R ** 0.5))
    rnn = rnn.to(DEV)
    xbuf = torch.randn(T, B + 3, D, generator=g).to(DEV)
    x = xbuf[:, 2:2 + B]  # a block of envs of a wider rollout
    h0 = (0.5 * torch.randn(B, R, generator=g)).to(DEV)
    dbuf = torch.zeros(T, B + 3, 1, dtype=torch.uint8)
    dbuf[:, 2:2 + B, 0] = rr.dones_pattern(T, B)
    dones = dbuf.to(DEV)[:, 2:2 + B, 0]
    gout = torch.randn(T, B, R, generator=g).to(DEV)
    return rnn, x, h0, dones, gout


def _fused(rnn, x, h0, dones, gout):
    out = fused_gru.gru_sequence(rnn, x, h0, dones)
    grads = torch.autograd.grad((out * gout).sum(), list(rnn.parameters()))
    return out.detach(), grads


@gpu
@pytest.mark.parametrize("T,B,R,D", CASES)
def test_gru_sequence_matches_float64_restatement(T, B, R, D):
    rnn, x, h0, dones, gout = _inputs(T, B, R, D)
    assert fused_gru.gru_fusable(rnn, x, T)
    calls = fused_gru.CALLS
    out, grads = _fused(rnn, x, h0, dones, gout)
    assert fused_gru.CALLS == calls + 1 and out.shape == (T, B, R)
    params = [p.detach() for p in rnn.parameters()]
    ref_out, ref_g = rr.masked_gru(x, h0, dones, *params, gout=gout, dtype=torch.float64)
    t32_out, t32_g = rr.masked_gru(x, h0, dones, *params, gout=gout, dtype=torch.float32)
    rows = [("out", out, ref_out, t32_out)] + [(n, g, r, t) for n, g, r, t in zip(NAMES, grads, ref_g, t32_g)]
    failed = []
    for name, got, ref, t32 in rows:
        assert got.shape == ref.shape, name
        e_torch, e_got = rr.rel_err(t32, ref), rr.rel_err(got, ref)
        bound = max(1e-5, 4.0 * e_torch)
        print(f"({T},{B},{R},{D}) {name}: torch fp32 {e_torch:.3e} bound {bound:.3e} fused {e_got:.3e}")
        if not e_got <= bound:
            failed.append((name, e_got, bound))
    assert not failed, failed
    # a second run gives identical bits (fixed summation order, no atomics)
    out2, grads2 = _fused(rnn, x, h0, dones, gout)
    assert torch.equal(out, out2)
    for a, b in zip(grads, grads2):
        assert torch.equal(a, b)


@gpu
@pytest.mark.parametrize("T,B,R,D", CASES)
def test_gru_step_iterated_with_resets_is_the_sequence_bit_for_bit(T, B, R, D):
    """The rollout step is the sequence kernel at T = 1: the same per-step arithmetic."""
    rnn, x, h0, dones, _ = _inputs(T, B, R, D, seed=7)
    with torch.no_grad():
        out = fused_gru.gru_sequence(rnn, x, h0, dones)
    h = h0.clone()
    first = torch.full_like(h0, float("nan"))
    for t in range(T):
        fused_gru.gru_step(rnn, x[t], h, h_prev_out=first if t == 0 else None)
        assert torch.equal(h, out[t]), t
        h.masked_fill_(dones[t].bool().view(B, 1), 0.0)  # the policy's reset(dones)
    assert torch.equal(first, h0)  # the second pointer holds the pre-step state of step 0


def test_gru_rejects_sizes_it_does_not_cover():
    """An unsupported size is GR_ERR_ARG before any launch (no device needed); gru_fusable sends it to torch."""
    lib = _abi.load()
    p = 0x10000

    def step(n=8, d=16, r=192):
        return lib.gr_gru_step(p, d, p, None, p, p, p, p, n, d, r, None)

    def fwd(t=4, b=8, d=16, r=192):
        return lib.gr_gru_seq_forward(p, b * d, d, p, p, b, p, p, p, p, t, b, d, r, p + 0x100000, p, None)

    def bwd(t=4, b=8, d=16, r=192):
        return lib.gr_gru_seq_backward(p, p, b * d, d, p, p, b, p, p, p, t, b, d, r, p, p, None)

    for r in (32, 96, 160, 320):
        assert step(r=r) == -1 and fwd(r=r) == -1 and bwd(r=r) == -1
        assert lib.gr_gru_scratch_floats(4, 8, r) == -1
    assert fwd(d=65) == -1 and fwd(d=0) == -1 and fwd(t=65) == -1 and fwd(b=0) == -1 and step(n=0) == -1
    assert bwd(d=65) == -1 and bwd(t=0) == -1
    assert fwd(t=64, b=2 ** 31 // (64 * 4 * 192) + 1) == -1  # past the 32-bit row offsets
    assert lib.gr_gru_scratch_floats(24, 1024, 192) > 24 * 1024 * 4 * 192
    rnn = torch.nn.GRU(16, 96)
    assert not fused_gru.gru_fusable(rnn, torch.zeros(4, 16))
    assert not fused_gru.gru_fusable(torch.nn.GRU(16, 192), torch.zeros(4, 16))  # CPU tensors
