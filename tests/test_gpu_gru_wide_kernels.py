"""The wide family of the fused GRU memory (gr_gru_wide_step / gr_gru_wide_seq_forward / gr_gru_wide_seq_backward,
csrc/gr_gru.hip; rsl_rl/fused_gru.py): input widths up to 256 and the input gradient gx, against the float64
restatement of the masked sequence with x a leaf (tests/gru_wide_ref.py), fed the op's own inputs, upcast.

Bound, as tests/test_gpu_gru_kernels.py: per case and per tensor, torch's own fp32 GRU on the CPU is measured against
float64 at run time, and the fused op must stay within max(1e-5, 4 x that error) of the tensor's norm; the 4 covers a
different summation order and the non-libm tanh, nothing else.

Cases (T, B, R, D): the first width past the narrow family's limit, odd; a partial env tile with D no multiple of 4;
x requiring a gradient at a narrow width; three env tiles at the recipe's widths; the recipe's T with a partial tile;
the largest.  x and dones are blocks of wider buffers; dones: recurrent_ref.dones_pattern."""
import pytest
import torch

import gru_wide_ref as wr
import recurrent_ref as rr
from generalizableracing_amd import _abi
from generalizableracing_amd.rsl_rl import fused_gru

gpu = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(1, 1, 64, 65), (5, 17, 64, 77), (5, 17, 64, 13), (5, 48, 192, 192), (24, 33, 192, 192), (3, 16, 256, 256)]
NAMES = ("gW_ih", "gW_hh", "gb_ih", "gb_hh")


def _inputs(T, B, R, D, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + 1000 * T + B + R + D)
    rnn = torch.nn.GRU(D, R)
    with torch.no_grad():
        for p in rnn.parameters():  # larger than the default init: the gates leave their linear range
            p.copy_(torch.randn(p.shape, generator=g) * (1.5 / R ** 0.5))
    rnn = rnn.to(DEV)
    xbuf = torch.randn(T, B + 3, D, generator=g).to(DEV)
    h0 = (0.5 * torch.randn(B, R, generator=g)).to(DEV)
    dbuf = torch.zeros(T, B + 3, 1, dtype=torch.uint8)
    dbuf[:, 2:2 + B, 0] = rr.dones_pattern(T, B)
    dones = dbuf.to(DEV)[:, 2:2 + B, 0]
    gout = torch.randn(T, B, R, generator=g).to(DEV)
    return rnn, xbuf, h0, dones, gout


def _fused(rnn, xbuf, B, h0, dones, gout):
    """x = a block of envs of a wider rollout buffer that requires a gradient: the op sees the strided view."""
    xb = xbuf.detach().clone().requires_grad_(True)
    x = xb[:, 2:2 + B]
    out = fused_gru.gru_sequence(rnn, x, h0, dones)
    grads = torch.autograd.grad((out * gout).sum(), list(rnn.parameters()) + [xb])
    gxb = grads[4]
    assert torch.count_nonzero(gxb[:, :2]) == 0 and torch.count_nonzero(gxb[:, 2 + B:]) == 0
    return out.detach(), grads[:4], gxb[:, 2:2 + B]


@gpu
@pytest.mark.parametrize("T,B,R,D", CASES)
def test_wide_sequence_and_gx_match_float64_restatement(T, B, R, D):
    rnn, xbuf, h0, dones, gout = _inputs(T, B, R, D)
    x = xbuf[:, 2:2 + B]
    assert fused_gru.gru_fusable(rnn, x, T)
    calls, wide = fused_gru.CALLS, fused_gru.WIDE_CALLS
    out, grads, gx = _fused(rnn, xbuf, B, h0, dones, gout)
    assert fused_gru.CALLS == calls + 1 and fused_gru.WIDE_CALLS == wide + 1
    assert out.shape == (T, B, R) and gx.shape == (T, B, D)
    params = [p.detach() for p in rnn.parameters()]
    ref_out, ref_g, ref_gx = wr.masked_gru_dx(x, h0, dones, *params, gout=gout, dtype=torch.float64)
    t32_out, t32_g, t32_gx = wr.masked_gru_dx(x, h0, dones, *params, gout=gout, dtype=torch.float32)
    rows = [("out", out, ref_out, t32_out)] + [(n, g, r, t) for n, g, r, t in zip(NAMES, grads, ref_g, t32_g)]
    rows.append(("gx", gx, ref_gx, t32_gx))
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
    out2, grads2, gx2 = _fused(rnn, xbuf, B, h0, dones, gout)
    assert torch.equal(out, out2) and torch.equal(gx, gx2)
    for a, b in zip(grads, grads2):
        assert torch.equal(a, b)


@gpu
@pytest.mark.parametrize("T,B,R,D", [c for c in CASES if c[0] > 1])
@pytest.mark.parametrize("which", ["first", "last"])
def test_gx_before_a_done_ignores_gout_after_it(T, B, R, D, which):
    """An env masked after step t' carries nothing back across it: with gout[t'+1:, b] changed, gx[:t'+1, b] keeps
    its bits (t' = the env's first done, then its last; envs without a done before T - 1 are left alone)."""
    rnn, xbuf, h0, dones, gout = _inputs(T, B, R, D, seed=3)
    _, _, gx = _fused(rnn, xbuf, B, h0, dones, gout)
    dn = dones.cpu()
    gout2 = gout.clone()
    cut = {}
    for b in range(B):
        ts = torch.nonzero(dn[:, b]).flatten().tolist()
        ts = [t for t in ts if t < T - 1]
        if ts:
            cut[b] = ts[0] if which == "first" else ts[-1]
            gout2[cut[b] + 1:, b] = gout2[cut[b] + 1:, b] * -3.0 + 1.0
    assert cut
    _, _, gx2 = _fused(rnn, xbuf, B, h0, dones, gout2)
    changed = 0
    for b, tp in cut.items():
        assert torch.equal(gx[:tp + 1, b], gx2[:tp + 1, b]), (b, tp)
        changed += int(not torch.equal(gx[tp + 1:, b], gx2[tp + 1:, b]))
    assert changed == len(cut)  # (the steps after the done did see the change)


@gpu
@pytest.mark.parametrize("T,B,R,D", CASES)
def test_wide_step_iterated_with_resets_is_the_sequence_bit_for_bit(T, B, R, D):
    """The step keeps the input projection inside its kernel, the sequence hoists it into one GEMM ahead of the serial
    kernel: the same MFMA chains, so the same bits."""
    rnn, xbuf, h0, dones, _ = _inputs(T, B, R, D, seed=7)
    x = xbuf[:, 2:2 + B]
    p = [q.detach() for q in rnn.parameters()]
    out, gates = torch.empty(T, B, R, device=DEV), torch.empty(T, B, 4 * R, device=DEV)
    outs = []
    for gt in (gates, None):  # with the gates saved (T > 1: the input projection hoisted into one GEMM) and without
        _abi.call("gr_gru_wide_seq_forward", x.data_ptr(), int(x.stride(0)), int(x.stride(1)), h0.data_ptr(),
                  dones.data_ptr(), int(dones.stride(0)), p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(),
                  p[3].data_ptr(), T, B, D, R, out.data_ptr(), gt.data_ptr() if gt is not None else None,
                  _abi.raw_stream(out.device))
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])
    h = h0.clone()
    first = torch.full_like(h0, float("nan"))
    for t in range(T):
        xt = x[t]
        _abi.call("gr_gru_wide_step", xt.data_ptr(), int(xt.stride(0)), h.data_ptr(),
                  first.data_ptr() if t == 0 else None, p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(),
                  p[3].data_ptr(), B, D, R, _abi.raw_stream(h.device))
        assert torch.equal(h, out[t]), t
        h.masked_fill_(dones[t].bool().view(B, 1), 0.0)  # the policy's reset(dones)
    assert torch.equal(first, h0)  # the second pointer holds the pre-step state of step 0
    if D > fused_gru.MAX_D:  # fused_gru.gru_step takes the wide entry point at these widths: the same bits
        h2 = h0.clone()
        fused_gru.gru_step(rnn, x[0], h2)
        assert torch.equal(h2, out[0])


@gpu
def test_narrow_call_without_input_gradient_takes_the_narrow_entry_points():
    T, B, R, D = 5, 17, 64, 13
    rnn, xbuf, h0, dones, gout = _inputs(T, B, R, D)
    x = xbuf[:, 2:2 + B]
    calls, wide = fused_gru.CALLS, fused_gru.WIDE_CALLS
    out = fused_gru.gru_sequence(rnn, x, h0, dones)
    grads = torch.autograd.grad((out * gout).sum(), list(rnn.parameters()))
    assert fused_gru.CALLS == calls + 1 and fused_gru.WIDE_CALLS == wide
    # and the wide family gives the same bits at this width
    out_w, grads_w, _ = _fused(rnn, xbuf, B, h0, dones, gout)
    assert fused_gru.WIDE_CALLS == wide + 1
    assert torch.equal(out.detach(), out_w)
    for a, b in zip(grads, grads_w):
        assert torch.equal(a, b)


def test_wide_entry_points_reject_sizes_they_do_not_cover():
    """An unsupported size is GR_ERR_ARG before any launch (no device needed)."""
    lib = _abi.load()
    p = 0x10000

    def step(n=8, d=192, r=192):
        return lib.gr_gru_wide_step(p, d, p, None, p, p, p, p, n, d, r, None)

    def fwd(t=4, b=8, d=192, r=192):
        return lib.gr_gru_wide_seq_forward(p, b * d, d, p, p, b, p, p, p, p, t, b, d, r, p + 0x100000, p, None)

    def bwd(t=4, b=8, d=192, r=192, gx=p, ld_b=None):
        ld_b = d if ld_b is None else ld_b
        return lib.gr_gru_wide_seq_backward(p, p, b * d, d, p, p, b, p, p, p, p, t, b, d, r, p, p, gx, b * ld_b, ld_b,
                                            None)

    def scratch(t=4, b=8, d=192, r=192):
        return lib.gr_gru_wide_scratch_floats(t, b, d, r)

    for r in (32, 96, 320):
        assert step(r=r) == -1 and fwd(r=r) == -1 and bwd(r=r) == -1 and scratch(r=r) == -1
    for d in (0, 257):
        assert step(d=d) == -1 and fwd(d=d) == -1 and bwd(d=d) == -1 and scratch(d=d) == -1
    assert fwd(t=65) == -1 and bwd(t=65) == -1 and scratch(t=65) == -1
    assert fwd(b=0) == -1 and bwd(b=0) == -1 and scratch(b=0) == -1 and step(n=0) == -1
    big = 2 ** 31 // (64 * 4 * 192) + 1  # past the 32-bit row offsets
    assert fwd(t=64, b=big) == -1 and bwd(t=64, b=big) == -1 and scratch(t=64, b=big) == -1
    assert step(n=2 ** 31 // (4 * 192) + 1) == -1
    assert bwd(ld_b=191) == -1  # gx rows narrower than d
    assert scratch(24, 1024, 192, 192) > 24 * 1024 * 4 * 192
    assert scratch(24, 1024, 256, 192) > scratch(24, 1024, 192, 192)
    # gru_fusable: the wide widths are covered, the next one is not
    assert not fused_gru.gru_fusable(torch.nn.GRU(257, 192), torch.zeros(4, 257))
    assert fused_gru.MAX_D_WIDE == 256
