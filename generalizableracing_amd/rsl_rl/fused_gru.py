"""The GRU memory of ActorCriticRecurrent as one device op each way (gr_gru_seq_forward / gr_gru_seq_backward) and
one launch per rollout step (gr_gru_step), csrc/gr_gru.hip.

The masked sequence over a mini-batch's [T, B] block, torch.nn.GRU's parameters and gate order (r, z, n):

    h' = h0 at t = 0, out[t-1] * (1 - dones[t-1]) after
    r = sigmoid(W_ir x + b_ir + W_hr h' + b_hr);  z = sigmoid(W_iz x + b_iz + W_hz h' + b_hz)
    n = tanh(W_in x + b_in + r (W_hn h' + b_hn));  out[t] = (1 - z) n + z h'

The forward saves out and the gates (r, z, n, W_hn h' + b_hn); the backward carries dh from t = T-1 to 0 under the
same mask and returns the four parameter gradients.  The stored h0 is a constant: no gradient.
The rollout step is the same kernel at T = 1, so stepping it with resets gives the sequence's bits.

Two families of entry points.  gr_gru_*: input width d <= 64, x a constant (ActorCriticRecurrent: x is the
observation).  gr_gru_wide_*: d <= 256 and dL/dx = W_ir^T da_r + W_iz^T da_z + W_in^T da_n (VisionActorCriticRecurrent:
x is the stem's feature, which trains).  A call with d <= 64 whose x needs no gradient takes the first, any other the
second; for d <= 64 both give the same bits.  The wide sequence computes x W_ih^T for all T B rows in one GEMM ahead
of the serial kernel (the same MFMA chains as the in-loop form, staged in the gates buffer); the rollout step keeps it
inside its kernel.
"""
from __future__ import annotations

import torch

from .. import _abi

# the number of sequences evaluated through gr_gru_seq_forward (tests and the timing script read it: the fused path
# was taken)
CALLS = 0
# of those, the ones through the wide family (gr_gru_wide_seq_forward)
WIDE_CALLS = 0

SIZES = (64, 128, 192, 256)  # hidden sizes gr_gru.hip instantiates
MAX_D, MAX_T = 64, 64  # (MAX_D: of the narrow family)
MAX_D_WIDE = 256


def gru_fusable(rnn, x: torch.Tensor, steps: int = 1) -> bool:
    """gr_gru_* cover this memory on these inputs: a one-layer unidirectional fp32 torch.nn.GRU with biases of a
    size the kernels instantiate, fp32 CUDA inputs, no autocast."""
    if not isinstance(rnn, torch.nn.GRU) or rnn.num_layers != 1 or rnn.bidirectional or not rnn.bias:
        return False
    if rnn.hidden_size not in SIZES or not 1 <= rnn.input_size <= MAX_D_WIDE or not 1 <= steps <= MAX_T:
        return False
    if not (x.is_cuda and x.dtype == torch.float32 and rnn.weight_hh_l0.is_cuda
            and rnn.weight_hh_l0.dtype == torch.float32):
        return False
    return not torch.is_autocast_enabled()


def _x_strides(x: torch.Tensor):
    """x [T, B, D] as the kernels address it (unit stride over D; the [T, B] strides free: a block of the storage)."""
    if x.stride(2) != 1 and x.shape[2] != 1:
        x = x.contiguous()
    return x, int(x.stride(0)), int(x.stride(1))


def _dones_bytes(dones: torch.Tensor, t: int, b: int):
    """dones [T, B] (any flag dtype, a trailing 1 allowed) as bytes with unit stride over B."""
    d = dones.reshape(t, b) if dones.dim() != 2 else dones
    if d.dtype == torch.bool:
        d = d.view(torch.uint8) if d.stride(1) == 1 else d.to(torch.uint8)
    elif d.dtype != torch.uint8:
        d = (d != 0).to(torch.uint8)
    if d.stride(1) != 1 and b != 1:
        d = d.contiguous()
    return d, int(d.stride(0))


class _GRUSeqFn(torch.autograd.Function):
    """out [T, B, R] of (x, h0, dones; W_ih, W_hh, b_ih, b_hh) with the backward above.  The backward leaves the saved
    tensors intact and writes new buffers, so a retained graph may run it again."""

    @staticmethod
    def forward(ctx, x, h0, dones, w_ih, w_hh, b_ih, b_hh):
        global CALLS, WIDE_CALLS
        wide = x.shape[2] > MAX_D or x.requires_grad
        w_ih, w_hh, b_ih, b_hh = (p.detach().contiguous() for p in (w_ih, w_hh, b_ih, b_hh))
        t, b, d = x.shape
        r = w_hh.shape[1]
        dev = x.device
        x, ldx_t, ldx_b = _x_strides(x.detach())
        h0 = h0.detach().reshape(b, r).contiguous()
        dn, ld_dn = _dones_bytes(dones, t, b)
        out = torch.empty(t, b, r, device=dev, dtype=torch.float32)
        gates = torch.empty(t, b, 4 * r, device=dev, dtype=torch.float32)
        _abi.call("gr_gru_wide_seq_forward" if wide else "gr_gru_seq_forward", x.data_ptr(), ldx_t, ldx_b,
                  h0.data_ptr(), dn.data_ptr(), ld_dn, w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(),
                  b_hh.data_ptr(), t, b, d, r, out.data_ptr(), gates.data_ptr(), _abi.raw_stream(dev))
        ctx.save_for_backward(x, h0, dn, w_hh, out, gates, *((w_ih,) if wide else ()))
        ctx.strides = (ldx_t, ldx_b, ld_dn, d)
        ctx.wide = wide
        CALLS += 1
        WIDE_CALLS += int(wide)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, h0, dn, w_hh, out, gates = ctx.saved_tensors[:6]
        ldx_t, ldx_b, ld_dn, d = ctx.strides
        t, b, r = out.shape
        dev = out.device
        gout = gout.float().contiguous()
        if ctx.wide:
            return _wide_backward(ctx, gout)
        scratch = torch.empty(int(_abi.load().gr_gru_scratch_floats(t, b, r)), device=dev, dtype=torch.float32)
        grads = torch.empty(3 * r * (d + r + 2), device=dev, dtype=torch.float32)
        _abi.call("gr_gru_seq_backward", gout.data_ptr(), x.data_ptr(), ldx_t, ldx_b, h0.data_ptr(), dn.data_ptr(),
                  ld_dn, w_hh.data_ptr(), out.data_ptr(), gates.data_ptr(), t, b, d, r, scratch.data_ptr(),
                  grads.data_ptr(), _abi.raw_stream(dev))
        o1, o2, o3 = 3 * r * d, 3 * r * (d + r), 3 * r * (d + r + 1)
        return (None, None, None, grads[:o1].view(3 * r, d), grads[o1:o2].view(3 * r, r), grads[o2:o3], grads[o3:])


def _wide_backward(ctx, gout):
    """_GRUSeqFn.backward through gr_gru_wide_seq_backward: the same flat parameter gradients, and gx [T, B, D] when
    x needs it."""
    x, h0, dn, w_hh, out, gates, w_ih = ctx.saved_tensors
    ldx_t, ldx_b, ld_dn, d = ctx.strides
    t, b, r = out.shape
    dev = out.device
    scratch = torch.empty(int(_abi.load().gr_gru_wide_scratch_floats(t, b, d, r)), device=dev, dtype=torch.float32)
    grads = torch.empty(3 * r * (d + r + 2), device=dev, dtype=torch.float32)
    gx = torch.empty(t, b, d, device=dev, dtype=torch.float32) if ctx.needs_input_grad[0] else None
    _abi.call("gr_gru_wide_seq_backward", gout.data_ptr(), x.data_ptr(), ldx_t, ldx_b, h0.data_ptr(), dn.data_ptr(),
              ld_dn, w_ih.data_ptr(), w_hh.data_ptr(), out.data_ptr(), gates.data_ptr(), t, b, d, r,
              scratch.data_ptr(), grads.data_ptr(), gx.data_ptr() if gx is not None else None, b * d, d,
              _abi.raw_stream(dev))
    o1, o2, o3 = 3 * r * d, 3 * r * (d + r), 3 * r * (d + r + 1)
    return (gx, None, None, grads[:o1].view(3 * r, d), grads[o1:o2].view(3 * r, r), grads[o2:o3], grads[o3:])


def gru_sequence(rnn, x, h0, dones):
    """The masked sequence of `rnn` (gru_fusable) over x [T, B, D] from h0 [B, R] (or [1, B, R]) with the rollout's
    dones [T, B]: out [T, B, R], differentiable in the four parameters and, where x requires it, in x."""
    return _GRUSeqFn.apply(x, h0, dones, rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)


def gru_step(rnn, x, h, h_prev_out=None):
    """One rollout step in place: h [N, R] <- GRU(x [N, D], h); h_prev_out [N, R] (the storage's h0, passed at rollout
    step 0 only) receives the pre-step state.  No gradient."""
    n, d = x.shape
    if x.stride(1) != 1 and d != 1:
        x = x.contiguous()
    w_ih, w_hh, b_ih, b_hh = (p.detach() for p in (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0,
                                                   rnn.bias_hh_l0))
    _abi.call("gr_gru_wide_step" if d > MAX_D else "gr_gru_step", x.data_ptr(), int(x.stride(0)), h.data_ptr(),
              h_prev_out.data_ptr() if h_prev_out is not None else None, w_ih.data_ptr(), w_hh.data_ptr(),
              b_ih.data_ptr(), b_hh.data_ptr(), n, d, rnn.hidden_size, _abi.raw_stream(x.device))
    return h
