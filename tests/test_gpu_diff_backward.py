"""gr_diff_backward against the float64 restatement (tests/bptt_ref.py) fed the kernel's own tape, upcast.

(T, N) in {(1, 1), (2, 65), (7, 321), (48, 64)}: one lane, a wave plus one, a block and a wave tail, the recipe's window;
both action lags; the forced resets of test_gpu_diff_record.py clipped to T.  Every env is compared; the error is
||dG[:, n, :]|| / ||G_ref[:, n, :]|| per env (where the reference is exactly zero the kernel's must be).  The bound is
not chosen here: it is, per case, 4 x the case's own fp32 floor that scripts/bptt_error_budget.py measures on the CPU for the fp32 torch
restatement against the float64 one on these windows (profiles/bptt_error_budget.json), because the kernel's operation
order differs from torch's and the floor is a sample."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import bptt_ref  # noqa: E402
import diff_window as dw  # noqa: E402
from generalizableracing_amd import _abi  # noqa: E402
from test_gpu_diff_record import DEV, make  # noqa: E402


@pytest.mark.parametrize("lag", [0, 1])
@pytest.mark.parametrize("T,N", dw.SHAPES)
def test_adjoint_against_float64(T, N, lag):
    bound = dw.case_bound(T, N, lag)  # 4 x this case's own floor
    env = make(N, lag, 1, True, t_max=T)
    g = torch.Generator().manual_seed(100 * T + lag)
    env.detach()
    for t in range(T):
        dw.force_timeouts(env, t, T, N)
        env.step(torch.randn(N, 4, generator=g).to(DEV))
    G = env.loss_action_grad().clone()
    G2 = env.loss_action_grad().clone()
    torch.cuda.synchronize()
    assert torch.equal(G.view(torch.int32), G2.view(torch.int32))  # a second run is bit-identical
    tape = env._diff.tape[:T].double().cpu()
    done = tape[:, _abi.DT_GOAL, :, 3] != 0
    for t, e in dw.forced_resets(T, N):
        assert bool(done[t, e])
    k = dict(env._diff.k, scale=1.0 / (T * N))
    ref = bptt_ref.window(bptt_ref.tape_fields(tape), k)
    assert torch.allclose(ref["losses"].float(), env._diff.losses[:T].cpu(), rtol=1e-5, atol=0)
    err, nz = dw.per_env_error(G.cpu(), ref["grad"])
    zero_ok = bool((G.cpu().permute(1, 0, 2)[~nz] == 0).all())
    worst = float(err.max()) if err.numel() else 0.0
    print(f"T {T} N {N} lag {lag}: max per-env error {worst:.3e} (bound {bound:.3e}), {int(nz.sum())}/{N} envs with a "
          f"non-zero reference, dones {int(done.sum())}")
    assert zero_ok
    if lag:
        assert not G[T - 1].any()  # no step of the window applies the last action
    assert int(nz.sum()) == (N if T > lag else 0)
    assert worst <= bound, (worst, bound)
    env.close()


def test_rows_past_32_bit_offsets_are_refused_without_a_device():
    cfg = _abi.default_config()
    cfg.num_envs = 321
    ctx = C.c_void_p()
    _abi.call("gr_create", C.byref(cfg), C.byref(ctx))
    lib = _abi.load()
    steps = 2 ** 31 // (_abi.GR_DIFF_PLANES * 321) + 1
    assert lib.gr_diff_backward(ctx, 16, steps, 1.0, 16, None) == -1  # GR_ERR_ARG, before any device use
    assert b"32-bit" in lib.gr_last_error(ctx)
    assert lib.gr_diff_backward(ctx, 16, 0, 1.0, 16, None) == -1
    lib.gr_destroy(ctx)
