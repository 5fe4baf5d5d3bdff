"""One BPTT iteration on the GPU: the fused path (HIP record / loss / adjoint kernels) against the torch path (the
reference's structure: autograd over the window) from the same seed, T = 8, N = 256.  The parameter gradients must agree
within 4 x the fp32 floor that scripts/bptt_error_budget.py measures for this window's shape (the (8, 256, lag 1) case of
profiles/bptt_error_budget.json), per parameter norm."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import diff_window as dw  # noqa: E402
from generalizableracing_amd.diff_rl import BPTT, BaseModel  # noqa: E402
from test_gpu_diff_record import DEV, make  # noqa: E402

T, N = dw.BPTT_SHAPE[:2]


def one_iteration(fused):
    torch.manual_seed(5)
    env = make(N, 1, 1, True, t_max=T, fused=fused)
    model = BaseModel(16, 16, 4, actor_hidden_dims=[256, 128], critic_hidden_dims=[256, 128], activation="lrelu")
    alg = BPTT(model, max_iterations=10, learning_rate=5e-4, optimizer="AdamW", device=DEV)
    alg.env = env
    obs = env.observe()["policy"]
    env.detach()
    for _ in range(T):
        a = alg.act(obs)
        o, _, term, tout, extras = env.step(a)
        obs = o["policy"].clone()
        alg.process_env_step(extras["losses"], extras["losses_detached"], term | tout)
    G = env.loss_action_grad()
    acts = alg.policy_actions(torch.stack(alg.obs).flatten(0, 1), torch.stack(alg.eps).flatten(0, 1))
    acts.backward(G.reshape(acts.shape))
    grads = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    alg.update(G)
    moved = [k for k, p in model.named_parameters() if k in grads and not torch.equal(p, before[k])]
    env.close()
    return grads, moved


def test_fused_and_torch_paths_agree():
    bound = dw.case_bound(*dw.BPTT_SHAPE)
    gf, moved = one_iteration(True)
    gt, _ = one_iteration(False)
    assert set(gf) == set(gt) and any(k.startswith("actor") for k in gf) and "std" in gf
    assert set(moved) == set(gf)  # the update moved every parameter that has a gradient
    for k in gf:
        err = float((gf[k] - gt[k]).norm() / gt[k].norm())
        print(f"{k}: |d grad| / |grad| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (k, err, bound)
