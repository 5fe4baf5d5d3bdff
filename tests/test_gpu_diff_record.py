"""gr_diff_record against the step kernel, bit for bit, and a differentiable env against a plain one.

The record kernel restates the lean forward arithmetic (action_scale, ctbr_compute<NO_MOTOR>, dd_explicit) in its own
translation unit; for every (env, step) the step does not reset, the row's x+ and (T+, tau+) must equal the planes
gr_step writes.  321 envs: a block tail and a wave tail of the 64-lane launch.  Both action lags (the action read
from the lag plane or squashed here), stage 0 and 1, 6 steps of N(0, 1) actions, time-outs forced through
episode_length_buf (env 0 at step 0, env 64 at step 3, env 320 at step 5).  On the CPU oracle these inputs give exactly
the three forced dones (0.998 of the pairs compared); at least 95 % must be compared here."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diff_window as dw  # noqa: E402
from generalizableracing_amd import _abi  # noqa: E402
from generalizableracing_amd.envs.racing_cfg import RacingEnvCfg, SceneCfg, SimCfg, TerrainCfg  # noqa: E402
from generalizableracing_amd.envs.racing_env import RacingEnv  # noqa: E402

DEV = "cuda:0"
N, T = 321, 6


def make(n, lag, stage, diff, t_max=T, fused=True):
    cfg = RacingEnvCfg(scene=SceneCfg(num_envs=n), sim=SimCfg(device=DEV), stage=stage,
                       terrain=TerrainCfg(num_cols=min(4, n), obstacles=False, regen_interval_s=None), overrides=dict(action_lag=lag),
                       is_differentiable_physics=diff, diff_window=t_max, diff_fused=fused)
    env = RacingEnv(cfg)
    env.reset()
    return env


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("lag", [0, 1])
def test_record_equals_step(lag, stage):
    env = make(N, lag, stage, True)
    plain = make(N, lag, stage, False)
    assert plain._diff is None and "losses" not in plain.extras
    g = torch.Generator().manual_seed(7)
    env.detach()
    compared = total = 0
    for t in range(T):
        dw.force_timeouts(env, t, T, N)
        dw.force_timeouts(plain, t, T, N)
        a = torch.randn(N, 4, generator=g).to(DEV)
        obs, rew, term, tout, extras = env.step(a)
        obs_p, rew_p, term_p, tout_p, extras_p = plain.step(a)
        assert set(extras_p) == {"log"} and plain._diff is None  # the flag off adds nothing to what step returns
        assert set(extras) == {"log", "losses", "losses_detached", "log_losses"}
        torch.cuda.synchronize()
        # the differentiable env is the plain env: same observations, rewards, flags and planes
        for x, y in ((obs["policy"], obs_p["policy"]), (obs["critic"], obs_p["critic"]), (rew, rew_p),
                     (env.state, plain.state)):
            assert np.array_equal(bits(x), bits(y)), t
        assert torch.equal(term, term_p) and torch.equal(tout, tout_p) and torch.equal(env.istate, plain.istate)
        done = (term | tout).cpu().numpy()
        for tt, e in dw.forced_resets(T, N):
            if tt == t:
                assert done[e], (t, e)
        row = env._diff.tape[t]
        live = ~done
        st = env.state
        for plane, src in ((_abi.DT_XP0, _abi.P_POSQ), (_abi.DT_XP1, _abi.P_QV), (_abi.DT_XP2, _abi.P_VW),
                           (_abi.DT_TT, _abi.P_CTRL)):
            assert np.array_equal(bits(row[plane])[live], bits(st[src])[live]), (t, plane)
        assert np.array_equal(bits(row[_abi.DT_XP3][:, 0])[live], bits(st[_abi.P_WA][:, 0])[live]), t
        assert np.array_equal(row[_abi.DT_GOAL][:, 3].cpu().numpy() != 0, done), t
        compared += int(live.sum())
        total += N
    assert compared >= 0.95 * total, (compared, total)
    assert env.diff_steps == T
    env.close()
    plain.close()


def test_tape_overflow_raises_before_any_launch():
    env = make(65, 1, 1, True, t_max=2)
    a = torch.zeros(65, 4, device=DEV)
    env.detach()
    env.step(a)
    env.step(a)
    calls = env._calls
    with pytest.raises(RuntimeError, match="detach"):
        env.step(a)
    assert env._calls == calls  # nothing was bound or launched
    env.detach()
    env.step(a)
    env.close()


def test_regeneration_interval_is_refused():
    cfg = RacingEnvCfg(scene=SceneCfg(num_envs=65), sim=SimCfg(device=DEV), stage=1,
                       terrain=TerrainCfg(num_cols=4, obstacles=False, regen_interval_s=0.03 * 4),
                       is_differentiable_physics=True, diff_window=8)
    with pytest.raises(ValueError, match="regen_interval_s"):
        RacingEnv(cfg)
