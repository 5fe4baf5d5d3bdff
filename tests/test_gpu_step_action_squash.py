"""The step kernel's action squash against the CPU oracle, bit for bit.

Under the one-step action lag the policy-observation wave of an env's 64-lane group loads the env's action, squashes
it (gr_tanhf) between the two workgroup barriers and hands it to the physics wave in an LDS row read after the second
barrier; without the lag, and in the obstacle kernels, the physics wave squashes it itself.  What can go wrong
there: a wrong lane or wave offset in the hand-over (env counts that leave a partial wave, a partial workgroup, more
than one workgroup), a row written after the barrier that publishes it, a stale lag plane, an action pointer cached
from an earlier call (two buffers passed alternately), a branch of the squash taken differently by the two roles
(the branch edges of gr_tanhf are forced into fixed envs every step), a first step after a reset (`azero`), and every
kernel instantiation with both lag settings.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from generalizableracing_amd import _abi  # noqa: E402
from generalizableracing_amd.envs.racing_cfg import RacingEnvCfg, SceneCfg, SimCfg, TerrainCfg  # noqa: E402
from generalizableracing_amd.envs.racing_env import RacingEnv  # noqa: E402

DEV = "cuda:0"
STEPS = 40
GUARD = 64  # rows allocated behind a sunk observation buffer; they must keep their fill
FILL = 7.0
LDS8 = ("step_kernel<true, false, 8, 1>", "step_kernel<true, false, 8>")


def _edges():
    """gr_tanhf's branch edges: the small-argument polynomial below 0.3, saturation above 9, both signs, with the
    float neighbours of each edge; zeros of both signs, far saturation and a denormal.  No NaN."""
    f = np.float32
    vals = [f(0.0), f(-0.0)]
    for edge in (f(0.3), f(9.0)):
        for s in (f(1.0), f(-1.0)):
            x = s * edge
            vals += [x, np.nextafter(x, f(np.inf)), np.nextafter(x, f(-np.inf))]
    vals += [f(20.0), f(-20.0), f(1e4), f(-1e4), f(1e-40)]
    out = np.array(vals, np.float32)
    assert out.size == 19 and not np.isnan(out).any() and out[-1] != 0.0
    return out


EDGES = _edges()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def bf16_rne(x):
    """Round to nearest even on the fp32 bits, NaN -> 0x7FC0 (the kernel's and c10::BFloat16's rule)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def make(n, lag=1, gates=8, obstacles=False, integrator="dd_explicit", **overrides):
    cfg = RacingEnvCfg(scene=SceneCfg(num_envs=n), sim=SimCfg(device=DEV), stage=1, integrator=integrator,
                       terrain=TerrainCfg(num_gates=gates, obstacles=obstacles),
                       overrides=dict(action_lag=lag, **overrides))
    env = RacingEnv(cfg)
    assert env.gr_config.action_lag == lag
    orc = oracle.from_env(env)
    orc.init()
    env.reset()
    orc.reset(None)
    return env, orc


def kernel_envs(env):
    torch.cuda.synchronize()
    return oracle.planes_to_envs(env.state.cpu().numpy(), env.istate.cpu().numpy())


def assert_step_equal(env, orc, out, where):
    """State planes, istate, policy and critic rows, aux, reward, terminated, time_out and dones."""
    _, rew, term, tout, _ = out
    assert np.array_equal(bits(rew.cpu().numpy()), bits(orc.reward)), where
    assert np.array_equal(term.cpu().numpy().astype(np.uint8), orc.terminated), where
    assert np.array_equal(tout.cpu().numpy().astype(np.uint8), orc.time_out), where
    assert np.array_equal(env._sets[env._cur]["dones"].cpu().numpy(), orc.dones), where
    got = kernel_envs(env)
    for name in oracle.ENV_DTYPE.names:
        g, w = bits(got[name]), bits(orc.envs[name])
        if not np.array_equal(g, w):
            i = np.argwhere(g != w)[0][0]
            raise AssertionError(f"{where}: field {name} of env {i}: kernel {got[name][i]} oracle {orc.envs[name][i]}")
    s = env.obs_buf
    for key, want in (("policy", orc.obs_policy), ("critic", orc.obs_critic)):
        assert np.array_equal(bits(s[key].cpu().numpy()), bits(want)), (where, key)
    assert np.array_equal(bits(s["auxiliary"].cpu().numpy()[:, 0]), bits(orc.obs_aux)), where


def actions_of(n, g, k):
    """randn x 1.2, with the squash's branch edges cycled through envs 0, 63, 64 and n - 1 (where present)."""
    a = (torch.randn(n, 4, generator=g) * 1.2).numpy().astype(np.float32)
    for j, i in enumerate(sorted({i for i in (0, 63, 64, n - 1) if 0 <= i < n})):
        for c in range(4):
            a[i, c] = EDGES[(k * 16 + j * 4 + c) % EDGES.size]
    return a


def randomize_episode_lengths(env, orc, n, g):
    eplen = torch.randint(0, 200, (n,), generator=g, dtype=torch.int32)
    env.episode_length_buf = eplen.to(DEV)
    orc.envs["ep_len"] = eplen.numpy()


def free_run(env, orc, n, seed, each_step=None, steps=STEPS):
    """`steps` steps from random episode lengths, the actions passed in two buffers alternately (the buffer not
    passed is overwritten before the call: a kernel reading a pointer kept from the call before sees other actions)
    -> (resets, first steps of an episode with the lagged previous action zeroed)."""
    g = torch.Generator().manual_seed(seed)
    randomize_episode_lengths(env, orc, n, g)
    bufs = [torch.empty(n, 4, device=DEV), torch.empty(n, 4, device=DEV)]
    assert bufs[0].data_ptr() != bufs[1].data_ptr()
    resets = azeros = 0
    for k in range(steps):
        a = actions_of(n, g, k)
        azeros += int(orc.envs["azero"].sum())
        bufs[k % 2].copy_(torch.from_numpy(a))
        bufs[(k + 1) % 2].fill_(0.75)
        out = env.step(bufs[k % 2])
        orc.step(a)
        torch.cuda.synchronize()
        assert_step_equal(env, orc, out, f"step {k}")
        if each_step is not None:
            each_step(k)
        resets += int(orc.dones.astype(bool).sum())
    return resets, azeros


@pytest.mark.parametrize("lag", [1, 0], ids=["lag1", "lag0"])
@pytest.mark.parametrize("n", [1, 63, 65, 255, 257, 1000])
def test_env_counts_bit_exact(n, lag):
    """The hand-over is lane t of a policy wave to lane t of the physics wave of the same 64 envs: a partial wave,
    a partial workgroup (dead lanes mirror env n - 1), more than one workgroup.  8-gate gate-only tracks: the
    headline instantiation where a workgroup's terrain types fit the LDS slice (1 and 1000 envs), the one reading
    the table from L2 where they do not."""
    env, orc = make(n, lag)
    assert env.step_kernel_name() in (LDS8[0], "step_kernel<false, false>"), env.step_kernel_name()
    resets, azeros = free_run(env, orc, n, seed=10 * n + lag)
    if n >= 255:  # resets happened, and with them first steps whose lagged action is zeroed
        assert resets >= 1 and azeros >= 1, (resets, azeros)
    env.close()


VARIANTS = {
    # id: (make() arguments, the instantiations it may launch)
    "gates8": (dict(), LDS8),
    "gates32": (dict(gates=32), ("step_kernel<true, false>", "step_kernel<false, false>")),
    "obstacles": (dict(obstacles=True), ("step_kernel<false, true, 0, 1>",)),
    "c5_rotor_dr": (dict(gates=32, dr_rotor=1), ("step_kernel<true, false>", "step_kernel<false, false>")),
    "rotor_dr_8gates": (dict(dr_rotor=1), ("step_kernel<true, false, 8>",)),
    "rotor_dr_obstacles": (dict(obstacles=True, dr_rotor=1), ("step_kernel<false, true>",)),
    "sim_substep": (dict(integrator="semi_implicit"), ("step_kernel<true, false, 8>",)),
    "sim_substep_obstacles": (dict(obstacles=True, integrator="semi_implicit"), ("step_kernel<false, true>",)),
}


@pytest.mark.parametrize("lag", [1, 0], ids=["lag1", "lag0"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kernel_variants_bit_exact(variant, lag):
    """Every other step_kernel instantiation, and the substepped integrator's branch of the physics wave, with and
    without the lag: 8- and 32-gate tracks, obstacle tracks (which keep the squash in the physics wave), C5's rotor DR,
    the substepped integrator."""
    n = 1000
    kw, names = VARIANTS[variant]
    env, orc = make(n, lag, **kw)
    assert env.step_kernel_name() in names, env.step_kernel_name()
    resets, azeros = free_run(env, orc, n, seed=len(variant) * 7 + lag)
    assert resets >= 1 and azeros >= 1, (resets, azeros)
    env.close()


def test_captured_steps_bit_exact():
    """Four steps captured in one graph on two action buffers passed alternately, replayed with new actions in the
    buffers each time: every replay squashes what the buffers hold then, and the state and the last step's outputs
    equal the oracle's after the same four steps."""
    n, glen, replays = 257, 4, 6
    env, orc = make(n, 1)
    g = torch.Generator().manual_seed(5)
    randomize_episode_lengths(env, orc, n, g)
    bufs = [torch.zeros(n, 4, device=DEV), torch.zeros(n, 4, device=DEV)]
    k = 0

    def eager(buf):
        nonlocal k
        a = actions_of(n, g, k)
        k += 1
        buf.copy_(torch.from_numpy(a))
        out = env.step(buf)
        orc.step(a)
        return out

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for j in range(2):
            eager(bufs[j])
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert_step_equal(env, orc, eager(bufs[0]), "eager")
    while env._calls % glen != 0:  # the call parity the captured launches were recorded with
        eager(bufs[env._calls % 2])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for j in range(glen):
            out = env.step(bufs[j % 2])
    for r in range(replays):
        a0, a1 = actions_of(n, g, k), actions_of(n, g, k + 1)
        k += 2
        bufs[0].copy_(torch.from_numpy(a0))
        bufs[1].copy_(torch.from_numpy(a1))
        graph.replay()
        for j in range(glen):
            orc.step(a1 if j % 2 else a0)
        torch.cuda.synchronize()
        assert_step_equal(env, orc, out, f"replay {r}")
    del graph
    env.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sink_rows_match_unsunk(dtype):
    """The observation sink's second row set at 257 envs with the squash handed over between the roles: fp32 bit for
    bit, bf16 by the round-to-nearest-even rule; GUARD rows behind the sunk rows keep their fill."""
    n = 257
    env, orc = make(n, 1)
    big_p = torch.full((n + GUARD, 16), FILL, device=DEV, dtype=dtype)
    big_c = torch.full((n + GUARD, 16), FILL, device=DEV, dtype=dtype)
    code = _abi.GR_DTYPE_F32 if dtype == torch.float32 else _abi.GR_DTYPE_BF16
    env._bind_obs_sink(big_p.data_ptr(), big_c.data_ptr(), code)

    def check(k):
        s = env.obs_buf
        for big, key in ((big_p, "policy"), (big_c, "critic")):
            rows = s[key].cpu().numpy()
            if dtype == torch.float32:
                got = big.cpu().numpy()
                assert np.array_equal(bits(got[:n]), bits(rows)), (key, k)
                assert np.array_equal(got[n:], np.full((GUARD, 16), FILL, np.float32)), (key, k)
            else:
                got = big.view(torch.int16).cpu().numpy().view(np.uint16)
                assert np.array_equal(got[:n], bf16_rne(rows)), (key, k)
                assert np.array_equal(got[n:], np.full((GUARD, 16), 0x40E0, np.uint16)), (key, k)  # bf16(7.0)

    free_run(env, orc, n, seed=7, each_step=check)
    env._bind_obs_sink(None, None, _abi.GR_DTYPE_F32)
    env.close()
