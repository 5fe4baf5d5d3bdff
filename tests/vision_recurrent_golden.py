"""What tests/golden/make_golden_vision_recurrent.py and tests/test_vision_recurrent_policy_cpu.py share: the shapes,
the hyper-parameters, the dones pattern and the seeded CPU generator of the observation rows (the fixture stores the
seed and a checksum, not the 72 x 96 images)."""
import torch

T, N, K, H, W, STATE = 6, 8, 4, 72, 96, 16
OBS = STATE + H * W
DIM, R, HEADS = 16, 16, [16, 16]
HP = dict(num_learning_epochs=2, num_mini_batches=2, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0,
          entropy_coef=0.005, learning_rate=5e-4, max_grad_norm=1.0, use_clipped_value_loss=True,
          schedule="adaptive", desired_kl=0.01)
# (t, env) of every done: make_golden_recurrent.py's pattern
DONES = [(0, 1), (T - 1, 2), (1, 3), (4, 3), (2, 4), (3, 4), (3, 6), (0, 7), (T - 1, 7)]
SEED_A, SEED_B = 11, 12  # recording (a): eval mode, DONES; (b): train mode, no done


def policy_kwargs():
    return dict(img_res=(H, W), dim_hidden_input=DIM, actor_hidden_dims=HEADS, critic_hidden_dims=HEADS,
                activation="lrelu", rnn_type="gru", rnn_hidden_size=R, rnn_num_layers=1, init_noise_std=1.0,
                noise_std_type="scalar")


def rows(g, *lead):
    """Observation rows [*lead, OBS] in float64: 16 state terms ~ N(0, 1), then a depth-like image: a per-row plane
    with noise, clipped to [0, 10] m."""
    state = torch.randn(*lead, STATE, generator=g, dtype=torch.float64)
    v = torch.linspace(0.0, 1.0, H, dtype=torch.float64).view(H, 1)
    u = torch.linspace(0.0, 1.0, W, dtype=torch.float64).view(1, W)
    a = torch.rand(*lead, 3, generator=g, dtype=torch.float64)
    img = 2.0 + 8.0 * (a[..., 0, None, None] * v + a[..., 1, None, None] * u) \
        + a[..., 2, None, None] * torch.randn(*lead, H, W, generator=g, dtype=torch.float64)
    return torch.cat([state, img.clamp(0.0, 10.0).reshape(*lead, H * W)], dim=-1)


def inputs(seed, dones_list):
    """-> obs, cobs [T, N, OBS], rew [T, N], dones [T, N] (long), time outs [T, N] (bool), last critic rows [N, OBS],
    and the warm-up rows (actor's, critic's) [N, OBS] that give the rollout a non-zero starting state."""
    g = torch.Generator().manual_seed(seed)
    obs, cobs = rows(g, T, N), rows(g, T, N)
    rew = torch.randn(T, N, generator=g, dtype=torch.float64) * 0.1
    dones = torch.zeros(T, N, dtype=torch.long)
    for t, e in dones_list:
        dones[t, e] = 1
    tout = (torch.rand(T, N, generator=g) < 0.5) & dones.bool()
    last = rows(g, N)
    warm = (rows(g, N), rows(g, N))
    return obs, cobs, rew, dones, tout, last, warm


def checksum(obs, cobs):
    return torch.stack([obs.sum(), cobs.sum(), (obs * obs).sum()])


def randomise_batchnorms(module, g):
    """Non-trivial affine parameters and running statistics for every BatchNorm (eval mode then differs from init)."""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(0.5 + torch.rand(c, generator=g, dtype=torch.float64))
                m.bias.copy_(0.1 * torch.randn(c, generator=g, dtype=torch.float64))
                m.running_mean.copy_(0.5 * torch.randn(c, generator=g, dtype=torch.float64))
                m.running_var.copy_(0.5 + torch.rand(c, generator=g, dtype=torch.float64))
