"""tests/bptt_ref.py (the float64 restatement of the differentiable window) against tests/golden/golden_bptt.npz, made
by tests/golden/make_golden_bptt.py from the reference's own DroneDynamics, CTBRController and loss functions in
float64: T = 6, N = 48, action lag 0 and 1, per-env gains / delays / mass / inertia / drag, resets at steps 0, 3 and 5,
gate centres per step.  Equal to 1e-9 of each tensor's largest magnitude (both sides float64 over at most 6 chained
steps; anything larger is a semantic difference): pins the sign, gamma, the cuts and the lag indexing."""
import os

import numpy as np
import pytest
import torch

import bptt_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_bptt.npz")


@pytest.mark.parametrize("lag", [0, 1])
def test_restatement_equals_the_reference(lag):
    g = dict(np.load(GOLD))
    tag = f"lag{lag}_"
    tape = {k: torch.from_numpy(g[tag + k]) for k in bptt_ref.TAPE_FIELDS}
    T, N = int(g["T"]), int(g["N"])
    # the thrust clamp of CTBRCfg (controller_diff.py:96-99) in python doubles
    k2, k1, k0 = 1.3298253500372892e-06, 0.0038360810526746033, -1.7689986848125325
    consts = {"dt": float(g["dt"]), "gravity": 9.81, "thrust_ratio": 3.0, "rate_bound": 6.0,
              "thrust_lo": 4 * (k2 * 150 ** 2 + k1 * 150 + k0), "thrust_hi": 4 * (k2 * 3000 ** 2 + k1 * 3000 + k0),
              "inertia": list(g["inertia_nominal"]), "dr_plant": 1, "lag": lag, "gamma": float(g["gamma"]),
              "weights": list(g["weights"]), "scale": 1.0 / (T * N)}
    assert int(tape["done"].sum()) == 4 and tape["done"][0, 0, 0] == 1 and tape["done"][5, 47, 0] == 1
    out = bptt_ref.window(tape, consts, a=torch.from_numpy(g[tag + "a"]))
    for name, want in (("losses", g[tag + "losses"]), ("terms", g[tag + "terms"]), ("grad", g[tag + "grad"])):
        want = torch.from_numpy(want)
        err = float((out[name] - want).abs().max())
        top = float(want.abs().max())
        assert top > 0
        assert err <= 1e-9 * top, (name, err, top)
    # and the tape's own leaf (u, shifted by the lag) gives the same gradient
    out_u = bptt_ref.window(tape, consts)
    assert float((out_u["grad"] - out["grad"]).abs().max()) <= 1e-9 * float(out["grad"].abs().max())
