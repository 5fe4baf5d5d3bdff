"""The PPO update's scalar kernels (csrc/gr_update.hip) called directly through _abi.call with GrPpoLossArgs /
GrAdamArgs, no policy around them, against the float64 restatement and bounds of tests/update_ref.py (shown fair and
sharp by tests/test_update_ref_cpu.py; logf / expf / sqrtf are counted at an assumed 2 ulp).

Losses (gr_ppo_loss_forward, _backward, _forward_loss, _backward_loss, _forward_backward): 24 cases over rows {1, 63,
64, 65, 255, 256, 257, 1031, 4099}, k {1, 2, 3, 4, 5, 8}, both value losses and clips 0.2 / 0.1, each with contiguous
tensors and with every input a column slice of one packed [rows, 61] buffer (bit-identical).  Every element of dmu and
dvalue, dstd, the sums, the means, the loss, acc (pre-loaded, and null) and kl_out are held to the bounds; 64 guard
rows past dmu / dvalue stay untouched; the scratch is poisoned with NaN; the combined and the one-pass forms equal the
two-pass form bit for bit, as do repeats.  Non-finite rows follow torch's autograd.

Adam (gr_adam_clip, _step, _clip_step over gr_adam_prepare's table) on segments of 1 .. 5000 elements, up to the
maximum of 64, at odd offsets with sentinel gaps, step counts up to 5e6, and gr_adaptive_lr on a table of KL values
either side of its fp32 thresholds."""
import ctypes as C

import numpy as np
import pytest
import torch

import update_ref as R
from generalizableracing_amd import _abi
from generalizableracing_amd._abi import GrAdamArgs, GrAdamSegment, GrPpoLossArgs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_COEF = 0.5
G_LOSS = 0.75
G2 = (G_LOSS, R.f32(np.float32(VALUE_COEF) * np.float32(G_LOSS)))  # the two-pass form's upstream gradients
GUARD, SENTINEL = 64, 12345.0
LD = 61  # the packed buffer's odd row stride
COLS = dict(mu=3, act=13, mu_old=23, sig_old=33, value=45, logp_old=47, adv=49, value_old=51, ret=53)
ACC0 = (1.5, -2.25)


def _stream():
    return _abi.raw_stream(torch.device(DEV))


# ---------------------------------------------------------------------------------------------------- losses
def _device_inputs(inp, packed):
    """The inputs on the device: contiguous, or column slices of one packed [rows, LD] buffer (std contiguous)."""
    if not packed:
        return {n: inp[n].to(DEV) for n in R.LOSS_FIELDS}
    rows, k = inp["mu"].shape
    buf = torch.full((rows, LD), 9.0e9, device=DEV)
    out = {"std": inp["std"].to(DEV)}
    for n, c in COLS.items():
        w = k if inp[n].dim() == 2 else 1
        buf[:, c:c + w] = inp[n].to(DEV).reshape(rows, w)
        out[n] = buf[:, c:c + w]
        assert out[n].stride(0) == LD and out[n].storage_offset() == c
    return out


def _loss_args(t, clip, clipped):
    a = GrPpoLossArgs()
    a.rows, a.k = t["mu"].shape
    a.clipped_value, a.clip = int(clipped), float(clip)
    for n in R.LOSS_FIELDS:
        setattr(a, n, t[n].data_ptr())
        if n != "std":
            setattr(a, "ld_" + n, t[n].stride(0))
    return a


def _run_losses(inp, clip, clipped, packed=False, poison=float("nan"), with_acc=True):
    """Every form once; returns CPU tensors keyed form.name.  Scratch is filled with `poison` before each call."""
    t = _device_inputs(inp, packed)
    a = _loss_args(t, clip, clipped)
    rows, k = inp["mu"].shape
    npart = _abi.load().gr_ppo_loss_partials(rows)
    s = _stream()
    out = {}
    new = lambda *shape: torch.full(shape, SENTINEL, device=DEV)
    scratch = lambda: torch.full((npart,), poison, device=DEV)
    g2 = torch.tensor(G2, device=DEV)
    gl = torch.tensor([G_LOSS], device=DEV)

    def grads(form, fn):
        dmu, dvalue, dstd = new(rows + GUARD, k), new(rows + GUARD), new(k)
        fn(dmu, dvalue, dstd)
        out[form + ".dmu"], out[form + ".dvalue"], out[form + ".dstd"] = dmu, dvalue, dstd

    def heads(form):
        h = dict(sums=new(3), loss=new(1), stats=new(3), acc=torch.tensor(ACC0, device=DEV), kl_out=new(1))
        for n, v in h.items():
            out[form + "." + n] = v
        accp, klp = (h["acc"].data_ptr(), h["kl_out"].data_ptr()) if with_acc else (None, None)
        return h, accp, klp

    part = scratch()
    out["F.sums"] = new(3)
    _abi.call("gr_ppo_loss_forward", C.byref(a), part.data_ptr(), out["F.sums"].data_ptr(), s)
    part_b = scratch()
    grads("B", lambda dmu, dv, ds: _abi.call("gr_ppo_loss_backward", C.byref(a), g2.data_ptr(), dmu.data_ptr(),
                                             dv.data_ptr(), part_b.data_ptr(), ds.data_ptr(), s))
    part_fl = scratch()
    h, accp, klp = heads("FL")
    _abi.call("gr_ppo_loss_forward_loss", C.byref(a), part_fl.data_ptr(), h["sums"].data_ptr(), VALUE_COEF,
              h["loss"].data_ptr(), h["stats"].data_ptr(), accp, klp, s)
    part_bl = scratch()
    grads("BL", lambda dmu, dv, ds: _abi.call("gr_ppo_loss_backward_loss", C.byref(a), gl.data_ptr(), VALUE_COEF,
                                              dmu.data_ptr(), dv.data_ptr(), part_bl.data_ptr(), ds.data_ptr(), s))
    part_fb, dpart_fb = scratch(), scratch()
    h, accp, klp = heads("FB")
    grads("FB", lambda dmu, dv, ds: _abi.call(
        "gr_ppo_loss_forward_backward", C.byref(a), gl.data_ptr(), VALUE_COEF, part_fb.data_ptr(), h["sums"].data_ptr(),
        h["loss"].data_ptr(), h["stats"].data_ptr(), accp, klp, dmu.data_ptr(), dv.data_ptr(), dpart_fb.data_ptr(),
        ds.data_ptr(), s))
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in out.items()}


def _same_bits(a, b):
    """The same bits element by element (a NaN matches a NaN: its payload is not part of any promise)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def _assert_forms_agree(o, rows):
    """The combined forms and the one-pass form against the two-pass form, bit for bit; the guard rows."""
    for form in ("B", "BL", "FB"):
        for n in ("dmu", "dvalue"):
            assert bool((o[f"{form}.{n}"][rows:] == SENTINEL).all()), (form, n, "guard rows written")
    for form in ("BL", "FB"):
        for n in ("dmu", "dvalue", "dstd"):
            assert _same_bits(o[f"{form}.{n}"], o[f"B.{n}"]), (form, n)
    # the means and the loss composed from gr_ppo_loss_forward's sums in the header's fp32 operations
    sums = o["F.sums"].numpy()
    inv = np.float32(1.0) / np.float32(rows)
    means = sums * inv
    loss = np.float32(means[0] + np.float32(VALUE_COEF) * means[1])
    for form in ("FL", "FB"):
        assert _same_bits(o[form + ".sums"], o["F.sums"]), form
        assert _same_bits(o[form + ".stats"], torch.from_numpy(means)), form
        assert _same_bits(o[form + ".loss"], torch.from_numpy(np.array([loss]))), form
    return means, loss


def _head_tensors(o):
    return dict(dmu=None, dvalue=None, sums=o["F.sums"], means=o["FL.stats"], loss=o["FL.loss"][0], dstd=o["B.dstd"])


@pytest.mark.parametrize("case", R.loss_cases(), ids=lambda c: "r{}-k{}-cv{}-c{}".format(*c[:4]))
def test_ppo_loss_kernels_match_float64(case):
    rows, k, clipped, clip, seed = case
    inp = R.loss_inputs(rows, k, clip, seed)
    ref = R.ppo_loss_ref(inp, clip, clipped, VALUE_COEF, G2)
    bnd = R.error_bounds(ref, inp, clip, clipped, VALUE_COEF, G2)
    assert int(bnd["exempt"].sum()) <= R.EXEMPT_CAP * rows and not bool((bnd["exempt"] & inp["edge"]).any())
    o = _run_losses(inp, clip, clipped)
    means, loss = _assert_forms_agree(o, rows)
    # acc += (surrogate, value) means; kl_out = the KL mean
    for form in ("FL", "FB"):
        acc = np.array(ACC0, dtype=np.float32) + means[:2]
        assert _same_bits(o[form + ".acc"], torch.from_numpy(acc)), form
        assert _same_bits(o[form + ".kl_out"], torch.from_numpy(means[2:3])), form
    # against float64
    got = _head_tensors(o)
    got["dmu"], got["dvalue"] = o["B.dmu"][:rows], o["B.dvalue"][:rows]
    r = R.loss_ratios(got, ref, bnd)
    print(f"rows {rows} k {k} clipped {clipped} clip {clip}: error / bound per row {r['rows']:.3f} sums {r['sums']:.3f}"
          f" exempt {int(bnd['exempt'].sum())}")
    R.record("gpu", "loss_rows", r["rows"])
    R.record("gpu", "loss_sums", r["sums"])
    assert r["rows"] <= 1.0 and r["sums"] <= 1.0, r
    for j in range(2):  # acc: the mean's bound and one addition
        err = abs(float(o["FL.acc"][j]) - (ACC0[j] + float(ref["means"][j])))
        assert err <= float(bnd["means"][j]) + R.U * abs(ACC0[j] + float(ref["means"][j]))
    # the packed layout, a zero-filled scratch (a repeat) and null acc / kl_out: the same bits
    for other in (_run_losses(inp, clip, clipped, packed=True), _run_losses(inp, clip, clipped, poison=0.0),
                  _run_losses(inp, clip, clipped, packed=True, with_acc=False)):
        for n, v in o.items():
            if n.endswith(".acc") or n.endswith(".kl_out"):
                continue
            assert _same_bits(other[n], v), n
    null = _run_losses(inp, clip, clipped, with_acc=False)
    for form in ("FL", "FB"):  # null sinks: not written
        assert _same_bits(null[form + ".acc"], torch.tensor(ACC0)) and float(null[form + ".kl_out"]) == SENTINEL


def test_ppo_loss_nonfinite_rows_follow_torch():
    """Row 5: logp_old -1e30 (ratio inf) with advantage 0; row 9: a NaN return; row 200: a NaN advantage; row 257:
    logp_old +1e30 (ratio 0).  The non-finite elements of dmu, dvalue, dstd and the sums are those of torch's autograd
    on the same inputs, and every other row is bit-identical to a run with ordinary values in those four rows.  Where
    float64 and fp32 torch disagree about a position, fp32 torch on the CPU decides: the kernel promises torch's
    fp32 behaviour (an overflow to inf happens in fp32 only)."""
    bad, plain = R.nonfinite_inputs()
    for clipped in (1, 0):
        want = R.ppo_loss_ref(bad, 0.2, clipped, VALUE_COEF, G2, dtype=torch.float32)
        o = _run_losses(bad, 0.2, clipped)
        p = _run_losses(plain, 0.2, clipped)
        _assert_forms_agree(o, 300)
        for n, w in (("B.dmu", want["dmu"]), ("B.dvalue", want["dvalue"]), ("B.dstd", want["dstd"]),
                     ("F.sums", want["sums"])):
            got = o[n][:300] if n in ("B.dmu", "B.dvalue") else o[n]
            assert torch.equal(torch.isfinite(got), torch.isfinite(w)), (n, clipped)
            assert torch.equal(torch.isnan(got), torch.isnan(w)), (n, clipped)
        rest = torch.ones(300, dtype=torch.bool)
        rest[list(R.NONFINITE_ROWS)] = False
        for n in ("B.dmu", "B.dvalue"):
            assert _same_bits(o[n][:300][rest], p[n][:300][rest]), n


# ----------------------------------------------------------------------------------------------- Adam, clip
BETAS, EPS = (0.9, 0.999), 1.0e-8
GAP = 777.0


class _Segments:
    """Parameters, gradients and moments as views into flat buffers at odd element offsets with sentinel gaps; the
    last segment of `sizes` is kept out of the table (a parameter without gradient).  Step slots are the segments'
    indices reversed."""

    def __init__(self, sizes, seed, steps_before, lr=1.0e-3, lr_tensor=False):
        self.sizes = sizes
        self.n = len(sizes) - 1  # in the table
        self.off, off = [], 1
        for n in sizes:
            self.off.append(off)
            off += n + 3
            off += 1 - off % 2  # odd
        self.total = off
        p, g, m, v = R.adam_state(self.total, seed)
        self.host = dict(p=p, g=g, m=m, v=v)
        self.dev = {n: torch.full((self.total,), GAP, device=DEV) for n in "pgmv"}
        for n in "pgmv":
            for o, sz in zip(self.off, sizes):
                self.dev[n][o:o + sz] = self.host[n][o:o + sz].to(DEV)
        self.slot = [len(sizes) - 1 - s for s in range(len(sizes))]
        self.steps_before = torch.tensor([float(steps_before[q % len(steps_before)]) for q in range(len(sizes))])
        self.step = self.steps_before.to(DEV)
        self.coef = torch.zeros(2 * len(sizes), device=DEV)
        self.norm = torch.full((1,), SENTINEL, device=DEV)
        self.lr_dev = torch.tensor([lr], device=DEV, dtype=torch.float32)
        table = (GrAdamSegment * self.n)()
        for s in range(self.n):
            e = table[s]
            e.param, e.grad, e.exp_avg, e.exp_avg_sq = (self.dev[n].data_ptr() + 4 * self.off[s] for n in "pgmv")
            e.numel, e.step_slot = sizes[s], self.slot[s]
        nblocks = C.c_int32()
        _abi.call("gr_adam_prepare", table, self.n, C.byref(nblocks))
        assert nblocks.value == sum((n + 1023) // 1024 for n in sizes[:self.n])
        self.table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
        self.part = torch.full((nblocks.value,), float("nan"), device=DEV, dtype=torch.float64)
        a = GrAdamArgs()
        a.nseg, a.nblocks = self.n, nblocks.value
        a.lr, a.beta1, a.beta2, a.eps = float(lr), BETAS[0], BETAS[1], EPS
        a.lr_ptr = self.lr_dev.data_ptr() if lr_tensor else None
        a.step, a.coef, a.part, a.seg = (self.step.data_ptr(), self.coef.data_ptr(), self.part.data_ptr(),
                                         self.table.data_ptr())
        self.args = a

    def set_grads(self, fn):
        """Replace the gradients (host and device) by fn(host gradient) inside the segments."""
        for o, sz in zip(self.off, self.sizes):
            self.host["g"][o:o + sz] = fn(self.host["g"][o:o + sz])
            self.dev["g"][o:o + sz] = self.host["g"][o:o + sz].to(DEV)

    def expected(self, name):
        """The untouched device buffer: the host state inside the segments, the sentinel in the gaps."""
        out = torch.full((self.total,), GAP)
        for o, sz in zip(self.off, self.sizes):
            out[o:o + sz] = self.host[name][o:o + sz]
        return out

    def seg(self, name, s, dev=True):
        src = self.dev[name].cpu() if dev else self.host[name]
        return src[self.off[s]:self.off[s] + self.sizes[s]]

    def assert_untouched_outside_table(self):
        """The gaps keep their sentinel, the left-out segment its state and its step count."""
        inside = torch.zeros(self.total, dtype=torch.bool)
        for o, sz in zip(self.off, self.sizes):
            inside[o:o + sz] = True
        last = len(self.sizes) - 1
        for n in "pgmv":
            assert bool((self.dev[n].cpu()[~inside] == GAP).all()), n
            assert _same_bits(self.seg(n, last), self.seg(n, last, dev=False)), n
        assert float(self.step[self.slot[last]]) == float(self.steps_before[self.slot[last]])


def _signed(g, mag):
    return torch.where(g < 0, torch.full((), -mag), torch.full((), mag))


def _sizes(layout):
    return R.adam_layout(layout) + [300]  # + the segment left out of the table


@pytest.mark.parametrize("layout", ["a", "a_rev", "b", "c"])
def test_adam_clip_norm_and_scaling(layout):
    """gr_adam_clip: below max_norm the gradients keep their bits, above it they are scaled within bound; zero
    gradients stay zero with norm 0; gradients of 1e-25 (squares underflow in fp32) and of 1e17 (squares overflow fp32)
    still report the right norm: it is accumulated in double."""
    sizes = _sizes(layout)
    for name, fn, max_norm in (("below", lambda g: g, 1.0e3), ("above", lambda g: _signed(g, 0.5) + g, 0.01),
                               ("zero", lambda g: g * 0.0, 1.0), ("tiny", lambda g: _signed(g, 1.0e-25), 1.0),
                               ("huge", lambda g: _signed(g, 1.0e17), 1.0)):
        sg = _Segments(sizes, 21, [3.0])
        sg.set_grads(fn)
        grads = [sg.seg("g", s, dev=False) for s in range(sg.n)]
        norm, coef = R.clip_ref(grads, max_norm)
        _abi.call("gr_adam_clip", C.byref(sg.args), max_norm, sg.norm.data_ptr(), _stream())
        torch.cuda.synchronize()
        got_norm = sg.norm.cpu()[0]
        print(layout, name, float(got_norm), norm, coef)
        assert R.norm_within_2ulp(got_norm, norm), (name, float(got_norm), norm)
        assert (coef == 1.0) == (name in ("below", "zero", "tiny"))
        worst = 0.0
        for s in range(sg.n):
            got = sg.seg("g", s)
            if coef == 1.0:
                assert _same_bits(got, grads[s]), (name, s)
            else:
                worst = max(worst, float(((got.double() - grads[s].double() * coef).abs()
                                          / R.clip_grad_bound(grads[s], coef)).max()))
        assert worst <= 1.0, (name, worst)
        if coef < 1.0:
            R.record("gpu", "clip", worst)
        for n in "pmv":  # the clip touches gradients only
            assert _same_bits(sg.dev[n].cpu(), sg.expected(n)), n
        assert torch.equal(sg.step.cpu(), sg.steps_before)
        sg.assert_untouched_outside_table()


@pytest.mark.parametrize("lr_tensor", [False, True], ids=["host_lr", "lr_ptr"])
@pytest.mark.parametrize("layout", ["a", "a_rev", "b", "c"])
def test_adam_step_matches_float64(layout, lr_tensor):
    """gr_adam_step from a random fp32 state, the slots' step counts set so that the call computes t in {1, 2, 10,
    1000, 100000, 5000000} (different counts in one call), against adam_ref within adam_bounds."""
    sizes = _sizes(layout)
    sg = _Segments(sizes, 31, [t - 1 for t in R.T_STEPS], lr_tensor=lr_tensor)
    lr = float(sg.lr_dev.cpu()[0]) if lr_tensor else 1.0e-3
    if lr_tensor:
        sg.args.lr = 123.0  # (overridden by lr_ptr)
    _abi.call("gr_adam_step", C.byref(sg.args), _stream())
    torch.cuda.synchronize()
    worst = 0.0
    for s in range(sg.n):
        t = int(sg.steps_before[sg.slot[s]]) + 1
        assert float(sg.step.cpu()[sg.slot[s]]) == float(t)
        p, g, m, v = (sg.seg(n, s, dev=False) for n in "pgmv")
        p2, m2, v2, x = R.adam_ref(p, g, m, v, t, lr, BETAS, EPS)
        e_p, e_m, e_v = R.adam_bounds(p2, m2, v2, x)
        assert _same_bits(sg.seg("g", s), g)
        for got, want, e in ((sg.seg("p", s), p2, e_p), (sg.seg("m", s), m2, e_m), (sg.seg("v", s), v2, e_v)):
            worst = max(worst, float(((got.double() - want).abs() / e).max()))
    print(layout, lr_tensor, "adam error / bound", worst)
    R.record("gpu", "adam", worst)
    assert worst <= 1.0
    sg.assert_untouched_outside_table()


@pytest.mark.parametrize("kl", [None, 0.05, 0.001, 0.01], ids=["no_kl", "kl_high", "kl_low", "kl_mid"])
@pytest.mark.parametrize("layout", ["a", "a_rev", "b"])
def test_adam_clip_step_equals_the_three_calls(layout, kl):
    """gr_adam_clip_step against gr_adaptive_lr + gr_adam_clip + gr_adam_step on the same state: every buffer, the
    step counts, the norm and the rate bit for bit."""
    sizes = _sizes(layout)
    res = []
    for fused in (False, True):
        sg = _Segments(sizes, 41, [t - 1 for t in R.T_STEPS], lr_tensor=True)
        klp = torch.tensor([kl if kl is not None else 0.0], device=DEV)
        s = _stream()
        if fused:
            _abi.call("gr_adam_clip_step", C.byref(sg.args), 0.05, sg.norm.data_ptr(),
                      klp.data_ptr() if kl is not None else None, sg.lr_dev.data_ptr() if kl is not None else None,
                      0.01, 1.0e-5, 1.0e-2, s)
        else:
            if kl is not None:
                _abi.call("gr_adaptive_lr", klp.data_ptr(), sg.lr_dev.data_ptr(), 0.01, 1.0e-5, 1.0e-2, s)
            _abi.call("gr_adam_clip", C.byref(sg.args), 0.05, sg.norm.data_ptr(), s)
            _abi.call("gr_adam_step", C.byref(sg.args), s)
        torch.cuda.synchronize()
        sg.assert_untouched_outside_table()
        res.append([sg.dev[n].cpu() for n in "pgmv"] + [sg.step.cpu(), sg.norm.cpu(), sg.lr_dev.cpu()])
    for a, b in zip(*res):
        assert _same_bits(a, b)
    want_lr = np.float32(1.0e-3) if kl is None else R.adaptive_lr_ref(kl, 1.0e-3, 0.01, 1.0e-5, 1.0e-2)
    assert np.float32(res[1][-1][0]) == want_lr
    assert (kl in (0.05, 0.001)) == (want_lr != np.float32(1.0e-3))


@pytest.mark.parametrize("desired", [0.01, 0.008])
def test_adaptive_lr_table(desired):
    """gr_adaptive_lr bit-equal to adaptive_lr_ref for KL values either side of, and at, fp32(2 desired) and
    fp32(desired / 2), 0, -1e-3, NaN and +inf, and rates at, near and between lr_min and lr_max."""
    table = R.adaptive_lr_table(desired)
    kl = torch.tensor(np.array([k for k, _ in table], dtype=np.float32), device=DEV)
    lr = torch.tensor(np.array([r for _, r in table], dtype=np.float32), device=DEV)
    s = _stream()
    for i in range(len(table)):
        _abi.call("gr_adaptive_lr", kl.data_ptr() + 4 * i, lr.data_ptr() + 4 * i, desired, 1.0e-5, 1.0e-2, s)
    torch.cuda.synchronize()
    got = lr.cpu().numpy()
    for i, (k, r) in enumerate(table):
        want = np.float32(R.adaptive_lr_ref(k, r, desired, 1.0e-5, 1.0e-2))
        assert got[i].tobytes() == want.tobytes(), (float(k), float(r), float(got[i]), float(want))
