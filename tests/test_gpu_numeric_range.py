"""The scalar arithmetic of bore_amd/csrc/mlp_math.h outside the band the other parity suites live in (hidden
pre-activations in [-2.2, 2.2], |logit| <= 2.1): saturated logits, the seams of the fit's hand-written exp / elu,
saturated activation gradients, and Adam from prepared slots -- read through the public entry points, finite values only.

Probe networks.  Every kernel matrix is a selector (at most one nonzero per row and per column; the nonzero is 1, a
power of two, or -- in the output layer behind an activation of exactly 1 -- the probed logit), so every MFMA sum has at
most one nonzero term and the pre-activation of a probed unit IS the table value (tests/test_numeric_range_host.py
asserts this in float32 and float64).  One Adam step on one row from m = v = 0 then returns, for every parameter, its
gradient (m / (1 - beta1)), the gradient's square (v / (1 - beta2)), the row's loss and the first update; `n_models`
covers a sweep in one launch.  The reference is oracle.fit in float64 on the same network with the float32-rounded
hyper-parameters the kernel receives (bore_adam_cfg holds floats: 1 - 0.9f differs from 0.1 by 4 x 2^-24).

Tolerances.  None of the suite's absolute terms: every bound is a count of roundings times 2^-24 times a float64
reference magnitude, carried through the network to first order by `grad_tolerances` / `adam_tolerances` below, where
each constant is derived.  Results whose reference lies under 2^-126 (below the normal float32 range, where the fit's
hardware exp2 / rcp / sqrt flush) are held to 2^-126 absolute.  tools/numeric_range_margin.py restates every
comparison with the float32 oracle in the kernel's place (profiles/numeric_range/oracle_margin.json: at most half of
each tolerance) and with five deliberately wrong formulas (three leave their tolerance by more than 3e5; two cannot
leave it, see test_numeric_range_host.py).  On the device every comparison records its worst error / tolerance
(profiles/numeric_range/parity_measured.json).

Sections: 1 the table, 2 the fit kernels (float32 flavours at B = 1 and B = 64; the bfloat16 fit against
oracle.loss_and_grads_bf16 on bfloat16-rounded values), 3 the IEEE-form kernels (forward, evaluate, value + input
gradient, screening ties, a flat restart; float32, streamed and bfloat16), 4 the LSTM kernels with saturated gates.
"""
import numpy as np
import pytest
import torch

from bore_amd import _lib, ops
from conftest import record_measurement
from numeric_range import *  # noqa: F401,F403  (the table, the probe networks, the tolerances, the references)
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

_measured = {}


SWITCHES = ("BORE_FIT_W8", "BORE_FIT_PAD", "BORE_STREAM")


def _switch(monkeypatch, env):
    """The kernel-choice switches of one flavour, and none of the others (as the existing tests set them)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- the device side ------------------------------------------------------------------------------------------------------
def gpu_fit(name, launch, B):
    D, units, out, _, env = ALL_FIT[name]
    desc = _lib.make_desc(D, units, launch["acts"], compute="bfloat16" if launch["bf16"] else "float32")
    models = launch["models"]
    L = len(models)
    th0 = np.stack([pack(k["p"]) for k in models])
    th = dev(th0)
    m = dev(np.stack([np.full(th0.shape[1], k.get("m0", 0.0), dtype=F32) for k in models]))
    v = dev(np.stack([np.full(th0.shape[1], k.get("v0", 0.0), dtype=F32) for k in models]))
    t = dev(np.array([k.get("t0", 0) for k in models], dtype=np.int64))
    X = dev(np.stack([k["row"] for k in models]).astype(F32).reshape(L, 1, D))
    z = dev(np.array([[k["z"]] for k in models], dtype=F32))
    perm = torch.zeros((L, 1, 1), dtype=torch.int32, device="cuda")
    lr, b1, b2 = launch["cfg"]
    loss = ops.mlp_fit(desc, th, m, v, t, X, z, 1, B, perm=perm, lr=lr, beta1=b1, beta2=b2, eps=EPS)
    torch.cuda.synchronize()
    th1 = th.cpu().numpy()
    return [dict(m=a, v=b, upd=c.astype(np.float64) - d.astype(np.float64), loss=e[0], t=int(f), theta=c)
            for a, b, c, d, e, f in zip(m.cpu().numpy(), v.cpu().numpy(), th1, th0, loss.cpu().numpy(), t.cpu().numpy())]


def _record(test, case, values):
    _measured.setdefault(test, {})[case] = values
    record_measurement("numeric_range/" + test, _measured[test])


def _run_fit_sweep(monkeypatch, name, sweep):
    _switch(monkeypatch, ALL_FIT[name][4])
    if name.startswith("streamed native"):          # premise: every entry point streams this network by itself
        assert ops.mlp_streamed(_lib.make_desc(ALL_FIT[name][0], ALL_FIT[name][1], _acts(len(ALL_FIT[name][1]), "relu", "linear"))) == 7
    worst, ran = {}, 0
    for B in ([64] if name in BF16_FIT else BATCHES):
        for launch, rows in sweep_reference(name, sweep):
            try:
                got = gpu_fit(name, launch, B)
            except _lib.UnsupportedError as e:            # listed with the library's message, not skipped silently
                _record("fit_" + sweep, "%s B=%d" % (name, B), {"unsupported": str(e)})
                continue
            ran += 1
            for (mdl, T), G in zip(rows, got):
                assert G["t"] == T["t"], (name, mdl["label"])              # adam_t is exact
                assert np.isfinite(G["theta"]).all() and np.isfinite(G["loss"]), (name, B, mdl["label"])
                r = ratios(G, T)
                for k, val in r.items():
                    if val > worst.get(k, (0.0, ""))[0]:
                        worst[k] = (val, "B=%d %s %s" % (B, launch["acts"], mdl["label"]))
                if sweep == "logit":
                    # sig - z never has the wrong sign: d loss / d logit is the output bias's gradient, m / (1 - beta1)
                    d = float(G["m"][-1])
                    assert d <= 0 if mdl["z"] == 1.0 else d >= 0, (name, B, mdl["label"], d)
    for k, (val, where) in sorted(worst.items()):
        print("%-28s %-8s %-6s %.3g of tol at %s" % (name, sweep, k, val, where))
    _record("fit_" + sweep, name, {k: round(val, 4) for k, (val, _) in worst.items()})
    assert ran, (name, sweep, "no launch was accepted")
    bad = {k: w for k, w in worst.items() if not (np.isfinite(w[0]) and w[0] <= 1.0)}
    assert not bad, (name, sweep, bad)


@pytest.mark.parametrize("name", list(ALL_FIT))
def test_fit_logit_sweep(gpu, monkeypatch, name):
    """d loss / d logit, every parameter's gradient and square, the row's loss and the first update at saturated
    logits (|x| up to 10 000, both labels, both sides of the 1 + e = 1 seam and of the 2^-126 and 2^-150 flushes)."""
    _run_fit_sweep(monkeypatch, name, "logit")


@pytest.mark.parametrize("name", [k for k, v in ALL_FIT.items() if len(v[1]) > 1])
def test_fit_hidden_sweep(gpu, monkeypatch, name):
    """Every hidden layer, every activation the flavour takes there: the activation (the next kernel's gradient reads
    every unit's output) and its derivative from a saturated output (the chain's unit), across the elu seam, ln 2,
    the relu kink and |a| up to 10 000."""
    _run_fit_sweep(monkeypatch, name, "hidden")


@pytest.mark.parametrize("name", list(ALL_FIT))
def test_fit_adam_sweep(gpu, monkeypatch, name):
    """adam_update and AdamClock from prepared slots: gradients from 0 and 1e-30 (g^2 underflows) to 1e19, v = 0 with
    m != 0, v = 1e30, t0 from 0 to 1e12, both beta pairs and learning rates; m', v', t and theta' - theta."""
    _run_fit_sweep(monkeypatch, name, "adam")


def _gpu_forward(D, units, acts, models, env):
    desc = _lib.make_desc(D, units, acts)
    th = dev(np.stack([pack(m["p"]) for m in models]))
    X = dev(np.stack([m["row"] for m in models]).astype(F32).reshape(len(models), 1, D))
    out = ops.mlp_forward(desc, th, X).cpu().numpy()[:, 0]
    return out


def _forward_sweep(name, D, units, env, fixed=None):
    worst = (0.0, "")
    for acts, models, ref, tol in forward_cases(D, units, fixed):
        np.testing.assert_allclose(forward_reference(acts, models), ref, rtol=1e-12, atol=0)   # the oracle agrees
        out = _gpu_forward(D, units, acts, models, env)
        assert np.isfinite(out).all(), (name, acts)
        diff = np.abs(out.astype(np.float64) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(diff == 0, 0.0, diff / tol)
        k = int(np.argmax(r))
        if r[k] > worst[0]:
            worst = (float(r[k]), models[k]["label"])
    print("%-28s forward %.3g of tol at %s" % (name, *worst))
    _record("forward", name, round(worst[0], 4))
    assert worst[0] <= 1.0, (name, worst)


@pytest.mark.parametrize("name", list(ACQ_FLAVOURS))
def test_forward_sweep(gpu, monkeypatch, name):
    """mlp_forward: act(x) at the logit sweep for every output activation and w_out * act(a) at the hidden sweep for every
    hidden activation and layer; relu and linear exactly, ocml's expm1f / tanhf / expf by their ulp bounds."""
    D, units, env = ACQ_FLAVOURS[name]
    _switch(monkeypatch, env)
    _forward_sweep(name, D, units, env)


def test_forward_sweep_static_shape_1(gpu, monkeypatch):
    _switch(monkeypatch, {})
    _forward_sweep("static 1 2-16-16-1", STATIC1[0], STATIC1[1], {}, fixed=STATIC1[2])


def _evaluate_sweep(name, D, units, env, outs=("linear", "sigmoid")):
    worst = (0.0, "")
    for out in outs:
        acts, single, (mix, acts_mix, X, z, mix_ref, mix_tol, mix_hits) = evaluate_cases(D, units, out)
        desc = _lib.make_desc(D, units, acts)
        th = dev(np.stack([pack(m["p"]) for m, _, _, _ in single]))
        Xs = dev(np.stack([m["row"] for m, _, _, _ in single]).astype(F32).reshape(len(single), 1, D))
        zs = dev(np.array([[m["z"]] for m, _, _, _ in single], dtype=F32))
        loss, acc = (a.cpu().numpy() for a in ops.mlp_evaluate(desc, th, Xs, zs))
        l65, a65 = (a.cpu().numpy() for a in ops.mlp_evaluate(
            _lib.make_desc(D, units, acts_mix), dev(pack(mix["p"])[None]), dev(X.astype(F32)[None]), dev(z.astype(F32)[None])))
        for (m, ref, tol, hit), l, a in zip(single, loss, acc):
            assert float(a) == hit, (name, out, m["label"], float(a), hit)
            r = _ratio(l, ref, tol)
            if r > worst[0]:
                worst = (r, "%s %s" % (out, m["label"]))
        assert round(float(a65[0]) * len(z)) == mix_hits and abs(float(a65[0]) - mix_hits / len(z)) <= U, (name, out, float(a65[0]))
        r = _ratio(l65[0], mix_ref, mix_tol)
        if r > worst[0]:
            worst = (r, "%s 65-row mix" % out)
    print("%-28s evaluate %.3g of tol at %s" % (name, *worst))
    _record("evaluate", name, round(worst[0], 4))
    assert worst[0] <= 1.0, (name, worst)


@pytest.mark.parametrize("name", list(ACQ_FLAVOURS))
def test_evaluate_sweep(gpu, monkeypatch, name):
    """mlp_evaluate's bce_loss at the logit sweep, one row per model and a 65-row mix; the accuracy of every row exact."""
    D, units, env = ACQ_FLAVOURS[name]
    _switch(monkeypatch, env)
    _evaluate_sweep(name, D, units, env)


def test_evaluate_sweep_static_shape_1(gpu, monkeypatch):
    _switch(monkeypatch, {})
    _evaluate_sweep("static 1 2-16-16-1", STATIC1[0], STATIC1[1], {}, outs=("sigmoid",))


@pytest.mark.parametrize("name", list(ACQ_FLAVOURS))
def test_accuracy_thresholds_the_output_at_exactly_one_half(gpu, monkeypatch, name):
    """accuracy_hit compares the OUTPUT with 0.5: a linear head at 0.5 and both float32 neighbours, a sigmoid head at
    logit 0 (output exactly 0.5) and +-2^-20, labels 0 and 1 -- every row its own model, and all rows of one model."""
    D, units, env = ACQ_FLAVOURS[name]
    _switch(monkeypatch, env)
    n = len(units)
    for out, xs in (("linear", HALF), ("sigmoid", [-2.0 ** -20, 0.0, 2.0 ** -20])):
        acts = _acts(n, "linear", out)
        desc = _lib.make_desc(D, units, acts)
        p, row = logit_model(D, units, 1.0, 1)
        cases = [(x, z) for x in xs for z in (0.0, 1.0)]
        o32 = [float(O.predict(p, acts, F32(x) * row[None])[0, 0]) for x, _ in cases]
        assert o32[2] == 0.5 and o32[0] < 0.5 < o32[4], o32                     # the float32 output IS one half, and is not
        hits = [float((o > 0.5) == (z > 0.5)) for o, (_, z) in zip(o32, cases)]
        assert hits == [1.0, 0.0, 1.0, 0.0, 0.0, 1.0]
        th = dev(np.stack([pack(p)] * len(cases)))
        X = dev(np.stack([F32(x) * row for x, _ in cases]).astype(F32).reshape(len(cases), 1, D))
        z = dev(np.array([[zz] for _, zz in cases], dtype=F32))
        _, acc = ops.mlp_evaluate(desc, th, X, z)
        _, acc_all = ops.mlp_evaluate(desc, th[:1].contiguous(), X.reshape(1, len(cases), D).contiguous(),
                                      z.reshape(1, len(cases)).contiguous())
        assert acc.cpu().numpy().tolist() == hits, (name, out, acc.cpu().numpy())
        assert abs(float(acc_all[0]) - 0.5) <= U, (name, out, float(acc_all[0]))
    _record("accuracy_at_one_half", name, "exact")


def test_accuracy_at_exactly_one_half_static_shape_1(gpu, monkeypatch):
    """Static shape 1 (relu, relu, sigmoid): the sigmoid head at logit 0 (output exactly 0.5) and +-2^-20, labels 0, 1."""
    _switch(monkeypatch, {})
    D, units, acts = STATIC1
    desc = _lib.make_desc(D, units, acts)
    cases = [(x, z) for x in (-2.0 ** -20, 0.0, 2.0 ** -20) for z in (0.0, 1.0)]
    models = [logit_model(D, units, x, i) for i, (x, _) in enumerate(cases)]
    o32 = [float(O.predict(p, acts, row[None])[0, 0]) for p, row in models]
    assert o32[2] == 0.5 and o32[0] < 0.5 < o32[4], o32
    hits = [float((o > 0.5) == (z > 0.5)) for o, (_, z) in zip(o32, cases)]
    assert hits == [1.0, 0.0, 1.0, 0.0, 0.0, 1.0]
    _, acc = ops.mlp_evaluate(desc, dev(np.stack([pack(p) for p, _ in models])),
                              dev(np.stack([row for _, row in models]).astype(F32).reshape(len(cases), 1, D)),
                              dev(np.array([[z] for _, z in cases], dtype=F32)))
    assert acc.cpu().numpy().tolist() == hits, acc.cpu().numpy()
    _record("accuracy_at_one_half", "static 1 2-16-16-1", "exact")


def _value_grad_sweep(name, D, units, env):
    worst = (0.0, "")
    desc = _lib.make_desc(D, units, _acts(len(units), "linear", "linear"))
    for transform, negate in TRANSFORM_CASES:
        p, acts, X, rv, tv, rg, tg = value_grad_case(D, units, transform, negate)
        val, grad = (a.cpu().numpy()[0] for a in ops.mlp_value_and_input_grad(desc, dev(pack(p)[None]), dev(X[None]),
                                                                               transform, negate))
        fin = _finite32(rv)
        assert fin.sum() >= len(rv) - 2
        # exp beyond the float32 range: the value is +inf, as the oracle's float32 answer; the gradient (inf * 0) is not compared
        assert np.array_equal(np.isposinf(val), ~fin), (name, transform, negate, val)
        r = max(_ratio(val[fin], rv[fin], tv[fin]), _ratio(grad[fin], rg[fin], tg[fin]))
        if r > worst[0]:
            worst = (r, "%s negate=%d" % (transform, negate))
        if transform == "sigmoid":           # u >= 17: T = 1 and dT = 0 exactly
            assert (val[np.array(VG_U) >= 17] == 1.0).all() and (grad[np.array(VG_U) >= 17] == 0.0).all()
    p, acts, X, rv, tv, rg, tg = value_grad_case(D, units, "exp", True, EXP_OVERFLOW)
    val, _ = ops.mlp_value_and_input_grad(desc, dev(pack(p)[None]), dev(X[None]), "exp", True)
    assert np.isposinf(val.cpu().numpy()).all() and (~_finite32(rv)).all() and (rv > 0).all()
    print("%-28s value_grad %.3g of tol at %s" % (name, *worst))
    _record("value_grad", name, round(worst[0], 4))
    assert worst[0] <= 1.0, (name, worst)


@pytest.mark.parametrize("name", list(ACQ_FLAVOURS))
def test_value_and_input_grad_sweep(gpu, monkeypatch, name):
    """objective_transform at u = +-17, +-40, +-88, +-104 for identity, sigmoid and exp, negated and not; exp at 89 and
    beyond is +inf."""
    D, units, env = ACQ_FLAVOURS[name]
    _switch(monkeypatch, env)
    _value_grad_sweep(name, D, units, env)


@pytest.mark.parametrize("b_out,const", [(100.0, 1.0), (-10000.0, 0.0)])
@pytest.mark.parametrize("name", SCREEN_FLAVOURS)
def test_screening_of_all_equal_predictions_takes_the_lowest_rows(gpu, monkeypatch, name, b_out, const):
    """Every prediction exactly 1.0 (or 0.0): screen_topk, sample_screen_topk and their streamed forms return rows
    0 .. R - 1, the documented tie rule."""
    D, units, env, compute = _acq(name)
    _switch(monkeypatch, env)
    p, acts = constant_model(D, units, b_out)
    desc = _lib.make_desc(D, units, acts, compute=compute)
    th = dev(np.stack([pack(p)] * 2))
    Ns, R = 300, 7
    X = np.random.RandomState(3).uniform(0, 1, size=(2, Ns, D))
    assert (O.predict(p, acts, X[0]) == const).all()
    lo, hi = np.zeros(D), np.ones(D)
    # (the LDS entry points refuse a network that only streams; the streamed ones take every network here)
    # (and the streamed kernels are float32 only)
    forms = [] if name.startswith("streamed native") else [(ops.screen_topk, ops.sample_screen_topk)]
    if compute == "float32":
        forms.append((ops.stream_screen_topk, ops.stream_sample_screen_topk))
    for screen, sample in forms:
        x0, idx, pred = (a.cpu().numpy() for a in screen(desc, th, dev(X), R, want_pred=True))
        assert (pred == const).all(), (name, pred.min(), pred.max())
        np.testing.assert_array_equal(idx, np.broadcast_to(np.arange(R), (2, R)))
        np.testing.assert_array_equal(x0, X[:, :R])
        x0, idx, pred = (a.cpu().numpy() for a in sample(desc, th, 5, Ns, lo, hi, R, want_pred=True))
        assert (pred == const).all()
        np.testing.assert_array_equal(idx, np.broadcast_to(np.arange(R), (2, R)))
    _record("screen_ties", "%s const=%g" % (name, const), "lowest rows")


@pytest.mark.parametrize("name", ["static 2 6-32-32-1", "generic -3 5-7-3-1", "generic 0 3-16x4-1",
                                  "streamed native 8-250-130-1", "bf16 static 3 16-64-64-64-1", "bf16 static 4 32-128-128-1"])
def test_restart_from_an_exactly_flat_point(gpu, monkeypatch, name):
    """lbfgsb_minimize / stream_lbfgsb_minimize / the bfloat16 kernel from a point where the gradient is exactly 0: nit = 0, nfev = 1, x = x0,
    the record the host build gives bit for bit (which the CPU file holds to SciPy's)."""
    import lbfgsb_host as H
    D, units, env, compute = _acq(name)
    _switch(monkeypatch, env)
    p, acts = flat_model(D, units)
    desc = _lib.make_desc(D, units, acts, compute=compute)
    th = dev(pack(p)[None])
    X0 = np.random.RandomState(8).uniform(0, 1, size=(1, 3, D))
    lo, hi = np.zeros(D), np.ones(D)
    entry = ops.stream_lbfgsb_minimize if name.startswith("streamed") else ops.lbfgsb_minimize
    x, fun, jac, info = (t.cpu().numpy() for t in entry(desc, th, dev(X0), lo, hi, "sigmoid", True, maxiter=5))

    def fg(xx):
        v, g = ops.mlp_value_and_input_grad(desc, th, dev(np.atleast_2d(xx)[None]), "sigmoid", True)
        return v.cpu().numpy()[0, 0], g.cpu().numpy()[0, 0]
    for r in range(3):
        h = H.minimize(fg, X0[0, r], (lo, hi), maxiter=5)
        assert (h.nit, h.nfev, h.status) == (0, 1, 0)
        np.testing.assert_array_equal(x[0, r], X0[0, r])
        np.testing.assert_array_equal(fun[0, r], 1.0)
        np.testing.assert_array_equal(jac[0, r], np.zeros(D))
        np.testing.assert_array_equal([h.nit, h.nfev, h.status, *h.task], info[0, r])
    _record("flat_restart", name, "nit=0 nfev=1 status=0")


def _lstm_close(test, label, got, ref, ref32, tol, worst):
    from test_gpu_lstm_shapes import _ratio as lratio
    dev32 = lratio(ref32, ref, **tol)
    k = max(1.0, 8.0 * dev32)
    assert k == 1.0, (test, label, dev32)       # (as in the LSTM suite: a widened bound must be looked at, not used unseen)
    r = lratio(got, ref, **{n: v * k for n, v in tol.items()})
    print("%-14s %-34s kernel %.3g of tol   fp32 oracle %.3g -> factor %.3g" % (test, label, r, dev32, k))
    assert np.isfinite(r) and r <= 1.0, (test, label, r, k)
    return max(worst, r), max(k, 1.0)


@pytest.mark.parametrize("key", list(LSTM_NETS))
def test_lstm_with_saturated_gates(gpu, key):
    """lstm_forward (both forms), lstm_evaluate, one lstm_fit step and lstm_value_and_input_grad against the float64
    oracle with the gates at 0 and 1 to float32 resolution and the cell state beyond 10."""
    import lstm_oracle as LO
    from test_gpu_lstm_shapes import (ADAM, EVAL_LOSS_TOL, FWD_TOL, GRAD_TOL, MV, VAL_TOL, _desc, _dev, _gpu_fit,
                                      _oracle_fit, _thetas)
    from test_gpu_lstm import FIT_TOL
    D, H, L, act = LSTM_NETS[key][:4]
    p, act, X32, Y, x = lstm_case(key)
    p32 = LO.as_dtype(p, F32)
    desc, th = _desc(D, H, L, act), _thetas([p])
    w, kmax = 0.0, 1.0
    out = ops.lstm_forward(desc, th, _dev(X32)[None], mask_value=MV)[0].cpu().numpy()
    w, k = _lstm_close(key, "forward many-to-many", out, LO.forward(p, act, X32, MV), LO.forward(p32, act, X32, MV, dtype=F32),
                       FWD_TOL, w)
    kmax = max(kmax, k)
    x32 = x.astype(F32)
    o2o = ops.lstm_forward(desc, th, _dev(x32)[None], num_steps=LSTM_T)[0].cpu().numpy()
    w, k = _lstm_close(key, "forward one-to-one", o2o, LO.one_to_one(p, act, x32, LSTM_T),
                       LO.one_to_one(p32, act, x32, LSTM_T, dtype=F32), FWD_TOL, w)
    kmax = max(kmax, k)
    # evaluate (no live logit within 1e-3 of the accuracy threshold: premise of the exact comparison)
    logits = LO.forward(p, act, X32, MV)
    live = np.any(X32 != MV, axis=-1)
    assert np.min(np.abs(logits[live] - 0.5)) > 1e-3
    loss, acc = ops.lstm_evaluate(desc, th, _dev(X32)[None], _dev(Y)[None], mask_value=MV)
    rl, ra = LO.evaluate(p, act, X32, Y, MV)
    w, k = _lstm_close(key, "evaluate loss", float(loss[0]), rl, LO.evaluate(p32, act, X32, Y, MV, dtype=F32)[0], EVAL_LOSS_TOL, w)
    kmax = max(kmax, k)
    np.testing.assert_allclose(float(acc[0]), ra, atol=1e-6)
    # one Adam step
    perms = np.random.RandomState(5).permutation(LSTM_N)[None].astype(np.int32)
    got = _gpu_fit(desc, [p], X32[None], Y[None], perms[None], 64, ADAM)
    ref = _oracle_fit(p, act, X32, Y, perms, 64, None, None, ADAM)
    ref32 = _oracle_fit(p, act, X32, Y, perms, 64, None, None, ADAM, dtype=F32)
    assert int(got["t"][0]) == ref["t"] == 1
    for name in ("loss", "theta", "m", "v"):
        w, k = _lstm_close(key, "fit " + name, got[name][0], ref[name], ref32[name], FIT_TOL[name], w)
        kmax = max(kmax, k)
    for transform in ("identity", "sigmoid"):
        val, grad = ops.lstm_value_and_input_grad(desc, th, _dev(x, np.float64)[None], LSTM_T, transform, True)
        rv, rg = LO.value_and_input_grad(p, act, x32, LSTM_T, transform, True)
        r32 = LO.value_and_input_grad(p32, act, x32, LSTM_T, transform, True, dtype=F32)
        w, k = _lstm_close(key, "value " + transform, val[0].cpu().numpy(), rv, r32[0], VAL_TOL, w)
        kmax = max(kmax, k)
        w, k = _lstm_close(key, "gradient " + transform, grad[0].cpu().numpy(), rg, r32[1], GRAD_TOL, w)
        kmax = max(kmax, k)
    _record("lstm", key, {"worst": round(w, 4), "largest_factor": round(kmax, 3)})


# ---- the bfloat16 acquisition kernels (the two wide static shapes) ------------------------------------------------------------
@pytest.mark.parametrize("name", list(BF16_FIT))
def test_bf16_forward_and_value_grad_sweep(gpu, monkeypatch, name):
    """compute = bfloat16: mlp_forward of the (bfloat16-rounded) logit and hidden sweeps under every activation, and
    mlp_value_and_input_grad at u = +-17 .. +-104, against the bfloat16 oracle.  Outputs are bfloat16-representable;
    relu and linear are exact; behind an inexact activation a last-bit difference of the float32 value may flip the
    rounding: one bfloat16 ulp.  The transformed VALUE is float32 arithmetic on an exact u: the float32 bounds."""
    D, units, _, _, _ = BF16_FIT[name]
    _switch(monkeypatch, {})
    n = len(units)
    logits = sorted(set(_bf(x) for x in LOGITS))
    worst = 0.0
    for out in HIDDEN_ACTS:
        acts = _acts(n, "relu", out)
        models = [dict(zip(("p", "row"), logit_model(D, units, x, i))) for i, x in enumerate(logits)]
        desc = _lib.make_desc(D, units, acts, compute="bfloat16")
        got = ops.mlp_forward(desc, dev(np.stack([pack(m["p"]) for m in models])),
                              dev(np.stack([m["row"] for m in models]).astype(F32).reshape(len(models), 1, D))).cpu().numpy()[:, 0]
        ref = np.array([O.forward_bf16([a.astype(F32) for a in m["p"]], acts, m["row"][None])[0, 0] for m in models])
        assert np.array_equal(got, O.bf16_round(got)), (name, out)
        if out in ("linear", "relu"):
            np.testing.assert_array_equal(got, ref)
        else:
            tol = _bf16_ulp(ref) + _floor(ref)
            worst = max(worst, _ratio(got, ref, tol))
    # the hidden sweep: w_out * act(a) in every hidden layer under every activation (h and the output are rounded; the
    # scaling by a power of two is exact)
    for layer in range(1, n):
        for act in HIDDEN_ACTS:
            values = sorted(set(_bf(a) for a in HIDDEN + (RELU_KINK if act == "relu" else [])))
            acts = _acts(n, "linear", "linear")
            acts[layer - 1] = act
            models = [dict(zip(("p", "row"), hidden_model(D, units, layer, values, i))) for i in range(len(values))]
            desc = _lib.make_desc(D, units, acts, compute="bfloat16")
            got = ops.mlp_forward(desc, dev(np.stack([pack(m["p"]) for m in models])),
                                  dev(np.stack([m["row"] for m in models]).astype(F32).reshape(len(models), 1, D))).cpu().numpy()[:, 0]
            ref = np.array([O.forward_bf16([a.astype(F32) for a in m["p"]], acts, m["row"][None])[0, 0] for m in models])
            assert np.array_equal(got, O.bf16_round(got)), (name, layer, act)
            if act in ("linear", "relu"):
                np.testing.assert_array_equal(got, ref)
            else:
                worst = max(worst, _ratio(got, ref, _bf16_ulp(ref) + _floor(ref)))
    desc = _lib.make_desc(D, units, _acts(n, "linear", "linear"), compute="bfloat16")
    for transform, negate in TRANSFORM_CASES:
        p, acts, X, rv, tv, rg, tg = value_grad_case(D, units, transform, negate)
        val, grad = (a.cpu().numpy()[0] for a in ops.mlp_value_and_input_grad(desc, dev(pack(p)[None]), dev(X[None]),
                                                                               transform, negate))
        with np.errstate(over="ignore", invalid="ignore"):
            bv, bg = O.value_and_input_grad_bf16([a.astype(F32) for a in p], acts, X, transform, negate)
        fin = _finite32(rv)
        assert np.array_equal(np.isposinf(val), ~fin) and np.array_equal(np.isposinf(bv), ~fin)
        worst = max(worst, _ratio(val[fin], rv[fin], tv[fin]))
        exact = transform == "identity"
        worst = max(worst, _ratio(grad[fin], bg[fin], (0.0 if exact else 1.0) * _bf16_ulp(bg[fin]) + _floor(bg[fin])))
        assert np.array_equal(grad[fin].astype(F32), O.bf16_round(grad[fin].astype(F32)))
    print("%-28s bf16 forward / value_grad %.3g of tol" % (name, worst))
    _record("bf16_acquisition", name, round(worst, 4))
    assert worst <= 1.0, (name, worst)
