"""The LSTM kernels (bore_lstm_*) against the fp64 oracle tests/lstm_oracle.py at the shapes tests/test_gpu_lstm.py
does not reach: several models per launch, every architecture bound, odd unit counts, tiles and tails, 1 and 16
steps, a non-zero head bias, distinct l2 factors per slot, non-default Adam, fully masked data.

Every network here has a head bias drawn from +-[0.25, 0.5] (``_weights``).

Tolerances.  Cases no deeper than the existing ones (T <= 5, at most 3 layers, H <= 32, D <= 16) use the tolerances
of tests/test_gpu_lstm.py unchanged: FIT_TOL, forward rtol=atol=2e-5, value rtol=2e-5 atol=2e-6, gradient rtol=2e-4
atol=2e-5, evaluate loss rtol=2e-5.  The deep cases (T = 16, four layers, 54-57 units, D = 64) take their tolerance
from the CPU alone: the oracle's own arithmetic is run a second time with every array in float32
(``lstm_oracle.*(dtype=np.float32)``), its largest deviation from the float64 run is expressed in units of the
existing tolerance (max |f32 - f64| / (atol + rtol |f64|)), and the tolerance of that quantity is the existing one
times max(1, 8 x that deviation) -- 8 because the kernel's fmaf chains and tree sums round in another order than
NumPy's, so the float32 run gives the scale and not the bits.  The deviation is computed in the test, from the test's
own inputs, never from the kernel.  Measured (NumPy 2.2, x86-64), deviation in units of the existing tolerance and the
factor it gives (1 = the existing tolerance stands):

  fit + evaluate (D->LxH act T)    loss     theta    m        v        evaluate loss   factor
  16->2x32 tanh  T=16  N=65 B=64   0.0019   0.0011   0.013    0.013    3.7e-07         1
  2->4x8   tanh  T=16  N=64 B=64   0.0010   0.0008   0.0005   0.013    0.0024          1
  64->1x16 linear T=3  N=33 B=16   0.0008   0.0039   0.025    0.014    4.1e-05         1
  2->1x54  elu   T=16  N=65 B=64   0.0011   0.0015   0.0034   0.013    0.0002          1
  2->1x57  elu   T=1   N=64 B=64   0.0008   0.0006   0.0005   0.013    0.0006          1
  value + input gradient, 16 steps   value    gradient
  2->2x32 elu                        0.0078   0.0027                                   1
  16->2x32 tanh                      0.038    0.0037                                   1
  5->2x7 sigmoid                     0.0083   0.0002                                   1
  forward                            many-to-many T=16   one-to-one T=1   one-to-one T=16
  16->2x32 tanh                      0.0033              0.0007           0.0033        1
  2->4x8 elu                         0.0015              0.0006           0.0011        1

float32 rounding alone stays below 4 % of the existing tolerances at every deep shape (the 0.013 of v is
1 - float32(0.999) against 1 - 0.999, a relative 1.3e-5), so 8 x the deviation is below 1 everywhere and the existing
tolerances stand for the deep cases too.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_oracle as O  # noqa: E402
from test_gpu_lstm import FIT_TOL, _hyperband_sequences  # noqa: E402

pytestmark = pytest.mark.gpu

FWD_TOL = dict(rtol=2e-5, atol=2e-5)
VAL_TOL = dict(rtol=2e-5, atol=2e-6)
GRAD_TOL = dict(rtol=2e-4, atol=2e-5)
EVAL_LOSS_TOL = dict(rtol=2e-5)
MV = -1.0
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7)


# -- helpers ---------------------------------------------------------------------------------------------
def _weights(D, H, L, rs):
    """lstm_oracle.init_weights with a head bias away from zero, rounded to float32 (what the device holds)."""
    p = O.init_weights(D, H, L, rs)
    p[-1] = rs.choice([-1.0, 1.0], size=1) * rs.uniform(0.25, 0.5, size=1)
    return [q.astype(np.float32).astype(np.float64) for q in p]


def _desc(D, H, L, act, l2k=None, l2b=None):
    from bore_amd import _lib
    return _lib.make_lstm_desc(D, L, H, act, l2k, l2b)


def _dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _thetas(models):
    return _dev(np.stack([O.pack(p) for p in models]))


def _is_deep(D, H, L, T):
    return T == 16 or L == 4 or H >= 54 or D == 64


def _ratio(a, b, rtol, atol=0.0):
    """max |a - b| in units of the tolerance atol + rtol |b|."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    diff = np.abs(a - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, diff / (atol + rtol * np.abs(b)))
    return float(np.max(r)) if r.size else 0.0


def _close(label, got, ref, tol, ref32=None):
    """assert_allclose at ``tol``, widened for a deep case by the float32 run of the oracle (module docstring).
    Prints what it measured before it asserts."""
    k, dev = 1.0, None
    if ref32 is not None:
        dev = _ratio(ref32, ref, **tol)
        k = max(1.0, 8.0 * dev)
        # the table of the module docstring says 1 for every deep case: a float32 run that deviates more (another
        # NumPy, another input) must be looked at and recorded there, not widen a tolerance unseen
        assert k == 1.0, "%s: the float32 oracle deviates by %.3g of the tolerance; the recorded factor is 1" % (label,
                                                                                                                dev)
    used = {n: v * k for n, v in tol.items()}
    print("%-40s kernel %.3g of tol%s" % (label, _ratio(got, ref, **used),
                                          "" if dev is None else "   fp32 oracle %.3g -> factor %.3g" % (dev, k)))
    np.testing.assert_allclose(got, ref, err_msg=label, **used)


def _oracle_fit(p0, act, X32, Y, perms, B, l2k, l2b, adam, dtype=np.float64, on_batch=None):
    p = O.as_dtype(p0, dtype)
    st = O.AdamState(p)
    hist = O.fit(p, act, st, X32, Y, perms, B, MV, l2k, l2b, dtype=dtype, on_batch=on_batch, **adam)
    return dict(theta=O.pack(p), m=O.pack(st.m), v=O.pack(st.v), loss=np.asarray(hist, dtype=np.float64), t=st.t)


def _gpu_fit(desc, models, X, Y, perms, B, adam):
    """One launch over len(models) networks: X [M,N,T,D], Y [M,N,T], perms [M,E,N]."""
    import torch
    from bore_amd import ops
    th = _thetas(models)
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    t = torch.zeros(len(models), dtype=torch.int64, device=th.device)
    hist = ops.lstm_fit(desc, th, m, v, t, _dev(X), _dev(Y), perms.shape[1], B, _dev(perms, np.int32), mask_value=MV,
                        **adam)
    return dict(theta=th.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy(), loss=hist.cpu().numpy(),
                t=t.cpu().numpy())


def _compare_fit(label, got, i, ref, ref32=None):
    for key in ("loss", "theta", "m", "v"):
        _close("%s %s" % (label, key), got[key][i], ref[key], FIT_TOL[key], None if ref32 is None else ref32[key])
    assert int(got["t"][i]) == ref["t"]


def _assert_no_logit_at_the_threshold(p, act, X32):
    """Guard on the inputs of an accuracy comparison: float32 must not be able to move a live logit across 0.5."""
    logits = O.forward(p, act, X32, MV)
    live = np.any(X32 != MV, axis=-1)
    assert not live.any() or np.min(np.abs(logits[live] - 0.5)) > 1e-3


def _compare_evaluate(label, desc, p, act, X32, Y, l2k, l2b, deep):
    from bore_amd import ops
    _assert_no_logit_at_the_threshold(p, act, X32)
    loss, acc = ops.lstm_evaluate(desc, _thetas([p]), _dev(X32)[None], _dev(Y)[None], mask_value=MV)
    rl, ra = O.evaluate(p, act, X32, Y, MV, l2k, l2b)
    r32 = O.evaluate(O.as_dtype(p, np.float32), act, X32, Y, MV, l2k, l2b, dtype=np.float32)[0] if deep else None
    _close(label + " evaluate loss", float(loss[0]), rl, EVAL_LOSS_TOL, r32)
    np.testing.assert_allclose(float(acc[0]), ra, atol=1e-6)


# -- 1. several models in one launch -----------------------------------------------------------------------
M_D, M_H, M_L, M_ACT, M_T = 5, 7, 2, "elu", 4


def _three_models(seed):
    rs = np.random.RandomState(seed)
    return rs, [_weights(M_D, M_H, M_L, rs) for _ in range(3)]


def test_models_per_launch_forward_many_to_many(gpu):
    from bore_amd import ops
    rs, models = _three_models(101)
    desc, th = _desc(M_D, M_H, M_L, M_ACT), _thetas(models)
    X = np.stack([_hyperband_sequences(rs, 130, M_T, M_D, MV)[0] for _ in range(3)]).astype(np.float32)
    Xd = _dev(X)
    out = ops.lstm_forward(desc, th, Xd, mask_value=MV).cpu().numpy()
    for i in range(3):
        one = ops.lstm_forward(desc, th[i:i + 1], Xd[i:i + 1], mask_value=MV).cpu().numpy()
        np.testing.assert_array_equal(out[i], one[0])
    _close("3 models m2m", out[1], O.forward(models[1], M_ACT, X[1], MV), FWD_TOL)


def test_models_per_launch_forward_one_to_one(gpu):
    from bore_amd import ops
    rs, models = _three_models(102)
    desc, th = _desc(M_D, M_H, M_L, M_ACT), _thetas(models)
    x = rs.uniform(size=(3, 130, M_D)).astype(np.float32)
    xd = _dev(x)
    out = ops.lstm_forward(desc, th, xd, num_steps=M_T).cpu().numpy()
    for i in range(3):
        one = ops.lstm_forward(desc, th[i:i + 1], xd[i:i + 1], num_steps=M_T).cpu().numpy()
        np.testing.assert_array_equal(out[i], one[0])
    _close("3 models o2o", out[1], O.one_to_one(models[1], M_ACT, x[1], M_T), FWD_TOL)


def test_models_per_launch_value_and_input_grad(gpu):
    from bore_amd import ops
    rs, models = _three_models(103)
    desc, th = _desc(M_D, M_H, M_L, M_ACT), _thetas(models)
    x = rs.uniform(size=(3, 130, M_D))
    xd = _dev(x, np.float64)
    val, grad = ops.lstm_value_and_input_grad(desc, th, xd, M_T, "sigmoid", True)
    val, grad = val.cpu().numpy(), grad.cpu().numpy()
    for i in range(3):
        v1, g1 = ops.lstm_value_and_input_grad(desc, th[i:i + 1], xd[i:i + 1], M_T, "sigmoid", True)
        np.testing.assert_array_equal(val[i], v1[0].cpu().numpy())
        np.testing.assert_array_equal(grad[i], g1[0].cpu().numpy())
    rv, rg = O.value_and_input_grad(models[1], M_ACT, x[1].astype(np.float32), M_T, "sigmoid", True)
    _close("3 models value", val[1], rv, VAL_TOL)
    _close("3 models grad", grad[1], rg, GRAD_TOL)


def test_models_per_launch_fit(gpu):
    rs, models = _three_models(104)
    N, B, E, l2 = 70, 32, 3, [1e-3] * (M_L + 1)
    desc = _desc(M_D, M_H, M_L, M_ACT, l2, l2)
    XY = [_hyperband_sequences(rs, N, M_T, M_D, MV) for _ in range(3)]
    X = np.stack([a for a, _ in XY]).astype(np.float32)
    Y = np.stack([b for _, b in XY])
    perms = np.stack([[rs.permutation(N) for _ in range(E)] for _ in range(3)]).astype(np.int32)
    got = _gpu_fit(desc, models, X, Y, perms, B, ADAM)
    for i in range(3):
        one = _gpu_fit(desc, models[i:i + 1], X[i:i + 1], Y[i:i + 1], perms[i:i + 1], B, ADAM)
        for key in ("theta", "m", "v", "t", "loss"):
            np.testing.assert_array_equal(got[key][i], one[key][0], err_msg=key)
    _compare_fit("3 models fit", got, 1, _oracle_fit(models[1], M_ACT, X[1], Y[1], perms[1], B, l2, l2, ADAM))


def test_models_per_launch_evaluate(gpu):
    from bore_amd import ops
    rs, models = _three_models(105)
    l2 = [1e-2] * (M_L + 1)
    desc, th = _desc(M_D, M_H, M_L, M_ACT, l2, l2), _thetas(models)
    XY = [_hyperband_sequences(rs, 150, M_T, M_D, MV) for _ in range(3)]
    X = np.stack([a for a, _ in XY]).astype(np.float32)
    Y = np.stack([b for _, b in XY])
    Xd, Yd = _dev(X), _dev(Y)
    loss, acc = (a.cpu().numpy() for a in ops.lstm_evaluate(desc, th, Xd, Yd, mask_value=MV))
    for i in range(3):
        l1, a1 = ops.lstm_evaluate(desc, th[i:i + 1], Xd[i:i + 1], Yd[i:i + 1], mask_value=MV)
        np.testing.assert_array_equal(loss[i], l1.cpu().numpy()[0])
        np.testing.assert_array_equal(acc[i], a1.cpu().numpy()[0])
    _assert_no_logit_at_the_threshold(models[1], M_ACT, X[1])
    rl, ra = O.evaluate(models[1], M_ACT, X[1], Y[1], MV, l2, l2)
    _close("3 models evaluate loss", loss[1], rl, EVAL_LOSS_TOL)
    np.testing.assert_allclose(acc[1], ra, atol=1e-6)


# -- 2. architectures in the fit and in evaluate -------------------------------------------------------------
def _kink_distance(p, act, X32):
    """Over the live steps of a forward pass: (smallest |candidate pre-activation| and |cell state|, the most negative
    candidate pre-activation)."""
    _, (C, live) = O.forward(p, act, X32, MV, cache=True)
    d, lowest = np.inf, np.inf
    for row in C:
        for t, k in enumerate(row):
            if live[:, t].any():
                d = min(d, np.min(np.abs(k["zg"][live[:, t]])), np.min(np.abs(k["c"][live[:, t]])))
                lowest = min(lowest, np.min(k["zg"][live[:, t]]))
    return d, lowest


ARCH_CASES = [
    # D, H, L, act, T, N, B, l2, seed
    (16, 32, 2, "tanh", 16, 65, 64, 1e-3, 1),      # the plugin's network at the step bound; trailing batch of one row
    (5, 7, 2, "elu", 4, 33, 16, 0.0, 2),           # odd H: rows of 29 floats, it / H with H = 7; trailing batch of one
    (5, 7, 2, "elu", 4, 10, 1, 1e-3, 3),           # batches of one row throughout
    (3, 16, 3, "sigmoid", 5, 7, 3, 1e-3, 4),       # three layers
    (2, 8, 4, "tanh", 16, 64, 64, 0.0, 5),         # BORE_LSTM_MAX_LAYERS and BORE_LSTM_MAX_STEPS together
    (64, 16, 1, "linear", 3, 33, 16, 1e-3, 6),     # BORE_LSTM_MAX_INPUT
    (2, 54, 1, "elu", 16, 65, 64, 0.0, 7),         # the most units at T = 16: 3456 items, the 7th slot partly filled
    (2, 57, 1, "elu", 1, 64, 64, 1e-3, 8),         # the most units at D = 2: all eight slots; T = 1
    (1, 1, 1, "tanh", 1, 1, 1, 0.0, 9),            # degenerate
    (5, 8, 1, "relu", 3, 1, 1, 0.0, 2446),         # relu on both sides of its kink, never near it (guards below)
]


@pytest.mark.parametrize("D,H,L,act,T,N,B,l2,seed", ARCH_CASES)
def test_architectures_fit_and_evaluate_match_the_oracle(gpu, D, H, L, act, T, N, B, l2, seed):
    rs = np.random.RandomState(seed)
    p0 = _weights(D, H, L, rs)
    X, Y = _hyperband_sequences(rs, N, T, D, MV)
    X32 = X.astype(np.float32)
    E = 3
    perms = np.stack([rs.permutation(N) for _ in range(E)]).astype(np.int32)
    l2s = [l2] * (L + 1)
    deep = _is_deep(D, H, L, T)
    label = "%d->%dx%d %s T=%d N=%d B=%d" % (D, L, H, act, T, N, B)
    on_batch = None
    if act == "relu":
        # fp32 and fp64 may take different sides of relu's kink: the case only means something away from it.  A
        # negative candidate at the FIRST live step leaves the cell state at exactly 0 (c = f 0 + i 0), which the
        # guard rejects, so all candidates of that step must be positive and the case is one sequence; at later
        # steps c = f c' + i 0 stays positive, so negative candidates are allowed there -- and required: without one
        # relu would be the identity throughout.  The seed was searched on the CPU for both.
        dist = [_kink_distance(p0, act, X32)]
        on_batch = lambda params, idx: dist.append(_kink_distance(params, act, X32[idx]))  # noqa: E731
    ref = _oracle_fit(p0, act, X32, Y, perms, B, l2s, l2s, ADAM, on_batch=on_batch)
    if act == "relu":
        near = min(d for d, _ in dist)
        assert near > 1e-4, "relu case: the oracle's trajectory comes within %.3g of the kink" % near
        assert all(low < -1e-4 for _, low in dist), "relu case: a batch never takes relu's zero branch"
    ref32 = _oracle_fit(p0, act, X32, Y, perms, B, l2s, l2s, ADAM, dtype=np.float32) if deep else None
    desc = _desc(D, H, L, act, l2s, l2s)
    got = _gpu_fit(desc, [p0], X32[None], Y[None], perms[None], B, ADAM)
    _compare_fit(label, got, 0, ref, ref32)
    _compare_evaluate(label, desc, p0, act, X32, Y, l2s, l2s, deep)


# -- 3. distinct l2 factors, non-default Adam ------------------------------------------------------------------
def test_distinct_l2_factors_and_adam_hyperparameters(gpu):
    D, H, L, act, T, N, B, E = 3, 16, 2, "elu", 3, 40, 16, 3
    l2k, l2b = [1e-3, 2e-3, 4e-3], [3e-3, 5e-4, 7e-3]
    adam = dict(lr=3e-3, beta1=0.8, beta2=0.99, eps=1e-6)
    rs = np.random.RandomState(31)
    p0 = _weights(D, H, L, rs)
    X, Y = _hyperband_sequences(rs, N, T, D, MV)
    X32 = X.astype(np.float32)
    perms = np.stack([rs.permutation(N) for _ in range(E)]).astype(np.int32)
    ref = _oracle_fit(p0, act, X32, Y, perms, B, l2k, l2b, adam)
    # the case can tell the slots apart: swapped, the oracle's losses move by more than 10x the tolerance
    swapped = _oracle_fit(p0, act, X32, Y, perms, B, l2b, l2k, adam)
    assert np.all(np.abs(swapped["loss"] - ref["loss"]) > 10 * FIT_TOL["loss"]["rtol"] * np.abs(ref["loss"]))
    rl = O.evaluate(p0, act, X32, Y, MV, l2k, l2b)[0]
    assert abs(O.evaluate(p0, act, X32, Y, MV, l2b, l2k)[0] - rl) > 10 * EVAL_LOSS_TOL["rtol"] * abs(rl)
    # ... and each Adam hyper-parameter: with any one of them at its default, theta leaves the tolerance
    for name in adam:
        other = _oracle_fit(p0, act, X32, Y, perms, B, l2k, l2b, dict(adam, **{name: ADAM[name]}))
        assert _ratio(other["theta"], ref["theta"], **FIT_TOL["theta"]) > 10, name
    desc = _desc(D, H, L, act, l2k, l2b)
    got = _gpu_fit(desc, [p0], X32[None], Y[None], perms[None], B, adam)
    _compare_fit("l2 per slot, Adam", got, 0, ref)
    _compare_evaluate("l2 per slot", desc, p0, act, X32, Y, l2k, l2b, False)


# -- 4. value + input gradient: tiles and step counts -----------------------------------------------------------
VG_SHAPES = [(2, 32, 2, "elu"), (16, 32, 2, "tanh"), (5, 7, 2, "sigmoid")]
VG_ROWS = (1, 63, 64, 65, 130)


@pytest.mark.parametrize("num_steps", [1, 2, 16])
@pytest.mark.parametrize("D,H,L,act", VG_SHAPES)
def test_value_and_input_grad_over_tiles_and_steps(gpu, D, H, L, act, num_steps):
    from bore_amd import ops
    rs = np.random.RandomState(1000 + 10 * D + num_steps)
    p = _weights(D, H, L, rs)
    p32 = O.as_dtype(p, np.float32)
    desc, th = _desc(D, H, L, act), _thetas([p])
    x = rs.uniform(size=(max(VG_ROWS), D))            # fp64 points; the device rounds them to fp32
    x32 = x.astype(np.float32)
    deep = _is_deep(D, H, L, num_steps)
    label = "%d->%dx%d %s steps=%d" % (D, L, H, act, num_steps)

    def check(n, transform, negate, rv, rg, r32):
        val, grad = ops.lstm_value_and_input_grad(desc, th, _dev(x[:n], np.float64)[None], num_steps, transform,
                                                  negate)
        val, grad = val[0].cpu().numpy(), grad[0].cpu().numpy()
        tag = "%s rows=%d %s%s" % (label, n, "-" if negate else "+", transform)
        _close(tag + " value", val, rv[:n], VAL_TOL, None if r32 is None else r32[0][:n])
        _close(tag + " grad", grad, rg[:n], GRAD_TOL, None if r32 is None else r32[1][:n])
        if transform == "identity":      # the value is the one-to-one prediction of the same points, bit for bit
            pred = ops.lstm_forward(desc, th, _dev(x32[:n])[None], num_steps=num_steps)[0].cpu().numpy()
            np.testing.assert_array_equal(-val if negate else val, pred)

    # rows are independent: one reference over 130 rows serves every row count
    def refs(transform, negate):
        rv, rg = O.value_and_input_grad(p, act, x32, num_steps, transform, negate)
        r32 = O.value_and_input_grad(p32, act, x32, num_steps, transform, negate, dtype=np.float32) if deep else None
        return rv, rg, r32

    base = refs("identity", True)
    for n in VG_ROWS:
        check(n, "identity", True, *base)
    # every transform and sign at one (num_steps, n_rows) point per shape
    if num_steps == {2: 16, 16: 2, 5: 1}[D]:
        for transform in ("identity", "sigmoid", "exp"):
            for negate in (True, False):
                if (transform, negate) != ("identity", True):
                    check(65, transform, negate, *refs(transform, negate))


# -- 5. forward at the bounds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H,L,act", [(16, 32, 2, "tanh"), (2, 8, 4, "elu")])
def test_forward_at_the_step_and_layer_bounds(gpu, D, H, L, act):
    from bore_amd import ops
    rs = np.random.RandomState(500 + D)
    p = _weights(D, H, L, rs)
    desc, th = _desc(D, H, L, act), _thetas([p])
    T = 16
    X32 = _hyperband_sequences(rs, 129, T, D, MV)[0].astype(np.float32)
    ref = O.forward(p, act, X32, MV)
    ref32 = O.forward(O.as_dtype(p, np.float32), act, X32, MV, dtype=np.float32)
    for n in (1, 64, 65, 129):
        out = ops.lstm_forward(desc, th, _dev(X32[:n])[None], mask_value=MV)[0].cpu().numpy()
        _close("%d->%dx%d m2m T=16 rows=%d" % (D, L, H, n), out, ref[:n], FWD_TOL, ref32[:n])
    x = rs.uniform(size=(65, D)).astype(np.float32)
    for T in (1, 16):
        o2o = ops.lstm_forward(desc, th, _dev(x)[None], num_steps=T)[0].cpu().numpy()
        m2m = ops.lstm_forward(desc, th, _dev(np.repeat(x[:, None], T, 1))[None], mask_value=1e9)[0].cpu().numpy()
        np.testing.assert_array_equal(o2o, m2m[:, T - 1])
        r32 = O.one_to_one(O.as_dtype(p, np.float32), act, x, T, dtype=np.float32)
        _close("%d->%dx%d o2o T=%d" % (D, L, H, T), o2o, O.one_to_one(p, act, x, T), FWD_TOL, r32)


# -- 6. fully masked data ------------------------------------------------------------------------------------------
MASK_D, MASK_H, MASK_L, MASK_ACT, MASK_T = 2, 32, 2, "elu", 4


def test_fit_with_a_batch_that_has_no_live_step(gpu):
    """Rows 0-7 are masked at every step and perm is the identity: the first Adam step of every epoch sees no live
    element.  Without l2 its gradient is zero: the very first step leaves theta, m and v untouched, the first step of
    a later epoch only lets Adam's moments decay (and still moves theta by them)."""
    N, B, E = 20, 8, 3
    rs = np.random.RandomState(61)
    p0 = _weights(MASK_D, MASK_H, MASK_L, rs)
    X, Y = _hyperband_sequences(rs, N, MASK_T, MASK_D, MV)
    X[:8], Y[:8] = MV, MV
    X32 = X.astype(np.float32)
    perms = np.tile(np.arange(N, dtype=np.int32), (E, 1))
    ref = _oracle_fit(p0, MASK_ACT, X32, Y, perms, B, None, None, ADAM)
    got = _gpu_fit(_desc(MASK_D, MASK_H, MASK_L, MASK_ACT), [p0], X32[None], Y[None], perms[None], B, ADAM)
    _compare_fit("first batch masked", got, 0, ref)


def test_fit_and_evaluate_with_every_step_masked(gpu):
    from bore_amd import ops
    N, B, E, l2 = 20, 8, 2, [1e-3] * (MASK_L + 1)
    rs = np.random.RandomState(62)
    p0 = _weights(MASK_D, MASK_H, MASK_L, rs)
    X32 = np.full((N, MASK_T, MASK_D), MV, dtype=np.float32)
    Y = np.full((N, MASK_T), MV)
    perms = np.stack([rs.permutation(N) for _ in range(E)]).astype(np.int32)
    ref = _oracle_fit(p0, MASK_ACT, X32, Y, perms, B, l2, l2, ADAM)
    pen = O._penalty(p0, l2, l2)[0]
    assert pen > 1e-3
    np.testing.assert_allclose(ref["loss"][0], pen, rtol=1e-2)     # 0 + the penalty (which the l2 steps shrink)
    desc = _desc(MASK_D, MASK_H, MASK_L, MASK_ACT, l2, l2)
    got = _gpu_fit(desc, [p0], X32[None], Y[None], perms[None], B, ADAM)
    _compare_fit("all masked", got, 0, ref)
    loss, acc = ops.lstm_evaluate(desc, _thetas([p0]), _dev(X32)[None], _dev(Y)[None], mask_value=MV)
    rl, ra = O.evaluate(p0, MASK_ACT, X32, Y, MV, l2, l2)
    assert ra == 0.0 and abs(rl - pen) < 1e-15
    assert float(acc[0]) == 0.0
    _close("all masked evaluate loss", float(loss[0]), pen, EVAL_LOSS_TOL)
