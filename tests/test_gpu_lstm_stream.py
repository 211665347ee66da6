"""The streamed LSTM kernels (bore_lstm_stream_*) against the fp64 oracle tests/lstm_oracle.py: networks the LDS
kernels refuse (48 inputs, a third layer, 64 and 128 units, 512 inputs, every bound of depth together), shapes that
cross the panel product's tiling (4H = 132: a second column pass; 33-deep reductions: two panels), several models per
launch, the bit properties of the flavour, fully masked data, and the model API on a 48-input factory.

Helpers and tolerances are those of tests/test_gpu_lstm_shapes.py and tests/test_gpu_lstm.py.  Cases no deeper than
T <= 5, L <= 3, H <= 32, D <= 16 use FIT_TOL, FWD_TOL, VAL_TOL, GRAD_TOL and EVAL_LOSS_TOL as they stand.  Every other
case takes the rule of tests/test_gpu_lstm_shapes.py: the oracle's own float32 run, computed in the test from the
test's inputs, gives the deviation in units of the existing tolerance, the tolerance is the existing one x
max(1, 8 x deviation), and ``_close`` asserts that the factor is the recorded one.  Measured on the CPU (NumPy 2.2,
x86-64; seed D + H + L + T, ``_weights``, ``_hyperband_sequences``), deviation of the float32 oracle in units of the
existing tolerance, and the factor it gives (1 = the existing tolerance stands):

  fit + evaluate (D->LxH act T)        loss     theta    m        v        evaluate loss   factor
  5->2x33   sigmoid T=3  N=65 B=16     0.0007   0.0018   0.020    0.013    0.0013          1
  3->1x7    relu    T=16 N=10 B=4      0.0006   0.0048   0.0005   0.013    0.0029          1
  48->2x32  elu     T=5  N=65 B=64     0.0015   0.0012   0.0019   0.013    0.0027          1
  16->3x32  elu     T=5  N=65 B=64     0.0007   0.0011   0.0049   0.013    0.0009          (not deep)
  2->1x64   tanh    T=1  N=64 B=64     0.0006   0.0007   0.0010   0.010    0.0008          1
  16->2x64  elu     T=5  N=70 B=64     0.0017   0.0014   0.0017   0.013    0.0009          1
  512->1x8  linear  T=2  N=33 B=16     0.0014   0.0035   0.082    0.014    0.0028          1
  2->1x128  elu     T=2  N=65 B=64     0.0018   0.0012   0.0013   0.013    0.0018          1
  64->4x64  tanh    T=16 N=65 B=64     0.0014   0.0019   0.012    0.012    0.0018          1
  130 / 70 rows, T steps               many-to-many   one-to-one   value    gradient
  5->2x33   sigmoid T=3                0.0055         0.0044       0.012    0.0001         1
  48->2x32  elu     T=5                0.0025         0.0023       0.0083   0.0017         1
  16->3x32  elu     T=5                0.0011         0.0012       0.0060   0.0008         (not deep)
  64->4x64  tanh    T=16               0.0043         0.0047       0.016    0.0023         1

The largest is 0.082 (m at 512 -> 1 x 8: sums over 512 inputs), so 8 x the deviation is below 1 everywhere and the
existing tolerances stand for every case.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_oracle as O  # noqa: E402
from test_gpu_lstm import FIT_TOL, _hyperband_sequences  # noqa: E402
from test_gpu_lstm_shapes import (ADAM, EVAL_LOSS_TOL, FWD_TOL, GRAD_TOL, MV, VAL_TOL,  # noqa: E402
                                  _close, _desc, _dev, _oracle_fit, _thetas, _weights)

pytestmark = pytest.mark.gpu

def _is_deep(D, H, L, T):
    return T > 5 or L > 3 or H > 32 or D > 16


def _stream_fit(desc, models, X, Y, perms, B, adam, state=None):
    """One bore_lstm_stream_fit launch over len(models) networks: X [M,N,T,D], Y [M,N,T], perms [M,E,N].  ``state``:
    (theta, m, v, t) device tensors of an earlier call to go on from."""
    import torch
    from bore_amd import ops
    if state is None:
        th = _thetas(models)
        state = (th, torch.zeros_like(th), torch.zeros_like(th),
                 torch.zeros(len(models), dtype=torch.int64, device=th.device))
    th, m, v, t = state
    hist = ops.lstm_stream_fit(desc, th, m, v, t, _dev(X), _dev(Y), perms.shape[1], B, _dev(perms, np.int32),
                               mask_value=MV, **adam)
    return dict(theta=th.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy(), loss=hist.cpu().numpy(),
                t=t.cpu().numpy(), state=state)


def _compare_fit(label, got, i, ref, ref32=None):
    for key in ("loss", "theta", "m", "v"):
        _close("%s %s" % (label, key), got[key][i], ref[key], FIT_TOL[key], None if ref32 is None else ref32[key])
    assert int(got["t"][i]) == ref["t"]


def _accuracy_atol(p, act, X32):
    """What float32 may move the accuracy by: the share of the live logits within 1e-3 of the 0.5 threshold (each may
    fall on either side), from the oracle alone.  0 at every shape here but 64->4x64 over 16 steps."""
    logits = O.forward(p, act, X32, MV)
    live = np.any(X32 != MV, axis=-1)
    near = np.count_nonzero(np.abs(logits[live] - 0.5) <= 1e-3)
    return 1e-6 + near / max(1, np.count_nonzero(live))


def _compare_evaluate(label, desc, p, act, X32, Y, l2k, l2b, deep):
    from bore_amd import ops
    loss, acc = ops.lstm_stream_evaluate(desc, _thetas([p]), _dev(X32)[None], _dev(Y)[None], mask_value=MV)
    rl, ra = O.evaluate(p, act, X32, Y, MV, l2k, l2b)
    r32 = O.evaluate(O.as_dtype(p, np.float32), act, X32, Y, MV, l2k, l2b, dtype=np.float32)[0] if deep else None
    _close(label + " evaluate loss", float(loss[0]), rl, EVAL_LOSS_TOL, r32)
    np.testing.assert_allclose(float(acc[0]), ra, atol=_accuracy_atol(p, act, X32))


# -- 1. fit + evaluate --------------------------------------------------------------------------------------------
FIT_CASES = [
    # D, H, L, act, T, N, B, l2
    (5, 33, 2, "sigmoid", 3, 65, 16, 0.0),     # 4H = 132: a second column pass of 4 columns; 33-deep reductions: two
                                               # panels; batches of 16 with a tail of 1
    (3, 7, 1, "relu", 16, 10, 4, 1e-3),        # 16 steps, ragged everything
    (48, 32, 2, "elu", 5, 65, 64, 1e-3),       # the plugin default on 48 inputs; LDS refuses it
    (16, 32, 3, "elu", 5, 65, 64, 0.0),        # third layer; LDS refuses
    (2, 64, 1, "tanh", 1, 64, 64, 0.0),        # one step; LDS refuses
    (16, 64, 2, "elu", 5, 70, 64, 1e-3),       # LDS refuses
    (512, 8, 1, "linear", 2, 33, 16, 0.0),     # at the streamed input bound
    (2, 128, 1, "elu", 2, 65, 64, 0.0),        # at the streamed unit bound
    (64, 64, 4, "tanh", 16, 65, 64, 0.0),      # every bound of depth together
]
E_FIT = 3


def _fit_inputs(D, H, L, act, T, N, B, l2):
    rs = np.random.RandomState(D + H + L + T)
    p0 = _weights(D, H, L, rs)
    X, Y = _hyperband_sequences(rs, N, T, D, MV)
    perms = np.stack([rs.permutation(N) for _ in range(E_FIT)]).astype(np.int32)
    return rs, p0, X.astype(np.float32), Y, perms, [l2] * (L + 1)


@pytest.mark.parametrize("D,H,L,act,T,N,B,l2", FIT_CASES)
def test_fit_and_evaluate_match_the_oracle(gpu, D, H, L, act, T, N, B, l2):
    _, p0, X32, Y, perms, l2s = _fit_inputs(D, H, L, act, T, N, B, l2)
    deep = _is_deep(D, H, L, T)
    label = "%d->%dx%d %s T=%d N=%d B=%d" % (D, L, H, act, T, N, B)
    ref = _oracle_fit(p0, act, X32, Y, perms, B, l2s, l2s, ADAM)
    ref32 = _oracle_fit(p0, act, X32, Y, perms, B, l2s, l2s, ADAM, dtype=np.float32) if deep else None
    desc = _desc(D, H, L, act, l2s, l2s)
    got = _stream_fit(desc, [p0], X32[None], Y[None], perms[None], B, ADAM)
    _compare_fit(label, got, 0, ref, ref32)
    _compare_evaluate(label, desc, p0, act, X32, Y, l2s, l2s, deep)


# -- 2. forward, value + input gradient -------------------------------------------------------------------------
ROW_CASES = [(D, H, L, act, T) for D, H, L, act, T, _, _, _ in (FIT_CASES[0], FIT_CASES[2], FIT_CASES[3], FIT_CASES[8])]


@pytest.mark.parametrize("D,H,L,act,T", ROW_CASES)
def test_forward_both_forms_over_two_tiles_and_a_tail(gpu, D, H, L, act, T):
    from bore_amd import ops
    rs = np.random.RandomState(D + H + L + T)
    p = _weights(D, H, L, rs)
    p32 = O.as_dtype(p, np.float32)
    desc, th = _desc(D, H, L, act), _thetas([p])
    deep = _is_deep(D, H, L, T)
    label = "%d->%dx%d %s T=%d" % (D, L, H, act, T)
    n = 130
    X32 = _hyperband_sequences(rs, n, T, D, MV)[0].astype(np.float32)
    out = ops.lstm_stream_forward(desc, th, _dev(X32)[None], mask_value=MV)[0].cpu().numpy()
    r32 = O.forward(p32, act, X32, MV, dtype=np.float32) if deep else None
    _close(label + " m2m", out, O.forward(p, act, X32, MV), FWD_TOL, r32)
    x = rs.uniform(size=(n, D)).astype(np.float32)
    o2o = ops.lstm_stream_forward(desc, th, _dev(x)[None], num_steps=T)[0].cpu().numpy()
    r32 = O.one_to_one(p32, act, x, T, dtype=np.float32) if deep else None
    _close(label + " o2o", o2o, O.one_to_one(p, act, x, T), FWD_TOL, r32)


@pytest.mark.parametrize("D,H,L,act,T", ROW_CASES)
def test_value_and_input_grad_matches_the_oracle(gpu, D, H, L, act, T):
    from bore_amd import ops
    rs = np.random.RandomState(D + H + L + T)
    p = _weights(D, H, L, rs)
    p32 = O.as_dtype(p, np.float32)
    desc, th = _desc(D, H, L, act), _thetas([p])
    deep = _is_deep(D, H, L, T)
    x = rs.uniform(size=(70, D))            # fp64 points; the device rounds them to fp32
    x32 = x.astype(np.float32)
    xd = _dev(x, np.float64)[None]
    for transform in ("identity", "sigmoid", "exp"):
        for negate in (True, False):
            val, grad = ops.lstm_stream_value_and_input_grad(desc, th, xd, T, transform, negate)
            rv, rg = O.value_and_input_grad(p, act, x32, T, transform, negate)
            r32 = O.value_and_input_grad(p32, act, x32, T, transform, negate, dtype=np.float32) if deep else (None,
                                                                                                              None)
            tag = "%d->%dx%d %s T=%d %s%s" % (D, L, H, act, T, "-" if negate else "+", transform)
            _close(tag + " value", val[0].cpu().numpy(), rv, VAL_TOL, r32[0])
            _close(tag + " grad", grad[0].cpu().numpy(), rg, GRAD_TOL, r32[1])


# -- 3. three models in one launch --------------------------------------------------------------------------------
M_D, M_H, M_L, M_ACT, M_T = 5, 7, 2, "elu", 4


def _three_models(seed):
    rs = np.random.RandomState(seed)
    return rs, [_weights(M_D, M_H, M_L, rs) for _ in range(3)]


def test_models_per_launch_forward(gpu):
    from bore_amd import ops
    rs, models = _three_models(201)
    desc, th = _desc(M_D, M_H, M_L, M_ACT), _thetas(models)
    X = np.stack([_hyperband_sequences(rs, 130, M_T, M_D, MV)[0] for _ in range(3)]).astype(np.float32)
    x = rs.uniform(size=(3, 130, M_D)).astype(np.float32)
    Xd, xd = _dev(X), _dev(x)
    m2m = ops.lstm_stream_forward(desc, th, Xd, mask_value=MV).cpu().numpy()
    o2o = ops.lstm_stream_forward(desc, th, xd, num_steps=M_T).cpu().numpy()
    for i in range(3):
        one = ops.lstm_stream_forward(desc, th[i:i + 1], Xd[i:i + 1], mask_value=MV).cpu().numpy()
        np.testing.assert_array_equal(m2m[i], one[0])
        one = ops.lstm_stream_forward(desc, th[i:i + 1], xd[i:i + 1], num_steps=M_T).cpu().numpy()
        np.testing.assert_array_equal(o2o[i], one[0])
        _close("3 models m2m %d" % i, m2m[i], O.forward(models[i], M_ACT, X[i], MV), FWD_TOL)
        _close("3 models o2o %d" % i, o2o[i], O.one_to_one(models[i], M_ACT, x[i], M_T), FWD_TOL)


def test_models_per_launch_value_and_input_grad(gpu):
    from bore_amd import ops
    rs, models = _three_models(203)
    desc, th = _desc(M_D, M_H, M_L, M_ACT), _thetas(models)
    x = rs.uniform(size=(3, 130, M_D))
    xd = _dev(x, np.float64)
    val, grad = ops.lstm_stream_value_and_input_grad(desc, th, xd, M_T, "sigmoid", True)
    val, grad = val.cpu().numpy(), grad.cpu().numpy()
    for i in range(3):
        v1, g1 = ops.lstm_stream_value_and_input_grad(desc, th[i:i + 1], xd[i:i + 1], M_T, "sigmoid", True)
        np.testing.assert_array_equal(val[i], v1[0].cpu().numpy())
        np.testing.assert_array_equal(grad[i], g1[0].cpu().numpy())
        rv, rg = O.value_and_input_grad(models[i], M_ACT, x[i].astype(np.float32), M_T, "sigmoid", True)
        _close("3 models value %d" % i, val[i], rv, VAL_TOL)
        _close("3 models grad %d" % i, grad[i], rg, GRAD_TOL)


def test_models_per_launch_fit(gpu):
    rs, models = _three_models(204)
    N, B, E, l2 = 70, 32, 3, [1e-3] * (M_L + 1)
    desc = _desc(M_D, M_H, M_L, M_ACT, l2, l2)
    XY = [_hyperband_sequences(rs, N, M_T, M_D, MV) for _ in range(3)]
    X = np.stack([a for a, _ in XY]).astype(np.float32)
    Y = np.stack([b for _, b in XY])
    perms = np.stack([[rs.permutation(N) for _ in range(E)] for _ in range(3)]).astype(np.int32)
    got = _stream_fit(desc, models, X, Y, perms, B, ADAM)
    for i in range(3):
        one = _stream_fit(desc, models[i:i + 1], X[i:i + 1], Y[i:i + 1], perms[i:i + 1], B, ADAM)
        for key in ("theta", "m", "v", "t", "loss"):
            np.testing.assert_array_equal(got[key][i], one[key][0], err_msg=key)
        ref = _oracle_fit(models[i], M_ACT, X[i], Y[i], perms[i], B, l2, l2, ADAM)
        _compare_fit("3 models fit %d" % i, got, i, ref)


def test_models_per_launch_evaluate(gpu):
    from bore_amd import ops
    rs, models = _three_models(205)
    l2 = [1e-2] * (M_L + 1)
    desc, th = _desc(M_D, M_H, M_L, M_ACT, l2, l2), _thetas(models)
    XY = [_hyperband_sequences(rs, 150, M_T, M_D, MV) for _ in range(3)]
    X = np.stack([a for a, _ in XY]).astype(np.float32)
    Y = np.stack([b for _, b in XY])
    Xd, Yd = _dev(X), _dev(Y)
    loss, acc = (a.cpu().numpy() for a in ops.lstm_stream_evaluate(desc, th, Xd, Yd, mask_value=MV))
    for i in range(3):
        l1, a1 = ops.lstm_stream_evaluate(desc, th[i:i + 1], Xd[i:i + 1], Yd[i:i + 1], mask_value=MV)
        np.testing.assert_array_equal(loss[i], l1.cpu().numpy()[0])
        np.testing.assert_array_equal(acc[i], a1.cpu().numpy()[0])
        rl, ra = O.evaluate(models[i], M_ACT, X[i], Y[i], MV, l2, l2)
        _close("3 models evaluate loss %d" % i, loss[i], rl, EVAL_LOSS_TOL)
        np.testing.assert_allclose(acc[i], ra, atol=_accuracy_atol(models[i], M_ACT, X[i]))


# -- 4. bit properties within the flavour, at 16 -> 2 x 64 over 5 steps ------------------------------------------------
P_D, P_H, P_L, P_ACT, P_T = 16, 64, 2, "elu", 5


@pytest.fixture(scope="module")
def prop():
    rs = np.random.RandomState(77)
    p = _weights(P_D, P_H, P_L, rs)
    return rs, p, _desc(P_D, P_H, P_L, P_ACT)


def test_one_to_one_equals_many_to_many_at_the_last_step(gpu, prop):
    from bore_amd import ops
    rs, p, desc = prop
    th = _thetas([p])
    x = rs.uniform(size=(130, P_D)).astype(np.float32)
    o2o = ops.lstm_stream_forward(desc, th, _dev(x)[None], num_steps=P_T)[0].cpu().numpy()
    m2m = ops.lstm_stream_forward(desc, th, _dev(np.repeat(x[:, None], P_T, 1))[None], mask_value=1e9)[0].cpu().numpy()
    np.testing.assert_array_equal(o2o, m2m[:, P_T - 1])


def test_identity_value_equals_forward_of_the_rounded_point(gpu, prop):
    from bore_amd import ops
    rs, p, desc = prop
    th = _thetas([p])
    x = rs.uniform(size=(70, P_D))
    val, _ = ops.lstm_stream_value_and_input_grad(desc, th, _dev(x, np.float64)[None], P_T, "identity", False)
    pred = ops.lstm_stream_forward(desc, th, _dev(x.astype(np.float32))[None], num_steps=P_T)
    np.testing.assert_array_equal(val[0].cpu().numpy(), pred[0].cpu().numpy())


def test_a_model_alone_gives_the_bits_of_a_multi_model_launch(gpu, prop):
    from bore_amd import ops
    rs, p, desc = prop
    models = [p, _weights(P_D, P_H, P_L, rs)]
    th = _thetas(models)
    x = rs.uniform(size=(2, 70, P_D))
    xd = _dev(x, np.float64)
    val, grad = ops.lstm_stream_value_and_input_grad(desc, th, xd, P_T, "sigmoid", True)
    for i in range(2):
        v1, g1 = ops.lstm_stream_value_and_input_grad(desc, th[i:i + 1], xd[i:i + 1], P_T, "sigmoid", True)
        np.testing.assert_array_equal(val[i].cpu().numpy(), v1[0].cpu().numpy())
        np.testing.assert_array_equal(grad[i].cpu().numpy(), g1[0].cpu().numpy())


def test_a_row_alone_gives_the_bits_of_a_full_tile(gpu, prop):
    from bore_amd import ops
    rs, p, desc = prop
    th = _thetas([p])
    x = rs.uniform(size=(64, P_D))
    xd = _dev(x, np.float64)
    val, grad = ops.lstm_stream_value_and_input_grad(desc, th, xd[None], P_T, "identity", True)
    pred = ops.lstm_stream_forward(desc, th, _dev(x.astype(np.float32))[None], num_steps=P_T)
    for r in (0, 17, 63):
        v1, g1 = ops.lstm_stream_value_and_input_grad(desc, th, xd[None, r:r + 1], P_T, "identity", True)
        np.testing.assert_array_equal(val[0, r].cpu().numpy(), v1[0, 0].cpu().numpy())
        np.testing.assert_array_equal(grad[0, r].cpu().numpy(), g1[0, 0].cpu().numpy())
        p1 = ops.lstm_stream_forward(desc, th, _dev(x[r:r + 1].astype(np.float32))[None], num_steps=P_T)
        np.testing.assert_array_equal(pred[0, r].cpu().numpy(), p1[0, 0].cpu().numpy())


def test_warm_start_and_reproducibility(gpu, prop):
    rs, p, desc = prop
    N, B, E = 70, 64, 2
    X, Y = _hyperband_sequences(rs, N, P_T, P_D, MV)
    X32 = X.astype(np.float32)
    perms = np.stack([rs.permutation(N) for _ in range(2 * E)]).astype(np.int32)

    def run(splits):
        got, e0, losses = None, 0, []
        for e in splits:
            got = _stream_fit(desc, [p], X32[None], Y[None], perms[None, e0:e0 + e], B, ADAM,
                              state=None if got is None else got["state"])
            losses.append(got["loss"])
            e0 += e
        return got["theta"], got["m"], got["v"], got["t"], np.concatenate(losses, 1)

    a, b, c = run([2 * E]), run([E, E]), run([2 * E])
    for x, y in zip(a, b):          # E + E epochs equal 2E epochs
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a, c):          # two runs are identical
        np.testing.assert_array_equal(x, y)
    assert int(a[3][0]) == 2 * E * -(-N // B)


# -- 5. fully masked data (the two last tests of tests/test_gpu_lstm_shapes.py) ----------------------------------------
MASK_D, MASK_H, MASK_L, MASK_ACT, MASK_T = 2, 32, 2, "elu", 4


def test_fit_with_a_batch_that_has_no_live_step(gpu):
    """Rows 0-7 are masked at every step and perm is the identity: the first Adam step of every epoch sees no live
    element; without l2 its gradient is zero."""
    N, B, E = 20, 8, 3
    rs = np.random.RandomState(61)
    p0 = _weights(MASK_D, MASK_H, MASK_L, rs)
    X, Y = _hyperband_sequences(rs, N, MASK_T, MASK_D, MV)
    X[:8], Y[:8] = MV, MV
    X32 = X.astype(np.float32)
    perms = np.tile(np.arange(N, dtype=np.int32), (E, 1))
    ref = _oracle_fit(p0, MASK_ACT, X32, Y, perms, B, None, None, ADAM)
    got = _stream_fit(_desc(MASK_D, MASK_H, MASK_L, MASK_ACT), [p0], X32[None], Y[None], perms[None], B, ADAM)
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
    desc = _desc(MASK_D, MASK_H, MASK_L, MASK_ACT, l2, l2)
    got = _stream_fit(desc, [p0], X32[None], Y[None], perms[None], B, ADAM)
    _compare_fit("all masked", got, 0, ref)
    loss, acc = ops.lstm_stream_evaluate(desc, _thetas([p0]), _dev(X32)[None], _dev(Y)[None], mask_value=MV)
    rl, ra = O.evaluate(p0, MASK_ACT, X32, Y, MV, l2, l2)
    assert ra == 0.0 and abs(rl - pen) < 1e-15
    assert float(acc[0]) == 0.0
    _close("all masked evaluate loss", float(loss[0]), pen, EVAL_LOSS_TOL)


# -- 6. the model API on a network the LDS kernels refuse ---------------------------------------------------------
def test_stacked_recurrent_factory_of_48_inputs(gpu):
    from scipy.optimize import Bounds
    from bore_amd import ops
    from bore_amd.layers import BinaryCrossentropy
    from bore_amd.models import StackedRecurrentFactory
    rs = np.random.RandomState(0)
    num_steps, input_dim, n = 5, 48, 64
    factory = StackedRecurrentFactory(input_dim=input_dim, output_dim=1, num_layers=2, num_units=32,
                                      layer_kws=dict(activation="elu"), seed=0)
    assert ops.lstm_streamed(factory._desc, num_steps) == 1
    net1 = factory.build_many_to_many()
    net1.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True), metrics=["accuracy"])
    X = rs.uniform(size=(n, num_steps, input_dim))
    Z = rs.randint(2, size=(n, num_steps, 1))
    hist = net1.fit(X, Z, epochs=10, batch_size=16)
    assert len(hist.history["loss"]) == 10 and hist.history["loss"][-1] < hist.history["loss"][0]
    loss, acc = net1.evaluate(X, Z)
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0
    net2 = factory.build_one_to_one(num_steps)
    for a, b in zip(net1.get_weights(), net2.get_weights()):
        np.testing.assert_array_equal(a, b)
    X_test = rs.uniform(size=(32, input_dim))
    X_test_tiled = np.tile(np.expand_dims(X_test, axis=1), reps=(1, num_steps, 1))
    np.testing.assert_array_equal(net1.predict(X_test_tiled)[:, -1], net2.predict(X_test))
    lb, ub = np.zeros(input_dim), np.ones(input_dim)
    res = net2.argmax(Bounds(lb=lb, ub=ub), num_starts=3, num_samples=256, print_fn=lambda s: None, random_state=rs)
    assert res is not None and np.all(res.x >= lb) and np.all(res.x <= ub)
    # argmax minimises transform(-f): with no transform the identity of the negated prediction
    _close("argmax fun", res.fun, -float(net2.predict(res.x[None])[0, 0]), VAL_TOL)
