"""CPU side of the weighted fits: the float64 checker tests/weighted_oracle.py against torch autograd and against the
oracle's own batch gradient, and the host helper that turns Keras' ``sample_weight`` / ``class_weight`` into one
float32 vector (bore_amd.data.resolve_sample_weight).  No GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import weighted_oracle as WO
from bore_amd.data import resolve_sample_weight
from oracle import bore_oracle as O

D, UNITS, ACTS = 3, [5, 7, 1], ["elu", "tanh", "linear"]
L2 = [1e-3, 1e-3, 2e-3, 0.0, 0.0, 0.0]


def case(seed=0, nb=11):
    rs = np.random.RandomState(seed)
    p = [a.astype(np.float64) for a in O.glorot_uniform_params(D, UNITS, rs)]
    for i in range(1, len(p), 2):
        p[i] = rs.normal(scale=0.1, size=p[i].shape)
    X = rs.uniform(-1, 1, size=(nb, D))
    z = (rs.uniform(size=nb) < 0.4).astype(np.float64)
    w = rs.uniform(0, 3, size=nb)
    w[2] = 0.0                                                      # a zero weight among the rows
    return p, X, z, w


def torch_loss_and_grads(p, X, z, w, l2):
    tp = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in p]
    h = torch.tensor(X)
    for l, act in enumerate(ACTS):
        h = h @ tp[2 * l] + tp[2 * l + 1]
        h = {"elu": torch.nn.functional.elu, "tanh": torch.tanh, "linear": lambda a: a}[act](h)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(
        h[:, 0], torch.tensor(z), weight=torch.tensor(w), reduction="sum") / len(X)
    for q, f in zip(tp, l2):
        if f:
            loss = loss + f * (q * q).sum()
    loss.backward()
    return float(loss.detach()), [q.grad.numpy() for q in tp]


def test_checker_matches_torch_autograd():
    p, X, z, w = case()
    loss, grads = WO.weighted_loss_and_grads(p, ACTS, X, z, w, l2=L2)
    tl, tg = torch_loss_and_grads(p, X, z, w, L2)
    np.testing.assert_allclose(float(loss), tl, rtol=1e-12)
    for a, b in zip(grads, tg):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-15)


def test_checker_with_unit_weights_is_the_oracles_batch_gradient():
    p, X, z, _ = case(1)
    loss, grads = WO.weighted_loss_and_grads(p, ACTS, X, z, np.ones(len(X)), l2=L2)
    rl, rg = O.loss_and_grads(p, ACTS, X, z, l2=L2)
    np.testing.assert_allclose(float(loss), float(rl), rtol=1e-12)
    for a, b in zip(grads, rg):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-15)


def test_checker_fit_with_unit_weights_is_the_oracles_fit():
    p, X, z, _ = case(2, nb=37)
    perms = np.stack([np.random.RandomState(5 + e).permutation(37) for e in range(2)])
    pa, pb = [a.copy() for a in p], [a.copy() for a in p]
    sa, sb = O.AdamState(pa), O.AdamState(pb)
    ha = WO.weighted_fit(pa, ACTS, sa, X, z, np.ones(37), perms, batch_size=16, l2=L2)
    hb = O.fit(pb, ACTS, sb, X, z, perms, batch_size=16, l2=L2, dtype=np.float64)
    np.testing.assert_allclose(ha, hb, rtol=1e-12)
    assert sa.t == sb.t == 6
    for a, b in zip(pa, pb):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)       # (six Adam steps on 1e-16 apart gradients)


def test_checker_evaluate():
    p, X, z, w = case(3)
    loss, acc = WO.weighted_evaluate(p, ACTS, X, z, w, l2=L2)
    a = O.forward(p, ACTS, X, logits=True)[:, 0]
    want = np.sum(w * (np.maximum(a, 0) - a * z + np.log1p(np.exp(-np.abs(a))))) / len(X) \
        + sum(f * np.sum(q * q) for q, f in zip(p, L2))
    assert loss == pytest.approx(want, rel=1e-12)
    assert acc == O.evaluate(p, ACTS, X, z, dtype=np.float64)[1]
    assert WO.weighted_evaluate(p, ACTS, X, z, np.ones(len(X)), l2=L2)[0] == pytest.approx(
        O.evaluate(p, ACTS, X, z, dtype=np.float64, l2=L2)[0], rel=1e-12)


# ---- the argument helper --------------------------------------------------------------------------------------------
def test_no_weights_is_none():
    assert resolve_sample_weight(5) is None
    assert resolve_sample_weight(5, np.zeros(5), None, None) is None


@pytest.mark.parametrize("shape", [(6,), (6, 1)])
def test_accepted_shapes_and_dtype(shape):
    w = np.arange(6, dtype=np.float64).reshape(shape) / 3
    out = resolve_sample_weight(6, None, w)
    assert out.dtype == np.float32 and out.shape == (6,) and out.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(out, (np.arange(6) / 3).astype(np.float32))
    np.testing.assert_array_equal(resolve_sample_weight(6, None, list(w.reshape(-1))), out)      # a plain list
    np.testing.assert_array_equal(resolve_sample_weight(6, None, torch.from_numpy(w)), out)      # a tensor


def test_class_weight_and_the_product():
    z = np.array([0, 1, 1, 0, 1], dtype=bool)
    cw = resolve_sample_weight(5, z, None, {0: 0.5, 1: 2.0})
    np.testing.assert_array_equal(cw, np.where(z, 2.0, 0.5).astype(np.float32))
    np.testing.assert_array_equal(resolve_sample_weight(5, z.astype(np.float32).reshape(5, 1), None, {1: 2.0, 0: 0.5}), cw)
    w = np.array([0.3, 1.7, 0.0, 2.5, 1.0])
    both = resolve_sample_weight(5, z, w, {0: 0.5, 1: 2.0})
    np.testing.assert_array_equal(both, (w * np.where(z, 2.0, 0.5)).astype(np.float32))
    assert both.dtype == np.float32


@pytest.mark.parametrize("bad", [np.ones(4), np.ones(6), np.ones((5, 2)), np.ones((1, 5)), np.ones((5, 1, 1)), 1.0,
                                 np.array(["a"] * 5)])
def test_wrong_sample_weight_is_a_value_error(bad):
    with pytest.raises(ValueError, match="sample_weight"):
        resolve_sample_weight(5, np.zeros(5), bad)


@pytest.mark.parametrize("bad", [{0: 1.0}, {1: 2.0}, {0: 1.0, 1: 2.0, 2: 3.0}, {0: 1.0, 2: 3.0}, {}, [0.5, 2.0], "balanced"])
def test_wrong_class_weight_is_a_value_error(bad):
    with pytest.raises(ValueError, match="class_weight"):
        resolve_sample_weight(5, np.zeros(5), None, bad)


def test_class_weight_needs_labels_of_the_right_length():
    with pytest.raises(ValueError, match="class_weight"):
        resolve_sample_weight(5, np.zeros(4), None, {0: 1.0, 1: 2.0})
    with pytest.raises(ValueError, match="class_weight"):
        resolve_sample_weight(5, None, None, {0: 1.0, 1: 2.0})


# ---- the weighted entry points' host side: refusals that come back before any HIP call --------------------------------
DUMMY = C.c_void_p(0x1000)                     # (a non-null pointer nothing dereferences)
INVALID, UNSUPPORTED, NEEDS_PERM = -1, -2, -5


def desc(D, units, out="sigmoid", compute="float32"):
    from bore_amd import _lib
    return _lib.make_desc(D, units, ["relu"] * (len(units) - 1) + [out], compute=compute)


def fit(d, weights=DUMMY, N=40, epochs=1, batch_size=64, perm=None, theta=DUMMY):
    """bore_mlp_fit_weighted (weights=None: bore_mlp_fit) on dummy pointers; returns (status, message)."""
    from bore_amd import _lib
    adam = _lib.AdamCfg(1e-3, 0.9, 0.999, 1e-7)
    L = _lib.lib()
    head = (C.byref(d), 1, theta, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY)
    tail = (N, epochs, batch_size, perm, 0, 0, 0, C.byref(adam), None, None)
    rc = L.bore_mlp_fit(*head, *tail) if weights is None else L.bore_mlp_fit_weighted(*head, weights, *tail)
    return rc, L.bore_last_error().decode()


def test_weighted_bfloat16_is_refused_by_name():
    rc, msg = fit(desc(32, [128, 128, 1], compute="bfloat16"))
    assert rc == UNSUPPORTED and "weighted fits are float32 only" in msg
    assert fit(desc(2, [16, 16, 1], compute="bfloat16"))[0] == UNSUPPORTED


def test_weighted_batch_mode_is_refused():
    from bore_amd import _lib
    L = _lib.lib()
    batch = (C.c_int64 * 64)()                                   # (any non-null bore_batch: the refusal comes first)
    L.bore_set_batch(C.cast(batch, C.c_void_p))
    try:
        rc, msg = fit(desc(2, [16, 16, 1]))
        assert rc == UNSUPPORTED and "batch mode" in msg and "sample_weight" in msg
    finally:
        L.bore_set_batch(None)


@pytest.mark.parametrize("d", [desc(2, [16, 16, 1]), desc(4, [32, 32, 1]), desc(5, [24, 12, 1]), desc(8, [256, 256, 1])],
                         ids=["static", "padded", "generic", "streamed"])
def test_a_weighted_requests_own_faults_read_as_the_unweighted_ones(d):
    """The request's checks are the unweighted entry point's, whichever route either takes."""
    for kw in (dict(theta=None), dict(epochs=-1), dict(N=0), dict(batch_size=0)):
        assert fit(d, **kw) == fit(d, weights=None, **kw) and fit(d, **kw)[0] == INVALID, kw
    assert fit(d, epochs=0)[0] == 0


def test_a_weighted_request_asks_for_perm_where_the_generic_carve_does():
    """The weights are read from memory, so the carve -- and the row bound of a device-drawn shuffle -- is the unweighted
    generic flavour's: 5->24-12-1 holds 9722 rows (tests/test_fit_host.py), weighted or not."""
    d = desc(5, [24, 12, 1])
    assert fit(d, N=9723) == fit(d, weights=None, N=9723) and fit(d, N=9723)[0] == NEEDS_PERM


def test_a_network_of_neither_flavour_keeps_its_message():
    d = desc(8, [600, 600, 1])
    rc, msg = fit(d)
    assert rc == UNSUPPORTED and "BORE_STREAM_MAX_UNITS" in msg and (rc, msg) == fit(d, weights=None)


# ---- the surface ------------------------------------------------------------------------------------------------------
def test_the_surface_names_the_arguments():
    from bore_amd import _lib, models, ops
    assert {"bore_mlp_fit_weighted", "bore_mlp_evaluate_weighted"} <= set(_lib.EXPORTS)
    assert "sample_weight" in inspect.signature(ops.mlp_fit).parameters
    assert "sample_weight" in inspect.signature(ops.mlp_evaluate).parameters
    fit = inspect.signature(models.Sequential.fit).parameters
    assert fit["sample_weight"].default is None and fit["class_weight"].default is None
    assert "sample_weight" in inspect.signature(models.Sequential.evaluate).parameters
    assert "class_weight" not in inspect.signature(models.Sequential.evaluate).parameters


def test_recurrent_and_bfloat16_models_refuse_weights_by_name():
    """Refused on the host, before a device is asked for."""
    from bore_amd import _lib, models
    net = models.StackedRecurrentFactory(2, 1, num_layers=1, num_units=4).build_many_to_many()
    net.compile(optimizer="adam", loss=models.BinaryCrossentropy(from_logits=True))
    x, y = np.zeros((3, 2, 2)), np.zeros((3, 2, 1))
    with pytest.raises(_lib.UnsupportedError, match="sample_weight"):
        net.fit(x, y, sample_weight=np.ones(3))
    with pytest.raises(_lib.UnsupportedError, match="class_weight"):
        net.fit(x, y, class_weight={0: 1.0, 1: 2.0})
    with pytest.raises(_lib.UnsupportedError, match="sample_weight"):
        net.evaluate(x, y, sample_weight=np.ones(3))
    m = models.Sequential(dtype_policy="mixed_bfloat16")
    m.add(models.Dense(64, activation="relu"))
    m.add(models.Dense(1))
    with pytest.raises(_lib.UnsupportedError, match="class_weight.*float32"):
        m.fit(np.zeros((4, 16)), np.zeros(4), class_weight={0: 1.0, 1: 2.0})
    with pytest.raises(_lib.UnsupportedError, match="sample_weight.*float32"):
        m.evaluate(np.zeros((4, 16)), np.zeros(4), sample_weight=np.ones(4))
