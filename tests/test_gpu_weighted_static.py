"""Weighted fits on the narrow static fit kernels (fit_body<SHAPE, NW, true>: shapes 1, 2, 5, 6, 7 on four waves, 2, 5, 6 on
eight, and the nets zero-padded onto them).

The contract: a weighted fit on a static kernel gives the weighted generic flavour's bits -- theta, m, v, t and the
epoch losses -- under every gather form (rows parked a step ahead, gathered from the LDS copy, gathered from global
memory), on four and on eight waves.  BORE_FIT_WEIGHTED_STATIC=0 sends the same request to the generic flavour, so every
comparison is that switch unset against 0 on the same inputs, with np.array_equal.  The static weighted kernels get no
tolerance of their own against the float64 checker: they are the same fit, held to tests/test_gpu_weighted.py's GEN_TOL.

Rows: the edges of the pipelined form (a last step of up to 48 rows; one-wave shuffles up to 64 rows, buckets above),
of the four- and two-epoch shuffle groups, of the eight-wave kernel's shuffle drawn an epoch ahead (N > 128), and steps
in which waves 1..3 own no rows.  Weights are distinct per row (a lane that read its neighbour's would change the
result), with exact zeros at a tenth of the rows and one row of 1e-3; targets soft (u / (1 + u), as LFBO makes them) in
half the cases."""
import numpy as np
import pytest
import torch

import weighted_oracle as WO
from bore_amd import _lib, ops
from bore_amd.engine import NativeEngine
from oracle import bore_oracle as O
from test_gpu_weighted import GEN_TOL, assert_same_bits, check_against, dev, pack, rand_model

pytestmark = pytest.mark.gpu

R, S, E, LIN = "relu", "sigmoid", "elu", "linear"
NETS = {
    "2-16-16-1": (1, 2, [16, 16, 1], [R, R, S]),
    "6-32-32-1": (2, 6, [32, 32, 1], [R, R, S]),
    "16-32-32-32-1": (5, 16, [32, 32, 32, 1], [E, E, E, LIN]),
    "16-32-32-1": (6, 16, [32, 32, 1], [R, R, S]),
    "16-16-16-1": (7, 16, [16, 16, 1], [E, E, S]),
    # fewer inputs than a static shape: fitted zero-padded on it (fit_padded), weighted too
    "4-32-32-1": (2, 4, [32, 32, 1], [R, R, S]),
    "6-32-32-32-1": (5, 6, [32, 32, 32, 1], [E, E, E, LIN]),
}
W8_SHAPES = (2, 5, 6)
ROWS = [5, 48, 49, 64, 65, 112, 113, 128, 129, 200]
WAVES = [(name, w8) for name, net in NETS.items() for w8 in ((0, 1) if net[0] in W8_SHAPES else (None,))]
B, EPOCHS, MODELS = 64, 5, 3


def make_desc(name):
    _, D, units, acts = NETS[name]
    return _lib.make_desc(D, units, acts)


def padded_desc(name):
    """The descriptor the request is planned as: the static shape's own input dimension."""
    shape, _, units, acts = NETS[name]
    return _lib.make_desc({1: 2, 2: 6}.get(shape, 16), units, acts)


def make_data(seed, name, N, soft, models=MODELS):
    """`models` data sets: parameters, X, targets, weights on [0, 3] -- distinct per row and per model, exact zeros at
    about a tenth of the rows, one row of 1e-3."""
    _, D, units, _ = NETS[name]
    rs = np.random.RandomState(seed)
    th = np.stack([pack(rand_model(rs, D, units)) for _ in range(models)])
    X = rs.uniform(size=(models, N, D)).astype(np.float32)
    if soft:
        u = np.where(rs.uniform(size=(models, N)) < 0.3, rs.uniform(0, 4, size=(models, N)), 0.0)
        z = (u / (1 + u)).astype(np.float32)
    else:
        z = (rs.uniform(size=(models, N)) < 0.3).astype(np.float32)
    w = rs.uniform(0, 3, size=(models, N)).astype(np.float32)
    for l in range(models):
        rows = rs.permutation(N)
        w[l, rows[:max(1, N // 10)]] = 0.0
        w[l, rows[max(1, N // 10)]] = 1e-3
        assert N > 256 or len(np.unique(w[l][w[l] > 0])) == (w[l] > 0).sum()
    return th, X, z, w


def fit(desc, th, X, z, w, epochs=EPOCHS, perm=None):
    """`models` fits in one launch (device-drawn shuffles unless `perm`) -> [theta, m, v, t, epoch loss] as numpy."""
    theta = dev(th)
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    t = torch.zeros(len(th), dtype=torch.int64, device="cuda")
    h = ops.mlp_fit(desc, theta, m, v, t, dev(X), dev(z), epochs, B, perm=None if perm is None else dev(perm),
                    seed=29, model_index0=2, epoch0=3, sample_weight=None if w is None else dev(w))
    return [x.cpu().numpy() for x in (theta, m, v, t, h)]


def route(monkeypatch, static, w8=None):
    for var in ("BORE_STREAM", "BORE_FIT_PAD", "BORE_FIT_WEIGHTED_STATIC", "BORE_FIT_W8"):
        monkeypatch.delenv(var, raising=False)
    if not static:
        monkeypatch.setenv("BORE_FIT_WEIGHTED_STATIC", "0")
    if w8 is not None:
        monkeypatch.setenv("BORE_FIT_W8", str(w8))


def both_routes(monkeypatch, desc, data, w8=None, **kw):
    route(monkeypatch, True, w8)
    a = fit(desc, *data, **kw)
    route(monkeypatch, False, w8)
    b = fit(desc, *data, **kw)
    return a, b


def explicit_perms(seed, N, epochs, models=MODELS):
    rs = np.random.RandomState(seed)
    return np.stack([[rs.permutation(N) for _ in range(epochs)] for _ in range(models)]).astype(np.int32)


# ---- the invariant: the generic weighted flavour's bits ------------------------------------------------------------
@pytest.mark.parametrize("name,w8", WAVES)
def test_static_weighted_fit_gives_the_generic_weighted_bits(gpu, monkeypatch, name, w8):
    shape = NETS[name][0]
    desc = make_desc(name)
    for i, N in enumerate(ROWS):
        route(monkeypatch, True, w8)
        plan = ops.fit_plan_query(padded_desc(name), MODELS, N, B, False, True)
        assert (plan["flavour"], plan["data_in_lds"], plan["w8"]) == (shape, 1, int(bool(w8))), N
        data = make_data(1000 + N, name, N, soft=(i + shape) % 2 == 0)
        a, b = both_routes(monkeypatch, desc, data, w8)
        assert np.isfinite(a[0]).all() and np.all(a[3] == EPOCHS * O.steps_per_epoch(N, B)), N
        for x, y, what in zip(a, b, ("theta", "m", "v", "t", "epoch loss")):
            assert np.array_equal(x, y), (N, what)
        # three models, three weight vectors: the models differ, and the weights are not dropped
        assert not np.array_equal(a[0][0], a[0][1])
    plain = fit(desc, data[0], data[1], data[2], None)
    assert not np.array_equal(plain[0], a[0])


@pytest.mark.parametrize("name,w8", WAVES)
def test_the_same_under_explicit_shuffles(gpu, monkeypatch, name, w8):
    desc = make_desc(name)
    for i, N in enumerate((5, 65, 200)):
        data = make_data(2000 + N, name, N, soft=i % 2 == 1)
        a, b = both_routes(monkeypatch, desc, data, w8, perm=explicit_perms(2100 + N, N, EPOCHS))
        assert np.isfinite(a[0]).all()
        for x, y, what in zip(a, b, ("theta", "m", "v", "t", "epoch loss")):
            assert np.array_equal(x, y), (N, what)


@pytest.mark.parametrize("name", ["2-16-16-1", "16-32-32-32-1"])
def test_the_same_with_the_data_set_left_in_global_memory(gpu, monkeypatch, name):
    """The smallest N (in steps of 64 rows) at which the weighted static plan no longer copies X, z and the weights
    into LDS: the third gather site.  One epoch; explicit shuffles if the plan cannot draw them for that many rows."""
    shape = NETS[name][0]
    desc = make_desc(name)
    route(monkeypatch, True)
    N, with_perm = None, False
    for n in range(192, 20000, 64):
        try:
            plan = ops.fit_plan_query(desc, 1, n, B, with_perm, True)
        except _lib.NeedsPermError:
            with_perm = True
            plan = ops.fit_plan_query(desc, 1, n, B, with_perm, True)
        if plan["flavour"] == shape and not plan["data_in_lds"]:
            N = n + 1                                     # (an odd last step)
            plan = ops.fit_plan_query(desc, 1, N, B, with_perm, True)
            assert plan["flavour"] == shape and not plan["data_in_lds"] and plan["o_w"] == 0
            break
    assert N is not None
    data = make_data(3000 + N, name, N, soft=shape == 5, models=1)
    perm = explicit_perms(3100, N, 1, models=1) if with_perm else None
    a, b = both_routes(monkeypatch, desc, data, epochs=1, perm=perm)
    assert np.isfinite(a[0]).all() and int(a[3][0]) == O.steps_per_epoch(N, B)
    assert_same_bits(a, b)
    plain = fit(desc, data[0], data[1], data[2], None, epochs=1, perm=perm)
    assert not np.array_equal(plain[0], a[0])


# ---- the float64 checker ----------------------------------------------------------------------------------------------
CHECKER = [("2-16-16-1", None), ("16-32-32-32-1", 0), ("16-32-32-32-1", 1)]
_refs = {}


def checker_ref(name, N):
    """The float64 trajectory on the shuffles the device draws for (seed 29, model 2, epoch 3 ..): once per (net, N)."""
    if (name, N) not in _refs:
        _, D, units, acts = NETS[name]
        th, X, z, w = make_data(4000 + N, name, N, soft=N == 100, models=1)
        rs = np.random.RandomState(4000 + N)                       # (make_data's first draws: the same parameters)
        p = rand_model(rs, D, units)
        assert np.array_equal(pack(p), th[0])
        perms = ops.shuffle_perm(29, 1, EPOCHS, N, model_index0=2, epoch0=3).cpu().numpy()[0]
        p64 = [a.astype(np.float64) for a in p]
        st = O.AdamState(p64)
        hist = WO.weighted_fit(p64, acts, st, X[0], z[0], w[0], perms, batch_size=B)
        ref = dict(theta=pack(p64), m=pack(st.m), v=pack(st.v), t=st.t, hist=hist)
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refs[(name, N)] = ((th, X, z, w), ref)
    return _refs[(name, N)]


@pytest.mark.parametrize("N", [48, 100])
@pytest.mark.parametrize("name,w8", CHECKER)
def test_static_weighted_fit_matches_the_checker(gpu, monkeypatch, name, w8, N):
    data, ref = checker_ref(name, N)
    route(monkeypatch, True, w8)
    assert ops.fit_plan_query(make_desc(name), 1, N, B, False, True)["flavour"] == NETS[name][0]
    got = fit(make_desc(name), *data)
    check_against(ref, got, GEN_TOL, EPOCHS * O.steps_per_epoch(N, B))


# ---- zero weights, unit weights ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w8", [("2-16-16-1", None), ("16-32-32-32-1", 0), ("16-32-32-32-1", 1), ("6-32-32-1", 1)])
def test_zero_weight_rows_are_inert_on_the_static_kernels(gpu, monkeypatch, name, w8):
    """Rows of weight 0 with X and z replaced by large finite values: the same theta, m, v, bit for bit."""
    desc = make_desc(name)
    route(monkeypatch, True, w8)
    for N in (48, 100, 129):
        th, X, z, w = make_data(5000 + N, name, N, soft=False)
        dead = w == 0.0
        assert dead.sum() >= MODELS * (N // 10)
        X2, z2 = X.copy(), z.copy()
        X2[dead] = 3e4
        z2[dead] = -7e3
        a = fit(desc, th, X, z, w)
        b = fit(desc, th, X2, z2, w)
        assert np.isfinite(a[0]).all() and np.isfinite(b[4]).all()
        for x, y, what in zip(a[:3], b[:3], ("theta", "m", "v")):
            assert np.array_equal(x, y), (N, what)


@pytest.mark.parametrize("name,w8", WAVES)
def test_unit_weights_on_the_static_route_are_the_unweighted_static_fit(gpu, monkeypatch, name, w8):
    desc = make_desc(name)
    route(monkeypatch, True, w8)
    for N in (48, 100, 129):
        assert ops.fit_plan_query(padded_desc(name), MODELS, N, B, False, True)["flavour"] == NETS[name][0]
        th, X, z, _ = make_data(6000 + N, name, N, soft=N == 100)
        plain = fit(desc, th, X, z, None)
        unit = fit(desc, th, X, z, np.ones_like(z))
        for x, y, what in zip(plain, unit, ("theta", "m", "v", "t", "epoch loss")):
            assert np.array_equal(x, y), (N, what)


# ---- end to end: the lock-step engine under LFBO weighting, on the static kernel ----------------------------------------
def quadratic(X):
    return np.sum((X - 0.3) ** 2, axis=-1)


ENGINE = dict(input_dim=2, units=(16, 16, 1), acts=(R, R, S), n_init=5, epochs=4, batch_size=64, num_starts=2,
              num_samples=64, objective=quadratic, seed=7, gamma=1 / 3, options=dict(maxiter=30, ftol=1e-9))
IDS = np.arange(3, 6)


def engine_run(steps):
    a = NativeEngine(IDS, groups=1, **ENGINE, weighting="lfbo")
    th0 = a.state()[0]
    a.run(steps)
    X, y = a.observations()
    out = dict(X=X, y=y, th0=th0, state=a.state())
    a.close()
    return out


def test_the_lfbo_engine_runs_the_static_kernel_to_the_generic_bits(gpu, monkeypatch):
    route(monkeypatch, True)
    assert ops.fit_plan_query(_lib.make_desc(2, [16, 16, 1], [R, R, S]), 3, 5, 64, False, True)["flavour"] == 1
    a = engine_run(3)
    first = engine_run(1)
    route(monkeypatch, False)
    b = engine_run(3)
    assert a["X"].shape == (3, 5 + 3, 2)
    assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["y"], b["y"])
    for x, y in zip(a["state"], b["state"]):
        assert np.array_equal(x, y)
    assert np.all(a["state"][3] == 4 * 3) and not np.array_equal(a["state"][0], a["th0"])
    # the first step by hand, switch unset: bore_lfbo_labels -> bore_mlp_fit_weighted on the static kernel
    route(monkeypatch, True)
    desc = _lib.make_desc(2, [16, 16, 1], [R, R, S])
    th, m, v, t = first["state"]
    for l in range(3):
        z, w = ops.lfbo_labels(dev(first["y"][l:l + 1, :5]), ENGINE["gamma"], "lfbo", True)
        theta = dev(first["th0"][l:l + 1])
        dm, dv = torch.zeros_like(theta), torch.zeros_like(theta)
        dt = torch.zeros(1, dtype=torch.int64, device="cuda")
        ops.mlp_fit(desc, theta, dm, dv, dt, dev(first["X"][l:l + 1, :5].astype(np.float32)), z, ENGINE["epochs"], 64,
                    seed=ENGINE["seed"], model_index0=int(IDS[l]), epoch0=0, want_loss=False, sample_weight=w)
        assert np.array_equal(theta.cpu().numpy()[0], th[l]) and np.array_equal(dm.cpu().numpy()[0], m[l])
        assert np.array_equal(dv.cpu().numpy()[0], v[l]) and int(dt[0]) == int(t[l]) == 4
