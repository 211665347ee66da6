"""Weighted fits on the device (Keras ``sample_weight`` / ``class_weight``: bore_mlp_fit_weighted,
bore_mlp_evaluate_weighted) against the float64 checker tests/weighted_oracle.py, on the two kernel flavours that take
weights: the generic LDS flavour and the streamed one (natively, and forced with BORE_STREAM=1).

Tolerances are the project's own for the same comparisons:
  generic fit (tests/test_gpu_parity.py, the fits against the float64 trajectory)
      epoch loss rtol 5e-5;  theta rtol 2e-4 / atol 1e-5;  m rtol 2e-3 / atol 1e-7;
      v rtol 1e-3 / atol 1e-10 -- that file's one bound on v against the float64 trajectory (the golden fits), the
      tighter of the bounds the project holds v to anywhere
  streamed fit (tests/test_gpu_stream.py)
      epoch loss rtol 5e-5;  theta rtol 2e-4 / atol 1e-5;  m rtol 1e-3 / atol 1e-7;  v rtol 1e-3 / atol 1e-10
  evaluate  loss rel 2e-5, accuracy equal to the unweighted call's
Everything the feature promises exactly is checked bit for bit: unit weights are the unweighted fit (whatever kernel
that one takes), w = 2 doubles the logged loss, zero-weight rows are inert, a model alone equals the model in a
multi-model launch, E + E epochs equal 2 E, class_weight equals the sample_weight it stands for."""
import numpy as np
import pytest
import torch

import weighted_oracle as WO
from bore_amd import _lib, ops
from bore_amd.layers import Dense
from bore_amd.models import BinaryCrossentropy, Sequential, StackedRecurrentFactory
from oracle import bore_oracle as O

pytestmark = pytest.mark.gpu

GENERIC = (3, [5, 7, 1], ["elu", "tanh", "linear"])
L2_LAYERS = [1e-3, 2e-3, 0.0]                                    # per layer (kernel and bias alike)
L2_TENSORS = [1e-3, 1e-3, 2e-3, 2e-3, 0.0, 0.0]                  # the same, per tensor (the oracle's form)
BIG = (16, [128, 128, 128, 1], ["elu", "elu", "elu", "linear"])  # refused by the LDS flavours: streamed natively
GEN_TOL = dict(hist=dict(rtol=5e-5), theta=dict(rtol=2e-4, atol=1e-5), m=dict(rtol=2e-3, atol=1e-7),
               v=dict(rtol=1e-3, atol=1e-10))
STREAM_TOL = dict(hist=dict(rtol=5e-5), theta=dict(rtol=2e-4, atol=1e-5), m=dict(rtol=1e-3, atol=1e-7),
                  v=dict(rtol=1e-3, atol=1e-10))


def pack(params):
    return np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in params])


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def rand_model(rs, D, units):
    p = O.glorot_uniform_params(D, units, rs)
    for i in range(1, len(p), 2):
        p[i] = rs.normal(scale=0.1, size=p[i].shape).astype(np.float32)
    return p


def make_case(seed, D, units, N, E, zeros=2):
    """Parameters, float32 data, labels, weights uniform on [0, 3] with `zeros` exact zeros, explicit shuffles."""
    rs = np.random.RandomState(seed)
    p = rand_model(rs, D, units)
    X = rs.uniform(size=(N, D)).astype(np.float32)
    z = (rs.uniform(size=N) < 0.3).astype(np.float32)
    w = rs.uniform(0, 3, size=N).astype(np.float32)
    w[rs.choice(N, size=zeros, replace=False)] = 0.0
    perms = np.stack([rs.permutation(N) for _ in range(E)]).astype(np.int32)
    return p, X, z, w, perms


def run_fit(desc, p, X, z, w, perms, E, B, **kw):
    """One model through ops.mlp_fit; -> [theta, m, v, t, epoch loss] as numpy."""
    N, D = X.shape
    theta = dev(pack(p)).reshape(1, -1)
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    h = ops.mlp_fit(desc, theta, m, v, t, dev(X).reshape(1, N, D), dev(z).reshape(1, N), E, B,
                    perm=None if perms is None else dev(perms).reshape(1, E, N),
                    sample_weight=None if w is None else dev(w).reshape(1, N), **kw)
    return [x.cpu().numpy() for x in (theta, m, v, t, h)]


def assert_same_bits(a, b):
    for name, x, y in zip(("theta", "m", "v", "t", "epoch loss"), a, b):
        np.testing.assert_array_equal(x, y, err_msg=name)


def stream(monkeypatch, on):
    if on:
        monkeypatch.setenv("BORE_STREAM", "1")
    else:
        monkeypatch.delenv("BORE_STREAM", raising=False)


# ---- the float64 references, computed once and left alone -----------------------------------------------------------
def reference(net, N, B, E, seed, l2):
    D, units, acts = net
    p, X, z, w, perms = make_case(seed, D, units, N, E)
    p64 = [a.astype(np.float64) for a in p]
    st = O.AdamState(p64)
    hist = WO.weighted_fit(p64, acts, st, X, z, w, perms, batch_size=B, l2=L2_TENSORS if l2 else None)
    ref = dict(theta=pack(p64), m=pack(st.m), v=pack(st.v), t=st.t, hist=hist)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return (p, X, z, w, perms), ref


@pytest.fixture(scope="module")
def generic_refs():
    return {(37, 16): reference(GENERIC, 37, 16, 3, 101, True),      # three steps an epoch, the last of 5 rows
            (150, 130): reference(GENERIC, 150, 130, 3, 102, True)}   # 130 rows: three sub-tiles of one step


@pytest.fixture(scope="module")
def big_ref():
    return reference(BIG, 70, 64, 2, 103, False)


def check_against(ref, got, tol, t_want):
    theta, m, v, t, h = got
    assert int(t[0]) == ref["t"] == t_want
    for name, g in (("hist", h[0]), ("theta", theta[0]), ("m", m[0]), ("v", v[0])):
        r = ref[name]
        err = np.abs(g - r) / (tol[name].get("atol", 0.0) + tol[name]["rtol"] * np.abs(r))
        print(f"{name}: largest error {err.max():.3f} of the tolerance")
        np.testing.assert_allclose(g, r, err_msg=name, **tol[name])


# ---- 1, 2: parity with the float64 checker ----------------------------------------------------------------------------
@pytest.mark.parametrize("N,B", [(37, 16), (150, 130)])
def test_generic_weighted_fit_matches_the_checker(gpu, monkeypatch, generic_refs, N, B):
    stream(monkeypatch, False)
    D, units, acts = GENERIC
    desc = _lib.make_desc(D, units, acts, L2_LAYERS, L2_LAYERS)
    assert ops.mlp_streamed(desc) == 0
    (p, X, z, w, perms), ref = generic_refs[(N, B)]
    got = run_fit(desc, p, X, z, w, perms, 3, B)
    check_against(ref, got, GEN_TOL, 3 * O.steps_per_epoch(N, B))
    # the weights are not dropped: the unweighted fit of the same request is somewhere else
    plain = run_fit(desc, p, X, z, None, perms, 3, B)
    assert np.abs(plain[4][0] - ref["hist"]).max() > 1e-2 * np.abs(ref["hist"]).max()


@pytest.mark.parametrize("N,B", [(37, 16), (150, 130)])
def test_forced_streamed_weighted_fit_matches_the_checker(gpu, monkeypatch, generic_refs, N, B):
    stream(monkeypatch, True)
    D, units, acts = GENERIC
    desc = _lib.make_desc(D, units, acts, L2_LAYERS, L2_LAYERS)
    (p, X, z, w, perms), ref = generic_refs[(N, B)]
    got = run_fit(desc, p, X, z, w, perms, 3, B)
    check_against(ref, got, STREAM_TOL, 3 * O.steps_per_epoch(N, B))
    plain = run_fit(desc, p, X, z, None, perms, 3, B)
    assert np.abs(plain[4][0] - ref["hist"]).max() > 1e-2 * np.abs(ref["hist"]).max()


def test_native_streamed_weighted_fit_matches_the_checker(gpu, monkeypatch, big_ref):
    stream(monkeypatch, False)
    D, units, acts = BIG
    desc = _lib.make_desc(D, units, acts)
    assert ops.mlp_streamed(desc) & 4                     # the fit's LDS check refuses it: the streamed flavour
    (p, X, z, w, perms), ref = big_ref
    got = run_fit(desc, p, X, z, w, perms, 2, 64)
    check_against(ref, got, STREAM_TOL, 2 * 2)
    plain = run_fit(desc, p, X, z, None, perms, 2, 64)
    assert np.abs(plain[4][0] - ref["hist"]).max() > 1e-2 * np.abs(ref["hist"]).max()


# ---- 3: unit weights are the unweighted fit ---------------------------------------------------------------------------
UNIT_NETS = [
    # (D, units, acts, l2, forced, N, B, explicit shuffles)
    pytest.param(*GENERIC, True, False, 37, 16, True, id="generic"),
    pytest.param(*GENERIC, True, False, 150, 130, True, id="generic-subtiles"),
    # unweighted: the static 2->16-16-1 kernel (device-drawn shuffles: its pipelined form); weighted: flavour 0
    pytest.param(2, [16, 16, 1], ["relu", "relu", "sigmoid"], False, False, 100, 64, False, id="static-2-16-16-1"),
    # unweighted: zero-padded onto static shape 5 (fit_padded); weighted: flavour 0 on the six inputs
    pytest.param(6, [32, 32, 32, 1], ["elu", "elu", "elu", "linear"], False, False, 100, 64, False, id="padded-6-32-32-32-1"),
    pytest.param(*GENERIC, True, True, 37, 16, True, id="forced-streamed"),
]


@pytest.mark.parametrize("D,units,acts,l2,forced,N,B,explicit", UNIT_NETS)
def test_unit_weights_give_the_unweighted_fits_bits(gpu, monkeypatch, D, units, acts, l2, forced, N, B, explicit):
    stream(monkeypatch, forced)
    monkeypatch.delenv("BORE_FIT_PAD", raising=False)
    lk = L2_LAYERS if l2 else None
    desc = _lib.make_desc(D, units, acts, lk, lk)
    E = 3
    p, X, z, _, perms = make_case(7 + N + D, D, units, N, E)
    kw = dict() if explicit else dict(seed=11, model_index0=3, epoch0=5)
    plain = run_fit(desc, p, X, z, None, perms if explicit else None, E, B, **kw)
    unit = run_fit(desc, p, X, z, np.ones(N, dtype=np.float32), perms if explicit else None, E, B, **kw)
    assert np.isfinite(plain[4]).all() and int(plain[3][0]) == E * O.steps_per_epoch(N, B)
    assert_same_bits(plain, unit)


# ---- 4: scale -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True], ids=["generic", "streamed"])
def test_weights_of_two_double_the_logged_loss(gpu, monkeypatch, forced):
    """No l2, one epoch of one batch: every row's term is doubled exactly, so is every partial sum."""
    stream(monkeypatch, forced)
    D, units, acts = GENERIC
    desc = _lib.make_desc(D, units, acts)
    N = 20
    p, X, z, _, perms = make_case(31, D, units, N, 1)
    plain = run_fit(desc, p, X, z, None, perms, 1, 32)
    twice = run_fit(desc, p, X, z, np.full(N, 2.0, dtype=np.float32), perms, 1, 32)
    assert plain[4].shape == (1, 1) and plain[4][0, 0] > 0
    np.testing.assert_array_equal(twice[4], np.float32(2.0) * plain[4])
    assert not np.array_equal(twice[0], plain[0])


# ---- 5: zero-weight rows are inert -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True], ids=["generic", "streamed"])
@pytest.mark.parametrize("N,B", [(37, 16), (150, 130)])
def test_zero_weight_rows_are_inert(gpu, monkeypatch, forced, N, B):
    stream(monkeypatch, forced)
    D, units, acts = GENERIC
    desc = _lib.make_desc(D, units, acts, L2_LAYERS, L2_LAYERS)
    p, X, z, w, perms = make_case(41 + N, D, units, N, 3, zeros=5)
    dead = w == 0.0
    assert dead.sum() == 5
    X2 = X.copy()
    X2[dead] = np.random.RandomState(42).uniform(-2, 2, size=(5, D)).astype(np.float32)   # other moderate values
    assert not np.array_equal(X, X2)
    a = run_fit(desc, p, X, z, w, perms, 3, B)
    b = run_fit(desc, p, X2, z, w, perms, 3, B)
    assert np.isfinite(a[0]).all()
    assert_same_bits(a, b)


# ---- 6: models are independent, launches compose ------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True], ids=["generic", "streamed"])
def test_three_models_with_three_weight_vectors_equal_three_launches(gpu, monkeypatch, forced):
    stream(monkeypatch, forced)
    D, units, acts = GENERIC
    desc = _lib.make_desc(D, units, acts, L2_LAYERS, L2_LAYERS)
    N, E, B = 37, 3, 16
    cases = [make_case(50 + l, D, units, N, E) for l in range(3)]
    theta = dev(np.stack([pack(c[0]) for c in cases]))
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    t = torch.zeros(3, dtype=torch.int64, device="cuda")
    h = ops.mlp_fit(desc, theta, m, v, t, dev(np.stack([c[1] for c in cases])), dev(np.stack([c[2] for c in cases])),
                    E, B, perm=dev(np.stack([c[4] for c in cases])), sample_weight=dev(np.stack([c[3] for c in cases])))
    together = [x.cpu().numpy() for x in (theta, m, v, t, h)]
    for l, (p, X, z, w, perms) in enumerate(cases):
        alone = run_fit(desc, p, X, z, w, perms, E, B)
        for name, x, y in zip(("theta", "m", "v", "t", "epoch loss"), together, alone):
            np.testing.assert_array_equal(x[l], y[0], err_msg=f"model {l}: {name}")
    assert not np.array_equal(together[0][0], together[0][1])


@pytest.mark.parametrize("forced", [False, True], ids=["generic", "streamed"])
def test_weighted_epochs_in_two_launches_equal_one_launch(gpu, monkeypatch, forced):
    stream(monkeypatch, forced)
    D, units, acts = GENERIC
    desc = _lib.make_desc(D, units, acts, L2_LAYERS, L2_LAYERS)
    N, E, B = 37, 2, 16
    p, X, z, w, perms = make_case(61, D, units, N, 2 * E)
    Xd, zd, wd = dev(X).reshape(1, N, D), dev(z).reshape(1, N), dev(w).reshape(1, N)
    perm = dev(perms).reshape(1, 2 * E, N)

    def run(splits):
        th = dev(pack(p)).reshape(1, -1)
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        t = torch.zeros(1, dtype=torch.int64, device="cuda")
        e0, hs = 0, []
        for e in splits:
            hs.append(ops.mlp_fit(desc, th, m, v, t, Xd, zd, e, B, perm=perm[:, e0:e0 + e].contiguous(),
                                  sample_weight=wd))
            e0 += e
        return [x.cpu().numpy() for x in (th, m, v, t, torch.cat(hs, dim=1))]

    assert_same_bits(run([2 * E]), run([E, E]))


# ---- 7: the model API ---------------------------------------------------------------------------------------------------
def new_model():
    D, units, acts = GENERIC
    model = Sequential(seed=3)
    for u, a in zip(units, acts):
        model.add(Dense(u, activation=a))
    model.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True), metrics=["accuracy"])
    model.build(D)
    return model


def model_state(model, hist):
    return [model.theta.cpu().numpy(), model.adam_m.cpu().numpy(), model.adam_v.cpu().numpy(),
            model.adam_t.cpu().numpy(), np.asarray(hist.history["loss"], dtype=np.float32)[None]]


def test_model_api_class_weight_sample_weight_and_their_product(gpu, monkeypatch):
    stream(monkeypatch, False)
    D, units, acts = GENERIC
    N, E, B = 37, 3, 16
    _, X, z, w, _ = make_case(71, D, units, N, E)
    zb = z > 0.5
    cw = {0: 0.5, 1: 2.0}
    as_sw = np.where(zb, 2.0, 0.5)

    def fit(**kw):
        model = new_model()
        return model, model_state(model, model.fit(X.astype(np.float64), zb, epochs=E, batch_size=B, **kw))

    _, by_class = fit(class_weight=cw)
    _, by_sample = fit(sample_weight=as_sw)
    assert_same_bits(by_class, by_sample)
    _, both = fit(sample_weight=w, class_weight=cw)
    _, product = fit(sample_weight=(w * as_sw).reshape(N, 1))                # (the (N, 1) form)
    assert_same_bits(both, product)
    _, plain = fit()
    assert not np.array_equal(by_class[0], plain[0]) and not np.array_equal(by_class[4], plain[4])
    # device tensors in: the same fit as host arrays in (the weights ride in the pinned staging copy there)
    model = new_model()
    on_dev = model_state(model, model.fit(dev(X), dev(z), epochs=E, batch_size=B, sample_weight=dev(w), class_weight=cw))
    assert_same_bits(both, on_dev)
    # ... and the ops-level call on the model's own initial weights and shuffle stream
    model, weighted = fit(sample_weight=w)
    fresh = new_model()
    desc = _lib.make_desc(D, units, acts)
    got = run_fit(desc, fresh.get_weights(), X, z, w, None, E, B, seed=fresh._shuffle_seed, epoch0=0)
    assert_same_bits(weighted, got)
    # per-epoch launches (callbacks) pass the weights through as well
    seen = []

    class Log:
        def on_epoch_end(self, epoch, logs):
            seen.append(logs["loss"])

    _, stepped = fit(sample_weight=w, callbacks=[Log()])
    assert len(seen) == E
    assert_same_bits(weighted, stepped)


def test_model_fit_of_a_long_data_set_passes_the_weights_on(gpu, monkeypatch):
    """More rows than the device draws a shuffle for in LDS (``NeedsPermError``): ``Sequential.fit`` then passes the
    stream's shuffles from their host statement, a few epochs per launch -- with the weights.  Equal, bit for bit, to
    the tensor-level launch with those shuffles; batch_size 2048, so the two epochs are 16 Adam steps."""
    from bore_amd import shuffle
    stream(monkeypatch, False)
    D, units, acts = GENERIC
    N, E, B = 15000, 2, 2048
    _, X, z, w, _ = make_case(75, D, units, N, 1)
    model = new_model()
    desc = _lib.make_desc(D, units, acts)
    p0 = model.get_weights()
    with pytest.raises(_lib.NeedsPermError):
        run_fit(desc, p0, X, z, w, None, E, B, seed=model._shuffle_seed)
    perms = shuffle.permutations(model._shuffle_seed, 1, E, N)[0].astype(np.int32)
    want = run_fit(desc, p0, X, z, w, perms, E, B)
    got = model_state(model, model.fit(X, z, epochs=E, batch_size=B, sample_weight=w))
    assert int(got[3][0]) == E * O.steps_per_epoch(N, B) == 16
    assert_same_bits(want, got)
    plain = run_fit(desc, p0, X, z, None, perms, E, B)
    assert not np.array_equal(plain[0], want[0])


# ---- 8: evaluate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True], ids=["generic", "streamed"])
def test_weighted_evaluate_matches_the_checker(gpu, monkeypatch, forced):
    stream(monkeypatch, forced)
    D, units, acts = GENERIC
    desc = _lib.make_desc(D, units, acts, L2_LAYERS, L2_LAYERS)
    N = 150
    p, X, z, w, _ = make_case(81, D, units, N, 1)
    theta = dev(pack(p)).reshape(1, -1)
    Xd, zd = dev(X).reshape(1, N, D), dev(z).reshape(1, N)
    loss, acc = ops.mlp_evaluate(desc, theta, Xd, zd, sample_weight=dev(w).reshape(1, N))
    loss0, acc0 = ops.mlp_evaluate(desc, theta, Xd, zd)
    rl, ra = WO.weighted_evaluate(p, acts, X, z, w, l2=L2_TENSORS)
    print(f"weighted evaluate: {float(loss[0])!r} against {rl!r}")
    assert float(loss[0]) == pytest.approx(rl, rel=2e-5)
    assert float(acc[0]) == float(acc0[0]) == pytest.approx(ra, abs=1e-6)
    assert abs(float(loss[0]) - float(loss0[0])) > 1e-2 * float(loss0[0])         # (the weights are not dropped)
    unit, _ = ops.mlp_evaluate(desc, theta, Xd, zd, sample_weight=torch.ones_like(zd))
    assert float(unit[0]) == pytest.approx(float(loss0[0]), rel=2e-5)


def test_model_evaluate_takes_sample_weight(gpu, monkeypatch):
    stream(monkeypatch, False)
    D, units, acts = GENERIC
    N = 37
    _, X, z, w, _ = make_case(82, D, units, N, 1)
    model = new_model()
    loss, acc = model.evaluate(X, z, sample_weight=w.reshape(N, 1))
    loss0, acc0 = model.evaluate(X, z)
    rl, _ = WO.weighted_evaluate(model.get_weights(), acts, X, z, w)
    assert loss == pytest.approx(rl, rel=2e-5) and acc == acc0 and loss != loss0


# ---- 9: refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(gpu, monkeypatch):
    stream(monkeypatch, False)
    # a bfloat16 descriptor with weights
    D, units = 16, [64, 64, 64, 1]
    desc = _lib.make_desc(D, units, ["relu"] * 3 + ["sigmoid"], compute="bfloat16")
    N = 70
    p, X, z, w, _ = make_case(91, D, units, N, 1)
    before = pack(p)
    theta = dev(before).reshape(1, -1)
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.UnsupportedError, match="float32"):
        ops.mlp_fit(desc, theta, m, v, t, dev(X).reshape(1, N, D), dev(z).reshape(1, N), 1, 64, seed=1,
                    sample_weight=dev(w).reshape(1, N))
    np.testing.assert_array_equal(theta.cpu().numpy()[0], before)
    assert int(t[0]) == 0
    # a recurrent model
    net = StackedRecurrentFactory(2, 1, num_layers=1, num_units=8, seed=0).build_many_to_many()
    net.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True))
    xs, ys = np.zeros((5, 3, 2)), np.zeros((5, 3, 1))
    with pytest.raises(_lib.UnsupportedError, match="sample_weight"):
        net.fit(xs, ys, sample_weight=np.ones(5))
    # a weight vector of the wrong length: a ValueError on the host, nothing launched
    model = new_model()
    th0 = model.theta.cpu().numpy().copy()
    Dg = GENERIC[0]
    for bad in (np.ones(N + 1), np.ones(N - 1), np.ones((N, 2))):
        with pytest.raises(ValueError, match="sample_weight"):
            model.fit(np.zeros((N, Dg)), z, epochs=1, batch_size=16, sample_weight=bad)
        with pytest.raises(ValueError, match="sample_weight"):
            model.evaluate(np.zeros((N, Dg)), z, sample_weight=bad)
    with pytest.raises(ValueError, match="class_weight"):
        model.fit(np.zeros((N, Dg)), z, epochs=1, batch_size=16, class_weight={0: 1.0})
    np.testing.assert_array_equal(model.theta.cpu().numpy(), th0)
    assert int(model.adam_t[0]) == 0 and model._epochs_seen == 0
    # the tensor-level operator checks the shape too
    gd = _lib.make_desc(*GENERIC)
    pg, Xg, zg, wg, _ = make_case(92, *GENERIC[:2], 37, 1)
    th = dev(pack(pg)).reshape(1, -1)
    tg = torch.zeros(1, dtype=torch.int64, device="cuda")
    for bad in (dev(wg[:-1]).reshape(1, 36), dev(wg), dev(wg.astype(np.float64)).reshape(1, 37)):
        with pytest.raises((ValueError, TypeError), match="sample_weight"):
            ops.mlp_fit(gd, th, torch.zeros_like(th), torch.zeros_like(th), tg, dev(Xg).reshape(1, 37, 3),
                        dev(zg).reshape(1, 37), 1, 16, seed=1, sample_weight=bad)
        with pytest.raises((ValueError, TypeError), match="sample_weight"):
            ops.mlp_evaluate(gd, th, dev(Xg).reshape(1, 37, 3), dev(zg).reshape(1, 37), sample_weight=bad)
    assert int(tg[0]) == 0
