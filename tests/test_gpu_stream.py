"""The streamed flavour (bore_amd/csrc/bore_stream.hip) against the float64 oracle: Dense networks
whose parameters do not fit one workgroup's LDS, and small ones forced onto the same kernels with
BORE_STREAM=1.  Tolerances are the project's own (tests/test_gpu_parity.py):
  forward / value      rtol 2e-5, atol 2e-6       input gradient   rtol 2e-4, atol 2e-5
  fit theta            rtol 2e-4, atol 1e-5       fit history      rtol 5e-5     step counter exact
  fit m / v            rtol 1e-3 (atol 1e-7 / 1e-10)
  evaluate             loss rel 2e-5, accuracy abs 1e-6
Properties the flavour promises are checked bit for bit: two runs, a row alone vs in a batch, a
model alone vs in a multi-model launch, device-drawn vs explicit shuffles.
"""
import warnings

import numpy as np
import pytest
import torch

from bore_amd import _lib, ops, shuffle
from oracle import bore_oracle as O

pytestmark = pytest.mark.gpu

# (D, units, activations, forced): native = refused by the LDS flavours; forced = BORE_STREAM=1
NATIVE = [
    (8, [256, 256, 1], ["relu", "elu", "linear"], False),
    (16, [128, 128, 128, 1], ["elu", "elu", "elu", "linear"], False),
    (8, [250, 130, 1], ["tanh", "relu", "sigmoid"], False),      # ragged widths beyond one panel
]
FORCED = [
    (5, [7, 3, 1], ["tanh", "sigmoid", "linear"], True),
    (1, [1], ["sigmoid"], True),
    (2, [16, 16, 1], ["relu", "relu", "sigmoid"], True),
]
SHAPES = NATIVE + FORCED
BIG = NATIVE[0]


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


def route(monkeypatch, desc, forced):
    """Put the request on the streamed kernels: natively (the query says so) or by the switch."""
    if forced:
        assert ops.mlp_streamed(desc) == 0
        monkeypatch.setenv("BORE_STREAM", "1")
    else:
        monkeypatch.delenv("BORE_STREAM", raising=False)
        assert ops.mlp_streamed(desc) == 7


@pytest.mark.parametrize("D,units,acts,forced", SHAPES)
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 131])
def test_forward_matches_oracle(gpu, monkeypatch, D, units, acts, forced, n_rows):
    rs = np.random.RandomState(D * 1000 + n_rows)
    p = rand_model(rs, D, units)
    X = rs.uniform(-1, 1, size=(n_rows, D)).astype(np.float32)
    desc = _lib.make_desc(D, units, acts)
    route(monkeypatch, desc, forced)
    out = ops.mlp_forward(desc, dev(pack(p)).reshape(1, -1), dev(X)).cpu().numpy()[0]
    ref64 = O.predict(p, acts, X, dtype=np.float64)[:, 0]
    np.testing.assert_allclose(out, ref64, rtol=2e-5, atol=2e-6)


def test_forward_of_several_models_sharing_the_rows(gpu, monkeypatch):
    D, units, acts, forced = BIG
    rs = np.random.RandomState(3)
    ps = [rand_model(rs, D, units) for _ in range(3)]
    X = rs.uniform(-1, 1, size=(131, D)).astype(np.float32)
    desc = _lib.make_desc(D, units, acts)
    route(monkeypatch, desc, forced)
    theta = dev(np.stack([pack(p) for p in ps]))
    out = ops.mlp_forward(desc, theta, dev(X)).cpu().numpy()
    for l, p in enumerate(ps):
        np.testing.assert_allclose(out[l], O.predict(p, acts, X, dtype=np.float64)[:, 0], rtol=2e-5, atol=2e-6)
        alone = ops.mlp_forward(desc, theta[l:l + 1].contiguous(), dev(X)).cpu().numpy()[0]
        np.testing.assert_array_equal(out[l], alone)


@pytest.mark.parametrize("D,units,acts,forced", SHAPES)
@pytest.mark.parametrize("transform,negate", [("identity", True), ("sigmoid", True), ("exp", True),
                                               ("sigmoid", False)])
def test_value_and_input_grad_matches_oracle(gpu, monkeypatch, D, units, acts, forced, transform, negate):
    rs = np.random.RandomState(D)
    p = rand_model(rs, D, units)
    R = 131
    X = rs.uniform(0, 1, size=(R, D))
    desc = _lib.make_desc(D, units, acts)
    route(monkeypatch, desc, forced)
    theta = dev(pack(p)).reshape(1, -1)
    val, grad = ops.mlp_value_and_input_grad(desc, theta, dev(X).reshape(1, R, D), transform, negate)
    assert val.dtype == torch.float32 and grad.dtype == torch.float64
    val, grad = val.cpu().numpy()[0], grad.cpu().numpy()[0]
    rv, rg = O.value_and_input_grad(p, acts, X, transform, dtype=np.float64)
    if not negate:   # sigmoid(f) = 1 - sigmoid(-f): the same float64 reference, reflected
        rv, rg = 1.0 - rv, -rg
    np.testing.assert_allclose(val, rv, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(grad, rg, rtol=2e-4, atol=2e-5)
    # rows are independent: a single row evaluates to the same bits as inside the batch
    v1, g1 = ops.mlp_value_and_input_grad(desc, theta, dev(X[5:6]).reshape(1, 1, D), transform, negate)
    assert v1.cpu().numpy()[0, 0] == val[5]
    np.testing.assert_array_equal(g1.cpu().numpy()[0, 0], grad[5])


def unpack(flat, D, units):
    out, off, k = [], 0, D
    for u in units:
        out.append(flat[off:off + k * u].reshape(k, u)); off += k * u
        out.append(flat[off:off + u]); off += u
        k = u
    return out


def fit_case(rs, D, units, N, E):
    p = rand_model(rs, D, units)
    X = rs.uniform(size=(N, D)).astype(np.float32)
    z = (rs.uniform(size=N) < 0.3).astype(np.float32)
    perms = np.stack([rs.permutation(N) for _ in range(E)]).astype(np.int32)
    return p, X, z, perms


def run_fit(desc, p, X, z, perms, E, B, **kw):
    N, D = X.shape
    theta = dev(pack(p)).reshape(1, -1)
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    h = ops.mlp_fit(desc, theta, m, v, t, dev(X).reshape(1, N, D), dev(z).reshape(1, N), E, B,
                    perm=None if perms is None else dev(perms).reshape(1, E, N), **kw)
    return theta, m, v, t, h


def check_fit(desc, acts, D, units, N, B, E, rs, l2=None):
    p, X, z, perms = fit_case(rs, D, units, N, E)
    p64 = [a.astype(np.float64) for a in p]
    st = O.AdamState(p64)
    hist = O.fit(p64, acts, st, X, z, perms, batch_size=B, l2=l2, dtype=np.float64)
    theta, m, v, t, h = run_fit(desc, p, X, z, perms, E, B)
    assert int(t[0]) == st.t == E * O.steps_per_epoch(N, B)
    np.testing.assert_allclose(h.cpu().numpy()[0], hist, rtol=5e-5)
    np.testing.assert_allclose(theta.cpu().numpy()[0], pack(p64), rtol=2e-4, atol=1e-5)
    np.testing.assert_allclose(m.cpu().numpy()[0], pack(st.m), rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(v.cpu().numpy()[0], pack(st.v), rtol=1e-3, atol=1e-10)
    # evaluate, on the weights the device fitted
    fitted = unpack(theta.cpu().numpy()[0], D, units)
    loss, acc = ops.mlp_evaluate(desc, theta, dev(X).reshape(1, N, D), dev(z).reshape(1, N))
    rl, ra = O.evaluate(fitted, acts, X, z, dtype=np.float64, l2=l2)
    assert float(loss[0]) == pytest.approx(float(rl), rel=2e-5)
    assert float(acc[0]) == pytest.approx(float(ra), abs=1e-6)


@pytest.mark.parametrize("D,units,acts,forced", SHAPES)
@pytest.mark.parametrize("N,B", [(1, 64), (64, 64), (65, 64), (70, 32), (7, 1), (150, 100)])
def test_fit_and_evaluate_match_oracle(gpu, monkeypatch, D, units, acts, forced, N, B):
    """A single row, the exact batch, batch + 1 (a 1-row partial batch still steps), several
    steps per epoch, batch_size 1, and a batch of more than 64 rows (two sub-tiles of one step)."""
    desc = _lib.make_desc(D, units, acts)
    route(monkeypatch, desc, forced)
    check_fit(desc, acts, D, units, N, B, 3, np.random.RandomState(N * 7 + B + D))


def test_fit_with_l2_on_the_hidden_layers(gpu, monkeypatch):
    D, units, acts, forced = BIG
    f = [1e-3, 1e-3, 0.0]
    desc = _lib.make_desc(D, units, acts, f, f)
    route(monkeypatch, desc, forced)
    check_fit(desc, acts, D, units, 70, 32, 3, np.random.RandomState(11), l2=[1e-3, 1e-3, 1e-3, 1e-3, 0.0, 0.0])
    check_fit(desc, acts, D, units, 150, 100, 3, np.random.RandomState(12), l2=[1e-3, 1e-3, 1e-3, 1e-3, 0.0, 0.0])


# ---- bit-level properties, at 8 -> 256-256-1 with N = 70 ----------------------------------------
def state(theta, m, v, t, h):
    return [x.cpu().numpy() for x in (theta, m, v, t, h)]


def test_the_same_fit_twice_gives_the_same_bits(gpu, monkeypatch):
    D, units, acts, forced = BIG
    desc = _lib.make_desc(D, units, acts)
    route(monkeypatch, desc, forced)
    p, X, z, perms = fit_case(np.random.RandomState(21), D, units, 70, 3)
    a = state(*run_fit(desc, p, X, z, perms, 3, 64))
    b = state(*run_fit(desc, p, X, z, perms, 3, 64))
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_three_models_in_one_launch_equal_three_launches(gpu, monkeypatch):
    D, units, acts, forced = BIG
    desc = _lib.make_desc(D, units, acts)
    route(monkeypatch, desc, forced)
    N, E, B = 70, 3, 64
    cases = [fit_case(np.random.RandomState(30 + l), D, units, N, E) for l in range(3)]
    theta = dev(np.stack([pack(c[0]) for c in cases]))
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    t = torch.zeros(3, dtype=torch.int64, device="cuda")
    h = ops.mlp_fit(desc, theta, m, v, t, dev(np.stack([c[1] for c in cases])), dev(np.stack([c[2] for c in cases])),
                    E, B, perm=dev(np.stack([c[3] for c in cases])))
    together = state(theta, m, v, t, h)
    for l, (p, X, z, perms) in enumerate(cases):
        alone = state(*run_fit(desc, p, X, z, perms, E, B))
        for x, y in zip(together, alone):
            np.testing.assert_array_equal(x[l], y[0])


def test_device_drawn_shuffles_are_the_projects_stream(gpu, monkeypatch):
    D, units, acts, forced = BIG
    desc = _lib.make_desc(D, units, acts)
    route(monkeypatch, desc, forced)
    N, E, B = 70, 3, 64
    p, X, z, _ = fit_case(np.random.RandomState(41), D, units, N, E)
    drawn = state(*run_fit(desc, p, X, z, None, E, B, seed=5, model_index0=2, epoch0=7))
    perms = shuffle.permutations(5, 1, E, N, model_index0=2, epoch0=7)[0]
    explicit = state(*run_fit(desc, p, X, z, perms, E, B))
    for x, y in zip(drawn, explicit):
        np.testing.assert_array_equal(x, y)


def test_warm_start_equals_one_long_fit(gpu, monkeypatch):
    D, units, acts, forced = BIG
    desc = _lib.make_desc(D, units, acts)
    route(monkeypatch, desc, forced)
    N, E = 70, 3
    p, X, z, perms = fit_case(np.random.RandomState(51), D, units, N, E)
    Xd, zd = dev(X).reshape(1, N, D), dev(z).reshape(1, N)
    perm = dev(perms).reshape(1, E, N)

    def run(splits):
        th = dev(pack(p)).reshape(1, -1)
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        t = torch.zeros(1, dtype=torch.int64, device="cuda")
        e0 = 0
        for e in splits:
            ops.mlp_fit(desc, th, m, v, t, Xd, zd, e, 64, perm=perm[:, e0:e0 + e].contiguous())
            e0 += e
        return th.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), int(t[0])

    a, b = run([E]), run([1, 2])
    assert a[3] == b[3] == 6
    for x, y in zip(a[:3], b[:3]):
        # identical arithmetic except beta^t restarts from pow() instead of a running product
        np.testing.assert_allclose(x, y, rtol=1e-6, atol=1e-9)


# ---- the public surface --------------------------------------------------------------------------
def branin01(X):
    x1, x2 = 15.0 * X[:, 0] - 5.0, 15.0 * X[:, 1]
    return ((x2 - 5.1 / (4 * np.pi ** 2) * x1 ** 2 + 5 / np.pi * x1 - 6) ** 2
            + 10 * (1 - 1 / (8 * np.pi)) * np.cos(x1) + 10)


def test_model_api_on_a_network_too_large_for_lds(gpu, monkeypatch):
    from scipy.optimize import Bounds
    from bore_amd.layers import BinaryCrossentropy, Dense
    from bore_amd.models import MaximizableSequential
    monkeypatch.delenv("BORE_STREAM", raising=False)
    rs = np.random.RandomState(0)
    X = rs.uniform(size=(40, 2))
    y = branin01(X)
    z = (y < np.quantile(y, 1 / 3)).astype(np.float64)
    model = MaximizableSequential(seed=1)
    for u, a in ((256, "relu"), (256, "relu"), (1, "linear")):
        model.add(Dense(u, activation=a))
    model.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True), metrics=["accuracy"])
    bounds = Bounds(lb=np.zeros(2), ub=np.ones(2))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        hist = model.fit(X, z, epochs=5, batch_size=64)
        assert ops.mlp_streamed(model._desc) == 7
        assert len(hist.history["loss"]) == 5 and np.all(np.isfinite(hist.history["loss"]))
        loss, acc = model.evaluate(X, z)
        assert np.isfinite(loss) and 0.0 <= acc <= 1.0
        assert model.predict(X).shape == (40, 1)
        results = model.maxima(bounds, num_starts=3, num_samples=64, print_fn=lambda s: None,
                               random_state=np.random.RandomState(7))
        best = model.argmax(bounds, num_starts=3, num_samples=64, print_fn=lambda s: None,
                            random_state=np.random.RandomState(7))
    assert len(results) == 3
    for res in results:
        assert np.all(res.x >= 0.0) and np.all(res.x <= 1.0)
        # the objective handed to L-BFGS-B is transform(-f(x)), the identity here
        np.testing.assert_allclose(res.fun, -float(model.predict(res.x[None])[0, 0]), rtol=2e-5, atol=2e-6)
    X_init = np.random.RandomState(7).uniform(low=np.zeros(2), high=np.ones(2), size=(64, 2))
    screened = -model.predict(X_init)[:, 0]
    assert min(res.fun for res in results) <= screened.min() + 2e-6
    assert best is not None and any(np.array_equal(best.x, res.x) for res in results)


def test_plugin_with_128_units(gpu, monkeypatch):
    from scipy.optimize import Bounds
    from bore_amd.plugins.classifier import ClassifierSuggester
    monkeypatch.delenv("BORE_STREAM", raising=False)
    bounds = Bounds(lb=np.zeros(3), ub=np.ones(3))
    sug = ClassifierSuggester(bounds, num_units=128, num_layers=2, num_random_init=4, num_steps_per_iter=20,
                              num_starts=2, num_samples=64, seed=0)
    sources = []
    for _ in range(4 + 5):
        x, info = sug.suggest()
        assert x.shape == (3,) and np.all(x >= 0.0) and np.all(x <= 1.0)
        sources.append(info["source"])
        sug.observe(x, float(np.sum((x - 0.3) ** 2)))
    assert "model" in sources, sources
    assert ops.mlp_streamed(sug.logit._desc) == 7          # 3 -> 128-128-128-1
    assert sug.last_fit is not None and all(np.isfinite(v) for v in sug.last_fit)


def test_bounds_are_named(gpu, monkeypatch):
    monkeypatch.delenv("BORE_STREAM", raising=False)
    desc = _lib.make_desc(8, [600, 600, 1], ["relu", "relu", "linear"])
    theta = torch.zeros((1, ops.param_count(desc)), dtype=torch.float32, device="cuda")
    X = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.UnsupportedError, match="BORE_STREAM_MAX_UNITS"):
        ops.mlp_forward(desc, theta, X)


def test_in_kernel_restarts_still_refuse(gpu, monkeypatch):
    monkeypatch.delenv("BORE_STREAM", raising=False)
    D, units, acts, _ = BIG
    desc = _lib.make_desc(D, units, acts)
    theta = dev(pack(rand_model(np.random.RandomState(0), D, units))).reshape(1, -1)
    x0 = torch.full((1, 2, D), 0.5, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.UnsupportedError, match="lock-step"):
        ops.lbfgsb_minimize(desc, theta, x0, [0.0] * D, [1.0] * D)
