"""Screening and L-BFGS-B restarts of the one-to-one recurrent network on the streamed LSTM kernels
(bore_lstm_stream_screen_topk, bore_lstm_stream_lbfgsb_minimize) and the opt-in route to them through the model
API and the Hyperband plugin.

The bar for the restarts is the project's standing one for every form of the optimiser: every record equals the
HOST build of lbfgsb.h fed the f and g of ops.lstm_stream_value_and_input_grad, bit for bit, no tolerance (the
streamed LSTM kernels give a row the bits it has in any tile, which is what makes that checkable).  SciPy's result on
the same f/g is printed, not asserted (tests/test_lbfgsb_host.py pins the host build to SciPy)."""
import warnings

import numpy as np
import pytest
from scipy.optimize import Bounds

import lbfgsb_host as H
from test_gpu_lstm_shapes import VAL_TOL, _desc, _dev, _thetas, _weights

pytestmark = pytest.mark.gpu

# (D, L, H, activation, T): fits LDS, ragged, one row of gates per lane group | 4H = 132: a second column pass,
# reductions 33 deep | streamed only, the plugin's widths
NETS = [(3, 1, 7, "relu", 4), (5, 2, 33, "sigmoid", 3), (48, 2, 32, "elu", 5)]
OPTS = dict(maxiter=1000, ftol=1e-9)
R_MAX = 9


def make(k_or_shape, n_models, seed):
    D, L, Hn, act, T = NETS[k_or_shape] if isinstance(k_or_shape, int) else k_or_shape
    rs = np.random.RandomState(seed)
    th = _thetas([_weights(D, Hn, L, rs) for _ in range(n_models)])
    return rs, _desc(D, Hn, L, act), th


def fg_of(desc, th_l, T, tr):
    from bore_amd import ops

    def fg(xx):
        v, g = ops.lstm_stream_value_and_input_grad(desc, th_l, _dev(np.atleast_2d(xx)[None], np.float64), T, tr, True)
        return v.cpu().numpy()[0], g.cpu().numpy()[0]
    return fg


def host(desc, th_l, T, tr, x0, lo, hi, **opts):
    f = fg_of(desc, th_l, T, tr)
    return H.minimize(lambda xx: tuple(a[0] for a in f(xx)), x0, (np.asarray(lo, float), np.asarray(hi, float)), **opts)


def run(desc, th, X0, lo, hi, T, tr, **opts):
    from bore_amd import ops
    return ops.lbfgsb_results_to_host(*ops.lstm_stream_lbfgsb_minimize(desc, th, _dev(X0, np.float64), lo, hi, T, tr, True,
                                                                       **opts))


def same_record(h, x, fun, jac, info, where):
    np.testing.assert_array_equal(h.x, x, err_msg=str(where))
    assert h.fun == fun, where
    np.testing.assert_array_equal(h.jac, jac, err_msg=str(where))
    assert (h.nit, h.nfev, h.status) == tuple(info[:3]), where
    assert h.task == tuple(info[3:]), where


_reference = {}


def reference(k, tr):
    """Network k with two models, nine starts each from U(-0.1, 1.1)^D -- some outside the box [0, 1]^D -- and the host
    build's record of every start.  Computed once per (network, transform); nobody writes to it."""
    if (k, tr) not in _reference:
        D, T = NETS[k][0], NETS[k][4]
        rs, desc, th = make(k, 2, 100 + k)
        X0 = rs.uniform(-0.1, 1.1, size=(2, R_MAX, D))
        lo, hi = np.zeros(D), np.ones(D)
        rec = [[host(desc, th[l:l + 1], T, tr, X0[l, r], lo, hi, **OPTS) for r in range(R_MAX)] for l in range(2)]
        _reference[(k, tr)] = (desc, th, X0, lo, hi, rec)
    return _reference[(k, tr)]


@pytest.mark.parametrize("tr", ["identity", "sigmoid"])
@pytest.mark.parametrize("k", range(len(NETS)))
def test_restarts_equal_the_host_build_bit_for_bit(gpu, k, tr):
    from bore_amd.optimizers import lockstep
    D, T = NETS[k][0], NETS[k][4]
    desc, th, X0, lo, hi, rec = reference(k, tr)
    for R in (1, 3, 4, 5, 9):       # 1: three waves idle; 5, 9: a second group with one problem
        x, fun, jac, info = run(desc, th, X0[:, :R], lo, hi, T, tr, **OPTS)
        assert ((x >= -1e-12) & (x <= 1 + 1e-12)).all()
        for l in range(2):
            for r in range(R):
                same_record(rec[l][r], x[l, r], fun[l, r], jac[l, r], info[l, r], (NETS[k], tr, R, l, r))
    # the reported value / gradient are the kernel's f/g at the reported x
    for l in range(2):
        v, g = fg_of(desc, th[l:l + 1], T, tr)(x[l])
        np.testing.assert_array_equal(v.astype(np.float64), fun[l])
        np.testing.assert_array_equal(g, jac[l])
    # SciPy's own state machines on the same f/g: printed, not asserted
    n_same, dfun = 0, []
    for l in range(2):
        ref = lockstep.minimize_lockstep(fg_of(desc, th[l:l + 1], T, tr), X0[l], bounds=Bounds(lo, hi), **OPTS)
        for r, s in enumerate(ref):
            dfun.append(abs(s.fun - fun[l, r]))
            n_same += ((s.nit, s.nfev, s.status) == tuple(info[l, r, :3]) and np.allclose(s.x, x[l, r], atol=1e-7))
    print(f"\n[lstm streamed lbfgsb vs scipy, {NETS[k]} {tr}] identical records {n_same}/{2 * R_MAX}; "
          f"|dfun| median {np.median(dfun):.1e}; nit max {info[:, :, 0].max()}")


@pytest.mark.parametrize("k", [1, 2])
def test_geometry_does_not_change_bits(gpu, k):
    D, T = NETS[k][0], NETS[k][4]
    rs, desc, th = make(k, 2, 100 + k)
    X0 = rs.uniform(-0.1, 1.1, size=(2, R_MAX, D))
    lo, hi = np.zeros(D), np.ones(D)
    both = run(desc, th, X0, lo, hi, T, "sigmoid", **OPTS)
    again = run(desc, th, X0, lo, hi, T, "sigmoid", **OPTS)
    for a, b in zip(both, again):                              # two runs
        np.testing.assert_array_equal(a, b)
    for l in range(2):                                         # a model alone
        alone = run(desc, th[l:l + 1], X0[l:l + 1], lo, hi, T, "sigmoid", **OPTS)
        for a, b in zip(both, alone):
            np.testing.assert_array_equal(a[l], b[0])
    first = run(desc, th, X0[:, :4], lo, hi, T, "sigmoid", **OPTS)   # nine starts in one call = 4 + 5
    rest = run(desc, th, np.ascontiguousarray(X0[:, 4:]), lo, hi, T, "sigmoid", **OPTS)
    for a, b, c in zip(both, first, rest):
        np.testing.assert_array_equal(a, np.concatenate([b, c], axis=1))


def value_grad_tile_floats(D, L, Hn, T):
    """bore_lstm_stream_value_and_input_grad's workspace of one 64-row tile (every region rounded up to 4 floats):
    per cell [x | h | 1] of every step, the head's [h | 1], gates and c of every step, mask, logits and their deltas,
    then one step's gate deltas, dh and dc per cell, the delta handed down and dx."""
    r4 = lambda n: (n + 3) & ~3                                                    # noqa: E731
    s = sum(r4(T * 64 * ((Hn if l else D) + Hn + 1)) for l in range(L))
    s += r4(T * 64 * (Hn + 1)) + r4(L * T * 64 * 4 * Hn) + r4(L * T * 64 * Hn) + 3 * r4(T * 64)
    return s + r4(64 * 4 * Hn) + 2 * r4(L * 64 * Hn) + r4(64 * Hn) + r4(64 * D)


def test_a_wave_takes_a_second_problem(gpu):
    """More groups of restarts than the call's workspace has tiles for: the grid shrinks and a workgroup walks several
    groups, i.e. a wave that finishes a problem re-zeroes its slot and starts its next one in the middle of the
    kernel.  The largest workspace within the streamed bounds is 64->4x64 over 16 steps: 1 966 080 floats of tile
    plus 8 D + 4 for the points and values (include/bore_hip.h), so two models have 64 MiB for 4 workgroups each and 18
    restarts are 5 groups of four -- workgroup 0 takes a second group, restarts 16 and 17.  One call of 18 against
    calls of 16 + 2.  Four iterations per problem: taking the next problem does not depend on how long the one before
    ran, a pass of this network is the most expensive there is, and the other tests run their problems to the end."""
    opts = dict(maxiter=4, ftol=1e-9)
    shape = (64, 4, 64, "elu", 16)
    D, L, Hn, act, T = shape
    tile = value_grad_tile_floats(D, L, Hn, T)
    per_wg = tile + 8 * D + 4
    wgs = (64 << 20) // (2 * per_wg * 4)                      # per model, of two
    assert tile == 1966080 and wgs == 4
    R = 4 * wgs + 2
    assert (R + 3) // 4 > wgs and R <= 64
    rs, desc, th = make(shape, 2, 11)
    X0 = rs.uniform(-0.1, 1.1, size=(2, R, D))
    lo, hi = np.zeros(D), np.ones(D)
    whole = run(desc, th, X0, lo, hi, T, "sigmoid", **opts)
    first = run(desc, th, np.ascontiguousarray(X0[:, :4 * wgs]), lo, hi, T, "sigmoid", **opts)
    rest = run(desc, th, np.ascontiguousarray(X0[:, 4 * wgs:]), lo, hi, T, "sigmoid", **opts)
    for a, b, c in zip(whole, first, rest):
        np.testing.assert_array_equal(a, np.concatenate([b, c], axis=1))
    x, fun, jac, info = whole
    assert (info[:, :, 1] >= 1).all() and info[:, 4 * wgs:, 0].max() >= 1      # (every record written; the late ones moved)
    for l, r in ((0, 0), (1, 1), (0, 16), (1, 16), (1, 17)):                    # first and second problems of the same waves
        same_record(host(desc, th[l:l + 1], T, "sigmoid", X0[l, r], lo, hi, **opts), x[l, r], fun[l, r], jac[l, r],
                    info[l, r], (l, r))


def test_limits_and_open_bounds(gpu):
    from bore_amd import ops
    D, L, Hn, act, T = NETS[1]
    rs, desc, th = make(1, 1, 0)
    X0 = rs.uniform(size=(1, 6, D))
    X0[0, 0, 0] = 0.0                                          # starts exactly on a bound
    X0[0, 1, 1] = 1.0
    X0[0, 2] = [1.0, 1.0, 0.0, 0.3, 0.0]
    lo, hi = [0, -np.inf, 0, -np.inf, 0], [1, 1, np.inf, np.inf, 1]
    for kw in (dict(maxiter=1), dict(maxiter=2), dict(maxfun=3), dict(maxls=2), dict(maxcor=2), dict()):
        x, fun, jac, info = (t[0] for t in run(desc, th, X0, lo, hi, T, "sigmoid", **kw))
        for r in range(6):
            same_record(host(desc, th, T, "sigmoid", X0[0, r], lo, hi, **kw), x[r], fun[r], jac[r], info[r], (kw, r))
        if "maxiter" in kw:
            assert (info[:, 2] == 1).all() and (info[:, 0] == kw["maxiter"]).all() and (info[:, 4] == 504).all()
        if "maxfun" in kw:                                     # (checked once per iteration: a line search may pass it)
            assert (info[:, 2] == 1).all() and (info[:, 1] >= 3).all() and (info[:, 1] <= 3 + 20).all()
    with pytest.raises(RuntimeError, match="lower bounds"):
        ops.lstm_stream_lbfgsb_minimize(desc, th, _dev(X0, np.float64), [1, 0, 0, 0, 0], [0, 1, 1, 1, 1], T)


@pytest.mark.parametrize("Ns", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("k", [1, 2])
def test_screening(gpu, k, Ns):
    from bore_amd import ops
    D, T = NETS[k][0], NETS[k][4]
    rs, desc, th = make(k, 2, 7 * Ns + k)
    X = rs.uniform(size=(2, Ns, D))
    if Ns >= 63:                                               # duplicated rows: equal predictions, the lower row wins
        X[:, 40] = X[:, 3]
        X[0, 60] = X[0, 3]
    # want[l][m]: model l on the candidates of model m
    want = [[ops.lstm_stream_forward(desc, th[l:l + 1], _dev(X[m].astype(np.float32))[None], num_steps=T).cpu().numpy()[0]
             for m in range(2)] for l in range(2)]
    for R in sorted({min(r, Ns) for r in (1, 5, 17, Ns)}):     # 17 and beyond: the sort branch
        for shared in (False, True):
            Xc = X[0] if shared else X
            x0, idx, pred = (t.cpu().numpy()
                             for t in ops.lstm_stream_screen_topk(desc, th, _dev(Xc, np.float64), R, T, want_pred=True))
            for l in range(2):
                Xl = X[0] if shared else X[l]
                np.testing.assert_array_equal(pred[l], want[l][0 if shared else l])
                order = np.lexsort((np.arange(Ns), -pred[l]))[:R]      # descending prediction, ties to the lower row
                np.testing.assert_array_equal(idx[l], order)
                np.testing.assert_array_equal(x0[l], Xl[idx[l]])
                # the reference's set, np.argpartition on -pred (the same values where a tie straddles the cut)
                part = np.argpartition(-pred[l], R - 1)[:R]
                np.testing.assert_array_equal(np.sort(pred[l][part]), np.sort(pred[l][order]))
                cut = np.sort(-pred[l])
                if R == Ns or cut[R - 1] < cut[R]:                     # no tie across the cut: the very same rows
                    assert set(part) == set(idx[l])
            x0n, idxn = ops.lstm_stream_screen_topk(desc, th, _dev(Xc, np.float64), R, T)   # no buffer of the caller's
            np.testing.assert_array_equal(idxn.cpu().numpy(), idx)
            np.testing.assert_array_equal(x0n.cpu().numpy(), x0)


def test_refusals_reach_python_by_name(gpu):
    from bore_amd import _lib, ops
    rs, desc, th = make((65, 1, 8, "elu", 2), 1, 0)
    with pytest.raises(_lib.UnsupportedError, match="BORE_DIM_MAX"):
        ops.lstm_stream_screen_topk(desc, th, _dev(rs.uniform(size=(8, 65)), np.float64), 2, 2)
    with pytest.raises(_lib.UnsupportedError, match="BORE_DIM_MAX"):
        ops.lstm_stream_lbfgsb_minimize(desc, th, _dev(np.full((1, 2, 65), 0.5), np.float64), np.zeros(65), np.ones(65), 2)


# ---- the public surface --------------------------------------------------------------------------------------------
COUNTED = ("lstm_stream_screen_topk", "lstm_stream_lbfgsb_minimize", "lstm_value_and_input_grad",
           "lstm_stream_value_and_input_grad")


def counted(monkeypatch):
    from bore_amd import ops
    calls = {name: 0 for name in COUNTED}

    def wrap(name, real):
        def wrapper(*args, **kwargs):
            calls[name] += 1
            return real(*args, **kwargs)
        return wrapper
    for name in COUNTED:
        monkeypatch.setattr(ops, name, wrap(name, getattr(ops, name)))
    return calls


def fitted_factory(D, seed=3):
    from bore_amd.layers import BinaryCrossentropy
    from bore_amd.models import StackedRecurrentFactory
    rs = np.random.RandomState(seed)
    factory = StackedRecurrentFactory(input_dim=D, output_dim=1, num_layers=2, num_units=32,
                                      layer_kws=dict(activation="elu"), seed=seed)
    net = factory.build_many_to_many()
    net.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True))
    net.fit(rs.uniform(size=(64, 5, D)), rs.randint(2, size=(64, 5, 1)), epochs=10, batch_size=16)
    return factory


def test_model_api_takes_the_device_route_only_when_asked(gpu, monkeypatch):
    from bore_amd import mixins, ops
    D, T = 48, 5
    factory = fitted_factory(D)
    assert ops.lstm_streamed(factory._desc, T) == 1            # (both routes on the same f/g flavour)
    bounds = Bounds(lb=np.zeros(D), ub=np.ones(D))
    kw = dict(num_starts=3, num_samples=64, print_fn=lambda s: None)
    calls = counted(monkeypatch)
    # the default-built network: the route it had, and the starts it hands to the restarts
    starts = []
    real_lockstep = mixins.lockstep.minimize_lockstep

    def spy(func, X0, **kwargs):
        starts.append(np.array(X0))
        return real_lockstep(func, X0, **kwargs)
    monkeypatch.setattr(mixins.lockstep, "minimize_lockstep", spy)
    default = factory.build_one_to_one(T, transform="sigmoid")
    assert (default.restart_mode, default.screen_mode) == ("lockstep", "host")
    ref = default.maxima(bounds, random_state=np.random.RandomState(7), **kw)
    assert calls["lstm_stream_screen_topk"] == 0 and calls["lstm_stream_lbfgsb_minimize"] == 0
    assert calls["lstm_stream_value_and_input_grad"] >= 1 and len(starts) == 1 and len(ref) == 3
    # asked for: one screening call, one restart call, no f/g launch of either flavour
    for name in COUNTED:
        calls[name] = 0
    net = factory.build_one_to_one(T, transform="sigmoid", acquisition="device")
    assert (net.restart_mode, net.screen_mode) == ("device", "device")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        results = net.maxima(bounds, random_state=np.random.RandomState(7), **kw)
    assert calls == {"lstm_stream_screen_topk": 1, "lstm_stream_lbfgsb_minimize": 1, "lstm_value_and_input_grad": 0,
                     "lstm_stream_value_and_input_grad": 0}, calls
    assert len(starts) == 1 and len(results) == 3
    # the default route's starts in the default route's order, each optimised as the host build optimises it
    for r, res in enumerate(results):
        h = host(factory._desc, factory.theta, T, "sigmoid", starts[0][r], np.zeros(D), np.ones(D), **OPTS)
        np.testing.assert_array_equal(res.x, h.x)
        np.testing.assert_array_equal(res.jac, h.jac)
        assert res.fun == h.fun and (res.nit, res.nfev, res.status) == (h.nit, h.nfev, h.status)
    best = net.argmax(bounds, random_state=np.random.RandomState(7), **kw)
    assert best is not None and np.all(best.x >= 0.0) and np.all(best.x <= 1.0)
    # a callable transform: asked for the device, told why not, and served by the default route
    for name in COUNTED:
        calls[name] = 0
    other = factory.build_one_to_one(T, transform=lambda u: u, acquisition="device")
    with pytest.warns(RuntimeWarning, match="callable transform"):
        assert len(other.maxima(bounds, random_state=np.random.RandomState(7), **kw)) == 3
    assert calls["lstm_stream_screen_topk"] == 0 and calls["lstm_stream_lbfgsb_minimize"] == 0
    assert calls["lstm_stream_value_and_input_grad"] >= 1
    with pytest.warns(RuntimeWarning, match="L-BFGS-B only"):
        assert len(net.maxima(bounds, method="SLSQP", random_state=np.random.RandomState(7), **kw)) == 3
    with pytest.raises(ValueError, match="acquisition"):
        factory.build_one_to_one(T, acquisition="gpu")


def test_a_network_that_fits_lds_runs_the_device_route_on_the_streamed_flavour(gpu, monkeypatch):
    from bore_amd import ops
    D, T = 16, 5
    factory = fitted_factory(D, seed=5)
    assert ops.lstm_streamed(factory._desc, T) == 0            # (predict: the LDS kernels; the device route: streamed)
    calls = counted(monkeypatch)
    net = factory.build_one_to_one(T, acquisition="device")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        results = net.maxima(Bounds(lb=np.zeros(D), ub=np.ones(D)), num_starts=3, num_samples=64,
                             print_fn=lambda s: None, random_state=np.random.RandomState(7))
    assert calls["lstm_stream_screen_topk"] == 1 and calls["lstm_stream_lbfgsb_minimize"] == 1
    assert calls["lstm_value_and_input_grad"] == 0 and calls["lstm_stream_value_and_input_grad"] == 0
    for res in results:
        assert np.all(res.x >= 0.0) and np.all(res.x <= 1.0)
        np.testing.assert_allclose(res.fun, -float(net.predict(res.x[None])[0, 0]), **VAL_TOL)


def test_what_the_kernels_refuse_warns_and_takes_the_default_route(gpu, monkeypatch):
    from bore_amd.models import StackedRecurrentFactory
    calls = counted(monkeypatch)
    kw = dict(num_starts=2, print_fn=lambda s: None)
    # more candidates than the selection ranks: the screening on the host, the restarts on the device all the same
    D, T = 48, 2
    net = StackedRecurrentFactory(input_dim=D, output_dim=1, layer_kws=dict(activation="elu"),
                                  seed=1).build_one_to_one(T, acquisition="device")
    with pytest.warns(RuntimeWarning, match="BORE_STREAM_MAX_SAMPLES"):
        res = net.maxima(Bounds(lb=np.zeros(D), ub=np.ones(D)), num_samples=16385, options=dict(maxiter=2),
                         random_state=np.random.RandomState(1), **kw)
    assert len(res) == 2 and calls["lstm_stream_lbfgsb_minimize"] == 1 and calls["lstm_stream_value_and_input_grad"] == 0
    # more than 64 inputs: neither kernel takes it, the lock-step route does
    for name in COUNTED:
        calls[name] = 0
    D = 65
    net = StackedRecurrentFactory(input_dim=D, output_dim=1, layer_kws=dict(activation="elu"),
                                  seed=1).build_one_to_one(T, acquisition="device")
    with pytest.warns(RuntimeWarning, match="BORE_DIM_MAX"):
        res = net.maxima(Bounds(lb=np.zeros(D), ub=np.ones(D)), num_samples=64, options=dict(maxiter=2),
                         random_state=np.random.RandomState(1), **kw)
    assert len(res) == 2 and calls["lstm_stream_value_and_input_grad"] >= 1


def test_bore_hyperband_passes_the_route_on(gpu, monkeypatch):
    from bore_amd.plugins import BOREHyperband, UniformFloat
    from bore_amd.plugins.types import DenseSpace
    calls = counted(monkeypatch)
    space = DenseSpace([UniformFloat("a", 0.0, 1.0), UniformFloat("b", -1.0, 1.0)])
    hb = BOREHyperband(space, eta=3, min_budget=1 / 9, max_budget=1, num_random_init=4, random_rate=None,
                       num_starts=2, num_samples=64, num_steps_per_iter=20, seed=0, acquisition="device")
    cg = hb.config_generator
    assert cg.acquisition == "device"

    class Job:
        def __init__(self, cfg, b, loss):
            self.kwargs, self.result, self.exception, self.id = dict(config=cfg, budget=b), dict(loss=loss), None, 0

    rs = np.random.RandomState(0)
    for _ in range(6):
        cfg, _info = cg.get_config(1 / 9)
        x = space.to_array(cfg)
        assert np.all(x >= 0.0) and np.all(x <= 1.0)
        cg.new_result(Job(cfg, 1 / 9, float(rs.uniform())))
    assert cg.funcs and all(f.restart_mode == "device" and f.screen_mode == "device" for f in cg.funcs.values())
    assert calls["lstm_stream_screen_topk"] >= 1 and calls["lstm_stream_lbfgsb_minimize"] >= 1
    assert calls["lstm_value_and_input_grad"] == 0 and calls["lstm_stream_value_and_input_grad"] == 0
    assert BOREHyperband(space, seed=0).config_generator.acquisition == "lockstep"
