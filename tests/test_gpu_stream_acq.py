"""Screening and L-BFGS-B restarts on the streamed kernels (bore_stream_screen_topk,
bore_stream_sample_screen_topk, bore_stream_lbfgsb_minimize): networks too large for one workgroup's
LDS, and small ones, which these entry points stream as well (odd input dimensions, ragged widths).

The bar for the restarts is the project's standing one for every form of the optimiser: every record
equals the HOST build of lbfgsb.h fed the f and g of ops.mlp_value_and_input_grad -- the streamed
kernels' (BORE_STREAM=1 around that call for the small networks) -- bit for bit, no tolerance.
SciPy's result on the same f/g is printed, not asserted (tests/test_lbfgsb_host.py pins the host
build to SciPy)."""
import os
import warnings

import numpy as np
import pytest
import torch
from scipy.optimize import Bounds

import lbfgsb_host as H
from bore_amd import _lib, ops
from bore_amd.optimizers import lockstep
from test_gpu_stream import branin01, dev, pack, rand_model

pytestmark = pytest.mark.gpu

# (D, units, activations, fits LDS): the small ones are streamed by the new entry points all the same
SMALL = [(1, [1], ["sigmoid"], True),
         (5, [7, 3, 1], ["tanh", "sigmoid", "linear"], True),
         (2, [16, 16, 1], ["relu", "relu", "sigmoid"], True)]
LARGE = [(8, [256, 256, 1], ["relu", "elu", "linear"], False),
         (16, [128, 128, 128, 1], ["elu", "elu", "elu", "linear"], False)]
NETS = SMALL + LARGE
OPTS = dict(maxiter=1000, ftol=1e-9)
R_MAX = 9


class streamed_route:
    """The f/g and forward calls inside run the streamed kernels: natively, or (a network that fits LDS) by the switch."""

    def __init__(self, small):
        self.small = small

    def __enter__(self):
        self.old = os.environ.get("BORE_STREAM")
        if self.small:
            os.environ["BORE_STREAM"] = "1"
        else:
            os.environ.pop("BORE_STREAM", None)

    def __exit__(self, *exc):
        os.environ.pop("BORE_STREAM", None)
        if self.old is not None:
            os.environ["BORE_STREAM"] = self.old


def make(D, units, acts, L, seed):
    rs = np.random.RandomState(seed)
    desc = _lib.make_desc(D, units, acts)
    th = dev(np.stack([pack(rand_model(rs, D, units)) for _ in range(L)]))
    return rs, desc, th


def fg_of(desc, th_l, tr, small):
    def fg(xx):
        with streamed_route(small):
            v, g = ops.mlp_value_and_input_grad(desc, th_l, dev(np.atleast_2d(xx)[None]), tr, True)
        return v.cpu().numpy()[0], g.cpu().numpy()[0]
    return fg


def run(desc, th, X0, lo, hi, tr, **opts):
    return ops.lbfgsb_results_to_host(*ops.stream_lbfgsb_minimize(desc, th, dev(X0), lo, hi, tr, True, **opts))


def same_record(h, x, fun, jac, info, where):
    np.testing.assert_array_equal(h.x, x, err_msg=str(where))
    assert h.fun == fun, where
    np.testing.assert_array_equal(h.jac, jac, err_msg=str(where))
    assert (h.nit, h.nfev, h.status) == tuple(info[:3]), where
    assert h.task == tuple(info[3:]), where


_reference = {}


def reference(k, tr):
    """Network k with two models, nine starts each from U(-0.1, 1.1) -- some outside the box [0, 1]^D -- and the host
    build's record of every start.  Computed once per (network, transform); nobody writes to it."""
    if (k, tr) not in _reference:
        D, units, acts, small = NETS[k]
        rs, desc, th = make(D, units, acts, 2, 100 + k)
        X0 = rs.uniform(-0.1, 1.1, size=(2, R_MAX, D))
        lo, hi = np.zeros(D), np.ones(D)
        host = [[H.minimize(lambda xx, f=fg_of(desc, th[l:l + 1], tr, small): tuple(a[0] for a in f(xx)),
                            X0[l, r], (lo, hi), **OPTS) for r in range(R_MAX)] for l in range(2)]
        _reference[(k, tr)] = (desc, th, X0, lo, hi, host)
    return _reference[(k, tr)]


@pytest.mark.parametrize("tr", ["identity", "sigmoid"])
@pytest.mark.parametrize("k", range(len(NETS)))
def test_restarts_equal_the_host_build_bit_for_bit(gpu, k, tr):
    D, units, acts, small = NETS[k]
    desc, th, X0, lo, hi, host = reference(k, tr)
    for R in (1, 3, 4, 5, 9):       # 1: three waves idle; 5, 9: a second group with one problem (a wave's second problem: below)
        x, fun, jac, info = run(desc, th, X0[:, :R], lo, hi, tr, **OPTS)
        assert ((x >= -1e-12) & (x <= 1 + 1e-12)).all()
        for l in range(2):
            for r in range(R):
                same_record(host[l][r], x[l, r], fun[l, r], jac[l, r], info[l, r], (units, tr, R, l, r))
    # the reported value / gradient are the kernel's f/g at the reported x
    for l in range(2):
        v, g = fg_of(desc, th[l:l + 1], tr, small)(x[l])
        np.testing.assert_array_equal(v.astype(np.float64), fun[l])
        np.testing.assert_array_equal(g, jac[l])
    # SciPy's own state machines on the same f/g: printed, not asserted
    n_same, dfun = 0, []
    for l in range(2):
        ref = lockstep.minimize_lockstep(fg_of(desc, th[l:l + 1], tr, small), X0[l], bounds=Bounds(lo, hi), **OPTS)
        for r, s in enumerate(ref):
            dfun.append(abs(s.fun - fun[l, r]))
            n_same += ((s.nit, s.nfev, s.status) == tuple(info[l, r, :3]) and np.allclose(s.x, x[l, r], atol=1e-7))
    print(f"\n[streamed lbfgsb vs scipy, {D}->{units} {tr}] identical records {n_same}/{2 * R_MAX}; "
          f"|dfun| median {np.median(dfun):.1e}")


@pytest.mark.parametrize("k", [1, 3])
def test_geometry_does_not_change_bits(gpu, k):
    D, units, acts, small = NETS[k]
    rs, desc, th = make(D, units, acts, 2, 100 + k)
    X0 = rs.uniform(-0.1, 1.1, size=(2, R_MAX, D))
    lo, hi = np.zeros(D), np.ones(D)
    both = run(desc, th, X0, lo, hi, "sigmoid", **OPTS)
    again = run(desc, th, X0, lo, hi, "sigmoid", **OPTS)
    for a, b in zip(both, again):                              # two runs
        np.testing.assert_array_equal(a, b)
    for l in range(2):                                         # a model alone
        alone = run(desc, th[l:l + 1], X0[l:l + 1], lo, hi, "sigmoid", **OPTS)
        for a, b in zip(both, alone):
            np.testing.assert_array_equal(a[l], b[0])
    first = run(desc, th, X0[:, :4], lo, hi, "sigmoid", **OPTS)   # nine starts in one call = 4 + 5
    rest = run(desc, th, np.ascontiguousarray(X0[:, 4:]), lo, hi, "sigmoid", **OPTS)
    for a, b, c in zip(both, first, rest):
        np.testing.assert_array_equal(a, np.concatenate([b, c], axis=1))


def test_a_wave_takes_a_second_problem(gpu):
    """More groups of restarts than the call's workspace has tiles for: the grid shrinks and a workgroup walks several
    groups, i.e. a wave that finishes a problem re-zeroes its slot and starts its next one in the middle of the
    kernel.  8->256-256-1 takes 2 x 64 x 521 floats of workspace per workgroup, so two models have 64 MiB for 125
    workgroups each: 505 restarts are 127 groups of four -- workgroups 0 and 1 take a second group, restarts 500..503
    and 504 -- while 500 restarts are 125 groups, one per workgroup.  One call of 505 against calls of 500 + 5."""
    D, units, acts, small = NETS[3]
    rs, desc, th = make(D, units, acts, 2, 11)
    R = 505
    assert 2 * 125 * (2 * 64 * (D + sum(units)) * 4) <= (64 << 20) < 2 * 126 * (2 * 64 * (D + sum(units)) * 4)
    X0 = rs.uniform(-0.1, 1.1, size=(2, R, D))
    lo, hi = np.zeros(D), np.ones(D)
    whole = run(desc, th, X0, lo, hi, "sigmoid", **OPTS)
    first = run(desc, th, np.ascontiguousarray(X0[:, :500]), lo, hi, "sigmoid", **OPTS)
    rest = run(desc, th, np.ascontiguousarray(X0[:, 500:]), lo, hi, "sigmoid", **OPTS)
    for a, b, c in zip(whole, first, rest):
        np.testing.assert_array_equal(a, np.concatenate([b, c], axis=1))
    x, fun, jac, info = whole
    assert (info[:, :, 1] >= 1).all() and info[:, 500:, 0].max() >= 1      # (every record written; the late ones moved)
    for l, r in ((0, 0), (1, 4), (0, 500), (1, 503), (1, 504)):           # first and second problems of the same waves
        h = H.minimize(lambda xx, f=fg_of(desc, th[l:l + 1], "sigmoid", small): tuple(a[0] for a in f(xx)),
                       X0[l, r], (lo, hi), **OPTS)
        same_record(h, x[l, r], fun[l, r], jac[l, r], info[l, r], (l, r))


def test_limits_and_open_bounds(gpu):
    D, units, acts = 4, [16, 1], ["tanh", "linear"]
    rs, desc, th = make(D, units, acts, 1, 0)
    X0 = rs.uniform(size=(1, 6, D))
    X0[0, 0, 0] = 0.0                                          # starts exactly on a bound
    X0[0, 1, 1] = 1.0
    X0[0, 2] = [1.0, 1.0, 0.0, 0.3]
    lo, hi = [0, -np.inf, 0, -np.inf], [1, 1, np.inf, np.inf]
    fg = fg_of(desc, th, "sigmoid", True)
    for kw in (dict(maxiter=1), dict(maxiter=2), dict(maxfun=3), dict(maxls=2), dict(maxcor=2), dict()):
        x, fun, jac, info = (t[0] for t in run(desc, th, X0, lo, hi, "sigmoid", **kw))
        for r in range(6):
            h = H.minimize(lambda xx: tuple(a[0] for a in fg(xx)), X0[0, r], (np.array(lo, float), np.array(hi, float)),
                           **kw)
            same_record(h, x[r], fun[r], jac[r], info[r], (kw, r))
        if "maxiter" in kw:
            assert (info[:, 2] == 1).all() and (info[:, 0] == kw["maxiter"]).all() and (info[:, 4] == 504).all()
        if "maxfun" in kw:                                     # (checked once per iteration: a line search may pass it)
            assert (info[:, 2] == 1).all() and (info[:, 1] >= 3).all() and (info[:, 1] <= 3 + 20).all()
    with pytest.raises(RuntimeError, match="lower bounds"):
        ops.stream_lbfgsb_minimize(desc, th, dev(X0), [1, 0, 0, 0], [0, 1, 1, 1])


@pytest.mark.parametrize("Ns", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("k", [1, 3])
def test_screening(gpu, k, Ns):
    D, units, acts, small = NETS[k]
    rs, desc, th = make(D, units, acts, 2, 7 * Ns + k)
    X = rs.uniform(size=(2, Ns, D))
    if Ns >= 63:                                               # duplicated rows: equal predictions, the lower row wins
        X[:, 40] = X[:, 3]
        X[0, 60] = X[0, 3]
    with streamed_route(small):      # want[l][m]: model l on the candidates of model m
        want = [[ops.mlp_forward(desc, th[l:l + 1], dev(X[m].astype(np.float32))).cpu().numpy()[0] for m in range(2)]
                for l in range(2)]
    for R in sorted({min(r, Ns) for r in (1, 5, 17, Ns)}):     # 17 and beyond: the sort branch
        for shared in (False, True):
            Xc = X[0] if shared else X
            x0, idx, pred = (t.cpu().numpy() for t in ops.stream_screen_topk(desc, th, dev(Xc), R, want_pred=True))
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
            x0n, idxn = ops.stream_screen_topk(desc, th, dev(Xc), R)   # without a prediction buffer of the caller's
            np.testing.assert_array_equal(idxn.cpu().numpy(), idx)
            np.testing.assert_array_equal(x0n.cpu().numpy(), x0)


@pytest.mark.parametrize("k,Ns,R", [(1, 77, 5), (3, 1000, 17), (4, 64, 64)])
def test_sampled_screening_equals_the_two_launches(gpu, k, Ns, R):
    D, units, acts, small = NETS[k]
    rs, desc, th = make(D, units, acts, 3, k)
    lo, hi = rs.uniform(-2, 0, size=D), rs.uniform(0.5, 3, size=D)
    Xc = ops.uniform_candidates(91, 3, Ns, lo, hi, model_index0=7, draw_index=4)
    a = ops.stream_screen_topk(desc, th, Xc, R, want_pred=True)
    b = ops.stream_sample_screen_topk(desc, th, 91, Ns, lo, hi, R, model_index0=7, draw_index=4, want_pred=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_sampled_screening_refuses_more_than_64_inputs(gpu):
    D, units = 65, [256, 256, 1]
    rs, desc, th = make(D, units, ["relu", "relu", "linear"], 1, 0)
    assert ops.mlp_streamed(desc) == 7
    with pytest.raises(_lib.UnsupportedError, match="BORE_DIM_MAX"):
        ops.stream_sample_screen_topk(desc, th, 1, 64, np.zeros(D), np.ones(D), 3)
    with pytest.raises(_lib.UnsupportedError, match="BORE_DIM_MAX"):
        ops.stream_lbfgsb_minimize(desc, th, dev(np.full((1, 2, D), 0.5)), np.zeros(D), np.ones(D))
    x0, idx = ops.stream_screen_topk(desc, th, dev(rs.uniform(size=(64, D))), 3)      # (rows in memory: any D)
    assert idx.shape == (1, 3)


# ---- the public surface --------------------------------------------------------------------------------------------
def counted(monkeypatch):
    calls = []
    real = ops.stream_lbfgsb_minimize

    def wrapper(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)
    monkeypatch.setattr(ops, "stream_lbfgsb_minimize", wrapper)
    return calls, real


def test_model_api_takes_the_device_route(gpu, monkeypatch):
    from bore_amd.layers import BinaryCrossentropy, Dense
    from bore_amd.models import MaximizableSequential
    monkeypatch.delenv("BORE_STREAM", raising=False)
    rs = np.random.RandomState(0)
    X = rs.uniform(size=(40, 2))
    y = branin01(X)
    z = (y < np.quantile(y, 1 / 3)).astype(np.float64)

    def build(**kw):
        model = MaximizableSequential(seed=1, **kw)
        for u, a in ((256, "relu"), (256, "relu"), (1, "linear")):
            model.add(Dense(u, activation=a))
        model.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True), metrics=["accuracy"])
        model.fit(X, z, epochs=5, batch_size=64)
        return model

    model = build()
    assert ops.mlp_streamed(model._desc) == 7
    bounds = Bounds(lb=np.zeros(2), ub=np.ones(2))
    calls, real = counted(monkeypatch)
    kw = dict(num_starts=3, num_samples=64, print_fn=lambda s: None)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        results = model.maxima(bounds, random_state=np.random.RandomState(7), **kw)
    assert len(calls) == 1 and len(results) == 3
    # the op itself from the reference's starts, in the reference's order
    X_init = np.random.RandomState(7).uniform(low=np.zeros(2), high=np.ones(2), size=(64, 2))
    order = np.argpartition(-model.predict(X_init)[:, 0], kth=2, axis=None)[:3]
    x, fun, jac, info = (t[0] for t in ops.lbfgsb_results_to_host(
        *real(model._desc, model.theta, dev(X_init[order][None]), [0.0, 0.0], [1.0, 1.0], "identity", True,
              maxiter=1000, ftol=1e-9)))
    for r, res in enumerate(results):
        np.testing.assert_array_equal(res.x, x[r])
        np.testing.assert_array_equal(res.jac, jac[r])
        assert res.fun == fun[r] and (res.nit, res.nfev, res.status) == tuple(info[r, :3])
        np.testing.assert_allclose(res.fun, -float(model.predict(res.x[None])[0, 0]), rtol=2e-5, atol=2e-6)
    # the host routes stay what they were
    del calls[:]
    model.restart_mode = "lockstep"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        host = model.maxima(bounds, random_state=np.random.RandomState(7), **kw)
    assert len(calls) == 0 and len(host) == 3
    model.restart_mode, model.screen_mode = "device", "host"
    literal = model.maxima(bounds, random_state=np.random.RandomState(7), **kw)
    assert len(calls) == 1                                     # (host screening, device restarts)
    for a, b in zip(results, literal):
        np.testing.assert_array_equal(a.x, b.x)
    # a callable transform: the host route, no error and no warning
    del calls[:]
    other = build(transform=lambda u: u)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert len(other.maxima(bounds, random_state=np.random.RandomState(7), **kw)) == 3
    assert len(calls) == 0


def test_plugin_with_128_units_takes_the_device_route(gpu, monkeypatch):
    from bore_amd.plugins.classifier import ClassifierSuggester
    monkeypatch.delenv("BORE_STREAM", raising=False)
    calls, _ = counted(monkeypatch)
    bounds = Bounds(lb=np.zeros(3), ub=np.ones(3))
    sug = ClassifierSuggester(bounds, num_units=128, num_layers=2, num_random_init=4, num_steps_per_iter=20,
                              num_starts=2, num_samples=64, seed=0)
    sources = []
    for _ in range(4 + 3):
        x, info = sug.suggest()
        assert x.shape == (3,) and np.all(x >= 0.0) and np.all(x <= 1.0)
        sources.append(info["source"])
        sug.observe(x, float(np.sum((x - 0.3) ** 2)))
    assert "model" in sources, sources
    assert ops.mlp_streamed(sug.logit._desc) == 7
    assert len(calls) >= 1
