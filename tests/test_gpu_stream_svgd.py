"""SVGD batch acquisition on the streamed kernels (bore_stream_svgd_optimize): networks too large for one
workgroup's LDS, and small ones, which the entry point streams as well (odd input dimensions, ragged widths).

The bar is the project's standing one for the device SVGD (tests/test_svgd.py): the particles of the host statement
(bore_amd/optimizers/svgd.py) driven by ops.mlp_value_and_input_grad -- the streamed kernels' (BORE_STREAM=1 around
that call for the small networks) -- to 1e-9 with a constant distortion, 1e-6 with ranks in the weights (a near-tie
can flip one)."""
import warnings

import numpy as np
import pytest
from scipy.optimize import Bounds

from bore_amd import _lib, ops
from bore_amd.optimizers.svgd import SVGD, DistortionConstant, DistortionExpDecay, RadialBasis
from test_gpu_stream import dev
from test_gpu_stream_acq import make, streamed_route

pytestmark = pytest.mark.gpu

# (D, units, activations, fits LDS)
NETS = {"5-7-3-1": (5, [7, 3, 1], ["tanh", "sigmoid", "linear"], True),
        "2-16-16-1": (2, [16, 16, 1], ["relu", "relu", "linear"], True),
        "8-256-256-1": (8, [256, 256, 1], ["relu", "elu", "linear"], False),
        "16-128x3-1": (16, [128, 128, 128, 1], ["elu", "elu", "elu", "linear"], False)}

# net, n, length_scale, lambd, transform, n_iter
CASES = [("5-7-3-1", 1, None, None, "identity", 200),       # a single particle: the median of one zero, the floor of h
         ("5-7-3-1", 8, None, None, "identity", 200),
         ("2-16-16-1", 63, 0.3, None, "sigmoid", 200),      # both sides of the 64-row chunk edge
         ("2-16-16-1", 64, None, None, "sigmoid", 200),
         ("2-16-16-1", 65, None, None, "exp", 60),
         ("2-16-16-1", 300, None, None, "sigmoid", 60),     # more particles than threads, five chunks, the last ragged
         ("8-256-256-1", 33, None, 0.5, "sigmoid", 200),
         ("16-128x3-1", 24, None, None, "sigmoid", 200),
         ("16-128x3-1", 130, 0.2, None, "sigmoid", 60)]     # three chunks


def host_fg(desc, th_l, tr, small):
    def func(X):
        with streamed_route(small):
            v, g = ops.mlp_value_and_input_grad(desc, th_l, dev(X[None]), tr, False)
        return v.cpu().numpy()[0].astype(np.float64), g.cpu().numpy()[0]
    return func


def host_svgd(ls, lambd, **kw):
    dist = DistortionConstant() if lambd is None else DistortionExpDecay(lambd=lambd)
    return SVGD(kernel=RadialBasis(length_scale=ls), distortion=dist, **kw)


def first_difference(desc, th_l, x0_l, lo, hi, tr, ls, lambd, kw, trajectory):
    """The first iteration after which device and host differ by more than 1e-12 (runs only when a case has failed)."""
    for k in range(1, len(trajectory) + 1):
        out = ops.stream_svgd_optimize(desc, th_l, dev(x0_l[None]), lo, hi, tr, length_scale=ls, lambd=lambd,
                                       **dict(kw, n_iter=k)).cpu().numpy()[0]
        d = np.abs(out - trajectory[k - 1]).max()
        if d > 1e-12:
            return k, d
    return None, 0.0


@pytest.mark.parametrize("net,n,ls,lambd,tr,n_iter", CASES)
def test_tracks_the_host_statement(gpu, net, n, ls, lambd, tr, n_iter):
    D, units, acts, small = NETS[net]
    L = 2
    rs, desc, th = make(D, units, acts, L, 31 * n + D)
    x0 = rs.uniform(size=(L, n, D))
    lo, hi = np.zeros(D), np.ones(D)
    kw = dict(n_iter=n_iter, step_size=1e-2, alpha=.9, eps=1e-6, tau=1.)
    out = ops.stream_svgd_optimize(desc, th, dev(x0), lo, hi, tr, length_scale=ls, lambd=lambd, **kw).cpu().numpy()
    assert out.shape == (L, n, D) and out.dtype == np.float64
    assert ((out >= 0) & (out <= 1)).all()
    assert (np.abs(out - x0) > 1e-4).any()                    # the particles moved
    tol = 1e-9 if lambd is None else 1e-6
    for l in range(L):
        trajectory = []
        ref = host_svgd(ls, lambd, **kw).optimize_from_init(host_fg(desc, th[l:l + 1], tr, small), x0[l],
                                                            bounds=[(0.0, 1.0)] * D,
                                                            callback=lambda x: trajectory.append(x.copy()))
        worst = np.abs(out[l] - ref).max()
        print(f"\n[streamed svgd vs host, {net} n={n} {tr} model {l}] max |device - host| = {worst:.2e} (bar {tol:.0e})")
        if not worst <= tol:
            k, d = first_difference(desc, th[l:l + 1], x0[l], lo, hi, tr, ls, lambd, kw, trajectory)
            pytest.fail(f"{net} n={n} model {l}: |device - host| = {worst:.3e} > {tol:.0e} after {n_iter} iterations; "
                        f"first difference above 1e-12 after iteration {k} ({d:.3e})")
    # no box: the same arithmetic without the clip
    free = ops.stream_svgd_optimize(desc, th, dev(x0), None, None, tr, length_scale=ls, lambd=lambd, n_iter=3,
                                    step_size=1e-2).cpu().numpy()
    assert np.isfinite(free).all()


@pytest.mark.parametrize("net,n", [("5-7-3-1", 8), ("16-128x3-1", 70)])
def test_bits_do_not_depend_on_geometry_or_on_the_run(gpu, net, n):
    D, units, acts, small = NETS[net]
    rs, desc, th = make(D, units, acts, 2, n)
    x0 = rs.uniform(size=(2, n, D))
    lo, hi = np.zeros(D), np.ones(D)
    kw = dict(n_iter=40, step_size=1e-2)

    def run(t, x, **over):
        return ops.stream_svgd_optimize(desc, t, dev(x), lo, hi, "sigmoid", **dict(kw, **over)).cpu().numpy()
    both = run(th, x0)
    np.testing.assert_array_equal(both, run(th, x0))                       # two runs
    for l in range(2):                                                     # a model alone
        np.testing.assert_array_equal(run(th[l:l + 1], x0[l:l + 1])[0], both[l])
    np.testing.assert_array_equal(run(th, x0, n_iter=0), x0)               # no iteration: x_init itself


def test_same_values_and_gradients_as_the_rows_kernel(gpu):
    """One iteration without repulsion and with a fixed length scale: the update is a function of f and its input
    gradient alone, so a wrong chunk offset into either shows (70 particles: a full chunk and a ragged one)."""
    D, units, acts, small = NETS["8-256-256-1"]
    n = 70
    rs, desc, th = make(D, units, acts, 2, 5)
    x0 = rs.uniform(size=(2, n, D))
    kw = dict(n_iter=1, step_size=1e-2, alpha=.9, eps=1e-6, tau=0.)
    out = ops.stream_svgd_optimize(desc, th, dev(x0), np.zeros(D), np.ones(D), "sigmoid", length_scale=0.5,
                                   **kw).cpu().numpy()
    for l in range(2):
        ref = host_svgd(0.5, None, **kw).optimize_from_init(host_fg(desc, th[l:l + 1], "sigmoid", small), x0[l],
                                                            bounds=[(0.0, 1.0)] * D)
        np.testing.assert_allclose(out[l], ref, rtol=0, atol=1e-9)
    assert (np.abs(out - x0) > 1e-4).any()


def test_model_api(gpu, monkeypatch):
    from bore_amd.layers import BinaryCrossentropy, Dense
    from bore_amd.models import BatchMaximizableSequential
    monkeypatch.delenv("BORE_STREAM", raising=False)
    D = 8
    rs = np.random.RandomState(0)
    X = rs.uniform(size=(64, D))
    y = np.sum((X - 0.3) ** 2, 1)
    z = y < np.quantile(y, 0.25)

    def build(transform):
        model = BatchMaximizableSequential(transform, seed=2)
        for u, a in ((256, "relu"), (256, "relu"), (1, None)):
            model.add(Dense(u, activation=a))
        model.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True))
        model.fit(X, z, epochs=5, batch_size=64)
        return model

    model = build("sigmoid")
    assert ops.mlp_streamed(model._desc) == 7
    calls = []
    real = ops.stream_svgd_optimize
    monkeypatch.setattr(ops, "stream_svgd_optimize", lambda *a, **k: calls.append(1) or real(*a, **k))
    bounds = Bounds(np.zeros(D), np.ones(D))
    kw = dict(n_iter=60, step_size=1e-2, random_state=5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        xa = model.argmax_batch(8, bounds, **kw)
        xb = model.argmax_batch(8, bounds, **kw)
    assert len(calls) == 2
    assert xa.shape == (8, D) and xa.dtype == np.float64 and np.array_equal(xa, xb)
    assert ((xa >= 0) & (xa <= 1)).all()
    model.svgd_mode = "host"
    host = model.argmax_batch(8, bounds, **kw)
    assert len(calls) == 2
    np.testing.assert_allclose(xa, host, rtol=0, atol=1e-9)
    # beyond the n^2 D up to which the kernel was measured no slower than the host driver: that driver, as before
    assert 80 * 80 * D > model.stream_svgd_max_work >= 64 * 64 * D
    model.svgd_mode = "device"
    with pytest.warns(RuntimeWarning, match="not faster than the host driver"):
        far = model.argmax_batch(80, bounds, n_iter=3, step_size=1e-2, random_state=5)
    assert len(calls) == 2 and far.shape == (80, D)
    model.stream_svgd_max_work = None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        np.testing.assert_allclose(model.argmax_batch(80, bounds, n_iter=3, step_size=1e-2, random_state=5), far,
                                   rtol=0, atol=1e-9)
    assert len(calls) == 3
    # a callable transform: the host driver, with the warning it always gave
    other = build(lambda u: u)
    with pytest.warns(RuntimeWarning, match="callable transform"):
        xc = other.argmax_batch(8, bounds, **kw)
    assert len(calls) == 3 and xc.shape == (8, D) and ((xc >= 0) & (xc <= 1)).all()   # (no further device call)
