"""Classifier ensembles on the device (bore_amd/csrc/bore_ensemble.hip): value + input gradient, screening and the
L-BFGS-B restarts over K members, the model layer and the plugin.

The checker is the numpy statement bore_amd.ensemble.ensemble_score over the float64 oracle's members, at the
project's own tolerances for value + gradient (tests/test_gpu_parity.py: val rtol 2e-5 / atol 2e-6, grad rtol 2e-4 /
atol 2e-5).  The statement divides by sigma, so the inputs are conditioned on the CPU first: min over the rows of
sqrt(var) >= 0.05 (independent random members have it; a seed that had not would be replaced, not the tolerance).
The restarts are held to the project's standing bar: every record equals the HOST build of lbfgsb.h fed
ops.ensemble_value_and_input_grad, bit for bit."""
import warnings

import numpy as np
import pytest
import torch
from scipy.optimize import Bounds

import lbfgsb_host as H
from bore_amd import _lib, ops
from bore_amd.ensemble import ensemble_score, ensemble_stats
from oracle import bore_oracle as O
from test_gpu_stream import dev, pack, rand_model

pytestmark = pytest.mark.gpu

# (D, units, activations, K): ragged widths; the narrow plugin-like shape; the plugin's network at the LDS end
NETS = [(3, [5, 7, 1], ["elu", "tanh", "linear"], 3),
        (2, [16, 16, 1], ["relu", "relu", "sigmoid"], 4),
        (16, [32, 32, 32, 1], ["elu", "elu", "elu", "linear"], 8)]
R = 131                       # 32 tiles of four rows and a tail of three
VAL_TOL = dict(rtol=2e-5, atol=2e-6)
GRAD_TOL = dict(rtol=2e-4, atol=2e-5)
_cases = {}


def case(k):
    """Net k: the members, the rows, the oracle's float64 F [K, R] and G [K, R, D].  Computed once; nobody writes."""
    if k not in _cases:
        D, units, acts, K = NETS[k]
        rs = np.random.RandomState(40)
        ps = [rand_model(rs, D, units) for _ in range(K)]
        X = rs.uniform(0, 1, size=(R, D))
        F = np.stack([O.predict(p, acts, X, dtype=np.float64)[:, 0] for p in ps])
        G = np.stack([-O.value_and_input_grad(p, acts, X, "identity", dtype=np.float64)[1] for p in ps])
        spread = np.sqrt(F.var(axis=0)).min()
        assert spread >= 0.05, f"net {k}: min sqrt(var) = {spread:.3g}: pick another seed"
        desc = _lib.make_desc(D, units, acts)
        theta = dev(np.stack([pack(p) for p in ps]))[None].contiguous()          # [1, K, P]
        _cases[k] = (desc, theta, ps, X, F, G)
    return _cases[k]


def fg(desc, theta, X, beta, transform="identity", negate=True):
    v, g = ops.ensemble_value_and_input_grad(desc, theta, dev(X), beta, transform, negate)
    assert v.dtype == torch.float32 and g.dtype == torch.float64
    return v.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("transform,negate", [("identity", True), ("sigmoid", True), ("exp", True), ("sigmoid", False)])
@pytest.mark.parametrize("beta", [0.0, 1.5])
@pytest.mark.parametrize("k", range(len(NETS)))
def test_value_and_grad_match_the_statement(gpu, k, beta, transform, negate):
    desc, theta, ps, X, F, G = case(k)
    want_v, want_g = ensemble_score(F, G, beta, transform, negate)
    val, grad = fg(desc, theta, X[None], beta, transform, negate)
    print(f"\n[ensemble f/g net {k} beta {beta} {transform} negate={negate}] max |dval| {np.abs(val[0] - want_v).max():.2e}"
          f", max |dgrad| {np.abs(grad[0] - want_g).max():.2e}")
    np.testing.assert_allclose(val[0], want_v, **VAL_TOL)
    np.testing.assert_allclose(grad[0], want_g, **GRAD_TOL)
    # a row alone: the bits it has in the batch (rows 5 and 130: the middle of a tile, the tail)
    for r in (5, 130):
        v1, g1 = fg(desc, theta, X[None, r:r + 1], beta, transform, negate)
        assert v1[0, 0] == val[0, r]
        np.testing.assert_array_equal(g1[0, 0], grad[0, r])


@pytest.mark.parametrize("k", range(len(NETS)))
def test_two_ensembles_in_one_call_equal_each_alone(gpu, k):
    desc, theta, ps, X, F, G = case(k)
    other = torch.flip(theta, dims=[1]) * 0.5                      # (another ensemble of the same shape)
    both = torch.cat([theta, other], dim=0).contiguous()
    XX = np.stack([X, X[::-1]])
    val, grad = fg(desc, both, XX, 1.5, "sigmoid")
    for e, th in enumerate((theta, other.contiguous())):
        v1, g1 = fg(desc, th, XX[e:e + 1], 1.5, "sigmoid")
        np.testing.assert_array_equal(v1[0], val[e])
        np.testing.assert_array_equal(g1[0], grad[e])


@pytest.mark.parametrize("transform", ["identity", "sigmoid"])
@pytest.mark.parametrize("k", range(len(NETS)))
def test_one_member_beta_zero_is_the_single_model_kernel(gpu, k, transform):
    desc, theta, ps, X, F, G = case(k)
    th1 = theta[:, :1].contiguous()
    val, grad = fg(desc, th1, X[None], 0.0, transform)
    v, g = ops.mlp_value_and_input_grad(desc, th1[0], dev(X[None]), transform, True)
    np.testing.assert_allclose(val, v.cpu().numpy(), **VAL_TOL)
    np.testing.assert_allclose(grad, g.cpu().numpy(), **GRAD_TOL)


# ---- screening ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ns,num_starts", [(1000, 5), (5, 5)])
@pytest.mark.parametrize("k", range(len(NETS)))
def test_screening(gpu, k, Ns, num_starts):
    desc, theta, ps, _, _, _ = case(k)
    D, units, acts, K = NETS[k]
    rs = np.random.RandomState(7 * Ns + k)
    X = rs.uniform(size=(Ns, D))
    if Ns >= 64:                                               # duplicated rows: equal scores, the lower row wins
        X[Ns - 1] = X[3]
        X[40] = X[3]
    beta = 1.5
    x0, idx, score = (t.cpu().numpy() for t in ops.ensemble_screen_topk(desc, theta, dev(X), num_starts, beta,
                                                                        want_score=True))
    assert score.dtype == np.float32 and idx.dtype == np.int32
    # idx: exactly the top-k of the kernel's own scores, descending, ties to the lower index
    order = np.lexsort((np.arange(Ns), -score[0].astype(np.float64)))[:num_starts]
    np.testing.assert_array_equal(idx[0], order)
    np.testing.assert_array_equal(x0[0], X[idx[0]])
    if Ns >= 64:
        assert score[0, 3] == score[0, 40] == score[0, Ns - 1]
    # the scores: the statement over the oracle's members, at the value tolerance
    F = np.stack([O.predict(p, acts, X, dtype=np.float64)[:, 0] for p in ps])
    np.testing.assert_allclose(score[0], ensemble_stats(F, beta)[2], **VAL_TOL)
    # per-ensemble candidates: the same bits as the shared form, whichever ensemble
    both = torch.cat([theta, theta], dim=0).contiguous()
    xs, ids, ss = (t.cpu().numpy() for t in ops.ensemble_screen_topk(desc, both, dev(X), num_starts, beta,
                                                                     want_score=True))
    xp, idp, sp = (t.cpu().numpy() for t in ops.ensemble_screen_topk(desc, both, dev(np.stack([X, X])), num_starts,
                                                                     beta, want_score=True))
    for e in range(2):
        for a, b, c in ((xs, xp, x0), (ids, idp, idx), (ss, sp, score)):
            np.testing.assert_array_equal(a[e], b[e])
            np.testing.assert_array_equal(a[e], c[0])
    # without a score buffer: the same picks
    x0n, idxn = ops.ensemble_screen_topk(desc, theta, dev(X), num_starts, beta)
    np.testing.assert_array_equal(idxn.cpu().numpy(), idx)
    np.testing.assert_array_equal(x0n.cpu().numpy(), x0)


# ---- restarts -------------------------------------------------------------------------------------------------------
def same_record(h, x, fun, jac, info, where):
    np.testing.assert_array_equal(h.x, x, err_msg=str(where))
    assert h.fun == fun, where
    np.testing.assert_array_equal(h.jac, jac, err_msg=str(where))
    assert (h.nit, h.nfev, h.status) == tuple(info[:3]), where
    assert h.task == tuple(info[3:]), where


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("maxcor", [3, 10])
@pytest.mark.parametrize("k", range(len(NETS)))
def test_restarts_equal_the_host_build_bit_for_bit(gpu, k, maxcor, fixed):
    desc, theta, ps, _, _, _ = case(k)
    D = NETS[k][0]
    rs = np.random.RandomState(300 + k)
    R0, beta, tr = 5, 1.5, "sigmoid"
    X0 = rs.uniform(-0.1, 1.1, size=(1, R0, D))                   # (some starts outside the box)
    lo, hi = np.zeros(D), np.ones(D)
    if fixed:
        lo[D - 1] = hi[D - 1] = 0.25                              # one fixed coordinate
    opts = dict(maxiter=30, maxcor=maxcor)
    x, fun, jac, info = (t[0] for t in ops.lbfgsb_results_to_host(
        *ops.ensemble_lbfgsb_minimize(desc, theta, dev(X0), lo, hi, beta, tr, True, **opts)))
    assert ((x >= lo - 1e-12) & (x <= hi + 1e-12)).all() and (info[:, 1] >= 1).all() and info[:, 0].max() >= 1

    def f(xx):
        v, g = fg(desc, theta, np.atleast_2d(xx)[None], beta, tr, True)
        return v[0, 0], g[0, 0]

    for r in range(R0):
        same_record(H.minimize(f, X0[0, r], (lo, hi), **opts), x[r], fun[r], jac[r], info[r], (k, maxcor, fixed, r))


def test_restarts_geometry_does_not_change_bits(gpu):
    """Nine starts (three groups of waves), two ensembles: each ensemble alone and 4 + 5 starts in two calls."""
    desc, theta, ps, _, _, _ = case(0)
    D = NETS[0][0]
    both = torch.cat([theta, torch.flip(theta, dims=[1]) * 0.5], dim=0).contiguous()
    X0 = np.random.RandomState(5).uniform(size=(2, 9, D))
    lo, hi = np.zeros(D), np.ones(D)

    def run(th, x0):
        return ops.lbfgsb_results_to_host(*ops.ensemble_lbfgsb_minimize(desc, th, dev(x0), lo, hi, 1.5, "identity", True,
                                                                        maxiter=30))

    whole = run(both, X0)
    for e in range(2):
        for a, b in zip(whole, run(both[e:e + 1].contiguous(), X0[e:e + 1])):
            np.testing.assert_array_equal(a[e], b[0])
    first, rest = run(both, np.ascontiguousarray(X0[:, :4])), run(both, np.ascontiguousarray(X0[:, 4:]))
    for a, b, c in zip(whole, first, rest):
        np.testing.assert_array_equal(a, np.concatenate([b, c], axis=1))


# ---- the model layer --------------------------------------------------------------------------------------------------
def blobs(N, D, seed):
    rs = np.random.RandomState(seed)
    X = rs.uniform(size=(N, D))
    y = np.sum((X - 0.4) ** 2, axis=1)
    return X, (y < np.quantile(y, 0.25)).astype(np.float32)


def build_ensemble(cls, K, seed=3, beta=1.0, units=(16, 16), D=2, **kw):
    from bore_amd.layers import BinaryCrossentropy, Dense
    m = cls(*kw.pop("args", ()), members=K, beta=beta, seed=seed, **kw)
    for u in units:
        m.add(Dense(u, activation="relu"))
    m.add(Dense(1))
    m.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True), metrics=["accuracy"])
    m.build(D)
    return m


@pytest.mark.parametrize("weighted", [False, True])
def test_fit_equals_lone_models_member_by_member(gpu, weighted):
    from bore_amd.models import EnsembleSequential
    K, N, E, B = 3, 40, 5, 16
    X, z = blobs(N, 2, 0)
    w = np.random.RandomState(1).uniform(0.5, 2.0, size=N).astype(np.float32) if weighted else None
    m = build_ensemble(EnsembleSequential, K)
    th0 = m.theta.clone()
    assert tuple(m.theta.shape) == (K, ops.param_count(m._desc)) and tuple(m.adam_t.shape) == (K,)
    hist = m.fit(X, z, epochs=E, batch_size=B, sample_weight=w)
    losses = []
    for k in range(K):                                      # a lone model: that member's weights, seed and shuffle stream
        th, am, av = th0[k:k + 1].clone(), torch.zeros_like(th0[k:k + 1]), torch.zeros_like(th0[k:k + 1])
        at = torch.zeros(1, dtype=torch.int64, device=th.device)
        W = None if w is None else dev(w)[None]
        losses.append(ops.mlp_fit(m._desc, th, am, av, at, dev(X.astype(np.float32))[None], dev(z)[None], E, B,
                                  seed=m._shuffle_seed, model_index0=k, sample_weight=W).cpu().numpy()[0])
        np.testing.assert_array_equal(m.theta[k].cpu().numpy(), th[0].cpu().numpy())
        np.testing.assert_array_equal(m.adam_m[k].cpu().numpy(), am[0].cpu().numpy())
        np.testing.assert_array_equal(m.adam_v[k].cpu().numpy(), av[0].cpu().numpy())
        assert int(m.adam_t[k]) == int(at[0]) == E * 3
    np.testing.assert_allclose(hist.history["loss"], np.mean(losses, axis=0), rtol=1e-6)
    # member 0 drew what a lone Sequential of this seed draws
    from bore_amd.layers import Dense
    from bore_amd.models import Sequential
    lone = Sequential([Dense(16, activation="relu"), Dense(16, activation="relu"), Dense(1)], seed=3)
    lone.build(2)
    np.testing.assert_array_equal(lone.theta[0].cpu().numpy(), th0[0].cpu().numpy())
    # the model layer's own path for member 0, whose shuffle stream is a lone model's: an actual Sequential.fit
    if not weighted:
        lone.compile(optimizer="adam", loss=m._loss)
        lone.fit(X, z, epochs=E, batch_size=B)
        np.testing.assert_array_equal(lone.theta[0].cpu().numpy(), m.theta[0].cpu().numpy())
        np.testing.assert_array_equal(lone.adam_m[0].cpu().numpy(), m.adam_m[0].cpu().numpy())
        np.testing.assert_array_equal(lone.adam_v[0].cpu().numpy(), m.adam_v[0].cpu().numpy())
        assert int(lone.adam_t[0]) == int(m.adam_t[0])
    # after the fit the members differ, and the surface holds together
    th = m.theta.cpu().numpy()
    assert all(np.abs(th[a] - th[b]).max() > 1e-3 for a in range(K) for b in range(a))
    pm = m.predict_members(X)
    assert pm.shape == (K, N, 1) and pm.dtype == np.float32
    mu, sd = m.predict(X), m.predict_std(X)
    assert mu.shape == sd.shape == (N, 1) and mu.dtype == sd.dtype == np.float32 and (sd > 0).all()
    np.testing.assert_allclose(mu[:, 0], pm[..., 0].astype(np.float64).mean(axis=0), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(sd[:, 0], pm[..., 0].astype(np.float64).std(axis=0), rtol=1e-4, atol=1e-6)
    loss, acc = m.evaluate(X, z)
    member_losses = [float(ops.mlp_evaluate(m._desc, m.theta[k:k + 1], dev(X.astype(np.float32))[None], dev(z)[None])[0][0])
                     for k in range(K)]
    assert loss == pytest.approx(np.mean(member_losses), rel=1e-6)
    assert acc == pytest.approx(np.mean((mu[:, 0] > 0.5) == (z > 0.5)))
    ws = m.get_weights(member=1)
    np.testing.assert_array_equal(np.concatenate([a.ravel() for a in ws]), th[1])
    m.set_weights(m.get_weights(member=2), member=0)
    np.testing.assert_array_equal(m.theta[0].cpu().numpy(), th[2])
    np.testing.assert_array_equal(m.theta[1].cpu().numpy(), th[1])


def test_fit_of_more_rows_than_the_device_shuffles(gpu):
    """More rows than an LDS ranks: ops.mlp_fit asks for explicit shuffles (NeedsPermError) and the model draws every
    member's from the host statement of its own stream -- the same bits as a lone fit handed that stream's shuffles."""
    from bore_amd import shuffle
    from bore_amd.models import EnsembleSequential
    K, N, B = 2, 20000, 256
    X, z = blobs(N, 2, 5)
    m = build_ensemble(EnsembleSequential, K, units=(8,))
    th0 = m.theta.clone()
    Xd, zd = dev(X.astype(np.float32))[None], dev(z)[None]
    with pytest.raises(_lib.NeedsPermError):
        ops.mlp_fit(m._desc, th0[:1].clone(), torch.zeros_like(th0[:1]), torch.zeros_like(th0[:1]),
                    torch.zeros(1, dtype=torch.int64, device=th0.device), Xd, zd, 1, B, seed=m._shuffle_seed)
    hist = m.fit(X, z, epochs=1, batch_size=B)
    assert np.isfinite(hist.history["loss"]).all() and m._epochs_seen == 1
    for k in range(K):
        th, am, av = th0[k:k + 1].clone(), torch.zeros_like(th0[k:k + 1]), torch.zeros_like(th0[k:k + 1])
        at = torch.zeros(1, dtype=torch.int64, device=th.device)
        perm = dev(shuffle.permutations(m._shuffle_seed, 1, 1, N, model_index0=k))
        ops.mlp_fit(m._desc, th, am, av, at, Xd, zd, 1, B, perm=perm)
        np.testing.assert_array_equal(m.theta[k].cpu().numpy(), th[0].cpu().numpy())
        np.testing.assert_array_equal(m.adam_v[k].cpu().numpy(), av[0].cpu().numpy())
        assert int(m.adam_t[k]) == int(at[0]) == -(-N // B)


def test_argmax_is_at_least_as_good_as_any_sample(gpu):
    """The reference's own property (its tests/test_models.py) on an ensemble of untrained activation-free nets."""
    from bore_amd.layers import Dense
    from bore_amd.models import MaximizableEnsembleSequential
    D = 4
    m = MaximizableEnsembleSequential("identity", members=3, beta=1.0, seed=8)
    m.add(Dense(8))
    m.add(Dense(8))
    m.add(Dense(1))
    m.build(D)
    rs = np.random.RandomState(42)
    bounds = Bounds(np.zeros(D), np.ones(D))
    opt = m.argmax(bounds, num_starts=5, num_samples=1024, print_fn=lambda s: None, random_state=rs)
    X_test = rs.uniform(size=(1024, D))
    assert opt is not None
    # the acquisition's own score: what argmax maximises
    assert m.predict_score(opt.x[None])[0, 0] >= m.predict_score(X_test).max()
    # beta = 0: the members' mean, predict itself
    m.beta = 0.0
    opt = m.argmax(bounds, num_starts=5, num_samples=1024, print_fn=lambda s: None, random_state=rs)
    assert m.predict(opt.x[None])[0, 0] >= m.predict(X_test).max()


@pytest.mark.parametrize("transform", ["identity", "sigmoid"])
def test_maxima_device_route_agrees_with_the_lockstep_route(gpu, transform):
    from bore_amd.models import MaximizableEnsembleSequential
    X, z = blobs(40, 2, 2)
    m = build_ensemble(MaximizableEnsembleSequential, 4, args=(transform,))
    m.fit(X, z, epochs=60, batch_size=16)
    bounds = Bounds(np.zeros(2), np.ones(2))
    kw = dict(num_starts=5, num_samples=1024, print_fn=lambda s: None)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)           # (neither route falls back)
        on_dev = m.maxima(bounds, random_state=np.random.RandomState(9), **kw)
        m.restart_mode, m.screen_mode = "lockstep", "host"
        on_host = m.maxima(bounds, random_state=np.random.RandomState(9), **kw)
    assert len(on_dev) == len(on_host) == 5
    ok = lambda r: bool(r.success or r.status == 1)
    same = sum(ok(a) == ok(b) and (not ok(a) or np.allclose(a.x, b.x, rtol=0, atol=1e-5)) for a, b in zip(on_dev, on_host))
    best_d = min((r.fun for r in on_dev if ok(r)), default=None)
    best_h = min((r.fun for r in on_host if ok(r)), default=None)
    print(f"\n[ensemble maxima {transform}] same restarts {same}/5, best fun device {best_d} host {best_h}")
    assert (best_d is None) == (best_h is None)
    assert best_d is None or abs(best_d - best_h) <= 1e-6
    assert same >= 4
    # num_starts = 0 and another SciPy method run on the host through the statement
    best = m.maxima(bounds, num_starts=0, num_samples=64, print_fn=lambda s: None, random_state=np.random.RandomState(1))
    assert len(best) == 1 and best[0].success
    m.restart_mode = "device"
    slsqp = m.maxima(bounds, num_starts=2, num_samples=64, method="SLSQP", options=dict(maxiter=20),
                     print_fn=lambda s: None, random_state=np.random.RandomState(1))
    assert len(slsqp) == 2 and all(np.isfinite(r.fun) for r in slsqp)


def test_a_refused_request_warns_and_still_returns(gpu):
    """Sixteen members of the plugin's network: the fit takes them, the ensemble kernels do not (K images > LDS)."""
    from bore_amd.models import MaximizableEnsembleDenseSequential
    from bore_amd.layers import BinaryCrossentropy
    m = MaximizableEnsembleDenseSequential("sigmoid", 16, 1, 2, 32, layer_kws=dict(activation="elu"), members=16, seed=0)
    m.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True))
    X, z = blobs(30, 16, 4)
    m.fit(X, z, epochs=3, batch_size=16)
    with pytest.raises(_lib.UnsupportedError, match="16 members' images"):
        ops.ensemble_value_and_input_grad(m._desc, m.theta[None], dev(X[None, :2]), 1.0)
    with pytest.warns(RuntimeWarning, match="16 members' images"):
        res = m.maxima(Bounds(np.zeros(16), np.ones(16)), num_starts=3, num_samples=64, options=dict(maxiter=5),
                       print_fn=lambda s: None, random_state=np.random.RandomState(0))
    assert len(res) == 3 and all(np.isfinite(r.fun) for r in res)


def test_streamed_network_is_refused_by_name(gpu):
    from bore_amd.layers import Dense
    from bore_amd.models import EnsembleSequential
    m = EnsembleSequential([Dense(256, activation="relu"), Dense(256, activation="relu"), Dense(1)], members=2, seed=0)
    with pytest.raises(_lib.UnsupportedError, match="streamed"):
        m.build(8)


# ---- the plugin --------------------------------------------------------------------------------------------------------
def drive(s, n):
    rs = np.random.RandomState(0)
    out = []
    for _ in range(n):
        x, info = s.suggest()
        s.observe(x, float(np.sum((np.asarray(x) - 0.3) ** 2) + 0.01 * rs.normal()))
        out.append((np.asarray(x).copy(), info["source"]))
    return out


def test_suggester_without_ensemble_is_todays_path_to_the_bit(gpu):
    from bore_amd.plugins.classifier import ClassifierSuggester
    kw = dict(bounds=Bounds(np.zeros(2), np.ones(2)), num_random_init=4, num_steps_per_iter=50, num_starts=3,
              num_samples=128, seed=11)
    a = drive(ClassifierSuggester(**kw), 8)
    b = drive(ClassifierSuggester(ensemble=None, **kw), 8)
    assert [s for _, s in a] == [s for _, s in b] and any(s == "model" for _, s in a)
    for (xa, _), (xb, _) in zip(a, b):
        np.testing.assert_array_equal(xa, xb)


@pytest.mark.parametrize("weighting", [None, "lfbo"])
def test_suggester_with_an_ensemble(gpu, weighting):
    from bore_amd.models import MaximizableEnsembleDenseSequential
    from bore_amd.plugins.classifier import ClassifierSuggester
    s = ClassifierSuggester(bounds=Bounds(np.zeros(2), np.ones(2)), num_random_init=4, num_steps_per_iter=50,
                            num_starts=3, num_samples=128, seed=11, random_rate=0.0, ensemble=4, beta=1.0,
                            weighting=weighting)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)           # (the device route takes it: no fallback)
        out = drive(s, 7)
    assert type(s.logit) is MaximizableEnsembleDenseSequential and tuple(s.logit.theta.shape)[0] == 4
    assert sum(src == "model" for _, src in out) >= 2 and np.isfinite(s.last_fit).all()
    assert all(((x >= 0) & (x <= 1)).all() for x, _ in out)
