"""LFBO weighting on the device: ``bore_lfbo_labels`` against its numpy statement bit for bit, a soft-label weighted fit
against the float64 checker (tests/weighted_oracle.py) at the tolerances tests/test_gpu_weighted.py holds the generic
and the streamed flavour to, the lock-step engines under a weighting (C++ host loop against the Python statement,
and against the chain done by hand), and the plugin.  Everything here needs an MI355X."""
import numpy as np
import pytest
import torch

import weighted_oracle as WO
from bore_amd import _lib, ops
from bore_amd.data import lfbo_targets
from bore_amd.engine import NativeEngine, ReplicaEngine
from bore_amd.plugins.classifier import ClassifierSuggester
from oracle import bore_oracle as O
from test_gpu_weighted import GEN_TOL, GENERIC, STREAM_TOL, check_against, dev, pack, rand_model, run_fit, stream

pytestmark = pytest.mark.gpu

MODES = [("ei", True), ("ei", False), ("lfbo", True), ("lfbo", False)]
GAMMAS = [0.0, 0.25, 1 / 3, 1.0]


# ---- the kernel -------------------------------------------------------------------------------------------------------
def label_batches(N):
    """Two [3, N] batches: three different data sets; and distinct values / ties at every threshold / all equal."""
    rs = np.random.RandomState(200 + N)
    ties = (np.arange(N) % 3)[rs.permutation(N)].astype(np.float64)
    return [np.stack([50.0 * rs.normal(size=N) - 7.0, rs.uniform(size=N), 1e-3 * rs.normal(size=N)]),
            np.stack([rs.normal(size=N), ties, np.full(N, 1.25)])]


@pytest.mark.parametrize("weighting,normalize", MODES)
@pytest.mark.parametrize("N", [1, 2, 5, 64, 65, 257])
def test_lfbo_labels_equal_the_numpy_statement_bit_for_bit(gpu, N, weighting, normalize):
    for y in label_batches(N):
        yd = dev(y)
        for gamma in GAMMAS:
            z, w, tau = ops.lfbo_labels(yd, gamma, weighting, normalize, want_tau=True)
            z, w, tau = z.cpu().numpy(), w.cpu().numpy(), tau.cpu().numpy()
            assert z.shape == w.shape == (3, N) and tau.shape == (3,)
            for l in range(3):
                rz, rw, rtau = lfbo_targets(y[l], gamma, weighting, normalize)
                assert tau[l] == np.quantile(y[l], gamma) == rtau, (l, gamma)
                np.testing.assert_array_equal(z[l], rz, err_msg=f"z: model {l}, gamma {gamma}")
                np.testing.assert_array_equal(w[l], rw, err_msg=f"w: model {l}, gamma {gamma}")
            if weighting == "ei":
                np.testing.assert_array_equal(z, ops.labels(yd, gamma).cpu().numpy())
            z2, w2 = ops.lfbo_labels(yd, gamma, weighting, normalize)         # (no tau asked for)
            assert torch.equal(z2.cpu(), torch.from_numpy(z)) and torch.equal(w2.cpu(), torch.from_numpy(w))


# ---- a soft-label weighted fit ------------------------------------------------------------------------------------------
FIT_N, FIT_B, FIT_E = 7, 4, 6


@pytest.fixture(scope="module")
def soft_fit_ref():
    """3->5-7-1, seven rows in batches of four, six epochs, explicit shuffles, "lfbo" targets: the float64 trajectory,
    computed once and left alone."""
    D, units, acts = GENERIC
    rs = np.random.RandomState(301)
    p = rand_model(rs, D, units)
    X = rs.uniform(size=(FIT_N, D)).astype(np.float32)
    y = np.sum((X.astype(np.float64) - 0.4) ** 2, axis=1) * 20.0
    z, w, _ = lfbo_targets(y, 1 / 3, "lfbo", True)
    hard = (y < np.quantile(y, 1 / 3)).astype(np.float32)
    assert 0 < hard.sum() < FIT_N and np.any((z > 0) & (z < 1)) and np.any(w != 1)
    perms = np.stack([rs.permutation(FIT_N) for _ in range(FIT_E)]).astype(np.int32)
    p64 = [a.astype(np.float64) for a in p]
    st = O.AdamState(p64)
    hist = WO.weighted_fit(p64, acts, st, X, z, w, perms, batch_size=FIT_B)
    ref = dict(theta=pack(p64), m=pack(st.m), v=pack(st.v), t=st.t, hist=hist)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return (p, X, z, w, hard, perms), ref


@pytest.mark.parametrize("forced", [False, True], ids=["generic", "streamed"])
def test_soft_label_weighted_fit_matches_the_checker(gpu, monkeypatch, soft_fit_ref, forced):
    stream(monkeypatch, forced)
    D, units, acts = GENERIC
    desc = _lib.make_desc(D, units, acts)
    assert ops.mlp_streamed(desc) == 0
    (p, X, z, w, hard, perms), ref = soft_fit_ref
    got = run_fit(desc, p, X, z, w, perms, FIT_E, FIT_B)
    check_against(ref, got, STREAM_TOL if forced else GEN_TOL, FIT_E * O.steps_per_epoch(FIT_N, FIT_B))
    # the weights and the soft targets are not dropped: the unweighted fit on the hard labels is somewhere else
    plain = run_fit(desc, p, X, hard, None, perms, FIT_E, FIT_B)
    assert np.abs(plain[4][0] - ref["hist"]).max() > 1e-2 * np.abs(ref["hist"]).max()


# ---- the engines --------------------------------------------------------------------------------------------------------
def quadratic(X):
    return np.sum((X - 0.3) ** 2, axis=-1)


NETS = {
    "static-2x16": dict(input_dim=2, units=(16, 16, 1), acts=("relu", "relu", "sigmoid")),   # has a static fit kernel
    "generic-3x5x7": dict(input_dim=3, units=(5, 7, 1), acts=("elu", "tanh", "sigmoid")),
    "streamed-8x256": dict(input_dim=8, units=(256, 256, 1), acts=("relu", "relu", "linear")),
}
IDS = np.arange(3, 6)
COMMON = dict(n_init=5, epochs=4, batch_size=4, num_starts=2, num_samples=64, objective=quadratic, seed=7,
              gamma=1 / 3, options=dict(maxiter=30, ftol=1e-9))
ENGINE_CASES = [(n, w) for n in ("static-2x16", "generic-3x5x7") for w in ("ei", "lfbo")] + [("streamed-8x256", "lfbo")]

_runs = {}


def native_run(name, groups, **kw):
    """A NativeEngine after three steps, once per request: observations and state."""
    key = (name, groups, tuple(sorted(kw.items())))
    if key not in _runs:
        a = NativeEngine(IDS, groups=groups, **NETS[name], **COMMON, **kw)
        th0 = a.state()[0]
        a.run(3)
        X, y = a.observations()
        _runs[key] = dict(X=X, y=y, th0=th0, state=a.state(), stats=a.take_stats())
        a.close()
    return _runs[key]


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("name,weighting", ENGINE_CASES)
def test_native_engine_equals_python_engine_under_a_weighting(gpu, name, weighting, groups):
    a = native_run(name, groups, weighting=weighting)
    b = ReplicaEngine(IDS, mode="device", groups=groups, **NETS[name], **COMMON, weighting=weighting)
    b.run(3)
    assert a["X"].shape == (3, 5 + 3, NETS[name]["input_dim"])
    assert np.array_equal(a["X"], b.X) and np.array_equal(a["y"], b.y)
    th, m, v, t = a["state"]
    assert np.array_equal(th, b.theta.cpu().numpy()) and np.array_equal(m, b.adam_m.cpu().numpy())
    assert np.array_equal(v, b.adam_v.cpu().numpy()) and np.array_equal(t, b.adam_t.cpu().numpy())
    assert np.all(t == 4 * (2 + 2 + 2)) and not np.array_equal(th, a["th0"])      # N = 5, 6, 7 in batches of 4
    assert a["stats"]["fit_launches"] == 3 * min(groups, 3)


@pytest.mark.parametrize("name,weighting,normalize", [("static-2x16", "lfbo", True), ("static-2x16", "ei", False),
                                                     ("generic-3x5x7", "lfbo", False)])
def test_the_engines_first_step_is_the_chain_done_by_hand(gpu, name, weighting, normalize):
    """After one step, a loop's theta / m / v are ``ops.lfbo_labels`` on its record followed by
    ``ops.mlp_fit(sample_weight=)`` with the engine's seed, ``model_index0`` and ``epoch0``.  For 2->16-16-1 this is
    also what shows the request left the static kernel: the weighted entry point has no other route."""
    net = NETS[name]
    a = NativeEngine(IDS, groups=1, **net, **COMMON, weighting=weighting, normalize_utility=normalize)
    th0 = a.state()[0]
    a.run(1)
    X, y = a.observations()
    th, m, v, t = a.state()
    a.close()
    D = net["input_dim"]
    desc = _lib.make_desc(D, list(net["units"]), list(net["acts"]))
    l = 1                                                   # the middle loop, alone
    yd = dev(y[l:l + 1, :5])
    z, w = ops.lfbo_labels(yd, COMMON["gamma"], weighting, normalize)
    theta = dev(th0[l:l + 1])
    dm, dv = torch.zeros_like(theta), torch.zeros_like(theta)
    dt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.mlp_fit(desc, theta, dm, dv, dt, dev(X[l:l + 1, :5].astype(np.float32)), z, COMMON["epochs"],
                COMMON["batch_size"], seed=COMMON["seed"], model_index0=int(IDS[l]), epoch0=0, want_loss=False,
                sample_weight=w)
    np.testing.assert_array_equal(theta.cpu().numpy()[0], th[l])
    np.testing.assert_array_equal(dm.cpu().numpy()[0], m[l])
    np.testing.assert_array_equal(dv.cpu().numpy()[0], v[l])
    assert int(dt[0]) == int(t[l]) == 4 * 2


def test_weighting_is_live_and_the_default_is_untouched(gpu):
    plain = native_run("generic-3x5x7", 1)
    none = native_run("generic-3x5x7", 1, weighting=None, normalize_utility=False)
    lfbo = native_run("generic-3x5x7", 1, weighting="lfbo")
    ei = native_run("generic-3x5x7", 1, weighting="ei")
    for k in ("X", "y"):
        assert np.array_equal(plain[k], none[k])
    for p, q in zip(plain["state"], none["state"]):
        assert np.array_equal(p, q)
    assert not np.array_equal(plain["state"][0], lfbo["state"][0])
    assert not np.array_equal(ei["state"][0], lfbo["state"][0])
    raw = native_run("generic-3x5x7", 1, weighting="lfbo", normalize_utility=False)
    assert not np.array_equal(raw["state"][0], lfbo["state"][0])
    # the Python statement without the argument: the same default
    b = ReplicaEngine(IDS, mode="device", groups=1, **NETS["generic-3x5x7"], **COMMON)
    b.run(3)
    assert np.array_equal(plain["X"], b.X) and np.array_equal(plain["state"][0], b.theta.cpu().numpy())


def test_the_numpy_stages_fit_on_lfbo_targets(gpu):
    """``ReplicaEngine.label()`` / ``fit()`` (the lock-step mode's stages) under a weighting: ``data.lfbo_targets`` per
    loop and the weighted fit -- the bits of the device statement's first fit."""
    net = NETS["generic-3x5x7"]
    b = ReplicaEngine(IDS, mode="lockstep", **net, **COMMON, weighting="lfbo")
    z, w = b.label()
    for l in range(3):
        rz, rw, _ = lfbo_targets(b.y[l], COMMON["gamma"], "lfbo", True)
        assert np.array_equal(z[l], rz) and np.array_equal(w[l], rw)
    b.fit(z, w)
    a = NativeEngine(IDS, groups=1, **net, **COMMON, weighting="lfbo")
    a.run(1)
    th = a.state()[0]
    a.close()
    assert np.array_equal(th, b.theta.cpu().numpy())


# ---- the plugin ---------------------------------------------------------------------------------------------------------
def test_the_suggester_fits_its_model_on_lfbo_data(gpu):
    def make():
        s = ClassifierSuggester(bounds=[(0.0, 1.0), (0.0, 1.0)], weighting="lfbo", num_epochs_per_iter=5, seed=11,
                                random_rate=None, num_random_init=10, num_starts=2, num_samples=64)
        rs = np.random.RandomState(5)
        for _ in range(12):
            x = rs.uniform(size=2)
            s.observe(x, float(np.sum((x - 0.4) ** 2)))
        return s

    s = make()
    x, info = s.suggest()
    assert info["source"] in ("model", "random:failed") and s.last_fit is not None
    # a model of the same seed, fitted by hand on the record's LFBO data
    t = make()
    model = t._build_compile_network()
    X, z, w = t.record.load_lfbo_data(t.gamma, "lfbo", True)
    model.fit(X, z, epochs=5, batch_size=t.batch_size, callbacks=[], verbose=False, sample_weight=w)
    for got, want in zip(s.logit.get_weights(), model.get_weights()):
        np.testing.assert_array_equal(got, want)
    loss, _ = model.evaluate(X, z, verbose=False, sample_weight=w)
    _, acc = model.evaluate(X, t.record.load_classification_data(t.gamma)[1], verbose=False)
    assert s.last_fit == (loss, acc)
    # ... and not the unweighted classifier's
    u = ClassifierSuggester(bounds=[(0.0, 1.0), (0.0, 1.0)], num_epochs_per_iter=5, seed=11, random_rate=None,
                            num_random_init=10, num_starts=2, num_samples=64)
    for xo, yo in zip(s.record.features, s.record.targets):
        u.observe(xo, yo)
    u.suggest()
    assert not np.array_equal(u.logit.get_weights()[0], s.logit.get_weights()[0])
