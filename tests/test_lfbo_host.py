"""LFBO weighting, host side (no GPU): ``data.lfbo_targets`` against a float64 restatement, the identity that makes
the soft-label form LFBO's objective, ``Record.load_lfbo_data``, what the plugins pass to ``fit`` / ``evaluate`` under
a weighting, the refusals, and ``bore_engine_cfg``'s layout with ``weighting`` where ``reserved`` was."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from bore_amd import _lib
from bore_amd.data import Record, classification_labels, lfbo_targets
from bore_amd.engine import NativeEngine, ReplicaEngine, lbfgsb_opts
from bore_amd.plugins.classifier import ClassifierSuggester
from bore_amd.plugins.hpbandster import BORE, BOREHyperband, SequenceClassifierConfigGenerator
from bore_amd.plugins.types import DenseSpace, UniformFloat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [("ei", True), ("ei", False), ("lfbo", True), ("lfbo", False)]
GAMMAS = [0.0, 0.25, 1 / 3, 1.0]


def restate(y, gamma, weighting, normalize):
    """The definition in float64, numpy's own sums: (z, w, tau, u)."""
    y = np.asarray(y, dtype=np.float64)
    tau = np.quantile(y, gamma)
    pos = y < tau
    u = np.where(pos, tau - y, 0.0)
    if normalize and pos.any():
        u = u / u[pos].mean()
    if weighting == "ei":
        return pos.astype(np.float64), np.where(pos, u, 1.0), tau, u
    return u / (1.0 + u), 1.0 + u, tau, u


def data_sets(N):
    """name -> y (N,): distinct values in other units, values with ties at every threshold, all equal."""
    rs = np.random.RandomState(100 + N)
    return {"distinct": 50.0 * rs.normal(size=N) - 7.0,
            "ties": (np.arange(N) % 3)[rs.permutation(N)].astype(np.float64),
            "all-equal": np.full(N, 1.25)}


def within_one_ulp(got, want64):
    want = want64.astype(np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


@pytest.mark.parametrize("weighting,normalize", MODES)
@pytest.mark.parametrize("N", [1, 2, 5, 65])
def test_lfbo_targets_against_the_float64_restatement(N, weighting, normalize):
    """The fp64 sum's error (at most N 2^-53 relative) is far below half a float32 ulp, so only the summation order can
    move the last float32 bit: one ulp."""
    for name, y in data_sets(N).items():
        for gamma in GAMMAS:
            z, w, tau = lfbo_targets(y, gamma, weighting, normalize)
            rz, rw, rtau, _ = restate(y, gamma, weighting, normalize)
            hard = classification_labels(y, gamma)
            assert isinstance(tau, np.float64) and tau == np.quantile(y, gamma) == rtau, (name, gamma)
            within_one_ulp(z, rz)
            within_one_ulp(w, rw)
            if weighting == "ei":
                assert np.array_equal(z, hard.astype(np.float32)), (name, gamma)
            else:                                   # a positive target exactly on the positives
                assert np.array_equal(z > 0, hard), (name, gamma)
            if not hard.any():                      # no positive: nothing divided, every row a plain negative
                assert np.all(z == 0) and np.all(w == 1)
    assert not classification_labels(data_sets(N)["all-equal"], 0.25).any()
    assert N == 1 or classification_labels(data_sets(N)["ties"], 1.0).any()


def test_ties_at_tau_are_negatives():
    y = np.array([2.0, 0.0, 2.0, 5.0, 2.0, 1.0, 7.0])
    assert np.quantile(y, 0.5) == 2.0
    z, w, tau = lfbo_targets(y, 0.5, "lfbo", False)
    assert tau == 2.0
    np.testing.assert_array_equal(z, np.array([0, 2 / 3, 0, 0, 0, 0.5, 0], dtype=np.float32))
    np.testing.assert_array_equal(w, np.array([1, 3, 1, 1, 1, 2, 1], dtype=np.float32))
    z, w, _ = lfbo_targets(y, 0.5, "ei", True)              # mean improvement 1.5
    np.testing.assert_array_equal(z, np.array([0, 1, 0, 0, 0, 1, 0], dtype=np.float32))
    np.testing.assert_array_equal(w, np.array([1, 2 / 1.5, 1, 1, 1, 1 / 1.5, 1], dtype=np.float32))


def test_normalisation_makes_the_targets_scale_free():
    y = data_sets(65)["distinct"]
    for weighting in ("ei", "lfbo"):
        a = lfbo_targets(y, 0.25, weighting, True)
        b = lfbo_targets(1024.0 * y, 0.25, weighting, True)          # (a power of two: exact in every step)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        c = lfbo_targets(1024.0 * y, 0.25, weighting, False)
        assert not np.array_equal(a[1], c[1])


def test_an_unknown_weighting_is_a_value_error():
    for bad in (None, "pi", 2):
        with pytest.raises(ValueError, match="weighting"):
            lfbo_targets(np.arange(4.0), 0.25, bad)
    with pytest.raises(ValueError, match="weighting"):
        _lib.weighting_code("pi")
    assert _lib.weighting_code(None) == 0 and _lib.weighting_code("ei", False) == 1
    assert _lib.weighting_code("lfbo") == 0x102


@pytest.mark.parametrize("normalize", [True, False])
def test_the_soft_label_form_is_the_lfbo_objective(normalize):
    """w BCE(f; z) with z = u / (1 + u), w = 1 + u equals u softplus(-f) + softplus(f): every row a negative of
    weight 1, a positive also a positive of weight u."""
    def softplus(a):
        return np.maximum(a, 0.0) + np.log1p(np.exp(-np.abs(a)))

    for y in data_sets(65).values():
        z, w, _, u = restate(y, 0.25, "lfbo", normalize)
        for f in (-30.0, -1.0, 0.0, 2.0, 30.0):
            bce = np.maximum(f, 0.0) - f * z + np.log1p(np.exp(-abs(f)))
            np.testing.assert_allclose(w * bce, u * softplus(-f) + softplus(f), rtol=1e-12, atol=0)


def test_record_load_lfbo_data():
    rec = Record()
    rs = np.random.RandomState(3)
    for _ in range(9):
        rec.append(rs.uniform(size=2), float(rs.normal()))
    X, z, w = rec.load_lfbo_data(1 / 3, "lfbo", normalize=False)
    Xc, zc = rec.load_classification_data(1 / 3)
    want = lfbo_targets(rec.load_target_vector(), 1 / 3, "lfbo", False)
    assert np.array_equal(X, Xc) and np.array_equal(z, want[0]) and np.array_equal(w, want[1])
    assert z.dtype == w.dtype == np.float32 and np.array_equal(z > 0, zc)
    _, z2, w2 = rec.load_lfbo_data(1 / 3, "lfbo")
    assert np.array_equal(w2, lfbo_targets(rec.load_target_vector(), 1 / 3, "lfbo", True)[1])
    assert not np.array_equal(w, w2)


# ---- plugins ----------------------------------------------------------------------------------------------------------
class FakeLogit:
    """Records what ``_update_classifier`` hands to the model."""

    def __init__(self):
        self.calls = []

    def fit(self, X, z, **kw):
        self.calls.append(("fit", X, z, kw))

    def evaluate(self, X, z, **kw):
        self.calls.append(("evaluate", X, z, kw))
        return (1.5, 0.25) if kw.get("sample_weight") is not None else (0.5, 0.875)


def suggester(**kw):
    s = ClassifierSuggester(bounds=[(0.0, 1.0), (0.0, 1.0)], gamma=1 / 3, num_epochs_per_iter=5, seed=0,
                            random_rate=None, **kw)
    rs = np.random.RandomState(5)
    for _ in range(12):
        x = rs.uniform(size=2)
        s.observe(x, float(np.sum((x - 0.4) ** 2)))
    s.logit = FakeLogit()
    return s


@pytest.mark.parametrize("weighting,normalize", MODES)
def test_the_suggester_fits_on_lfbo_targets_and_takes_the_accuracy_from_the_hard_labels(weighting, normalize):
    s = suggester(weighting=weighting, normalize_utility=normalize)
    s._update_classifier()
    X, hard = s.record.load_classification_data(1 / 3)
    z, w, _ = lfbo_targets(s.record.load_target_vector(), 1 / 3, weighting, normalize)
    (f, fX, fz, fkw), (e1, e1X, e1z, e1kw), (e2, e2X, e2z, e2kw) = s.logit.calls
    assert (f, e1, e2) == ("fit", "evaluate", "evaluate")
    assert np.array_equal(fX, X) and np.array_equal(fz, z) and np.array_equal(fkw["sample_weight"], w)
    assert fkw["epochs"] == 5 and fkw["batch_size"] == 64
    assert np.array_equal(e1X, X) and np.array_equal(e1z, z) and np.array_equal(e1kw["sample_weight"], w)
    assert np.array_equal(e2z, hard) and e2kw.get("sample_weight") is None
    assert s.last_fit == (1.5, 0.875)           # the weighted objective, the accuracy of the hard labels


def test_the_suggester_without_a_weighting_calls_what_it_called():
    s = suggester()
    assert s.weighting is None
    s._update_classifier()
    X, hard = s.record.load_classification_data(1 / 3)
    (f, fX, fz, fkw), (e, eX, ez, ekw) = s.logit.calls
    assert (f, e) == ("fit", "evaluate") and np.array_equal(fz, hard) and np.array_equal(ez, hard)
    assert fkw == dict(epochs=5, batch_size=64, callbacks=[], verbose=False) and ekw == dict(verbose=False)
    assert s.last_fit == (0.5, 0.875)
    with pytest.raises(ValueError, match="weighting"):
        ClassifierSuggester(bounds=[(0.0, 1.0)], weighting="pi")


def space():
    return DenseSpace([UniformFloat("a", 0.0, 1.0), UniformFloat("b", 0.0, 1.0)], seed=0)


def test_bore_hands_the_weighting_to_its_suggester():
    b = BORE(space(), seed=0, weighting="lfbo", normalize_utility=False)
    s = b.config_generator._suggester
    assert s.weighting == "lfbo" and s.normalize_utility is False
    s = BORE(space(), seed=0).config_generator._suggester
    assert s.weighting is None and s.normalize_utility is True


def test_the_multi_fidelity_plugin_refuses_a_weighting_by_name():
    with pytest.raises(_lib.UnsupportedError, match="weighting='lfbo'.*recurrent"):
        BOREHyperband(space(), seed=0, weighting="lfbo")
    with pytest.raises(_lib.UnsupportedError, match="weighting='ei'.*recurrent"):
        SequenceClassifierConfigGenerator(space(), 0.25, 10, 0.1, False, {}, dict(weighting="ei"),
                                          dict(num_starts=5), 0)
    assert BOREHyperband(space(), seed=0).config_generator.record is not None       # (None: as before)


# ---- the engine's configuration -------------------------------------------------------------------------------------
def test_engine_cfg_keeps_its_layout_with_weighting_where_reserved_was(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bore_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d %d %d %d\\n", sizeof(bore_engine_cfg), '
                   'offsetof(bore_engine_cfg, weighting), offsetof(bore_engine_cfg, work_queue), BORE_ABI_VERSION, '
                   'BORE_WEIGHTING_EI, BORE_WEIGHTING_LFBO, BORE_WEIGHTING_NORMALIZE); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    # the parent's: 144 bytes, `reserved` the last int32 at 140, right behind work_queue
    assert got == [144, 140, 136, 12, 1, 2, 0x100]
    assert C.sizeof(_lib.EngineCfg) == 144 and _lib.EngineCfg.weighting.offset == 140
    assert (_lib.WEIGHTING["ei"], _lib.WEIGHTING["lfbo"], _lib.WEIGHTING_NORMALIZE) == (1, 2, 0x100)


def create(D, units, weighting, compute="float32", async_loops=0):
    """bore_engine_create on valid host arrays (tests/test_engine_nets_host.py's form); -> (code, message, handle)."""
    desc = _lib.make_desc(D, units, ["relu"] * (len(units) - 1) + ["linear"], compute=compute)
    P = int(_lib.lib().bore_param_count(C.byref(desc)))
    L, n_init = 2, 10
    rs = np.random.RandomState(0)
    low, high = np.zeros(D), np.ones(D)
    dpp = C.POINTER(C.c_double)
    cfg = _lib.EngineCfg(L, 1, 3, n_init, 3, 64, 3, 64, _lib.TRANSFORM["identity"], 1, async_loops, 0, 0.25,
                         _lib.AdamCfg(1e-3, 0.9, 0.999, 1e-7), lbfgsb_opts(dict(maxiter=30, ftol=1e-9)),
                         low.ctypes.data_as(dpp), high.ctypes.data_as(dpp), -1, 0, -1, weighting)
    theta = rs.uniform(-0.1, 0.1, size=(L, P)).astype(np.float32)
    X0, y0 = rs.uniform(size=(L, n_init, D)), rs.uniform(size=(L, n_init))
    mt = np.empty((L, 625), dtype=np.uint32)
    for i in range(L):
        _, key, pos, _, _ = np.random.RandomState(3 + i).get_state()
        mt[i, :624], mt[i, 624] = key, pos
    cb = _lib.OBJECTIVE_FN(lambda xp, n, d, yp, user: 1)
    h = C.c_void_p()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.lib().bore_engine_create(C.byref(desc), C.byref(cfg), vp(theta), vp(X0), vp(y0), vp(mt), cb, None,
                                       C.byref(h))
    msg = _lib.lib().bore_last_error().decode()
    if rc == 0:
        _lib.lib().bore_engine_destroy(h)
    return rc, msg, h


@pytest.mark.parametrize("weighting", [1, 2, 0x101, 0x102])
def test_the_asynchronous_schedule_refuses_a_weighting_by_name(weighting):
    rc, msg, h = create(2, [16, 16, 1], weighting, async_loops=1)
    assert rc == -2 and not h.value, (rc, msg)
    assert msg.startswith("engine_create: weighting") and "async_loops = 0" in msg


def test_a_bfloat16_engine_refuses_a_weighting_by_name():
    rc, msg, h = create(32, [128, 128, 1], 0x102, compute="bfloat16")
    assert rc == -2 and not h.value, (rc, msg)
    assert msg.startswith("engine_create: weighting") and "weighted fits are float32 only" in msg


@pytest.mark.parametrize("weighting", [3, 0x100, 0x200 | 2, -1])
def test_an_unknown_weighting_code_is_invalid_at_create(weighting):
    rc, msg, h = create(2, [16, 16, 1], weighting)
    assert rc == -1 and not h.value and "unknown weighting" in msg, (rc, msg)


def test_lfbo_labels_refuses_before_any_launch():
    """Mode 0, an unknown mode, N and gamma out of bore_labels' bounds, bad pointers: all before any HIP call."""
    L = _lib.lib()
    one = C.c_void_p(8)             # (never dereferenced: every call below is refused first)
    call = lambda N, gamma, weighting: L.bore_lfbo_labels(1, one, N, gamma, weighting, one, one, None, None)
    for weighting in (0, 3, 0x100, 0x202):
        assert call(5, 0.25, weighting) == -1 and b"unknown weighting" in L.bore_last_error()
    for N in (0, 16385):
        assert call(N, 0.25, 2) == -2 and b"outside 1..16384" in L.bore_last_error()
    for gamma in (-0.1, 1.5, float("nan")):
        assert call(5, gamma, 2) == -1 and b"gamma" in L.bore_last_error()
    assert L.bore_lfbo_labels(0, one, 5, 0.25, 2, one, one, None, None) == -1
    assert L.bore_lfbo_labels(1, None, 5, 0.25, 2, one, one, None, None) == -1
    assert L.bore_lfbo_labels(1, one, 5, 0.25, 2, one, None, None, None) == -1


def test_lfbo_labels_refuses_batch_mode():
    """As the weighted fit does (tests/test_stream_acq_host.py's form: the refusal comes before any HIP call)."""
    L = _lib.lib()
    one = C.c_void_p(8)
    batch = np.zeros(64, dtype=np.int64)              # (any non-null bore_batch)
    L.bore_set_batch(batch.ctypes.data_as(C.c_void_p))
    try:
        for weighting in (1, 2, 0x101, 0x102):
            assert L.bore_lfbo_labels(1, one, 5, 0.25, weighting, one, one, None, None) == -2
            assert b"lfbo_labels" in L.bore_last_error() and b"batch mode" in L.bore_last_error()
    finally:
        L.bore_set_batch(None)
    assert L.bore_lfbo_labels(1, one, 0, 0.25, 2, one, one, None, None) == -2     # (and out of it, the plain checks again)
    assert b"outside 1..16384" in L.bore_last_error()


@pytest.mark.parametrize("cls", [NativeEngine, ReplicaEngine])
def test_the_python_engines_take_a_weighting(cls):
    p = inspect.signature(cls.__init__).parameters
    assert p["weighting"].default is None and p["normalize_utility"].default is True
    with pytest.raises(ValueError, match="weighting"):
        cls(np.arange(2), device="cpu", weighting="pi")             # (raised before anything touches a device)


def test_the_python_statement_refuses_bfloat16_with_a_weighting():
    with pytest.raises(_lib.UnsupportedError, match="float32 only"):
        ReplicaEngine(np.arange(2), device="cpu", input_dim=32, units=(128, 128, 1), weighting="lfbo",
                      compute="bfloat16")
