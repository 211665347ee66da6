"""Classifier ensembles without a GPU: the numpy statement of the score (bore_amd/ensemble.py) against central
differences and against the single-model oracle; the host side of the ensemble entry points -- the plan query's
verdicts and every refusal that comes back before a launch, with its message, in the stated order (raw ctypes with
dummy non-null pointers: nothing is ever dereferenced); argument validation of the classes and the plugins."""
import ctypes as C

import numpy as np
import pytest

from bore_amd import _lib, ops
from bore_amd.ensemble import MAX_MEMBERS, VAR_FLOOR, ensemble_score, ensemble_stats
from oracle import bore_oracle as O

DUMMY = C.c_void_p(0x1000)
INVALID, UNSUPPORTED = -1, -2
ACTS = ["elu", "tanh", "linear"]
D, UNITS = 3, [5, 7, 1]


def members(K, seed):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(K):
        p = O.glorot_uniform_params(D, UNITS, rs, dtype=np.float64)
        for i in range(1, len(p), 2):
            p[i] = rs.normal(scale=0.1, size=p[i].shape)
        out.append(p)
    return out


def oracle_fg(ps, X):
    """F [K, R] and G [K, R, D] of the float64 oracle's members."""
    F = np.stack([O.predict(p, ACTS, X, dtype=np.float64)[:, 0] for p in ps])
    G = np.stack([-O.value_and_input_grad(p, ACTS, X, "identity", dtype=np.float64)[1] for p in ps])
    return F, G


# ---- the statement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("negate", [True, False])
@pytest.mark.parametrize("transform", ["identity", "sigmoid", "exp"])
@pytest.mark.parametrize("beta", [0.0, 1.5])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_gradient_against_central_differences(K, beta, transform, negate):
    ps = members(K, 10 + K)
    X = np.random.RandomState(K).uniform(-1, 1, size=(6, D))
    val, grad = ensemble_score(*oracle_fg(ps, X), beta, transform, negate)
    h = 1e-6
    num = np.empty_like(grad)
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        vp = ensemble_score(*oracle_fg(ps, X + e), beta, transform, negate)[0]
        vm = ensemble_score(*oracle_fg(ps, X - e), beta, transform, negate)[0]
        num[:, d] = (vp - vm) / (2 * h)
    np.testing.assert_allclose(grad, num, rtol=1e-5, atol=0)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_identical_members_weigh_one_over_K(K):
    p = members(1, 3)[0]
    X = np.random.RandomState(0).uniform(-1, 1, size=(9, D))
    F, G = oracle_fg([p] * K, X)
    mu, sigma, s, c = ensemble_stats(F, 1.5)
    np.testing.assert_allclose(c, 1.0 / K, rtol=0, atol=1e-9)
    np.testing.assert_allclose(sigma, np.sqrt(VAR_FLOOR), rtol=1e-6)
    val, grad = ensemble_score(F, G, 1.5, "identity", False)
    np.testing.assert_allclose(grad, G[0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(val, F[0] + 1.5e-6, rtol=0, atol=1e-9)      # (a constant shift of beta sqrt(floor))


@pytest.mark.parametrize("transform", ["identity", "sigmoid", "exp"])
def test_beta_zero_single_member_is_the_single_model_objective(transform):
    p = members(1, 4)[0]
    X = np.random.RandomState(1).uniform(-1, 1, size=(9, D))
    val, grad = ensemble_score(*oracle_fg([p], X), 0.0, transform, True)
    want_v, want_g = O.value_and_input_grad(p, ACTS, X, transform, dtype=np.float64)
    np.testing.assert_array_equal(val, want_v)            # (the value: the same bits under every transform)
    if transform == "identity":                           # (negation is exact: the same bits)
        np.testing.assert_array_equal(grad, want_g)
    # (the oracle scales the output delta by T' BEFORE the backward products, the statement the gradient after them:
    # the same float64 products in another order, a few eps over the three layers)
    np.testing.assert_allclose(grad, want_g, rtol=1e-13, atol=0)
    # un-negated, identity: the model's own output and gradient, exactly
    F, G = oracle_fg([p], X)
    val, grad = ensemble_score(F, G, 0.0, "identity", False)
    np.testing.assert_array_equal(val, F[0])
    np.testing.assert_array_equal(grad, G[0])


def test_statement_refuses_bad_arguments():
    F, G = np.zeros((2, 3)), np.zeros((2, 3, 4))
    for beta in (-0.1, np.nan, np.inf):
        with pytest.raises(ValueError, match="beta"):
            ensemble_score(F, G, beta)
    with pytest.raises(ValueError, match="transform"):
        ensemble_score(F, G, 0.0, "tanh")
    with pytest.raises(ValueError, match="G"):
        ensemble_score(F, np.zeros((3, 3, 4)), 0.0)
    with pytest.raises(ValueError, match="F"):
        ensemble_stats(np.zeros(3))


# ---- the plan query and the refusals, before any HIP call ------------------------------------------------------------
def desc(Din, units, compute="float32"):
    return _lib.make_desc(Din, units, ["elu"] * (len(units) - 1) + ["linear"], compute=compute)


NARROW = desc(2, [16, 16, 1])
PLUGIN = desc(16, [32, 32, 32, 1])
K_MSG = "an ensemble has 1..16 members (BORE_ENSEMBLE_MAX_MEMBERS), got %d"


def plan(d, K, beta=1.0, maxcor=10, n_ens=1, batch_mode=0):
    out = (C.c_int32 * len(ops.ENSEMBLE_PLAN_FIELDS))()
    L = _lib.lib()
    rc = L.bore_ensemble_plan_query(C.byref(d), n_ens, K, beta, maxcor, batch_mode, out, len(out))
    return rc, L.bore_last_error().decode(), dict(zip(ops.ENSEMBLE_PLAN_FIELDS, out))


def test_plan_narrow_network_takes_sixteen_members():
    rc, _, p = plan(NARROW, 16)
    assert rc == 0
    assert p["K"] == 16 and p["P_lds"] == 3 * (16 * 18 + 16) and p["image_bytes"] == 16 * 4 * p["P_lds"]
    assert p["waves"] == 4 and p["lds_bytes"] <= 160 * 1024
    assert p["lds_bytes"] == p["image_bytes"] + p["pass_bytes"] + 4 * p["ens_base"] + 16
    assert p["ens_base"] * 4 == p["o_prob"] * 4 + p["waves"] * p["slot_bytes"]
    # the carve: regions in order, 16-byte multiples, the images K x P_lds floats
    order = ["o_layout", "o_pre", "o_theta", "o_x", "o_wave", "o_f", "o_g", "o_val", "o_grad", "total"]
    offs = [p[k] for k in order]
    assert offs == sorted(offs) and all(o % 4 == 0 for o in offs)
    assert p["o_x"] - p["o_theta"] == 16 * p["P_lds"] and p["o_f"] - p["o_wave"] == 4 * p["wave_floats"]
    assert p["wave_floats"] >= 16 + 16 + 1 + 2 * 16
    assert ops.ensemble_plan_query(NARROW, 1, 16, 1.0, 10) == p
    # without restarts: no slots, the region at the start of the dynamic LDS
    rc, _, q = plan(NARROW, 16, maxcor=0)
    assert rc == 0 and q["waves"] == 0 and q["ens_base"] == 0 and q["lds_bytes"] == q["image_bytes"] + q["pass_bytes"] + 16


def test_plan_plugin_network_fits_eight_members_not_sixteen():
    rc, _, p = plan(PLUGIN, 8)
    assert rc == 0 and p["P_lds"] == 3408 and p["image_bytes"] == 8 * 13632 and 1 <= p["waves"] <= 4
    assert p["lds_bytes"] <= 160 * 1024
    rc, msg, _ = plan(PLUGIN, 16)
    assert rc == UNSUPPORTED
    assert f"16 members' images ({16 * 13632} B)" in msg and "(> 163840)" in msg and "fewer members" in msg
    for maxcor in (0, 10):                                    # (the images alone do not fit: the same refusal either way)
        assert plan(PLUGIN, 16, maxcor=maxcor)[:2] == (rc, msg)
    with pytest.raises(_lib.UnsupportedError, match="16 members' images"):
        ops.ensemble_plan_query(PLUGIN, 1, 16)


def test_plan_restart_slots_are_counted():
    """The most members of the plugin's network that fit for value + gradient and screening: no restart slot fits beside
    them at maxcor = 32, and the message carries the byte counts."""
    ok = [K for K in range(1, 17) if plan(PLUGIN, K, maxcor=0)[0] == 0]
    K = ok[-1]
    assert ok == list(range(1, K + 1)) and 8 <= K < 16
    rc, msg, _ = plan(PLUGIN, K, maxcor=32)
    assert rc == UNSUPPORTED and f"{K} members' images ({K * 13632} B)" in msg and "restart slots" in msg
    assert "maxcor = 32" in msg and "D = 16" in msg


@pytest.mark.parametrize("K", [0, -1, 17])
def test_plan_member_count_out_of_range(K):
    assert plan(NARROW, K)[:2] == (UNSUPPORTED, "ensemble_plan_query: " + K_MSG % K)


def test_plan_refusals_each_by_name():
    who = "ensemble_plan_query: "
    assert plan(desc(2, [16, 16, 1], compute="bfloat16"), 4)[:2] == \
        (UNSUPPORTED, who + "the ensemble kernels take compute = float32 members only")
    assert plan(desc(2, [16, 16, 2]), 4)[:2] == (INVALID, who + "the last Dense layer must have 1 unit")
    assert plan(NARROW, 4, beta=-0.5)[:2] == (INVALID, who + "beta must be finite and >= 0 (got -0.5)")
    assert plan(NARROW, 4, beta=float("nan"))[0] == INVALID and "beta must be finite" in plan(NARROW, 4, beta=float("nan"))[1]
    assert plan(NARROW, 4, beta=float("inf"))[0] == INVALID
    assert plan(NARROW, 4, n_ens=0)[:2] == (INVALID, who + "n_ensembles must be 1..65535 (got 0)")
    assert plan(desc(65, [16, 1]), 4)[:2] == (UNSUPPORTED, who + "the restarts take D <= BORE_DIM_MAX = 64 (got 65)")
    assert plan(desc(65, [16, 1]), 4, maxcor=0)[0] == 0
    assert plan(NARROW, 4, maxcor=33)[:2] == (UNSUPPORTED, "lbfgsb_minimize: maxcor must be 1..32")
    assert plan(NARROW, 4, batch_mode=1)[:2] == (UNSUPPORTED, who + "batch mode (bore_set_batch) takes no ensembles")


def test_plan_order_of_the_refusals():
    """K, compute, the last layer, beta, the LDS, batch mode: a request wrong in several ways is told the first."""
    bf16_two = desc(16, [32, 32, 32, 2], compute="bfloat16")
    two = desc(16, [32, 32, 32, 2])
    assert "members" in plan(bf16_two, 17, beta=-1.0, batch_mode=1)[1]
    assert "float32 members only" in plan(bf16_two, 16, beta=-1.0, batch_mode=1)[1]
    assert "last Dense layer" in plan(two, 16, beta=-1.0, batch_mode=1)[1]
    assert "beta must be" in plan(PLUGIN, 16, beta=-1.0, batch_mode=1)[1]
    assert "16 members' images" in plan(PLUGIN, 16, batch_mode=1)[1]
    assert "batch mode" in plan(PLUGIN, 8, batch_mode=1)[1]


def fg(d, K, beta=1.0, n_ens=1, transform=0, n_rows=4, null=()):
    p = {k: (None if k in null else DUMMY) for k in ["theta", "X", "val", "grad"]}
    L = _lib.lib()
    rc = L.bore_ensemble_value_and_input_grad(C.byref(d), n_ens, K, p["theta"], p["X"], n_rows, beta, transform, 1,
                                              p["val"], p["grad"], None)
    return rc, L.bore_last_error().decode()


def screen(d, K, beta=1.0, n_samples=256, num_starts=4, null=()):
    p = {k: (None if k in null else DUMMY) for k in ["theta", "X_init", "x0", "idx"]}
    L = _lib.lib()
    rc = L.bore_ensemble_screen_topk(C.byref(d), 1, K, p["theta"], p["X_init"], n_samples, 0, beta, num_starts,
                                     p["x0"], p["idx"], None, None)
    return rc, L.bore_last_error().decode()


def restarts(d, K, beta=1.0, num_starts=4, transform=1, lo=0.0, hi=1.0, null=(), **opts):
    o = dict(maxcor=10, maxiter=15000, maxfun=15000, maxls=20, ftol=2.22e-9, gtol=1e-5)
    o.update(opts)
    o = _lib.LbfgsbOpts(o["maxcor"], o["maxiter"], o["maxfun"], o["maxls"], o["ftol"], o["gtol"])
    n = max(d.input_dim, 1)
    lb, ub = (C.c_double * n)(*([lo] * n)), (C.c_double * n)(*([hi] * n))
    p = {k: (None if k in null else DUMMY) for k in ["theta", "x0", "x", "fun", "jac", "info"]}
    L = _lib.lib()
    rc = L.bore_ensemble_lbfgsb_minimize(C.byref(d), 1, K, p["theta"], beta, transform, 1, p["x0"], num_starts, lb, ub,
                                         C.byref(o), p["x"], p["fun"], p["jac"], p["info"], None)
    return rc, L.bore_last_error().decode()


@pytest.mark.parametrize("call,who", [(fg, "ensemble_value_and_input_grad"), (screen, "ensemble_screen_topk"),
                                      (restarts, "ensemble_lbfgsb_minimize")])
def test_entry_points_share_the_bounds(call, who):
    assert call(NARROW, 17) == (UNSUPPORTED, f"{who}: " + K_MSG % 17)
    assert call(NARROW, 0) == (UNSUPPORTED, f"{who}: " + K_MSG % 0)
    assert call(desc(2, [16, 16, 1], compute="bfloat16"), 4) == \
        (UNSUPPORTED, f"{who}: the ensemble kernels take compute = float32 members only")
    assert call(desc(2, [16, 16, 2]), 4) == (INVALID, f"{who}: the last Dense layer must have 1 unit")
    assert call(NARROW, 4, beta=-1.0) == (INVALID, f"{who}: beta must be finite and >= 0 (got -1)")
    rc, msg = call(PLUGIN, 16)
    assert rc == UNSUPPORTED and msg.startswith(f"{who}: 16 members' images (218112 B) plus the pass workspace")
    rc, msg = call(NARROW, 4, null=("theta",))
    assert rc == INVALID and "null pointer" in msg
    L = _lib.lib()
    batch = (C.c_int64 * 64)()                                   # (any non-null bore_batch: the refusal comes first)
    L.bore_set_batch(C.cast(batch, C.c_void_p))
    try:
        assert call(NARROW, 4) == (UNSUPPORTED, f"{who}: batch mode (bore_set_batch) takes no ensembles")
        assert "members" in call(NARROW, 17)[1]                 # (the bounds come before batch mode)
        # batch mode comes LAST: behind what is wrong with the entry point's own arguments
        assert "null pointer" in call(NARROW, 4, null=("theta",))[1]
        if call is fg:
            assert fg(NARROW, 4, transform=7)[1] == f"{who}: unknown transform 7"
            assert fg(NARROW, 4, n_rows=-1)[1] == f"{who}: n_rows < 0"
            assert "batch mode" in fg(NARROW, 4, n_rows=0)[1]
        elif call is screen:
            assert screen(NARROW, 4, n_samples=0)[1] == f"{who}: n_samples out of range"
            assert screen(NARROW, 4, num_starts=257)[1] == f"{who}: need 1 <= num_starts <= n_samples"
            assert "BORE_STREAM_MAX_SAMPLES = 16384" in screen(NARROW, 4, n_samples=16385)[1]
        else:
            assert restarts(NARROW, 4, maxcor=33)[1] == "lbfgsb_minimize: maxcor must be 1..32"
            assert restarts(NARROW, 4, lo=1.0, hi=0.0)[1].startswith("LBFGSB - one of the lower bounds")
            rc, msg = restarts(PLUGIN, 11, maxcor=32)             # (the restart slots' LDS: before batch mode too)
            assert rc == UNSUPPORTED and "restart slots" in msg
    finally:
        L.bore_set_batch(None)


def test_entry_points_own_arguments():
    assert fg(NARROW, 4, transform=7) == (INVALID, "ensemble_value_and_input_grad: unknown transform 7")
    assert fg(NARROW, 4, n_rows=-1) == (INVALID, "ensemble_value_and_input_grad: n_rows < 0")
    assert fg(NARROW, 4, n_rows=0)[0] == 0                                     # (nothing to do: no launch)
    assert screen(NARROW, 4, n_samples=0) == (INVALID, "ensemble_screen_topk: n_samples out of range")
    assert screen(NARROW, 4, num_starts=257) == (INVALID, "ensemble_screen_topk: need 1 <= num_starts <= n_samples")
    rc, msg = screen(NARROW, 4, n_samples=16385)
    assert rc == UNSUPPORTED and "BORE_STREAM_MAX_SAMPLES = 16384" in msg
    # the restarts: bore_lbfgsb_minimize's verdicts and texts
    assert restarts(NARROW, 4, num_starts=0) == (INVALID, "lbfgsb_minimize: num_starts < 1")
    assert restarts(NARROW, 4, maxcor=33) == (UNSUPPORTED, "lbfgsb_minimize: maxcor must be 1..32")
    assert restarts(NARROW, 4, maxls=0) == (INVALID, "lbfgsb_minimize: maxls must be positive.")
    assert restarts(NARROW, 4, lo=1.0, hi=0.0) == (INVALID, "LBFGSB - one of the lower bounds is greater than an upper bound.")
    assert restarts(desc(65, [16, 1]), 4) == (UNSUPPORTED, "lbfgsb_minimize: input_dim must be 1..64")
    assert restarts(NARROW, 4, null=("x0",)) == (INVALID, "lbfgsb_minimize: null pointer")


# ---- classes and plugins: arguments, no GPU ---------------------------------------------------------------------
def test_model_classes_validate_their_arguments():
    from bore_amd.models import (EnsembleDenseSequential, EnsembleSequential, MaximizableEnsembleDenseSequential,
                                 MaximizableEnsembleSequential)
    for K in (0, 17, 2.5, True, -1):
        with pytest.raises(ValueError, match="members"):
            EnsembleSequential(members=K)
    for beta in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta"):
            MaximizableEnsembleSequential("sigmoid", members=3, beta=beta)
    with pytest.raises(_lib.UnsupportedError, match="mixed_bfloat16"):
        EnsembleSequential(members=2, dtype_policy="mixed_bfloat16")
    with pytest.raises(ValueError, match="transform"):
        MaximizableEnsembleSequential("tanh", members=2)
    m = MaximizableEnsembleDenseSequential("sigmoid", 4, 1, 2, 8, layer_kws=dict(activation="elu"), members=3, beta=0.5,
                                           seed=1)
    assert (m.members, m.beta, len(m.layers), m._input_dim) == (3, 0.5, 4, 4)
    assert m.transform.name == "sigmoid" and m._func_min.transform.negate
    assert EnsembleDenseSequential(4, 1, 0, 8).members == 4 and MAX_MEMBERS == _lib.ENSEMBLE_MAX_MEMBERS == 16
    with pytest.raises(ValueError, match="member must be"):
        m._member(3)


def test_suggester_and_plugins_validate_ensemble():
    from bore_amd.models import MaximizableDenseSequential, MaximizableEnsembleDenseSequential
    from bore_amd.plugins.classifier import ClassifierSuggester
    from bore_amd.plugins.hpbandster import BORE, BOREHyperband
    from bore_amd.plugins.types import DenseSpace, UniformFloat
    box = (np.zeros(2), np.ones(2))
    from scipy.optimize import Bounds
    b = Bounds(*box)
    for K in (0, 17, 1.5):
        with pytest.raises(ValueError, match="members"):
            ClassifierSuggester(bounds=b, ensemble=K)
    with pytest.raises(ValueError, match="beta"):
        ClassifierSuggester(bounds=b, ensemble=4, beta=-1.0)
    s = ClassifierSuggester(bounds=b, ensemble=4, beta=2.0, weighting="lfbo", seed=0)
    assert (s.ensemble, s.beta, s.weighting) == (4, 2.0, "lfbo")
    net = s._build_compile_network()
    assert type(net) is MaximizableEnsembleDenseSequential and (net.members, net.beta) == (4, 2.0)
    plain = ClassifierSuggester(bounds=b, seed=0)
    assert plain.ensemble is None and type(plain._build_compile_network()) is MaximizableDenseSequential
    space = DenseSpace([UniformFloat("a", 0.0, 1.0), UniformFloat("b", 0.0, 1.0)], seed=0)
    bore = BORE(space, ensemble=3, beta=0.5, seed=0)
    assert (bore.config_generator._suggester.ensemble, bore.config_generator._suggester.beta) == (3, 0.5)
    assert BORE(space, seed=0).config_generator._suggester.ensemble is None
    with pytest.raises(_lib.UnsupportedError, match="ensemble=3"):
        BOREHyperband(space, ensemble=3)
