"""The host side of bore_lbfgsb_minimize, bore_screen_topk and bore_sample_screen_topk (no GPU): status code and message
of every refusal that comes back before a launch, and which one wins for a request that is wrong in two ways.  Raw
ctypes with dummy non-null pointers (nothing is ever dereferenced on the device; the bounds, which the host reads, are
real arrays)."""
import ctypes as C

import pytest

from bore_amd import _lib

DUMMY = C.c_void_p(0x1000)
INVALID, UNSUPPORTED = -1, -2
STREAMED = ("this entry point keeps the whole network in LDS -- forward, evaluate, value + input gradient and fit stream "
            "such float32 networks from global memory, the bore_stream_* entry points screen and restart on them, and "
            "what those refuse the model API runs through the lock-step L-BFGS-B around the streamed kernels")
BF16_SHAPES = ("compute = bfloat16 is available for the wide static shapes only (16->64-64-64-1, "
               "32->128-128-1; any activations, no l2)")
TWO_UNITS_L = "lbfgsb_minimize: the last Dense layer must have 1 unit"
TWO_UNITS_S = "screen_topk: the last Dense layer must have 1 unit"
BOUNDS = "LBFGSB - one of the lower bounds is greater than an upper bound."


def desc(D, units, compute="float32"):
    return _lib.make_desc(D, units, ["relu"] * (len(units) - 1) + ["sigmoid"], compute=compute)


NARROW = desc(2, [16, 16, 1])
TWO_OUT = desc(2, [16, 16, 2])
NARROW_BF16 = desc(2, [16, 16, 1], compute="bfloat16")
TOO_LARGE = desc(8, [176, 176, 1])     # (the network fits the LDS; one problem's workspace beside it does not)
L_POINTERS = ["desc", "theta", "x0", "lb", "ub", "opts", "x", "fun", "jac", "info"]


def box(D, lo=0.0, hi=1.0):
    return (C.c_double * max(D, 1))(*([lo] * max(D, 1))), (C.c_double * max(D, 1))(*([hi] * max(D, 1)))


def restarts(d, n_models=1, num_starts=4, transform=1, null=(), lo=0.0, hi=1.0, **opts):
    """bore_lbfgsb_minimize on dummy pointers, those named in `null` being NULL; returns (status, message)."""
    o = dict(maxcor=10, maxiter=15000, maxfun=15000, maxls=20, ftol=2.22e-9, gtol=1e-5)
    o.update(opts)
    o = _lib.LbfgsbOpts(o["maxcor"], o["maxiter"], o["maxfun"], o["maxls"], o["ftol"], o["gtol"])
    lb, ub = box(d.input_dim, lo, hi)
    p = {k: (None if k in null else DUMMY) for k in L_POINTERS}
    L = _lib.lib()
    rc = L.bore_lbfgsb_minimize(None if "desc" in null else C.byref(d), n_models, p["theta"], transform, 1, p["x0"],
                                num_starts, None if "lb" in null else lb, None if "ub" in null else ub,
                                None if "opts" in null else C.byref(o), p["x"], p["fun"], p["jac"], p["info"], None)
    return rc, L.bore_last_error().decode()


def screen(d, n_models=1, n_samples=256, num_starts=4, sampled=False, null=()):
    """bore_screen_topk (sampled: bore_sample_screen_topk) on dummy pointers; returns (status, message)."""
    p = {k: (None if k in null else DUMMY) for k in ["theta", "X_init", "x0", "idx", "pred"]}
    L = _lib.lib()
    if sampled:
        low, high = box(d.input_dim)
        rc = L.bore_sample_screen_topk(C.byref(d), n_models, p["theta"], 7, 0, 0, n_samples,
                                       None if "low" in null else low, None if "high" in null else high, num_starts,
                                       p["x0"], p["idx"], p["pred"], None)
    else:
        rc = L.bore_screen_topk(C.byref(d), n_models, p["theta"], p["X_init"], n_samples, 0, num_starts, p["x0"],
                                p["idx"], p["pred"], None)
    return rc, L.bore_last_error().decode()


@pytest.fixture
def batch_mode():
    """Batch mode with an all-zero bore_batch: set, but incomplete."""
    L = _lib.lib()
    batch = (C.c_int64 * 64)()
    L.bore_set_batch(C.cast(batch, C.c_void_p))
    yield
    L.bore_set_batch(None)


# ---- bore_lbfgsb_minimize -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", L_POINTERS)
def test_restarts_null_pointer(which):
    assert restarts(NARROW, null=(which,)) == (INVALID, "lbfgsb_minimize: null pointer")


def test_restarts_no_models():
    assert restarts(NARROW, n_models=0) == (INVALID, "n_models must be >= 1 (got 0)")


@pytest.mark.parametrize("D", [0, 65])
def test_restarts_input_dim_out_of_range(D):
    assert restarts(desc(D, [16, 16, 1])) == (UNSUPPORTED, "lbfgsb_minimize: input_dim must be 1..64")


def test_restarts_no_starts():
    assert restarts(NARROW, num_starts=0) == (INVALID, "lbfgsb_minimize: num_starts < 1")


def test_restarts_unknown_transform():
    assert restarts(NARROW, transform=3) == (INVALID, "lbfgsb_minimize: unknown transform 3")
    assert restarts(NARROW, transform=-1) == (INVALID, "lbfgsb_minimize: unknown transform -1")


@pytest.mark.parametrize("maxcor", [0, 33])
def test_restarts_maxcor_out_of_range(maxcor):
    assert restarts(NARROW, maxcor=maxcor) == (UNSUPPORTED, "lbfgsb_minimize: maxcor must be 1..32")


def test_restarts_maxls_zero():
    assert restarts(NARROW, maxls=0) == (INVALID, "lbfgsb_minimize: maxls must be positive.")


@pytest.mark.parametrize("opt", [dict(maxiter=-1), dict(maxfun=-1), dict(ftol=-1e-9)])
def test_restarts_negative_limit(opt):
    assert restarts(NARROW, **opt) == (INVALID, "lbfgsb_minimize: negative limit/tolerance")


def test_restarts_lower_bound_above_upper():
    assert restarts(NARROW, lo=1.0, hi=0.0) == (INVALID, BOUNDS)


def test_restarts_two_output_units():
    assert restarts(TWO_OUT) == (INVALID, TWO_UNITS_L)


def test_restarts_bfloat16_on_a_narrow_shape():
    assert restarts(NARROW_BF16) == (UNSUPPORTED, BF16_SHAPES)


def test_restarts_problem_state_does_not_fit():
    assert restarts(TOO_LARGE, maxcor=32) == (
        UNSUPPORTED, "lbfgsb_minimize: one problem's state does not fit in LDS beside the network; " + STREAMED)


def test_restarts_too_many_blocks(monkeypatch):
    """More than 65 535 workgroups per model: beyond the grid of the one-problem-per-wave mapping (2^22 workgroups)
    by size alone, and within it when BORE_LBFGSB_QUEUE = 0 keeps one workgroup per four restarts."""
    assert restarts(NARROW, num_starts=(1 << 24) + 4) == (UNSUPPORTED, "lbfgsb_minimize: too many restarts")
    monkeypatch.setenv("BORE_LBFGSB_QUEUE", "0")
    assert restarts(NARROW, num_starts=4 * 65536) == (UNSUPPORTED, "lbfgsb_minimize: too many restarts")


def test_restarts_batch_mode_with_17_starts(batch_mode):
    assert restarts(NARROW, num_starts=17) == (
        UNSUPPORTED, "lbfgsb_minimize: batch mode needs num_starts <= 16 in one workgroup")


def test_restarts_batch_mode_with_an_incomplete_batch(batch_mode):
    assert restarts(NARROW, num_starts=4) == (INVALID, "lbfgsb_minimize: incomplete bore_batch")
    assert restarts(NARROW, num_starts=16) == (INVALID, "lbfgsb_minimize: incomplete bore_batch")


# ---- bore_screen_topk, bore_sample_screen_topk --------------------------------------------------------------------
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("which", ["theta", "x0", "idx"])
def test_screen_null_pointer(which, sampled):
    assert screen(NARROW, null=(which,), sampled=sampled) == (INVALID, "screen_topk: null pointer")


def test_screen_null_candidates():
    assert screen(NARROW, null=("X_init",)) == (INVALID, "screen_topk: null pointer")


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("n_samples", [0, (1 << 20) + 1])
def test_screen_samples_out_of_range(n_samples, sampled):
    assert screen(NARROW, n_samples=n_samples, sampled=sampled) == (INVALID, "screen_topk: n_samples out of range")


@pytest.mark.parametrize("num_starts", [0, 257])
def test_screen_starts_out_of_range(num_starts):
    assert screen(NARROW, num_starts=num_starts) == (INVALID, "screen_topk: need 1 <= num_starts <= n_samples")


def test_screen_no_models():
    assert screen(NARROW, n_models=0) == (INVALID, "n_models must be >= 1 (got 0)")


def test_screen_input_dim_zero():
    assert screen(desc(0, [16, 16, 1])) == (INVALID, "bad bore_mlp_desc")


def test_screen_two_output_units():
    assert screen(TWO_OUT) == (INVALID, TWO_UNITS_S)


def test_screen_bfloat16_on_a_narrow_shape():
    assert screen(NARROW_BF16) == (UNSUPPORTED, BF16_SHAPES)
    assert screen(NARROW_BF16, sampled=True) == (UNSUPPORTED, BF16_SHAPES)


def test_screen_network_does_not_fit():
    rc, msg = screen(desc(8, [256, 256, 1]))
    assert rc == UNSUPPORTED
    assert msg == "model needs 340436 B of LDS per workgroup (> 163840) at 16 rows per tile; " + STREAMED


@pytest.mark.parametrize("which", ["low", "high"])
def test_sampled_screen_null_bounds(which):
    assert screen(NARROW, sampled=True, null=(which,)) == (INVALID, "sample_screen_topk: null bounds")


def test_sampled_screen_input_dim_beyond_the_box():
    assert screen(desc(65, [16, 16, 1]), sampled=True) == (UNSUPPORTED, "sample_screen_topk: D must be 1..64")


def test_screen_batch_mode_takes_the_sampled_form_only(batch_mode):
    assert screen(NARROW) == (INVALID, "screen_topk: batch mode needs the sampled form")


# ---- two faults at once ---------------------------------------------------------------------------------------------
def test_which_fault_wins(monkeypatch):
    """The checks in the order a request meets them.  Restarts: pointers, n_models, the input dimension, num_starts, the
    transform, the options, the box -- then what the planning finds: a problem that does not fit, the output layer,
    batch mode's limits, the grid, the kernel.  Screening: n_samples, num_starts, n_models and the network's capacity,
    the output layer, pointers, batch mode, the sampled form's box -- then the kernel."""
    assert restarts(NARROW, null=("jac",), n_models=0) == (INVALID, "lbfgsb_minimize: null pointer")
    assert restarts(desc(0, [16, 16, 1]), n_models=0) == (INVALID, "n_models must be >= 1 (got 0)")
    assert restarts(desc(65, [16, 16, 1]), num_starts=0) == (UNSUPPORTED, "lbfgsb_minimize: input_dim must be 1..64")
    assert restarts(NARROW, num_starts=0, transform=7) == (INVALID, "lbfgsb_minimize: num_starts < 1")
    assert restarts(NARROW, transform=7, maxcor=0) == (INVALID, "lbfgsb_minimize: unknown transform 7")
    assert restarts(NARROW, maxcor=33, maxls=0) == (UNSUPPORTED, "lbfgsb_minimize: maxcor must be 1..32")
    assert restarts(NARROW, maxls=0, maxiter=-1) == (INVALID, "lbfgsb_minimize: maxls must be positive.")
    assert restarts(NARROW, maxfun=-1, lo=1.0, hi=0.0) == (INVALID, "lbfgsb_minimize: negative limit/tolerance")
    # late refusals -- the carve, the output layer, the grid, the kernel -- against an earlier argument fault
    assert restarts(TOO_LARGE, maxcor=32, lo=1.0, hi=0.0) == (INVALID, BOUNDS)
    assert restarts(TWO_OUT, lo=1.0, hi=0.0) == (INVALID, BOUNDS)
    assert restarts(TWO_OUT, maxcor=33) == (UNSUPPORTED, "lbfgsb_minimize: maxcor must be 1..32")
    assert restarts(NARROW, num_starts=(1 << 24) + 4, null=("info",)) == (INVALID, "lbfgsb_minimize: null pointer")
    assert restarts(NARROW_BF16, transform=7) == (INVALID, "lbfgsb_minimize: unknown transform 7")
    # among the late ones: the output layer before the grid, the grid before the kernel
    assert restarts(TWO_OUT, num_starts=(1 << 24) + 4) == (INVALID, TWO_UNITS_L)
    assert restarts(desc(2, [16, 16, 2], compute="bfloat16")) == (INVALID, TWO_UNITS_L)
    assert restarts(NARROW_BF16, num_starts=(1 << 24) + 4) == (UNSUPPORTED, "lbfgsb_minimize: too many restarts")

    assert screen(NARROW, n_samples=0, num_starts=0) == (INVALID, "screen_topk: n_samples out of range")
    assert screen(NARROW, num_starts=300, n_models=0) == (INVALID, "screen_topk: need 1 <= num_starts <= n_samples")
    assert screen(NARROW, n_models=0, null=("theta",)) == (INVALID, "n_models must be >= 1 (got 0)")
    assert screen(TWO_OUT, null=("idx",)) == (INVALID, TWO_UNITS_S)
    assert screen(NARROW, null=("X_init",), n_samples=0) == (INVALID, "screen_topk: null pointer")
    assert screen(desc(65, [16, 16, 1]), sampled=True, null=("low",)) == (UNSUPPORTED, "sample_screen_topk: D must be 1..64")
    assert screen(desc(65, [16, 16, 1]), sampled=True, null=("x0",)) == (INVALID, "screen_topk: null pointer")
    assert screen(NARROW_BF16, null=("idx",)) == (INVALID, "screen_topk: null pointer")
    assert screen(NARROW_BF16, sampled=True, null=("high",)) == (INVALID, "sample_screen_topk: null bounds")


def test_which_fault_wins_in_batch_mode(batch_mode):
    assert restarts(TWO_OUT, num_starts=17) == (INVALID, TWO_UNITS_L)
    assert restarts(NARROW, num_starts=17, lo=1.0, hi=0.0) == (INVALID, BOUNDS)
    assert restarts(NARROW_BF16, num_starts=17) == (
        UNSUPPORTED, "lbfgsb_minimize: batch mode needs num_starts <= 16 in one workgroup")
    assert restarts(NARROW_BF16, num_starts=4) == (INVALID, "lbfgsb_minimize: incomplete bore_batch")
    assert screen(NARROW, null=("theta",)) == (INVALID, "screen_topk: null pointer")
    assert screen(TWO_OUT) == (INVALID, TWO_UNITS_S)
    assert screen(NARROW, n_samples=0) == (INVALID, "screen_topk: n_samples out of range")
