"""bore_mlp_fit's host side (no GPU): status code and message of every refusal that comes back before any HIP call,
and which one wins for a request that is wrong in two ways.  Raw ctypes with dummy non-null pointers (nothing is
ever dereferenced on the device)."""
import ctypes as C

import pytest

from bore_amd import _lib

DUMMY = C.c_void_p(0x1000)
POINTERS = ["theta", "adam_m", "adam_v", "adam_t", "X", "z", "adam"]
INVALID, UNSUPPORTED, NEEDS_PERM = -1, -2, -5


def desc(D, units, out="sigmoid", compute="float32"):
    return _lib.make_desc(D, units, ["relu"] * (len(units) - 1) + [out], compute=compute)


def fit(d, n_models=1, N=40, epochs=1, batch_size=64, perm=None, null=()):
    """bore_mlp_fit on dummy pointers, those named in `null` being NULL; returns (status, message)."""
    adam = _lib.AdamCfg(1e-3, 0.9, 0.999, 1e-7)
    p = {k: (None if k in null else DUMMY) for k in POINTERS}
    L = _lib.lib()
    rc = L.bore_mlp_fit(C.byref(d), n_models, p["theta"], p["adam_m"], p["adam_v"], p["adam_t"], p["X"], p["z"], N,
                        epochs, batch_size, perm, 0, 0, 0, None if "adam" in null else C.byref(adam), None, None)
    return rc, L.bore_last_error().decode()


NARROW = desc(2, [16, 16, 1])


def test_batch_size_zero():
    assert fit(NARROW, batch_size=0) == (INVALID, "fit: batch_size must be positive (got 0)")


@pytest.mark.parametrize("N", [0, (1 << 24) + 1])
def test_rows_out_of_range(N):
    assert fit(NARROW, N=N) == (INVALID, "fit: N=%d out of range" % N)


def test_no_models():
    assert fit(NARROW, n_models=0) == (INVALID, "n_models must be >= 1 (got 0)")


def test_two_output_units():
    assert fit(desc(2, [16, 16, 2])) == (INVALID, "fit: the last Dense layer must have 1 unit (binary classifier)")


def test_relu_output_layer():
    assert fit(desc(2, [16, 16, 1], out="relu")) == (
        INVALID, "fit: BCE needs a sigmoid or linear (from_logits) output layer")


@pytest.mark.parametrize("which", POINTERS)
def test_null_pointer(which):
    assert fit(NARROW, null=(which,)) == (INVALID, "fit: null pointer")


def test_negative_epochs():
    assert fit(NARROW, epochs=-1) == (INVALID, "fit: epochs < 0")


def test_zero_epochs_is_done_without_a_launch():
    assert fit(NARROW, epochs=0)[0] == 0
    assert fit(desc(5, [24, 12, 1]), epochs=0)[0] == 0          # (a run-time layout)


def test_bfloat16_on_a_shape_that_is_not_wide():
    rc, msg = fit(desc(2, [16, 16, 1], compute="bfloat16"))
    assert rc == UNSUPPORTED
    assert msg == ("compute = bfloat16 is available for the wide static shapes only (16->64-64-64-1, "
                   "32->128-128-1; any activations, no l2)")


def test_bfloat16_with_32_row_batches():
    assert fit(desc(32, [128, 128, 1], compute="bfloat16"), batch_size=32) == (
        UNSUPPORTED, "fit_bf16: batch_size must be 64 (got 32)")


def test_bfloat16_checks_come_in_their_own_order():
    wide = desc(32, [128, 128, 1], compute="bfloat16")
    assert fit(wide, N=0, epochs=-1) == (INVALID, "fit_bf16: N=0 out of range")
    assert fit(wide, epochs=-1, n_models=0) == (INVALID, "fit_bf16: epochs < 0")
    assert fit(wide, null=("z",)) == (INVALID, "fit_bf16: null pointer")
    assert fit(wide, epochs=0)[0] == 0


@pytest.mark.parametrize("d,most", [(NARROW, 10421), (desc(5, [24, 12, 1]), 9722)])
def test_a_drawn_shuffle_that_does_not_fit_asks_for_perm(d, most):
    """The first N past what the LDS holds beside the network (the last N that fits would launch)."""
    rc, msg = fit(d, N=most + 1)
    assert rc == NEEDS_PERM
    assert msg == ("fit: N=%d rows exceed what one workgroup's LDS holds beside this network when the epoch's shuffle "
                   "is drawn on the device (at most %d rows): pass explicit shuffles (`perm`, e.g. from "
                   "bore_amd.shuffle.permutations) -- any N then" % (most + 1, most))
    with pytest.raises(_lib.NeedsPermError):
        _lib.check(rc)


def test_which_fault_wins():
    """The checks in the order a request meets them: sizes, the network's capacity, the shuffle's, the output layer,
    the pointers, epochs -- and only then a carve that does not fit."""
    assert fit(NARROW, batch_size=0, null=("theta",)) == (INVALID, "fit: batch_size must be positive (got 0)")
    assert fit(NARROW, batch_size=0, N=0) == (INVALID, "fit: batch_size must be positive (got 0)")
    assert fit(NARROW, N=0, n_models=0) == (INVALID, "fit: N=0 out of range")
    assert fit(NARROW, n_models=0, null=("X",)) == (INVALID, "n_models must be >= 1 (got 0)")
    assert fit(NARROW, N=10422, null=("X",))[0] == NEEDS_PERM
    assert fit(desc(2, [16, 16, 2], out="relu")) == (
        INVALID, "fit: the last Dense layer must have 1 unit (binary classifier)")
    assert fit(desc(2, [16, 16, 1], out="relu"), null=("adam",)) == (
        INVALID, "fit: BCE needs a sigmoid or linear (from_logits) output layer")
    assert fit(NARROW, epochs=-1, null=("adam_t",)) == (INVALID, "fit: null pointer")
    # 16->64-64-64-1 with 128-row batches: the network and the shuffle fit, the carve with the gradient sums between
    # sub-tiles does not -- reported after the request's own faults
    assert fit(desc(16, [64, 64, 64, 1]), batch_size=128, null=("theta",)) == (INVALID, "fit: null pointer")
    assert fit(desc(16, [64, 64, 64, 1]), batch_size=128, epochs=-1) == (INVALID, "fit: epochs < 0")
    assert fit(desc(16, [64, 64, 64, 1]), batch_size=128, epochs=0)[0] == 0


def test_a_net_that_would_be_fitted_zero_padded_gets_the_same_answers():
    """4->32-32-1 runs on 6->32-32-1's static kernels through a repacked copy: not before its request is in order."""
    assert fit(desc(4, [32, 32, 1]), null=("theta",)) == (INVALID, "fit: null pointer")
    assert fit(desc(4, [32, 32, 1]), epochs=-1) == (INVALID, "fit: epochs < 0")
    assert fit(desc(4, [32, 32, 1]), epochs=0)[0] == 0
    assert fit(desc(4, [32, 32, 1]), N=0) == (INVALID, "fit: N=0 out of range")
    assert fit(desc(4, [32, 32, 1]), n_models=0) == (INVALID, "n_models must be >= 1 (got 0)")
    assert fit(desc(4, [32, 32, 1], out="relu")) == (
        INVALID, "fit: BCE needs a sigmoid or linear (from_logits) output layer")


def test_batch_mode_takes_no_perm_and_no_bfloat16():
    L = _lib.lib()
    batch = (C.c_int64 * 64)()                                   # (any non-null bore_batch: the refusals come first)
    L.bore_set_batch(C.cast(batch, C.c_void_p))
    try:
        assert fit(NARROW, perm=DUMMY) == (INVALID, "fit: no perm / epoch_loss in batch mode")
        assert fit(desc(32, [128, 128, 1], compute="bfloat16")) == (UNSUPPORTED, "fit: batch mode is float32 only")
    finally:
        L.bore_set_batch(None)


def test_the_streamed_query_leaves_no_error_behind():
    L = _lib.lib()
    fit(NARROW, batch_size=0)                                    # (something in bore_last_error)
    assert L.bore_mlp_streamed(C.byref(desc(8, [256, 256, 1]))) == 7
    assert L.bore_last_error() == b""
    fit(NARROW, batch_size=0)
    assert L.bore_mlp_streamed(C.byref(NARROW)) == 0
    assert L.bore_last_error() == b""
