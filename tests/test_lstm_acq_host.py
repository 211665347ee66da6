"""The acquisition entry points of the streamed LSTM flavour without a GPU (bore_lstm_stream_screen_topk,
bore_lstm_stream_lbfgsb_minimize): both symbols exist and are declared, and with null device pointers every verdict
is reached in the documented order -- n_models and T, the streamed bounds by name, D <= BORE_DIM_MAX, the candidates
and the starts, the options and the box -- before "null pointer", the answer to an accepted request."""
import ctypes
import os
import re

import pytest

E_INVALID, E_UNSUPPORTED = -1, -2
NEW = ("bore_lstm_stream_screen_topk", "bore_lstm_stream_lbfgsb_minimize")
ACCEPTED = [(3, 1, 7, 4), (5, 2, 33, 3), (48, 2, 32, 5), (64, 4, 64, 16), (16, 2, 32, 5)]        # (D, L, H, T)
BEYOND = [((2, 1, 129, 5), "BORE_LSTM_STREAM_MAX_UNITS"), ((513, 1, 8, 5), "BORE_LSTM_STREAM_MAX_INPUT"),
          ((2, 1, 8, 17), "BORE_LSTM_MAX_STEPS")]


@pytest.fixture(scope="module")
def built():
    from bore_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_native()
    return _lib.lib()


def _desc(D, L, H):
    from bore_amd import _lib
    return _lib.make_lstm_desc(D, L, H, "elu")


def _screen(lib, D, L, H, T, n_models=1, n_samples=100, R=5):
    rc = lib.bore_lstm_stream_screen_topk(ctypes.byref(_desc(D, L, H)), n_models, None, None, n_samples, 0, T, R, None,
                                          None, None, None)
    return rc, lib.bore_last_error().decode()


def _restarts(lib, D, L, H, T, n_models=1, R=5, low=None, high=None, transform=0, **opts):
    from bore_amd import _lib
    o = dict(maxcor=10, maxiter=15000, maxfun=15000, maxls=20, ftol=2.2e-9, gtol=1e-5)
    o.update(opts)
    cfg = _lib.LbfgsbOpts(o["maxcor"], o["maxiter"], o["maxfun"], o["maxls"], o["ftol"], o["gtol"])
    lo = (ctypes.c_double * D)(*(low if low is not None else [0.0] * D))
    hi = (ctypes.c_double * D)(*(high if high is not None else [1.0] * D))
    rc = lib.bore_lstm_stream_lbfgsb_minimize(ctypes.byref(_desc(D, L, H)), n_models, None, T, transform, 1, None, R,
                                              lo, hi, ctypes.byref(cfg), None, None, None, None, None)
    return rc, lib.bore_last_error().decode()


def test_the_symbols_are_exported_and_declared(built):
    from bore_amd import _lib
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "bore_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert getattr(built, name) is not None
        assert re.search(r"\bint " + name + r"\(", header), name


@pytest.mark.parametrize("call", [_screen, _restarts])
@pytest.mark.parametrize("shape", ACCEPTED)
def test_an_accepted_request_answers_null_pointer(built, call, shape):
    rc, msg = call(built, *shape)
    assert rc == E_INVALID and "null pointer" in msg, (rc, msg)


@pytest.mark.parametrize("call", [_screen, _restarts])
@pytest.mark.parametrize("shape,bound", BEYOND)
def test_a_network_beyond_the_streamed_bounds_names_its_bound(built, call, shape, bound):
    # (with everything behind it wrong as well: the bound is what is reported)
    D = shape[0]
    kw = dict(n_samples=20000, R=0) if call is _screen else dict(R=0, low=[2.0] * D)
    rc, msg = call(built, *shape, **kw)
    assert rc == E_UNSUPPORTED and bound in msg, (rc, msg)


@pytest.mark.parametrize("call", [_screen, _restarts])
def test_sizes_come_first(built, call):
    rc, msg = call(built, 2, 1, 129, 5, n_models=0)
    assert rc == E_INVALID and "n_models" in msg, (rc, msg)
    rc, msg = call(built, 2, 1, 129, 0)                                # T = 0 in front of the bound on the units
    assert rc == E_INVALID and "at least one step" in msg, (rc, msg)
    rc, msg = call(built, 65, 1, 8, 17)                                # T = 17 in front of D = 65
    assert rc == E_UNSUPPORTED and "BORE_LSTM_MAX_STEPS" in msg, (rc, msg)


@pytest.mark.parametrize("call", [_screen, _restarts])
def test_more_than_64_inputs_names_dim_max(built, call):
    kw = dict(n_samples=20000) if call is _screen else dict(R=0)
    rc, msg = call(built, 65, 2, 32, 5, **kw)                          # (within the streamed bounds: 65 <= 512)
    assert rc == E_UNSUPPORTED and "BORE_DIM_MAX" in msg, (rc, msg)


def test_screening_candidates_and_starts(built):
    rc, msg = _screen(built, 48, 2, 32, 5, n_samples=16385, R=0)
    assert rc == E_UNSUPPORTED and "BORE_STREAM_MAX_SAMPLES" in msg, (rc, msg)
    assert _screen(built, 48, 2, 32, 5, n_samples=16384, R=5)[1].endswith("null pointer")
    rc, msg = _screen(built, 48, 2, 32, 5, n_samples=0)
    assert rc == E_INVALID and "n_samples" in msg, (rc, msg)
    for R in (101, 0, -1):
        rc, msg = _screen(built, 48, 2, 32, 5, n_samples=100, R=R)
        assert rc == E_INVALID and "1 <= num_starts <= n_samples" in msg, (R, rc, msg)
    assert _screen(built, 48, 2, 32, 5, n_samples=100, R=100)[1].endswith("null pointer")


def test_restarts_starts_options_and_box(built):
    rc, msg = _restarts(built, 48, 2, 32, 5, R=0, low=[2.0] * 48)
    assert rc == E_INVALID and "num_starts < 1" in msg, (rc, msg)
    rc, msg = _restarts(built, 48, 2, 32, 5, transform=99, low=[2.0] * 48)
    assert rc == E_INVALID and "unknown transform" in msg, (rc, msg)
    rc, msg = _restarts(built, 48, 2, 32, 5, maxcor=33, low=[2.0] * 48)
    assert rc == E_UNSUPPORTED and "maxcor" in msg, (rc, msg)
    rc, msg = _restarts(built, 48, 2, 32, 5, maxls=0)
    assert rc == E_INVALID and "maxls" in msg, (rc, msg)
    rc, msg = _restarts(built, 3, 1, 7, 4, low=[0.0, 0.5, 0.0], high=[1.0, 0.25, 1.0])      # low > high
    assert rc == E_INVALID and "lower bounds" in msg, (rc, msg)
    inf = float("inf")
    rc, msg = _restarts(built, 3, 1, 7, 4, low=[-inf, 0.0, 5.0], high=[inf, inf, -inf])     # open sides bind nothing
    assert rc == E_INVALID and msg.endswith("null pointer"), (rc, msg)
