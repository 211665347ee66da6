"""The streamed flavour of the LSTM entry points without a GPU: which flavour takes which network
(bore_lstm_streamed), and that every bore_lstm_stream_* verdict is reached before any pointer is looked at and
before any HIP call -- with null data pointers an accepted shape answers BORE_E_INVALID ("null pointer"), a refused
one BORE_E_UNSUPPORTED with its bound by name."""
import ctypes
import os

import pytest

E_INVALID, E_UNSUPPORTED = -1, -2
LDS_SHAPES = [(40, 2, 32, 5), (16, 2, 32, 16)]                                       # (D, L, H, T)
STREAMED_SHAPES = [(48, 2, 32, 5), (2, 3, 32, 5), (2, 1, 64, 1), (16, 2, 64, 5), (33, 2, 32, 16)]
REFUSED = [((2, 1, 129, 5), "BORE_LSTM_STREAM_MAX_UNITS"), ((513, 1, 8, 5), "BORE_LSTM_STREAM_MAX_INPUT"),
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


def _streamed(lib, D, L, H, T):
    rc = lib.bore_lstm_streamed(ctypes.byref(_desc(D, L, H)), T)
    return rc, lib.bore_last_error().decode()


def _forward_verdict(lib, D, L, H, T):
    rc = lib.bore_lstm_stream_forward(ctypes.byref(_desc(D, L, H)), 1, None, None, 1, T, 0, 0.0, None, None)
    return rc, lib.bore_last_error().decode()


@pytest.mark.parametrize("shape", LDS_SHAPES)
def test_networks_the_lds_flavour_takes(built, shape):
    assert _streamed(built, *shape)[0] == 0


@pytest.mark.parametrize("shape", STREAMED_SHAPES)
def test_networks_only_the_streamed_flavour_takes(built, shape):
    from bore_amd import ops
    assert _streamed(built, *shape)[0] == 1
    D, L, H, T = shape
    assert ops.lstm_streamed(_desc(D, L, H), T) == 1
    # ... and the LDS entry point keeps refusing them, for capacity
    rc = built.bore_lstm_forward(ctypes.byref(_desc(D, L, H)), 1, None, None, 1, T, 0, 0.0, None, None)
    assert rc == E_UNSUPPORTED and "LDS" in built.bore_last_error().decode()


@pytest.mark.parametrize("shape,bound", REFUSED)
def test_networks_neither_flavour_takes_name_the_bound(built, shape, bound):
    from bore_amd import _lib, ops
    rc, msg = _streamed(built, *shape)
    assert rc == E_UNSUPPORTED and bound in msg, (rc, msg)
    D, L, H, T = shape
    with pytest.raises(_lib.UnsupportedError, match=bound):
        ops.lstm_streamed(_desc(D, L, H), T)


def test_streamed_query_refuses_a_bad_descriptor(built):
    rc, msg = _streamed(built, 0, 1, 8, 5)
    assert rc == E_INVALID and "input_dim" in msg
    assert built.bore_lstm_streamed(None, 5) == E_INVALID
    assert _streamed(built, 2, 1, 8, 0)[0] == E_INVALID


@pytest.mark.parametrize("shape", LDS_SHAPES + STREAMED_SHAPES)
def test_stream_forward_decides_before_it_looks_at_a_pointer(built, shape):
    rc, msg = _forward_verdict(built, *shape)
    assert rc == E_INVALID and "null pointer" in msg, (rc, msg)


@pytest.mark.parametrize("shape,bound", REFUSED)
def test_stream_forward_names_the_bound_it_refuses(built, shape, bound):
    rc, msg = _forward_verdict(built, *shape)
    assert rc == E_UNSUPPORTED and bound in msg, (rc, msg)


def test_stream_fit_refuses_batches_above_one_tile(built):
    from bore_amd import _lib
    one = ctypes.c_float(0.0)
    t = ctypes.c_int64(0)
    cfg = _lib.AdamCfg(1e-3, 0.9, 0.999, 1e-7)
    p = ctypes.cast(ctypes.byref(one), ctypes.c_void_p)     # never read: the verdict comes first
    rc = built.bore_lstm_stream_fit(ctypes.byref(_desc(48, 2, 32)), 1, p, p, p,
                                    ctypes.cast(ctypes.byref(t), ctypes.c_void_p), p, p, 100, 5, -1.0, 1, 65, None,
                                    ctypes.byref(cfg), None, None)
    msg = built.bore_last_error().decode()
    assert rc == E_UNSUPPORTED and "batch_size 65 > 64" in msg, (rc, msg)
