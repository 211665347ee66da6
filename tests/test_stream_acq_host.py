"""Screening and restarts for streamed networks, host side (no GPU): the three C-ABI symbols, their
declarations, and the refusals that come back before any HIP call -- each naming its bound."""
import ctypes as C
import re

import numpy as np
import pytest

from bore_amd import _lib, ops

NEW = {"bore_stream_screen_topk": "bore_screen_topk",
       "bore_stream_sample_screen_topk": "bore_sample_screen_topk",
       "bore_stream_lbfgsb_minimize": "bore_lbfgsb_minimize"}


def desc(D, units, compute="float32"):
    return _lib.make_desc(D, units, ["relu"] * (len(units) - 1) + ["linear"], compute=compute)


def declaration(header, name):
    """The parameter list of `name` in the header, white space squeezed."""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_symbols_are_exported_declared_and_built():
    with open(_lib.HEADER) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for new, old in NEW.items():
        assert new in _lib.EXPORTS
        assert declaration(header, new) == declaration(header, old)       # the documented signatures: their counterparts'
        assert hasattr(raw, new)
        assert getattr(_lib.lib(), new).argtypes == getattr(_lib.lib(), old).argtypes
    assert re.search(r"#define\s+BORE_STREAM_MAX_SAMPLES\s+16384\b", header)
    assert _lib.STREAM_MAX_SAMPLES == 16384
    assert _lib.abi_version_of_header() == 12                              # additive
    assert _lib.lib().bore_abi_version() == 12


# ---- refusals before any HIP call: raw ctypes, dummy non-null pointers (nothing is ever dereferenced on the device) ----
DUMMY = C.c_void_p(0x1000)


def restarts(d, D, maxcor=10, n_models=1, num_starts=2):
    box = (C.c_double * D)(*([0.0] * D)), (C.c_double * D)(*([1.0] * D))
    opts = _lib.LbfgsbOpts(maxcor, 1000, 15000, 20, 1e-9, 1e-5)
    return _lib.lib().bore_stream_lbfgsb_minimize(C.byref(d), n_models, DUMMY, 0, 1, DUMMY, num_starts, box[0], box[1],
                                                  C.byref(opts), DUMMY, DUMMY, DUMMY, DUMMY, None)


def screen(d, n_samples=64, num_starts=3):
    return _lib.lib().bore_stream_screen_topk(C.byref(d), 1, DUMMY, DUMMY, n_samples, 0, num_starts, DUMMY, DUMMY, None,
                                              None)


def sample_screen(d, D, n_samples=64, num_starts=3):
    box = (C.c_double * D)(*([0.0] * D)), (C.c_double * D)(*([1.0] * D))
    return _lib.lib().bore_stream_sample_screen_topk(C.byref(d), 1, DUMMY, 7, 0, 0, n_samples, box[0], box[1], num_starts,
                                                     DUMMY, DUMMY, None, None)


def refused(rc, code, pattern):
    assert rc == code, (rc, _lib.lib().bore_last_error())
    with pytest.raises(_lib.UnsupportedError if code == -2 else RuntimeError, match=pattern):
        _lib.check(rc)


def test_more_than_64_inputs_names_the_bound():
    d = desc(65, [256, 256, 1])
    refused(restarts(d, 65), -2, "BORE_DIM_MAX")
    refused(sample_screen(d, 65), -2, "BORE_DIM_MAX")


@pytest.mark.parametrize("maxcor", [0, 33])
def test_maxcor_outside_1_to_32(maxcor):
    refused(restarts(desc(8, [256, 256, 1]), 8, maxcor=maxcor), -2, r"maxcor must be 1\.\.32")


def test_bfloat16_is_refused_by_all_three():
    d = desc(8, [256, 256, 1], compute="bfloat16")
    refused(restarts(d, 8), -2, "bfloat16")
    refused(screen(d), -2, "bfloat16")
    refused(sample_screen(d, 8), -2, "bfloat16")


def test_a_width_of_513_names_the_bound():
    d = desc(8, [513, 513, 1])
    refused(restarts(d, 8), -2, "BORE_STREAM_MAX_UNITS")
    refused(screen(d), -2, "BORE_STREAM_MAX_UNITS")
    refused(sample_screen(d, 8), -2, "BORE_STREAM_MAX_UNITS")


def test_more_starts_than_samples():
    d = desc(8, [256, 256, 1])
    refused(screen(d, n_samples=4, num_starts=5), -1, "num_starts")
    refused(sample_screen(d, 8, n_samples=4, num_starts=5), -1, "num_starts")


def test_more_samples_than_one_workgroup_ranks_names_the_bound():
    refused(screen(desc(8, [256, 256, 1]), n_samples=16385), -2, "BORE_STREAM_MAX_SAMPLES")


def test_batch_mode_is_refused():
    L = _lib.lib()
    batch = np.zeros(64, dtype=np.int64)              # (any non-null bore_batch: the refusal comes first)
    L.bore_set_batch(batch.ctypes.data_as(C.c_void_p))
    try:
        refused(restarts(desc(8, [256, 256, 1]), 8), -2, "batch mode")
        refused(screen(desc(8, [256, 256, 1])), -2, "batch mode")
    finally:
        L.bore_set_batch(None)


def test_the_streamed_query_is_unchanged():
    assert ops.mlp_streamed(desc(2, [16, 16, 1])) == 0
    assert ops.mlp_streamed(desc(8, [256, 256, 1])) == 7
