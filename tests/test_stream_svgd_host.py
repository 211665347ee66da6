"""SVGD batch acquisition for streamed networks, host side (no GPU): the C-ABI symbol, its declaration, and the
refusals that come back before any HIP call -- each naming its bound."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from bore_amd import _lib, ops

NEW, OLD = "bore_stream_svgd_optimize", "bore_svgd_optimize"


def desc(D, units, compute="float32"):
    return _lib.make_desc(D, units, ["relu"] * (len(units) - 1) + ["linear"], compute=compute)


def declaration(header, name):
    """The parameter list of `name` in the header, white space squeezed."""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_symbol_is_exported_declared_and_built():
    with open(_lib.HEADER) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert NEW in _lib.EXPORTS
    assert declaration(header, NEW) == declaration(header, OLD)
    assert header.index("bore_stream_lbfgsb_minimize") < header.index(NEW)
    assert hasattr(C.CDLL(_lib.LIB_PATH), NEW)
    assert getattr(_lib.lib(), NEW).argtypes == getattr(_lib.lib(), OLD).argtypes
    assert getattr(_lib.lib(), NEW).restype is C.c_int
    assert _lib.abi_version_of_header() == 12                              # additive
    assert _lib.lib().bore_abi_version() == 12


# ---- refusals before any HIP call: raw ctypes, dummy non-null pointers (nothing is ever dereferenced on the device) ----
DUMMY = C.c_void_p(0x1000)


def svgd(d, D, n=8, n_models=1, distortion=0, lb=True, ub=True, n_iter=10):
    box = (C.c_double * D)(*([0.0] * D)), (C.c_double * D)(*([1.0] * D))
    opts = _lib.SvgdOpts(n_iter, distortion, 1e-2, .9, 1e-6, 1., -1., 1.)
    return _lib.lib().bore_stream_svgd_optimize(C.byref(d), n_models, DUMMY, 1, DUMMY, n, box[0] if lb else None,
                                                box[1] if ub else None, C.byref(opts), DUMMY, None)


def refused(rc, code, pattern):
    assert rc == code, (rc, _lib.lib().bore_last_error())
    with pytest.raises(_lib.UnsupportedError if code == -2 else RuntimeError, match=pattern):
        _lib.check(rc)


def test_bfloat16_is_refused():
    refused(svgd(desc(8, [256, 256, 1], compute="bfloat16"), 8), -2, "bfloat16")
    refused(svgd(desc(32, [128, 128, 1], compute="bfloat16"), 32), -2, "bfloat16")   # (a shape the LDS form takes)


def test_more_than_64_inputs_names_the_bound():
    refused(svgd(desc(65, [256, 256, 1]), 65), -2, "BORE_DIM_MAX")


def test_a_width_of_513_names_the_bound():
    refused(svgd(desc(8, [513, 513, 1]), 8), -2, "BORE_STREAM_MAX_UNITS")


def test_a_last_layer_of_two_units():
    refused(svgd(desc(8, [256, 256, 2]), 8), -1, "last Dense layer must have 1 unit")


@pytest.mark.parametrize("n", [0, 4097])
def test_particles_outside_1_to_4096(n):
    refused(svgd(desc(8, [256, 256, 1]), 8, n=n), -2, r"1\.\.4096 particles")


def test_lb_without_ub():
    refused(svgd(desc(8, [256, 256, 1]), 8, ub=False), -1, "lb and ub go together")
    refused(svgd(desc(8, [256, 256, 1]), 8, lb=False), -1, "lb and ub go together")


def test_bad_options():
    refused(svgd(desc(8, [256, 256, 1]), 8, distortion=2), -1, "bad options")
    refused(svgd(desc(8, [256, 256, 1]), 8, n_iter=-1), -1, "bad options")


def test_particle_state_too_large_for_lds_names_n_D_and_the_bytes():
    # 4 x 4096 x 8 doubles of state alone are 1 MiB
    need = 4 * 8 * 4096 * 8 + 16 * 4096
    rc = svgd(desc(8, [256, 256, 1]), 8, n=4096)
    refused(rc, -2, r"4096 particles in 8 dimensions need \d+ B of LDS")
    said = int(re.search(rb"need (\d+) B of LDS", _lib.lib().bore_last_error()).group(1))
    assert need < said < need + 64 * 1024                                # (+ the panels and the select's scratch)
    # the first request that does not fit at D = 8: 272 bytes a particle, 1 KiB of select scratch and 16 bytes of
    # alignment beside the 55080 + 64 bytes of the panels, in 160 KiB
    room = 160 * 1024 - 55080 - 64 - 16 - 4 * (256 + 8)
    n = room // (32 * 8 + 16) + 1
    refused(svgd(desc(8, [256, 256, 1]), 8, n=n), -2, rf"{n} particles in 8 dimensions need \d+ B of LDS")
    refused(svgd(desc(2, [16, 16, 1]), 2, n=4096), -2, "LDS")              # (a network that fits LDS: the same bound)


def test_more_workspace_than_a_call_allows_itself_is_refused_not_walked():
    d = desc(8, [512] * 7 + [1])
    tile = 2 * 64 * (8 + 7 * 512 + 1) * 4
    assert 64 * tile > (64 << 20) >= 36 * tile
    refused(svgd(d, 8, n_models=64), -2, "STREAM_WS_BYTES")
    refused(svgd(d, 8, n_models=64), -2, "64 MiB")


def test_batch_mode_is_refused():
    L = _lib.lib()
    batch = np.zeros(64, dtype=np.int64)              # (any non-null bore_batch: the refusal comes first)
    L.bore_set_batch(batch.ctypes.data_as(C.c_void_p))
    try:
        refused(svgd(desc(8, [256, 256, 1]), 8), -2, "batch mode")
    finally:
        L.bore_set_batch(None)


def test_null_pointers():
    d = desc(8, [256, 256, 1])
    opts = _lib.SvgdOpts(1, 0, 1e-2, .9, 1e-6, 1., -1., 1.)
    L = _lib.lib()
    assert L.bore_stream_svgd_optimize(C.byref(d), 1, DUMMY, 0, None, 8, None, None, C.byref(opts), DUMMY, None) == -1
    assert L.bore_stream_svgd_optimize(C.byref(d), 1, None, 0, DUMMY, 8, None, None, C.byref(opts), DUMMY, None) == -1
    assert L.bore_stream_svgd_optimize(C.byref(d), 1, DUMMY, 0, DUMMY, 8, None, None, None, DUMMY, None) == -1


def test_the_wrapper_checks_its_arguments_before_the_library():
    d = desc(8, [256, 256, 1])
    th = torch.zeros(1, 8)                              # (never looked at: the arguments below are wrong first)
    with pytest.raises(ValueError, match="x_init"):
        ops.stream_svgd_optimize(d, th, torch.zeros(4, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="unknown transform"):
        ops.stream_svgd_optimize(d, th, torch.zeros(1, 4, 8, dtype=torch.float64), transform="cube")
    with pytest.raises(ValueError, match="low and high"):
        ops.stream_svgd_optimize(d, th, torch.zeros(1, 4, 8, dtype=torch.float64), low=np.zeros(8))
