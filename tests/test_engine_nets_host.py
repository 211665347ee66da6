"""The replica engine's host side for bfloat16 and streamed networks (no GPU): what `bore_engine_create` refuses
before any HIP call -- on a machine without a GPU a HIP call would fail with BORE_E_HIP instead -- and the `compute`
argument of the Python engines."""
import ctypes as C
import inspect

import numpy as np
import pytest

from bore_amd import _lib
from bore_amd.engine import NativeEngine, ReplicaEngine, ShardedEngine, lbfgsb_opts

E_UNSUPPORTED = -2
L, N_INIT = 2, 10


def create(D, units, compute="float32", async_loops=0, batch_size=64):
    """bore_engine_create on valid host arrays; returns (code, message, handle)."""
    desc = _lib.make_desc(D, units, ["relu"] * (len(units) - 1) + ["linear"], compute=compute)
    P = int(_lib.lib().bore_param_count(C.byref(desc)))
    assert P > 0
    rs = np.random.RandomState(0)
    low, high = np.zeros(D), np.ones(D)
    dpp = C.POINTER(C.c_double)
    cfg = _lib.EngineCfg(L, 1, 3, N_INIT, 3, batch_size, 3, 64, _lib.TRANSFORM["identity"], 1, async_loops, 0, 0.25,
                         _lib.AdamCfg(1e-3, 0.9, 0.999, 1e-7), lbfgsb_opts(dict(maxiter=30, ftol=1e-9)),
                         low.ctypes.data_as(dpp), high.ctypes.data_as(dpp), -1, 0, -1, 0)
    theta = rs.uniform(-0.1, 0.1, size=(L, P)).astype(np.float32)
    X0, y0 = rs.uniform(size=(L, N_INIT, D)), rs.uniform(size=(L, N_INIT))
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
    if rc == 0:                             # (a machine with a GPU and a request the engine takes)
        _lib.lib().bore_engine_destroy(h)
    return rc, msg, h


@pytest.mark.parametrize("D,units,compute,what", [
    (32, [128, 128, 1], "bfloat16", "a bfloat16 network"),
    (8, [256, 256, 1], "float32", "a streamed network"),
])
def test_the_asynchronous_schedule_refuses_bf16_and_streamed_networks(D, units, compute, what):
    rc, msg, h = create(D, units, compute, async_loops=1)
    assert rc == E_UNSUPPORTED and not h.value, (rc, msg)
    assert msg.startswith("engine_create: the asynchronous schedule launches in batch mode (bore_set_batch)")
    assert what in msg and msg.endswith("on the lock-step schedule (async_loops = 0)")


def test_lockstep_refuses_a_narrow_bf16_network_with_the_library_sentence():
    rc, msg, h = create(2, [16, 16, 1], "bfloat16")
    assert rc == E_UNSUPPORTED and not h.value, (rc, msg)
    assert msg == ("compute = bfloat16 is available for the wide static shapes only (16->64-64-64-1, "
                   "32->128-128-1; any activations, no l2)")


def test_lockstep_refuses_a_bf16_batch_size_other_than_64():
    rc, msg, h = create(32, [128, 128, 1], "bfloat16", batch_size=32)
    assert rc == E_UNSUPPORTED and not h.value, (rc, msg)
    assert msg == "fit_bf16: batch_size must be 64 (got 32)"


def test_lockstep_refuses_a_network_of_neither_flavour_with_the_bound_named():
    desc = _lib.make_desc(8, [513, 513, 1], ["relu", "relu", "linear"])
    want_rc = _lib.lib().bore_mlp_streamed(C.byref(desc))
    want_msg = _lib.lib().bore_last_error().decode()
    rc, msg, h = create(8, [513, 513, 1])
    assert rc == want_rc == E_UNSUPPORTED and not h.value, (rc, msg)
    assert msg == want_msg and "BORE_STREAM_MAX_UNITS" in msg and "513" in msg


@pytest.mark.parametrize("cls", [NativeEngine, ReplicaEngine])
def test_the_python_engines_take_compute(cls):
    p = inspect.signature(cls.__init__).parameters
    assert "compute" in p and p["compute"].default == "float32"


@pytest.mark.parametrize("cls", [NativeEngine, ReplicaEngine])
def test_an_unknown_compute_is_make_descs_value_error(cls):
    with pytest.raises(ValueError, match="compute must be one of"):
        cls(np.arange(2), device="cpu", compute="float16")     # (raised before anything touches a device)


def test_the_sharded_engine_hands_its_keywords_on():
    p = inspect.signature(ShardedEngine.__init__).parameters
    assert p["kw"].kind is inspect.Parameter.VAR_KEYWORD


@pytest.mark.parametrize("cls", [NativeEngine, ReplicaEngine])
def test_the_python_engines_take_a_box(cls):
    p = inspect.signature(cls.__init__).parameters
    assert p["low"].default is None and p["high"].default is None


@pytest.mark.parametrize("bad", [dict(low=(0.0, 1.0), high=(1.0, 0.5)), dict(low=(0.0, np.nan)), dict(high=(np.inf, 1.0)),
                                 dict(low=(-np.inf, 0.0)), dict(low=(0.0,)), dict(high=(1.0, 1.0, 1.0)), dict(low=0.0)])
def test_a_bad_box_is_a_value_error_before_any_device_call(bad):
    """low > high, a non-finite bound, a wrong length: refused by all three engines (ShardedEngine hands its keywords
    on) before anything touches a device."""
    for make in (NativeEngine, ReplicaEngine, lambda ids, **kw: ShardedEngine(ids, shards=2, **kw)):
        with pytest.raises(ValueError, match="low|high"):
            make(np.arange(4), device="cpu", **bad)


def test_the_box_is_the_unit_box_by_default_and_admits_a_fixed_coordinate():
    from bore_amd.engine import box
    lo, hi = box(None, None, 3)
    assert np.array_equal(lo, np.zeros(3)) and np.array_equal(hi, np.ones(3)) and lo.dtype == hi.dtype == np.float64
    lo, hi = box([-5, 0.5], (10, 0.5), 2)
    assert np.array_equal(lo, [-5.0, 0.5]) and np.array_equal(hi, [10.0, 0.5])
