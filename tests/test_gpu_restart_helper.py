"""The job board of the fused loop kernel's restart phase (bore_amd/csrc/bore_argmax.hip: RestartJobs; lbfgsb.h: JOB
BOARD): idle waves form and factor K for the waves that own a restart, speculatively at the top of an L-BFGS-B
iteration or exactly once the sets are known.  Who runs formk, and when, must not show in a single bit: the engine
with the board (BORE_LBFGSB_HELPER unset / 1), without it (0), with every speculative result dropped (2) and with
helpers that take nothing (3) gives the lock-step engine's observations and classifier state -- the lock-step chain
runs the stand-alone restart kernel, which has no board.  The counters of bore_debug_helper_stats say that the paths
were in fact taken."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(epochs=20, n_init=10)
MODES = [None, "0", "2", "3"]


def run_engine(loops, num_starts, objective, **kw):
    """4 iterations in two run(2) calls -> (observations X, y, theta, adam m, v, t)."""
    from bore_amd.engine import NativeEngine
    eng = NativeEngine(np.arange(loops), num_starts=num_starts, objective=objective, **KW, **kw)
    eng.run(2)
    eng.run(2)
    out = eng.observations() + eng.state()
    eng.close()
    return out


@functools.lru_cache(maxsize=None)
def lockstep(loops, num_starts):
    return run_engine(loops, num_starts, "branin01")


def stats(reset):
    from bore_amd import _lib
    L = _lib.lib()
    L.bore_debug_helper_stats.argtypes = [C.c_void_p, C.c_int]
    L.bore_debug_helper_stats.restype = C.c_int
    out = (C.c_longlong * 5)()
    assert L.bore_debug_helper_stats(out, int(reset)) == 0
    return dict(zip(("speculative", "committed", "dropped", "taken", "withdrawn"), out))


def same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("BORE_LBFGSB_HELPER", raising=False)
    else:
        monkeypatch.setenv("BORE_LBFGSB_HELPER", mode)


@pytest.mark.parametrize("num_starts", [1, 2, 3, 4])
def test_resident_engine_equals_lockstep_in_every_mode(gpu, monkeypatch, num_starts):
    """Three, two, one and no idle wave at the start of the restart phase (a finished restart's wave helps too)."""
    ref = lockstep(6, num_starts)
    for mode in MODES:
        set_mode(monkeypatch, mode)
        got = run_engine(6, num_starts, "branin01", async_loops=True)
        assert same(ref, got), (num_starts, mode)


def test_work_queue_engine_equals_lockstep_in_every_mode(gpu, monkeypatch):
    ref = lockstep(3, 3)
    for mode in MODES:
        set_mode(monkeypatch, mode)
        got = run_engine(3, 3, "branin01", async_loops=True, work_queue=True)
        assert same(ref, got), mode


def test_counters_say_which_paths_ran(gpu, monkeypatch):
    """Branin at these sizes already takes every path, the wrong guess included (its restarts run into the faces of
    the unit square: a fifth of the speculative jobs is dropped), so there is no second objective.  (y = x0 + x1, whose
    optimum is the corner, cannot serve: several restarts end in the corner with equal values, and the lock-step engine
    itself does not repeat its own trajectories on it -- with or without the board.)"""
    ref = lockstep(6, 3)
    seen = {}
    for mode in (None, "0", "2", "3"):
        set_mode(monkeypatch, mode)
        stats(True)
        got = run_engine(6, 3, "branin01", async_loops=True)
        seen[mode] = stats(False)
        assert same(ref, got), mode
    print(seen)
    on, off, exact, lone = seen[None], seen["0"], seen["2"], seen["3"]
    assert on["speculative"] > 0 and on["committed"] > 0 and on["dropped"] >= 1
    assert not any(off.values())                                  # the kernels without the board ran
    assert exact["committed"] == 0 and exact["taken"] > 0 and exact["dropped"] == exact["speculative"] > 0
    assert lone["committed"] == 0 and lone["taken"] == 0 and lone["withdrawn"] > 0
