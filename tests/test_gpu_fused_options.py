"""The fused loop kernel (bore_amd/csrc/bore_iter.hip) at every engine option, one option at a time, bit for bit.

One launch of the fused kernel runs append, labels, fit, sample + screen, the L-BFGS-B restarts and the pick with its
own LDS carve, its own launch plans and -- 2->16-16-1, at most four restarts -- the job board.  The reference is the same
``NativeEngine`` on the lock-step schedule (``groups=2``): the stand-alone kernels, which have no board, no fused carve
and no residency, and which are themselves held against the host build of lbfgsb.h, the float64 oracle and
``ReplicaEngine`` (tests/test_gpu_lbfgsb_maxcor.py, test_gpu_lbfgsb_paths.py, test_gpu_argmax.py, and
``test_lockstep_engine_equals_python_engine_in_a_box`` below).  Every comparison is ``np.array_equal``: observations,
the four arrays of the classifier state, ``none_results`` and ``n_fg_requests``.

Every case asserts the route it took (``route``): a fused engine times no fit of its own (``fit_ms == 0``) and counts an
in-kernel stamp per loop-iteration; the launch chain times its fit."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ELU3 = ("elu", "elu", "elu", "linear")


def branin_native(X):
    """Branin-Hoo on its native box [-5, 10] x [0, 15]."""
    x1, x2 = X[..., 0], X[..., 1]
    return ((x2 - 5.1 / (4 * np.pi ** 2) * x1 ** 2 + 5 / np.pi * x1 - 6) ** 2
            + 10 * (1 - 1 / (8 * np.pi)) * np.cos(x1) + 10)


def far_bowl(X):
    """Smooth, minimum inside [1000, 1001] x [-3, -2.5]."""
    u, v = X[..., 0] - 1000.0, X[..., 1] + 3.0
    return (u - 0.3) ** 2 + 4.0 * (v - 0.2) ** 2 + 0.1 * np.sin(5.0 * (u + v))


def plugin_objective(X):
    return np.sum((X - 0.4) ** 2, axis=-1) + 0.1 * np.sin(5.0 * X.sum(axis=-1))


def skewed_objective(X):
    """For the 16-dimensional box below: the same shape, about the box's own centre."""
    Z = (X - LOW16) / np.where(HIGH16 > LOW16, HIGH16 - LOW16, 1.0)
    return np.sum((Z - 0.4) ** 2, axis=-1) + 0.1 * np.sin(5.0 * Z.sum(axis=-1))


# an asymmetric box in 16 dimensions, mixed signs and widths, coordinate 7 fixed
LOW16 = np.array([-5.0, 0.0, 2.0, -1.0, 0.0, 10.0, -0.5, 0.25, 0.0, -3.0, 1.0, 0.0, -20.0, 0.0, 0.5, -1.0])
HIGH16 = np.array([10.0, 15.0, 3.0, 1.0, 0.125, 11.0, 0.5, 0.25, 1.0, -2.5, 4.0, 1.0, 20.0, 2.0, 0.75, 0.0])

SHAPE1 = dict(loops=6, epochs=20, num_samples=64, n_init=10, objective="branin01")
SHAPE5 = dict(loops=5, input_dim=16, units=(32, 32, 32, 1), acts=ELU3, transform="sigmoid", gamma=1.0 / 3.0, epochs=12,
              num_samples=128, num_starts=5, n_init=20, objective=plugin_objective)
# the largest maxcor the batch-mode restart plan takes for 16->32-32-32-1 at five restarts (one workgroup, four waves:
# tests/test_acq_plan_host.py::test_the_fused_kernels_restart_plans pins it through bore_lbfgsb_plan_query)
SHAPE5_MAXCOR_MOST = 19

FORMS = dict(resident={}, inlined=dict(resident_wait_us=0), queue=dict(work_queue=True))


def freeze(kw):
    def f(v):
        if isinstance(v, dict):
            return tuple(sorted((k, f(u)) for k, u in v.items()))
        if isinstance(v, (list, tuple, np.ndarray)):
            return tuple(f(u) for u in v)
        return v
    return tuple(sorted((k, f(v)) for k, v in kw.items()))


def thaw(frozen):
    kw = dict(frozen)
    if "options" in kw:
        kw["options"] = dict(kw["options"])
    return kw


def run_engine(kw, steps=(2, 2), **schedule):
    """The engine of `kw` (loops: how many) on the given schedule, advanced by `steps` -> (the six arrays, statistics
    since creation)."""
    from bore_amd.engine import NativeEngine
    kw = dict(kw)
    eng = NativeEngine(np.arange(kw.pop("loops")), **kw, **schedule)
    try:
        for n in steps:
            eng.run(n)
        return eng.observations() + eng.state(), eng.take_stats()
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _lockstep(frozen, steps):
    out, st = run_engine(thaw(frozen), steps, groups=2)
    for a in out:
        a.setflags(write=False)
    return out, st


def lockstep(kw, steps=(2, 2)):
    """The reference of an option set, computed once."""
    return _lockstep(freeze(kw), tuple(steps))


def route(st, loops, n_steps):
    """"fused" or "chain", from the engine's own statistics."""
    if st["fit_ms"] == 0.0:
        assert st["phase_iterations"] == loops * n_steps, st
        return "fused"
    assert st["fit_ms"] > 0
    return "chain"


def same(ref, got):
    (ra, rs), (ga, gs) = ref, got
    names = ("X", "y", "theta", "adam_m", "adam_v", "adam_t")
    diff = [n for n, p, q in zip(names, ra, ga) if not np.array_equal(p, q)]
    assert not diff, diff
    assert gs["none_results"] == rs["none_results"] and gs["n_fg_requests"] == rs["n_fg_requests"], (gs, rs)


def set_helper(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("BORE_LBFGSB_HELPER", raising=False)
    else:
        monkeypatch.setenv("BORE_LBFGSB_HELPER", mode)


def helper_stats(reset):
    from bore_amd import _lib
    L = _lib.lib()
    L.bore_debug_helper_stats.argtypes = [C.c_void_p, C.c_int]
    L.bore_debug_helper_stats.restype = C.c_int
    out = (C.c_longlong * 5)()
    assert L.bore_debug_helper_stats(out, int(reset)) == 0
    return dict(zip(("speculative", "committed", "dropped", "taken", "withdrawn"), out))


def opts(**o):
    """The engine's default L-BFGS-B options (maxiter 1000, ftol 1e-9) with `o` over them."""
    return dict(options=dict(dict(maxiter=1000, ftol=1e-9), **o))


# ---- 2 -> 16-16-1 ------------------------------------------------------------------------------------------------------
# LDS of the restart phase in batch mode (bore_lbfgsb_plan_query, one workgroup of four waves; test_acq_plan_host.py
# pins these): three restarts 26 832 B at maxcor 10, 35 184 B at 12, 62 016 B at 17, 160 512 B at 29 -- a whole CU's LDS:
# one loop per CU --, refused from 30; 16 restarts at maxcor 10 123 200 B, 8 at maxcor 17 157 696 B.
NATIVE_BOX = dict(low=(-5.0, 0.0), high=(10.0, 15.0), objective=branin_native)
FAR_BOX = dict(low=(1000.0, -3.0), high=(1001.0, -2.5), objective=far_bowl)
FIXED_BOX = dict(low=(0.0, 0.5), high=(1.0, 0.5))
CASES1 = {
    "maxcor3": opts(maxcor=3),                # the history wraps within a few iterations
    "maxcor5": opts(maxcor=5),
    "maxcor12": opts(maxcor=12),
    "maxcor17": opts(maxcor=17),              # the board's spare blocks do not fit: exact jobs only
    "maxcor29": opts(maxcor=29),              # the largest plan
    "sigmoid": dict(transform="sigmoid"),
    "exp": dict(transform="exp"),
    "gamma0.1": dict(gamma=0.1),              # an interpolated quantile at N = 10 .. 13
    "gamma0.5": dict(gamma=0.5),              # half the rows positive
    "starts1": dict(num_starts=1),
    "starts2": dict(num_starts=2),
    "starts4": dict(num_starts=4),
    "starts8": dict(num_starts=8),            # a wave takes several problems: no board
    "starts16": dict(num_starts=16),
    "starts8_maxcor17": dict(num_starts=8, **opts(maxcor=17)),     # the edge of that plan
    "maxiter2": opts(maxiter=2),              # status 1: taken by the pick
    "maxfun6": opts(maxfun=6),
    "maxls1": opts(maxls=1),                  # abnormal line searches -> None -> fallback draws
    "ftol1e-3": opts(ftol=1e-3),
    "gtol1e-2": opts(gtol=1e-2),
    "samples3": dict(num_samples=3),          # = num_starts: every candidate chosen
    "samples1000": dict(num_samples=1000),    # a tail that is no multiple of 64
    "n_init2": dict(n_init=2),                # the smallest record with a real quantile
    "epochs1": dict(epochs=1),
    "dedup_maxiter2": dict(deduplicate=True, **opts(maxiter=2)),   # the filter over early, repeated stops
    "native_box": NATIVE_BOX,                 # mixed signs
    "far_box": FAR_BOX,                       # coarse float32 images: many shortcut hits
    "fixed_box": FIXED_BOX,                   # a fixed variable in the two-variable form
}


def case1(name):
    return dict(SHAPE1, **CASES1[name])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CASES1))
def test_shape1_fused_equals_lockstep(gpu, monkeypatch, name, form):
    kw = case1(name)
    ref = lockstep(kw)
    assert route(ref[1], kw["loops"], 4) == "chain"
    for helper in (None, "0"):
        set_helper(monkeypatch, helper)
        got = run_engine(kw, async_loops=True, **FORMS[form])
        assert route(got[1], kw["loops"], 4) == "fused", (name, form, helper)
        same(ref, got)
        if name == "maxls1":
            # (every restart of a loop ended in an abnormal line search: the fallback point, drawn from the loop's
            # MT19937 state on the async host path and in the lock-step finalize)
            assert ref[1]["none_results"] > 0 and got[1]["none_results"] > 0
        if name == "far_box":
            # (x ~ 1000: float32 spacing 6e-5 -- trial points whose float32 image is the last one's are served by
            # evaluate2's shortcut without running the network)
            assert got[1]["n_fg_rows"] < got[1]["n_fg_requests"], got[1]


@pytest.mark.parametrize("name,expect", [("maxcor5", "speculative"), ("maxcor17", "exact"), ("maxcor29", "exact"),
                                         ("fixed_box", "any")])
def test_shape1_job_board_counters(gpu, monkeypatch, name, expect):
    """Resident, board on.  maxcor 5: the spare wn / snd blocks lie in LDS the fit phase has anyway -- speculative jobs
    run and some are committed.  maxcor 17 and 29: they do not fit (iteration_plan: big_wave = 0; by the plans' sizes
    from maxcor 13 at three restarts) -- exact jobs only."""
    kw = case1(name)
    ref = lockstep(kw)
    set_helper(monkeypatch, None)
    helper_stats(True)
    got = run_engine(kw, async_loops=True)
    seen = helper_stats(False)
    print(name, seen)
    assert route(got[1], kw["loops"], 4) == "fused"
    same(ref, got)
    if expect == "speculative":
        assert seen["speculative"] > 0 and seen["committed"] > 0, seen
    elif expect == "exact":
        assert seen["speculative"] == 0 and seen["taken"] + seen["withdrawn"] > 0, seen
    else:
        assert seen["dropped"] >= 0, seen


def test_shape1_three_loops_per_cu(gpu, monkeypatch):
    """More loops than two per CU: the resident kernel of three loops per CU (no board), sigmoid, maxcor 5."""
    import torch
    set_helper(monkeypatch, None)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    kw = dict(loops=2 * cus + 40, epochs=4, num_samples=64, n_init=60, objective="branin01", transform="sigmoid",
              **opts(maxcor=5))
    ref = lockstep(kw, (3,))
    got = run_engine(kw, (3,), async_loops=True)
    assert got[1]["loops_per_cu"] == 3 and got[1]["side_by_side_workgroups"] == kw["loops"]
    assert route(got[1], kw["loops"], 3) == "fused"
    same(ref, got)


# ---- 16 -> 32-32-32-1 (no board on this shape) -----------------------------------------------------------------------------
CASES5 = {
    "maxcor5": opts(maxcor=5),
    "maxcor_most": opts(maxcor=SHAPE5_MAXCOR_MOST),
    "identity": dict(transform="identity"),
    "exp": dict(transform="exp"),
    "acts_rtss": dict(acts=("relu", "tanh", "sigmoid", "sigmoid")),
    "acts_trel": dict(acts=("tanh", "relu", "elu", "linear")),
    "starts1_maxcor5": dict(num_starts=1, **opts(maxcor=5)),
    "starts16_maxcor5": dict(num_starts=16, **opts(maxcor=5)),
    "maxiter2": opts(maxiter=2),
    "skewed_box": dict(low=LOW16, high=HIGH16, objective=skewed_objective),
}


@pytest.mark.parametrize("form", ["resident", "queue"])
@pytest.mark.parametrize("name", list(CASES5))
def test_shape5_fused_equals_lockstep(gpu, name, form):
    kw = dict(SHAPE5, **CASES5[name])
    ref = lockstep(kw)
    assert route(ref[1], kw["loops"], 4) == "chain"
    got = run_engine(kw, async_loops=True, **FORMS[form])
    assert route(got[1], kw["loops"], 4) == "fused", (name, form)
    same(ref, got)


# ---- the reference under the new arguments ---------------------------------------------------------------------------------
@pytest.mark.parametrize("box", [NATIVE_BOX, FAR_BOX], ids=["native_box", "far_box"])
def test_lockstep_engine_equals_python_engine_in_a_box(gpu, box):
    """The lock-step NativeEngine against ReplicaEngine(mode="device") with low / high, at the hard settings of
    test_native_engine_equals_python_engine.  The fallback draw rs.uniform(low, high) is stated twice -- C++ (bore_engine.hip:
    finalize, take_async_result) and numpy (ReplicaEngine._finalize): this is where the two statements meet."""
    from bore_amd.engine import NativeEngine, ReplicaEngine
    kw = dict(num_samples=64, epochs=20, deduplicate=True, **box)
    a = NativeEngine(np.arange(3, 14), groups=3, **kw)
    b = ReplicaEngine(np.arange(3, 14), mode="device", groups=2, **kw)
    try:
        a.run(12)
        b.run(12)
        Xa, ya = a.observations()
        assert Xa.shape == (11, 22, 2)
        lo, hi = np.array(box["low"]), np.array(box["high"])
        assert (Xa >= lo).all() and (Xa <= hi).all()
        assert np.array_equal(Xa, b.X) and np.array_equal(ya, b.y)
        th, m, v, t = a.state()
        assert np.array_equal(th, b.theta.cpu().numpy()) and np.array_equal(m, b.adam_m.cpu().numpy())
        assert np.array_equal(v, b.adam_v.cpu().numpy()) and np.array_equal(t, b.adam_t.cpu().numpy())
        assert a.take_stats()["none_results"] == b.stats["none_results"]
    finally:
        a.close()


# ---- refusal or fallback -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_size", [32, 7])
@pytest.mark.parametrize("shape", [1, 5])
def test_other_batch_sizes_run_the_launch_chain(gpu, shape, batch_size):
    """include/bore_hip.h, async_loops: one fused kernel per loop-iteration where the model and the request have one,
    "otherwise the launch chain".  The fused kernel's fit phase is the static fit of 64-row batches; with another
    batch_size fit_plan picks the run-time-layout fit in batch mode (bore_kernel_flavour(desc, false) < 0), which the
    fused kernel has no phase for -- iteration_plan's "static shape 1, or 5 at 16 inputs, one workgroup per loop".  Before
    the engine took its schedule from that probe, such an engine failed to be created (UnsupportedError with that
    message): the network alone said "fused"."""
    kw = dict(SHAPE1 if shape == 1 else SHAPE5, batch_size=batch_size)
    ref = lockstep(kw)
    got = run_engine(kw, async_loops=True)
    assert route(got[1], kw["loops"], 4) == "chain"
    same(ref, got)


# Records of 16 -> 32-32-32-1 (measured on creation, three loops): 2 000 and 3 000 rows fused, one loop per CU; 4 000 rows the
# launch chain; from 5 000 the batch-mode fit refuses for the chain as well ("fit: theta+tile+perm need 165184 B of LDS").
# An engine's records start at 2 x n_init rows and double when a run would overfill them.
GROWTH = dict(loops=3, epochs=1, num_samples=32, num_starts=1, n_init=1000, options=dict(maxiter=2))
GROWTH_STEPS = (1000, 2)          # 2 000 rows: the records are full; two more: 4 000 rows


def test_shape5_leaves_the_fused_kernel_when_the_records_grow(gpu):
    """With records of 4 000 rows the Adam slots no longer lie in LDS beside the epoch's shuffle (fit_plan:
    state_in_lds), the fit leaves the static kernel, and the re-probe of the schedule (async_run) sends the engine to the
    launch chain -- where it used to return iteration_plan's refusal from the middle of bore_engine_run.  One trajectory
    throughout, the lock-step engine's.  (One epoch, one restart of two iterations: a thousand loop-iterations within
    the second or two a case may take.)"""
    from bore_amd.engine import NativeEngine
    kw = dict(SHAPE5, **GROWTH)
    ref = lockstep(kw, GROWTH_STEPS)
    kw = dict(kw)
    loops = kw.pop("loops")
    eng = NativeEngine(np.arange(loops), async_loops=True, **kw)
    try:
        eng.run(GROWTH_STEPS[0])
        assert route(eng.take_stats(), loops, GROWTH_STEPS[0]) == "fused"
        eng.run(GROWTH_STEPS[1])
        assert route(eng.take_stats(), loops, GROWTH_STEPS[1]) == "chain"
        got = eng.observations() + eng.state()
    finally:
        eng.close()
    assert got[0].shape == (loops, 2002, 16)
    diff = [n for n, p, q in zip(("X", "y", "theta", "adam_m", "adam_v", "adam_t"), ref[0], got) if not np.array_equal(p, q)]
    assert not diff, diff


@pytest.mark.parametrize("async_kw", [{}, dict(work_queue=True), dict(resident_wait_us=0)])
def test_what_neither_route_takes_is_refused_at_creation(gpu, async_kw):
    """maxcor 30 with three restarts on 2->16-16-1: the batch-mode restart plan needs more than a CU's LDS for one
    workgroup -- the fused kernel and the chain both launch in batch mode.  Refused by name before any launch; the
    half-made engine is destroyed (the Python object holds no handle) and the next engine is created as usual."""
    from bore_amd import _lib
    from bore_amd.engine import NativeEngine
    kw = dict(SHAPE1, **opts(maxcor=30))
    loops = kw.pop("loops")
    calls = []

    def objective(X):
        calls.append(X.shape)
        return np.sum((X - 0.3) ** 2, axis=-1)

    with pytest.raises(_lib.UnsupportedError, match="batch mode needs num_starts <= 16 in one workgroup"):
        NativeEngine(np.arange(loops), async_loops=True, **dict(kw, objective=objective), **async_kw)
    assert calls == [(loops, kw["n_init"], 2)]      # (the initial design; no launch asked for a value)
    # the lock-step schedule takes the same request (several workgroups per loop)
    out, st = run_engine(dict(kw, loops=loops), groups=2)
    assert st["fit_ms"] > 0
    got = run_engine(dict(SHAPE1), async_loops=True, **async_kw)
    same(lockstep(dict(SHAPE1)), got)
