"""ctypes driver for the host build of bore_amd/csrc/lbfgsb.h (test scaffolding)."""
import ctypes as C
import os
import subprocess

import numpy as np
from scipy.optimize import OptimizeResult

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "lbfgsb_host.cpp")
HDR = os.path.join(os.path.dirname(HERE), "bore_amd", "csrc", "lbfgsb.h")
HDR_CARVE = os.path.join(os.path.dirname(HERE), "bore_amd", "csrc", "stream_restart.h")
SO = os.path.join(HERE, "native", "liblbfgsb_host.so")
_CB = C.CFUNCTYPE(None, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))
_lib = None


def lib():
    global _lib
    if _lib is None:
        if (not os.path.exists(SO)
                or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in (SRC, HDR, HDR_CARVE))):
            subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                            SRC, "-o", SO], check=True)
        _lib = C.CDLL(SO)
        _lib.lbfgsb_host_minimize.restype = C.c_int
        _lib.lbfgsb_host_minimize_form.restype = C.c_int
        _lib.lbfgsb_host_minimize_events.restype = C.c_int
        assert _lib.lbfgsb_host_event_count() == len(EVENT_NAMES)
    return _lib


# the events lbfgsb.h reports to the host build, in the order of its EV_* enum
EVENT_NAMES = ("projected_start fixed_variable free_variable unconstrained_iteration first_step_not_boxed "
               "cauchy_singular_refresh formk_refresh cmprlb_refresh subsm_refresh formt_refresh subsm_hit_bound "
               "subsm_backtrack nfree_zero enter leave ls_cache_hit ls_not_descent ls_maxls ls_fail_refresh abnormal "
               "update_skipped info_minus5 history_wrapped").split()
LAYOUT_NAMES = ("ws wy sy ss wt snd wn z r d t xp x g xlast glast wa rwt rwn rsy rsq").split()


def layout(n, m, big_outside=False):
    """make_work's layout for (n, m): ({pointer name: offset in doubles from dw -- snd / wn from `big` when big_outside},
    {int array: offset from iw}, dwork_size, big_size, iwork_size)."""
    off, ioff, sizes = (C.c_int * 21)(), (C.c_int * 3)(), (C.c_int * 3)()
    lib().lbfgsb_host_layout(int(n), int(m), int(bool(big_outside)), off, ioff, sizes)
    return (dict(zip(LAYOUT_NAMES, off)), dict(zip(("index", "iwhere", "indx2"), ioff)), sizes[0], sizes[1], sizes[2])


CARVE_NAMES = "o_box o_vote o_prob prob_floats o_dw o_iw waves lds_bytes room".split()


def stream_restart_carve(D, maxcor, static_bytes, max_waves=4):
    """stream_restart_carve of bore_amd/csrc/stream_restart.h (the streamed restart kernels' dynamic LDS, float
    offsets): (fits, {CARVE_NAMES: value}, sizeof(State), dwork_size(D, maxcor), iwork_size(D))."""
    out, sizes = (C.c_longlong * 9)(), (C.c_int * 3)()
    fits = lib().lbfgsb_host_stream_restart_carve(int(D), int(maxcor), C.c_longlong(int(static_bytes)), int(max_waves),
                                                  out, sizes)
    return bool(fits), dict(zip(CARVE_NAMES, out)), sizes[0], sizes[1], sizes[2]


def minimize(fun, x0, bounds, maxcor=10, ftol=2.2204460492503131e-09, gtol=1e-5, maxfun=15000,
             maxiter=15000, maxls=20, form=0, events=False):
    """fun(x) -> (f, g).  bounds: (lb, ub) arrays with +-inf for open sides.
    form: 0 reverse communication, 1 the routine calls the evaluation (DIRECT), 2 DIRECT with the
    two-variable line search in registers (lbfgsb.h).
    events: also res.events, {name: how often the run passed that LB_EVENT of lbfgsb.h} for EVENT_NAMES."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    n = x0.size
    lb, ub = (np.broadcast_to(np.asarray(b, dtype=np.float64), n).copy() for b in bounds)
    nbd = np.zeros(n, dtype=np.int32)
    for i in range(n):
        lo, up = np.isfinite(lb[i]), np.isfinite(ub[i])
        nbd[i] = 2 if lo and up else 1 if lo else 3 if up else 0
    l = np.where(np.isfinite(lb), lb, 0.0)
    u = np.where(np.isfinite(ub), ub, 0.0)

    def cb(n_, xp, fp, gp):
        x = np.ctypeslib.as_array(xp, shape=(n_,)).copy()
        f, g = fun(x)
        fp[0] = float(f)
        g = np.asarray(g, dtype=np.float64)
        for i in range(n_):
            gp[i] = g[i]

    xo, go = np.empty(n), np.empty(n)
    fo = C.c_double()
    oi = np.zeros(5, dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    args = (int(form), n, maxcor, dp(x0), dp(l), dp(u), ip(nbd), C.c_double(ftol / np.finfo(float).eps), C.c_double(gtol),
            maxiter, maxfun, maxls, _CB(cb), dp(xo), C.byref(fo), dp(go), ip(oi))
    if events:
        ev = np.zeros(len(EVENT_NAMES), dtype=np.int32)
        lib().lbfgsb_host_minimize_events(*args, ip(ev))
    else:
        lib().lbfgsb_host_minimize_form(*args)
    res = OptimizeResult(x=xo, fun=fo.value, jac=go, nit=int(oi[0]), nfev=int(oi[1]),
                          status=int(oi[2]), success=oi[2] == 0, task=(int(oi[3]), int(oi[4])))
    if events:
        res.events = dict(zip(EVENT_NAMES, ev.tolist()))
    return res
