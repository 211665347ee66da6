"""ctypes driver for tests/native/restart_helper_host.cpp: the host board that checks the rule of the restart phase's
job board (bore_amd/csrc/lbfgsb.h: JOB BOARD).  Shared by tests/test_restart_helper_host.py and
tools/restart_helper_prediction.py.  Test scaffolding; CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import bore_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "restart_helper_host.cpp")
NAMES = ("formk sets_kept speculated guess_held same_bytes mismatch moved moved_accepted dropped nfree_changed").split()
_CB = C.CFUNCTYPE(None, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))


def build(directory):
    """Compiles the board into `directory` and loads it."""
    so = os.path.join(str(directory), "librestart_helper_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", SRC, "-o", so], check=True)
    lib = C.CDLL(so)
    assert lib.restart_helper_host_count() == len(NAMES)
    return lib


def new_counts():
    return np.zeros(len(NAMES), dtype=np.int64)


def run(lib, fun, x0, lo, hi, counts, maxcor=10, maxiter=1000, ftol=1e-9, gtol=1e-5):
    """One problem with the board and once more without (the library compares the two: x, f, g, nit, nfev, status and
    task must be the same bits); adds the board's counts to `counts`.  Returns (nit, nfev, status, task, msg)."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    n = x0.size
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), n), np.broadcast_to(np.asarray(hi, dtype=np.float64), n)
    fin_lo, fin_hi = np.isfinite(lo), np.isfinite(hi)
    nbd = np.where(fin_lo & fin_hi, 2, np.where(fin_lo, 1, np.where(fin_hi, 3, 0))).astype(np.int32)
    l, u = np.ascontiguousarray(np.where(fin_lo, lo, 0.0)), np.ascontiguousarray(np.where(fin_hi, hi, 0.0))

    def cb(n_, xp, fp, gp):
        f, g = fun(np.ctypeslib.as_array(xp, shape=(n_,)).copy())
        fp[0] = float(f)
        np.ctypeslib.as_array(gp, shape=(n_,))[:] = np.asarray(g, dtype=np.float64)

    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    info = np.zeros(5, dtype=np.int32)
    rc = lib.restart_helper_host_run(n, maxcor, dp(x0), dp(l), dp(u), nbd.ctypes.data_as(C.POINTER(C.c_int)),
                                     C.c_double(ftol / np.finfo(float).eps), C.c_double(gtol), maxiter, 15000, 20, _CB(cb),
                                     counts.ctypes.data_as(C.POINTER(C.c_longlong)), info.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0, "the run with the board differs from the run without"
    return tuple(int(v) for v in info)


def branin01(X):
    """Branin on the unit square (the headline's objective)."""
    x1, x2 = 15.0 * X[:, 0] - 5.0, 15.0 * X[:, 1]
    return ((x2 - 5.1 / (4 * np.pi ** 2) * x1 ** 2 + 5.0 / np.pi * x1 - 6.0) ** 2
            + 10.0 * (1.0 - 1.0 / (8 * np.pi)) * np.cos(x1) + 10.0)


def config1_problems(loops, iterations=25, restarts=3, samples=1024):
    """Restart problems as config-1 loops meet them: the oracle's BO loop on Branin as bench.py's CPU baseline runs it
    (10 initial points, gamma 0.25, 2->16-16-1 fitted 200 one-batch epochs per iteration with its weights and Adam
    state carried over, `restarts` starts = the best of `samples` uniform points) for `iterations` iterations per loop.
    Yields (fg, x0) for every restart of every iteration -- fg in the oracle's float32 arithmetic."""
    from scipy.optimize import Bounds
    acts = ["relu", "relu", "sigmoid"]
    bounds = Bounds(np.zeros(2), np.ones(2))
    for loop in range(loops):
        rs = np.random.RandomState(9000 + 1000 * loop)
        p = O.glorot_uniform_params(2, [16, 16, 1], rs)
        st = O.AdamState(p)
        X = rs.uniform(size=(10, 2))
        y = branin01(X)
        for _ in range(iterations):
            z, _ = O.labels(y, 0.25)
            perms = np.stack([rs.permutation(len(y)) for _ in range(200)])
            O.fit(p, acts, st, X, z, perms, batch_size=64)
            X_init = rs.uniform(size=(samples, 2))
            f_init = -O.predict(p, acts, X_init).squeeze(axis=-1)
            frozen = [q.copy() for q in p]
            fg = lambda x, q=frozen: tuple(O.value_and_input_grad(q, acts, x, "identity"))
            for i in np.argpartition(f_init, kth=restarts - 1, axis=None)[:restarts]:
                yield fg, X_init[i]
            res = O.argmax(p, acts, bounds, num_starts=restarts, num_samples=samples, random_state=rs, X_init=X_init)
            x = res.x if res is not None else rs.uniform(size=2)
            X = np.vstack([X, x])
            y = np.append(y, branin01(x[None])[0])
