"""Time of `maxima` for networks too large for one workgroup's LDS on one MI355X, by route:
  device    screening and restarts on the streamed kernels (bore_stream_screen_topk + bore_stream_lbfgsb_minimize)
  lockstep  restart_mode="lockstep" + screen_mode="host": predict + argpartition, then SciPy's L-BFGS-B state
            machines in lock-step around bore_mlp_value_and_input_grad -- the only route before the device one
16->128-128-128-1 and 8->256-256-1 after a short fit, num_starts 5, num_samples 1024, transform identity and the
plugin's sigmoid.  Wall clock around the call (it returns host results: the device is idle again when it does), the
median of REPS calls after WARMUP, the same candidates in every call; nit / nfev of every restart beside the times.
Every (shape, transform) runs in a child process of its own under a time limit; the first one that fails ends the run.
Writes profiles/stream/acq_time.json (or the path given)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "16x128x128x128x1": (16, [128, 128, 128], "elu"),
    "8x256x256x1": (8, [256, 256], "relu"),
}
CASES = [(s, t) for s in SHAPES for t in ("identity", "sigmoid")]
LIMIT_S = 240
WARMUP, REPS = 2, 9


def child(shape, transform):
    import numpy as np
    import torch
    from scipy.optimize import Bounds

    from bore_amd import ops
    from bore_amd.layers import BinaryCrossentropy, Dense
    from bore_amd.models import MaximizableSequential

    torch.cuda.set_device(0)
    D, hidden, act = SHAPES[shape]
    rs = np.random.RandomState(0)
    X = rs.uniform(size=(40, D))
    y = np.sum((X - 0.3) ** 2, axis=1)
    z = (y < np.quantile(y, 1 / 3)).astype(np.float64)
    model = MaximizableSequential(transform=transform, seed=1)
    for u in hidden:
        model.add(Dense(u, activation=act))
    model.add(Dense(1, activation="linear"))
    model.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True))
    model.fit(X, z, epochs=5, batch_size=64)
    assert ops.mlp_streamed(model._desc) == 7
    bounds = Bounds(lb=np.zeros(D), ub=np.ones(D))
    res = dict(shape=shape, transform=transform, num_starts=5, num_samples=1024, routes={})
    for route, modes in (("device", ("device", "device")), ("lockstep", ("lockstep", "host"))):
        model.restart_mode, model.screen_mode = modes
        times, out = [], None
        for rep in range(WARMUP + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.maxima(bounds, num_starts=5, num_samples=1024, print_fn=lambda s: None,
                               random_state=np.random.RandomState(7))
            torch.cuda.synchronize()
            if rep >= WARMUP:
                times.append(1e3 * (time.perf_counter() - t0))
        res["routes"][route] = dict(ms_median=float(np.median(times)), ms_min=float(np.min(times)),
                                    ms_max=float(np.max(times)), nit=[int(r.nit) for r in out],
                                    nfev=[int(r.nfev) for r in out], fun=[float(r.fun) for r in out])
    d, h = res["routes"]["device"], res["routes"]["lockstep"]
    res["lockstep_over_device"] = h["ms_median"] / d["ms_median"]
    print("RESULT " + json.dumps(res))


def main(out):
    results = []
    for shape, transform in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, transform],
                           capture_output=True, text=True, timeout=LIMIT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"{shape} {transform}: exit status {p.returncode}; nothing more is run")
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(note="one model per call; ms of one maxima(num_starts=5, num_samples=1024), wall clock, "
                            f"median of {REPS} after {WARMUP} warm-up calls",
                       results=results), f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stream", "acq_time.json"))
