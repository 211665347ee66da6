"""Time of `argmax_batch` for networks too large for one workgroup's LDS on one MI355X, by route:
  device  svgd_mode="device": all iterations in one launch on the streamed kernels (bore_stream_svgd_optimize)
  host    svgd_mode="host": bore_amd/optimizers/svgd.py, one streamed value + input-gradient launch, a download and a
          float64 numpy step per iteration -- the only route before the device one
16->128-128-128-1 and 8->256-256-1 after a short fit, one model, batch_size 8, 32 and 64, the reference's n_iter = 1000,
transform sigmoid.  Wall clock around the call (it returns host results: the device is idle again when it does), the
two routes ALTERNATING call by call in one process, the median of REPS calls each after WARMUP, the same draw in every
call; max |device - host| of the particles beside the times.
Every (shape, batch_size) runs in a child process of its own under a time limit; the first one that fails ends the
run.  Writes profiles/stream/svgd_time.json (or the path given) with the source digest of the library that ran."""
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
CASES = [(s, b) for s in SHAPES for b in (8, 32, 64)]
LIMIT_S = 240
WARMUP, REPS = 2, 7
N_ITER = 1000


def child(shape, batch_size):
    import warnings

    import numpy as np
    import torch
    from scipy.optimize import Bounds

    from bore_amd import ops
    from bore_amd.layers import BinaryCrossentropy, Dense
    from bore_amd.models import BatchMaximizableSequential

    torch.cuda.set_device(0)
    D, hidden, act = SHAPES[shape]
    rs = np.random.RandomState(0)
    X = rs.uniform(size=(64, D))
    y = np.sum((X - 0.3) ** 2, axis=1)
    z = (y < np.quantile(y, 0.25)).astype(np.float64)
    model = BatchMaximizableSequential("sigmoid", seed=1)
    for u in hidden:
        model.add(Dense(u, activation=act))
    model.add(Dense(1, activation="linear"))
    model.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True))
    model.fit(X, z, epochs=5, batch_size=64)
    assert ops.mlp_streamed(model._desc) == 7
    model.stream_svgd_max_work = None          # (the kernel itself, also where argmax_batch would choose the host driver)
    bounds = Bounds(lb=np.zeros(D), ub=np.ones(D))
    times, out = dict(device=[], host=[]), {}
    # (a device call that stepped aside to the host would time the wrong route)
    warnings.filterwarnings("error", message=".*svgd_mode='device' cannot take this request.*")
    for rep in range(WARMUP + REPS):
        for route in ("device", "host"):
            model.svgd_mode = route
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[route] = model.argmax_batch(batch_size, bounds, n_iter=N_ITER, random_state=5)
            torch.cuda.synchronize()
            if rep >= WARMUP:
                times[route].append(1e3 * (time.perf_counter() - t0))
    res = dict(shape=shape, batch_size=batch_size, n_iter=N_ITER, transform="sigmoid", routes={},
               max_abs_device_minus_host=float(np.abs(out["device"] - out["host"]).max()))
    for route, t in times.items():
        res["routes"][route] = dict(ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t)))
    res["host_over_device"] = res["routes"]["host"]["ms_median"] / res["routes"]["device"]["ms_median"]
    print("RESULT " + json.dumps(res))


def main(out, commit):
    from bore_amd import _lib
    digest = _lib.built_digest()
    assert digest == _lib.source_digest(), "the library was not built from these sources"
    results = []
    for shape, batch_size in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, str(batch_size)],
                           capture_output=True, text=True, timeout=LIMIT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"{shape} batch_size {batch_size}: exit status {p.returncode}; nothing more is run")
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(note=f"one model per call; ms of one argmax_batch(batch_size, n_iter={N_ITER}), wall clock, the "
                            f"routes alternating, median of {REPS} after {WARMUP} warm-up calls each",
                       commit=commit, csrc_digest=digest, results=results), f, indent=1)


def head_commit():
    try:
        p = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        return p.stdout.strip() if p.returncode == 0 and p.stdout.strip() else None
    except OSError:
        return None


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        args = sys.argv[1:]
        commit = None
        if "--commit" in args:                 # (a tree without its history: say which commit it is)
            k = args.index("--commit")
            commit = args[k + 1]
            del args[k:k + 2]
        main(args[0] if args else os.path.join(ROOT, "profiles", "stream", "svgd_time.json"), commit or head_commit())
