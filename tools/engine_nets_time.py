"""Time of the replica engine's lock-step schedule on the networks it took last, on one MI355X: the C++ host loop
(NativeEngine) against the same stages enqueued by the interpreter (ReplicaEngine, mode="device", select="device").
  32->128-128-1      compute="bfloat16" (BASELINE config 5)
  16->128-128-128-1  float32, streamed (ClassifierSuggester(num_units=128, num_layers=2) on 16 inputs)
64 and 256 loops in one group and in 4 (each group steps on its own stream), n_init 10, 20 epochs, 1024 candidates,
3 restarts of at most 100 iterations, a quadratic objective evaluated by numpy for both engines.  Each engine runs
2 warm-up iterations; then the two alternate, REPS times each, wall clock around one run(ITERS) -- which returns
when every loop's objective value of the last iteration is known --, and the median of the REPS is reported in ms
per BO iteration of all loops.  Every (network, loops, groups) case runs in a child process of its own under a
time limit; the first one that fails ends the run.  Writes profiles/engine_nets/engine_nets_time.json (or the path given)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NETS = {
    "bf16 32x128x128x1": dict(input_dim=32, units=(128, 128, 1), acts=("relu", "relu", "linear"),
                              compute="bfloat16"),
    "f32 16x128x128x128x1": dict(input_dim=16, units=(128, 128, 128, 1), acts=("elu", "elu", "elu", "linear"),
                                 compute="float32"),
}
LOOPS = (64, 256)
GROUPS = (1, 4)
CASES = [(n, L, G) for n in NETS for L in LOOPS for G in GROUPS]
SETTINGS = dict(n_init=10, epochs=20, num_samples=1024, num_starts=3, options=dict(maxiter=100, ftol=1e-9))
WARMUP, ITERS, REPS = 2, 5, 5
LIMIT_S = 120


def quadratic(X):
    import numpy as np
    return np.sum((X - 0.3) ** 2, axis=-1)


def child(net, L, G):
    import numpy as np
    import torch

    from bore_amd import _lib, ops
    from bore_amd.engine import NativeEngine, ReplicaEngine

    torch.cuda.set_device(0)
    kw = dict(NETS[net], objective=quadratic, groups=G, **SETTINGS)
    ids = np.arange(L)
    engines = dict(native=NativeEngine(ids, **kw), replica=ReplicaEngine(ids, mode="device", select="device", **kw))
    for e in engines.values():
        e.run(WARMUP)
    torch.cuda.synchronize()
    times = {k: [] for k in engines}
    for _ in range(REPS):
        for k, e in engines.items():
            t0 = time.perf_counter()
            e.run(ITERS)
            times[k].append(1e3 * (time.perf_counter() - t0) / ITERS)
    same = bool(np.array_equal(engines["native"].X, engines["replica"].X))
    desc = _lib.make_desc(kw["input_dim"], list(kw["units"]), list(kw["acts"]), compute=kw["compute"])
    res = dict(network=net, loops=L, groups=G, streamed_mask=ops.mlp_streamed(desc), same_observations=same,
               ms_per_iteration={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
                                 for k, v in times.items()})
    res["replica_over_native"] = res["ms_per_iteration"]["replica"]["median"] / res["ms_per_iteration"]["native"]["median"]
    engines["native"].close()
    print("RESULT " + json.dumps(res))


def main(out):
    results = []
    os.makedirs(os.path.dirname(out), exist_ok=True)
    for net, L, G in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", net, str(L), str(G)],
                           capture_output=True, text=True, timeout=LIMIT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"{net}, {L} loops, {G} groups: exit status {p.returncode}; nothing more is run")
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        print(json.dumps(results[-1]), flush=True)
        with open(out, "w") as f:
            json.dump(dict(note=f"ms per BO iteration of all loops: wall clock around run({ITERS}), the two engines "
                                f"alternating, median of {REPS} after {WARMUP} warm-up iterations; settings below",
                           settings=SETTINGS, results=results), f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "engine_nets", "engine_nets_time.json"))
