"""What LFBO weighting costs on one MI355X.
  1. bore_lfbo_labels ("lfbo", normalised) against bore_labels at 512 models of N = 113 rows.  Both launch on torch's
     current stream, so device events time them: a large matrix product is queued first, and the events and BURST
     launches are issued while it runs, so the events bracket the launches' device time back to back and no host time
     between them.  ms per launch, median of 11 bursts after 3 warm-up bursts.
  2. ms per BO iteration of the lock-step engine (NativeEngine, 512 loops, groups=1) at 2->16-16-1 and at
     16->32-32-32-1, weighting=None against "lfbo".  The engine works on streams of its own, where an event recorded
     on torch's stream says nothing, and run() returns only when every loop's objective value of the last iteration
     is known: the iteration is the host's wall time (perf_counter around run(ITERS), a device synchronize on either
     side), median of 11 after a warm-up run.  Device events give the split: the engine's own fit_ms / argmax_ms are
     HIP events on its streams around its two big kernels.  Under a weighting these static-shape networks fit on the
     weighted instantiations of their static kernels (BORE_FIT_WEIGHTED_STATIC=0 in the environment: on the generic
     flavour, as before those existed); fit_ms says what the weighting costs.
Every case runs in a child process of its own under a time limit; the first one that fails ends the run.
Writes profiles/lfbo/lfbo_time.json (or the path given)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NETS = {
    "2x16x16x1": dict(input_dim=2, units=(16, 16, 1), acts=("relu", "relu", "sigmoid")),
    "16x32x32x32x1": dict(input_dim=16, units=(32, 32, 32, 1), acts=("elu", "elu", "elu", "linear")),
}
LOOPS, N_LABELS, REPS, ITERS, BURST = 512, 113, 11, 5, 20
SETTINGS = dict(n_init=10, epochs=100, batch_size=64, num_samples=1024, num_starts=3, gamma=0.25,
                options=dict(maxiter=100, ftol=1e-9))
LIMIT_S = 150


def quadratic(X):
    import numpy as np
    return np.sum((X - 0.3) ** 2, axis=-1)


def summary(v):
    import numpy as np
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def burst_ms(fn, reps, warmup):
    """ms per call of fn on torch's current stream, by device events around BURST calls queued behind a busy device."""
    import torch
    a = torch.randn(8192, 8192, device="cuda")
    out, behind = [], True
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.mm(a, a)
        torch.mm(a, a)              # (several ms of device work: everything below is queued before it ends)
        e0.record()
        for _ in range(BURST):
            fn()
        e1.record()
        queued = not e0.query()     # the product still ran when the last launch was queued: no host time inside
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1) / BURST)
            behind = behind and queued
    return out, behind


def wall_ms(fn, reps):
    """Host wall ms of fn, the device idle before and after."""
    import time

    import torch
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def labels_child():
    import numpy as np
    import torch

    from bore_amd import ops

    torch.cuda.set_device(0)
    y = torch.from_numpy(np.random.RandomState(0).normal(size=(LOOPS, N_LABELS))).cuda()
    plain, q0 = burst_ms(lambda: ops.labels(y, 0.25), REPS, 3)
    lfbo, q1 = burst_ms(lambda: ops.lfbo_labels(y, 0.25, "lfbo", True), REPS, 3)
    res = dict(case="labels", models=LOOPS, N=N_LABELS, launches_per_burst=BURST, all_queued_behind_busy_device=q0 and q1,
               ms=dict(bore_labels=summary(plain), bore_lfbo_labels=summary(lfbo)))
    res["lfbo_over_plain"] = res["ms"]["bore_lfbo_labels"]["median"] / res["ms"]["bore_labels"]["median"]
    print("RESULT " + json.dumps(res))


def engine_child(net, weighting):
    import numpy as np
    import torch

    from bore_amd.engine import NativeEngine

    torch.cuda.set_device(0)
    weighting = None if weighting == "none" else weighting
    eng = NativeEngine(np.arange(LOOPS), groups=1, objective=quadratic, weighting=weighting, **NETS[net], **SETTINGS)
    eng.run(2)
    eng.take_stats()
    ms = [t / ITERS for t in wall_ms(lambda: eng.run(ITERS), REPS)]
    st = eng.take_stats()
    res = dict(case="engine", network=net, weighting=weighting, loops=LOOPS, rows_at_end=eng.N,
               ms_per_iteration=summary(ms), fit_ms_per_iteration=st["fit_ms"] / st["fit_launches"],
               argmax_ms_per_iteration=st["argmax_ms"] / st["argmax_launches"])
    eng.close()
    print("RESULT " + json.dumps(res))


def main(out):
    results = []
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cases = [("--labels",)] + [("--engine", n, w) for n in NETS for w in ("none", "lfbo")]
    for case in cases:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), *case], capture_output=True, text=True,
                           timeout=LIMIT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"{case}: exit status {p.returncode}; nothing more is run")
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        print(json.dumps(results[-1]), flush=True)
        with open(out, "w") as f:
            json.dump(dict(note=f"median of {REPS}.  labels: device events around {BURST} launches queued behind a busy "
                                f"device, ms per launch.  engine: host wall ms per BO iteration of all {LOOPS} loops "
                                f"around run({ITERS}) after 2 warm-up iterations (the engine's streams are its own; "
                                f"run() returns when the iteration's work is done), records growing from "
                                f"{SETTINGS['n_init']} rows; fit / argmax ms: the engine's HIP events.  settings below",
                           settings=SETTINGS, results=results),
                      f, indent=1)
    by = {(r["network"], r["weighting"]): r for r in results if r["case"] == "engine"}
    for n in NETS:
        a, b = by[(n, None)], by[(n, "lfbo")]
        print(f"{n}: iteration {a['ms_per_iteration']['median']:.3f} -> {b['ms_per_iteration']['median']:.3f} ms, "
              f"fit {a['fit_ms_per_iteration']:.3f} -> {b['fit_ms_per_iteration']:.3f} ms "
              f"({b['fit_ms_per_iteration'] / a['fit_ms_per_iteration']:.2f}x)")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--labels":
        labels_child()
    elif len(sys.argv) > 1 and sys.argv[1] == "--engine":
        engine_child(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lfbo", "lfbo_time.json"))
