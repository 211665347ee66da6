"""Classifier ensembles on one MI355X: what K members cost.

  fit      EnsembleSequential(members=K).fit for K in 1, 4, 8, 16 against one Sequential.fit: N = 100 rows, 200 epochs,
           batch_size 64, networks 2->16-16-1 (relu) and 16->32-32-32-1 (elu), logit heads.  The claim under test: "K
           members in about the time of one" (one workgroup per member, K <= the device's compute units).
  maxima   5 restarts from 1 024 candidates, transform identity and sigmoid, after a short fit: the ensemble's device
           route (bore_ensemble_screen_topk + bore_ensemble_lbfgsb_minimize) for K in 1, 4, 8, against
           MaximizableSequential.maxima of ONE model (its device route: the code path of the parent commit, untouched)
           and against the ensemble's own lock-step route (restart_mode="lockstep", screen_mode="host": one
           ops.mlp_value_and_input_grad launch of K models per round, the statement on the host).

Wall clock around calls that end in a device synchronise, and device events around the same calls (the fit: the launch
alone; maxima returns host results, so its device time is not separable and only the wall clock is given); the routes of
a group ALTERNATE call by call; the median of REPS calls of each after WARMUP of each.  Writes
profiles/ensemble/ensemble_time.json (or the path given)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NETS = {"2x16x16x1": (2, [16, 16], "relu"), "16x32x32x32x1": (16, [32, 32, 32], "elu")}
WARMUP, REPS = 2, 11
N, EPOCHS, BATCH = 100, 200, 64


def main(out):
    import numpy as np
    import torch
    from scipy.optimize import Bounds

    from bore_amd import _lib
    from bore_amd.layers import BinaryCrossentropy, Dense
    from bore_amd.models import MaximizableEnsembleSequential, MaximizableSequential

    torch.cuda.set_device(0)

    def make(net, transform, K=None):
        D, hidden, act = NETS[net]
        m = MaximizableSequential(transform, seed=1) if K is None else \
            MaximizableEnsembleSequential(transform, members=K, beta=1.0, seed=1)
        for u in hidden:
            m.add(Dense(u, activation=act))
        m.add(Dense(1))
        m.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True))
        m.build(D)
        return m

    def alternate(calls):
        """{name: callable} -> {name: dict(wall ms, device ms)}: the callables alternating, each ending synchronised."""
        wall, devt = {k: [] for k in calls}, {k: [] for k in calls}
        for rep in range(WARMUP + REPS):
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= WARMUP:
                    wall[name].append(1e3 * (time.perf_counter() - t0))
                    devt[name].append(e0.elapsed_time(e1))
        return {k: dict(ms_wall_median=float(np.median(wall[k])), ms_wall_min=float(np.min(wall[k])),
                        ms_wall_max=float(np.max(wall[k])), ms_device_median=float(np.median(devt[k]))) for k in calls}

    results = dict(fit=[], maxima=[])
    for net, (D, hidden, act) in NETS.items():
        rs = np.random.RandomState(0)
        X = rs.uniform(size=(N, D))
        y = np.sum((X - 0.4) ** 2, axis=1)
        z = (y < np.quantile(y, 0.25)).astype(np.float32)
        # ---- fit ----
        models = {"single": make(net, "identity")}
        models.update({f"K={K}": make(net, "identity", K) for K in (1, 4, 8, 16)})
        r = alternate({k: (lambda m=m: m.fit(X, z, epochs=EPOCHS, batch_size=BATCH)) for k, m in models.items()})
        for k in r:
            r[k]["over_single_wall"] = r[k]["ms_wall_median"] / r["single"]["ms_wall_median"]
            r[k]["over_single_device"] = r[k]["ms_device_median"] / r["single"]["ms_device_median"]
        results["fit"].append(dict(net=net, N=N, epochs=EPOCHS, batch_size=BATCH, routes=r))
        print(json.dumps(results["fit"][-1]), flush=True)
        # ---- maxima ----
        bounds = Bounds(np.zeros(D), np.ones(D))
        for transform in ("identity", "sigmoid"):
            calls, last = {}, {}

            def add(name, m):
                m.fit(X, z, epochs=50, batch_size=BATCH)

                def run():
                    last[name] = m.maxima(bounds, num_starts=5, num_samples=1024, print_fn=lambda s: None,
                                          random_state=np.random.RandomState(7))
                calls[name] = run

            add("single", make(net, transform))
            for K in (1, 4, 8):
                add(f"K={K} device", make(net, transform, K))
                m = make(net, transform, K)
                m.restart_mode, m.screen_mode = "lockstep", "host"
                add(f"K={K} lockstep", m)
            r = alternate(calls)
            for k in r:
                del r[k]["ms_device_median"]           # (maxima waits for the device inside: the wall clock is the time)
                r[k]["over_single"] = r[k]["ms_wall_median"] / r["single"]["ms_wall_median"]
                r[k]["nit"] = [int(s.nit) for s in last[k]]
                r[k]["nfev"] = [int(s.nfev) for s in last[k]]
                r[k]["fun"] = [float(s.fun) for s in last[k]]
            for K in (1, 4, 8):
                r[f"K={K} device"]["lockstep_over_device"] = \
                    r[f"K={K} lockstep"]["ms_wall_median"] / r[f"K={K} device"]["ms_wall_median"]
            results["maxima"].append(dict(net=net, transform=transform, num_starts=5, num_samples=1024, routes=r))
            print(json.dumps(results["maxima"][-1]), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(note=f"one MI355X; ms per call; the routes of a group alternating, median of {REPS} after {WARMUP} "
                            "warm-up calls of each; wall clock around a call that ends synchronised, device events around "
                            "the same call", source_digest=_lib.source_digest(), **results), f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ensemble", "ensemble_time.json"))
