"""What a weighted fit of a static shape costs on the static kernels (GPU box): ms per ``ops.mlp_fit`` of one model,
N = 100, batch_size 64, 200 epochs, at 2->16-16-1 and 16->32-32-32-1 -- device events after a warm-up, the routes
alternating inside every repetition, median of REPS.

  a  unweighted            the static kernel, this build
  b  weighted static       sample weights uniform on [0, 3]: the static kernel, this build
  c  weighted generic      the same request with BORE_FIT_WEIGHTED_STATIC=0: flavour 0, this build
  d  weighted, other tree  the same request in another checkout of this project (the parent commit's, built), where
                           every weighted fit is flavour 0: a child process in that tree, so that it loads its own
                           Python and its own libbore_hip.so, once before and once after this build's runs

usage: python tools/weighted_static_fit_time.py [--other TREE] [out.json]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, N, B, E = 11, 100, 64, 200
NETS = {"2->16-16-1": (2, [16, 16, 1], ["relu", "relu", "sigmoid"]),
        "16->32-32-32-1": (16, [32, 32, 32, 1], ["elu", "elu", "elu", "linear"])}
LIMIT_S = 120


def summary(v):
    import numpy as np
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)),
                spread=float((np.max(v) - np.min(v)) / np.median(v)))


def measure(tree, routes):
    """{net: {route: [ms] * REPS}} and the bits' agreement, with bore_amd taken from `tree`."""
    sys.path.insert(0, tree)
    import numpy as np
    import torch

    from bore_amd import _lib, ops

    for var in ("BORE_STREAM", "BORE_FIT_PAD", "BORE_FIT_W8", "BORE_FIT_WEIGHTED_STATIC"):
        os.environ.pop(var, None)
    res = {}
    for net, (D, units, acts) in NETS.items():
        rs = np.random.RandomState(0)
        desc = _lib.make_desc(D, units, acts)
        P = ops.param_count(desc)
        X = torch.from_numpy(rs.uniform(size=(1, N, D)).astype(np.float32)).cuda()
        z = torch.from_numpy((rs.uniform(size=(1, N)) < 0.25).astype(np.float32)).cuda()
        W = torch.from_numpy(rs.uniform(0, 3, size=(1, N)).astype(np.float32)).cuda()
        th0 = torch.from_numpy(rs.normal(scale=0.2, size=(1, P)).astype(np.float32)).cuda()

        def one(route, epochs, timed):
            if route == "c":
                os.environ["BORE_FIT_WEIGHTED_STATIC"] = "0"
            th = th0.clone()
            m, v = torch.zeros_like(th), torch.zeros_like(th)
            t = torch.zeros(1, dtype=torch.int64, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.mlp_fit(desc, th, m, v, t, X, z, epochs, B, seed=1, want_loss=False, sample_weight=None if route == "a" else W)
            e1.record()
            torch.cuda.synchronize()
            os.environ.pop("BORE_FIT_WEIGHTED_STATIC", None)
            return e0.elapsed_time(e1) if timed else th

        finals = {r: one(r, 5, False) for r in routes}          # warm-up: code objects loaded, LDS limits raised
        times = {r: [] for r in routes}
        for _ in range(REPS):
            for r in routes:
                times[r].append(one(r, E, True))
        res[net] = dict(ms=times)
        if "b" in routes and "c" in routes:
            res[net]["weighted_static_equals_weighted_generic"] = torch.equal(finals["b"], finals["c"])
            res[net]["weighted_differs_from_unweighted"] = not torch.equal(finals["b"], finals["a"])
    return res


def other_tree(tree):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], cwd=tree, capture_output=True,
                       text=True, timeout=LIMIT_S, env={k: v for k, v in os.environ.items() if k != "BORE_LIB_PATH"})
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit(f"the weighted fit in {tree}: exit status {p.returncode}; nothing more is run")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main(argv):
    other = None
    if argv[:1] == ["--other"]:
        other, argv = os.path.abspath(argv[1]), argv[2:]
    before = other_tree(other) if other else None
    this = measure(ROOT, ("a", "b", "c"))
    after = other_tree(other) if other else None
    out = dict(workload=f"one model, N {N}, batch_size {B}, {E} epochs, device events, routes alternating, median of {REPS}"
                        + ("; d: a child process in the other tree before and after, 2 x %d repetitions" % REPS if other else ""))
    for net in NETS:
        r = {k: summary(v) for k, v in this[net]["ms"].items()}
        if other:
            r["d"] = summary(before[net]["ms"]["d"] + after[net]["ms"]["d"])
            r["d"]["median_before_ms"] = summary(before[net]["ms"]["d"])["median_ms"]
            r["d"]["median_after_ms"] = summary(after[net]["ms"]["d"])["median_ms"]
            r["b_over_d"] = r["b"]["median_ms"] / r["d"]["median_ms"]
            r["c_over_d"] = r["c"]["median_ms"] / r["d"]["median_ms"]
        r["b_over_a"] = r["b"]["median_ms"] / r["a"]["median_ms"]
        r["c_over_a"] = r["c"]["median_ms"] / r["a"]["median_ms"]
        r["theta_after_warm_up"] = {k: v for k, v in this[net].items() if k != "ms"}
        out[net] = r
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if argv:
        os.makedirs(os.path.dirname(os.path.abspath(argv[0])), exist_ok=True)
        with open(argv[0], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        print("RESULT " + json.dumps(measure(sys.argv[2], ("d",))))
    else:
        main(sys.argv[1:])
