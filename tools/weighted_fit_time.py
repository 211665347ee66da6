"""What a weighted fit costs (GPU box): ms per ``ops.mlp_fit`` of 16->32-32-32-1 elu, N = 100, batch_size 64, 200 epochs,
on the routes a request can take -- device events after a warm-up, the routes alternating inside every repetition,
median of REPS.

  static              unweighted, as shipped: static shape 5 (eight waves for one model)
  generic w4 / w8     unweighted on the generic flavour with four / eight waves.  An exact static shape has no switch
                      that sends it there, so the descriptor carries an l2 factor of 1e-30 on the output bias: it
                      matches no static shape any more and moves no bit of the result (the penalty and its gradient
                      underflow against every sum they meet), but the kernel does the per-step penalty work
  weighted            sample weights uniform on [0, 3]: flavour 0, four waves
  weighted l2         the same on the l2 descriptor: the like-for-like partner of "generic w4"

usage: python tools/weighted_fit_time.py [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bore_amd import _lib, ops

REPS = 11
D, UNITS, ACTS, N, B, E = 16, [32, 32, 32, 1], ["elu", "elu", "elu", "linear"], 100, 64, 200
os.environ.pop("BORE_STREAM", None)
os.environ.pop("BORE_FIT_PAD", None)
rs = np.random.RandomState(0)
plain = _lib.make_desc(D, UNITS, ACTS)
tiny = [0.0, 0.0, 0.0, 1e-30]
with_l2 = _lib.make_desc(D, UNITS, ACTS, None, tiny)
P = ops.param_count(plain)
X = torch.from_numpy(rs.uniform(size=(1, N, D)).astype(np.float32)).cuda()
z = torch.from_numpy((rs.uniform(size=(1, N)) < 0.25).astype(np.float32)).cuda()
W = torch.from_numpy(rs.uniform(0, 3, size=(1, N)).astype(np.float32)).cuda()
th0 = torch.from_numpy(rs.normal(scale=0.2, size=(1, P)).astype(np.float32)).cuda()

ROUTES = {  # name -> (descriptor, BORE_FIT_W8 or None, sample weights)
    "static": (plain, None, None),
    "generic_w4": (with_l2, "0", None),
    "generic_w8": (with_l2, "1", None),
    "weighted": (plain, None, W),
    "weighted_l2": (with_l2, None, W),
}


def one(route, epochs, timed):
    desc, w8, sw = ROUTES[route]
    if w8 is None:
        os.environ.pop("BORE_FIT_W8", None)
    else:
        os.environ["BORE_FIT_W8"] = w8
    th = th0.clone()
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ops.mlp_fit(desc, th, m, v, t, X, z, epochs, B, seed=1, want_loss=False, sample_weight=sw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) if timed else th


finals = {r: one(r, 5, False) for r in ROUTES}          # warm-up: code objects loaded, LDS limits raised
# the l2 factor moves no bit, and the generic flavours agree with the static kernel (the project's invariant)
same = dict(generic_w4_equals_static=torch.equal(finals["static"], finals["generic_w4"]),
            generic_w8_equals_static=torch.equal(finals["static"], finals["generic_w8"]),
            weighted_l2_equals_weighted=torch.equal(finals["weighted"], finals["weighted_l2"]),
            weighted_differs_from_static=not torch.equal(finals["weighted"], finals["static"]))
times = {r: [] for r in ROUTES}
for _ in range(REPS):
    for r in ROUTES:
        times[r].append(one(r, E, True))
out = {r: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v))) for r, v in times.items()}
out["ratio_weighted_l2_over_generic_w4"] = out["weighted_l2"]["median_ms"] / out["generic_w4"]["median_ms"]
out["ratio_weighted_over_generic_w4"] = out["weighted"]["median_ms"] / out["generic_w4"]["median_ms"]
out["ratio_generic_w4_over_static"] = out["generic_w4"]["median_ms"] / out["static"]["median_ms"]
out["ratio_weighted_over_static"] = out["weighted"]["median_ms"] / out["static"]["median_ms"]
out["theta_after_warm_up"] = same
out["workload"] =f"{D}->{'-'.join(map(str, UNITS))} elu, N {N}, batch_size {B}, {E} epochs, median of {REPS}"
text = json.dumps(out, indent=1)
print(text, flush=True)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
