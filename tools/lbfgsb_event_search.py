#!/usr/bin/env python3
"""Which events of lbfgsb.h (LB_EVENT) can the restart cases reach at all?  CPU only.

Runs the host build of lbfgsb.h, fed the oracle's f and g, over the nets of tests/lbfgsb_paths.py with other seeds and
weight scales than the table's, under every bound pattern, and counts the events per net.  An event with zero hits over
all nets is one the GPU premises cannot ask for: DESIGN.md "Restarts" lists it as not reached by search, with the
number of problems tried.

  python tools/lbfgsb_event_search.py [--seeds 6] [--starts 5] [--out profiles/lbfgsb_paths/cpu_search.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import lbfgsb_host as H  # noqa: E402
import lbfgsb_paths as T  # noqa: E402

SCALES = [(1.0, 3.0), (2.0, 6.0), (1.5, 8.0)]          # (soft, hard)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=6)
    ap.add_argument("--starts", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbfgsb_paths", "cpu_search.json"))
    a = ap.parse_args()
    per_net, total, problems = {}, dict.fromkeys(H.EVENT_NAMES, 0), 0
    for name in list(T.NETS) + ["lstm"]:
        counts, tried = dict.fromkeys(H.EVENT_NAMES, 0), 0
        for seed in range(1000, 1000 + a.seeds):
            for soft, hard in SCALES:
                if name == "lstm":
                    T.LSTM.update(seed=seed, soft=soft, hard=hard)
                else:
                    T.NETS[name] = T.NETS[name][:5] + (seed, soft, hard)
                T._made.pop(name, None)
                rs = np.random.RandomState(seed)
                for pattern in T.PATTERNS:
                    fg = T.oracle_fg(name, pattern in ("f", "g"))
                    for tag, lo, hi in T.bounds_of(pattern, T.dim(name)):
                        for x0 in rs.uniform(-0.1, 1.1, size=(a.starts, T.dim(name))):
                            r = H.minimize(fg, x0, (lo, hi), events=True, **T.opts_for(3 if pattern == "w" else 10))
                            for k, v in r.events.items():
                                counts[k] += v
                            tried += 1
        per_net[name] = dict(problems=tried, events=counts)
        problems += tried
        for k, v in counts.items():
            total[k] += v
        print(name, tried, {k: v for k, v in counts.items() if v}, flush=True)
    out = dict(problems=problems, seeds=a.seeds, starts=a.starts, scales=SCALES, maxiter=T.MAXITER, total=total,
               not_reached=[k for k, v in total.items() if v == 0], per_net=per_net)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("problems", problems, "not reached:", out["not_reached"])


if __name__ == "__main__":
    main()
