#!/usr/bin/env python3
"""How often does the job board's guess hold?  CPU only.

Per L-BFGS-B iteration that calls formk (wrk set), over the restart problems of config-1 loops (the oracle's BO loop on
Branin as bench.py's CPU baseline runs it, 25 iterations per loop: tests/restart_helper_host.py), on the host build of
lbfgsb.h: was nothing entering or leaving and nfree unchanged (`sets_kept`), had the previous iteration ended with a
BFGS update so that the job could be posted before cauchy (`speculated`), and did the guess hold (`guess_held`).
Every held guess is also checked: formk at the top of the iteration must leave the bytes of the call in its place.

  python tools/restart_helper_prediction.py [--loops 8] [--out profiles/restart_helper/prediction.json]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import restart_helper_host as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restart_helper", "prediction.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        lib = R.build(tmp)
        counts, nit, nfev, problems = R.new_counts(), 0, 0, 0
        for fg, x0 in R.config1_problems(a.loops):
            info = R.run(lib, fg, x0, 0.0, 1.0, counts)
            nit, nfev, problems = nit + info[0], nfev + info[1], problems + 1
    c = dict(zip(R.NAMES, counts.tolist()))
    out = dict(problems=problems, iterations=nit, evaluations=nfev, formk_calls_wrk_set=c["formk"],
               sets_kept=c["sets_kept"], speculated=c["speculated"], guess_held=c["guess_held"],
               same_bytes=c["same_bytes"], mismatch=c["mismatch"], entered_or_left=c["moved"],
               entered_or_left_accepted=c["moved_accepted"], dropped=c["dropped"],
               rate_sets_kept=c["sets_kept"] / max(c["formk"], 1), rate_guess_held=c["guess_held"] / max(c["formk"], 1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
