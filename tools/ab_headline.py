"""Headline benchmark of another checkout of this project (the parent commit's, built) against this tree's, on one GPU
box: `bench.py --gpus 1 --steps S --warmup W` in each tree in turn -- other, this, this, other, other, ... so that
neither is always the first of a pair -- every run a fresh
process in its own tree under a time limit, so each loads its own Python and its own libbore_hip.so.  The first run
that fails ends everything.  Writes the values, both medians and whether this tree's median lies inside the other's
min .. max spread to profiles/lfbo/ab_headline.txt (or --out).
usage: python tools/ab_headline.py OTHER_TREE [--runs 5] [--steps 100] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 120


def headline(tree, steps, warmup):
    with tempfile.TemporaryDirectory() as tmp:      # (the side file bench_detail_n1.json: not wanted here)
        p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                            "--detail-dir", tmp], cwd=tree, capture_output=True, text=True, timeout=LIMIT_S,
                           env={k: v for k, v in os.environ.items() if k != "BORE_LIB_PATH"})
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit(f"bench.py in {tree}: exit status {p.returncode}; nothing more is run")
    line = json.loads(p.stdout.strip().splitlines()[-1])
    return float(line["value"]), float(line["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="parent", help="what the other tree is called in the file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lfbo", "ab_headline.txt"))
    a = ap.parse_args()
    trees = ((a.label, os.path.abspath(a.other)), ("this", ROOT))
    res = {name: [] for name, _ in trees}
    for i in range(a.runs):
        for name, tree in (trees if i % 2 == 0 else trees[::-1]):     # (other, this, this, other, ...: neither is always first)
            res[name].append(headline(tree, a.steps, a.warmup))
            print(f"run {i + 1} {name:8s} {res[name][-1][0]:10.0f} it/s  {res[name][-1][1]:.4f} ms per step", flush=True)
    med = {name: statistics.median(v for v, _ in r) for name, r in res.items()}
    lo, hi = min(v for v, _ in res[a.label]), max(v for v, _ in res[a.label])
    inside = lo <= med["this"] <= hi
    text = [f"bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup} (headline, BO-iterations/s), one MI355X, one session,",
            f"{a.label} and this tree alternating ({a.label}, this, this, {a.label}, ...), {a.runs} runs each, every run a fresh",
            "process in its own checkout (its own Python, its own libbore_hip.so).  tools/ab_headline.py.", ""]
    for name, _ in trees:
        text.append(f"  {name:8s}" + " ".join(f"{v:9.0f}" for v, _ in res[name]) + f"    median {med[name]:9.0f}"
                    + (f"   spread {lo:.0f} .. {hi:.0f}" if name == a.label else "")
                    + "   (ms per step " + " ".join(f"{m:.4f}" for _, m in res[name]) + ")")
    text += ["", f"  this tree's median {'lies inside' if inside else 'LIES OUTSIDE'} the spread of the {a.label}'s runs "
                 f"({100 * (med['this'] / med[a.label] - 1):+.2f} % against the {a.label}'s median)."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))
    return 0 if inside else 1


if __name__ == "__main__":
    sys.exit(main())
