"""profiles/numeric_range/oracle_margin.json: tests/test_gpu_numeric_range.py's comparisons with the float32 oracle in the
kernel's place, the float32 oracle's worst Adam ratios per group of the table (which the tests' Adam tolerance reads), and
the sensitivity factors (CPU only; python tools/numeric_range_margin.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numeric_range as NR  # noqa: E402

path = NR.MARGIN_JSON
os.makedirs(os.path.dirname(path), exist_ok=True)


def dump(data):
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


rnd = lambda d: {k: (rnd(v) if isinstance(v, dict) else v if isinstance(v, list) else float("%.4g" % v)) for k, v in d.items()}
# (the Adam ratios first: the tolerances of every fit comparison read them from the file)
adam = rnd(NR.measure_adam_f32_ratio())
dump({"adam_f32_ratio": adam})
NR.f32_adam_ratio.cache_clear()
out = rnd(NR.oracle_margins(adam))
dump(out)
print({k: max(v.values()) for k, v in out.items() if k not in ("dropped", "sensitivity")}, out["sensitivity"])
