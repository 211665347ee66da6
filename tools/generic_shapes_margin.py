"""profiles/generic_shapes/oracle_margin.json: tests/test_gpu_generic_shapes.py's comparisons with the float32 oracle in
the kernel's place (CPU only; python tools/generic_shapes_margin.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from test_gpu_generic_shapes import oracle_margins  # noqa: E402

out = {k: {c: float("%.4g" % r) for c, r in v.items()} for k, v in oracle_margins().items()}
os.makedirs(os.path.join(ROOT, "profiles", "generic_shapes"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "generic_shapes", "oracle_margin.json"), "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print({k: max(v.values()) for k, v in out.items() if k not in ("output_std", "fit_l2_swap")},
      "min output std %.3g, min l2 swap %.3g" % (min(out["output_std"].values()), min(out["fit_l2_swap"].values())))
