"""Record tests/golden/ref_mf_record.npz from the reference's own MultiFidelityRecord (bore/data.py:51-261).

Run once, by hand, where the reference checkout is available (pure numpy: no TensorFlow needed):

    python tests/golden/make_golden_mf.py /path/to/reference

The tests read only the recorded arrays."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def appends():
    """A Hyperband-like append sequence over budgets 1/9, 1/3, 1: three brackets, leading gaps (configs
    first sampled in a higher bracket), trailing gaps (not promoted), a repeated (x, b) and tied values at
    the quantile."""
    rs = np.random.RandomState(5)
    xs = [np.round(rs.uniform(size=3), 6) for _ in range(14)]
    seq = []
    for i in range(9):                            # bracket 0, rung 0
        seq.append((i, float(np.round(rs.uniform(), 3)), 1 / 9))
    seq[3] = (3, 0.25, 1 / 9)
    seq[4] = (4, 0.25, 1 / 9)                     # ties
    for i in (0, 3, 4):                           # promoted to rung 1
        seq.append((i, float(np.round(rs.uniform(), 3)), 1 / 3))
    seq.append((3, 0.5, 1.0))                     # promoted to rung 2
    for i in range(9, 12):                        # bracket 1: starts at rung 1 (leading gaps)
        seq.append((i, float(np.round(rs.uniform(), 3)), 1 / 3))
    seq.append((9, 0.25, 1.0))
    seq.append((12, 0.75, 1.0))                   # bracket 2: starts at the top
    seq.append((13, 0.125, 1.0))
    seq.append((0, 0.33, 1 / 3))                  # a repeated (x, b)
    return xs, seq


def main(ref_root):
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_data", os.path.join(ref_root, "bore", "data.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    xs, seq = appends()
    rec = mod.MultiFidelityRecord(gamma=1 / 3)
    for i, y, b in seq:
        rec.append(xs[i], y, b)
    out = dict(xs=np.array(xs), seq_index=np.array([s[0] for s in seq]), seq_y=np.array([s[1] for s in seq]),
               seq_b=np.array([s[2] for s in seq]), budgets=np.array(rec.budgets()),
               rung_sizes=np.array(rec.rung_sizes()), thresholds=np.array(rec.thresholds()),
               num_features=np.array(rec.num_features()), size=np.array(rec.size()),
               features=rec.load_feature_matrix())
    for t in range(rec.num_rungs()):
        out[f"binary_labels_{t}"] = np.asarray(rec.binary_labels(t))
        out[f"targets_{t}"] = np.asarray(rec.targets(t))
    out["highest_rung"] = np.array([-1 if rec.highest_rung(min_size=s) is None else rec.highest_rung(min_size=s)
                                    for s in range(0, 14)])
    for name, pad in (("m1", -1.0), ("tiny", 1e-9)):
        for binary in (True, False):
            X, Y = rec.sequences(pad_value=pad, binary=binary)
            out[f"seq_{name}_{int(binary)}_X"] = X
            out[f"seq_{name}_{int(binary)}_Y"] = Y
    probes = np.array([xs[2], xs[2] + 1e-9, xs[2] + 1e-3, np.zeros(3), xs[13]])
    out["dup_probes"] = probes
    out["dup"] = np.array([rec.is_duplicate(p) for p in probes])
    np.savez_compressed(os.path.join(HERE, "ref_mf_record.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BORE_REFERENCE", ".."))
