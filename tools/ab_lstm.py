"""A/B of two builds of libbore_hip.so on the recurrent classifier, both flavours (lstm_*, lstm_stream_*) and all four
entry points: bit-identity of every result, then the timings of tools/lstm_time.py and tools/lstm_stream_time.py under
either library (needs the GPU).  usage: python tools/ab_lstm.py [other] [--no-time] [--out=DIR]  (one child per library through
BORE_LIB_PATH, the libraries alternating, twice: the shipped one and bore_amd/csrc/libbore_hip_<other>.so, default prev)

The inputs are small and take every path the scalar helpers of lstm_math.h sit on: 3 inputs, 2 cells of 5 units (so
in_dim differs between the cells), 3 steps, 2 models, each of the five activations; forward (many-to-many with masked
steps, one-to-one) and value + input gradient (three transforms x negate) over 135 rows = two tiles and a tail of 7;
a fit of N = 70 in batches of 32 (a tail batch of 6) over 3 epochs with distinct l2 factors on a cell kernel, a cell
bias and the head, masked steps, one row masked throughout and the epoch losses; evaluate on the fit's data.
The dumped arrays and the timers' JSON go to DIR (default: a fresh temporary directory)."""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, H, L, T, M, ROWS, N, B, E, MV = 3, 5, 2, 3, 2, 135, 70, 32, 3, -1.0
TIMERS = ("lstm_time", "lstm_stream_time")


def child(tag, OUT):
    import numpy as np, torch
    from bore_amd import _lib, ops
    out = {}
    for flavour in ("lstm_", "lstm_stream_"):
        op = lambda name: getattr(ops, flavour + name)  # noqa: E731
        for act in ("linear", "relu", "elu", "sigmoid", "tanh"):
            rs = np.random.RandomState(11)
            desc = _lib.make_lstm_desc(D, L, H, act, l2_kernel=[1e-3, 0.0, 2e-3], l2_bias=[0.0, 5e-4, 7e-4])
            P = ops.lstm_param_count(desc)
            cuda = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
            th = cuda(rs.normal(scale=0.5, size=(M, P)).astype(np.float32))
            key = lambda name: f"{flavour}{act}_{name}"  # noqa: E731
            Xs = rs.uniform(-1.0, 1.0, size=(M, ROWS, T, D)).astype(np.float32)
            Xs[:, 3, 0] = Xs[:, 70, 1] = Xs[:, 134, 2] = Xs[:, 5] = MV    # leading, middle, trailing; a whole row
            out[key("forward_m2m")] = op("forward")(desc, th, cuda(Xs), mask_value=MV).cpu().numpy()
            x1 = rs.uniform(-1.0, 1.0, size=(M, ROWS, D))
            out[key("forward_121")] = op("forward")(desc, th, cuda(x1.astype(np.float32)), num_steps=T).cpu().numpy()
            for tr in ("identity", "sigmoid", "exp"):
                for neg in (False, True):
                    val, grad = op("value_and_input_grad")(desc, th, cuda(x1), T, tr, neg)
                    out[key(f"val_{tr}_{int(neg)}")], out[key(f"grad_{tr}_{int(neg)}")] = val.cpu().numpy(), grad.cpu().numpy()
            X = rs.uniform(-1.0, 1.0, size=(M, N, T, D)).astype(np.float32)
            X[:, 1, 0] = X[:, 40, 1] = X[:, 69, 2] = X[:, 33] = MV
            X, y = cuda(X), cuda((rs.uniform(size=(M, N, T)) < 0.4).astype(np.float32))
            m, v = torch.zeros_like(th), torch.zeros_like(th)
            t = torch.zeros(M, dtype=torch.int64, device="cuda")
            perm = ops.shuffle_perm(5, M, E, N)
            losses = op("fit")(desc, th, m, v, t, X, y, E, B, perm, mask_value=MV, want_loss=True)
            loss, acc = op("evaluate")(desc, th, X, y, mask_value=MV)
            for name, a in (("theta", th), ("m", m), ("v", v), ("t", t), ("epoch_loss", losses), ("loss", loss), ("acc", acc)):
                out[key(name)] = a.cpu().numpy()
    np.savez(os.path.join(OUT, f"ab_lstm_{tag}.npz"), **out)
    print(f"{tag}: {len(out)} arrays", flush=True)


def leaves(d, prefix=""):
    for k, v in d.items():
        if isinstance(v, dict) and "median" in v and "min" in v:
            yield prefix + k, v
        elif isinstance(v, dict):
            yield from leaves(v, prefix + k + " ")
        elif isinstance(v, float):
            yield prefix + k, dict(median=v, min=v, max=v)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    import numpy as np
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    other = args[0] if args else "prev"
    libs = {"new": os.path.join(ROOT, "bore_amd", "csrc", "libbore_hip.so"),
            "prev": os.path.join(ROOT, "bore_amd", "csrc", f"libbore_hip_{other}.so")}
    OUT = next((a[6:] for a in sys.argv[1:] if a.startswith("--out=")), None) or tempfile.mkdtemp(prefix="ab_lstm_")
    os.makedirs(OUT, exist_ok=True)
    runs = [(tag, path, rnd) for rnd in (1, 2) for tag, path in libs.items()]  # (twice, alternating)
    for tag, path, rnd in runs:
        subprocess.run([sys.executable, __file__, "--child", f"{tag}{rnd}", OUT], env=dict(os.environ, BORE_LIB_PATH=path),
                       check=True, timeout=300)
    ref = np.load(os.path.join(OUT, "ab_lstm_prev1.npz"))
    different = 0
    for name in ("new1", "new2", "prev2"):      # (prev2: the parent against itself, run to run)
        a = np.load(os.path.join(OUT, f"ab_lstm_{name}.npz"))
        diff = [k for k in ref.files if not np.array_equal(a[k], ref[k])]
        different += len(diff) if name != "prev2" else 0
        print(f"{name} against prev1: {len(ref.files) - len(diff)} of {len(ref.files)} arrays bit-identical"
              + "".join(f"\n  DIFFERENT {k}: max abs diff {np.abs(a[k].astype(np.float64) - ref[k]).max():g}" for k in diff))
    if "--no-time" not in sys.argv:
        for tag, path, rnd in runs:
            for tool in TIMERS:
                subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool + ".py"),
                                os.path.join(OUT, f"{tool}_{tag}{rnd}.json")], env=dict(os.environ, BORE_LIB_PATH=path),
                               check=True, timeout=300, stdout=subprocess.DEVNULL)
        for tool in TIMERS:
            t = {f"{tag}{rnd}": dict(leaves(json.load(open(os.path.join(OUT, f"{tool}_{tag}{rnd}.json")))))
                 for tag, _, rnd in runs}
            print(f"{tool}: parent's min .. max over its two children | this build's two medians")
            for k in t["prev1"]:
                if k.startswith(("shape", "floor")) or k in ("steps", "N", "batch_size", "rows", "repeats"):
                    continue
                lo = min(t["prev1"][k]["min"], t["prev2"][k]["min"])
                hi = max(t["prev1"][k]["max"], t["prev2"][k]["max"])
                meds = [t["new1"][k]["median"], t["new2"][k]["median"]]
                flag = "".join("  OUTSIDE by %+.2f %%" % (100 * (m - (hi if m > hi else lo)) / (hi if m > hi else lo))
                               for m in meds if not lo <= m <= hi)
                print(f"  {k:60s} {lo:10.4f} .. {hi:10.4f} | {meds[0]:10.4f} {meds[1]:10.4f}{flag}")
    sys.exit(1 if different else 0)
