"""A/B of two builds of libbore_hip.so on the fits: bit-identity of the results and time per Adam step, median
(min .. max) of REPS timed calls (GPU box).  usage: python tools/ab_fit.py [other]  (runs itself once per library:
the shipped one and bore_amd/csrc/libbore_hip_<other>.so, default prev)"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [("shape3_f32", 16, [64, 64, 64, 1], "float32"), ("shape3_bf16", 16, [64, 64, 64, 1], "bfloat16"),
         ("shape4_bf16", 32, [128, 128, 1], "bfloat16"), ("shape2_f32", 6, [32, 32, 1], "float32"),
         ("shape1_f32", 2, [16, 16, 1], "float32"), ("stream_f32", 8, [256, 256, 1], "float32")]  # (the streamed flavour)
REPS = 7


def child(tag):
    import numpy as np, torch
    from bore_amd import _lib, ops
    out = {}
    for name, D, units, compute in CASES:
        rs = np.random.RandomState(7)
        acts = ["relu"] * (len(units) - 1) + ["sigmoid"]
        desc = _lib.make_desc(D, units, acts, compute=compute)
        P = ops.param_count(desc)
        L, N, E = 3, 200, 40
        th = torch.from_numpy(rs.normal(scale=0.2, size=(L, P)).astype(np.float32)).cuda()
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        t = torch.zeros(L, dtype=torch.int64, device="cuda")
        X = torch.from_numpy(rs.uniform(size=(L, N, D)).astype(np.float32)).cuda()
        z = torch.from_numpy((rs.uniform(size=(L, N)) < 0.25).astype(np.float32)).cuda()
        ops.mlp_fit(desc, th, m, v, t, X, z, E, 64, seed=3, want_loss=False)   # also the warm-up
        steps, us = E * -(-N // 64), []
        for r in range(1, REPS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.mlp_fit(desc, th, m, v, t, X, z, E, 64, seed=3, epoch0=r * E, want_loss=False)
            torch.cuda.synchronize()
            us.append(1e6 * (time.perf_counter() - t0) / steps)
        print(f"{tag} {name}: {np.median(us):7.2f} ({min(us):.2f} .. {max(us):.2f}) us per Adam step "
              f"({L} models, N={N}, {REPS} calls)", flush=True)
        out[name + "_th"], out[name + "_m"], out[name + "_v"] = (a.cpu().numpy() for a in (th, m, v))
    np.savez(os.path.join(ROOT, "gpurun_out", f"ab_{tag}.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) > 2:
        child(sys.argv[2])
        sys.exit(0)
    import numpy as np
    other = sys.argv[1] if len(sys.argv) > 1 else "prev"
    libs = {"new": os.path.join(ROOT, "bore_amd", "csrc", "libbore_hip.so"),
            "prev": os.path.join(ROOT, "bore_amd", "csrc", f"libbore_hip_{other}.so")}
    for tag, path in 2 * list(libs.items()):  # (twice, alternating: drift hits both builds alike)
        subprocess.run([sys.executable, __file__, "--child", tag], env=dict(os.environ, BORE_LIB_PATH=path), check=True)
    a, b = (np.load(os.path.join(ROOT, "gpurun_out", f"ab_{t}.npz")) for t in ("new", "prev"))
    for k in a.files:
        same = np.array_equal(a[k], b[k])
        print(f"{k}: {'bit-identical' if same else 'DIFFERENT, max abs diff %g' % np.abs(a[k] - b[k]).max()}")
