"""Timings of the streamed flavour (bore_amd/csrc/bore_stream.hip) on one MI355X, device events after warm-up:
ms per Adam step of 16->128-128-128-1 and 8->256-256-1 at N = 64 and 200 (batch_size 64, one model = one
workgroup = one CU), a 1024-row forward and a 1024-row value + input gradient of each.
Every measurement runs in a child process of its own under a time limit; the first one that fails ends the run.
Writes profiles/stream/stream_time.json (or the path given)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "16x128x128x128x1": (16, [128, 128, 128, 1], ["elu", "elu", "elu", "linear"]),
    "8x256x256x1": (8, [256, 256, 1], ["relu", "relu", "linear"]),
}
CASES = [(s, c) for s in SHAPES for c in ("fit_N64", "fit_N200", "forward_1024", "value_and_input_grad_1024")]
LIMIT_S = 120

# One CU's floors (the streamed kernels): fp32 MFMA 256 flop / cycle at 2.4 GHz, and ~70 GB/s of
# L2 reads per CU.  An Adam step at 64 rows: 3 products of 2 x 64 x P flop; theta read three times (forward,
# backward, update), m and v read and written, theta written: 32 P bytes.
CU_FLOPS, CU_L2_BYTES = 256 * 2.4e9, 70e9


def floors(P, rows):
    return dict(arithmetic_us=1e6 * 6.0 * rows * P / CU_FLOPS, bytes_us=1e6 * 32.0 * P / CU_L2_BYTES)


def child(shape, case):
    import numpy as np
    import torch

    from bore_amd import _lib, ops

    def events(fn, reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / reps

    torch.cuda.set_device(0)
    D, units, acts = SHAPES[shape]
    desc = _lib.make_desc(D, units, acts)
    assert ops.mlp_streamed(desc) == 7
    P = ops.param_count(desc)
    rs = np.random.RandomState(0)
    th = torch.from_numpy(rs.uniform(-0.1, 0.1, size=(1, P)).astype(np.float32)).cuda()
    res = dict(shape=shape, case=case, P=P)
    if case.startswith("fit_N"):
        N, B = int(case[5:]), 64
        steps_per_epoch = -(-N // B)
        epochs = 200 // steps_per_epoch
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        t = torch.zeros(1, dtype=torch.int64, device="cuda")
        X = torch.from_numpy(rs.uniform(size=(1, N, D)).astype(np.float32)).cuda()
        z = torch.from_numpy((rs.uniform(size=(1, N)) < 0.3).astype(np.float32)).cuda()
        perm = ops.shuffle_perm(1, 1, epochs, N)
        fit = lambda: ops.mlp_fit(desc, th, m, v, t, X, z, epochs, B, perm=perm, want_loss=False)  # noqa: E731
        fit()
        ms = events(fit, 3)
        n_steps = epochs * steps_per_epoch
        res.update(steps=n_steps, ms_per_fit=ms, ms_per_step=ms / n_steps, floors=floors(P, min(N, B)))
    elif case == "forward_1024":
        Xf = torch.from_numpy(rs.uniform(size=(1024, D)).astype(np.float32)).cuda()
        fw = lambda: ops.mlp_forward(desc, th, Xf)  # noqa: E731
        fw()
        res.update(ms=events(fw, 20))
    else:
        Xg = torch.from_numpy(rs.uniform(size=(1, 1024, D))).cuda()
        vg = lambda: ops.mlp_value_and_input_grad(desc, th, Xg, "sigmoid", True)  # noqa: E731
        vg()
        res.update(ms=events(vg, 20))
    print("RESULT " + json.dumps(res))


def main(out):
    results = []
    for shape, case in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, case], capture_output=True,
                           text=True, timeout=LIMIT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"{shape} {case}: exit status {p.returncode}; nothing more is run")
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(note="one model per launch: one workgroup on one CU, the rest of the device idle",
                       results=results), f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stream", "stream_time.json"))
