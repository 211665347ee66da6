"""Timings of both flavours of the multi-fidelity classifier on one MI355X (device events, after warm-up):
ms per Adam step at N = 64, B = 64 (one step per epoch), ms per 1024-row value + input gradient and ms per 1024-row
one-to-one forward.  The plugin default 16->2x32 over 5 steps in BOTH flavours, alternating them repeat by repeat in
the same process (the LDS figure is the comparison point), and the streamed flavour alone at 48->2x32 and 16->2x64,
which the LDS kernels refuse.  Writes profiles/lstm/lstm_stream_time.json (or the path given): the median of the
repeats and their range."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bore_amd import _lib, ops  # noqa: E402

T, N, B, STEPS, ROWS, REPEATS = 5, 64, 64, 200, 1024, 7


def events(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def workloads(D, H, L, flavour):
    """{name: (callable, calls per timed window, units of work per call)} of one network on one flavour."""
    op = lambda name: getattr(ops, ("lstm_stream_" if flavour == "streamed" else "lstm_") + name)  # noqa: E731
    desc = _lib.make_lstm_desc(D, L, H, "elu")
    P = ops.lstm_param_count(desc)
    rs = np.random.RandomState(0)
    th0 = torch.from_numpy(rs.uniform(-0.1, 0.1, size=(1, P)).astype(np.float32)).cuda()
    th = th0.clone()
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    X = torch.from_numpy(rs.uniform(size=(1, N, T, D)).astype(np.float32)).cuda()
    y = torch.from_numpy((rs.uniform(size=(1, N, T)) < 0.3).astype(np.float32)).cuda()
    perm = ops.shuffle_perm(1, 1, STEPS, N)
    Xg = torch.from_numpy(rs.uniform(size=(1, ROWS, D))).cuda()
    Xf = Xg.to(torch.float32)
    return dict(
        fit_ms_per_step=(lambda: op("fit")(desc, th, m, v, t, X, y, STEPS, B, perm, mask_value=-1.0, want_loss=False),
                         2, STEPS),
        value_and_input_grad_1024_ms=(lambda: op("value_and_input_grad")(desc, th0, Xg, T, "sigmoid", True), 20, 1),
        forward_1024_ms=(lambda: op("forward")(desc, th0, Xf, num_steps=T), 20, 1))


def main(out):
    torch.cuda.set_device(0)
    nets = [((16, 32, 2), ("lds", "streamed")), ((48, 32, 2), ("streamed",)), ((16, 64, 2), ("streamed",))]
    res = dict(steps=T, N=N, batch_size=B, adam_steps_per_fit_call=STEPS, rows=ROWS, repeats=REPEATS, networks={})
    for (D, H, L), flavours in nets:
        assert ops.lstm_streamed(_lib.make_lstm_desc(D, L, H, "elu"), T) == (0 if "lds" in flavours else 1)
        work = {f: workloads(D, H, L, f) for f in flavours}
        times = {f: {k: [] for k in work[f]} for f in flavours}
        for f in flavours:                       # warm-up: every kernel and shape of the timed windows
            for fn, _, _ in work[f].values():
                fn()
        torch.cuda.synchronize()
        for _ in range(REPEATS):                 # the flavours alternate repeat by repeat
            for f in flavours:
                for k, (fn, calls, units) in work[f].items():
                    times[f][k].append(events(fn, calls) / units)
        res["networks"]["%d->%dx%d" % (D, L, H)] = {
            f: {k: dict(median=float(np.median(ts)), min=float(min(ts)), max=float(max(ts)))
                for k, ts in times[f].items()} for f in flavours}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lstm", "lstm_stream_time.json"))
