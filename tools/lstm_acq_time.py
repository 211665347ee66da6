"""Time of `maxima` for the one-to-one recurrent network on one MI355X, by route:
  device    acquisition="device": screening and restarts on the streamed LSTM kernels
            (bore_lstm_stream_screen_topk + bore_lstm_stream_lbfgsb_minimize)
  lockstep  the default: predict + argpartition, then SciPy's L-BFGS-B state machines in lock-step around
            bore_lstm[_stream]_value_and_input_grad
16->2x32 (fits LDS: the default route runs the LDS kernels, the device route the streamed ones) and 48->2x32 (streamed
on both routes), T = 5, after a short fit; num_starts 5, num_samples 1024, transform identity and the plugin's
sigmoid.  Wall clock around the call (it returns host results: the device is idle again when it does), the two routes
ALTERNATING call by call, the median of REPS calls of each after WARMUP of each, the same candidates in every call;
nit / nfev of every restart of both routes side by side.  Beside them, for the estimate of where a round goes: a
five-row value + input gradient call of the streamed flavour, as the host sees it (launch, wait, download: what a
lock-step round pays besides SciPy) and as the device sees it (events around 20 back-to-back launches: what a pass of
the device route's round costs, its rows being four).
Every (shape, transform) runs in a child process of its own under a time limit; the first one that fails ends the run.
Writes profiles/lstm/lstm_acq_time.json (or the path given)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"16x2x32": 16, "48x2x32": 48}      # input dimensions; two cells of 32 units, elu
T = 5
CASES = [(s, t) for s in SHAPES for t in ("identity", "sigmoid")]
LIMIT_S = 240
WARMUP, REPS = 2, 9


def child(shape, transform):
    import numpy as np
    import torch
    from scipy.optimize import Bounds

    from bore_amd import ops
    from bore_amd.layers import BinaryCrossentropy
    from bore_amd.models import StackedRecurrentFactory

    torch.cuda.set_device(0)
    D = SHAPES[shape]
    rs = np.random.RandomState(0)
    factory = StackedRecurrentFactory(input_dim=D, output_dim=1, num_layers=2, num_units=32,
                                      layer_kws=dict(activation="elu"), seed=1)
    net = factory.build_many_to_many()
    net.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True))
    net.fit(rs.uniform(size=(64, T, D)), rs.randint(2, size=(64, T, 1)), epochs=10, batch_size=16)
    nets = dict(device=factory.build_one_to_one(T, transform=transform, acquisition="device"),
                lockstep=factory.build_one_to_one(T, transform=transform))
    bounds = Bounds(lb=np.zeros(D), ub=np.ones(D))
    res = dict(shape=shape, T=T, transform=transform, num_starts=5, num_samples=1024,
               lstm_streamed=int(ops.lstm_streamed(factory._desc, T)), routes={})
    times, out = dict(device=[], lockstep=[]), {}
    for rep in range(WARMUP + REPS):
        for route in ("device", "lockstep"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[route] = nets[route].maxima(bounds, num_starts=5, num_samples=1024, print_fn=lambda s: None,
                                            random_state=np.random.RandomState(7))
            torch.cuda.synchronize()
            if rep >= WARMUP:
                times[route].append(1e3 * (time.perf_counter() - t0))
    for route in ("device", "lockstep"):
        res["routes"][route] = dict(ms_median=float(np.median(times[route])), ms_min=float(np.min(times[route])),
                                    ms_max=float(np.max(times[route])), nit=[int(r.nit) for r in out[route]],
                                    nfev=[int(r.nfev) for r in out[route]], fun=[float(r.fun) for r in out[route]])
    res["lockstep_over_device"] = res["routes"]["lockstep"]["ms_median"] / res["routes"]["device"]["ms_median"]
    # one five-row f/g call of the streamed flavour: as a lock-step round pays for it, and the launch alone
    Xd = torch.from_numpy(rs.uniform(size=(1, 5, D))).cuda()
    call = lambda: ops.lstm_stream_value_and_input_grad(factory._desc, factory.theta, Xd, T, transform, True)  # noqa: E731
    wall = []
    for rep in range(WARMUP + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v, g = call()
        v.cpu(), g.cpu()
        if rep >= WARMUP:
            wall.append(1e3 * (time.perf_counter() - t0))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        call()
    e1.record()
    torch.cuda.synchronize()
    res["fg_five_rows"] = dict(ms_host_round_trip_median=float(np.median(wall)), ms_device_per_launch=e0.elapsed_time(e1) / 20)
    print("RESULT " + json.dumps(res))


def main(out):
    results = []
    for shape, transform in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, transform],
                           capture_output=True, text=True, timeout=LIMIT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"{shape} {transform}: exit status {p.returncode}; nothing more is run")
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(note="one model per call; ms of one maxima(num_starts=5, num_samples=1024), wall clock, the two "
                            f"routes alternating, median of {REPS} after {WARMUP} warm-up calls of each",
                       results=results), f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lstm", "lstm_acq_time.json"))
