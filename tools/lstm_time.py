"""Timings of the multi-fidelity classifier on one MI355X (device events, after warm-up):
us per Adam step and ms per fit at the plugin default (D=16, H=32, L=2, T=5; N 64 and 200; 1000 steps),
ms per 1024-row bore_lstm_value_and_input_grad, and the wall time of one get_config.
Writes profiles/lstm/lstm_time.json (or the path given)."""
import json
import logging
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bore_amd import _lib, ops  # noqa: E402

FLOOR_US = 45.0   # single-CU fp32 arithmetic floor of one Adam step at B=64, T=5 (DESIGN: the LSTM path)


def events(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def main(out):
    torch.cuda.set_device(0)
    D, H, L, T, B = 16, 32, 2, 5, 64
    desc = _lib.make_lstm_desc(D, L, H, "elu")
    P = ops.lstm_param_count(desc)
    rs = np.random.RandomState(0)
    res = dict(shape=dict(D=D, H=H, L=L, T=T, batch_size=B), floor_us_per_step=FLOOR_US)
    for N in (64, 200):
        steps_per_epoch = -(-N // B)
        epochs = 1000 // steps_per_epoch
        th = torch.from_numpy(rs.uniform(-0.1, 0.1, size=(1, P)).astype(np.float32)).cuda()
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        t = torch.zeros(1, dtype=torch.int64, device="cuda")
        X = torch.from_numpy(rs.uniform(size=(1, N, T, D)).astype(np.float32)).cuda()
        y = torch.from_numpy((rs.uniform(size=(1, N, T)) < 0.3).astype(np.float32)).cuda()
        perm = ops.shuffle_perm(1, 1, epochs, N)
        fit = lambda: ops.lstm_fit(desc, th, m, v, t, X, y, epochs, B, perm, mask_value=-1.0)  # noqa: E731
        fit()
        ms = events(fit, 3)
        n_steps = epochs * steps_per_epoch
        res[f"fit_N{N}"] = dict(steps=n_steps, ms_per_fit=ms, us_per_step=1e3 * ms / n_steps,
                                x_floor=1e3 * ms / n_steps / FLOOR_US)
    Xg = torch.from_numpy(rs.uniform(size=(1, 1024, D))).cuda()
    vg = lambda: ops.lstm_value_and_input_grad(desc, th, Xg, T, "sigmoid", True)  # noqa: E731
    vg()
    res["value_and_input_grad_1024_ms"] = events(vg, 20)
    Xf = torch.from_numpy(rs.uniform(size=(1, 1024, D)).astype(np.float32)).cuda()
    fw = lambda: ops.lstm_forward(desc, th, Xf, num_steps=T)  # noqa: E731
    fw()
    res["forward_1024_ms"] = events(fw, 20)
    # one get_config of the plugin default on a 5-rung record (about 60 configurations)
    from bore_amd.plugins import SequenceClassifierConfigGenerator, UniformFloat
    from bore_amd.plugins.types import DenseSpace
    space = DenseSpace([UniformFloat(f"x{i}", 0.0, 1.0) for i in range(D)])
    cg = SequenceClassifierConfigGenerator(
        space, gamma=1 / 3, num_random_init=10, random_rate=None, retrain=False,
        classifier_kws=dict(mask_value=-1.0), fit_kws=dict(batch_size=64, num_steps_per_iter=1000),
        optimizer_kws=dict(num_starts=5), seed=0, logger=logging.getLogger("lstm_time"))
    budgets = 3.0 ** -np.arange(4, -1, -1)

    class Job:
        def __init__(self, cfg, b):
            self.kwargs, self.exception, self.id = dict(config=cfg, budget=b), None, 0
            self.result = dict(loss=float(np.sum((space.to_array(cfg) - 0.3) ** 2) + rs.normal(scale=1 - b)))

    for i in range(60):
        cfg = space.sample_configuration()
        for b in budgets[:1 + (i % 5 == 0) + (i % 9 == 0) + (i % 15 == 0) + (i % 30 == 0)]:
            cg.new_result(Job(cfg, b))
    cg.get_config(1.0)
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        cg.get_config(1.0)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - w0)
    res["get_config_wall_s"] = dict(median=float(np.median(walls)), all=walls, configs=cg.record.num_features(),
                                    rung_sizes=cg.record.rung_sizes())
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lstm", "lstm_time.json"))
