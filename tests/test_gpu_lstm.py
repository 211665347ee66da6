"""The multi-fidelity classifier (bore_lstm_*) on the GPU against the fp64 oracle tests/lstm_oracle.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

# tolerances of the Dense fit against its oracle (tests/test_gpu_parity.py, edge shapes)
FIT_TOL = dict(theta=dict(rtol=2e-4, atol=1e-5), m=dict(rtol=1e-3, atol=1e-7), v=dict(rtol=1e-3, atol=1e-10),
               loss=dict(rtol=5e-5))


def _desc(D, H, L, act, l2=0.0):
    from bore_amd import _lib
    return _lib.make_lstm_desc(D, L, H, act, [l2] * (L + 1), [l2] * (L + 1))


def _hyperband_sequences(rs, N, T, D, mask_value):
    """Sequences as MultiFidelityRecord.sequences lays them out: leading gaps (sampled in a higher bracket),
    trailing gaps (not promoted), a few complete ones."""
    X = np.repeat(rs.uniform(size=(N, 1, D)), T, axis=1)
    Y = (rs.uniform(size=(N, T)) < 0.4).astype(np.float64)
    for n in range(N):
        lo = rs.randint(0, T) if n % 3 == 1 else 0
        hi = rs.randint(lo + 1, T + 1) if n % 3 == 2 else T
        X[n, :lo] = mask_value
        X[n, hi:] = mask_value
        Y[n, :lo] = mask_value
        Y[n, hi:] = mask_value
    return X, Y


def _theta(params):
    import torch
    return torch.from_numpy(O.pack(params).astype(np.float32)).cuda().reshape(1, -1)


@pytest.mark.parametrize("D,H,L,act", [(2, 32, 2, "elu"), (16, 32, 2, "tanh"), (5, 8, 1, "relu"),
                                       (3, 16, 3, "sigmoid"), (4, 32, 1, "linear")])
def test_forward_both_forms_and_input_grad_match_the_oracle(gpu, D, H, L, act):
    import torch
    from bore_amd import ops
    rs = np.random.RandomState(D + H + L)
    p = O.init_weights(D, H, L, rs)
    p32 = [q.astype(np.float32).astype(np.float64) for q in p]
    desc, th = _desc(D, H, L, act), _theta(p)
    T, mv = 5, -1.0
    X, _ = _hyperband_sequences(rs, 70, T, D, mv)
    out = ops.lstm_forward(desc, th, torch.from_numpy(X.astype(np.float32)).cuda()[None], mask_value=mv)
    ref = O.forward(p32, act, X.astype(np.float32), mv)
    np.testing.assert_allclose(out[0].cpu().numpy(), ref, rtol=2e-5, atol=2e-5)   # fp32 vs fp64, 5 chained steps
    # one-to-one == many-to-many at the last step on tiled input, bit for bit (reference test_models.py:53-111)
    x = rs.uniform(size=(130, D)).astype(np.float32)
    o2o = ops.lstm_forward(desc, th, torch.from_numpy(x).cuda()[None], num_steps=T)[0].cpu().numpy()
    m2m = ops.lstm_forward(desc, th, torch.from_numpy(np.repeat(x[:, None], T, 1)).cuda()[None],
                           mask_value=1e9)[0].cpu().numpy()
    np.testing.assert_array_equal(o2o, m2m[:, T - 1])
    np.testing.assert_allclose(o2o, O.one_to_one(p32, act, x, T), rtol=2e-5, atol=2e-5)
    for transform in ("identity", "sigmoid", "exp"):
        for negate in (True, False):
            xd = rs.uniform(size=(7, D))
            val, grad = ops.lstm_value_and_input_grad(desc, th, torch.from_numpy(xd).cuda()[None], 3, transform,
                                                      negate)
            rv, rg = O.value_and_input_grad(p32, act, xd.astype(np.float32), 3, transform, negate)
            np.testing.assert_allclose(val[0].cpu().numpy(), rv, rtol=2e-5, atol=2e-6)
            np.testing.assert_allclose(grad[0].cpu().numpy(), rg, rtol=2e-4, atol=2e-5)
            # the value is the one-to-one prediction of the same (fp32-rounded) point, bit for bit
            if transform == "identity" and not negate:
                pr = ops.lstm_forward(desc, th, torch.from_numpy(xd.astype(np.float32)).cuda()[None], num_steps=3)
                np.testing.assert_array_equal(val[0].cpu().numpy(), pr[0].cpu().numpy())


@pytest.mark.parametrize("N,T,act,l2", [(1, 1, "elu", 0.0), (10, 3, "tanh", 1e-3), (64, 5, "elu", 0.0),
                                        (65, 5, "tanh", 1e-3), (200, 3, "elu", 1e-3), (200, 5, "tanh", 0.0),
                                        (10, 1, "elu", 0.0), (65, 3, "elu", 0.0)])
def test_fit_trajectory_matches_the_oracle(gpu, N, T, act, l2):
    import torch
    from bore_amd import ops
    D, H, L, B, E, mv = 2, 32, 2, 64, 3, -1.0
    rs = np.random.RandomState(N * 7 + T)
    p = [q.astype(np.float32).astype(np.float64) for q in O.init_weights(D, H, L, rs)]
    X, Y = _hyperband_sequences(rs, N, T, D, mv)
    perms = np.stack([rs.permutation(N) for _ in range(E)]).astype(np.int32)
    desc, th = _desc(D, H, L, act, l2), _theta(p)
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    t = torch.zeros(1, dtype=torch.int64, device=th.device)
    hist = ops.lstm_fit(desc, th, m, v, t, torch.from_numpy(X.astype(np.float32)).cuda()[None],
                        torch.from_numpy(Y.astype(np.float32)).cuda()[None], E, B,
                        torch.from_numpy(perms).cuda()[None], mask_value=mv)
    st = O.AdamState(p)
    ref = O.fit(p, act, st, X.astype(np.float32), Y, perms, B, mv, [l2] * (L + 1), [l2] * (L + 1))
    np.testing.assert_allclose(hist[0].cpu().numpy(), ref, **FIT_TOL["loss"])
    np.testing.assert_allclose(th[0].cpu().numpy(), O.pack(p), **FIT_TOL["theta"])
    np.testing.assert_allclose(m[0].cpu().numpy(), O.pack(st.m), **FIT_TOL["m"])
    np.testing.assert_allclose(v[0].cpu().numpy(), O.pack(st.v), **FIT_TOL["v"])
    assert int(t[0]) == E * -(-N // B)


def test_warm_start_and_reproducibility(gpu):
    import torch
    from bore_amd import ops
    D, H, L, N, T, B, E, mv = 16, 32, 2, 70, 5, 64, 4, -1.0
    rs = np.random.RandomState(3)
    p = O.init_weights(D, H, L, rs)
    X, Y = _hyperband_sequences(rs, N, T, D, mv)
    perms = np.stack([rs.permutation(N) for _ in range(2 * E)]).astype(np.int32)
    desc = _desc(D, H, L, "elu")
    Xd = torch.from_numpy(X.astype(np.float32)).cuda()[None]
    Yd = torch.from_numpy(Y.astype(np.float32)).cuda()[None]

    def run(splits):
        th = _theta(p)
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        t = torch.zeros(1, dtype=torch.int64, device=th.device)
        e0, losses = 0, []
        for e in splits:
            losses.append(ops.lstm_fit(desc, th, m, v, t, Xd, Yd, e, B,
                                       torch.from_numpy(perms[e0:e0 + e]).cuda()[None], mask_value=mv))
            e0 += e
        return th.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), int(t[0]), torch.cat(losses, 1).cpu().numpy()

    a, b, c = run([2 * E]), run([E, E]), run([2 * E])
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a, c):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a[4], b[4])
    assert a[3] == b[3] == 2 * E * -(-N // B)


def test_evaluate_matches_the_oracle_with_masks(gpu):
    import torch
    from bore_amd import ops
    for D, H, L, act, l2 in ((2, 32, 2, "elu", 0.0), (7, 16, 1, "tanh", 1e-2)):
        rs = np.random.RandomState(D)
        p = [q.astype(np.float32).astype(np.float64) for q in O.init_weights(D, H, L, rs)]
        X, Y = _hyperband_sequences(rs, 150, 4, D, -1.0)
        Y = np.where(Y == -1.0, -1.0, (rs.uniform(size=Y.shape) < 0.5).astype(float))
        loss, acc = ops.lstm_evaluate(_desc(D, H, L, act, l2), _theta(p),
                                      torch.from_numpy(X.astype(np.float32)).cuda()[None],
                                      torch.from_numpy(Y.astype(np.float32)).cuda()[None], mask_value=-1.0)
        rl, ra = O.evaluate(p, act, X.astype(np.float32), Y, -1.0, [l2] * (L + 1), [l2] * (L + 1))
        np.testing.assert_allclose(float(loss[0]), rl, rtol=2e-5)
        np.testing.assert_allclose(float(acc[0]), ra, atol=1e-6)


@pytest.mark.parametrize("seed", [0, 42, 8888])
def test_stacked_recurrent_factory(gpu, seed):
    """The reference's tests/test_models.py:53-111, ported."""
    from scipy.optimize import Bounds
    from bore_amd.layers import BinaryCrossentropy
    from bore_amd.models import StackedRecurrentFactory
    rs = np.random.RandomState(seed)
    num_steps, input_dim, n = 5, 2, 64
    factory = StackedRecurrentFactory(input_dim=input_dim, output_dim=1, num_layers=2, num_units=32,
                                      layer_kws=dict(activation="elu"), seed=seed)
    net1 = factory.build_many_to_many()
    net1.compile(optimizer="adam", loss=BinaryCrossentropy(from_logits=True))
    X = rs.uniform(size=(n, num_steps, input_dim))
    Z = rs.randint(2, size=(n, num_steps, 1))
    net1.fit(X, Z, epochs=10, batch_size=16)
    net2 = factory.build_one_to_one(num_steps)
    for a, b in zip(net1.get_weights(), net2.get_weights()):
        np.testing.assert_array_equal(a, b)
    X_test = rs.uniform(size=(32, input_dim))
    X_test_tiled = np.tile(np.expand_dims(X_test, axis=1), reps=(1, num_steps, 1))
    np.testing.assert_array_equal(net1.predict(X_test_tiled)[:, -1], net2.predict(X_test))
    res = net2.argmax(Bounds(lb=np.zeros(input_dim), ub=np.ones(input_dim)), num_starts=3, num_samples=256,
                      print_fn=lambda s: None, random_state=rs)
    assert res is not None
    assert np.all(net2.predict(res.x[None]) >= net2.predict(X_test))


def test_generator_end_to_end_against_an_oracle_driven_fit(gpu):
    import logging
    from bore_amd import shuffle as S
    from bore_amd.plugins import SequenceClassifierConfigGenerator, UniformFloat
    from bore_amd.plugins.types import DenseSpace
    space = DenseSpace([UniformFloat("x0", -5.0, 10.0), UniformFloat("x1", 0.0, 15.0)])
    budgets = 1.0 * 3.0 ** -np.linspace(4, 0, 5)
    cg = SequenceClassifierConfigGenerator(
        space, gamma=1 / 3, num_random_init=6, random_rate=0.1, retrain=False,
        classifier_kws=dict(num_layers=2, num_units=32, activation="elu", mask_value=-1.0),
        fit_kws=dict(batch_size=64, num_steps_per_iter=100),
        optimizer_kws=dict(transform="sigmoid", num_starts=5, num_samples=256), seed=7,
        logger=logging.getLogger("test_lstm"))
    noise = np.random.RandomState(11)

    class Job:
        def __init__(self, cfg, b):
            x0, x1 = cfg["x0"], cfg["x1"]
            f = (x1 - 5.1 / (4 * np.pi ** 2) * x0 ** 2 + 5 / np.pi * x0 - 6) ** 2 + 10 * (1 - 1 / (8 * np.pi)) * \
                np.cos(x0) + 10
            self.kwargs = dict(config=cfg, budget=b)
            self.result = dict(loss=float(f + noise.normal(scale=5.0 * (1 - b))))
            self.exception, self.id = None, 0

    seen, checked = [], False
    for it in range(30):
        rung = [0, 0, 0, 1, 1, 2, 3, 4][it % 8]
        net = cg.logit
        before = None
        if cg.record.highest_rung(min_size=6) is not None and not checked and net.adam_m is not None:
            before = (net.get_weights(), net.get_optimizer_state(), net._epochs_seen)
            inputs, targets = cg.record.sequences(binary=True, pad_value=-1.0)
        cfg, _ = cg.get_config(budgets[rung])
        x = space.to_array(cfg)
        assert np.all(x >= 0) and np.all(x <= 1)
        assert not any(np.allclose(x, s) for s in seen)
        seen.append(x)
        if before is not None and len(net.get_optimizer_state()) == 3 and net._epochs_seen > before[2]:
            E = net._epochs_seen - before[2]
            N = inputs.shape[0]
            perms = S.permutations(cg.model_factory._shuffle_seed, 1, E, N, epoch0=before[2])[0]
            p = [w.astype(np.float64) for w in before[0]]
            st = O.AdamState(p)
            m0, v0, t0 = before[1]
            st.m = O.unpack(m0, 2, 32, 2)
            st.v = O.unpack(v0, 2, 32, 2)
            st.t = t0
            O.fit(p, "elu", st, inputs.astype(np.float32), targets[..., 0], perms, 64, -1.0)
            # ~100 chained fp32 Adam steps (the Dense long-fit test allows 2e-3 after 400)
            np.testing.assert_allclose(O.pack(net.get_weights()), O.pack(p), rtol=2e-3, atol=2e-4)
            checked = True
        for b in budgets[:rung + 1]:
            cg.new_result(Job(cfg, b))
    assert checked
    assert set(cg.funcs) <= set(range(5)) and cg.funcs


def test_unsupported_shapes_name_their_bound(gpu):
    import torch
    from bore_amd import _lib, ops
    from bore_amd._lib import UnsupportedError
    th = torch.zeros(1, ops.lstm_param_count(_desc(2, 128, 1, "elu")), device="cuda")
    with pytest.raises(UnsupportedError, match="BORE_LSTM_MAX_UNITS"):
        ops.lstm_forward(_desc(2, 128, 1, "elu"), th, torch.zeros(1, 3, 2, device="cuda"), num_steps=2)
    d = _desc(2, 32, 2, "elu")
    th = torch.zeros(1, ops.lstm_param_count(d), device="cuda")
    with pytest.raises(UnsupportedError, match="BORE_LSTM_MAX_STEPS"):
        ops.lstm_forward(d, th, torch.zeros(1, 3, 17, 2, device="cuda"))
    m, v, t = torch.zeros_like(th), torch.zeros_like(th), torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(UnsupportedError, match="64"):
        ops.lstm_fit(d, th, m, v, t, torch.zeros(1, 80, 3, 2, device="cuda"), torch.zeros(1, 80, 3, device="cuda"),
                     1, 80, torch.arange(80, dtype=torch.int32, device="cuda").reshape(1, 1, 80))
    with pytest.raises(UnsupportedError, match="LDS"):
        d = _desc(64, 64, 2, "elu")
        ops.lstm_forward(d, torch.zeros(1, ops.lstm_param_count(d), device="cuda"),
                         torch.zeros(1, 3, 64, device="cuda"), num_steps=2)
    assert _lib.lib().bore_abi_version() == 12
