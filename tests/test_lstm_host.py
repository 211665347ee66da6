"""The multi-fidelity path without a GPU: MultiFidelityRecord against the reference's recorded vectors,
the fp64 LSTM oracle against finite differences, the C descriptor, and the generator's control flow."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- MultiFidelityRecord ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mf():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_mf_record.npz"))
    from bore_amd.data import MultiFidelityRecord
    rec = MultiFidelityRecord(gamma=1 / 3)
    for i, y, b in zip(g["seq_index"], g["seq_y"], g["seq_b"]):
        rec.append(g["xs"][i], float(y), float(b))
    return g, rec


def test_multi_fidelity_record_equals_the_reference(mf):
    g, rec = mf
    np.testing.assert_array_equal(rec.budgets(), g["budgets"])
    np.testing.assert_array_equal(rec.rung_sizes(), g["rung_sizes"])
    np.testing.assert_array_equal(rec.thresholds(), g["thresholds"])
    assert rec.num_features() == int(g["num_features"]) and rec.size() == int(g["size"])
    np.testing.assert_array_equal(rec.load_feature_matrix(), g["features"])
    for t in range(rec.num_rungs()):
        np.testing.assert_array_equal(rec.binary_labels(t), g[f"binary_labels_{t}"])
        np.testing.assert_array_equal(rec.targets(t), g[f"targets_{t}"])
    got = [-1 if rec.highest_rung(min_size=s) is None else rec.highest_rung(min_size=s) for s in range(14)]
    np.testing.assert_array_equal(got, g["highest_rung"])
    for name, pad in (("m1", -1.0), ("tiny", 1e-9)):
        for binary in (True, False):
            X, Y = rec.sequences(pad_value=pad, binary=binary)
            np.testing.assert_array_equal(X, g[f"seq_{name}_{int(binary)}_X"])
            np.testing.assert_array_equal(Y, g[f"seq_{name}_{int(binary)}_Y"])
    np.testing.assert_array_equal([rec.is_duplicate(p) for p in g["dup_probes"]], g["dup"])


def test_record_keeps_the_reference_quirks():
    from bore_amd.data import MultiFidelityRecord
    rec = MultiFidelityRecord(gamma=0.5)
    x = np.array([0.1, 0.2])
    rec.append(x, 1.0, 1.0)
    rec.append(x, 2.0, 1.0)               # same (x, b): value replaced, target appended again
    rec.append(np.array([0.3, 0.4]), 2.0, 1.0)
    assert rec.rung_sizes() == [3] and rec.num_features() == 2
    np.testing.assert_array_equal(rec.binary_labels(0), [True, True, True])   # <= at the (tied) quantile
    X, Y = rec.sequences(pad_value=-1.0, binary=False)
    assert Y[0, 0, 0] == 2.0


# -- the oracle --------------------------------------------------------------------------------------
def _masked_data(rs, n, T, D, mv):
    X = rs.uniform(size=(n, T, D))
    X[0, 0] = mv                      # leading
    X[1, T // 2] = mv                 # middle
    X[2, T - 1] = mv                  # trailing
    Y = (rs.uniform(size=(n, T)) < 0.5).astype(float)
    return X, Y


@pytest.mark.parametrize("act", ["elu", "tanh", "sigmoid"])
def test_oracle_gradients_match_central_differences(act):
    rs = np.random.RandomState(1)
    D, H, L, T, n, mv = 3, 4, 2, 5, 4, -1.0
    p = O.init_weights(D, H, L, rs)
    X, Y = _masked_data(rs, n, T, D, mv)
    l2 = [1e-2] * (L + 1)
    _, g = O.loss_and_grads(p, act, X, Y, mv, l2, l2)
    th, gf, e = O.pack(p), O.pack(g), 1e-6
    f = lambda v: O.loss_and_grads(O.unpack(v, D, H, L), act, X, Y, mv, l2, l2)[0]  # noqa: E731
    for i in rs.choice(th.size, 40, replace=False):
        a, b = th.copy(), th.copy()
        a[i] += e
        b[i] -= e
        fd = (f(a) - f(b)) / (2 * e)
        assert abs(fd - gf[i]) < 1e-8 + 1e-5 * abs(fd), (i, fd, gf[i])
    x = rs.uniform(size=(3, D))
    for tr in ("identity", "sigmoid", "exp"):
        _, gx = O.value_and_input_grad(p, act, x, 3, tr, True)
        for k in range(D):
            a, b = x.copy(), x.copy()
            a[:, k] += e
            b[:, k] -= e
            fd = (O.value_and_input_grad(p, act, a, 3, tr, True)[0] - O.value_and_input_grad(p, act, b, 3, tr, True)[0]) / (2 * e)
            np.testing.assert_allclose(fd, gx[:, k], atol=1e-8, rtol=1e-5)


def test_oracle_masked_steps_keep_the_state_and_the_forms_agree():
    rs = np.random.RandomState(2)
    D, H, L, T = 2, 5, 2, 4
    p = O.init_weights(D, H, L, rs)
    X = rs.uniform(size=(3, T, D))
    X[:, 2] = -1.0
    logits, (C, live) = O.forward(p, "elu", X, -1.0, cache=True)
    assert not live[:, 2].any()
    for l in range(L):
        np.testing.assert_array_equal(C[l][2]["h"], C[l][1]["h"])
    np.testing.assert_array_equal(logits[:, 2], logits[:, 1])    # the output of a masked step: the previous one
    x = rs.uniform(size=(6, D))
    np.testing.assert_array_equal(O.forward(p, "elu", np.repeat(x[:, None], T, 1), 1e9)[:, -1],
                                  O.one_to_one(p, "elu", x, T))


# -- the C descriptor ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    from bore_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_native()
    return _lib.lib()


def test_param_count_and_bad_descriptors(built):
    from bore_amd import _lib, ops
    assert ops.lstm_param_count(_lib.make_lstm_desc(2, 2, 32, "elu")) == 12833
    assert ops.lstm_param_count(_lib.make_lstm_desc(16, 2, 32, "elu")) == 14625
    d = _lib.make_lstm_desc(0, 2, 32, "elu")
    with pytest.raises(RuntimeError, match="input_dim"):
        ops.lstm_param_count(d)
    with pytest.raises(_lib.UnsupportedError, match="BORE_LSTM_MAX_LAYERS"):
        _lib.make_lstm_desc(2, 5, 32, "elu")
    with pytest.raises(ValueError, match="activation"):
        _lib.make_lstm_desc(2, 1, 8, "softplus")
    from bore_amd.models import StackedRecurrentFactory
    f = StackedRecurrentFactory(16, 1, layer_kws=dict(activation="elu"))
    assert f.count_params() == 14625


def test_reachable_lstm_bounds_are_the_lds_budget(built):
    """The layout is decided before any pointer is looked at and before any HIP call, so bore_lstm_forward with null
    data pointers reports that verdict alone: BORE_E_UNSUPPORTED with the LDS message for a network that does not fit
    one workgroup's 160 KB, BORE_E_INVALID ("null pointer") for one that does."""
    from bore_amd import _lib

    def verdict(D, L, H, T):
        d = _lib.make_lstm_desc(D, L, H, "elu")
        rc = built.bore_lstm_forward(ctypes.byref(d), 1, None, None, 1, T, 0, 0.0, None, None)
        return rc, built.bore_last_error().decode()

    def fits(D, L, H, T):
        rc, msg = verdict(D, L, H, T)
        assert (rc == -1 and "null pointer" in msg) or (rc == -2 and "LDS" in msg), (rc, msg)
        return rc == -1

    # BORE_LSTM_MAX_UNITS is 64, but no network of 59 or more units fits: not at the smallest shape, hence at none
    for H in range(59, 65):
        rc, msg = verdict(1, 1, H, 1)
        assert rc == -2 and "LDS" in msg and "%d units" % H in msg, (H, rc, msg)
    assert fits(1, 1, 58, 1)
    # one layer: 57 units at 2 inputs and one step, 54 at 16 steps
    assert fits(2, 1, 57, 1) and not fits(2, 1, 58, 1)
    assert fits(2, 1, 54, 16) and not fits(2, 1, 55, 16)
    assert fits(2, 1, 56, 1) and "187408 B of LDS" in verdict(2, 1, 64, 1)[1]
    # the plugin default, 2 x 32 units, at every D <= 16 and T <= 16 (151376 B of 163840 at 16 inputs and 16 steps)
    for D in (1, 2, 16):
        for T in (1, 5, 16):
            assert fits(D, 2, 32, T), (D, T)
    # a third layer of 32 units does not fit any more
    rc, msg = verdict(2, 3, 32, 5)
    assert rc == -2 and "182032 B of LDS" in msg, (rc, msg)


def test_lstm_descriptor_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from bore_amd import _lib
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bore_hip.h"\nint main(void){printf("%zu %zu %zu '
                   '%zu %zu", sizeof(bore_lstm_desc), offsetof(bore_lstm_desc, act), offsetof(bore_lstm_desc, '
                   'l2_kernel), offsetof(bore_lstm_desc, l2_bias), offsetof(bore_lstm_desc, output_dim));return 0;}\n')
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.LstmDesc
    assert got == [ctypes.sizeof(S), S.act.offset, S.l2_kernel.offset, S.l2_bias.offset, S.output_dim.offset]


def test_factory_keeps_the_reference_asserts():
    from bore_amd.models import StackedRecurrentFactory
    with pytest.raises(AssertionError):
        StackedRecurrentFactory(2, 1, layer_kws=dict(return_sequences=True))
    with pytest.raises(AssertionError):
        StackedRecurrentFactory(2, 1, final_layer_kws=dict(activation="sigmoid"))


# -- the generator with a stub network -----------------------------------------------------------------
class _StubNet:
    def __init__(self):
        self.fits = []

    def compile(self, **kw):
        pass

    def summary(self, print_fn=print):
        pass

    def fit(self, x, y, epochs, batch_size, callbacks, verbose):
        self.fits.append((x.shape, epochs, batch_size))

    def evaluate(self, x, y, verbose=False):
        return [0.5, 0.5]


class _StubOneToOne:
    def __init__(self, steps):
        self.steps = steps

    def argmax(self, bounds, filter_fn, random_state, **kw):
        from scipy.optimize import OptimizeResult
        return OptimizeResult(x=random_state.uniform(bounds.lb, bounds.ub), fun=-0.5)


class _StubFactory:
    def __init__(self, **kw):
        self.built = []
        self.net = _StubNet()

    def build_many_to_many(self, mask_value):
        self.mask_value = mask_value
        return self.net

    def build_one_to_one(self, num_steps, transform=None):
        self.built.append(num_steps)
        return _StubOneToOne(num_steps)


def _generator(monkeypatch, **kw):
    import bore_amd.models
    from bore_amd.plugins import SequenceClassifierConfigGenerator, UniformFloat
    from bore_amd.plugins.types import DenseSpace
    monkeypatch.setattr(bore_amd.models, "StackedRecurrentFactory", _StubFactory)
    space = DenseSpace([UniformFloat("a", 0.0, 1.0), UniformFloat("b", -1.0, 1.0)])
    args = dict(gamma=1 / 3, num_random_init=4, random_rate=None, retrain=False,
                classifier_kws=dict(mask_value=-1.0), fit_kws=dict(batch_size=2, num_steps_per_iter=10),
                optimizer_kws=dict(num_starts=3), seed=0)
    args.update(kw)
    return SequenceClassifierConfigGenerator(space, **args)


class _Job:
    def __init__(self, cfg, b, loss):
        self.kwargs, self.result, self.exception, self.id = dict(config=cfg, budget=b), dict(loss=loss), None, 0


def test_generator_is_random_until_a_rung_fills_then_fits_with_the_epochs_rule(monkeypatch):
    cg = _generator(monkeypatch)
    net = cg.model_factory.net
    rs = np.random.RandomState(0)
    for i in range(4):
        cfg, _ = cg.get_config(1 / 9)
        assert not net.fits
        cg.new_result(_Job(cfg, 1 / 9, float(rs.uniform())))
    cfg, _ = cg.get_config(1 / 9)
    assert len(net.fits) == 1 and cg.model_factory.built == [1]
    shape, epochs, bs = net.fits[0]
    assert shape == (4, 1, 2) and bs == 2 and epochs == 10 // 2      # num_steps_per_iter // ceil(4 / 2)
    for i in range(4):                                               # fill rung 1
        cfg, _ = cg.get_config(1 / 3)
        cg.new_result(_Job(cfg, 1 / 3, float(rs.uniform())))
    cg.get_config(1 / 3)
    cg.get_config(1 / 3)
    assert cg.model_factory.built == [1, 2] and sorted(cg.funcs) == [0, 1]   # one cached net per rung
    assert cg.model_factory.mask_value == -1.0


def test_generator_defaults_and_refusals(monkeypatch):
    with pytest.raises(NotImplementedError):
        _generator(monkeypatch, retrain=True)
    cg = _generator(monkeypatch, classifier_kws={})
    assert cg.mask_value == 1e-9 and cg.num_epochs is None


def test_bore_hyperband_builds_the_ladder(monkeypatch):
    import bore_amd.models
    from bore_amd.plugins import BOREHyperband, UniformFloat
    from bore_amd.plugins.types import DenseSpace
    monkeypatch.setattr(bore_amd.models, "StackedRecurrentFactory", _StubFactory)
    hb = BOREHyperband(DenseSpace([UniformFloat("a", 0.0, 1.0)]), eta=3, min_budget=1 / 81, max_budget=1, seed=1)
    assert hb.max_SH_iter == 5
    np.testing.assert_allclose(hb.budgets, [1 / 81, 1 / 27, 1 / 9, 1 / 3, 1])
    cg = hb.config_generator
    assert cg.mask_value == -1.0 and cg.num_starts == 5 and cg.num_steps_per_iter == 1000 and cg.num_epochs is None
    assert abs(cg.gamma - 1 / 3) < 1e-12 and hb.config["max_SH_iter"] == 5
