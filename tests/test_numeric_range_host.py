"""CPU side of tests/test_gpu_numeric_range.py: the probe networks place their table values exactly, the float32 oracle
keeps within half of every tolerance the device test applies (so a device failure is the kernel's, not the
reference's), deliberately wrong formulas leave those tolerances, and the flat-start restart of the host build agrees
with SciPy."""
import json
import os

import numpy as np
import pytest
from scipy.optimize import Bounds, minimize

import lbfgsb_host as H
import numeric_range as NR
from oracle import bore_oracle as O

F32 = np.float32


def _margins():
    with open(NR.MARGIN_JSON) as f:
        return json.load(f)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_probe_networks_place_every_table_value_exactly(dtype):
    """In float64 and in float32 the pre-activation of every probed unit EQUALS the table value, for every flavour's
    network: selector kernels leave one nonzero term per sum."""
    for name, (D, units, out, allowed, _) in NR.FIT_FLAVOURS.items():
        n = len(units)
        for launch in NR.sweep_models(name, "logit"):
            for mdl in launch["models"]:
                pre = NR.preactivations(mdl["p"], launch["acts"], mdl["row"], dtype)
                assert pre[-1].shape == (1,) and float(pre[-1][0]) == mdl["value"], (name, mdl["label"])
        for launch in NR.sweep_models(name, "hidden"):
            for i, mdl in enumerate(launch["models"]):
                l = int(mdl["label"].split()[1])
                pre = NR.preactivations(mdl["p"], launch["acts"], mdl["row"], dtype)[l - 1]
                values = [float(F32(b)) for b in mdl["p"][2 * (l - 1) + 1]]
                assert [float(x) for x in pre] == values and mdl["value"] in values, (name, mdl["label"])
                # the chain's unit holds this model's value and is the one the output kernel reads
                c = int(np.flatnonzero(mdl["p"][-2][:, 0])[0])
                assert float(pre[c]) == mdl["value"], (name, mdl["label"])
        for launch in NR.sweep_models(name, "adam"):
            for mdl in launch["models"][:8]:
                hs = O.forward([a.astype(dtype) for a in mdl["p"]], launch["acts"], mdl["row"][None].astype(dtype),
                               return_all=True, logits=True)
                assert float(hs[-1][0, 0]) == 0.0                     # logit 0: d loss / d logit = +-0.5
                front = [float(x) for x in hs[-2][0] if x != 0]          # the activations in front of the output kernel
                assert set(front) <= {float(F32(2 * g)) for g in NR.ADAM_G}, (name, mdl["label"])
    # every table value is a float32
    for x in NR.LOGITS + NR.HIDDEN + NR.RELU_KINK + NR.VG_U:
        assert float(F32(x)) == x
    assert len(NR.LOGITS) == 33 and len(NR.HIDDEN) == 22


def test_the_adam_probe_delivers_its_gradients():
    """The output kernel's float64 gradients of the Adam probe are +-g (g = half of a float32 input: exact), for a
    one-layer and a deep network."""
    for D, units in ((17, [1]), (3, [16, 16, 16, 16, 1])):
        n = len(units)
        for sign in (1, -1):
            p, row = NR.adam_model(D, units, NR.ADAM_G, sign)
            G = NR.grad_tolerances(p, NR._acts(n, "relu", "linear"), row, float(sign < 0))
            want = [sign * 0.5 * float(F32(2 * g)) for g in NR.ADAM_G]
            assert [float(x) for x in G["g"][-2][:len(want), 0]] == want


def test_committed_margins_are_current_and_within_one_half():
    M = _margins()
    assert M["dropped"] == []                                  # nothing dropped: both sides of every seam are kept
    for key in ("fit_logit", "fit_hidden", "fit_adam", "fit_bf16", "forward", "evaluate", "value_grad"):
        assert M[key] and max(M[key].values()) <= 0.5, (key, max(M[key].values()))
    assert max(M["value_grad exp"].values()) <= 1.0            # (numpy's float32 exp is itself a one-ulp function)
    assert max(M["adam_f32_ratio"].values()) <= 0.5            # so the Adam bound is the operation count
    assert set(M["fit_logit"]) == set(NR.FIT_FLAVOURS) and set(M["forward"]) == set(NR.ACQ_FLAVOURS) | {"static 1 2-16-16-1"}
    # recomputed here for three networks (the tool recomputes them all): the file is this tree's
    for name in ("static 1 2-16-16-1", "generic -2 5-1-1"):
        for sweep in ("logit", "hidden"):
            assert NR._worst(NR.oracle_fit_ratios(name, sweep)) == pytest.approx(M["fit_" + sweep][name], rel=0.05)
    assert NR._worst(NR.oracle_fit_ratios("generic -1 17-1", "adam")) == pytest.approx(M["fit_adam"]["generic -1 17-1"], rel=0.05)
    now = NR.measure_adam_f32_ratio()         # (to 5 %: another numpy may round a float32 exp or log1p the other way)
    assert set(now) == set(M["adam_f32_ratio"]) and all(now[k] == pytest.approx(M["adam_f32_ratio"][k], rel=0.05, abs=0.01) for k in now)


def test_wrong_formulas_leave_the_tolerances():
    """On the oracle's side, through the same comparisons.  Three of the five leave their tolerance by five orders of
    magnitude.  Two cannot, whatever the kernel does, and are recorded as measured:
    - the elu series one float past the seam: 0.05 of the bound (0.23 for fit_elu as written).  Its truncation there is
      x^5 / 120 = 2^-26 |x|, a twentieth of the header's bound -- the seam could sit anywhere near -1/32.
    - beta^t as a float32 running product, read on the output kernel alone (theta = 0) at t0 = 999: 0.087 of the bound,
      the SAME figure as without the swap.  After a thousand float32 products beta2^t is 0.36770025 against the rounded
      double power's 0.36770016; through 1 - beta2^t and the square root that moves alpha by less than one float32
      ulp, and here by none.  The swap is not a defect a float32 comparison can see."""
    S = NR.sensitivity()
    recorded = _margins()["sensitivity"]
    assert set(S) == set(recorded) and all(S[k] == pytest.approx(recorded[k], rel=0.05) for k in S)
    for k in ("expm1 as exp(x) - 1 near 0", "exp flushed at 2^-100", "eps inside the square root"):
        assert S[k] >= 10, (k, S[k])
    assert S["fit_elu as written, at the seam"] <= 0.5
    assert S["elu series one float past the seam"] <= 0.5
    assert S["beta^t as a float32 running product"] == S["output kernel at t0 = 999, no swap"] <= 0.5


def test_flat_start_host_build_against_scipy():
    """sigmoid transform at u >= 39: T = 1 and dT = 0 exactly in float32, so the projected gradient is 0 at the start:
    SciPy and the host build of lbfgsb.h both stop with nit = 0, nfev = 1, status 0, x = x0."""
    for name in ("static 2 6-32-32-1", "generic -3 5-7-3-1"):
        D, units, _ = NR.ACQ_FLAVOURS[name]
        p, acts = NR.flat_model(D, units)
        fg = lambda x: O.value_and_input_grad(p, acts, x, "sigmoid")
        lo, hi = np.zeros(D), np.ones(D)
        for x0 in np.random.RandomState(8).uniform(0, 1, size=(3, D)):
            v, g = fg(x0)
            assert v == 1.0 and not g.any()
            a = minimize(fg, x0, jac=True, method="L-BFGS-B", bounds=Bounds(lo, hi), options=dict(maxiter=5))
            b = H.minimize(fg, x0, (lo, hi), maxiter=5)
            assert (a.nit, a.nfev, a.status) == (b.nit, b.nfev, b.status) == (0, 1, 0)
            np.testing.assert_array_equal(a.x, x0)
            np.testing.assert_array_equal(b.x, x0)
            assert b.fun == 1.0 and not b.jac.any() and b.task[0] == 4          # CONVERGENCE: projected gradient


def test_saturated_constant_models_are_exactly_constant():
    for b_out, const in ((100.0, 1.0), (-10000.0, 0.0)):
        p, acts = NR.constant_model(6, [32, 32, 1], b_out)
        X = np.random.RandomState(3).uniform(0, 1, size=(300, 6))
        assert (O.predict(p, acts, X) == const).all()
