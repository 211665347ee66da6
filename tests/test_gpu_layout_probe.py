"""Exact integer-network probes for the bfloat16 and wide-shape kernels: fit_bf16_mfma.h, arg_bf16_mfma.h, the TileOrder
round trip of theta, m and v in a wide fit, and the float32 wide fits that share it (32->128-128-1 "in rounds").

The networks of tests/layout_probe.py have small integer weights, biases and inputs: every product is an integer, every
partial sum stays below 2^24, so every order of summation gives the same float32 value and its bfloat16 rounding is
deterministic.  The device must then EQUAL the oracle: a bit that differs is a misplaced element (fragment or tile
mapping, a row block dropped or counted twice, an Adam slot in the wrong place, a model offset) or a wrong rounding mode,
not noise.  tests/test_layout_probe_host.py checks the premises on the CPU and prints which mutation of the parameters
each probe sees.

Sections (both shapes, compute bfloat16 and float32, three models with their own networks and data per launch):
  A  mlp_forward              rows {1, 15, 16, 17, 63, 64, 65, 133}, per-model and shared X            exact
  B  mlp_value_and_input_grad identity transform, both signs, the same row counts                      exact
  C  screen_topk              predictions, picks (ties to the lower row, against the oracle) and x0     exact
  F1 zero-gradient decay      unique Adam slots through 1 and 3 epochs, one and two launches: m, v, t   exact, theta bound
  F2 one live batch           the gradient of one batch read back from m and v                          exact, theta bound,
                                                                                                        loss one rounding
  E  mlp_evaluate             float32: loss one rounding, accuracy exact
Everything is np.array_equal but two comparisons, both derived (layout_probe.adam_trajectory, layout_probe.mean_of):
theta after Adam steps -- fit_rcp, fit_sqrt and the final fmaf round -- and a division by N.  Their worst error / bound is
recorded beside the comparisons that are exact (profiles/layout_probe/parity_measured.json).  What stays with the tolerance tests of test_gpu_parity.py:
random-weight behaviour, and batches whose size is no power of two (1 / rows is then inexact and the sums depend on
their order)."""
import functools

import numpy as np
import pytest
import torch

import layout_probe as LP
from bore_amd import _lib, ops
from conftest import record_measurement
from layout_probe import EPS, F32, pack
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

CASES = [(name, compute) for name in LP.SHAPES for compute in LP.COMPUTES]
CASE_IDS = ["%s %s" % c for c in CASES]
VARIANT_IDS = ["relu", "linear"]
B = LP.BATCH
_rows = LP.rows_of
_measured = {}


def _record(test, case, value):
    _measured.setdefault(test, {})[case] = value
    record_measurement("layout_probe/" + test, _measured[test])


def _desc(name, compute, linear=False):
    D, units, _ = LP.SHAPES[name]
    return _lib.make_desc(D, units, LP.networks(name, linear)[0][0]["acts"], compute=compute)


def _theta(name, linear=False):
    return np.stack([pack(net["p"]) for net, _ in LP.networks(name, linear)])


# ---- references, once per module -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_rows(name, compute, linear):
    """Per model i and data set j (j = i: its own rows; j = 0: the shared rows): output, and value / gradient for
    both signs, of all canonical rows.  Rows are independent, so a launch of n rows is compared with the first n."""
    nets = LP.networks(name, linear)
    out = {}
    for i, (net, _) in enumerate(nets):
        for j in {i, 0}:
            X = nets[j][1]
            out[i, j] = dict(out=LP.ref_forward(net, X, compute),
                             vg={neg: LP.ref_value_grad(net, X, compute, neg) for neg in (True, False)})
    return out


@pytest.mark.parametrize("linear", LP.VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("name,compute", CASES, ids=CASE_IDS)
def test_forward_equals_the_oracle(gpu, name, compute, linear):
    """A: mlp_forward, per-model X and one X shared by the three models."""
    nets, ref = LP.networks(name, linear), _ref_rows(name, compute, linear)
    desc, th = _desc(name, compute, linear), dev(_theta(name, linear))
    for n in LP.ROWS:
        own = ops.mlp_forward(desc, th, dev(np.stack([X[:n] for _, X in nets]).astype(F32))).cpu().numpy()
        shared = ops.mlp_forward(desc, th, dev(nets[0][1][:n].astype(F32))).cpu().numpy()
        for i in range(LP.N_MODELS):
            assert np.array_equal(own[i], ref[i, i]["out"][:n]), (n, i, "per-model X")
            assert np.array_equal(shared[i], ref[i, 0]["out"][:n]), (n, i, "shared X")
    _record("forward", "%s %s %s" % (name, compute, VARIANT_IDS[linear]), "exact")


@pytest.mark.parametrize("linear", LP.VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("name,compute", CASES, ids=CASE_IDS)
def test_value_and_input_gradient_equal_the_oracle(gpu, name, compute, linear):
    """B: mlp_value_and_input_grad under the identity transform, T(-f) and T(f)."""
    nets, ref = LP.networks(name, linear), _ref_rows(name, compute, linear)
    desc, th = _desc(name, compute, linear), dev(_theta(name, linear))
    for n in LP.ROWS:
        X = dev(np.stack([X[:n] for _, X in nets]))
        for negate in (True, False):
            val, grad = (a.cpu().numpy() for a in ops.mlp_value_and_input_grad(desc, th, X, "identity", negate))
            for i in range(LP.N_MODELS):
                v, g = ref[i, i]["vg"][negate]
                assert np.array_equal(val[i], v[:n]), (n, i, negate, "value")
                assert np.array_equal(grad[i], g[:n]), (n, i, negate, "gradient")
    _record("value_and_input_grad", "%s %s %s" % (name, compute, VARIANT_IDS[linear]), "exact")


# ---- C: screening ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _candidates(name, compute, Ns):
    """Integer candidates [3, Ns, D] and the oracle's predictions [3, Ns]."""
    nets = LP.networks(name)
    X = np.stack([LP.make_inputs(name, 900 + i, Ns) for i in range(LP.N_MODELS)])
    return X, np.stack([LP.ref_forward(net, X[i], compute) for i, (net, _) in enumerate(nets)])


def _check_screen(name, compute, Ns, R):
    X, want = _candidates(name, compute, Ns)
    x0, idx, pred = (a.cpu().numpy() for a in ops.screen_topk(_desc(name, compute), dev(_theta(name)), dev(X), R, want_pred=True))
    for i in range(LP.N_MODELS):
        assert np.array_equal(pred[i], want[i]), (Ns, R, i, "predictions")
        picks = np.lexsort((np.arange(Ns), -want[i]))[:R]         # descending prediction, ties to the lower row
        assert np.array_equal(idx[i], picks), (Ns, R, i, "picks")
        assert np.array_equal(x0[i], X[i][picks]), (Ns, R, i, "x0")
    return min(len(np.unique(w)) for w in want)


@pytest.mark.parametrize("name,compute", CASES, ids=CASE_IDS)
def test_screening_equals_the_oracle(gpu, monkeypatch, name, compute):
    """C: screen_topk on integer candidates in memory: both selection branches of screen_select (R <= 16: R passes; beyond:
    the bitonic sort).  The predictions tie heavily (the bfloat16 outputs of 1000 rows take a few hundred values), so the
    lower-row rule is held to the oracle's predictions, not to the kernel's own."""
    monkeypatch.delenv("BORE_SCREEN_SPLIT", raising=False)
    for Ns in (64, 100, 1000):
        for R in (1, 7, 16, 17, Ns):
            distinct = _check_screen(name, compute, Ns, R)
        if compute == "bfloat16":
            assert distinct < Ns, "the candidates do not tie"
    for split in ("0", "1"):            # one workgroup per model / predictions spread over several, then one selects
        monkeypatch.setenv("BORE_SCREEN_SPLIT", split)
        for R in (16, 17):
            _check_screen(name, compute, 2048, R)
    _record("screening", "%s %s" % (name, compute), "exact")


# ---- F1: zero-gradient decay ----------------------------------------------------------------------------------------------------
def _fit(desc, state, X, z, epochs, perm=None, seed=0, epoch0=0):
    lr, b1, b2 = LP.ADAM
    loss = ops.mlp_fit(desc, state["th"], state["m"], state["v"], state["t"], X, z, epochs, B, perm=perm, seed=seed,
                       epoch0=epoch0, lr=lr, beta1=b1, beta2=b2, eps=EPS)
    torch.cuda.synchronize()
    return loss.cpu().numpy()


def _state(th0, m0, v0, t0):
    return dict(th=dev(th0.astype(F32)), m=dev(np.asarray(m0, dtype=F32)), v=dev(np.asarray(v0, dtype=F32)),
                t=dev(np.asarray(t0, dtype=np.int64)))


def _host(state):
    return {k: a.cpu().numpy() for k, a in state.items()}


@functools.lru_cache(maxsize=None)
def _decay(name, i, t0, steps):
    """Model i's trajectory through `steps` zero-gradient steps from the unique slots (the same for both computes)."""
    th0 = _theta(name)
    m0, v0 = LP.unique_slots(LP.N_MODELS, th0.shape[1])
    return LP.adam_trajectory(th0[i], m0[i], v0[i], t0, [None] * steps)


def _check_state(got, want, where, worst):
    """m, v and t bit for bit; theta within the trajectory's bound.  -> the worst theta error / bound so far."""
    for i, T in enumerate(want):
        assert int(got["t"][i]) == T["t"], (where, i, "adam_t")
        assert np.array_equal(got["m"][i], T["m"]), (where, i, "m", int(np.sum(got["m"][i] != T["m"])))
        assert np.array_equal(got["v"][i], T["v"]), (where, i, "v", int(np.sum(got["v"][i] != T["v"])))
        r = LP.worst_ratio(got["th"][i], T["theta"], T["tol"])
        assert r <= 1.0, (where, i, "theta", r)
        worst = max(worst, r)
    return worst


def _other_form(name, compute):
    """One further N that puts the fit of device-drawn shuffles in its other form, or None where there is none within
    2048 rows.  bfloat16: the fp32-MFMA kernel once the shuffle no longer fits beside the bf16-MFMA kernel's weight
    images -- from 785 rows for 32->128-128-1, from 4401 for 16->64-64-64-1 (tests/native/fit_plan_dump.hip), which is
    beyond this file's sizes.  float32: the data set in LDS or in memory (fit_plan_query's data_in_lds), whichever
    N = 200 does not have; the nearest such N."""
    if compute == "bfloat16":
        return 785 if name == "32-128-128-1" else None
    desc, other = _desc(name, compute), []
    base = ops.fit_plan_query(desc, LP.N_MODELS, 200, B)["data_in_lds"]
    for N in range(1, 2049):
        try:
            if ops.fit_plan_query(desc, LP.N_MODELS, N, B)["data_in_lds"] != base:
                other.append(N)
        except _lib.UnsupportedError:         # (the shuffle of this many rows is not drawn on the device)
            break
    return min(other, key=lambda N: abs(N - 200)) if other else None


@pytest.mark.parametrize("name,compute", CASES, ids=CASE_IDS)
def test_zero_gradient_decay_keeps_every_adam_slot_in_its_place(gpu, name, compute):
    """F1: all labels 1, so every delta is exactly 0 whatever the batch.  Premise first: from m = v = 0 an epoch leaves
    theta, m and v untouched bit for bit and its loss is 0.  Then from slots that are unique per element of the launch
    (v0 > 0, both signs of m0) and t0 = 0 and 5 across the models: 1 epoch, 3 epochs, and 1 + 2 epochs in two launches,
    shuffles drawn on the device.  m and v equal the numpy float32 recurrence bit for bit, adam_t is exact, theta lies
    within the derived bound of the float64 recurrence."""
    nets = LP.networks(name)
    desc, th0 = _desc(name, compute), _theta(name)
    P = th0.shape[1]
    m0, v0 = LP.unique_slots(LP.N_MODELS, P)
    other = _other_form(name, compute)
    sizes = [1, 63, 64, 65, 200] + ([other] if other else [])
    worst = 0.0
    for N in sizes:
        X = dev(np.stack([_rows(X, N) for _, X in nets]).astype(F32))
        z = dev(np.ones((LP.N_MODELS, N), dtype=F32))
        steps = -(-N // B)
        st = _state(th0, np.zeros_like(th0), np.zeros_like(th0), [0, 5, 0])
        loss = _fit(desc, st, X, z, 1, seed=3)
        got = _host(st)
        assert np.array_equal(got["th"], th0) and not got["m"].any() and not got["v"].any(), (N, "the premise")
        assert not loss.any() and got["t"].tolist() == [steps, 5 + steps, steps], (N, "the premise", loss)
        for t0s in ((0, 5, 0), (5, 0, 5)):
            want = lambda E: [_decay(name, i, t0s[i], E * steps) for i in range(LP.N_MODELS)]
            one = _state(th0, m0, v0, t0s)
            assert not _fit(desc, one, X, z, 1, seed=3).any()
            worst = _check_state(_host(one), want(1), (N, t0s, "1 epoch"), worst)
            three = _state(th0, m0, v0, t0s)
            assert not _fit(desc, three, X, z, 3, seed=3).any()
            worst = _check_state(_host(three), want(3), (N, t0s, "3 epochs"), worst)
            assert not _fit(desc, one, X, z, 2, seed=3, epoch0=1).any()
            worst = _check_state(_host(one), want(3), (N, t0s, "1 + 2 epochs"), worst)
    print("%s %s: decay, sizes %s, worst theta error / bound %.3g" % (name, compute, sizes, worst))
    _record("decay_theta", "%s %s" % (name, compute), round(worst, 4))
    _record("decay_m_v_t", "%s %s" % (name, compute), "exact")


# ---- F2: one live batch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("linear", LP.VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("name,compute", CASES, ids=CASE_IDS)
def test_one_live_batch_returns_its_gradient_through_the_adam_slots(gpu, name, compute, linear):
    """F2: explicit shuffles; every row has label 1 but the rows of one batch of the epoch (the first, a middle one, the
    last partial one -- sizes 64, 32, 8 and 1: powers of two, so 1 / rows is exact), whose labels are mixed.  From
    m = v = 0 the inert batches before it leave the state alone, the live one writes its gradient into m and v, the
    ones behind it decay them: m and v equal the float32 recurrence fed the oracle's exact gradient, bit for bit; theta
    lies within the derived bound; the epoch's loss is the integer sum of the live label-0 logits over N, one rounding."""
    nets = LP.networks(name, linear)
    desc, th0 = _desc(name, compute, linear), _theta(name, linear)
    worst = worst_loss = 0.0
    for N, live in LP.LIVE:
        case = LP.live_case(name, linear, N, live)
        X, z, perm = (np.stack([c[k] for c in case]) for k in ("X", "z", "perm"))
        n_batches = -(-N // B)
        want, want_loss = [], []
        for i, (net, _) in enumerate(nets):
            rows = case[i]["rows"]
            logits, g = LP.ref_fit_grads(net, X[i][rows], z[i][rows], compute)
            grads = [None] * live + [pack(g).astype(np.float64)] + [None] * (n_batches - live - 1)
            want.append(LP.adam_trajectory(th0[i], np.zeros_like(th0[i]), np.zeros_like(th0[i]), 0, grads))
            want_loss.append(LP.mean_of(LP.loss_sum(logits, z[i][rows]), N))
        st = _state(th0, np.zeros_like(th0), np.zeros_like(th0), [0] * LP.N_MODELS)
        loss = _fit(desc, st, dev(X.astype(F32)), dev(z.astype(F32)), 1, perm=dev(perm[:, None, :]))
        got = _host(st)
        assert all(np.any(T["m"]) for T in want)
        worst = _check_state(got, want, (N, live), worst)
        for i, (ref, half_ulp) in enumerate(want_loss):
            r = abs(float(loss[i, 0]) - ref) / half_ulp
            assert r <= 1.0, (N, live, i, "loss", float(loss[i, 0]), ref)
            worst_loss = max(worst_loss, r)
    print("%s %s %s: live batch, worst theta error / bound %.3g" % (name, compute, VARIANT_IDS[linear], worst))
    _record("live_batch_theta", "%s %s %s" % (name, compute, VARIANT_IDS[linear]), round(worst, 4))
    _record("live_batch_loss", "%s %s %s" % (name, compute, VARIANT_IDS[linear]), round(worst_loss, 4))
    _record("live_batch_m_v_t", "%s %s %s" % (name, compute, VARIANT_IDS[linear]), "exact")


# ---- E: evaluate -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LP.SHAPES))
def test_evaluate_equals_the_integer_sum(gpu, name):
    """E: mlp_evaluate on the float32 descriptors, mixed labels: the loss is the integer sum of the label-0 logits over N
    (one rounding: the kernel divides two float32 values), the accuracy -- every logit is above 0.5, so the share of
    label-1 rows -- exact."""
    nets = LP.networks(name)
    desc, th = _desc(name, "float32"), dev(_theta(name))
    worst = 0.0
    for N in LP.EVAL_N:
        X, z = (np.stack(a) for a in zip(*LP.eval_case(name, N)))
        loss, acc = (a.cpu().numpy() for a in ops.mlp_evaluate(desc, th, dev(X.astype(F32)), dev(z.astype(F32))))
        for i, (net, _) in enumerate(nets):
            ref, half_ulp = LP.mean_of(LP.loss_sum(LP.ref_forward(net, X[i], "float32"), z[i]), N)
            r = abs(float(loss[i]) - ref) / half_ulp if ref else float(loss[i] != 0)
            assert r <= 1.0, (N, i, "loss", float(loss[i]), ref)
            assert acc[i] == F32(z[i].sum()) / F32(N), (N, i, "accuracy")
            worst = max(worst, r)
    _record("evaluate_loss", name, round(worst, 4))
    _record("evaluate_accuracy", name, "exact")
