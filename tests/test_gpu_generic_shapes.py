"""The run-time-layout kernel flavours (mlp_shapes.h: -1 .. -4 for up to four Dense layers of any width, 0 for five to
eight; layout tables read from LDS) against the float64 oracle, in every LDS kernel family: forward, value + input
gradient, fit, evaluate, screening, L-BFGS-B restarts and SVGD.  The static shapes 1 - 5 have their oracle tests in
test_gpu_parity.py / test_gpu_argmax.py / test_svgd.py; the networks a caller builds himself took these flavours with
self-consistency tests only.

One table of networks (NETS) serves every family.  Tolerances are the project's (DESIGN.md 2 and the tests named at
each constant), unchanged.  Every input here was chosen on the CPU so that the oracle's own float32 arithmetic stays
within HALF of the tolerance against its float64 arithmetic at every element (``oracle_margins`` below restates each
comparison with the float32 oracle in the kernel's place; tools/generic_shapes_margin.py writes the ratios to
profiles/generic_shapes/oracle_margin.json, and each test's docstring quotes the worst one).  Nothing is masked out of
a comparison.  On the device each test records its worst error / tolerance ratio (conftest.record_measurement; the
committed copy is profiles/generic_shapes/parity_measured.json).
"""
import functools

import numpy as np
import pytest
import torch

import lbfgsb_host as H
from bore_amd import _lib, ops
from conftest import record_measurement
from oracle import bore_oracle as O
from oracle.svgd_oracle import SVGD, DistortionConstant, DistortionExpDecay, RadialBasis
from test_gpu_parity import dev, pack, rand_model, unpack

pytestmark = pytest.mark.gpu

# ---- the networks ---------------------------------------------------------------------------------------------------
# key: (D, units, activations, gain, seed).  `gain` multiplies every Glorot kernel (biases stay rand_model's
# N(0, 0.1)): Glorot weights through five to eight layers collapse to a constant output, which would test nothing --
# every network's float64 output over the test inputs has a standard deviation above STD_FLOOR (asserted).
NETS = {
    # flavour -1: one layer, D one past a 16-tile (two k-tiles, the second holding one live row)
    "17-1": (17, [1], ["linear"], 1.0, 1),
    # flavour -2: hidden sigmoid (0.5 in A_1's padded columns 17 .. 31), ragged on both sides of the 16-tile
    "15-17-1": (15, [17, 1], ["sigmoid", "linear"], 2.0, 2),
    # flavour -3: three k-tiles of input (33), widths 15 / 33, hidden sigmoid, sigmoid output
    "33-15-33-1": (33, [15, 33, 1], ["tanh", "sigmoid", "sigmoid"], 3.0, 3),
    # flavour -3: hidden width 1 (a 16-wide tile with one live column, k = 1 into the next layer)
    "5-1-16-1": (5, [1, 16, 1], ["elu", "relu", "linear"], 2.0, 4),
    # flavour -4: widths one past, at and one short of the tile; hidden sigmoid in the first layer
    "9-17-16-15-1": (9, [17, 16, 15, 1], ["sigmoid", "elu", "tanh", "linear"], 2.0, 5),
    # flavour 0: five layers, every activation
    "3-16x4-1": (3, [16, 16, 16, 16, 1], ["relu", "elu", "tanh", "sigmoid", "linear"], 2.0, 6),
    # flavour 0: BORE_MAX_LAYERS = 8 layers, ragged widths, hidden sigmoids at widths 7 and 9 (nine and seven padded
    # columns of 0.5)
    "6-12-20-7-33-9-16-5-1": (6, [12, 20, 7, 33, 9, 16, 5, 1],
                              ["tanh", "relu", "sigmoid", "elu", "sigmoid", "tanh", "elu", "linear"], 2.0, 7),
    # flavour -3, the tile-shrinking branch of check_common (acquisition tests only; its fit streams).  LDS bytes from
    # bore_make_layout: Np = 32, 96, 96, 16; theta image P_lds = 32*98+96 + 96*98+96 + 96*18+16 = 14 480 floats
    # = 57 920 B; a tile row holds lda = 34 + 98 + 98 + 18 = 248 floats (with_deltas 0), twice that with D_0 .. D_n
    # (with_deltas 2); the rows kernels add BORE_BATCH_MAX + BORE_LAYOUT_FLOATS + 4 = 192 floats = 768 B.
    #   rows   with_deltas 0                      with_deltas 2
    #   64     57 920 + 63 488 + 768 = 122 176    57 920 + 126 976 + 768 = 185 664  (> 163 840: shrinks)
    #   48     57 920 + 47 616 + 768 = 106 304    57 920 +  95 232 + 768 = 153 920  (fits: value + gradient runs here)
    #   32     57 920 + 31 744 + 768 =  90 432    57 920 +  63 488 + 768 = 122 176
    #   16     57 920 + 15 872 + 768 =  74 560    57 920 +  31 744 + 768 =  90 432
    "24-96-96-1": (24, [96, 96, 1], ["relu", "tanh", "linear"], 1.0, 8),
}
SHRINK = "24-96-96-1"
FIT_NETS = [k for k in NETS if k != SHRINK]
DEEP5, DEEP8 = "3-16x4-1", "6-12-20-7-33-9-16-5-1"
STD_FLOOR = 0.05

# ---- tolerances (rtol, atol), all from the existing suite -------------------------------------------------------------
FWD_TOL = (2e-5, 2e-6)          # forward / value
GRAD_TOL = (2e-4, 2e-5)         # input gradient
FD_TOL = (2e-3, 2e-4)           # test_value_and_input_grad_matches_oracle: central differences, not negated
THETA_TOL = (1e-4, 5e-6)        # theta after a few Adam steps
M_TOL, V_TOL = (1e-3, 1e-7), (1e-3, 1e-9)   # test_sixteen_input_static_fits_against_the_float64_trajectory
LOSS_TOL = (2e-5, 0.0)
LONG_THETA_TOL, LONG_LOSS_TOL = (2e-4, 1e-5), (5e-5, 0.0)   # test_fit_edge_shapes_against_oracle
EVAL_TOL = (2e-5, 0.0)          # test_fit_reproduces_float64_golden_trajectory

FWD_ROWS = [1, 15, 16, 17, 63, 64, 65, 131]
SHRINK_ROWS = [47, 48, 49]
TRANSFORMS = [("identity", True), ("sigmoid", True), ("exp", True), ("sigmoid", False)]
FIT_CASES = [(100, 64, 3), (65, 64, 3), (40, 16, 2), (150, 100, 2)]    # 6, 6, 6 and 4 Adam steps
LONG_FIT = (100, 64, 40)                                               # 80 steps
LONG_NETS = ["15-17-1", "9-17-16-15-1"]
L2_NETS = ["15-17-1", DEEP8]
L2_A, L2_B = 1e-3, 3e-3
EVAL_ROWS = [1, 63, 64, 65, 200]

_measured = {}


def _ratio(got, ref, tol):
    """max |got - ref| in units of the tolerance atol + rtol |ref|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    diff = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, diff / (tol[1] + tol[0] * np.abs(ref)))
    return float(np.max(r)) if r.size else 0.0


def _check(test, case, label, got, ref, tol, worst):
    """One comparison: prints and returns its ratio (folded into `worst`), fails above 1."""
    r = _ratio(got, ref, tol)
    print("%-28s %-34s %-10s %.3g of tol" % (test, case, label, r))
    assert np.isfinite(r) and r <= 1.0, "%s %s %s: %.3g of the tolerance rtol=%g atol=%g" % (test, case, label, r, *tol)
    return max(worst, r)


def _record(test, case, worst):
    _measured.setdefault(test, {})[case] = round(worst, 4)
    record_measurement("generic_shapes/" + test, _measured[test])


def _desc(key, out_act=None, l2=False):
    D, units, acts, _, _ = NETS[key]
    acts = list(acts) if out_act is None else list(acts[:-1]) + [out_act]
    lk, lb = _l2_layers(len(units)) if l2 else (None, None)
    return _lib.make_desc(D, units, acts, lk, lb), acts


def _l2_layers(n):
    """Kernel and bias factors, different per layer and from each other: L2_A / L2_B alternating, the bias the other."""
    return [L2_A if i % 2 == 0 else L2_B for i in range(n)], [L2_B if i % 2 == 0 else L2_A for i in range(n)]


def _l2_tensors(n, swap=False):
    lk, lb = _l2_layers(n)
    if swap:
        lk, lb = lb, lk
    return [f for pair in zip(lk, lb) for f in pair]


def _flavour(key):
    """mlp_shapes.h, bore_kernel_flavour: none of NETS has a static shape's widths."""
    n = len(NETS[key][1])
    return -n if n <= 4 else 0


def _model(key, i=0):
    """float32 parameters of model `i` of a network (Keras order), kernels scaled by the network's gain."""
    D, units, _, gain, seed = NETS[key]
    p = rand_model(np.random.RandomState(1000 * seed + i), D, units)
    for j in range(0, len(p), 2):
        p[j] = (p[j] * np.float32(gain)).astype(np.float32)
    return p


@functools.lru_cache(maxsize=None)
def _fwd_inputs(key, i=0):
    D = NETS[key][0]
    X = np.random.RandomState(77 + 13 * NETS[key][4] + i).uniform(-1, 1, size=(131, D)).astype(np.float32)
    ref = O.predict(_model(key, i), NETS[key][2], X, dtype=np.float64)[:, 0]
    assert ref.std() > STD_FLOOR, (key, ref.std())
    return X, ref


@functools.lru_cache(maxsize=None)
def _vg_inputs(key, i=0):
    D = NETS[key][0]
    return np.random.RandomState(91 + 17 * NETS[key][4] + i).uniform(0, 1, size=(131, D))


@functools.lru_cache(maxsize=None)
def _vg_ref(key, transform, negate, i=0):
    p, acts, X = _model(key, i), NETS[key][2], _vg_inputs(key, i)
    if negate:
        return tuple(O.value_and_input_grad(p, acts, X, transform, dtype=np.float64))
    # T(f) (the SVGD form): closed-form value, central differences for the gradient (test_gpu_parity.py)
    assert transform == "sigmoid"
    sig = lambda f: 1 / (1 + np.exp(-f))
    f64 = lambda Z: O.predict(p, acts, Z, dtype=np.float64)[:, 0]
    h, rg = 1e-6, np.zeros_like(X)
    for j in range(X.shape[1]):
        e = np.zeros(X.shape[1])
        e[j] = h
        rg[:, j] = (sig(f64(X + e)) - sig(f64(X - e))) / (2 * h)
    return sig(f64(X)), rg


def _fit_inputs(key, N, B, E, i=0):
    D, _, _, _, seed = NETS[key]
    rs = np.random.RandomState(seed * 100003 + N * 131 + B * 7 + E + 977 * i)
    X = rs.uniform(size=(N, D)).astype(np.float32)
    z = (rs.uniform(size=N) < 0.3).astype(np.float32)
    perms = np.stack([rs.permutation(N) for _ in range(E)]).astype(np.int32)
    return _model(key, i), X, z, perms


@functools.lru_cache(maxsize=None)
def _fit_ref(key, N, B, E, l2=False, swap=False, dtype=np.float64, i=0):
    """The oracle's trajectory from _fit_inputs: dict of packed theta / m / v, t and the epoch losses."""
    p0, X, z, perms = _fit_inputs(key, N, B, E, i)
    acts = NETS[key][2]       # (a sigmoid output trains through its logits: the same trajectory as a linear one)
    p = [a.astype(dtype) for a in p0]
    st = O.AdamState(p)
    l2s = _l2_tensors(len(acts), swap) if l2 else None
    hist = O.fit(p, acts, st, X, z, perms, batch_size=B, l2=l2s, dtype=dtype)
    return dict(theta=pack64(p), m=pack64(st.m), v=pack64(st.v), t=st.t, loss=np.asarray(hist, dtype=np.float64))


def pack64(params):
    return np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in params])


def _gpu_fit(desc, thetas, X, z, perms, B):
    """One launch over len(thetas) models; X [L,N,D], z [L,N], perms [L,E,N]."""
    th = dev(np.stack(thetas).astype(np.float32))
    L = th.shape[0]
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    t = torch.zeros(L, dtype=torch.int64, device="cuda")
    loss = ops.mlp_fit(desc, th, m, v, t, dev(X), dev(z), perms.shape[1], B, perm=dev(perms))
    return dict(theta=th.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy(), t=t.cpu().numpy(),
                loss=loss.cpu().numpy())


def _compare_fit(test, case, got, ref, long_fit=False):
    w = 0.0
    assert int(got["t"][0]) == ref["t"]                       # the Adam counter is exact
    if long_fit:
        w = _check(test, case, "theta", got["theta"][0], ref["theta"], LONG_THETA_TOL, w)
        return _check(test, case, "loss", got["loss"][0], ref["loss"], LONG_LOSS_TOL, w)
    w = _check(test, case, "theta", got["theta"][0], ref["theta"], THETA_TOL, w)
    w = _check(test, case, "m", got["m"][0], ref["m"], M_TOL, w)
    w = _check(test, case, "v", got["v"][0], ref["v"], V_TOL, w)
    return _check(test, case, "loss", got["loss"][0], ref["loss"], LOSS_TOL, w)


@functools.lru_cache(maxsize=None)
def _eval_inputs(key, out_act, N, l):
    """Rows for evaluate at the trained theta of the first FIT_CASES fit (float64 oracle, rounded to float32), model
    l of 2 with its own data.  Premise of the exact accuracy comparison, asserted here on the float64 output: no row
    within 1e-3 of the 0.5 threshold."""
    D = NETS[key][0]
    acts = list(NETS[key][2][:-1]) + [out_act]
    theta = _fit_ref(key, *FIT_CASES[0], i=l)["theta"].astype(np.float32)
    p = unpack(theta, D, NETS[key][1])
    for attempt in range(64):       # the first seed of this case's sequence that satisfies the premise
        rs = np.random.RandomState(NETS[key][4] * 7919 + N * 3 + l + (0 if out_act == "linear" else 50000) + 100000 * attempt)
        X = rs.uniform(size=(N, D)).astype(np.float32)
        z = (rs.uniform(size=N) < 0.3).astype(np.float32)
        out = O.predict(p, acts, X, dtype=np.float64)[:, 0]
        if np.min(np.abs(out - 0.5)) >= 1e-3:
            break
    assert np.min(np.abs(out - 0.5)) >= 1e-3, (key, out_act, N, l, float(np.min(np.abs(out - 0.5))))
    return theta, p, acts, X, z


SCREEN_NETS = ["33-15-33-1", DEEP8, SHRINK]
SCREEN_CASES = [(77, 5), (1000, 16), (300, 300)]


def _screen_inputs(key, Ns, R, L=2):
    return np.random.RandomState(Ns + R + NETS[key][4]).uniform(-1, 1, size=(L, Ns, NETS[key][0]))


# ---- premises ---------------------------------------------------------------------------------------------------------
def _lds_bytes(D, units, rows, with_deltas, extra_floats):
    """bore_make_layout + check_common restated: theta image + tile + extra, in bytes."""
    up = lambda x: (x + 15) // 16 * 16
    w = [D] + list(units)
    p_lds = sum(up(w[l - 1]) * (up(w[l]) + 2) + up(w[l]) for l in range(1, len(w)))
    row = sum(up(x) + 2 for x in w)
    tile = up(rows) * row * (1 if with_deltas == 0 else 2)
    return 4 * (p_lds + tile + extra_floats)


def test_the_networks_take_the_lds_flavours_and_the_shrinking_one_shrinks(gpu):
    for key, (D, units, acts, _, _) in NETS.items():
        desc, _ = _desc(key)
        # (bore_kernel_flavour: -n_layers up to four layers, 0 beyond -- unless the widths are a static shape's)
        assert units not in ([16, 16, 1], [32, 32, 1], [64, 64, 64, 1], [128, 128, 1], [32, 32, 32, 1])
        assert _flavour(key) == (-len(units) if len(units) <= 4 else 0) and desc.n_layers == len(units) <= 8
        # bits 0 / 1: forward + evaluate / value + gradient on the streamed flavour; bit 2: the fit
        assert ops.mlp_streamed(desc) == (4 if key == SHRINK else 0), key
    # the premise of the shrinking network (the table at NETS): BORE_BATCH_MAX + BORE_LAYOUT_FLOATS + 4 extra floats
    D, units = NETS[SHRINK][0], NETS[SHRINK][1]
    extra, lds = 64 + 124 + 4, 160 * 1024
    assert _lds_bytes(D, units, 64, 0, extra) == 122176 <= lds
    assert _lds_bytes(D, units, 64, 2, extra) == 185664 > lds
    assert _lds_bytes(D, units, 48, 2, extra) == 153920 <= lds
    assert [_lds_bytes(D, units, r, 0, extra) for r in (48, 32, 16)] == [106304, 90432, 74560]
    assert [_lds_bytes(D, units, r, 2, extra) for r in (32, 16)] == [122176, 90432]


# ---- 1. forward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(NETS))
def test_forward_against_the_oracle(gpu, key):
    """Every 16-row block and 64-row tile boundary (and 47 / 48 / 49 rows for the shrinking network, whose forward tile
    nevertheless stays at 64).  Worst float32-oracle ratio: 0.28 of the tolerance (the eight-layer network)."""
    desc, acts = _desc(key)
    X, ref = _fwd_inputs(key)
    th = dev(pack(_model(key))).reshape(1, -1)
    w = 0.0
    for n in FWD_ROWS + (SHRINK_ROWS if key == SHRINK else []):
        out = ops.mlp_forward(desc, th, dev(X[:n])).cpu().numpy()[0]
        w = _check("forward", key, "n=%d" % n, out, ref[:n], FWD_TOL, w)
    _record("forward", key, w)


# ---- 2. value and input gradient --------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform,negate", TRANSFORMS)
@pytest.mark.parametrize("key", list(NETS))
def test_value_and_input_grad_against_the_oracle(gpu, key, transform, negate):
    """131 rows (three tiles of 48 for the shrinking network, two of 64 and a tail otherwise); a single row gives the
    bits it gives in the batch (rows 0, 47, 130: first, last of a 48-row tile, last).  Worst float32-oracle ratio: 0.30
    of the tolerance (9->17-16-15-1, exp)."""
    desc, acts = _desc(key)
    D, X = NETS[key][0], _vg_inputs(key)
    th = dev(pack(_model(key))).reshape(1, -1)
    val, grad = ops.mlp_value_and_input_grad(desc, th, dev(X).reshape(1, 131, D), transform, negate)
    assert val.dtype == torch.float32 and grad.dtype == torch.float64
    val, grad = val.cpu().numpy()[0], grad.cpu().numpy()[0]
    rv, rg = _vg_ref(key, transform, negate)
    case = "%s %s%s" % (key, transform, "" if negate else " +")
    w = _check("value_grad", case, "value", val, rv, FWD_TOL, 0.0)
    w = _check("value_grad", case, "grad", grad, rg, GRAD_TOL if negate else FD_TOL, w)
    for r in (0, 47, 130):
        v1, g1 = ops.mlp_value_and_input_grad(desc, th, dev(X[r:r + 1]).reshape(1, 1, D), transform, negate)
        np.testing.assert_array_equal(v1.cpu().numpy()[0, 0], val[r])
        np.testing.assert_array_equal(g1.cpu().numpy()[0, 0], grad[r])
    _record("value_grad", case, w)


# ---- 3. several models per launch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["33-15-33-1", DEEP8])
def test_several_models_per_launch_forward_and_value_grad(gpu, key):
    """n_models = 3 on the LDS path, shared rows and per-model rows: each model's results are the bits of its own
    launch; model 1 against the oracle.  Worst float32-oracle ratio for model 1: 0.21 forward (the eight-layer
    network), 0.015 value + gradient."""
    desc, acts = _desc(key)
    D, L = NETS[key][0], 3
    th = dev(np.stack([pack(_model(key, i)) for i in range(L)]))
    Xf = np.stack([_fwd_inputs(key, i)[0] for i in range(L)])
    Xg = np.stack([_vg_inputs(key, i) for i in range(L)])
    per = ops.mlp_forward(desc, th, dev(Xf)).cpu().numpy()
    shared = ops.mlp_forward(desc, th, dev(Xf[1])).cpu().numpy()
    val, grad = (a.cpu().numpy() for a in ops.mlp_value_and_input_grad(desc, th, dev(Xg), "sigmoid", True))
    vs, gs = (a.cpu().numpy() for a in ops.mlp_value_and_input_grad(
        desc, th, dev(np.broadcast_to(Xg[1], Xg.shape).copy()), "sigmoid", True))
    for i in range(L):
        one = th[i:i + 1]
        np.testing.assert_array_equal(ops.mlp_forward(desc, one, dev(Xf[i])).cpu().numpy()[0], per[i])
        np.testing.assert_array_equal(ops.mlp_forward(desc, one, dev(Xf[1])).cpu().numpy()[0], shared[i])
        for Xi, v, g in ((Xg[i], val[i], grad[i]), (Xg[1], vs[i], gs[i])):
            v1, g1 = ops.mlp_value_and_input_grad(desc, one, dev(Xi[None]), "sigmoid", True)
            np.testing.assert_array_equal(v1.cpu().numpy()[0], v)
            np.testing.assert_array_equal(g1.cpu().numpy()[0], g)
    w = _check("models", key, "forward", per[1], _fwd_inputs(key, 1)[1], FWD_TOL, 0.0)
    w = _check("models", key, "shared", shared[1], _fwd_inputs(key, 1)[1], FWD_TOL, w)
    rv, rg = _vg_ref(key, "sigmoid", True, 1)
    w = _check("models", key, "value", val[1], rv, FWD_TOL, w)
    w = _check("models", key, "grad", grad[1], rg, GRAD_TOL, w)
    w = _check("models", key, "grad shared", gs[1], rg, GRAD_TOL, w)
    _record("models", key, w)


# ---- 4. fit -----------------------------------------------------------------------------------------------------------
def _fit_both_wave_counts(monkeypatch, test, case, key, N, B, E, l2=False, long_fit=False):
    desc, acts = _desc(key, l2=l2)
    p0, X, z, perms = _fit_inputs(key, N, B, E)
    ref = _fit_ref(key, N, B, E, l2)
    assert ref["t"] == E * O.steps_per_epoch(N, B)
    outs, w = [], 0.0
    for w8 in ("0", "1"):
        monkeypatch.setenv("BORE_FIT_W8", w8)
        got = _gpu_fit(desc, [pack(p0)], X[None], z[None], perms[None], B)
        w = max(w, _compare_fit(test, case + " w8=" + w8, got, ref, long_fit))
        outs.append(got)
    # where the launch takes the eight-wave kernel (flavours -1 .. -4 with more than four weight-gradient tiles and
    # the Adam slots in LDS: 33->15-33-1 with nine and 9->17-16-15-1 with six) its bits are the four-wave kernel's;
    # elsewhere the two launches are the same kernel
    # (with l2 the reported loss adds the waves' shares of the penalty by LDS float atomics, in the order the waves
    # arrive: to the oracle's tolerance above, not to the bit; the state does not depend on it)
    for name in ("theta", "m", "v", "t") + (() if l2 else ("loss",)):
        np.testing.assert_array_equal(outs[0][name], outs[1][name], err_msg=name)
    _record(test, case, w)


@pytest.mark.parametrize("N,B,E", FIT_CASES)
@pytest.mark.parametrize("key", FIT_NETS)
def test_fit_against_the_float64_trajectory(gpu, monkeypatch, key, N, B, E):
    """theta, m, v, t and the epoch losses after 6, 6, 6 and 4 Adam steps: two steps per epoch with a full and a
    partial tile, a one-row last step, 16-row batches, and 100-row batches in 64 + 36-row sub-tiles; four-wave and
    eight-wave kernels.  Worst float32-oracle ratio: 0.057 of the tolerance (the eight-layer network, N = 40, B = 16);
    0.013 of it is the float32 rounding of 1 - beta2 in v, common to every case."""
    _fit_both_wave_counts(monkeypatch, "fit", "%s N=%d B=%d E=%d" % (key, N, B, E), key, N, B, E)


@pytest.mark.parametrize("key", LONG_NETS)
def test_long_fit_with_a_hidden_sigmoid_against_the_float64_trajectory(gpu, monkeypatch, key):
    """80 Adam steps of the two ragged nets whose first hidden layer is a sigmoid of width 17: A_1 has 15 padded
    columns that hold sigmoid(0) = 0.5 unless masked (mlp_regs.h, `< L.w[l]`), and the Adam task list's padding slots
    must keep working on zeros.  A padded column's 0.5 that reached a real weight would show here: in a numpy
    restatement of the step, letting ONE padded column of A_1 (0.5) into the next layer's sums through a padded weight
    row that Adam no longer holds at zero moves the float64 theta by 40 (15->17-1) and 44 (9->17-16-15-1) times this
    tolerance and the losses by 197 and 103 times theirs.  Worst float32-oracle ratio: 0.012 of the tolerance."""
    N, B, E = LONG_FIT
    _fit_both_wave_counts(monkeypatch, "fit_long", "%s N=%d B=%d E=%d" % (key, N, B, E), key, N, B, E, long_fit=True)


# ---- 5. fit with l2 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,E", [FIT_CASES[0], FIT_CASES[3]])
@pytest.mark.parametrize("key", L2_NETS)
def test_fit_with_l2_per_layer_against_the_float64_trajectory(gpu, monkeypatch, key, N, B, E):
    """kernel_regularizer / bias_regularizer l2 factors L2_A / L2_B alternating per layer, the bias taking the other
    one: a kernel that read a bias's factor (or a neighbouring layer's) leaves the tolerance -- on the CPU, the oracle
    with the two swapped moves theta by 239 to 551 times THETA_TOL (oracle_margins, "fit_l2_swap").  Worst
    float32-oracle ratio: 0.026 of the tolerance."""
    _fit_both_wave_counts(monkeypatch, "fit_l2", "%s N=%d B=%d E=%d" % (key, N, B, E), key, N, B, E, l2=True)


# ---- 6. warm start and replicas at a deep network ---------------------------------------------------------------------
def test_warm_start_and_replicas_at_the_eight_layer_network(gpu):
    """Two fits of E epochs == one of 2E (device-drawn shuffles continued through epoch0), and three models in one
    launch == three launches, bit for bit."""
    key, L, N, E, B = DEEP8, 3, 90, 3, 64
    desc, acts = _desc(key)
    ins = [_fit_inputs(key, N, B, E, i) for i in range(L)]
    th0 = [pack(p0) for p0, _, _, _ in ins]
    X, z = np.stack([a[1] for a in ins]), np.stack([a[2] for a in ins])

    def run(sel, splits):
        th = dev(np.stack([th0[i] for i in sel]))
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        t = torch.zeros(len(sel), dtype=torch.int64, device="cuda")
        losses, e0 = [], 0
        for e in splits:
            losses.append(ops.mlp_fit(desc, th, m, v, t, dev(X[sel]), dev(z[sel]), e, B, seed=21,
                                      model_index0=int(sel[0]), epoch0=e0))
            e0 += e
        return [a.cpu().numpy() for a in (th, m, v, t, torch.cat(losses, dim=1))]

    whole = run([0, 1, 2], [2 * E])
    assert (whole[3] == 2 * E * O.steps_per_epoch(N, B)).all() and np.isfinite(whole[0]).all()
    for a, b in zip(whole, run([0, 1, 2], [E, E])):
        np.testing.assert_array_equal(a, b)
    for i in range(L):
        for a, b in zip(whole, run([i], [2 * E])):
            np.testing.assert_array_equal(a[i], b[0])
    assert not np.array_equal(whole[0][0], whole[0][1])


# ---- 7. evaluate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("key", FIT_NETS)
def test_evaluate_against_the_oracle(gpu, key, l2):
    """bore_mlp_evaluate on the LDS path: two models with their own trained weights and data, N on and off the tile,
    sigmoid and logits outputs, with and without the l2 penalties; accuracy exact (no row left out).  Worst
    float32-oracle ratio: 0.020 of the tolerance, and the same accuracy."""
    w = 0.0
    for out_act in ("sigmoid", "linear"):
        desc, acts = _desc(key, out_act, l2)
        l2s = _l2_tensors(len(acts)) if l2 else None
        for N in EVAL_ROWS:
            ins = [_eval_inputs(key, out_act, N, l) for l in range(2)]
            loss, acc = ops.mlp_evaluate(desc, dev(np.stack([a[0] for a in ins])), dev(np.stack([a[3] for a in ins])),
                                         dev(np.stack([a[4] for a in ins])))
            loss, acc = loss.cpu().numpy(), acc.cpu().numpy()
            for l, (theta, p, _, X, z) in enumerate(ins):
                rl, ra = O.evaluate(p, acts, X, z, dtype=np.float64, l2=l2s)
                w = _check("evaluate", "%s l2=%d" % (key, l2), "%s N=%d m%d" % (out_act, N, l), loss[l], rl, EVAL_TOL, w)
                assert round(float(acc[l]) * N) == round(ra * N), (key, out_act, N, l, float(acc[l]), ra)
                assert abs(float(acc[l]) - ra) <= 1e-6
    _record("evaluate", "%s l2=%d" % (key, l2), w)


# ---- 8. screening -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ns,R", SCREEN_CASES)
@pytest.mark.parametrize("key", SCREEN_NETS)
def test_screen_topk_at_run_time_layouts(gpu, key, Ns, R):
    """Predictions are mlp_forward's bits on the float32-cast rows (and so held to the oracle by the forward test);
    the picks are the lexsort order of the kernel's own predictions.  Worst float32-oracle ratio: 0.43 of the tolerance (the
    eight-layer network, 1000 rows)."""
    desc, acts = _desc(key)
    D, L = NETS[key][0], 2
    params = [_model(key, i) for i in range(L)]
    th = dev(np.stack([pack(p) for p in params]))
    X = _screen_inputs(key, Ns, R, L)
    x0, idx, pred = (a.cpu().numpy() for a in ops.screen_topk(desc, th, dev(X), R, want_pred=True))
    fwd = ops.mlp_forward(desc, th, dev(X.astype(np.float32))).cpu().numpy()
    np.testing.assert_array_equal(pred, fwd)
    w = 0.0
    for l in range(L):
        w = _check("screen", "%s Ns=%d R=%d" % (key, Ns, R), "pred m%d" % l, pred[l],
                   O.predict(params[l], acts, X[l], dtype=np.float64)[:, 0], FWD_TOL, w)
        order = np.lexsort((np.arange(Ns), -pred[l]))[:R]          # descending value, ties by row
        np.testing.assert_array_equal(idx[l], order)
        np.testing.assert_array_equal(x0[l], X[l][order])
    _record("screen", "%s Ns=%d R=%d" % (key, Ns, R), w)


def test_sample_screen_topk_equals_the_two_launches_at_the_eight_layer_network(gpu):
    key, L, Ns, R = DEEP8, 2, 1000, 16
    desc, acts = _desc(key)
    D = NETS[key][0]
    th = dev(np.stack([pack(_model(key, i)) for i in range(L)]))
    rs = np.random.RandomState(5)
    lo, hi = rs.uniform(-2, 0, size=D), rs.uniform(0.5, 3, size=D)
    Xc = ops.uniform_candidates(91, L, Ns, lo, hi, model_index0=7, draw_index=4)
    a = ops.screen_topk(desc, th, Xc, R, want_pred=True)
    b = ops.sample_screen_topk(desc, th, 91, Ns, lo, hi, R, model_index0=7, draw_index=4, want_pred=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ---- 9. restarts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,tr", [("15-17-1", "sigmoid"), ("33-15-33-1", "identity"), (DEEP5, "exp"),
                                    (DEEP8, "sigmoid")])
def test_device_lbfgsb_equals_the_host_build_at_run_time_layouts(gpu, key, tr):
    """Every record of bore_lbfgsb_minimize is the host build of lbfgsb.h fed mlp_value_and_input_grad of the same
    model (which the value + gradient test holds to the oracle), bit for bit; the reported fun / jac are the rows
    kernel's at the reported x.  (No SciPy agreement share is asserted: none has been measured for these networks.)"""
    desc, acts = _desc(key)
    D, L, R = NETS[key][0], 2, 5
    th = dev(np.stack([pack(_model(key, i)) for i in range(L)]))
    X0 = np.random.RandomState(NETS[key][4]).uniform(-0.1, 1.1, size=(L, R, D))     # some starts outside the box
    lo, hi = np.zeros(D), np.ones(D)
    opts = dict(maxiter=30)
    x, fun, jac, info = (t.cpu().numpy() for t in ops.lbfgsb_minimize(desc, th, dev(X0), lo, hi, tr, True, **opts))
    assert ((x >= -1e-12) & (x <= 1 + 1e-12)).all()
    assert (info[:, :, 0] > 0).any()                                               # the searches iterate
    for l in range(L):
        def fg(xx):
            v, g = ops.mlp_value_and_input_grad(desc, th[l:l + 1], dev(np.atleast_2d(xx)[None]), tr, True)
            return v.cpu().numpy()[0, 0], g.cpu().numpy()[0, 0]
        for r in range(R):
            h = H.minimize(fg, X0[l, r], (lo, hi), **opts)
            np.testing.assert_array_equal(h.x, x[l, r])
            np.testing.assert_array_equal(h.fun, fun[l, r])
            np.testing.assert_array_equal(h.jac, jac[l, r])
            np.testing.assert_array_equal([h.nit, h.nfev, h.status, *h.task], info[l, r])
            v, g = fg(x[l, r])
            np.testing.assert_array_equal(v, fun[l, r])
            np.testing.assert_array_equal(g, jac[l, r])


# ---- 10. SVGD ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lambd", [(8, None), (70, None), (70, 0.5)])
@pytest.mark.parametrize("key", ["15-17-1", DEEP5])
def test_device_svgd_tracks_the_host_statement_at_run_time_layouts(gpu, key, n, lambd):
    """svgd_kernel (8 particles) and svgd_big_kernel (70) against SVGD.optimize_from_init driven by the device f / g,
    60 iterations, at test_svgd.py's bars."""
    desc, acts = _desc(key)
    D = NETS[key][0]
    th = dev(pack(_model(key))[None])
    x0 = np.random.RandomState(n + NETS[key][4]).uniform(size=(1, n, D))
    kw = dict(n_iter=60, step_size=1e-2, alpha=.9, eps=1e-6, tau=1.)
    out = ops.svgd_optimize(desc, th, dev(x0), np.zeros(D), np.ones(D), "sigmoid", lambd=lambd, **kw).cpu().numpy()
    assert ((out >= 0) & (out <= 1)).all() and (np.abs(out - x0) > 1e-4).any()

    def func(X):
        v, g = ops.mlp_value_and_input_grad(desc, th, dev(X[None]), "sigmoid", False)
        return v.cpu().numpy()[0].astype(np.float64), g.cpu().numpy()[0]
    dist = DistortionConstant() if lambd is None else DistortionExpDecay(lambd=lambd)
    ref = SVGD(kernel=RadialBasis(length_scale=None), distortion=dist, **kw).optimize_from_init(
        func, x0[0], bounds=[(0.0, 1.0)] * D)
    atol = 1e-9 if lambd is None else 1e-6
    case = "%s n=%d lambd=%s" % (key, n, lambd)
    _record("svgd", case, _check("svgd", case, "particles", out[0], ref, (0.0, atol), 0.0))


# ---- the float32 oracle in the kernel's place (CPU; tools/generic_shapes_margin.py) -------------------------------------
def oracle_margins():
    """Every oracle comparison above with the float32 oracle standing in for the kernel: worst ratio per case.  The
    inputs are kept only while every ratio is at most 0.5."""
    f32 = np.float32
    out = {"forward": {}, "value_grad": {}, "fit": {}, "fit_long": {}, "fit_l2": {}, "fit_l2_swap": {}, "evaluate": {},
           "screen": {}, "output_std": {}}
    for key in SCREEN_NETS:
        for Ns, R in SCREEN_CASES:
            X = _screen_inputs(key, Ns, R)
            out["screen"]["%s Ns=%d R=%d" % (key, Ns, R)] = max(
                _ratio(O.predict(_model(key, l), NETS[key][2], X[l])[:, 0],
                       O.predict(_model(key, l), NETS[key][2], X[l], dtype=np.float64)[:, 0], FWD_TOL) for l in range(2))
    for key in NETS:
        acts = NETS[key][2]
        for i in range(3):
            X, ref = _fwd_inputs(key, i)
            out["forward"]["%s m%d" % (key, i)] = _ratio(O.predict(_model(key, i), acts, X)[:, 0], ref, FWD_TOL)
            out["output_std"]["%s m%d" % (key, i)] = float(ref.std())
            for tr, neg in TRANSFORMS:
                rv, rg = _vg_ref(key, tr, neg, i)
                v, g = O.value_and_input_grad(_model(key, i), acts, _vg_inputs(key, i), tr)
                if not neg:       # sigmoid(f) = 1 - sigmoid(-f), gradient negated
                    v, g = f32(1) - v, -g
                out["value_grad"]["%s %s%s m%d" % (key, tr, "" if neg else " +", i)] = max(
                    _ratio(v, rv, FWD_TOL), _ratio(g, rg, GRAD_TOL if neg else FD_TOL))

    def fit_ratio(a, b, long_fit):
        if long_fit:
            return max(_ratio(a["theta"], b["theta"], LONG_THETA_TOL), _ratio(a["loss"], b["loss"], LONG_LOSS_TOL))
        return max(_ratio(a["theta"], b["theta"], THETA_TOL), _ratio(a["m"], b["m"], M_TOL),
                   _ratio(a["v"], b["v"], V_TOL), _ratio(a["loss"], b["loss"], LOSS_TOL))
    for key in FIT_NETS:
        for N, B, E in FIT_CASES:
            out["fit"]["%s N=%d B=%d E=%d" % (key, N, B, E)] = fit_ratio(
                _fit_ref(key, N, B, E, dtype=f32), _fit_ref(key, N, B, E), False)
    for key in LONG_NETS:
        out["fit_long"][key] = fit_ratio(_fit_ref(key, *LONG_FIT, dtype=f32), _fit_ref(key, *LONG_FIT), True)
    for key in L2_NETS:
        for N, B, E in (FIT_CASES[0], FIT_CASES[3]):
            case = "%s N=%d B=%d E=%d" % (key, N, B, E)
            ref = _fit_ref(key, N, B, E, True)
            out["fit_l2"][case] = fit_ratio(_fit_ref(key, N, B, E, True, dtype=f32), ref, False)
            # (not a margin: how far the kernel / bias factors swapped move the float64 theta, in tolerances)
            out["fit_l2_swap"][case] = _ratio(_fit_ref(key, N, B, E, True, True)["theta"], ref["theta"], THETA_TOL)
    for key in FIT_NETS:
        for l2 in (False, True):
            w = 0.0
            for out_act in ("sigmoid", "linear"):
                for N in EVAL_ROWS:
                    for l in range(2):
                        theta, p, acts, X, z = _eval_inputs(key, out_act, N, l)
                        l2s = _l2_tensors(len(acts)) if l2 else None
                        a, b = O.evaluate(p, acts, X, z, l2=l2s), O.evaluate(p, acts, X, z, dtype=np.float64, l2=l2s)
                        assert a[1] == b[1]
                        w = max(w, _ratio(a[0], b[0], EVAL_TOL))
            out["evaluate"]["%s l2=%d" % (key, l2)] = w
    return out
