"""Everything tests/test_gpu_numeric_range.py and tests/test_numeric_range_host.py share, with no device in it: the table
of probe values, the probe networks, the tolerances, the float64 references of every sweep, and -- for
tools/numeric_range_margin.py -- the float32 oracle in the kernel's place and the deliberately wrong formulas.  See the
docstring of tests/test_gpu_numeric_range.py for the design."""
import contextlib
import functools
import json
import os

import numpy as np

from oracle import bore_oracle as O

F32 = np.float32


def pack(params):
    return np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in params])

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN_JSON = os.path.join(ROOT, "profiles", "numeric_range", "oracle_margin.json")

U = 2.0 ** -24            # half an ulp of a float32 in [1, 2): the relative bound of ONE correctly rounded operation
RND = 2 * U               # budget per counted rounding / "<= 1 ulp" hardware operation: one ulp is at most 2^-23
#                           relative, and the float32 oracle (half an ulp per operation) then stays within half of it
FLOOR = 2.0 ** -126       # smallest normal float32
DENORM = 2.0 ** -149      # one float32 denormal step
SIG_OPS = 5               # fit_bce's sigmoid: exp2, the feedback fma, the add, rcp, the multiply ("<= 1 ulp" each, mlp_math.h);
#                           the bound on sig is SIG_OPS * 2^-24 * sig_ref
# ulp bounds of the ocml functions the IEEE forms call (HIP math API, maximum ulp error): expf 1, expm1f 1, log1pf 1,
# tanhf 2; IEEE division and every + - * are correctly rounded (half an ulp, budgeted RND as above)
K_EXP, K_EXPM1, K_LOG1P, K_TANH = 1, 1, 1, 2


def _f(x):
    return float(F32(x))


def _nb(x):
    """A float32 seam with both float32 neighbours."""
    x = F32(x)
    return [float(np.nextafter(x, F32(-np.inf))), float(x), float(np.nextafter(x, F32(np.inf)))]


# ---- 1. the probe values (one table) ------------------------------------------------------------------------------------
SEAM_RCP = 16.6355        # 1 + e^-x rounds to 1 just beyond
_LOGIT_POS = [2.0 ** -20, 1, 8] + _nb(SEAM_RCP) + [17, 40, 87, 87.5, 88, 100, 103.9, 104.5, 1000, 10000]
LOGITS = [0.0] + [_f(s * x) for x in _LOGIT_POS for s in (1, -1)]
SEAM_ELU, LN2 = -0.03125, -0.6931472
HIDDEN = ([_f(s * x) for x in (2.0 ** -30, 1e-3) for s in (1, -1)] + _nb(SEAM_ELU) + [-0.5] + _nb(LN2)
          + [_f(x) for x in (-1, -5, -17, -87, -88, -104, -10000, 1, 20, 100, 10000)])
RELU_KINK = [2.0 ** -126, -2.0 ** -126, 0.0]
NEVER_DROPPED = set(_nb(SEAM_ELU) + _nb(SEAM_RCP) + [-x for x in _nb(SEAM_RCP)])
ADAM_G = [0.0, 1e-30, 1e-23, 1e-20, 1e-12, 1e-7, 1e-3, 1.0, 1e3, 1e15, 1e19]     # and their negatives (label 1)
ADAM_SLOTS = [(_f(a), _f(b)) for a, b in [(0.0, 0.0), (1e-3, 1e-6), (-1e-3, 0.0), (1e-20, 1e-38), (1.0, 1e30)]]   # (m0, v0)
ADAM_T0 = [0, 1, 9, 999, 10 ** 4, 10 ** 6, 2 ** 31, 10 ** 12]
ADAM_CFGS = [(lr, b1, b2) for (b1, b2) in ((0.9, 0.999), (0.0, 0.5)) for lr in (1e-3, 1.0)]
EPS = 1e-7
HIDDEN_ACTS = ["linear", "relu", "elu", "sigmoid", "tanh"]

# ---- 2. the fit kernels ---------------------------------------------------------------------------------------------------
# name: (D, units, output activation, hidden activations the flavour allows (None = any), environment)
# (BORE_FIT_W8 = 0 where the eight-wave kernel would otherwise be chosen by the launch size, so that each name is one kernel)
W4, W8 = {"BORE_FIT_W8": "0"}, {"BORE_FIT_W8": "1"}
FIT_FLAVOURS = {
    "static 1 2-16-16-1": (2, [16, 16, 1], "sigmoid", ["relu"], W4),
    "static 2 6-32-32-1": (6, [32, 32, 1], "linear", None, W4),
    "static 3 16-64-64-64-1": (16, [64, 64, 64, 1], "linear", None, W4),
    "static 5 16-32-32-32-1": (16, [32, 32, 32, 1], "linear", None, W4),
    "fit-only 6 16-32-32-1": (16, [32, 32, 1], "sigmoid", None, W4),
    "fit-only 7 16-16-16-1": (16, [16, 16, 1], "linear", None, W4),
    "padded 3-32-32-32-1": (3, [32, 32, 32, 1], "linear", None, dict(W4, BORE_FIT_PAD="1")),
    "eight-wave 6-32-32-1": (6, [32, 32, 1], "linear", None, W8),
    "eight-wave 9-17-16-15-1": (9, [17, 16, 15, 1], "linear", None, W8),
    "generic -1 17-1": (17, [1], "linear", None, W4),
    "generic -2 5-1-1": (5, [1, 1], "sigmoid", None, W4),
    "generic -3 5-7-3-1": (5, [7, 3, 1], "linear", None, W4),
    "generic -4 9-17-16-15-1": (9, [17, 16, 15, 1], "linear", None, W4),
    "generic 0 3-16x4-1": (3, [16, 16, 16, 16, 1], "linear", None, W4),
    "streamed forced 5-7-3-1": (5, [7, 3, 1], "linear", None, {"BORE_STREAM": "1"}),
    "streamed native 8-250-130-1": (8, [250, 130, 1], "linear", None, {}),     # (ragged widths beyond one panel)
}
# the mixed-precision fit (bore_mlp_fit with compute = bfloat16: the two wide static shapes, 64-row batches), against
# oracle.loss_and_grads_bf16; every probe value is rounded to bfloat16 first
BF16_FIT = {
    "bf16 static 3 16-64-64-64-1": (16, [64, 64, 64, 1], "linear", None, {}),
    "bf16 static 4 32-128-128-1": (32, [128, 128, 1], "linear", None, {}),
}
ALL_FIT = dict(FIT_FLAVOURS, **BF16_FIT)
BATCHES = [1, 64]         # B = 1 (a one-row tile: the run-time-layout kernels) and B = 64 (a partial batch of one row)


def _ulp32(x):
    """Spacing of float32 at |x|."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def _bf16_ulp(x):
    """One bfloat16 ulp at |x| (a normal value): 2^(exponent - 7)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(x > 0, 2.0 ** (np.floor(np.log2(np.where(x > 0, x, 1.0))) - 7), 0.0)


def _floor(ref, floor=FLOOR):
    """The absolute allowance where the reference lies under the normal range."""
    return np.where(np.abs(ref) < FLOOR, floor, 0.0)


# ---- probe networks ---------------------------------------------------------------------------------------------------
def _zeros(D, units):
    p, k = [], D
    for u in units:
        p += [np.zeros((k, u)), np.zeros(u)]
        k = u
    return p


def _chain(p, widths, first, c0, value=1.0):
    """Selector kernels from layer `first` (1-based) on: unit j of layer l - 1 feeds unit j of layer l with weight
    `value`, for every j below both widths.  Returns the unit of the last HIDDEN layer that unit c0 of layer first - 1
    reaches, c0 itself (the output kernel is left to the caller)."""
    for l in range(first, len(widths) - 1):
        k, w = widths[l - 1], widths[l]
        for j in range(min(k, w)):
            p[2 * (l - 1)][j, j] = value
        assert c0 < min(k, w)
    return c0


def _chain_unit(widths, first, i):
    """A unit of layer first - 1 from which the chain never leaves the narrower side: index below every later width."""
    return i % min(widths[first - 1:-1])


def logit_model(D, units, x, i):
    """Input e_j, a chain of ones through relu / linear hidden layers, output kernel x at the chain's end: logit = 1 * x."""
    widths = [D] + list(units)
    p = _zeros(D, units)
    j0 = _chain_unit(widths, 1, i)
    row = np.zeros(D)
    row[j0] = 1.0
    c = _chain(p, widths, 1, j0)
    p[-2][c, 0] = x
    return p, row


def hidden_model(D, units, layer, values, i, w_out=2.0 ** -10):
    """All-zero row; the biases of hidden layer `layer` hold `values` rotated so that the chain's unit holds values[i];
    ones carry every unit on through the later (linear / relu) layers; the output kernel holds w_out at the chain's end."""
    widths = [D] + list(units)
    p = _zeros(D, units)
    c0 = _chain_unit(widths, layer + 1, i)
    w = widths[layer]
    p[2 * (layer - 1) + 1][:] = [values[(i + j - c0) % len(values)] for j in range(w)]
    c = _chain(p, widths, layer + 1, c0)
    p[-2][c, 0] = w_out
    return p, np.zeros(D)


def _bf(x):
    return float(O.bf16_round(F32(x)))


def adam_model(D, units, gs, sign, rnd=_f):
    """Logit 0 (zero output kernel and bias): d loss / d logit = 0.5 (label 0) or -0.5 (label 1) up to the fit's sigmoid
    of 0.  The activations in front of the output kernel are 2 |g_j| (inputs of a one-layer net, biases of the first
    hidden layer otherwise, carried by ones through relu layers), so the output kernel's gradients are +-g_j."""
    widths = [D] + list(units)
    p = _zeros(D, units)
    row = np.zeros(D)
    if len(units) == 1:
        row[:len(gs)] = [rnd(2 * g) for g in gs]
    else:
        p[1][:len(gs)] = [rnd(2 * g) for g in gs]
        _chain(p, widths, 2, 0)
    return p, row


def adam_capacity(D, units):
    return D if len(units) == 1 else min(units[:-1])


# ---- tolerances -----------------------------------------------------------------------------------------------------------
def act_tolerance(act, a, h, fit):
    """|act(a) - h| allowed, a exact.  fit_elu: the header's claim (absolute 2^-24 AND relative 2e-6); ocml expm1f / tanhf
    by their ulp bounds; sigmoid_stable: expf (K_EXP ulp, weight e / (1 + e) <= 1/2 for x >= 0, 1 for x < 0), the add
    and the division -- at most (2 K_EXP + 2) roundings' worth; relu and linear are exact."""
    a, h = np.asarray(a, dtype=np.float64), np.asarray(h, dtype=np.float64)
    if act == "elu":
        t = np.minimum(U, 2e-6 * np.abs(h)) if fit else K_EXPM1 * RND * np.abs(h)
        t = np.where(a < 0, t, 0.0)
    elif act == "sigmoid":
        t = (2 * K_EXP + 2) * RND * np.abs(h)
    elif act == "tanh":
        t = K_TANH * RND * np.abs(h)
    else:
        return np.zeros_like(h)
    return t + _floor(h, FLOOR if fit else DENORM)


def act_grad_tolerance(act, h, th):
    """|act'(h) - ref| allowed for an output h known to th: the formula's sensitivity to h plus its own roundings."""
    h = np.asarray(h, dtype=np.float64)
    if act == "elu":
        return np.where(h > 0, 0.0, th + RND * np.abs(h + 1))
    if act == "sigmoid":
        return np.abs(1 - 2 * h) * th + th * th + 2 * RND * np.abs(h * (1 - h))
    if act == "tanh":
        return 2 * np.abs(h) * th + th * th + RND * (h * h + np.abs(1 - h * h))
    return np.zeros_like(h)


def grad_tolerances(p, acts, row, z, fit=True, bf16=False, fit_act=None):
    """float64 loss and gradients of one row (O.loss_and_grads' algebra) with a first-order error bound for each: every
    input is exact, every selector product is exact, each further operation adds its rounding budget.
    bf16: the mixed-precision step rounds every layer output, the logit and every delta to bfloat16; where the float32
    value in front of such a rounding is not exact, a last-bit difference can flip it: one bfloat16 ulp more.
    Returns dict(loss, tloss, g, tg, logit, tlogit, delta, tdelta)."""
    n = len(acts)
    fit_act = fit if fit_act is None else fit_act       # (the bfloat16 fit: fit_bce's arithmetic, ocml's activations)
    flip = (lambda v, t: np.where(t > 0, _bf16_ulp(v), 0.0)) if bf16 else (lambda v, t: 0.0)
    h, th = np.asarray(row, dtype=np.float64), np.zeros(len(row))
    hs, ths = [h], [th]
    for l in range(n):
        W, b = p[2 * l], p[2 * l + 1]
        s = h @ W
        pre = s + b
        tpre = th @ np.abs(W) + RND * np.abs(pre) * ((s != 0) & (b != 0))     # (the bias add rounds only if both are nonzero)
        if l == n - 1:
            tpre = tpre + flip(pre, tpre)
            break
        h = O._act(acts[l], pre)
        th = np.abs(O._act_grad_from_output(acts[l], h)) * tpre + act_tolerance(acts[l], pre, h, fit_act)
        th = th + flip(h, th)
        hs.append(h)
        ths.append(th)
    x, tx = pre, tpre
    e = np.exp(-np.abs(x))
    sig = np.where(x >= 0, 1 / (1 + e), e / (1 + e))
    delta = sig - z
    # sig: SIG_OPS operations of one ulp, carried through the subtraction unchanged, plus half an ulp of the result;
    # the logit's own error through sig' <= 1/4
    tdelta = SIG_OPS * U * sig + sig * (1 - sig) * tx + 0.5 * _ulp32(delta) + _floor(delta)
    tdelta = tdelta + flip(delta, tdelta)
    # loss = max(x, 0) - x z + log1p(e): z is 0 or 1, so the first two terms are x, 0 or -x exactly; e to 3 roundings
    # (exp2, feedback, fma) in the fit and K_EXP ulp in the IEEE form, weighted by d log1p / d e * e = e / (1 + e);
    # log1pf's K_LOG1P ulp; the final add and the epoch's division by N; the logit's error through |sig - z|; where
    # log1p(e) lies under 2^-126, the fit's flush (2^-126) -- the IEEE form (bce_loss in evaluate) is held to ONE DENORMAL STEP
    lin = np.maximum(x, 0) - x * z
    loss = lin + np.log1p(e)
    tloss = ((3 if fit else K_EXP) * RND * e / (1 + e) + K_LOG1P * RND * np.log1p(e) + 2 * RND * np.abs(loss)
             + np.abs(delta) * tx + _floor(np.log1p(e), FLOOR if fit else DENORM))
    g, tg = [None] * (2 * n), [None] * (2 * n)
    d, td = delta, tdelta
    for l in range(n - 1, -1, -1):
        gw = np.outer(hs[l], d)
        g[2 * l], tg[2 * l] = gw, np.outer(np.abs(hs[l]), td) + np.outer(ths[l], np.abs(d) + td) + RND * np.abs(gw)
        g[2 * l + 1], tg[2 * l + 1] = d.copy(), td.copy()
        if l > 0:
            W = p[2 * l]
            back, tback = d @ W.T, td @ np.abs(W).T
            tback = tback + RND * np.abs(back)                    # (delta x weight: one rounding)
            ag = O._act_grad_from_output(acts[l - 1], hs[l])
            tag = act_grad_tolerance(acts[l - 1], hs[l], ths[l])
            d = back * ag
            td = tback * np.abs(ag) + (np.abs(back) + tback) * tag + RND * np.abs(d)
            td = td + flip(d, td)
    tg = [t + _floor(a) for t, a in zip(tg, g)]
    return dict(loss=float(loss[0]), tloss=float(tloss[0]), g=g, tg=tg, logit=float(x[0]), delta=float(delta[0]),
                tdelta=float(tdelta[0]))


def _cat(arrs):
    return np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in arrs])


def alpha_tolerance(t, b1, b2):
    """Relative bound on AdamClock's step size lr sqrtf(1 - (float) b2^t) / (1 - (float) b1^t): the powers are rounded to
    float32 (2^-24 relative each) before 1 - beta^t cancels, which multiplies that by beta^t / (1 - beta^t) -- 499 at
    t = 2 for beta2 = 0.999, halved by the square root; then the two subtractions, sqrtf, the product and the
    division, all IEEE: 4.5 roundings' worth.  Budgeted at RND per rounding like everything else here."""
    b1p, b2p = np.power(b1, float(t)), np.power(b2, float(t))
    return RND * (0.5 * b2p / (1 - b2p) + b1p / (1 - b1p) + 4.5)


def adam_tolerances(g, tg, theta, m0, v0, t0, lr, b1, b2, eps, f32_ratio):
    """adam_update in float64 from prepared slots (float64 arrays / the float32-rounded hyper-parameters) with bounds for
    m', v' and the update theta' - theta, by operation count:
      m' = m + (g - m)(1 - b1): three roundings;  v' = v + (g g - v)(1 - b2): four;
      update = -(m' alpha) rcp(sqrt(v') + eps): the product m' alpha (which may itself fall under 2^-126 while the
      update does not), sqrt and rcp at one ulp each, the add, the last product, and alpha's own bound.
    The formula itself loses accuracy in float32 (1 - beta2^t at small t, g - m at beta1 = 0), so the bound on the update
    is the larger of this count and twice the float32 oracle's worst ratio against it over the same (t0, betas, lr)
    group of the table: `f32_ratio`, measured on the CPU by tools/numeric_range_margin.py, never on the kernel."""
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    alpha = float(O.adam_alpha(t0 + 1, lr, b1, b2, np.float64))
    m1 = m0 + (g - m0) * omb1
    tm = omb1 * tg + RND * (2 * np.abs(g - m0) * omb1 + np.abs(m1)) + _floor(m1)
    v1 = v0 + (g * g - v0) * omb2
    tv = (omb2 * (2 * np.abs(g) * tg + tg * tg) + RND * (g * g * omb2 + 2 * np.abs(g * g - v0) * omb2 + np.abs(v1))
          + _floor(v1))
    s = np.sqrt(v1)
    ts = np.minimum(0.5 * tv / np.where(s > 0, s, 1.0), np.sqrt(tv)) + RND * s     # (sqrt(v + d) - sqrt(v) <= sqrt(d))
    ts = np.where(s > 0, ts, np.sqrt(tv))
    den = s + eps
    ma = m1 * alpha
    tma = tm * alpha + np.abs(ma) * (alpha_tolerance(t0 + 1, b1, b2) + RND) + _floor(ma)
    upd = -ma / den
    tupd = tma / den + np.abs(upd) * ((ts + RND * den) / den + 2 * RND)             # the add, rcp, the last product
    tupd = tupd * max(1.0, 2 * f32_ratio)
    tupd = tupd + _ulp32(theta + upd) + _floor(upd)    # theta' is rounded once more (budgeted a whole ulp); read as theta' - theta
    return dict(m=m1, tm=tm, v=v1, tv=tv, upd=upd, tupd=tupd, alpha=alpha)


def _hyper(lr, b1, b2):
    """The float32-rounded hyper-parameters (bore_adam_cfg), as float64."""
    return _f(lr), _f(b1), _f(b2), _f(EPS)


@functools.lru_cache(maxsize=None)
def f32_adam_ratio():
    """profiles/numeric_range/oracle_margin.json, 'adam_f32_ratio': see adam_tolerances."""
    with open(MARGIN_JSON) as f:
        return json.load(f)["adam_f32_ratio"]


def adam_key(t0, lr, b1, b2):
    return "t0=%d lr=%g betas=%g,%g" % (t0, lr, b1, b2)


# ---- sweeps: lists of models with their float64 references and tolerances -------------------------------------------------
def _acts(n_layers, hidden, out):
    return [hidden] * (n_layers - 1) + [out]


def sweep_models(name, sweep):
    """-> list of launches: dict(acts, cfg (lr, b1, b2), models [dict(p, row, z, m0, v0, t0, label)])."""
    D, units, out, allowed, _ = ALL_FIT[name]
    return _sweep_models(D, tuple(units), out, None if allowed is None else tuple(allowed), name in BF16_FIT, sweep)


def _sweep_models(D, units, out, allowed, bf16, sweep):
    units = list(units)
    n = len(units)
    launches = []
    rnd = _bf if bf16 else _f
    if sweep == "logit":
        logits = sorted(set(_bf(x) for x in LOGITS)) if bf16 else LOGITS
        models = [dict(zip(("p", "row"), logit_model(D, units, x, i)), z=z, label="x=%r z=%d" % (x, z), value=x)
                  for i, (x, z) in enumerate((x, z) for x in logits for z in (0.0, 1.0))]
        launches.append(dict(acts=_acts(n, "relu", out), cfg=ADAM_CFGS[0], models=models))
    elif sweep == "hidden":
        for layer in range(1, n):
            for act in (allowed or HIDDEN_ACTS):
                values = (HIDDEN if allowed is None else []) + (RELU_KINK if act == "relu" else [])
                if bf16:
                    values = sorted(set(_bf(a) for a in values))
                acts = _acts(n, "relu" if allowed else "linear", out)
                acts[layer - 1] = act
                models = [dict(zip(("p", "row"), hidden_model(D, units, layer, values, i)), z=float(i % 2),
                               label="layer %d %s a=%r" % (layer, act, a), value=a) for i, a in enumerate(values)]
                launches.append(dict(acts=acts, cfg=ADAM_CFGS[0], models=models))
    elif sweep == "adam":
        cap = adam_capacity(D, units)
        chunks = [ADAM_G[k:k + cap] for k in range(0, len(ADAM_G), cap)]
        for cfg in ADAM_CFGS:
            models = [dict(zip(("p", "row"), adam_model(D, units, gs, sign, rnd)), z=float(sign < 0), m0=m0, v0=v0, t0=t0,
                           label="g=%s%r m0=%g v0=%g t0=%d" % ("-" if sign < 0 else "", gs, m0, v0, t0))
                      for t0 in ADAM_T0 for (m0, v0) in ADAM_SLOTS for sign in (1, -1) for gs in chunks]
            launches.append(dict(acts=_acts(n, "relu", out), cfg=cfg, models=models))
    else:
        raise ValueError(sweep)
    for launch in launches:
        launch["bf16"] = bf16
    return launches


def reference(launch, mdl, dtype=np.float64):
    """One Adam step of oracle.fit in `dtype` from the model's slots: packed m, v, theta' - theta, the loss and t."""
    lr, b1, b2, eps = _hyper(*launch["cfg"])
    p = [a.astype(dtype) for a in mdl["p"]]
    th0 = _cat(p)
    st = O.AdamState(p)
    st.t = mdl.get("t0", 0)
    for a, b in zip(st.m, st.v):
        a += dtype(mdl.get("m0", 0.0))
        b += dtype(mdl.get("v0", 0.0))
    with np.errstate(over="ignore", under="ignore"):
        hist = O.fit(p, launch["acts"], st, mdl["row"][None], np.array([mdl["z"]]), np.zeros((1, 1), dtype=np.int64),
                     batch_size=1, lr=lr, beta1=b1, beta2=b2, eps=eps, dtype=dtype)
    return dict(m=_cat(st.m), v=_cat(st.v), upd=_cat(p) - th0, loss=float(hist[0]), t=st.t)


def tolerances(launch, mdl):
    """Reference values and bounds of one model: dict(m, tm, v, tv, upd, tupd, loss, tloss, delta)."""
    lr, b1, b2, eps = _hyper(*launch["cfg"])
    with np.errstate(over="ignore", under="ignore"):
        G = grad_tolerances(mdl["p"], launch["acts"], mdl["row"], mdl["z"])
        t0 = mdl.get("t0", 0)
        A = adam_tolerances(_cat(G["g"]), _cat(G["tg"]), _cat(mdl["p"]), mdl.get("m0", 0.0), mdl.get("v0", 0.0), t0,
                            lr, b1, b2, eps,
                            launch["f32_ratio"] if "f32_ratio" in launch else f32_adam_ratio()[adam_key(t0, *launch["cfg"])])
    return dict(A, loss=G["loss"], tloss=G["tloss"], delta=G["delta"], logit=G["logit"])


def tolerances_bf16(launch, mdl):
    """The mixed-precision step: gradients from oracle.loss_and_grads_bf16 (float32; in a probe network every product
    is bfloat16 x bfloat16 and exact), bounded by grad_tolerances(bf16=True): the float32 bounds plus one bfloat16 ulp
    at every rounding whose operand is not exact.  The update is float32 Adam, as in the float32 fit."""
    lr, b1, b2, eps = _hyper(*launch["cfg"])
    acts = launch["acts"]
    p32 = [a.astype(F32) for a in mdl["p"]]
    assert all(np.array_equal(O.bf16_round(a), a) for a in p32) and np.array_equal(O.bf16_round(mdl["row"].astype(F32)), mdl["row"])
    with np.errstate(over="ignore", under="ignore"):
        loss, g = O.loss_and_grads_bf16(p32, acts, mdl["row"][None].astype(F32), np.array([mdl["z"]], dtype=F32))
        G = grad_tolerances(mdl["p"], acts, mdl["row"], mdl["z"], fit=True, bf16=True, fit_act=False)
        g = [np.asarray(a, dtype=np.float64) for a in g]
        # (the float64 algebra and the bfloat16 oracle are two statements of one step: within the bound of each other)
        assert all((np.abs(a - b) <= t).all() for a, b, t in zip(g, G["g"], G["tg"])), mdl["label"]
        t0 = mdl.get("t0", 0)
        A = adam_tolerances(_cat(g), _cat(G["tg"]), _cat(mdl["p"]), mdl.get("m0", 0.0), mdl.get("v0", 0.0), t0, lr, b1,
                            b2, eps, f32_adam_ratio()[adam_key(t0, *launch["cfg"])])
    return dict(A, loss=float(loss), tloss=G["tloss"], delta=G["delta"], logit=G["logit"], t=t0 + 1)


def ratios(got, T, sel=slice(None)):
    """Worst |got - ref| / tolerance of m, v, the update (over the parameters `sel`) and the loss of one model."""
    out = {}
    for k, tk in (("m", "tm"), ("v", "tv"), ("upd", "tupd")):
        diff = np.abs(np.asarray(got[k], dtype=np.float64) - T[k])[sel]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(diff == 0, 0.0, diff / T[tk][sel])
        out[k] = float(np.max(r))
    d = abs(float(got["loss"]) - T["loss"])
    out["loss"] = 0.0 if d == 0 else (d / T["tloss"] if T["tloss"] > 0 else np.inf)
    return out


def sweep_reference(name, sweep):
    """[(launch, [(model, tolerances)])], with the agreement of `tolerances`' float64 algebra and oracle.fit asserted.
    Computed once per distinct network: flavours that differ only in the kernel they select share it."""
    D, units, out, allowed, _ = ALL_FIT[name]
    return _sweep_reference(D, tuple(units), out, None if allowed is None else tuple(allowed), name in BF16_FIT, sweep)


@functools.lru_cache(maxsize=None)
def _sweep_reference(D, units, out_act, allowed, bf16, sweep):
    name = "%d->%s" % (D, "-".join(map(str, units)))
    out = []
    for launch in _sweep_models(D, units, out_act, allowed, bf16, sweep):
        rows = []
        if launch["bf16"]:
            out.append((launch, [(mdl, tolerances_bf16(launch, mdl)) for mdl in launch["models"]]))
            continue
        for mdl in launch["models"]:
            T, R = tolerances(launch, mdl), reference(launch, mdl)
            r = ratios(R, T)           # (the two float64 statements differ by float64 roundings only)
            assert max(r.values()) < 1e-6, (name, sweep, mdl["label"], r)
            rows.append((mdl, dict(T, m=R["m"], v=R["v"], upd=R["upd"], loss=R["loss"], t=R["t"])))
        out.append((launch, rows))
    return out


# ---- the float32 oracle in the kernel's place, and wrong formulas (CPU; tools/numeric_range_margin.py) -------------------
def oracle_fit_ratios(name, sweep, dtype=F32):
    """Per model: (label, value, ratios) of oracle.fit in `dtype` against the float64 reference."""
    out = []
    for launch, rows in sweep_reference(name, sweep):
        for mdl, T in rows:
            out.append((mdl["label"], mdl.get("value"), ratios(reference(launch, mdl, dtype), T)))
    return out


def oracle_fit_bf16_ratios(name, sweep):
    """oracle.fit_bf16 (float32 Adam on the bfloat16 step) against the bounds of the mixed-precision sweeps."""
    out = []
    for launch, rows in sweep_reference(name, sweep):
        lr, b1, b2, eps = _hyper(*launch["cfg"])
        for mdl, T in rows:
            p = [a.astype(F32) for a in mdl["p"]]
            th0 = _cat(p)
            st = O.AdamState(p)
            st.t = mdl.get("t0", 0)
            for a, b in zip(st.m, st.v):
                a += F32(mdl.get("m0", 0.0))
                b += F32(mdl.get("v0", 0.0))
            with np.errstate(over="ignore", under="ignore"):
                h = O.fit_bf16(p, launch["acts"], st, mdl["row"][None], np.array([mdl["z"]]), np.zeros((1, 1), dtype=np.int64),
                               lr=lr, beta1=b1, beta2=b2, eps=eps)
            out.append((mdl["label"], mdl.get("value"),
                        ratios(dict(m=_cat(st.m), v=_cat(st.v), upd=_cat(p) - th0, loss=h[0]), T)))
    return out


def measure_adam_f32_ratio():
    """Worst error of the float32 oracle's update against the float64 one, in units of adam_tolerances' operation
    count, per (t0, betas, lr) group of the Adam table, on the one-layer probe network (the update's arithmetic does not
    depend on the network)."""
    D, units = 17, [1]
    out = {}
    for cfg in ADAM_CFGS:
        launch = dict(acts=["linear"], cfg=cfg, f32_ratio=0.0)
        for t0 in ADAM_T0:
            w = 0.0
            for m0, v0 in ADAM_SLOTS:
                for sign in (1, -1):
                    p, row = adam_model(D, units, ADAM_G, sign)
                    mdl = dict(p=p, row=row, z=float(sign < 0), m0=m0, v0=v0, t0=t0)
                    w = max(w, ratios(reference(launch, mdl, F32), tolerances(launch, mdl))["upd"])
            out[adam_key(t0, *cfg)] = w
    return out


# ---- 3. the IEEE-form kernels: forward, evaluate, value + input gradient, screening, a flat restart ------------------------
# name: (D, units, environment); every hidden and output activation is free except where noted
ACQ_FLAVOURS = {
    "static 2 6-32-32-1": (6, [32, 32, 1], {}),
    "static 3 16-64-64-64-1": (16, [64, 64, 64, 1], {}),
    "static 4 32-128-128-1": (32, [128, 128, 1], {}),
    "static 5 16-32-32-32-1": (16, [32, 32, 32, 1], {}),
    "generic -1 17-1": (17, [1], {}),
    "generic -2 5-1-1": (5, [1, 1], {}),
    "generic -3 5-7-3-1": (5, [7, 3, 1], {}),
    "generic -4 9-17-16-15-1": (9, [17, 16, 15, 1], {}),
    "generic 0 3-16x4-1": (3, [16, 16, 16, 16, 1], {}),
    "streamed forced 5-7-3-1": (5, [7, 3, 1], {"BORE_STREAM": "1"}),
    "streamed native 8-250-130-1": (8, [250, 130, 1], {}),
}
STATIC1 = (2, [16, 16, 1], ["relu", "relu", "sigmoid"])      # static shape 1 fixes its activations: its own cases below
VG_U = [_f(s * u) for u in (17, 40, 88, 104) for s in (1, -1)]
EXP_OVERFLOW = [89.0, 104.0, 1000.0]                          # expf(u) = +inf in float32 (from 88.73 on)
EVAL_MIX = [(x, z) for x in LOGITS for z in (0.0, 1.0)][:65]


def _finite32(x):
    """Which float64 values are finite as float32."""
    with np.errstate(over="ignore"):
        return np.isfinite(np.asarray(x).astype(F32))


def _ratio(got, ref, tol):
    diff = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, diff / tol)
    return float(np.max(r)) if r.size else 0.0


def forward_cases(D, units, fixed=None):
    """-> [(acts, [model], ref, tol)]: the logit sweep under every output activation, the hidden sweep under every
    hidden activation in every layer (output linear, reading w_out * act(a))."""
    n, cases = len(units), []
    for out in ([fixed[-1]] if fixed else HIDDEN_ACTS):
        acts = _acts(n, "relu", out)
        models = [dict(zip(("p", "row"), logit_model(D, units, x, i)), label="%s(%r)" % (out, x)) for i, x in enumerate(LOGITS)]
        x = np.array(LOGITS)
        ref = O._act(out, x)
        cases.append((acts, models, ref, act_tolerance(out, x, ref, False)))
    if fixed:
        return cases
    w_out = 2.0 ** -10
    for layer in range(1, n):
        for act in HIDDEN_ACTS:
            values = HIDDEN + (RELU_KINK if act == "relu" else [])
            acts = _acts(n, "linear", "linear")
            acts[layer - 1] = act
            models = [dict(zip(("p", "row"), hidden_model(D, units, layer, values, i, w_out)),
                           label="layer %d %s(%r)" % (layer, act, a)) for i, a in enumerate(values)]
            a = np.array(values)
            h = O._act(act, a)
            ref = w_out * h
            cases.append((acts, models, ref, w_out * act_tolerance(act, a, h, False) + _floor(ref, DENORM)))
    return cases


def forward_reference(acts, models, dtype=np.float64):
    return np.array([O.predict(m["p"], acts, m["row"][None], dtype=dtype)[0, 0] for m in models])


def evaluate_cases(D, units, out):
    """-> (acts, one-row models [(model, loss_ref, tol, hit)], the 65-row mix (model, X, z, loss_ref, tol, hits))."""
    n = len(units)
    acts = _acts(n, "relu", out)
    single = []
    for i, (x, z) in enumerate((x, z) for x in LOGITS for z in (0.0, 1.0)):
        p, row = logit_model(D, units, x, i)
        G = grad_tolerances(p, acts, row, z, fit=False)
        o = float(O._sigmoid(np.float64(x))) if out == "sigmoid" else x
        single.append((dict(p=p, row=row, z=z, label="x=%r z=%d" % (x, z)), G["loss"], G["tloss"], float((o > 0.5) == (z > 0.5))))
    # the mix: linear hidden layers carry the input on, logit = x_r * 1
    p, row = logit_model(D, units, 1.0, 3)
    acts_mix = _acts(n, "linear", out)
    X = np.outer([x for x, _ in EVAL_MIX], row)
    z = np.array([zz for _, zz in EVAL_MIX])
    G = [grad_tolerances(p, acts_mix, X[r], z[r], fit=False) for r in range(len(z))]
    N = len(z)
    losses = np.array([g["loss"] for g in G])
    # a float32 sum of N terms in any order: at most N - 1 roundings of partial sums no larger than the total of the
    # magnitudes; then the division by N
    tol = (sum(g["tloss"] for g in G) + (N - 1) * RND * np.abs(losses).sum()) / N + RND * abs(losses.mean())
    o = O._sigmoid(X @ row) if out == "sigmoid" else X @ row
    hits = int(((o > 0.5) == (z > 0.5)).sum())
    return acts, single, (dict(p=p), acts_mix, X, z, float(losses.mean()), float(tol), hits)


HALF = _nb(0.5)


TRANSFORM_CASES = [(tr, neg) for tr in ("identity", "sigmoid", "exp") for neg in (True, False)]


def value_grad_case(D, units, transform, negate, us=VG_U):
    """One model (ones through linear layers: f = x_j), one row per u = +-f.  -> (p, acts, X, value ref / tol, grad ref / tol)."""
    n = len(units)
    acts = _acts(n, "linear", "linear")
    p, row = logit_model(D, units, 1.0, 2)
    sign = -1.0 if negate else 1.0
    X = np.outer([sign * u for u in us], row)
    q = [a.copy() for a in p]
    if not negate:          # T(f) = T(-(-f)): the oracle's T(-f) on the network with its output negated
        q[-2], q[-1] = -q[-2], -q[-1]
    with np.errstate(over="ignore", invalid="ignore"):
        rv, rg = O.value_and_input_grad(q, acts, X, transform, dtype=np.float64)
    u = np.array(us)
    if transform == "identity":
        tv, tg = np.zeros_like(rv), np.zeros_like(rv)
    elif transform == "sigmoid":
        tv = act_tolerance("sigmoid", u, rv, False)
        tg = act_grad_tolerance("sigmoid", rv, tv)
    else:
        tv = K_EXP * RND * np.abs(rv) + _floor(rv, DENORM)
        tg = tv
    with np.errstate(invalid="ignore"):             # (inf * 0 in the rows beyond expf's range, which are not compared)
        tg = np.outer(tg, row) + _floor(rg, DENORM)
    return p, acts, X, rv, tv, rg, tg


SCREEN_FLAVOURS = ["static 2 6-32-32-1", "static 3 16-64-64-64-1", "generic -3 5-7-3-1", "generic 0 3-16x4-1",
                   "streamed native 8-250-130-1", "bf16 static 3 16-64-64-64-1", "bf16 static 4 32-128-128-1"]


def _acq(name):
    """(D, units, environment, compute) of an acquisition flavour; the bfloat16 ones are the wide static shapes."""
    if name in BF16_FIT:
        return BF16_FIT[name][0], BF16_FIT[name][1], {}, "bfloat16"
    return ACQ_FLAVOURS[name] + ("float32",)


def constant_model(D, units, b_out):
    """Ones from every input through linear layers into a sigmoid head whose bias saturates it: exactly 1.0 or 0.0."""
    p, _ = logit_model(D, units, 1.0, 0)
    p[-1][0] = b_out
    return p, _acts(len(units), "linear", "sigmoid")


def flat_model(D, units):
    """f = x_j - 40 through linear layers: u = -f >= 39 on the unit box, sigmoid(u) = 1 and dT = 0 exactly."""
    p, row = logit_model(D, units, 1.0, 1)
    p[-1][0] = -40.0
    return p, _acts(len(units), "linear", "linear")


# ---- the float32 oracle in the kernel's place, and wrong formulas on the oracle's side (CPU) ------------------------------
def preactivations(p, acts, row, dtype):
    """The pre-activation vectors of every layer, computed in `dtype`."""
    h, out = np.asarray(row, dtype=dtype), []
    for l, act in enumerate(acts):
        pre = h @ p[2 * l].astype(dtype) + p[2 * l + 1].astype(dtype)
        out.append(pre)
        h = O._act(act, pre)
    return out


@contextlib.contextmanager
def _patched(**attrs):
    old = {k: getattr(O, k) for k in attrs}
    try:
        for k, v in attrs.items():
            setattr(O, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(O, k, v)


def _worst(rows, keys=("m", "v", "upd", "loss")):
    return max(max(r[k] for k in keys) for _, _, r in rows)


def _fit_elu_f32(a, seam_shift=0):
    """mlp_math.h's fit_elu in numpy float32; seam_shift = 1 moves the series' range one float past -1/32."""
    a = np.asarray(a, dtype=F32)
    xn = np.minimum(a, F32(0))
    big = np.exp2(xn * F32(1.442695040888963)).astype(F32) - F32(1)
    ser = xn * (xn * (xn * (xn * F32(1 / 24) + F32(1 / 6)) + F32(0.5)) + F32(1))
    seam = F32(SEAM_ELU) if not seam_shift else np.nextafter(np.nextafter(F32(SEAM_ELU), F32(-1)), F32(-1))
    return np.where(a > 0, a, np.where(xn > seam, ser, big)).astype(F32)


SENSITIVITY_NET = "generic -3 5-7-3-1"


def sensitivity():
    """Five wrong formulas in the float32 oracle, each through the comparison that should notice: the worst ratio."""
    out = {}
    name = SENSITIVITY_NET
    act0 = O._act
    refs = {sweep: sweep_reference(name, sweep) for sweep in ("logit", "hidden", "adam")}     # (before anything is patched)

    def only(sweep, keep, sel=slice(None)):
        rows = []
        for launch, ms in refs[sweep]:
            for mdl, T in ms:
                if keep(launch, mdl):
                    rows.append((mdl["label"], mdl.get("value"), ratios(reference(launch, mdl, F32), T, sel)))
        return rows
    near0 = lambda launch, mdl: "elu" in launch["acts"] and -1e-2 < mdl["value"] < 0
    # 1. expm1 replaced by exp(x) - 1 near 0
    bad = lambda n, a: np.where(a > 0, a, np.exp(np.minimum(a, a.dtype.type(0))) - a.dtype.type(1)) if n == "elu" else act0(n, a)
    with _patched(_act=bad):
        out["expm1 as exp(x) - 1 near 0"] = _worst(only("hidden", near0))
    # 2. the fit's elu with the series applied one float past the seam, at the seam's lower neighbour (the kernel's own
    # formula in float32; as written it keeps within the bound, seam_shift = 0)
    seam = lambda launch, mdl: "elu" in launch["acts"] and mdl["value"] == _nb(SEAM_ELU)[0]
    for shift, key in ((0, "fit_elu as written, at the seam"), (1, "elu series one float past the seam")):
        with _patched(_act=lambda n, a, s=shift: _fit_elu_f32(a, s).astype(a.dtype) if n == "elu" else act0(n, a)):
            out[key] = _worst(only("hidden", seam), keys=("m",))
    # 3. e^-x flushed below 2^-100 instead of 2^-126
    def flushed(a):
        e = np.exp(-np.abs(a))
        return np.where(e < a.dtype.type(2.0 ** -100), a.dtype.type(0), e)
    sig = lambda a: np.where(a >= 0, 1 / (1 + flushed(a)), flushed(a) / (1 + flushed(a))).astype(a.dtype)
    bce = lambda a, z: np.maximum(a, a.dtype.type(0)) - a * z + np.log1p(flushed(a))
    with _patched(_sigmoid=sig, bce_with_logits=bce):
        out["exp flushed at 2^-100"] = _worst(only("logit", lambda launch, mdl: abs(mdl["value"]) == 87.0))

    # 4. Adam's eps inside the square root
    def step_eps_inside(params, grads, st, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7):
        dt = params[0].dtype.type
        st.t += 1
        alpha = O.adam_alpha(st.t, lr, beta1, beta2, params[0].dtype)
        for p, g, m, v in zip(params, grads, st.m, st.v):
            m += (g - m) * (dt(1) - dt(beta1))
            v += (g * g - v) * (dt(1) - dt(beta2))
            p -= (m * alpha) / np.sqrt(v + dt(eps))
    with _patched(adam_step=step_eps_inside):
        out["eps inside the square root"] = _worst(only("adam", lambda launch, mdl: mdl["t0"] == 999), keys=("upd",))

    # 5. 1 - beta^t in float32 from a float32 running product
    @functools.lru_cache(maxsize=None)
    def running(beta, t):
        b = F32(1)
        for _ in range(t):
            b = F32(b * F32(beta))
        return b

    def alpha_running(t, lr, beta1, beta2, dtype=np.float32):
        dt = np.dtype(dtype).type
        return dt(dt(lr) * np.sqrt(dt(1) - dt(running(float(beta2), t))) / (dt(1) - dt(running(float(beta1), t))))
    # read on the output kernel alone (theta = 0 there, so the update is not hidden behind the rounding of a large
    # theta'; its gradients are the table's +-g) at t0 = 999, where beta2^t = 0.37 and a thousand float32 products have
    # rounded; the same selection without the swap is recorded beside it
    D, units = FIT_FLAVOURS[name][0], FIT_FLAVOURS[name][1]
    P = sum(a.size for a in _zeros(D, units))
    out_kernel = slice(P - 1 - units[-2], P - 1)
    pick = lambda launch, mdl: mdl["t0"] == 999 and launch["cfg"][1] == 0.9
    out["output kernel at t0 = 999, no swap"] = _worst(only("adam", pick, out_kernel), keys=("upd",))
    with _patched(adam_alpha=alpha_running):
        out["beta^t as a float32 running product"] = _worst(only("adam", pick, out_kernel), keys=("upd",))
    return out


def oracle_margins(adam_ratio=None):
    """Every comparison above with the float32 oracle standing in for the kernel: the worst ratio per sweep and flavour
    (kept only while at most 0.5; nothing had to be dropped), and the sensitivity factors.  "value_grad exp" is the one
    comparison whose stand-in cannot keep to one half: its bound is expf's one ulp, and numpy's float32 exp is a one-ulp
    function itself (0.96 of the bound at u = 17)."""
    out = {"adam_f32_ratio": adam_ratio or measure_adam_f32_ratio(), "dropped": [], "fit_logit": {}, "fit_hidden": {},
           "fit_adam": {}, "forward": {}, "evaluate": {}, "value_grad": {}, "value_grad exp": {}}
    for name, (D, units, _, _, _) in FIT_FLAVOURS.items():
        for sweep in ("logit", "hidden", "adam"):
            rows = oracle_fit_ratios(name, sweep)
            if rows:
                out["fit_" + sweep][name] = _worst(rows)
    out["fit_bf16"] = {"%s %s" % (name, sweep): _worst(oracle_fit_bf16_ratios(name, sweep))
                       for name in BF16_FIT for sweep in ("logit", "hidden", "adam")}
    acq = dict(ACQ_FLAVOURS, **{"static 1 2-16-16-1": (STATIC1[0], STATIC1[1], {})})
    for name, (D, units, _) in acq.items():
        fixed = STATIC1[2] if name.startswith("static 1") else None
        out["forward"][name] = max(_ratio(forward_reference(acts, models, F32), ref, tol)
                                   for acts, models, ref, tol in forward_cases(D, units, fixed))
        w = 0.0
        for o in (("sigmoid",) if fixed else ("linear", "sigmoid")):
            acts, single, (mix, acts_mix, X, z, mix_ref, mix_tol, _) = evaluate_cases(D, units, o)
            for m, ref, tol, _ in single:
                w = max(w, _ratio(O.evaluate(m["p"], acts, m["row"][None], np.array([m["z"]]))[0], ref, tol))
            w = max(w, _ratio(O.evaluate(mix["p"], acts_mix, X, z)[0], mix_ref, mix_tol))
        out["evaluate"][name] = w
        if fixed:
            continue
        w = {"value_grad": 0.0, "value_grad exp": 0.0}
        for tr, neg in TRANSFORM_CASES:
            p, acts, X, rv, tv, rg, tg = value_grad_case(D, units, tr, neg)
            q = [a.copy() for a in p]
            if not neg:
                q[-2], q[-1] = -q[-2], -q[-1]
            with np.errstate(over="ignore", invalid="ignore"):
                v, g = O.value_and_input_grad(q, acts, X, tr)
            fin = _finite32(rv)
            assert np.array_equal(np.isposinf(v), ~fin)
            k = "value_grad exp" if tr == "exp" else "value_grad"
            w[k] = max(w[k], _ratio(v[fin], rv[fin], tv[fin]), _ratio(g[fin], rg[fin], tg[fin]))
        for k in w:
            out[k][name] = w[k]
    out["sensitivity"] = sensitivity()
    return out


# ---- 4. the LSTM kernels with saturated gates -------------------------------------------------------------------------------
# bore_lstm.hip has its own actf and its gates saturate in ordinary use.  Gate biases of +-20 in every sign combination
# over the units (input, forget, output), a positive candidate bias where input and forget are both open: those cells
# grow every step and pass |c| = 10 within T = 16 (asserted on the oracle).  Tolerances: the LSTM suite's, widened by
# its rule -- max(1, 8 x the float32 oracle's deviation in units of the tolerance), computed here from the inputs alone.
# key: (D, H, L, activation, seed, candidate bias).  (2->2x32 with elu, the plugin's activation, is left out on purpose: its
# unbounded cells feed back through the recurrent kernels, and with any biases tried (candidate 0.7 .. 3, recurrent
# kernels down to a quarter) the float32 ORACLE leaves the suite's theta tolerance 4- to 48-fold after one Adam step --
# the rule would widen the bound until it holds nothing.  tanh at the plugin's widths; elu at H = 7 with a candidate
# bias of 0.7, where the float32 oracle stays within 0.04 of every tolerance and the factor is 1 throughout.)
LSTM_NETS = {"2->2x32 tanh": (2, 32, 2, "tanh", 11, 3.0), "5->2x7 elu": (5, 7, 2, "elu", 12, 0.7)}
LSTM_T, LSTM_N = 16, 33


@functools.lru_cache(maxsize=None)
def lstm_case(key):
    import lstm_oracle as LO
    from test_gpu_lstm import _hyperband_sequences
    from test_gpu_lstm_shapes import MV, _weights
    D, H, L, act, seed, g_bias = LSTM_NETS[key]
    rs = np.random.RandomState(seed)
    p = _weights(D, H, L, rs)
    u = np.arange(H)
    s = lambda k: np.where((u // k) % 2 == 0, 1.0, -1.0)
    for l in range(L):
        b = p[3 * l + 2]
        b[0:H], b[H:2 * H], b[3 * H:4 * H] = 20 * s(1), 20 * s(2), 20 * s(4)
        b[2 * H:3 * H][(s(1) > 0) & (s(2) > 0)] = g_bias
    X, Y = _hyperband_sequences(rs, LSTM_N, LSTM_T, D, MV)
    X32 = X.astype(F32)
    _, (C, _) = LO.forward(p, act, X32, MV, cache=True)
    gates = np.concatenate([np.concatenate([C[l][t][g].ravel() for g in "ifo"]) for l in range(L) for t in range(LSTM_T)])
    assert max(float(np.abs(C[l][LSTM_T - 1]["c"]).max()) for l in range(L)) >= 10          # the cell state reaches |c| >= 10
    assert (gates < 1e-8).any() and (gates > 1 - 1e-8).any()                               # gates saturated on both sides
    x = rs.uniform(size=(9, D))
    return p, act, X32, Y, x


__all__ = [_n for _n in dir() if not _n.startswith("__")]
