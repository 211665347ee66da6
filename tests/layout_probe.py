"""Integer-network probes for the two wide static shapes (16->64-64-64-1 and 32->128-128-1): everything
tests/test_layout_probe_host.py and tests/test_gpu_layout_probe.py share, with no device in it.

The idea.  With small integer weights, biases and inputs every product is an integer and every partial sum of a layer
stays below 2^24, so a float32 sum gives the same value in ANY order, and the bfloat16 rounding of that value is
deterministic: a kernel has to equal the oracle bit for bit, whatever its tiling, fragment order or reduction tree.
What a difference then means is a misplaced element or a wrong rounding mode, never noise.  The roundings are real
(layer outputs reach 2^16; a few input columns hold 9-bit integers, every odd one of which is an exact bfloat16 tie).

Contents: the generator (`make_net`, `make_inputs`), the references (the oracle per compute mode, a restatement with a
free choice of the matrix product for the order-free premise, the float32 Adam slots, AdamClock's step size, the theta
reference with its derived bound) and the mutation table."""
import contextlib
import functools

import numpy as np

from numeric_range import EPS, F32, _hyper, _ulp32, adam_tolerances, pack  # noqa: F401  (pack: for the device file)
from oracle import bore_oracle as O

# name: (D, units, density of each kernel matrix)
SHAPES = {
    "16-64-64-64-1": (16, [64, 64, 64, 1], (0.5, 0.25, 0.25, 1.0)),
    "32-128-128-1": (32, [128, 128, 1], (0.5, 0.2, 1.0)),
}
COMPUTES = ("bfloat16", "float32")
WEIGHT_VALUES = (-2, -1, 1, 2, 3)
FIT_BIAS = 128             # the output bias: every logit >= 128, sigmoid exactly 1.0f and e^-logit exactly 0 (see make_net)
PROBE_ROWS = 133           # the canonical rows: every host premise and every device comparison uses a prefix of them
ROWS = (1, 15, 16, 17, 63, 64, 65, 133)
VARIANTS = (False, True)   # relu hidden layers; the first hidden layer linear
N_MODELS = 3               # models per launch, each with its own network and data
LIMIT = 2.0 ** 24
ADAM = (1e-3, 0.9, 0.999)  # lr, beta1, beta2 of every probe fit (eps = numeric_range.EPS)


def tie_columns(D):
    """The input columns that hold 9-bit integers in every thirty-second row."""
    return (1, D - 3)


def make_inputs(name, seed, n=PROBE_ROWS):
    """(n, D) float64 integers in [0, 3]; every thirty-second row holds an odd integer in [257, 511] in one of the tie
    columns: an exact tie between two bfloat16 values, down (e.g. 257 -> 256) or up (259 -> 260).  Row 0 holds one of
    each, so that a single-row launch rounds both ways too.  (Few rows, and few first-layer weights on those columns --
    make_net --, so that the sum of a data set's logits stays below 2^24 and the loss probes are order-free as well.)  Row 1 is all zero and rows 2 .. 31 keep a growing
    share of their entries, up to 0.4: their activations are small enough for every rounding to be exact, so a bias or a single weight that is
    off shows there even in the deep layers, where the other rows' outputs are rounded to multiples of 2^10."""
    D = SHAPES[name][0]
    rs = np.random.RandomState(1000 + seed)
    X = rs.randint(0, 4, size=(n, D)).astype(np.float64)
    cols = tie_columns(D)
    for r in range(0, n, 32):
        X[r, cols[(r // 32) % 2]] = 2 * rs.randint(128, 256) + 1
    X[0, cols[0]], X[0, cols[1]] = 257.0, 259.0
    X[1:32] *= rs.uniform(size=X[1:32].shape) < np.linspace(0.0, 0.4, 31)[:n - 1, None]
    return X


def make_net(name, seed, linear=False):
    """-> dict(p=[float32 W1 (in, out), b1, ...], acts, name, seed).  Kernel matrices from WEIGHT_VALUES masked to
    the layer's density, biases in [-3, 3], hidden activations relu (`linear`: the first hidden layer is linear), output
    linear.  A relu unit that none of the canonical rows of this seed switches on would hide its row of the next
    kernel matrix from every probe: its column and bias are negated (if it has no weight at all, its bias becomes 1).
    Every network is the FIT VARIANT: the output matrix is non-negative and without zeros (a hidden unit with output
    weight 0 would be invisible to every probe) and the output bias is FIT_BIAS, so that every logit is >= 128.  Then
    e^-logit is 0 in float32 (it is below 2^-149 from 104 on), sigmoid is exactly 1.0f in the IEEE form and in the fit's
    (`fit_bce`: 1 + ex is 1, rcp(1) is 1), a label-1 row has loss 0 and gradient 0, and a label-0 row has loss = logit and
    d loss / d logit = 1, all exactly.  The forward, input-gradient and screening probes use the same networks: the
    sharpness premise (tests/test_layout_probe_host.py) needs all three probes on a network."""
    D, units, density = SHAPES[name]
    rs = np.random.RandomState(seed)
    acts = ["relu"] * (len(units) - 1) + ["linear"]
    if linear:
        acts[0] = "linear"
    h = O.bf16_round(make_inputs(name, seed).astype(F32)).astype(np.float64)
    p, k = [], D
    for l, (u, dens) in enumerate(zip(units, density)):
        mask = rs.uniform(size=(k, u)) < dens
        if l == 0:          # (the 9-bit inputs reach few units)
            mask[list(tie_columns(D))] &= rs.uniform(size=(2, u)) < 0.3
        W = rs.choice(WEIGHT_VALUES, size=(k, u)) * mask
        b = rs.randint(-3, 4, size=u)
        W, b = W.astype(np.float64), b.astype(np.float64)
        if l == len(units) - 1:
            W, b = np.abs(W), np.full(u, float(FIT_BIAS))
        if acts[l] == "relu":
            pre = h @ W + b
            dead = ~(pre > 0).any(axis=0)
            W[:, dead], b[dead] = -W[:, dead], -b[dead]
            b[dead & ~((h @ W + b) > 0).any(axis=0)] = 1.0
        h = O.bf16_round(O._act(acts[l], h @ W + b).astype(F32)).astype(np.float64)
        p += [W.astype(F32), b.astype(F32)]
        k = u
    return dict(p=p, acts=acts, name=name, seed=seed)


@functools.lru_cache(maxsize=None)
def networks(name, linear=False):
    """The N_MODELS networks of one launch (one descriptor: the same activations) with their canonical inputs:
    [(net, X)], built once.  `linear`: the variant whose first hidden layer is linear."""
    base = (7 if name.startswith("16") else 57) + (20 if linear else 0)
    return [(make_net(name, base + i, linear=linear), make_inputs(name, base + i)) for i in range(N_MODELS)]


def all_networks():
    """Every (shape name, linear variant, model index, net, X) the device file uses."""
    return [(name, linear, i, net, X) for name in SHAPES for linear in VARIANTS
            for i, (net, X) in enumerate(networks(name, linear))]


def labels(seed, n):
    """Mixed labels, a quarter of them 0 (the rows whose logits the loss sums: few enough for the sum to stay below
    2^24), both classes present from two rows on."""
    z = (np.random.RandomState(2000 + seed).uniform(size=n) >= 0.25).astype(np.float64)
    if n > 1:
        z[0], z[1] = 0.0, 1.0
    return z


def rows_of(X, n):
    """The first n of the canonical rows, repeated cyclically beyond them."""
    return np.resize(X, (n, X.shape[1])) if n > len(X) else X[:n]


BATCH = 64
# F2: (N, the live batch) -- 64 rows alone, first and in the middle; last batches of 8, 32 and 1 rows (powers of two)
LIVE = [(64, 0), (200, 0), (200, 1), (200, 3), (160, 2), (129, 2)]
EVAL_N = (1, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def live_case(name, linear, N, live):
    """Per model of the launch: dict(X (N, D), z (N,), perm (N,) int32, rows: the live batch's row indices).  Every row
    has label 1 but the live batch's, whose labels are mixed (one row: label 0)."""
    rs = np.random.RandomState(31 * N + live)
    out = []
    for net, X in networks(name, linear):
        perm = rs.permutation(N).astype(np.int32)
        rows = perm[live * BATCH:(live + 1) * BATCH]
        assert len(rows) & (len(rows) - 1) == 0, "1 / rows must be exact"
        z = np.ones(N)
        z[rows] = labels(net["seed"] + N, len(rows)) if len(rows) > 1 else 0.0
        out.append(dict(X=rows_of(X, N), z=z, perm=perm, rows=rows))
    return out


@functools.lru_cache(maxsize=None)
def eval_case(name, N):
    """Per model: (X (N, D), z (N,)) of the evaluate probe."""
    return [(rows_of(X, N), labels(net["seed"] + N, N)) for net, X in networks(name)]


# ---- references: the oracle per compute mode ---------------------------------------------------------------------------
def _p64(net):
    return [a.astype(np.float64) for a in net["p"]]


def ref_forward(net, X, compute):
    """Model output of the rows X, (n,): bfloat16 -> oracle.forward_bf16; float32 -> oracle.predict in float64 (no
    rounding happens anywhere, so the float64 result IS the float32 result)."""
    if compute == "bfloat16":
        return O.forward_bf16(net["p"], net["acts"], X)[:, 0]
    return O.predict(net["p"], net["acts"], X, dtype=np.float64)[:, 0]


def ref_value_grad(net, X, compute, negate):
    """[T(+-f(x)), gradient] under the identity transform."""
    if compute == "bfloat16":
        return O.value_and_input_grad_bf16(net["p"], net["acts"], X, "identity", negate)
    q = _p64(net)
    if not negate:          # T(f) = T(-(-f)): the oracle's T(-f) on the network with its output negated
        q[-2], q[-1] = -q[-2], -q[-1]
    v, g = O.value_and_input_grad(q, net["acts"], X, "identity", dtype=np.float64)
    return v, g


def ref_fit_grads(net, Xb, zb, compute):
    """-> (logits (nb,), gradients) of one batch: oracle.loss_and_grads_bf16, or oracle.loss_and_grads in float64."""
    if compute == "bfloat16":
        _, g = O.loss_and_grads_bf16(net["p"], net["acts"], Xb.astype(F32), zb.astype(F32))
        return O.forward_bf16(net["p"], net["acts"], Xb)[:, 0], g
    _, g = O.loss_and_grads(_p64(net), net["acts"], Xb.astype(np.float64), zb.astype(np.float64))
    return O.predict(net["p"], net["acts"], Xb, dtype=np.float64)[:, 0], g


def loss_sum(logits, z):
    """Sum of the rows' loss terms where e^-logit is 0 in float32: the logit for label 0, 0 for label 1
    (max(x, 0) - x z + log1p(0))."""
    logits = np.asarray(logits, dtype=np.float64)
    assert (logits >= FIT_BIAS).all() and np.array_equal(np.round(logits), logits)
    assert np.sum(np.where(np.asarray(z) > 0.5, 0.0, logits)) < LIMIT, "the loss sum would depend on its order"
    return float(np.sum(np.where(np.asarray(z) > 0.5, 0.0, np.asarray(logits, dtype=np.float64))))


def mean_of(total, n):
    """-> (total / n exactly, half a float32 ulp of it: what ONE rounding allows -- the kernels divide the exact float32
    sum by (float) n, IEEE)."""
    assert float(F32(total)) == total
    return float(total) / n, 0.5 * float(_ulp32(float(total) / n))


# ---- the restatement with a free matrix product (the order-free premise) ------------------------------------------------
class Exact:
    """float64 products that also record the largest sum of magnitudes, in units of `unit` (1 for integers, 1 / rows for
    the fit's backward pass), and that every result is a multiple of the unit."""
    dtype = np.float64

    def __init__(self):
        self.worst, self.unit = 0.0, 1.0

    def __call__(self, A, B):
        out = A @ B
        self.worst = max(self.worst, float((np.abs(A) @ np.abs(B)).max()) / self.unit)
        assert np.array_equal(np.round(out / self.unit), out / self.unit), "a value is not a multiple of the unit"
        return out


class Shuffled:
    """float32 products that add the k terms one at a time in a shuffled order."""
    dtype = F32
    unit = 1.0

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)

    def __call__(self, A, B):
        acc = np.zeros((A.shape[0], B.shape[1]), dtype=F32)
        for k in self.rs.permutation(A.shape[1]):
            acc += A[:, k, None] * B[None, k, :]
        return acc


def _rnd(a, bf16):
    """Round to bfloat16 (the values are exact in float32 by the premise under test)."""
    if not bf16:
        return a
    a32 = a.astype(F32)
    assert np.array_equal(a32.astype(np.float64), a.astype(np.float64))
    return O.bf16_round(a32).astype(a.dtype)


def restate(net, X, mm, compute, z=None, negate=True):
    """The three probed quantities with the matrix product `mm`: dict(out (n,), grad (n, D), g [fit gradients] when `z`
    is given).  The rounding points are the oracle's: weights, biases, inputs, every layer output and every delta but
    the input gradient itself."""
    bf, dt = compute == "bfloat16", mm.dtype
    p, acts = net["p"], net["acts"]
    n = len(acts)
    W = [_rnd(p[2 * l].astype(dt), bf) for l in range(n)]
    b = [_rnd(p[2 * l + 1].astype(dt), bf) for l in range(n)]
    mm.unit = 1.0
    hs = [_rnd(np.asarray(X).astype(dt), bf)]
    for l in range(n):
        hs.append(_rnd(O._act(acts[l], mm(hs[-1], W[l]) + b[l]), bf))
    out = dict(out=hs[-1][:, 0])
    rows = len(hs[0])
    delta = np.full((rows, 1), -1.0 if negate else 1.0, dtype=dt)
    for l in range(n - 1, -1, -1):
        back = mm(delta, W[l].T)
        delta = back if l == 0 else _rnd(back * O._act_grad_from_output(acts[l - 1], hs[l]), bf)
    out["grad"] = delta
    if z is not None:
        mm.unit = 1.0 / rows
        assert rows & (rows - 1) == 0, "1 / rows must be exact"
        delta = _rnd((O._sigmoid(hs[-1]) - np.asarray(z).reshape(rows, 1).astype(dt)) / dt(rows), bf)
        g = [None] * (2 * n)
        for l in range(n - 1, -1, -1):
            g[2 * l] = mm(hs[l].T, delta)
            g[2 * l + 1] = mm(np.ones((1, rows), dtype=dt), delta)[0]
            if l > 0:
                delta = _rnd(mm(delta, W[l].T) * O._act_grad_from_output(acts[l - 1], hs[l]), bf)
        out["g"] = g
    return out


def oracle_probes(net, X, compute, z=None, negate=True):
    """The same dict from the oracle functions the device is compared with."""
    v, grad = ref_value_grad(net, X, compute, negate)
    out = dict(out=ref_forward(net, X, compute), grad=grad, val=v)
    if z is not None:
        out["g"] = ref_fit_grads(net, X, z, compute)[1]
    return out


def rounded_share(net, X):
    """Per layer, the share of outputs that bfloat16 really rounds (forward, bfloat16 arithmetic)."""
    hs = O.forward_bf16(net["p"], net["acts"], X, return_all=True)
    out = []
    for l, act in enumerate(net["acts"]):
        pre = O._act(act, hs[l] @ O.bf16_round(net["p"][2 * l]) + O.bf16_round(net["p"][2 * l + 1])).astype(F32)
        out.append(float(np.mean(O.bf16_round(pre) != pre)))
    return out


# ---- Adam: the float32 slots, AdamClock's step size, theta with its bound ---------------------------------------------------
def adam_clock(t0, steps, lr=ADAM[0], beta1=ADAM[1], beta2=ADAM[2]):
    """AdamClock (mlp_math.h) in numpy: the beta powers run in float64 from pow(beta, t0), are rounded to float32 at
    use, and lr sqrtf(1 - b2^t) / (1 - b1^t) is formed in float32.  -> the float32 step sizes of steps t0 + 1 ..."""
    lr, b1, b2 = F32(lr), F32(beta1), F32(beta2)
    b1p, b2p = np.power(np.float64(b1), np.float64(t0)), np.power(np.float64(b2), np.float64(t0))
    out = []
    for _ in range(steps):
        b1p, b2p = b1p * np.float64(b1), b2p * np.float64(b2)
        out.append(F32(F32(lr * np.sqrt(F32(1) - F32(b2p))) / F32(F32(1) - F32(b1p))))
    return out


def adam_slot_step(m, v, g, beta1=ADAM[1], beta2=ADAM[2]):
    """adam_update's slots, bit for bit: m += (g - m) * omb1, v += (g * g - v) * omb2 in float32 with omb = 1.f - beta
    formed from the float32 hyper-parameters.  In place on float32 arrays."""
    assert m.dtype == F32 and v.dtype == F32
    g = np.asarray(g, dtype=F32)
    omb1, omb2 = F32(1) - F32(beta1), F32(1) - F32(beta2)
    m += (g - m) * omb1
    v += (g * g - v) * omb2


def adam_trajectory(theta0, m0, v0, t0, grads, cfg=ADAM):
    """`len(grads)` Adam steps from packed float32 theta0 / m0 / v0 (t0 steps behind them); grads[k] is the packed EXACT
    gradient of step k, or None for a zero gradient.  -> dict(m, v: the float32 slots the device must hold bit for
    bit; theta, tol: the float64 weights and the bound on the device's).

    The bound is adam_tolerances' (tests/numeric_range.py), one step at a time and summed: each step starts from the
    exact float32 slots, so it carries the roundings of that step alone -- |update| x (the roundings of m', v', the
    product with alpha, sqrt, the add, rcp: 1 ulp each) x 2^-24, alpha's own bound, and the rounding of the new weight.
    No absolute term.  (Its factor for the float32 formula's own loss is 1: the float32 oracle stays within 0.2 of the
    count over the whole table, profiles/numeric_range/oracle_margin.json.)  A step whose slots and gradient are all
    zero leaves theta alone exactly (-(0 alpha) rcp(eps) = -0) and adds nothing to the bound."""
    lr, b1, b2, eps = _hyper(*cfg)
    m, v = np.array(m0, dtype=F32), np.array(v0, dtype=F32)
    theta = np.asarray(theta0, dtype=np.float64).copy()
    tol = np.zeros_like(theta)
    for k, g in enumerate(grads):
        g64 = np.zeros_like(theta) if g is None else np.asarray(g, dtype=np.float64)
        if g is not None:
            assert np.array_equal(g64.astype(F32).astype(np.float64), g64), "the gradient must be exact in float32"
        if g is not None or m.any() or v.any():
            with np.errstate(under="ignore"):
                A = adam_tolerances(g64, 0.0, theta, m.astype(np.float64), v.astype(np.float64), t0 + k, lr, b1, b2,
                                    eps, 0.0)
            theta = theta + A["upd"]
            tol = tol + A["tupd"]
        adam_slot_step(m, v, g64.astype(F32), cfg[1], cfg[2])
    return dict(m=m, v=v, theta=theta, tol=tol, t=t0 + len(grads))


def unique_slots(n_models, P):
    """F1's prepared slots: m0, v0 [n_models, P] float32, every element of a launch distinct, v0 > 0, m0 of both
    signs, all exact in float32 (multiples of 2^-16 and 2^-14 below 2^17 of them)."""
    i = np.arange(n_models * P, dtype=np.float64).reshape(n_models, P) + 1.0
    m0 = np.where(i % 2 == 0, 1.0, -1.0) * i * 2.0 ** -16
    v0 = i * 2.0 ** -14
    return m0.astype(F32), v0.astype(F32)


def worst_ratio(got, ref, tol):
    """Largest |got - ref| / tol (0 where they agree exactly; inf where they differ and nothing is allowed)."""
    diff = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, diff / tol)
    return float(np.max(r)) if r.size else 0.0


# ---- the mutation table: what a layout bug does to a parameter list -----------------------------------------------------------
def _copy(p):
    return [a.copy() for a in p]


def swap_rows(p, l, rs):
    """Two input units of layer l's kernel matrix change places."""
    q = _copy(p)
    i, j = rs.choice(q[2 * l].shape[0], size=2, replace=False)
    q[2 * l][[i, j]] = q[2 * l][[j, i]]
    return q


def swap_columns(p, l, rs):
    """Two output units of layer l's kernel matrix change places (the biases stay)."""
    q = _copy(p)
    if q[2 * l].shape[1] < 2:
        return None
    i, j = rs.choice(q[2 * l].shape[1], size=2, replace=False)
    q[2 * l][:, [i, j]] = q[2 * l][:, [j, i]]
    return q


def swap_biases(p, l, rs):
    q = _copy(p)
    if q[2 * l + 1].shape[0] < 2:
        return None
    i, j = rs.choice(q[2 * l + 1].shape[0], size=2, replace=False)
    q[2 * l + 1][[i, j]] = q[2 * l + 1][[j, i]]
    return q


def bump_element(p, l, rs):
    """One element of layer l's kernel matrix is off by one."""
    q = _copy(p)
    W = q[2 * l]
    W[rs.randint(W.shape[0]), rs.randint(W.shape[1])] += 1
    return q


MUTATIONS = {"row swap": swap_rows, "column swap": swap_columns, "bias swap": swap_biases, "element + 1": bump_element}
EVERY = ("row swap", "column swap", "bias swap")     # kinds every sample of which must be seen
ELEMENT_FLOOR = 0.9
SAMPLES = 120


def sample_mutation(kind, p, l, rs):
    """A mutation of `kind` in layer l that really changes the parameters (swapping two equal biases is no mutation);
    None where the layer has nothing to swap."""
    for _ in range(1000):
        q = MUTATIONS[kind](p, l, rs)
        if q is None:
            return None
        if any(not np.array_equal(a, b) for a, b in zip(p, q)):
            return q
    raise AssertionError("no effective %s in layer %d" % (kind, l))


@contextlib.contextmanager
def truncating():
    """oracle.bf16_round replaced by truncation: the wrong rounding mode."""
    old = O.bf16_round

    def trunc(x):
        u = np.ascontiguousarray(x, dtype=F32).view(np.uint32) & np.uint32(0xFFFF0000)
        return u.view(F32).reshape(np.shape(x))
    O.bf16_round = trunc
    try:
        yield
    finally:
        O.bf16_round = old


def probes_differ(a, b):
    """Which of two probe dicts' quantities differ."""
    out = []
    for k in a:
        same = all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) if k == "g" else np.array_equal(a[k], b[k])
        if not same:
            out.append(k)
    return out


def detects(net, X, z, q, base=None, compute="bfloat16"):
    """Is the mutated parameter list q seen by the forward, the input-gradient or the first-step fit-gradient probe (the
    first 64 rows as one batch)?  Forward first: the others run only where it is blind."""
    mut = dict(net, p=q)
    if not np.array_equal(ref_forward(net, X, compute) if base is None else base["out"], ref_forward(mut, X, compute)):
        return "out"
    if not np.array_equal(ref_value_grad(net, X, compute, True)[1] if base is None else base["grad"],
                          ref_value_grad(mut, X, compute, True)[1]):
        return "grad"
    g0 = ref_fit_grads(net, X[:64], z[:64], compute)[1] if base is None else base["g"]
    g1 = ref_fit_grads(mut, X[:64], z[:64], compute)[1]
    if any(not np.array_equal(a, b) for a, b in zip(g0, g1)):
        return "g"
    return None
