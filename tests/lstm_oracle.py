"""fp64 numpy oracle of the multi-fidelity classifier (StackedRecurrentFactory, bore/models.py:48-104).

TEST INFRASTRUCTURE ONLY, like oracle/bore_oracle.py (whose activation, BCE and Adam helpers it uses).
TensorFlow 2.5 (the reference's pin, setup.py:42) cannot run here, so its rules are restated:

  cell      Keras LSTMCell (implementation 2): z = x.W + h.U + b, gate order i, f, c, o;
            i, f, o = sigmoid (recurrent_activation, the TF 2.x default); c' = f c + i act(z_c);
            h' = o act(c')                                  [keras/layers/recurrent.py LSTMCell.call]
  masking   Masking(mask_value): step t is live iff any feature != mask_value; RNN over a mask keeps h
            and c on a masked step and outputs the previous output (zeros before the first live
            step)                                           [keras.backend.rnn, zero_output_for_mask=False]
  loss      BCE from logits per element, the mask as sample weight, SUM_OVER_BATCH_SIZE = the weighted
            sum divided by ALL n*T elements, plus l2 * sum(w^2) of W and b of every cell (never U) and
            of the head when regularised                    [losses_utils.compute_weighted_loss, TF 2.5]
  accuracy  binary_accuracy on the model output (the logit) at 0.5, weighted by the mask
  fit       one permutation of the sequences per epoch; logged loss = batch losses (before each update)
            averaged with batch-size weights; Keras Adam (oracle.bore_oracle.adam_step)

Every function takes ``dtype`` (default float64: the oracle).  With ``dtype=np.float32`` and float32 parameters the
same operations run in float32 throughout.  That run is no reference: it measures what float32 rounding alone costs
at a given depth, and the GPU tests derive the tolerances of the deep shapes from it (``as_dtype`` casts a parameter
list).
"""
import numpy as np

from oracle.bore_oracle import AdamState, _act, _act_grad_from_output, _sigmoid, _transform, adam_step, \
    bce_with_logits

__all__ = ["unpack", "pack", "as_dtype", "forward", "one_to_one", "loss_and_grads", "evaluate", "fit",
           "value_and_input_grad", "AdamState", "init_weights"]


def shapes(D, H, L):
    out = []
    for l in range(L):
        out += [((H if l else D), 4 * H), (H, 4 * H), (4 * H,)]
    return out + [(H, 1), (1,)]


def unpack(theta, D, H, L, dtype=np.float64):
    theta = np.asarray(theta, dtype=dtype).ravel()
    out, off = [], 0
    for s in shapes(D, H, L):
        n = int(np.prod(s))
        out.append(theta[off:off + n].reshape(s).copy())
        off += n
    assert off == theta.size
    return out


def pack(params):
    return np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in params])


def as_dtype(params, dtype):
    """A copy of the parameter list in ``dtype``."""
    return [np.array(p, dtype=dtype) for p in params]


def init_weights(D, H, L, rs):
    """Random weights with the Keras initialisers' scales (tests only need plausible values)."""
    ps = []
    for l in range(L):
        fan = H if l else D
        lim = np.sqrt(6.0 / (fan + 4 * H))
        ps.append(rs.uniform(-lim, lim, size=(fan, 4 * H)))
        ps.append(rs.uniform(-0.3, 0.3, size=(H, 4 * H)))
        b = rs.uniform(-0.1, 0.1, size=4 * H)
        b[H:2 * H] += 1.0
        ps.append(b)
    lim = np.sqrt(6.0 / (H + 1))
    ps.append(rs.uniform(-lim, lim, size=(H, 1)))
    ps.append(np.zeros(1))
    return ps


def _live(X, mask_value):
    if mask_value is None:
        return np.ones(X.shape[:2], dtype=bool)
    return np.any(X != mask_value, axis=-1)


def forward(params, act, X, mask_value=None, cache=False, dtype=np.float64):
    """Many-to-many: X [n, T, D] -> logits [n, T] (mask_value None: no Masking layer).  The cache keeps, per layer and
    step, the gates, the candidate's pre-activation ``zg`` and the cell state ``c`` before the mask is applied."""
    X = np.asarray(X, dtype=dtype)
    n, T, D = X.shape
    L = (len(params) - 2) // 3
    H = params[1].shape[0]
    live = _live(X, mask_value)
    h = [np.zeros((n, H), dtype=dtype) for _ in range(L)]
    c = [np.zeros((n, H), dtype=dtype) for _ in range(L)]
    logits = np.zeros((n, T), dtype=dtype)
    C = [[None] * T for _ in range(L)]
    Wo, bo = params[-2], params[-1]
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(T):
            inp = X[:, t]
            m = live[:, t][:, None]
            for l in range(L):
                W, U, b = params[3 * l:3 * l + 3]
                z = inp @ W + h[l] @ U + b
                i, f = _sigmoid(z[:, :H]), _sigmoid(z[:, H:2 * H])
                g, o = _act(act, z[:, 2 * H:3 * H]), _sigmoid(z[:, 3 * H:])
                cn = f * c[l] + i * g
                hn = o * _act(act, cn)
                C[l][t] = dict(inp=inp, hp=h[l], cp=c[l], i=i, f=f, g=g, o=o, c=cn, zg=z[:, 2 * H:3 * H])
                c[l] = np.where(m, cn, c[l])
                h[l] = np.where(m, hn, h[l])
                C[l][t]["h"] = h[l]
                inp = h[l]
            logits[:, t] = h[L - 1] @ Wo[:, 0] + bo[0]
    if cache:
        return logits, (C, live)
    return logits


def one_to_one(params, act, x, num_steps, dtype=np.float64):
    """RepeatVector(num_steps) -> RNNs -> Dense: x [n, D] -> [n]."""
    X = np.repeat(np.asarray(x, dtype=dtype)[:, None, :], num_steps, axis=1)
    return forward(params, act, X, None, dtype=dtype)[:, -1]


def backward(params, act, cache, dlogits):
    """BPTT from d loss / d logits [n, T]: (grads in get_weights order, dx [n, T, D]), in the dtype of dlogits."""
    C, live = cache
    dt = dlogits.dtype
    L = (len(params) - 2) // 3
    T = len(C[0])
    H = params[1].shape[0]
    n = dlogits.shape[0]
    Wo = params[-2]
    grads = [np.zeros_like(p) for p in params]
    for t in range(T):
        grads[-2][:, 0] += C[L - 1][t]["h"].T @ dlogits[:, t]
        grads[-1][0] += dlogits[:, t].sum()
    dh = [np.zeros((n, H), dtype=dt) for _ in range(L)]
    dc = [np.zeros((n, H), dtype=dt) for _ in range(L)]
    D = C[0][0]["inp"].shape[1]
    dx = np.zeros((n, T, D), dtype=dt)
    for t in range(T - 1, -1, -1):
        above = dlogits[:, t][:, None] * Wo[:, 0][None, :]
        m = live[:, t][:, None]
        for l in range(L - 1, -1, -1):
            W, U, _ = params[3 * l:3 * l + 3]
            k = C[l][t]
            dht = dh[l] + above
            ac = _act(act, k["c"])
            dct = dc[l] + dht * k["o"] * _act_grad_from_output(act, ac)
            dz = np.concatenate([dct * k["g"] * k["i"] * (1 - k["i"]), dct * k["cp"] * k["f"] * (1 - k["f"]),
                                 dct * k["i"] * _act_grad_from_output(act, k["g"]),
                                 dht * ac * k["o"] * (1 - k["o"])], axis=1)
            dz = np.where(m, dz, dt.type(0))
            grads[3 * l] += k["inp"].T @ dz
            grads[3 * l + 1] += k["hp"].T @ dz
            grads[3 * l + 2] += dz.sum(axis=0)
            dh[l] = np.where(m, dz @ U.T, dht)
            dc[l] = np.where(m, dct * k["f"], dc[l])
            above = dz @ W.T
        dx[:, t] = above
    return grads, dx


def _penalty(params, l2k, l2b):
    """l2 terms: per cell (W, b) and the head (index L); U never."""
    L = (len(params) - 2) // 3
    pen, g = 0.0, [np.zeros_like(p) for p in params]
    for l in range(L + 1):
        fk = (l2k or [0] * (L + 1))[l] if l2k and l < len(l2k) else 0.0
        fb = (l2b or [0] * (L + 1))[l] if l2b and l < len(l2b) else 0.0
        iw, ib = (3 * l, 3 * l + 2) if l < L else (len(params) - 2, len(params) - 1)
        for idx, f in ((iw, fk), (ib, fb)):
            if f:
                f = params[idx].dtype.type(f)
                pen += f * np.sum(params[idx] ** 2)
                g[idx] = 2 * f * params[idx]
    return pen, g


def loss_and_grads(params, act, X, Y, mask_value, l2k=None, l2b=None, dtype=np.float64):
    logits, cache = forward(params, act, X, mask_value, cache=True, dtype=dtype)
    live = cache[1]
    n, T = logits.shape
    Y = np.asarray(Y, dtype=dtype).reshape(n, T)
    zero, nT = logits.dtype.type(0), logits.dtype.type(n * T)
    with np.errstate(over="ignore", invalid="ignore"):
        el = np.where(live, bce_with_logits(logits, Y), zero)
    loss = el.sum() / nT
    dlog = np.where(live, (_sigmoid(logits) - Y) / nT, zero)
    grads, _ = backward(params, act, cache, dlog)
    pen, gp = _penalty(params, l2k, l2b)
    return loss + pen, [a + b for a, b in zip(grads, gp)]


def evaluate(params, act, X, Y, mask_value, l2k=None, l2b=None, dtype=np.float64):
    logits = forward(params, act, X, mask_value, dtype=dtype)
    live = _live(np.asarray(X, dtype=dtype), mask_value)
    n, T = logits.shape
    Y = np.asarray(Y, dtype=dtype).reshape(n, T)
    with np.errstate(over="ignore", invalid="ignore"):
        el = np.where(live, bce_with_logits(logits, Y), logits.dtype.type(0))
    pen, _ = _penalty(params, l2k, l2b)
    acc = np.sum(live & ((logits > 0.5) == (Y > 0.5))) / max(np.sum(live), 1)
    return float(el.sum() / logits.dtype.type(n * T) + pen), float(acc)


def fit(params, act, st, X, Y, perms, batch_size, mask_value, l2k=None, l2b=None, lr=1e-3, beta1=0.9,
        beta2=0.999, eps=1e-7, dtype=np.float64, on_batch=None):
    """Keras fit over sequences with explicit permutations; in place; returns the logged losses.
    ``on_batch(params, idx)`` is called before every Adam step (tests that guard their own inputs look there)."""
    X = np.asarray(X, dtype=dtype)
    Y = np.asarray(Y, dtype=dtype).reshape(X.shape[:2])
    N = X.shape[0]
    hist = []
    for perm in np.asarray(perms):
        tot = 0.0
        for s in range(0, N, batch_size):
            idx = perm[s:s + batch_size]
            if on_batch is not None:
                on_batch(params, idx)
            loss, grads = loss_and_grads(params, act, X[idx], Y[idx], mask_value, l2k, l2b, dtype)
            adam_step(params, grads, st, lr, beta1, beta2, eps)
            tot += float(loss) * len(idx)
        hist.append(tot / N)
    return np.asarray(hist)


def value_and_input_grad(params, act, X, num_steps, transform="identity", negate=True, dtype=np.float64):
    """convert(one_to_one, transform) with negate: (T(+-f(x)) [R], d/dx [R, D]), summed over the steps."""
    X = np.asarray(X, dtype=dtype)
    R = X.shape[0]
    Xs = np.repeat(X[:, None, :], num_steps, axis=1)
    logits, cache = forward(params, act, Xs, None, cache=True, dtype=dtype)
    s = logits.dtype.type(-1.0 if negate else 1.0)
    val, dT = _transform(transform, s * logits[:, -1])
    dlog = np.zeros((R, num_steps), dtype=dtype)
    dlog[:, -1] = s * dT
    _, dx = backward(params, act, cache, dlog)
    return val, dx.sum(axis=1)
