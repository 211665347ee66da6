"""The float64 checker of the weighted fits (Keras ``sample_weight`` / ``class_weight``), composed from the oracle's
public pieces without touching the oracle:

  a step over a batch of nb rows minimises  (1/nb) sum_i w_i loss_i + l2 penalties      (SUM_OVER_BATCH_SIZE)

so the batch gradient is  sum_i w_i grads(row i alone) / nb  -- ``oracle.bore_oracle.loss_and_grads`` on single rows,
whose "mean over the batch" is then the row's own term -- with the l2 terms added once, and ``adam_step`` does the rest.
The logged epoch loss is the batch losses averaged with batch-size weights, as ``oracle.bore_oracle.fit`` logs it.
Shared by tests/test_weighted_host.py (which holds it against torch autograd) and tests/test_gpu_weighted.py."""
import numpy as np

from oracle import bore_oracle as O


def weighted_loss_and_grads(params, acts, Xb, zb, wb, l2=None):
    """-> (loss, grads) of (1/nb) sum_i w_i BCE_i + sum_k l2_k |theta_k|^2, in the dtype of ``params``."""
    dt = params[0].dtype.type
    nb = Xb.shape[0]
    loss = dt(0)
    grads = [np.zeros_like(p) for p in params]
    for i in range(nb):
        li, gi = O.loss_and_grads(params, acts, Xb[i:i + 1], zb[i:i + 1])
        loss = loss + dt(wb[i]) * li
        for g, d in zip(grads, gi):
            g += dt(wb[i]) * d
    loss = loss / dt(nb)
    grads = [g / dt(nb) for g in grads]
    if l2 is not None:
        for k, f in enumerate(l2):
            if f:
                f = dt(f)
                loss = loss + f * np.sum(params[k] * params[k])
                grads[k] = grads[k] + dt(2) * f * params[k]
    return loss, grads


def weighted_fit(params, acts, st, X, z, w, perms, batch_size=64, l2=None, dtype=np.float64, **adam):
    """``oracle.bore_oracle.fit`` under row weights ``w``: updates ``params`` / ``st`` in place, returns the logged
    epoch losses."""
    Xc, zc, wc = np.asarray(X, dtype=dtype), np.asarray(z).astype(dtype), np.asarray(w).astype(dtype)
    N = Xc.shape[0]
    hist = []
    for perm in np.asarray(perms):
        tot = 0.0
        for s in range(0, N, batch_size):
            idx = perm[s:s + batch_size]
            loss, grads = weighted_loss_and_grads(params, acts, Xc[idx], zc[idx], wc[idx], l2=l2)
            O.adam_step(params, grads, st, **adam)
            tot += float(loss) * len(idx)
        hist.append(tot / N)
    return np.asarray(hist)


def weighted_evaluate(params, acts, X, z, w, l2=None, dtype=np.float64):
    """Keras ``evaluate(sample_weight=w)``: (sum_i w_i BCE_i / N + penalties, the UNWEIGHTED accuracy)."""
    p = [np.asarray(q, dtype=dtype) for q in params]
    Xc, zc = np.asarray(X, dtype=dtype), np.asarray(z).astype(dtype).reshape(-1, 1)
    a = O.forward(p, acts, Xc, logits=True)
    loss = float(np.sum(np.asarray(w, dtype=dtype).reshape(-1, 1) * O.bce_with_logits(a, zc)) / len(Xc))
    if l2 is not None:
        for q, f in zip(p, l2):
            if f:
                loss += float(f) * float(np.sum(q * q))
    return loss, O.evaluate(p, acts, Xc, z, dtype=dtype)[1]
