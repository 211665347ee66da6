"""Classifier ensembles: the statement of the acquisition score the HIP kernels are held to.

An ensemble is K members of one network description.  With f_k(x) member k's output (what ``predict`` returns: a
logit or a probability, as the net is built), sums taken in the order k = 0 .. K-1::

    mu    = (1/K) sum_k f_k
    d_k   = f_k - mu
    v     = (1/K) sum_k d_k^2
    sigma = sqrt(v + VAR_FLOOR)
    s     = mu + beta sigma                      beta >= 0, finite
    grad s = sum_k c_k grad f_k,                 c_k = 1/K + beta d_k / (K sigma)

an upper confidence bound on the classifier: the members' disagreement is the uncertainty.  The floor makes sigma
smooth -- no branch at sigma = 0; identical members get c_k = 1/K up to rounding; K = 1 gives s = f + beta 1e-6, a
constant shift.  beta = 0 is the mean, and with K = 1 the single-model objective.

``ensemble_score`` is this in numpy, float64 throughout: the documentation, the checker of
``bore_ensemble_value_and_input_grad`` / ``bore_ensemble_screen_topk`` (bore_amd/csrc/bore_ensemble.hip, which combine
float32 f_k in float64 and apply T to float32(s)), and the host route of the ensemble models, fed by ONE
``ops.mlp_value_and_input_grad`` call with ``n_models = K``.
"""
from __future__ import annotations

import numpy as np

VAR_FLOOR = 1e-12          # include/bore_hip.h BORE_ENSEMBLE_VAR_FLOOR
MAX_MEMBERS = 16           # include/bore_hip.h BORE_ENSEMBLE_MAX_MEMBERS


def check_beta(beta):
    beta = float(beta)
    if not (beta >= 0.0 and np.isfinite(beta)):
        raise ValueError(f"beta must be finite and >= 0, got {beta!r}")
    return beta


def check_members(members):
    if isinstance(members, bool) or int(members) != members:
        raise ValueError(f"members must be an integer, got {members!r}")
    if not 1 <= int(members) <= MAX_MEMBERS:
        raise ValueError(f"an ensemble has 1..{MAX_MEMBERS} members, got {members!r}")
    return int(members)


def ensemble_stats(F, beta=0.0):
    """F [K, R] -> (mu, sigma, s, c): mu, sigma, s [R] and the members' gradient weights c [K, R], float64."""
    F = np.asarray(F, dtype=np.float64)
    if F.ndim != 2 or F.shape[0] < 1:
        raise ValueError(f"F: expected [K >= 1, R], got shape {F.shape}")
    beta = check_beta(beta)
    K = F.shape[0]
    total = np.zeros(F.shape[1])
    for k in range(K):
        total = total + F[k]
    mu = total / K
    d = F - mu
    v = np.zeros(F.shape[1])
    for k in range(K):
        v = v + d[k] * d[k]
    sigma = np.sqrt(v / K + VAR_FLOOR)
    s = mu + beta * sigma
    c = 1.0 / K + beta * d / (K * sigma)
    return mu, sigma, s, c


def _transform(transform, u):
    """T(u) and T'(u) of a named transform, float64."""
    if transform == "identity":
        return u, np.ones_like(u)
    if transform == "sigmoid":
        e = np.exp(-np.abs(u))
        t = np.where(u >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        return t, t * (1.0 - t)
    if transform == "exp":
        t = np.exp(u)
        return t, t
    raise ValueError(f"transform must be one of ('identity', 'sigmoid', 'exp'), got {transform!r}")


def ensemble_score(F, G, beta=0.0, transform="identity", negate=True):
    """The optimiser's objective over an ensemble: ``(val [R], grad [R, D])`` of T(-s) (``negate``) or T(s).

    F [K, R]: the members' outputs; G [K, R, D]: their input gradients.  float64 throughout."""
    G = np.asarray(G, dtype=np.float64)
    mu, sigma, s, c = ensemble_stats(F, beta)
    if G.ndim != 3 or G.shape[:2] != c.shape:
        raise ValueError(f"G: expected [K, R, D] with K, R = {c.shape}, got shape {G.shape}")
    gs = np.zeros(G.shape[1:])
    for k in range(G.shape[0]):
        gs = gs + c[k][:, None] * G[k]
    sign = -1.0 if negate else 1.0
    val, dT = _transform(transform, sign * s)
    return val, (sign * dT)[:, None] * gs
