"""Observation store + label step of the BO loop (behaviour of bore/data.py:4-48).

``load_classification_data`` is the per-iteration label step that precedes ``fit``
(README.rst:89-90): the gamma-quantile of the targets (numpy's default linear
interpolation) splits the observations, with STRICT ``<`` so ties at the threshold are
negatives.
"""
import numpy as np


class Record:
    """Append-only (x, y[, budget]) log."""

    def __init__(self):
        self.features, self.targets, self.budgets = [], [], []

    def size(self):
        return len(self.targets)

    def append(self, x, y, b=None):
        self.features.append(x)
        self.targets.append(y)
        if b is not None:
            self.budgets.append(b)

    def load_feature_matrix(self):
        return np.vstack(self.features)

    def load_target_vector(self):
        return np.hstack(self.targets)

    def load_regression_data(self):
        return self.load_feature_matrix(), self.load_target_vector()

    def load_classification_data(self, gamma):
        """-> X (N, D) float64, z (N,) bool with z = y < quantile(y, gamma)."""
        X, y = self.load_regression_data()
        return X, classification_labels(y, gamma)

    def load_lfbo_data(self, gamma, weighting, normalize=True):
        """-> X (N, D) float64, z (N,) float32 targets, w (N,) float32 row weights: ``lfbo_targets`` of the record's
        ``y``, for ``fit(X, z, sample_weight=w)``."""
        X, y = self.load_regression_data()
        z, w, _ = lfbo_targets(y, gamma, weighting, normalize)
        return X, z, w

    def is_duplicate(self, x, rtol=1e-5, atol=1e-8):
        """True if ``x`` is allclose to any stored feature vector (the ``filter_fn`` hook of
        ``argmax``: bore/plugins/hpbandster/base.py:210-214)."""
        for prev in self.features:
            if np.allclose(prev, x, rtol=rtol, atol=atol):
                return True
        return False


def classification_labels(y, gamma):
    """z = y < np.quantile(y, gamma)   (bore/data.py:33-34)."""
    y = np.asarray(y)
    return np.less(y, np.quantile(y, q=gamma))


LFBO_WEIGHTINGS = ("ei", "lfbo")
_LFBO_THREADS = 256      # bore_lfbo_labels' workgroup: the order of the sum below is the kernel's


def lfbo_targets(y, gamma, weighting, normalize=True):
    """Targets and row weights of likelihood-free BO (LFBO, Song et al. 2022, expected-improvement utility) for one
    loop's ``y`` (N,): ``(z, w, tau)`` as float32 / float32 / float64 -- the numpy statement of ``bore_lfbo_labels``,
    equal to it bit for bit, its summation order included.

    ``tau = np.quantile(y, gamma)``, ``u = tau - y`` where ``y < tau`` (strictly, as ``Record``: ties are negatives)
    and 0 elsewhere.  ``normalize``: ``u /= mean of u over the positives``, which makes the class balance independent
    of the objective's units; with no positive nothing is divided and every row is a plain negative.

    ``"ei"``:   ``z = y < tau``, ``w = u`` on the positives and 1 elsewhere (the classifier of BORE with the positives
                weighted by their improvement).
    ``"lfbo"``: ``z = u / (1 + u)``, ``w = 1 + u``.  Per row ``w * BCE(f; z) = u * softplus(-f) + softplus(f)``:
                every row a negative of weight 1 and each positive also a positive of weight u -- LFBO's objective.

    All arithmetic is float64, rounded to float32 once at the end."""
    if weighting not in LFBO_WEIGHTINGS:
        raise ValueError(f"weighting must be one of {LFBO_WEIGHTINGS} (got {weighting!r})")
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    tau = np.float64(np.quantile(y, q=gamma))
    pos = np.less(y, tau)
    u = np.where(pos, tau - y, 0.0)
    n_pos = int(pos.sum())
    if normalize and n_pos > 0:
        # thread t adds u[t], u[t + 256], ... in that order; then p[t] += p[t + h] for h = 128, 64, ..., 1
        T = _LFBO_THREADS
        rows = np.zeros((-(-len(u) // T), T))
        rows.reshape(-1)[:len(u)] = u
        part = np.zeros(T)
        for row in rows:
            part = part + row
        h = T // 2
        while h:
            part[:h] = part[:h] + part[h:2 * h]
            h //= 2
        u = u / (part[0] / np.float64(n_pos))
    if weighting == "ei":
        z, w = pos.astype(np.float64), np.where(pos, u, 1.0)
    else:
        z, w = u / (1.0 + u), 1.0 + u
    return z.astype(np.float32), w.astype(np.float32), tau


def _host_array(a):
    """numpy view of an array-like or a torch tensor (downloaded)."""
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def resolve_sample_weight(n_rows, y=None, sample_weight=None, class_weight=None):
    """Keras ``fit(sample_weight=, class_weight=)`` as ONE float32 vector of ``n_rows`` row weights, or None when
    neither is given (the unweighted fit).  Pure host code.

    ``sample_weight``: shape (N,) or (N, 1).  ``class_weight``: ``{0: a, 1: b}`` -- the row's weight is multiplied by
    ``b`` where the label is 1 and by ``a`` otherwise (``y``: the labels, needed for it alone); with both given the
    two multiply (in float64, rounded to float32 once).  Anything else is a ``ValueError``."""
    if sample_weight is None and class_weight is None:
        return None
    n_rows = int(n_rows)
    w = np.ones(n_rows, dtype=np.float64)
    if sample_weight is not None:
        sw = _host_array(sample_weight)
        if sw.shape not in ((n_rows,), (n_rows, 1)):
            raise ValueError(f"sample_weight: expected shape ({n_rows},) or ({n_rows}, 1), got {sw.shape}")
        if sw.dtype.kind not in "fiub":
            raise ValueError(f"sample_weight: expected numbers, got dtype {sw.dtype}")
        w = w * sw.reshape(n_rows).astype(np.float64)
    if class_weight is not None:
        if not isinstance(class_weight, dict) or set(class_weight) != {0, 1}:
            raise ValueError("class_weight: expected a dict with exactly the keys 0 and 1 (a binary classifier), got "
                             f"{class_weight!r}")
        if y is None:
            raise ValueError("class_weight needs the labels")
        z = _host_array(y).reshape(-1)
        if z.shape != (n_rows,):
            raise ValueError(f"class_weight: {z.shape[0]} labels for {n_rows} rows")
        w = w * np.where(z.astype(np.float64) == 1.0,float(class_weight[1]), float(class_weight[0]))
    return np.ascontiguousarray(w, dtype=np.float32)


class MultiFidelityRecord:
    """Observations of a Hyperband run, keyed by configuration and budget (behaviour of
    bore/data.py:51-261).  A rung is a budget; rungs are numbered by increasing budget.  Labels at a rung
    are ``y <= quantile(y_rung, gamma)`` -- note ``<=``, where ``Record`` uses ``<``.  Recording the same
    ``(x, b)`` twice replaces the value in the per-configuration table but appends to the rung's target
    list again (as the reference does).  Configurations keep their insertion order."""

    def __init__(self, gamma=None):
        self._data = {}          # key(x) -> {budget: y}
        self._targets = {}       # budget -> [y, ...] in arrival order
        self.gamma = gamma

    @staticmethod
    def compute_key(x):
        return tuple(x.tolist())

    def append(self, x, y, b):
        self._data.setdefault(self.compute_key(x), {})[b] = y
        self._targets.setdefault(b, []).append(y)

    def num_rungs(self):
        return len(self._targets)

    def budgets(self, reverse=False):
        return sorted(self._targets, reverse=reverse)

    def budget(self, t):
        return self.budgets()[t]

    def _rung_size_from_budget(self, b):
        return len(self._targets[b])

    def highest_rung(self, min_size=1):
        """The highest rung with at least ``min_size`` observations, or None."""
        best = None
        for t, b in enumerate(self.budgets()):
            if self._rung_size_from_budget(b) >= min_size:
                best = t
        return best

    def rung_sizes(self):
        return [self._rung_size_from_budget(b) for b in self.budgets()]

    def rung_size(self, t):
        return self._rung_size_from_budget(self.budget(t))

    def size(self):
        return sum(self.rung_sizes())

    def load_feature_matrix(self):
        return np.vstack(self._data)

    def num_features(self):
        return len(self._data)

    def _targets_from_budget(self, b):
        return self._targets[b]

    def targets(self, t):
        return self._targets_from_budget(self.budget(t))

    def _threshold_from_budget(self, b):
        return np.quantile(self._targets_from_budget(b), q=self.gamma)

    def threshold(self, t):
        return self._threshold_from_budget(self.budget(t))

    def thresholds(self):
        return [self._threshold_from_budget(b) for b in self.budgets()]

    def _binary_labels_from_budget(self, b):
        return np.less_equal(self._targets_from_budget(b), self._threshold_from_budget(b))

    def binary_labels(self, t):
        return self._binary_labels_from_budget(self.budget(t))

    def sequences_dict(self, pad_value=-1., binary=True, return_indices=False):
        """key -> list over the rungs of the label (binary) or value, ``pad_value`` where the configuration
        has no observation; with ``return_indices`` also key -> list of "observed" flags."""
        assert not binary or self.gamma is not None, \
            "Must instantiate with `gamma` specified for binary labels!"
        seqs = {k: [] for k in self._data}
        seen = {k: [] for k in self._data}
        for b in self.budgets():
            tau = self._threshold_from_budget(b)
            for k, dct in self._data.items():
                have = b in dct
                if have:
                    seqs[k].append(int(dct[b] <= tau) if binary else dct[b])
                else:
                    seqs[k].append(pad_value)
                seen[k].append(have)
        return (seqs, seen) if return_indices else seqs

    def sequences(self, pad_value=-1., binary=True):
        """(inputs [n, T, D] float64 with ``pad_value`` rows at the rungs a configuration lacks,
        targets [n, T, 1])."""
        seqs, seen = self.sequences_dict(pad_value=pad_value, binary=binary, return_indices=True)
        inputs, targets = [], []
        for k, ys in seqs.items():
            seq = np.full((len(ys), len(k)), pad_value, dtype="float64")
            seq[seen[k]] = np.array(k)
            inputs.append(seq)
            targets.append(np.expand_dims(ys, axis=-1))
        return np.stack(inputs, axis=0), np.stack(targets, axis=0)

    def is_duplicate(self, x, rtol=1e-5, atol=1e-8):
        return any(np.allclose(np.array(k), x, rtol=rtol, atol=atol) for k in self._data)
