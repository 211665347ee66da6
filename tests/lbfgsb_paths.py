"""The case table of the restart kernels' bound kinds and recovery paths: nets, weight scales, seeds, bound patterns and
starts, shared by tests/test_lbfgsb_host.py (CPU: the oracle's f and g show that every premise is met) and
tests/test_gpu_lbfgsb_paths.py (the device, held to the host build).  NumPy only; nobody writes to what it returns.

Bound patterns over D variables, lo = 0 and hi = 1 where finite:
  a   every side open
  b   lower bound only on even variables, upper bound only on odd ones
  c   nbd 0, 1, 2, 3 cycling over the variables (D = 2: two problems of two kinds each)
  d   the box with one fixed variable lo[k] = hi[k] = 0.4, k the first variable and, for D > 2, in a second problem the
      last; the starts are drawn from U(-0.1, 1.1), so they lie off the fixed value and are projected onto it
  e   the box with starts on corners and faces (every coordinate 0, 1 or drawn)
  f   the box with the weights scaled up ("hard": saturated units, flat regions, line searches at the float32 floor)
  g   pattern c's bounds with the hard weights: the backtracking fallback of subsm needs a projected step that is no
      descent direction, which the open sides of a saturated net give far more often than the box does
  w   pattern b at maxcor 3, so that the history wraps
Patterns a-e and w use a net's "soft" scale, under which the objective is bounded (a sigmoid output, a sigmoid transform
or tanh layers): with a linear output and the identity transform an all-open problem runs off."""
import numpy as np

from oracle import bore_oracle as O

INF = np.inf
PATTERNS = ["a", "b", "c", "d", "e", "f", "g", "w"]
MAXITER = 40
RELU3, TANH3 = ["relu", "relu", "sigmoid"], ["tanh", "tanh", "linear"]
# name: (D, units, activations, compute, transform, seed, soft scale, hard scale)
NETS = {
    "2-16-16-1": (2, [16, 16, 1], RELU3, "float32", "identity", 37, 1.0, 3.0),
    "5-24-12-1": (5, [24, 12, 1], TANH3, "float32", "identity", 2, 2.0, 8.0),
    "16-24-12-1": (16, [24, 12, 1], TANH3, "float32", "identity", 6, 1.0, 4.0),
    "6-32-32-1": (6, [32, 32, 1], TANH3, "float32", "identity", 3, 1.5, 6.0),
    "16-32-32-32-1": (16, [32, 32, 32, 1], ["elu"] * 3 + ["linear"], "float32", "sigmoid", 5, 1.0, 3.0),
    "16-64-64-64-1": (16, [64, 64, 64, 1], ["relu"] * 3 + ["linear"], "float32", "sigmoid", 16, 1.0, 3.0),
    "16-64-64-64-1 bf16": (16, [64, 64, 64, 1], ["relu"] * 3 + ["linear"], "bfloat16", "sigmoid", 3, 1.0, 1.5),
    "32-128-128-1 bf16": (32, [128, 128, 1], ["relu", "relu", "linear"], "bfloat16", "sigmoid", 24, 1.0, 1.5),
    "8-256-256-1": (8, [256, 256, 1], ["relu", "elu", "linear"], "float32", "sigmoid", 7, 1.0, 3.0),
    "5-7-3-1": (5, [7, 3, 1], ["tanh", "sigmoid", "linear"], "float32", "sigmoid", 1, 1.0, 3.0),
}
LSTM_SHAPE = (3, 1, 7, "relu", 4)            # (D, layers, hidden, activation, steps: the smallest of test_gpu_lstm_acq.py)
LSTM = dict(seed=101, transform="sigmoid", soft=1.0, hard=4.0)
# family: (nets, restarts per launch, BORE_LBFGSB_* knobs, streamed)
FAMILIES = {
    "four_wave_static": (["2-16-16-1"], 9, {}, None),
    "run_time_layout": (["5-24-12-1", "16-24-12-1"], 7, {}, None),
    "lane_per_problem": (["6-32-32-1"], 9, dict(COOP_GRID=0), None),
    "two_workgroups_per_cu": (["6-32-32-1"], 9, dict(OCC2=1), None),
    "twelve_waves": (["6-32-32-1", "16-32-32-32-1"], 13, dict(WAVES=12), None),
    "eight_waves_float32": (["16-64-64-64-1"], 9, dict(WAVES=8), None),
    "eight_waves_bfloat16": (["16-64-64-64-1 bf16"], 9, dict(WAVES=8), None),
    "pooled_bfloat16": (["32-128-128-1 bf16"], 9, dict(WAVES=8, BIG=1), None),
    "queue": (["6-32-32-1"], 9, dict(QUEUE=1), None),
    "streamed": (["8-256-256-1", "5-7-3-1"], 7, {}, True),
    "lstm_streamed": (["lstm"], 9, {}, True),
}
PER_FAMILY = ["ls_fail_refresh", "ls_cache_hit", "update_skipped", "enter", "leave", "subsm_hit_bound", "subsm_backtrack",
              "unconstrained_iteration", "first_step_not_boxed", "fixed_variable", "free_variable", "clipped_start",
              "history_wrapped"]
WHOLE_FILE = ["formk_refresh", "abnormal", "nfree_zero", "info_minus5", "ls_maxls"]


def bounds_of(pattern, D):
    """The problems of a pattern: [(tag, lo, hi)]."""
    lo, hi = np.zeros(D), np.ones(D)
    i = np.arange(D)
    if pattern == "a":
        return [("open", np.full(D, -INF), np.full(D, INF))]
    if pattern in ("b", "w"):
        return [("lower even, upper odd", np.where(i % 2 == 0, 0.0, -INF), np.where(i % 2 == 1, 1.0, INF))]
    if pattern in ("c", "g"):
        def kinds(k):
            return np.where((k == 1) | (k == 2), 0.0, -INF), np.where(k >= 2, 1.0, INF)
        if D == 2:
            return [("nbd 0 1",) + kinds(np.array([0, 1])), ("nbd 2 3",) + kinds(np.array([2, 3]))]
        return [("nbd cycling",) + kinds(i % 4)]
    if pattern == "d":
        out = []
        for k in ([0] if D <= 2 else [0, D - 1]):
            l, u = lo.copy(), hi.copy()
            l[k] = u[k] = 0.4
            out.append(("fixed %d" % k, l, u))
        return out
    return [("box", lo, hi)]


_made = {}


def weights(name):
    """(soft, hard): the net's parameters at its two weight scales -- Dense: the oracle's list [W, b, ...] (float32);
    "lstm": lstm_oracle's list, rounded to float32."""
    if name not in _made:
        if name == "lstm":
            import lstm_oracle as LO
            D, L, Hn, act, T = LSTM_SHAPE
            rs = np.random.RandomState(LSTM["seed"])
            p = LO.init_weights(D, Hn, L, rs)
            p[-1] = rs.choice([-1.0, 1.0], size=1) * rs.uniform(0.25, 0.5, size=1)
            _made[name] = tuple([(q * s).astype(np.float32).astype(np.float64) for q in p]
                                for s in (LSTM["soft"], LSTM["hard"]))
        else:
            D, units, acts, compute, tr, seed, soft, hard = NETS[name]
            rs = np.random.RandomState(seed)
            p = O.glorot_uniform_params(D, units, rs)
            for k in range(1, len(p), 2):
                p[k] = rs.normal(scale=0.1, size=p[k].shape).astype(np.float32)
            _made[name] = tuple([q * np.float32(s) if k % 2 == 0 else q.copy() for k, q in enumerate(p)]
                                for s in (soft, hard))
    return _made[name]


def dim(name):
    return LSTM_SHAPE[0] if name == "lstm" else NETS[name][0]


def launches(family, name):
    """The launches of one net of a family: [(pattern, tag, lo, hi, X0 [R, D], hard, maxcor)], the starts from the
    net's own stream."""
    R = FAMILIES[family][1]
    D = dim(name)
    rs = np.random.RandomState(7000 + sum(map(ord, family + name)))
    out = []
    for pattern in PATTERNS:
        for tag, lo, hi in bounds_of(pattern, D):
            X0 = rs.uniform(-0.1, 1.1, size=(R, D))
            if pattern == "e":
                pick = rs.randint(0, 3, size=(R, D))
                X0 = np.where(pick == 0, 0.0, np.where(pick == 1, 1.0, np.clip(X0, 0.0, 1.0)))
            out.append((pattern, tag, lo, hi, X0, pattern in ("f", "g"), 3 if pattern == "w" else 10))
    return out


def oracle_fg(name, hard):
    """x -> (f, g) of the net in the oracle's arithmetic of its compute type."""
    p = weights(name)[1 if hard else 0]
    if name == "lstm":
        import lstm_oracle as LO
        D, L, Hn, act, T = LSTM_SHAPE
        q = LO.as_dtype(p, np.float32)

        def fg(x):
            v, g = LO.value_and_input_grad(q, act, x[None], T, LSTM["transform"], True, np.float32)
            return float(v[0]), g[0].astype(np.float64)
        return fg
    D, units, acts, compute, tr = NETS[name][:5]
    if compute == "bfloat16":
        def fg(x):
            v, g = O.value_and_input_grad_bf16(p, acts, x, tr)
            return float(v[0]), g[0]
        return fg
    return lambda x: tuple(O.value_and_input_grad(p, acts, x, tr))


def opts_for(maxcor):
    return dict(maxcor=maxcor, maxiter=MAXITER, ftol=1e-9)


def add_events(total, res, x0=None, lo=None, hi=None):
    """Adds a record's events to `total`; with the start and its bounds also `clipped_start`: the start lay outside
    its bounds.  (lbfgsb_init clips the start as SciPy's wrapper does, so the projection in the routine's own `active`
    step never moves a point and the event projected_start cannot occur through lbfgsb_init: the clipped start is the
    projection a caller sees.)"""
    for k, v in res.events.items():
        total[k] = total.get(k, 0) + v
    if x0 is not None:
        total["clipped_start"] = total.get("clipped_start", 0) + int(np.any((x0 < lo) | (x0 > hi)))
    return total
