"""The premises of tests/test_gpu_layout_probe.py, checked on the CPU with the oracle alone (tests/layout_probe.py): for
every network the device file uses, that the probed quantities do not depend on the order of summation, that the
bfloat16 roundings in them are real, that the probes see what a layout bug does (the mutation table, printed), and that
the Adam slots of the decay probe are unique."""
import numpy as np
import pytest

import layout_probe as LP
from numeric_range import _hyper, alpha_tolerance
from oracle import bore_oracle as O

NETS = LP.all_networks()
IDS = ["%s%s model %d" % (name, " linear" if linear else "", i) for name, linear, i, _, _ in NETS]


def _same(a, b):
    return not LP.probes_differ(a, {k: b[k] for k in a})


@pytest.mark.parametrize("case", NETS, ids=IDS)
@pytest.mark.parametrize("compute", LP.COMPUTES)
def test_probed_quantities_do_not_depend_on_the_order_of_summation(case, compute):
    """The oracle equals a float64 restatement and a float32 restatement that adds the k terms in a shuffled order, bit
    for bit; every value is an integer (fit gradients: an integer over the batch's power of two) and every sum of
    magnitudes -- so every partial sum in any order -- stays below 2^24."""
    name, _, _, net, X = case
    z = LP.labels(net["seed"], len(X))
    # all rows; one row with the other sign; the live batches of the device file: 64 rows, last batches of 32, 8 and 1
    runs = [(X, None, True), (X[:1], None, False)] + [(X[-nb:], z[-nb:], True) for nb in (64, 32, 8, 1)]
    for Xr, zr, negate in runs:
        want = LP.oracle_probes(net, Xr, compute, z=zr, negate=negate)
        exact = LP.Exact()
        assert _same(LP.restate(net, Xr, exact, compute, z=zr, negate=negate), want)
        assert exact.worst + LP.FIT_BIAS < LP.LIMIT, exact.worst
        assert _same(LP.restate(net, Xr, LP.Shuffled(net["seed"]), compute, z=zr, negate=negate), want)
        for k in ("out", "grad", "val"):
            assert np.array_equal(np.round(want[k]), want[k]) and np.abs(want[k]).max() < LP.LIMIT
        if zr is not None:
            nb = len(zr)
            assert all(np.array_equal(np.round(g * nb), g * nb) and np.abs(g * nb).max() < LP.LIMIT for g in want["g"])
    # e^-logit is 0 in float32 for every row, and a few Adam steps of 1e-3 cannot change that
    assert LP.ref_forward(net, X, compute).min() >= LP.FIT_BIAS


@pytest.mark.parametrize("case", NETS, ids=IDS)
def test_the_roundings_are_real(case):
    """At least one layer rounds more than half of its outputs; the rounded inputs include an exact tie each way, in
    row 0 already; the fit gradients of every tensor are not all equal."""
    name, _, _, net, X = case
    share = LP.rounded_share(net, X)
    print("%s: share of outputs rounded per layer %s" % (name, np.round(share, 3)))
    assert max(share) > 0.5
    for rows in (X[:1], X):
        x32 = rows.astype(np.float32)
        r = O.bf16_round(x32)
        tie = (x32 != r) & (np.abs(x32 - r) == 1) & (x32 >= 256)        # (odd 9-bit integers: exactly between two bfloat16)
        assert (tie & (r < x32)).any() and (tie & (r > x32)).any()
    g = LP.ref_fit_grads(net, X[:64], LP.labels(net["seed"], 64), "bfloat16")[1]
    assert all(len(np.unique(a)) > 1 for a in g[:-1])


@pytest.mark.parametrize("name", list(LP.SHAPES))
def test_the_loss_sums_are_order_free(name):
    """Every loss the device file reads is a sum of integer logits (label 0) and exact zeros (label 1) that stays below
    2^24 -- loss_sum asserts it -- for the data of the live-batch and the evaluate probes, in both arithmetics."""
    for compute in LP.COMPUTES:
        for linear in LP.VARIANTS:
            for N, live in LP.LIVE:
                for net, c in zip(LP.networks(name, linear), LP.live_case(name, linear, N, live)):
                    rows = c["rows"]
                    assert (c["z"][rows] == 0).any() and c["z"].sum() >= N - len(rows)
                    assert sorted(c["perm"]) == list(range(N))
                    total = LP.loss_sum(LP.ref_fit_grads(net[0], c["X"][rows], c["z"][rows], compute)[0], c["z"][rows])
                    assert total > 0 and LP.mean_of(total, N)[1] > 0
        for N in LP.EVAL_N:
            for net, (X, z) in zip(LP.networks(name), LP.eval_case(name, N)):
                assert LP.loss_sum(LP.ref_forward(net[0], X, "float32"), z) >= 0


_table = {}


@pytest.mark.parametrize("case", NETS, ids=IDS)
def test_the_probes_see_what_a_layout_bug_does(case):
    """120 sampled mutations per layer and kind, on the bfloat16 oracle (the blunter of the two: a rounding can swallow
    a change): every row swap, column swap and bias swap changes the forward, the input-gradient or the first-step
    fit-gradient probe; one element off by one does so in at least 0.9 of the samples of every layer."""
    name, _, i, net, X = case
    z = LP.labels(net["seed"], len(X))
    base = LP.oracle_probes(net, X, "bfloat16")
    base["g"] = LP.ref_fit_grads(net, X[:64], z[:64], "bfloat16")[1]
    rs = np.random.RandomState(net["seed"])
    bad = []
    for l in range(len(net["acts"])):
        for kind in LP.MUTATIONS:
            seen = sampled = 0
            for _ in range(LP.SAMPLES):
                q = LP.sample_mutation(kind, net["p"], l, rs)
                if q is None:
                    break
                sampled += 1
                seen += LP.detects(net, X, z, q, base) is not None
            if not sampled:
                continue
            _table[(IDS[NETS.index(case)], l + 1, kind)] = (seen, sampled)
            print("%-36s layer %d %-12s %3d / %3d" % (IDS[NETS.index(case)], l + 1, kind, seen, sampled))
            if seen < (sampled if kind in LP.EVERY else LP.ELEMENT_FLOOR * sampled):
                bad.append((l + 1, kind, seen, sampled))
    assert not bad, bad


@pytest.mark.parametrize("name", list(LP.SHAPES))
def test_truncation_is_visible(name):
    """Truncation in place of round-to-nearest-even changes the forward probe of every network."""
    for net, X in LP.networks(name) + LP.networks(name, True):
        want = LP.ref_forward(net, X, "bfloat16")
        with LP.truncating():
            got = LP.ref_forward(net, X, "bfloat16")
        assert not np.array_equal(got, want)
        assert np.array_equal(LP.ref_forward(net, X, "bfloat16"), want)     # (the oracle is itself again)


@pytest.mark.parametrize("name", list(LP.SHAPES))
def test_the_decay_probes_slots_are_unique(name):
    """F1's prepared slots: one distinct value per element of a launch, exact in float32, v0 > 0; and they stay
    distinct under the recurrence the device is compared with (a slot written to another element's place is seen
    after every step)."""
    D, units, _ = LP.SHAPES[name]
    P = sum(a.size for a in LP.networks(name)[0][0]["p"])
    m0, v0 = LP.unique_slots(LP.N_MODELS, P)
    assert m0.dtype == np.float32 and (v0 > 0).all() and (m0 > 0).any() and (m0 < 0).any()
    assert len(np.unique(m0)) == m0.size == len(np.unique(v0)) == LP.N_MODELS * P
    m, v = m0.copy(), v0.copy()
    for _ in range(39):             # the longest decay of the device file: three epochs of 13 steps
        LP.adam_slot_step(m, v, 0.0)
        assert len(np.unique(m)) == m.size == len(np.unique(v))


def test_the_clock_and_the_trajectory_restate_the_oracle():
    """adam_clock is oracle.adam_alpha to within the bound tests/numeric_range.py derives for AdamClock; adam_trajectory's
    slots are oracle.adam_step's in float32, bit for bit, and its theta lies within its own bound of the float32 oracle's."""
    lr, b1, b2, _ = _hyper(*LP.ADAM)           # (the float32-rounded hyper-parameters the kernel receives)
    for t0 in (0, 5):
        for k, a in enumerate(LP.adam_clock(t0, 40)):
            ref = float(O.adam_alpha(t0 + k + 1, lr, b1, b2, dtype=np.float64))
            assert abs(float(a) - ref) <= alpha_tolerance(t0 + k + 1, b1, b2) * ref
    rs = np.random.RandomState(0)
    P = 50
    th0 = rs.randint(-3, 4, size=P).astype(np.float32)
    m0, v0 = LP.unique_slots(1, P)
    grads = [None, (rs.randint(-99, 100, size=P) / 64.0), None, None]
    T = LP.adam_trajectory(th0, m0[0], v0[0], 5, grads)
    p = [th0.copy()]
    st = O.AdamState(p)
    st.t, st.m, st.v = 5, [m0[0].copy()], [v0[0].copy()]
    for g in grads:
        O.adam_step(p, [np.zeros(P, dtype=np.float32) if g is None else g.astype(np.float32)], st, *LP.ADAM, eps=LP.EPS)
    assert np.array_equal(st.m[0], T["m"]) and np.array_equal(st.v[0], T["v"]) and st.t == T["t"]
    assert LP.worst_ratio(p[0], T["theta"], T["tol"]) <= 1.0
    assert (T["tol"] < 1e-5).all() and (np.abs(T["theta"] - th0) > 1e-5).any()       # (and the bound binds)
    # from zero slots a zero gradient moves nothing and allows nothing
    Z = LP.adam_trajectory(th0, np.zeros(P), np.zeros(P), 0, [None, None])
    assert np.array_equal(Z["theta"], th0) and not Z["tol"].any() and not Z["m"].any()
