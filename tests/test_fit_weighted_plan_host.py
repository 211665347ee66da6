"""What bore_mlp_fit_weighted plans, through bore_fit_plan_query (no GPU): weighted requests of the narrow static shapes
take their own flavour, every other weighted request the generic flavour with the unweighted generic carve, and the
carve of a weighted static plan holds what fit_body<SHAPE, NW, true> indexes.

The kernel-side assertions are written from fit_body (bore_amd/csrc/bore_hip.hip), not from the planner:
  stage    [KC0 + 1][256] floats at o_stage, KC0 = ceil(D / 4) k-chunks of the first layer; the weighted kernel parks
           the weight in the label plane (slot of lane 16 + m16), so it parks KC0 + 1 floats per lane like the unweighted
  perm     [PG][N] ints at o_perm for device-drawn shuffles (PG = perm_group(N, 256); the pipelined form uses two of
           them), [N] for an explicit one; perm2 [N] when perm_ahead
  m, v     P_lds floats each when state_in_lds;  X [N][D], z [N], w [N] when data_in_lds (w: weighted static plans)
  the layout copy parked behind everything: (o_layout + BORE_LAYOUT_FLOATS + 4) floats within 160 KiB"""
import ctypes as C
import os

import pytest

from bore_amd import _lib, ops

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_BYTES = 163840
THREADS = 256
R, S, E, LIN = "relu", "sigmoid", "elu", "linear"
# (the networks and activations of tests/native/fit_plan_dump.hip)
STATIC = {1: ("2-16-16-1", 2, [16, 16, 1], R, S), 2: ("6-32-32-1", 6, [32, 32, 1], R, S),
          5: ("16-32-32-32-1", 16, [32, 32, 32, 1], E, LIN), 6: ("16-32-32-1", 16, [32, 32, 1], R, S),
          7: ("16-16-16-1", 16, [16, 16, 1], E, S)}
W8_SHAPES = (2, 5, 6)
OTHERS = {"16-64-64-64-1": (16, [64, 64, 64, 1], R, S), "5-24-12-1": (5, [24, 12, 1], R, S),
          "8-32-32-32-32-1": (8, [32, 32, 32, 32, 1], R, S)}
NS = [1, 5, 48, 49, 64, 65, 112, 113, 128, 129, 512, 513]
CARVE = [f for f in ops.FIT_PLAN_FIELDS if f not in ("flavour", "w8")]


def make(D, units, hidden, out):
    return _lib.make_desc(D, units, [hidden] * (len(units) - 1) + [out])


def layout_tail():
    """BORE_LAYOUT_FLOATS + 4, from the library: a generic plan's lds_floats is its o_layout + BORE_LAYOUT_FLOATS."""
    p = ops.fit_plan_query(make(*OTHERS["8-32-32-32-32-1"]), 1, 10, 16)
    assert p["flavour"] == 0
    return p["lds_floats"] - p["o_layout"] + 4


@pytest.fixture
def switch_unset(monkeypatch):
    monkeypatch.delenv("BORE_FIT_WEIGHTED_STATIC", raising=False)
    monkeypatch.delenv("BORE_FIT_W8", raising=False)


def perm_group(N):
    g = THREADS // ((N + 63) & ~63)
    return 4 if g >= 4 else 2 if g >= 2 else 1


def regions(p, N, D, with_perm, kc0):
    """[(name, start, end)] of what the weighted static kernel indexes under plan p."""
    r = [("theta", 0, p["P_lds"]), ("tile", p["o_tile"], p["o_tile"] + p["tile_floats"]), ("zt", p["o_zt"], p["o_zt"] + 64),
         ("misc", p["o_misc"], p["o_misc"] + 8), ("stage", p["o_stage"], p["o_stage"] + (kc0 + 1) * THREADS)]
    if p["perm_in_lds"]:
        r.append(("perm", p["o_perm"], p["o_perm"] + (1 if with_perm else perm_group(N)) * N))
    if p["state_in_lds"]:
        r += [("m", p["o_m"], p["o_m"] + p["P_lds"]), ("v", p["o_v"], p["o_v"] + p["P_lds"])]
    if p["data_in_lds"]:
        r += [("X", p["o_X"], p["o_X"] + N * D), ("z", p["o_z"], p["o_z"] + N), ("w", p["o_w"], p["o_w"] + N)]
    if p["perm_ahead"]:
        r.append(("perm2", p["o_perm2"], p["o_perm2"] + N))
    return r


@pytest.mark.parametrize("shape", sorted(STATIC))
def test_static_shapes_take_their_own_flavour(switch_unset, shape):
    _, D, units, hidden, out = STATIC[shape]
    desc = make(D, units, hidden, out)
    for N in NS:
        for with_perm in (False, True):
            for n_models, cus in ((1, 256), (3, 3), (4, 3), (257, 256)):
                p = ops.fit_plan_query(desc, n_models, N, 64, with_perm, True, cus)
                assert p["flavour"] == shape, (N, with_perm)
                assert p["w8"] == int(shape in W8_SHAPES and cus >= n_models), (N, with_perm, n_models, cus)
                assert p["state_in_lds"] == 1 and p["perm_in_lds"] == 1


@pytest.mark.parametrize("name,batch_size", [(STATIC[s][0], b) for s in sorted(STATIC) for b in (16, 128)]
                         + [(n, 64) for n in OTHERS])
def test_everything_else_plans_the_generic_flavour_with_the_unweighted_generic_carve(switch_unset, monkeypatch, name,
                                                                                  batch_size):
    net = OTHERS.get(name) or next(v[1:] for v in STATIC.values() if v[0] == name)
    desc = make(*net)
    # the unweighted GENERIC carve: an unweighted request plans flavour -n_layers with the same carve where the network
    # has at most four layers (the layout copy apart: lds_floats), so the reference is the weighted plan with the
    # switch off -- the parent's plan -- and the unweighted plan where both are flavour 0
    for N in NS:
        for with_perm in (False, True):
            try:
                w = ops.fit_plan_query(desc, 1, N, batch_size, with_perm, True)
            except _lib.NeedsPermError as refusal:     # (the wide net: no room to draw 512 rows' shuffle -- as before)
                assert name == "16-64-64-64-1" and N >= 512 and not with_perm
                monkeypatch.setenv("BORE_FIT_WEIGHTED_STATIC", "0")
                with pytest.raises(_lib.NeedsPermError) as parent:
                    ops.fit_plan_query(desc, 1, N, batch_size, with_perm, True)
                monkeypatch.delenv("BORE_FIT_WEIGHTED_STATIC")
                assert str(parent.value) == str(refusal)
                continue
            assert w["flavour"] == 0 and w["w8"] == 0 and w["o_w"] == 0 and w["stage_floats"] == 0
            u = ops.fit_plan_query(desc, 1, N, batch_size, with_perm, False)
            assert u["flavour"] <= 0 or name == "16-64-64-64-1"
            if u["flavour"] <= 0:
                same = [f for f in CARVE if f not in ("lds_floats", "perm_ahead", "o_perm2", "total", "o_layout")]
                assert {f: w[f] for f in same} == {f: u[f] for f in same}, (N, with_perm)
            if u["flavour"] == 0:
                assert {f: w[f] for f in CARVE} == {f: u[f] for f in CARVE}, (N, with_perm)
            monkeypatch.setenv("BORE_FIT_WEIGHTED_STATIC", "0")
            assert ops.fit_plan_query(desc, 1, N, batch_size, with_perm, True) == w
            monkeypatch.delenv("BORE_FIT_WEIGHTED_STATIC")


@pytest.mark.parametrize("shape", sorted(STATIC))
def test_the_weighted_static_carve_holds_what_the_kernel_indexes(switch_unset, shape):
    _, D, units, hidden, out = STATIC[shape]
    desc = make(D, units, hidden, out)
    kc0 = (D + 3) // 4
    tail = layout_tail()
    seen_without_data = False
    for N in NS + [2000, 4000, 9000]:
        for with_perm in (False, True):
            try:
                p = ops.fit_plan_query(desc, 1, N, 64, with_perm, True)
            except _lib.UnsupportedError:          # (NeedsPermError: too many rows for a device-drawn shuffle)
                assert N > 513 and not with_perm
                continue
            if p["flavour"] != shape:              # (an explicit perm too long for LDS: the generic fallback)
                assert N > 513 and p["flavour"] == 0 and p["o_w"] == 0
                continue
            assert p["stage_floats"] >= (kc0 + 1) * THREADS
            assert p["o_stage"] + (kc0 + 1) * THREADS <= p["o_perm"]
            if p["data_in_lds"]:
                assert p["o_w"] >= p["o_z"] + N and p["o_w"] + N <= p["total"]
            else:
                assert p["o_w"] == 0 and p["o_X"] == 0 and p["o_z"] == 0
                seen_without_data = True
            r = sorted(regions(p, N, D, with_perm, kc0), key=lambda x: x[1])
            for (na, _, ea), (nb, sb, _) in zip(r, r[1:]):
                assert ea <= sb, (N, with_perm, na, nb)
            assert r[-1][2] <= p["total"] <= p["o_layout"] <= p["lds_floats"]
            assert p["o_keys"] % 4 == 0 and p["o_perm"] <= p["o_keys"]
            assert (p["o_layout"] + tail) * 4 <= LDS_BYTES
    assert seen_without_data            # (the sweep reaches the gather from global memory)


def golden_parent_plans():
    """{(net, N, perm): {field: value}} from the parent build's tests/native/fit_plan_dump text (B = 64, no batch mode)."""
    names = dict(tile="o_tile", zt="o_zt", misc="o_misc", stage="o_stage", m="o_m", v="o_v", perm="o_perm",
                 perm2="o_perm2", keys="o_keys", X="o_X", z="o_z", g="o_g", layout="o_layout")
    plans = {}
    with open(os.path.join(HERE, "golden", "fit_plan_static_unweighted.txt")) as f:
        for line in f:
            head, rest = line.split(" -> ")
            net, N, B, perm, batch = head.split()
            assert B == "B=64" and batch == "batch=0"
            kv = dict(t.split("=") for t in rest.replace("|", " ").split())
            assert kv.pop("rc") == "0"
            plans[(net, int(N[2:]), int(perm[5:]))] = {names.get(k, k): int(v) for k, v in kv.items()}
    return plans


def test_the_unweighted_query_is_unmoved(switch_unset, monkeypatch):
    plans = golden_parent_plans()
    assert len(plans) == 60
    for setting in (None, "0", "1"):
        if setting is not None:
            monkeypatch.setenv("BORE_FIT_WEIGHTED_STATIC", setting)
        for (net, N, with_perm), want in plans.items():
            shape = next(s for s, v in STATIC.items() if v[0] == net)
            got = ops.fit_plan_query(make(*STATIC[shape][1:]), 1, N, 64, with_perm, False)
            assert got["flavour"] == shape and got["o_w"] == 0
            assert {k: got[k] for k in want if k in got} == {k: v for k, v in want.items() if k in got}, (net, N, with_perm)
            assert set(CARVE) - {"o_w", "stage_floats"} <= set(want)


def test_the_switch_sends_every_weighted_plan_to_the_generic_flavour(switch_unset, monkeypatch):
    monkeypatch.setenv("BORE_FIT_WEIGHTED_STATIC", "0")
    for shape, (_, D, units, hidden, out) in STATIC.items():
        for N in NS:
            for with_perm in (False, True):
                p = ops.fit_plan_query(make(D, units, hidden, out), 1, N, 64, with_perm, True)
                assert p["flavour"] == 0 and p["w8"] == 0 and p["o_w"] == 0 and p["stage_floats"] == 0
    monkeypatch.setenv("BORE_FIT_WEIGHTED_STATIC", "1")
    assert ops.fit_plan_query(make(*STATIC[5][1:]), 1, 100, 64, False, True)["flavour"] == 5


def test_the_query_refuses_what_the_entry_point_refuses(switch_unset):
    desc = make(*STATIC[1][1:])
    with pytest.raises(RuntimeError, match="batch_size"):
        ops.fit_plan_query(desc, 1, 10, 0)
    with pytest.raises(_lib.NeedsPermError):
        ops.fit_plan_query(make(*OTHERS["5-24-12-1"]), 1, 9723, 64, False, True)
    with pytest.raises(_lib.UnsupportedError, match="float32"):
        ops.fit_plan_query(_lib.make_desc(16, [64, 64, 64, 1], [R, R, R, S], compute="bfloat16"), 1, 10, 64)
    out = (C.c_int32 * 4)()            # (fewer fields than the plan has: BORE_E_INVALID)
    assert _lib.lib().bore_fit_plan_query(C.byref(desc), 1, 10, 64, 0, 0, 256, out, 4) == -1
