"""The restart launch as lbfgsb_plan carves it, against what lbfgsb_body and the restart kernels index (no GPU).

bore_lbfgsb_plan_query returns the plan of a request as integers.  Every assertion below is written from the kernel's
side (bore_amd/csrc/bore_argmax.hip: lbfgsb_body, the lbfgsb_kernel* launch bounds), not from the planner's: a plan that
passes hands no wave a workspace outside the launch's LDS, whatever maxcor (1..32), network, number of models and of
restarts, batch mode, CU count and BORE_LBFGSB_* knobs it was made for."""
import ctypes as C
import itertools

import numpy as np
import pytest

import lbfgsb_host as H
from bore_amd import _lib

FIELDS = ("kernel flavour slots waves blocks lds_floats pool_doubles PB queue o_tile o_vals o_box o_prob o_state o_dw o_iw "
          "o_res o_queue o_layout prob_floats total").split()
W4_F32, W4_BF16, OCC2, W8_F32, W8_BF16, W12 = range(6)          # RestartKernel
LAUNCH_BOUND = np.array([4, 4, 4, 8, 8, 12])                    # waves: __launch_bounds__ of lbfgsb_kernel{,_occ2,_w8,_w12}
LDS_BYTES = 163840
KNOBS = ["BORE_LBFGSB_COOP_GRID", "BORE_LBFGSB_WAVES", "BORE_LBFGSB_BIG", "BORE_LBFGSB_QUEUE", "BORE_LBFGSB_OCC2"]

STARTS = [1, 3, 4, 5, 8, 12, 13, 16, 17, 21, 70, 1024]          # (tests/native/acq_plan_dump.hip: kStarts)
MODELS = [1, 3, 64, 65, 256, 1024]
MAXCOR = list(range(1, 33))
R, S, E, T, LIN = "relu", "sigmoid", "elu", "tanh", "linear"
# the ten networks of tests/native/acq_plan_dump.hip ...
DUMP_NETS = {
    "2-16-16-1": (2, [16, 16, 1], R, S), "6-32-32-1": (6, [32, 32, 1], R, S),
    "16-64-64-64-1": (16, [64, 64, 64, 1], R, S), "32-128-128-1": (32, [128, 128, 1], R, S),
    "16-32-32-32-1": (16, [32, 32, 32, 1], E, LIN), "9-32-32-32-1": (9, [32, 32, 32, 1], E, LIN),
    "5-24-12-1": (5, [24, 12, 1], R, S), "10-48-1": (10, [48, 1], R, LIN),
    "8-176-176-1": (8, [176, 176, 1], R, S), "2-16-16-2": (2, [16, 16, 2], R, S),
}
# ... and float32 run-time layouts whose weights leave room for three, two and one problem at maxcor 10 (found with the
# query, walking down from 64->128-128-1 and 8->150-150-1, which are refused: test_the_tight_networks_are_tight pins it)
TIGHT_NETS = {"8-72-72-1": (8, [72, 72, 1], R, S), "8-100-100-1": (8, [100, 100, 1], R, S),
              "64-104-104-1": (64, [104, 104, 1], R, S)}
TIGHT_SLOTS = {"8-72-72-1": 3, "8-100-100-1": 2, "64-104-104-1": 1}
# the knob settings of the dump (the values the GPU tests use), at maxcor 10 ...
SETTINGS = [
    dict(COOP_GRID=4194304), dict(COOP_GRID=0), dict(OCC2=0), dict(OCC2=1), dict(WAVES=4), dict(WAVES=8), dict(WAVES=12),
    dict(QUEUE=0), dict(QUEUE=3), dict(QUEUE=7), dict(QUEUE=7, WAVES=8, OCC2=1), dict(QUEUE=7, WAVES=8, BIG=1),
    dict(QUEUE=0, WAVES=8, BIG=1), dict(QUEUE=7, WAVES=8, BIG=0), dict(QUEUE=7, WAVES=12), dict(QUEUE=0, WAVES=12),
    dict(QUEUE=5, WAVES=4, OCC2=1), dict(BIG=0), dict(BIG=1),
    dict(COOP_GRID=0, WAVES=12, QUEUE=7, OCC2=1, BIG=1),
]
# ... and the two that force a carve or a queue, at every maxcor (with and without the eight-wave kernel forced)
SETTINGS_EVERY_MAXCOR = [dict(BIG=1), dict(QUEUE=1), dict(BIG=1, WAVES=8), dict(QUEUE=1, WAVES=8), dict(BIG=1, QUEUE=1)]

_DWORK = {}


def dwork_size(D, m, outside):
    """lbfgsb::dwork_size, asked of the host build of the same header."""
    key = (D, m, bool(outside))
    if key not in _DWORK:
        _DWORK[key] = H.layout(D, m, outside)[2]
    return _DWORK[key]


def make(net, compute="float32"):
    D, units, hidden, out = net
    return _lib.make_desc(D, units, [hidden] * (len(units) - 1) + [out], compute=compute)


def plans(desc, requests):
    """bore_lbfgsb_plan_query for every (n_models, num_starts, maxcor, cus, batch, many_waves) of `requests`:
    (requests as an int array [n][6], rc [n], fields [n][21])."""
    L = _lib.lib()
    req = np.asarray(list(requests), dtype=np.int64).reshape(-1, 6)
    out = np.zeros((len(req), len(FIELDS)), dtype=np.int32)
    rc = np.zeros(len(req), dtype=np.int64)
    row = (C.c_int32 * len(FIELDS))()
    query, ref = L.bore_lbfgsb_plan_query, C.byref(desc)
    for i, (nm, rs, m, cus, batch, mw) in enumerate(req.tolist()):
        rc[i] = query(ref, nm, rs, m, cus, batch, mw, row, len(FIELDS))
        out[i] = row
    return req, rc, out


def violations(desc, req, rc, out):
    """{contract item: boolean mask over the planned (rc 0) requests that break it}, and the requests planned."""
    ok = rc == 0
    req, out = req[ok], out[ok].astype(np.int64)
    f = dict(zip(FIELDS, out.T))
    Rr, m, batch = req[:, 1], req[:, 2], req[:, 4] != 0
    D = desc.input_dim
    np_ = np.minimum(f["PB"], Rr)                       # lbfgsb_body: problems of a full workgroup
    queue = f["queue"] != 0
    # (lbfgsb_body: BIG_OK = ALWAYS_COOP && SHAPE == 4, compiled for bfloat16 in lbfgsb_kernel_w8 alone; a.big != NULL
    # exactly when the plan asks for a pool)
    uses_pool = (f["kernel"] == W8_BF16) & (f["flavour"] == 4) & (f["pool_doubles"] > 0)
    dw = np.array([dwork_size(D, int(mi), bool(pi)) for mi, pi in zip(m, uses_pool)], dtype=np.int64).reshape(-1)
    bad = {}
    # 1. LDS bounds and order (the regions lbfgsb_body addresses from smem)
    bad["1 LDS bounds and order"] = ~((f["lds_floats"] * 4 <= LDS_BYTES) & (f["total"] <= f["lds_floats"])
                                      & (f["o_tile"] <= f["o_vals"]) & (f["o_vals"] < f["o_box"]) & (f["o_box"] < f["o_prob"])
                                      & (f["o_prob"] < f["o_res"]) & (f["o_res"] <= f["o_queue"])
                                      & (f["o_queue"] < f["o_layout"])
                                      & (f["o_prob"] + f["slots"] * f["prob_floats"] <= f["o_res"])
                                      & (f["o_queue"] + 3 <= f["total"])          # (qnext[0..2])
                                      # batch mode: res [multi ? np : 4][D + 3] doubles, cnt[4], execs[np]
                                      & (~batch | (f["o_res"] + 2 * np.maximum(np_, 4) * (D + 3) + 4 + np_ <= f["o_queue"])))
    # 2. the problem block holds what make_work lays into it (base + o_dw: doubles; base + o_iw: 3 D ints)
    bad["2 problem block size"] = ~((f["prob_floats"] >= 2 * dw + 3 * D) & (f["o_iw"] == 2 * dw)
                                    & (f["o_dw"] + 2 * dw <= f["o_iw"])
                                    & ((f["pool_doubles"] == 0)
                                       | (uses_pool & (f["pool_doubles"] == 8 * 2 * m * (2 * m + 1)))))
    # 3. every slot index a wave forms is below `slots` (queue: slot wv for wv < min(NW, np); else slot myp < np)
    bad["3 slot indices"] = ~np.where(queue, np.minimum(f["waves"], np_) <= f["slots"], np_ <= f["slots"])
    # 4. launch bounds; the ALWAYS_COOP kernels carry no lane-per-problem loop; that loop's map is four waves x 16 lanes
    coop_only = np.isin(f["kernel"], [OCC2, W8_F32, W8_BF16, W12])
    bad["4 launch bounds"] = ~((f["waves"] >= 1) & (f["waves"] <= LAUNCH_BOUND[f["kernel"]])
                               & (~coop_only | (np_ <= f["waves"]) | queue)
                               & (coop_only | queue | batch | (np_ <= f["waves"]) | ((f["waves"] == 4) & (np_ <= 64)))
                               & (~batch | ((f["waves"] == 4) & (np_ <= 16))))
    # 5. alignment: float4 zeroing of a slot, fp64 regions on 16 bytes, the int workspace on 8
    bad["5 alignment"] = ~((f["o_box"] % 4 == 0) & (f["o_prob"] % 4 == 0) & (f["prob_floats"] % 4 == 0)
                           & (f["o_dw"] % 4 == 0) & (f["o_iw"] % 2 == 0))
    # 6. the grid covers every restart exactly once; batch mode keeps a loop in one workgroup
    bad["6 grid"] = ~(((f["blocks"] - 1) * f["PB"] < Rr) & (Rr <= f["blocks"] * f["PB"]) & (f["blocks"] <= 65535)
                      & (f["blocks"] >= 1) & (~batch | (f["PB"] >= Rr)))
    return bad, req, out


COUNTS = {}


def check(desc, requests, label):
    req, rc, out = plans(desc, requests)
    bad, req_ok, out_ok = violations(desc, req, rc, out)
    for item, mask in bad.items():
        COUNTS[item] = COUNTS.get(item, 0) + int(mask.sum())
    COUNTS["plans"] = COUNTS.get("plans", 0) + len(req_ok)
    COUNTS["refused"] = COUNTS.get("refused", 0) + int((rc != 0).sum())
    print("%s: %d planned, %d refused; violations %s"
          % (label, len(req_ok), int((rc != 0).sum()), {k: int(v.sum()) for k, v in bad.items() if v.any()}))
    for item, mask in bad.items():
        first = [dict(zip("n_models num_starts maxcor cus batch many_waves".split(), req_ok[i].tolist()),
                      **dict(zip(FIELDS, out_ok[i].tolist()))) for i in np.flatnonzero(mask)[:2]]
        assert not mask.any(), (label, item, int(mask.sum()), first)
    return req, rc, out


@pytest.fixture
def knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)

    def setting(values):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in values.items():
            monkeypatch.setenv("BORE_LBFGSB_" + k, str(v))
    return setting


def grid(models=MODELS, starts=STARTS, maxcor=MAXCOR, cus=(8, 256), modes=((0, 1), (1, 0), (0, 0), (1, 1))):
    return [(nm, rs, m, c, b, mw) for nm, rs, m, c, (b, mw) in itertools.product(models, starts, maxcor, cus, modes)]


ALL_NETS = dict(DUMP_NETS, **TIGHT_NETS)


@pytest.mark.parametrize("compute", ["float32", "bfloat16"])
@pytest.mark.parametrize("name", list(ALL_NETS))
def test_every_plan_meets_what_the_kernels_index(name, compute, knobs):
    """Knobs unset: maxcor 1..32 x n_models x num_starts x batch mode off / on x with / without the many-wave kernels
    x 8 / 256 CUs."""
    check(make(ALL_NETS[name], compute), grid(), "%s %s" % (name, compute))


@pytest.mark.parametrize("D0", [1, 17, 33, 49])
def test_every_plan_of_a_run_time_net_of_every_input_dimension(D0, knobs):
    """D -> 16-1 (tanh, linear) for every D in 1..64: the problem's dimension is the other size the workspace layout
    depends on (odd n pads every vector; m n odd pads the history)."""
    for D in range(D0, D0 + 16):
        for compute in ("float32", "bfloat16"):
            check(make((D, [16, 1], T, LIN), compute), grid(cus=(256,), modes=((0, 1), (1, 0))), "%d-16-1 %s" % (D, compute))


@pytest.mark.parametrize("name", list(ALL_NETS))
def test_every_plan_under_the_forced_choices(name, knobs):
    """The knob settings the GPU tests use, at maxcor 10; BORE_LBFGSB_BIG=1 and BORE_LBFGSB_QUEUE=1 -- the two that
    force a carve and a queue -- at every maxcor."""
    for compute in ("float32", "bfloat16"):
        desc = make(ALL_NETS[name], compute)
        for values in SETTINGS:
            knobs(values)
            check(desc, grid(maxcor=[10], cus=(256,), modes=((0, 1),)), "%s %s %s" % (name, compute, values))
        for values in SETTINGS_EVERY_MAXCOR:
            knobs(values)
            check(desc, grid(cus=(256,), modes=((0, 1),)), "%s %s %s" % (name, compute, values))


def test_the_tight_networks_are_tight(knobs):
    """The premise of the two extra networks: float32, run-time layout, and at the default maxcor their weights leave
    room for one to three workspaces -- fewer than the four waves of their kernel -- while many restarts and many
    models would have the planner queue."""
    for name, net in TIGHT_NETS.items():
        req, rc, out = plans(make(net), grid(maxcor=[10], cus=(256,), modes=((0, 1),)))
        assert (rc == 0).all(), name
        f = dict(zip(FIELDS, out.T))
        assert (f["flavour"] <= 0).all() and (f["kernel"] == W4_F32).all(), name
        assert (f["slots"] == np.minimum(req[:, 1], TIGHT_SLOTS[name])).all(), (name, sorted(set(f["slots"].tolist())))
        assert (f["queue"] == 0).all() and (f["PB"] <= f["slots"]).all()      # (no queue below four slots)
        assert (f["blocks"] == -(-req[:, 1] // f["PB"])).all()


def test_the_recorded_miscarves_are_gone(knobs):
    """The two requests the issue names.  32->128-128-1 in bfloat16 at maxcor 32 pooled (PB2 > PB) onto the four-wave
    kernel, whose body has no pool; 2->16-16-1 at maxcor 32 with 3 models x 1024 restarts queued four waves onto two
    slots.  Now: no pool at four slots or fewer, forced or not; no queue below four slots."""
    wide = make(DUMP_NETS["32-128-128-1"], "bfloat16")
    for big in (None, 1):
        knobs({} if big is None else dict(BIG=big))
        _, rc, out = plans(wide, [(64, 17, 32, 256, 0, 1)])
        p = dict(zip(FIELDS, out[0].tolist()))
        assert rc[0] == 0 and p["kernel"] == W4_BF16 and p["pool_doubles"] == 0 and p["slots"] <= 4, p
        assert p["prob_floats"] >= 2 * dwork_size(32, 32, False) + 96
    knobs({})
    _, rc, out = plans(make(DUMP_NETS["2-16-16-1"]), [(3, 1024, 32, 256, 0, 1)])
    p = dict(zip(FIELDS, out[0].tolist()))
    assert rc[0] == 0 and (p["slots"], p["waves"], p["PB"], p["queue"], p["blocks"]) == (2, 4, 2, 0, 512), p
    # the pool is still taken where it yields more than four slots (the eight-wave kernel, maxcor 10: eight)
    _, rc, out = plans(wide, [(64, 17, 10, 256, 0, 1)])
    p = dict(zip(FIELDS, out[0].tolist()))
    assert rc[0] == 0 and p["kernel"] == W8_BF16 and p["slots"] == 8 and p["pool_doubles"] == 8 * 20 * 21, p


def test_the_query_refuses_like_the_entry_point(knobs):
    L = _lib.lib()
    d = make(DUMP_NETS["2-16-16-1"])
    row = (C.c_int32 * len(FIELDS))()

    def ask(desc=d, n_models=1, num_starts=4, maxcor=10, cus=256, batch=0, many=1, n_out=len(FIELDS)):
        rc = L.bore_lbfgsb_plan_query(C.byref(desc), n_models, num_starts, maxcor, cus, batch, many, row, n_out)
        return rc, L.bore_last_error().decode()
    assert ask()[0] == 0
    assert ask(maxcor=0) == (-2, "lbfgsb_minimize: maxcor must be 1..32")
    assert ask(maxcor=33) == (-2, "lbfgsb_minimize: maxcor must be 1..32")
    assert ask(num_starts=0) == (-1, "lbfgsb_minimize: num_starts < 1")
    assert ask(n_models=0) == (-1, "n_models must be >= 1 (got 0)")
    assert ask(desc=make((65, [16, 16, 1], R, S))) == (-2, "lbfgsb_minimize: input_dim must be 1..64")
    assert ask(num_starts=17, batch=1) == (-2, "lbfgsb_minimize: batch mode needs num_starts <= 16 in one workgroup")
    assert ask(cus=0)[0] == -1 and ask(n_out=20)[0] == -1
    assert ask(desc=make(DUMP_NETS["2-16-16-2"])) == (-1, "lbfgsb_minimize: the last Dense layer must have 1 unit")


def test_the_fused_kernels_restart_plans(knobs):
    """The batch-mode plans (a loop's restarts in one workgroup of four waves: what the fused loop kernel's restart phase
    and the asynchronous launch chain run) that tests/test_gpu_fused_options.py picks its maxcor and num_starts by: bytes
    of LDS, and where the plan stops taking the request."""
    def lds_bytes(desc, num_starts, maxcor, n_models=6):
        _, rc, out = plans(desc, [(n_models, num_starts, maxcor, 256, 1, 0)])
        f = dict(zip(FIELDS, out[0].tolist()))
        if rc[0]:
            assert rc[0] == -2
            return None
        assert (f["blocks"], f["waves"], f["PB"]) == (1, 4, num_starts) and f["flavour"] > 0, f
        return 4 * f["lds_floats"]
    small, plugin = make(DUMP_NETS["2-16-16-1"]), make(DUMP_NETS["16-32-32-32-1"])
    # 2->16-16-1, three restarts: 29 is the largest maxcor -- a whole CU's LDS, one loop per CU
    assert {m: lds_bytes(small, 3, m) for m in (3, 5, 10, 12, 13, 17, 29, 30)} == {
        3: 8256, 5: 11904, 10: 26832, 12: 35184, 13: 39936, 17: 62016, 29: 160512, 30: None}
    assert lds_bytes(small, 16, 10) == 123200
    assert lds_bytes(small, 8, 17) == 157696 and lds_bytes(small, 8, 18) is None        # the edge of that plan
    # 16->32-32-32-1, five restarts: 19 is the largest
    assert {m: lds_bytes(plugin, 5, m, 5) for m in (5, 17, 19, 20)} == {5: 39008, 17: 135968, 19: 159968, 20: None}
    assert lds_bytes(plugin, 1, 5, 5) == 20096 and lds_bytes(plugin, 16, 5, 5) == 92240
    assert all(b <= LDS_BYTES for b in (160512, 159968))
