"""The device L-BFGS-B restarts at every kind of maxcor -- 1, odd, above 10, 32 -- on every restart kernel.

maxcor is the workspace layout (lbfgsb::make_work), the LDS carve, how many problems share a workgroup, which kernel is
launched, whether the matrix pool is used and how many waves a streamed kernel gives a problem; before this file the
device only ever ran 2, 4 and 10.  The bar is the standing one: every record -- x, fun, jac, nit, nfev, status, task --
equals the HOST build of lbfgsb.h fed the device's own f and g, bit for bit, no tolerance.

A case tests the history's wrap-around only if a search outlasts the history: the cases marked `premise` assert that at
least two of their restarts end with nit > maxcor.  Their networks were chosen on the CPU (oracle f/g, host build): two
variables or relu + sigmoid end within a dozen iterations, sixteen inputs with tanh (weights scaled up) or relu layers
under a linear output run past 32.  maxiter = min(2 maxcor + 8, 72), starts from U(-0.1, 1.1), ftol = 1e-9; the host
reference pays one launch per evaluation, hence at most two models and nine starts (thirteen for twelve waves)."""

import numpy as np
import pytest
import torch

import lbfgsb_host as H
import test_acq_plan_host as P
import test_gpu_lstm_acq as LA
import test_gpu_stream_acq as SA
from bore_amd import _lib, ops
from test_gpu_argmax import dev, pack, rand_model
from test_gpu_stream_acq import same_record

pytestmark = pytest.mark.gpu

KNOBS = ["BORE_LBFGSB_COOP_GRID", "BORE_LBFGSB_WAVES", "BORE_LBFGSB_BIG", "BORE_LBFGSB_QUEUE", "BORE_LBFGSB_OCC2"]
RELU3, TANH3, TANH4 = ["relu", "relu", "sigmoid"], ["tanh", "tanh", "linear"], ["tanh"] * 3 + ["linear"]
# name: (D, units, activations, compute, transform, seed, weight scale, models)
NETS = {
    "2-16-16-1": (2, [16, 16, 1], RELU3, "float32", "identity", 1, 1.0, 2),
    "5-24-12-1": (5, [24, 12, 1], TANH3, "float32", "identity", 2, 8.0, 1),
    "16-24-12-1": (16, [24, 12, 1], TANH3, "float32", "identity", 6, 4.0, 1),
    "6-32-32-1": (6, [32, 32, 1], TANH3, "float32", "identity", 3, 6.0, 1),
    "16-64-64-64-1": (16, [64, 64, 64, 1], ["relu"] * 3 + ["linear"], "float32", "sigmoid", 16, 1.0, 1),
    "16-64-64-64-1 bf16": (16, [64, 64, 64, 1], ["relu"] * 3 + ["linear"], "bfloat16", "sigmoid", 16, 1.0, 1),
    "32-128-128-1 bf16": (32, [128, 128, 1], ["relu", "relu", "linear"], "bfloat16", "sigmoid", 9, 1.0, 1),
    "8-256-256-1": (8, [256, 256, 1], ["relu", "elu", "linear"], "float32", "sigmoid", 7, 1.0, 1),
    "5-7-3-1": (5, [7, 3, 1], ["tanh", "sigmoid", "linear"], "float32", "sigmoid", 101, 1.0, 2),
}
R_DRAWN = 13


def opts_for(maxcor):
    return dict(maxcor=maxcor, maxiter=min(2 * maxcor + 8, 72), ftol=1e-9)


@pytest.fixture
def knobs(monkeypatch):
    def setting(**values):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in values.items():
            monkeypatch.setenv("BORE_LBFGSB_" + k, str(v))
    setting()
    return setting


_cases, _host = {}, {}


def case(name, D=None):
    """(desc, theta, X0 [models][R_DRAWN][D], lo, hi, transform) of NETS[name] -- `D`: the D -> 16-1 net of the dimension's
    edges.  Made once; nobody writes to it."""
    key = (name, D)
    if key not in _cases:
        Dn, units, acts, compute, tr, seed, scale, L = NETS[name] if D is None else (D, [16, 1], ["tanh", "linear"], "float32",
                                                                                      "identity", 200 + D, 3.0, 1)
        rs = np.random.RandomState(seed)
        models = [rand_model(rs, Dn, units) for _ in range(L)]
        for p in models:
            for i in range(0, len(p), 2):
                p[i] *= np.float32(scale)
        X0 = rs.uniform(-0.1, 1.1, size=(L, R_DRAWN, Dn))
        _cases[key] = (_lib.make_desc(Dn, units, acts, compute=compute), dev(np.stack([pack(p) for p in models])), X0,
                       np.zeros(Dn), np.ones(Dn), tr)
    return _cases[key]


def host_records(key, maxcor, R, streamed=None):
    """The host build's record of restarts 0..R-1 of every model of case `key` at `maxcor`, fed the device's f and g
    (`streamed`: the streamed kernels', True = by the switch for a network that fits LDS).  Computed once per start."""
    desc, th, X0, lo, hi, tr = case(*key)
    out = []
    for l in range(X0.shape[0]):
        if streamed is None:
            def fg(xx, l=l):
                v, g = ops.mlp_value_and_input_grad(desc, th[l:l + 1], dev(np.atleast_2d(xx)[None]), tr, True)
                return v.cpu().numpy()[0], g.cpu().numpy()[0]
        else:
            fg = SA.fg_of(desc, th[l:l + 1], tr, streamed)
        for r in range(R):
            k = (key, maxcor, streamed, l, r)
            if k not in _host:
                _host[k] = H.minimize(lambda xx: tuple(a[0] for a in fg(xx)), X0[l, r], (lo, hi), **opts_for(maxcor))
        out.append([_host[(key, maxcor, streamed, l, r)] for r in range(R)])
    return out


def check(key, maxcor, R, premise=False, streamed=None, where=()):
    """One launch of R restarts per model at `maxcor` against the host build; returns info."""
    desc, th, X0, lo, hi, tr = case(*key)
    X = np.ascontiguousarray(X0[:, :R])
    entry = ops.lbfgsb_minimize if streamed is None else ops.stream_lbfgsb_minimize
    x, fun, jac, info = ops.lbfgsb_results_to_host(*entry(desc, th, dev(X), lo, hi, tr, True, **opts_for(maxcor)))
    host = host_records(key, maxcor, R, streamed)
    for l in range(X.shape[0]):
        for r in range(R):
            same_record(host[l][r], x[l, r], fun[l, r], jac[l, r], info[l, r], (key, maxcor, l, r) + tuple(where))
    long_ones = int((info[:, :, 0] > maxcor).sum())
    print("%s maxcor %d %s: nit %s; %d restarts outlast the history" % (key, maxcor, where, info[:, :, 0].tolist(), long_ones))
    if premise:
        assert long_ones >= 2, (key, maxcor, info[:, :, 0].tolist())
    return info


def plan(key, maxcor, R):
    """bore_lbfgsb_plan_query for the launch `check` makes under the knobs set now: the plan, held to the contract of
    tests/test_acq_plan_host.py first."""
    desc, th, X0 = case(*key)[:3]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    req, rc, out = P.plans(desc, [(X0.shape[0], R, maxcor, cus, 0, 1)])
    assert rc[0] == 0, _lib.lib().bore_last_error()
    bad = P.violations(desc, req, rc, out)[0]
    assert not any(m.any() for m in bad.values()), {k: bool(m.any()) for k, m in bad.items()}
    return dict(zip(P.FIELDS, out[0].tolist()))


# ---- the four-wave kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxcor", [1, 3, 5, 11, 17, 31, 32])
def test_four_wave_static_kernel(gpu, knobs, maxcor):
    """2->16-16-1 (static shape 1), two models x three restarts.  At maxcor 32 two workspaces fit beside the weights:
    the third restart goes to a second workgroup."""
    p = plan(("2-16-16-1",), maxcor, 3)
    assert p["kernel"] == P.W4_F32 and p["flavour"] == 1
    if maxcor == 32:
        assert (p["slots"], p["PB"], p["blocks"], p["queue"]) == (2, 2, 2, 0)
    check(("2-16-16-1",), maxcor, 3)


@pytest.mark.parametrize("maxcor", [11, 32])
def test_four_wave_static_kernel_with_searches_that_outlast_the_history(gpu, knobs, maxcor):
    """Two variables under relu + sigmoid end within a dozen iterations: the premise of the four-wave float32 family
    sits at sixteen inputs, 16->64-64-64-1 held to four waves."""
    knobs(WAVES=4)
    assert plan(("16-64-64-64-1",), maxcor, 3)["kernel"] == P.W4_F32
    check(("16-64-64-64-1",), maxcor, 3, premise=True)


@pytest.mark.parametrize("maxcor", [1, 3, 5, 11, 17, 31, 32])
def test_run_time_layout_kernel(gpu, knobs, maxcor):
    """5->24-12-1, tanh layers under a linear output, weights x 8: five variables outlast 11 and 17 corrections, not 32
    (the 16-input case below)."""
    p = plan(("5-24-12-1",), maxcor, 5)
    assert p["kernel"] == P.W4_F32 and p["flavour"] == -3
    check(("5-24-12-1",), maxcor, 5, premise=maxcor in (11, 17))


def test_run_time_layout_kernel_at_maxcor_32_with_searches_that_outlast_it(gpu, knobs):
    assert plan(("16-24-12-1",), 32, 5)["flavour"] == -3
    check(("16-24-12-1",), 32, 5, premise=True)


@pytest.mark.parametrize("maxcor", [3, 11])
def test_lane_per_problem(gpu, knobs, maxcor):
    knobs(COOP_GRID=0)
    p = plan(("6-32-32-1",), maxcor, 9)
    assert p["kernel"] == P.W4_F32 and p["queue"] == 0 and p["PB"] == 9 and p["slots"] == 9      # (nine lanes' problems)
    check(("6-32-32-1",), maxcor, 9, premise=True)


# ---- the two launches lbfgsb_plan used to carve wrongly -------------------------------------------------------------
def test_former_miscarve_queue_over_two_slots(gpu, knobs):
    """2->16-16-1, one model, five restarts, maxcor 32, BORE_LBFGSB_QUEUE=1: planned slots=2 PB=5 queue=1 on four waves
    -- waves 2 and 3 in blocks that were never carved.  Now one workgroup per two restarts, no queue."""
    knobs(QUEUE=1)
    desc, th, X0, lo, hi, tr = case(("2-16-16-1"))
    key = ("2-16-16-1 one model",)
    _cases[key + (None,)] = (desc, th[:1], X0[:1], lo, hi, tr)
    p = plan(key, 32, 5)
    print("former miscarve, float32:", p)
    assert p["kernel"] == P.W4_F32 and (p["slots"], p["waves"], p["PB"], p["queue"], p["blocks"]) == (2, 4, 2, 0, 3)
    check(key, 32, 5)


@pytest.mark.parametrize("big", [None, 1])
def test_former_miscarve_pool_on_the_four_wave_kernel(gpu, knobs, big):
    """32->128-128-1 in bfloat16, maxcor 32, nine restarts, BORE_LBFGSB_WAVES=8 (BORE_LBFGSB_BIG unset and 1): pooled
    onto lbfgsb_kernel<4,bf16>, whose body has no pool.  Now the four-wave kernel over blocks that hold the matrices."""
    knobs(WAVES=8, **({} if big is None else dict(BIG=big)))
    p = plan(("32-128-128-1 bf16",), 32, 9)
    print("former miscarve, bfloat16:", p)
    assert p["kernel"] == P.W4_BF16 and p["pool_doubles"] == 0 and p["slots"] <= 4
    check(("32-128-128-1 bf16",), 32, 9, premise=True, where=("BIG", big))


# ---- two workgroups per CU, twelve and eight waves, the queue --------------------------------------------------------
@pytest.mark.parametrize("maxcor", [5, 15, 17])
def test_two_workgroups_per_cu(gpu, knobs, maxcor):
    """BORE_LBFGSB_OCC2=1 takes the two-per-CU kernel where two workgroups' LDS fit a CU: at maxcor 5 and 15 (76 KB), not
    at 17 (four workspaces of 20 KB), where the forced choice falls back to the one-per-CU kernel -- same bits."""
    knobs(OCC2=1)
    p = plan(("6-32-32-1",), maxcor, 5)
    assert p["kernel"] == (P.OCC2 if p["lds_floats"] * 4 <= P.LDS_BYTES // 2 else P.W4_F32)
    assert (p["kernel"] == P.OCC2) == (maxcor < 17)
    check(("6-32-32-1",), maxcor, 5, premise=maxcor >= 15)


@pytest.mark.parametrize("maxcor", [5, 11, 17])
def test_twelve_waves(gpu, knobs, maxcor):
    """Thirteen restarts: twelve waves and a second workgroup -- or, past the maxcor at which twelve workspaces no
    longer fit beside the weights, as many waves as do."""
    knobs(WAVES=12)
    p = plan(("6-32-32-1",), maxcor, 13)
    fit = (P.LDS_BYTES // 4 - (p["lds_floats"] - p["slots"] * p["prob_floats"])) // p["prob_floats"]
    assert p["kernel"] == P.W12 and p["waves"] == p["slots"] == min(12, fit), (p, fit)
    print("twelve waves asked at maxcor %d: %d launched" % (maxcor, p["waves"]))
    if maxcor == 17:
        assert p["waves"] < 12
    check(("6-32-32-1",), maxcor, 13, premise=maxcor >= 11)


@pytest.mark.parametrize("maxcor", [5, 11])
def test_eight_waves_float32(gpu, knobs, maxcor):
    knobs(WAVES=8)
    p = plan(("16-64-64-64-1",), maxcor, 9)
    assert p["kernel"] == P.W8_F32 and 4 < p["waves"] <= 8
    check(("16-64-64-64-1",), maxcor, 9, premise=maxcor == 11)


@pytest.mark.parametrize("maxcor", [5, 11])
@pytest.mark.parametrize("name,big", [("16-64-64-64-1 bf16", None), ("32-128-128-1 bf16", 0), ("32-128-128-1 bf16", 1)])
def test_eight_waves_bfloat16(gpu, knobs, name, big, maxcor):
    """Both wide shapes; 32->128-128-1 with the optimiser's matrices in LDS and in the device pool (an odd maxcor there:
    zero_big's pairs over 2m (2m + 1) doubles, a pool slot's eight strides of big_wave doubles)."""
    knobs(WAVES=8, **({} if big is None else dict(BIG=big)))
    p = plan((name,), maxcor, 9)
    assert p["kernel"] == P.W8_BF16 and 4 < p["waves"] <= 8 and (p["pool_doubles"] > 0) == (big == 1), p
    check((name,), maxcor, 9, premise=maxcor == 11 and name.startswith("32"), where=("BIG", big))


def test_queue_with_slot_reuse(gpu, knobs):
    knobs(QUEUE=1)
    p = plan(("6-32-32-1",), 11, 9)
    assert p["queue"] == 1 and p["blocks"] == 1 and p["PB"] == 9 and p["slots"] == 4      # (waves take a second and third problem)
    check(("6-32-32-1",), 11, 9, premise=True)


# ---- the streamed kernels -------------------------------------------------------------------------------------------
def streamed_waves(D, maxcor, lstm=False):
    """How many of its four waves bore_stream_lbfgsb_minimize (bore_lstm_stream_lbfgsb_minimize) gives a problem: the
    workspaces that fit the LDS beside the panels.  sizeof(StreamLds): a[2][64 x 34], b[2][32 x 144] floats, the layout
    (BORE_LAYOUT_FLOATS, read off a plan), pre[10], zt[64], red[4]; lbfgsb::State is 328 bytes.  The sizes are exact to
    a few hundred bytes; the callers assert that the answer does not hinge on 2 KB."""
    p = P.plans(P.make(P.DUMP_NETS["2-16-16-1"]), [(1, 1, 10, 256, 0, 1)])[2][0]
    layout_floats = int(p[P.FIELDS.index("lds_floats")] - p[P.FIELDS.index("o_layout")])
    stream_lds = 4 * (2 * 64 * 34 + 2 * 32 * 144 + layout_floats + 10 + 64 + 4)
    box = 4 * (4 * ((D + 1) & ~1) + ((D + 3) & ~3) + 4)
    prob = 4 * (84 + 2 * H.layout(D, maxcor)[2] + ((3 * D + 3) & ~3))
    room = 163840 - stream_lds - (256 if lstm else 0) - 64 - box
    assert min(4, (room - 2048) // prob) == min(4, (room + 2048) // prob), (D, maxcor)
    return min(4, room // prob)


@pytest.mark.parametrize("maxcor", [1, 5, 11, 32])
@pytest.mark.parametrize("name", ["8-256-256-1", "5-7-3-1"])
def test_streamed_dense(gpu, knobs, name, maxcor):
    """Five restarts.  At maxcor 32 a problem's workspace is 66 KB: one of the four waves holds a problem and walks the
    five.  Five and eight variables do not outlast 32 corrections (the 16-input case below)."""
    waves = streamed_waves(NETS[name][0], maxcor)
    assert waves == (1 if maxcor == 32 else 4)
    check((name,), maxcor, 5, premise=maxcor == 11 and name == "8-256-256-1", streamed=NETS[name][1][0] < 256)


def test_streamed_dense_at_maxcor_32_with_searches_that_outlast_it(gpu, knobs):
    assert streamed_waves(16, 32) == 1
    check(("16-24-12-1",), 32, 5, premise=True, streamed=True)


LSTM_SMALL = (3, 1, 7, "relu", 4)          # (the smallest shape of tests/test_gpu_lstm_acq.py)
LSTM_LONG = (48, 2, 32, "elu", 5)          # (its streamed-only shape: the plugin's widths)


def check_lstm(shape, maxcor, seed, scale, tr, premise):
    D, L, Hn, act, T = shape
    rs, desc, th = LA.make(shape, 1, seed)
    th = (th.double() * scale).float()
    X0 = rs.uniform(-0.1, 1.1, size=(1, 5, D))
    lo, hi = np.zeros(D), np.ones(D)
    x, fun, jac, info = LA.run(desc, th, X0, lo, hi, T, tr, **opts_for(maxcor))
    for r in range(5):
        same_record(LA.host(desc, th, T, tr, X0[0, r], lo, hi, **opts_for(maxcor)), x[0, r], fun[0, r], jac[0, r],
                    info[0, r], (shape, maxcor, r))
    long_ones = int((info[:, :, 0] > maxcor).sum())
    print("lstm %s maxcor %d: nit %s" % (shape, maxcor, info[0, :, 0].tolist()))
    if premise:
        assert long_ones >= 2, info[0, :, 0].tolist()


@pytest.mark.parametrize("maxcor", [5, 11, 32])
def test_streamed_lstm(gpu, knobs, maxcor):
    """Three variables end within ten iterations (the 48-input case below holds the premises)."""
    assert streamed_waves(3, maxcor, lstm=True) == (1 if maxcor == 32 else 4)
    check_lstm(LSTM_SMALL, maxcor, 100, 1.0, "sigmoid", False)


@pytest.mark.parametrize("maxcor", [11, 32])
def test_streamed_lstm_with_searches_that_outlast_the_history(gpu, knobs, maxcor):
    assert streamed_waves(48, maxcor, lstm=True) == (1 if maxcor == 32 else 4)
    check_lstm(LSTM_LONG, maxcor, 2, 1.5, "identity", True)


# ---- the dimension's edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,maxcor", [(1, 5), (1, 10), (63, 5), (63, 10), (64, 5), (64, 10), (33, 11)])
def test_the_dimensions_edges(gpu, knobs, D, maxcor):
    """D -> 16-1 (tanh, linear) on the LDS kernel and streamed: one variable; 63 and 64 -- the first time a
    lane-per-variable loop has no idle lane --; 33 with maxcor 11: both odd, so is m n."""
    assert plan(("edge", D), maxcor, 5)["flavour"] == -2
    check(("edge", D), maxcor, 5)
    check(("edge", D), maxcor, 5, streamed=True)


# ---- the engines take maxcor from the same options: the lock-step chain, and the fused loop kernel -----------------------
@pytest.mark.parametrize("maxcor", [5, 17])
def test_native_engine_equals_python_engine_at_other_maxcor(gpu, knobs, maxcor):
    """NativeEngine on the lock-step schedule (groups=3: the stand-alone kernels) and on the asynchronous one (the fused
    loop kernel, whose restart phase is planned in batch mode: one workgroup per loop) against ReplicaEngine."""
    from bore_amd.engine import NativeEngine, ReplicaEngine
    kw = dict(epochs=20, num_samples=64, deduplicate=True, options=dict(maxiter=1000, ftol=1e-9, maxcor=maxcor))
    a = NativeEngine(np.arange(3, 14), groups=3, **kw)
    b = ReplicaEngine(np.arange(3, 14), mode="device", groups=2, **kw)
    a.run(6)
    b.run(6)
    Xa, ya = a.observations()
    assert Xa.shape == (11, 16, 2)
    assert np.array_equal(Xa, b.X) and np.array_equal(ya, b.y)
    th, m, v, t = a.state()
    assert np.array_equal(th, b.theta.cpu().numpy()) and np.array_equal(v, b.adam_v.cpu().numpy())
    assert a.take_stats()["n_fg_rows"] == b.stats["n_fg_rows"]
    f = NativeEngine(np.arange(3, 14), async_loops=True, **kw)
    f.run(6)
    Xf, yf = f.observations()
    assert np.array_equal(Xf, b.X) and np.array_equal(yf, b.y)
    th, m, v, t = f.state()
    assert np.array_equal(th, b.theta.cpu().numpy()) and np.array_equal(v, b.adam_v.cpu().numpy())
    st = f.take_stats()
    assert st["fit_ms"] == 0.0 and st["phase_iterations"] == 11 * 6          # the fused kernel ran
    assert st["n_fg_requests"] == b.stats["n_fg_rows"]                        # (n_fg_rows: less what the image shortcut served)
    for eng in (a, f):
        eng.close()
