"""The device L-BFGS-B restarts on every bound kind and through their recovery branches, on every restart kernel family.

Before this file every restart test but one posed the box [0, 1]^D: the lane-parallel nbd branches of init, projgr,
cauchy, freev and lnsrlb only ever saw nbd == 2, no problem had every side open (the branch of lbfgsb_advance that
skips cauchy and freev) or a fixed variable, and nothing recorded which recovery branch a run took.  The cases are
those of tests/lbfgsb_paths.py -- patterns a (open), b (lower even / upper odd), c (nbd 0 1 2 3 cycling), d (a fixed
variable), e (starts on corners and faces), f (hard weights), g (c with hard weights), w (b at maxcor 3) -- on one
test function per family, parametrised over the patterns.

The bar is the standing one: x, fun, jac, nit, nfev, status and task of every restart equal the HOST build of lbfgsb.h
fed the device's own f and g, bit for bit, no tolerance; every result is finite; the launch runs on the kernel its
family names (bore_lbfgsb_plan_query, held to the plan contract first).

Premises.  The host records fed the device's f and g are the very runs the device equals, so their event counters
(LB_EVENT, lbfgsb_host.minimize(events=True)) are the device's paths.  Per family, summed over its cases, each of
lbfgsb_paths.PER_FAMILY occurs at least once; over the whole file each of WHOLE_FILE does, formk_refresh also on a
many-wave family.  tests/test_lbfgsb_host.py shows on the CPU, with the oracle's f and g, that every one of them is met
three times per family.
  * clipped_start stands in for the event projected_start (prjctd): lbfgsb_init clips the start (as SciPy's wrapper does) before
    the routine's own projection sees it, so that projection never moves a point through any entry of the library
    and its event cannot occur; what is asserted is that starts outside their bounds are posed (an input condition).
  * Waived: formk_refresh on the pooled 32->128-128-1 bfloat16 family.  The CPU search (tools/lbfgsb_event_search.py,
    profiles/lbfgsb_paths/cpu_search.json) met none there; it holds on the eight-wave float32 sibling, the twelve-wave
    family and others (DESIGN.md "Restarts").
The fused loop kernel takes its box from the engine and stays out of scope."""
import json

import numpy as np
import pytest
import torch

import lbfgsb_host as H
import lbfgsb_paths as T
import test_acq_plan_host as P
import test_gpu_lstm_acq as LA
import test_gpu_lstm_shapes as LS
import test_gpu_stream_acq as SA
from bore_amd import _lib, ops
from test_gpu_lbfgsb_maxcor import knobs, same_record, streamed_waves  # noqa: F401  (knobs: a fixture)
from test_gpu_parity import dev, pack

pytestmark = pytest.mark.gpu

MANY_WAVES = ["twelve_waves", "eight_waves_float32", "eight_waves_bfloat16", "pooled_bfloat16"]
WAIVED = {"pooled_bfloat16": ["formk_refresh"]}        # (whole-file premises a family is excused from; see above)
_nets, _measured = {}, {}


def net(name, hard):
    """(desc, theta on the device [1, P]) of a net of the table at its soft or hard scale.  Made once."""
    if (name, hard) not in _nets:
        p = T.weights(name)[1 if hard else 0]
        if name == "lstm":
            D, L, Hn, act, steps = T.LSTM_SHAPE
            _nets[(name, hard)] = (LS._desc(D, Hn, L, act), LS._thetas([p]))
        else:
            D, units, acts, compute = T.NETS[name][:4]
            _nets[(name, hard)] = (_lib.make_desc(D, units, acts, compute=compute), dev(pack(p)[None]))
    return _nets[(name, hard)]


def device_fg(family, name, hard):
    """x -> (f, g) as the family's kernels evaluate them."""
    desc, th = net(name, hard)
    if name == "lstm":
        fg = LA.fg_of(desc, th, T.LSTM_SHAPE[4], T.LSTM["transform"])
    elif T.FAMILIES[family][3]:
        fg = SA.fg_of(desc, th, T.NETS[name][4], T.NETS[name][1][0] < 256)
    else:
        tr = T.NETS[name][4]

        def fg(xx):
            v, g = ops.mlp_value_and_input_grad(desc, th, dev(np.atleast_2d(xx)[None]), tr, True)
            return v.cpu().numpy()[0], g.cpu().numpy()[0]
    return lambda xx: tuple(a[0] for a in fg(xx))


def launch(family, name, X0, lo, hi, hard, maxcor):
    desc, th = net(name, hard)
    opts = T.opts_for(maxcor)
    if name == "lstm":
        return LA.run(desc, th, X0[None], lo, hi, T.LSTM_SHAPE[4], T.LSTM["transform"], **opts)
    entry = ops.stream_lbfgsb_minimize if T.FAMILIES[family][3] else ops.lbfgsb_minimize
    return ops.lbfgsb_results_to_host(*entry(desc, th, dev(X0[None]), lo, hi, T.NETS[name][4], True, **opts))


def planned(family, name, maxcor):
    """The launch runs on the family's kernel: the plan of bore_lbfgsb_plan_query under the knobs set now (the streamed
    entries have no plan: the waves they give a problem)."""
    R = T.FAMILIES[family][1]
    if T.FAMILIES[family][3]:
        assert streamed_waves(T.dim(name), maxcor, lstm=name == "lstm") == 4
        return
    desc = net(name, False)[0]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    req, rc, out = P.plans(desc, [(1, R, maxcor, cus, 0, 1)])
    assert rc[0] == 0, _lib.lib().bore_last_error()
    bad = P.violations(desc, req, rc, out)[0]
    assert not any(m.any() for m in bad.values()), {k: bool(m.any()) for k, m in bad.items()}
    p = dict(zip(P.FIELDS, out[0].tolist()))
    want = dict(four_wave_static=P.W4_F32, run_time_layout=P.W4_F32, lane_per_problem=P.W4_F32, queue=P.W4_F32,
                two_workgroups_per_cu=P.OCC2, twelve_waves=P.W12, eight_waves_float32=P.W8_F32,
                eight_waves_bfloat16=P.W8_BF16, pooled_bfloat16=P.W8_BF16)[family]
    assert p["kernel"] == want, (family, name, p)
    if family == "four_wave_static":
        assert p["flavour"] == 1
    if family == "run_time_layout":
        assert p["flavour"] == -3
    if family == "lane_per_problem":
        assert p["queue"] == 0 and p["PB"] == p["slots"] == R          # (a lane per problem)
    if family == "twelve_waves":
        assert p["waves"] == 12 and p["blocks"] == 2
    if family in ("eight_waves_float32", "eight_waves_bfloat16", "pooled_bfloat16"):
        assert p["waves"] == 8 and (p["pool_doubles"] > 0) == (family == "pooled_bfloat16")
    if family == "queue":
        assert p["queue"] == 1 and p["blocks"] == 1 and p["PB"] == R


def run_pattern(family, pattern, knobs):
    """Every launch of `pattern` of every net of `family` against the host build; the events of the host records.
    Run once per (family, pattern)."""
    if (family, pattern) in _measured:
        return _measured[(family, pattern)]
    knobs(**T.FAMILIES[family][2])
    events = {}
    for name in T.FAMILIES[family][0]:
        for pat, tag, lo, hi, X0, hard, maxcor in T.launches(family, name):
            if pat != pattern:
                continue
            planned(family, name, maxcor)
            x, fun, jac, info = launch(family, name, X0, lo, hi, hard, maxcor)
            assert np.isfinite(x).all() and np.isfinite(fun).all() and np.isfinite(jac).all(), (family, name, pat, tag)
            fg = device_fg(family, name, hard)
            for r in range(X0.shape[0]):
                h = H.minimize(fg, X0[r], (lo, hi), events=True, **T.opts_for(maxcor))
                same_record(h, x[0, r], fun[0, r], jac[0, r], info[0, r], (family, name, pat, tag, r))
                T.add_events(events, h, X0[r], lo, hi)
    _measured[(family, pattern)] = events
    return events


def family_events(family, knobs):
    total = {}
    for pattern in T.PATTERNS:
        for k, v in run_pattern(family, pattern, knobs).items():
            total[k] = total.get(k, 0) + v
    return total


@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_four_wave_static_kernel(gpu, knobs, pattern):
    """2->16-16-1 (static shape 1), nine restarts; pattern c as two problems of two kinds each."""
    run_pattern("four_wave_static", pattern, knobs)


@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_run_time_layout_kernel(gpu, knobs, pattern):
    """5->24-12-1 and 16->24-12-1, seven restarts each."""
    run_pattern("run_time_layout", pattern, knobs)


@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_lane_per_problem(gpu, knobs, pattern):
    """BORE_LBFGSB_COOP_GRID=0, 6->32-32-1: the sequential code on the device, every Coop{0, 1} branch."""
    run_pattern("lane_per_problem", pattern, knobs)


@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_two_workgroups_per_cu(gpu, knobs, pattern):
    run_pattern("two_workgroups_per_cu", pattern, knobs)


@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_twelve_waves(gpu, knobs, pattern):
    """6->32-32-1 and the plugin's 16->32-32-32-1, thirteen restarts: twelve waves and a second workgroup."""
    run_pattern("twelve_waves", pattern, knobs)


@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_eight_waves_float32(gpu, knobs, pattern):
    run_pattern("eight_waves_float32", pattern, knobs)


@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_eight_waves_bfloat16(gpu, knobs, pattern):
    run_pattern("eight_waves_bfloat16", pattern, knobs)


@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_pooled_bfloat16(gpu, knobs, pattern):
    """32->128-128-1 with the optimiser's matrices in the device pool (BORE_LBFGSB_BIG=1): zero_big / big_stale."""
    run_pattern("pooled_bfloat16", pattern, knobs)


@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_queue(gpu, knobs, pattern):
    """BORE_LBFGSB_QUEUE=1: four waves take nine problems from a queue, a slot is used again."""
    run_pattern("queue", pattern, knobs)


@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_streamed_dense(gpu, knobs, pattern):
    """8->256-256-1 (streamed natively) and 5->7-3-1 (by the switch)."""
    run_pattern("streamed", pattern, knobs)


@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_streamed_lstm(gpu, knobs, pattern):
    run_pattern("lstm_streamed", pattern, knobs)


@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_every_family_meets_its_premises(gpu, knobs, family):
    """Summed over the family's cases, every per-family event occurred (the cases run here if they have not yet)."""
    total = family_events(family, knobs)
    print("EVENTS_MEASURED " + json.dumps({family: {p: _measured[(family, p)] for p in T.PATTERNS}}, sort_keys=True))
    missing = [k for k in T.PER_FAMILY if total.get(k, 0) < 1]
    assert not missing, (family, missing, total)
    assert total["projected_start"] == 0          # (lbfgsb_init has clipped the start: see the module docstring)


def test_the_file_meets_its_premises(gpu, knobs):
    totals = {f: family_events(f, knobs) for f in T.FAMILIES}
    for k in T.WHOLE_FILE:
        assert sum(t.get(k, 0) for t in totals.values()) >= 1, k
    hit = [f for f in MANY_WAVES if totals[f].get("formk_refresh", 0) >= 1]
    print("formk_refresh on the many-wave families:", {f: totals[f].get("formk_refresh", 0) for f in MANY_WAVES})
    assert [f for f in hit if "formk_refresh" not in WAIVED.get(f, [])], totals
