"""The dynamic LDS of the streamed restart kernels as stream_restart_carve lays it out, against what the kernels index
(no GPU).

bore_amd/csrc/stream_restart.h is host code over lbfgsb.h and integers; the host build of the tests exports it.  Every
assertion below is written from the kernel's side (bore_amd/csrc/bore_stream.hip: stream_restart_drive, which both
stream_lbfgsb_kernel and lstm_stream_lbfgsb_kernel run), not from the carve's: from the 16-byte aligned start of the
dynamic region, in floats, the driver puts lo and hi of the box (De = D rounded up to even doubles each) and nbd (D
ints) at o_box, four votes at o_vote, and wave w's slot at o_prob + w * prob_floats -- the parked State at its start,
make_work's doubles at o_dw, its ints at o_iw -- zeroes a slot as float4 and reads fp64 as 16-byte pairs."""
import itertools

import pytest

import lbfgsb_host as H

LDS_BYTES = 163840
SLACK = 64                     # beside the static LDS: its alignment, and the <= 15 bytes the driver skips to align
DENSE_STATIC = 55080           # sizeof(StreamLds): what stream_lbfgsb_kernel holds statically
LSTM_STATIC = 55080 + 64 * 4   # ... and lstm_stream_lbfgsb_kernel: the panels and rows[64]
DIMS = [1, 2, 3, 63, 64]
MAXCOR = list(range(1, 33))
# static bytes at which D = 3, maxcor = 10 (a slot of 8032 B behind 80 B of box and votes) comes out with 4, 3, 2, 1
# and 0 waves: each count's last byte and the next one (found with the function, pinned here)
EDGES = {131552: 4, 131553: 3, 139584: 3, 139585: 2, 147616: 2, 147617: 1, 155648: 1, 155649: 0}
STATICS = [0, DENSE_STATIC, LSTM_STATIC] + sorted(EDGES) + [LDS_BYTES - SLACK, LDS_BYTES, LDS_BYTES + 4096]


def check(D, m, static, max_waves=4):
    fits, c, state_bytes, dwork, iwork = H.stream_restart_carve(D, m, static, max_waves)
    De = (D + 1) & ~1
    what = (D, m, static, max_waves, c)
    # alignment: every offset a multiple of 4 floats
    for k in ("o_box", "o_vote", "o_prob", "prob_floats", "o_dw", "o_iw"):
        assert c[k] % 4 == 0 and c[k] >= 0, (k, what)
    # box | vote | slots, in this order, none into the next
    assert c["o_box"] + 4 * De + D <= c["o_vote"], what
    assert c["o_vote"] + 4 <= c["o_prob"], what
    # a slot: State | 2 * dwork_size floats at o_dw | iwork_size ints at o_iw
    assert state_bytes <= 4 * c["o_dw"], what
    assert c["o_dw"] + 2 * dwork <= c["o_iw"], what
    assert c["o_iw"] + iwork <= c["prob_floats"], what
    # the launch holds what the waves address (16: the alignment skip) and fits the CU beside the static LDS
    assert 0 <= c["waves"] <= max_waves and fits == (c["waves"] >= 1), what
    used = 4 * (c["o_prob"] + c["waves"] * c["prob_floats"])
    assert used + 16 <= c["lds_bytes"], what
    if fits:
        assert static + c["lds_bytes"] <= LDS_BYTES, what
    # no wave exactly when one slot does not fit; never a slot fewer than fit (up to max_waves)
    one = static + SLACK + 4 * (c["o_prob"] + c["prob_floats"])
    assert (c["waves"] == 0) == (one > LDS_BYTES), what
    if c["waves"] < max_waves:
        assert static + SLACK + 4 * (c["o_prob"] + (c["waves"] + 1) * c["prob_floats"]) > LDS_BYTES, what
    return c


@pytest.mark.parametrize("D", DIMS)
def test_the_carve_holds_what_the_driver_indexes(D):
    seen = set()
    for m, static in itertools.product(MAXCOR, STATICS):
        seen.add(check(D, m, static)["waves"])
    assert seen == {0, 1, 2, 3, 4}, seen
    for m, static, max_waves in itertools.product((1, 10, 32), (0, DENSE_STATIC, 147616), (1, 2, 3)):
        check(D, m, static, max_waves)


def test_the_pinned_edges():
    for static, waves in EDGES.items():
        assert check(3, 10, static)["waves"] == waves, static
    c = check(3, 10, DENSE_STATIC)
    assert (c["o_box"], c["o_vote"], c["o_prob"], c["prob_floats"]) == (0, 20, 24, 2008), c
    # what the two kernels get at the ends of the range: the largest problem leaves one wave, the default four
    for static in (DENSE_STATIC, LSTM_STATIC):
        assert check(64, 32, static)["waves"] == 1
        assert check(63, 17, static)["waves"] == 2
        assert check(64, 10, static)["waves"] == 4
        assert check(1, 1, static)["waves"] == 4
    assert check(64, 32, DENSE_STATIC)["room"] == 107400 and check(64, 32, LSTM_STATIC)["room"] == 107144
