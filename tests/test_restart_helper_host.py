"""The rule of the restart phase's job board (bore_amd/csrc/lbfgsb.h: JOB BOARD), on the host build: whenever the guess
`nothing enters or leaves the free set` holds, formk run at the TOP of the iteration on a copy of the workspace, with
the guessed sets, leaves the bytes in wn / snd / rwn that the call in its usual place leaves; the rule rejects every
iteration in which a variable entered or left.  tests/native/restart_helper_host.cpp is the board that checks it; here
it is fed the oracle's f and g over the bound patterns of tests/lbfgsb_paths.py and over config-1 problems (2->16-16-1
in the oracle's BO loop on Branin), and built once more as a program of its own under -fsanitize=address,undefined.
What this proves is the PROPERTY the device's rule relies on (same bytes whenever the guess holds, over every bound
pattern); the host board states the rule itself a second time, so the device's own comparison, its switching of the
live and spare blocks and its drop and wait paths are held by tests/test_gpu_restart_helper.py, bit for bit."""
import os
import subprocess

import pytest

import lbfgsb_paths as T
import restart_helper_host as R


@pytest.fixture(scope="module")
def board(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("restart_helper"))


def check(counts):
    c = dict(zip(R.NAMES, counts.tolist()))
    assert c["mismatch"] == 0 and c["same_bytes"] == c["guess_held"], c
    assert c["moved_accepted"] == 0 and c["nfree_changed"] == 0, c
    return c


def test_bound_patterns(board):
    """Every pattern of the case table on its two smallest float32 nets: open sides, one-sided bounds, fixed variables,
    corner starts, saturated weights, a wrapping history (formk's shift)."""
    counts = R.new_counts()
    for name in ("2-16-16-1", "5-24-12-1"):
        for pattern, tag, lo, hi, X0, hard, maxcor in T.launches("four_wave_static", name):
            fg = T.oracle_fg(name, hard)
            for x0 in X0[:4]:
                R.run(board, fg, x0, lo, hi, counts, **T.opts_for(maxcor))
    c = check(counts)
    print(c)
    assert c["guess_held"] > 0 and c["moved"] > 0 and c["dropped"] > 0


def test_config_1_problems(board):
    """Every restart of the first eight iterations of one oracle loop, as the headline runs them."""
    counts = R.new_counts()
    for fg, x0 in R.config1_problems(1, iterations=8):
        R.run(board, fg, x0, 0.0, 1.0, counts)
    c = check(counts)
    print(c)
    assert c["guess_held"] > 0


def test_stand_alone_program_under_asan_and_ubsan(tmp_path):
    """The same board over analytic objectives (n = 2..7, maxcor 3 and 10, three bound patterns), as a program of its
    own built with the sanitizers."""
    exe = str(tmp_path / "restart_helper_host")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-DRESTART_HELPER_MAIN", R.SRC, "-o", exe],
                        capture_output=True, text=True)
    if cc.returncode != 0 and any(s in cc.stderr for s in ("-lasan", "-lubsan", "libasan", "libubsan", "fsanitize")):
        pytest.skip("no sanitizer runtime in this toolchain: " + cc.stderr[-200:])
    assert cc.returncode == 0, cc.stderr[-2000:]   # (anything else is an error of the source)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "restart helper rule ok" in out.stdout, out.stdout[-500:] + out.stderr[-2000:]
