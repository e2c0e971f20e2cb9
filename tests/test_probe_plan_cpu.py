"""CPU: the host arithmetic every verified time-parallel pass shares (csrc/plan.hpp) -- the sample positions of the
forgetting probe (probe_starts), the reading of its curve (curve_last, warmup_of, warmup_wide_of), the longest warm-up
it measures (probe_wmax, probe_wmax_wide) and the plan of a forward-only pass (plan_pass, which csrc/seg_host.hpp
uploads for bhmm_score and bhmm_filter).  tests/probe_plan_driver.cpp prints them; they are compared with
restatements in Python integers and with what the drivers of the existing plan tests print for the same inputs.

fill_wide_block (seg_host.hpp) is not covered here: it calls gauss_pdf_constants of host_common.hpp, which includes
the kernel headers, so it does not build with the host compiler alone.  The GPU suites of bhmm_score and bhmm_filter
compare its blocks' results with the oracle."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 256


def _compile(tmp, name):
    exe = str(tmp / name)
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bhmm_amd", "csrc"),
                    os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("probe_plan")
    return {name: _compile(tmp, name) for name in ("probe_plan_driver", "score_plan_driver", "score_tile_plan_driver")}


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, stdout=subprocess.PIPE,
                          timeout=60).stdout.decode()


def _offsets(lengths, first=0):
    return [int(x) for x in np.concatenate([[first], first + np.cumsum(lengths)]).astype(np.int64)]


# ---- probe_starts ----------------------------------------------------------------------------------------------

def _starts_restated(off, Wmax):
    """the loop every probe had in the parent commit, in Python integers (all operands are non-negative: // is the
    division of C++)"""
    K = len(off) - 1
    longk = [k for k in range(K) if off[k + 1] - off[k] >= Wmax]
    out = []
    for i in range(P):
        k = longk[i % len(longk)]
        room = off[k + 1] - off[k] - Wmax + 1
        rep, reps = i // len(longk), (P + len(longk) - 1) // len(longk)
        out.append(off[k] + (room - 1) * rep // max(reps - 1, 1))
    return out


START_CASES = {
    "one trajectory of exactly Wmax steps (room 1)": (32, [32], 0),
    "one long trajectory (reps = P)": (1024, [100000], 0),
    "300 long trajectories (reps = 1)": (64, [64 + 7 * (k % 11) for k in range(300)], 0),
    "3 long among 5 short and 2 empty": (128, [5, 127, 4000, 0, 128, 31, 0, 129, 64, 1], 0),
    "a non-zero first offset": (128, [5, 127, 4000, 0, 128, 31, 0, 129, 64, 1], 98765),
}


@pytest.mark.parametrize("case", sorted(START_CASES))
def test_probe_starts(drivers, case):
    Wmax, lengths, first = START_CASES[case]
    off = _offsets(lengths, first)
    out = _run(drivers["probe_plan_driver"], "starts", Wmax, P, *off)
    starts = [int(line.split()[1]) for line in out.splitlines()]
    assert len(starts) == P
    assert starts == _starts_restated(off, Wmax)
    for s in starts:
        k = max(k for k in range(len(lengths)) if off[k] <= s and lengths[k] > 0)
        assert lengths[k] >= Wmax                      # in a trajectory of at least Wmax steps ...
        assert off[k] <= s and s + Wmax <= off[k + 1]  # ... and Wmax steps are left to its end
    if case.startswith("one long"):
        assert starts[0] == 0 and starts[-1] == 100000 - 1024 and len(set(starts)) == P
    if case.startswith("300"):
        assert starts == [off[k] for k in range(P)]    # one visit each, at the start


def test_probe_starts_do_not_depend_on_the_origin(drivers):
    Wmax, lengths, first = START_CASES["a non-zero first offset"]
    a = _starts_restated(_offsets(lengths, 0), Wmax)
    out = _run(drivers["probe_plan_driver"], "starts", Wmax, P, *_offsets(lengths, first))
    assert [int(line.split()[1]) - first for line in out.splitlines()] == a


def test_longest_warmup_the_probe_measures(drivers):
    for maxT in (0, 1, 63, 64, 65, 71, 72, 127, 128, 143, 144, 2047, 2048, 2055, 16383, 16384, 16400, 10 ** 9):
        out = dict(line.split() for line in _run(drivers["probe_plan_driver"], "wmax", maxT).splitlines())
        narrow = min(1024, maxT // 2) // 4 * 4
        wide = min(8192, maxT // 2) // 8 * 8
        assert int(out["narrow"]) == (narrow if narrow >= 32 else 0), maxT   # no probe below 32
        assert int(out["wide"]) == (wide if wide >= 64 else 0), maxT         # no probe below 64


# ---- the reading of the curve ----------------------------------------------------------------------------------

def _narrow(last, Wmax):
    w = math.ceil(1.15 * (last + 2))
    return min(max(16, (w + 3) // 4 * 4), Wmax)


def _wide(last):
    w = math.ceil(1.5 * (last + 2))
    return max(16, (w + 7) // 8 * 8)


def _read(drivers, Wmax, target, both, entries):
    out = _run(drivers["probe_plan_driver"], "read", Wmax, repr(target), int(both),
               *["%d:%r" % (i, v) for i, v in entries])
    r = dict(line.split() for line in out.splitlines())
    return int(r["last"]), int(r["narrow"]), int(r["wide"])


@pytest.mark.parametrize("Wmax", [32, 64])
def test_curve_reading(drivers, Wmax):
    t = 1e-13
    # all below the target: last = -1, the floor of 16
    for both in (False, True):
        assert _read(drivers, Wmax, t, both, [(3, 1e-14), (Wmax + 5, 9e-14)]) == (-1, 16, 16)
    assert _narrow(-1, Wmax) == 16 and _wide(-1) == 16
    # a single spike at index 0
    assert _read(drivers, Wmax, t, False, [(0, 1.0)]) == (0, 16, 16)
    assert (_narrow(0, Wmax), _wide(0)) == (16, 16)
    # a spike at Wmax - 1: the narrow rule caps at Wmax; the wide rule does not, its callers cap (bhmm_score,
    # bhmm_filter) or make no statement (the E-step at 9..64 states: last + 2 >= Wmax)
    last, narrow, wide = _read(drivers, Wmax, t, False, [(Wmax - 1, 2e-13)])
    assert last == Wmax - 1 and last + 2 >= Wmax
    assert narrow == Wmax == _narrow(last, Wmax)
    assert wide == _wide(last) and wide > Wmax and wide % 8 == 0
    assert wide == {32: 56, 64: 104}[Wmax]
    # the entry exactly at the target counts (>=), in float
    assert _read(drivers, Wmax, t, False, [(9, float(np.float32(t)))])[0] == 9
    # a backward half that is worse than the forward half, read both ways
    entries = [(3, 1e-9), (Wmax + 20, 1e-9), (Wmax + 21, 1e-14)]
    assert _read(drivers, Wmax, t, False, entries) == (3, _narrow(3, Wmax), _wide(3))
    assert _read(drivers, Wmax, t, True, entries) == (20, _narrow(20, Wmax), _wide(20))
    assert (_narrow(3, Wmax), _wide(3)) == (16, 16)
    assert (_narrow(20, Wmax), _wide(20)) == (min(28, Wmax), 40)
    # in between: the rules against the arithmetic, every reading
    for last in range(0, Wmax - 1):
        assert _read(drivers, Wmax, t, False, [(last, 1.0)]) == (last, _narrow(last, Wmax), _wide(last))


# ---- the plan of a forward-only pass ---------------------------------------------------------------------------

PLAN_CASES = [
    [1, 2, 37, 500, 3001, 64, 129, 20000],
    [0, 5, 0, 0, 1, 70000, 0],
    [1],
    [0, 0],
    [3, 4, 5, 255, 256, 257, 259, 260, 261, 511, 513, 1023, 1025],
    [8192] * 4,
]


@pytest.mark.parametrize("asked", [0, 4, 258, 1024])
@pytest.mark.parametrize("case", range(len(PLAN_CASES)))
def test_plan_of_a_pass_is_the_plan_the_existing_drivers_print(drivers, case, asked):
    lengths = PLAN_CASES[case]
    off = _offsets(lengths, 17)
    ntraj = "ntraj %d\n" % sum(1 for T in lengths if T > 0)
    for np_ in (16, 32, 64):   # 9..64 states
        want = _run(drivers["score_plan_driver"], np_, 1024, asked, *off)
        assert _run(drivers["probe_plan_driver"], "plan", np_, 1024, asked, *off) == want + ntraj
    for simd in (1024, 16):    # 65..128 states
        want = _run(drivers["score_tile_plan_driver"], simd, asked, *off)
        assert _run(drivers["probe_plan_driver"], "tileplan", simd, asked, *off) == want + ntraj
