"""CPU: the acceptance protocol every verified pass of bhmm_filter, bhmm_posterior_decode and
bhmm_posterior_marginals runs (csrc/plan.hpp: two_attempts), and the doubling of a warm-up bhmm_score shares with it
(doubled).  tests/protocol_driver.cpp runs two_attempts with a scripted pass and prints the warm-up of every call, the
fallback counter, `verified` and the return code; every expectation is an exact integer.  The same driver prints
the integer rules of the segment-parallel backward draw (draw_seglen, draw_next_warmup; path_api.hip: seg_draw)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 30                  # the cap of every path but the matrix-core ones
SCORE_TILE_W_MAX = 1 << 20     # ... and theirs
BHMM_OK = 0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("protocol") / "protocol_driver")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bhmm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "protocol_driver.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def _out(driver, *args):
    return subprocess.run([driver] + [str(a) for a in args], check=True, stdout=subprocess.PIPE,
                          timeout=60).stdout.decode().splitlines()


def _run(driver, W, cap, script, counter=5):
    """(warm-ups the pass was called with, what the call added to the counter, verified, return code)"""
    lines = _out(driver, "run", W, cap, script, counter)
    calls = [int(l.split()[1]) for l in lines if l.startswith("call ")]
    tail = dict(l.split() for l in lines if not l.startswith("call "))
    assert len(calls) + 3 == len(lines)
    return calls, int(tail["counter"]) - counter, int(tail["verified"]), int(tail["rc"])


def test_verified_at_once(driver):
    assert _run(driver, 96, CAP, "v") == ([96], 0, 1, BHMM_OK)


def test_failed_then_verified(driver):
    assert _run(driver, 96, CAP, "fv") == ([96, 192], 1, 1, BHMM_OK)
    assert _run(driver, 96, 150, "fv") == ([96, 150], 1, 1, BHMM_OK)     # min(2 W, cap)


def test_failed_twice(driver):
    assert _run(driver, 96, CAP, "ff") == ([96, 192], 1, 0, BHMM_OK)     # no third call, one fallback


def test_abandon_on_the_first_call(driver):
    assert _run(driver, 96, CAP, "a") == ([96], 0, 0, BHMM_OK)


def test_abandon_on_the_second_call(driver):
    assert _run(driver, 96, CAP, "fa") == ([96, 192], 1, 0, BHMM_OK)


@pytest.mark.parametrize("code", [2, 3, 4])
def test_an_error_code_is_returned_unchanged_and_ends_the_call(driver, code):
    assert _run(driver, 96, CAP, "%dv" % code) == ([96], 0, 0, code)
    assert _run(driver, 96, CAP, "f%dv" % code) == ([96, 192], 1, 0, code)


def test_the_counter_is_cumulative(driver):
    assert _run(driver, 16, CAP, "ff", counter=0)[1] == 1
    assert _run(driver, 16, CAP, "ff", counter=41)[1] == 1


def test_caps(driver):
    assert _out(driver, "cap") == ["tile %d" % SCORE_TILE_W_MAX]
    assert _run(driver, 600000000, CAP, "ff")[0] == [600000000, 1 << 30]             # 2 W does not fit an int
    assert _run(driver, 786432, "tile", "ff")[0] == [786432, SCORE_TILE_W_MAX]
    assert _run(driver, 0, "tile", "ff")[0] == [0, 0]                                # the unsegmented tile plan
    assert _out(driver, "doubled", 600000000, CAP) == ["doubled %d" % (1 << 30)]
    assert _out(driver, "doubled", 786432, "tile") == ["doubled %d" % SCORE_TILE_W_MAX]
    assert _out(driver, "doubled", 0, "tile") == ["doubled 0"]
    assert _out(driver, "doubled", 288, CAP) == ["doubled 576"]


def _seglen(driver, total, want):
    return int(_out(driver, "draw_seglen", total, want)[0].split()[1])


def _next_warmup(driver, W, mismatch, nseg):
    return int(_out(driver, "draw_next_warmup", W, mismatch, nseg)[0].split()[1])


def test_draw_constants(driver):
    assert _out(driver, "draw") == ["seglen_min 64", "start 64", "max 4096", "rounds 16"]


def test_draw_segment_length(driver):
    """max(ceil(total / want), 64)"""
    want = 2048
    for total in (0, 1, want, want + 1, 64 * want):
        assert _seglen(driver, total, want) == 64                    # the floor
    assert _seglen(driver, 64 * want + 1, want) == 65                # rounds up
    assert _seglen(driver, 100 * want, want) == 100
    assert _seglen(driver, 100 * want + 1, want) == 101
    assert _seglen(driver, 1 << 31, 1024) == 1 << 21                 # a 2^31-step total
    assert _seglen(driver, (1 << 31) + 1, 1024) == (1 << 21) + 1
    assert _seglen(driver, 1 << 31, 1) == 1 << 31                    # (a length no int holds)
    assert _seglen(driver, 1, 1) == 64 and _seglen(driver, 65, 1) == 65


def test_draw_next_warmup(driver):
    """twice the warm-up while more than a tenth of the segments were left to the fix-up, up to 4096"""
    assert _next_warmup(driver, 64, 0, 147) == 64
    assert _next_warmup(driver, 64, 10, 100) == 64                   # exactly a tenth: not more than a tenth
    assert _next_warmup(driver, 64, 11, 100) == 128
    assert _next_warmup(driver, 64, 1, 9) == 128
    assert _next_warmup(driver, 2048, 50, 100) == 4096
    assert _next_warmup(driver, 4096, 50, 100) == 4096               # stays
    assert _next_warmup(driver, 4096, 100, 100) == 4096
    # mismatch * 10 does not fit an int: 3e9 > 2^31 - 1 segments doubles, 2147483640 does not
    assert _next_warmup(driver, 64, 300000000, 2147483647) == 128
    assert _next_warmup(driver, 64, 214748364, 2147483647) == 64
    assert _next_warmup(driver, 64, 214748365, 2147483647) == 128
