"""CPU: the segment plan and the tile table of bhmm_score for 65 to 128 states.  Both are
host-only code (csrc/plan.hpp: score_tile_seglen, plan_segments, plan_tiles); tests/score_tile_plan_driver.cpp makes
them the way score_api.hip does and prints them.  Checked here: the segments cover every trajectory exactly once and
in order, inner starts are multiples of four, a trajectory no longer than a segment gets one segment, every segment
sits in exactly one tile row and empty rows are -1, the automatic length gives one tile per compute unit with a floor
of 256 steps, and the plan is a function of (offsets, SIMD count, asked length) alone.  The kernel needs a device:
tests/test_score_tile_gpu.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLOOR = 256   # plan::SCORE_TILE_MIN_SEGLEN


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("score_tile_plan") / "score_tile_plan_driver")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bhmm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "score_tile_plan_driver.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def _plan(exe, simd, asked, offsets):
    out = subprocess.run([exe, str(simd), str(asked)] + [str(int(o)) for o in offsets], check=True,
                         stdout=subprocess.PIPE, timeout=60).stdout.decode()
    seglen, segs, traj0, tiles = None, [], None, []
    for line in out.splitlines():
        w = line.split()
        if w[0] == "seglen":
            seglen = int(w[1])
        elif w[0] == "seg":
            segs.append((int(w[1]), int(w[2]), int(w[3])))
        elif w[0] == "traj0":
            traj0 = [int(x) for x in w[1:]]
        elif w[0] == "tile":
            tiles.append([int(x) for x in w[1:]])
    return seglen, segs, traj0, tiles, out


def _offsets(lengths, first=0):
    return np.concatenate([[first], first + np.cumsum(lengths)]).astype(np.int64)


# the length lists of test_score_wide_cpu.py::CASES, and bench.py's 128 x 10 000
RAGGED = [1, 2, 37, 500, 3001, 64, 129, 20000]
CASES = [
    RAGGED,
    [0, 5, 0, 0, 1, 70000, 0],          # empty trajectories between and at the ends
    [1],                                # a single step
    [1, 1, 1, 1],
    [3, 4, 5, 255, 256, 257, 259, 260, 261, 511, 513, 1023, 1025],
    [100000] * 128,                     # the shape of BASELINE configs[3]
    [2047, 2048, 2049, 4095, 4097, 8191, 123457],
    [10000] * 128,                      # bench.py's 65- and 128-state configurations
]


def _check(lengths, seglen, segs, traj0, tiles):
    K = len(lengths)
    assert seglen > 0 and seglen % 4 == 0
    assert len(traj0) == K + 1 and traj0[0] == 0 and traj0[K] == len(segs)
    for k, T in enumerate(lengths):
        mine = segs[traj0[k]:traj0[k + 1]]
        assert all(s[0] == k for s in mine)
        if T == 0:
            assert mine == []
            continue
        # covered exactly once, in order, without holes
        t = 0
        for _, t0, ln in mine:
            assert t0 == t and ln > 0
            t += ln
        assert t == T
        # inner starts at multiples of four; lengths within three steps of the asked one
        assert all(t0 % 4 == 0 for _, t0, _ in mine)
        assert all(ln <= seglen + 3 for _, _, ln in mine)
        assert len(mine) <= -(-T // seglen)
        if T <= seglen:
            assert len(mine) == 1       # no boundary: the exact recursion
    assert sum(traj0[k + 1] - traj0[k] for k in range(K)) == len(segs)
    # every segment in exactly one tile row; the other rows are -1; no tile is empty
    rows = [s for t in tiles for s in t]
    assert all(len(t) == 16 for t in tiles)
    assert sorted(s for s in rows if s != -1) == list(range(len(segs)))
    assert all(s >= -1 for s in rows)
    assert all(any(s != -1 for s in t) for t in tiles)
    assert len(tiles) <= len(segs) // 16 + 2
    # segments that start a trajectory (no warm-up) do not share a tile with those that have one
    for t in tiles:
        kinds = {segs[s][1] == 0 for s in t if s != -1}
        assert len(kinds) == 1


@pytest.mark.parametrize("asked", [0, 1, 4, 255, 256, 258, 1024, 100000])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_plan_covers_every_trajectory_once(driver, case, asked):
    lengths = CASES[case]
    seglen, segs, traj0, tiles, _ = _plan(driver, 1024, asked, _offsets(lengths))
    if asked > 0:
        assert seglen == (asked + 3) // 4 * 4     # the caller's length, rounded up to a multiple of four
    else:
        assert seglen >= FLOOR
    _check(lengths, seglen, segs, traj0, tiles)


def test_automatic_length_fills_the_device(driver):
    # one workgroup per compute unit for one model: 16 * SIMDs / 4 segments, but never shorter than 256 steps
    for lengths, simd, want in (([100000] * 128, 1024, 3128), ([10000] * 128, 1024, 316), ([10000] * 128, 16, 20000),
                                ([10000] * 128, 4096, 256), ([1000] * 8, 1024, 256)):
        seglen, segs, traj0, tiles, _ = _plan(driver, simd, 0, _offsets(lengths))
        total = sum(lengths)
        rows = 16 * (simd // 4)
        assert seglen % 4 == 0 and seglen >= FLOOR
        assert seglen == (max(-(-total // rows), FLOOR) + 3) // 4 * 4
        assert seglen == want
        _check(lengths, seglen, segs, traj0, tiles)
    # 128 x 10 000 on 1024 SIMDs: 32 segments per trajectory, 256 tiles (8 of first segments, 248 of the others)
    _, segs, _, tiles, _ = _plan(driver, 1024, 0, _offsets([10000] * 128))
    assert len(segs) == 128 * 32
    assert len(tiles) == 256


def test_plan_depends_on_its_inputs_only(driver):
    rng = np.random.default_rng(3)
    lengths = [int(x) for x in rng.integers(0, 30000, 40)]
    a = _plan(driver, 1024, 0, _offsets(lengths))
    assert _plan(driver, 1024, 0, _offsets(lengths))[4] == a[4]          # the same call again
    assert _plan(driver, 1024, 0, _offsets(lengths, first=12345))[4] == a[4]   # offsets relative to any origin
    b = _plan(driver, 1024, 512, _offsets(lengths))
    assert _plan(driver, 7, 512, _offsets(lengths))[4] == b[4]           # a given length: nothing else matters
    assert b[4] != a[4]
    _check(lengths, b[0], b[1], b[2], b[3])
