"""CPU: the segment plan of bhmm_score for 9 to 64 states.  The plan is host-only code
(csrc/plan.hpp: score_seglen, then plan_segments); tests/score_plan_driver.cpp makes it the way score_api.hip
does and prints it.  Checked here: the segments cover every trajectory exactly once and in order, inner starts are
multiples of four, a trajectory no longer than a segment gets one segment, the automatic length is a multiple of four
of at least 2048 steps, and the plan is a function of (offsets, lanes per segment, SIMD count, seglen) alone.  The
option names need a context, hence a device: tests/test_score_wide_gpu.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("score_plan") / "score_plan_driver")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bhmm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "score_plan_driver.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def _plan(exe, np_, simd, asked, offsets):
    out = subprocess.run([exe, str(np_), str(simd), str(asked)] + [str(int(o)) for o in offsets], check=True,
                         stdout=subprocess.PIPE, timeout=60).stdout.decode()
    seglen, segs, traj0 = None, [], None
    for line in out.splitlines():
        w = line.split()
        if w[0] == "seglen":
            seglen = int(w[1])
        elif w[0] == "seg":
            segs.append((int(w[1]), int(w[2]), int(w[3])))
        elif w[0] == "traj0":
            traj0 = [int(x) for x in w[1:]]
    return seglen, segs, traj0, out


def _offsets(lengths, first=0):
    return np.concatenate([[first], first + np.cumsum(lengths)]).astype(np.int64)


RAGGED = [1, 2, 37, 500, 3001, 64, 129, 20000]
CASES = [
    RAGGED,
    [0, 5, 0, 0, 1, 70000, 0],          # empty trajectories between and at the ends
    [1],                                # a single step
    [1, 1, 1, 1],
    [3, 4, 5, 255, 256, 257, 259, 260, 261, 511, 513, 1023, 1025],
    [100000] * 128,                     # the shape of BASELINE configs[3]
    [2047, 2048, 2049, 4095, 4097, 8191, 123457],
]


def _check(lengths, seglen, segs, traj0):
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
    # every segment belongs to a trajectory's range
    assert sum(traj0[k + 1] - traj0[k] for k in range(K)) == len(segs)


@pytest.mark.parametrize("asked", [0, 1, 4, 255, 256, 258, 1024, 100000])
@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("np_", [16, 32, 64])
def test_plan_covers_every_trajectory_once(driver, np_, case, asked):
    lengths = CASES[case]
    seglen, segs, traj0, _ = _plan(driver, np_, 1024, asked, _offsets(lengths))
    if asked > 0:
        assert seglen == (asked + 3) // 4 * 4     # the caller's length, rounded up to a multiple of four
    else:
        assert seglen >= 2048
    _check(lengths, seglen, segs, traj0)


def test_automatic_length_fills_the_device(driver):
    # two wavefronts per SIMD for one model: 2 * SIMDs * (64 / NP) segments, but never shorter than 2048 steps
    lengths = [100000] * 128
    for np_, simd, want in ((64, 1024, 6252), (32, 1024, 3128), (16, 1024, 2048), (64, 16, 400000), (64, 4096, 2048)):
        seglen, segs, traj0, _ = _plan(driver, np_, simd, 0, _offsets(lengths))
        total = sum(lengths)
        groups = 2 * simd * (64 // np_)
        assert seglen % 4 == 0 and seglen >= 2048
        assert seglen == (max(-(-total // groups), 2048) + 3) // 4 * 4
        assert seglen == want
        _check(lengths, seglen, segs, traj0)
    # configs[3] on 1024 SIMDs: 16 segments per trajectory
    _, segs, _, _ = _plan(driver, 64, 1024, 0, _offsets(lengths))
    assert len(segs) == 128 * 16


def test_plan_depends_on_its_inputs_only(driver):
    rng = np.random.default_rng(3)
    lengths = [int(x) for x in rng.integers(0, 30000, 40)]
    a = _plan(driver, 32, 1024, 0, _offsets(lengths))
    assert _plan(driver, 32, 1024, 0, _offsets(lengths))[3] == a[3]          # the same call again
    assert _plan(driver, 32, 1024, 0, _offsets(lengths, first=12345))[3] == a[3]   # offsets relative to any origin
    b = _plan(driver, 32, 1024, 512, _offsets(lengths))
    assert _plan(driver, 16, 7, 512, _offsets(lengths))[3] == b[3]           # a given length: nothing else matters
    assert b[3] != a[3]
    _check(lengths, b[0], b[1], b[2])
