"""CPU: the integer rules of the Viterbi passes (csrc/plan.hpp: vit_*), printed by tests/protocol_driver.cpp and checked
with exact integers.  The segment lengths are compared with their Python restatements in tests/viterbi_matrix_cases.py
(seglen_wide, seglen_gen), on which the plans that tests/test_viterbi_matrix_gpu.py asserts are built: the library
(path_api.hip: wide_seg_viterbi; gen_api.hip: gen_seg_viterbi, gen_rows_viterbi) calls the same functions."""
import itertools

import pytest

from tests import viterbi_matrix_cases as vc
from tests.test_protocol_cpu import _out, driver  # noqa: F401  (the driver's build is that file's fixture)

BHMM_OK = 0
STATES = (9, 16, 17, 32, 33, 64, 65, 128, 129, 256)


def _seglens(driver, totals, n, W, per_simd, warmups):
    np_ = vc.np_of(n) if n <= 64 else 0
    lines = _out(driver, "vit_seglen", ",".join(str(t) for t in totals), n, np_, W, per_simd, warmups, vc.NUM_SIMD)
    assert len(lines) == len(totals)
    return [int(l.split()[1]) for l in lines]


def _seglen(driver, total, n, W, per_simd, warmups):
    return _seglens(driver, [total], n, W, per_simd, warmups)[0]


def _slots(n, per_simd):
    """segments that fill the device once: the `want` of the pass for n states"""
    if n <= 64:
        return per_simd * vc.NUM_SIMD * (64 // vc.np_of(n))
    return per_simd * vc.NUM_SIMD if n <= 128 else 4 * (vc.NUM_SIMD // 4)


@pytest.mark.parametrize("n", STATES)
def test_segment_lengths_are_the_restated_ones(driver, n):
    """totals on both sides of one segment per slot at every fill length tried (W below and above each of them), both
    sides of a multiple of the slot count, and the sums of the GPU cases' lengths"""
    for per_simd, warmups in itertools.product((1, 2, 3), (1, 2, 3)):
        if n > 64 and warmups > 1:
            continue        # (65..128 states: one warm-up with the margin rule on; above: no such option)
        if n > 128 and per_simd > 1:
            continue
        slots = _slots(n, per_simd)
        totals = [0, 1, slots - 1, slots, slots + 1, 40 * slots - 1, 40 * slots, 40 * slots + 1, 300 * slots + 7,
                  sum(vc.S1_LENGTHS), sum(vc.S6_LENGTHS)]
        for W in (8, 16, 40, 128, 288, 2400):
            want = [vc.seglen_wide(t, n, W, per_simd, warmups) if n <= 64 else vc.seglen_gen(t, n, W, per_simd) for t in totals]
            assert _seglens(driver, totals, n, W, per_simd, warmups) == want, (n, W, per_simd, warmups)


def test_segment_lengths_at_a_total_past_2_to_the_31(driver):
    assert _seglen(driver, 1 << 33, 64, 128, 1, 2) == 1 << 23
    assert _seglen(driver, (1 << 33) + 1, 100, 128, 1, 1) == (1 << 23) + 1
    assert _seglen(driver, (1 << 33) + 1, 200, 128, 1, 1) == (1 << 23) + 8


def _w(driver, spec_W, vit_W, total, margin=1, mend=1, per_simd=1):
    return {k: int(v) for k, v in
            (l.split() for l in _out(driver, "vit_w", spec_W, vit_W, total, vc.NUM_SIMD, per_simd, margin, mend))}


def test_first_warmups(driver):
    """E-step's length to a multiple of 8, at least 64 (128 unprobed); 9..64 states at most 128; 65..128 states up to
    four times, 129..256 six times the E-step's without the mending round, both bounded by the fill length"""
    assert _w(driver, 0, 0, 10 ** 6)["estep"] == 128 and _w(driver, 1, 0, 10 ** 6)["estep"] == 64
    assert _w(driver, 281, 0, 10 ** 6)["estep"] == 288 and _w(driver, 288, 0, 10 ** 6)["estep"] == 288
    assert _w(driver, 288, 0, 10 ** 6)["wide"] == 128 and _w(driver, 70, 0, 10 ** 6)["wide"] == 72
    assert _w(driver, 288, 48, 10 ** 6)["wide"] == 48                        # what the last call left
    # fill length of 10^6 steps: ceil(10^6 / 1024) = 977 -> 984
    w = _w(driver, 288, 0, 10 ** 6)
    assert (w["gen_cap"], w["gen"], w["rows"]) == (984, 288, 288)            # min(4 x 288, 984); mending: the E-step's
    w = _w(driver, 288, 0, 10 ** 6, mend=0)
    assert (w["gen"], w["rows"]) == (984, 1480)                              # the cap; min(6 x 288, 3 x 984 / 2 = 1476 -> 1480)
    w = _w(driver, 288, 0, 10 ** 7, mend=0)
    assert (w["gen_cap"], w["gen"], w["rows"]) == (1152, 1152, 1728)         # four and six times
    w = _w(driver, 288, 0, 1000, mend=0)
    assert (w["gen_cap"], w["gen"], w["rows"]) == (288, 288, 288)            # never below the E-step's
    assert _w(driver, 288, 0, 10 ** 6, margin=0, mend=0)["gen"] == 288       # no margin rule: the E-step's
    assert _w(driver, 288, 0, 10 ** 6, per_simd=2)["gen_cap"] == 496         # 489 -> 496
    w = _w(driver, 288, 40, 10 ** 6, mend=0)
    assert (w["gen"], w["rows"]) == (40, 40)


def test_next_warmup(driver):
    def nxt(W, longer, cap):
        return int(_out(driver, "vit_next_warmup", W, longer, cap)[0].split()[1])
    assert nxt(128, 0, 288) == 128
    assert nxt(128, 1, 288) == 256 and nxt(256, 1, 288) == 288               # min(2 W, cap)
    assert nxt(288, 1, 288) == 288 and nxt(512, 1, 288) == 512               # at or beyond the cap: stays


def test_rows_give_up(driver):
    def gu(fails, W, maxT):
        return int(_out(driver, "vit_rows_give_up", fails, W, maxT)[0].split()[1])
    assert gu(1, 288, 6000) == 0
    assert gu(2, 288, 6000) == 1                                             # the second failure in a row
    assert gu(1, 1500, 6000) == 0 and gu(1, 1501, 6000) == 1                 # 4 W > maxT
    assert gu(1, 1 << 30, 1 << 33) == 0                                      # (4 W does not fit an int)


def _chunk(driver, vit_W, bad, explore, script, spec_W=288, fixed=0):
    """(warm-up of every attempt, the state left: (vit_W, vit_bad, vit_explore), last verdict accepted, return code)"""
    lines = _out(driver, "vit_chunk", vit_W, bad, explore, spec_W, fixed, script)
    calls = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("call ")]
    assert [f for _, f in calls] == [1] + [0] * (len(calls) - 1)             # only the first attempt is `first`
    tail = dict(l.split() for l in lines if not l.startswith("call "))
    return ([w for w, _ in calls], (int(tail["W"]), int(tail["bad"]), int(tail["explore"])), int(tail["accepted"]),
            int(tail["rc"]))


def test_exploration_verified_at_the_shorter_length(driver):
    assert _chunk(driver, 0, 0, 1, "a") == ([288], (288, 0, 1), 1, BHMM_OK)         # new observations: the E-step's
    assert _chunk(driver, 288, 0, 1, "a") == ([216], (216, 0, 1), 1, BHMM_OK)       # three quarters
    assert _chunk(driver, 216, 0, 1, "a") == ([168], (168, 0, 1), 1, BHMM_OK)       # 162 -> 168
    assert _chunk(driver, 168, 0, 1, "a") == ([128], (128, 0, 1), 1, BHMM_OK)       # 126 -> 128


def test_exploration_failed_and_back_to_the_last_good_length(driver):
    assert _chunk(driver, 216, 0, 1, "fa") == ([168, 216], (216, 168, 0), 1, BHMM_OK)
    # merely tolerable is not enough for a shorter length
    assert _chunk(driver, 216, 0, 1, "ca") == ([168, 216], (216, 168, 0), 1, BHMM_OK)
    # ... the search has ended, on these observations for good
    assert _chunk(driver, 216, 168, 0, "a") == ([216], (216, 168, 0), 1, BHMM_OK)
    assert _chunk(driver, 216, 168, 1, "a") == ([216], (216, 168, 0), 1, BHMM_OK)   # 168 failed before: not again
    # the last good length out of tolerance under this model: doubled, one attempt left
    assert _chunk(driver, 216, 0, 1, "ffa") == ([168, 216, 432], (432, 168, 0), 1, BHMM_OK)
    assert _chunk(driver, 216, 0, 1, "fff") == ([168, 216, 432], (216, 168, 0), 0, BHMM_OK)
    assert _chunk(driver, 216, 0, 1, "fc") == ([168, 216], (216, 168, 0), 0, BHMM_OK)  # tolerable, close: serial kernel


def test_exploration_floor_of_32(driver):
    assert _chunk(driver, 40, 0, 1, "a") == ([32], (32, 0, 1), 1, BHMM_OK)          # 30 -> 32
    assert _chunk(driver, 36, 0, 1, "a") == ([32], (32, 0, 1), 1, BHMM_OK)          # 27 -> 32
    assert _chunk(driver, 32, 0, 1, "a") == ([32], (32, 0, 0), 1, BHMM_OK)          # 24 -> 32: not shorter, search over
    assert _chunk(driver, 16, 0, 1, "a") == ([16], (16, 0, 0), 1, BHMM_OK)          # a forced 16 is never lengthened to 32


def test_without_exploration(driver):
    assert _chunk(driver, 0, 0, 1, "ffa", spec_W=100) == ([100, 200, 400], (400, 0, 1), 1, BHMM_OK)
    assert _chunk(driver, 0, 0, 1, "fff", spec_W=100) == ([100, 200, 400], (0, 0, 1), 0, BHMM_OK)
    assert _chunk(driver, 0, 0, 1, "c", spec_W=100) == ([100], (100, 0, 1), 0, BHMM_OK)
    assert _chunk(driver, 216, 0, 1, "a", fixed=1) == ([216], (216, 0, 1), 1, BHMM_OK)   # the caller fixed spec_W
    assert _chunk(driver, 216, 0, 1, "fa", fixed=1) == ([216, 432], (432, 0, 1), 1, BHMM_OK)


@pytest.mark.parametrize("code", [2, 4])
def test_an_error_code_ends_the_attempts(driver, code):
    assert _chunk(driver, 0, 0, 1, "%da" % code) == ([288], (0, 0, 1), 0, code)
    assert _chunk(driver, 216, 0, 1, "f%da" % code) == ([168, 216], (216, 168, 0), 0, code)
