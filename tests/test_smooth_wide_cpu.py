"""No GPU: the time-segmented path of bhmm_posterior_decode / bhmm_posterior_marginals for 9 to 64 states exists in
the built library -- all 54 instantiations of k_smooth_wide_bwd are in the gfx950 code object, the header, the
context and the option table name the new options, the threshold is admissible -- and the planner of the budgeted
workspace (csrc/plan.hpp: smooth_ranges) cuts the plan into aligned ranges of whole segments; its driver
(tests/smooth_ranges_driver.cpp) is built as a stand-alone program with -fsanitize=address,undefined."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bhmm_amd.h")
CSRC = os.path.join(ROOT, "bhmm_amd", "csrc")


def test_every_instantiation_is_in_the_gfx950_code_object():
    """16 / 32 / 64 lanes per segment x gaussian / discrete B^T in LDS / discrete B^T read ahead x decode to bytes /
    decode to int32 / rows double / rows float / projection double / projection float"""
    from bhmm_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    names = set(m.decode() for m in re.findall(rb"_ZN4bhmm17k_smooth_wide_bwdILi\d[A-Za-z0-9_]*", blob))
    want = set()
    for np_ in (16, 32, 64):
        for kind, lds in ((0, 0), (1, 1), (1, 0)):
            for stage, ot in ((0, "h"), (0, "i"), (1, "d"), (1, "f"), (2, "d"), (2, "f")):
                want.add("_ZN4bhmm17k_smooth_wide_bwdILi%dELi%dELb%dELi%dE%sEEvPKNS_14ScoreWideModelEiPKlNS_4SegsE"
                         % (np_, kind, lds, stage, ot))
    assert len(want) == 54
    missing = [w for w in want if not any(x.startswith(w) for x in names)]
    assert not missing, missing[:4]
    assert b"k_smooth_flags" in blob
    # the forward half it launches, and the kernels of the generic route, are still there
    for np_ in (16, 32, 64):
        for kind, lds in ((0, 0), (1, 1), (1, 0)):
            assert ("_ZN4bhmm13k_filter_wideILi%dELi%dELb%dEdLb0ELb0EEEv" % (np_, kind, lds)).encode() in blob
    for pt in ("h", "i"):
        assert ("_ZN4bhmm15k_post_gamma_rmI%sEE" % pt).encode() in blob
    for ot in ("d", "f"):
        assert ("_ZN4bhmm14k_marg_rows_rmI%sEE" % ot).encode() in blob


def test_header_context_and_option_table_name_the_new_options():
    raw = open(HEADER).read()
    for anchor in (r"int\s+bhmm_posterior_decode\s*\(", r"#define\s+BHMM_MARG_F32"):
        m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*" + anchor, raw, re.S)
        assert m, anchor
        text = m.group(1)
        for word in ("smooth_wide", "smooth_seglen", "smooth_W", "smooth_ws_mb", "smooth_segments",
                     "smooth_wide_min_total", "k_smooth_wide_bwd"):
            assert word in text, (anchor, word)
    ctx = open(os.path.join(CSRC, "ctx.hpp")).read()
    for word in ("smooth_wide", "smooth_seglen", "smooth_W", "smooth_ws_mb", "smooth_nseg", "smooth_ntraj",
                 "smooth_seglen_opt", "smooth_segments", "struct SmoothBufs", "} smooth;"):
        assert word in ctx, word
    api = open(os.path.join(CSRC, "bhmm_amd.hip")).read()
    for word in ("smooth_wide", "smooth_seglen", "smooth_W", "smooth_ws_mb"):      # a setter and a getter
        assert api.count('"%s"' % word) == 2, word
    for word in ("smooth_segments", "smooth_wide_min_total"):                      # read-only: the getter alone
        assert api.count('"%s"' % word) == 1, word


def test_threshold_is_a_power_of_two_not_below_the_floor():
    internal = open(os.path.join(CSRC, "host_internal.hpp")).read()
    m = re.search(r"SMOOTH_WIDE_MIN_TOTAL\s*=\s*(\d+)\s*;", internal)
    assert m
    v = int(m.group(1))
    assert v >= 32768 and v & (v - 1) == 0


def test_kernel_header_builds_on_the_family_and_the_makefile_has_the_object():
    text = open(os.path.join(CSRC, "smooth_wide_kernels.hpp")).read()
    for inc in ("wide_kernels.hpp", "score_wide_kernels.hpp", "marg_kernels.hpp"):
        assert '#include "%s"' % inc in text
    for name in ("rows_of_group<NP>", "dot16(", "wgroup_sum<NP>", "wgroup_mask<NP>", "wide_emit<NP, KIND, true>",
                 "wide_load<KIND>", "WIDE_PF", "MARG_QMAX", "fast_rcp("):
        assert name in text, name
    for defined in (r"struct\s+ScoreWideModel", r"struct\s+Segs\b", r"double\s+wgroup_sum\s*\(", r"MARG_QMAX\s*="):
        assert not re.search(defined, text), defined
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(OBJDIR)/smooth_wide.o" in mk and "smooth_wide.hip" in mk and "smooth_wide_kernels.hpp" in mk
    # the forward half is launched, not copied: the unit instantiates no k_filter_wide of its own
    unit = open(os.path.join(CSRC, "smooth_wide.hip")).read()
    assert "filter_wide_launch(" in unit and "filter_wide_kernels.hpp" not in unit


# ---- the ranges of the budgeted workspace ---------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """built once, with the address and undefined-behaviour sanitizers, as a stand-alone program"""
    exe = str(tmp_path_factory.mktemp("smooth_ranges") / "smooth_ranges_driver")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bhmm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "smooth_ranges_driver.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def _ranges(exe, group, row_bytes, budget, lens):
    r = subprocess.run([exe, str(group), str(row_bytes), str(budget)] + [str(int(x)) for x in lens],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    out = [tuple(int(x) for x in line.split()[1:]) for line in r.stdout.decode().splitlines()]
    _invariants(out, group, row_bytes, budget, lens)
    return out


def _invariants(ranges, group, row_bytes, budget, lens):
    """consecutive whole segments, every segment once; starts aligned to the group; whole groups except at the end
    of the plan; the steps are the segments' own; within the budget unless the range is a single group"""
    nseg = len(lens)
    assert (ranges[0][0] if ranges else 0) == 0 and (ranges[-1][1] if ranges else 0) == nseg
    for i, (s0, s1, steps) in enumerate(ranges):
        assert s0 < s1 and s0 % group == 0
        assert s1 % group == 0 or s1 == nseg
        assert steps == sum(lens[s0:s1])
        if i:
            assert s0 == ranges[i - 1][1]
        if budget > 0 and steps * row_bytes > budget:
            assert s1 - s0 <= group
        if budget > 0 and s1 < nseg:            # greedy: the next group would not have fitted
            assert (steps + sum(lens[s1:s1 + group])) * row_bytes > budget


def test_budget_below_one_segment_gives_one_aligned_group_per_range(driver):
    lens = [256] * 10
    for group in (1, 2, 4):
        got = _ranges(driver, group, 64 * 8, 1000, lens)
        want = [(s, min(s + group, 10), 256 * (min(s + group, 10) - s)) for s in range(0, 10, group)]
        assert got == want


def test_exact_fit(driver):
    lens = [100] * 8
    row = 12 * 8
    # two groups of two segments fit exactly; one byte less and they do not
    assert _ranges(driver, 2, row, 400 * row, lens) == [(0, 4, 400), (4, 8, 400)]
    assert _ranges(driver, 2, row, 400 * row - 1, lens) == [(0, 2, 200), (2, 4, 200), (4, 6, 200), (6, 8, 200)]


def test_budget_zero_gives_one_range(driver):
    lens = [5, 1, 2048, 3, 700]
    for group in (1, 2, 4):
        assert _ranges(driver, group, 9 * 8, 0, lens) == [(0, 5, sum(lens))]
    assert _ranges(driver, 4, 9 * 8, 0, []) == []


def test_ragged_last_range(driver):
    lens = [300, 300, 300, 300, 300, 300, 300, 17]
    got = _ranges(driver, 1, 8, 8 * 1000, lens)
    assert got == [(0, 3, 900), (3, 6, 900), (6, 8, 317)]


def test_nseg_not_a_multiple_of_the_group(driver):
    lens = [64, 64, 64, 64, 64, 64, 1]              # 7 segments, groups of 4: the last workgroup is partial
    assert _ranges(driver, 4, 8, 8 * 256, lens) == [(0, 4, 256), (4, 7, 129)]
    assert _ranges(driver, 4, 8, 8 * 10000, lens) == [(0, 7, 385)]
    assert _ranges(driver, 2, 8, 8 * 128, lens) == [(0, 2, 128), (2, 4, 128), (4, 6, 128), (6, 7, 1)]
    assert _ranges(driver, 2, 8, 8 * 130, lens) == [(0, 2, 128), (2, 4, 128), (4, 7, 129)]
    # segments of very different lengths: a long one alone exceeds the budget and still gets its range
    lens = [10, 5000, 10, 10, 10]
    assert _ranges(driver, 1, 8, 8 * 100, lens) == [(0, 1, 10), (1, 2, 5000), (2, 5, 30)]
