"""No GPU: the matrix-core path of bhmm_posterior_decode / bhmm_posterior_marginals for 65 to 128 states exists in the
built library -- all 96 instantiations of k_smooth_tile_bwd are in the gfx950 code object, the header, the context and
the option table name the new options, the threshold is admissible, the Makefile has the four objects -- and the
planner of the budgeted workspace (csrc/plan.hpp: smooth_tile_ranges) cuts the plan into ranges of whole segments with
tile tables of their own; its driver (tests/smooth_tile_ranges_driver.cpp) is built as a stand-alone program with
-fsanitize=address,undefined."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bhmm_amd.h")
CSRC = os.path.join(ROOT, "bhmm_amd", "csrc")


def test_every_instantiation_is_in_the_gfx950_code_object():
    """5 .. 8 column tiles x gaussian / discrete x all 16 NT states or fewer x decode to bytes / decode to int32 / rows
    double / rows float / projection double / projection float"""
    from bhmm_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    names = set(m.decode() for m in re.findall(rb"_ZN4bhmm17k_smooth_tile_bwdILi\d[A-Za-z0-9_]*", blob))
    want = set()
    for nt in (5, 6, 7, 8):
        for kind in (0, 1):
            for full in (0, 1):
                for form in range(6):
                    want.add("_ZN4bhmm17k_smooth_tile_bwdILi%dELi%dELb%dELi%dEEEvPKNS_14ScoreTileModelEPKl"
                             "NS_4SegsENS_8TilePlanE" % (nt, kind, full, form))
    assert len(want) == 96
    missing = [w for w in want if not any(x.startswith(w) for x in names)]
    assert not missing, missing[:4]
    assert b"k_smooth_tile_flags" in blob and b"k_smooth_tile_check" in blob
    # the forward half it launches, and the kernels of the generic route, are still there
    for nt in (5, 6, 7, 8):
        for kind in (0, 1):
            for full in (0, 1):
                assert ("_ZN4bhmm13k_filter_tileILi%dELi%dELb%dEdLb0ELb0EEEv" % (nt, kind, full)).encode() in blob
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
        for word in ("smooth_tile", "smooth_tile_min_total", "k_smooth_tile_bwd", "k_filter_tile", "smooth_seglen",
                     "smooth_W", "smooth_ws_mb", "smooth_segments"):
            assert word in text, (anchor, word)
    ctx = open(os.path.join(CSRC, "ctx.hpp")).read()
    for word in ("int smooth_tile = -1", "smooth_tile_nseg", "smooth_tile_ntraj", "smooth_tile_seglen_opt",
                 "struct SmoothTileBufs", "} smooth_tile;"):
        assert word in ctx, word
    api = open(os.path.join(CSRC, "bhmm_amd.hip")).read()
    assert api.count('"smooth_tile"') == 2                       # a setter and a getter
    assert api.count('"smooth_tile_min_total"') == 1             # read-only: the getter alone
    assert "smooth_tile must be -1, 0 or 1" in api


def test_threshold_is_a_power_of_two_not_below_the_floor():
    internal = open(os.path.join(CSRC, "host_internal.hpp")).read()
    m = re.search(r"SMOOTH_TILE_MIN_TOTAL\s*=\s*(\d+)\s*;", internal)
    assert m
    v = int(m.group(1))
    assert v >= 32768 and v & (v - 1) == 0


def test_kernel_header_builds_on_the_family_and_the_makefile_has_the_objects():
    text = open(os.path.join(CSRC, "smooth_tile_kernels.hpp")).read()
    for inc in ("tile_kernels.hpp", "score_tile_kernels.hpp", "filter_tile_kernels.hpp", "marg_kernels.hpp"):
        assert '#include "%s"' % inc in text
    for name in ("TileGeo<NT>", "SCORE_TILE_THREADS", "gauss_pdf4_issue(", "row16_sum(", "tile_prow(", "MARG_QMAX",
                 "WIDE_TROUBLE_EXP", "__builtin_amdgcn_mfma_f64_16x16x4f64", "m.A[(int64_t)j * n + i]"):
        assert name in text, name
    for defined in (r"struct\s+ScoreTileModel", r"struct\s+Segs\b", r"struct\s+TileGeo", r"double\s+row16_sum\s*\(",
                    r"MARG_QMAX\s*="):
        assert not re.search(defined, text), defined
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for nt in (5, 6, 7, 8):
        assert "$(OBJDIR)/smooth_tile_%d.o" % nt in mk
    assert "$(OBJDIR)/smooth_tile.o" in mk and "smooth_tile_nt.hip" in mk and "-DSMOOTH_TILE_NT_VALUE=$*" in mk
    # the forward half is launched, not copied: the units instantiate no k_filter_tile of their own
    unit = open(os.path.join(CSRC, "smooth_tile.hip")).read()
    assert "filter_tile_launch<" in unit and "FILTER_TILE_LAUNCH_DECL(extern," in unit
    assert "FILTER_TILE_LAUNCH_DECL(," not in unit
    assert "k_filter_tile" not in open(os.path.join(CSRC, "smooth_tile_nt.hip")).read()


# ---- the ranges of the budgeted workspace and their tile tables ---------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """built once, with the address and undefined-behaviour sanitizers, as a stand-alone program"""
    exe = str(tmp_path_factory.mktemp("smooth_tile_ranges") / "smooth_tile_ranges_driver")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bhmm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "smooth_tile_ranges_driver.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def _plan(exe, row_bytes, budget, seglen, lengths):
    r = subprocess.run([exe, str(row_bytes), str(budget), str(seglen)] + [str(int(x)) for x in lengths],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    segs, ranges, tiles = [], [], {"tilef": [], "tileb": []}
    for line in r.stdout.decode().splitlines():
        tag, *v = line.split()
        v = [int(x) for x in v]
        if tag == "seg":
            segs.append(tuple(v))
        elif tag == "range":
            ranges.append(tuple(v))
        else:
            assert len(v) == 16
            tiles[tag].append(v)
    _invariants(segs, ranges, tiles, row_bytes, budget, lengths)
    return segs, ranges, tiles


def _invariants(segs, ranges, tiles, row_bytes, budget, lengths):
    """every segment in exactly one range; every range's tile tables hold exactly its segments, once per direction;
    edge-class segments in tiles of their own; within the budget unless the range is a single segment"""
    nseg = len(segs)
    assert sum(ln for _, _, ln in segs) == sum(lengths)
    assert (ranges[0][0] if ranges else 0) == 0 and (ranges[-1][1] if ranges else 0) == nseg
    f_next = b_next = 0
    for i, (s0, s1, steps, f0, nf, b0, nb) in enumerate(ranges):
        assert s0 < s1
        if i:
            assert s0 == ranges[i - 1][1]
        assert steps == sum(ln for _, _, ln in segs[s0:s1])
        if budget > 0 and steps * row_bytes > budget:
            assert s1 - s0 == 1
        if budget > 0 and s1 < nseg:                 # greedy: the next segment would not have fitted
            assert (steps + segs[s1][2]) * row_bytes > budget
        assert (f0, b0) == (f_next, b_next)          # the tables are concatenated in range order
        f_next, b_next = f0 + nf, b0 + nb
        for tag, t0, nt, backward in (("tilef", f0, nf, False), ("tileb", b0, nb, True)):
            mine = tiles[tag][t0:t0 + nt]
            named = sorted(s for tile in mine for s in tile if s >= 0)
            assert named == list(range(s0, s1)), (tag, i)
            for tile in mine:
                live = [s for s in tile if s >= 0]
                assert live, "an empty tile"
                assert tile[:len(live)] == live      # (empty slots behind the segments)
                edge = set()
                for s in live:
                    traj, t_start, ln = segs[s]
                    edge.add(t_start + ln >= lengths[traj] if backward else t_start == 0)
                assert len(edge) == 1, (tag, tile)
    assert f_next == len(tiles["tilef"]) and b_next == len(tiles["tileb"])


LENGTHS = [20000, 7000, 1, 12345, 64, 3001]


def test_budget_below_one_segment_gives_one_segment_per_range(driver):
    segs, ranges, tiles = _plan(driver, 128 * 8, 1000, 1000, LENGTHS)
    assert len(ranges) == len(segs) and all(r[1] - r[0] == 1 and r[4] == 1 and r[6] == 1 for r in ranges)


def test_exact_fit(driver):
    row = 100 * 8
    segs, ranges, _ = _plan(driver, row, 2000 * row, 1000, [4000, 4000])
    assert [ln for _, _, ln in segs] == [1000] * 8
    assert [r[:3] for r in ranges] == [(0, 2, 2000), (2, 4, 2000), (4, 6, 2000), (6, 8, 2000)]
    _, ranges, _ = _plan(driver, row, 2000 * row - 1, 1000, [4000, 4000])
    assert [r[:3] for r in ranges] == [(s, s + 1, 1000) for s in range(8)]


def test_budget_zero_gives_one_range_which_is_the_whole_plan(driver):
    segs, ranges, tiles = _plan(driver, 128 * 8, 0, 256, LENGTHS)
    assert len(ranges) == 1 and ranges[0][:3] == (0, len(segs), sum(LENGTHS))
    # the forward table of the whole plan is plan_tiles' own: the classes in order, longest first inside each
    assert _plan(driver, 128 * 8, 1 << 40, 256, LENGTHS)[1:] == (ranges, tiles)
    assert _plan(driver, 65 * 8, 0, 256, []) == ([], [], {"tilef": [], "tileb": []})


def test_ragged_last_range(driver):
    segs, ranges, _ = _plan(driver, 8, 8 * 3000, 1000, [7000, 17])
    assert [ln for _, _, ln in segs] == [1000] * 7 + [17]
    assert [r[:3] for r in ranges] == [(0, 3, 3000), (3, 6, 3000), (6, 8, 1017)]


def test_ranges_whose_segment_count_is_no_multiple_of_16(driver):
    # 40 segments of 256 and one of 1: ranges of 17 (two classes, so 1 + 16 -> 2 tiles forward), 17 and 7
    segs, ranges, tiles = _plan(driver, 8, 8 * 17 * 256, 256, [40 * 256, 1])
    assert [r[1] - r[0] for r in ranges] == [17, 17, 7]
    assert ranges[0][4] == 2 and ranges[0][6] == 2       # forward: the trajectory's first segment alone + 16
    assert ranges[1][4] == 2 and ranges[1][6] == 2       # 17 segments of one class: 16 + 1
    assert ranges[2][4] == 2 and ranges[2][6] == 2       # forward: the one-step trajectory starts (edge) + 6 others;
    #                                                      backward: two segments end a trajectory (edge) + 5 others
    # a long segment alone exceeds the budget and still gets its range
    _, ranges, _ = _plan(driver, 8, 8 * 100, 0, [10, 5000, 10, 10, 10])
    assert [r[:3] for r in ranges] == [(0, 1, 10), (1, 2, 5000), (2, 5, 30)]
