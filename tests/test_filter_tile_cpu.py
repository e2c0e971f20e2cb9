"""No GPU: the matrix-core path of bhmm_filter for 65 to 128 states exists in the built library -- every
instantiation of k_filter_tile is in the gfx950 code object, the header, the context and the option table name the
new options, the threshold is admissible, the kernel header builds on the headers it names, and the Makefile has the
new objects."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bhmm_amd.h")
CSRC = os.path.join(ROOT, "bhmm_amd", "csrc")


def test_every_instantiation_is_in_the_gfx950_code_object():
    """NT = 5 .. 8 x gaussian / discrete x FULL or not x double / float x rows / projection x with / without logc"""
    from bhmm_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    names = set(m.decode() for m in re.findall(rb"_ZN4bhmm13k_filter_tileILi\d[A-Za-z0-9_]*", blob))
    want = set()
    for nt in (5, 6, 7, 8):
        for kind in (0, 1):
            for full in (0, 1):
                for ot in ("d", "f"):
                    for proj in (0, 1):
                        for lc in (0, 1):
                            want.add("_ZN4bhmm13k_filter_tileILi%dELi%dELb%dE%sLb%dELb%dEEEvPKNS_14ScoreTileModelEPKlNS_4SegsE"
                                     "NS_8TilePlanE" % (nt, kind, full, ot, proj, lc))
    assert len(want) == 128
    missing = [w for w in want if not any(x.startswith(w) for x in names)]
    assert not missing, missing[:4]
    assert b"k_filter_tile_redo" in blob and b"k_filter_tile_check" in blob
    # the kernels that were there before
    for ot in ("d", "f"):
        for kind in (0, 1, 2):
            assert ("_ZN4bhmm15k_filter_serialILi%dE%sEE" % (kind, ot)).encode() in blob
    assert len(set(re.findall(rb"_ZN4bhmm12k_score_tileILi\dELi\dELb\dEEEvPKNS_14ScoreTileModelE", blob))) == 16


def test_header_context_and_option_table_name_the_new_options():
    raw = open(HEADER).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*#define\s+BHMM_FILT_F32", raw, re.S)
    assert m, "the comment on bhmm_filter"
    text = m.group(1)
    for word in ("filter_tile", "filter_tile_min_total", "filter_redone", "filter_seglen", "filter_W", "filter_path",
                 "k_filter_tile"):
        assert word in text, word
    ctx = open(os.path.join(CSRC, "ctx.hpp")).read()
    for word in ("filter_tile", "filter_redone", "filt_tile_nseg", "filt_tile_ntiles", "filt_tile_seglen_opt",
                 "tile_seg"):
        assert word in ctx, word
    api = open(os.path.join(CSRC, "bhmm_amd.hip")).read()
    for word in ("filter_tile", "filter_tile_min_total", "filter_redone"):
        assert '"%s"' % word in api, word
    # filter_tile can be set, the other two are read-only: they appear in the getter alone
    assert api.count('"filter_tile"') == 2
    assert api.count('"filter_tile_min_total"') == 1 and api.count('"filter_redone"') == 1


def test_threshold_is_a_power_of_two_not_below_the_floor():
    internal = open(os.path.join(CSRC, "host_internal.hpp")).read()
    m = re.search(r"FILTER_TILE_MIN_TOTAL\s*=\s*(\d+)\s*;", internal)
    assert m
    v = int(m.group(1))
    assert v >= 32768 and v & (v - 1) == 0
    # the constants of the calibration are shared, not typed twice
    assert len(re.findall(r"constexpr\s+\w+\s+SCORE_TILE_MARGIN\s*=", internal)) == 1
    for unit in ("score_api.hip", "filter_api.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        assert not re.search(r"constexpr\s+\w+\s+SCORE_TILE_\w+\s*=", text), unit
        assert "score_tile_extrapolate(" in text, unit


def test_kernel_header_includes_what_it_builds_on():
    text = open(os.path.join(CSRC, "filter_tile_kernels.hpp")).read()
    for inc in ("tile_kernels.hpp", "score_kernels.hpp", "score_tile_kernels.hpp", "marg_kernels.hpp"):
        assert '#include "%s"' % inc in text
    # their helpers are used, not defined again
    for name in ("row16_sum(", "row16_max_i32(", "tile_prow(", "gauss_pdf4_issue(", "TileGeo<NT>", "MARG_QMAX",
                 "ScoreTileModel", "WIDE_TROUBLE_EXP"):
        assert name in text, name
    for defined in (r"struct\s+TileGeo", r"struct\s+ScoreTileModel", r"double\s+row16_sum\s*\(", r"int\s+tile_prow\s*\(",
                    r"void\s+gauss_pdf4_issue\s*\(", r"#define\s+WIDE_TROUBLE_EXP", r"MARG_QMAX\s*="):
        assert not re.search(defined, text), defined
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in text
    serial = open(os.path.join(CSRC, "filter_kernels.hpp")).read()
    assert re.search(r"const uint8_t \*__restrict__ only\)", serial)


def test_makefile_has_the_new_objects():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for nt in (5, 6, 7, 8):
        assert "$(OBJDIR)/filter_tile_%d.o" % nt in mk
    assert re.search(r"\$\(OBJDIR\)/filter_tile_%\.o:\s*filter_tile_nt\.hip\s+filter_tile_launch\.hpp\s+filter_tile_kernels\.hpp",
                     mk)
    assert "-DFILTER_TILE_NT_VALUE=$*" in mk
    for name in ("filter_tile_nt.hip", "filter_tile_launch.hpp", "filter_tile_kernels.hpp"):
        assert os.path.exists(os.path.join(CSRC, name)), name
