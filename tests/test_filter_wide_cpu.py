"""No GPU: the time-parallel path of bhmm_filter for 9 to 64 states exists in the built library -- all 72
instantiations of k_filter_wide are in the gfx950 code object, the header names the new options, and the inline
DPP instructions of the new translation unit keep their wait states (the check of tests/test_static_checks.py,
run over filter_wide.hip)."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bhmm_amd.h")
CSRC = os.path.join(ROOT, "bhmm_amd", "csrc")


def test_every_instantiation_is_in_the_gfx950_code_object():
    """16 / 32 / 64 lanes per segment x gaussian / discrete B^T in LDS / discrete B^T read ahead x double / float
    x rows / projection x with / without logc"""
    from bhmm_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    names = set(m.decode() for m in re.findall(rb"_ZN4bhmm13k_filter_wideILi\d[A-Za-z0-9_]*", blob))
    want = set()
    for np_ in (16, 32, 64):
        for kind, lds in ((0, 0), (1, 1), (1, 0)):
            for ot in ("d", "f"):
                for proj in (0, 1):
                    for lc in (0, 1):
                        want.add("_ZN4bhmm13k_filter_wideILi%dELi%dELb%dE%sLb%dELb%dEEEvPKNS_14ScoreWideModelEiPKlNS_4SegsE"
                                 % (np_, kind, lds, ot, proj, lc))
    assert len(want) == 72
    missing = [w for w in want if not any(x.startswith(w) for x in names)]
    assert not missing, missing[:4]
    # the segment counterparts of the check and the fix-up, and the kernels that were there before
    assert b"k_filter_seg_check" in blob
    for ot in ("d", "f"):
        assert ("_ZN4bhmm17k_filter_seg_buryI%sEE" % ot).encode() in blob
        for kind in (0, 1, 2):
            assert ("_ZN4bhmm15k_filter_serialILi%dE%sEE" % (kind, ot)).encode() in blob
    assert len(set(re.findall(rb"_ZN4bhmm14k_filter_sweepILi\dELi\dELb\dE[df]Lb\dELb\dEEEvPKNS_5ModelIXT_EEEiNS_6ChunksEi",
                              blob))) == 256


def test_header_names_the_new_options():
    raw = open(HEADER).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*#define\s+BHMM_FILT_F32", raw, re.S)
    assert m, "the comment on bhmm_filter"
    text = m.group(1)
    for word in ("filter_seglen", "filter_parallel", "filter_segments", "filter_wide_min_total", "filter_W",
                 "filter_fallbacks", "filter_path", "k_filter_wide"):
        assert word in text, word
    ctx = open(os.path.join(CSRC, "ctx.hpp")).read()
    for word in ("filter_seglen", "filter_parallel", "filter_segments", "filt_nseg", "filt_seglen_opt"):
        assert word in ctx, word
    api = open(os.path.join(CSRC, "bhmm_amd.hip")).read()
    for word in ("filter_seglen", "filter_parallel", "filter_segments", "filter_wide_min_total"):
        assert '"%s"' % word in api, word
    internal = open(os.path.join(CSRC, "host_internal.hpp")).read()
    m = re.search(r"FILTER_WIDE_MIN_TOTAL\s*=\s*(\d+)\s*;", internal)
    assert m and int(m.group(1)) >= 32768 and int(m.group(1)) & (int(m.group(1)) - 1) == 0


def test_kernel_headers_it_builds_on_are_included_not_copied():
    text = open(os.path.join(CSRC, "filter_wide_kernels.hpp")).read()
    for inc in ("wide_kernels.hpp", "score_kernels.hpp", "score_wide_kernels.hpp"):
        assert '#include "%s"' % inc in text
    assert "rows_of_group<NP>" in text and "dot16(" in text and "wgroup_sum<NP>" in text
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(OBJDIR)/filter_wide.o" in mk and "filter_wide.hip" in mk


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc') and shutil.which('hipcc') is None,
                    reason='needs hipcc')
def test_inline_dpp_instructions_of_the_new_unit_keep_their_wait_states():
    """tools/check_dpp_hazard.py over the assembly of filter_wide.hip: no VALU instruction writes a DPP source
    within the two wait states before its read"""
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    tmp = tempfile.mkdtemp(prefix='fwdpp')
    try:
        out = os.path.join(tmp, 'filter_wide.s')
        subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-munsafe-fp-atomics',
                               '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC, '--cuda-device-only', '-S',
                               os.path.join(CSRC, 'filter_wide.hip'), '-o', out], stderr=subprocess.DEVNULL,
                              timeout=900)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'check_dpp_hazard.py'), out],
                           capture_output=True, text=True, timeout=900)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'instructions checked, 0 hazard(s)' in r.stdout
    assert int(r.stdout.split()[0]) > 1000
