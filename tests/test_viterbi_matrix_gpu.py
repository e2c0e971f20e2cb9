"""Segment-parallel Viterbi over EVERY instantiation, emission kind and segment edge, byte for byte against the C
oracle: orc.viterbi(A, pobs, pi) on orc.pobs_gaussian / orc.pobs_discrete, np.array_equal, no tolerance anywhere.

Every case checks eng.viterbi (int32) and eng.viterbi_u8, and asserts WHICH kernel produced the path -- the library
hands a call to the serial kernel whenever a segmented pass is not accepted, and the result is then still right:
    segmented / chunked plan meant:  viterbi_chunked == 1 and, from 9 states on, viterbi_segments > trajectories;
    serial kernel meant:             viterbi_chunked == 0.
viterbi_seg_per_simd = 1 throughout, so that batches of a few thousand steps are cut into segments at all.

What the dispatch tables say (and the cases follow):
  * 8 states and fewer (path_api.hip, chunk_viterbi): k_viterbi_chunks<4 | 8, KIND, MARGIN> on the chunk plan of
    set_observations(chunk=...); four lanes per chunk up to 4 states, eight above.  MARGIN = true is a second pass that
    runs only when some boundary is within tolerance but not bit-identical.  No fix-up rounds here.
  * 9 .. 64 states (wide_seg_viterbi): k_wide_viterbi_seg<16 | 32 | 64, KIND, FIX>.  Gaussian and discrete observations are evaluated in
    the step (KIND as given); FIX = true is a fix-up round or the mending round.
  * 65 .. 128 states (gen_api.hip, gen_seg_viterbi): k_gen_viterbi_seg<FIX> on a materialised emission matrix
    (gen_pobs), so the kind only changes how that matrix is made.
  * 129 .. 256 states (gen_rows_viterbi): k_gen_viterbi_rows<4, 2[, MEND]>, first pass only: NO fix-up rounds exist
    (seg_viterbi is called with max_rounds = 0), a pass that is neither bit-identical nor accepted by the margins goes to
    the serial kernel.
  * 257 states and more (gen_serial_viterbi): k_gen_viterbi_fwd, serial.

The conditions the forced cases rest on ("this warm-up leaves boundaries that differ", "the ties lie on the path",
"exactly these rows are ones") are established on the same inputs in tests/test_viterbi_matrix_cpu.py.

Which test executes which instantiation (G, D, E: gaussian, discrete, explicit; [..] the test's parameters):
  k_viterbi_chunks<4, G|D|E, false>      test_chunk_plans_8_states_and_fewer[2|3|4-kind]
  k_viterbi_chunks<4, G|D|E, true>       test_margin_pass_8_states_and_fewer[4-kind]      (pass ran and was accepted)
  k_viterbi_chunks<8, G|D|E, false>      test_chunk_plans_8_states_and_fewer[5|7|8-kind]
  k_viterbi_chunks<8, G|D|E, true>       test_margin_pass_8_states_and_fewer[8-kind]
  k_wide_viterbi_seg<16, G|D|E, false>   test_default_policy_9_to_64_states[9|15|16-kind]
  k_wide_viterbi_seg<16, G|D|E, true>    test_forced_fixup_rounds_9_to_64_states[9|15|16-kind]   (rounds >= 1 asserted)
  k_wide_viterbi_seg<32, G|D|E, false>   test_default_policy_9_to_64_states[17|31|32-kind]
  k_wide_viterbi_seg<32, G|D|E, true>    test_forced_fixup_rounds_9_to_64_states[17|31|32-kind]
  k_wide_viterbi_seg<64, G|D|E, false>   test_default_policy_9_to_64_states[33|48|63|64-kind]
  k_wide_viterbi_seg<64, G|D|E, true>    test_forced_fixup_rounds_9_to_64_states[33|48|63|64-kind]
  ... <16|32|64, G, true> as mending     test_forced_mismatch_with_mending_and_margins_on[15|31|63]
  k_gen_viterbi_seg<false>               test_above_64_states[65|66|127|128-kind]
  k_gen_viterbi_seg<true>                test_forced_mismatch_above_64_states[66-gaussian-32]   (mending and rounds)
      (no KIND: gen_api.hip, gen_viterbi_run calls gen_pobs first and the kernel reads the matrix, VitCall::obs)
  k_gen_viterbi_rows<4, 2>               test_above_64_states[129|130|255|256-kind]
  k_gen_viterbi_rows<4, 2, true>         test_forced_mismatch_above_64_states[130-gaussian-128]   (mended pass accepted)
      (no fix-up round at 129..256: gen_rows_viterbi passes max_rounds = 0 to seg_viterbi and its f.pass ignores `fix`)
  k_gen_viterbi_fwd                      test_257_states_take_the_serial_kernel; k_wide_viterbi_fwd<8|16|32|64, kind>:
                                         the serial halves of test_twin_states_across_the_seams and
                                         test_serial_fallback_8_states_and_fewer

Every case prints one line with the counters of its calls."""
import numpy as np
import pytest

from tests import viterbi_matrix_cases as vc

pytestmark = pytest.mark.gpu

COUNTERS = ("viterbi_chunked", "viterbi_segments", "viterbi_W", "viterbi_mismatch", "viterbi_far", "viterbi_rounds",
            "viterbi_mended", "viterbi_margin_used", "viterbi_margin_close", "viterbi_close", "spec_last_dev")


_device_checked = []


def _assert_device():
    """the segment counts asserted below restate the planner for 4 x 256 SIMDs (vc.NUM_SIMD); the library sizes its
    plans by 4 x hipDeviceAttributeMultiprocessorCount, which is what torch reports"""
    if not _device_checked:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert 4 * cus == vc.NUM_SIMD, "this device has %d compute units: the plans restated in " \
            "tests/viterbi_matrix_cases.py are those of %d" % (cus, vc.NUM_SIMD // 4)
        _device_checked.append(cus)


def _engine(c, before=(), after=(), chunk=0):
    """an engine on the case's observations; `before` / `after`: options set before / after set_observations (the
    adaptive state of an observation set -- viterbi_W, the margin rule's "wanted" -- is reset by set_observations)"""
    from bhmm_amd.engine import Engine
    _assert_device()
    eng = Engine(0)
    eng.set_option("viterbi_seg_per_simd", 1)
    for name, value in before:
        eng.set_option(name, value)
    eng.set_observations(c["kind"], c["obs"], c["n"], nsymbols=c["nsymbols"], chunk=chunk)
    for name, value in after:
        eng.set_option(name, value)
    return eng


def _counters(eng):
    return {k[8:] if k.startswith("viterbi_") else k: eng.get_option(k) for k in COUNTERS}


def _assert_kernel(c, s, meant, label):
    if meant == "segmented":
        assert s["chunked"] == 1, "%s: the serial kernel decided (%s)" % (label, s)
        if c["n"] >= 9:
            assert s["segments"] > len(c["lengths"]), "%s: %d segments" % (label, s["segments"])
    elif meant == "serial":
        assert s["chunked"] == 0, "%s: not the serial kernel (%s)" % (label, s)


def _run(eng, c, label, meant="segmented", calls=1, first=None):
    """`calls` x viterbi and one viterbi_u8, each compared with the oracle and each with the kernel assertion;
    first(counters): further assertions on the first call.  Returns the counters of every call."""
    ref = vc.case_reference(c)
    m = c["model"]
    seen = []
    for i in range(calls):
        paths = eng.viterbi(*m)
        s = _counters(eng)
        seen.append(s)
        for k, (p, r) in enumerate(zip(paths, ref)):
            assert p.dtype == np.int32 and np.array_equal(p, r), \
                "%s, call %d, trajectory %d: %d of %d steps differ, first at %d (%s)" % (
                    label, i, k, int((p != r).sum()), len(r), int(np.flatnonzero(p != r)[0]), s)
        _assert_kernel(c, s, meant, "%s, call %d" % (label, i))
        if i == 0 and first is not None:
            first(s)
    if c["n"] <= 256:                # (one byte per step holds 256 states)
        p8 = eng.viterbi_u8(*m)
        s = _counters(eng)
        seen.append(s)
        r8 = np.concatenate(ref).astype(np.uint8)
        assert p8.dtype == np.uint8 and np.array_equal(p8, r8), \
            "%s, viterbi_u8: %d steps differ (%s)" % (label, int((p8 != r8).sum()), s)
        _assert_kernel(c, s, meant, label + ", viterbi_u8")
    print("%s: " % label + " | ".join(
        "chunked %d segs %d W %d mism %d far %d rounds %d mended %d margin %d/%d close %d dev %.2g" % (
            s["chunked"], s["segments"], s["W"], s["mismatch"], s["far"], s["rounds"], s["mended"], s["margin_used"],
            s["margin_close"], s["close"], s["spec_last_dev"]) for s in seen))
    return seen


# ---- 1. the instantiation matrix, 9 to 64 states -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", vc.KINDS)
@pytest.mark.parametrize("n", vc.S1_STATES)
def test_default_policy_9_to_64_states(n, kind):
    """k_wide_viterbi_seg<NP, KIND, false> (and <.., true> where the policy needs a round): ragged lengths with 1, 2, a
    trajectory shorter than the warm-up and long ones; three calls."""
    c = vc.s1a_case(n, kind)
    eng = _engine(c)
    try:
        _run(eng, c, "n=%d %s default" % (n, kind), calls=3)
    finally:
        eng.close()


def _rounds_ran(s):
    assert s["mismatch"] >= 1 and s["rounds"] >= 1, s


@pytest.mark.parametrize("kind", vc.KINDS)
@pytest.mark.parametrize("n", vc.S1_STATES)
def test_forced_fixup_rounds_9_to_64_states(n, kind):
    """k_wide_viterbi_seg<NP, KIND, true> as a fix-up round: the slowly forgetting model, a warm-up of 16 steps and the
    margin rule off.  That this warm-up leaves boundaries that differ is established in test_viterbi_matrix_cpu.py
    (test_forced_warmup_leaves_boundaries_that_differ); here the rounds must have run, and the paths are the
    oracle's.  The plan is the one restated there: segments of 2 W (of 4 W if the library doubled the warm-up)."""
    c = vc.s1b_case(n, kind)
    eng = _engine(c, before=[("viterbi_margin", 0)], after=[("viterbi_W", vc.S1B_W)])
    try:
        seen = _run(eng, c, "n=%d %s forced rounds" % (n, kind), calls=3, first=_rounds_ran)
        assert seen[0]["margin_used"] == 0 and seen[0]["mended"] == 0
        total = sum(c["lengths"])
        plans = [len(vc.plan(c["lengths"], vc.seglen_wide(total, n, W))) for W in (vc.S1B_W, 2 * vc.S1B_W)]
        assert seen[0]["segments"] in plans, (seen[0]["segments"], plans)
    finally:
        eng.close()


@pytest.mark.parametrize("n", [15, 31, 63])
def test_forced_mismatch_with_mending_and_margins_on(n):
    """The same once per NP with the margin rule asked for at once and the mending round allowed: the segments that are
    far run again alone (k_wide_viterbi_seg<NP, KIND, true> with a tolerance) when they are at most half of all, else
    the rounds run."""
    c = vc.s1b_case(n, "gaussian")

    def first(s):
        assert s["mismatch"] >= 1 and (s["mended"] >= 1 or s["rounds"] >= 1), s
    eng = _engine(c, after=[("viterbi_margin", 2), ("viterbi_mend", 1), ("viterbi_W", vc.S1B_W)])
    try:
        _run(eng, c, "n=%d gaussian forced, mending and margins on" % n, calls=3, first=first)
    finally:
        eng.close()


# ---- 2. eight states and fewer --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", vc.KINDS)
@pytest.mark.parametrize("n", vc.S2_STATES)
def test_chunk_plans_8_states_and_fewer(n, kind):
    """k_viterbi_chunks<4 | 8, KIND, .> on chunks of 16, 64 and 300 steps over lengths (5000, 1, 2, 257, 63); three
    calls each (later calls try a shorter warm-up).  A model that forgets quickly: the chunked run stands.
    viterbi_close and spec_last_dev are printed, not asserted."""
    c = vc.s2_case(n, kind)
    for chunk in vc.S2_CHUNKS:
        eng = _engine(c, chunk=chunk)
        try:
            _run(eng, c, "n=%d %s chunk=%d" % (n, kind, chunk), calls=3)
        finally:
            eng.close()


@pytest.mark.parametrize("kind", vc.KINDS)
@pytest.mark.parametrize("n", vc.S2_STATES)
def test_serial_fallback_8_states_and_fewer(n, kind):
    """spec_W = 2 on a model that hardly forgets: the warm-ups of 2, 4 and 8 steps leave boundaries out of tolerance
    (test_viterbi_matrix_cpu.py), the serial kernel decides."""
    c = vc.s2_case(n, kind, slow=True)
    for chunk in vc.S2_CHUNKS:
        eng = _engine(c, before=[("spec_W", 2)], chunk=chunk)
        try:
            _run(eng, c, "n=%d %s chunk=%d spec_W=2" % (n, kind, chunk), meant="serial")
        finally:
            eng.close()


@pytest.mark.parametrize("kind", vc.KINDS)
@pytest.mark.parametrize("layout", [4, 8])
def test_margin_pass_8_states_and_fewer(layout, kind):
    """k_viterbi_chunks<4 | 8, KIND, true>, the pass that counts close decisions, is launched only when some chunk
    boundary is within the tolerance (1e-11) but not bit-identical (path_api.hip: the loop over `pass`) -- read off
    spec_last_dev, the largest deviation of the last check: 0 < dev <= 1e-11.  Such boundaries are rare (the vectors
    of two starts are far apart or, a few steps later, the same to the bit), so every state count of the layout is run
    with warm-ups from 8 to 64 steps over 312 chunks of 16 steps, and the paths of every call are the oracle's.  A
    call that ran the pass is accepted exactly when the pass counted no close decision (path_api.hip: done = ... ||
    (h[0] == 0 && h[2] == 0)), so on those calls viterbi_chunked == (viterbi_close == 0) is asserted, and per
    (layout, kind) cell at least one of them must have been accepted: its back-pointers, written by the MARGIN = true
    instantiation, are then what was compared with the oracle.  (Section 2 of the issue prints viterbi_close and
    spec_last_dev without asserting them; here spec_last_dev serves only as the did-it-run check of this extra
    test, and viterbi_close only to say which kernel's path was compared.)"""
    ran = []
    for n in (2, 3, 4) if layout == 4 else (5, 7, 8):
        c = vc.s2_case(n, kind)
        eng = _engine(c, chunk=16)
        try:
            for W in vc.S2_MARGIN_W:
                eng.set_option("spec_W", W)
                seen = _run(eng, c, "n=%d %s chunk=16 spec_W=%d" % (n, kind, W), meant=None)
                for s in seen:
                    if 0.0 < s["spec_last_dev"] <= 1e-11:
                        assert (s["chunked"] == 1) == (s["close"] == 0), (n, W, s)
                        ran.append((n, W, s["spec_last_dev"], int(s["chunked"])))
        finally:
            eng.close()
    print("layout %d %s: the pass with the close-decision count ran at (n, spec_W, deviation, accepted) %s"
          % (layout, kind, ran))
    assert ran, "no call had boundaries within tolerance that were not bit-identical"
    assert any(r[3] == 1 for r in ran), "no call that ran the pass was accepted: %s" % (ran,)


# ---- 3. ties that a seam decides ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", [(n, k) for n in sorted(vc.TWINS) for k in vc.TWIN_KINDS[n]])
def test_twin_states_across_the_seams(n, kind):
    """State i' an exact copy of state i: v[i] == v[i'] to the bit at every step, every decision a twin wins is a tie
    and the first maximum -- the lower index -- is the reference's.  The pairs straddle octets, rows of 16, halves of
    a wavefront (3 | 35), the ends (0 | n - 1), the two target states of a lane of k_gen_viterbi_seg (63 | 64 | 65 and
    0 | 127) and the candidate ranges of k_gen_viterbi_rows (103 | 104 and 0 | 199 of 200).  That the lower twins are on the path
    (and end trajectories) is established in test_viterbi_matrix_cpu.py.  Segmented, then the serial kernels."""
    c = vc.twin_case(n, kind)
    chunk = 64 if n <= 8 else 0
    eng = _engine(c, chunk=chunk)
    try:
        _run(eng, c, "n=%d %s twins" % (n, kind), calls=2)
    finally:
        eng.close()
    eng = _engine(c, before=[("spec_enabled", 0)], chunk=chunk)
    try:
        _run(eng, c, "n=%d %s twins, serial" % (n, kind), meant="serial")
    finally:
        eng.close()


# ---- 4. geometry --------------------------------------------------------------------------------------------------------------
S4_CASES = [(n, k) for n in vc.S4_STATES for k in vc.S4_KINDS]


def _geo(n, kind, lengths, tag, label, nseg=None):
    c = vc.s4_case(n, kind, lengths, tag)
    want = len(vc.plan(lengths, vc.s4_seglen(n, sum(lengths)))) if nseg is None else nseg
    eng = _engine(c)
    try:
        # (one segment per trajectory "is the serial kernel", path_api.hip: the plan is made, the pass is not run)
        seen = _run(eng, c, "n=%d %s %s" % (n, kind, label), meant="serial" if want <= len(lengths) else "segmented")
        for s in seen:
            assert s["segments"] == want, "%s: %d segments, meant %d" % (label, s["segments"], want)
    finally:
        eng.close()


@pytest.mark.parametrize("n,kind", S4_CASES)
def test_every_phase_of_the_64_step_grid(n, kind):
    """A trajectory of p = 1, 37, 63, 64, 65 steps in front of one of 6000: the long one starts at o0 & 63 = p & 63 --
    the observation register of the 64-state kernel reloads at (gt - (o0 + tw)) & 63 == 0, checkpoints are written at
    ((o0 + tw) + r) & 63 == 63.  And fifteen trajectories of 1 .. 15 steps in front of it (o0 = 120)."""
    for p in vc.S4_PHASES:
        _geo(n, kind, (p, 6000), p, "phase %d" % p)
    _geo(n, kind, tuple(range(1, 16)) + (6000,), 100, "1..15 in front")


@pytest.mark.parametrize("n,kind", S4_CASES)
def test_lengths_around_the_reload_the_checkpoint_and_the_walk_plan(n, kind):
    """63 .. 65, 127 .. 129, 255 .. 257 and 511 .. 513 steps (64: reload and checkpoint; 256: the shortest segment of
    the walks' own plan) next to 6000 steps, without which the batch would not be segmented at all."""
    _geo(n, kind, vc.S4_RELOAD, 200, "63..513")


@pytest.mark.parametrize("n,kind", S4_CASES)
def test_segment_counts_around_the_lane_groups(n, kind):
    """One trajectory of exactly s segments, s around the multiples of the segments per wavefront and per workgroup
    (4 and 16 at NP 16, 2 and 8 at NP 32, 1 and 4 at NP 64; the eight wavefronts of k_gen_viterbi_seg; the four rows
    of k_gen_viterbi_rows).  The count is read back and asserted.  64 states, one segment: the planner makes the
    plan of one segment and the call goes to the serial kernel, which is asserted."""
    for s in vc.S4_COUNTS[n]:
        T = vc.s4_count_length(n, s)
        _geo(n, kind, (T,), 300 + s, "%d segments" % s, nseg=s)


# ---- 5. the ones rule inside the step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", vc.S5_STATES)
def test_all_underflow_rows_inside_segments_and_warmups(n):
    """Gaussian observations 60 sigma and more from every state -- a row of zeros that outputmodel.py:126-130 turns
    into ones -- at step 0, the last step, the first and last step of an interior segment, inside a warm-up and, at 64
    states, on a reload step of the observation register and on the step before one.  The rule lives in the step of
    k_wide_viterbi_seg (a ballot over the lanes of the segment's group, wgroup_mask -- padding lanes are IN that mask
    and stay out of the way only because their density is an exact zero, cn_j = 0) and nothing in wide_seg_viterbi
    looks at it: the segmented run stands (a row of ones is a step like any other for the boundary check)."""
    c = vc.s5_case(n)
    eng = _engine(c)
    try:
        seen = _run(eng, c, "n=%d ones rule" % n, calls=3)
        assert seen[0]["segments"] == c["nseg"], (seen[0]["segments"], c["nseg"])
    finally:
        eng.close()


# ---- 6. above 64 states ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", vc.S6_CASES)
def test_above_64_states(n, kind):
    """k_gen_viterbi_seg (65, 66, 127, 128: one and two target states in the last lanes) and k_gen_viterbi_rows<4, 2>
    (129, 130, 255, 256), lengths (6000, 1, 700, 2); three calls."""
    c = vc.s6_case(n, kind)
    eng = _engine(c)
    try:
        _run(eng, c, "n=%d %s" % (n, kind), calls=3)
    finally:
        eng.close()


@pytest.mark.parametrize("n,kind,W", vc.S6_FORCED)
def test_forced_mismatch_above_64_states(n, kind, W):
    """A warm-up that leaves boundaries that differ (test_viterbi_matrix_cpu.py, test_forced_warmup_above_64_states):
    k_gen_viterbi_seg<true> as mending or fix-up round at 66 states; k_gen_viterbi_rows<4, 2, true>, the mending
    round, at 130.  There a mended pass that is not accepted (a segment that does not meet a kept vector, or a close
    decision on the path) goes to the serial kernel and the mending kernel's splices would be compared with nothing:
    so model and warm-up are chosen (the far boundaries counted on the CPU) such that the mended pass IS accepted,
    and viterbi_chunked == 1, viterbi_segments > trajectories and mended >= 1 are asserted on it."""
    c = vc.s6_forced_case(n, kind)

    def first(s):
        assert s["mismatch"] >= 1 and (s["mended"] >= 1 or s["rounds"] >= 1), s
        if n > 128:
            assert s["mended"] >= 1 and s["rounds"] == 0 and s["margin_used"] == 1, s
    eng = _engine(c, after=[("viterbi_W", W)])
    try:
        _run(eng, c, "n=%d %s forced W=%d" % (n, kind, W), calls=3, first=first)
    finally:
        eng.close()


def test_257_states_take_the_serial_kernel():
    """three trajectories, batched, through the engine: k_gen_viterbi_fwd (no segmented kernel above 256 states)"""
    c = vc.s257_case()
    eng = _engine(c)
    try:
        _run(eng, c, "n=257", meant="serial", calls=2)
    finally:
        eng.close()
