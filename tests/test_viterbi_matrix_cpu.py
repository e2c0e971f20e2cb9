"""The inputs of tests/test_viterbi_matrix_gpu.py, checked against the oracle alone (no GPU): what that file relies
on -- "this warm-up leaves boundaries that differ", "these ties lie on the path", "exactly these rows are ones" -- is
established here on the same cases (tests/viterbi_matrix_cases.py builds them from their arguments alone), not hoped
for there."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import viterbi_matrix_cases as vc


def test_planner_restatement():
    """plan() against the properties of plan::plan_segments the cases lean on: ceil(T / L) segments of a trajectory,
    boundaries on multiples of four, every step covered once"""
    for lengths, L in (((9001, 1, 2, 50, 6000, 300), 256), ((6000, 1, 2, 11, 3000), 32), ((4350,), 256), ((63, 64, 65), 64)):
        segs = vc.plan(lengths, L)
        for k, T in enumerate(lengths):
            mine = [(t0, ln) for kk, t0, ln in segs if kk == k]
            assert len(mine) == -(-T // L)
            assert mine[0][0] == 0 and sum(ln for _, ln in mine) == T
            assert all(t0 % 4 == 0 for t0, _ in mine)
            assert all(a[0] + a[1] == b[0] for a, b in zip(mine, mine[1:]))


# ---- section 1 (b): the forced warm-up leaves boundaries that differ ---------------------------------------------------
@pytest.mark.parametrize("kind", vc.KINDS)
@pytest.mark.parametrize("n", vc.S1_STATES)
def test_forced_warmup_leaves_boundaries_that_differ(n, kind):
    """Slowly forgetting model, W = 16, segments of 2 W = 32 steps: started from the uniform vector W steps early, the
    max-product vector at some segment boundary (the first 1500 steps of every trajectory are looked at) differs from
    the serial one by more than 1e-6 relative -- and, since the library doubles the warm-up once before it gives the
    observations up, the same for W = 32 on its segments of 64."""
    c = vc.s1b_case(n, kind)
    total = sum(c["lengths"])
    for W in (vc.S1B_W, 2 * vc.S1B_W):
        L = vc.seglen_wide(total, n, W)
        assert L == 2 * W                       # (not the device-filling length: the plan is the one restated here)
        dev = vc.case_boundary_deviation(c, L, W, upto=1500)
        worst = max(dev.values())
        off = sum(1 for d in dev.values() if d > 1e-6)
        print("n=%d %s W=%d: %d of %d boundaries further than 1e-6, worst %.3g" % (n, kind, W, off, len(dev), worst))
        if W == vc.S1B_W:
            assert worst > 1e-6


# ---- section 2: the slowly forgetting model defeats the warm-ups of 2, 4 and 8 steps -----------------------------------------
@pytest.mark.parametrize("kind", vc.KINDS)
@pytest.mark.parametrize("n", vc.S2_STATES)
def test_warmups_of_2_4_8_do_not_verify_for_8_states_and_fewer(n, kind):
    """spec_W = 2: k_viterbi_chunks is tried with 2, 4 and 8 steps (path_api.hip, three attempts, doubling).  Wherever
    the chunk plan cuts the long trajectory, that is not enough: at more than half of ALL positions (every fourth of
    the first 1500 is looked at; measured: two thirds at 2 states gaussian, all of them elsewhere) the vector reached
    from the uniform one is further than 1e-6 from the serial one -- the check's tolerance is 1e-11 -- so the serial
    kernel must decide."""
    c = vc.s2_case(n, kind, slow=True)
    A, pi = c["model"][0], c["model"][1]
    pobs = vc.pobs_of(kind, c["obs"], c["model"])[0]
    for W in (2, 4, 8):
        d = np.array(list(vc.boundary_deviation(A, pobs, pi, list(range(16, 1500, 4)), W).values()))
        assert (d > 1e-6).mean() > 0.5, (W, (d > 1e-6).mean())


# ---- section 3: the ties lie on the path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", [(n, k) for n in sorted(vc.TWINS) for k in vc.TWIN_KINDS[n]])
def test_twins_are_exact_copies_and_the_lower_one_is_on_the_path(n, kind):
    c = vc.twin_case(n, kind)
    A, pi, p0, p1 = c["model"]
    cls, twin = vc.twin_classes(n)
    pobs = vc.pobs_of(kind, c["obs"], c["model"])
    for i, j in vc.TWINS[n]:
        assert np.array_equal(A[i], A[j]) and np.array_equal(A[:, i], A[:, j]) and pi[i] == pi[j], (i, j)
        for po in pobs:
            assert np.array_equal(po[:, i], po[:, j]), (i, j)
    ref = vc.case_reference(c)
    flat = np.concatenate(ref)
    visits = np.bincount(flat, minlength=n)
    for i, j in vc.TWINS[n]:
        lo, hi = int(cls[i]), max(i, j)
        assert visits[lo] >= 20, "state %d visited %d times" % (lo, visits[lo])
        assert visits[hi] == 0 and (cls[i] == i or visits[i] == 0), (i, j)
    # the first-maximum rule of the FINAL state (_hidden.c:262-267) decides too: trajectories end in a twin class
    ends = [int(p[-1]) for p in ref]
    assert sum(1 for e in ends if e in twin) >= 2, ends
    print("n=%d %s: visits of the lower twins %s, final states %s" % (n, kind, [int(visits[t]) for t in twin], ends))


# ---- section 5: exactly the planted rows are ones ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", vc.S5_STATES)
def test_planted_observations_are_the_only_all_underflow_rows(n):
    c = vc.s5_case(n)
    _, _, mu, sig = c["model"]
    for k, o in enumerate(c["obs"]):
        po = orc.pobs_gaussian(o, mu, sig)
        ones = np.flatnonzero(np.all(po == 1.0, axis=1))
        want = sorted(c["where"].values()) if k == 1 else []
        assert list(ones) == want, (k, list(ones), want)
        assert np.all(po.sum(axis=1) > 0.0)
    # the places are where they are meant to be, in the plan of the GPU run
    L, W, o0 = c["seglen"], vc.S5_W, c["lengths"][0]
    segs = [(t0, ln) for k, t0, ln in vc.plan(c["lengths"], L) if k == 1]
    starts = [t0 for t0, _ in segs]
    w = c["where"]
    assert w["first step of a segment"] in starts[1:-1] and w["last step of a segment"] + 1 in starts[1:-1]
    t0 = min(s for s in starts if s > w["inside a warm-up"])
    assert t0 - W < w["inside a warm-up"] == t0 - W // 2
    if n == 64:
        for name, phase in (("run step & 63 == 0", 0), ("run step & 63 == 63", 63)):
            t = w[name]
            t0 = max(s for s in starts if s <= t)
            tw = t0 - W                                       # (the run of a segment starts W steps early)
            assert tw > 0 and t0 <= t < t0 + dict(segs)[t0]
            assert ((o0 + t) - (o0 + tw)) & 63 == phase


# ---- section 6: the forced cases above 64 states ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind,W", vc.S6_FORCED)
def test_forced_warmup_above_64_states(n, kind, W):
    """65..128 states (fix-up rounds exist): some boundary further than 1e-6.  129..256 (k_gen_viterbi_rows<4, 2, MEND>
    runs only when at most half of the boundaries are further than 1e-12, seg_viterbi in path_api.hip): at least one
    boundary further than 1e-6, and fewer than a third further than 1e-13."""
    c = vc.s6_forced_case(n, kind)
    L = vc.seglen_gen(sum(c["lengths"]), n, W)
    assert L == W
    dev = vc.case_boundary_deviation(c, L, W, upto=None if n > 128 else 1500)
    d = np.array(list(dev.values()))
    nseg = len(vc.plan(c["lengths"], L))
    print("n=%d %s W=%d: %d segments, %d boundaries further than 1e-6, %d further than 1e-13, worst %.3g"
          % (n, kind, W, nseg, (d > 1e-6).sum(), (d > 1e-13).sum(), d.max()))
    assert (d > 1e-6).sum() >= 1
    if n > 128:
        assert 3 * (d > 1e-13).sum() < nseg


def test_segment_counts_of_the_geometry_cases():
    """lengths of section 4 that give exactly s segments under the planner rule"""
    for n, counts in vc.S4_COUNTS.items():
        for s in counts:
            T = vc.s4_count_length(n, s)
            assert len(vc.plan((T,), vc.s4_seglen(n, T))) == s, (n, s, T)
