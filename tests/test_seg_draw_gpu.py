"""The protocol around the segment-parallel backward draw (csrc/path_api.hip: seg_draw) at 9..64 and at more than
64 states: fix-up rounds, the serial fallback of a call in which a draw found no state, and the repeat of a call
on exact alpha rows -- with the counters each of them leaves.  Paths and counts are the oracle's
(_hidden.c:283-305,330-378), state for state, on the caller's uniforms."""
import functools

import numpy as np
import pytest

from bhmm_amd import _lib
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

CASES = [(20, "discrete"), (64, "gaussian"), (100, "gaussian")]
LENGTHS = (9000, 1, 300)       # 64-step segments (the shortest), about 145 of them against 3 trajectories
M = 18


def _model(n, rng, kind):
    A = rng.random((n, n)) + 0.05
    A += np.eye(n) * (2.0 + 0.05 * n)
    A /= A.sum(axis=1)[:, None]
    pi = rng.dirichlet(np.ones(n))
    if kind == "gaussian":
        return A, pi, np.linspace(-6, 6, n), rng.uniform(0.6, 1.4, n)
    return A, pi, rng.dirichlet(np.ones(M), n), None


def _plant(alpha, A, u, steps, delta=1e-12):
    """u with the uniforms of `steps` moved to delta above / below (alternating) an interior edge of the reference's
    cumulative sums at that step, given the states the unchanged later steps draw (a change at t only moves steps
    <= t, so the steps are planted from the top): draws that any watch records.  Returns (u, how many it planted)."""
    u = u.copy()
    T, n = alpha.shape
    planted = 0
    for j, t in enumerate(sorted(steps, reverse=True)):
        path = orc.sample_path(alpha, A, u=u)
        ps = alpha[t].copy() if t == T - 1 else alpha[t] * A[:, path[t + 1]]      # _hidden.c:349 / :365
        S = 0.0
        for x in ps:
            S += x                                                              # _normalize, ascending
        p = ps / S
        acc = np.cumsum(p)
        cand = [q for q in range(n - 1) if p[q] > 1e-4 and p[q + 1] > 1e-4 and 1e-3 < acc[q] < 1 - 1e-3]
        if cand:
            u[t] = acc[cand[len(cand) // 2]] * (1.0 + (1 if j % 2 == 0 else -1) * delta)
            planted += 1
    return u, planted


@functools.lru_cache(maxsize=None)
def _case(n, kind):
    """(model, observations, uniforms, the oracle's paths, its counts): computed once per case, never written to.
    The uniforms are valid ones; six of the long trajectory's sit 1e-12 from a cumulative-sum edge, so that a
    watch has draws to record (random ones come that close once in a million calls)."""
    rng = np.random.default_rng(7300 + n)
    model = _model(n, rng, kind)
    A, pi, p0, p1 = model
    if kind == "gaussian":
        obs = [rng.normal(0, 3.5, T) for T in LENGTHS]
        pobs = [orc.pobs_gaussian(o, p0, p1) for o in obs]
    else:
        obs = [rng.integers(0, M, T).astype(np.int32) for T in LENGTHS]
        pobs = [orc.pobs_discrete(o, p0) for o in obs]
    u = [rng.random(T) for T in LENGTHS]
    alphas = [orc.forward(A, po, pi)[1] for po in pobs]
    steps = [int(t) for t in rng.choice(np.arange(LENGTHS[0] // 8, LENGTHS[0] - 3), size=6, replace=False)]
    u[0], planted = _plant(alphas[0], A, u[0], steps)
    assert planted >= 4
    ref = [orc.sample_path(al, A, u=uu) for al, uu in zip(alphas, u)]
    return model, obs, u, ref, orc.path_counts(ref, n)


def _engine(n, kind, obs):
    from bhmm_amd.engine import Engine
    eng = Engine(0)
    eng.set_option("sample_seg_per_simd", 1)
    eng.set_observations(kind, obs, n, nsymbols=M if kind == "discrete" else 0)
    return eng


def _is_ref(got, ref, counts):
    paths, C, n0, _ = got
    return (sum(int((p != r).sum()) for p, r in zip(paths, ref)) == 0 and np.array_equal(C, counts[0]) and
            np.array_equal(n0, counts[1]))


@pytest.mark.parametrize("n,kind", CASES)
def test_a_draw_that_finds_no_state_goes_through_the_rounds_to_the_serial_kernel(n, kind):
    """A uniform of 1.5 in the middle of the long trajectory: the segment kernels clamp the state and raise the
    status word, the rounds do not accept, the serial kernel decides the call -- BHMM_ERR_CHOICE -- on rows of the
    serial recursion, and no draw of the abandoned rounds is looked at.  The context is sound afterwards: the
    same engine returns the oracle's paths for the valid uniforms, over time segments."""
    model, obs, u, ref, counts = _case(n, kind)
    bad = [uu.copy() for uu in u]
    bad[0][LENGTHS[0] // 2] = 1.5
    eng = _engine(n, kind, obs)
    with pytest.raises(_lib.BhmmAmdError, match="found no state") as err:
        eng.sample_paths(*model, u=bad)
    assert err.value.code == _lib.ERR_CHOICE
    assert eng.get_option("sample_segmented") == 0
    assert eng.get_option("sample_forward_segmented") == 0
    assert eng.get_option("draw_events") == 0
    assert _is_ref(eng.sample_paths(*model, u=u), ref, counts)
    assert eng.get_option("sample_segmented") == 1
    eng.close()


@pytest.mark.parametrize("n,kind", CASES)
def test_rounds_and_the_forced_repeat_leave_the_first_trip_s_counters(n, kind):
    """The draw over time segments with its fix-up rounds, then the forced repeat on exact rows (draw_test_redo
    with a wide watch): the oracle's paths and counts both times; after a repeat the rows are the serial
    recursion's, draw_redone is set and draw_events / draw_checked are those of the first trip (the repeat has no
    watch: its own would be 0).  (On this model the first round leaves no segment to the fix-up -- sample_mismatch
    and sample_rounds, printed below, are 0 at all three cases -- so a fix-up round is not asserted here;
    tests/test_seg_draw_rounds_gpu.py asserts them, on slowly mixing models.)"""
    model, obs, u, ref, counts = _case(n, kind)
    eng = _engine(n, kind, obs)
    assert _is_ref(eng.sample_paths(*model, u=u), ref, counts)
    assert eng.get_option("sample_segmented") == 1
    fwd_seg = eng.get_option("sample_forward_segmented")
    print("n=%d %s: sample_forward_segmented %d sample_mismatch %d sample_rounds %d sample_W %d segments %d" % (
        n, kind, fwd_seg, eng.get_option("sample_mismatch"), eng.get_option("sample_rounds"),
        eng.get_option("sample_W"), eng.get_option("sample_segments")))
    eng.set_option("draw_watch_tol", 1e-9)
    eng.set_option("draw_test_redo", 1)
    assert _is_ref(eng.sample_paths(*model, u=u), ref, counts)
    print("   forced repeat: draw_redone %d draw_events %d draw_checked %d" % (
        eng.get_option("draw_redone"), eng.get_option("draw_events"), eng.get_option("draw_checked")))
    if fwd_seg == 1:
        assert eng.get_option("draw_redone") == 1
        assert eng.get_option("draw_events") > 0 and eng.get_option("draw_checked") > 0
    assert eng.get_option("sample_forward_segmented") == 0 and eng.get_option("draw_alpha_dev") == 0
    eng.close()
