"""CPU: the inputs of test_score_range_gpu.py do reach the weak point they are made for.  The two lazy scaling
schedules of bhmm_score (k_score_wide<.., LAZY>: measured and applied on steps r % 4 == 3; k_score_tile: measured
on r % 4 == 2, applied on r % 4 == 3) are restated in numpy doubles WITHOUT a look at the exit sum, run on those
inputs and compared with the exact 80-bit recursion (tests/score_range_cases.py).  For every state count and
emission kind the case list must hold, per tail length, a trajectory whose exit sum ends in the denormal range
unnoticed and whose log-likelihood is wrong there, one that ends below 2^-900 but normal, and one that flushes to
zero: without them the GPU test would pass whatever the kernels did.

Tail length 1 on the lane-group kernel is the one exception, by construction of that kernel: a row that is itself
below 2^-959 is taken times 2^900 (the rescue rule of wide_emit), so no single step can carry a refreshed vector
into the denormal range.  There the restatement has to agree with the reference instead."""
import numpy as np
import pytest

from tests import score_range_cases as sc

DENORM_MIN, NORMAL_MIN = np.ldexp(1.0, -1074), np.ldexp(1.0, -1022)


def _bands(route, kind, n, M):
    c = sc.build(route, kind, n, M)
    ll, S, trouble = sc.restated(route, kind, n, M)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(ll / c.ref - 1)
    quiet = ~trouble
    denorm = quiet & (S >= DENORM_MIN) & (S < NORMAL_MIN)
    low = quiet & (S >= NORMAL_MIN) & (S < sc.RANGE_MIN)
    flushed = S == 0.0
    return c, err, quiet, denorm, low, flushed, S


@pytest.mark.parametrize("route,n,kind,M", [("wide",) + x for x in sc.WIDE_CASES] + [("tile",) + x for x in sc.TILE_CASES])
def test_inputs_reach_the_window(route, n, kind, M):
    c, err, quiet, denorm, low, flushed, S = _bands(route, kind, n, M)
    assert len(c.obs) == len(c.ctrl) == len(c.cases)
    assert sum(len(o) for o in c.obs) + sum(len(o) for o in c.ctrl) < 8000
    assert set(c.T) >= set(range(c.kmax, 12)) | {37, 64, 129, 262}
    for k in range(1, c.kmax + 1):
        tk = c.k == k
        assert set(c.e[tk]) == set(sc.TARGETS)
        wrong = denorm & tk & (err > 1e-9)
        print(route, kind, n, M, "tail", k, "denormal and unnoticed", int((denorm & tk).sum()), "of them wrong",
              int(wrong.sum()), "worst", float(np.max(err[wrong])) if wrong.any() else 0.0, "| low",
              int((low & tk).sum()), "| flushed", int((flushed & tk).sum()))
        if route == "wide" and k == 1:
            # the rescue rule: every finite answer of the restatement is right
            fin = tk & quiet & np.isfinite(c.ref) & (S >= sc.RANGE_MIN)
            assert fin.sum() >= 20 and np.all(err[fin] < 1e-11)
            assert not denorm[tk].any()
        else:
            assert wrong.any()
            assert (low & tk).any()
            assert (flushed & tk).any()
    assert low.any() and flushed.any()


@pytest.mark.parametrize("n,kind,M", sc.WIDE_CASES)
def test_guard_fires_where_the_counters_are_asserted(n, kind, M):
    """What the GPU test asserts of score_fallbacks follows from the inputs: with the exit sum held to 2^-900, no
    trajectory of the targets -700 and -890 is out of range, none of the control copies is, and every target
    below -900 has one that is."""
    c, err, quiet, denorm, low, flushed, S = _bands("wide", kind, n, M)
    flagged = ~quiet | ~(S >= sc.RANGE_MIN) | ~np.isfinite(S)
    for e in sc.TARGETS:
        te = c.e == e
        if e in sc.IN_RANGE:
            assert not flagged[te].any()
            assert np.all(err[te] < 1e-11)
        else:
            assert flagged[te].any()
    for o in c.ctrl:
        ll, Sc, tr, _ = sc.lazy_run("wide", c.tuned[0], c.tuned[1], sc.rows_double(kind, c.tuned, o))
        assert not tr and Sc >= sc.RANGE_MIN


def test_reference_is_the_oracle_on_benign_data():
    """The 80-bit reference against the oracle's forward pass where both are exact: the control copies."""
    from oracle import oracle as orc
    c = sc.build("wide", "gaussian", 17, 0)
    A, pi, mu, sig = c.tuned
    ref = np.array([orc.forward(A, orc.pobs_gaussian(o, mu, sig), pi)[0] for o in c.ctrl])
    np.testing.assert_allclose(c.ref_ctrl, ref, rtol=1e-12)
    d = sc.build("tile", "discrete", 65, 64)
    ref = np.array([orc.forward(d.tuned[0], orc.pobs_discrete(o, d.tuned[2]), d.tuned[1])[0] for o in d.ctrl])
    np.testing.assert_allclose(d.ref_ctrl, ref, rtol=1e-12)
