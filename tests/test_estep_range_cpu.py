"""CPU: the inputs of test_estep_range_gpu.py do reach the weak point they are made for, and its bounds can be met.
The forward schedules of the lazily scaled E-step (k_wide_fwd<.., LAZY>: measured and taken off on steps
r % 4 == 3, no rescue of denormal rows; k_tile_fwd: measured on r % 4 == 2, taken off on r % 4 == 3) are restated
in numpy (tests/estep_range_cases.py) WITHOUT a look at the exit sum, run over the trajectories of
tests/score_range_cases.py and held to the 80-bit E-step under the BOUNDS of tests/test_tile_matrix_gpu.py:

  * per case and tail length there are trajectories that no refresh notices and that end below 2^-900; among them
    the double-precision restatement has a log-likelihood outside its bound and, for discrete emissions, a last
    gamma row outside its bound (gaussian: that row is one-hot on the widest state in any arithmetic) -- without
    them the GPU test would pass whatever the kernels did;
  * the same restatement in long double is inside every bound: the defect is the number range, not the schedule;
  * a float64 E-step that normalises every step and applies the 2^900 rule stays below a tenth of every bound, so a
    correct double-precision kernel can meet them;
  * what is left out is what the module text says, and no more than 6 % of a case's list."""
import numpy as np
import pytest

from tests import estep_range_cases as ec
from tests import score_range_cases as sc
from tests.test_tile_matrix_gpu import BOUNDS, _compare, _frac

L = np.longdouble
CASES = [("wide",) + x for x in ec.WIDE_CASES] + [("tile",) + x for x in ec.TILE_CASES]
IDS = ["%s-%d-%s%d" % x for x in CASES]


@pytest.mark.parametrize("route,n,kind,M", CASES, ids=IDS)
def test_unnoticed_batches_catch_the_defect(route, n, kind, M):
    r = ec.reference(route, kind, n, M)
    c = r.c
    assert not r.trouble[r.unnoticed].any() and np.all(r.S[r.unnoticed] < sc.RANGE_MIN)
    ref_ll = np.array([np.nan if x is None else x[0] for x in r.ref])
    np.testing.assert_allclose(ref_ll[r.kept], c.ref[r.kept], rtol=1e-15)       # (the two 80-bit recursions agree)
    for k in range(1, ec.kmax_of(route) + 1):
        b = ec.batch(route, kind, n, M, "unnoticed %d" % k)
        assert len(b.index) >= 1, "tail %d: no trajectory ends unnoticed below 2^-900" % k
        fl = [_frac(r.ll[i], r.ref[i][0], *BOUNDS["logL"]) for i in b.index]
        with np.errstate(under="ignore", invalid="ignore"):
            fg = [_frac(r.last[i] / r.last[i].sum(), r.ref[i][1][-1], *BOUNDS["gamma"]) for i in b.index]
        print(route, kind, n, M, "tail", k, "unnoticed", len(b.index), "logL outside", int(np.sum(np.array(fl) > 1)),
              "worst %.3g" % max(fl), "| last gamma row outside", int(np.sum(np.array(fg) > 1)), "worst %.3g" % max(fg))
        assert max(fl) > 1.0
        if kind == "discrete":
            assert max(fg) > 1.0
    # the same schedule without a number range
    worst = [0.0, 0.0]
    for i in np.flatnonzero(r.kept):
        ll, S, _, a = ec.estep_run(route, c.tuned[0], c.tuned[1], sc.rows_exact(kind, c.tuned, c.obs[i]))
        worst[0] = max(worst[0], _frac(ll, r.ref[i][0], *BOUNDS["logL"]))
        worst[1] = max(worst[1], _frac((a / S).astype(np.float64), r.ref[i][1][-1], *BOUNDS["gamma"]))
    print(route, kind, n, M, "in long double: logL %.3g, last gamma row %.3g of bound" % tuple(worst))
    assert max(worst) <= 1.0


@pytest.mark.parametrize("route,n,kind,M", CASES, ids=IDS)
def test_batches_are_what_the_gpu_test_takes_them_for(route, n, kind, M):
    r = ec.reference(route, kind, n, M)
    c = r.c
    # left out: only trajectories of probability zero, only discrete one-step tails on a column that is zero
    out = ~r.kept
    assert out.sum() <= ec.LEFT_OUT_CAP * len(c.obs)
    for i in np.flatnonzero(out):
        assert kind == "discrete" and c.k[i] == 1 and np.all(c.tuned[2][:, c.obs[i][-1]] == 0.0)
    print(route, kind, n, M, "left out", int(out.sum()), "of", len(c.obs))
    # every kept trajectory is in exactly one batch
    assert np.array_equal(r.unnoticed.astype(int) + r.other + r.in_range, r.kept.astype(int))
    seen = np.concatenate([ec.batch(route, kind, n, M, name).index for name in ec.batch_names(route)])
    assert sorted(seen) == list(np.flatnonzero(r.kept))
    # in range: the restated schedule finds nothing and ends inside the range, control copies included
    assert not r.trouble[r.in_range].any() and np.all(r.S[r.in_range] >= sc.RANGE_MIN)
    for o in c.ctrl + [r.benign]:
        _, S, tr, _ = ec.estep_run(route, c.tuned[0], c.tuned[1], sc.rows_double(kind, c.tuned, o))
        assert not tr and S >= sc.RANGE_MIN
    # (the matrix-core schedule looks at a measurement only on the step after it: few tails of up to four steps
    # are caught by a refresh at all)
    print(route, kind, n, M, "other:", int(r.other.sum()), "of them flagged by a refresh", int(r.trouble[r.other].sum()),
          "flushed to zero", int((r.S[r.other] == 0).sum()))
    assert route == "tile" or r.trouble[r.other].any()
    # sizes, and the argument for counting steps from the trajectory's start
    for name in ec.batch_names(route):
        b = ec.batch(route, kind, n, M, name)
        assert max(b.lengths[:-1], default=0) <= 262 and b.lengths[-1] == ec.BENIGN_T and len(b.lengths) <= 250
        assert ec.assert_warmups_on_four(b.lengths) > len(b.lengths)
        assert all(np.all(np.isfinite(v)) for v in b.want.values())
        np.testing.assert_allclose(b.want["gamma"].sum(axis=1), 1.0, rtol=0, atol=1e-14)
        np.testing.assert_allclose(b.want["counts"].sum(), sum(b.lengths), rtol=1e-13)


@pytest.mark.parametrize("route,n,kind,M", CASES, ids=IDS)
def test_a_double_precision_estep_can_meet_the_bounds(route, n, kind, M):
    for name in ec.batch_names(route):
        b = ec.batch(route, kind, n, M, name)
        A, pi, p0, _ = b.model
        res = [ec.careful_estep(A, pi, rows) for rows in b.rows]
        got = dict(logL=np.array([x[0] for x in res]), gamma=np.concatenate([x[1] for x in res]),
                   C=sum(x[2] for x in res), gamma0=sum(x[1][0] for x in res), counts=sum(x[1].sum(axis=0) for x in res))
        if kind == "gaussian":
            got["sum_gd"] = sum((x[1] * (o[:, None] - p0[None, :])).sum(axis=0) for o, x in zip(b.obs, res))
            got["sum_gdd"] = sum((x[1] * (o[:, None] - p0[None, :]) ** 2).sum(axis=0) for o, x in zip(b.obs, res))
        else:
            sym = np.zeros((M, n))
            for o, x in zip(b.obs, res):
                np.add.at(sym, o, x[1])
            got["symbols"] = sym.T
        _compare(got, b.want, "%s n=%d %s M=%d %s, float64 numpy" % (route, n, kind, M, name), scale=0.1)


@pytest.mark.parametrize("route,n,kind,M", CASES, ids=IDS)
def test_single_step_batch_is_unnoticed_and_wrong_in_doubles(route, n, kind, M):
    """One-step trajectories at 2^-1000 .. 2^-1060: no refresh, a positive exit sum below 2^-900 each, pi o p wrong in
    doubles at the low end (logL, and the one gamma row where the emissions are discrete), right in long double, and
    within a tenth of the bounds for the float64 E-step with the 2^900 rule."""
    b = ec.single_step_batch(route, kind, n, M)
    A, pi = b.model[0], b.model[1]
    fl, fg = [], []
    for rows, ref, o in zip(b.rows[:-1], b.ref[:-1], b.obs[:-1]):
        ll, S, tr, a = ec.estep_run(route, A, pi, rows)
        assert not tr and 0 < S < sc.RANGE_MIN
        with np.errstate(under="ignore"):
            fl.append(_frac(ll, ref[0], *BOUNDS["logL"]))
            fg.append(_frac(a / S, ref[1][-1], *BOUNDS["gamma"]))
        ll, S, _, a = ec.estep_run(route, A, pi, sc.rows_exact(kind, b.model, o))
        assert _frac(ll, ref[0], *BOUNDS["logL"]) <= 1 and _frac((a / S).astype(np.float64), ref[1][-1], *BOUNDS["gamma"]) <= 1
        got = ec.careful_estep(A, pi, rows)
        assert _frac(got[0], ref[0], *BOUNDS["logL"]) <= 0.1 and _frac(got[1], ref[1], *BOUNDS["gamma"]) <= 0.1
    print(route, kind, n, M, "single step: logL", " ".join("%.3g" % x for x in fl), "| gamma row",
          " ".join("%.3g" % x for x in fg), "of bound")
    assert max(fl) > 1.0
    if kind == "discrete":
        assert max(fg) > 1.0
    assert ec.assert_warmups_on_four(b.lengths) > len(b.lengths)


def test_the_tile_schedule_is_the_one_of_the_scoring_kernel():
    """k_tile_fwd and k_score_tile share their schedule (no rescue rule in either): the restatement made from
    k_tile_fwd gives what sc.lazy_run("tile") gives, bit for bit; the lane-group one differs from sc.lazy_run("wide")
    exactly where a row lies in the denormal range."""
    c = sc.build("tile", "discrete", 65, 64)
    for o in c.obs:
        rows = sc.rows_double("discrete", c.tuned, o)
        x, y = ec.tile_estep(c.tuned[0], c.tuned[1], rows), sc.lazy_run("tile", c.tuned[0], c.tuned[1], rows)
        assert x[0] == y[0] and x[1] == y[1] and x[2] == y[2] and np.array_equal(x[3], y[3])
    c = sc.build("wide", "discrete", 17, 32)
    differ = 0
    for o in c.obs:
        rows = sc.rows_double("discrete", c.tuned, o)
        x, y = ec.wide_estep(c.tuned[0], c.tuned[1], rows), sc.lazy_run("wide", c.tuned[0], c.tuned[1], rows)
        low = bool(np.any(np.all(rows < sc.RESCUE_MIN, axis=1) & np.any(rows != 0, axis=1)))
        assert low or (x[0] == y[0] and x[1] == y[1] and np.array_equal(x[3], y[3]))
        differ += x[1] != y[1]
    assert differ > 0


def test_explicit_batches_are_the_discrete_rows():
    b, d = ec.batch("wide", "explicit", 16, 32, "unnoticed 2"), ec.batch("wide", "discrete", 16, 32, "unnoticed 2")
    assert b.model[2] is None and "symbols" not in b.want and np.array_equal(b.want["gamma"], d.want["gamma"])
    assert all(o.shape == (T, 16) and o.dtype == np.float64 for o, T in zip(b.obs, b.lengths))
    assert all(np.array_equal(o, d.model[2][:, s].T) for o, s in zip(b.obs, d.obs))


def test_compare_fails_on_a_moved_entry_and_on_a_nan():
    b = ec.batch("wide", "discrete", 9, 32, "unnoticed 1")
    same = {k: np.array(v, dtype=np.float64) for k, v in b.want.items()}
    _compare(same, b.want, "unchanged")
    for key, (rtol, atol) in BOUNDS.items():
        if key not in b.want:
            continue
        at = np.unravel_index(np.argmax(np.abs(b.want[key])), np.shape(b.want[key]))
        moved = {k: v.copy() for k, v in same.items()}
        moved[key][at] += 2.0 * (atol + rtol * abs(b.want[key][at]))
        with pytest.raises(AssertionError):
            _compare(moved, b.want, key + " moved by twice its bound")
        moved[key][at] = np.nan
        with pytest.raises(AssertionError):
            _compare(moved, b.want, key + " with a NaN")
