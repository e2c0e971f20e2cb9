"""GPU: the time-segmented path of bhmm_posterior_decode / bhmm_posterior_marginals for 9 to 64 states (k_filter_wide
forward, k_smooth_wide_bwd backward; post_path / marg_path 2) against the CPU oracle's gamma, under the rules of
tests/test_posterior_gpu.py and tests/test_marginals_gpu.py (imported, not restated): the path exact wherever the
oracle's gap between its two largest gamma exceeds 1e-9, at most 1e-4 of a case's steps left out, the confidence
within 1e-7 on all steps, rows at that module's fp64 (rtol 1e-8, atol 1e-13) and fp32 (1e-7) bounds, projections
those bounds carried through the sum.  Every engine sets smooth_wide = 1 unless the test is about the choice.

The data of every case that compares a path come from the _*_case functions below, so that the share of steps the
rule leaves out can be counted with the oracle alone, without a GPU."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_filter_gpu import ATOL64 as F_ATOL64, RTOL64 as F_RTOL64
from tests.test_marginals_gpu import ATOL64, RTOL64, _check as _check_rows, _weights
from tests.test_posterior_gpu import (CONF_TOL, GAP, LENGTHS, MAX_LEFT_OUT, _check, _oracle_gammas, _rand_model,
                                      _rand_obs)

pytestmark = pytest.mark.gpu

KINDS = [("gaussian", 0), ("discrete", 64), ("discrete", 1000)]   # M = 1000: B^T beyond LDS at 32 and 64 lanes


def _engine():
    from bhmm_amd.engine import Engine
    return Engine(0)


def _smooth_engine(kind, obs, n, M, seglen=0, wide=1):
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    eng.set_option("smooth_wide", wide)
    eng.set_option("smooth_seglen", seglen)
    return eng


def _cat(xs):
    return np.concatenate([np.asarray(x) for x in xs])


def _clear(g):
    """steps of one trajectory where the oracle's two largest gamma are more than GAP apart"""
    if g.shape[1] < 2 or g.shape[0] == 0:
        return np.ones(g.shape[0], dtype=bool)
    top = np.sort(g, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) > GAP


def _paths_equal_off_gap(gammas, pa, pb):
    for g, a, b in zip(gammas, pa, pb):
        c = _clear(g)
        assert np.array_equal(np.asarray(a)[c], np.asarray(b)[c])


def _rows_within(a, b, factor, ref=None):
    """|a - b| within factor times the fp64 row bound of tests/test_marginals_gpu.py"""
    ref = b if ref is None else ref
    assert np.all(np.abs(a - b) <= factor * (ATOL64 + RTOL64 * np.abs(ref)))


# ---- the data of the cases (seeds checked on the CPU against MAX_LEFT_OUT) --------------------------
def _parity_case(n, kind, M, stay):
    rng = np.random.default_rng(3000 * n + M + stay)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    return obs, _rand_model(kind, n, M, rng, stay=float(stay)), rng


def _forced_case(kind, M, stay):
    rng = np.random.default_rng(31 + stay)
    n = 24
    obs = _rand_obs(kind, n, M, [30000, 20000, 12345], rng)
    return n, obs, _rand_model(kind, n, M, rng, stay=float(stay)), rng


def _invariance_case(n, kind, M):
    rng = np.random.default_rng(5 + n)
    obs = _rand_obs(kind, n, M, [20000, 7000, 1, 12345, 64, 3001], rng)
    return obs, _rand_model(kind, n, M, rng, stay=3.0), rng


def _consistency_case(n, kind, M):
    rng = np.random.default_rng(300 + n + M)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    return obs, _rand_model(kind, n, M, rng, stay=2.0), rng


EDGE_LENGTHS = [1024, 256, 257, 255, 512, 4, 2048]


def _near_ends_case(kind, M):
    rng = np.random.default_rng(8)
    n = 17
    obs = _rand_obs(kind, n, M, EDGE_LENGTHS, rng)
    return n, obs, _rand_model(kind, n, M, rng, stay=2.0), rng


def _outlier_case(n):
    """the construction of tests/test_filter_wide_gpu.py (means within 0.08: one observation, one range), without
    the NaN; seglen 256 cuts the 3000 steps into 12 segments that start at 250 q rounded down to 4"""
    rng = np.random.default_rng(17)
    A, pi, _, _ = _rand_model("gaussian", n, 0, rng, stay=2.0)
    mu, sig = 0.02 * np.arange(n) / (n / 4.0), np.ones(n)
    obs = [rng.normal(0, 1, T) for T in (3000, 500, 1)]
    obs[0][100] = 1e6          # every density underflows to zero: a row of ones; inside a segment
    obs[0][1999] = -1e6        # ... the last step of a segment (inside the backward warm-up of none, the forward of the next)
    obs[0][2248] = 1e6         # ... the first step of a segment
    obs[0][2260] = -1e6        # ... inside the backward warm-up of the segment before
    obs[1][0] = 1e6            # ... the first step of a trajectory
    obs[1][499] = -1e6         # ... the last step of a trajectory: b starts from ones over it
    obs[0][1200] = 37.9        # densities of about 1e-312: a denormal row
    obs[0][1201] = 37.9
    obs[0][1000] = 37.9        # ... as the first step of a segment, in the backward warm-up of the one before
    obs[0][999] = -37.9        # ... as the last step of a segment, in the forward warm-up of the next
    obs[1][300] = -37.9
    gammas = []
    for o in obs:
        pobs = orc.pobs_gaussian(o, mu, sig)
        bad = ~np.all(np.isfinite(pobs), axis=1) | np.all(pobs == 0.0, axis=1)
        pobs[bad] = 1.0
        # gamma does not see a factor on an emission row.  The denormal rows go to the oracle times 2^900 (exact, the
        # same values): its backward recursion multiplies them by beta ~ 1 / n and rounds those products in the
        # denormal range, to 28 bits at 40 states -- on the rows as they are, the oracle's own gamma is 1.01 of the
        # fp64 bound away from the one computed this way (step 299 of trajectory 1; 0.22 of it at 12 states)
        den = pobs.max(axis=1) < 2.0 ** -959
        pobs[den] = np.ldexp(pobs[den], 900)
        gammas.append(orc.gamma(orc.forward(A, pobs, pi)[1], orc.backward(A, pobs)))
    den = orc.pobs_gaussian(obs[0][1200:1201], mu, sig)
    assert 0.0 < den.max() < 2.3e-308       # (the row IS denormal)
    return obs, (A, pi, mu, sig), gammas, rng


def _full_case():
    rng = np.random.default_rng(64)
    n, K, T = 64, 128, 100000
    model = _rand_model("gaussian", n, 0, rng)
    flat = rng.normal(0, 3, K * T)
    return n, K, T, model, [flat[k * T:(k + 1) * T] for k in range(K)]


def _all_forms(eng, model, n, rng, results, label):
    """decode with confidence, rows in both dtypes, projections on 1, 3 and 8 columns in both dtypes"""
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("post_path") == 2
    results.append(("decode", paths, conf, None, None, label))
    for dtype in (np.float64, np.float32):
        rows = eng.posterior_marginals(*model, dtype=dtype)
        assert eng.get_option("marg_path") == 2
        results.append(("rows", rows, None, dtype, None, "%s %s" % (label, np.dtype(dtype).name)))
        for Q in (1, 3, 8):
            V = _weights(n, Q, model, rng)
            rows = eng.posterior_marginals(*model, weights=V, dtype=dtype)
            assert eng.get_option("marg_path") == 2
            results.append(("rows", rows, None, dtype, V, "%s %s Q=%d" % (label, np.dtype(dtype).name, Q)))


def _check_all(gammas, results):
    for what, out, conf, dtype, V, label in results:
        if what == "decode":
            _check(gammas, out, conf, label)
        else:
            _check_rows(gammas, out, dtype, V, label)


# ---- 1. oracle parity -----------------------------------------------------------------------------
@pytest.mark.parametrize("stay", [0, 20])
@pytest.mark.parametrize("kind,M", KINDS)
@pytest.mark.parametrize("n", [9, 16, 17, 32, 33, 64])         # both edges of every lane-group class
def test_parity(n, kind, M, stay):
    obs, model, rng = _parity_case(n, kind, M, stay)
    gammas = _oracle_gammas(kind, obs, model)
    eng = _smooth_engine(kind, obs, n, M)
    results = []
    for seglen in (0, 256, 1000):
        eng.set_option("smooth_seglen", seglen)
        assert eng.get_option("smooth_seglen") == seglen
        before = eng.get_option("post_fallbacks"), eng.get_option("marg_fallbacks")
        _all_forms(eng, model, n, rng, results, "n=%d %s M=%d seglen=%d stay=%d" % (n, kind, M, seglen, stay))
        assert eng.get_option("smooth_segments") >= len(LENGTHS)
        if stay == 0:
            assert (eng.get_option("post_fallbacks"), eng.get_option("marg_fallbacks")) == before
    eng.close()
    _check_all(gammas, results)


# ---- 2. which path a call takes ---------------------------------------------------------------------
# The automatic rule (smooth_wide = -1, at least smooth_wide_min_total steps), per lanes per segment and call form
# (decode, decode with confidences, rows, projection): smooth_wide_auto of csrc/smooth_wide_launch.hpp, derived from
# profiles/smooth/smooth_wide_time.json (tools/smooth_wide_time.py).
AUTO = {16: (False, False, False, False), 32: (False, False, False, False), 64: (False, False, False, False)}


def _paths_of_the_four_forms(eng, model, n, rng):
    """(post_path of decode, of decode with confidences, marg_path of rows, of a projection)"""
    got = []
    eng.posterior_decode(*model)
    got.append(eng.get_option("post_path"))
    eng.posterior_decode(*model, confidence=True)
    got.append(eng.get_option("post_path"))
    eng.posterior_marginals(*model, dtype=np.float32)
    got.append(eng.get_option("marg_path"))
    eng.posterior_marginals(*model, weights=_weights(n, 2, model, rng))
    got.append(eng.get_option("marg_path"))
    return tuple(int(x) for x in got)


@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_path_selection(kind, M):
    rng = np.random.default_rng(77 + M)
    n = 24
    eng = _engine()
    min_total = int(eng.get_option("smooth_wide_min_total"))
    assert min_total >= 32768 and min_total & (min_total - 1) == 0
    assert eng.get_option("smooth_wide") == -1
    model = _rand_model(kind, n, M, rng, stay=1.0)
    # a default engine on a small set stays on the generic path
    small = _rand_obs(kind, n, M, LENGTHS, rng)
    eng.set_observations(kind, small, n, nsymbols=M)
    assert _paths_of_the_four_forms(eng, model, n, rng) == (0, 0, 0, 0)
    assert eng.get_option("smooth_segments") == 0
    # the automatic rule on exactly min_total + 301 steps, in every lane-group class
    big = [min_total - 5000, 5000, 1, 300]
    for nn in (12, 24, 64):
        m = _rand_model(kind, nn, M, rng, stay=1.0)
        eng.set_observations(kind, _rand_obs(kind, nn, M, big, rng), nn, nsymbols=M)
        np_ = 16 if nn <= 16 else (32 if nn <= 32 else 64)
        assert _paths_of_the_four_forms(eng, m, nn, rng) == tuple(2 if a else 0 for a in AUTO[np_]), nn
    # smooth_wide = 0 stays on the generic path on any set, 1 takes the new one
    eng.set_observations(kind, _rand_obs(kind, n, M, big, rng), n, nsymbols=M)
    eng.set_option("smooth_wide", 0)
    assert _paths_of_the_four_forms(eng, model, n, rng) == (0, 0, 0, 0)
    eng.set_option("smooth_wide", 1)
    assert _paths_of_the_four_forms(eng, model, n, rng) == (2, 2, 2, 2)
    assert eng.get_option("smooth_segments") > len(big)
    with pytest.raises(ValueError):
        eng.set_option("smooth_wide", 2)
    for read_only in ("smooth_segments", "smooth_wide_min_total"):
        with pytest.raises(ValueError):
            eng.set_option(read_only, 1)
    eng.close()
    # 65 states and explicit pobs are not eligible
    eng = _engine()
    eng.set_option("smooth_wide", 1)
    m65 = _rand_model("gaussian", 65, 0, rng)
    eng.set_observations("gaussian", [rng.normal(0, 3, 500)], 65)
    eng.posterior_decode(*m65)
    eng.posterior_marginals(*m65)
    assert eng.get_option("post_path") == 0 and eng.get_option("marg_path") == 0
    A, pi, mu, sig = _rand_model("gaussian", 12, 0, rng)
    eng.set_observations("explicit", [orc.pobs_gaussian(rng.normal(0, 3, 500), mu, sig)], 12)
    eng.posterior_decode(A, pi)
    eng.posterior_marginals(A, pi)
    assert eng.get_option("post_path") == 0 and eng.get_option("marg_path") == 0
    assert eng.get_option("smooth_segments") == 0
    eng.close()


# ---- 3. forced protocol ---------------------------------------------------------------------------
@pytest.mark.parametrize("stay", [5, 200])    # 200: twice the warm-up fails as well, the generic path decides
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_forced_fallback(kind, M, stay):
    n, obs, model, rng = _forced_case(kind, M, stay)
    eng = _smooth_engine(kind, obs, n, M, seglen=512)
    eng.set_option("smooth_W", 8)                              # far too short: the check must fail
    before = eng.get_option("post_fallbacks"), eng.get_option("marg_fallbacks")
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("post_path") == 2                    # (the FIRST pass was the time-segmented one)
    rows = eng.posterior_marginals(*model)
    assert eng.get_option("marg_path") == 2
    assert eng.get_option("post_fallbacks") == before[0] + 1
    assert eng.get_option("marg_fallbacks") == before[1] + 1
    eng.close()
    gammas = _oracle_gammas(kind, obs, model)
    _check(gammas, paths, conf, "forced %s stay=%d" % (kind, stay))
    _check_rows(gammas, rows, np.float64, None, "forced %s stay=%d" % (kind, stay))
    if stay == 200:     # the answer is the generic path's
        ref = _smooth_engine(kind, obs, n, M, wide=0)
        p0, c0 = ref.posterior_decode(*model, confidence=True)
        assert ref.get_option("post_path") == 0
        ref.close()
        assert np.array_equal(_cat(p0), _cat(paths)) and np.array_equal(_cat(c0), _cat(conf))


# ---- 4. invariance ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [12, 40, 64])
def test_invariance(n, kind, M):
    import torch
    from bhmm_amd import _lib
    obs, model, rng = _invariance_case(n, kind, M)
    V = _weights(n, 3, model, rng)
    gammas = _oracle_gammas(kind, obs, model)
    eng = _smooth_engine(kind, obs, n, M)
    total = int(eng.offsets[-1])

    def run():
        p, c = eng.posterior_decode(*model, confidence=True)
        r = eng.posterior_marginals(*model)
        q = eng.posterior_marginals(*model, weights=V)
        assert eng.get_option("post_path") == 2 and eng.get_option("marg_path") == 2
        return [np.array(x) for x in p], _cat(c), _cat(r), _cat(q), eng.get_option("smooth_segments")

    got = {}
    for seglen in (256, 1000, 0):
        eng.set_option("smooth_seglen", seglen)
        got[seglen] = run()
    assert got[256][4] > got[1000][4] > got[0][4]
    p0, c0, r64, q64, _ = got[0]
    for seglen in (256, 1000):
        p, c, r, q, _ = got[seglen]
        _rows_within(r, r64, 2)
        assert np.all(np.abs(q - q64) <= 2 * (np.abs(V).sum(axis=0) * ATOL64 + RTOL64 * (r64 @ np.abs(V))))
        _paths_equal_off_gap(gammas, p, p0)
    # the workspace budget (1 MiB: 2048 rows of 64 states -- many ranges), repeated calls: all bitwise
    for mb in (8192, 1, 0):
        eng.set_option("smooth_ws_mb", mb)
        assert eng.get_option("smooth_ws_mb") == mb
        p, c, r, q, _ = run()
        assert np.array_equal(_cat(p), _cat(p0)) and np.array_equal(c, c0)
        assert np.array_equal(r, r64) and np.array_equal(q, q64)
    eng.set_option("smooth_ws_mb", 1)
    assert np.array_equal(_cat(eng.posterior_decode(*model)), _cat(p0))           # confidence off: the same path
    # fp32 is the rounded fp64 result: the conversion is the last operation
    r32 = _cat(eng.posterior_marginals(*model, dtype=np.float32))
    q32 = _cat(eng.posterior_marginals(*model, weights=V, dtype=np.float32))
    assert r32.dtype == np.float32 and np.array_equal(r32, r64.astype(np.float32))
    assert np.array_equal(q32, q64.astype(np.float32))
    # device output, tensor and raw address: bitwise the host output
    for dtype, tdtype, ref in ((np.float64, torch.float64, r64), (np.float32, torch.float32, r32)):
        t = torch.full((total, n), -1.0, dtype=tdtype, device="cuda:0")
        eng.posterior_marginals(*model, dtype=dtype, out=t)
        eng.sync()
        assert np.array_equal(t.cpu().numpy(), ref)
        t.fill_(-1.0)
        torch.cuda.synchronize()
        assert eng.posterior_marginals(*model, dtype=dtype, out=t.data_ptr()) is None
        eng.sync()
        assert np.array_equal(t.cpu().numpy(), ref)
    tp = torch.full((total, 3), -1.0, dtype=torch.float32, device="cuda:0")
    eng.posterior_marginals(*model, weights=V, dtype=np.float32, out=tp)
    eng.sync()
    assert np.array_equal(tp.cpu().numpy(), q32)
    assert eng.get_option("marg_path") == 2
    # int32 through the C entry
    A, pi, e0, e1 = eng._model_ptrs(*model)
    p32 = np.empty(total, dtype=np.int32)
    c32 = np.empty(total, dtype=np.float32)
    _lib.check(eng._L.bhmm_posterior_decode(eng._h, A, pi, e0, e1, ctypes.c_void_p(p32.ctypes.data), 0,
                                            ctypes.c_void_p(c32.ctypes.data)))
    assert eng.get_option("post_path") == 2
    assert np.array_equal(p32, _cat(p0).astype(np.int32)) and np.array_equal(c32, c0)
    eng.close()


# ---- 5. consistency --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [12, 40, 64])
def test_consistency(n, kind, M):
    obs, model, rng = _consistency_case(n, kind, M)
    gammas = _oracle_gammas(kind, obs, model)
    eng = _smooth_engine(kind, obs, n, M, seglen=512)
    rows = eng.posterior_marginals(*model)
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("marg_path") == 2 and eng.get_option("post_path") == 2
    eng.set_option("filter_parallel", 1)
    filt = eng.filter_states(*model, increments=False)[0]
    eng.set_option("smooth_wide", 0)
    rows0 = eng.posterior_marginals(*model)
    paths0, conf0 = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("marg_path") == 0 and eng.get_option("post_path") == 0
    eng.close()
    compared = 0
    worst = 0.0
    for g, r, p, c, f in zip(gammas, rows, paths, conf, filt):
        clear = _clear(g)
        assert np.array_equal(r.argmax(axis=1)[clear], p.astype(np.int64)[clear])
        compared += int(clear.sum())
        worst = max(worst, float(np.abs(r.max(axis=1) - c.astype(np.float64)).max()))
        np.testing.assert_allclose(r[-1], f[-1], rtol=F_RTOL64, atol=F_ATOL64)      # gamma_{T-1} = alpha^_{T-1}
    print("n=%d %s: %d steps compared, worst |max row - conf| %.3g" % (n, kind, compared, worst))
    assert compared > 0.99 * sum(LENGTHS)
    assert worst <= CONF_TOL
    # path 2 against path 0
    _rows_within(_cat(rows), _cat(rows0), 2)
    _paths_equal_off_gap(gammas, paths, paths0)
    assert np.all(np.abs(_cat(conf).astype(np.float64) - _cat(conf0)) <= 2 * CONF_TOL)


# ---- 6. edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M,n", [("gaussian", 0, 12), ("discrete", 16, 33), ("gaussian", 0, 64)])
def test_single_step(kind, M, n):
    rng = np.random.default_rng(2 + n)
    obs = _rand_obs(kind, n, M, [1], rng)
    model = _rand_model(kind, n, M, rng)
    eng = _smooth_engine(kind, obs, n, M)
    results = []
    _all_forms(eng, model, n, rng, results, "T=1 %s n=%d" % (kind, n))
    assert eng.get_option("smooth_segments") == 1
    eng.close()
    _check_all(_oracle_gammas(kind, obs, model), results)


@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_warm_ups_that_reach_past_both_trajectory_ends(kind, M):
    """lengths that are multiples of the segment length, one step more and one step less; a warm-up longer than
    the distance to either end of the trajectory: those segments start exactly"""
    n, obs, model, rng = _near_ends_case(kind, M)
    gammas = _oracle_gammas(kind, obs, model)
    eng = _smooth_engine(kind, obs, n, M, seglen=256)
    results = []
    for W in (0, 600, 100000):
        eng.set_option("smooth_W", W)
        assert eng.get_option("smooth_W") == W
        _all_forms(eng, model, n, rng, results, "near ends %s W=%d" % (kind, W))
    assert eng.get_option("post_fallbacks") == 0 and eng.get_option("marg_fallbacks") == 0
    eng.close()
    _check_all(gammas, results)


@pytest.mark.parametrize("n", [12, 40])
def test_gaussian_outliers_and_denormal_rows(n):
    obs, model, gammas, rng = _outlier_case(n)
    eng = _smooth_engine("gaussian", obs, n, 0, seglen=256)
    results = []
    _all_forms(eng, model, n, rng, results, "outliers n=%d" % n)
    assert eng.get_option("smooth_segments") == 12 + 2 + 1
    assert eng.get_option("post_fallbacks") == 0 and eng.get_option("marg_fallbacks") == 0
    eng.close()
    _check_all(gammas, results)


def _outcome(call):
    try:
        return ("ok", call())
    except Exception as e:      # noqa: BLE001 (the two routes must raise the same thing)
        return ("error", type(e).__name__, str(e))


def _same_outcome(a, b):
    assert a[0] == b[0], (a[0], b[0], a[1:] if a[0] == "error" else "", b[1:] if b[0] == "error" else "")
    if a[0] == "error":
        assert a[1:] == b[1:]
        return
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y, equal_nan=True)


def _both_calls(kind, obs, n, M, model, wide):
    """the outcomes of the two calls on a fresh engine, and what the fallback counters and the path say"""
    eng = _smooth_engine(kind, obs, n, M, seglen=256, wide=wide)
    dec = _outcome(lambda: [_cat(x) for x in eng.posterior_decode(*model, confidence=True)])
    path = eng.get_option("post_path")
    mar = _outcome(lambda: [_cat(eng.posterior_marginals(*model))])
    counters = (eng.get_option("post_fallbacks"), eng.get_option("marg_fallbacks"))
    path = (path, eng.get_option("marg_path"))
    eng.close()
    return dec, mar, counters, path


@pytest.mark.parametrize("n", [12, 40])
def test_nan_observation_takes_the_generic_route(n):
    rng = np.random.default_rng(23 + n)
    obs = [rng.normal(0, 3, T) for T in (3000, 500, 1)]
    obs[0][700] = np.nan
    model = _rand_model("gaussian", n, 0, rng, stay=1.0)
    d1, m1, c1, path1 = _both_calls("gaussian", obs, n, 0, model, 1)
    d0, m0, c0, path0 = _both_calls("gaussian", obs, n, 0, model, 0)
    assert path1 == (2, 2) and path0 == (0, 0)
    _same_outcome(d1, d0)
    _same_outcome(m1, m0)
    assert c1 == (0, 0)


@pytest.mark.parametrize("z", [150, 2500])
@pytest.mark.parametrize("n,M", [(12, 5), (40, 1000)])
def test_symbol_no_state_emits_takes_the_generic_route(n, M, z):
    """the known-step construction of tests/test_filter_wide_gpu.py"""
    rng = np.random.default_rng(4 + n)
    obs = [rng.integers(0, M - 1, T).astype(np.int32) for T in (5000, 3000, 4000)]
    obs[1][z] = M - 1                     # the last symbol appears in trajectory 1 only, at step z
    A, pi, B, _ = _rand_model("discrete", n, M, rng, stay=1.0)
    A[0, n - 1] = A[n - 1, 0] = 0.0       # (structural zeros in A as well)
    A /= A.sum(axis=1)[:, None]
    B[:, M - 1] = 0.0                     # no state emits the last symbol
    B[::2, 0] = 0.0
    B /= B.sum(axis=1)[:, None]
    model = (A, pi, B, None)
    d1, m1, c1, path1 = _both_calls("discrete", obs, n, M, model, 1)
    d0, m0, c0, path0 = _both_calls("discrete", obs, n, M, model, 0)
    assert path1 == (2, 2) and path0 == (0, 0)
    _same_outcome(d1, d0)
    _same_outcome(m1, m0)
    assert c1 == (0, 0)


@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_lagged(kind, M):
    rng = np.random.default_rng(13)
    n, lag = 20, 3
    obs = _rand_obs(kind, n, M, [9000, 1000, 37, 5], rng)
    model = _rand_model(kind, n, M, rng, stay=2.0)
    views = [(k, s) for k in range(len(obs)) for s in range(lag) if len(obs[k]) > s]
    cut = [np.ascontiguousarray(obs[k][s::lag]) for k, s in views]
    eng = _engine()
    eng.set_option("smooth_wide", 1)
    eng.set_option("smooth_seglen", 256)
    eng.set_observations_lagged(kind, obs, lag, views, n, nsymbols=M)
    lp, lc = eng.posterior_decode(*model, confidence=True)
    lr = eng.posterior_marginals(*model)
    assert eng.get_option("post_path") == 2 and eng.get_option("marg_path") == 2
    eng.set_observations(kind, cut, n, nsymbols=M)
    pp, pc = eng.posterior_decode(*model, confidence=True)
    pr = eng.posterior_marginals(*model)
    assert eng.get_option("post_path") == 2 and eng.get_option("marg_path") == 2   # (the options survive)
    eng.close()
    assert len(lp) == len(pp) == len(views)
    for a, b in zip(list(lp) + list(lc) + list(lr), list(pp) + list(pc) + list(pr)):
        assert np.array_equal(a, b)
    gammas = _oracle_gammas(kind, cut, model)
    _check(gammas, lp, lc, "lagged %s" % kind)
    _check_rows(gammas, lr, np.float64, None, "lagged %s" % kind)


# ---- 7. no side effects ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_no_side_effects(kind, M):
    rng = np.random.default_rng(9)
    n = 24
    obs = _rand_obs(kind, n, M, [30000, 7000, 1, 12345], rng)
    m1 = _rand_model(kind, n, M, rng, stay=2.0)
    m2 = _rand_model(kind, n, M, rng, stay=5.0)
    other = _rand_model(kind, n, M, rng, stay=1.0)
    V = _weights(n, 2, other, rng)
    opts = ("score_fallbacks", "score_path", "score_segments", "score_W_max", "score_seglen", "score_W",
            "filter_W", "filter_fallbacks", "filter_path", "filter_seglen", "filter_parallel", "filter_segments",
            "post_W", "post_ws_mb", "marg_W", "marg_ws_mb")

    def sequence(smoothing):
        eng = _engine()
        eng.set_observations(kind, obs, n, nsymbols=M)
        eng.set_option("score_seglen", 1000)                        # (plans of their own that must survive)
        eng.set_option("filter_parallel", 1)
        eng.set_option("filter_seglen", 512)
        if smoothing:
            eng.set_option("smooth_wide", 1)
            eng.set_option("smooth_seglen", 256)
        out = []
        for m in (m1, m2, m1):          # (carried boundaries, warm-up state: a sequence of E-steps)
            if smoothing:
                eng.posterior_decode(*other, confidence=True)
                assert eng.get_option("post_path") == 2
            r = eng.estep(*m, store_gamma=True)
            out += [r.packed.copy(), r.logL_k.copy()]
            if smoothing:
                eng.posterior_marginals(*other, weights=V, dtype=np.float32)
                assert eng.get_option("marg_path") == 2
            out += [eng.gamma(k) for k in range(len(obs))]          # the stored gamma of THAT E-step
            out.append(eng.score([m1, m2]))
            if smoothing:
                eng.posterior_marginals(*other)
                eng.set_option("smooth_seglen", 512)                # (the smoothing plan is made again)
            out.append(_cat(eng.viterbi(*m)))
            paths, C, n0, emis = eng.sample_paths(*m, seed=11)
            out += [_cat(paths) if isinstance(paths, (list, tuple)) else np.asarray(paths), C, n0]
            if smoothing:
                eng.posterior_decode(*other)
            rows, logc = eng.filter_states(*m)
            out += [_cat(rows), _cat(logc)]
            out.append(eng.score([m2, m1]))
            out.append(np.array([eng.get_option(o) for o in opts]))
        eng.close()
        return out

    plain, mixed = sequence(False), sequence(True)
    assert len(plain) == len(mixed)
    for a, b in zip(plain, mixed):
        assert np.array_equal(a, b)


# ---- 8. full size ------------------------------------------------------------------------------------
def test_full_size_64_states():
    """the shape of configs[3]: 64 states, 128 trajectories of 1e5 steps, gaussian; decoding with confidences, and
    float32 rows left on the device"""
    import torch
    n, K, T, model, obs = _full_case()
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    eng.set_option("smooth_wide", 1)
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("post_path") == 2 and eng.get_option("post_fallbacks") == 0
    rows = torch.empty((K * T, n), dtype=torch.float32, device="cuda:0")
    eng.posterior_marginals(*model, dtype=np.float32, out=rows)
    eng.sync()
    assert eng.get_option("marg_path") == 2 and eng.get_option("marg_fallbacks") == 0
    assert eng.get_option("smooth_segments") > K
    eng.close()
    picks = [0, K - 1]
    gammas = _oracle_gammas("gaussian", [obs[k] for k in picks], model)
    _check(gammas, [paths[k] for k in picks], [conf[k] for k in picks], "full size decode")
    _check_rows(gammas, [rows[k * T:(k + 1) * T].cpu().numpy() for k in picks], np.float32, None, "full size rows")
