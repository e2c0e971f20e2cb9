"""GPU: the matrix-core path of bhmm_posterior_decode / bhmm_posterior_marginals for 65 to 128 states (k_filter_tile
forward, k_smooth_tile_bwd backward; post_path / marg_path 3) against the CPU oracle's gamma, under the rules of
tests/test_posterior_gpu.py and tests/test_marginals_gpu.py (imported, not restated): the path exact wherever the
oracle's gap between its two largest gamma exceeds GAP, at most MAX_LEFT_OUT of a case's steps left out, the confidence
within CONF_TOL on all steps, rows at that module's fp64 and fp32 bounds, projections those bounds carried through the
sum.  Every engine sets smooth_tile = 1 unless the test is about the choice.

The 48 parity cases were checked on the CPU with the oracle alone: of 23 734 steps each, 0 are left out by the GAP
rule (the smallest top-two gap is 9.05e-9, at n = 113, M = 1000, stay 0), so the MAX_LEFT_OUT cap hides nothing."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_filter_gpu import ATOL64 as F_ATOL64, RTOL64 as F_RTOL64
from tests.test_marginals_gpu import ATOL64, RTOL64, TOL32, _check as _check_rows, _weights
from tests.test_posterior_gpu import (CONF_TOL, GAP, LENGTHS, MAX_LEFT_OUT, _check, _oracle_gammas, _rand_model,
                                      _rand_obs)

pytestmark = pytest.mark.gpu

KINDS = [("gaussian", 0), ("discrete", 64), ("discrete", 1000)]
assert LENGTHS == [1, 2, 37, 500, 3001, 64, 129, 20000] and MAX_LEFT_OUT == 1e-4


def _engine():
    from bhmm_amd.engine import Engine
    return Engine(0)


def _smooth_engine(kind, obs, n, M, seglen=0, tile=1):
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    eng.set_option("smooth_tile", tile)
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


def _rows_within(a, b, factor):
    """|a - b| within factor times the fp64 row bound of tests/test_marginals_gpu.py"""
    assert np.all(np.abs(a - b) <= factor * (ATOL64 + RTOL64 * np.abs(b)))


def _all_forms(eng, model, n, rng, results, label):
    """decode with confidence, rows in both dtypes, projections on 1, 3 and 8 columns in both dtypes"""
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("post_path") == 3
    results.append(("decode", paths, conf, None, None, label))
    for dtype in (np.float64, np.float32):
        rows = eng.posterior_marginals(*model, dtype=dtype)
        assert eng.get_option("marg_path") == 3
        results.append(("rows", rows, None, dtype, None, "%s %s" % (label, np.dtype(dtype).name)))
        for Q in (1, 3, 8):
            V = _weights(n, Q, model, rng)
            rows = eng.posterior_marginals(*model, weights=V, dtype=dtype)
            assert eng.get_option("marg_path") == 3
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
@pytest.mark.parametrize("n", [65, 80, 81, 96, 100, 112, 113, 128])   # every NT, column tiles filled exactly and not
def test_parity(n, kind, M, stay):
    rng = np.random.default_rng(3000 * n + M + stay)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=float(stay))
    gammas = _oracle_gammas(kind, obs, model)
    eng = _smooth_engine(kind, obs, n, M)
    results = []
    for seglen in (0, 1000, 4000):
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
# The automatic rule (smooth_tile = -1, at least smooth_tile_min_total steps) per call form (decode, decode with
# confidences, rows, projection): smooth_tile_auto of csrc/smooth_tile_api.hpp, read off
# profiles/smooth/smooth_tile_time.json (tools/smooth_tile_time.py; the table in DESIGN.md section 18).
AUTO = (False, False, False, False)


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
    rng = np.random.default_rng(78 + M)
    n = 100
    eng = _engine()
    min_total = int(eng.get_option("smooth_tile_min_total"))
    assert min_total >= 32768 and min_total & (min_total - 1) == 0
    assert eng.get_option("smooth_tile") == -1
    model = _rand_model(kind, n, M, rng, stay=1.0)
    # a default engine on a small set stays on the generic path
    small = _rand_obs(kind, n, M, [1, 37, 500, 3001], rng)
    eng.set_observations(kind, small, n, nsymbols=M)
    assert _paths_of_the_four_forms(eng, model, n, rng) == (0, 0, 0, 0)
    assert eng.get_option("smooth_segments") == 0
    # the automatic rule on exactly min_total + 301 steps
    big = [min_total - 5000, 5000, 1, 300]
    for nn in (65, 128):
        m = _rand_model(kind, nn, M, rng, stay=1.0)
        eng.set_observations(kind, _rand_obs(kind, nn, M, big, rng), nn, nsymbols=M)
        assert _paths_of_the_four_forms(eng, m, nn, rng) == tuple(3 if a else 0 for a in AUTO), nn
    # smooth_tile = 0 stays on the generic path on any set, 1 takes the new one; smooth_wide does not matter here
    eng.set_observations(kind, _rand_obs(kind, n, M, big, rng), n, nsymbols=M)
    eng.set_option("smooth_tile", 0)
    eng.set_option("smooth_wide", 1)
    assert _paths_of_the_four_forms(eng, model, n, rng) == (0, 0, 0, 0)
    eng.set_option("smooth_tile", 1)
    eng.set_option("smooth_wide", 0)
    assert _paths_of_the_four_forms(eng, model, n, rng) == (3, 3, 3, 3)
    assert eng.get_option("smooth_segments") > len(big)
    with pytest.raises(ValueError):
        eng.set_option("smooth_tile", 2)
    for read_only in ("smooth_segments", "smooth_tile_min_total"):
        with pytest.raises(ValueError):
            eng.set_option(read_only, 1)
    eng.close()
    # 64 and 129 states and explicit pobs are not eligible
    eng = _engine()
    eng.set_option("smooth_tile", 1)
    for nn in (64, 129):
        mm = _rand_model("gaussian", nn, 0, rng)
        eng.set_observations("gaussian", [rng.normal(0, 3, 500)], nn)
        eng.posterior_decode(*mm)
        eng.posterior_marginals(*mm)
        assert eng.get_option("post_path") == 0 and eng.get_option("marg_path") == 0
    A, pi, mu, sig = _rand_model("gaussian", 70, 0, rng)
    eng.set_observations("explicit", [orc.pobs_gaussian(rng.normal(0, 3, 500), mu, sig)], 70)
    eng.posterior_decode(A, pi)
    eng.posterior_marginals(A, pi)
    assert eng.get_option("post_path") == 0 and eng.get_option("marg_path") == 0
    assert eng.get_option("smooth_segments") == 0
    eng.close()


# ---- 3. forced protocol ---------------------------------------------------------------------------
@pytest.mark.parametrize("stay", [5, 200])    # 200: twice the warm-up fails as well, the generic path decides
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_forced_fallback(kind, M, stay):
    rng = np.random.default_rng(33 + stay)
    n = 100
    obs = _rand_obs(kind, n, M, [9000, 5000, 2345], rng)
    model = _rand_model(kind, n, M, rng, stay=float(stay))
    eng = _smooth_engine(kind, obs, n, M, seglen=512)
    eng.set_option("smooth_W", 4)                              # far too short
    before = eng.get_option("post_fallbacks"), eng.get_option("marg_fallbacks")
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("post_path") == 3                    # (the FIRST pass was the matrix-core one)
    rows = eng.posterior_marginals(*model)
    assert eng.get_option("marg_path") == 3
    after = eng.get_option("post_fallbacks"), eng.get_option("marg_fallbacks")
    eng.close()
    if stay == 200:     # the check must fail
        assert after == (before[0] + 1, before[1] + 1)
    else:               # verified, or one retry
        assert before[0] <= after[0] <= before[0] + 1 and before[1] <= after[1] <= before[1] + 1
    gammas = _oracle_gammas(kind, obs, model)
    _check(gammas, paths, conf, "forced %s stay=%d" % (kind, stay))
    _check_rows(gammas, rows, np.float64, None, "forced %s stay=%d" % (kind, stay))


# ---- 4. the workspace budget ------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_budget(kind, M):
    import torch
    from bhmm_amd import _lib
    n = 128
    rng = np.random.default_rng(5 + n)
    obs = _rand_obs(kind, n, M, [20000, 7000, 1, 12345, 64, 3001], rng)
    model = _rand_model(kind, n, M, rng, stay=3.0)
    V = _weights(n, 3, model, rng)
    gammas = _oracle_gammas(kind, obs, model)
    eng = _smooth_engine(kind, obs, n, M)
    total = int(eng.offsets[-1])

    def run():
        p, c = eng.posterior_decode(*model, confidence=True)
        r = eng.posterior_marginals(*model)
        q = eng.posterior_marginals(*model, weights=V)
        assert eng.get_option("post_path") == 3 and eng.get_option("marg_path") == 3
        return [np.array(x) for x in p], _cat(c), _cat(r), _cat(q)

    got = {}
    for mb in (0, 8192, 1):          # 1 MiB: 1024 rows of 128 states -- many ranges
        eng.set_option("smooth_ws_mb", mb)
        assert eng.get_option("smooth_ws_mb") == mb
        got[mb] = run()
        again = run()                # repeats at a fixed budget: bitwise
        for a, b in zip([_cat(got[mb][0])] + list(got[mb][1:]), [_cat(again[0])] + list(again[1:])):
            assert np.array_equal(a, b)
        _check(gammas, got[mb][0], np.split(got[mb][1], np.cumsum([len(o) for o in obs])[:-1]), "budget %d" % mb)
        _check_rows(gammas, np.split(got[mb][2], np.cumsum([len(o) for o in obs])[:-1]), np.float64, None,
                    "budget %d" % mb)
    for a, b in zip(got[0][1:], got[8192][1:]):            # both are one range, the whole plan
        assert np.array_equal(a, b)
    # the tiles change with the ranges: each is within the bound of the same oracle rows, so within twice the bound
    # of each other; paths equal off the GAP steps
    p0, c0, r0, q0 = got[0]
    p1, c1, r1, q1 = got[1]
    _rows_within(r1, r0, 2)
    assert np.all(np.abs(q1 - q0) <= 2 * (np.abs(V).sum(axis=0) * ATOL64 + RTOL64 * (r0 @ np.abs(V))))
    _paths_equal_off_gap(gammas, p1, p0)
    # at the smallest budget: output location and path element type, bitwise
    r32 = _cat(eng.posterior_marginals(*model, dtype=np.float32))
    assert r32.dtype == np.float32 and np.array_equal(r32, r1.astype(np.float32))    # the conversion is last
    for dtype, tdtype, ref in ((np.float64, torch.float64, r1), (np.float32, torch.float32, r32)):
        t = torch.full((total, n), -1.0, dtype=tdtype, device="cuda:0")
        eng.posterior_marginals(*model, dtype=dtype, out=t)
        eng.sync()
        assert np.array_equal(t.cpu().numpy(), ref)
        t.fill_(-1.0)
        torch.cuda.synchronize()
        assert eng.posterior_marginals(*model, dtype=dtype, out=t.data_ptr()) is None
        eng.sync()
        assert np.array_equal(t.cpu().numpy(), ref)
        pinned = torch.full((total, n), -1.0, dtype=tdtype).pin_memory()
        eng.posterior_marginals(*model, dtype=dtype, out=pinned)
        assert np.array_equal(pinned.numpy(), ref)
    tp = torch.full((total, 3), -1.0, dtype=torch.float64, device="cuda:0")
    eng.posterior_marginals(*model, weights=V, out=tp)
    eng.sync()
    assert np.array_equal(tp.cpu().numpy(), q1)
    assert np.array_equal(_cat(eng.posterior_decode(*model)), _cat(p1))              # confidence off: the same path
    A, pi, e0, e1 = eng._model_ptrs(*model)                                          # int32 through the C entry
    p32 = np.empty(total, dtype=np.int32)
    c32 = np.empty(total, dtype=np.float32)
    _lib.check(eng._L.bhmm_posterior_decode(eng._h, A, pi, e0, e1, ctypes.c_void_p(p32.ctypes.data), 0,
                                            ctypes.c_void_p(c32.ctypes.data)))
    assert eng.get_option("post_path") == 3
    assert np.array_equal(p32, _cat(p1).astype(np.int32)) and np.array_equal(c32, c1)
    eng.close()


# ---- 5. consistency --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [70, 128])
def test_consistency(n, kind, M):
    rng = np.random.default_rng(300 + n + M)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=2.0)
    gammas = _oracle_gammas(kind, obs, model)
    eng = _smooth_engine(kind, obs, n, M, seglen=512)
    rows = eng.posterior_marginals(*model)
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("marg_path") == 3 and eng.get_option("post_path") == 3
    filt = eng.filter_states(*model, increments=False)[0]
    eng.set_option("smooth_tile", 0)
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
    # path 3 against path 0
    _rows_within(_cat(rows), _cat(rows0), 2)
    _paths_equal_off_gap(gammas, paths, paths0)
    assert np.all(np.abs(_cat(conf).astype(np.float64) - _cat(conf0)) <= 2 * CONF_TOL)


# ---- 6. edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("kind,M,n", [("gaussian", 0, 65), ("discrete", 16, 97), ("gaussian", 0, 128)])
def test_shortest_trajectories(kind, M, n, T):
    rng = np.random.default_rng(2 + n + T)
    obs = _rand_obs(kind, n, M, [T], rng)
    model = _rand_model(kind, n, M, rng)
    eng = _smooth_engine(kind, obs, n, M)
    results = []
    _all_forms(eng, model, n, rng, results, "T=%d %s n=%d" % (T, kind, n))
    assert eng.get_option("smooth_segments") == 1
    eng.close()
    _check_all(_oracle_gammas(kind, obs, model), results)


EDGE_LENGTHS = [1024, 256, 257, 255, 512, 4, 2048]


@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_warm_ups_that_reach_past_both_trajectory_ends(kind, M):
    """lengths that are multiples of the segment length, one step more and one step less; warm-ups longer than the
    distance to either end of the trajectory (and than whole trajectories): those segments start exactly"""
    rng = np.random.default_rng(8)
    n = 81
    obs = _rand_obs(kind, n, M, EDGE_LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=2.0)
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


# ---- 7. trouble: the generic route answers, nothing is counted ------------------------------------------
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


def _both_calls(kind, obs, n, M, model, tile):
    """the outcomes of the two calls on a fresh engine, and what the fallback counters and the path say"""
    eng = _smooth_engine(kind, obs, n, M, seglen=256, tile=tile)
    dec = _outcome(lambda: [_cat(x) for x in eng.posterior_decode(*model, confidence=True)])
    path = eng.get_option("post_path")
    mar = _outcome(lambda: [_cat(eng.posterior_marginals(*model))])
    counters = (eng.get_option("post_fallbacks"), eng.get_option("marg_fallbacks"))
    path = (path, eng.get_option("marg_path"))
    eng.close()
    return dec, mar, counters, path


def _generic_route_answers(kind, obs, n, M, model):
    d1, m1, c1, path1 = _both_calls(kind, obs, n, M, model, 1)
    d0, m0, c0, path0 = _both_calls(kind, obs, n, M, model, 0)
    assert path1 == (3, 3) and path0 == (0, 0)
    _same_outcome(d1, d0)
    _same_outcome(m1, m0)
    assert c1 == (0, 0)


# seglen 256 cuts the 3000 steps of trajectory 0 into 12 segments that start at 250 q rounded down to 4
@pytest.mark.parametrize("where", ["inside", "segment_first", "segment_last", "backward_warmup", "forward_warmup",
                                   "trajectory_first", "trajectory_last", "nan"])
def test_gaussian_outlier_takes_the_generic_route(where):
    n = 100
    rng = np.random.default_rng(17)
    obs = [rng.normal(0, 3, T) for T in (3000, 500, 1)]
    k, t, v = {"inside": (0, 100, 1e6), "segment_first": (0, 2248, 1e6), "segment_last": (0, 1999, -1e6),
               "backward_warmup": (0, 2260, -1e6), "forward_warmup": (0, 1990, 1e6), "trajectory_first": (1, 0, 1e6),
               "trajectory_last": (1, 499, -1e6), "nan": (0, 700, np.nan)}[where]
    obs[k][t] = v               # 1e6: every density underflows to zero
    model = _rand_model("gaussian", n, 0, rng, stay=1.0)
    _generic_route_answers("gaussian", obs, n, 0, model)


@pytest.mark.parametrize("z", [150, 2500])
@pytest.mark.parametrize("n,M", [(65, 5), (128, 1000)])
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
    _generic_route_answers("discrete", obs, n, M, (A, pi, B, None))


# ---- 8. no side effects ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_no_side_effects(kind, M):
    rng = np.random.default_rng(9)
    n = 100
    obs = _rand_obs(kind, n, M, [9000, 3000, 1, 2345], rng)
    m1 = _rand_model(kind, n, M, rng, stay=2.0)
    m2 = _rand_model(kind, n, M, rng, stay=5.0)
    other = _rand_model(kind, n, M, rng, stay=1.0)
    V = _weights(n, 2, other, rng)
    opts = ("score_fallbacks", "score_path", "score_segments", "score_W_max", "score_seglen", "score_W",
            "filter_W", "filter_fallbacks", "filter_path", "filter_seglen", "filter_parallel", "filter_segments",
            "filter_tile", "filter_redone", "post_W", "post_ws_mb", "marg_W", "marg_ws_mb")

    def sequence(smoothing):
        eng = _engine()
        eng.set_observations(kind, obs, n, nsymbols=M)
        eng.set_option("score_seglen", 1000)                        # (plans of their own that must survive)
        eng.set_option("filter_tile", 1)
        eng.set_option("filter_seglen", 512)
        if smoothing:
            eng.set_option("smooth_tile", 1)
            eng.set_option("smooth_seglen", 256)
        out = []
        for m in (m1, m2, m1):          # (carried boundaries, warm-up state: a sequence of E-steps)
            if smoothing:
                eng.posterior_decode(*other, confidence=True)
                assert eng.get_option("post_path") == 3
            r = eng.estep(*m, store_gamma=True)
            out += [r.packed.copy(), r.logL_k.copy()]
            if smoothing:
                eng.posterior_marginals(*other, weights=V, dtype=np.float32)
                assert eng.get_option("marg_path") == 3
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


# ---- 9. full shape -----------------------------------------------------------------------------------
def test_full_shape_128_states():
    """128 states, 128 trajectories of 1e4 steps, gaussian; decoding with confidences, and float32 rows left on the
    device.  Three trajectories against the oracle, mass identities on the rest"""
    import torch
    rng = np.random.default_rng(128)
    n, K, T = 128, 128, 10000
    model = _rand_model("gaussian", n, 0, rng)
    flat = rng.normal(0, 3, K * T)
    obs = [flat[k * T:(k + 1) * T] for k in range(K)]
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    eng.set_option("smooth_tile", 1)
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("post_path") == 3 and eng.get_option("post_fallbacks") == 0
    rows = torch.empty((K * T, n), dtype=torch.float32, device="cuda:0")
    eng.posterior_marginals(*model, dtype=np.float32, out=rows)
    eng.sync()
    assert eng.get_option("marg_path") == 3 and eng.get_option("marg_fallbacks") == 0
    assert eng.get_option("smooth_segments") > K
    eng.close()
    picks = [0, K // 2, K - 1]
    gammas = _oracle_gammas("gaussian", [obs[k] for k in picks], model)
    _check(gammas, [paths[k] for k in picks], [conf[k] for k in picks], "full shape decode")
    _check_rows(gammas, [rows[k * T:(k + 1) * T].cpu().numpy() for k in picks], np.float32, None, "full shape rows")
    # every element is within TOL32 of a gamma row, which sums to one: the sum of n of them within n TOL32
    mass = rows.sum(dim=1, dtype=torch.float64)
    assert float((mass - 1.0).abs().max()) <= n * TOL32
    assert int(_cat(paths).max()) < n
    # the largest element within TOL32 of the largest gamma, the confidence within CONF_TOL of it
    top = rows.max(dim=1).values.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(top - _cat(conf).astype(np.float64)) <= TOL32 + CONF_TOL)
