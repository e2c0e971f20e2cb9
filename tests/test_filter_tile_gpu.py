"""GPU: the matrix-core path of bhmm_filter for 65 to 128 states (k_filter_tile, filter_path 3) against the CPU
oracle, by the route and under the bounds of tests/test_filter_gpu.py (imported, not copied): fp64 rows rtol 1e-8 /
atol 1e-13, fp32 rows 1e-7, projections those bounds carried through the sum, logc within its derived bound, the
sum of logc against the oracle's logL at 1e-11.  No step is left out of any comparison.

Figures of a run on an MI355X at the full shape (128 states, 128 x 1e4): fp32 rows 0.28 of their bound, fp64 logc
within 3.6e-15 of the oracle, the sums of logc within 2.9e-16 (relative) of Engine.score."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_filter_gpu import (ATOL64, RTOL64, RTOL_SUM, TOL32, _cat, _check_forms, _check_logc, _check_rows,
                                   _engine, _run_forms, _truth, _truth_pobs)
from tests.test_marginals_gpu import LENGTHS, _rand_model, _rand_obs, _weights

pytestmark = pytest.mark.gpu

KINDS = [("gaussian", 0), ("discrete", 64), ("discrete", 1000)]


def _tile_engine(kind, obs, n, M, seglen=0, tile=1):
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    eng.set_option("filter_tile", tile)
    eng.set_option("filter_seglen", seglen)
    return eng


# ---- 1. oracle parity -----------------------------------------------------------------------------
@pytest.mark.parametrize("stay", [0, 20])
@pytest.mark.parametrize("kind,M", KINDS)
@pytest.mark.parametrize("n", [65, 80, 81, 96, 100, 112, 113, 128])   # every NT, column tiles filled exactly and not
def test_parity_tile(n, kind, M, stay):
    rng = np.random.default_rng(3000 * n + M + stay)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=float(stay))
    truth = _truth(kind, obs, model)
    eng = _tile_engine(kind, obs, n, M)
    for seglen in (0, 1000, 4000):
        eng.set_option("filter_seglen", seglen)
        assert eng.get_option("filter_seglen") == seglen
        before = eng.get_option("filter_fallbacks")
        results = _run_forms(eng, model, n, rng, 3)
        assert eng.get_option("filter_segments") >= len(LENGTHS)
        _check_forms(truth, results, "tile n=%d %s M=%d seglen=%d stay=%d" % (n, kind, M, seglen, stay))
        if stay == 0:
            assert eng.get_option("filter_fallbacks") == before
            assert eng.get_option("filter_redone") == 0
    eng.close()


# ---- 2. which path a call takes ---------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_which_path(kind, M):
    rng = np.random.default_rng(78 + M)
    n = 100
    eng = _engine()
    min_total = int(eng.get_option("filter_tile_min_total"))
    assert min_total >= 32768 and min_total & (min_total - 1) == 0
    assert eng.get_option("filter_tile") == -1
    with pytest.raises(ValueError):
        eng.set_option("filter_tile", 2)
    with pytest.raises(ValueError):
        eng.set_option("filter_tile_min_total", 1)      # read-only
    with pytest.raises(ValueError):
        eng.set_option("filter_redone", 1)              # read-only
    big = [min_total - 5000, 5000, 1, 300]              # exactly min_total + 301 steps
    model = _rand_model(kind, n, M, rng, stay=1.0)
    obs = _rand_obs(kind, n, M, big, rng)
    truth = _truth(kind, obs, model)
    eng.set_observations(kind, obs, n, nsymbols=M)
    r3, l3 = eng.filter_states(*model)                   # a default call
    assert eng.get_option("filter_path") == 3 and eng.get_option("filter_segments") > len(big)
    eng.set_option("filter_tile", 0)
    r0, l0 = eng.filter_states(*model)
    assert eng.get_option("filter_path") == 0 and eng.get_option("filter_segments") == 0
    eng.set_option("filter_tile", 1)
    eng.set_option("filter_parallel", 0)
    eng.filter_states(*model, probabilities=False)
    assert eng.get_option("filter_path") == 0
    eng.set_option("filter_parallel", -1)
    eng.set_option("filter_tile", -1)
    for lab, (r, l) in (("automatic", (r3, l3)), ("filter_tile=0", (r0, l0))):
        _check_rows(truth, r, np.float64, None, "%s %s" % (lab, kind))
        _check_logc(truth, l, np.float64, "%s %s" % (lab, kind))
    a, b = _cat(r3), _cat(r0)
    worst = float((np.abs(a - b) / (ATOL64 + RTOL64 * np.abs(b))).max())
    print("path 3 against path 0: worst row difference / bound %.3g, worst |logc difference| %.3g"
          % (worst, float(np.abs(_cat(l3) - _cat(l0)).max())))
    assert worst <= 1.0
    assert np.all(np.abs(_cat(l3) - _cat(l0)) <= 2 * RTOL64)
    # the same default call on a small set stays on the serial kernel
    small = _rand_obs(kind, n, M, LENGTHS, rng)
    eng.set_observations(kind, small, n, nsymbols=M)
    eng.filter_states(*model, probabilities=False)
    assert eng.get_option("filter_path") == 0
    eng.close()
    # 129 states and explicit pobs are not eligible
    eng = _engine()
    m129 = _rand_model(kind, 129, M, rng)
    eng.set_observations(kind, _rand_obs(kind, 129, M, [500], rng), 129, nsymbols=M)
    eng.set_option("filter_tile", 1)
    eng.filter_states(*m129, probabilities=False)
    assert eng.get_option("filter_path") == 0
    A, pi, mu, sig = _rand_model("gaussian", n, 0, rng)
    eng.set_observations("explicit", [orc.pobs_gaussian(rng.normal(0, 3, 500), mu, sig)], n)
    eng.filter_states(A, pi)
    assert eng.get_option("filter_path") == 0
    eng.close()


# ---- 3. forced protocol ---------------------------------------------------------------------------
@pytest.mark.parametrize("stay", [5, 200])    # 200: twice the warm-up fails as well, the serial kernel decides
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_forced_fallback(kind, M, stay):
    rng = np.random.default_rng(32 + stay)
    n = 100
    obs = _rand_obs(kind, n, M, [12000, 8000, 2345], rng)
    model = _rand_model(kind, n, M, rng, stay=float(stay))     # slowly mixing
    eng = _tile_engine(kind, obs, n, M, seglen=512)
    eng.set_option("filter_W", 8)                              # far too short: the check must fail
    before = eng.get_option("filter_fallbacks")
    results = _run_forms(eng, model, n, rng, 3)                # (the FIRST pass was the matrix-core one)
    assert eng.get_option("filter_fallbacks") >= before + len(results)
    eng.close()
    _check_forms(_truth(kind, obs, model), results, "forced %s stay=%d" % (kind, stay))


# ---- 4. trajectories outside the kernel's range are done again, the others stand ----------------------
def test_redo_zero_probability_discrete():
    rng = np.random.default_rng(41)
    n, M, z = 100, 64, 3001
    obs = [rng.integers(0, M - 1, T).astype(np.int32) for T in (6000, 5999, 6001, 6002)]
    clean = [o.copy() for o in obs]
    obs[1][z] = M - 1                     # the last symbol appears in trajectory 1 only, at step z
    A, pi, B, _ = _rand_model("discrete", n, M, rng, stay=1.0)
    B[:, M - 1] = 0.0                     # no state emits the last symbol
    B /= B.sum(axis=1)[:, None]
    model = (A, pi, B, None)
    V = _weights(n, 2, (A, pi, np.arange(float(n)), None), rng)
    cut = [obs[0], obs[1][:z], obs[2], obs[3]]
    truth = _truth("discrete", cut, model)
    eng = _tile_engine("discrete", obs, n, M, seglen=512)
    got = {}
    for dtype in (np.float64, np.float32):
        for weights in (None, V):
            rows, logc = eng.filter_states(*model, weights=weights, dtype=dtype)
            assert eng.get_option("filter_path") == 3 and eng.get_option("filter_redone") == 1
            label = "zero at %d %s%s" % (z, np.dtype(dtype).name, "" if weights is None else " Q=2")
            assert not any(np.any(np.isnan(r)) for r in rows) and not any(np.any(np.isnan(l)) for l in logc)
            _check_rows(truth, [rows[0], rows[1][:z], rows[2], rows[3]], dtype, weights, label)
            _check_logc(truth, [logc[0], logc[1][:z], logc[2], logc[3]], dtype, label, dense=False)
            assert rows[1].shape[0] == 5999 and np.all(rows[1][z:] == 0.0)
            assert np.all(logc[1][z:] == -np.inf)
            got[(dtype, weights is None)] = (rows, logc)
    assert eng.get_option("filter_fallbacks") == 0
    # the other three trajectories: bitwise what the call gives without that symbol in the set
    eng.set_observations("discrete", clean, n, nsymbols=M)
    for dtype in (np.float64, np.float32):
        for weights in (None, V):
            rows, logc = eng.filter_states(*model, weights=weights, dtype=dtype)
            assert eng.get_option("filter_path") == 3 and eng.get_option("filter_redone") == 0
            r1, l1 = got[(dtype, weights is None)]
            for k in (0, 2, 3):
                assert np.array_equal(rows[k], r1[k]) and np.array_equal(logc[k], l1[k])
    eng.close()


def test_redo_gaussian_outlier_and_nan():
    rng = np.random.default_rng(43)
    n = 100
    model = _rand_model("gaussian", n, 0, rng, stay=2.0)
    A, pi, mu, sig = model
    obs = [rng.normal(0, 3, T) for T in (6000, 5999, 6001, 6002)]
    obs[0][2500] = 1e6         # every density underflows to zero: a row of ones
    obs[2][777] = np.nan       # a NaN observation: a row of ones
    truth = []
    for o in obs:
        pobs = orc.pobs_gaussian(np.where(np.isnan(o), 1e6, o), mu, sig)
        bad = ~np.all(np.isfinite(pobs), axis=1) | np.all(pobs == 0.0, axis=1)
        pobs[bad] = 1.0
        truth.append(_truth_pobs(A, pobs, pi))
    eng = _tile_engine("gaussian", obs, n, 0, seglen=512)
    results = _run_forms(eng, model, n, rng, 3)
    assert eng.get_option("filter_redone") == 2 and eng.get_option("filter_path") == 3
    assert eng.get_option("filter_fallbacks") == 0
    eng.close()
    _check_forms(truth, results, "outlier and NaN")


# ---- 5. invariance ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [80, 100, 128])
def test_invariance(n, kind, M):
    import torch
    rng = np.random.default_rng(6 + n)
    obs = _rand_obs(kind, n, M, [12000, 7000, 1, 5345, 64, 3001], rng)
    model = _rand_model(kind, n, M, rng, stay=3.0)
    V = _weights(n, 3, model, rng)
    eng = _tile_engine(kind, obs, n, M)
    total = int(eng.offsets[-1])
    got = {}
    for seglen in (512, 1000, 0):
        eng.set_option("filter_seglen", seglen)
        r, l = (_cat(x) for x in eng.filter_states(*model))
        p = _cat(eng.filter_states(*model, weights=V, increments=False)[0])
        assert eng.get_option("filter_path") == 3
        got[seglen] = (r, l, p, eng.get_option("filter_segments"))
    assert got[512][3] > got[1000][3]
    r64, l64, p64, _ = got[0]
    scale = np.abs(V).sum(axis=0)
    for seglen in (512, 1000):
        r, l, p, _ = got[seglen]
        assert np.all(np.abs(r - r64) <= 2 * (ATOL64 + RTOL64 * np.abs(r64)))
        assert np.all(np.abs(l - l64) <= 2 * (RTOL64 + ATOL64))
        assert np.all(np.abs(p - p64) <= 2 * (scale * ATOL64 + RTOL64 * (r64 @ np.abs(V))))
    # repeated calls; rows with and without logc, logc with and without rows
    again = eng.filter_states(*model)
    assert np.array_equal(_cat(again[0]), r64) and np.array_equal(_cat(again[1]), l64)
    assert np.array_equal(_cat(eng.filter_states(*model, increments=False)[0]), r64)
    assert np.array_equal(_cat(eng.filter_states(*model, probabilities=False)[1]), l64)
    # fp32 is the rounded fp64 result: the conversion is the last operation
    r32, l32 = (_cat(x) for x in eng.filter_states(*model, dtype=np.float32))
    p32 = _cat(eng.filter_states(*model, weights=V, dtype=np.float32, increments=False)[0])
    assert np.array_equal(r32, r64.astype(np.float32)) and np.array_equal(l32, l64.astype(np.float32))
    assert np.array_equal(p32, p64.astype(np.float32))
    # device output, tensors and raw addresses: bitwise the host output
    for dtype, tdtype, rref, lref, pref in ((np.float64, torch.float64, r64, l64, p64),
                                            (np.float32, torch.float32, r32, l32, p32)):
        t = torch.full((total, n), -1.0, dtype=tdtype, device="cuda:0")
        tl = torch.full((total,), -1.0, dtype=tdtype, device="cuda:0")
        eng.filter_states(*model, dtype=dtype, out=t, out_increments=tl)
        eng.sync()
        assert np.array_equal(t.cpu().numpy(), rref) and np.array_equal(tl.cpu().numpy(), lref)
        t.fill_(-1.0)
        tl.fill_(-1.0)
        torch.cuda.synchronize()
        assert eng.filter_states(*model, dtype=dtype, out=t.data_ptr(), out_increments=tl.data_ptr()) == (None, None)
        eng.sync()
        assert np.array_equal(t.cpu().numpy(), rref) and np.array_equal(tl.cpu().numpy(), lref)
        tl.fill_(-1.0)
        torch.cuda.synchronize()
        eng.filter_states(*model, dtype=dtype, probabilities=False, out_increments=tl)
        eng.sync()
        assert np.array_equal(tl.cpu().numpy(), lref)
        tp = torch.full((total, 3), -1.0, dtype=tdtype, device="cuda:0")
        eng.filter_states(*model, weights=V, dtype=dtype, increments=False, out=tp)
        eng.sync()
        assert np.array_equal(tp.cpu().numpy(), pref)
    assert eng.get_option("filter_path") == 3 and eng.get_option("filter_redone") == 0
    eng.close()


# ---- 6. consistency with score and the smoothed marginals ------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [72, 128])
def test_consistent_with_score_and_marginals(n, kind, M):
    rng = np.random.default_rng(301 + n + M)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=2.0)
    eng = _tile_engine(kind, obs, n, M, seglen=512)
    rows, logc = eng.filter_states(*model)
    assert eng.get_option("filter_path") == 3
    score = eng.score([model])[0]
    assert eng.get_option("score_path") == 3
    marg = eng.posterior_marginals(*model)
    eng.close()
    sums = np.array([l.sum() for l in logc])
    print("n=%d %s: worst |sum logc - score| / |score| %.3g" % (n, kind, float((np.abs(sums - score) / np.abs(score)).max())))
    np.testing.assert_allclose(sums, score, rtol=RTOL_SUM)
    for r, g in zip(rows, marg):            # gamma_{T-1} = alpha^_{T-1}
        np.testing.assert_allclose(r[-1], g[-1], rtol=RTOL64, atol=ATOL64)


# ---- 7. no side effects ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_no_side_effects(kind, M):
    rng = np.random.default_rng(10)
    n, n2 = 100, 24
    obs = _rand_obs(kind, n, M, [9000, 3000, 1, 2345], rng)
    obs2 = _rand_obs(kind, n2, M, [9000, 3000, 1, 2345], rng)
    m1 = _rand_model(kind, n, M, rng, stay=2.0)
    m2 = _rand_model(kind, n, M, rng, stay=5.0)
    other = _rand_model(kind, n, M, rng, stay=1.0)
    small = _rand_model(kind, n2, M, rng, stay=2.0)
    V = _weights(n, 2, other, rng)
    opts = ("post_W", "post_ws_mb", "post_fallbacks", "post_path", "marg_W", "marg_ws_mb", "marg_fallbacks",
            "marg_path", "score_fallbacks", "score_path", "score_segments", "score_W_max", "score_seglen")

    def sequence(filtering):
        eng = _engine()
        eng.set_observations(kind, obs, n, nsymbols=M)
        eng.set_option("score_seglen", 1000)                        # (a score plan of its own that must survive)
        second = _engine()                                          # a second engine on the 9..64-state path
        second.set_observations(kind, obs2, n2, nsymbols=M)
        second.set_option("filter_parallel", 1)
        if filtering:
            eng.set_option("filter_tile", 1)
            eng.set_option("filter_seglen", 512)
        eng.posterior_decode(*m1)                                   # (so that the counters say something)
        out = []
        for m in (m1, m2):              # (carried boundaries, warm-up state: a sequence of E-steps)
            if filtering:
                eng.filter_states(*other)
            r = eng.estep(*m, store_gamma=True)
            out += [r.packed.copy(), r.logL_k.copy()]
            if filtering:
                eng.filter_states(*other, weights=V, dtype=np.float32)
            out += [eng.gamma(k) for k in range(len(obs))]          # the stored gamma of THAT E-step
            out.append(eng.score([m1, m2]))
            if filtering:
                eng.filter_states(*m, probabilities=False)
                eng.set_option("filter_seglen", 1000)               # (the filter plan is made again)
            out.append(_cat(eng.viterbi(*m)))
            out.append(eng.score([m2, m1]))
            fr, fl = second.filter_states(*small)
            assert second.get_option("filter_path") == 2
            out += [_cat(fr), _cat(fl)]
            if filtering:
                eng.filter_states(*m)
                assert eng.get_option("filter_path") == 3
            out.append(_cat(eng.posterior_decode(*m)))
            out.append(_cat(eng.posterior_marginals(*m)))
            out.append(np.array([eng.get_option(o) for o in opts]))
        second.close()
        eng.close()
        return out

    plain, mixed = sequence(False), sequence(True)
    assert len(plain) == len(mixed)
    for a, b in zip(plain, mixed):
        assert np.array_equal(a, b)


# ---- 8. full shape -----------------------------------------------------------------------------------
def test_full_shape_128_states():
    """128 states, 128 trajectories of 1e4 steps, gaussian; float32 rows and float64 logc left on the device"""
    import torch
    rng = np.random.default_rng(128)
    n, K, T = 128, 128, 10000
    model = _rand_model("gaussian", n, 0, rng)
    flat = rng.normal(0, 3, K * T)
    obs = [flat[k * T:(k + 1) * T] for k in range(K)]
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    rows = torch.empty((K * T, n), dtype=torch.float32, device="cuda:0")
    logc = torch.empty(K * T, dtype=torch.float64, device="cuda:0")
    eng.filter_states(*model, dtype=np.float32, increments=False, out=rows)        # a default call
    assert eng.get_option("filter_path") == 3
    eng.filter_states(*model, probabilities=False, out_increments=logc)
    assert eng.get_option("filter_path") == 3 and eng.get_option("filter_fallbacks") == 0
    assert eng.get_option("filter_redone") == 0
    eng.sync()
    score = eng.score([model])[0]
    eng.close()
    sums = logc.view(K, T).sum(dim=1).cpu().numpy()
    print("full shape: worst |sum logc - score| / |score| %.3g" % float((np.abs(sums - score) / np.abs(score)).max()))
    np.testing.assert_allclose(sums, score, rtol=RTOL_SUM)
    picks = [0, K - 1]
    truth = _truth("gaussian", [obs[k] for k in picks], model)
    _check_rows(truth, [rows[k * T:(k + 1) * T].cpu().numpy() for k in picks], np.float32, None, "full shape rows")
    _check_logc(truth, [logc[k * T:(k + 1) * T].cpu().numpy() for k in picks], np.float64, "full shape logc")
    assert TOL32 == 1e-7
