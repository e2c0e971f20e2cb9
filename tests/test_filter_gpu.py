"""GPU: bhmm_filter / Engine.filter_states / bhmm_amd.filter_states -- the filtered probabilities alpha^_t(i) of
every step and the increments log c_t = log p(o_t | o_0 .. o_{t-1}), in double or float, plain or projected,
against the CPU oracle: orc.forward(A, pobs, pi) on orc.pobs_gaussian / orc.pobs_discrete gives the rows, and
log c_t is computed from them in numpy (c_0 = sum pi o p_0, c_t = (alpha^_{t-1} A) . p_t).

Tolerances (the project's own, or derived from them):
  fp64 rows    rtol 1e-8, atol 1e-13 -- the gamma rule of tests/test_estep_gpu.py;
  fp32 rows    1e-7 absolute;
  projections  those two bounds carried through the sum, as tests/test_marginals_gpu.py::_check does;
  fp64 logc    |err| <= rtol + atol * (sum_j (sum_i A_ij) p_t(j)) / c_t: a row within atol + rtol * alpha^_{t-1}(i)
               per entry moves c_t = sum_i alpha^_{t-1}(i) sum_j A_ij p_t(j) by at most
               atol * sum_i sum_j A_ij p_t(j) + rtol * c_t, and d log c = dc / c to first order.  At t = 0 no row
               enters c_0 = sum_j pi_j p_0(j); the same form with pi in the place of the row, i.e.
               rtol + atol * (sum_j p_0(j)) / c_0, is used there (it is not smaller than rtol);
  fp32 logc    that bound plus 2^-24 * |want| (the rounding of the float);
  sum_t logc   against the oracle's logL: rtol 1e-11, the RTOL of tests/test_score_gpu.py.
No step is left out of any comparison."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_marginals_gpu import LENGTHS, _rand_model, _rand_obs, _weights

pytestmark = pytest.mark.gpu

RTOL64, ATOL64 = 1e-8, 1e-13
TOL32 = 1e-7
RTOL_SUM = 1e-11


def _engine():
    from bhmm_amd.engine import Engine
    return Engine(0)


def _cat(xs):
    return np.concatenate([np.asarray(x) for x in xs])


def _truth_pobs(A, pobs, pi):
    """(rows, logc, extra, logL) of one trajectory from its emission rows; extra: the factor of atol in the
    bound of logc"""
    A, pi = np.asarray(A, dtype=np.float64), np.asarray(pi, dtype=np.float64)
    logL, alpha = orc.forward(A, pobs, pi)
    c = np.empty(len(pobs))
    extra = np.empty(len(pobs))
    c[0] = np.dot(pi, pobs[0])
    extra[0] = pobs[0].sum() / c[0]
    c[1:] = np.einsum('tj,tj->t', alpha[:-1] @ A, pobs[1:])
    extra[1:] = (pobs[1:] @ A.sum(axis=0)) / c[1:]
    return alpha, np.log(c), extra, logL


def _pobs(kind, o, model):
    return orc.pobs_gaussian(o, model[2], model[3]) if kind == "gaussian" else orc.pobs_discrete(o, model[2])


def _truth(kind, obs, model):
    return [_truth_pobs(model[0], _pobs(kind, o, model), model[1]) for o in obs]


def _check_rows(truth, rows, dtype, V=None, label=""):
    """every row against the oracle; prints the worst figures before it asserts"""
    dtype = np.dtype(dtype)
    scale = np.ones(truth[0][0].shape[1]) if V is None else np.abs(V).sum(axis=0)
    worst_abs = worst_ratio = 0.0
    for (a, _, _, _), r in zip(truth, rows):
        want = a if V is None else a @ V
        assert r.shape == want.shape and r.dtype == dtype, (label, r.shape, want.shape, r.dtype)
        err = np.abs(r.astype(np.float64) - want)
        assert np.all(np.isfinite(err)), label
        worst_abs = max(worst_abs, float((err / np.where(scale > 0, scale, 1.0)).max()))
        if dtype == np.float64:
            bound = scale * ATOL64 + RTOL64 * (np.abs(a) if V is None else a @ np.abs(V))
        else:
            bound = scale * TOL32 * np.ones_like(want)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        worst_ratio = max(worst_ratio, float(ratio.max()))
    print("%s: worst |row - oracle| / scale %.3g, worst error / bound %.3g" % (label, worst_abs, worst_ratio))
    assert worst_ratio <= 1.0, label


def _check_logc(truth, logc, dtype, label="", dense=True):
    """dense: the model has no structural zeros, so the bound itself must stay far below 1e-6"""
    dtype = np.dtype(dtype)
    worst_abs = worst_ratio = worst_bound = worst_sum = 0.0
    for (_, want, extra, logL), l in zip(truth, logc):
        assert l.shape == want.shape and l.dtype == dtype, (label, l.shape, l.dtype)
        got = l.astype(np.float64)
        err = np.abs(got - want)
        assert np.all(np.isfinite(err)), label
        bound = RTOL64 + ATOL64 * extra
        worst_bound = max(worst_bound, float(bound.max()))
        if dtype == np.float32:
            bound = bound + 2.0 ** -24 * np.abs(want)
        worst_abs = max(worst_abs, float(err.max()))
        worst_ratio = max(worst_ratio, float((err / bound).max()))
        if dtype == np.float64:
            worst_sum = max(worst_sum, abs(got.sum() - logL) / abs(logL))
    print("%s: worst |logc - oracle| %.3g, worst error / bound %.3g, largest fp64 bound %.3g, worst sum rel. %.3g"
          % (label, worst_abs, worst_ratio, worst_bound, worst_sum))
    assert not dense or worst_bound < 1e-6, label
    assert worst_ratio <= 1.0, label
    assert worst_sum <= RTOL_SUM, label


def _run_forms(eng, model, n, rng, path):
    """every output form of both dtypes on the loaded observations: [(rows, logc, dtype, V, label)]"""
    results = []
    for dtype in (np.float64, np.float32):
        name = np.dtype(dtype).name
        rows, logc = eng.filter_states(*model, dtype=dtype)
        assert eng.get_option("filter_path") == path
        results.append((rows, logc, dtype, None, name))
        for Q in (1, 2, 8):
            V = _weights(n, Q, model, rng)
            rows, logc = eng.filter_states(*model, weights=V, dtype=dtype, increments=Q == 2)
            assert eng.get_option("filter_path") == path
            assert (logc is not None) == (Q == 2)
            results.append((rows, logc, dtype, V, "%s Q=%d" % (name, Q)))
        rows, logc = eng.filter_states(*model, dtype=dtype, probabilities=False)
        assert rows is None and eng.get_option("filter_path") == path
        results.append((None, logc, dtype, None, "%s logc alone" % name))
    return results


def _check_forms(truth, results, label):
    for rows, logc, dtype, V, lab in results:
        if rows is not None:
            _check_rows(truth, rows, dtype, V, "%s %s" % (label, lab))
        if logc is not None:
            _check_logc(truth, logc, dtype, "%s %s" % (label, lab))


# ---- 1. oracle parity, fused path -----------------------------------------------------------------
@pytest.mark.parametrize("stay", [0, 20])
@pytest.mark.parametrize("chunk", [0, 64, 100000])
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 3), ("discrete", 64), ("discrete", 1000)])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_parity_fused(n, kind, M, chunk, stay):
    rng = np.random.default_rng(1000 * n + M + chunk % 7 + stay)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=float(stay))
    truth = _truth(kind, obs, model)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=chunk)
    results = _run_forms(eng, model, n, rng, 1)
    fallbacks = eng.get_option("filter_fallbacks")
    eng.close()
    _check_forms(truth, results, "fused n=%d %s M=%d chunk=%d stay=%d" % (n, kind, M, chunk, stay))
    if stay == 0:
        assert fallbacks == 0


# ---- 2. the same parity on the serial path ---------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [9, 24, 64, 100, 200])
def test_parity_serial(n, kind, M):
    rng = np.random.default_rng(7 * n + M)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng)
    truth = _truth(kind, obs, model)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    results = _run_forms(eng, model, n, rng, 0)
    eng.close()
    _check_forms(truth, results, "serial n=%d %s" % (n, kind))


@pytest.mark.parametrize("n", [3, 8, 12, 100])
def test_parity_explicit_pobs(n):
    import bhmm_amd
    rng = np.random.default_rng(50 + n)
    A, pi, mu, sig = _rand_model("gaussian", n, 0, rng)
    o = rng.normal(0, 3, 5000)
    pobs = orc.pobs_gaussian(o, mu, sig)
    truth = [_truth_pobs(A, pobs, pi)]
    V = _weights(n, 2, (A, pi, mu, sig), rng)
    for dtype in (np.float64, np.float32):
        rows, logc = bhmm_amd.hidden.filter_states(A, pobs, pi, dtype=dtype)
        _check_rows(truth, [rows], dtype, None, "explicit n=%d" % n)
        _check_logc(truth, [logc], dtype, "explicit n=%d" % n)
        rows, logc = bhmm_amd.hidden.filter_states(A, pobs, pi, weights=V, dtype=dtype, increments=False)
        assert logc is None
        _check_rows(truth, [rows], dtype, V, "explicit n=%d Q=2" % n)
        rows, logc = bhmm_amd.hidden.filter_states(A, pobs, pi, dtype=dtype, probabilities=False)
        assert rows is None
        _check_logc(truth, [logc], dtype, "explicit n=%d logc alone" % n)
    eng = _engine()
    eng.set_observations("explicit", [pobs], n)
    eng.filter_states(A, pi)
    assert eng.get_option("filter_path") == 0
    eng.close()


# ---- 3. forced protocol ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_forced_fallback(kind, M):
    rng = np.random.default_rng(31)
    n = 8
    obs = _rand_obs(kind, n, M, [60000, 40000, 12345], rng)
    model = _rand_model(kind, n, M, rng, stay=200.0)     # slowly mixing
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=512)
    eng.set_option("filter_W", 4)                        # far too short: the check must fail
    assert eng.get_option("filter_W") == 4
    before = eng.get_option("filter_fallbacks")
    results = _run_forms(eng, model, n, rng, 1)          # (the FIRST pass was the fused one)
    assert eng.get_option("filter_fallbacks") > before
    eng.close()
    _check_forms(_truth(kind, obs, model), results, "forced %s" % kind)


# ---- 4. invariance, all bitwise --------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_invariance(kind, M):
    import torch
    rng = np.random.default_rng(5)
    n = 8
    obs = _rand_obs(kind, n, M, [20000, 7000, 1, 12345, 64, 3001], rng)
    model = _rand_model(kind, n, M, rng, stay=3.0)
    V = _weights(n, 3, model, rng)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=256)
    total = int(eng.offsets[-1])
    r64, l64 = (_cat(x) for x in eng.filter_states(*model))
    p64 = _cat(eng.filter_states(*model, weights=V)[0])
    again = eng.filter_states(*model)
    assert np.array_equal(_cat(again[0]), r64) and np.array_equal(_cat(again[1]), l64)      # repeated calls
    # rows with and without logc requested, logc with and without rows
    assert np.array_equal(_cat(eng.filter_states(*model, increments=False)[0]), r64)
    assert np.array_equal(_cat(eng.filter_states(*model, weights=V, increments=False)[0]), p64)
    assert np.array_equal(_cat(eng.filter_states(*model, probabilities=False)[1]), l64)
    # fp32 is the rounded fp64 result: the conversion is the last operation
    r32, l32 = (_cat(x) for x in eng.filter_states(*model, dtype=np.float32))
    p32 = _cat(eng.filter_states(*model, weights=V, dtype=np.float32)[0])
    assert r32.dtype == np.float32 and np.array_equal(r32, r64.astype(np.float32))
    assert l32.dtype == np.float32 and np.array_equal(l32, l64.astype(np.float32))
    assert np.array_equal(p32, p64.astype(np.float32))
    assert np.array_equal(_cat(eng.filter_states(*model, dtype=np.float32, increments=False)[0]), r32)
    # a caller's host buffers
    out, outl = np.empty((total, n)), np.empty(total)
    rv, lv = eng.filter_states(*model, out=out, out_increments=outl)
    assert np.array_equal(out, r64) and np.array_equal(outl, l64)
    assert np.shares_memory(rv[0], out) and np.shares_memory(lv[1], outl)
    # device output, tensors and raw addresses: bitwise the host output
    for dtype, tdtype, rref, lref in ((np.float64, torch.float64, r64, l64), (np.float32, torch.float32, r32, l32)):
        t = torch.full((total, n), -1.0, dtype=tdtype, device="cuda:0")
        tl = torch.full((total,), -1.0, dtype=tdtype, device="cuda:0")
        tv, tlv = eng.filter_states(*model, dtype=dtype, out=t, out_increments=tl)
        eng.sync()
        assert np.array_equal(t.cpu().numpy(), rref) and np.array_equal(tl.cpu().numpy(), lref)
        assert tv[1].shape == (7000, n) and tv[1].data_ptr() == t[20000:].data_ptr()
        assert tlv[1].shape == (7000,) and tlv[1].data_ptr() == tl[20000:].data_ptr()
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
    tp = torch.empty((total, 3), dtype=torch.float32, device="cuda:0")
    eng.filter_states(*model, weights=V, dtype=np.float32, increments=False, out=tp)
    eng.sync()
    assert np.array_equal(tp.cpu().numpy(), p32)
    # pinned host tensors
    th = torch.empty((total, n), dtype=torch.float64).pin_memory()
    thl = torch.empty(total, dtype=torch.float64).pin_memory()
    eng.filter_states(*model, out=th, out_increments=thl)
    assert np.array_equal(th.numpy(), r64) and np.array_equal(thl.numpy(), l64)
    assert eng.get_option("filter_path") == 1
    # the C ABI refuses what it cannot do
    from bhmm_amd import _lib
    A, pi, e0, e1 = eng._model_ptrs(*model)
    buf = np.empty((total, n))
    bp = ctypes.c_void_p(buf.ctypes.data)
    for Vp, Q, rp, lp, flags in ((None, 2, bp, None, 0), (_lib.dp(V), 0, bp, None, 0),
                                 (_lib.dp(np.ones((n, 9))), 9, bp, None, 0), (None, 0, bp, None, 4),
                                 (None, 0, None, None, 0)):
        with pytest.raises(ValueError):
            _lib.check(eng._L.bhmm_filter(eng._h, A, pi, e0, e1, Vp, Q, rp, lp, flags))
    eng.close()


# ---- 5. consistency with score and the smoothed marginals ------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [2, 5, 8, 12])
def test_consistent_with_score_and_marginals(n, kind, M):
    rng = np.random.default_rng(300 + n + M)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=2.0)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=128)
    rows, logc = eng.filter_states(*model)
    score = eng.score([model])[0]
    marg = eng.posterior_marginals(*model)
    eng.close()
    sums = np.array([l.sum() for l in logc])
    print("n=%d %s: worst |sum logc - score| / |score| %.3g" % (n, kind, float((np.abs(sums - score) / np.abs(score)).max())))
    np.testing.assert_allclose(sums, score, rtol=RTOL_SUM)
    # gamma_{T-1} = alpha^_{T-1}
    for r, g in zip(rows, marg):
        np.testing.assert_allclose(r[-1], g[-1], rtol=RTOL64, atol=ATOL64)


# ---- 6. edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 64])
def test_gaussian_outliers_nan_and_denormal_rows(chunk):
    rng = np.random.default_rng(17)
    n = 4
    A, pi, _, _ = _rand_model("gaussian", n, 0, rng, stay=2.0)
    mu, sig = np.array([0.0, 0.02, 0.04, 0.06]), np.ones(n)
    model = (A, pi, mu, sig)
    obs = [rng.normal(0, 1, T) for T in (3000, 500, 1)]
    obs[0][100] = 1e6          # every density underflows to zero: a row of ones
    obs[0][1999] = -1e6
    obs[0][700] = np.nan       # a NaN observation: a row of ones
    obs[1][0] = 1e6            # ... at the first step
    obs[0][1200] = 37.9        # densities of about 1e-312: a denormal row
    obs[0][1201] = 37.9
    obs[1][300] = -37.9
    truth = []
    for o in obs:
        pobs = orc.pobs_gaussian(np.where(np.isnan(o), 1e6, o), mu, sig)
        bad = ~np.all(np.isfinite(pobs), axis=1) | np.all(pobs == 0.0, axis=1)
        pobs[bad] = 1.0
        truth.append(_truth_pobs(A, pobs, pi))
    den = orc.pobs_gaussian(obs[0][1200:1201], mu, sig)
    assert 0.0 < den.max() < 2.3e-308       # (the row IS denormal)
    eng = _engine()
    eng.set_observations("gaussian", obs, n, chunk=chunk)
    results = _run_forms(eng, model, n, rng, 1)
    eng.close()
    _check_forms(truth, results, "outliers chunk=%d" % chunk)


@pytest.mark.parametrize("z", [150, 2500])
@pytest.mark.parametrize("chunk", [0, 64])
def test_zero_probability_from_a_known_step(chunk, z):
    rng = np.random.default_rng(4)
    n, M = 3, 4
    obs = [rng.integers(0, 3, T).astype(np.int32) for T in (5000, 3000, 4000)]
    obs[1][z] = 3                         # symbol 3 appears in trajectory 1 only, at step z
    A = np.array([[0.7, 0.3, 0.0], [0.4, 0.5, 0.1], [0.0, 0.3, 0.7]])
    B = np.array([[0.0, 0.5, 0.5, 0.0], [0.3, 0.2, 0.5, 0.0], [0.6, 0.0, 0.4, 0.0]])   # no state emits symbol 3
    pi = np.array([0.5, 0.5, 0.0])
    model = (A, pi, B, None)
    V = _weights(n, 2, (A, pi, np.arange(3.0), None), rng)
    # trajectory 1: the ordinary rows before step z
    cut = [obs[0], obs[1][:z], obs[2]]
    truth = _truth("discrete", cut, model)
    eng = _engine()
    eng.set_observations("discrete", obs, n, nsymbols=M, chunk=chunk)
    for dtype in (np.float64, np.float32):
        for weights in (None, V):
            rows, logc = eng.filter_states(*model, weights=weights, dtype=dtype)
            assert eng.get_option("filter_path") == 1
            label = "zero at %d chunk=%d %s%s" % (z, chunk, np.dtype(dtype).name, "" if weights is None else " Q=2")
            assert not any(np.any(np.isnan(r)) for r in rows) and not any(np.any(np.isnan(l)) for l in logc)
            _check_rows(truth, [rows[0], rows[1][:z], rows[2]], dtype, weights, label)
            _check_logc(truth, [logc[0], logc[1][:z], logc[2]], dtype, label, dense=False)
            assert rows[1].shape[0] == 3000 and np.all(rows[1][z:] == 0.0)
            assert np.all(logc[1][z:] == -np.inf)
        rows, logc = eng.filter_states(*model, dtype=dtype, probabilities=False)
        assert np.all(logc[1][z:] == -np.inf) and np.all(np.isfinite(logc[1][:z]))
    assert eng.get_option("filter_fallbacks") == 0
    # the same on the serial path
    from bhmm_amd import hidden
    pobs = orc.pobs_discrete(obs[1], B)
    rows, logc = hidden.filter_states(A, pobs, pi)
    _check_rows(truth[1:2], [rows[:z]], np.float64, None, "zero at %d explicit" % z)
    _check_logc(truth[1:2], [logc[:z]], np.float64, "zero at %d explicit" % z, dense=False)
    assert np.all(rows[z:] == 0.0) and np.all(logc[z:] == -np.inf)
    eng.close()


@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_lagged(kind, M):
    rng = np.random.default_rng(13)
    n, lag = 6, 3
    obs = _rand_obs(kind, n, M, [9000, 1000, 37, 5], rng)
    model = _rand_model(kind, n, M, rng, stay=2.0)
    views = [(k, s) for k in range(len(obs)) for s in range(lag) if len(obs[k]) > s]
    cut = [np.ascontiguousarray(obs[k][s::lag]) for k, s in views]
    eng = _engine()
    eng.set_observations_lagged(kind, obs, lag, views, n, nsymbols=M, chunk=128)
    lagged = eng.filter_states(*model)
    assert eng.get_option("filter_path") == 1
    eng.set_observations(kind, cut, n, nsymbols=M, chunk=128)
    plain = eng.filter_states(*model)
    eng.close()
    assert len(lagged[0]) == len(plain[0]) == len(views)
    for a, b in zip(lagged[0] + lagged[1], plain[0] + plain[1]):
        assert np.array_equal(a, b)
    truth = _truth(kind, cut, model)
    _check_rows(truth, lagged[0], np.float64, None, "lagged %s" % kind)
    _check_logc(truth, lagged[1], np.float64, "lagged %s" % kind)


@pytest.mark.parametrize("kind,M,n", [("gaussian", 0, 3), ("discrete", 16, 8), ("gaussian", 0, 12)])
def test_single_step(kind, M, n):
    rng = np.random.default_rng(2 + n)
    obs = _rand_obs(kind, n, M, [1], rng)
    model = _rand_model(kind, n, M, rng)
    truth = _truth(kind, obs, model)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    results = _run_forms(eng, model, n, rng, 1 if n <= 8 else 0)
    eng.close()
    _check_forms(truth, results, "T=1 %s n=%d" % (kind, n))


# ---- 7. no side effects ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_no_side_effects(kind, M):
    rng = np.random.default_rng(9)
    n = 8
    obs = _rand_obs(kind, n, M, [30000, 7000, 1, 12345], rng)
    m1 = _rand_model(kind, n, M, rng, stay=2.0)
    m2 = _rand_model(kind, n, M, rng, stay=5.0)
    other = _rand_model(kind, n, M, rng, stay=1.0)
    V = _weights(n, 2, other, rng)
    opts = ("post_W", "post_ws_mb", "post_fallbacks", "post_path", "marg_W", "marg_ws_mb", "marg_fallbacks",
            "marg_path", "score_fallbacks", "score_path")

    def sequence(filtering):
        eng = _engine()
        eng.set_observations(kind, obs, n, nsymbols=M, chunk=256)
        eng.posterior_decode(*m1)                                   # (so that the counters say something)
        out = []
        for m in (m1, m2, m1):          # (carried boundaries, warm-up state: a sequence of E-steps)
            if filtering:
                eng.filter_states(*other)
            r = eng.estep(*m, store_gamma=True)
            out += [r.packed.copy(), r.logL_k.copy()]
            if filtering:
                eng.filter_states(*other, weights=V, dtype=np.float32)
            out += [eng.gamma(k) for k in range(len(obs))]          # the stored gamma of THAT E-step
            if filtering:
                eng.filter_states(*m, probabilities=False)
            out.append(_cat(eng.viterbi(*m)))
            out.append(eng.score([m1, m2]))
            if filtering:
                eng.filter_states(*m)
            out.append(_cat(eng.posterior_decode(*m)))
            out.append(_cat(eng.posterior_marginals(*m)))
            out.append(np.array([eng.get_option(o) for o in opts]))
        assert not filtering or eng.get_option("filter_path") == 1
        eng.close()
        return out

    plain, mixed = sequence(False), sequence(True)
    assert len(plain) == len(mixed)
    for a, b in zip(plain, mixed):
        assert np.array_equal(a, b)


# ---- 8. estimator and module function ---------------------------------------------------------------
def test_estimator_and_module_function():
    import bhmm_amd
    rng = np.random.default_rng(21)
    n = 3
    A, pi, mu, sig = _rand_model("gaussian", n, 0, rng, stay=4.0)
    hmm = bhmm_amd.gaussian_hmm(pi, A, mu, sig)
    obs = _rand_obs("gaussian", n, 0, [4000, 300, 2], rng)
    est = bhmm_amd.MaximumLikelihoodEstimator(obs, n, initial_model=hmm, output="gaussian", maxit=4, accuracy=1e-12)
    est.fit()
    Ae, pie, m0, s0 = est._estep_model
    assert not np.array_equal(Ae, est.hmm.transition_matrix)
    truth = _truth("gaussian", obs, (Ae, pie, m0, s0))
    rows, logc = est.filter_states()
    _check_rows(truth, rows, np.float64, None, "estimator")
    _check_logc(truth, logc, np.float64, "estimator")
    V = np.column_stack([np.array([1.0, 0.0, 0.0]), m0])
    proj, none = est.filter_states(weights=V, dtype=np.float32, increments=False)
    assert none is None
    _check_rows(truth, proj, np.float32, V, "estimator Q=2 float32")
    # the module function, under the same parameters
    last = bhmm_amd.gaussian_hmm(pie, Ae, m0, s0)
    rows, logc = bhmm_amd.filter_states(obs, last)
    _check_rows(truth, rows, np.float64, None, "module")
    _check_logc(truth, logc, np.float64, "module")
    none, l32 = bhmm_amd.filter_states(obs, last, dtype=np.float32, probabilities=False)
    assert none is None
    _check_logc(truth, l32, np.float32, "module float32 logc alone")
    cut = bhmm_amd.lag_observations(obs, 2)
    rows, logc = bhmm_amd.filter_states(obs, last, lag=2)
    assert len(rows) == len(cut)
    tl = _truth("gaussian", cut, (Ae, pie, m0, s0))
    _check_rows(tl, rows, np.float64, None, "module lag 2")
    _check_logc(tl, logc, np.float64, "module lag 2")
