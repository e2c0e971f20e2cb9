"""GPU: bhmm_posterior_marginals / Engine.posterior_marginals / bhmm_amd.posterior_marginals -- gamma_t(i) of every
step, in double or float, plain or projected on a few columns, against the CPU oracle's gamma
(oracle.estep(..., want_gamma=True)): the fused path (up to 8 states), the generic one (E-step + gamma rows), the
fallback protocol, bitwise invariances, consistency with posterior_decode and the absence of side effects.

Tolerances (the project's own): fp64 rows rtol 1e-8, atol 1e-13 -- the rule tests/test_estep_gpu.py applies to
Engine.gamma; fp32 rows 1e-7 absolute -- the CONF_TOL of tests/test_posterior_gpu.py (fp32 rounding of a value
<= 1, about 3e-8, plus the parity); projections the same two bounds scaled by sum_i |V[i][q]| per column, against
g @ V computed in fp64.  Scaled means: a row within atol + rtol * g_i per entry gives a projection within
sum_i |V[i][q]| (atol + rtol * g_i) = atol * sum_i |V[i][q]| + rtol * (g @ |V|)[q] -- the row rule carried through
the sum, entry by entry (no more than (atol + rtol) * sum_i |V[i][q]|, its coarsest form); fp32: 1e-7 * sum_i
|V[i][q]|."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

RTOL64, ATOL64 = 1e-8, 1e-13
TOL32 = 1e-7
GAP = 1e-9          # tests/test_posterior_gpu.py
CONF_TOL = 1e-7     # tests/test_posterior_gpu.py
LENGTHS = [1, 2, 37, 500, 3001, 64, 129, 20000]


def _engine():
    from bhmm_amd.engine import Engine
    return Engine(0)


def _rand_A(n, rng, stay=0.0):
    A = rng.random((n, n)) + 0.05
    A += stay * np.eye(n) * A.sum(axis=1)[:, None]
    return A / A.sum(axis=1)[:, None]


def _rand_model(kind, n, M, rng, stay=0.0):
    A = _rand_A(n, rng, stay)
    pi = rng.random(n) + 0.1
    pi /= pi.sum()
    if kind == "gaussian":
        return (A, pi, np.sort(rng.normal(0, 3, n)), rng.uniform(0.5, 2.0, n))
    B = rng.random((n, M)) + 0.01
    return (A, pi, B / B.sum(axis=1)[:, None], None)


def _rand_obs(kind, n, M, lengths, rng):
    if kind == "gaussian":
        return [rng.normal(0, 3, T) for T in lengths]
    return [rng.integers(0, M, T).astype(np.int32) for T in lengths]


def _oracle_gammas(kind, obs, model):
    A, pi, p0, p1 = model
    return orc.estep(kind, obs, A, pi, p0, p1, want_gamma=True)["gammas"]


def _weights(n, Q, model, rng):
    """(n, Q): an indicator column first, the state means (gaussian) or state indices second, random beyond"""
    V = rng.normal(0, 2, (n, Q))
    V[:, 0] = (np.arange(n) % 2 == 0)
    if Q > 1:
        V[:, 1] = model[2] if model[3] is not None else np.arange(n, dtype=float)
    return V


def _check(gammas, rows, dtype, V=None, label=""):
    """every row against the oracle under the module's tolerances; prints the worst figures first"""
    scale = np.ones(gammas[0].shape[1]) if V is None else np.abs(V).sum(axis=0)
    worst_abs = worst_ratio = 0.0
    for g, r in zip(gammas, rows):
        want = g if V is None else g @ V
        assert r.shape == want.shape and r.dtype == dtype, (label, r.shape, want.shape, r.dtype)
        if want.size == 0:
            continue
        err = np.abs(r.astype(np.float64) - want)
        assert np.all(np.isfinite(err)), label
        worst_abs = max(worst_abs, float((err / np.where(scale > 0, scale, 1.0)).max()))
        if dtype == np.float64:
            bound = scale * ATOL64 + RTOL64 * (np.abs(g) if V is None else g @ np.abs(V))
        else:
            bound = scale * TOL32 * np.ones_like(want)
        # (an all-zero column of V has bound 0: its projection must be exactly 0)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        worst_ratio = max(worst_ratio, float(ratio.max()))
    print("%s: worst |row - oracle| / scale %.3g, worst error / bound %.3g" % (label, worst_abs, worst_ratio))
    assert worst_ratio <= 1.0, label


# ---- 1. oracle parity, fused path -----------------------------------------------------------------
@pytest.mark.parametrize("stay", [0, 20])
@pytest.mark.parametrize("chunk", [0, 64, 100000])
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 3), ("discrete", 64), ("discrete", 1000)])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_parity_fused(n, kind, M, chunk, stay):
    rng = np.random.default_rng(1000 * n + M + chunk % 7 + stay)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=float(stay))
    gam = _oracle_gammas(kind, obs, model)
    label = "fused n=%d %s M=%d chunk=%d stay=%d" % (n, kind, M, chunk, stay)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=chunk)
    results = []
    for dtype in (np.float64, np.float32):
        rows = eng.posterior_marginals(*model, dtype=dtype)
        assert eng.get_option("marg_path") == 1
        results.append((rows, dtype, None, "%s %s" % (label, np.dtype(dtype).name)))
        for Q in (1, 3, 8):
            V = _weights(n, Q, model, rng)
            rows = eng.posterior_marginals(*model, weights=V, dtype=dtype)
            assert eng.get_option("marg_path") == 1
            results.append((rows, dtype, V, "%s %s Q=%d" % (label, np.dtype(dtype).name, Q)))
    fallbacks = eng.get_option("marg_fallbacks")
    eng.close()
    for rows, dtype, V, lab in results:
        _check(gam, rows, dtype, V, lab)
    if stay == 0:
        assert fallbacks == 0


# ---- 2. the same parity on the generic path --------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [12, 40, 100])
def test_parity_generic(n, kind, M):
    rng = np.random.default_rng(7 * n + M)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng)
    gam = _oracle_gammas(kind, obs, model)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    for dtype in (np.float64, np.float32):
        rows = eng.posterior_marginals(*model, dtype=dtype)
        assert eng.get_option("marg_path") == 0
        _check(gam, rows, dtype, None, "generic n=%d %s %s" % (n, kind, np.dtype(dtype).name))
        V = _weights(n, 3, model, rng)
        rows = eng.posterior_marginals(*model, weights=V, dtype=dtype)
        _check(gam, rows, dtype, V, "generic n=%d %s %s Q=3" % (n, kind, np.dtype(dtype).name))
    eng.close()


@pytest.mark.parametrize("n", [3, 8, 12])
def test_parity_explicit_pobs(n):
    import bhmm_amd
    rng = np.random.default_rng(50 + n)
    A, pi, mu, sig = _rand_model("gaussian", n, 0, rng)
    o = rng.normal(0, 3, 5000)
    pobs = orc.pobs_gaussian(o, mu, sig)
    g = orc.gamma(orc.forward(A, pobs, pi)[1], orc.backward(A, pobs))
    V = _weights(n, 2, (A, pi, mu, sig), rng)
    for dtype in (np.float64, np.float32):
        _check([g], [bhmm_amd.hidden.posterior_marginals(A, pobs, pi, dtype=dtype)], dtype, None, "explicit n=%d" % n)
        _check([g], [bhmm_amd.hidden.posterior_marginals(A, pobs, pi, weights=V, dtype=dtype)], dtype, V,
               "explicit n=%d Q=2" % n)
    eng = _engine()
    eng.set_observations("explicit", [pobs], n)
    eng.posterior_marginals(A, pi)
    assert eng.get_option("marg_path") == 0
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
    eng.set_option("marg_W", 2)                          # far too short: the check must fail
    before = eng.get_option("marg_fallbacks")
    rows = eng.posterior_marginals(*model)
    assert eng.get_option("marg_fallbacks") > before
    assert eng.get_option("marg_path") == 1              # (the FIRST pass was the fused one)
    eng.close()
    _check(_oracle_gammas(kind, obs, model), rows, np.float64, None, "forced %s" % kind)


# ---- 4. invariance, all bitwise --------------------------------------------------------------------
def _cat(xs):
    return np.concatenate([np.asarray(x) for x in xs])


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
    r64 = _cat(eng.posterior_marginals(*model))
    p64 = _cat(eng.posterior_marginals(*model, weights=V))
    assert np.array_equal(_cat(eng.posterior_marginals(*model)), r64)            # repeated calls
    # a workspace budget that forces several ranges of chunk groups
    assert (eng.num_chunks + 63) // 64 >= 3
    eng.set_option("marg_ws_mb", 1)      # 256 steps * 8 states * 64 lanes * 8 B = 1 MiB: one group per range
    r1, p1 = _cat(eng.posterior_marginals(*model)), _cat(eng.posterior_marginals(*model, weights=V))
    eng.set_option("marg_ws_mb", 0)      # unbounded
    r0, p0 = _cat(eng.posterior_marginals(*model)), _cat(eng.posterior_marginals(*model, weights=V))
    assert np.array_equal(r1, r0) and np.array_equal(p1, p0)
    assert np.array_equal(r0, r64) and np.array_equal(p0, p64)
    # fp32 is the rounded fp64 result: the conversion is the last operation
    r32 = _cat(eng.posterior_marginals(*model, dtype=np.float32))
    p32 = _cat(eng.posterior_marginals(*model, weights=V, dtype=np.float32))
    assert r32.dtype == np.float32 and np.array_equal(r32, r64.astype(np.float32))
    assert np.array_equal(p32, p64.astype(np.float32))
    # a caller's host buffer
    out = np.empty((total, n))
    views = eng.posterior_marginals(*model, out=out)
    assert np.array_equal(out, r64) and views[0].base is not None and np.shares_memory(views[0], out)
    # device output, tensor and raw address: bitwise the host output
    for dtype, tdtype, ref in ((np.float64, torch.float64, r64), (np.float32, torch.float32, r32)):
        t = torch.full((total, n), -1.0, dtype=tdtype, device="cuda:0")
        tv = eng.posterior_marginals(*model, dtype=dtype, out=t)
        eng.sync()
        assert np.array_equal(t.cpu().numpy(), ref)
        assert tv[1].shape == (7000, n) and tv[1].data_ptr() == t[20000:].data_ptr()
        t.fill_(-1.0)
        torch.cuda.synchronize()
        assert eng.posterior_marginals(*model, dtype=dtype, out=t.data_ptr()) is None
        eng.sync()
        assert np.array_equal(t.cpu().numpy(), ref)
    tp = torch.empty((total, 3), dtype=torch.float32, device="cuda:0")
    eng.posterior_marginals(*model, weights=V, dtype=np.float32, out=tp)
    eng.sync()
    assert np.array_equal(tp.cpu().numpy(), p32)
    # pinned host tensor
    th = torch.empty((total, n), dtype=torch.float64).pin_memory()
    eng.posterior_marginals(*model, out=th)
    assert np.array_equal(th.numpy(), r64)
    assert eng.get_option("marg_path") == 1
    # the C ABI refuses what it cannot do
    from bhmm_amd import _lib
    A, pi, e0, e1 = eng._model_ptrs(*model)
    buf = np.empty((total, n))
    for Vp, Q, flags in ((None, 2, 0), (_lib.dp(V), 0, 0), (_lib.dp(np.ones((n, 9))), 9, 0), (None, 0, 4)):
        with pytest.raises(ValueError):
            _lib.check(eng._L.bhmm_posterior_marginals(eng._h, A, pi, e0, e1, Vp, Q,
                                                       ctypes.c_void_p(buf.ctypes.data), flags))
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
    lagged = eng.posterior_marginals(*model)
    assert eng.get_option("marg_path") == 1
    eng.set_observations(kind, cut, n, nsymbols=M, chunk=128)
    plain = eng.posterior_marginals(*model)
    eng.close()
    assert len(lagged) == len(plain) == len(views)
    assert all(np.array_equal(a, b) for a, b in zip(lagged, plain))
    _check(_oracle_gammas(kind, cut, model), lagged, np.float64, None, "lagged %s" % kind)


# ---- 5. consistency with the decoder -----------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [2, 5, 8])
def test_consistent_with_posterior_decode(n, kind, M):
    rng = np.random.default_rng(300 + n + M)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=2.0)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=128)
    rows = eng.posterior_marginals(*model)
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("marg_path") == 1 and eng.get_option("post_path") == 1
    eng.close()
    compared = 0
    worst = 0.0
    for g, r, p, c in zip(_oracle_gammas(kind, obs, model), rows, paths, conf):
        top = np.sort(g, axis=1)[:, -2:]
        clear = (top[:, 1] - top[:, 0]) > GAP
        assert np.array_equal(r.argmax(axis=1)[clear], p.astype(np.int64)[clear])
        compared += int(clear.sum())
        worst = max(worst, float(np.abs(r.max(axis=1) - c.astype(np.float64)).max()))
    print("n=%d %s: %d steps compared, worst |max row - conf| %.3g" % (n, kind, compared, worst))
    assert compared > 0.99 * sum(LENGTHS)
    assert worst <= CONF_TOL


@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 16)])
@pytest.mark.parametrize("n,twin", [(2, (0, 1)), (5, (1, 3)), (8, (2, 7))])
def test_identical_states_have_identical_columns(n, twin, kind, M):
    rng = np.random.default_rng(77 + n)
    lo, hi = twin
    A = rng.random((n, n)) + 0.05
    A[hi, :] = A[lo, :]                 # identical rows
    A[:, hi] = A[:, lo]                 # identical columns
    A[hi, hi] = A[lo, lo] = A[lo, hi] = A[hi, lo]
    A /= A.sum(axis=1)[:, None]
    assert np.array_equal(A[hi], A[lo]) and np.array_equal(A[:, hi], A[:, lo])
    pi = rng.random(n) + 0.1
    pi[hi] = pi[lo]
    pi /= pi.sum()
    if kind == "gaussian":
        mu, sig = rng.normal(0, 3, n), rng.uniform(0.5, 2.0, n)
        mu[hi], sig[hi] = mu[lo], sig[lo]
        model = (A, pi, mu, sig)
        obs = [rng.normal(mu[lo], 2.0, T) for T in (5000, 777, 1)]
    else:
        B = rng.random((n, M)) + 0.01
        B /= B.sum(axis=1)[:, None]
        B[hi] = B[lo]
        model = (A, pi, B, None)
        obs = [rng.integers(0, M, T).astype(np.int32) for T in (5000, 777, 1)]
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=64)
    for dtype in (np.float64, np.float32):
        rows = eng.posterior_marginals(*model, dtype=dtype)
        assert eng.get_option("marg_path") == 1
        for r in rows:
            assert np.array_equal(r[:, lo], r[:, hi])
            assert r[:, lo].max() > 0
    eng.close()


# ---- 6. no side effects ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_no_side_effects(kind, M):
    rng = np.random.default_rng(9)
    n = 8
    obs = _rand_obs(kind, n, M, [30000, 7000, 1, 12345], rng)
    m1 = _rand_model(kind, n, M, rng, stay=2.0)
    m2 = _rand_model(kind, n, M, rng, stay=5.0)
    other = _rand_model(kind, n, M, rng, stay=1.0)
    V = _weights(n, 2, other, rng)
    post_opts = ("post_W", "post_ws_mb", "post_fallbacks", "post_path")

    def sequence(marginals):
        eng = _engine()
        eng.set_observations(kind, obs, n, nsymbols=M, chunk=256)
        eng.posterior_decode(*m1)                                   # (so that the post_* counters say something)
        out = []
        for m in (m1, m2, m1):          # (carried boundaries, warm-up state: a sequence of E-steps)
            if marginals:
                eng.posterior_marginals(*other)
            r = eng.estep(*m, store_gamma=True)
            out += [r.packed.copy(), r.logL_k.copy()]
            if marginals:
                eng.posterior_marginals(*other, weights=V, dtype=np.float32)
            out += [eng.gamma(k) for k in range(len(obs))]          # the stored gamma of THAT E-step
            if marginals:
                eng.posterior_marginals(*m)
            out.append(_cat(eng.viterbi(*m)))
            out.append(eng.score([m1, m2]))
            out.append(_cat(eng.posterior_decode(*m)))
            out.append(np.array([eng.get_option(o) for o in post_opts]))
        assert not marginals or eng.get_option("marg_path") == 1
        eng.close()
        return out

    plain, mixed = sequence(False), sequence(True)
    assert len(plain) == len(mixed)
    for a, b in zip(plain, mixed):
        assert np.array_equal(a, b)


# ---- 7. estimator and module function ---------------------------------------------------------------
def test_estimator_and_module_function():
    import bhmm_amd
    rng = np.random.default_rng(21)
    n = 3
    A, pi, mu, sig = _rand_model("gaussian", n, 0, rng, stay=4.0)
    hmm = bhmm_amd.gaussian_hmm(pi, A, mu, sig)
    obs = _rand_obs("gaussian", n, 0, [4000, 300, 2], rng)
    kw = dict(initial_model=hmm, output="gaussian", maxit=4, accuracy=1e-12)
    est = bhmm_amd.MaximumLikelihoodEstimator(obs, n, **kw)
    est.fit()
    est_g = bhmm_amd.MaximumLikelihoodEstimator(obs, n, store_gamma=True, **kw)
    est_g.fit()
    got, stored = est.hidden_state_probabilities, est_g.hidden_state_probabilities
    assert len(got) == len(stored) == len(obs)
    for a, b in zip(got, stored):
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=RTOL64, atol=ATOL64)
    # the parameters of the last E-step, through the module function
    Ae, pie, m0, s0 = est._estep_model
    assert not np.array_equal(Ae, est.hmm.transition_matrix)
    last = bhmm_amd.gaussian_hmm(pie, Ae, m0, s0)
    mod = bhmm_amd.posterior_marginals(obs, last)
    for a, b in zip(mod, stored):
        np.testing.assert_allclose(a, b, rtol=RTOL64, atol=ATOL64)
    _check(_oracle_gammas("gaussian", obs, (Ae, pie, m0, s0)), got, np.float64, None, "estimator")
    V = np.column_stack([np.array([1.0, 0.0, 0.0]), m0])
    proj = est.posterior_marginals(weights=V, dtype=np.float32)
    _check(_oracle_gammas("gaussian", obs, (Ae, pie, m0, s0)), proj, np.float32, V, "estimator Q=2 float32")
    lagged = bhmm_amd.posterior_marginals(obs, last, lag=2)
    cut = bhmm_amd.lag_observations(obs, 2)
    assert len(lagged) == len(cut)
    _check(_oracle_gammas("gaussian", cut, (Ae, pie, m0, s0)), lagged, np.float64, None, "module lag 2")


# ---- 8. full size, configs[1] --------------------------------------------------------------------------
def test_full_size_configs1():
    import torch
    rng = np.random.default_rng(2)
    n, K, T = 8, 256, 100000
    model = _rand_model("gaussian", n, 0, rng, stay=3.0)
    obs = [rng.normal(0, 3, T) for _ in range(K)]
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    out = torch.empty((K * T, n), dtype=torch.float32, device="cuda:0")
    views = eng.posterior_marginals(*model, dtype=np.float32, out=out)
    eng.sync()
    assert eng.get_option("marg_path") == 1
    eng.close()
    assert len(views) == K
    sums = out.sum(dim=1, dtype=torch.float64)
    dev = float((sums - 1.0).abs().max())
    print("configs[1]: worst |row sum - 1| %.3g" % dev)
    assert dev <= 1e-6
    sel = [0, 85, K - 1]
    _check(_oracle_gammas("gaussian", [obs[k] for k in sel], model), [views[k].cpu().numpy() for k in sel],
           np.float32, None, "configs[1]")
