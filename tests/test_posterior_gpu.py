"""GPU: bhmm_posterior_decode / Engine.posterior_decode / bhmm_amd.posterior_decode -- argmax_i gamma_t(i) and
max_i gamma_t(i) of every step against the CPU oracle's gamma, on the fused path (up to 8 states) and the generic
one (E-step + gamma rows), the fallback protocol, bitwise invariances and the absence of side effects.

Comparison rule (all parity tests): a step is left out of the PATH comparison only when the oracle's gap
between its two largest gamma is <= 1e-9 (the E-step's stated parity is 1e-11), at most 1e-4 of a case's
steps may be left out, every other step must match exactly; the confidence must be within 1e-7 on ALL steps
(fp32 rounding of a value <= 1, about 3e-8, plus the parity)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

GAP = 1e-9
CONF_TOL = 1e-7
MAX_LEFT_OUT = 1e-4


def _engine():
    from bhmm_amd.engine import Engine
    return Engine(0)


# models and data as tests/test_score_gpu.py (_rand_model / _rand_obs)
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


def _check(gammas, paths, conf=None, label=""):
    """The comparison rule of the module docstring; returns (steps, left out)."""
    steps = left = 0
    worst = 0.0
    for k, g in enumerate(gammas):
        T, n = g.shape
        assert paths[k].shape == (T,)
        if T == 0:
            continue
        if n > 1:
            top = np.sort(g, axis=1)[:, -2:]
            close = (top[:, 1] - top[:, 0]) <= GAP
        else:
            close = np.zeros(T, dtype=bool)
        want = g.argmax(axis=1)
        got = np.asarray(paths[k]).astype(np.int64)
        assert got.min() >= 0 and got.max() < n
        bad = np.nonzero((got != want) & ~close)[0]
        assert bad.size == 0, "%s trajectory %d: %d steps differ, first at %d (gamma %r)" % (
            label, k, bad.size, bad[0], g[bad[0]])
        steps += T
        left += int(close.sum())
        if conf is not None:
            assert conf[k].dtype == np.float32 and conf[k].shape == (T,)
            worst = max(worst, float(np.abs(conf[k].astype(np.float64) - g.max(axis=1)).max()))
    print("%s: %d steps, %d left out, worst |conf - oracle| %.3g" % (label, steps, left, worst))
    assert left <= MAX_LEFT_OUT * steps
    if conf is not None:
        assert worst <= CONF_TOL
    return steps, left


LENGTHS = [1, 2, 37, 500, 3001, 64, 129, 20000]


# ---- 1. oracle parity, fused path -----------------------------------------------------------------
@pytest.mark.parametrize("stay", [0, 20])
@pytest.mark.parametrize("chunk", [0, 64, 100000])
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 3), ("discrete", 64), ("discrete", 1000)])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_parity_fused(n, kind, M, chunk, stay):
    rng = np.random.default_rng(1000 * n + M + chunk % 7 + stay)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=float(stay))
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=chunk)
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("post_path") == 1
    fallbacks = eng.get_option("post_fallbacks")
    eng.close()
    assert all(p.dtype == np.uint8 for p in paths)
    _check(_oracle_gammas(kind, obs, model), paths, conf, "fused n=%d %s M=%d chunk=%d stay=%d" % (n, kind, M, chunk, stay))
    if stay == 0:
        assert fallbacks == 0


# ---- 2. the same parity on the generic path --------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [12, 40, 100])
def test_parity_generic(n, kind, M):
    rng = np.random.default_rng(7 * n + M)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("post_path") == 0
    only = eng.posterior_decode(*model)
    eng.close()
    _check(_oracle_gammas(kind, obs, model), paths, conf, "generic n=%d %s" % (n, kind))
    assert all(np.array_equal(a, b) for a, b in zip(paths, only))


@pytest.mark.parametrize("n", [3, 8, 12])
def test_parity_explicit_pobs(n):
    import bhmm_amd
    rng = np.random.default_rng(50 + n)
    A, pi, mu, sig = _rand_model("gaussian", n, 0, rng)
    o = rng.normal(0, 3, 5000)
    pobs = orc.pobs_gaussian(o, mu, sig)
    path, conf = bhmm_amd.hidden.posterior_decode(A, pobs, pi, confidence=True)
    alpha = orc.forward(A, pobs, pi)[1]
    g = orc.gamma(alpha, orc.backward(A, pobs))
    _check([g], [path], [conf], "explicit n=%d" % n)
    assert np.array_equal(bhmm_amd.hidden.posterior_decode(A, pobs, pi), path)
    eng = _engine()
    eng.set_observations("explicit", [pobs], n)
    eng.posterior_decode(A, pi)
    assert eng.get_option("post_path") == 0
    eng.close()


# ---- 3. forced protocol ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_forced_fallback(kind, M):
    rng = np.random.default_rng(31)
    n = 8
    lengths = [60000, 40000, 12345]
    obs = _rand_obs(kind, n, M, lengths, rng)
    model = _rand_model(kind, n, M, rng, stay=200.0)     # slowly mixing
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=512)
    eng.set_option("post_W", 2)                          # far too short: the check must fail
    before = eng.get_option("post_fallbacks")
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("post_fallbacks") > before
    assert eng.get_option("post_path") == 1              # (the FIRST pass was the fused one)
    eng.close()
    _check(_oracle_gammas(kind, obs, model), paths, conf, "forced %s" % kind)


# ---- 4. invariance, all bitwise --------------------------------------------------------------------
def _cat(xs):
    return np.concatenate([np.asarray(x) for x in xs])


@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_invariance(kind, M):
    rng = np.random.default_rng(5)
    n = 8
    obs = _rand_obs(kind, n, M, [20000, 7000, 1, 12345, 64, 3001], rng)
    model = _rand_model(kind, n, M, rng, stay=3.0)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=256)
    p0, c0 = eng.posterior_decode(*model, confidence=True)
    p0, c0 = _cat(p0), _cat(c0)
    # repeated calls
    p1, c1 = eng.posterior_decode(*model, confidence=True)
    assert np.array_equal(_cat(p1), p0) and np.array_equal(_cat(c1), c0)
    # confidence off: the same path
    assert np.array_equal(_cat(eng.posterior_decode(*model)), p0)
    # a caller's buffer
    out = np.empty(p0.size, dtype=np.uint8)
    views = eng.posterior_decode(*model, out=out)
    assert np.array_equal(out, p0) and views[0].base is out
    # a workspace budget that forces several ranges of chunk groups
    groups = (eng.num_chunks + 63) // 64
    assert groups >= 3
    eng.set_option("post_ws_mb", 1)      # 256 steps * 8 states * 64 lanes * 8 B = 1 MiB: one group per range
    p2, c2 = eng.posterior_decode(*model, confidence=True)
    assert np.array_equal(_cat(p2), p0) and np.array_equal(_cat(c2), c0)
    eng.set_option("post_ws_mb", 0)      # unbounded
    p3, c3 = eng.posterior_decode(*model, confidence=True)
    assert np.array_equal(_cat(p3), p0) and np.array_equal(_cat(c3), c0)
    # int32 through the C ABI
    A, pi, e0, e1 = eng._model_ptrs(*model)
    p32 = np.empty(p0.size, dtype=np.int32)
    c32 = np.empty(p0.size, dtype=np.float32)
    from bhmm_amd import _lib
    _lib.check(eng._L.bhmm_posterior_decode(eng._h, A, pi, e0, e1, ctypes.c_void_p(p32.ctypes.data), 0,
                                            ctypes.c_void_p(c32.ctypes.data)))
    assert np.array_equal(p32, p0.astype(np.int32)) and np.array_equal(c32, c0)
    assert eng.get_option("post_path") == 1
    eng.close()


@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_no_side_effects(kind, M):
    rng = np.random.default_rng(9)
    n = 8
    obs = _rand_obs(kind, n, M, [30000, 7000, 1, 12345], rng)
    m1 = _rand_model(kind, n, M, rng, stay=2.0)
    m2 = _rand_model(kind, n, M, rng, stay=5.0)
    other = _rand_model(kind, n, M, rng, stay=1.0)

    def sequence(decode):
        eng = _engine()
        eng.set_observations(kind, obs, n, nsymbols=M, chunk=256)
        out = []
        for m in (m1, m2, m1):          # (carried boundaries, warm-up state: a sequence of E-steps)
            if decode:
                eng.posterior_decode(*other, confidence=True)
            r = eng.estep(*m)
            out += [r.packed.copy(), r.logL_k.copy()]
            if decode:
                eng.posterior_decode(*m)
            out.append(_cat(eng.viterbi(*m)))
            if decode:
                eng.posterior_decode(*other)
            out.append(eng.score([m1, m2]))
        assert not decode or eng.get_option("post_path") == 1
        eng.close()
        return out

    plain, mixed = sequence(False), sequence(True)
    assert len(plain) == len(mixed)
    for a, b in zip(plain, mixed):
        assert np.array_equal(a, b)


def test_u8_needs_at_most_256_states():
    from bhmm_amd import _lib
    n = 300
    rng = np.random.default_rng(3)
    A, pi, mu, sig = _rand_model("gaussian", n, 0, rng)
    obs = [rng.normal(0, 3, 50)]
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    Ap, pip, e0, e1 = eng._model_ptrs(A, pi, mu, sig)
    buf = np.empty(50, dtype=np.uint8)
    with pytest.raises(ValueError):
        _lib.check(eng._L.bhmm_posterior_decode(eng._h, Ap, pip, e0, e1, ctypes.c_void_p(buf.ctypes.data), 1, None))
    paths = eng.posterior_decode(A, pi, mu, sig)
    assert paths[0].dtype == np.int32
    _check(_oracle_gammas("gaussian", obs, (A, pi, mu, sig)), paths, None, "n=300")
    # an invalid model is refused as by bhmm_score
    bad = A.copy()
    bad[0, 0] += 0.5
    with pytest.raises(ValueError):
        eng.posterior_decode(bad, pi, mu, sig)
    eng.close()


# ---- 5. exact ties -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 16)])
@pytest.mark.parametrize("n,twin", [(2, (0, 1)), (5, (1, 3)), (8, (2, 7))])
def test_exact_ties(n, twin, kind, M):
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
        # the pair where most of the data lie, so that it often holds the maximum
        model = (A, pi, mu, sig)
        obs = [rng.normal(mu[lo], 2.0, T) for T in (5000, 777, 1)]
    else:
        B = rng.random((n, M)) + 0.01
        B[lo, : M // 2] += 1.0
        B /= B.sum(axis=1)[:, None]
        B[hi] = B[lo]
        model = (A, pi, B, None)
        obs = [rng.integers(0, M, T).astype(np.int32) for T in (5000, 777, 1)]
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=64)
    paths = eng.posterior_decode(*model)
    assert eng.get_option("post_path") == 1
    eng.close()
    gam = _oracle_gammas(kind, obs, model)
    hits = 0
    for p, g in zip(paths, gam):
        assert not np.any(p == hi)                       # never the higher index of the pair
        pair_max = np.isclose(g[:, lo], g.max(axis=1), rtol=0, atol=1e-12)
        others = np.delete(g, [lo, hi], axis=1)
        clear = pair_max & ((others.max(axis=1) if others.size else np.zeros(len(g))) < g[:, lo] - GAP)
        assert np.all(p[clear] == lo)
        hits += int(clear.sum())
    assert hits > 100


# ---- 6. lagged observations ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_lagged(kind, M):
    rng = np.random.default_rng(13)
    n, lag = 6, 3
    obs = _rand_obs(kind, n, M, [9000, 1000, 37, 5], rng)
    model = _rand_model(kind, n, M, rng, stay=2.0)
    views = [(k, s) for k in range(len(obs)) for s in range(lag) if len(obs[k]) > s]
    eng = _engine()
    eng.set_observations_lagged(kind, obs, lag, views, n, nsymbols=M, chunk=128)
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("post_path") == 1
    eng.close()
    cut = [np.ascontiguousarray(obs[k][s::lag]) for k, s in views]
    _check(_oracle_gammas(kind, cut, model), paths, conf, "lagged %s" % kind)


def test_module_function_and_estimator():
    import bhmm_amd
    rng = np.random.default_rng(21)
    n = 3
    A, pi, mu, sig = _rand_model("gaussian", n, 0, rng, stay=4.0)
    hmm = bhmm_amd.gaussian_hmm(pi, A, mu, sig)
    obs = _rand_obs("gaussian", n, 0, [4000, 300, 2], rng)
    paths, conf = bhmm_amd.posterior_decode(obs, hmm, confidence=True)
    _check(_oracle_gammas("gaussian", obs, (A, pi, mu, sig)), paths, conf, "module")
    lagged = bhmm_amd.posterior_decode(obs, hmm, lag=2)
    cut = bhmm_amd.lag_observations(obs, 2)
    assert len(lagged) == len(cut)
    _check(_oracle_gammas("gaussian", cut, (A, pi, mu, sig)), lagged, None, "module lag 2")
    est = bhmm_amd.MaximumLikelihoodEstimator(obs, n, initial_model=hmm, output="gaussian", maxit=3)
    est.fit()
    m = est.hmm
    par0, par1 = m.output_model.parameters()
    ep, ec = est.posterior_decode(confidence=True)
    _check(_oracle_gammas("gaussian", obs, (m.transition_matrix, m.initial_distribution, par0, par1)), ep, ec,
           "estimator")
    assert all(np.array_equal(a, b) for a, b in zip(est.posterior_decode(), ep))


# ---- 7. full size, configs[1] --------------------------------------------------------------------------
def test_full_size_configs1():
    rng = np.random.default_rng(2)
    n, K, T = 8, 256, 100000
    model = _rand_model("gaussian", n, 0, rng, stay=3.0)
    obs = [rng.normal(0, 3, T) for _ in range(K)]
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    paths, conf = eng.posterior_decode(*model, confidence=True)
    assert eng.get_option("post_path") == 1
    eng.close()
    assert len(paths) == K
    for p in paths:
        assert p.shape == (T,) and p.max() < n
    sel = [0, 85, 170, K - 1]
    _check(_oracle_gammas("gaussian", [obs[k] for k in sel], model), [paths[k] for k in sel],
           [conf[k] for k in sel], "configs[1]")
