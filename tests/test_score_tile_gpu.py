"""GPU: bhmm_score for 65 to 128 states on the matrix-core kernel (k_score_tile) --
against the CPU oracle's forward pass, the E-step, and itself (batch invariance, forced fallback, zero
probability and the range flag, no side effects on the E-step / Viterbi / sampling state, other observation
sources, the neighbouring paths).  The helpers are those of test_score_wide_gpu.py, restated."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

RTOL = 1e-11


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


def _oracle(kind, obs, model):
    A, pi, p0, p1 = model
    out = []
    for o in obs:
        pobs = orc.pobs_gaussian(o, p0, p1) if kind == "gaussian" else orc.pobs_discrete(o, p0)
        out.append(orc.forward(A, pobs, pi)[0])
    return np.array(out)


def _check_oracle(kind, obs, models, logL):
    assert logL.shape == (len(models), len(obs))
    for s, m in enumerate(models):
        ref = _oracle(kind, obs, m)
        print("model", s, "max rel", np.max(np.abs(logL[s] / ref - 1)))
        np.testing.assert_allclose(logL[s], ref, rtol=RTOL)


LENGTHS = [1, 2, 37, 500, 3001, 64, 129, 20000]
PARITY = [(n, "gaussian", 0) for n in (65, 80, 81, 96, 100, 112, 113, 128)] + \
         [(n, "discrete", M) for n in (65, 100, 128) for M in (3, 64, 1000)]


# ---- 1. oracle parity ------------------------------------------------------------------------------
@pytest.mark.parametrize("seglen", [0, 256, 100000])
@pytest.mark.parametrize("n,kind,M", PARITY)
def test_oracle_parity(n, kind, M, seglen):
    rng = np.random.default_rng(100 * n + M + seglen % 7)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    models = [_rand_model(kind, n, M, rng) for _ in range(3)]
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    eng.set_option("score_seglen", seglen)
    assert eng.get_option("score_seglen") == seglen
    logL = eng.score(models)
    assert eng.get_option("score_path") == 3
    print("segments", eng.get_option("score_segments"), "W_max", eng.get_option("score_W_max"), "fallbacks",
          eng.get_option("score_fallbacks"))
    _check_oracle(kind, obs, models, logL)
    assert np.all(np.isfinite(logL))
    if seglen == 256:
        # quickly mixing models: the segmented kernel itself verified
        assert eng.get_option("score_segments") > len(obs)
        assert eng.get_option("score_fallbacks") == 0
        assert eng.get_option("score_W_max") >= 32 and eng.get_option("score_W_max") % 4 == 0
    if seglen == 100000:
        assert eng.get_option("score_segments") == len(obs)   # one segment per trajectory: the exact recursion
        assert eng.get_option("score_W_max") == 0
    eng.close()


# ---- 2. batch invariance ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_batch_invariance(kind, M):
    n = 100
    rng = np.random.default_rng(7 + n)
    obs = _rand_obs(kind, n, M, [20000, 7000, 1, 12345], rng)
    models = [_rand_model(kind, n, M, rng, stay=3.0 * s / 7) for s in range(8)]
    other = _rand_model(kind, n, M, rng, stay=1.0)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    eng.set_option("score_seglen", 1024)
    batch = eng.score(models)
    assert eng.get_option("score_path") == 3
    assert eng.get_option("score_segments") > len(obs)
    singles = np.stack([eng.score([m])[0] for m in models])
    assert np.array_equal(batch, singles)
    perm = rng.permutation(8)
    assert np.array_equal(eng.score([models[i] for i in perm]), batch[perm])
    assert np.array_equal(eng.score(models), batch)
    for _ in range(3):
        eng.estep(*other)
    assert np.array_equal(eng.score(models), batch)
    _check_oracle(kind, obs, models, batch)
    eng.close()


# ---- 3. forced fallback ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [65, 128])
def test_forced_fallback(n, kind, M):
    rng = np.random.default_rng(9 + n)
    obs = _rand_obs(kind, n, M, [20000, 5000, 17], rng)
    models = [_rand_model(kind, n, M, rng, stay=4.0) for _ in range(3)]   # second eigenvalue about 0.8
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    eng.set_option("score_seglen", 256)
    ref = eng.score(models)
    before = eng.get_option("score_fallbacks")
    print("unforced: W_max", eng.get_option("score_W_max"), "fallbacks", before)
    eng.set_option("score_W", 4)
    forced = eng.score(models)
    assert eng.get_option("score_path") == 3
    assert eng.get_option("score_fallbacks") > before   # four steps cannot forget at a second eigenvalue of 0.8
    _check_oracle(kind, obs, models, forced)
    _check_oracle(kind, obs, models, ref)
    np.testing.assert_allclose(forced, ref, rtol=RTOL)
    eng.close()


# ---- 4. zero probability and the range flag --------------------------------------------------------
@pytest.mark.parametrize("n", [65, 128])
def test_zero_probability_is_minus_inf(n):
    rng = np.random.default_rng(4 + n)
    M = 6
    obs = [rng.integers(0, 5, T).astype(np.int32) for T in (5000, 3000, 4000)]
    obs[1][1500] = 5                      # symbol 5 appears in trajectory 1 only
    good = _rand_model("discrete", n, M, rng)
    B = good[2].copy()
    B[:, 5] = 0.0                         # ... and no state of this model emits it
    B /= B.sum(axis=1)[:, None]
    bad = (good[0], good[1], B, None)
    # reachability: state n-1 is never entered from pi = e0 under A, and only state n-1 emits symbol 0
    A = _rand_A(n, rng)
    A[:n - 1, n - 1] = 0.0
    A /= A.sum(axis=1)[:, None]
    B2 = rng.random((n, M)) + 0.01
    B2[:n - 1, 0] = 0.0
    B2[n - 1] = 0.0
    B2[n - 1, 0] = 1.0
    B2 /= B2.sum(axis=1)[:, None]
    pi0 = np.zeros(n)
    pi0[0] = 1.0
    unreach = (A, pi0, B2, None)
    for seglen in (0, 256):
        eng = _engine()
        eng.set_observations("discrete", obs, n, nsymbols=M)
        eng.set_option("score_seglen", seglen)
        alone = eng.score([good])
        logL = eng.score([good, bad, unreach])
        assert eng.get_option("score_path") == 3
        if seglen:
            assert eng.get_option("score_segments") > len(obs)
        assert not np.any(np.isnan(logL))
        assert np.array_equal(logL[0], alone[0])    # the good model: bit for bit what it scores alone
        _check_oracle("discrete", obs, [good], logL[:1])
        assert logL[1, 1] == -np.inf
        np.testing.assert_allclose(logL[1, [0, 2]], _oracle("discrete", [obs[0], obs[2]], bad), rtol=RTOL)
        assert np.all(logL[2] == -np.inf)
        eng.close()


# ---- 5. no side effects ----------------------------------------------------------------------------
STATE = ("spec_W", "wide_segments", "wide_segment_len", "wide_fwd_segments", "tile", "tile_reason", "spec_ok",
         "spec_fail", "careful", "viterbi_segments", "viterbi_W", "sample_segments", "sample_W")


@pytest.mark.parametrize("n,kind,M", [(100, "gaussian", 0), (80, "discrete", 12), (128, "gaussian", 0)])
def test_no_side_effects_paths(n, kind, M):
    rng = np.random.default_rng(12 + n + M)
    obs = _rand_obs(kind, n, M, [30000, 20000, 99], rng)
    m = _rand_model(kind, n, M, rng, stay=3.0)
    others = [_rand_model(kind, n, M, rng) for _ in range(3)]
    res = []
    for with_score in (False, True):
        eng = _engine()
        eng.set_observations(kind, obs, n, nsymbols=M)
        eng.set_option("score_seglen", 1024)
        state = []
        r0 = eng.estep(*m)
        state.append([eng.get_option(o) for o in STATE])
        if with_score:
            eng.score(others)
            assert eng.get_option("score_path") == 3 and eng.get_option("score_segments") > len(obs)
        v = eng.viterbi(*m)
        state.append([eng.get_option(o) for o in STATE])
        if with_score:
            eng.score(others)
        p, C, n0, emis = eng.sample_paths(*m, seed=3)
        state.append([eng.get_option(o) for o in STATE])
        if with_score:
            eng.score(others)
        r = eng.estep(*m)
        state.append([eng.get_option(o) for o in STATE])
        res.append((v, p, C, n0, emis, r0.packed.copy(), r.packed.copy(), r.logL_k.copy(), state))
        eng.close()
    a, b = res
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert np.array_equal(x, y)
    for x, y in zip(a[2:4] + a[5:8], b[2:4] + b[5:8]):
        assert np.array_equal(x, y)
    if kind == "discrete":
        assert np.array_equal(a[4], b[4])   # the sampler's symbol counts: integer-valued sums, exact in any order
    else:
        # gaussian emission sums: the counts bit for bit; sum d and sum d^2 are floating-point atomic sums over the
        # (bit-identical) paths, whose last bits differ between two runs of the same sequence WITHOUT any score call
        assert np.array_equal(a[4][0], b[4][0])
        np.testing.assert_allclose(a[4], b[4], rtol=1e-12)
    assert a[8] == b[8]


# ---- 6. other observation sources ------------------------------------------------------------------
def test_lagged_and_device_observations():
    import torch
    from bhmm_amd.api import lag_observations
    rng = np.random.default_rng(21)
    n, M = 96, 7
    base = _rand_obs("discrete", n, M, [9000, 4000], rng)
    models = [_rand_model("discrete", n, M, rng, stay=2.0) for _ in range(3)]
    lagged = lag_observations(base, 3)
    host = _engine()
    host.set_observations("discrete", [np.ascontiguousarray(o) for o in lagged], n, nsymbols=M)
    host.set_option("score_seglen", 512)
    ref = host.score(models)
    assert host.get_option("score_path") == 3 and host.get_option("score_segments") > len(lagged)
    host.close()
    eng = _engine()
    eng.set_observations_lagged("discrete", lagged.base, lagged.lag, lagged.views, n, nsymbols=M)
    eng.set_option("score_seglen", 512)
    assert np.array_equal(eng.score(models), ref)
    eng.close()
    flat = np.concatenate(base).astype(np.int32)
    t = torch.from_numpy(flat).to("cuda:0")
    off = np.array([0, len(base[0]), len(flat)], dtype=np.int64)
    h2 = _engine()
    h2.set_observations("discrete", base, n, nsymbols=M)
    h2.set_option("score_seglen", 512)
    ref2 = h2.score(models)
    h2.close()
    dev = _engine()
    dev.set_observations_device("discrete", t.data_ptr(), off, n, nsymbols=M)
    dev.set_option("score_seglen", 512)
    assert np.array_equal(dev.score(models), ref2)
    dev.close()
    _check_oracle("discrete", base, models, ref2)


# ---- 7. borders: the neighbouring paths keep theirs -------------------------------------------------
def test_borders():
    rng = np.random.default_rng(77)
    lengths = [700, 1, 2500]
    # 129 states: the exact serial recursion
    n = 129
    obs = _rand_obs("gaussian", n, 0, lengths, rng)
    models = [_rand_model("gaussian", n, 0, rng) for _ in range(2)]
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    logL = eng.score(models)
    assert eng.get_option("score_path") == 0 and eng.get_option("score_segments") == 0
    _check_oracle("gaussian", obs, models, logL)
    eng.close()
    # explicit pobs at 100 states: the same
    n = 100
    pobs = [rng.random((300, n)) + 0.01, rng.random((40, n))]
    A = _rand_A(n, rng)
    pi = np.full(n, 1.0 / n)
    eng = _engine()
    eng.set_observations("explicit", pobs, n)
    logL = eng.score([(A, pi, None, None)])
    assert eng.get_option("score_path") == 0
    np.testing.assert_allclose(logL[0], [orc.forward(A, p, pi)[0] for p in pobs], rtol=RTOL)
    eng.close()
    # 64 states: k_score_wide
    n = 64
    obs = _rand_obs("gaussian", n, 0, lengths, rng)
    models = [_rand_model("gaussian", n, 0, rng) for _ in range(2)]
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    logL = eng.score(models)
    assert eng.get_option("score_path") == 2
    _check_oracle("gaussian", obs, models, logL)
    eng.close()


# ---- 8. full size: bench.py's 128-state secondary configuration --------------------------------------
def test_full_size():
    import torch
    from bench import metastable_matrix, stationary
    n, K, T = 128, 128, 10000
    rng = np.random.default_rng(n)
    A = metastable_matrix(n, rng)
    pi = stationary(A)
    mu, sig = np.linspace(-5, 5, n), np.linspace(0.5, 2.0, n)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(n)
    obs = torch.randn(K * T, dtype=torch.float64, device="cuda:0", generator=g) * 3.0
    eng = _engine()
    eng.set_observations_device("gaussian", obs.data_ptr(), np.arange(K + 1, dtype=np.int64) * T, n)
    models = [(0.9 * A + 0.1 / n, pi, mu + 0.05, sig)]
    for i in range(3):
        w = 0.85 + 0.04 * i
        models.append((w * A + (1 - w) / n, pi, mu + 0.02 * (i + 1), sig))
    logL = eng.score(models)
    assert eng.get_option("score_path") == 3
    assert eng.get_option("score_segments") > K
    print("segments", eng.get_option("score_segments"), "W_max", eng.get_option("score_W_max"))
    assert eng.get_option("score_fallbacks") == 0
    for s, m in enumerate(models):
        res = eng.estep(*m)
        print("model", s, "score", logL[s].sum(), "estep", res.loglik, "max rel per trajectory",
              np.max(np.abs(logL[s] / res.logL_k - 1)))
        np.testing.assert_allclose(logL[s], res.logL_k, rtol=RTOL)
    two = [obs[k * T:(k + 1) * T].cpu().numpy() for k in (0, K - 1)]
    for s, m in enumerate(models):
        np.testing.assert_allclose(logL[s][[0, K - 1]], _oracle("gaussian", two, m), rtol=RTOL)
    eng.close()
