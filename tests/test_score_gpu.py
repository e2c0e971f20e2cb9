"""GPU: bhmm_score / Engine.score / bhmm_amd.score -- the forward-only log-likelihood of several models on
the loaded observations, against the CPU oracle's forward pass, the E-step, and itself (batch invariance,
no side effects on the E-step / Viterbi / sampling state)."""
import numpy as np
import pytest

from conftest import split
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
        np.testing.assert_allclose(logL[s], _oracle(kind, obs, m), rtol=RTOL)


LENGTHS = [1, 2, 37, 500, 3001, 64, 129]


# ---- 1. oracle parity ------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 64, 100000])
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 3), ("discrete", 64), ("discrete", 1000)])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("layout", [1, 2])
def test_oracle_parity(layout, n, kind, M, chunk):
    rng = np.random.default_rng(100 * n + M + chunk % 7)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    models = [_rand_model(kind, n, M, rng) for _ in range(3)]
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=chunk)
    eng.set_option("score_layout", layout)
    logL = eng.score(models)
    _check_oracle(kind, obs, models, logL)
    assert np.all(np.isfinite(logL))
    # quickly mixing models: the chunk-parallel kernel itself verified, nothing fell back to the serial path
    assert eng.get_option("score_fallbacks") == 0
    eng.close()


@pytest.mark.parametrize("chunk", [0, 64, 100000])
def test_goldens(golden, chunk):
    g = golden("g8_ragged")
    obs = split(g["obs"], g["lengths"])
    eng = _engine()
    eng.set_observations("gaussian", obs, 8, chunk=chunk)
    logL = eng.score([(g["A"], g["pi"], g["mu"], g["sigma"])])
    np.testing.assert_allclose(logL[0], g["logL"], rtol=RTOL)
    eng.close()
    # outliers: all-zero emission rows become rows of ones (outputmodel.py:126-130)
    g = golden("g8_outliers")
    eng = _engine()
    eng.set_observations("gaussian", [g["obs"]], 8, chunk=chunk)
    logL = eng.score([(g["A"], g["pi"], g["mu"], g["sigma"])])
    np.testing.assert_allclose(logL[0, 0], float(g["logL"]), rtol=RTOL)
    eng.close()
    # structural zeros in A, B and pi
    g = golden("d3_zeros")
    eng = _engine()
    eng.set_observations("discrete", [g["obs"]], 3, nsymbols=4, chunk=chunk)
    logL = eng.score([(g["A"], g["pi"], g["B"], None)])
    np.testing.assert_allclose(logL[0, 0], float(g["logL"]), rtol=RTOL)
    eng.close()
    g = golden("d8_ragged")
    obs = split(g["obs"], g["lengths"])
    eng = _engine()
    eng.set_observations("discrete", obs, 8, nsymbols=64, chunk=chunk)
    m = (g["A"], g["pi"], g["B"], None)
    _check_oracle("discrete", obs, [m], eng.score([m]))
    eng.close()


# ---- 2. batch invariance ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("layout", [1, 2])
def test_batch_invariance(layout, kind, M):
    rng = np.random.default_rng(7)
    n = 8
    obs = _rand_obs(kind, n, M, [20000, 7000, 1, 12345], rng)
    models = [_rand_model(kind, n, M, rng, stay=float(s)) for s in range(8)]
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=256)
    eng.set_option("score_layout", layout)
    batch = eng.score(models)
    singles = np.stack([eng.score([m])[0] for m in models])
    assert np.array_equal(batch, singles)
    perm = rng.permutation(8)
    assert np.array_equal(eng.score([models[i] for i in perm]), batch[perm])
    assert np.array_equal(eng.score(models), batch)
    _check_oracle(kind, obs, models, batch)
    assert eng.get_option("score_fallbacks") == 0
    eng.close()


# ---- 3. agreement with the E-step ------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_agrees_with_estep(kind, M):
    rng = np.random.default_rng(11)
    n = 6
    obs = _rand_obs(kind, n, M, [50000, 33333, 10, 4096], rng)
    m = _rand_model(kind, n, M, rng, stay=3.0)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    res = eng.estep(*m)
    logL = eng.score([m])
    np.testing.assert_allclose(logL[0], res.logL_k, rtol=RTOL)
    np.testing.assert_allclose(logL[0].sum(), res.loglik, rtol=RTOL)
    assert eng.get_option("score_fallbacks") == 0
    eng.close()


# ---- 4. / 5. no side effects, fallback ---------------------------------------------------------------
def _em_sequence(kind, obs, n, M, models, others, score_W=None):
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=512)
    if score_W is not None:
        eng.set_option("score_W", score_W)
    out = []
    for i, m in enumerate(models):
        res = eng.estep(*m)
        out.append((res.packed.copy(), res.logL_k.copy(), eng.get_option("spec_W"),
                    eng.get_option("carry_ok"), eng.get_option("carry_fail"), eng.get_option("spec_fail")))
        if others is not None:
            eng.score(others)
    fb = eng.get_option("score_fallbacks")
    eng.close()
    return out, fb


def _assert_same_sequence(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0])
        assert np.array_equal(x[1], y[1])
        assert x[2:] == y[2:]


@pytest.mark.parametrize("score_W", [None, 4])
def test_no_side_effects_estep(score_W):
    rng = np.random.default_rng(5)
    n, M = 4, 16
    obs = _rand_obs("discrete", n, M, [60000, 40000, 333], rng)
    base = _rand_model("discrete", n, M, rng, stay=20.0)
    # an EM-like sequence: models that move a little from one iteration to the next
    models = []
    for i in range(5):
        A = base[0] + 0.002 * i * np.eye(n)
        A /= A.sum(axis=1)[:, None]
        models.append((A, base[1], base[2], None))
    others = [_rand_model("discrete", n, M, rng, stay=s) for s in (0.0, 30.0)]
    plain, _ = _em_sequence("discrete", obs, n, M, models, None)
    mixed, fb = _em_sequence("discrete", obs, n, M, models, others, score_W=score_W)
    _assert_same_sequence(plain, mixed)
    if score_W == 4:
        assert fb > 0   # a four-step warm-up cannot verify these slowly mixing models


def test_fallback_correct():
    rng = np.random.default_rng(9)
    n, M = 3, 5
    obs = _rand_obs("discrete", n, M, [20000, 5000, 17], rng)
    models = [_rand_model("discrete", n, M, rng, stay=40.0) for _ in range(3)]
    eng = _engine()
    eng.set_observations("discrete", obs, n, nsymbols=M, chunk=64)
    ref = eng.score(models)
    assert eng.get_option("score_fallbacks") == 0
    eng.set_option("score_W", 2)
    assert eng.get_option("score_W") == 2
    forced = eng.score(models)
    assert eng.get_option("score_fallbacks") > 0
    _check_oracle("discrete", obs, models, forced)
    np.testing.assert_allclose(forced, ref, rtol=RTOL)
    eng.close()


def test_no_side_effects_paths():
    rng = np.random.default_rng(12)
    n = 8
    obs = _rand_obs("gaussian", n, 0, [30000, 20000, 99], rng)
    m = _rand_model("gaussian", n, 0, rng, stay=5.0)
    others = [_rand_model("gaussian", n, 0, rng) for _ in range(3)]
    res = []
    for with_score in (False, True):
        eng = _engine()
        eng.set_observations("gaussian", obs, n, chunk=1024)
        eng.estep(*m)
        if with_score:
            eng.score(others)
        v = eng.viterbi(*m)
        if with_score:
            eng.score(others)
        p, C, n0, emis = eng.sample_paths(*m, seed=3)
        if with_score:
            eng.score(others)
        r = eng.estep(*m)
        res.append((v, p, C, n0, emis, r.packed.copy(), eng.get_option("spec_W")))
        eng.close()
    a, b = res
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert np.array_equal(x, y)
    for x, y in zip(a[2:6], b[2:6]):
        assert np.array_equal(x, y)
    assert a[6] == b[6]


def test_zero_probability_is_minus_inf():
    rng = np.random.default_rng(4)
    n, M = 3, 4
    obs = [rng.integers(0, 3, T).astype(np.int32) for T in (5000, 300, 4000)]
    obs[1][150] = 3                       # symbol 3 appears in trajectory 1 only
    good = _rand_model("discrete", n, M, rng)
    B = good[2].copy()
    B[:, 3] = 0.0                         # ... and no state of this model emits it
    B /= B.sum(axis=1)[:, None]
    bad = (good[0], good[1], B, None)
    # reachability: state 2 is never entered from pi = e0 under A, and only state 2 emits symbol 0
    A = np.array([[0.7, 0.3, 0.0], [0.4, 0.6, 0.0], [0.3, 0.3, 0.4]])
    B2 = np.array([[0.0, 0.5, 0.3, 0.2], [0.0, 0.2, 0.4, 0.4], [1.0, 0.0, 0.0, 0.0]])
    unreach = (A, np.array([1.0, 0.0, 0.0]), B2, None)
    for chunk in (0, 64):
        eng = _engine()
        eng.set_observations("discrete", obs, n, nsymbols=M, chunk=chunk)
        logL = eng.score([good, bad, unreach])
        assert not np.any(np.isnan(logL))
        _check_oracle("discrete", obs, [good], logL[:1])
        assert logL[1, 1] == -np.inf
        np.testing.assert_allclose(logL[1, [0, 2]], _oracle("discrete", [obs[0], obs[2]], bad), rtol=RTOL)
        assert np.all(logL[2] == -np.inf)
        eng.close()


def test_invalid_model():
    rng = np.random.default_rng(1)
    obs = _rand_obs("gaussian", 2, 0, [100], rng)
    eng = _engine()
    eng.set_observations("gaussian", obs, 2)
    A, pi, mu, sg = _rand_model("gaussian", 2, 0, rng)
    with pytest.raises(ValueError, match="model 1"):
        eng.score([(A, pi, mu, sg), (A * 1.5, pi, mu, sg)])
    with pytest.raises(ValueError):
        eng.score([(A, pi, mu, np.array([1.0, -1.0]))])
    with pytest.raises(ValueError):
        eng.score([(A, pi, np.array([np.nan, 0.0]), sg)])
    eng.close()


# ---- 6. other observation sources ------------------------------------------------------------------
def test_lagged_and_device_observations():
    import torch
    from bhmm_amd.api import lag_observations
    rng = np.random.default_rng(21)
    n, M = 5, 7
    base = _rand_obs("discrete", n, M, [9000, 4000], rng)
    models = [_rand_model("discrete", n, M, rng, stay=2.0) for _ in range(3)]
    lagged = lag_observations(base, 3)
    host = _engine()
    host.set_observations("discrete", [np.ascontiguousarray(o) for o in lagged], n, nsymbols=M)
    ref = host.score(models)
    host.close()
    eng = _engine()
    eng.set_observations_lagged("discrete", lagged.base, lagged.lag, lagged.views, n, nsymbols=M)
    assert np.array_equal(eng.score(models), ref)
    eng.close()
    flat = np.concatenate(base).astype(np.int32)
    t = torch.from_numpy(flat).to("cuda:0")
    off = np.array([0, len(base[0]), len(flat)], dtype=np.int64)
    h2 = _engine()
    h2.set_observations("discrete", base, n, nsymbols=M)
    ref2 = h2.score(models)
    h2.close()
    dev = _engine()
    dev.set_observations_device("discrete", t.data_ptr(), off, n, nsymbols=M)
    assert np.array_equal(dev.score(models), ref2)
    dev.close()
    _check_oracle("discrete", base, models, ref2)


# ---- 7. more than 8 states (exact serial path) ---------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 10)])
@pytest.mark.parametrize("n", [16, 64])
def test_many_states(n, kind, M):
    rng = np.random.default_rng(n + M)
    obs = _rand_obs(kind, n, M, [700, 1, 250], rng)
    models = [_rand_model(kind, n, M, rng) for _ in range(2)]
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    _check_oracle(kind, obs, models, eng.score(models))
    eng.close()


@pytest.mark.parametrize("n", [2, 3])
def test_explicit_pobs(n):
    # (n = 3: the serial kernel reads rows of n doubles, not of the padded width)
    rng = np.random.default_rng(2 + n)
    pobs = [rng.random((300, n)) + 0.01, rng.random((40, n))]
    A = _rand_A(n, rng)
    pi = np.full(n, 1.0 / n)
    eng = _engine()
    eng.set_observations("explicit", pobs, n)
    logL = eng.score([(A, pi, None, None)])
    np.testing.assert_allclose(logL[0], [orc.forward(A, p, pi)[0] for p in pobs], rtol=RTOL)
    eng.close()


# ---- 8. Python layer --------------------------------------------------------------------------------
def test_python_layer():
    import bhmm_amd
    from bhmm_amd import MaximumLikelihoodEstimator
    rng = np.random.default_rng(31)
    n = 3
    obs = _rand_obs("gaussian", n, 0, [2000, 1500], rng)
    hmm = bhmm_amd.estimate_hmm(obs, n, maxit=5)
    sampled = bhmm_amd.bayesian_hmm(obs, hmm, nsample=5)
    tot = bhmm_amd.score(obs, sampled)
    per = bhmm_amd.score(obs, sampled, per_trajectory=True)
    assert tot.shape == (5,) and per.shape == (5, 2)
    for s, h in enumerate(sampled.sampled_hmms):
        m = (h.transition_matrix, h.initial_distribution, h.output_model.means, h.output_model.sigmas)
        np.testing.assert_allclose(per[s], _oracle("gaussian", obs, m), rtol=RTOL)
        np.testing.assert_allclose(tot[s], per[s].sum(), rtol=1e-14)
    one = bhmm_amd.score(obs, hmm)
    assert one.shape == (1,)
    est = MaximumLikelihoodEstimator(obs, n, initial_model=hmm, output="gaussian", maxit=3)
    cur = est.score()
    m = (hmm.transition_matrix, hmm.initial_distribution, hmm.output_model.means, hmm.output_model.sigmas)
    np.testing.assert_allclose(cur[0], _oracle("gaussian", obs, m).sum(), rtol=RTOL)
    np.testing.assert_allclose(est.score(sampled.sampled_hmms), tot, rtol=RTOL)
    np.testing.assert_allclose(est.score(sampled), tot, rtol=RTOL)   # a SampledHMM: its sampled models


# ---- 9. full size -----------------------------------------------------------------------------------
def test_full_size():
    import torch
    from bhmm_amd.engine import synth_observations
    rng = np.random.default_rng(3000)
    n, M, K, T = 8, 64, 1024, 1000000
    A = _rand_A(n, rng, stay=50.0)
    pi = np.full(n, 1.0 / n)
    B = rng.dirichlet(np.ones(M), size=n)
    obs = torch.empty(K * T, dtype=torch.int32, device="cuda:0")
    synth_observations("discrete", obs.data_ptr(), A, pi, B, None, K, T, seed=5)
    torch.cuda.synchronize()
    eng = _engine()
    eng.set_observations_device("discrete", obs.data_ptr(), np.arange(K + 1, dtype=np.int64) * T, n, nsymbols=M)
    models = [(0.9 * A + 0.1 / n, pi, 0.8 * B + 0.2 / M, None)]
    for i in range(3):
        A2 = A + 0.05 * (i + 1) * np.eye(n)
        models.append((A2 / A2.sum(axis=1)[:, None], pi, B, None))
    logL = eng.score(models)
    assert eng.get_option("score_fallbacks") == 0
    for s, m in enumerate(models):
        res = eng.estep(*m)
        np.testing.assert_allclose(logL[s].sum(), res.loglik, rtol=RTOL)
    eng.close()
