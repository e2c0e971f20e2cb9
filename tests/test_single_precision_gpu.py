"""Single-precision E-step (BHMM_FLAG_SINGLE, estep_f32.hpp) on the GPU: the accuracy contract
against the fp64 oracle, the fallbacks to the fp64 path, interleaving with fp64 E-steps on one
context, bitwise reproducibility and the mixed-precision EM of the estimator.

Contract (each fp32 E-step against oracle.estep):
  log-likelihoods (per trajectory and sum)   1e-6 relative
  C, state counts, sum gamma_0               1e-5 of the row total (state counts: of all steps;
                                             sum gamma_0: of K)
  sum gamma (o - mu)                         1e-5 * sum_t gamma_t(i) sigma_i
  sum gamma (o - mu)^2                       1e-5 relative
  discrete symbol counts                     1e-5 of the state's total
"""
import numpy as np
import pytest

import bhmm_amd
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

TOL_L = 1e-6
TOL_C = 1e-5


def _engine():
    from bhmm_amd.engine import Engine
    return Engine(0)


def _model(n, kind, M=0, seed=0, lifetime=(5.0, 40.0), offset=1000.0):
    rng = np.random.default_rng(seed)
    life = rng.uniform(lifetime[0], lifetime[1], n)
    A = rng.random((n, n)) + 0.05
    np.fill_diagonal(A, 0.0)
    A = A / A.sum(axis=1)[:, None] * (1.0 / life)[:, None]
    A[np.diag_indices(n)] = 1.0 - 1.0 / life
    pi = rng.random(n) + 0.1
    pi /= pi.sum()
    if kind == 'gaussian':
        mu = offset + np.linspace(-3.0, 3.0, n) * (1.0 + 0.1 * rng.random(n))
        sigma = 0.6 + 0.6 * rng.random(n)
        return A, pi, mu, sigma
    B = rng.random((n, M)) ** 3 + 1e-3
    B /= B.sum(axis=1)[:, None]
    return A, pi, B, None


def _sample(A, kind, par0, par1, lengths, seed):
    """Observations of the model: hidden path by vectorised geometric dwell times (the chain's
    exit law, then the jump law), emissions by inverse CDF."""
    rng = np.random.default_rng(seed)
    n = A.shape[0]
    stay = np.diag(A)
    J = A - np.diag(stay)
    J = J / J.sum(axis=1)[:, None]
    out = []
    for T in lengths:
        states, total, s = [], 0, rng.integers(n)
        while total < T:
            d = rng.geometric(1.0 - stay[s], size=1)[0]
            states.append(np.full(d, s))
            total += d
            s = rng.choice(n, p=J[s])
        S = np.concatenate(states)[:T] if states else np.zeros(0, int)
        if kind == 'gaussian':
            out.append(par0[S] + par1[S] * rng.standard_normal(T))
        else:
            cdf = np.cumsum(par0, axis=1)
            u = rng.random(T)
            o = np.zeros(T, dtype=np.int64)
            for i in range(n):
                sel = S == i
                o[sel] = np.searchsorted(cdf[i], u[sel], side='right')
            out.append(np.minimum(o, par0.shape[1] - 1).astype(np.int32))
    return out


def _oracle_stats(kind, obs, A, pi, par0, par1):
    r = orc.estep(kind, obs, A, pi, par0, par1, want_gamma=True)
    if kind == 'gaussian':
        mu = np.asarray(par0)
        r['sd'] = sum((g * (o[:, None] - mu[None, :])).sum(axis=0) for o, g in zip(obs, r['gammas']))
        r['sdd'] = sum((g * (o[:, None] - mu[None, :]) ** 2).sum(axis=0) for o, g in zip(obs, r['gammas']))
    else:
        cnt = np.zeros((A.shape[0], par0.shape[1]))
        for o, g in zip(obs, r['gammas']):
            orc.update_pout(o, g, cnt)
        r['cnt'] = cnt
    return r


def _check_contract(res, ref, kind, K, par1=None):
    np.testing.assert_allclose(res.logL_k, ref['logL'], rtol=TOL_L, atol=0)
    np.testing.assert_allclose(res.loglik, ref['logL'].sum(), rtol=TOL_L, atol=0)
    rows = ref['C'].sum(axis=1)
    assert np.all(np.abs(res.C - ref['C']) <= TOL_C * rows[:, None] + 1e-300), \
        np.max(np.abs(res.C - ref['C']) / np.maximum(rows[:, None], 1e-300))
    total = ref['state_counts'].sum()
    assert np.all(np.abs(res.state_counts - ref['state_counts']) <= TOL_C * total)
    assert np.all(np.abs(res.gamma0_sum - ref['gamma0_sum']) <= TOL_C * K)
    sc = ref['state_counts']
    if kind == 'gaussian':
        assert np.all(np.abs(res.sum_gd - ref['sd']) <= TOL_C * sc * par1 + 1e-300)
        np.testing.assert_allclose(res.sum_gdd, ref['sdd'], rtol=TOL_C, atol=0)
    else:
        assert np.all(np.abs(res.symbol_counts - ref['cnt']) <= TOL_C * sc[:, None] + 1e-300)


RAGGED = [1, 5, 63, 700, 3001, 20000]


@pytest.mark.parametrize('chunk', [0, 64, 100000])
@pytest.mark.parametrize('kind,M', [('gaussian', 0), ('discrete', 3), ('discrete', 64), ('discrete', 1000)])
@pytest.mark.parametrize('n', [2, 3, 4, 5, 7, 8])
def test_parity(n, kind, M, chunk):
    A, pi, par0, par1 = _model(n, kind, M, seed=n * 7 + M)
    obs = _sample(A, kind, par0, par1, RAGGED, seed=n + M)
    ref = _oracle_stats(kind, obs, A, pi, par0, par1)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=chunk)
    res = eng.estep(A, pi, par0, par1, single=True)
    assert eng.get_option('f32_used') == 1.0
    assert eng.get_option('f32_fallbacks') == 0.0
    _check_contract(res, ref, kind, len(obs), par1)
    eng.close()


def test_parity_long_discrete():
    A, pi, B, _ = _model(8, 'discrete', 64, seed=11, lifetime=(20.0, 200.0))
    obs = _sample(A, 'discrete', B, None, [1000000] * 4, seed=3)
    ref = _oracle_stats('discrete', obs, A, pi, B, None)
    eng = _engine()
    eng.set_observations('discrete', obs, 8, nsymbols=64)
    res = eng.estep(A, pi, B, single=True)
    assert eng.get_option('f32_used') == 1.0
    _check_contract(res, ref, 'discrete', 4)
    eng.close()


@pytest.mark.parametrize('kind,M', [('gaussian', 0), ('discrete', 16)])
def test_parity_lagged(kind, M):
    A, pi, par0, par1 = _model(5, kind, M, seed=5)
    base = _sample(A, kind, par0, par1, [4000, 2500], seed=9)
    lag = 3
    views = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2)]
    obs = [base[k][s::lag] for k, s in views]
    ref = _oracle_stats(kind, obs, A, pi, par0, par1)
    eng = _engine()
    eng.set_observations_lagged(kind, base, lag, views, 5, nsymbols=M, chunk=64)
    res = eng.estep(A, pi, par0, par1, single=True)
    assert eng.get_option('f32_used') == 1.0
    _check_contract(res, ref, kind, len(obs), par1)
    eng.close()


def test_parity_stats_dev():
    import torch
    A, pi, mu, sigma = _model(8, 'gaussian', seed=2)
    obs = _sample(A, 'gaussian', mu, sigma, RAGGED, seed=4)
    ref = _oracle_stats('gaussian', obs, A, pi, mu, sigma)
    eng = _engine()
    eng.set_observations('gaussian', obs, 8, chunk=64)
    buf = torch.zeros(eng.stats_size, dtype=torch.float64, device='cuda:0')
    eng.estep_launch(A, pi, mu, sigma, stats_dev=buf.data_ptr(), single=True)
    res = eng.estep_fetch()
    assert eng.get_option('f32_used') == 1.0
    _check_contract(res, ref, 'gaussian', len(obs), sigma)
    np.testing.assert_array_equal(buf.cpu().numpy(), res.packed)
    eng.close()


def _rare_state_model(p_enter, M=16, seed=13):
    # 4-state discrete model whose state 0 is entered with probability p_enter per step (and left after
    # two steps on average): its occupancy is about 2 p_enter of all steps
    A, pi, B, _ = _model(4, 'discrete', M, seed=seed)
    A[1:, 0] = p_enter
    A[1:, 1:] *= ((1.0 - p_enter) / A[1:, 1:].sum(axis=1))[:, None]
    A[0] = [0.5, 0.2, 0.2, 0.1]
    pi = np.array([p_enter, 0.4, 0.3, 0.3 - p_enter])
    return A, pi, B


def test_parity_rarely_occupied_state():
    # state 0 holds ~100 of 50 000 steps: resolved in fp32, within the contract of its own (small) total
    A, pi, B = _rare_state_model(1e-3)
    obs = _sample(A, 'discrete', B, None, [30000, 15000, 5000], seed=5)
    ref = _oracle_stats('discrete', obs, A, pi, B, None)
    assert ref['state_counts'][0] < 1e-2 * ref['state_counts'].sum()
    eng = _engine()
    eng.set_observations('discrete', obs, 4, nsymbols=16, chunk=64)
    res = eng.estep(A, pi, B, single=True)
    assert eng.get_option('f32_used') == 1.0
    _check_contract(res, ref, 'discrete', len(obs))
    eng.close()


def test_nearly_unoccupied_state_falls_back():
    # state 0 holds ~1e-5 of a step in total: its symbol counts are below what the fixed-point count tables
    # resolve (gamma < 2^-32 on every step would leave its row zero), so the E-step runs fp64
    A, pi, B = _rare_state_model(1e-10)
    obs = _sample(A, 'discrete', B, None, [30000, 15000, 5000], seed=5)
    ref = _oracle_stats('discrete', obs, A, pi, B, None)
    eng = _engine()
    eng.set_observations('discrete', obs, 4, nsymbols=16, chunk=64)
    res = eng.estep(A, pi, B, single=True)
    _assert_fallback(eng, 0, res, _fresh_fp64('discrete', obs, 4, 16, 64, A, pi, B, None))
    _check_contract(res, ref, 'discrete', len(obs))
    assert np.all(res.symbol_counts.sum(axis=1) > 0)
    eng.close()


# ---- fallbacks: fp64 statistics, bitwise those of a fresh context --------------------------------
def _fresh_fp64(kind, obs, n, M, chunk, A, pi, par0, par1, store_gamma=False):
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=chunk)
    res = eng.estep(A, pi, par0, par1, store_gamma=store_gamma)
    eng.close()
    return res


def _assert_fallback(eng, before, res, ref):
    assert eng.get_option('f32_used') == 0.0
    assert eng.get_option('f32_fallbacks') == before + 1
    np.testing.assert_array_equal(res.packed, ref.packed)
    np.testing.assert_array_equal(res.logL_k, ref.logL_k)


def test_fallback_gaussian_outlier():
    A, pi, mu, sigma = _model(4, 'gaussian', seed=3)
    obs = _sample(A, 'gaussian', mu, sigma, [3000, 500], seed=1)
    obs[0][1234] = mu.max() + 25.0 * sigma.max()    # every fp32 density underflows, fp64's do not
    eng = _engine()
    eng.set_observations('gaussian', obs, 4, chunk=64)
    res = eng.estep(A, pi, mu, sigma, single=True)
    _assert_fallback(eng, 0, res, _fresh_fp64('gaussian', obs, 4, 0, 64, A, pi, mu, sigma))
    eng.close()


def test_fallback_store_gamma():
    A, pi, B, _ = _model(4, 'discrete', 8, seed=4)
    obs = _sample(A, 'discrete', B, None, [2000, 300], seed=2)
    eng = _engine()
    eng.set_observations('discrete', obs, 4, nsymbols=8, chunk=64)
    res = eng.estep(A, pi, B, store_gamma=True, single=True)
    _assert_fallback(eng, 0, res, _fresh_fp64('discrete', obs, 4, 8, 64, A, pi, B, None, store_gamma=True))
    eng.close()


def test_fallback_nine_states():
    A, pi, mu, sigma = _model(9, 'gaussian', seed=9)
    obs = _sample(A, 'gaussian', mu, sigma, [3000, 800], seed=3)
    eng = _engine()
    eng.set_observations('gaussian', obs, 9)
    res = eng.estep(A, pi, mu, sigma, single=True)
    _assert_fallback(eng, 0, res, _fresh_fp64('gaussian', obs, 9, 0, 0, A, pi, mu, sigma))
    eng.close()


def test_fallback_boundary_check():
    # slowly mixing, weakly informative: one warm-up step cannot find the boundary vectors
    n = 4
    A = np.full((n, n), 0.0005 / (n - 1))
    np.fill_diagonal(A, 0.9995)
    pi = np.full(n, 1.0 / n)
    mu = np.linspace(0.0, 0.6, n)
    sigma = np.full(n, 1.0)
    obs = _sample(A, 'gaussian', mu, sigma, [20000, 5000], seed=6)
    eng = _engine()
    eng.set_observations('gaussian', obs, n, chunk=64)
    eng.set_option('f32_W', 1)
    res = eng.estep(A, pi, mu, sigma, single=True)
    assert eng.get_option('f32_last_dev') > eng.get_option('f32_tol')
    _assert_fallback(eng, 0, res, _fresh_fp64('gaussian', obs, n, 0, 64, A, pi, mu, sigma))
    eng.close()


# ---- fp64 E-steps around fp32 ones on one context ---------------------------------------------------
@pytest.mark.parametrize('kind,M', [('gaussian', 0), ('discrete', 32)])
def test_interleaved_fp64_unaffected(kind, M):
    A0, pi, p0, p1 = _model(8, kind, M, seed=21)
    obs = _sample(A0, kind, p0, p1, [40000, 30000, 7000], seed=8)
    eng = _engine()
    eng.set_observations(kind, obs, 8, nsymbols=M, chunk=256)
    eng.set_option('carry', 1)
    rng = np.random.default_rng(0)
    A, par0 = A0.copy(), p0.copy()
    for it, single in enumerate([False, False, True, False, True, True, False, False]):
        # an EM-like sequence: small changes of the model
        A = A * (1.0 + 0.002 * rng.standard_normal(A.shape))
        A /= A.sum(axis=1)[:, None]
        if kind == 'gaussian':
            par0 = par0 + 0.002 * rng.standard_normal(par0.shape)
        else:
            par0 = par0 * (1.0 + 0.002 * rng.random(par0.shape))
            par0 /= par0.sum(axis=1)[:, None]
        res = eng.estep(A, pi, par0, p1, single=single)
        ref = _oracle_stats(kind, obs, A, pi, par0, p1)
        if single:
            assert eng.get_option('f32_used') == 1.0
            _check_contract(res, ref, kind, len(obs), p1)
        else:
            assert eng.get_option('f32_used') == 0.0
            np.testing.assert_allclose(res.logL_k, ref['logL'], rtol=1e-9)
            np.testing.assert_allclose(res.C, ref['C'], rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(res.gamma0_sum, ref['gamma0_sum'], rtol=1e-9, atol=1e-14)
            np.testing.assert_allclose(res.state_counts, ref['state_counts'], rtol=1e-9, atol=1e-12)
    eng.close()


def test_reproducible():
    A, pi, B, _ = _model(8, 'discrete', 64, seed=31)
    obs = _sample(A, 'discrete', B, None, [50000, 20000, 9, 3000], seed=7)
    eng = _engine()
    eng.set_observations('discrete', obs, 8, nsymbols=64, chunk=128)
    r1 = eng.estep(A, pi, B, single=True)
    r2 = eng.estep(A, pi, B, single=True)
    assert eng.get_option('f32_used') == 1.0
    np.testing.assert_array_equal(r1.packed, r2.packed)
    np.testing.assert_array_equal(r1.logL_k, r2.logL_k)
    eng.close()


# ---- mixed-precision EM ------------------------------------------------------------------------------
def _em_pair(obs, n, output, init):
    res = {}
    for prec in ('float64', 'mixed'):
        res[prec] = bhmm_amd.estimate_hmm(obs, n, output=output, initial_model=init, accuracy=1e-8,
                                          estep_precision=prec)
    return res['float64'], res['mixed']


def _compare_em(h64, hmx, output):
    np.testing.assert_allclose(hmx.initial_distribution, h64.initial_distribution, atol=1e-5)
    np.testing.assert_allclose(hmx.transition_matrix, h64.transition_matrix, atol=1e-5)
    if output == 'gaussian':
        np.testing.assert_allclose(hmx.output_model.means, h64.output_model.means, atol=1e-5)
        np.testing.assert_allclose(hmx.output_model.sigmas, h64.output_model.sigmas, atol=1e-5)
    else:
        np.testing.assert_allclose(hmx.output_model.output_probabilities,
                                   h64.output_model.output_probabilities, atol=1e-5)
    assert abs(hmx.likelihood - h64.likelihood) <= 1e-6 * abs(h64.likelihood)


def _mixed_estimator(obs, n, output, init, prec='mixed'):
    from bhmm_amd.estimators.maximum_likelihood import MaximumLikelihoodEstimator
    est = MaximumLikelihoodEstimator(obs, n, initial_model=init, output=output, accuracy=1e-8,
                                     estep_precision=prec)
    est.fit()
    return est


def test_em_mixed_gaussian():
    from bhmm_amd.util import testsystems
    model, obs, _ = testsystems.generate_synthetic_observations(
        nstates=3, ntrajectories=8, length=20000, output='gaussian', rng=np.random.RandomState(5))
    init = bhmm_amd.init_hmm(obs, 3, output='gaussian')
    h64, hmx = _em_pair(obs, 3, 'gaussian', init)
    _compare_em(h64, hmx, 'gaussian')
    est = _mixed_estimator(obs, 3, 'gaussian', init)
    assert 'float32' in est.estep_precisions
    assert est.estep_precisions[-2:] == ['float64', 'float64']
    f32 = _mixed_estimator(obs, 3, 'gaussian', init, prec='float32')
    assert np.isfinite(f32.likelihood) and 'float32' in f32.estep_precisions


def test_em_mixed_discrete():
    from bhmm_amd.util import testsystems
    model, obs, _ = testsystems.generate_synthetic_observations(
        nstates=4, ntrajectories=8, length=20000, output='discrete', rng=np.random.RandomState(6))
    obs = [np.asarray(o, dtype=np.int32) for o in obs]
    init = bhmm_amd.init_hmm(obs, 4, output='discrete')
    h64, hmx = _em_pair(obs, 4, 'discrete', init)
    _compare_em(h64, hmx, 'discrete')
    est = _mixed_estimator(obs, 4, 'discrete', init)
    assert 'float32' in est.estep_precisions
    assert est.estep_precisions[-2:] == ['float64', 'float64']
    f32 = _mixed_estimator(obs, 4, 'discrete', init, prec='float32')
    assert np.isfinite(f32.likelihood) and 'float32' in f32.estep_precisions
