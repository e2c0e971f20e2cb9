"""Host side of the Gibbs sampler for gaussian-mixture emissions (no GPU):
bhmm_gibbs_parameters_gmm against bhmm_gibbs_parameters_mvn and the Dirichlet's moments, the draw rule of
bhmm_gmm_path_components restated in numpy (tests/gmm_draw_ref.py) against e_c / sum e, and
GaussianMixtureOutputModel.sample_from_statistics."""
import numpy as np
import pytest

import bhmm_amd
from bhmm_amd.estimators._native import GibbsParametersGmm, GibbsParametersMvn
from bhmm_amd.output_models import GaussianMixtureOutputModel
from bhmm_amd.output_models.mvgaussian import pack_moments
from tests import gmm_draw_ref as ref


def _counts(rng, n):
    C = rng.integers(1, 40, size=(n, n)).astype(np.float64)
    n0 = rng.integers(0, 4, size=n).astype(np.float64)
    return C, n0


def _component_statistics(rng, nm, D, ctype, counts):
    """current means / covariances of nm components and the packed moments of `counts` points each about the means"""
    mu = rng.normal(size=(nm, D)) * 3.0
    cov = np.array([np.eye(D) * (0.5 + q % 3) + 0.1 for q in range(nm)])
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    if ctype == 'diag':
        cov = np.array([np.diag(c) for c in cov])
    S0, S1, S2 = [], [], []
    for q in range(nm):
        d = rng.normal(size=(int(counts[q]), D)) * 1.3 + 0.2
        S0.append(float(counts[q]))
        S1.append(d.sum(axis=0))
        S2.append(d.T.dot(d) if ctype == 'full' else (d * d).sum(axis=0))
    return mu, cov, pack_moments(S0, np.array(S1), np.array(S2), ctype)


# ---- M = 1 is the multivariate gaussian kind ------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("reversible", [True, False])
def test_one_component_is_the_mvgaussian_kind(reversible, ctype):
    rng = np.random.default_rng(31 + reversible)
    n, D = 4, 3
    C, n0 = _counts(rng, n)
    mu, cov, mom = _component_statistics(rng, n, D, ctype, [0, 1, 25, 60])
    prior_C, prior_n0 = np.full((n, n), 0.5), np.full(n, 0.25)
    packed = np.concatenate([C.ravel(), n0, mom])
    seed, sweep = 0xFEED, 3
    m = GibbsParametersMvn(n, D, ctype, prior_C=prior_C, prior_n0=prior_n0, reversible=reversible, nsteps=50)
    T1, p1, mu1, cov1 = m(packed, mu, cov, seed, sweep)
    for prior_w in (None, np.full((n, 1), 3.5), np.zeros((n, 1))):
        g = GibbsParametersGmm(n, 1, D, ctype, prior_C=prior_C, prior_n0=prior_n0, prior_w=prior_w,
                               reversible=reversible, nsteps=50)
        T2, p2, w2, mu2, cov2 = g(packed, np.ones((n, 1)), mu[:, None], cov[:, None], seed, sweep)
        assert np.array_equal(T1, T2) and np.array_equal(p1, p2)
        assert np.array_equal(mu1, mu2[:, 0]) and np.array_equal(cov1, cov2[:, 0])
        assert np.array_equal(w2, np.ones((n, 1)))
        assert g.info[0] == m.info[0] and g.info[1] == m.info[1] and g.info[2] == 0


# ---- means and covariances per component are the mvgaussian draws over n M labels ----------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
def test_components_are_drawn_as_states_of_the_mvgaussian_kind(ctype):
    rng = np.random.default_rng(77)
    n, M, D = 3, 4, 2
    nm = n * M
    counts = rng.integers(5, 50, size=nm)
    counts[2], counts[7] = 0, 1
    mu, cov, mom = _component_statistics(rng, nm, D, ctype, counts)
    seed, sweep = 12345, 9
    # the mvgaussian call sees n M states: its transition part differs, its emission part comes first on the stream
    Cb, n0b = _counts(rng, nm)
    m = GibbsParametersMvn(nm, D, ctype, reversible=False, nsteps=1)
    _, _, mu1, cov1 = m(np.concatenate([Cb.ravel(), n0b, mom]), mu, cov, seed, sweep)
    C, n0 = _counts(rng, n)
    g = GibbsParametersGmm(n, M, D, ctype, prior_w=np.ones((n, M)), reversible=False, nsteps=1)
    w0 = np.full((n, M), 1.0 / M)
    _, _, w2, mu2, cov2 = g(np.concatenate([C.ravel(), n0, mom]), w0, mu.reshape(n, M, D),
                            cov.reshape((n, M) + cov.shape[1:]), seed, sweep)
    assert np.array_equal(mu1, mu2.reshape(nm, D))
    assert np.array_equal(cov1, cov2.reshape(cov.shape))
    assert g.info[1] == m.info[1]
    np.testing.assert_allclose(w2.sum(axis=1), 1.0, rtol=0, atol=4e-16)
    assert np.all(w2 > 0.0)
    # the empty component keeps its parameters and has a positive weight from the prior
    assert np.array_equal(mu2.reshape(nm, D)[2], mu[2]) and np.array_equal(cov2.reshape(cov.shape)[2], cov[2])
    assert w2.ravel()[2] > 0.0


# ---- the weights ---------------------------------------------------------------------------------------------
def test_weight_moments():
    """4000 draws on fixed counts against the Dirichlet's mean and variance, within five standard errors (those of
    the mean from the known variance, those of the variance from the drawn sample itself)"""
    rng = np.random.default_rng(3)
    n, M, D, nd = 2, 3, 1, 4000
    counts = np.array([4.0, 11.0, 0.0, 30.0, 2.0, 7.0])
    prior_w = np.array([[1.0, 0.5, 2.0], [0.25, 1.0, 1.0]])
    mu, cov, mom = _component_statistics(rng, n * M, D, 'diag', counts)
    packed = np.concatenate([np.ones(n * n), np.ones(n), mom])
    g = GibbsParametersGmm(n, M, D, 'diag', prior_w=prior_w, reversible=False, nsteps=1)
    w0 = np.full((n, M), 1.0 / M)
    ws = np.empty((nd, n, M))
    for s in range(nd):
        ws[s] = g(packed, w0, mu.reshape(n, M, D), cov.reshape(n, M, D), 20250101, s)[2]
    alpha = prior_w + counts.reshape(n, M)
    a0 = alpha.sum(axis=1, keepdims=True)
    mean = alpha / a0
    var = alpha * (a0 - alpha) / (a0 * a0 * (a0 + 1.0))
    np.testing.assert_allclose(ws.sum(axis=2), 1.0, rtol=0, atol=4e-16)
    assert np.all(np.abs(ws.mean(axis=0) - mean) <= 5 * np.sqrt(var / nd))
    sq = (ws - mean) ** 2
    assert np.all(np.abs(sq.mean(axis=0) - var) <= 5 * sq.std(axis=0, ddof=1) / np.sqrt(nd))


def test_zero_alpha_gives_weight_zero_and_an_untouched_component():
    rng = np.random.default_rng(4)
    n, M, D = 2, 3, 2
    counts = np.array([10.0, 0.0, 20.0, 0.0, 0.0, 0.0])
    prior_w = np.array([[1.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    mu, cov, mom = _component_statistics(rng, n * M, D, 'full', counts)
    packed = np.concatenate([np.ones(n * n), np.ones(n), mom])
    g = GibbsParametersGmm(n, M, D, 'full', prior_w=prior_w, reversible=False, nsteps=1)
    w0 = np.array([[0.2, 0.3, 0.5], [0.6, 0.3, 0.1]])
    _, _, w, m2, c2 = g(packed, w0, mu.reshape(n, M, D), cov.reshape(n, M, D, D), 5, 0)
    assert w[0, 1] == 0.0 and w[0, 0] > 0.0 and w[0, 2] > 0.0
    assert abs(w[0].sum() - 1.0) <= 4e-16
    assert np.array_equal(w[1], w0[1])                    # every alpha of the state is 0: its weights stay
    assert np.array_equal(m2[0, 1], mu[1]) and np.array_equal(c2[0, 1], cov[1])
    assert not np.array_equal(m2[0, 0], mu[0])
    assert g.info[2] == 1


def test_empty_component_with_a_positive_prior():
    rng = np.random.default_rng(6)
    n, M, D = 1, 2, 2
    mu, cov, mom = _component_statistics(rng, 2, D, 'diag', [40.0, 0.0])
    packed = np.concatenate([[3.0], [1.0], mom])
    g = GibbsParametersGmm(n, M, D, 'diag', prior_w=np.ones((1, 2)), reversible=False, nsteps=1)
    _, _, w, m2, c2 = g(packed, np.array([[0.5, 0.5]]), mu.reshape(1, 2, D), cov.reshape(1, 2, D), 8, 2)
    assert 0.0 < w[0, 1] < 1.0 and g.info[2] == 0
    assert np.array_equal(m2[0, 1], mu[1]) and np.array_equal(c2[0, 1], cov[1])


def test_invalid_arguments():
    n, M, D = 2, 2, 2
    with pytest.raises(ValueError):
        GibbsParametersGmm(n, M, D, 'spherical')
    with pytest.raises(ValueError):
        GibbsParametersGmm(n, M, D, 'full', prior_w=np.ones((n, M + 1)))
    g = GibbsParametersGmm(n, M, D, 'diag', reversible=False, nsteps=1)
    packed = np.concatenate([np.ones(n * n), np.ones(n), np.zeros(n * M * (1 + 2 * D))])
    w, mu, cov = np.full((n, M), 0.5), np.zeros((n, M, D)), np.ones((n, M, D))
    g(packed, w, mu, cov, 1, 0)
    with pytest.raises(ValueError):
        g(packed[:-1], w, mu, cov, 1, 0)
    with pytest.raises(ValueError):
        g(packed, w, mu[:, :1], cov, 1, 0)
    bad = GibbsParametersGmm(n, M, D, 'diag', prior_w=-np.ones((n, M)), reversible=False, nsteps=1)
    with pytest.raises(ValueError):
        bad(packed, w, mu, cov, 1, 0)


# ---- the draw rule ---------------------------------------------------------------------------------------------
def test_draw_rule_frequencies():
    """M = 3, fixed a: the picks over 2e5 counter values against e_c / sum e, within five standard errors"""
    nd = 200000
    for a in ([-1.0, 0.5, -0.2], [3.0, -2.0, 2.5], [-700.0, -705.0, -698.5]):
        a = np.array(a)
        p = np.exp(a - a.max())
        p /= p.sum()
        g = np.arange(nd, dtype=np.uint64) + np.uint64(12345)
        pick = ref.draw_rule(np.tile(a, (nd, 1)), ref.draw_key(99), g)
        freq = np.bincount(pick, minlength=3) / nd
        assert np.all(np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / nd)), (a, freq, p)


def test_draw_rule_skips_weight_zero_and_keeps_the_first_on_nan():
    nd = 20000
    g = np.arange(nd, dtype=np.uint64)
    a = np.tile(np.array([-np.inf, 0.0, -np.inf, 0.0]), (nd, 1))
    pick = ref.draw_rule(a, ref.draw_key(1), g)
    assert set(np.unique(pick)) == {1, 3}
    assert abs((pick == 1).mean() - 0.5) <= 5 * np.sqrt(0.25 / nd)
    a = np.tile(np.array([-np.inf, np.nan, np.nan]), (nd, 1))
    assert np.all(ref.draw_rule(a, ref.draw_key(1), g) == 1)
    # one component: nothing is compared
    assert np.all(ref.draw_rule(np.zeros((nd, 1)), ref.draw_key(1), g) == 0)


def test_uniforms_restate_the_host_generator():
    """uniform01(key, x) is draw x + 1 of the host generator's u01 on the same key"""
    from tests.host_rng_ref import Rng
    r = Rng(0, 0)
    r.key = ref.draw_key(2024)
    want = np.array([r.u01() for _ in range(50)])
    got = ref.uniform01(ref.draw_key(2024), np.arange(50, dtype=np.uint64))
    assert np.array_equal(want, got)
    assert ref.draw_key(2024) != ref.draw_key(2025) and ref.draw_key(7) != 7


# ---- the numpy parameter path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
def test_numpy_rule_gives_valid_parameters(ctype):
    rng = np.random.default_rng(15)
    N, M, D = 2, 3, 3
    counts = np.array([30.0, 0.0, 12.0, 2.0, 50.0, 9.0])
    mu, cov, mom = _component_statistics(rng, N * M, D, ctype, counts)
    from bhmm_amd.output_models.gaussian_mixture import unpack_component_moments
    w0 = np.full((N, M), 1.0 / M)
    om = GaussianMixtureOutputModel(N, w0, mu.reshape(N, M, D), cov.reshape((N, M) + cov.shape[1:]),
                                    covariance_type=ctype)
    S0, S1, S2 = unpack_component_moments(mom, N, M, D, ctype)
    kept = om.sample_from_statistics(S0, S1, S2, rng=np.random.RandomState(3), weights_prior=1.0)
    assert kept == (1 if ctype == 'full' else 0)              # two points in three dimensions
    np.testing.assert_allclose(om.weights.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    assert np.all(om.weights > 0.0)
    assert np.array_equal(om.means[0, 1], mu[1])             # the empty component keeps its parameters
    for i in range(N):
        for c in range(M):
            if ctype == 'full':
                assert np.array_equal(om.covariances[i, c], om.covariances[i, c].T)
                np.linalg.cholesky(om.covariances[i, c])
            else:
                assert np.all(om.covariances[i, c] > 0.0)
    # a sparse prior: the empty component takes weight exactly 0
    om.sample_from_statistics(S0, S1, S2, rng=np.random.RandomState(4), weights_prior=0.0)
    assert om.weights[0, 1] == 0.0 and abs(om.weights[0].sum() - 1.0) <= 1e-15
    with pytest.raises(ValueError):
        om.sample_from_statistics(S0, S1, S2, weights_prior=-1.0)


# ---- the public names ------------------------------------------------------------------------------------------
def test_refusals_and_names():
    w = np.array([[0.5, 0.5], [1.0, 0.0]])
    mu = np.zeros((2, 2, 2))
    mu[1] += 3.0
    cov = np.tile(np.eye(2), (2, 2, 1, 1))
    model = bhmm_amd.gaussian_mixture_hmm([0.5, 0.5], [[0.9, 0.1], [0.1, 0.9]], w, mu, cov)
    obs = [np.zeros((10, 2))]
    with pytest.raises(NotImplementedError, match='process_group'):
        bhmm_amd.BayesianGaussianMixtureHMMSampler(obs, 2, initial_model=model, process_group=object())
    with pytest.raises(ValueError):
        bhmm_amd.BayesianGaussianMixtureHMMSampler(obs, 2)
    mv = bhmm_amd.mvgaussian_hmm([0.5, 0.5], [[0.9, 0.1], [0.1, 0.9]], [[0.0, 0.0], [3.0, 3.0]], [np.eye(2)] * 2)
    with pytest.raises(ValueError):
        bhmm_amd.BayesianGaussianMixtureHMMSampler(obs, 2, initial_model=mv)
    with pytest.raises(ValueError):
        bhmm_amd.bayesian_gaussian_mixture_hmm(obs, mv)
    for fn in (bhmm_amd.bayesian_hmm, bhmm_amd.bayesian_mvgaussian_hmm):
        with pytest.raises(NotImplementedError, match='bayesian_gaussian_mixture_hmm'):
            fn(obs, model)
