"""Host side of the gaussian-mixture emissions per state (no GPU): the layouts of par0, par1
and the per-component moment blocks, the M-step of GaussianMixtureOutputModel against plain numpy with the
starved-component rule, the generators, the initial model, the argument checks that need no device and the refusals.
"""
import os

import numpy as np
import pytest

import bhmm_amd
from bhmm_amd import _lib
from bhmm_amd.output_models.gaussian_mixture import (GaussianMixtureOutputModel, pack_component_moments,
                                                     pack_parameters, unpack_component_moments, unpack_parameters)
from bhmm_amd.output_models.mvgaussian import moment_stride

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(rng, N, M, D, ctype):
    w = rng.dirichlet(np.full(M, 2.0), N)
    mu = rng.normal(size=(N, M, D)) * 3.0
    if ctype == 'full':
        B = rng.normal(size=(N, M, D, D))
        cov = np.einsum('icab,icdb->icad', B, B) + 0.5 * np.eye(D)
    else:
        cov = rng.random((N, M, D)) + 0.5
    return w, mu, cov


@pytest.mark.parametrize("ctype", ["full", "diag"])
def test_parameter_and_moment_layouts(ctype):
    rng = np.random.default_rng(0)
    N, M, D = 3, 4, 5
    w, mu, cov = _model(rng, N, M, D, ctype)
    om = GaussianMixtureOutputModel(N, w, mu, cov, covariance_type=ctype)
    par0, par1 = om.parameters()
    assert par0.shape == (N, M, 1 + D) and par1.shape == cov.shape
    assert np.array_equal(par0[:, :, 0], w) and np.array_equal(par0[:, :, 1:], mu) and np.array_equal(par1, cov)
    w2, mu2, cov2 = unpack_parameters(*pack_parameters(w, mu, cov))
    assert np.array_equal(w2, w) and np.array_equal(mu2, mu) and np.array_equal(cov2, cov)
    om.set_parameters(par0 * 1.0, par1 * 2.0)
    assert np.array_equal(om.weights, w) and np.array_equal(om.covariances, 2.0 * cov)
    # the moment blocks: component (i, c) is block i * M + c of the layout of bhmm_mvn_moments
    S0, S1 = rng.random((N, M)), rng.normal(size=(N, M, D))
    S2 = cov * 3.0
    packed = pack_component_moments(S0, S1, S2, ctype)
    ms = moment_stride(D, ctype)
    assert packed.shape == (N * M * ms,)
    blk = packed.reshape(N, M, ms)
    assert np.array_equal(blk[:, :, 0], S0) and np.array_equal(blk[:, :, 1:1 + D], S1)
    if ctype == 'full':
        il = np.tril_indices(D)
        assert np.array_equal(blk[1, 2, 1 + D:], S2[1, 2][il])
    else:
        assert np.array_equal(blk[1, 2, 1 + D:], S2[1, 2])
    a, b, c = unpack_component_moments(packed, N, M, D, ctype)
    assert np.array_equal(a, S0) and np.array_equal(b, S1) and np.allclose(c, S2, rtol=0, atol=0)
    from bhmm_amd.engine import EStepResult
    n = N
    head = np.concatenate([[-12.5], rng.random(n), rng.random(n * n), rng.random(n)])
    res = EStepResult('gaussian_mixture', n, M, np.concatenate([head, packed]), None, D, ctype)
    assert res.loglik == -12.5 and np.array_equal(res.S0, S0) and np.array_equal(res.S1, S1)
    assert np.array_equal(res.S2, S2) and np.array_equal(res.moments, packed)
    sub = om.sub_output_model([2, 0])
    assert sub.nstates == 2 and np.array_equal(sub.means, om.means[[2, 0]]) and sub.ncomponents == M


@pytest.mark.parametrize("min_covar", [0.0, 0.01])
@pytest.mark.parametrize("ctype", ["full", "diag"])
def test_mstep_against_numpy_with_a_starved_component(ctype, min_covar):
    rng = np.random.default_rng(3)
    N, M, D, T = 2, 3, 3, 400
    w, mu, cov = _model(rng, N, M, D, ctype)
    om = GaussianMixtureOutputModel(N, w, mu, cov, covariance_type=ctype, min_covar=min_covar)
    x = rng.normal(size=(T, D)) * 2.0
    u = rng.random((T, N, M))
    u[:, 1, 2] *= 1e-10                                  # starved: far below 1e-8 of its state's weight
    S0 = u.sum(axis=0)
    d = x[:, None, None, :] - mu[None]
    S1 = (u[..., None] * d).sum(axis=0)
    S2f = (u[..., None, None] * d[..., :, None] * d[..., None, :]).sum(axis=0)
    S2 = S2f if ctype == 'full' else np.einsum('icaa->ica', S2f).copy()
    om.estimate_from_statistics(S0, S1, S2)
    np.testing.assert_allclose(om.weights, S0 / S0.sum(axis=1)[:, None], rtol=1e-14)
    assert om.weights[1, 2] < 1e-8
    for i in range(N):
        for c in range(M):
            if (i, c) == (1, 2):
                assert np.array_equal(om.means[i, c], mu[i, c]) and np.array_equal(om.covariances[i, c], cov[i, c])
                continue
            m1 = (u[:, i, c, None] * x).sum(axis=0) / S0[i, c]
            dd = x - m1
            c1 = (u[:, i, c, None, None] * dd[:, :, None] * dd[:, None, :]).sum(axis=0) / S0[i, c] + min_covar * np.eye(D)
            np.testing.assert_allclose(om.means[i, c], m1, rtol=1e-11, atol=1e-12)
            got = om.covariances[i, c]
            np.testing.assert_allclose(got, c1 if ctype == 'full' else np.diag(c1), rtol=1e-10, atol=1e-11)
    # a state without any weight fails as it does for one gaussian per state
    S0z = S0.copy()
    S0z[0] = 0.0
    with pytest.raises(RuntimeError):
        om.estimate_from_statistics(S0z, S1, S2)
    with pytest.raises(ValueError):
        om.estimate_from_statistics(S0[:, :2], S1, S2)
    with pytest.raises(ValueError):
        om.estimate_from_packed(np.zeros(7))


def test_generators_draw_from_the_right_components():
    rng = np.random.default_rng(5)
    N, M, D = 2, 3, 2
    w = np.array([[0.2, 0.5, 0.3], [0.6, 0.0, 0.4]])
    mu = np.zeros((N, M, D))
    mu[:, :, 0] = 100.0 * np.arange(M)[None, :]
    mu[:, :, 1] = 1000.0 * np.arange(N)[:, None]
    cov = np.array([[np.eye(D)] * M] * N)
    om = GaussianMixtureOutputModel(N, w, mu, cov)
    n = 20000
    for i in range(N):
        x, comp = om.generate_observations_from_state(i, n, rng=rng, return_components=True)
        assert x.shape == (n, D)
        near = np.rint(x[:, 0] / 100.0).astype(np.int64)
        assert np.array_equal(near, comp) and np.all(np.abs(x[:, 1] - 1000.0 * i) < 10.0)
        share = np.bincount(comp, minlength=M) / n
        se = np.sqrt(w[i] * (1.0 - w[i]) / n)
        assert np.all(np.abs(share - w[i]) <= 4.0 * se)
        for c in range(M):
            if w[i, c] > 0:
                np.testing.assert_allclose(x[comp == c].mean(axis=0), mu[i, c], atol=5.0 / np.sqrt(n * w[i, c]))
    s = rng.integers(0, N, 500)
    traj = om.generate_observation_trajectory(s, rng=rng)
    assert traj.shape == (500, D) and np.array_equal(np.rint(traj[:, 1] / 1000.0).astype(np.int64), s)
    assert om.generate_observation_from_state(1, rng=rng).shape == (D,)


@pytest.mark.parametrize("ctype", ["full", "diag"])
def test_init_model_is_deterministic_and_valid(ctype):
    rng = np.random.default_rng(2)
    D, M = 3, 3
    blobs = [np.array([-10.0, -3.0, 0.0]), np.array([-10.0, 3.0, 0.0]), np.array([10.0, 0.0, -3.0]),
             np.array([10.0, 0.0, 3.0])]
    obs = [np.concatenate([b + rng.normal(size=(120, D)) for b in blobs]), blobs[0] + rng.normal(size=(50, D))]
    a = bhmm_amd.init_gaussian_mixture_hmm(obs, 2, M, covariance_type=ctype)
    b = bhmm_amd.init_gaussian_mixture_hmm(obs, 2, M, covariance_type=ctype)
    for om in (a.output_model,):
        assert om.model_type == 'gaussian_mixture' and om.ncomponents == M and om.dimension == D
        assert om.weights.shape == (2, M) and np.all(om.weights >= 1e-3 / (1 + M * 1e-3))
        np.testing.assert_allclose(om.weights.sum(axis=1), 1.0, rtol=1e-14)
        cv = om.covariances if ctype == 'diag' else np.linalg.eigvalsh(om.covariances)
        assert np.all(cv > 0)
    for x, y in ((a.output_model.weights, b.output_model.weights), (a.output_model.means, b.output_model.means),
                 (a.output_model.covariances, b.output_model.covariances), (a.transition_matrix, b.transition_matrix)):
        assert np.array_equal(x, y)
    # the two states are the two sides, their components the blobs of a side
    assert np.all(a.output_model.means[0, :, 0] < 0) and np.all(a.output_model.means[1, :, 0] > 0)
    # a state with fewer than M (D + 1) points: still valid weights and positive-definite covariances
    few = [np.concatenate([blobs[0] + rng.normal(size=(200, D)), blobs[2] + rng.normal(size=(7, D))])]
    h = bhmm_amd.init_gaussian_mixture_hmm(few, 2, M, covariance_type=ctype)
    om = h.output_model
    np.testing.assert_allclose(om.weights.sum(axis=1), 1.0, rtol=1e-14)
    assert np.all(om.weights > 0) and np.all(np.isfinite(om.means))
    cv = om.covariances if ctype == 'diag' else np.linalg.eigvalsh(om.covariances)
    assert np.all(cv > 0)
    assert bhmm_amd.init_hmm(obs, 2, output='gaussian_mixture', ncomponents=2).output_model.ncomponents == 2
    assert bhmm_amd.init_hmm(obs, 2).output_model.model_type == 'mvgaussian'       # (never guessed)
    with pytest.raises(ValueError):
        bhmm_amd.init_hmm(obs, 2, output='gaussian_mixture')


def test_output_model_shapes():
    N, M, D = 2, 2, 2
    w, mu, cov = np.full((N, M), 0.5), np.zeros((N, M, D)), np.array([[np.eye(D)] * M] * N)
    GaussianMixtureOutputModel(N, w, mu, cov)
    GaussianMixtureOutputModel(N, w, mu, np.ones((N, M, D)), covariance_type='diag')
    for bad in (dict(weights=np.full((N, M), 0.6)), dict(weights=np.array([[1.5, -0.5], [0.5, 0.5]])),
                dict(weights=np.full((N, 3), 1.0 / 3)), dict(means=np.zeros((N, D))), dict(covariances=np.ones((N, M, D))),
                dict(covariance_type='tied'), dict(min_covar=-1.0), dict(means=np.zeros((N, M, 65)))):
        kw = dict(weights=w, means=mu, covariances=cov)
        kw.update(bad)
        with pytest.raises(ValueError):
            GaussianMixtureOutputModel(N, **kw)
    with pytest.raises(ValueError):                     # N M > 4096
        GaussianMixtureOutputModel(N, np.full((N, 2049), 1.0 / 2049), np.zeros((N, 2049, 1)), np.ones((N, 2049, 1)),
                                   covariance_type='diag')


def test_new_symbols_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "bhmm_amd.h")).read()
    L = _lib.load()
    for name in ("bhmm_gmm_emissions", "bhmm_gmm_fetch_resp", "bhmm_gmm_moments", "bhmm_logpdf_gmm"):
        assert "int %s(" % name in text, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    assert bhmm_amd.GmmEngine.__mro__[1] is bhmm_amd.MvnEngine


def test_device_entry_points_check_their_arguments_without_a_device():
    L = _lib.load()
    assert L.bhmm_gmm_emissions(None, 1, None, None, None, 0, 0) == _lib.ERR_INVALID
    assert L.bhmm_gmm_fetch_resp(None, None) == _lib.ERR_INVALID
    assert L.bhmm_gmm_moments(None, None, None, 0, None) == _lib.ERR_INVALID
    x, out = np.zeros((4, 2)), np.zeros((4, 1))
    mu, cov = np.zeros((1, 2, 2)), np.array([[np.eye(2)] * 2])

    def call(w, M=2, cov=cov, N=1):
        return L.bhmm_logpdf_gmm(_lib.dp(out), _lib.dp(x), 4, 2, N, M, _lib.dp(np.asarray(w, dtype=np.float64)),
                                 _lib.dp(mu), _lib.dp(cov), 0)
    assert call([0.5, 0.6]) == _lib.ERR_INVALID                     # does not sum to 1
    assert call([0.5, 0.5 + 1e-7]) == _lib.ERR_INVALID              # (1e-8 is the tolerance)
    assert call([1.5, -0.5]) == _lib.ERR_INVALID                    # negative
    assert call([0.5, np.nan]) == _lib.ERR_INVALID
    assert call([0.5, 0.5], M=0) == _lib.ERR_INVALID
    assert call([0.5, 0.5], M=4097) == _lib.ERR_INVALID             # N M > 4096
    bad = cov.copy()
    bad[0, 1] = [[1.0, 2.0], [2.0, 1.0]]
    assert call([0.5, 0.5], cov=bad) == _lib.ERR_SIGMA
    assert b"sum to 1" in L.bhmm_last_error() or call([0.5, 0.6]) == _lib.ERR_INVALID


def test_refusals_that_need_no_device():
    N, M, D = 2, 2, 2
    model = bhmm_amd.gaussian_mixture_hmm(np.ones(N) / N, np.full((N, N), 0.5), np.full((N, M), 0.5),
                                          np.zeros((N, M, D)), np.array([[np.eye(D)] * M] * N))
    assert model.output_model.model_type == 'gaussian_mixture'
    obs = [np.zeros((10, D))]
    with pytest.raises(NotImplementedError, match='process_group'):
        bhmm_amd.MaximumLikelihoodEstimator(obs, N, initial_model=model, process_group=object())
    with pytest.raises(NotImplementedError, match='float64'):
        bhmm_amd.MaximumLikelihoodEstimator(obs, N, initial_model=model, estep_precision='mixed')
    with pytest.raises(NotImplementedError, match='Gibbs'):
        bhmm_amd.bayesian_hmm(obs, model)
    with pytest.raises(NotImplementedError, match='Gibbs'):
        bhmm_amd.bayesian_mvgaussian_hmm(obs, model)
    with pytest.raises(NotImplementedError, match='Gibbs'):
        bhmm_amd.BayesianHMMSampler(obs, N, initial_model=model)
    with pytest.raises(ValueError):
        bhmm_amd.MaximumLikelihoodEstimator(obs, N, initial_model=model, ncomponents=3)
    mv = bhmm_amd.mvgaussian_hmm(np.ones(N) / N, np.full((N, N), 0.5), np.zeros((N, D)), np.array([np.eye(D)] * N))
    with pytest.raises(ValueError):
        bhmm_amd.MaximumLikelihoodEstimator(obs, N, initial_model=mv, ncomponents=2)
