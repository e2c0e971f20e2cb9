"""Host side of the multivariate gaussian emissions (no GPU): bhmm_host_mvn_prepare, bhmm_host_mvn_mstep, the packed
moment layout, the output model's shape validation, the initial model, and the stand-alone sanitizer run of the two
host functions.  The yardsticks are numpy (np.linalg.cholesky, the two-pass weighted mean / covariance)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bhmm_amd
from bhmm_amd import _lib
from bhmm_amd.output_models.mvgaussian import (MultivariateGaussianOutputModel, moment_stride, pack_moments,
                                               unpack_moments)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def _rand_cov(rng, D, scale=1.0, kappa=1e3):
    """a covariance whose Cholesky factor has condition number about kappa"""
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    s = scale * np.logspace(0, -np.log10(kappa), D) if D > 1 else np.array([scale])
    Lm = Q * s[None, :]
    S = Lm.dot(Lm.T)
    return 0.5 * (S + S.T)


def _prepare(covs, cov_type, N, D):
    L = _lib.load()
    full = cov_type == _lib.COV_FULL
    chol = np.zeros((N, D, D) if full else (N, D))
    winv = np.zeros((N, D * (D + 1) // 2 if full else D))
    cst = np.zeros(N)
    rc = L.bhmm_host_mvn_prepare(N, D, cov_type, _lib.dp(_lib.f64(covs)), _lib.dp(chol), _lib.dp(winv), _lib.dp(cst))
    return rc, chol, winv, cst


@pytest.mark.parametrize("D", [1, 2, 3, 8, 17, 64])
def test_prepare_full_matches_numpy_cholesky(D):
    rng = np.random.default_rng(D)
    N = 3
    covs = np.array([_rand_cov(rng, D, scale=10.0 ** rng.uniform(-2, 2)) for _ in range(N)])
    rc, chol, winv, cst = _prepare(covs, _lib.COV_FULL, N, D)
    assert rc == _lib.OK
    il = np.tril_indices(D)
    for i in range(N):
        ref = np.linalg.cholesky(covs[i])
        kappa = np.linalg.cond(ref)
        # the Cholesky factor of a perturbed matrix: relative change <= about D * eps * kappa(L)^2 / sqrt 2 (Sun 1991);
        # numpy's own factor carries that error, the long double one a fraction of it
        assert np.abs(chol[i] - ref).max() <= 8 * D * EPS * kappa ** 2 * np.abs(ref).max()
        assert np.all(np.triu(chol[i], 1) == 0.0)
        W = np.zeros((D, D))
        W[il] = winv[i]
        assert np.abs(W.dot(chol[i]) - np.eye(D)).max() <= 8 * D * EPS * kappa
        want = -np.log(np.diag(ref)).sum() - 0.5 * D * np.log(2 * np.pi)
        assert abs(cst[i] - want) <= 16 * D * EPS * max(1.0, abs(want)) * kappa


def test_prepare_diag():
    rng = np.random.default_rng(1)
    N, D = 4, 5
    var = 10.0 ** rng.uniform(-4, 4, (N, D))
    rc, chol, winv, cst = _prepare(var, _lib.COV_DIAG, N, D)
    assert rc == _lib.OK
    np.testing.assert_allclose(chol, np.sqrt(var), rtol=2 * EPS)
    np.testing.assert_allclose(winv, 1.0 / np.sqrt(var), rtol=4 * EPS)
    np.testing.assert_allclose(cst, -0.5 * np.log(var).sum(axis=1) - 0.5 * D * np.log(2 * np.pi), rtol=1e-14)


def test_prepare_refuses_bad_covariances():
    N, D = 2, 3
    good = np.array([np.eye(D), np.eye(D)])
    bad = good.copy()
    bad[1, 2, 2] = -1.0                                   # not positive definite
    assert _prepare(bad, _lib.COV_FULL, N, D)[0] == _lib.ERR_SIGMA
    bad = good.copy()
    bad[1] = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])   # symmetric, indefinite
    assert _prepare(bad, _lib.COV_FULL, N, D)[0] == _lib.ERR_SIGMA
    bad = good.copy()
    bad[0, 0, 1] = 0.5                                    # not symmetric
    assert _prepare(bad, _lib.COV_FULL, N, D)[0] == _lib.ERR_INVALID
    for v in (np.nan, np.inf):
        bad = good.copy()
        bad[0, 1, 1] = v
        assert _prepare(bad, _lib.COV_FULL, N, D)[0] == _lib.ERR_INVALID
    assert _prepare(np.array([[1.0, 0.0, 1.0], [1.0, 1.0, 1.0]]), _lib.COV_DIAG, N, D)[0] == _lib.ERR_SIGMA
    assert _prepare(np.array([[1.0, np.nan, 1.0], [1.0, 1.0, 1.0]]), _lib.COV_DIAG, N, D)[0] == _lib.ERR_INVALID
    L = _lib.load()
    assert L.bhmm_host_mvn_prepare(N, 65, 0, _lib.dp(np.zeros(N * 65 * 65)), None, None, None) == _lib.ERR_INVALID
    assert L.bhmm_host_mvn_prepare(N, D, 2, _lib.dp(good), None, None, None) == _lib.ERR_INVALID
    assert L.bhmm_host_mvn_prepare(N, D, 0, None, None, None, None) == _lib.ERR_INVALID
    assert b"covs" in L.bhmm_last_error()


def _two_pass(x, g, ctype, min_covar):
    """the M-step as the definition has it: weighted mean, then the weighted covariance about it"""
    N, D = g.shape[1], x.shape[1]
    mu = np.empty((N, D))
    cov = np.empty((N, D, D))
    for i in range(N):
        w = g[:, i]
        mu[i] = (w[:, None] * x).sum(axis=0) / w.sum()
        d = x - mu[i]
        cov[i] = (w[:, None, None] * d[:, :, None] * d[:, None, :]).sum(axis=0) / w.sum() + min_covar * np.eye(D)
    if ctype == 'diag':
        cov = np.array([np.diag(c) for c in cov])
    return mu, cov


def _moments(x, g, mu_old, ctype):
    N, D = g.shape[1], x.shape[1]
    S0 = g.sum(axis=0)
    S1 = np.empty((N, D))
    S2 = np.empty((N, D, D))
    for i in range(N):
        d = x - mu_old[i]
        S1[i] = (g[:, i, None] * d).sum(axis=0)
        S2[i] = (g[:, i, None, None] * d[:, :, None] * d[:, None, :]).sum(axis=0)
    if ctype == 'diag':
        S2 = np.array([np.diag(c) for c in S2])
    return S0, S1, S2


@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("min_covar", [0.0, 0.25])
def test_mstep_matches_two_pass_formula(ctype, min_covar):
    rng = np.random.default_rng(5)
    T, N, D = 400, 3, 4
    x = rng.normal(size=(T, D)) * np.array([1.0, 3.0, 0.2, 10.0]) + 5.0
    g = rng.random((T, N))
    g /= g.sum(axis=1)[:, None]
    mu_old = rng.normal(size=(N, D)) + 5.0
    cov_old = np.array([np.eye(D)] * N) if ctype == 'full' else np.ones((N, D))
    om = MultivariateGaussianOutputModel(N, mu_old, cov_old, covariance_type=ctype, min_covar=min_covar)
    om.estimate_from_statistics(*_moments(x, g, mu_old, ctype))
    mu, cov = _two_pass(x, g, ctype, min_covar)
    # moments about a mean a few sigma off: cancellation of delta delta^T against S2 / S0 costs |delta|^2 / var
    np.testing.assert_allclose(om.means, mu, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(om.covariances, cov, rtol=1e-10, atol=1e-10)
    if ctype == 'full':
        assert np.array_equal(om.covariances, om.covariances.transpose(0, 2, 1))


def test_mstep_refuses_a_degenerate_state():
    N, D = 2, 2
    om = MultivariateGaussianOutputModel(N, np.zeros((N, D)), np.array([np.eye(D)] * N))
    S0 = np.array([10.0, 10.0])
    S1 = np.zeros((N, D))
    S2 = np.array([np.eye(D) * 10.0, np.array([[10.0, 10.0], [10.0, 10.0]])])    # state 1: rank one
    with pytest.raises(RuntimeError):
        om.estimate_from_statistics(S0, S1, S2)
    om = MultivariateGaussianOutputModel(N, np.zeros((N, D)), np.array([np.eye(D)] * N), min_covar=1e-3)
    om.estimate_from_statistics(S0, S1, S2)            # min_covar makes it definite
    assert np.linalg.eigvalsh(om.covariances[1]).min() > 0
    om = MultivariateGaussianOutputModel(N, np.zeros((N, D)), np.array([np.eye(D)] * N))
    with pytest.raises(RuntimeError):                   # a state without weight
        om.estimate_from_statistics(np.array([10.0, 0.0]), S1, np.array([np.eye(D) * 10.0, np.zeros((D, D))]))


def test_packed_layout():
    assert moment_stride(1, 'full') == 3 and moment_stride(1, 'diag') == 3
    assert moment_stride(3, 'full') == 1 + 3 + 6 and moment_stride(3, 'diag') == 1 + 3 + 3
    assert moment_stride(64, 'full') == 1 + 64 + 2080 and moment_stride(64, 'diag') == 129
    with pytest.raises(ValueError):
        moment_stride(3, 'tied')
    rng = np.random.default_rng(0)
    N, D = 2, 3
    S0, S1 = rng.random(N), rng.random((N, D))
    S2 = rng.random((N, D, D))
    S2 = S2 + S2.transpose(0, 2, 1)
    p = pack_moments(S0, S1, S2, 'full')
    assert p.shape == (N * 10,)
    # per state: S0, S1, then the lower triangle row by row
    assert p[0] == S0[0] and np.array_equal(p[1:4], S1[0])
    assert np.array_equal(p[4:10], [S2[0, 0, 0], S2[0, 1, 0], S2[0, 1, 1], S2[0, 2, 0], S2[0, 2, 1], S2[0, 2, 2]])
    for a, b in zip(unpack_moments(p, N, D, 'full'), (S0, S1, S2)):
        assert np.array_equal(a, b)
    Sd = rng.random((N, D))
    p = pack_moments(S0, S1, Sd, 'diag')
    assert p.shape == (N * 7,) and np.array_equal(p[4:7], Sd[0])
    for a, b in zip(unpack_moments(p, N, D, 'diag'), (S0, S1, Sd)):
        assert np.array_equal(a, b)
    from bhmm_amd.engine import EStepResult
    n = 2
    packed = np.concatenate([np.arange(1 + n + n * n + n, dtype=np.float64), pack_moments(S0, S1, S2, 'full')])
    res = EStepResult('mvgaussian', n, 0, packed, None, D, 'full')
    assert np.array_equal(res.S0, S0) and np.array_equal(res.S1, S1) and np.array_equal(res.S2, S2)
    assert res.loglik == 0.0 and res.C.shape == (n, n)


def test_output_model_shapes():
    N, D = 3, 2
    mu, cov = np.zeros((N, D)), np.array([np.eye(D)] * N)
    om = MultivariateGaussianOutputModel(N, mu, cov)
    assert om.model_type == 'mvgaussian' and om.dimension == D and om.covariance_type == 'full'
    assert om.parameters()[0].shape == (N, D) and om.parameters()[1].shape == (N, D, D)
    assert MultivariateGaussianOutputModel(N, mu, np.ones((N, D)), covariance_type='diag').parameters()[1].shape == (N, D)
    sub = om.sub_output_model([0, 2])
    assert sub.nstates == 2 and sub.means.shape == (2, D) and sub.covariances.shape == (2, D, D)
    for bad in (lambda: MultivariateGaussianOutputModel(N, np.zeros(N), cov),
                lambda: MultivariateGaussianOutputModel(N, np.zeros((N + 1, D)), cov),
                lambda: MultivariateGaussianOutputModel(N, mu, np.ones((N, D))),
                lambda: MultivariateGaussianOutputModel(N, mu, cov, covariance_type='diag'),
                lambda: MultivariateGaussianOutputModel(N, mu, cov, covariance_type='tied'),
                lambda: MultivariateGaussianOutputModel(N, mu, cov, min_covar=-1.0),
                lambda: MultivariateGaussianOutputModel(N, np.zeros((N, 65)), np.ones((N, 65)), covariance_type='diag'),
                lambda: om.estimate_from_statistics(np.ones(N), np.zeros((N, D)), np.ones((N, D))),
                lambda: om.estimate_from_packed(np.zeros(5))):
        with pytest.raises(ValueError):
            bad()
    om.set_parameters(np.ones(N * D), np.stack([2 * np.eye(D)] * N).ravel())
    assert om.means.shape == (N, D) and om.covariances[1, 1, 1] == 2.0
    rng = np.random.RandomState(0)
    assert om.generate_observation_from_state(1, rng=rng).shape == (D,)
    assert om.generate_observations_from_state(1, 7, rng=rng).shape == (7, D)
    assert om.generate_observation_trajectory(np.array([0, 1, 2, 2, 0]), rng=rng).shape == (5, D)
    model = bhmm_amd.mvgaussian_hmm(np.ones(N) / N, np.eye(N), mu, cov)
    assert model.output_model.model_type == 'mvgaussian' and model.nstates == N
    from bhmm_amd.api import _guess_output_type
    assert _guess_output_type([np.zeros((4, 2))]) == 'mvgaussian'
    assert _guess_output_type([np.zeros(4)]) == 'gaussian'


def _clusters(seed=0, T=3000):
    rng = np.random.default_rng(seed)
    centres = np.array([[-10.0, 0.0], [0.0, 12.0], [10.0, -3.0]])
    P = np.array([[0.9, 0.05, 0.05], [0.05, 0.9, 0.05], [0.05, 0.05, 0.9]])
    obs = []
    for _ in range(2):
        s = np.empty(T, dtype=np.int64)
        s[0] = 0
        u = rng.random(T)
        for t in range(1, T):
            s[t] = np.searchsorted(np.cumsum(P[s[t - 1]]), u[t])
        obs.append(centres[s] + rng.normal(size=(T, 2)))
    return obs, centres, P


@pytest.mark.parametrize("ctype", ["full", "diag"])
def test_init_model_is_deterministic_and_finds_the_clusters(ctype):
    obs, centres, P = _clusters()
    a = bhmm_amd.init_mvgaussian_hmm(obs, 3, covariance_type=ctype)
    b = bhmm_amd.init_mvgaussian_hmm(obs, 3, covariance_type=ctype)
    for x, y in ((a.transition_matrix, b.transition_matrix), (a.initial_distribution, b.initial_distribution),
                 (a.output_model.means, b.output_model.means), (a.output_model.covariances, b.output_model.covariances)):
        assert np.array_equal(x, y)
    # states ordered by the first coordinate, as the generating centres are; 2000 points per cluster, sigma 1
    assert np.abs(a.output_model.means - centres).max() < 0.15
    cov = a.output_model.covariances
    assert cov.shape == ((3, 2, 2) if ctype == 'full' else (3, 2))
    np.testing.assert_allclose(cov if ctype == 'diag' else np.array([np.diag(c) for c in cov]), 1.0, atol=0.15)
    np.testing.assert_allclose(a.transition_matrix, P, atol=0.03)
    np.testing.assert_allclose(a.transition_matrix.sum(axis=1), 1.0, rtol=1e-12)
    assert bhmm_amd.init_hmm(obs, 3).output_model.model_type == 'mvgaussian'


def test_new_symbols_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "bhmm_amd.h")).read()
    L = _lib.load()
    for name in ("bhmm_ctx_set_observations_mvn", "bhmm_mvn_emissions", "bhmm_mvn_fetch_scale", "bhmm_mvn_fetch_rows",
                 "bhmm_mvn_moments", "bhmm_logpdf_mvn", "bhmm_host_mvn_prepare", "bhmm_host_mvn_mstep"):
        assert "int %s(" % name in text, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    assert _lib.COV_FULL == 0 and _lib.COV_DIAG == 1 and _lib.MVN_MAX_D == 64
    for macro in ("BHMM_COV_FULL 0", "BHMM_COV_DIAG 1", "BHMM_MVN_MAX_D 64"):
        assert "#define " + macro in text


def test_device_entry_points_refuse_without_observations():
    """argument validation that needs no device"""
    L = _lib.load()
    assert L.bhmm_mvn_emissions(None, None, None, 0) == _lib.ERR_INVALID
    assert L.bhmm_mvn_fetch_scale(None, None, None) == _lib.ERR_INVALID
    assert L.bhmm_mvn_moments(None, None, None, 0, None) == _lib.ERR_INVALID
    x = np.zeros((4, 2))
    assert L.bhmm_logpdf_mvn(None, _lib.dp(x), 4, 2, 1, _lib.dp(np.zeros(2)), _lib.dp(np.eye(2)), 0) == _lib.ERR_INVALID
    out = np.zeros((4, 1))
    assert L.bhmm_logpdf_mvn(_lib.dp(out), _lib.dp(np.zeros((4, 65))), 4, 65, 1, _lib.dp(np.zeros(65)),
                             _lib.dp(np.ones(65)), 1) == _lib.ERR_INVALID
    assert L.bhmm_logpdf_mvn(_lib.dp(out), _lib.dp(x), 4, 2, 1, _lib.dp(np.zeros(2)),
                             _lib.dp(np.array([[1.0, 2.0], [2.0, 1.0]])), 0) == _lib.ERR_SIGMA


def test_estimator_refuses_what_this_kind_does_not_do():
    N, D = 2, 2
    model = bhmm_amd.mvgaussian_hmm(np.ones(N) / N, np.full((N, N), 0.5), np.zeros((N, D)), np.array([np.eye(D)] * N))
    obs = [np.zeros((10, D))]
    with pytest.raises(NotImplementedError):
        bhmm_amd.MaximumLikelihoodEstimator(obs, N, initial_model=model, process_group=object())
    with pytest.raises(NotImplementedError):
        bhmm_amd.MaximumLikelihoodEstimator(obs, N, initial_model=model, estep_precision='mixed')
    with pytest.raises(NotImplementedError):
        bhmm_amd.bayesian_hmm(obs, model)


SAN_DRIVER = r"""
#include <math.h>
#include <stdio.h>
#include <vector>
#include "include/bhmm_amd.h"
int main()
{
    int bad = 0;
    for (int cov_type = 0; cov_type < 2; ++cov_type)
        for (int D : {1, 2, 7, 64}) {
            const int N = 3;
            const size_t cs = cov_type ? D : (size_t)D * D, fs = cov_type ? D : (size_t)D * (D + 1) / 2;
            std::vector<double> covs(N * cs, 0.0), chol(N * cs), winv(N * fs), cst(N);
            for (int i = 0; i < N; ++i)
                for (int a = 0; a < D; ++a) {
                    if (cov_type) {
                        covs[i * cs + a] = 1.0 + a + i;
                    } else {
                        for (int b = 0; b < D; ++b)
                            covs[i * cs + (size_t)a * D + b] = (a == b ? D + 1.0 + i : 0.0) + 1.0 / (1.0 + a + b);
                    }
                }
            bad += bhmm_host_mvn_prepare(N, D, cov_type, covs.data(), chol.data(), winv.data(), cst.data()) != BHMM_OK;
            bad += bhmm_host_mvn_prepare(N, D, cov_type, covs.data(), nullptr, nullptr, nullptr) != BHMM_OK;
            const size_t ms = 1 + D + fs;
            std::vector<double> mom(N * ms, 0.0), mu(N * D, 1.0), mu2(N * D), cov2(N * cs);
            for (int i = 0; i < N; ++i) {
                mom[i * ms] = 10.0;
                for (int a = 0; a < D; ++a) {
                    mom[i * ms + 1 + a] = 0.5 * a;
                    mom[i * ms + 1 + D + (cov_type ? a : (size_t)a * (a + 1) / 2 + a)] = 100.0 * D * D;
                }
            }
            bad += bhmm_host_mvn_mstep(N, D, cov_type, mom.data(), mu.data(), 0.01, mu2.data(), cov2.data()) != BHMM_OK;
            mom[0] = 0.0; // a state without weight
            bad += bhmm_host_mvn_mstep(N, D, cov_type, mom.data(), mu.data(), 0.0, mu2.data(), cov2.data()) != BHMM_ERR_SIGMA;
            covs[0] = -1.0;
            bad += bhmm_host_mvn_prepare(N, D, cov_type, covs.data(), chol.data(), winv.data(), cst.data()) != BHMM_ERR_SIGMA;
            covs[0] = NAN;
            bad += bhmm_host_mvn_prepare(N, D, cov_type, covs.data(), chol.data(), winv.data(), cst.data()) != BHMM_ERR_INVALID;
        }
    printf("mvn host sanitizer run: %d failures\n", bad);
    return bad != 0;
}
"""


def test_host_functions_under_the_sanitizers(tmp_path):
    """The two host functions in a stand-alone program built with -fsanitize=address,undefined from the same sources
    as the host sanitizer build (host_model.cpp, host_api.cpp, host_rev_avx2.cpp)."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "bhmm_amd", "csrc")
    drv = tmp_path / "mvn_san.cpp"
    # (invalid_arg / set_error live in the device unit of the library: the driver brings its own)
    drv.write_text('#include <string>\nnamespace bhmm { static std::string g; int invalid_arg(const std::string &m) '
                   '{ g = m; return 3; } void set_error(const std::string &m) { g = m; } }\n' + SAN_DRIVER)
    exe = str(tmp_path / "mvn_san")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    avx = str(tmp_path / "host_rev_avx2.o")
    subprocess.check_call([cxx] + san + ["-std=c++17", "-ffp-contract=off", "-mavx2", "-mfma", "-c", "-o", avx,
                                         os.path.join(csrc, "host_rev_avx2.cpp")])
    subprocess.check_call([cxx] + san + ["-std=c++17", "-ffp-contract=off", "-I", ROOT, "-o", exe, str(drv),
                                         os.path.join(csrc, "host_model.cpp"), os.path.join(csrc, "host_api.cpp"), avx,
                                         "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "0 failures" in out.stdout
