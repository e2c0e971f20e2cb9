"""Host side of the Poisson count emissions (no GPU): bhmm_host_pois_mstep, PoissonOutputModel, the guess of the
output type, the initial model, the three symbols of the C ABI, the refusals that need no device, and the stand-alone
sanitizer run of the host M-step.  The yardsticks are numpy and math.lgamma."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import bhmm_amd
from bhmm_amd import _lib
from bhmm_amd.api import _guess_output_type
from bhmm_amd.output_models.poisson import PoissonOutputModel, check_observation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUE_RATES = np.array([[0.3, 1.0], [5.0, 2.0], [20.0, 30.0]])


def _mstep(moments, rates):
    N, D = rates.shape
    new = np.full((N, D), np.nan)
    rc = _lib.load().bhmm_host_pois_mstep(N, D, _lib.dp(_lib.f64(moments)), _lib.dp(_lib.f64(rates)), _lib.dp(new))
    return rc, new


def _packed(S0, S1, S2=None):
    N, D = S1.shape
    m = np.zeros((N, 1 + 2 * D))
    m[:, 0] = S0
    m[:, 1:1 + D] = S1
    m[:, 1 + D:] = np.nan if S2 is None else S2      # (never read)
    return m.ravel()


# ---- M-step -------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(1, 1), (3, 2), (4, 7), (2, 64)])
def test_mstep_is_the_weighted_mean_of_the_counts(N, D):
    rng = np.random.default_rng(100 * N + D)
    T = 400
    rates = rng.uniform(0.2, 20.0, (N, D))
    x = rng.poisson(rates[rng.integers(0, N, T)]).astype(np.float64)
    g = rng.random((T, N))
    g /= g.sum(axis=1)[:, None]
    S0 = g.sum(axis=0)
    S1 = np.array([(g[:, i, None] * (x - rates[i])).sum(axis=0) for i in range(N)])
    rc, new = _mstep(_packed(S0, S1), rates)
    assert rc == _lib.OK
    want = g.T.dot(x) / S0[:, None]                  # sum gamma x / sum gamma
    np.testing.assert_allclose(new, want, rtol=1e-12)


def test_mstep_state_without_weight_keeps_its_rates_and_negative_rounds_to_zero():
    rates = np.array([[1.5, 0.25], [3.0, 7.0], [1e-17, 2.0]])
    S0 = np.array([4.0, 0.0, 2.0])
    # state 2, channel 0: every count was 0, S1 = -S0 * lambda, and lambda + S1 / S0 may round below zero
    S1 = np.array([[2.0, -0.5], [123.0, -5.0], [-2.0 * 1e-17 * (1 + 2 ** -50), 1.0]])
    rc, new = _mstep(_packed(S0, S1), rates)
    assert rc == _lib.OK
    np.testing.assert_allclose(new[0], [2.0, 0.125], rtol=1e-12)
    assert np.array_equal(new[1], rates[1])          # S0 = 0: kept, nothing degenerate
    assert new[2, 0] == 0.0 and not np.signbit(new[2, 0])
    assert rates[2, 0] + S1[2, 0] / S0[2] < 0.0      # (the case is what it says)
    np.testing.assert_allclose(new[2, 1], 2.5, rtol=1e-12)


def test_mstep_refuses_bad_arguments():
    L = _lib.load()
    z = np.zeros(5)
    assert L.bhmm_host_pois_mstep(1, 1, None, None, None) == _lib.ERR_INVALID
    assert L.bhmm_host_pois_mstep(0, 1, _lib.dp(z), _lib.dp(z), _lib.dp(z)) == _lib.ERR_INVALID
    assert L.bhmm_host_pois_mstep(1, 65, _lib.dp(z), _lib.dp(z), _lib.dp(z)) == _lib.ERR_INVALID


# ---- output model -----------------------------------------------------------------------------
def test_output_model_shapes_and_refusals():
    om = PoissonOutputModel(3, TRUE_RATES)
    assert om.model_type == 'poisson' and om.dimension == 2 and om.nstates == 3
    assert np.array_equal(om.rates, TRUE_RATES)
    par0, par1 = om.parameters()
    assert np.array_equal(par0, TRUE_RATES) and par1 is None
    om.set_parameters(TRUE_RATES[::-1], None)
    assert np.array_equal(om.rates, TRUE_RATES[::-1])
    sub = om.sub_output_model([2, 0])
    assert sub.nstates == 2 and np.array_equal(sub.rates, om.rates[[2, 0]])
    with pytest.raises(ValueError):
        PoissonOutputModel(3, [[1.0, 2.0], [3.0, -0.1], [1.0, 1.0]])      # negative rate
    with pytest.raises(ValueError):
        PoissonOutputModel(3, [[1.0, 2.0], [3.0, np.inf], [1.0, 1.0]])
    with pytest.raises(ValueError):
        PoissonOutputModel(2, TRUE_RATES)                                 # wrong number of states
    with pytest.raises(ValueError):
        PoissonOutputModel(1, np.ones((1, 65)))
    with pytest.raises(ValueError):
        om.log_p_obs(np.array([[1.0, 0.5]]))                              # fractional count
    with pytest.raises(ValueError):
        om.log_p_obs(np.array([[1, -1]]))                                 # negative count
    with pytest.raises(ValueError):
        om.log_p_obs(np.zeros((4, 3)))                                    # wrong D
    with pytest.raises(ValueError):
        om.log_p_obs(np.zeros(4))
    x = check_observation(np.array([[0, 3], [2, 1]], dtype=np.int32))
    assert x.dtype == np.float64 and x.shape == (2, 2) and x.flags.c_contiguous
    assert np.array_equal(check_observation(np.array([[0.0, 3.0]])), [[0.0, 3.0]])
    model = bhmm_amd.poisson_hmm(np.ones(3) / 3, np.full((3, 3), 1.0 / 3), TRUE_RATES)
    assert model.output_model.model_type == 'poisson' and model.nstates == 3


def test_log_p_obs_against_math_lgamma():
    rng = np.random.default_rng(5)
    N, D, T = 4, 5, 60
    rates = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (N, D)))
    rates[1, 2] = 0.0
    x = rng.poisson(np.minimum(rates[rng.integers(0, N, T)], 50.0))
    x[:10, 2] = 0                 # rate 0 with count 0 in state 1: the term is 0
    x[10:20, 2] = 3               # ... with a positive count: -inf
    om = PoissonOutputModel(N, rates)
    got = om.log_p_obs(x)
    assert got.shape == (T, N)
    for t in range(T):
        for i in range(N):
            want = 0.0
            for d in range(D):
                lam, k = float(rates[i, d]), int(x[t, d])
                if lam == 0.0:
                    want += 0.0 if k == 0 else -math.inf
                else:
                    want += k * math.log(lam) - lam - math.lgamma(k + 1.0)
            if math.isinf(want):
                assert got[t, i] == -np.inf
            else:
                assert abs(got[t, i] - want) <= 1e-12 * (1.0 + abs(want)), (t, i)
    assert np.all(np.isfinite(got[:10, 1])) and np.all(got[10:20, 1] == -np.inf)
    np.testing.assert_array_equal(om.p_obs(x), np.exp(got))
    assert om.log_p_obs(np.zeros((0, D))).shape == (0, N)


def test_generators_are_reproducible_under_a_seeded_rng():
    om = PoissonOutputModel(3, TRUE_RATES)
    s = np.random.default_rng(1).integers(0, 3, 200)
    a = om.generate_observation_trajectory(s, rng=np.random.default_rng(7))
    b = om.generate_observation_trajectory(s, rng=np.random.default_rng(7))
    assert a.shape == (200, 2) and np.issubdtype(a.dtype, np.integer) and np.array_equal(a, b) and a.min() >= 0
    assert not np.array_equal(a, om.generate_observation_trajectory(s, rng=np.random.default_rng(8)))
    c = om.generate_observations_from_state(2, 50, rng=np.random.default_rng(3))
    assert c.shape == (50, 2) and np.array_equal(c, om.generate_observations_from_state(2, 50, rng=np.random.default_rng(3)))
    d = om.generate_observation_from_state(1, rng=np.random.default_rng(3))
    assert d.shape == (2,) and np.array_equal(d, om.generate_observation_from_state(1, rng=np.random.default_rng(3)))
    check_observation(a)          # what the generators make is what the kind takes


# ---- guessing and the initial model ---------------------------------------------------------------
def test_guess_output_type():
    assert _guess_output_type([np.zeros((4, 2), int)]) == 'poisson'
    assert _guess_output_type([np.zeros((4, 2))]) == 'mvgaussian'
    assert _guess_output_type([np.zeros(4, int)]) == 'discrete'
    assert _guess_output_type([np.zeros(4)]) == 'gaussian'


def _three_clusters(n=3000):
    rng = np.random.default_rng(0)
    P = np.array([[0.9, 0.05, 0.05], [0.05, 0.9, 0.05], [0.05, 0.05, 0.9]])
    s = np.empty(n, dtype=np.int64)
    s[0] = 0
    u = rng.random(n)
    for t in range(1, n):
        s[t] = np.searchsorted(np.cumsum(P[s[t - 1]]), u[t])
    s = np.minimum(s, 2)
    return rng.poisson(TRUE_RATES[s]), P


def test_init_poisson_hmm():
    x, P = _three_clusters()
    obs = [x[:1000], x[1000:]]
    a = bhmm_amd.init_poisson_hmm(obs, 3)
    b = bhmm_amd.init_poisson_hmm(obs, 3)
    assert a.output_model.model_type == 'poisson'
    assert np.array_equal(a.output_model.rates, b.output_model.rates)            # deterministic
    assert np.array_equal(a.transition_matrix, b.transition_matrix)
    got = a.output_model.rates
    got = got[np.argsort(got.sum(axis=1))]
    print("init rates", got.tolist())
    np.testing.assert_allclose(got, TRUE_RATES, rtol=0.10)
    np.testing.assert_allclose(a.transition_matrix.sum(axis=1), 1.0, rtol=1e-12)
    np.testing.assert_allclose(a.initial_distribution.sum(), 1.0, rtol=1e-12)
    assert bhmm_amd.init_hmm(obs, 3).output_model.model_type == 'poisson'      # guessed from the integer arrays
    # a channel that is all zero in a cluster does not start at rate 0
    z = [np.concatenate([np.zeros((50, 1), int), np.full((50, 1), 9)])]
    r = bhmm_amd.init_poisson_hmm(z, 2).output_model.rates
    # (0.5 / points of the cluster; the mixture refinement counts them softly: a zero has weight e^-9 in the bright state)
    np.testing.assert_allclose(np.sort(r[:, 0]), [0.5 / 50, 9.0], rtol=1e-3)
    with pytest.raises(ValueError):
        bhmm_amd.init_poisson_hmm([np.array([[0.5, 1.0]] * 10)], 2)


# ---- ABI and refusals ----------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "bhmm_amd.h")).read()
    L = _lib.load()
    for name in ("bhmm_pois_emissions", "bhmm_logpdf_poisson", "bhmm_host_pois_mstep"):
        assert "int %s(" % name in text, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    for name in ("poisson_hmm", "init_poisson_hmm", "PoissonOutputModel", "PoissonEngine"):
        assert hasattr(bhmm_amd, name), name


def test_device_entry_points_refuse_null_arguments():
    L = _lib.load()
    assert L.bhmm_pois_emissions(None, None) == _lib.ERR_INVALID
    assert L.bhmm_pois_emissions(None, _lib.dp(np.ones(2))) == _lib.ERR_INVALID
    x, r, out = np.zeros((4, 2)), np.ones((1, 2)), np.zeros((4, 1))
    assert L.bhmm_logpdf_poisson(None, _lib.dp(x), 4, 2, 1, _lib.dp(r)) == _lib.ERR_INVALID
    assert L.bhmm_logpdf_poisson(_lib.dp(out), None, 4, 2, 1, _lib.dp(r)) == _lib.ERR_INVALID
    assert L.bhmm_logpdf_poisson(_lib.dp(out), _lib.dp(x), 4, 2, 1, None) == _lib.ERR_INVALID
    assert L.bhmm_logpdf_poisson(_lib.dp(out), _lib.dp(x), 0, 2, 1, _lib.dp(r)) == _lib.ERR_INVALID
    # shape and rates are checked before anything touches a device
    assert L.bhmm_logpdf_poisson(_lib.dp(out), _lib.dp(np.zeros((4, 65))), 4, 65, 1, _lib.dp(np.ones(65))) \
        == _lib.ERR_INVALID
    assert L.bhmm_logpdf_poisson(_lib.dp(out), _lib.dp(x), 4, 2, 1, _lib.dp(np.array([1.0, -1.0]))) == _lib.ERR_INVALID
    assert L.bhmm_logpdf_poisson(_lib.dp(out), _lib.dp(x), 4, 2, 1, _lib.dp(np.array([1.0, np.nan]))) == _lib.ERR_INVALID


def test_estimator_and_samplers_refuse_what_this_kind_does_not_do():
    model = bhmm_amd.poisson_hmm(np.ones(3) / 3, np.full((3, 3), 1.0 / 3), TRUE_RATES)
    obs = [np.zeros((10, 2), int)]
    with pytest.raises(NotImplementedError, match='process_group'):
        bhmm_amd.MaximumLikelihoodEstimator(obs, 3, initial_model=model, process_group=object())
    with pytest.raises(NotImplementedError, match='float64'):
        bhmm_amd.MaximumLikelihoodEstimator(obs, 3, initial_model=model, estep_precision='mixed')
    with pytest.raises(NotImplementedError, match='Gibbs'):
        bhmm_amd.bayesian_hmm(obs, model)
    with pytest.raises(NotImplementedError, match='Gibbs'):
        bhmm_amd.bayesian_mvgaussian_hmm(obs, model)
    with pytest.raises(NotImplementedError, match='Gibbs'):
        bhmm_amd.bayesian_gaussian_mixture_hmm(obs, model)
    with pytest.raises(NotImplementedError, match='Gibbs'):
        bhmm_amd.BayesianHMMSampler(obs, 3, initial_model=model)


# ---- sanitizer run ---------------------------------------------------------------------------------
SAN_DRIVER = r"""
#include <math.h>
#include <stdio.h>
#include <vector>
#include "include/bhmm_amd.h"
int main()
{
    int bad = 0;
    for (int D : {1, 2, 7, 64}) {
        const int N = 3;
        const size_t ms = 1 + 2 * (size_t)D;
        std::vector<double> mom(N * ms, 0.0), old(N * D), fresh(N * D, -1.0);
        for (int i = 0; i < N; ++i) {
            mom[i * ms] = i == 1 ? 0.0 : 10.0; // state 1 has no weight
            for (int a = 0; a < D; ++a) {
                old[i * D + a] = 1.0 + a + i;
                mom[i * ms + 1 + a] = i == 2 ? -1000.0 : 0.5 * a; // state 2 would go below zero
            }
        }
        bad += bhmm_host_pois_mstep(N, D, mom.data(), old.data(), fresh.data()) != BHMM_OK;
        for (int a = 0; a < D; ++a) {
            bad += fabs(fresh[a] - (old[a] + 0.05 * a)) > 1e-12;
            bad += fresh[D + a] != old[D + a];
            bad += fresh[2 * D + a] != 0.0;
        }
        bad += bhmm_host_pois_mstep(N, D, nullptr, old.data(), fresh.data()) != BHMM_ERR_INVALID;
    }
    bad += bhmm_host_pois_mstep(1, 65, nullptr, nullptr, nullptr) != BHMM_ERR_INVALID;
    printf("poisson host sanitizer run: %d failures\n", bad);
    return bad != 0;
}
"""


def test_host_mstep_under_the_sanitizers(tmp_path):
    """bhmm_host_pois_mstep in a stand-alone program built with -fsanitize=address,undefined from host_model.cpp,
    host_api.cpp and host_rev_avx2.cpp, as tests/test_mvn_host.py builds its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "bhmm_amd", "csrc")
    drv = tmp_path / "pois_san.cpp"
    # (invalid_arg / set_error live in the device unit of the library: the driver brings its own)
    drv.write_text('#include <string>\nnamespace bhmm { static std::string g; int invalid_arg(const std::string &m) '
                   '{ g = m; return 3; } void set_error(const std::string &m) { g = m; } }\n' + SAN_DRIVER)
    exe = str(tmp_path / "pois_san")
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
