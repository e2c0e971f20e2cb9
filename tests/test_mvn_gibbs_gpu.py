"""Gibbs sampling for multivariate gaussian emissions on the GPU: the moments of a hidden path
(k_mvn_path_moments) against numpy, the draw with its moments against sample_paths, one sweep of the sampler against
the host draw on statistics recomputed in numpy, D = 1 against the gaussian sampler, and a chain.

The moments are held to the bound of test_mvn_gpu.py::test_moments: |got - fsum(terms)| <= 1e-12 (1 + sum |term|),
the terms formed in numpy from x - mu."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 255, 256, 257, 1023, 1025, 4097, 20000)    # several tiles and workgroups, every ragged edge


def _engine(obs, n):
    from bhmm_amd.engine import MvnEngine
    eng = MvnEngine(0)
    eng.set_observations('mvgaussian', obs, n)
    return eng


def _split(x, lengths):
    off = np.concatenate([[0], np.cumsum(lengths)])
    return [x[off[k]:off[k + 1]] for k in range(len(lengths))]


def _data(D, n, seed, lengths=LENGTHS, far=0.0):
    rng = np.random.default_rng(seed)
    T = sum(lengths)
    x = rng.normal(size=(T, D)) * 10.0 ** rng.uniform(-1, 1, D) + far
    mu = far + rng.normal(size=(n, D))
    return x, mu, rng


def _check_moments(got, x, path, mu, ctype, label=""):
    """every entry against fsum of its numpy terms; a state that does not occur: exact zeros.  Returns the largest
    error / bound."""
    from bhmm_amd.output_models.mvgaussian import moment_stride
    n, D = mu.shape
    ms = moment_stride(D, ctype)
    got = got.reshape(n, ms)
    il = np.tril_indices(D)
    worst = 0.0
    for i in range(n):
        idx = np.nonzero(path == i)[0]
        assert got[i, 0] == float(idx.size), (label, i)
        if idx.size == 0:
            assert np.all(got[i] == 0.0), (label, i)
            continue
        d = x[idx] - mu[i]
        t2 = d[:, il[0]] * d[:, il[1]] if ctype == 'full' else d * d
        terms = np.concatenate([d, t2], axis=1)
        ref = np.array([math.fsum(col) for col in terms.T.tolist()])
        bound = 1e-12 * (1.0 + np.abs(terms).sum(axis=0))
        err = np.abs(got[i, 1:] - ref)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (label, i, float((err / bound).max()))
    return worst


# ---- 1. moments against numpy ---------------------------------------------------------------------------------
# every D of {1, 2, 3, 5, 8, 17, 32, 64} and every n of {1, 3, 8, 9, 20, 64}; (64, 64) full and diag, (17, 64) full
# and (32, 20) full keep the slab in global memory, the rest in LDS; D >= 13 full runs the 4 x 4 block items
CASES = [(1, 1), (2, 3), (3, 8), (5, 9), (8, 20), (17, 64), (32, 8), (64, 3), (1, 64), (2, 64), (3, 20), (5, 1),
         (8, 64), (17, 9), (32, 20), (64, 64)]


@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("D,n", CASES)
def test_path_moments_random_path(D, n, ctype):
    x, mu, rng = _data(D, n, 100 * D + n)
    path = rng.integers(0, n, size=x.shape[0]).astype(np.int32)
    eng = _engine(_split(x, LENGTHS), n)
    try:
        got = eng.path_moments(path, mu, ctype)
        again = eng.path_moments(path, mu, ctype)
        ms = eng.get_option("mvn_path_moments_ms")
    finally:
        eng.close()
    assert np.array_equal(got.view(np.int64), again.view(np.int64))
    worst = _check_moments(got, x, path, mu, ctype, "random")
    print("path moments D=%d n=%d %s: largest error / bound = %.3g, %.3f ms" % (D, n, ctype, worst, ms))


@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("D,n", [(3, 8), (17, 3), (8, 64)])
def test_path_moments_adversarial_paths(D, n, ctype):
    x, mu, rng = _data(D, n, 7 * D + n)
    T = x.shape[0]
    one = np.full(T, n - 1, dtype=np.int32)                              # every step in one state
    flip = (np.arange(T) % n).astype(np.int32)                          # the state changes at every step
    missing = rng.integers(0, max(n - 1, 1), size=T).astype(np.int32)   # state n - 1 never occurs
    sticky = np.repeat(rng.integers(0, n, size=T // 50 + 1), 50)[:T].astype(np.int32)   # long dwells
    eng = _engine(_split(x, LENGTHS), n)
    try:
        for name, path in (("one", one), ("flip", flip), ("missing", missing), ("sticky", sticky)):
            _check_moments(eng.path_moments(path, mu, ctype), x, path, mu, ctype, name)
    finally:
        eng.close()


@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("D,n", [(2, 200), (17, 200), (8, 200), (2, 4096)])
def test_path_moments_many_states(D, n, ctype):
    """int32 paths beyond one byte; (17, 200) and (8, 200) full keep the slab in global memory"""
    lengths = (257, 4097, 1)
    x, mu, rng = _data(D, n, 3 * D + n, lengths=lengths)
    path = rng.integers(0, n, size=x.shape[0]).astype(np.int32)
    path[:300] = n - 1
    eng = _engine(_split(x, lengths), n)
    try:
        got = eng.path_moments(path, mu, ctype)
        if n > 256:
            with pytest.raises(ValueError):
                eng.path_moments(path.astype(np.uint8), mu, ctype)       # one byte does not hold these states
    finally:
        eng.close()
    _check_moments(got, x, path, mu, ctype, "many")


@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("D,n", [(3, 8), (17, 3)])
def test_path_moments_far_from_the_origin(D, n, ctype):
    """means 1e6 sigma from the origin: the mean is subtracted first, so the same bound holds"""
    rng = np.random.default_rng(D)
    T = sum(LENGTHS)
    x = 1e6 + rng.normal(size=(T, D))
    mu = 1e6 + 0.3 * rng.normal(size=(n, D))
    path = rng.integers(0, n, size=T).astype(np.int32)
    eng = _engine(_split(x, LENGTHS), n)
    try:
        got = eng.path_moments(path, mu, ctype)
    finally:
        eng.close()
    _check_moments(got, x, path, mu, ctype, "far")


# ---- 2. repeatability and forms -------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("D,n", [(2, 3), (8, 20), (17, 64), (64, 64)])
def test_path_moments_same_bits_for_every_form(D, n, ctype):
    import torch
    x, mu, rng = _data(D, n, 11 * D + n)
    p32 = rng.integers(0, n, size=x.shape[0]).astype(np.int32)
    p8 = p32.astype(np.uint8)
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    eng = _engine(_split(x, LENGTHS), n)
    try:
        base = eng.path_moments(p32, mu, ctype)
        forms = {
            "again": eng.path_moments(p32, mu, ctype),
            "u8": eng.path_moments(p8, mu, ctype),
            "list": eng.path_moments([p32[off[k]:off[k + 1]] for k in range(len(LENGTHS))], mu, ctype),
            "dev32": eng.path_moments(torch.from_numpy(p32).to('cuda:0'), mu, ctype),
            "dev8": eng.path_moments(torch.from_numpy(p8).to('cuda:0'), mu, ctype),
            "host tensor": eng.path_moments(torch.from_numpy(p8), mu, ctype),
        }
    finally:
        eng.close()
    for name, got in forms.items():
        assert np.array_equal(base.view(np.int64), got.view(np.int64)), name


# ---- 3. invalid states and reuse ------------------------------------------------------------------------------
def test_state_outside_raises_and_the_engine_lives():
    import torch
    D, n = 3, 5
    lengths = (300, 1, 700)
    x, mu, rng = _data(D, n, 1, lengths=lengths)
    path = rng.integers(0, n, size=x.shape[0]).astype(np.int32)
    eng = _engine(_split(x, lengths), n)
    try:
        good = eng.path_moments(path, mu)
        for where in (0, 299, 300, 1000):
            for bad_state in (n, -1, 2 ** 31 - 1):
                bad = path.copy()
                bad[where] = bad_state
                with pytest.raises(ValueError):
                    eng.path_moments(bad, mu)
                with pytest.raises(ValueError):
                    eng.path_moments(torch.from_numpy(bad).to('cuda:0'), mu, 'diag')
        b8 = path.astype(np.uint8)
        b8[17] = n
        with pytest.raises(ValueError):
            eng.path_moments(b8, mu)
        with pytest.raises(ValueError):
            eng.path_moments(path[:-1], mu)
        with pytest.raises(ValueError):
            eng.path_moments(path, mu[:, :2])
        assert np.array_equal(eng.path_moments(path, mu), good)
    finally:
        eng.close()


# ---- 4. the one-hot route -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("D,n", [(2, 8), (8, 3), (17, 9)])
def test_one_hot_rows_through_the_soft_moments_agree(D, n, ctype):
    import torch
    from bhmm_amd.output_models.mvgaussian import moment_stride
    lengths = (300, 1, 411, 2000)
    x, mu, rng = _data(D, n, 5 * D + n, lengths=lengths)
    path = rng.integers(0, n, size=x.shape[0]).astype(np.int32)
    g = np.zeros((x.shape[0], n))
    g[np.arange(x.shape[0]), path] = 1.0
    eng = _engine(_split(x, lengths), n)
    try:
        hard = eng.path_moments(path, mu, ctype)
        soft = eng.moments(torch.from_numpy(g).to('cuda:0'), mu, ctype)
    finally:
        eng.close()
    ms = moment_stride(D, ctype)
    il = np.tril_indices(D)
    for i in range(n):
        d = x[path == i] - mu[i]
        t2 = d[:, il[0]] * d[:, il[1]] if ctype == 'full' else d * d
        mag = np.concatenate([[float(d.shape[0])], np.abs(d).sum(axis=0), np.abs(t2).sum(axis=0)])
        bound = 2 * 1e-12 * (1.0 + mag)                        # the sum of the two bounds
        assert np.all(np.abs(hard[i * ms:(i + 1) * ms] - soft[i * ms:(i + 1) * ms]) <= bound), i


# ---- 5. the draw with its moments -----------------------------------------------------------------------------
def _model(n, D, seed, ctype='full', sep=4.0):
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) * 0.2 + np.eye(n) * 3.0
    A /= A.sum(axis=1)[:, None]
    pi = rng.random(n) + 0.5
    pi /= pi.sum()
    mu = rng.normal(size=(n, D)) * 0.3
    mu[:, 0] += sep * np.arange(n)
    cov = np.empty((n, D, D))
    for i in range(n):
        Q = rng.normal(size=(D, D)) * 0.2 + np.eye(D)
        cov[i] = Q.dot(Q.T) * rng.uniform(0.7, 1.4)
        cov[i] = 0.5 * (cov[i] + cov[i].T)
    if ctype == 'diag':
        cov = np.array([np.diag(c) for c in cov])
    return A, pi, mu, cov


def _simulate(A, pi, mu, cov, lengths, seed):
    rng = np.random.default_rng(seed)
    n, D = mu.shape
    fac = [np.linalg.cholesky(c) if c.ndim == 2 else np.diag(np.sqrt(c)) for c in cov]
    obs, states = [], []
    for T in lengths:
        s = np.empty(T, dtype=np.int64)
        s[0] = rng.choice(n, p=pi)
        for t in range(1, T):
            s[t] = rng.choice(n, p=A[s[t - 1]])
        z = rng.normal(size=(T, D))
        obs.append(mu[s] + np.einsum('tab,tb->ta', np.array(fac)[s], z))
        states.append(s)
    return obs, states


@pytest.mark.parametrize("explicit_u", [False, True])
@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("n", [3, 8, 12, 70])
def test_sample_paths_moments(n, ctype, explicit_u):
    """n = 3 and 8: the chunked sampler, 12: the wide one, 70: the generic one"""
    D = 3
    lengths = (700, 1, 333, 1500)
    A, pi, mu, cov = _model(n, D, n, ctype, sep=1.5)
    rng = np.random.default_rng(n + 1)
    x = rng.normal(size=(sum(lengths), D)) + mu[rng.integers(0, n, size=sum(lengths))]
    obs = _split(x, lengths)
    u = [rng.random(T) for T in lengths] if explicit_u else None
    eng = _engine(obs, n)
    try:
        ref_paths, ref_C, ref_n0, _ = eng.sample_paths(A, pi, mu, cov, u=u, seed=77, want_paths=True)
        paths, C, n0, mom = eng.sample_paths_moments(A, pi, mu, cov, u=u, seed=77, want_paths=True)
        none, C2, n02, mom2 = eng.sample_paths_moments(A, pi, mu, cov, u=u, seed=77, want_paths=False)
        after = eng.sample_paths(A, pi, mu, cov, u=u, seed=77, want_paths=True)      # the engine goes on as before
    finally:
        eng.close()
    assert none is None
    for a, b, c in zip(ref_paths, paths, after[0]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(ref_C, C) and np.array_equal(ref_n0, n0)
    assert np.array_equal(C, C2) and np.array_equal(n0, n02) and np.array_equal(after[1], C)
    assert np.array_equal(mom.view(np.int64), mom2.view(np.int64))
    _check_moments(mom, x, np.concatenate(paths), mu, ctype, "drawn")


# ---- 6. one sweep end to end ----------------------------------------------------------------------------------
def _numpy_stats(obs, paths, mu, n, ctype):
    from bhmm_amd.output_models.mvgaussian import pack_moments
    D = mu.shape[1]
    C, n0 = np.zeros((n, n)), np.zeros(n)
    for p in paths:
        n0[p[0]] += 1
        np.add.at(C, (p[:-1], p[1:]), 1.0)
    x, s = np.concatenate(obs), np.concatenate(paths)
    S0, S1 = np.zeros(n), np.zeros((n, D))
    S2 = np.zeros((n, D, D) if ctype == 'full' else (n, D))
    for i in range(n):
        d = x[s == i] - mu[i]
        S0[i], S1[i] = d.shape[0], d.sum(axis=0)
        S2[i] = d.T.dot(d) if ctype == 'full' else (d * d).sum(axis=0)
    return np.concatenate([C.ravel(), n0, pack_moments(S0, S1, S2, ctype)])


@pytest.mark.parametrize("reversible", [True, False])
@pytest.mark.parametrize("ctype", ["full", "diag"])
def test_one_sweep_equals_the_host_draw_on_numpy_statistics(ctype, reversible):
    import bhmm_amd
    from bhmm_amd.estimators._native import GibbsParametersMvn
    n, D = 3, 2
    A, pi, mu, cov = _model(n, D, 31, ctype)
    obs, _ = _simulate(A, pi, mu, cov, (1000,) * 4, 32)
    model = bhmm_amd.mvgaussian_hmm(pi, A, mu, cov, covariance_type=ctype)
    smp = bhmm_amd.BayesianHMMSampler(obs, n, initial_model=model, reversible=reversible, output='mvgaussian')
    smp._update(seed=4242, keep_paths=True)
    paths = smp.model.hidden_state_trajectories
    packed = _numpy_stats(obs, paths, mu, n, ctype)
    draw = GibbsParametersMvn(n, D, ctype, prior_C=smp.prior_C, prior_n0=smp.prior_n0, reversible=reversible,
                              stationary=False, nsteps=smp.transition_matrix_sampling_steps)
    T, p0, m, c = draw(packed, mu, cov, smp._param_seed, smp._sweep)
    np.testing.assert_allclose(smp.model.transition_matrix, T, rtol=1e-9)
    np.testing.assert_allclose(smp.model.initial_distribution, p0, rtol=1e-9)
    np.testing.assert_allclose(smp.model.output_model.means, m, rtol=1e-9)
    np.testing.assert_allclose(smp.model.output_model.covariances, c, rtol=1e-9, atol=1e-12)
    assert not np.array_equal(m, mu)


@pytest.mark.parametrize("ctype", ["full", "diag"])
def test_numpy_parameter_path(ctype):
    import bhmm_amd
    n, D = 3, 2
    A, pi, mu, cov = _model(n, D, 41, ctype)
    obs, _ = _simulate(A, pi, mu, cov, (1000,) * 4, 42)
    model = bhmm_amd.mvgaussian_hmm(pi, A, mu, cov, covariance_type=ctype)
    smp = bhmm_amd.BayesianHMMSampler(obs, n, initial_model=model, output='mvgaussian', native_parameters=False)
    smp._rng = np.random.RandomState(3)
    for _ in range(3):
        smp._update(seed=None, keep_paths=False)
    om = smp.model.output_model
    assert np.all(np.isfinite(om.means)) and not np.array_equal(om.means, mu)
    for i in range(n):
        c = om.covariances[i]
        if ctype == 'full':
            assert np.array_equal(c, c.T)
            np.linalg.cholesky(c)
        else:
            assert np.all(c > 0.0) and np.all(np.isfinite(c))
    assert np.allclose(smp.model.transition_matrix.sum(axis=1), 1.0)


# ---- 7. D = 1 against the gaussian sampler --------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
def test_one_dimension_follows_the_gaussian_sampler(ctype):
    """Same data, seed and sweeps.  (A draw on a cumulative-sum edge could differ between the kinds -- their forward
    rows differ in the last bits -- with a chance of about 1e-11 per run; seed 5 has none.)"""
    import bhmm_amd
    n = 3
    A, pi, mu, cov = _model(n, 1, 51, 'full')
    obs, _ = _simulate(A, pi, mu, cov, (500,) * 4, 52)
    sig = np.sqrt(cov[:, 0, 0])
    var = cov if ctype == 'full' else cov[:, 0, :]
    g = bhmm_amd.BayesianHMMSampler([o[:, 0] for o in obs], n, output='gaussian',
                                    initial_model=bhmm_amd.gaussian_hmm(pi, A, mu[:, 0], sig))
    m = bhmm_amd.BayesianHMMSampler(obs, n, output='mvgaussian',
                                    initial_model=bhmm_amd.mvgaussian_hmm(pi, A, mu, var, covariance_type=ctype))
    for sweep in range(5):
        seed = 5 if sweep == 0 else None
        g._update(seed=seed, keep_paths=True)
        m._update(seed=seed, keep_paths=True)
        for a, b in zip(g.model.hidden_state_trajectories, m.model.hidden_state_trajectories):
            assert np.array_equal(a, b), sweep
        np.testing.assert_allclose(m.model.output_model.means[:, 0], g.model.output_model.means, rtol=1e-9)
        np.testing.assert_allclose(np.sqrt(m.model.output_model.covariances.reshape(n)),
                                   g.model.output_model.sigmas, rtol=1e-9)
        np.testing.assert_allclose(m.model.transition_matrix, g.model.transition_matrix, rtol=1e-9)


# ---- 8. a chain -----------------------------------------------------------------------------------------------
def test_chain():
    import bhmm_amd
    n, D = 3, 2
    A = np.array([[0.95, 0.04, 0.01], [0.03, 0.94, 0.03], [0.02, 0.04, 0.94]])
    pi = np.array([0.4, 0.3, 0.3])
    mu = np.array([[0.0, 0.0], [10.0, 0.0], [0.0, 10.0]])                  # 10 sigma apart
    cov = np.array([[[1.0, 0.3], [0.3, 1.0]], [[1.0, -0.2], [-0.2, 1.0]], [[1.0, 0.0], [0.0, 1.0]]])
    obs, _ = _simulate(A, pi, mu, cov, (2000,) * 8, 61)
    model = bhmm_amd.mvgaussian_hmm(pi, A, mu, cov)
    a = bhmm_amd.bayesian_mvgaussian_hmm(obs, model, nsample=50, seed=9)
    b = bhmm_amd.bayesian_mvgaussian_hmm(obs, model, nsample=50, seed=9)
    assert len(a.sampled_hmms) == 50
    for ha, hb in zip(a.sampled_hmms, b.sampled_hmms):
        assert np.array_equal(ha.transition_matrix, hb.transition_matrix)
        assert np.array_equal(ha.output_model.means, hb.output_model.means)
        assert np.array_equal(ha.output_model.covariances, hb.output_model.covariances)
        for c in ha.output_model.covariances:
            np.linalg.cholesky(c)
    assert np.all(np.abs(a.means_mean - mu) <= 0.1)                        # sigma = 1
    assert a.means_std.shape == (n, D) and a.covariances_std.shape == (n, D, D)
    assert np.shape(a.covariances_conf) == (2, n, D, D)
    logL = bhmm_amd.score(obs, a)
    assert logL.shape == (50,) and np.all(np.isfinite(logL))
    with pytest.raises(NotImplementedError):
        bhmm_amd.bayesian_hmm(obs, model)
