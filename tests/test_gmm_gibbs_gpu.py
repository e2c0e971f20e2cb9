"""Gibbs sampling for gaussian-mixture emissions on the GPU: the component draw of
k_gmm_draw_components against a long-double reference, its reproducibility, stream offsets, the moments of the labels,
the draw after the path draw (bhmm_gmm_sample_paths), one sweep of the sampler against the host draw, M = 1 against the
multivariate gaussian sampler, and a chain.

The draw is held to tests/gmm_draw_ref.py: a_tic of the state a step is in, in long double by forward substitution by
hand (the yardstick of test_gmm_gpu.py), p_c = e_c / s_c, the uniforms restated.  A decision u < p_c is undecided when
|u - p_c| <= p_c (4 max_{c' <= c} B_tc' + 16 M eps), B the bound of DESIGN.md section 25 on the device's a_tic: the
margin is twice the bound on a difference of two a, plus the exps and the sum.  The seeded inputs have no undecided
decision (asserted from the reference alone; about steps x M x 1e-11 are expected), so every label must be the
reference's."""
import copy

import numpy as np
import pytest

from tests import gmm_draw_ref as ref
from tests.test_gmm_gpu import EPS, _engine, _l_ref, _par, _rand_cov
from tests.test_mvn_gibbs_gpu import _check_moments, _split

pytestmark = pytest.mark.gpu

LENGTHS = (700, 1, 333, 1500)   # 2534 steps: ten workgroups, the last one partial; a one-step trajectory
TOTAL = sum(LENGTHS)
CASES = [(3, 2, 2), (8, 4, 3), (1, 16, 5), (12, 3, 17), (70, 2, 2), (64, 64, 1), (3, 3, 64)]


# ---- the reference -------------------------------------------------------------------------------------------
def _a_of_path(x, path, w, mu, cov, ctype):
    """a_tic (T, M) in long double of the state the path is in (-inf where w = 0) and the bound B (T, M) on the
    device's a_tic: b_tic + 2 eps (|log w| + |l|), b_tic = 64 D eps kappa_2 (1 + |z|^2) + 16 eps |c|"""
    N, M, D = mu.shape
    T = x.shape[0]
    a = np.full((T, M), -np.inf, dtype=np.longdouble)
    B = np.zeros((T, M))
    for i in np.unique(path):
        idx = np.nonzero(path == i)[0]
        l, z2, c, kappa = _l_ref(x[idx], mu[i], cov[i], ctype)
        b = 64 * D * EPS * kappa[None, :] * (1.0 + z2) + 16 * EPS * np.abs(c)[None, :]
        pos = w[i] > 0
        logw = np.log(w[i, pos].astype(np.longdouble))
        a[np.ix_(idx, np.nonzero(pos)[0])] = l[:, pos] + logw[None]
        B[np.ix_(idx, np.nonzero(pos)[0])] = b[:, pos] + 2 * EPS * (np.abs(logw.astype(np.float64))[None]
                                                                     + np.abs(l[:, pos].astype(np.float64)))
    return a, B


def _mix_case(D, N, M, ctype, rng, lengths=None):
    """N M components of comparable scale (0.7 to 1.5) with kappa_2(L) <= 3.2, means a few sigma apart, points drawn
    from the components: the bound B on a_tic stays small, so that a decision within the margin is as rare as the
    module's docstring says.  Dirichlet(2) weights, w[0, 0] = 0 wherever M > 1."""
    n = N * M
    scales = rng.uniform(0.7, 1.5, n)
    kap = 10.0 ** rng.uniform(0, 0.5, n)
    if ctype == 'full':
        cov = np.array([_rand_cov(rng, D, s, k) for s, k in zip(scales, kap)])
        fac = np.array([np.linalg.cholesky(c) for c in cov])
    else:
        sd = np.array([s * np.logspace(0, -np.log10(k), D)[rng.permutation(D)] if D > 1 else np.array([s])
                       for s, k in zip(scales, kap)])
        cov = sd * sd
        fac = np.array([np.diag(s) for s in sd])
    mu = rng.normal(size=(n, D)) * 2.0 / np.sqrt(D)
    w = rng.dirichlet(np.full(M, 2.0), N) if M > 1 else np.ones((N, 1))
    if M > 1:
        w[0, 0] = 0.0
        w[0] /= w[0].sum()
    obs = []
    for T in (lengths or LENGTHS):
        j = rng.integers(0, n, T)
        obs.append(mu[j] + np.einsum('tab,tb->ta', fac[j], rng.normal(size=(T, D))))
    return obs, w, mu.reshape(N, M, D), cov.reshape((N, M) + cov.shape[1:])


def _reference(x, path, w, mu, cov, ctype, seed, g=None):
    M = mu.shape[1]
    a, B = _a_of_path(x, path, w, mu, cov, ctype)
    if g is None:
        g = np.arange(x.shape[0], dtype=np.uint64)
    return ref.reference_labels(a, B, path, M, ref.draw_key(seed), g)


def _fixed_paths(N):
    """a constant path; one that changes state every step (a wavefront holds min(N, 64) states); one that changes
    exactly between steps 63 | 64 and 255 | 256 and across the trajectory ends"""
    t = np.arange(TOTAL)
    ends = np.cumsum(LENGTHS)[:-1]
    edges = np.zeros(TOTAL, dtype=np.int64)
    for e in [64, 256] + list(ends):
        edges[e:] += 1
    return {"constant": np.full(TOTAL, N - 1, dtype=np.int32), "flip": (t % N).astype(np.int32),
            "edges": ((edges + (N > 1)) % N).astype(np.int32)}


def _transition_model(N, seed):
    rng = np.random.default_rng(seed)
    A = rng.random((N, N)) * 0.2 + np.eye(N) * 3.0
    A /= A.sum(axis=1)[:, None]
    pi = rng.random(N) + 0.5
    return A, pi / pi.sum()


# ---- 1. draws against the reference --------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("N,M,D", CASES)
def test_draws_against_the_reference(N, M, D, ctype):
    rng = np.random.default_rng(1000 * N + 10 * M + D)
    obs, w, mu, cov = _mix_case(D, N, M, ctype, rng, lengths=LENGTHS)
    assert w[0, 0] == 0.0 and abs(w[0].sum() - 1.0) < 1e-12
    x = np.concatenate(obs)
    par0, par1 = _par(w, mu, cov)
    A, pi = _transition_model(N, N + M)
    seed = 20 + N
    eng = _engine(obs, N)
    try:
        drawn, _, _, _ = eng.sample_paths(A, pi, par0, par1, seed=seed, want_paths=True)
        paths = dict(_fixed_paths(N), drawn=np.concatenate(drawn).astype(np.int32))
        got = {name: eng.draw_components(p, seed=seed) for name, p in paths.items()}
    finally:
        eng.close()
    for name, p in paths.items():
        want, undecided = _reference(x, p, w, mu, cov, ctype, seed)
        assert not undecided.any(), (name, int(undecided.sum()))       # (from the reference alone: take another seed)
        labels, mom = got[name]
        assert labels.dtype == np.int32 and labels.shape == (TOTAL,)
        assert np.array_equal(labels // M, p), name
        bad = np.nonzero(labels != want)[0]
        assert bad.size == 0, (name, bad[:5], labels[bad[:5]], want[bad[:5]])
        assert not np.any(labels == 0), name                          # component (0, 0) has weight zero
        _check_moments(mom, x, labels, mu.reshape(N * M, D), ctype, name)
    if N > 1 and M > 1:     # the draw is a draw: more than one component of some state occurs
        assert np.unique(got["flip"][0]).size > N


def test_one_component_gives_the_path():
    N, M, D = 3, 1, 2
    rng = np.random.default_rng(5)
    obs, w, mu, cov = _mix_case(D, N, M, 'full', rng, lengths=LENGTHS)
    path = rng.integers(0, N, size=TOTAL).astype(np.int32)
    eng = _engine(obs, N)
    try:
        eng.emissions(*_par(w, mu, cov))
        labels, mom = eng.draw_components(path, seed=3)
        mvn_like = eng.draw_components(path, seed=4)[1]
    finally:
        eng.close()
    assert np.array_equal(labels, path)
    assert np.array_equal(mom, mvn_like)
    _check_moments(mom, np.concatenate(obs), path, mu.reshape(N, D), 'full', "M = 1")


# ---- 2. the same bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("N,M,D", [(3, 2, 2), (8, 4, 3), (12, 3, 17)])
def test_same_bits_for_every_form(N, M, D, ctype):
    import torch
    rng = np.random.default_rng(7 * N + M)
    obs, w, mu, cov = _mix_case(D, N, M, ctype, rng, lengths=LENGTHS)
    p32 = np.repeat(rng.integers(0, N, size=TOTAL // 40 + 1), 40)[:TOTAL].astype(np.int32)
    p8 = p32.astype(np.uint8)
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    eng = _engine(obs, N)
    try:
        eng.emissions(*_par(w, mu, cov))
        base = eng.draw_components(p32, seed=11)
        forms = {
            "again": eng.draw_components(p32, seed=11),
            "u8": eng.draw_components(p8, seed=11),
            "list": eng.draw_components([p32[off[k]:off[k + 1]] for k in range(len(LENGTHS))], seed=11),
            "dev32": eng.draw_components(torch.from_numpy(p32).to('cuda:0'), seed=11),
            "dev8": eng.draw_components(torch.from_numpy(p8).to('cuda:0'), seed=11),
        }
        none, mom = eng.draw_components(p32, seed=11, want_labels=False)
        other = eng.draw_components(p32, seed=12)
        ms = eng.get_option("gmm_draw_ms")
    finally:
        eng.close()
    for name, (labels, m) in forms.items():
        assert np.array_equal(base[0], labels), name
        assert np.array_equal(base[1].view(np.int64), m.view(np.int64)), name
    assert none is None and np.array_equal(base[1].view(np.int64), mom.view(np.int64))
    assert not np.array_equal(base[0], other[0])        # another seed, other components
    assert ms > 0.0


# ---- 3. stream offsets -----------------------------------------------------------------------------------------
def test_stream_offsets_place_the_trajectories():
    N, M, D = 3, 3, 2
    rng = np.random.default_rng(9)
    obs, w, mu, cov = _mix_case(D, N, M, 'full', rng, lengths=LENGTHS)
    par = _par(w, mu, cov)
    path = np.repeat(rng.integers(0, N, size=TOTAL // 25 + 1), 25)[:TOTAL].astype(np.int32)
    pieces = _split(path, LENGTHS)
    soff = np.array([5000, 3, 2 ** 33, 100000], dtype=np.int64)

    def run(ks, offsets):
        eng = _engine([obs[k] for k in ks], N)
        try:
            eng.emissions(*par)
            if offsets is not None:
                eng.set_stream_offsets(offsets)
            return eng.draw_components(np.concatenate([pieces[k] for k in ks]), seed=21)[0]
        finally:
            eng.close()
    plain = run(range(4), None)
    whole = run(range(4), soff)
    first, second = run([0, 1], soff[:2]), run([2, 3], soff[2:])
    assert np.array_equal(whole, np.concatenate([first, second]))
    assert not np.array_equal(whole, plain)
    x = np.concatenate(obs)
    want, undecided = _reference(x, path, w, mu, cov, 'full', 21, g=ref.stream_positions(LENGTHS, soff))
    assert not undecided.any()
    assert np.array_equal(whole, want)
    want0, undecided0 = _reference(x, path, w, mu, cov, 'full', 21)
    assert not undecided0.any() and np.array_equal(plain, want0)


# ---- 4. moments of the labels ----------------------------------------------------------------------------------
def _plain_mixture(N, M, D, ctype, seed, far=0.0):
    rng = np.random.default_rng(seed)
    mu = far + rng.normal(size=(N, M, D)) * 2.0
    cov = np.ones((N, M, D)) * rng.uniform(0.5, 2.0, size=(N, M, 1))
    if ctype == 'full':
        cov = cov[..., None] * np.eye(D)
    w = rng.dirichlet(np.full(M, 2.0), N)
    path = rng.integers(0, N, size=TOTAL).astype(np.int32)
    comp = rng.integers(0, M, size=TOTAL)
    x = mu[path, comp] + rng.normal(size=(TOTAL, D))
    return x, path, w, mu, cov


@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("N,M,D,far", [(3, 2, 2, 0.0), (64, 64, 2, 0.0), (3, 3, 64, 0.0), (8, 4, 8, 0.0),
                                       (3, 2, 3, 1e6)])
def test_moments_of_the_labels(N, M, D, far, ctype):
    """up to 4096 labels (the slab in global memory) and D = 64; one case 1e6 sigma from the origin"""
    x, path, w, mu, cov = _plain_mixture(N, M, D, ctype, N + M + D, far)
    eng = _engine(_split(x, LENGTHS), N)
    try:
        eng.emissions(*_par(w, mu, cov))
        labels, mom = eng.draw_components(path, seed=31)
    finally:
        eng.close()
    assert np.array_equal(labels // M, path)
    worst = _check_moments(mom, x, labels, mu.reshape(N * M, D), ctype, "labels")
    print("component moments N=%d M=%d D=%d %s: largest error / bound = %.3g" % (N, M, D, ctype, worst))


# ---- 5. the draw after the path draw ---------------------------------------------------------------------------
@pytest.mark.parametrize("explicit_u", [False, True])
@pytest.mark.parametrize("n", [3, 12, 70])
def test_sample_paths_components(n, explicit_u):
    """n = 3: the chunked sampler, 12: the wide one, 70: the generic one"""
    M, D = 3, 3
    rng = np.random.default_rng(n)
    obs, w, mu, cov = _mix_case(D, n, M, 'full', rng, lengths=LENGTHS)
    x = np.concatenate(obs)
    par0, par1 = _par(w, mu, cov)
    A, pi = _transition_model(n, n)
    u = [rng.random(T) for T in LENGTHS] if explicit_u else None
    eng = _engine(obs, n)
    try:
        ref_paths, ref_C, ref_n0, _ = eng.sample_paths(A, pi, par0, par1, u=u, seed=77, want_paths=True)
        paths, labels, C, n0, mom = eng.sample_paths_components(A, pi, par0, par1, u=u, seed=77, want_paths=True,
                                                                want_labels=True)
        none, none2, C2, n02, mom2 = eng.sample_paths_components(A, pi, par0, par1, u=u, seed=77)
        given = eng.draw_components(np.concatenate(ref_paths).astype(np.int32), seed=77)
        after = eng.sample_paths(A, pi, par0, par1, u=u, seed=77, want_paths=True)    # the engine goes on as before
        res = eng.estep(A, pi, par0, par1)
    finally:
        eng.close()
    assert none is None and none2 is None
    for a, b, c in zip(ref_paths, paths, after[0]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(ref_C, C) and np.array_equal(ref_n0, n0)
    assert np.array_equal(C, C2) and np.array_equal(n0, n02) and np.array_equal(after[1], C)
    assert np.array_equal(mom.view(np.int64), mom2.view(np.int64))
    flat = np.concatenate(labels)
    assert np.array_equal(flat // M, np.concatenate(paths))
    assert np.array_equal(flat, given[0]) and np.array_equal(mom.view(np.int64), given[1].view(np.int64))
    _check_moments(mom, x, flat, mu.reshape(n * M, D), 'full', "drawn")
    assert np.isfinite(res.loglik) and np.all(np.isfinite(res.packed))


# ---- 6. invalid input ------------------------------------------------------------------------------------------
def test_state_outside_raises_and_the_engine_lives():
    """input validation: the kernel finds the state before it indexes anything with it"""
    import torch
    N, M, D = 5, 2, 3
    rng = np.random.default_rng(1)
    obs, w, mu, cov = _mix_case(D, N, M, 'full', rng, lengths=LENGTHS)
    path = rng.integers(0, N, size=TOTAL).astype(np.int32)
    eng = _engine(obs, N)
    try:
        with pytest.raises(ValueError):
            eng.draw_components(path)                         # no emissions yet
        eng.emissions(*_par(w, mu, cov))
        good = eng.draw_components(path, seed=2)
        for where in (0, 699, 700, 2533):
            for bad_state in (N, -1, 2 ** 31 - 1):
                bad = path.copy()
                bad[where] = bad_state
                with pytest.raises(ValueError):
                    eng.draw_components(bad, seed=2)
                with pytest.raises(ValueError):
                    eng.draw_components(torch.from_numpy(bad).to('cuda:0'), seed=2)
        b8 = path.astype(np.uint8)
        b8[17] = N
        with pytest.raises(ValueError):
            eng.draw_components(b8, seed=2)
        with pytest.raises(ValueError):
            eng.draw_components(path[:-1], seed=2)
        again = eng.draw_components(path, seed=2)
    finally:
        eng.close()
    assert np.array_equal(good[0], again[0]) and np.array_equal(good[1], again[1])


def test_not_a_mixture_is_invalid():
    from bhmm_amd import _lib
    N, M, D = 3, 2, 2
    rng = np.random.default_rng(2)
    obs, w, mu, cov = _mix_case(D, N, M, 'full', rng, lengths=LENGTHS)
    A, pi = _transition_model(N, 1)
    path = np.zeros(TOTAL, dtype=np.int32)
    eng = _engine(obs, N)
    try:
        eng.emissions(*_par(w, mu, cov))
        eng.draw_components(path)
        L, h = eng._L, eng._h
        mom = np.empty(N * M * (1 + D + D * (D + 1) // 2))
        C, n0 = np.zeros((N, N), dtype=np.int64), np.zeros(N, dtype=np.int64)
        assert L.bhmm_mvn_emissions(h, _lib.dp(_lib.f64(mu[:, 0])), _lib.dp(_lib.f64(cov[:, 0])), _lib.COV_FULL) == _lib.OK
        assert L.bhmm_gmm_path_components(h, path.ctypes.data, 0, 0, 1, None, _lib.dp(mom)) == _lib.ERR_INVALID
        assert L.bhmm_gmm_sample_paths(h, _lib.dp(_lib.f64(A)), _lib.dp(_lib.f64(pi)), None, 1, None, None, _lib.lp(C),
                                       _lib.lp(n0), _lib.dp(mom)) == _lib.ERR_INVALID
        eng._loaded = None                                      # (the rows on the device are not the engine's any more)
        eng.emissions(*_par(w, mu, cov))
        eng.draw_components(path)
    finally:
        eng.close()


# ---- 7. one sweep end to end -----------------------------------------------------------------------------------
def _mixture_model(ctype, seed):
    """N = 2, M = 2, D = 2: components 10 sigma apart inside and between states"""
    import bhmm_amd
    A = np.array([[0.95, 0.05], [0.04, 0.96]])
    pi = np.array([0.5, 0.5])
    w = np.array([[0.6, 0.4], [0.3, 0.7]])
    mu = np.array([[[0.0, 0.0], [10.0, 0.0]], [[0.0, 10.0], [10.0, 10.0]]])
    cov = np.array([[[[1.0, 0.3], [0.3, 1.0]], [[1.0, -0.2], [-0.2, 1.0]]],
                    [[[1.0, 0.0], [0.0, 1.0]], [[0.8, 0.1], [0.1, 1.2]]]])
    if ctype == 'diag':
        cov = np.array([[np.diag(c) for c in row] for row in cov])
    model = bhmm_amd.gaussian_mixture_hmm(pi, A, w, mu, cov, covariance_type=ctype)
    rng = np.random.default_rng(seed)
    return model, A, pi, w, mu, cov, rng


def _simulate(model, lengths, rng):
    A, pi = model.transition_matrix, model.initial_distribution
    n = A.shape[0]
    obs = []
    for T in lengths:
        s = np.empty(T, dtype=np.int64)
        s[0] = rng.choice(n, p=pi)
        for t in range(1, T):
            s[t] = rng.choice(n, p=A[s[t - 1]])
        obs.append(model.output_model.generate_observation_trajectory(s, rng=rng))
    return obs


def _numpy_stats(obs, paths, labels, mu, ctype):
    from bhmm_amd.output_models.mvgaussian import pack_moments
    N, M, D = mu.shape
    C, n0 = np.zeros((N, N)), np.zeros(N)
    for p in paths:
        n0[p[0]] += 1
        np.add.at(C, (p[:-1], p[1:]), 1.0)
    x, lab = np.concatenate(obs), np.concatenate(labels)
    mf = mu.reshape(N * M, D)
    S0, S1 = np.zeros(N * M), np.zeros((N * M, D))
    S2 = np.zeros((N * M, D, D) if ctype == 'full' else (N * M, D))
    for q in range(N * M):
        d = x[lab == q] - mf[q]
        S0[q], S1[q] = d.shape[0], d.sum(axis=0)
        S2[q] = d.T.dot(d) if ctype == 'full' else (d * d).sum(axis=0)
    return np.concatenate([C.ravel(), n0, pack_moments(S0, S1, S2, ctype)])


@pytest.mark.parametrize("reversible", [True, False])
@pytest.mark.parametrize("ctype", ["full", "diag"])
def test_one_sweep_equals_the_host_draw_on_numpy_statistics(ctype, reversible):
    import bhmm_amd
    from bhmm_amd.estimators._native import GibbsParametersGmm
    model, A, pi, w, mu, cov, rng = _mixture_model(ctype, 32)
    N, M, D = mu.shape
    obs = _simulate(model, (1000,) * 4, rng)
    smp = bhmm_amd.BayesianGaussianMixtureHMMSampler(obs, N, initial_model=model, reversible=reversible,
                                                     weights_prior=np.array([[1.0, 2.0], [0.5, 1.0]]))
    smp._update(seed=4242, keep_paths=True)
    paths, labels = smp.model.hidden_state_trajectories, smp.component_labels
    for p, l in zip(paths, labels):
        assert np.array_equal(l // M, p)
    packed = _numpy_stats(obs, paths, labels, mu, ctype)
    draw = GibbsParametersGmm(N, M, D, ctype, prior_C=smp.prior_C, prior_n0=smp.prior_n0, prior_w=smp.prior_w,
                              reversible=reversible, stationary=False, nsteps=smp.transition_matrix_sampling_steps)
    T, p0, w2, m2, c2 = draw(packed, w, mu, cov, smp._param_seed, smp._sweep)
    om = smp.model.output_model
    np.testing.assert_allclose(smp.model.transition_matrix, T, rtol=1e-9)
    np.testing.assert_allclose(smp.model.initial_distribution, p0, rtol=1e-9)
    np.testing.assert_allclose(om.weights, w2, rtol=1e-9)
    np.testing.assert_allclose(om.means, m2, rtol=1e-9)
    np.testing.assert_allclose(om.covariances, c2, rtol=1e-9, atol=1e-12)
    assert not np.array_equal(m2, mu) and not np.array_equal(w2, w)


def test_numpy_parameter_path():
    import bhmm_amd
    model, A, pi, w, mu, cov, rng = _mixture_model('full', 42)
    obs = _simulate(model, (1000,) * 4, rng)
    smp = bhmm_amd.BayesianGaussianMixtureHMMSampler(obs, 2, initial_model=model, native_parameters=False)
    smp._rng = np.random.RandomState(3)
    for _ in range(3):
        smp._update(seed=None, keep_paths=False)
    om = smp.model.output_model
    assert np.all(np.isfinite(om.means)) and not np.array_equal(om.means, mu)
    np.testing.assert_allclose(om.weights.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    for c in om.covariances.reshape(-1, 2, 2):
        assert np.array_equal(c, c.T)
        np.linalg.cholesky(c)


# ---- 8. M = 1 against the multivariate gaussian sampler --------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
def test_one_component_follows_the_mvgaussian_sampler(ctype):
    import bhmm_amd
    from tests.test_mvn_gibbs_gpu import _model, _simulate as _simulate_mvn
    n, D = 3, 2
    A, pi, mu, cov = _model(n, D, 51, ctype)
    obs, _ = _simulate_mvn(A, pi, mu, cov, (500,) * 4, 52)
    m = bhmm_amd.BayesianHMMSampler(obs, n, output='mvgaussian',
                                    initial_model=bhmm_amd.mvgaussian_hmm(pi, A, mu, cov, covariance_type=ctype))
    g = bhmm_amd.BayesianGaussianMixtureHMMSampler(
        obs, n, initial_model=bhmm_amd.gaussian_mixture_hmm(pi, A, np.ones((n, 1)), mu[:, None], cov[:, None],
                                                            covariance_type=ctype))
    for sweep in range(5):
        seed = 5 if sweep == 0 else None
        m._update(seed=seed, keep_paths=True)
        g._update(seed=seed, keep_paths=True)
        for a, b in zip(m.model.hidden_state_trajectories, g.model.hidden_state_trajectories):
            assert np.array_equal(a, b), sweep
        np.testing.assert_allclose(g.model.output_model.means[:, 0], m.model.output_model.means, rtol=1e-9)
        np.testing.assert_allclose(g.model.output_model.covariances[:, 0], m.model.output_model.covariances, rtol=1e-9)
        np.testing.assert_allclose(g.model.transition_matrix, m.model.transition_matrix, rtol=1e-9)
        assert np.array_equal(g.model.output_model.weights, np.ones((n, 1)))


# ---- 9. a chain ------------------------------------------------------------------------------------------------
def test_chain():
    import bhmm_amd
    model, A, pi, w, mu, cov, rng = _mixture_model('full', 61)
    N, M, D = mu.shape
    obs = _simulate(model, (2000,) * 8, rng)
    a = bhmm_amd.bayesian_gaussian_mixture_hmm(obs, model, nsample=50, seed=9)
    b = bhmm_amd.bayesian_gaussian_mixture_hmm(obs, copy.deepcopy(model), nsample=50, seed=9)
    assert len(a.sampled_hmms) == 50
    for ha, hb in zip(a.sampled_hmms, b.sampled_hmms):
        assert np.array_equal(ha.transition_matrix, hb.transition_matrix)
        assert np.array_equal(ha.initial_distribution, hb.initial_distribution)
        assert np.array_equal(ha.output_model.weights, hb.output_model.weights)
        assert np.array_equal(ha.output_model.means, hb.output_model.means)
        assert np.array_equal(ha.output_model.covariances, hb.output_model.covariances)
        for c in ha.output_model.covariances.reshape(-1, D, D):
            np.linalg.cholesky(c)
        np.testing.assert_allclose(ha.output_model.weights.sum(axis=1), 1.0, rtol=0, atol=4e-16)
    assert np.all(np.abs(a.means_mean - mu) <= 0.1)                        # sigma = 1
    assert np.all(np.abs(a.weights_mean - w) <= 0.05)                      # posterior sd about 0.008
    assert a.weights_std.shape == (N, M) and np.shape(a.weights_conf) == (2, N, M)
    assert a.means_std.shape == (N, M, D) and np.shape(a.covariances_conf) == (2, N, M, D, D)
    logL = bhmm_amd.score(obs, a)
    assert logL.shape == (50,) and np.all(np.isfinite(logL))
    for fn in (bhmm_amd.bayesian_hmm, bhmm_amd.bayesian_mvgaussian_hmm):
        with pytest.raises(NotImplementedError):
            fn(obs, model)
    with pytest.raises(NotImplementedError):
        bhmm_amd.BayesianHMMSampler(obs, N, initial_model=model)
    eng = _engine(obs[:1], N)
    try:
        with pytest.raises(NotImplementedError):
            eng.path_moments(np.zeros(2000, dtype=np.int32), mu)
        with pytest.raises(NotImplementedError):
            eng.sample_paths_moments(A, pi, *model.output_model.parameters())
    finally:
        eng.close()
