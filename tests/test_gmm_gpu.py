"""GPU: gaussian-mixture emissions per state -- k_gmm_rows (bhmm_gmm_emissions, bhmm_logpdf_gmm), k_gmm_weights and the
moment kernels over the components (bhmm_gmm_moments), GmmEngine, MaximumLikelihoodEstimator(output=
'gaussian_mixture') and the functional wrappers.

The yardsticks are written here in numpy and use none of the code under test:
  L_ti     a long-double log-sum-exp over long-double component densities, each by forward substitution by hand on a
           Cholesky factor made by hand.  Bound: max over the components with w > 0 of
           [b_tic + 2 eps (|log w_ic| + |l_tic|)], plus 16 M eps, plus 4 eps |L_ti|, with b_tic = 64 D eps kappa_2
           (1 + |z|^2) + 16 eps |c| the bound on l of tests/test_mvn_gpu.py: a log-sum-exp moves by at most the
           largest perturbation of its arguments; the M exps, rescalings and additions each carry a couple of ulp
           on a sum in [1, M]; the last addition rounds eps |L|; the factor 2 is the margin.  A float64 numpy
           implementation with the online sum stays at 0.21 of it on these cases.
  log r    error <= the bound of a_tic plus the bound of L_ti; sum_c exp(log r) = 1 within (M + 8) eps.
  moments  math.fsum over numpy terms made from the fetched weights, bound 1e-12 (1 + sum |term|) per entry.
  the rest the oracle's forward / backward on float64 numpy-made mixture rows, an explicit-kind Engine fed those rows,
           and MvnEngine on the expanded N M-state model.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
PI_LD = 4 * np.arctan(LD(1))
LENGTHS = (300, 0, 1, 411)      # 712 steps: three workgroups, the last one partial; an empty and a one-step trajectory


# ---- the yardsticks --------------------------------------------------------------------------------------
def _chol_ld(S):
    D = S.shape[0]
    S = S.astype(LD)
    L = np.zeros((D, D), dtype=LD)
    for a in range(D):
        for b in range(a + 1):
            s = S[a, b] - (L[a, :b] * L[b, :b]).sum()
            L[a, b] = np.sqrt(s) if a == b else s / L[b, b]
    return L


def _l_ref(x, mu, cov, ctype):
    """l (T, n) in long double by forward substitution, |z|^2 (T, n), c (n,), kappa_2(L_i) (n,) of n gaussians"""
    T, D = x.shape
    n = mu.shape[0]
    l = np.empty((T, n), dtype=LD)
    z2 = np.empty((T, n))
    c = np.empty(n, dtype=LD)
    kappa = np.empty(n)
    for i in range(n):
        d = x.astype(LD) - mu[i].astype(LD)
        if ctype == 'diag':
            sd = np.sqrt(cov[i].astype(LD))
            z = d / sd
            c[i] = -np.log(sd).sum() - LD(D) / 2 * np.log(2 * PI_LD)
            kappa[i] = float(sd.max() / sd.min())
        else:
            L = _chol_ld(cov[i])
            z = np.zeros((T, D), dtype=LD)
            for a in range(D):
                z[:, a] = (d[:, a] - (z[:, :a] * L[a, :a]).sum(axis=1)) / L[a, a]
            c[i] = -np.log(np.diag(L)).sum() - LD(D) / 2 * np.log(2 * PI_LD)
            kappa[i] = np.linalg.cond(L.astype(np.float64))
        q = (z * z).sum(axis=1)
        l[:, i] = -q / 2 + c[i]
        z2[:, i] = q.astype(np.float64)
    return l, z2, c.astype(np.float64), kappa


def _mix_ref(x, w, mu, cov, ctype):
    """Long double: a (T, N, M) (-inf where w = 0), L (T, N); float64: the bound on a (T, N, M; 0 where w = 0) and
    the bound on L (T, N)."""
    N, M, D = mu.shape
    l, z2, c, kappa = _l_ref(x, mu.reshape(N * M, D), cov.reshape((N * M,) + cov.shape[2:]), ctype)
    T = x.shape[0]
    b = (64 * D * EPS * kappa[None, :] * (1.0 + z2) + 16 * EPS * np.abs(c)[None, :]).reshape(T, N, M)
    l = l.reshape(T, N, M)
    pos = w > 0
    logw = np.full((N, M), -np.inf, dtype=LD)
    logw[pos] = np.log(w[pos].astype(LD))
    a = l + logw[None]
    amax = a.max(axis=2)
    L = amax + np.log(np.exp(a - amax[:, :, None]).sum(axis=2))
    lw64 = np.where(pos, np.abs(logw.astype(np.float64)), 0.0)
    ba = np.where(pos[None], b + 2 * EPS * (lw64[None] + np.abs(l.astype(np.float64))), 0.0)
    bL = ba.max(axis=2) + 16 * M * EPS + 4 * EPS * np.abs(L.astype(np.float64))
    return a, L, ba, bL


def _np_l(x, mu, cov, ctype):
    """float64 numpy: l (T, n) of n gaussians"""
    T, D = x.shape
    n = mu.shape[0]
    l = np.empty((T, n))
    for i in range(n):
        d = x - mu[i]
        if ctype == 'diag':
            sd = np.sqrt(cov[i])
            z = d / sd
            logdet = np.log(sd).sum()
        else:
            L = np.linalg.cholesky(cov[i])
            z = np.linalg.solve(L, d.T).T
            logdet = np.log(np.diag(L)).sum()
        l[:, i] = -0.5 * (z * z).sum(axis=1) - logdet - 0.5 * D * math.log(2 * math.pi)
    return l


def _np_mix(x, w, mu, cov, ctype):
    """float64 numpy: L (T, N), the responsibilities r (T, N, M), m (T,), the scaled rows (T, N)"""
    N, M, D = mu.shape
    l = _np_l(x, mu.reshape(N * M, D), cov.reshape((N * M,) + cov.shape[2:]), ctype).reshape(-1, N, M)
    with np.errstate(divide='ignore'):
        a = l + np.log(w)[None]
    amax = a.max(axis=2)
    e = np.exp(a - amax[:, :, None])
    s = e.sum(axis=2)
    L = amax + np.log(s)
    m = L.max(axis=1)
    return L, e / s[:, :, None], m, np.exp(L - m[:, None])


def _np_scaled(obs, w, mu, cov, ctype):
    """per trajectory the numpy-made rows, m_t and responsibilities, and the shifts"""
    N, M, _ = mu.shape
    rows, ms, rs = [], [], []
    for o in obs:
        if len(o):
            _, r, m, row = _np_mix(o, w, mu, cov, ctype)
        else:
            m, row, r = np.zeros(0), np.zeros((0, N)), np.zeros((0, N, M))
        rows.append(row), ms.append(m), rs.append(r)
    return rows, ms, np.array([math.fsum(m.tolist()) for m in ms]), rs


def _oracle_estep(rows, A, pi):
    from oracle import oracle as orc
    n = A.shape[0]
    logL = np.zeros(len(rows))
    g0, C, sc, gammas = np.zeros(n), np.zeros((n, n)), np.zeros(n), []
    for k, r in enumerate(rows):
        if len(r) == 0:
            gammas.append(np.zeros((0, n)))
            continue
        logL[k], alpha = orc.forward(A, r, pi)
        beta = orc.backward(A, r)
        g = orc.gamma(alpha, beta)
        gammas.append(g)
        g0 += g[0]
        sc += g.sum(axis=0)
        if len(r) > 1:
            C += orc.transition_counts(alpha, beta, A, r)
    return dict(logL=logL, gamma0_sum=g0, C=C, state_counts=sc, gammas=gammas)


# ---- inputs ------------------------------------------------------------------------------------------------
def _rand_cov(rng, D, scale, kappa):
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    s = scale * np.logspace(0, -math.log10(kappa), D) if D > 1 else np.array([scale])
    Lm = Q * s[None, :]
    S = Lm.dot(Lm.T)
    return 0.5 * (S + S.T)


def _mix_case(D, N, M, ctype, rng, lengths=LENGTHS, zero_first=True):
    """N M components with kappa_2(L) <= 1e3 and scales from 1e-2 to 1e2, points out to 30 sigma of a component;
    Dirichlet(0.5) weights, w[0, 0] = 0 wherever M > 1 (the first component is the skipped one)"""
    n = N * M
    scales = 10.0 ** rng.uniform(-2, 2, n)
    kap = 10.0 ** rng.uniform(0, 3, n)
    if ctype == 'full':
        cov = np.array([_rand_cov(rng, D, s, k) for s, k in zip(scales, kap)])
        fac = np.array([np.linalg.cholesky(c) for c in cov])
    else:
        sd = np.array([s * np.logspace(0, -math.log10(k), D)[rng.permutation(D)] if D > 1 else np.array([s])
                       for s, k in zip(scales, kap)])
        cov = sd * sd
        fac = np.array([np.diag(s) for s in sd])
    mu = rng.normal(size=(n, D)) * 3.0 * scales[:, None]
    w = rng.dirichlet(np.full(M, 0.5), N) if M > 1 else np.ones((N, 1))
    if M > 1 and zero_first:
        w[0, 0] = 0.0
        w[0] /= w[0].sum()
    obs = []
    for T in lengths:
        j = rng.integers(0, n, T)
        f = rng.choice([1.0, 1.0, 1.0, 5.0, 30.0], T)
        g = rng.normal(size=(T, D)) / math.sqrt(D) * f[:, None]
        obs.append(mu[j] + np.einsum('tab,tb->ta', fac[j], g) if T else np.zeros((0, D)))
    return obs, w, mu.reshape(N, M, D), cov.reshape((N, M) + cov.shape[1:])


def _par(w, mu, cov):
    return np.concatenate([w[:, :, None], mu], axis=2), cov


def _engine(obs, n):
    from bhmm_amd.engine import GmmEngine
    eng = GmmEngine(0)
    eng.set_observations('gaussian_mixture', obs, n)
    return eng


_CASES_NM = [(1, 1), (1, 2), (3, 3), (2, 5), (1, 16), (2, 17)]


def _density_cases():
    out = []
    for D in (1, 2, 5, 17, 64):
        for N, M in _CASES_NM:
            if D == 64 and (N, M) not in ((1, 2), (3, 3)):
                continue
            for ctype in ('full', 'diag'):
                out.append((D, N, M, ctype))
    return out


# ---- 1. mixture log-densities ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,M,ctype", _density_cases())
def test_log_densities(D, N, M, ctype):
    from bhmm_amd import GaussianMixtureOutputModel
    rng = np.random.default_rng(10000 * D + 100 * N + 2 * M + (ctype == 'diag'))
    obs, w, mu, cov = _mix_case(D, N, M, ctype, rng)
    x = np.concatenate(obs, axis=0)
    _, Lref, _, bL = _mix_ref(x, w, mu, cov, ctype)
    L = GaussianMixtureOutputModel(N, w, mu, cov, covariance_type=ctype).log_p_obs(x)
    err = np.abs((L.astype(LD) - Lref).astype(np.float64))
    print("D=%d N=%d M=%d %s: L error / bound = %.3g" % (D, N, M, ctype, (err / bL).max()))
    assert np.all(err <= bL), "L error %.3g x the bound" % (err / bL).max()


# ---- 2. rows, m_t, shifts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("D,N,M", [(2, 3, 3), (5, 2, 5), (17, 1, 16), (3, 20, 2)])
def test_rows_scales_and_shifts(D, N, M, ctype):
    """(3, 20, 2): N M > 16 and N > 16 -- the raw L is parked in the rows and they are rescaled at the end"""
    from bhmm_amd import GaussianMixtureOutputModel
    rng = np.random.default_rng(20000 * D + 100 * N + 2 * M + (ctype == 'diag'))
    obs, w, mu, cov = _mix_case(D, N, M, ctype, rng)
    x = np.concatenate(obs, axis=0)
    _, _, _, bL = _mix_ref(x, w, mu, cov, ctype)
    L = GaussianMixtureOutputModel(N, w, mu, cov, covariance_type=ctype).log_p_obs(x)
    eng = _engine(obs, N)
    try:
        eng.emissions(*_par(w, mu, cov))
        rows, m, shift = eng.emission_rows(), eng.step_scales(), eng.shifts
        # ... and the same with responsibilities: the blocks of states are half as wide then
        eng.emissions(*_par(w, mu, cov), want_resp=True)
        rows2, m2, shift2 = eng.emission_rows(), eng.step_scales(), eng.shifts
    finally:
        eng.close()
    assert np.array_equal(m, L.max(axis=1))
    assert np.all(rows.max(axis=1) == 1.0)
    assert np.array_equal(rows, rows2) and np.array_equal(m, m2) and np.array_equal(shift, shift2)
    rown = np.exp(L.astype(LD) - m.astype(LD)[:, None]).astype(np.float64)
    big = rown >= 1e-290
    rel = bL + 4 * EPS
    rerr = np.abs(rows - rown)
    print("D=%d N=%d M=%d %s: row error / bound = %.3g" % (D, N, M, ctype, (rerr[big] / (rown[big] * rel[big])).max()))
    assert np.all(rerr[big] <= rown[big] * rel[big])
    assert np.all(rows[~big] < 2e-290)
    off = np.concatenate([[0], np.cumsum([len(o) for o in obs])])
    for k in range(len(obs)):
        mk = m[off[k]:off[k + 1]]
        want = math.fsum(mk.tolist())
        tol = (-(-len(mk) // 256) + 9) * EPS * np.abs(mk).sum()
        assert abs(shift[k] - want) <= tol, k
        if len(mk) <= 1:
            assert shift[k] == want


# ---- 3. one component is the existing kind ---------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("N", [3, 20])
@pytest.mark.parametrize("D", [2, 17])
def test_one_component_is_the_multivariate_gaussian_kind_bitwise(D, N, ctype):
    from bhmm_amd.engine import MvnEngine
    rng = np.random.default_rng(300 * D + N)
    obs, w, mu, cov = _mix_case(D, N, 1, ctype, rng)
    assert np.all(w == 1.0)
    mv = MvnEngine(0)
    gm = _engine(obs, N)
    try:
        mv.set_observations('mvgaussian', obs, N)
        mv.emissions(mu[:, 0], cov[:, 0])
        a = (mv.emission_rows(), mv.step_scales(), mv.shifts)
        for resp in (False, True):
            gm.emissions(*_par(w, mu, cov), force=True, want_resp=resp)
            b = (gm.emission_rows(), gm.step_scales(), gm.shifts)
            for u, v in zip(a, b):
                assert np.array_equal(u.view(np.int64), v.view(np.int64))
        assert np.all(gm.responsibilities() == 0.0)
    finally:
        mv.close()
        gm.close()


# ---- 4. log responsibilities -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("D,N,M", [(2, 3, 3), (5, 2, 5), (17, 2, 17), (3, 20, 2), (1, 1, 16)])
def test_log_responsibilities(D, N, M, ctype):
    rng = np.random.default_rng(40000 * D + 100 * N + 2 * M + (ctype == 'diag'))
    obs, w, mu, cov = _mix_case(D, N, M, ctype, rng)
    x = np.concatenate(obs, axis=0)
    aref, Lref, ba, bL = _mix_ref(x, w, mu, cov, ctype)
    eng = _engine(obs, N)
    try:
        eng.emissions(*_par(w, mu, cov), want_resp=True)
        lr = eng.responsibilities()
    finally:
        eng.close()
    assert lr.shape == (x.shape[0], N, M)
    pos = w > 0
    assert np.all(lr[:, ~pos] == -np.inf)                               # a zero weight: exactly -inf
    assert np.all(lr[:, pos] <= 0.0)
    ref = aref - Lref[:, :, None]
    err = np.abs((lr[:, pos].astype(LD) - ref[:, pos]).astype(np.float64))
    bound = (ba + bL[:, :, None])[:, pos]
    print("D=%d N=%d M=%d %s: log r error / bound = %.3g" % (D, N, M, ctype, (err / bound).max()))
    assert np.all(err <= bound)
    tot = np.array([[math.fsum(np.exp(lr[t, i]).tolist()) for i in range(N)] for t in range(x.shape[0])])
    print("D=%d N=%d M=%d %s: |sum_c r - 1| / eps = %.3g" % (D, N, M, ctype, np.abs(tot - 1.0).max() / EPS))
    assert np.all(np.abs(tot - 1.0) <= (M + 8) * EPS)


def test_nan_observation_spoils_its_own_trajectory_only():
    rng = np.random.default_rng(9)
    N, M = 3, 3
    obs, w, mu, cov = _mix_case(2, N, M, 'full', rng, lengths=(300, 1, 411))
    obs[2][100, 1] = np.nan
    eng = _engine(obs, N)
    try:
        eng.emissions(*_par(w, mu, cov), want_resp=True)
        rows, m, shift, lr = eng.emission_rows(), eng.step_scales(), eng.shifts, eng.responsibilities()
    finally:
        eng.close()
    t = 300 + 1 + 100
    assert np.all(np.isnan(rows[t])) and np.isnan(m[t]) and np.isnan(shift[2]) and np.all(np.isnan(lr[t]))
    assert np.all(np.isfinite(np.delete(rows, t, axis=0))) and np.all(np.isfinite(np.delete(m, t)))
    assert np.all(np.isfinite(shift[:2]))
    assert np.all(np.isfinite(np.delete(lr, t, axis=0)[:, w > 0])) and not np.any(np.isnan(np.delete(lr, t, axis=0)))


# ---- 5. moments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("N,M", [(3, 3), (2, 17)])
@pytest.mark.parametrize("D", [2, 5, 17])
def test_moments(D, N, M, ctype):
    import torch
    from bhmm_amd.output_models.gaussian_mixture import unpack_component_moments
    rng = np.random.default_rng(50000 * D + 100 * N + 2 * M + (ctype == 'diag'))
    obs, w, mu, cov = _mix_case(D, N, M, ctype, rng)
    x = np.concatenate(obs, axis=0)
    T = x.shape[0]
    g = rng.random((T, N)) ** 3 + 1e-6
    eng = _engine(obs, N)
    try:
        gd = torch.from_numpy(g).to('cuda:0')
        eng.emissions(*_par(w, mu, cov), want_resp=True)
        lr = eng.responsibilities()
        a = eng.moments(gd, None, ctype)
        u = eng.responsibilities()
        with pytest.raises(ValueError):                                 # the log responsibilities are used up
            eng.moments(gd, None, ctype)
        eng.emissions(*_par(w, mu, cov), want_resp=True)                # (made again: they were used up)
        b = eng.moments(gd, None, ctype)
    finally:
        eng.close()
    assert np.array_equal(a.view(np.int64), b.view(np.int64))           # bitwise the same from call to call
    want_u = g[:, :, None] * np.exp(lr)
    assert np.all(np.abs(u - want_u) <= 4 * EPS * want_u)
    S0, S1, S2 = unpack_component_moments(a, N, M, D, ctype)
    worst = 0.0
    for i in range(N):
        for c in range(M):
            d = x - mu[i, c]
            uu = u[:, i, c]
            terms = [(S0[i, c], uu)]
            terms += [(S1[i, c, p], uu * d[:, p]) for p in range(D)]
            if ctype == 'full':
                terms += [(S2[i, c, p, q], uu * d[:, p] * d[:, q]) for p in range(D) for q in range(p + 1)]
            else:
                terms += [(S2[i, c, p], uu * d[:, p] * d[:, p]) for p in range(D)]
            for got, t in terms:
                bound = 1e-12 * (1.0 + np.abs(t).sum())
                err = abs(got - math.fsum(t.tolist()))
                worst = max(worst, err / bound)
                assert err <= bound
    print("moments D=%d N=%d M=%d %s: largest error / bound = %.3g" % (D, N, M, ctype, worst))


# ---- 6 .. 9: one synthetic problem per shape ---------------------------------------------------------------------
def _problem(n, M, D, seed, T=(700, 333, 1, 1200), ctype='full'):
    """an n-state model whose states are 8 apart along the first axis and whose components sit 2.5 apart along the
    second (the last), moderate covariances, and trajectories drawn from it"""
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) * 0.2 + np.eye(n) * 3.0
    A /= A.sum(axis=1)[:, None]
    pi = rng.random(n) + 0.5
    pi /= pi.sum()
    w = rng.dirichlet(np.full(M, 4.0), n)
    mu = rng.normal(size=(n, M, D)) * 0.3
    mu[:, :, 0] += 8.0 * np.arange(n)[:, None]
    mu[:, :, -1] += 2.5 * np.arange(M)[None, :]
    cov = np.array([[_rand_cov(rng, D, rng.uniform(0.7, 1.2), 3.0) for _ in range(M)] for _ in range(n)])
    fac = np.array([[np.linalg.cholesky(c) for c in cc] for cc in cov])
    if ctype == 'diag':
        cov = np.einsum('icaa->ica', cov).copy()
        fac = np.array([[np.diag(np.sqrt(c)) for c in cc] for cc in cov])
    obs, paths, comps = [], [], []
    for Tk in T:
        s = np.zeros(Tk, dtype=np.int64)
        u = rng.random(Tk)
        for t in range(Tk):
            p = pi if t == 0 else A[s[t - 1]]
            s[t] = min(n - 1, np.searchsorted(np.cumsum(p), u[t]))
        v = rng.random(Tk)
        c = np.array([min(M - 1, np.searchsorted(np.cumsum(w[s[t]]), v[t])) for t in range(Tk)], dtype=np.int64)
        obs.append(mu[s, c] + np.einsum('tab,tb->ta', fac[s, c], rng.normal(size=(Tk, D))) if Tk else np.zeros((0, D)))
        paths.append(s)
        comps.append(c)
    return A, pi, w, mu, cov, obs, paths, comps


@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("n", [3, 9])
def test_estep_against_the_oracle(n, M, ctype):
    A, pi, w, mu, cov, obs, _, _ = _problem(n, M, 2, 11 * n + M, ctype=ctype)
    rows, _, shifts, rs = _np_scaled(obs, w, mu, cov, ctype)
    ref = _oracle_estep(rows, A, pi)
    want = ref['logL'] + shifts
    p0, p1 = _par(w, mu, cov)
    eng = _engine(obs, n)
    try:
        res = eng.estep(A, pi, p0, p1)
        packed = eng.estep_fetch_packed()
        sc = eng.score([(A, pi, p0, p1)])
    finally:
        eng.close()
    np.testing.assert_allclose(res.logL_k, want, rtol=1e-11)
    np.testing.assert_allclose(sc[0], res.logL_k, rtol=1e-11)
    assert abs(res.loglik - want.sum()) <= 1e-11 * abs(want.sum())
    for got, want_ in ((res.C, ref['C']), (res.gamma0_sum, ref['gamma0_sum'])):
        big = want_ >= 1e-290
        np.testing.assert_allclose(got[big], want_[big], rtol=1e-9)
        assert np.all(got[~big] < 2e-290)
    np.testing.assert_allclose(res.state_counts, ref['state_counts'], rtol=1e-9)
    S0 = sum((g[:, :, None] * r).sum(axis=0) for g, r in zip(ref['gammas'], rs))
    assert res.kind == 'gaussian_mixture' and res.S0.shape == (n, M) and res.S1.shape == (n, M, 2)
    assert res.S2.shape == ((n, M, 2, 2) if ctype == 'full' else (n, M, 2))
    np.testing.assert_allclose(res.S0, S0, rtol=1e-9)
    assert packed.shape == (1 + n + n * n + n + res.moments.size,) and packed[0] == res.loglik
    assert np.array_equal(packed[-res.moments.size:], res.moments)


def test_against_the_expanded_model_on_the_multivariate_gaussian_engine():
    """(N, M) = (3, 3) against MvnEngine on 9 states, A'[(i,c),(j,c')] = A_ij w_jc', pi'[(i,c)] = pi_i w_ic: the two
    sides run on different kernel families (up to 8 states against 9 to 64)."""
    from bhmm_amd.engine import MvnEngine
    n, M, D = 3, 3, 2
    A, pi, w, mu, cov, obs, _, _ = _problem(n, M, D, 77)
    rng = np.random.default_rng(1)
    mu = mu + rng.normal(size=mu.shape) * 0.3                            # (a model some way off the generating one)
    Ax = np.repeat((A[:, :, None] * w[None, :, :]).reshape(n, n * M), M, axis=0)
    pix = (pi[:, None] * w).reshape(n * M)
    p0, p1 = _par(w, mu, cov)
    gm = _engine(obs, n)
    mv = MvnEngine(0)
    try:
        a = gm.estep(A, pi, p0, p1)
        ga = gm.posterior_marginals(A, pi, p0, p1)
        mv.set_observations('mvgaussian', obs, n * M)
        b = mv.estep(Ax, pix, mu.reshape(n * M, D), cov.reshape(n * M, D, D))
        gb = mv.posterior_marginals(Ax, pix, mu.reshape(n * M, D), cov.reshape(n * M, D, D))
    finally:
        gm.close()
        mv.close()
    np.testing.assert_allclose(a.logL_k, b.logL_k, rtol=2e-11)
    np.testing.assert_allclose(a.S0.reshape(-1), b.S0, rtol=2e-9)
    np.testing.assert_allclose(a.S1.reshape(n * M, D), b.S1, rtol=2e-9)
    np.testing.assert_allclose(a.S2.reshape(n * M, D, D), b.S2, rtol=2e-9)
    for x, y in zip(ga, gb):
        np.testing.assert_allclose(x, y.reshape(-1, n, M).sum(axis=2), rtol=0, atol=1e-9)


@pytest.mark.parametrize("n", [3, 9])
def test_every_call_equals_the_explicit_engine_on_numpy_rows(n):
    from bhmm_amd.engine import Engine
    M = 2
    A, pi, w, mu, cov, obs, paths, _ = _problem(n, M, 2, 40 + n)
    rows, ms, shifts, _ = _np_scaled(obs, w, mu, cov, 'full')
    p0, p1 = _par(w, mu, cov)
    ex = Engine(0)
    gm = _engine(obs, n)
    W = np.random.default_rng(0).random((n, n, 2))
    flat = np.concatenate(paths).astype(np.int32)
    u = [np.random.default_rng(5).random(len(o)) for o in obs]
    try:
        ex.set_observations('explicit', rows, n)
        for a, b in zip(gm.viterbi(A, pi, p0, p1), ex.viterbi(A, pi)):
            assert np.array_equal(a, b)
        for a, b in zip(gm.posterior_decode(A, pi, p0, p1), ex.posterior_decode(A, pi)):
            assert np.array_equal(a, b)
        for a, b in zip(gm.posterior_marginals(A, pi, p0, p1), ex.posterior_marginals(A, pi)):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)
        for a, b in zip(gm.posterior_transitions(A, pi, p0, p1), ex.posterior_transitions(A, pi)):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)
        for a, b in zip(gm.posterior_transitions(A, pi, p0, p1, weights=W), ex.posterior_transitions(A, pi, weights=W)):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)
        fr, fl = gm.filter_states(A, pi, p0, p1)
        er, el = ex.filter_states(A, pi)
        ll = gm.score([(A, pi, p0, p1)])[0]
        for k in range(len(obs)):
            np.testing.assert_allclose(fr[k], er[k], rtol=0, atol=1e-9)
            np.testing.assert_allclose(fl[k], el[k] + ms[k], rtol=0, atol=1e-9)
            assert abs(math.fsum(fl[k].tolist()) - ll[k]) <= 1e-11 * max(1.0, abs(ll[k]))
        got = gm.path_logprob(flat, [(A, pi, p0, p1)])
        want = ex.path_logprob(flat, [(A, pi, None, None)]) + shifts[None, :]
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(gm.decode_logprob(A, pi, p0, p1), ex.decode_logprob(A, pi) + shifts, rtol=1e-11,
                                   atol=1e-11)
        r1, r2 = gm.decode_runs(A, pi, p0, p1, stats=True), ex.decode_runs(A, pi, stats=True)
        assert np.array_equal(r1.start, r2.start) and np.array_equal(r1.state, r2.state)
        assert np.array_equal(r1.jumps, r2.jumps)
        s1, s2 = gm.sample_paths(A, pi, p0, p1, u=u), ex.sample_paths(A, pi, u=u)
        for k in range(len(obs)):
            assert np.array_equal(s1[0][k], s2[0][k])
        assert np.array_equal(s1[1], s2[1]) and np.array_equal(s1[2], s2[2])
        assert gm.kind == 'gaussian_mixture' and gm.dimension == 2 and gm.ncomponents == M
    finally:
        ex.close()
        gm.close()


def test_functional_wrappers_accept_the_model():
    import bhmm_amd
    n, M = 3, 2
    A, pi, w, mu, cov, obs, paths, _ = _problem(n, M, 2, 43)
    obs, paths = obs[:3], paths[:3]
    model = bhmm_amd.gaussian_mixture_hmm(pi, A, w, mu, cov)
    assert model.output_model.model_type == 'gaussian_mixture'
    rows, ms, shifts, _ = _np_scaled(obs, w, mu, cov, 'full')
    ref = _oracle_estep(rows, A, pi)
    np.testing.assert_allclose(bhmm_amd.score(obs, model, per_trajectory=True)[0], ref['logL'] + shifts, rtol=1e-11)
    for a, b in zip(bhmm_amd.posterior_marginals(obs, model), ref['gammas']):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)
    for a, b in zip(bhmm_amd.posterior_decode(obs, model), ref['gammas']):
        assert np.array_equal(a, b.argmax(axis=1))
    jumps = bhmm_amd.posterior_transitions(obs, model)
    assert [len(j) for j in jumps] == [len(o) - 1 for o in obs]
    fr, fl = bhmm_amd.filter_states(obs, model)
    assert abs(sum(float(l.sum()) for l in fl) - (ref['logL'] + shifts).sum()) <= 1e-10 * abs(shifts.sum())
    assert bhmm_amd.decode_segments(obs, model).count >= 3
    lp = bhmm_amd.path_logprob(obs, model, paths=[p.astype(np.int32) for p in paths])
    assert lp.shape == (1, 3) and np.all(np.isfinite(lp)) and np.all(lp[0] <= ref['logL'] + shifts)


# ---- 9. EM ---------------------------------------------------------------------------------------------------------
def _numpy_mstep(obs, gammas, rs, ctype):
    x = np.concatenate(obs, axis=0)
    u = np.concatenate([g[:, :, None] * r for g, r in zip(gammas, rs)], axis=0)
    n, M = u.shape[1:]
    D = x.shape[1]
    S0 = u.sum(axis=0)
    w = S0 / S0.sum(axis=1)[:, None]
    mu, cov = np.empty((n, M, D)), np.empty((n, M, D, D))
    for i in range(n):
        for c in range(M):
            mu[i, c] = (u[:, i, c, None] * x).sum(axis=0) / S0[i, c]
            d = x - mu[i, c]
            cov[i, c] = (u[:, i, c, None, None] * d[:, :, None] * d[:, None, :]).sum(axis=0) / S0[i, c]
    return w, mu, (cov if ctype == 'full' else np.einsum('icaa->ica', cov).copy())


@pytest.mark.parametrize("n,M,ctype", [(3, 2, 'full'), (3, 3, 'diag'), (9, 2, 'full')])
def test_em_step_equals_the_numpy_mstep_on_the_oracles_statistics(n, M, ctype):
    import bhmm_amd
    A, pi, w, mu, cov, obs, _, _ = _problem(n, M, 2, 60 + n, ctype=ctype)
    rng = np.random.default_rng(1)
    mu0 = mu + rng.normal(size=mu.shape) * 0.3
    cov0 = cov * 1.3
    model = bhmm_amd.gaussian_mixture_hmm(pi, A, w, mu0, cov0, covariance_type=ctype)
    rows, _, shifts, rs = _np_scaled(obs, w, mu0, cov0, ctype)
    ref = _oracle_estep(rows, A, pi)
    w1, mu1, cov1 = _numpy_mstep(obs, ref['gammas'], rs, ctype)
    T1 = ref['C'] / ref['C'].sum(axis=1)[:, None]
    pi1 = ref['gamma0_sum'] / ref['gamma0_sum'].sum()
    est = bhmm_amd.MaximumLikelihoodEstimator(obs, n, initial_model=model, reversible=False)
    ll = est.em_step()
    assert abs(ll - (ref['logL'] + shifts).sum()) <= 1e-11 * abs((ref['logL'] + shifts).sum())
    om = est.hmm.output_model
    np.testing.assert_allclose(om.weights, w1, rtol=1e-9)
    np.testing.assert_allclose(om.means, mu1, rtol=1e-9)
    np.testing.assert_allclose(om.covariances, cov1, rtol=1e-9)
    np.testing.assert_allclose(est.hmm.transition_matrix, T1, rtol=1e-9)
    np.testing.assert_allclose(est.hmm.initial_distribution, pi1, rtol=1e-9)


def _synthetic(seed=0):
    """two states, two blobs each: the states 24 apart along the first axis, their blobs 8 apart along the second"""
    rng = np.random.default_rng(seed)
    mu = np.array([[[-12.0, -4.0], [-12.0, 4.0]], [[12.0, -4.0], [12.0, 4.0]]])
    cov = np.array([[[[1.0, 0.3], [0.3, 0.5]], [[0.6, -0.2], [-0.2, 1.2]]],
                    [[[1.5, 0.0], [0.0, 0.4]], [[0.8, 0.2], [0.2, 0.9]]]])
    w = np.array([[0.35, 0.65], [0.6, 0.4]])
    P = np.array([[0.97, 0.03], [0.04, 0.96]])
    fac = np.array([[np.linalg.cholesky(c) for c in cc] for cc in cov])
    obs, paths, comps = [], [], []
    for T in (3000, 2000):
        s = np.zeros(T, dtype=np.int64)
        u = rng.random(T)
        for t in range(1, T):
            s[t] = min(1, np.searchsorted(np.cumsum(P[s[t - 1]]), u[t]))
        c = (rng.random(T) >= w[s, 0]).astype(np.int64)
        obs.append(mu[s, c] + np.einsum('tab,tb->ta', fac[s, c], rng.normal(size=(T, 2))))
        paths.append(s)
        comps.append(c)
    return w, mu, cov, P, obs, paths, comps


def test_ten_em_steps_never_lower_the_likelihood():
    import bhmm_amd
    w, mu, cov, P, obs, _, _ = _synthetic()
    model = bhmm_amd.gaussian_mixture_hmm(np.ones(2) / 2, np.full((2, 2), 0.2) + 0.6 * np.eye(2), np.full((2, 2), 0.5),
                                          mu + 1.0, np.array([[np.eye(2) * 2.0] * 2] * 2))
    assert model.output_model.min_covar == 0.0
    est = bhmm_amd.MaximumLikelihoodEstimator(obs, 2, initial_model=model)
    ll = [est.em_step() for _ in range(10)]
    print("log-likelihoods:", ll)
    for a, b in zip(ll[:-1], ll[1:]):
        assert b - a >= -1e-9 * abs(a)
    assert ll[-1] > ll[0]


def test_a_starved_component_keeps_its_mean_and_covariance():
    import bhmm_amd
    w, mu, cov, P, obs, _, _ = _synthetic()
    mu0 = mu + 0.5
    mu0[1, 1] = [1e3, 1e3]                                              # 1e3 sigma from all data
    cov0 = np.array([[np.eye(2)] * 2] * 2)
    model = bhmm_amd.gaussian_mixture_hmm(np.ones(2) / 2, P, np.array([[0.5, 0.5], [0.7, 0.3]]), mu0, cov0)
    est = bhmm_amd.MaximumLikelihoodEstimator(obs, 2, initial_model=model)
    ll = [est.em_step() for _ in range(4)]
    om = est.hmm.output_model
    assert np.array_equal(om.means[1, 1], mu0[1, 1]) and np.array_equal(om.covariances[1, 1], cov0[1, 1])
    assert om.weights[1, 1] < 1e-8 and abs(om.weights[1].sum() - 1.0) <= 4 * EPS
    for a, b in zip(ll[:-1], ll[1:]):
        assert b - a >= -1e-9 * abs(a)
    assert ll[-1] > ll[0]


def test_estimate_hmm_recovers_the_blobs():
    import bhmm_amd
    w, mu, cov, P, obs, paths, comps = _synthetic()
    hmm = bhmm_amd.estimate_hmm(obs, 2, output='gaussian_mixture', ncomponents=2)
    om = hmm.output_model
    assert om.model_type == 'gaussian_mixture' and om.ncomponents == 2
    s, c = np.concatenate(paths), np.concatenate(comps)
    counts = np.array([[np.sum((s == i) & (c == k)) for k in range(2)] for i in range(2)])
    got_mu, got_w = om.means.reshape(4, 2), om.weights.reshape(4)
    got_state = np.repeat(np.arange(2), 2)
    used = set()
    for i in range(2):
        for k in range(2):
            j = int(np.argmin(((got_mu - mu[i, k]) ** 2).sum(axis=1)))
            assert j not in used
            used.add(j)
            se = np.sqrt(np.diag(cov[i, k]) / counts[i, k])
            dev = np.abs(got_mu[j] - mu[i, k]) / se
            nstate = counts[i].sum()
            share = counts[i, k] / nstate
            se_w = math.sqrt(w[i, k] * (1.0 - w[i, k]) / nstate)
            print("blob (%d, %d): mean off by %s standard errors, weight %.4f (true %.2f, share %.4f, se %.4f)"
                  % (i, k, dev, got_w[j], w[i, k], share, se_w))
            assert np.all(dev <= 3.0)
            assert abs(got_w[j] - w[i, k]) <= 3.0 * se_w
            # the two blobs of a state are components of ONE estimated state
            assert got_state[j] == got_state[int(np.argmin(((got_mu - mu[i, 1 - k]) ** 2).sum(axis=1)))]
    assert len(hmm.hidden_state_trajectories) == 2


# ---- 10. errors -----------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    import bhmm_amd
    from bhmm_amd import _lib
    n, M, D = 2, 2, 2
    A, pi = np.full((n, n), 0.5), np.ones(n) / n
    w = np.full((n, M), 0.5)
    mu = np.zeros((n, M, D))
    mu[:, 1] += 1.0
    cov = np.array([[np.eye(D)] * M] * n)
    obs = [np.random.default_rng(0).normal(size=(50, D))]
    p0, p1 = _par(w, mu, cov)
    eng = _engine(obs, n)

    def usable():
        assert np.all(np.isfinite(eng.score([(A, pi, p0, p1)])))

    try:
        for bad_w in (np.array([[0.5, 0.6], [0.5, 0.5]]), np.array([[1.5, -0.5], [0.5, 0.5]]),
                      np.array([[0.5, np.nan], [0.5, 0.5]])):
            with pytest.raises(ValueError):                                 # (BHMM_ERR_INVALID)
                eng.score([(A, pi) + _par(bad_w, mu, cov)])
            usable()
        with pytest.raises(ValueError):                                     # par0 of the wrong shape
            eng.score([(A, pi, mu, cov)])
        with pytest.raises(ValueError):
            eng.score([(A, pi, p0[:, :, :2], p1)])
        usable()
        with pytest.raises(ValueError):                                     # N M > 4096
            eng.score([(A, pi, np.zeros((n, 2049, 1 + D)), np.ones((n, 2049, D)))])
        rc = _lib.load().bhmm_gmm_emissions(eng._h, 2049, _lib.dp(np.full((n, 2049), 1.0 / 2049)),
                                            _lib.dp(np.zeros((n, 2049, D))), _lib.dp(np.ones((n, 2049, D))),
                                            _lib.COV_DIAG, 0)
        assert rc == _lib.ERR_INVALID
        usable()
        gd = torch.ones(50 * n, dtype=torch.float64, device='cuda:0')
        eng.emissions(p0, p1, force=True)                                   # without responsibilities
        with pytest.raises(ValueError):
            eng.moments(gd, None, 'full')
        usable()
        with pytest.raises(NotImplementedError):
            eng.estep(A, pi, p0, p1, single=True)
        with pytest.raises(NotImplementedError):
            eng.estep_launch(A, pi, p0, p1, stats_dev=gd.data_ptr())
        with pytest.raises(NotImplementedError):
            eng.set_observations_lagged('gaussian_mixture', obs, 2, [(0, 0)], n)
        with pytest.raises(NotImplementedError):
            eng.path_moments(np.zeros(50, dtype=np.int32), mu)
        with pytest.raises(NotImplementedError):
            eng.sample_paths_moments(A, pi, p0, p1)
        with pytest.raises(ValueError):
            eng.set_observations('mvgaussian', obs, n)
        usable()
        assert np.isfinite(eng.estep(A, pi, p0, p1).loglik)
    finally:
        eng.close()
    model = bhmm_amd.gaussian_mixture_hmm(pi, A, w, mu, cov)
    with pytest.raises(NotImplementedError):
        bhmm_amd.MaximumLikelihoodEstimator(obs, n, initial_model=model, process_group=object())
    with pytest.raises(NotImplementedError):
        bhmm_amd.MaximumLikelihoodEstimator(obs, n, initial_model=model, estep_precision='float32')
    with pytest.raises(NotImplementedError):
        bhmm_amd.bayesian_hmm(obs, model)
    with pytest.raises(NotImplementedError):
        bhmm_amd.bayesian_mvgaussian_hmm(obs, model)
    with pytest.raises(NotImplementedError):
        bhmm_amd.BayesianHMMSampler(obs, n, initial_model=model)
    p = bhmm_amd.GaussianMixtureOutputModel(n, w, mu, cov).p_obs(obs[0])
    assert p.shape == (50, n) and np.all(p > 0)
