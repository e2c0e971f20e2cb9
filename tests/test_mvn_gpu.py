"""GPU: multivariate gaussian emissions -- k_mvn_rows / k_mvn_shift (bhmm_mvn_emissions, bhmm_logpdf_mvn),
k_mvn_moments (bhmm_mvn_moments), MvnEngine, MaximumLikelihoodEstimator(output='mvgaussian') and the functional
wrappers.

The yardsticks are written here in numpy and do not use the code under test:
  rows     forward substitution by hand in np.longdouble on a Cholesky factor made by hand in np.longdouble.
           Bound on l_ti: 64 D eps kappa_2(L_i) (1 + |z|^2) + 16 eps |c_i| -- the backward error of a triangular solve
           (D eps per row, amplified by kappa_2(L_i)) carried into -|z|^2 / 2, plus the rounding of the constant; 64 is
           the margin over a float64 numpy implementation, which stays below 0.18 of it on these inputs.
  moments  math.fsum over numpy terms, bound 1e-12 (1 + sum |term|) per entry as in test_path_logprob_gpu.py: a
           thread adds a few hundred terms serially, the slices and partials a few dozen more, each term carries a few
           ulp -- about 1e-14 sum |term|, the factor 100 is the margin.
  the rest the oracle's forward / backward on float64 numpy-made scaled rows, and an explicit-kind Engine fed those
           rows.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
PI_LD = 4 * np.arctan(LD(1))


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
    """l (T, N) in long double by forward substitution, |z|^2 (T, N), c (N,), kappa_2(L_i) (N,)"""
    T, D = x.shape
    N = mu.shape[0]
    l = np.empty((T, N), dtype=LD)
    z2 = np.empty((T, N))
    c = np.empty(N, dtype=LD)
    kappa = np.empty(N)
    for i in range(N):
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


def _l_bound(D, z2, c, kappa):
    return 64 * D * EPS * kappa[None, :] * (1.0 + z2) + 16 * EPS * np.abs(c)[None, :]


def _np_rows(x, mu, cov, ctype):
    """float64 numpy: l, m, the scaled rows"""
    T, D = x.shape
    N = mu.shape[0]
    l = np.empty((T, N))
    for i in range(N):
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
    m = l.max(axis=1)
    return l, m, np.exp(l - m[:, None])


def _np_scaled(obs, mu, cov, ctype):
    """per trajectory the numpy-made rows and m_t, and the shifts"""
    rows, ms = [], []
    for o in obs:
        if len(o):
            _, m, r = _np_rows(o, mu, cov, ctype)
        else:
            m, r = np.zeros(0), np.zeros((0, mu.shape[0]))
        rows.append(r)
        ms.append(m)
    return rows, ms, np.array([math.fsum(m.tolist()) for m in ms])


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


def _rows_case(D, N, ctype, rng, far=False, lengths=(300, 0, 1, 411)):
    """covariances with kappa_2(L_i) <= 1e3 and scales from 1e-2 to 1e2, points out to 30 sigma; far: every mean
    1e6 sigma from the origin"""
    scales = 10.0 ** rng.uniform(-2, 2, N)
    kap = 10.0 ** rng.uniform(0, 3, N)
    if ctype == 'full':
        cov = np.array([_rand_cov(rng, D, s, k) for s, k in zip(scales, kap)])
        fac = np.array([np.linalg.cholesky(c) for c in cov])
    else:
        sd = np.array([s * np.logspace(0, -math.log10(k), D)[rng.permutation(D)] if D > 1 else np.array([s])
                       for s, k in zip(scales, kap)])
        cov = sd * sd
        fac = np.array([np.diag(s) for s in sd])
    mu = rng.normal(size=(N, D)) * 3.0 * scales[:, None]
    if far:
        mu += 1e6 * scales.max() * np.ones(D) / math.sqrt(D)
    # (the default: 712 steps, three workgroups of 256, the last one partial; an empty trajectory, one of one step)
    obs = []
    for T in lengths:
        j = rng.integers(0, N, T)
        f = rng.choice([1.0, 1.0, 1.0, 5.0, 30.0], T)
        g = rng.normal(size=(T, D)) / math.sqrt(D) * f[:, None]
        obs.append(mu[j] + np.einsum('tab,tb->ta', fac[j], g) if T else np.zeros((0, D)))
    return obs, mu, cov


def _engine(obs, n):
    from bhmm_amd.engine import MvnEngine
    eng = MvnEngine(0)
    eng.set_observations('mvgaussian', obs, n)
    return eng


def _check_rows(obs, mu, cov, ctype, label):
    from bhmm_amd import MultivariateGaussianOutputModel
    N, D = mu.shape
    x = np.concatenate(obs, axis=0)
    lref, z2, c, kappa = _l_ref(x, mu, cov, ctype)
    bound = _l_bound(D, z2, c, kappa)
    om = MultivariateGaussianOutputModel(N, mu, cov, covariance_type=ctype)
    l = om.log_p_obs(x)
    err = np.abs((l.astype(LD) - lref).astype(np.float64))
    print("%s: l error / bound = %.3g" % (label, (err / bound).max()))
    assert np.all(err <= bound), "%s: l error %.3g x the bound" % (label, (err / bound).max())
    eng = _engine(obs, N)
    try:
        eng.emissions(mu, cov)
        rows, m, shift = eng.emission_rows(), eng.step_scales(), eng.shifts
    finally:
        eng.close()
    # m_t and the rows are consistent with the l of the same kernel ...
    assert np.array_equal(m, l.max(axis=1))
    assert np.all(rows.max(axis=1) == 1.0)
    # The rows equal exp(l - max l) of those l within the bound on l_ti plus 4 eps, relative (the subtraction rounds
    # eps |l - m|, exp a few ulp).  A row entry below 1e-290 is all but subnormal and carries no relative accuracy:
    # there both must be that small.
    rown = np.exp(l.astype(LD) - m.astype(LD)[:, None]).astype(np.float64)
    big = rown >= 1e-290
    rel = bound + 4 * EPS
    rerr = np.abs(rows - rown)
    print("%s: row error / bound = %.3g" % (label, (rerr[big] / (rown[big] * rel[big])).max()))
    assert np.all(rerr[big] <= rown[big] * rel[big]), label
    assert np.all(rows[~big] < 2e-290), label
    # Against the yardstick's exp(l - max l) an entry carries the error of TWO l: its own and that of the largest
    # one, which no implementation can take out (where the largest l belongs to an ill-conditioned state and the entry
    # to a well-conditioned one, the entry's own bound is a thousandth of the other: measured 1.58 x the entry's own
    # bound + 4 eps at D = 2, N = 9, full, with every l at 0.01 of its bound).  So: the sum of the two bounds, + 4 eps.
    mref = lref.max(axis=1)
    am = lref.argmax(axis=1)
    assert np.all(np.abs((m.astype(LD) - mref).astype(np.float64)) <= bound.max(axis=1))
    rref = np.exp(lref - mref[:, None]).astype(np.float64)
    big = rref >= 1e-290
    rel = bound + bound[np.arange(len(am)), am][:, None] + 4 * EPS
    rerr = np.abs(rows - rref)
    print("%s: row error against the yardstick / bound = %.3g" % (label, (rerr[big] / (rref[big] * rel[big])).max()))
    assert np.all(rerr[big] <= rref[big] * rel[big]), label
    assert np.all(rows[~big] < 2e-290), label
    off = np.concatenate([[0], np.cumsum([len(o) for o in obs])])
    for k in range(len(obs)):
        mk = m[off[k]:off[k + 1]]
        want = math.fsum(mk.tolist())
        # a thread adds every 256th value serially, then eight levels of a tree
        tol = (-(-len(mk) // 256) + 9) * EPS * np.abs(mk).sum()
        assert abs(shift[k] - want) <= tol, (label, k)
        if len(mk) <= 1:
            assert shift[k] == want


# ---- 1. rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("N", [1, 3, 8, 9, 20])
@pytest.mark.parametrize("D", [1, 2, 3, 5, 8, 17, 64])
def test_rows(D, N, ctype):
    rng = np.random.default_rng(1000 * D + 10 * N + (ctype == 'diag'))
    obs, mu, cov = _rows_case(D, N, ctype, rng)
    _check_rows(obs, mu, cov, ctype, "D=%d N=%d %s" % (D, N, ctype))


@pytest.mark.parametrize("ctype", ["full", "diag"])
def test_rows_more_states_than_one_block(ctype):
    """more than ROWS_NB = 16 states at a time go through the rows themselves: 40 is two full blocks and a part"""
    rng = np.random.default_rng(77)
    obs, mu, cov = _rows_case(3, 40, ctype, rng)
    _check_rows(obs, mu, cov, ctype, "D=3 N=40 %s" % ctype)


@pytest.mark.parametrize("ctype", ["full", "diag"])
def test_rows_far_from_the_origin(ctype):
    rng = np.random.default_rng(5)
    obs, mu, cov = _rows_case(3, 3, ctype, rng, far=True)
    _check_rows(obs, mu, cov, ctype, "far %s" % ctype)


def test_nan_observation_spoils_its_own_trajectory_only():
    rng = np.random.default_rng(9)
    obs, mu, cov = _rows_case(2, 3, 'full', rng, lengths=(300, 1, 411))
    A = np.full((3, 3), 0.1) + 0.7 * np.eye(3)
    pi = np.ones(3) / 3
    eng = _engine(obs, 3)
    try:
        clean = eng.score([(A, pi, mu, cov)])[0]
        bad = [o.copy() for o in obs]
        bad[2][100, 1] = np.nan
        eng.set_observations('mvgaussian', bad, 3)
        eng.emissions(mu, cov)
        rows, m, shift = eng.emission_rows(), eng.step_scales(), eng.shifts
        t = 300 + 1 + 100
        assert np.all(np.isnan(rows[t])) and np.isnan(m[t]) and np.isnan(shift[2])
        assert np.all(np.isfinite(np.delete(rows, t, axis=0))) and np.all(np.isfinite(np.delete(m, t)))
        assert np.all(np.isfinite(shift[:2]))
        got = eng.score([(A, pi, mu, cov)])[0]
        assert np.array_equal(got[:2], clean[:2]) and np.isnan(got[2])
    finally:
        eng.close()


# ---- 2. moments --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["full", "diag"])
@pytest.mark.parametrize("D,N", [(1, 1), (2, 3), (3, 8), (5, 9), (8, 20), (17, 3), (64, 2), (1, 100), (2, 100)])
def test_moments(D, N, ctype):
    """(1, 100) and (2, 100): more outputs than one workgroup holds and the widest staging of gamma columns (87 and 53
    states per block of 256 outputs, more than 64 KiB of LDS at D = 1)"""
    import torch
    from bhmm_amd.output_models.mvgaussian import unpack_moments
    rng = np.random.default_rng(100 * D + N)
    lengths = [300, 0, 1, 411]
    T = sum(lengths)
    x = rng.normal(size=(T, D)) * 10.0 ** rng.uniform(-1, 1, D) + 50.0
    mu = 50.0 + rng.normal(size=(N, D))
    g = rng.random((T, N)) ** 3
    g /= g.sum(axis=1)[:, None]
    off = np.concatenate([[0], np.cumsum(lengths)])
    eng = _engine([x[off[k]:off[k + 1]] for k in range(len(lengths))], N)
    try:
        gd = torch.from_numpy(g).to('cuda:0')
        a = eng.moments(gd, mu, ctype)
        b = eng.moments(gd, mu, ctype)
    finally:
        eng.close()
    assert np.array_equal(a.view(np.int64), b.view(np.int64))         # bitwise the same from call to call
    S0, S1, S2 = unpack_moments(a, N, D, ctype)
    worst = 0.0
    for i in range(N):
        d = x - mu[i]
        terms = [(S0[i], g[:, i])]
        terms += [(S1[i, p], g[:, i] * d[:, p]) for p in range(D)]
        if ctype == 'full':
            terms += [(S2[i, p, q], g[:, i] * d[:, p] * d[:, q]) for p in range(D) for q in range(p + 1)]
        else:
            terms += [(S2[i, p], g[:, i] * d[:, p] * d[:, p]) for p in range(D)]
        for got, t in terms:
            bound = 1e-12 * (1.0 + np.abs(t).sum())
            err = abs(got - math.fsum(t.tolist()))
            worst = max(worst, err / bound)
            assert err <= bound
    print("moments D=%d N=%d %s: largest error / bound = %.3g" % (D, N, ctype, worst))


# ---- 3 .. 5: one synthetic problem per (n, D), shared -----------------------------------------------------------
def _problem(n, D, seed, T=(700, 333, 1, 1200), ctype='full'):
    """an n-state model with separated means and moderate covariances, and trajectories drawn from it"""
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) * 0.2 + np.eye(n) * 3.0
    A /= A.sum(axis=1)[:, None]
    pi = rng.random(n) + 0.5
    pi /= pi.sum()
    mu = rng.normal(size=(n, D)) * 0.5
    mu[:, 0] += 6.0 * np.arange(n)
    cov = np.array([_rand_cov(rng, D, rng.uniform(0.7, 1.5), 4.0) for _ in range(n)])
    fac = np.array([np.linalg.cholesky(c) for c in cov])
    if ctype == 'diag':
        cov = np.array([np.diag(c) for c in cov])
        fac = np.array([np.diag(np.sqrt(c)) for c in cov])
    obs, paths = [], []
    for Tk in T:
        s = np.zeros(Tk, dtype=np.int64)
        u = rng.random(Tk)
        for t in range(Tk):
            p = pi if t == 0 else A[s[t - 1]]
            s[t] = min(n - 1, np.searchsorted(np.cumsum(p), u[t]))
        obs.append(mu[s] + np.einsum('tab,tb->ta', fac[s], rng.normal(size=(Tk, D))) if Tk else np.zeros((0, D)))
        paths.append(s)
    return A, pi, mu, cov, obs, paths


@pytest.mark.parametrize("n,D,ctype", [(3, 2, 'full'), (9, 3, 'full'), (3, 5, 'diag'), (70, 2, 'full')])
def test_loglik_and_counts_against_the_oracle(n, D, ctype):
    A, pi, mu, cov, obs, _ = _problem(n, D, 11 * n + D, ctype=ctype)
    rows, _, shifts = _np_scaled(obs, mu, cov, ctype)
    ref = _oracle_estep(rows, A, pi)
    want = ref['logL'] + shifts
    eng = _engine(obs, n)
    try:
        res = eng.estep(A, pi, mu, cov)
        packed = eng.estep_fetch_packed()
        sc = eng.score([(A, pi, mu, cov), (A, pi, mu + 0.01, cov)])
    finally:
        eng.close()
    np.testing.assert_allclose(res.logL_k, want, rtol=1e-11)
    np.testing.assert_allclose(sc[0], want, rtol=1e-11)
    assert abs(res.loglik - want.sum()) <= 1e-11 * abs(want.sum())
    assert np.all(sc[1] != sc[0])                                       # (the second model made its own rows)
    # relative, as everywhere; a count below 1e-290 (a transition between states hundreds of sigma apart) is all but
    # subnormal and has no relative accuracy to hold: there both must be that small
    for got, want_ in ((res.C, ref['C']), (res.gamma0_sum, ref['gamma0_sum'])):
        big = want_ >= 1e-290
        np.testing.assert_allclose(got[big], want_[big], rtol=1e-9)
        assert np.all(got[~big] < 2e-290)
    np.testing.assert_allclose(res.state_counts, ref['state_counts'], rtol=1e-9)
    np.testing.assert_allclose(res.S0, ref['state_counts'], rtol=1e-9)
    assert packed.shape == (1 + n + n * n + n + res.moments.size,) and packed[0] == res.loglik
    assert np.array_equal(packed[-res.moments.size:], res.moments)


def test_one_dimension_equals_the_gaussian_kind():
    from bhmm_amd.engine import Engine
    n = 4
    A, pi, mu, cov, obs, _ = _problem(n, 1, 3)
    sig = np.sqrt(cov[:, 0, 0])
    e1 = Engine(0)
    e2 = _engine(obs, n)
    try:
        e1.set_observations('gaussian', [o[:, 0] for o in obs], n)
        a = e1.estep(A, pi, mu[:, 0], sig)
        b = e2.estep(A, pi, mu, cov)
        c = e2.estep(A, pi, mu, cov[:, :, 0])                          # the diagonal form of the same model
    finally:
        e1.close()
        e2.close()
    for r in (b, c):
        np.testing.assert_allclose(r.logL_k, a.logL_k, rtol=1e-11)
        np.testing.assert_allclose(r.C, a.C, rtol=1e-9)
        # (sum gamma (o - mu) is a difference around zero: its scale is sum gamma times sigma)
        assert np.all(np.abs(r.S1[:, 0] - a.sum_gd) <= 1e-9 * a.state_counts * sig)
        np.testing.assert_allclose(r.S2.reshape(n), a.sum_gdd, rtol=1e-9)


# ---- 4. everything else through the wrapper ----------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 9])
def test_every_call_equals_the_explicit_engine_on_numpy_rows(n):
    """Rows and m_t of the kernel are within 64 D eps kappa (1 + |z|^2) ~ 1e-11 of the numpy ones on this problem
    (D = 2, kappa = 4, |z|^2 < 60); a posterior or filtered probability feels the rows of a mixing time, a few dozen
    steps: 1e-9 absolute.  A path log-probability adds T such terms: 1e-11 of its size.  The decoded paths have
    margins far above that (means six sigma apart)."""
    from bhmm_amd.engine import Engine
    A, pi, mu, cov, obs, paths = _problem(n, 2, 40 + n)
    rows, ms, shifts = _np_scaled(obs, mu, cov, 'full')
    ex = Engine(0)
    mv = _engine(obs, n)
    W = np.random.default_rng(0).random((n, n, 2))
    flat = np.concatenate(paths).astype(np.int32)
    try:
        ex.set_observations('explicit', rows, n)
        for a, b in zip(mv.viterbi(A, pi, mu, cov), ex.viterbi(A, pi)):
            assert np.array_equal(a, b)
        for a, b in zip(mv.posterior_decode(A, pi, mu, cov), ex.posterior_decode(A, pi)):
            assert np.array_equal(a, b)
        for a, b in zip(mv.posterior_marginals(A, pi, mu, cov), ex.posterior_marginals(A, pi)):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)
        for a, b in zip(mv.posterior_transitions(A, pi, mu, cov), ex.posterior_transitions(A, pi)):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)
        for a, b in zip(mv.posterior_transitions(A, pi, mu, cov, weights=W), ex.posterior_transitions(A, pi, weights=W)):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)
        fr, fl = mv.filter_states(A, pi, mu, cov)
        er, el = ex.filter_states(A, pi)
        ll = mv.score([(A, pi, mu, cov)])[0]
        for k in range(len(obs)):
            np.testing.assert_allclose(fr[k], er[k], rtol=0, atol=1e-9)
            np.testing.assert_allclose(fl[k], el[k] + ms[k], rtol=0, atol=1e-9)
            # the increments sum to the log-likelihood
            assert abs(math.fsum(fl[k].tolist()) - ll[k]) <= 1e-11 * max(1.0, abs(ll[k]))
        got = mv.path_logprob(flat, [(A, pi, mu, cov)])
        want = ex.path_logprob(flat, [(A, pi, None, None)]) + shifts[None, :]
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(mv.decode_logprob(A, pi, mu, cov), ex.decode_logprob(A, pi) + shifts, rtol=1e-11,
                                   atol=1e-11)
        r1, r2 = mv.decode_runs(A, pi, mu, cov, stats=True), ex.decode_runs(A, pi, stats=True)
        assert np.array_equal(r1.start, r2.start) and np.array_equal(r1.state, r2.state)
        assert np.array_equal(r1.jumps, r2.jumps)
        assert mv.kind == 'mvgaussian' and mv.dimension == 2
    finally:
        ex.close()
        mv.close()


def test_remaining_wrappers_equal_the_explicit_engine_on_the_same_rows():
    """viterbi_u8, posterior_decode with confidences, the path draws and filter_states into device tensors: the
    wrapper adds the emissions and, for the increments, m_t ON THE DEVICE -- nothing else.  The explicit engine is
    fed the rows the kernel made, so everything but the increments is bitwise equal."""
    import torch
    from bhmm_amd.engine import Engine
    n = 3
    A, pi, mu, cov, obs, _ = _problem(n, 2, 47)
    ex = Engine(0)
    mv = _engine(obs, n)
    try:
        mv.emissions(mu, cov)
        rows, m = mv.emission_rows(), mv.step_scales()
        off = mv.offsets
        total = int(off[-1])
        ex.set_observations('explicit', [rows[off[k]:off[k + 1]] for k in range(len(obs))], n)
        assert np.array_equal(mv.viterbi_u8(A, pi, mu, cov), ex.viterbi_u8(A, pi))
        dev = torch.empty(total, dtype=torch.uint8, device='cuda:0')
        mv.viterbi_u8(A, pi, mu, cov, out=dev)
        assert np.array_equal(dev.cpu().numpy(), ex.viterbi_u8(A, pi))
        (p1, c1), (p2, c2) = mv.posterior_decode(A, pi, mu, cov, confidence=True), ex.posterior_decode(A, pi, confidence=True)
        for k in range(len(obs)):
            assert np.array_equal(p1[k], p2[k]) and np.array_equal(c1[k], c2[k]) and c1[k].dtype == np.float32
        a, b = mv.sample_paths(A, pi, mu, cov, seed=5), ex.sample_paths(A, pi, seed=5)
        for k in range(len(obs)):
            assert np.array_equal(a[0][k], b[0][k])
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] is None and b[3] is None
        assert mv.path_stats_size == ex.path_stats_size == n * n + n
        sa = torch.zeros(mv.path_stats_size, dtype=torch.float64, device='cuda:0')
        sb = torch.zeros_like(sa)
        pa = mv.sample_paths_dev(A, pi, mu, cov, sa.data_ptr(), seed=5, want_paths=True)
        pb = ex.sample_paths_dev(A, pi, None, None, sb.data_ptr(), seed=5, want_paths=True)
        mv.sync(), ex.sync()
        for k in range(len(obs)):
            assert np.array_equal(pa[k], pb[k]) and np.array_equal(pa[k], a[0][k])
        assert np.array_equal(sa.cpu().numpy(), sb.cpu().numpy())
        C, n0, emis = mv.unpack_path_stats(sa.cpu().numpy())
        assert np.array_equal(C, a[1]) and np.array_equal(n0, a[2]) and emis is None
        # increments into a device tensor: m_t is added there
        tr = torch.empty((total, n), dtype=torch.float64, device='cuda:0')
        tl = torch.empty(total, dtype=torch.float64, device='cuda:0')
        fr, fl = mv.filter_states(A, pi, mu, cov, out=tr, out_increments=tl)
        er, el = ex.filter_states(A, pi)
        assert np.array_equal(tr.cpu().numpy(), np.concatenate(er, axis=0))
        # (one addition per step: half an ulp of the sum)
        got, want = tl.cpu().numpy(), np.concatenate(el) + m
        assert np.all(np.abs(got - want) <= EPS * np.abs(want))
        assert fl[1].data_ptr() == tl.data_ptr() + 8 * int(off[1])
        hr, hl = mv.filter_states(A, pi, mu, cov)
        assert np.array_equal(np.concatenate(hl), got)
    finally:
        ex.close()
        mv.close()


def test_functional_wrappers_accept_the_model():
    import bhmm_amd
    n = 3
    A, pi, mu, cov, obs, paths = _problem(n, 2, 43)
    obs, paths = obs[:3], paths[:3]
    model = bhmm_amd.mvgaussian_hmm(pi, A, mu, cov)
    rows, ms, shifts = _np_scaled(obs, mu, cov, 'full')
    ref = _oracle_estep(rows, A, pi)
    np.testing.assert_allclose(bhmm_amd.score(obs, model, per_trajectory=True)[0], ref['logL'] + shifts, rtol=1e-11)
    for a, b in zip(bhmm_amd.posterior_marginals(obs, model), ref['gammas']):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)
    dec = bhmm_amd.posterior_decode(obs, model)
    for a, b in zip(dec, ref['gammas']):
        assert np.array_equal(a, b.argmax(axis=1))
    jumps = bhmm_amd.posterior_transitions(obs, model)
    assert [len(j) for j in jumps] == [len(o) - 1 for o in obs]
    fr, fl = bhmm_amd.filter_states(obs, model)
    assert abs(sum(float(l.sum()) for l in fl) - (ref['logL'] + shifts).sum()) <= 1e-10 * abs(shifts.sum())
    segs = bhmm_amd.decode_segments(obs, model)
    assert segs.count >= 3
    lp = bhmm_amd.path_logprob(obs, model, paths=[p.astype(np.int32) for p in paths])
    assert lp.shape == (1, 3) and np.all(np.isfinite(lp)) and np.all(lp[0] <= ref['logL'] + shifts)


# ---- 5. one EM step ------------------------------------------------------------------------------------------
def _numpy_mstep(obs, gammas, ctype):
    n = gammas[0].shape[1]
    x = np.concatenate(obs, axis=0)
    g = np.concatenate(gammas, axis=0)
    D = x.shape[1]
    mu, cov = np.empty((n, D)), np.empty((n, D, D))
    for i in range(n):
        w = g[:, i]
        mu[i] = (w[:, None] * x).sum(axis=0) / w.sum()
        d = x - mu[i]
        cov[i] = (w[:, None, None] * d[:, :, None] * d[:, None, :]).sum(axis=0) / w.sum()
    return mu, (cov if ctype == 'full' else np.array([np.diag(c) for c in cov]))


@pytest.mark.parametrize("n,ctype", [(3, 'full'), (3, 'diag'), (9, 'full')])
def test_em_step_equals_the_numpy_mstep_on_the_oracles_statistics(n, ctype):
    import bhmm_amd
    A, pi, mu, cov, obs, _ = _problem(n, 2, 60 + n, ctype=ctype)
    # a model some way off the generating one
    rng = np.random.default_rng(1)
    mu0 = mu + rng.normal(size=mu.shape) * 0.3
    cov0 = cov * 1.3
    model = bhmm_amd.mvgaussian_hmm(pi, A, mu0, cov0, covariance_type=ctype)
    rows, _, shifts = _np_scaled(obs, mu0, cov0, ctype)
    ref = _oracle_estep(rows, A, pi)
    mu1, cov1 = _numpy_mstep(obs, ref['gammas'], ctype)
    T1 = ref['C'] / ref['C'].sum(axis=1)[:, None]
    pi1 = ref['gamma0_sum'] / ref['gamma0_sum'].sum()
    est = bhmm_amd.MaximumLikelihoodEstimator(obs, n, initial_model=model, reversible=False)
    ll = est.em_step()
    assert abs(ll - (ref['logL'] + shifts).sum()) <= 1e-11 * abs((ref['logL'] + shifts).sum())
    om = est.hmm.output_model
    np.testing.assert_allclose(om.means, mu1, rtol=1e-9)
    if ctype == 'diag':
        np.testing.assert_allclose(om.covariances, cov1, rtol=1e-9)
    else:
        # variances: relative.  An off-diagonal entry is a difference around zero (a correlation times two standard
        # deviations): it is held on the scale of those, sqrt(S_aa S_bb)
        sd = np.sqrt(np.einsum('iaa->ia', cov1))
        assert np.all(np.abs(om.covariances - cov1) <= 1e-9 * sd[:, :, None] * sd[:, None, :])
        np.testing.assert_allclose(np.einsum('iaa->ia', om.covariances), np.einsum('iaa->ia', cov1), rtol=1e-9)
    np.testing.assert_allclose(est.hmm.transition_matrix, T1, rtol=1e-9)
    np.testing.assert_allclose(est.hmm.initial_distribution, pi1, rtol=1e-9)


def _synthetic(seed=0):
    rng = np.random.default_rng(seed)
    mu = np.array([[-4.0, 0.0], [0.0, 5.0], [5.0, -1.0]])
    cov = np.array([[[1.0, 0.3], [0.3, 0.5]], [[0.6, -0.2], [-0.2, 1.2]], [[1.5, 0.0], [0.0, 0.4]]])
    P = np.array([[0.95, 0.03, 0.02], [0.04, 0.94, 0.02], [0.03, 0.03, 0.94]])
    fac = np.array([np.linalg.cholesky(c) for c in cov])
    obs, paths = [], []
    for T in (3000, 2000):
        s = np.zeros(T, dtype=np.int64)
        u = rng.random(T)
        for t in range(1, T):
            s[t] = min(2, np.searchsorted(np.cumsum(P[s[t - 1]]), u[t]))
        obs.append(mu[s] + np.einsum('tab,tb->ta', fac[s], rng.normal(size=(T, 2))))
        paths.append(s)
    return mu, cov, P, obs, paths


def test_ten_em_steps_never_lower_the_likelihood():
    import bhmm_amd
    mu, cov, P, obs, _ = _synthetic()
    model = bhmm_amd.mvgaussian_hmm(np.ones(3) / 3, np.full((3, 3), 0.1) + 0.7 * np.eye(3), mu + 1.0,
                                    np.array([np.eye(2) * 2.0] * 3))
    est = bhmm_amd.MaximumLikelihoodEstimator(obs, 3, initial_model=model)
    ll = [est.em_step() for _ in range(10)]
    print("log-likelihoods:", ll)
    for a, b in zip(ll[:-1], ll[1:]):
        assert b - a >= -1e-9 * abs(a)
    assert ll[-1] > ll[0]


def test_estimate_hmm_recovers_the_generating_means():
    import bhmm_amd
    mu, cov, P, obs, paths = _synthetic()
    hmm = bhmm_amd.estimate_hmm(obs, 3)
    assert hmm.output_model.model_type == 'mvgaussian'
    counts = np.bincount(np.concatenate(paths), minlength=3)
    se = np.sqrt(np.array([np.diag(c) for c in cov]) / counts[:, None])
    dev = np.abs(hmm.output_model.means - mu) / se
    print("deviation of the means in standard errors:", dev)
    assert np.all(dev <= 3.0)
    assert len(hmm.hidden_state_trajectories) == 2


# ---- 6. errors ------------------------------------------------------------------------------------------------
def test_errors():
    import bhmm_amd
    from bhmm_amd.engine import MvnEngine
    n, D = 2, 2
    A, pi = np.full((n, n), 0.5), np.ones(n) / n
    mu, cov = np.zeros((n, D)), np.array([np.eye(D)] * n)
    obs = [np.random.default_rng(0).normal(size=(50, D))]
    eng = _engine(obs, n)
    try:
        bad = cov.copy()
        bad[1] = [[1.0, 2.0], [2.0, 1.0]]
        with pytest.raises(RuntimeError):                                   # not positive definite
            eng.score([(A, pi, mu, bad)])
        with pytest.raises(ValueError):                                     # no emissions made: nothing is loaded
            eng.viterbi(A, pi, mu, cov[:, :1])
        assert np.all(np.isfinite(eng.score([(A, pi, mu, cov)])))           # (the engine is still usable)
        with pytest.raises(ValueError):
            eng.set_observations('mvgaussian', [np.zeros((5, 65))], n)      # D = 65
        with pytest.raises(ValueError):
            eng.set_observations('mvgaussian', [np.zeros(5)], n)
        with pytest.raises(ValueError):
            eng.set_observations('gaussian', [np.zeros(5)], n)
    finally:
        eng.close()
    with pytest.raises(ValueError):
        bhmm_amd.MultivariateGaussianOutputModel(n, np.zeros((n, 65)), np.ones((n, 65)), covariance_type='diag')
    model = bhmm_amd.mvgaussian_hmm(pi, A, mu, cov)
    with pytest.raises(NotImplementedError):
        bhmm_amd.MaximumLikelihoodEstimator(obs, n, initial_model=model, process_group=object())
    with pytest.raises(NotImplementedError):
        bhmm_amd.MaximumLikelihoodEstimator(obs, n, initial_model=model, estep_precision='float32')
    with pytest.raises(NotImplementedError):
        bhmm_amd.bayesian_hmm(obs, model)
    om = bhmm_amd.MultivariateGaussianOutputModel(n, mu, bad)
    with pytest.raises(RuntimeError):
        om.log_p_obs(obs[0])
    p = bhmm_amd.MultivariateGaussianOutputModel(n, mu, cov).p_obs(obs[0])
    assert p.shape == (50, n) and np.all(p > 0)
