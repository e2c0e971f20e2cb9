"""GPU: Poisson count emissions -- k_pois_rows (bhmm_pois_emissions, bhmm_logpdf_poisson), PoissonEngine,
MaximumLikelihoodEstimator(output='poisson') and the functional wrappers.

The yardsticks are written here in numpy and do not use the code under test:
  rows     l_ti = sum_d x_td log lambda_id - sum_d lambda_id in np.longdouble, log x! from a cumulative long-double table
           of log k.  Bound on l_ti: 4 (D + 4) eps sum_d (x_td |log lambda_id| + lambda_id) -- D fused multiply-adds and
           the subtraction of Lambda_i, each half an ulp of a partial sum that the sum of magnitudes bounds, the rounding
           of log lambda and of Lambda_i; 4 is the margin (a float64 numpy restatement stays below 0.06 of it).  Bound on
           the step constant: 64 eps (1 + sum_d lgamma(x_td + 1)) -- a device lgamma may carry a few ulp per term.
           A row is exp(l_ti - m_t) with m_t = l_tj of the largest state and is held to rtol (bound_ti + bound_tj +
           4 eps): the bounds of both log-densities, and the exp.
  moments  math.fsum over numpy terms, bound 1e-12 (1 + sum |term|) per entry, as in test_mvn_gpu.py.
  the rest the oracle's forward / backward on float64 numpy-made scaled rows, and an explicit-kind Engine fed those
           rows.
"""
import itertools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])
TRUE_RATES = np.array([[0.3, 1.0], [5.0, 2.0], [20.0, 30.0]])


# ---- the yardsticks --------------------------------------------------------------------------------------
def _ld_ref(x, rates):
    """(l (T, N), c (T,)) in long double, and the two bounds (T, N), (T,)"""
    x = np.asarray(x, dtype=np.float64)
    T, D = x.shape
    N = rates.shape[0]
    xl, rl = x.astype(LD), rates.astype(LD)
    with np.errstate(divide='ignore'):
        ll = np.log(rl)
    l = np.zeros((T, N), dtype=LD)
    mag = np.zeros((T, N))
    for d in range(D):
        with np.errstate(invalid='ignore'):
            l += np.where(xl[:, d, None] == 0, LD(0), xl[:, d, None] * ll[None, :, d])
            mag += np.where(x[:, d, None] == 0, 0.0, x[:, d, None] * np.abs(np.log(np.maximum(rates[None, :, d], 1e-300))))
    l -= rl.sum(axis=1)[None, :]
    mag += rates.sum(axis=1)[None, :]
    kmax = int(np.nanmax(x)) if T else 0
    table = np.concatenate([[LD(0)], np.cumsum(np.log(np.arange(1, kmax + 1, dtype=LD)))]) if kmax else np.zeros(1, dtype=LD)
    lf = table[np.nan_to_num(x).astype(np.int64)]
    c = -lf.sum(axis=1)
    bound_l = 4.0 * (D + 4) * EPS * mag
    bound_c = 64.0 * EPS * (1.0 + _lgamma(np.nan_to_num(x) + 1.0).sum(axis=1))
    return l, c, bound_l, bound_c


def _np_rows(x, rates):
    """float64 restatement: (l, c, m, rows) with m = 0 and a zero row where every l is -inf"""
    x = np.asarray(x, dtype=np.float64)
    T, D = x.shape
    N = rates.shape[0]
    with np.errstate(divide='ignore'):
        ll = np.log(rates)
    l = np.zeros((T, N))
    lam = np.zeros(N)
    for d in range(D):
        with np.errstate(invalid='ignore'):
            l += np.where(x[:, d, None] == 0, 0.0, x[:, d, None] * ll[None, :, d])
        lam += rates[:, d]
    l -= lam[None, :]
    c = -_lgamma(x + 1.0).sum(axis=1) if T else np.zeros(0)
    m = l.max(axis=1) if T else np.zeros(0)
    m = np.where(np.isneginf(m), 0.0, m)
    with np.errstate(invalid='ignore'):
        rows = np.exp(l - m[:, None])
    return l, c, m, rows


def _np_scaled(obs, rates):
    """per trajectory the numpy-made rows and step scales m_t + c_t, and the shifts"""
    rows, scales = [], []
    for o in obs:
        _, c, m, r = _np_rows(o, rates)
        rows.append(r)
        scales.append(m + c)
    return rows, scales, np.array([math.fsum(s.tolist()) for s in scales])


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
def _split(x, lengths):
    off = np.concatenate([[0], np.cumsum(lengths)])
    return [x[off[k]:off[k + 1]] for k in range(len(lengths))]


def _lengths(total):
    """several ragged trajectories, one of them empty"""
    if total == 1:
        return [0, 1]
    a = total // 3
    return [a, 0, 1, total - a - 1]


def _rows_case(N, D, total, rng):
    """rates log-uniform in [1e-3, 1e4]; every step drawn from the rates of some state"""
    rates = np.exp(rng.uniform(math.log(1e-3), math.log(1e4), (N, D)))
    x = rng.poisson(rates[rng.integers(0, N, total)])
    return _split(x, _lengths(total)), rates


def _engine(obs, n):
    from bhmm_amd.engine import PoissonEngine
    eng = PoissonEngine(0)
    eng.set_observations('poisson', obs, n)
    return eng


def _check_rows(eng, obs, rates, label):
    from bhmm_amd import _lib
    N = rates.shape[0]
    x = np.concatenate(obs, axis=0)
    l, c, bl, bc = _ld_ref(x, rates)
    m = l.max(axis=1)
    jmax = l.argmax(axis=1)
    eng.set_observations('poisson', obs, N)
    eng.emissions(rates)
    rows, scale, shift = eng.emission_rows(), eng.step_scales(), eng.shifts
    assert rows.shape == l.shape and np.all(np.isfinite(rows)) and np.all(rows.max(axis=1) == 1.0)
    want = np.exp((l - m[:, None]).astype(np.float64))
    # a row entry is exp(l_ti - l_tj), j the largest state: BOTH l carry their bound (held to the bound of l_ti alone,
    # a float64 numpy restatement misses by a factor 1.8 where lambda_j is large and lambda_i is not)
    rtol = bl + bl[np.arange(len(x)), jmax][:, None] + 4.0 * EPS
    big = want >= 1e-290
    err = np.abs(rows - want)
    worst_row = float((err[big] / (rtol[big] * want[big])).max())
    assert np.all(err[big] <= rtol[big] * want[big]), (label, worst_row)
    assert np.all(rows[~big] < 2e-290)
    # the step scale m_t + c_t: the l of the largest state and the constant, each within its bound
    bm = bl[np.arange(len(x)), jmax]
    serr = np.abs(scale.astype(LD) - (m + c)).astype(np.float64)
    worst_scale = float((serr / (bm + bc)).max())
    assert np.all(serr <= bm + bc), (label, worst_scale)
    # l_ti + c_t itself, from the same kernel (bhmm_logpdf_poisson)
    logp = np.empty((len(x), N))
    _lib.check(_lib.load().bhmm_logpdf_poisson(_lib.dp(logp), _lib.dp(_lib.f64(x)), len(x), x.shape[1], N,
                                               _lib.dp(_lib.f64(rates))))
    lerr = np.abs(logp.astype(LD) - (l + c[:, None])).astype(np.float64)
    worst_l = float((lerr / (bl + bc[:, None])).max())
    assert np.all(lerr <= bl + bc[:, None]), (label, worst_l)
    # shifts: the sum of the scales the device made, in any order
    off = eng.offsets
    for k in range(len(obs)):
        s = scale[off[k]:off[k + 1]]
        assert abs(shift[k] - math.fsum(s.tolist())) <= 4.0 * EPS * max(len(s), 1) * np.abs(s).sum()
    print("%s: largest error / bound: rows %.3g, scale %.3g, log-density %.3g" % (label, worst_row, worst_scale, worst_l))


# ---- 1. rows against long double ---------------------------------------------------------------------------
SHAPES = [(N, 3) for N in (1, 3, 8, 16, 17, 33)] + [(17, D) for D in (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 64)]


@pytest.mark.parametrize("N,D", SHAPES)
def test_rows(N, D):
    """every N at D = 3 (below, at and above ROWS_NB, more than two blocks of states), every D at N = 17 (both edges
    of every dimension class); each at 1, 255, 256, 257 and 700 steps"""
    rng = np.random.default_rng(1000 * N + D)
    eng = None
    try:
        for total in (1, 255, 256, 257, 700):
            obs, rates = _rows_case(N, D, total, rng)
            if eng is None:
                eng = _engine(obs, N)
            _check_rows(eng, obs, rates, "N=%d D=%d T=%d" % (N, D, total))
    finally:
        if eng is not None:
            eng.close()


def test_rows_most_states_widest_class():
    rng = np.random.default_rng(3364)
    obs, rates = _rows_case(33, 64, 257, rng)
    eng = _engine(obs, 33)
    try:
        _check_rows(eng, obs, rates, "N=33 D=64 T=257")
    finally:
        eng.close()


# ---- 2. the special rules ------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def test_zero_rate_with_zero_count_is_the_model_without_that_channel():
    rng = np.random.default_rng(2)
    N, D = 5, 4
    rates = rng.uniform(0.5, 8.0, (N, D))
    rates[:, 2] = [0.0, 3.0, 0.0, 0.0, 1e-3]            # a dead channel in three states
    x = rng.poisson(rates[rng.integers(0, N, 600)])
    x[:, 2] = 0
    keep = [0, 1, 3]
    full, less = _engine([x], N), _engine([x[:, keep]], N)
    try:
        full.emissions(rates)
        r_full = full.emission_rows()
        # the channel removed: the states that had rate 0 there give bitwise the same l; the others lose their term
        # exp(-rate), so compare state by state through the log-densities of the three-channel model
        dead = [0, 2, 3]
        less.emissions(rates[:, keep])
        from bhmm_amd.output_models.poisson import PoissonOutputModel
        from bhmm_amd import _lib
        a, b = np.empty((600, N)), np.empty((600, N))
        L = _lib.load()
        _lib.check(L.bhmm_logpdf_poisson(_lib.dp(a), _lib.dp(_lib.f64(x)), 600, D, N, _lib.dp(_lib.f64(rates))))
        _lib.check(L.bhmm_logpdf_poisson(_lib.dp(b), _lib.dp(_lib.f64(x[:, keep])), 600, 3, N,
                                         _lib.dp(_lib.f64(rates[:, keep]))))
        assert np.all(np.isfinite(a))
        assert np.array_equal(_bits(a[:, dead]), _bits(b[:, dead]))      # the term is exactly 0
        # a model whose EVERY state is dead in the channel: the whole row is bitwise that of the smaller model
        r2 = rates.copy()
        r2[:, 2] = 0.0
        full.emissions(r2)
        assert np.array_equal(_bits(full.emission_rows()), _bits(less.emission_rows()))
        assert np.array_equal(_bits(full.step_scales()), _bits(less.step_scales()))
        assert np.array_equal(_bits(full.shifts), _bits(less.shifts))
        assert not np.array_equal(r_full, full.emission_rows())
        assert np.all(np.isfinite(PoissonOutputModel(N, r2).log_p_obs(x)))
    finally:
        full.close()
        less.close()


def test_zero_rate_with_a_positive_count_removes_that_state_only():
    rng = np.random.default_rng(3)
    N, D = 4, 3
    rates = rng.uniform(0.5, 8.0, (N, D))
    x = rng.poisson(rates[rng.integers(0, N, 300)]) + 1      # every count positive
    dead = rates.copy()
    dead[1, 0] = 0.0
    eng = _engine([x], N)
    others = [0, 2, 3]
    try:
        eng.emissions(dead)
        got, sg = eng.emission_rows(), eng.step_scales()
        assert np.all(got[:, 1] == 0.0) and np.all(got[:, others].max(axis=1) == 1.0)
        # the same model without state 1 (its rate matters to nothing else)
        sub = _engine([x], 3)
        try:
            sub.emissions(rates[others])
            assert np.array_equal(_bits(got[:, others]), _bits(sub.emission_rows()))
            assert np.array_equal(_bits(sg), _bits(sub.step_scales()))
        finally:
            sub.close()
    finally:
        eng.close()


def test_impossible_step_and_nan_count_spoil_their_own_trajectory_only():
    rng = np.random.default_rng(4)
    N, D = 3, 2
    rates = rng.uniform(0.5, 8.0, (N, D))
    rates[:, 1] = 0.0                                        # channel 1 is dark in every state
    A = np.full((N, N), 0.1) + 0.7 * np.eye(N)
    pi = np.ones(N) / N
    obs = [rng.poisson(rates[rng.integers(0, N, T)]) for T in (300, 1, 411)]
    eng = _engine(obs, N)
    try:
        clean = eng.score([(A, pi, rates, None)])[0]
        assert np.all(np.isfinite(clean))
        bad = [o.copy() for o in obs]
        bad[2][100, 1] = 2                                   # impossible under every state
        eng.set_observations('poisson', bad, N)
        eng.emissions(rates)
        rows, scale, shift = eng.emission_rows(), eng.step_scales(), eng.shifts
        t = 300 + 1 + 100
        c_t = -math.lgamma(bad[2][100, 0] + 1.0) - math.lgamma(3.0)
        assert np.all(rows[t] == 0.0) and abs(scale[t] - c_t) <= 64 * EPS * (1.0 - c_t)      # m_t = 0: the scale is c_t
        assert np.all(np.delete(rows, t, axis=0).max(axis=1) == 1.0) and np.all(np.isfinite(shift))
        got = eng.score([(A, pi, rates, None)])[0]
        assert np.array_equal(got[:2], clean[:2]) and got[2] == -np.inf
        nan = [o.astype(np.float64) for o in obs]
        nan[2][100, 0] = np.nan
        eng.set_observations('poisson', nan, N)
        eng.emissions(rates)
        rows, scale, shift = eng.emission_rows(), eng.step_scales(), eng.shifts
        assert np.all(np.isnan(rows[t])) and np.isnan(scale[t]) and np.isnan(shift[2])
        assert np.all(np.isfinite(np.delete(rows, t, axis=0))) and np.all(np.isfinite(np.delete(scale, t)))
        got = eng.score([(A, pi, rates, None)])[0]
        assert np.array_equal(got[:2], clean[:2]) and np.isnan(got[2])
    finally:
        eng.close()


def test_bad_counts_in_a_device_buffer_are_refused():
    """A count of -1 or 0.5 on the device: ValueError (BHMM_ERR_INVALID) from the call that makes the rows, nothing is
    loaded.  The counts belong to the observation set, so no earlier emissions on the SAME set can have succeeded;
    what stays usable is checked both ways there are: the engine takes the good buffer again and makes bitwise the
    rows it made before, and a refused RATE leaves the loaded rows of the good set in use."""
    import torch
    from bhmm_amd import _lib
    rng = np.random.default_rng(5)
    N, D = 3, 2
    A = np.full((N, N), 0.1) + 0.7 * np.eye(N)
    pi = np.ones(N) / N
    x = rng.poisson(TRUE_RATES[rng.integers(0, N, 600)]).astype(np.float64)
    off = np.array([0, 200, 600], dtype=np.int64)
    good = torch.from_numpy(x).to('cuda:0')
    from bhmm_amd.engine import PoissonEngine
    eng = PoissonEngine(0)
    try:
        eng.set_observations_device('poisson', good.data_ptr(), off, N, dimension=D)
        ll = eng.score([(A, pi, TRUE_RATES, None)])
        rows = eng.emission_rows()
        host = _engine(_split(x, [200, 400]), N)
        try:
            assert np.array_equal(_bits(host.score([(A, pi, TRUE_RATES, None)])), _bits(ll))
        finally:
            host.close()
        for rate in (-1.0, np.nan, np.inf):                  # a refused rate: the loaded rows stay in use
            r = TRUE_RATES.copy()
            r[1, 1] = rate
            with pytest.raises(ValueError):
                eng.score([(A, pi, r, None)])
            assert _lib.load().bhmm_pois_emissions(eng._h, _lib.dp(r)) == _lib.ERR_INVALID
            assert np.array_equal(_bits(eng.emission_rows()), _bits(rows))
            assert [len(p) for p in eng.viterbi(A, pi, TRUE_RATES)] == [200, 400]
            assert np.array_equal(_bits(eng.score([(A, pi, TRUE_RATES, None)])), _bits(ll))
        for value in (-1.0, 0.5):
            y = x.copy()
            y[399, 1] = value
            bad = torch.from_numpy(y).to('cuda:0')
            eng.set_observations_device('poisson', bad.data_ptr(), off, N, dimension=D)
            with pytest.raises(ValueError):
                eng.score([(A, pi, TRUE_RATES, None)])
            with pytest.raises(ValueError):                  # nothing was loaded: no model call works
                eng.viterbi(A, pi, TRUE_RATES)
            eng.set_observations_device('poisson', good.data_ptr(), off, N, dimension=D)
            assert np.array_equal(_bits(eng.score([(A, pi, TRUE_RATES, None)])), _bits(ll))
            assert np.array_equal(_bits(eng.emission_rows()), _bits(rows))
        with pytest.raises(ValueError):                      # host arrays are checked before they are uploaded
            eng.set_observations('poisson', [np.array([[1.0, 0.5]])], N)
        with pytest.raises(ValueError):
            eng.set_observations('poisson', [np.array([[1, -1]])], N)
    finally:
        eng.close()


def test_all_zero_counts_and_a_count_of_a_million():
    N, D = 3, 2
    eng = _engine([np.zeros((300, D), int)], N)
    try:
        eng.emissions(TRUE_RATES)
        rows, scale = eng.emission_rows(), eng.step_scales()
        lam = TRUE_RATES[:, 0] + TRUE_RATES[:, 1]
        want = np.exp(-(lam - lam.min()))
        np.testing.assert_allclose(rows, np.tile(want, (300, 1)), rtol=4 * EPS)
        assert np.all(rows[:, 0] == 1.0) and np.all(scale == -lam.min())      # c_t = 0 exactly
        big = np.array([[1e6, 1e6 - 1], [1e6 + 3, 1e6]])
        rates = np.array([[1e6, 1e6], [1e6 * (1 + 1e-3), 1e6], [1.0, 1.0]])
        eng.set_observations('poisson', [big], N)
        _check_rows(eng, [big], rates, "counts of 1e6")
        got = eng.step_scales()
        # Stirling: log Poisson(k; k) = -log(2 pi k) / 2 - 1 / (12 k) + ..., twice
        assert abs(got[1] - 2 * (-0.5 * math.log(2 * math.pi * 1e6))) < 1e-2
    finally:
        eng.close()


# ---- 3. bhmm_logpdf_poisson -------------------------------------------------------------------------------------
def test_logpdf_poisson():
    from bhmm_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(6)
    N, D, T = 17, 5, 300
    rates = np.exp(rng.uniform(math.log(1e-3), math.log(1e4), (N, D)))
    rates[3, 1] = 0.0
    x = rng.poisson(rates[rng.integers(0, N, T)]).astype(np.float64)
    out = np.empty((T, N))
    _lib.check(L.bhmm_logpdf_poisson(_lib.dp(out), _lib.dp(x), T, D, N, _lib.dp(rates)))
    l, c, bl, bc = _ld_ref(x, rates)
    want = l + c[:, None]
    inf = np.isneginf(want.astype(np.float64))
    assert inf.any() and np.array_equal(np.isneginf(out), inf)
    err = np.abs(out[~inf].astype(LD) - want[~inf]).astype(np.float64)
    assert np.all(err <= (bl + bc[:, None])[~inf])
    assert L.bhmm_logpdf_poisson(_lib.dp(out), _lib.dp(np.zeros((4, 65))), 4, 65, 1, _lib.dp(np.ones(65))) == _lib.ERR_INVALID
    bad = rates.copy()
    bad[0, 0] = -1e-3
    assert L.bhmm_logpdf_poisson(_lib.dp(out), _lib.dp(x), T, D, N, _lib.dp(bad)) == _lib.ERR_INVALID
    y = x.copy()
    y[7, 2] = 1.5
    assert L.bhmm_logpdf_poisson(_lib.dp(out), _lib.dp(y), T, D, N, _lib.dp(rates)) == _lib.ERR_INVALID
    y[7, 2] = -2.0
    assert L.bhmm_logpdf_poisson(_lib.dp(out), _lib.dp(y), T, D, N, _lib.dp(rates)) == _lib.ERR_INVALID


# ---- 4. repeatability ----------------------------------------------------------------------------------------------
def test_repeatable_and_cached():
    import torch
    rng = np.random.default_rng(7)
    N, D = 17, 3
    lengths = [300, 0, 1, 411]
    rates = rng.uniform(0.2, 9.0, (N, D))
    x = rng.poisson(rates[rng.integers(0, N, sum(lengths))])
    assert x.dtype == np.int64
    g = rng.random((sum(lengths), N)) ** 3
    g /= g.sum(axis=1)[:, None]
    gd = torch.from_numpy(g).to('cuda:0')
    a, b = _engine(_split(x, lengths), N), _engine(_split(x.astype(np.float64), lengths), N)
    try:
        res = []
        for eng in (a, a, b):
            eng.emissions(rates, force=True)
            res.append((eng.emission_rows(), eng.step_scales(), eng.shifts.copy(), eng.moments(gd, rates, 'diag')))
        for other in res[1:]:
            for u, v in zip(res[0], other):
                assert np.array_equal(_bits(u), _bits(v))
        # unchanged rates: the rows are not made again -- the engine keeps what it fetched after the one pass
        kept = a._shift
        assert a.emissions(rates.copy()) == 'diag' and a._shift is kept
        a.emissions(rates + 0.5)
        assert a._shift is not kept and not np.array_equal(a._shift, kept)
        a.emissions(rates)
        assert np.array_equal(_bits(a._shift), _bits(kept))
    finally:
        a.close()
        b.close()


# ---- 5. the E-step ---------------------------------------------------------------------------------------------------
def _problem(n, D, seed, T=(300, 133, 1, 420)):
    """an n-state model with moderate rates (dark and bright channels) and trajectories drawn from it"""
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) * 0.2 + np.eye(n) * 3.0
    A /= A.sum(axis=1)[:, None]
    pi = rng.random(n) + 0.5
    pi /= pi.sum()
    rates = np.exp(rng.uniform(math.log(0.2), math.log(12.0), (n, D)))
    obs, paths = [], []
    for Tk in T:
        s = np.zeros(Tk, dtype=np.int64)
        u = rng.random(Tk)
        for t in range(Tk):
            p = pi if t == 0 else A[s[t - 1]]
            s[t] = min(n - 1, np.searchsorted(np.cumsum(p), u[t]))
        obs.append(rng.poisson(rates[s]) if Tk else np.zeros((0, D), int))
        paths.append(s)
    return A, pi, rates, obs, paths


@pytest.mark.parametrize("n,D", [(3, 2), (8, 2), (17, 2), (3, 8), (8, 8), (17, 8)])
def test_estep_against_the_oracle(n, D):
    A, pi, rates, obs, _ = _problem(n, D, 11 * n + D)
    rows, _, shifts = _np_scaled(obs, rates)
    ref = _oracle_estep(rows, A, pi)
    want = ref['logL'] + shifts
    eng = _engine(obs, n)
    try:
        res = eng.estep(A, pi, rates, None)
        packed = eng.estep_fetch_packed()
        sc = eng.score([(A, pi, rates, None), (A, pi, rates * 1.01, None)])
    finally:
        eng.close()
    print("logL", res.logL_k.tolist(), "error", np.abs(res.logL_k - want).tolist())
    assert np.all(np.abs(res.logL_k - want) <= 1e-11 * (1.0 + np.abs(want)))
    assert np.all(np.abs(sc[0] - want) <= 1e-11 * (1.0 + np.abs(want)))
    assert abs(res.loglik - want.sum()) <= 1e-11 * (1.0 + abs(want.sum()))
    assert np.all(sc[1] != sc[0])                                       # (the second model made its own rows)
    np.testing.assert_allclose(res.C, ref['C'], rtol=1e-9)
    np.testing.assert_allclose(res.gamma0_sum, ref['gamma0_sum'], rtol=1e-9)
    np.testing.assert_allclose(res.state_counts, ref['state_counts'], rtol=1e-9)
    np.testing.assert_allclose(res.S0, ref['state_counts'], rtol=1e-9)
    # S1 = sum gamma (x - lambda): a difference around zero, held on the scale of sum gamma |x - lambda|
    x = np.concatenate(obs, axis=0).astype(np.float64)
    g = np.concatenate(ref['gammas'], axis=0)
    for i in range(n):
        d = x - rates[i]
        assert np.all(np.abs(res.S1[i] - g[:, i].dot(d)) <= 1e-9 * g[:, i].dot(np.abs(d)))
    assert res.kind == 'poisson' and res.S2.shape == (n, D)
    assert packed.shape == (1 + n + n * n + n + res.moments.size,) and packed[0] == res.loglik
    assert np.array_equal(packed[-res.moments.size:], res.moments)


@pytest.mark.parametrize("n,D", [(3, 2), (17, 8)])
def test_moments_against_fsum(n, D):
    import torch
    from bhmm_amd.output_models.mvgaussian import unpack_moments
    rng = np.random.default_rng(100 * D + n)
    lengths = [300, 0, 1, 411]
    rates = rng.uniform(0.2, 9.0, (n, D))
    x = rng.poisson(rates[rng.integers(0, n, sum(lengths))])
    g = rng.random((sum(lengths), n)) ** 3
    g /= g.sum(axis=1)[:, None]
    eng = _engine(_split(x, lengths), n)
    try:
        got = eng.moments(torch.from_numpy(g).to('cuda:0'), rates, 'diag')
    finally:
        eng.close()
    S0, S1, _ = unpack_moments(got, n, D, 'diag')
    for i in range(n):
        d = x - rates[i]
        for val, t in [(S0[i], g[:, i])] + [(S1[i, p], g[:, i] * d[:, p]) for p in range(D)]:
            assert abs(val - math.fsum(t.tolist())) <= 1e-12 * (1.0 + np.abs(t).sum())


# ---- 6. every call -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 17])
def test_functional_wrappers_equal_the_explicit_engine_on_numpy_rows(n):
    """The rows and scales of the kernel are within 4 (D + 4) eps sum (x |log lambda| + lambda) ~ 1e-12 of the numpy
    ones on this problem (D = 2, counts of a few dozen at most); a posterior or filtered probability feels the rows of
    a mixing time, a few dozen steps: 1e-9 absolute, the bound of the explicit calls' own tests.  A log-likelihood or
    path log-probability adds T such terms: 1e-11 of its size."""
    import bhmm_amd
    from bhmm_amd.engine import Engine
    A, pi, rates, obs, paths = _problem(n, 2, 40 + n)
    model = bhmm_amd.poisson_hmm(pi, A, rates)
    others = [bhmm_amd.poisson_hmm(pi, A, rates * f) for f in (1.1, 0.8)]
    rows, scales, shifts = _np_scaled(obs, rates)
    W = np.random.default_rng(0).random((n, 2))
    ex = Engine(0)
    try:
        ex.set_observations('explicit', rows, n)
        # score: a stack of three models
        sc = bhmm_amd.score(obs, [model] + others, per_trajectory=True)
        assert sc.shape == (3, len(obs))
        want = ex.score([(A, pi, None, None)])[0] + shifts
        assert np.all(np.abs(sc[0] - want) <= 1e-11 * (1.0 + np.abs(want)))
        for s, f in ((1, 1.1), (2, 0.8)):
            r2, _, sh2 = _np_scaled(obs, rates * f)
            e2 = Engine(0)
            try:
                e2.set_observations('explicit', r2, n)
                w2 = e2.score([(A, pi, None, None)])[0] + sh2
            finally:
                e2.close()
            assert np.all(np.abs(sc[s] - w2) <= 1e-11 * (1.0 + np.abs(w2)))
        assert np.allclose(bhmm_amd.score(obs, model), want.sum(), rtol=1e-11)
        for a, b in zip(bhmm_amd.posterior_decode(obs, model), ex.posterior_decode(A, pi)):
            assert np.array_equal(a, b)
        for a, b in zip(bhmm_amd.posterior_marginals(obs, model), ex.posterior_marginals(A, pi)):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)
        for a, b in zip(bhmm_amd.posterior_marginals(obs, model, weights=W), ex.posterior_marginals(A, pi, weights=W)):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)
        for a, b in zip(bhmm_amd.posterior_transitions(obs, model), ex.posterior_transitions(A, pi)):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)
        fr, fl = bhmm_amd.filter_states(obs, model)
        er, el = ex.filter_states(A, pi)
        for k in range(len(obs)):
            np.testing.assert_allclose(fr[k], er[k], rtol=0, atol=1e-9)
            np.testing.assert_allclose(fl[k], el[k] + scales[k], rtol=0, atol=1e-9)
            assert abs(math.fsum(fl[k].tolist()) - want[k]) <= 1e-9          # the increments sum to the log-likelihood
        for method in ('viterbi', 'posterior'):
            r1, r2 = bhmm_amd.decode_segments(obs, model, method=method), ex.decode_runs(A, pi, method=method)
            assert np.array_equal(r1.offsets, r2.offsets) and np.array_equal(r1.start, r2.start)
            assert np.array_equal(r1.length, r2.length) and np.array_equal(r1.state, r2.state)
        plist = [p.astype(np.int32) for p in paths]
        got = bhmm_amd.path_logprob(obs, [model], paths=plist)
        flat = np.concatenate(plist)
        w = ex.path_logprob(flat, [(A, pi, None, None)]) + shifts[None, :]
        np.testing.assert_allclose(got, w, rtol=1e-11, atol=1e-11)
        vit = bhmm_amd.path_logprob(obs, model)                               # the Viterbi path, decoded and scored
        np.testing.assert_allclose(vit, ex.decode_logprob(A, pi) + shifts, rtol=1e-11, atol=1e-11)
        assert np.all(vit <= want + 1e-11 * (1.0 + np.abs(want)))
        assert np.all(got[0] <= vit + 1e-11 * (1.0 + np.abs(vit)))            # no path beats the Viterbi path
    finally:
        ex.close()


def test_all_paths_of_a_short_trajectory_sum_to_the_likelihood():
    import bhmm_amd
    n, T = 3, 6
    A, pi, rates, _, _ = _problem(n, 2, 77)
    x = np.random.default_rng(8).poisson(rates[[0, 1, 1, 2, 0, 2]])
    allp = np.array(list(itertools.product(range(n), repeat=T)), dtype=np.int32)      # (729, 6)
    model = bhmm_amd.poisson_hmm(pi, A, rates)
    obs = [x] * len(allp)
    lp = bhmm_amd.path_logprob(obs, model, paths=allp.ravel())[0]
    ll = bhmm_amd.score([x], model, per_trajectory=True)[0, 0]
    total = math.fsum(np.exp(lp).tolist())
    print("sum over paths", total, "likelihood", math.exp(ll))
    assert abs(total - math.exp(ll)) <= 1e-10 * math.exp(ll)


# ---- 7. EM ---------------------------------------------------------------------------------------------------------------
def _synthetic():
    rng = np.random.default_rng(0)
    P = np.array([[0.95, 0.03, 0.02], [0.04, 0.94, 0.02], [0.03, 0.03, 0.94]])
    obs, paths = [], []
    for T in (2000,) * 4:
        s = np.zeros(T, dtype=np.int64)
        s[0] = rng.integers(0, 3)
        u = rng.random(T)
        for t in range(1, T):
            s[t] = min(2, np.searchsorted(np.cumsum(P[s[t - 1]]), u[t]))
        obs.append(rng.poisson(TRUE_RATES[s]))
        paths.append(s)
    return obs, paths


def test_twenty_em_steps_never_lower_the_likelihood_and_find_the_rates():
    import bhmm_amd
    obs, paths = _synthetic()
    print("points per state", np.bincount(np.concatenate(paths), minlength=3).tolist())
    model = bhmm_amd.init_poisson_hmm(obs, 3)
    est = bhmm_amd.MaximumLikelihoodEstimator(obs, 3, initial_model=model)
    ll = [est.em_step() for _ in range(20)]
    print("log-likelihoods:", ll)
    for a, b in zip(ll[:-1], ll[1:]):
        assert b - a >= -1e-9 * (1.0 + abs(a))
    got = est.hmm.output_model.rates
    got = got[np.argsort(got.sum(axis=1))]
    print("fitted rates", got.tolist())
    np.testing.assert_allclose(got, TRUE_RATES, rtol=0.10)


def test_estimate_hmm_takes_the_route_for_integer_arrays():
    import bhmm_amd
    obs, _ = _synthetic()
    assert obs[0].dtype == np.int64
    hmm = bhmm_amd.estimate_hmm(obs, 3)
    assert hmm.output_model.model_type == 'poisson'
    got = hmm.output_model.rates
    np.testing.assert_allclose(got[np.argsort(got.sum(axis=1))], TRUE_RATES, rtol=0.10)
    assert len(hmm.hidden_state_trajectories) == 4


@pytest.mark.parametrize("n", [3, 17])
def test_em_step_equals_the_numpy_restatement(n):
    import bhmm_amd
    A, pi, rates, obs, _ = _problem(n, 2, 60 + n)
    rates0 = rates * np.random.default_rng(1).uniform(0.8, 1.25, rates.shape)      # some way off the generating one
    model = bhmm_amd.poisson_hmm(pi, A, rates0)
    rows, _, shifts = _np_scaled(obs, rates0)
    ref = _oracle_estep(rows, A, pi)
    x = np.concatenate(obs, axis=0).astype(np.float64)
    g = np.concatenate(ref['gammas'], axis=0)
    rates1 = g.T.dot(x) / g.sum(axis=0)[:, None]
    T1 = ref['C'] / ref['C'].sum(axis=1)[:, None]
    pi1 = ref['gamma0_sum'] / ref['gamma0_sum'].sum()
    est = bhmm_amd.MaximumLikelihoodEstimator(obs, n, initial_model=model, reversible=False)
    ll = est.em_step()
    want = (ref['logL'] + shifts).sum()
    assert abs(ll - want) <= 1e-11 * (1.0 + abs(want))
    np.testing.assert_allclose(est.hmm.output_model.rates, rates1, rtol=1e-9)
    np.testing.assert_allclose(est.hmm.transition_matrix, T1, rtol=1e-9)
    np.testing.assert_allclose(est.hmm.initial_distribution, pi1, rtol=1e-9)


# ---- 8. errors -------------------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    N, D = 3, 2
    A, pi = np.full((N, N), 1.0 / 3), np.ones(N) / N
    obs = [np.random.default_rng(0).poisson(TRUE_RATES[np.arange(60) % 3])]
    eng = _engine(obs, N)
    try:
        with pytest.raises(ValueError):
            eng.score([(A, pi, TRUE_RATES[:, :1], None)])                 # wrong D
        with pytest.raises(ValueError):
            eng.score([(A, pi, TRUE_RATES, TRUE_RATES)])                  # par1 must be None
        with pytest.raises(ValueError):
            eng.viterbi(A, pi)                                            # no rates
        assert np.all(np.isfinite(eng.score([(A, pi, TRUE_RATES, None)])))
        gd = torch.ones(60 * N, dtype=torch.float64, device='cuda:0')
        with pytest.raises(NotImplementedError):
            eng.estep(A, pi, TRUE_RATES, None, single=True)
        with pytest.raises(NotImplementedError):
            eng.estep_launch(A, pi, TRUE_RATES, None, stats_dev=gd.data_ptr())
        with pytest.raises(NotImplementedError):
            eng.set_observations_lagged('poisson', obs, 2, [(0, 0)], N)
        with pytest.raises(NotImplementedError):
            eng.sample_paths_moments(A, pi, TRUE_RATES, None)
        with pytest.raises(ValueError):
            eng.set_observations('mvgaussian', obs, N)
        with pytest.raises(ValueError):
            eng.set_observations('poisson', [np.zeros((5, 65), int)], N)
        assert np.isfinite(eng.estep(A, pi, TRUE_RATES, None).loglik)
        pm = eng.path_moments(np.arange(60, dtype=np.int32) % 3, TRUE_RATES, 'diag')       # inherited, hard labels
        x = obs[0].astype(np.float64)
        for i in range(N):
            assert pm.reshape(N, 1 + 2 * D)[i, 0] == 20.0
            np.testing.assert_allclose(pm.reshape(N, 1 + 2 * D)[i, 1:1 + D], (x[i::3] - TRUE_RATES[i]).sum(axis=0),
                                       rtol=1e-12, atol=1e-12)
    finally:
        eng.close()
