"""GPU: 513 to 4096 hidden states -- the seven eighths of the range the C ABI accepts (bhmm_ctx_set_observations
refuses only above 4096) in which every call has ONE route: tile_gen_capable is false, so the E-step is
k_gen_forward<false> / k_gen_backward<.., false> / k_gen_xi_gemm, Viterbi k_gen_viterbi_fwd<false>, the draw
k_gen_sample<false>, score and filter the serial kernels.  Everything is compared with the float64 CPU oracle
(oracle/oracle.py); no GPU call is checked against another GPU call alone.

State counts (each for a reason) and trajectory lengths (a single step, two steps, a first and a last step):

    513   first n without the matrix-core route; thread 0 alone owns a third state        (24, 1, 2, 9)
    1025  first n with a second state per thread in k_score_serial / k_filter_serial
          (only j = 1024), sixteen wavefronts in score_block_reduce                       (24, 1, 2, 9)
    2050  gen_nsplit falls to 1 (2048 still gives 2), ragged last xi tile, backward
          kernel still below 64 KiB of LDS                                                (6, 1, 3)
    2650  the backward kernel's (3 n + 257) * 8 bytes of LDS just above 64 KiB (from 2646 on)     (6, 1, 3)
    4095  backward and sample kernels above 64 KiB of LDS, forward exactly at 64 KiB;
          every thread but the last owns 16 states                                        (6, 1, 3)
    4096  the limit: forward kernel 16 bytes above 64 KiB, 16384-workgroup xi grid        (4, 1, 2)

(4096: with (6, 1, 3) two tests took more than 10 s, most of it in the oracle on the CPU, whose walks down the columns
of a matrix exactly 4096 doubles wide are far slower than at 4095.)

Bounds: those of tests/test_general_n_gpu.py for the E-step (logL rtol 1e-11; C and state counts rtol 1e-9 / atol
1e-12; gamma0 and every stored gamma row rtol 1e-9 / atol 1e-14; sum C = sum (T - 1) within 1e-11), of
tests/test_big_gpu.py for sum_gd / sum_gdd (rtol 1e-8 / atol 1e-9) and the symbol counts (rtol 1e-9 / atol 1e-12),
of tests/test_score_gpu.py for the scores (rtol 1e-11), of tests/test_filter_gpu.py::test_parity_serial for the
filter, of tests/test_posterior_gpu.py / tests/test_marginals_gpu.py::test_parity_generic for posterior decoding and
marginals; Viterbi paths, sampled paths and their counts, alpha / beta rows of the hidden API and everything about
runs are compared exactly.  An ordered sum of 4096 positive terms carries at most about 4096 * 2^-53 = 5e-13 of
relative error, so the bounds have room at the largest n; every E-step prints its worst deviation as a fraction of
its bound.

Model, data and oracle results are built once per (n, kind) and shared by all tests of that pair (the oracle costs
more than the kernels up here); nothing below writes to them.  The seeds were chosen on the CPU so that what a test
presupposes of the ORACLE holds (asserted on the oracle alone, before any comparison): no emission row of a
gaussian case lies in the denormal range (where the oracle itself keeps only a few digits), and for posterior
decoding the smallest gap between the two largest gamma of a step is at least 1e-7 -- with fewer than 100 steps per
case the MAX_LEFT_OUT cap of tests/test_posterior_gpu.py allows no step to be left out of the path comparison."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc
from tests.filter_oracle_engine import FilterOracleEngine
from tests.oracle_engine import OracleEngine
from tests.test_filter_gpu import _check_logc, _check_rows, _truth_pobs
from tests.test_general_n_gpu import _model
from tests.test_marginals_gpu import _check as _check_marginals
from tests.test_marginals_gpu import _weights
from tests.test_path_runs_gpu import _rle, _same
from tests.test_posterior_gpu import GAP, MAX_LEFT_OUT, _check
from tests.test_tile_matrix_gpu import _frac

pytestmark = pytest.mark.gpu

M = 37
KINDS = ("gaussian", "discrete", "explicit")
LENGTHS = {513: (24, 1, 2, 9), 1025: (24, 1, 2, 9), 2050: (6, 1, 3), 2650: (6, 1, 3), 4095: (6, 1, 3), 4096: (4, 1, 2)}
ALL = [(513, "gaussian"), (513, "discrete"), (513, "explicit"), (1025, "gaussian"), (1025, "discrete"),
       (1025, "explicit"), (2050, "discrete"), (2650, "discrete"), (4095, "discrete"), (4096, "gaussian"),
       (4096, "discrete")]
SCORED = [(513, "gaussian"), (513, "discrete"), (1025, "gaussian"), (1025, "discrete"), (1025, "explicit"),
          (4096, "gaussian"), (4096, "discrete")]
DECODED = [(513, "gaussian"), (513, "discrete"), (1025, "gaussian"), (1025, "discrete")]
MIN_GAP = 1e-7
# (rtol, atol): tests/test_general_n_gpu.py, tests/test_big_gpu.py
BOUNDS = dict(logL=(1e-11, 0.0), C=(1e-9, 1e-12), gamma0=(1e-9, 1e-14), counts=(1e-9, 1e-12), gamma=(1e-9, 1e-14),
              Csum=(1e-11, 0.0), sum_gd=(1e-8, 1e-9), sum_gdd=(1e-8, 1e-9), symbols=(1e-9, 1e-12))
RTOL_SCORE = 1e-11


def _ids(cases):
    return ["%d-%s" % c for c in cases]


# ---- one model, one data set and one oracle result per (n, kind) ----------------------------------------
class _Case(object):
    def __init__(self, n, kind):
        self.n, self.kind, self.M = n, kind, (M if kind == "discrete" else 0)
        self.lengths = LENGTHS[n]
        self.label = "n=%d %s" % (n, kind)
        rng = np.random.default_rng(9000 + 10 * n + KINDS.index(kind))
        self.model = _model(n, rng, kind, M, sparse=0.3)
        if kind == "gaussian":
            self.obs = [rng.normal(0, 0.06 * n, T) for T in self.lengths]
        elif kind == "discrete":
            self.obs = [rng.integers(0, M, T).astype(np.int32) for T in self.lengths]
        else:
            self.obs = [rng.random((T, n)) ** 3 + 1e-5 for T in self.lengths]
        self.u = [rng.random(T) for T in self.lengths]
        self._memo = {}

    def _once(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def pobs_under(self, model, obs=None):
        obs = self.obs if obs is None else obs
        if self.kind == "gaussian":
            return [orc.pobs_gaussian(o, model[2], model[3]) for o in obs]
        if self.kind == "discrete":
            return [orc.pobs_discrete(o, model[2]) for o in obs]
        return obs

    @property
    def pobs(self):
        def make():
            pobs = self.pobs_under(self.model)
            if self.kind == "gaussian":      # (of the oracle alone: its rows keep their digits)
                for p in pobs:
                    assert p.max(axis=1).min() > 1e-290, "%s: an emission row in the denormal range" % self.label
            return pobs
        return self._once("pobs", make)

    @property
    def forward(self):
        """[(logL, alpha rows)] of the oracle"""
        A, pi = self.model[:2]
        return self._once("forward", lambda: [orc.forward(A, p, pi) for p in self.pobs])

    @property
    def truth(self):
        """[(rows, logc, extra, logL)] as tests/test_filter_gpu.py::_truth_pobs returns them, from the rows of
        `forward` (one oracle pass less per case)"""
        def make():
            A, pi = (np.asarray(x, dtype=np.float64) for x in self.model[:2])
            out = []
            for p, (logL, alpha) in zip(self.pobs, self.forward):
                c, extra = np.empty(len(p)), np.empty(len(p))
                c[0] = np.dot(pi, p[0])
                extra[0] = p[0].sum() / c[0]
                c[1:] = np.einsum('tj,tj->t', alpha[:-1] @ A, p[1:])
                extra[1:] = (p[1:] @ A.sum(axis=0)) / c[1:]
                out.append((alpha, np.log(c), extra, logL))
            return out
        return self._once("truth", make)

    @property
    def model2(self):
        """a second, different model of the same shape"""
        return self._once("model2", lambda: _model(self.n, np.random.default_rng(77000 + self.n), self.kind, M,
                                                   sparse=0.3))

    @property
    def estep(self):
        def make():
            n = self.n
            A, pi, p0, p1 = self.model
            if self.kind == "explicit":      # the per-trajectory loop of tests/test_general_n_gpu.py
                lls, Cs, g0, sc, gam = [], np.zeros((n, n)), np.zeros(n), np.zeros(n), []
                for o, (ll, al) in zip(self.obs, self.forward):
                    be = orc.backward(A, o)
                    gm = orc.gamma(al, be)
                    lls.append(ll)
                    gam.append(gm)
                    g0 += gm[0]
                    sc += gm.sum(axis=0)
                    if len(o) > 1:
                        Cs += orc.transition_counts(al, be, A, o)
                ref = dict(logL=np.array(lls), C=Cs, gamma0_sum=g0, state_counts=sc, gammas=gam)
            else:
                ref = orc.estep(self.kind, self.obs, A, pi, p0, p1, want_gamma=True)
            want = dict(logL=ref["logL"], C=ref["C"], gamma0=ref["gamma0_sum"], counts=ref["state_counts"],
                        gamma=np.concatenate(ref["gammas"]), Csum=float(sum(max(T - 1, 0) for T in self.lengths)))
            if self.kind == "gaussian":      # the formula of tests/test_big_gpu.py
                want["sum_gd"] = sum((g * (o[:, None] - p0[None, :])).sum(axis=0)
                                     for o, g in zip(self.obs, ref["gammas"]))
                want["sum_gdd"] = sum((g * (o[:, None] - p0[None, :]) ** 2).sum(axis=0)
                                      for o, g in zip(self.obs, ref["gammas"]))
            elif self.kind == "discrete":
                cnt = np.zeros((n, M))
                for o, g in zip(self.obs, ref["gammas"]):
                    orc.update_pout(o, g, cnt)
                want["symbols"] = cnt
            want["gammas"] = ref["gammas"]
            return want
        return self._once("estep", make)

    def engine(self, obs=None):
        from bhmm_amd.engine import Engine
        eng = Engine(0)
        eng.set_observations(self.kind, self.obs if obs is None else obs, self.n, nsymbols=self.M)
        return eng


_CASES = {}


def _case(n, kind):
    if (n, kind) not in _CASES:
        _CASES[(n, kind)] = _Case(n, kind)
    return _CASES[(n, kind)]


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _CASES.clear()       # (up to three n x n matrices per case)


# ---- 1. E-step -------------------------------------------------------------------------------------------
def _estep_checked(case, eng):
    """one E-step with stored gamma against the oracle, every quantity printed as a fraction of its bound; then
    the same E-step without gamma"""
    want = case.estep
    res = eng.estep(*case.model, store_gamma=True)
    assert eng.get_option("tile") == 0, "%s: not the order-faithful family" % case.label
    got = dict(logL=res.logL_k, C=res.C, gamma0=res.gamma0_sum, counts=res.state_counts, Csum=res.C.sum(),
               gamma=np.concatenate([eng.gamma(k) for k in range(len(case.lengths))]))
    if case.kind == "gaussian":
        got.update(sum_gd=res.sum_gd, sum_gdd=res.sum_gdd)
    elif case.kind == "discrete":
        got.update(symbols=res.symbol_counts)
    fr = dict((key, _frac(v, want[key], *BOUNDS[key])) for key, v in got.items())
    print("%s (tile 0): " % case.label + ", ".join("%s %.3g" % kv for kv in fr.items()) + " of bound")
    for key, v in fr.items():
        assert v <= 1.0, "%s: %s at %.3g of its bound" % (case.label, key, v)
    for k, g in enumerate(want["gammas"]):       # (every stored row of every trajectory, by the neighbour's call)
        np.testing.assert_allclose(eng.gamma(k), g, rtol=1e-9, atol=1e-14)
    plain = eng.estep(*case.model)
    assert eng.get_option("tile") == 0
    if case.kind == "discrete":                  # (the symbol table is summed with atomics)
        np.testing.assert_allclose(plain.packed, res.packed, rtol=1e-12, atol=0.0)
    else:
        assert np.array_equal(plain.packed, res.packed), case.label
    assert np.array_equal(plain.logL_k, res.logL_k)


@pytest.mark.parametrize("n,kind", ALL, ids=_ids(ALL))
def test_estep(n, kind):
    case = _case(n, kind)
    eng = case.engine()
    try:
        _estep_checked(case, eng)
    finally:
        eng.close()


# ---- 2. Viterbi ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", ALL, ids=_ids(ALL))
def test_viterbi(n, kind):
    case = _case(n, kind)
    A, pi = case.model[:2]
    want = [orc.viterbi(A, p, pi) for p in case.pobs]
    eng = case.engine()
    try:
        paths = eng.viterbi(*case.model)
        assert eng.get_option("viterbi_chunked") == 0
        with pytest.raises(ValueError):
            eng.viterbi_u8(*case.model)
    finally:
        eng.close()
    for p, w in zip(paths, want):
        assert p.dtype == np.int32 and np.array_equal(p, w), case.label


# ---- 3. path sampling ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", ALL, ids=_ids(ALL))
def test_sample_paths(n, kind):
    case = _case(n, kind)
    A, pi, p0, p1 = case.model
    want = [orc.sample_path(al, A, u=u) for (_, al), u in zip(case.forward, case.u)]
    wC, wn0 = orc.path_counts(want, n)
    eng = case.engine()
    try:
        paths, C, n0, _ = eng.sample_paths(A, pi, p0, p1, u=case.u)
        assert eng.get_option("sample_segmented") == 0
        seeded = eng.sample_paths(A, pi, p0, p1, seed=77) if kind != "explicit" else None
        assert eng.get_option("sample_segmented") == 0
    finally:
        eng.close()
    print("%s: sample_segmented 0" % case.label)
    for p, w in zip(paths, want):
        assert np.array_equal(p, w), case.label
    assert np.array_equal(C, wC) and np.array_equal(n0, wn0)
    if seeded is not None:                       # the device stream, as tests/test_general_n_gpu.py
        oe = OracleEngine()
        oe.set_observations(kind, case.obs, n, nsymbols=case.M)
        rp, rC, rn0, remis = oe.sample_paths(A, pi, p0, p1, seed=77)
        for p, w in zip(seeded[0], rp):
            assert np.array_equal(p, w), case.label
        assert np.array_equal(seeded[1], rC) and np.array_equal(seeded[2], rn0)
        np.testing.assert_allclose(seeded[3], remis, rtol=1e-10, atol=1e-9)


# ---- 4. / 5. score and filter: special data at 1025 ------------------------------------------------------
def _outlier_obs(case):
    """gaussian: every density exactly zero in the middle of the 24-step trajectory (a row of ones, as the oracle's
    pobs_gaussian(ignore_outliers=True) has it), and a NaN observation (a row of ones too)"""
    obs = [o.copy() for o in case.obs]
    obs[0][12] = 1e6
    obs[0][18] = np.nan
    mu, sig = case.model[2:]
    pobs = []
    for o in obs:                                # (the rule of tests/test_filter_gpu.py for these rows)
        p = orc.pobs_gaussian(np.where(np.isnan(o), 1e6, o), mu, sig)
        bad = ~np.all(np.isfinite(p), axis=1) | np.all(p == 0.0, axis=1)
        p[bad] = 1.0
        pobs.append(p)
    assert np.all(pobs[0][12] == 1.0) and np.all(pobs[0][18] == 1.0)
    return obs, pobs


ZSYM, ZSTEP = M - 1, 5


def _zero_symbol(case):
    """discrete: a model no state of which emits symbol ZSYM, and data in which it occurs once, at step ZSTEP of
    trajectory 0"""
    A, pi, B, _ = case.model
    Bz = B.copy()
    Bz[:, ZSYM] = 0.0
    Bz /= Bz.sum(axis=1)[:, None]
    obs = [np.where(o == ZSYM, 0, o).astype(np.int32) for o in case.obs]
    obs[0][ZSTEP] = ZSYM
    return obs, (A, pi, Bz, None)


def _scores(case, model, pobs=None):
    pobs = case.pobs_under(model) if pobs is None else pobs
    return np.array([orc.forward(model[0], p, model[1])[0] for p in pobs])


@pytest.mark.parametrize("n,kind", SCORED, ids=_ids(SCORED))
def test_score(n, kind):
    case = _case(n, kind)
    m1, m2 = case.model, case.model2
    want = np.stack([np.array([ll for ll, _ in case.forward]), _scores(case, m2)])
    eng = case.engine()
    try:
        got = eng.score([m1, m2])                # (two models: the A_all + s * n * n offsets)
        assert eng.get_option("score_path") == 0
    finally:
        eng.close()
    assert got.shape == want.shape and np.all(np.isfinite(want))
    print("%s (score_path 0): worst |score - oracle| / |oracle| %.3g, bound %.3g"
          % (case.label, float((np.abs(got - want) / np.abs(want)).max()), RTOL_SCORE))
    np.testing.assert_allclose(got, want, rtol=RTOL_SCORE)
    if n != 1025 or kind == "explicit":
        return
    if kind == "gaussian":
        obs, pobs = _outlier_obs(case)
        want = np.stack([_scores(case, m1, pobs), _scores(case, m2, _outlier_pobs_under(case, obs, m2))])
        eng = case.engine(obs)
        try:
            got = eng.score([m1, m2])
            assert eng.get_option("score_path") == 0
        finally:
            eng.close()
        print("%s outlier + NaN: worst |score - oracle| / |oracle| %.3g"
              % (case.label, float((np.abs(got - want) / np.abs(want)).max())))
        np.testing.assert_allclose(got, want, rtol=RTOL_SCORE)
    else:
        obs, mz = _zero_symbol(case)
        cut = [obs[0][:ZSTEP]] + obs[1:]          # (trajectory 0 under mz: -inf, not compared)
        want = np.stack([_scores(case, mz, case.pobs_under(mz, cut)), _scores(case, m2, case.pobs_under(m2, obs))])
        eng = case.engine(obs)
        try:
            got = eng.score([mz, m2])
            assert eng.get_option("score_path") == 0
        finally:
            eng.close()
        assert got[0, 0] == -np.inf              # trajectory 0 under the model that cannot emit its symbol
        np.testing.assert_allclose(got[0, 1:], want[0, 1:], rtol=RTOL_SCORE)
        np.testing.assert_allclose(got[1], want[1], rtol=RTOL_SCORE)
        assert np.all(np.isfinite(got[1]))


def _outlier_pobs_under(case, obs, model):
    out = []
    for o in obs:
        p = orc.pobs_gaussian(np.where(np.isnan(o), 1e6, o), model[2], model[3])
        p[~np.all(np.isfinite(p), axis=1) | np.all(p == 0.0, axis=1)] = 1.0
        out.append(p)
    return out


def _filter_checked(case, eng, model, truth, label, upto=None):
    """rows and increments in fp64, a projection on two columns, fp32 rows: all on the serial kernel; upto: the
    steps of each trajectory that are compared (None: all)"""
    cut = (lambda xs: xs) if upto is None else (lambda xs: [x[:u] for x, u in zip(xs, upto)])
    rng = np.random.default_rng(5)
    rows, logc = eng.filter_states(*model)
    assert eng.get_option("filter_path") == 0
    _check_rows(truth, cut(rows), np.float64, None, label)
    _check_logc(truth, cut(logc), np.float64, label, dense=False)      # (A has structural zeros)
    V = _weights(case.n, 2, model, rng)
    proj, none = eng.filter_states(*model, weights=V, increments=False)
    assert none is None and eng.get_option("filter_path") == 0
    _check_rows(truth, cut(proj), np.float64, V, label + " Q=2")
    r32, l32 = eng.filter_states(*model, dtype=np.float32)
    assert eng.get_option("filter_path") == 0
    _check_rows(truth, cut(r32), np.float32, None, label + " float32")
    _check_logc(truth, cut(l32), np.float32, label + " float32", dense=False)
    return rows, logc, proj


@pytest.mark.parametrize("n,kind", SCORED, ids=_ids(SCORED))
def test_filter(n, kind):
    case = _case(n, kind)
    A, pi = case.model[:2]
    truth = case.truth
    if kind != "explicit" and n <= 1025:         # the estimator's test double computes the same rows and increments
        foe = FilterOracleEngine()
        foe.set_observations(kind, case.obs, n, nsymbols=case.M)
        orows, ologc = foe.filter_states(*case.model)
        for (a, lc, _, _), r, l in zip(truth, orows, ologc):
            assert np.array_equal(a, r) and np.array_equal(lc, l)
    eng = case.engine()
    try:
        rows, logc, _ = _filter_checked(case, eng, case.model, truth, case.label + " (filter_path 0)")
    finally:
        eng.close()
    want = np.array([ll for ll, _ in case.forward])
    sums = np.array([l.sum() for l in logc])
    np.testing.assert_allclose(sums, want, rtol=1e-11)      # the increments of a trajectory sum to its score
    if n != 1025 or kind == "explicit":
        return
    if kind == "gaussian":
        obs, pobs = _outlier_obs(case)
        eng = case.engine(obs)
        try:
            _filter_checked(case, eng, case.model, [_truth_pobs(A, p, pi) for p in pobs], case.label + " outlier + NaN")
        finally:
            eng.close()
    else:
        obs, mz = _zero_symbol(case)
        upto = [ZSTEP] + [len(o) for o in obs[1:]]
        truth = [_truth_pobs(A, p, pi) for p in case.pobs_under(mz, [o[:u] for o, u in zip(obs, upto)])]
        eng = case.engine(obs)
        try:
            rows, logc, proj = _filter_checked(case, eng, mz, truth, case.label + " zero from step %d" % ZSTEP, upto)
        finally:
            eng.close()
        assert rows[0].shape == (case.lengths[0], n) and np.all(rows[0][ZSTEP:] == 0.0)
        assert np.all(proj[0][ZSTEP:] == 0.0) and np.all(logc[0][ZSTEP:] == -np.inf)
        assert all(np.all(np.isfinite(l)) for l in logc[1:]) and np.all(np.isfinite(logc[0][:ZSTEP]))


# ---- 6. posterior decoding and marginals -----------------------------------------------------------------
@pytest.mark.parametrize("n,kind", DECODED, ids=_ids(DECODED))
def test_posterior_decoding_and_marginals(n, kind):
    from bhmm_amd import _lib
    case = _case(n, kind)
    gam = case.estep["gammas"]
    # of the oracle alone: no step is a near-tie, so none may be left out
    gap = min(float(np.diff(np.sort(g, axis=1)[:, -2:], axis=1).min()) for g in gam)
    print("%s: smallest gap between the two largest gamma of a step %.3g" % (case.label, gap))
    assert gap >= MIN_GAP > GAP and MAX_LEFT_OUT * sum(case.lengths) < 1
    eng = case.engine()
    try:
        paths, conf = eng.posterior_decode(*case.model, confidence=True)
        assert eng.get_option("post_path") == 0
        Ap, pip, e0, e1 = eng._model_ptrs(*case.model)
        buf = np.empty(sum(case.lengths), dtype=np.uint8)
        with pytest.raises(ValueError):          # the one-byte form
            _lib.check(eng._L.bhmm_posterior_decode(eng._h, Ap, pip, e0, e1, ctypes.c_void_p(buf.ctypes.data), 1, None))
        results = []
        rng = np.random.default_rng(6)
        for dtype in (np.float64, np.float32):   # the forms of tests/test_marginals_gpu.py::test_parity_generic
            rows = eng.posterior_marginals(*case.model, dtype=dtype)
            assert eng.get_option("marg_path") == 0
            V = _weights(n, 3, case.model, rng)
            results.append((rows, dtype, None))
            results.append((eng.posterior_marginals(*case.model, weights=V, dtype=dtype), dtype, V))
            assert eng.get_option("marg_path") == 0
    finally:
        eng.close()
    assert all(p.dtype == np.int32 for p in paths)
    steps, left = _check(gam, paths, conf, case.label + " (post_path 0)")
    assert left == 0 and steps == sum(case.lengths)
    for rows, dtype, V in results:
        _check_marginals(gam, rows, dtype, V, "%s (marg_path 0) %s%s" % (case.label, np.dtype(dtype).name,
                                                                         "" if V is None else " Q=3"))


# ---- 7. the single-trajectory hidden API -----------------------------------------------------------------
@pytest.mark.parametrize("n,T", [(513, 30), (1025, 30), (4096, 6)])
def test_hidden_api(n, T):
    """what tests/test_general_n_gpu.py::test_hidden_api_any_number_of_states asserts, under its bounds (that
    function fixes its own lengths): alpha and beta rows and the paths bit for bit, logL to 1e-12, counts to 1e-9"""
    from bhmm_amd import _lib, hidden
    rng = np.random.default_rng(n)
    A, pi, _, _ = _model(n, rng, "explicit")
    pobs = rng.random((T, n)) ** 4 + 1e-6
    pobs[2] = 0.0
    pobs[2, n - 3] = 0.7                                     # a row with a single possible state
    ll_ref, a_ref = orc.forward(A, pobs, pi)
    b_ref = orc.backward(A, pobs)
    ll, alpha = hidden.forward(A, pobs, pi)
    beta = hidden.backward(A, pobs)
    np.testing.assert_allclose(ll, ll_ref, rtol=1e-12)
    assert np.array_equal(alpha, a_ref) and np.array_equal(beta, b_ref)
    g = hidden.state_probabilities(alpha, beta)
    np.testing.assert_allclose(g, orc.gamma(a_ref, b_ref), rtol=1e-12, atol=1e-300)
    C = hidden.transition_counts(alpha, beta, A, pobs)
    np.testing.assert_allclose(C, orc.transition_counts(a_ref, b_ref, A, pobs), rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(C.sum(), T - 1, rtol=1e-11)
    assert np.array_equal(hidden.viterbi(A, pobs, pi), orc.viterbi(A, pobs, pi))
    u = orc.libc_uniforms(T, 5)
    L = _lib.load()
    path = np.empty(T, dtype=np.int32)
    _lib.check(L.bhmm_sample_path(_lib.ip(path), _lib.dp(_lib.f64(a_ref)), _lib.dp(_lib.f64(A)),
                                  _lib.dp(_lib.f64(u)), n, T))
    assert np.array_equal(path, orc.sample_path(a_ref, A, u=u))


# ---- 8. the limit ----------------------------------------------------------------------------------------
def test_4097_states_are_refused_and_the_library_stays_usable():
    from bhmm_amd import _lib, hidden
    from bhmm_amd.engine import Engine
    n = 4097
    A = np.full((n, n), 1.0 / n)
    pi = np.full(n, 1.0 / n)
    pobs = np.full((2, n), 0.5)
    eng = Engine(0)
    try:
        with pytest.raises(ValueError, match="4096"):        # bhmm_ctx_set_observations
            eng.set_observations("discrete", [np.zeros(3, dtype=np.int32)], n, nsymbols=M)
        with pytest.raises(ValueError, match="4096"):
            eng.set_observations("explicit", [pobs], n)
    finally:
        eng.close()
    alpha = np.full((2, n), -1.0)
    with pytest.raises(ValueError, match="4096"):
        hidden.forward(A, pobs, pi, alpha_out=alpha)
    assert np.all(alpha == -1.0)                             # nothing was written
    rows = np.full((2, n), 1.0 / n)
    C = np.full((n, n), -1.0)
    with pytest.raises(ValueError, match="4096"):
        hidden.transition_counts(rows, rows, A, pobs, out=C)
    assert np.all(C == -1.0)
    path = np.full(2, -1, dtype=np.int32)
    u = np.array([0.25, 0.75])
    L = _lib.load()
    assert L.bhmm_sample_path(_lib.ip(path), _lib.dp(rows), _lib.dp(A), _lib.dp(u), n, 2) == _lib.ERR_INVALID
    with pytest.raises(ValueError, match="4096"):
        _lib.check(L.bhmm_sample_path(_lib.ip(path), _lib.dp(rows), _lib.dp(A), _lib.dp(u), n, 2))
    assert np.all(path == -1)
    # a fresh engine right afterwards: the E-step comparison of test_estep
    case = _case(513, "discrete")
    eng = case.engine()
    try:
        _estep_checked(case, eng)
    finally:
        eng.close()


# ---- 9. runs of a path with large state indices ------------------------------------------------------------
def test_path_runs_with_4096_states():
    """the global-atomics branch of the statistics (far above STATS_LDS_MAX_N): runs, dwell table and the
    4096 x 4096 jump matrix of a short int32 path that holds the states 0, 255, 256 and 4095"""
    from bhmm_amd.engine import Engine
    n = 4096
    lengths = [61, 1, 30, 2]
    total = sum(lengths)
    rng = np.random.default_rng(12)
    path = rng.choice(np.array([0, 255, 256, 4095, 4094, 1024, 2047, 2048]), total).astype(np.int32)
    path[[0, 1, 2, 3, 61, 62, total - 1]] = [4095, 0, 255, 256, 4095, 256, 4095]
    path[10:20] = 4095                           # a dwell
    for s in (0, 255, 256, 4095):
        assert (path == s).any()
    ref = _rle(path, lengths, n)
    eng = Engine(0)
    try:
        eng.set_observations("gaussian", [np.zeros(T) for T in lengths], n)
        _same(eng.path_runs(path, stats=True), ref, True, "n=4096 host")
        assert eng.get_option("runs_count") == ref[0][-1]
        _same(eng.path_runs(path), ref, False, "n=4096 host, no statistics")
        with pytest.raises(ValueError):          # one byte per step does not hold these states
            eng.path_runs(path.astype(np.uint8))
        with pytest.raises(ValueError):          # decode_runs: up to 256 states, as before
            eng.decode_runs(np.full((n, n), 1.0 / n), np.full(n, 1.0 / n), np.zeros(n), np.ones(n))
    finally:
        eng.close()
