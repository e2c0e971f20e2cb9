"""GPU: bhmm_posterior_transitions / Engine.posterior_transitions / bhmm_amd.posterior_transitions -- the pair
posterior xi_t(i, j) of every transition, as the probability of a jump or projected on a few pair weightings, in
double or float, against rows formed from the committed oracle alone (orc.pobs_*, orc.forward, orc.backward:
x_t = alpha_t[:, None] * A * (pobs_(t+1) * beta_(t+1))[None, :], normalised per step, numpy fp64;
tests/transitions_oracle_engine.py): the fused path (up to 8 states), the generic one (filter + marginals + pair
rows), the fallback protocol, bitwise invariances, consistency with posterior_marginals and the E-step's counts, and
the absence of side effects.

Tolerances: the project's own row rule of tests/test_marginals_gpu.py (fp64 rtol 1e-8, atol 1e-13 per entry of a
normalised row; fp32 1e-7 absolute), carried through the pair sum exactly as that file carries it through g @ V: an
entry xi_ij within atol + rtol * xi_ij gives a projection within
    1e-13 * sum_ij |W_ijq| + 1e-8 * (xi_t . |W|)_q            (fp64)
    1e-7 * sum_ij |W_ijq|                                     (fp32).
The jump form is the projection on the off-diagonal mask.  No new numbers, no excluded rows."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc
from tests.transitions_oracle_engine import jump_mask, oracle_rows

pytestmark = pytest.mark.gpu

RTOL64, ATOL64 = 1e-8, 1e-13
TOL32 = 1e-7
LENGTHS = [1, 2, 37, 500, 3001, 64, 129, 20000]


def _engine():
    from bhmm_amd.engine import Engine
    return Engine(0)


def _rand_A(n, rng, stay=0.0):
    A = rng.random((n, n)) + 0.05
    A += stay * np.eye(n) * A.sum(axis=1)[:, None]
    return A / A.sum(axis=1)[:, None]


def _rand_model(kind, n, M, rng, stay=0.0):
    A = _rand_A(n, rng, stay)
    pi = rng.random(n) + 0.1
    pi /= pi.sum()
    if kind == "gaussian":
        return (A, pi, np.sort(rng.normal(0, 3, n)), rng.uniform(0.5, 2.0, n))
    B = rng.random((n, M)) + 0.01
    return (A, pi, B / B.sum(axis=1)[:, None], None)


def _rand_obs(kind, n, M, lengths, rng):
    if kind == "gaussian":
        return [rng.normal(0, 3, T) for T in lengths]
    return [rng.integers(0, M, T).astype(np.int32) for T in lengths]


def _weights(n, Q, rng):
    """(n, n, Q): the off-diagonal mask first, one unit pair second, random beyond"""
    W = rng.normal(0, 2, (n, n, Q))
    W[:, :, 0] = jump_mask(n)[:, :, 0]
    if Q > 1:
        W[:, :, 1] = 0.0
        W[0, n - 1, 1] = 1.0
    return W


def _unit_pairs(n, pairs):
    W = np.zeros((n, n, len(pairs)))
    for q, (i, j) in enumerate(pairs):
        W[i, j, q] = 1.0
    return W


def _as2d(r):
    r = np.asarray(r)
    return r[:, None] if r.ndim == 1 else r


def _check(refs, rows, dtype, W, label=""):
    """every row against the oracle under the module's tolerances; prints the worst figures first.  refs: what
    oracle_rows returned for the weights W"""
    scale = np.abs(W).sum(axis=(0, 1))
    worst_abs = worst_ratio = 0.0
    for (want, wabs), r in zip(refs, rows):
        assert r.shape == want.shape and r.dtype == dtype, (label, r.shape, want.shape, r.dtype)
        if want.size == 0:
            continue
        err = np.abs(r.astype(np.float64) - want)
        assert np.all(np.isfinite(err)), label
        if dtype == np.float64:
            bound = scale * ATOL64 + RTOL64 * wabs
        else:
            bound = scale * TOL32 * np.ones_like(want)
        worst_abs = max(worst_abs, float((err / np.where(scale > 0, scale, 1.0)).max()))
        # (an all-zero column of W has bound 0: its projection must be exactly 0)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        worst_ratio = max(worst_ratio, float(ratio.max()))
    print("%s: worst |row - oracle| / scale %.3g, worst error / bound %.3g" % (label, worst_abs, worst_ratio))
    assert worst_ratio <= 1.0, label


def _check_jump(refs, rows, dtype, n, label):
    """the jump form under the bound of its defining projection (sum_ij |mask| = n * n - n)"""
    assert all(np.asarray(r).ndim == 1 for r in rows), label
    _check(refs, [_as2d(r) for r in rows], dtype, jump_mask(n), label)


# ---- 1. oracle parity, fused path -----------------------------------------------------------------
@pytest.mark.parametrize("stay", [0, 20])
@pytest.mark.parametrize("chunk", [0, 64, 100000])
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 3), ("discrete", 64), ("discrete", 1000)])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_parity_fused(n, kind, M, chunk, stay):
    import torch
    rng = np.random.default_rng(1000 * n + M + chunk % 7 + stay)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=float(stay))
    label = "fused n=%d %s M=%d chunk=%d stay=%d" % (n, kind, M, chunk, stay)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=chunk)
    total = int(eng.offsets[-1])
    results = []
    for dtype in (np.float64, np.float32):
        rows = eng.posterior_transitions(*model, dtype=dtype)
        assert eng.get_option("pair_path") == 1
        results.append((rows, dtype, None, "%s %s jump" % (label, np.dtype(dtype).name)))
        for Q in (1, 3, 8):
            W = _weights(n, Q, rng)
            rows = eng.posterior_transitions(*model, weights=W, dtype=dtype)
            assert eng.get_option("pair_path") == 1
            results.append((rows, dtype, W, "%s %s Q=%d" % (label, np.dtype(dtype).name, Q)))
    # the device-buffer form, once: every row of the buffer, the zero rows included
    W3 = results[-2][2]
    t = torch.full((total, 3), -1.0, dtype=torch.float32, device="cuda:0")
    views = eng.posterior_transitions(*model, weights=W3, dtype=np.float32, out=t)
    eng.sync()
    dev = t.cpu().numpy()
    fallbacks = eng.get_option("pair_fallbacks")
    off = np.asarray(eng.offsets)
    eng.close()
    assert np.array_equal(dev[off[1:] - 1], np.zeros((len(obs), 3), dtype=np.float32))   # last row: exactly zero
    assert all(v.shape == (T - 1, 3) for v, T in zip(views, LENGTHS))
    assert all(np.array_equal(dev[off[k]:off[k + 1] - 1], results[-2][0][k]) for k in range(len(obs)))
    for rows, dtype, W, lab in results:
        refs = oracle_rows(kind, obs, model, W)
        if W is None:
            _check_jump(refs, rows, dtype, n, lab)
        else:
            _check(refs, rows, dtype, W, lab)
    if stay == 0:
        assert fallbacks == 0


# ---- 2. the same parity on the generic path --------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [12, 40, 100])
def test_parity_generic(n, kind, M):
    rng = np.random.default_rng(7 * n + M)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng)
    W = _weights(n, 3, rng)
    ref_j, ref_p = oracle_rows(kind, obs, model), oracle_rows(kind, obs, model, W)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    for dtype in (np.float64, np.float32):
        rows = eng.posterior_transitions(*model, dtype=dtype)
        assert eng.get_option("pair_path") == 0
        _check_jump(ref_j, rows, dtype, n, "generic n=%d %s %s jump" % (n, kind, np.dtype(dtype).name))
        rows = eng.posterior_transitions(*model, weights=W, dtype=dtype)
        assert eng.get_option("pair_path") == 0
        _check(ref_p, rows, dtype, W, "generic n=%d %s %s Q=3" % (n, kind, np.dtype(dtype).name))
    eng.close()


@pytest.mark.parametrize("n", [3, 12])
def test_parity_explicit_pobs(n):
    import bhmm_amd
    rng = np.random.default_rng(50 + n)
    A, pi, mu, sig = _rand_model("gaussian", n, 0, rng)
    pobs = orc.pobs_gaussian(rng.normal(0, 3, 5000), mu, sig)
    W = _weights(n, 2, rng)
    model = (A, pi, None, None)
    ref_j, ref_p = oracle_rows("explicit", [pobs], model), oracle_rows("explicit", [pobs], model, W)
    for dtype in (np.float64, np.float32):
        _check_jump(ref_j, [bhmm_amd.hidden.posterior_transitions(A, pobs, pi, dtype=dtype)], dtype, n,
                    "explicit n=%d jump" % n)
        _check(ref_p, [bhmm_amd.hidden.posterior_transitions(A, pobs, pi, weights=W, dtype=dtype)], dtype, W,
               "explicit n=%d Q=2" % n)
    eng = _engine()
    eng.set_observations("explicit", [pobs], n)
    eng.posterior_transitions(A, pi)
    assert eng.get_option("pair_path") == 0
    eng.close()


@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_generic_against_fused_at_8_states(kind, M):
    rng = np.random.default_rng(88 + M)
    n = 8
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=2.0)
    W = _weights(n, 3, rng)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=64)
    fj, fp = eng.posterior_transitions(*model), eng.posterior_transitions(*model, weights=W)
    assert eng.get_option("pair_path") == 1 and eng.get_option("pair_fused") == 1
    eng.set_option("pair_fused", 0)
    gj, gp = eng.posterior_transitions(*model), eng.posterior_transitions(*model, weights=W)
    assert eng.get_option("pair_path") == 0
    eng.close()
    ref_j, ref_p = oracle_rows(kind, obs, model), oracle_rows(kind, obs, model, W)
    _check_jump(ref_j, gj, np.float64, n, "pair_fused 0 %s jump" % kind)
    _check(ref_p, gp, np.float64, W, "pair_fused 0 %s Q=3" % kind)
    # ... and against the fused result under the same bound (the fused rows standing where the oracle's did)
    mask = jump_mask(n)
    _check([(_as2d(f), ra) for f, (_, ra) in zip(fj, ref_j)], [_as2d(g) for g in gj], np.float64, mask,
           "pair_fused 0 against fused %s jump" % kind)
    _check([(f, ra) for f, (_, ra) in zip(fp, ref_p)], gp, np.float64, W, "pair_fused 0 against fused %s Q=3" % kind)


# ---- 3. forced protocol ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_forced_fallback(kind, M):
    rng = np.random.default_rng(31)
    n = 8
    obs = _rand_obs(kind, n, M, [60000, 40000, 12345], rng)
    model = _rand_model(kind, n, M, rng, stay=200.0)     # slowly mixing
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=512)
    eng.set_option("pair_W", 2)                          # far too short: the check must fail
    before = eng.get_option("pair_fallbacks")
    rows = eng.posterior_transitions(*model)
    assert eng.get_option("pair_fallbacks") > before
    assert eng.get_option("pair_path") == 1              # (the FIRST pass was the fused one)
    eng.close()
    _check_jump(oracle_rows(kind, obs, model), rows, np.float64, n, "forced %s" % kind)


# ---- 4. invariance, all bitwise --------------------------------------------------------------------
def _cat(xs):
    return np.concatenate([np.asarray(x) for x in xs])


@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_invariance(kind, M):
    import torch
    rng = np.random.default_rng(5)
    n = 8
    obs = _rand_obs(kind, n, M, [20000, 7000, 1, 12345, 64, 3001], rng)
    model = _rand_model(kind, n, M, rng, stay=3.0)
    W = _weights(n, 3, rng)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=256)
    total = int(eng.offsets[-1])
    j64 = _cat(eng.posterior_transitions(*model))
    p64 = _cat(eng.posterior_transitions(*model, weights=W))
    assert np.array_equal(_cat(eng.posterior_transitions(*model)), j64)            # repeated calls
    assert np.array_equal(_cat(eng.posterior_transitions(*model, weights=W)), p64)
    # a workspace budget that forces several ranges of chunk groups: the straddling pair of a range's first chunk
    # is then written by a lane of a later launch
    assert (eng.num_chunks + 63) // 64 >= 3
    eng.set_option("pair_ws_mb", 1)      # 256 steps * 8 states * 64 lanes * 8 B = 1 MiB: one group per range
    j1, p1 = _cat(eng.posterior_transitions(*model)), _cat(eng.posterior_transitions(*model, weights=W))
    eng.set_option("pair_ws_mb", 0)      # unbounded
    j0, p0 = _cat(eng.posterior_transitions(*model)), _cat(eng.posterior_transitions(*model, weights=W))
    assert np.array_equal(j1, j0) and np.array_equal(p1, p0)
    assert np.array_equal(j0, j64) and np.array_equal(p0, p64)
    # fp32 is the rounded fp64 result: the conversion is the last operation
    j32 = _cat(eng.posterior_transitions(*model, dtype=np.float32))
    p32 = _cat(eng.posterior_transitions(*model, weights=W, dtype=np.float32))
    assert j32.dtype == np.float32 and np.array_equal(j32, j64.astype(np.float32))
    assert np.array_equal(p32, p64.astype(np.float32))
    # the jump form is the projection on the off-diagonal mask, bitwise -- alone and as one column of several
    for dtype, ref in ((np.float64, j64), (np.float32, j32)):
        assert np.array_equal(_cat(eng.posterior_transitions(*model, weights=jump_mask(n), dtype=dtype))[:, 0], ref)
    assert np.array_equal(p64[:, 0], j64) and np.array_equal(p32[:, 0], j32)       # (column 0 of W is the mask)
    # a caller's host buffer: every row, the zero rows of the trajectories' ends included
    off = np.asarray(eng.offsets)
    keep = np.ones(total, dtype=bool)
    keep[off[1:] - 1] = False
    out = np.full(total, -1.0)
    views = eng.posterior_transitions(*model, out=out)
    assert np.array_equal(out[keep], j64) and np.all(out[~keep] == 0.0)
    assert views[0].base is not None and np.shares_memory(views[0], out)
    full64, full32 = out.copy(), out.astype(np.float32)
    # device output, tensor and raw address: bitwise the host output
    for dtype, tdtype, ref in ((np.float64, torch.float64, full64), (np.float32, torch.float32, full32)):
        t = torch.full((total,), -1.0, dtype=tdtype, device="cuda:0")
        tv = eng.posterior_transitions(*model, dtype=dtype, out=t)
        eng.sync()
        assert np.array_equal(t.cpu().numpy(), ref)
        assert tv[1].shape == (6999,) and tv[1].data_ptr() == t[20000:].data_ptr()
        t.fill_(-1.0)
        torch.cuda.synchronize()
        assert eng.posterior_transitions(*model, dtype=dtype, out=t.data_ptr()) is None
        eng.sync()
        assert np.array_equal(t.cpu().numpy(), ref)
    tp = torch.empty((total, 3), dtype=torch.float32, device="cuda:0")
    eng.posterior_transitions(*model, weights=W, dtype=np.float32, out=tp)
    eng.sync()
    assert np.array_equal(tp.cpu().numpy()[keep], p32) and np.all(tp.cpu().numpy()[~keep] == 0.0)
    # pinned host tensor
    th = torch.empty((total, 3), dtype=torch.float64).pin_memory()
    eng.posterior_transitions(*model, weights=W, out=th)
    assert np.array_equal(th.numpy()[keep], p64)
    assert eng.get_option("pair_path") == 1
    # the C ABI refuses what it cannot do
    from bhmm_amd import _lib
    A, pi, e0, e1 = eng._model_ptrs(*model)
    buf = np.empty((total, 8))
    for Wp, Q, flags in ((None, 2, 0), (_lib.dp(W), 0, 0), (_lib.dp(np.ones((n, n, 9))), 9, 0), (None, 0, 4)):
        with pytest.raises(ValueError):
            _lib.check(eng._L.bhmm_posterior_transitions(eng._h, A, pi, e0, e1, Wp, Q,
                                                         ctypes.c_void_p(buf.ctypes.data), flags))
    eng.close()


@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_lagged(kind, M):
    rng = np.random.default_rng(13)
    n, lag = 6, 3
    obs = _rand_obs(kind, n, M, [9000, 1000, 37, 5], rng)
    model = _rand_model(kind, n, M, rng, stay=2.0)
    W = _weights(n, 2, rng)
    views = [(k, s) for k in range(len(obs)) for s in range(lag) if len(obs[k]) > s]
    cut = [np.ascontiguousarray(obs[k][s::lag]) for k, s in views]
    eng = _engine()
    eng.set_observations_lagged(kind, obs, lag, views, n, nsymbols=M, chunk=128)
    lagged, lagged_p = eng.posterior_transitions(*model), eng.posterior_transitions(*model, weights=W)
    assert eng.get_option("pair_path") == 1
    eng.set_observations(kind, cut, n, nsymbols=M, chunk=128)
    plain, plain_p = eng.posterior_transitions(*model), eng.posterior_transitions(*model, weights=W)
    eng.close()
    assert len(lagged) == len(plain) == len(views)
    assert all(np.array_equal(a, b) for a, b in zip(lagged, plain))
    assert all(np.array_equal(a, b) for a, b in zip(lagged_p, plain_p))
    _check_jump(oracle_rows(kind, cut, model), lagged, np.float64, n, "lagged %s" % kind)


# ---- 5. consistency with what exists ----------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [2, 5, 8])
def test_row_and_column_sums_are_the_marginals(n, kind, M):
    """W_q[i][j] = (i == q): gamma_t(q); W_q[i][j] = (j == q): gamma_(t+1)(q).  Both sides carry the fp64 row
    bound: |difference| <= 2 * (1e-13 * n + 1e-8 * gamma) -- sum_ij |W_ijq| = n, (xi . |W|)_q = gamma(q)"""
    rng = np.random.default_rng(300 + n + M)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=2.0)
    Wi, Wj = np.zeros((n, n, n)), np.zeros((n, n, n))
    for q in range(n):
        Wi[q, :, q] = 1.0
        Wj[:, q, q] = 1.0
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=128)
    gam = eng.posterior_marginals(*model)
    rows_i = eng.posterior_transitions(*model, weights=Wi)
    rows_j = eng.posterior_transitions(*model, weights=Wj)
    assert eng.get_option("pair_path") == 1 and eng.get_option("marg_path") == 1
    eng.close()
    worst = 0.0
    for g, ri, rj in zip(gam, rows_i, rows_j):
        if len(g) < 2:
            assert ri.shape == rj.shape == (0, n)
            continue
        for got, want in ((ri, g[:-1]), (rj, g[1:])):
            bound = (ATOL64 * n + RTOL64 * want) + (ATOL64 + RTOL64 * want)     # pair side + marginals side
            worst = max(worst, float((np.abs(got - want) / bound).max()))
    print("n=%d %s: worst |projection - marginal| / bound %.3g" % (n, kind, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [3, 8])
def test_sum_over_time_is_the_transition_count(n, kind, M):
    """projections on unit pair matrices, eight pairs per call, summed over t, against orc.transition_counts per
    trajectory: within the per-row fp64 bounds summed over t (sum_ij |W| = 1, (xi . |W|) = xi_ij):
    1e-13 * (T - 1) + 1e-8 * C_ij"""
    rng = np.random.default_rng(500 + n + M)
    lengths = [1, 2, 37, 3001, 129]
    obs = _rand_obs(kind, n, M, lengths, rng)
    model = _rand_model(kind, n, M, rng, stay=2.0)
    A, pi, par0, par1 = model
    pairs = [(i, j) for i in range(n) for j in range(n)]
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=64)
    C = [np.zeros((n, n)) for _ in obs]
    for p0 in range(0, len(pairs), 8):
        grp = pairs[p0:p0 + 8]
        rows = eng.posterior_transitions(*model, weights=_unit_pairs(n, grp))
        assert eng.get_option("pair_path") == 1
        for k, r in enumerate(rows):
            for q, (i, j) in enumerate(grp):
                C[k][i, j] = r[:, q].sum()
    eng.close()
    worst = 0.0
    for k, o in enumerate(obs):
        pobs = orc.pobs_gaussian(o, par0, par1) if kind == "gaussian" else orc.pobs_discrete(o, par0)
        if len(o) < 2:
            assert np.all(C[k] == 0.0)
            continue
        want = orc.transition_counts(orc.forward(A, pobs, pi)[1], orc.backward(A, pobs), A, pobs)
        bound = ATOL64 * (len(o) - 1) + RTOL64 * want
        worst = max(worst, float((np.abs(C[k] - want) / bound).max()))
    print("n=%d %s: worst |sum_t xi - C| / bound %.3g" % (n, kind, worst))
    assert worst <= 1.0


# ---- 6. no side effects ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_no_side_effects(kind, M):
    rng = np.random.default_rng(9)
    n = 8
    obs = _rand_obs(kind, n, M, [30000, 7000, 1, 12345], rng)
    m1 = _rand_model(kind, n, M, rng, stay=2.0)
    m2 = _rand_model(kind, n, M, rng, stay=5.0)
    other = _rand_model(kind, n, M, rng, stay=1.0)
    W = _weights(n, 2, rng)
    opts = ("post_W", "post_ws_mb", "post_fallbacks", "post_path", "marg_W", "marg_ws_mb", "marg_fallbacks",
            "marg_path")

    def sequence(pairs):
        eng = _engine()
        eng.set_observations(kind, obs, n, nsymbols=M, chunk=256)
        eng.posterior_decode(*m1)                                   # (so that the post_* counters say something)
        eng.posterior_marginals(*m1)                                # (... and the marg_* ones)
        out = []
        for m in (m1, m2, m1):          # (carried boundaries, warm-up state: a sequence of E-steps)
            if pairs:
                eng.posterior_transitions(*other)
            r = eng.estep(*m, store_gamma=True)
            out += [r.packed.copy(), r.logL_k.copy()]
            if pairs:
                eng.posterior_transitions(*other, weights=W, dtype=np.float32)
            out += [eng.gamma(k) for k in range(len(obs))]          # the stored gamma of THAT E-step
            if pairs:
                eng.posterior_transitions(*m)
            out.append(_cat(eng.viterbi(*m)))
            out.append(eng.score([m1, m2]))
            out.append(_cat(eng.posterior_decode(*m)))
            out.append(_cat(eng.posterior_marginals(*m)))
            out.append(np.array([eng.get_option(o) for o in opts]))
        assert not pairs or eng.get_option("pair_path") == 1
        eng.close()
        return out

    plain, mixed = sequence(False), sequence(True)
    assert len(plain) == len(mixed)
    for a, b in zip(plain, mixed):
        assert np.array_equal(a, b)


# ---- 7. estimator and module function ---------------------------------------------------------------
def test_estimator_and_module_function():
    import bhmm_amd
    rng = np.random.default_rng(21)
    n = 3
    A, pi, mu, sig = _rand_model("gaussian", n, 0, rng, stay=4.0)
    hmm = bhmm_amd.gaussian_hmm(pi, A, mu, sig)
    obs = _rand_obs("gaussian", n, 0, [4000, 300, 2], rng)
    est = bhmm_amd.MaximumLikelihoodEstimator(obs, n, initial_model=hmm, output="gaussian", maxit=4, accuracy=1e-12)
    est.fit()
    Ae, pie, m0, s0 = last_model = est._estep_model
    assert not np.array_equal(Ae, est.hmm.transition_matrix)
    ref_j = oracle_rows("gaussian", obs, last_model)
    got = est.posterior_transitions()
    assert len(got) == len(obs) and got[2].shape == (1,)
    _check_jump(ref_j, got, np.float64, n, "estimator jump")
    W = _unit_pairs(n, [(0, 1), (1, 0), (2, 2)])
    proj = est.posterior_transitions(weights=W, dtype=np.float32)
    _check(oracle_rows("gaussian", obs, last_model, W), proj, np.float32, W, "estimator Q=3 float32")
    # the parameters of the last E-step, through the module function
    last = bhmm_amd.gaussian_hmm(pie, Ae, m0, s0)
    mod = bhmm_amd.posterior_transitions(obs, last)
    _check_jump(ref_j, mod, np.float64, n, "module jump")
    assert all(np.array_equal(a, b) for a, b in zip(mod, got))
    lagged = bhmm_amd.posterior_transitions(obs, last, lag=2, weights=W)
    cut = bhmm_amd.lag_observations(obs, 2)
    assert len(lagged) == len(cut)
    _check(oracle_rows("gaussian", list(cut), last_model, W), lagged, np.float64, W, "module lag 2")


# ---- 8. full size, configs[1] --------------------------------------------------------------------------
def test_full_size_configs1():
    import torch
    rng = np.random.default_rng(2)
    n, K, T = 8, 256, 100000
    model = _rand_model("gaussian", n, 0, rng, stay=3.0)
    obs = [rng.normal(0, 3, T) for _ in range(K)]
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    out = torch.empty(K * T, dtype=torch.float32, device="cuda:0")
    views = eng.posterior_transitions(*model, dtype=np.float32, out=out)
    eng.sync()
    assert eng.get_option("pair_path") == 1
    eng.close()
    assert len(views) == K and views[0].shape == (T - 1,)
    lo, hi = float(out.min()), float(out.max())
    print("configs[1]: jump probabilities in [%.3g, %.9g]" % (lo, hi))
    assert lo >= 0.0 and hi <= 1.0 + 1e-6
    assert bool((out.view(K, T)[:, -1] == 0).all())
    sel = [0, 85, K - 1]
    _check_jump(oracle_rows("gaussian", [obs[k] for k in sel], model), [views[k].cpu().numpy() for k in sel],
                np.float32, n, "configs[1]")


# ---- 9. the call's state is the context's --------------------------------------------------------------
PAIR_DEFAULTS = {"pair_fused": 1.0, "pair_W": 0.0, "pair_ws_mb": 8192.0, "pair_rows": -1.0, "pair_fallbacks": 0.0,
                 "pair_path": 0.0, "pair_rows_kernel": 0.0}


def _raw_get(L, h, door, name):
    """(status, value) of one option through bhmm_ctx_get_option or bhmm_pair_get_option"""
    v = ctypes.c_double(-12345.0)
    rc = getattr(L, door)(h, name.encode(), ctypes.byref(v))
    return rc, v.value


def _pair_options(L, h):
    out = {}
    for name in PAIR_DEFAULTS:
        by_ctx, by_pair = _raw_get(L, h, "bhmm_ctx_get_option", name), _raw_get(L, h, "bhmm_pair_get_option", name)
        assert by_ctx[0] == 0 and by_ctx == by_pair, name
        out[name] = by_ctx[1]
    return out


def test_state_dies_with_the_context():
    """options set on a context that is destroyed without bhmm_pair_release reach no later context, whichever
    address it is made at"""
    from bhmm_amd import _lib
    L = _lib.load()
    for _ in range(4):
        h = ctypes.c_void_p()
        assert L.bhmm_ctx_create(ctypes.byref(h), 0, None) == 0
        for name, value in (("pair_fused", 0.0), ("pair_W", 7.0), ("pair_rows", 0.0)):
            assert L.bhmm_ctx_set_option(h, name.encode(), value) == 0
        assert _raw_get(L, h, "bhmm_pair_get_option", "pair_W") == (0, 7.0)
        assert L.bhmm_ctx_destroy(h) == 0
    h = ctypes.c_void_p()
    assert L.bhmm_ctx_create(ctypes.byref(h), 0, None) == 0
    try:
        assert _pair_options(L, h) == PAIR_DEFAULTS
    finally:
        L.bhmm_ctx_destroy(h)


def test_options_by_both_doors():
    from bhmm_amd import _lib
    rng = np.random.default_rng(31)
    n = 3
    eng = _engine()
    eng.set_observations("gaussian", _rand_obs("gaussian", n, 0, [50], rng), n)
    L, h = eng._L, eng._h
    doors = ("bhmm_ctx", "bhmm_pair")
    values = {"pair_W": 11.0, "pair_ws_mb": 3.0, "pair_fused": 0.0, "pair_rows": 1.0}
    for setter, getter in (doors, doors[::-1]):
        for name, value in values.items():
            assert getattr(L, setter + "_set_option")(h, name.encode(), value) == 0, (setter, name)
            assert _raw_get(L, h, getter + "_get_option", name) == (0, value), (getter, name)
            assert eng.get_option(name) == value
        values = {"pair_W": 0.0, "pair_ws_mb": 0.0, "pair_fused": 1.0, "pair_rows": 0.0}   # (second round: other values)
    before = _pair_options(L, h)
    for door in doors:
        assert getattr(L, door + "_set_option")(h, b"pair_path", 1.0) == _lib.ERR_INVALID           # read-only
        assert b"unknown or read-only option" in L.bhmm_last_error()
        assert getattr(L, door + "_set_option")(h, b"pair_nonsense", 1.0) == _lib.ERR_INVALID
        assert _raw_get(L, h, door + "_get_option", "pair_nonsense")[0] == _lib.ERR_INVALID
        assert getattr(L, door + "_set_option")(h, b"pair_rows", 2.0) == _lib.ERR_INVALID           # out of range
        assert b"pair_rows is -1, 0 or 1" in L.bhmm_last_error()
        assert getattr(L, door + "_set_option")(h, b"pair_ws_mb", -1.0) == _lib.ERR_INVALID         # negative
        assert b"pair_ws_mb outside [0, 2^30]" in L.bhmm_last_error()
    # the pair doors take the names of this call alone
    assert L.bhmm_pair_set_option(h, b"post_W", 5.0) == _lib.ERR_INVALID
    assert _raw_get(L, h, "bhmm_pair_get_option", "post_W")[0] == _lib.ERR_INVALID
    assert eng.get_option("post_W") == 0
    assert _pair_options(L, h) == before
    eng.close()


def test_release_then_go_on():
    eng = _engine()

    def calls():
        out = []
        for n, opts in ((3, {"pair_W": 40, "pair_ws_mb": 1}), (12, {"pair_rows": 1})):
            r = np.random.default_rng(100 + n)
            obs = _rand_obs("gaussian", n, 0, [300, 1, 77], r)
            model, W = _rand_model("gaussian", n, 0, r, stay=2.0), _weights(n, 3, r)
            eng.set_observations("gaussian", obs, n, chunk=64)
            for name, value in opts.items():
                eng.set_option(name, value)
            out.append(_cat(eng.posterior_transitions(*model, weights=W)))
            assert eng.get_option("pair_path") == (1 if n == 3 else 0)
            assert eng.get_option("pair_rows_kernel") == (1 if n == 12 else 0)
        return out

    before = calls()
    assert _pair_options(eng._L, eng._h) != PAIR_DEFAULTS
    assert eng._L.bhmm_pair_release(eng._h) == 0
    assert _pair_options(eng._L, eng._h) == PAIR_DEFAULTS
    after = calls()
    assert eng._L.bhmm_pair_release(eng._h) == 0
    assert eng._L.bhmm_pair_release(eng._h) == 0            # (nothing left: still fine)
    eng.close()
    for a, b in zip(before, after):
        assert a.size and np.array_equal(a, b)


@pytest.mark.parametrize("rows", [0, 1])
def test_kept_copies(rows):
    """A, W and the operand matrices are uploaded only where they differ from the kept host copy: every call of a
    sequence on ONE engine gives bitwise what a fresh engine gives for that call alone"""
    rng = np.random.default_rng(33)
    n, big = 12, 20
    obs = _rand_obs("gaussian", n, 0, [40, 1, 2, 17], rng)
    obs_big = _rand_obs("gaussian", big, 0, [40, 1, 2, 17], rng)
    m1, m2 = _rand_model("gaussian", n, 0, rng, stay=2.0), _rand_model("gaussian", n, 0, rng, stay=1.0)
    m2 = (m2[0],) + m1[1:]                                   # (A2 with the rest of model 1: A alone changes)
    m3 = _rand_model("gaussian", big, 0, rng, stay=2.0)
    W1, W2, W3 = _weights(n, 4, rng), _weights(n, 4, rng), _weights(big, 4, rng)
    steps = [(obs, m1, W1), (obs, m1, W1), (obs, m1, W2), (obs, m2, W2), (obs, m2, None),
             (obs, m2, np.ascontiguousarray(W1[:, :, :2])), (obs_big, m3, W3)]

    def run(eng, o, model, W):
        if eng.nstates != len(model[1]):
            eng.set_observations("gaussian", o, len(model[1]))
        return _cat(eng.posterior_transitions(*model, weights=W))

    def fresh():
        eng = _engine()
        eng.set_option("pair_rows", rows)
        return eng

    one = fresh()
    got = [run(one, *s) for s in steps]
    assert one.get_option("pair_path") == 0 and one.get_option("pair_rows_kernel") == rows
    one.close()
    for i, s in enumerate(steps):
        eng = fresh()
        want = run(eng, *s)
        eng.close()
        assert want.size and np.array_equal(got[i], want), "step %d" % i
