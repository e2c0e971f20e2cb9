"""GPU: k_pair_tile, the matrix-core row kernel of the generic path of bhmm_posterior_transitions (option
pair_rows), against rows formed from the committed oracle alone
(tests/transitions_oracle_engine.py) and against the other two kernels: every column-tile count and its edges,
trajectory ends anywhere in a tile, partial and single tiles, states the model never enters, explicit pobs, and the
bitwise properties (repeatable, float = rounded double, the cached matrices follow A, W, Q and the form).

Tolerances: those of tests/test_transitions_gpu.py, unchanged --
    1e-13 * sum_ij |W_ijq| + 1e-8 * (xi_t . |W|)_q            (fp64)
    1e-7 * sum_ij |W_ijq|                                     (fp32);
the jump form is the projection on the off-diagonal mask."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.transitions_oracle_engine import jump_mask, oracle_rows

pytestmark = pytest.mark.gpu

RTOL64, ATOL64 = 1e-8, 1e-13
TOL32 = 1e-7
LENGTHS = [1, 2, 15, 16, 17, 1, 31, 33, 300, 1, 1, 47]      # total 465: ends inside tiles, several in one tile


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


def _as2d(r):
    r = np.asarray(r)
    return r[:, None] if r.ndim == 1 else r


def _check(refs, rows, dtype, W, label=""):
    """every row against refs (what oracle_rows returned for W) under the module's tolerances"""
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
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        worst_ratio = max(worst_ratio, float(ratio.max()))
    print("%s: worst |row - oracle| / scale %.3g, worst error / bound %.3g" % (label, worst_abs, worst_ratio))
    assert worst_ratio <= 1.0, label


def _check_jump(refs, rows, dtype, n, label):
    assert all(np.asarray(r).ndim == 1 for r in rows), label
    _check(refs, [_as2d(r) for r in rows], dtype, jump_mask(n), label)


def _cat(xs):
    return np.concatenate([np.asarray(x) for x in xs])


# ---- 1. selection ----------------------------------------------------------------------------------------
def test_selection():
    rng = np.random.default_rng(1)
    eng = _engine()
    assert eng.get_option("pair_rows") == -1
    eng.set_option("pair_rows", 1)
    assert eng.get_option("pair_rows") == 1
    with pytest.raises(ValueError):
        eng.set_option("pair_rows", 2)
    with pytest.raises(ValueError):
        eng.set_option("pair_rows_kernel", 1)            # read-only
    n = 12
    obs = _rand_obs("gaussian", n, 0, [40, 7], rng)
    model = _rand_model("gaussian", n, 0, rng)
    eng.set_observations("gaussian", obs, n)
    ref = oracle_rows("gaussian", obs, model)
    rows = eng.posterior_transitions(*model)
    assert eng.get_option("pair_rows_kernel") == 1 and eng.get_option("pair_path") == 0
    _check_jump(ref, rows, np.float64, n, "selection pair_rows 1")
    eng.set_option("pair_rows", 0)
    assert eng.get_option("pair_rows") == 0
    rows = eng.posterior_transitions(*model)
    assert eng.get_option("pair_rows_kernel") == 0 and eng.get_option("pair_path") == 0
    _check_jump(ref, rows, np.float64, n, "selection pair_rows 0")
    eng.close()
    # more than 128 states: k_pair_rows whatever the option says
    n = 130
    obs = _rand_obs("gaussian", n, 0, [40, 7], rng)
    model = _rand_model("gaussian", n, 0, rng)
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    eng.set_option("pair_rows", 1)
    rows = eng.posterior_transitions(*model)
    assert eng.get_option("pair_rows_kernel") == 0 and eng.get_option("pair_path") == 0
    eng.close()
    _check_jump(oracle_rows("gaussian", obs, model), rows, np.float64, n, "selection 130 states")


# ---- 2. oracle parity, every column-tile count and its edges ------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
@pytest.mark.parametrize("n", [9, 16, 17, 32, 33, 48, 64, 65, 96, 100, 128])
def test_parity(n, kind, M):
    rng = np.random.default_rng(11 * n + M)
    obs = _rand_obs(kind, n, M, LENGTHS, rng)
    model = _rand_model(kind, n, M, rng)
    W3, W8 = _weights(n, 3, rng), _weights(n, 8, rng)
    ref_j = oracle_rows(kind, obs, model)
    ref_3, ref_8 = oracle_rows(kind, obs, model, W3), oracle_rows(kind, obs, model, W8)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M)
    eng.set_option("pair_rows", 1)
    got = []
    for dtype in (np.float64, np.float32):
        name = "tile n=%d %s %s" % (n, kind, np.dtype(dtype).name)
        got.append((ref_j, eng.posterior_transitions(*model, dtype=dtype), dtype, None, name + " jump"))
        assert eng.get_option("pair_rows_kernel") == 1 and eng.get_option("pair_path") == 0
        got.append((ref_3, eng.posterior_transitions(*model, weights=W3, dtype=dtype), dtype, W3, name + " Q=3"))
        got.append((ref_8, eng.posterior_transitions(*model, weights=W8, dtype=dtype), dtype, W8, name + " Q=8"))
        assert eng.get_option("pair_rows_kernel") == 1
    eng.close()
    for ref, rows, dtype, W, label in got:
        assert [len(r) for r in rows] == [T - 1 for T in LENGTHS]
        if W is None:
            _check_jump(ref, rows, dtype, n, label)
        else:
            _check(ref, rows, dtype, W, label)


# ---- 3. tile edges of the whole array --------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [[1], [2], [3, 1], [16], [15, 1], [17, 15], [16, 16, 16]])
def test_tile_edges(lengths):
    import torch
    rng = np.random.default_rng(170 + sum(lengths))
    n = 17
    obs = _rand_obs("gaussian", n, 0, lengths, rng)
    model = _rand_model("gaussian", n, 0, rng)
    W = _weights(n, 3, rng)
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    eng.set_option("pair_rows", 1)
    total = int(eng.offsets[-1])
    off = np.asarray(eng.offsets)
    assert total == sum(lengths)
    tj = torch.full((total,), -1.0, dtype=torch.float64, device="cuda:0")
    eng.posterior_transitions(*model, out=tj)
    tp = torch.full((total, 3), -1.0, dtype=torch.float32, device="cuda:0")
    eng.posterior_transitions(*model, weights=W, dtype=np.float32, out=tp)
    eng.sync()
    assert eng.get_option("pair_rows_kernel") == 1
    eng.close()
    dj, dp = tj.cpu().numpy(), tp.cpu().numpy()
    # the last row of every trajectory: exactly zero (the buffers were filled with -1)
    assert np.array_equal(dj[off[1:] - 1], np.zeros(len(lengths)))
    assert np.array_equal(dp[off[1:] - 1], np.zeros((len(lengths), 3), dtype=np.float32))
    label = "edges %s" % (lengths,)
    _check_jump(oracle_rows("gaussian", obs, model), [dj[off[k]:off[k + 1] - 1] for k in range(len(lengths))],
                np.float64, n, label + " jump")
    _check(oracle_rows("gaussian", obs, model, W), [dp[off[k]:off[k + 1] - 1] for k in range(len(lengths))],
           np.float32, W, label + " Q=3 float32")


# ---- 4. states the model never enters ---------------------------------------------------------------------------
def unentered_model(rng):
    """17 states, gaussian: column 5 of A zero with pi_5 = 0 (never entered), state 3 absorbing"""
    n = 17
    A, pi, mu, sig = _rand_model("gaussian", n, 0, rng)
    A[:, 5] = 0.0
    A[3, :] = 0.0
    A[3, 3] = 1.0
    A /= A.sum(axis=1)[:, None]
    pi[5] = 0.0
    pi /= pi.sum()
    return A, pi, mu, sig


def test_states_never_entered():
    rng = np.random.default_rng(4)
    n = 17
    lengths = [1, 2, 15, 16, 17, 33, 300]
    model = unentered_model(rng)
    obs = _rand_obs("gaussian", n, 0, lengths, rng)
    W = _weights(n, 3, rng)
    ref_j, ref_p = oracle_rows("gaussian", obs, model), oracle_rows("gaussian", obs, model, W)
    assert all(np.all(np.isfinite(r)) for r, _ in ref_j + ref_p)
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    eng.set_option("pair_rows", 1)
    for dtype in (np.float64, np.float32):
        rows = eng.posterior_transitions(*model, dtype=dtype)
        assert eng.get_option("pair_rows_kernel") == 1
        assert all(np.all(np.isfinite(r)) for r in rows)
        _check_jump(ref_j, rows, dtype, n, "unentered %s jump" % np.dtype(dtype).name)
        rows = eng.posterior_transitions(*model, weights=W, dtype=dtype)
        assert all(np.all(np.isfinite(r)) for r in rows)
        _check(ref_p, rows, dtype, W, "unentered %s Q=3" % np.dtype(dtype).name)
    eng.close()


# ---- 5. against the other kernels --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 64)])
def test_against_rows_and_fused_at_8_states(kind, M):
    rng = np.random.default_rng(88 + M)
    n = 8
    lengths = [1, 2, 37, 500, 3001, 64, 129]
    obs = _rand_obs(kind, n, M, lengths, rng)
    model = _rand_model(kind, n, M, rng, stay=2.0)
    W = _weights(n, 3, rng)
    eng = _engine()
    eng.set_observations(kind, obs, n, nsymbols=M, chunk=64)
    fj, fp = eng.posterior_transitions(*model), eng.posterior_transitions(*model, weights=W)
    assert eng.get_option("pair_path") == 1
    eng.set_option("pair_fused", 0)
    eng.set_option("pair_rows", 0)
    rj, rp = eng.posterior_transitions(*model), eng.posterior_transitions(*model, weights=W)
    assert eng.get_option("pair_path") == 0 and eng.get_option("pair_rows_kernel") == 0
    eng.set_option("pair_rows", 1)
    tj, tp = eng.posterior_transitions(*model), eng.posterior_transitions(*model, weights=W)
    assert eng.get_option("pair_path") == 0 and eng.get_option("pair_rows_kernel") == 1
    eng.close()
    ref_j, ref_p = oracle_rows(kind, obs, model), oracle_rows(kind, obs, model, W)
    _check_jump(ref_j, tj, np.float64, n, "tile at 8 states %s jump" % kind)
    _check(ref_p, tp, np.float64, W, "tile at 8 states %s Q=3" % kind)
    mask = jump_mask(n)
    for other, oj, op in (("k_pair_rows", rj, rp), ("fused", fj, fp)):
        _check([(_as2d(f), ra) for f, (_, ra) in zip(oj, ref_j)], [_as2d(g) for g in tj], np.float64, mask,
               "tile against %s %s jump" % (other, kind))
        _check([(f, ra) for f, (_, ra) in zip(op, ref_p)], tp, np.float64, W,
               "tile against %s %s Q=3" % (other, kind))


def test_against_rows_at_40_states():
    rng = np.random.default_rng(40)
    n = 40
    obs = _rand_obs("gaussian", n, 0, LENGTHS, rng)
    model = _rand_model("gaussian", n, 0, rng)
    W = _weights(n, 3, rng)
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    eng.set_option("pair_rows", 0)
    rj, rp = eng.posterior_transitions(*model), eng.posterior_transitions(*model, weights=W)
    assert eng.get_option("pair_rows_kernel") == 0
    eng.set_option("pair_rows", 1)
    tj, tp = eng.posterior_transitions(*model), eng.posterior_transitions(*model, weights=W)
    assert eng.get_option("pair_rows_kernel") == 1
    eng.close()
    ref_j, ref_p = oracle_rows("gaussian", obs, model), oracle_rows("gaussian", obs, model, W)
    _check([(_as2d(f), ra) for f, (_, ra) in zip(rj, ref_j)], [_as2d(g) for g in tj], np.float64, jump_mask(n),
           "tile against k_pair_rows n=40 jump")
    _check([(f, ra) for f, (_, ra) in zip(rp, ref_p)], tp, np.float64, W, "tile against k_pair_rows n=40 Q=3")


# ---- 6. explicit pobs -------------------------------------------------------------------------------------------
def test_explicit_pobs():
    rng = np.random.default_rng(62)
    n = 12
    A, pi, mu, sig = _rand_model("gaussian", n, 0, rng)
    pobs = orc.pobs_gaussian(rng.normal(0, 3, 5000), mu, sig)
    W = _weights(n, 2, rng)
    model = (A, pi, None, None)
    eng = _engine()
    eng.set_observations("explicit", [pobs], n)
    eng.set_option("pair_rows", 1)
    got = []
    for dtype in (np.float64, np.float32):
        got.append((eng.posterior_transitions(A, pi, dtype=dtype),
                    eng.posterior_transitions(A, pi, weights=W, dtype=dtype), dtype))
        assert eng.get_option("pair_rows_kernel") == 1 and eng.get_option("pair_path") == 0
    eng.close()
    ref_j, ref_p = oracle_rows("explicit", [pobs], model), oracle_rows("explicit", [pobs], model, W)
    for rj, rp, dtype in got:
        _check_jump(ref_j, rj, dtype, n, "explicit tile %s jump" % np.dtype(dtype).name)
        _check(ref_p, rp, dtype, W, "explicit tile %s Q=2" % np.dtype(dtype).name)


# ---- 7. bitwise properties ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [20, 70])
def test_bitwise(n):
    import torch
    rng = np.random.default_rng(700 + n)
    obs = _rand_obs("gaussian", n, 0, LENGTHS, rng)
    model = _rand_model("gaussian", n, 0, rng)
    W1, W2 = _weights(n, 3, rng), _weights(n, 3, rng)
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    eng.set_option("pair_rows", 1)
    total = int(eng.offsets[-1])
    j64 = _cat(eng.posterior_transitions(*model))
    p64 = _cat(eng.posterior_transitions(*model, weights=W1))
    assert np.array_equal(_cat(eng.posterior_transitions(*model)), j64)                      # repeated calls
    assert np.array_equal(_cat(eng.posterior_transitions(*model, weights=W1)), p64)
    assert np.array_equal(_cat(eng.posterior_transitions(*model, weights=W1)), p64)
    # float is the rounded double
    j32 = _cat(eng.posterior_transitions(*model, dtype=np.float32))
    p32 = _cat(eng.posterior_transitions(*model, weights=W1, dtype=np.float32))
    assert j32.dtype == np.float32 and np.array_equal(j32, j64.astype(np.float32))
    assert np.array_equal(p32, p64.astype(np.float32))
    # the cached matrices follow the weights ...
    q64 = _cat(eng.posterior_transitions(*model, weights=W2))
    assert not np.array_equal(q64[:, 2], p64[:, 2])
    assert np.array_equal(_cat(eng.posterior_transitions(*model, weights=W1)), p64)
    # ... the form ...
    assert np.array_equal(_cat(eng.posterior_transitions(*model)), j64)
    assert np.array_equal(_cat(eng.posterior_transitions(*model, weights=W1)), p64)
    assert np.array_equal(_cat(eng.posterior_transitions(*model)), j64)
    # ... and the transition matrix
    other = (_rand_A(n, rng),) + tuple(model[1:])
    o64 = _cat(eng.posterior_transitions(*other))
    assert not np.array_equal(o64, j64)
    assert np.array_equal(_cat(eng.posterior_transitions(*model)), j64)
    # a device buffer holds what the host result holds, the zero rows besides
    off = np.asarray(eng.offsets)
    keep = np.ones(total, dtype=bool)
    keep[off[1:] - 1] = False
    t = torch.full((total, 3), -1.0, dtype=torch.float64, device="cuda:0")
    eng.posterior_transitions(*model, weights=W1, out=t)
    eng.sync()
    assert eng.get_option("pair_rows_kernel") == 1
    eng.close()
    dev = t.cpu().numpy()
    assert np.array_equal(dev[keep], p64) and np.all(dev[~keep] == 0.0)


# ---- 8. row sums ---------------------------------------------------------------------------------------------------
def test_column_sums_are_the_marginals():
    """W_q[i][j] = (j == q): gamma_(t+1)(q).  Both sides carry the fp64 row bound, as in
    test_transitions_gpu.py::test_row_and_column_sums_are_the_marginals:
    |difference| <= (1e-13 * n + 1e-8 * gamma) + (1e-13 + 1e-8 * gamma)"""
    rng = np.random.default_rng(320)
    n = 20
    obs = _rand_obs("gaussian", n, 0, LENGTHS, rng)
    model = _rand_model("gaussian", n, 0, rng, stay=2.0)
    qs = [0, 1, 5, 9, 15, 16, 18, 19]
    Wj = np.zeros((n, n, 8))
    for k, q in enumerate(qs):
        Wj[:, q, k] = 1.0
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    eng.set_option("pair_rows", 1)
    gam = eng.posterior_marginals(*model)
    rows = eng.posterior_transitions(*model, weights=Wj)
    assert eng.get_option("pair_rows_kernel") == 1
    eng.close()
    worst = 0.0
    for g, r in zip(gam, rows):
        if len(g) < 2:
            assert r.shape == (0, 8)
            continue
        want = g[1:][:, qs]
        bound = (ATOL64 * n + RTOL64 * want) + (ATOL64 + RTOL64 * want)     # pair side + marginals side
        worst = max(worst, float((np.abs(r - want) / bound).max()))
    print("n=%d: worst |projection - marginal| / bound %.3g" % (n, worst))
    assert worst <= 1.0
