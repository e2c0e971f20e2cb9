"""GPU: bhmm_path_logprob / bhmm_decode_logprob and the layers above them (Engine.path_logprob, Engine.decode_logprob,
bhmm_amd.path_logprob, MaximumLikelihoodEstimator.hidden_state_logprob, hidden.path_logprob): the joint
log-probability log p(s, O | model) of given or decoded hidden paths.

The yardstick (_terms, _ref) is written here, independent of the code under test: it forms the terms of the
definition in numpy float64 and adds each trajectory's terms with math.fsum.  The bound is
|got - ref| <= 1e-12 * (1 + sum_t |term_t|), derived, not measured: a lane adds at most pathlp_lane terms serially,
the trees add a few dozen levels, each term carries a few ulp from log, the division and the square -- together
about 1e-14 * sum |term|; the factor 100 over that is the margin.  Results that are -inf or NaN must match exactly.

The directed cases read pathlp_tile and pathlp_lane from the engine instead of assuming them."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


# ---- the yardstick --------------------------------------------------------------------------------------
def _terms(kind, o, s, model):
    """the T terms of one trajectory: log pi(s_0) + e_0, then log A(s_t-1, s_t) + e_t"""
    A, pi, p0, p1 = model
    s = np.asarray(s).astype(np.int64)
    if s.size == 0:
        return np.zeros(0)
    with np.errstate(divide="ignore"):
        lA, lpi = np.log(np.asarray(A, dtype=np.float64)), np.log(np.asarray(pi, dtype=np.float64))
        if kind == "gaussian":
            mu, sg = np.asarray(p0, dtype=np.float64)[s], np.asarray(p1, dtype=np.float64)[s]
            e = -0.5 * ((np.asarray(o, dtype=np.float64) - mu) / sg) ** 2 - np.log(sg) - LOG_SQRT_2PI
        elif kind == "discrete":
            e = np.log(np.asarray(p0, dtype=np.float64))[s, np.asarray(o).astype(np.int64)]
        else:
            e = np.log(np.asarray(o, dtype=np.float64))[np.arange(s.size), s]
    t = np.empty(s.size)
    t[0] = lpi[s[0]] + e[0]
    t[1:] = lA[s[:-1], s[1:]] + e[1:]
    return t


def _fsum(t):
    if np.isnan(t).any():
        return math.nan
    if np.isinf(t).any():
        assert not (t == np.inf).any()
        return -math.inf
    return math.fsum(t.tolist())


def _ref(kind, obs, paths, models):
    """(S, K) reference values and the (S, K) sums of |term|"""
    ref = np.zeros((len(models), len(obs)))
    mag = np.zeros_like(ref)
    for m, model in enumerate(models):
        for k, (o, s) in enumerate(zip(obs, paths)):
            t = _terms(kind, o, s, model)
            ref[m, k] = _fsum(t)
            mag[m, k] = np.abs(t[np.isfinite(t)]).sum()
    return ref, mag


def _check(got, ref, mag, label=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float64, label
    special = ~np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), label
    assert np.array_equal(got[special & ~np.isnan(ref)], ref[special & ~np.isnan(ref)]), label
    err = np.abs(got[~special] - ref[~special])
    bound = 1e-12 * (1.0 + mag[~special])
    print("%s: largest error / bound = %.3g" % (label, (err / bound).max() if err.size else 0.0))
    assert np.all(err <= bound), "%s: error %.3g over the bound %.3g" % (label, (err / bound).max(), 1.0)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# ---- helpers ---------------------------------------------------------------------------------------------
def _rand_model(kind, n, M, rng, stay=2.0):
    A = rng.random((n, n)) + 0.05
    A += stay * np.eye(n) * A.sum(axis=1)[:, None]
    A /= A.sum(axis=1)[:, None]
    pi = rng.random(n) + 0.1
    pi /= pi.sum()
    if kind == "gaussian":
        return (A, pi, np.sort(rng.normal(0, 3, n)), rng.uniform(0.5, 2.0, n))
    B = rng.random((n, M)) + 0.01
    return (A, pi, B / B.sum(axis=1)[:, None], None)


def _rand_obs(kind, M, lengths, rng):
    if kind == "gaussian":
        return [rng.normal(0, 3, int(T)) for T in lengths]
    return [rng.integers(0, M, int(T)).astype(np.int32) for T in lengths]


def _rand_paths(n, lengths, rng, dtype=np.uint8):
    return [rng.integers(0, n, int(T)).astype(dtype) for T in lengths]


def _engine(kind, obs, n, M=0):
    from bhmm_amd.engine import Engine
    eng = Engine(0)
    eng.set_observations(kind, obs, n, nsymbols=M)
    return eng


def _on_device(path):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(path)).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    return t


def _sizes():
    eng = _engine("gaussian", [np.zeros(1)], 2)
    S, L = int(eng.get_option("pathlp_tile")), int(eng.get_option("pathlp_lane"))
    eng.close()
    assert S > 0 and L > 0 and S % (64 * L) == 0 and S >= 128 * L
    return S, L


# ---- 1. boundaries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 5)])
def test_boundaries(kind, M):
    """Trajectory boundaries at the first and last step of a lane's span, of a wavefront's, of a tile's and of the
    whole path; empty trajectories between others, trajectories of one step, one that spans at least three tiles
    (here: it begins in tile 1 and ends in tile 4) and one tile with more trajectories than it has lanes."""
    S, L = _sizes()
    n, total = 3, 4 * S + 7
    lanes = S // L
    many = lanes + 44                                    # one-step trajectories in tile 1: more than its lanes
    starts = {0, 1, L - 1, L, L + 1, 64 * L - 1, 64 * L, 64 * L + 1, S - 1, S, S + 1, total - 1}
    starts |= set(range(S + 2, S + 2 + many + 1))        # ... the last of them begins the long trajectory
    starts = sorted(starts)
    assert starts[-2] == S + 2 + many and S + 2 + many < 2 * S and total < 5 * S
    lengths = np.diff(starts + [total]).tolist()
    assert max(lengths) > 2 * S + S // 2 and lengths.count(1) > lanes
    for at in (len(lengths), len(lengths) - 1, 9, 9, 4, 0, 0):    # empty ones: last, before the last, two in a row, first
        lengths.insert(at, 0)
    assert sum(lengths) == total
    rng = np.random.default_rng(17)
    obs = _rand_obs(kind, M, lengths, rng)
    models = [_rand_model(kind, n, M, rng), _rand_model(kind, n, M, rng, stay=0.0)]
    paths = _rand_paths(n, lengths, rng)
    ref, mag = _ref(kind, obs, paths, models)
    eng = _engine(kind, obs, n, M)
    got = eng.path_logprob(np.concatenate(paths), models)
    _check(got, ref, mag, "boundaries %s" % kind)
    assert np.array_equal(got[:, np.array(lengths) == 0], np.zeros((2, lengths.count(0))))
    assert np.array_equal(_bits(eng.path_logprob(paths, models)), _bits(got))     # a list per trajectory
    assert eng.get_option("pathlp_ms") > 0
    eng.close()


# ---- 2. bitwise ------------------------------------------------------------------------------------------
def test_bitwise():
    S, L = _sizes()
    n = 5
    lengths = [S + 3, 0, 2 * L + 1, 1, 2 * S - 1, 37]
    rng = np.random.default_rng(23)
    obs = _rand_obs("gaussian", 0, lengths, rng)
    models = [_rand_model("gaussian", n, 0, rng) for _ in range(3)]
    flat = np.concatenate(_rand_paths(n, lengths, rng))
    eng = _engine("gaussian", obs, n)
    first = eng.path_logprob(flat, models)
    assert np.all(np.isfinite(first))
    assert np.array_equal(_bits(eng.path_logprob(flat, models)), _bits(first))                  # a second call
    dev = _on_device(flat)
    assert np.array_equal(_bits(eng.path_logprob(dev, models)), _bits(first))                   # host = device
    assert np.array_equal(dev.cpu().numpy(), flat)                                              # read in place
    assert np.array_equal(_bits(eng.path_logprob(flat.astype(np.int32), models)), _bits(first))  # u8 = int32
    assert np.array_equal(_bits(eng.path_logprob(_on_device(flat.astype(np.int32)), models)), _bits(first))
    for m in range(3):                                                                          # alone = in a stack
        alone = eng.path_logprob(flat, [models[m]])
        assert np.array_equal(_bits(alone[0]), _bits(first[m]))
        for pos in range(3):
            stack = [models[(m + 1) % 3]] * 3
            stack[pos] = models[m]
            assert np.array_equal(_bits(eng.path_logprob(flat, stack)[pos]), _bits(first[m]))
    eng.close()


# ---- 3. state counts -------------------------------------------------------------------------------------
def test_state_counts_and_kinds():
    """1, 8, 9, 64, 129 and 256 states in bytes, 300 in int32; discrete with M = 1 and M = 64: both values of
    pathlp_table (the log-transition table in LDS / through L2) occur."""
    S, L = _sizes()
    lengths = [S + 37, 0, 5, L, S // 2 + 1]
    seen = set()
    cases = [("gaussian", n, 0, np.uint8) for n in (1, 8, 9, 64, 129, 256)] + [("gaussian", 300, 0, np.int32)]
    cases += [("discrete", 8, 1, np.uint8), ("discrete", 8, 64, np.uint8), ("discrete", 64, 64, np.uint8),
              ("discrete", 129, 64, np.uint8), ("discrete", 129, 1, np.uint8)]
    for kind, n, M, dtype in cases:
        rng = np.random.default_rng(1000 * n + M)
        obs = _rand_obs(kind, M, lengths, rng)
        models = [_rand_model(kind, n, M, rng), _rand_model(kind, n, M, rng)]
        paths = _rand_paths(n, lengths, rng, dtype)
        if n > 1:
            paths[0][[0, 7, S + 36]] = n - 1             # the highest state, at both ends of a trajectory
        ref, mag = _ref(kind, obs, paths, models)
        eng = _engine(kind, obs, n, M)
        got = eng.path_logprob(np.concatenate(paths), models)
        seen.add(int(eng.get_option("pathlp_table")))
        eng.close()
        _check(got, ref, mag, "%s n=%d M=%d" % (kind, n, M))
    assert seen == {0, 1}


def test_explicit_pobs_through_hidden():
    from bhmm_amd import hidden
    S, L = _sizes()
    n, T = 4, S + 19
    rng = np.random.default_rng(41)
    A, pi, _, _ = _rand_model("gaussian", n, 0, rng)
    pobs = rng.random((T, n)) + 1e-3
    path = rng.integers(0, n, T)
    t = _terms("explicit", pobs, path, (A, pi, None, None))
    got = hidden.path_logprob(A, pobs, pi, path)
    assert isinstance(got, float)
    _check(np.array([[got]]), np.array([[_fsum(t)]]), np.array([[np.abs(t).sum()]]), "explicit pobs")
    pobs[T // 2, path[T // 2]] = 0.0                     # a zero on the path
    assert hidden.path_logprob(A, pobs, pi, path) == -math.inf


# ---- 4. zeros and NaN ------------------------------------------------------------------------------------
@pytest.mark.parametrize("long", [False, True])
def test_zeros_and_nan(long):
    """A zero in A, in pi, in B on the path of trajectory 1 of 3: -inf there, finite in the other two; one NaN
    observation: NaN for its trajectory only.  Short trajectories share lanes of one tile, long ones span tiles."""
    S, L = _sizes()
    n, M = 3, 4
    lengths = [S + 5, 2 * S + 3, 77] if long else [40, 50, 30]
    rng = np.random.default_rng(59 + int(long))

    def run(kind, obs, paths, model, label, want):
        ref, mag = _ref(kind, obs, paths, [model])
        assert [("nan" if math.isnan(x) else "-inf" if x == -math.inf else "finite") for x in ref[0]] == want, label
        eng = _engine(kind, obs, n, M if kind == "discrete" else 0)
        got = eng.path_logprob(np.concatenate(paths), [model])
        eng.close()
        _check(got, ref, mag, label)

    # paths that never go 0 -> 1, except trajectory 1 once; none starts in state 2, except trajectory 1
    paths = []
    for k, T in enumerate(lengths):
        p = rng.integers(0, n, T).astype(np.uint8)
        p[0] = 0
        for t in range(1, T):
            if p[t - 1] == 0 and p[t] == 1:
                p[t] = 2
        paths.append(p)
    A, pi, mu, sg = _rand_model("gaussian", n, 0, rng)
    obs = _rand_obs("gaussian", 0, lengths, rng)
    A0 = A.copy()
    A0[0, 1] = 0.0
    A0 /= A0.sum(axis=1)[:, None]
    jump = [p.copy() for p in paths]
    at = lengths[1] - 7
    jump[1][at - 1:at + 1] = [0, 1]
    jump[1][at + 1] = 1
    run("gaussian", obs, jump, (A0, pi, mu, sg), "zero in A", ["finite", "-inf", "finite"])
    run("gaussian", obs, paths, (A0, pi, mu, sg), "zero in A, not on a path", ["finite"] * 3)
    pi0 = np.array([0.6, 0.4, 0.0])
    first = [p.copy() for p in paths]
    first[1][0] = 2
    run("gaussian", obs, first, (A, pi0, mu, sg), "zero in pi", ["finite", "-inf", "finite"])
    nan = [o.copy() for o in obs]
    nan[1][lengths[1] // 2] = np.nan
    run("gaussian", nan, paths, (A, pi, mu, sg), "NaN observation", ["finite", "nan", "finite"])
    # a zero in B: symbol 3 is impossible in state 1; only trajectory 1 meets the pair
    Ad, pid, B, _ = _rand_model("discrete", n, M, rng)
    B[1, 3] = 0.0
    B /= B.sum(axis=1)[:, None]
    dobs = _rand_obs("discrete", M, lengths, rng)
    for k in range(3):
        dobs[k][(paths[k] == 1) & (dobs[k] == 3)] = 0
    dobs[1][5], zb = 3, [p.copy() for p in paths]
    zb[1][5] = 1
    if zb[1][4] == 0:
        zb[1][4] = 2
    run("discrete", dobs, zb, (Ad, pid, B, None), "zero in B", ["finite", "-inf", "finite"])


# ---- 5. invalid arguments --------------------------------------------------------------------------------
def test_invalid_state_and_misaligned_pointer():
    import torch
    from bhmm_amd import _lib
    S, L = _sizes()
    n = 4
    lengths = [S + 5, 3, 2 * L]
    total = sum(lengths)
    rng = np.random.default_rng(61)
    obs = _rand_obs("gaussian", 0, lengths, rng)
    model = _rand_model("gaussian", n, 0, rng)
    paths = _rand_paths(n, lengths, rng)
    good = np.concatenate(paths)
    ref, mag = _ref("gaussian", obs, paths, [model])
    eng = _engine("gaussian", obs, n)
    A, pi, p0, p1 = (np.ascontiguousarray(x[None]) for x in model)
    out = np.full(len(lengths), 123.0)
    for where in (0, L + 1, S, total - 1):                          # a state equal to n, host and device
        bad = good.copy()
        bad[where] = n
        with pytest.raises(ValueError):
            eng.path_logprob(bad, [model])
        with pytest.raises(ValueError):
            eng.path_logprob(_on_device(bad), [model])
        rc = eng._L.bhmm_path_logprob(eng._h, ctypes.c_void_p(bad.ctypes.data), 1, 0, 1, _lib.dp(A), _lib.dp(pi),
                                      _lib.dp(p0), _lib.dp(p1), _lib.dp(out))
        assert rc == _lib.ERR_INVALID and np.all(out == 123.0)      # nothing is delivered
        _check(eng.path_logprob(good, [model]), ref, mag, "the call after a refusal")
    bad32 = good.astype(np.int32)
    bad32[7] = -1
    with pytest.raises(ValueError):
        eng.path_logprob(bad32, [model])
    shifted = torch.zeros(total + 16, dtype=torch.uint8, device="cuda:0")[1:total + 1]
    assert shifted.data_ptr() % 16 == 1 and shifted.is_contiguous()
    with pytest.raises(ValueError):
        eng.path_logprob(shifted, [model])                          # a misaligned device pointer
    rc = eng._L.bhmm_path_logprob(eng._h, ctypes.c_void_p(shifted.data_ptr()), 1, 1, 1, _lib.dp(A), _lib.dp(pi),
                                  _lib.dp(p0), _lib.dp(p1), _lib.dp(out))
    assert rc == _lib.ERR_INVALID                                   # ... refused by the C call as well
    rc = eng._L.bhmm_path_logprob(eng._h, None, 1, 0, 1, _lib.dp(A), _lib.dp(pi), _lib.dp(p0), _lib.dp(p1),
                                  _lib.dp(out))
    assert rc == _lib.ERR_INVALID
    notstoch = A.copy()
    notstoch[0, 0, 0] += 0.5                                        # validated as by bhmm_score
    rc = eng._L.bhmm_path_logprob(eng._h, ctypes.c_void_p(good.ctypes.data), 1, 0, 1, _lib.dp(notstoch), _lib.dp(pi),
                                  _lib.dp(p0), _lib.dp(p1), _lib.dp(out))
    assert rc == _lib.ERR_INVALID and np.all(out == 123.0)
    _check(eng.path_logprob(good, [model]), ref, mag, "after the refusals")
    eng.close()


# ---- 6. enumeration identity -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 4)])
def test_enumeration_identity(kind, M):
    """n = 3, T = 6, one observation sequence as K = 3^6 trajectories, trajectory k with the k-th of all paths: the
    logsumexp of the joint log-probabilities is the log-likelihood, their maximum is the Viterbi path's."""
    n, T = 3, 6
    K = n ** T
    rng = np.random.default_rng(71)
    A, pi = _rand_model("gaussian", n, 0, rng, stay=1.0)[:2]
    if kind == "gaussian":
        model = (A, pi, np.array([-1.5, 0.2, 1.8]), np.array([0.9, 0.7, 1.1]))   # no density below 1e-300
        seq = rng.normal(0, 1.5, T)
    else:
        model = (A, pi) + _rand_model("discrete", n, M, rng)[2:]
        seq = rng.integers(0, M, T).astype(np.int32)
    digits = (np.arange(K)[:, None] // n ** np.arange(T - 1, -1, -1)[None, :]) % n
    paths = [digits[k].astype(np.uint8) for k in range(K)]
    obs = [seq.copy() for _ in range(K)]
    ref, mag = _ref(kind, obs, paths, [model])
    eng = _engine(kind, obs, n, M)
    logp = eng.path_logprob(np.concatenate(paths), [model])
    _check(logp, ref, mag, "all paths, %s" % kind)
    logp = logp[0]
    score = eng.score([model])[0]
    assert np.ptp(score) <= 1e-11
    top = logp.max()
    lse = top + math.log(math.fsum(np.exp(logp - top).tolist()))
    print("logsumexp - score = %.3g" % (lse - score[0]))
    assert abs(lse - score[0]) <= 1e-11
    vit = eng.viterbi_u8(*model).reshape(K, T)
    assert np.array_equal(vit, np.repeat(vit[:1], K, axis=0))
    kstar = int((vit[0].astype(np.int64) * n ** np.arange(T - 1, -1, -1)).sum())
    assert np.array_equal(digits[kstar], vit[0])
    assert logp[kstar] == top and int(np.argmax(ref[0])) == kstar
    dec = eng.decode_logprob(*model, method="viterbi")
    _check(dec[None], np.repeat(ref[:, kstar:kstar + 1], K, axis=1), np.repeat(mag[:, kstar:kstar + 1], K, axis=1),
           "decode_logprob viterbi, %s" % kind)
    assert abs(dec[0] - top) <= 1e-12 * (1.0 + mag[0, kstar])
    eng.close()


# ---- 7. decode consistency -------------------------------------------------------------------------------
def _cycle_model(n, rng):
    """a sparse A -- state i stays or moves on to i + 1 (mod n) -- whose even states emit alike and whose odd states
    emit alike (up to a small perturbation): where in the cycle a trajectory is stays uncertain, the largest marginal
    changes between states i and i + 2, and the posterior path, decoded step by step, takes jumps the model
    forbids; the Viterbi path cannot"""
    A = np.zeros((n, n))
    for i in range(n):
        A[i, i], A[i, (i + 1) % n] = 0.9, 0.1
    pi = np.full(n, 1.0 / n)
    mu = 2.0 * (np.arange(n) % 2) + rng.normal(0, 0.05, n)
    return A, pi, mu, np.full(n, 1.0)


def _sample_cycle(model, T, rng):
    A, pi, mu, sg = model
    n = len(pi)
    move = rng.random(T) < 0.1
    s = (rng.integers(0, n) + np.cumsum(move)) % n
    return rng.normal(mu[s], sg[s])


DEC_SEED = 83   # checked on the CPU oracle (forward, backward, gamma, argmax): the posterior path of every one of the
                # four trajectories takes a forbidden jump at n = 8 and at n = 16


@pytest.mark.parametrize("n", [8, 16])
def test_decode_consistency(n):
    S, L = _sizes()
    rng = np.random.default_rng(DEC_SEED + n)
    lengths = [3 * S + 5, 3 * S - 1, 2 * S + L + 1, 3 * S + 64 * L]
    model = _cycle_model(n, rng)
    A = model[0]
    obs = [_sample_cycle(model, T, rng) for T in lengths]
    eng = _engine("gaussian", obs, n)
    score = eng.score([model])[0]
    vit = eng.viterbi_u8(*model).copy()
    post = np.concatenate(eng.posterior_decode(*model))
    smp = np.concatenate(eng.sample_paths(*model, seed=5)[0]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(lengths)])
    cut = lambda flat: [flat[off[k]:off[k + 1]] for k in range(len(lengths))]   # noqa: E731
    forbidden = np.array([bool((A[p[:-1], p[1:]] == 0).any()) for p in cut(post)])
    assert forbidden.any()                                  # (DEC_SEED)
    assert not any((A[p[:-1], p[1:]] == 0).any() for p in cut(vit))
    rv, mv = _ref("gaussian", obs, cut(vit), [model])
    rp, mp = _ref("gaussian", obs, cut(post), [model])
    rs, ms = _ref("gaussian", obs, cut(smp), [model])
    dv = eng.decode_logprob(*model, method="viterbi")
    pv = eng.path_logprob(vit, [model])[0]
    assert np.array_equal(_bits(dv), _bits(pv)) and np.all(np.isfinite(dv))
    _check(dv[None], rv, mv, "decode_logprob viterbi n=%d" % n)
    dp = eng.decode_logprob(*model, method="posterior")
    _check(dp[None], rp, mp, "decode_logprob posterior n=%d" % n)
    assert np.all(dp[forbidden] == -math.inf) and np.all(np.isfinite(dp[~forbidden]))
    assert np.array_equal(_bits(dp), _bits(eng.path_logprob(post, [model])[0]))
    ps = eng.path_logprob(smp, [model])[0]
    _check(ps[None], rs, ms, "sampled path n=%d" % n)
    bound = 1e-12 * (1.0 + mv[0])
    assert np.all(dv >= dp - bound) and np.all(dv >= ps - bound)
    for x in (dv, dp, ps):
        assert np.all(x <= score + 1e-12 * (1.0 + np.abs(score)))
    # the decoders left what they leave after decode_runs: the existing calls answer as before
    assert np.array_equal(eng.viterbi_u8(*model), vit)
    assert np.array_equal(np.concatenate(eng.posterior_decode(*model)), post)
    eng.close()


# ---- 8. lagged set, top level, estimator -------------------------------------------------------------------
def test_lagged_views_are_trajectories():
    import bhmm_amd
    from bhmm_amd.engine import Engine
    S, L = _sizes()
    n, lag = 4, 2
    rng = np.random.default_rng(97)
    base = [rng.normal(0, 3, T) for T in (2 * S + 11, 1, S - 3, 40)]
    lagged = bhmm_amd.lag_observations(base, lag)
    assert len(lagged) == 6 and lagged.views[1] == (0, 1)
    lengths = [len(o) for o in lagged]
    models = [_rand_model("gaussian", n, 0, rng) for _ in range(2)]
    paths = _rand_paths(n, lengths, rng)
    ref, mag = _ref("gaussian", list(lagged), paths, models)
    eng = Engine(0)
    eng.set_observations_lagged("gaussian", lagged.base, lag, lagged.views, n)
    _check(eng.path_logprob(np.concatenate(paths), models), ref, mag, "lagged views")
    eng.close()
    hmms = [bhmm_amd.gaussian_hmm(m[1], m[0], m[2], m[3]) for m in models]
    _check(bhmm_amd.path_logprob(base, hmms, paths=paths, lag=lag), ref, mag, "bhmm_amd.path_logprob, lag 2")
    one = bhmm_amd.path_logprob(base, hmms[0], paths=np.concatenate(paths).astype(np.int32), lag=lag)
    assert np.array_equal(_bits(one[0]), _bits(bhmm_amd.path_logprob(base, hmms, paths=paths, lag=lag)[0]))


def test_top_level_decode_and_estimator():
    import bhmm_amd
    from tests.test_path_runs_gpu import _three_state_data
    obs, (A, mu, sig) = _three_state_data(11, [400, 437, 3, 474])
    init = bhmm_amd.gaussian_hmm([0.4, 0.3, 0.3], 0.8 * A + 0.2 / 3, mu + 0.4, sig * 1.3)
    est = bhmm_amd.MaximumLikelihoodEstimator(obs, 3, initial_model=init, reversible=False, accuracy=1e-4, maxit=15)
    hmm = est.fit()
    model = (hmm.transition_matrix, hmm.initial_distribution) + tuple(hmm.output_model.parameters())
    want = {"viterbi": [np.asarray(p) for p in est.compute_viterbi_paths()], "posterior": est.posterior_decode()}
    for method in ("viterbi", "posterior"):
        ref, mag = _ref("gaussian", obs, want[method], [model])
        got = est.hidden_state_logprob(method=method)
        assert got.shape == (4,)
        _check(got[None], ref, mag, "hidden_state_logprob %s" % method)
        top = bhmm_amd.path_logprob(obs, hmm, method=method)
        assert top.shape == (4,)
        _check(top[None], ref, mag, "bhmm_amd.path_logprob %s" % method)
    with pytest.raises(ValueError):
        est.hidden_state_logprob(method="gibbs")
