"""GPU: bhmm_path_runs / bhmm_decode_runs / bhmm_runs_fetch and the layers above them (Engine.path_runs,
Engine.decode_runs, bhmm_amd.decode_segments, MaximumLikelihoodEstimator.hidden_state_segments): the dwell segments
(runs) of a path and their statistics against a numpy run-length encoder written here (_rle), independent of the
code under test.  All of it is integer work: every comparison is array_equal.

The directed cases put a change of state or a trajectory start at every flat position where the kernels change
what they do -- the first and last step of a lane's span, of a wave's, of a tile's, of the path -- and read the tile
and lane sizes from the engine (options runs_tile, runs_lane) instead of assuming them."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---- the yardstick --------------------------------------------------------------------------------------
def _rle(path, lengths, n):
    """(run_off, start, length, state, dwell, jumps) of a flat path cut at the trajectory lengths"""
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    run_off, S, L, Q = [0], [], [], []
    dwell, jumps = np.zeros((n, 5), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    for k in range(len(lengths)):
        p = np.asarray(path[off[k]:off[k + 1]]).astype(np.int64)
        if p.size:
            s = np.concatenate([[0], np.flatnonzero(np.diff(p)) + 1])
            ln = np.diff(np.concatenate([s, [p.size]]))
            q = p[s]
            cens = np.zeros(s.size, dtype=bool)
            cens[0] = cens[-1] = True
            np.add.at(dwell[:, 0], q, 1)
            np.add.at(dwell[:, 1], q, ln)
            np.maximum.at(dwell[:, 2], q, ln)
            np.add.at(dwell[:, 3], q[cens], 1)
            np.add.at(dwell[:, 4], q[cens], ln[cens])
            np.add.at(jumps, (q[:-1], q[1:]), 1)
            S.append(s), L.append(ln), Q.append(q)
        run_off.append(run_off[-1] + (s.size if p.size else 0))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)  # noqa: E731
    return np.array(run_off, dtype=np.int64), cat(S, np.int64), cat(L, np.int64), cat(Q, np.int32), dwell, jumps


def _same(res, ref, stats=True, label=""):
    off, s, ln, q, dwell, jumps = ref
    assert res.offsets.dtype == np.int64 and res.start.dtype == np.int64
    assert res.length.dtype == np.int64 and res.state.dtype == np.int32
    assert np.array_equal(res.offsets, off), label
    assert np.array_equal(res.start, s), label
    assert np.array_equal(res.length, ln), label
    assert np.array_equal(res.state, q), label
    if stats:
        assert res.dwell.dtype == np.int64 and res.jumps.dtype == np.int64
        assert np.array_equal(res.dwell, dwell), label
        assert np.array_equal(res.jumps, jumps), label
        assert not np.diag(res.jumps).any()
    else:
        assert res.dwell is None and res.jumps is None
    for k in range(len(off) - 1):        # trajectory(k): the three views of one trajectory
        a, b = off[k], off[k + 1]
        ts, tl, tq = res.trajectory(k)
        assert np.array_equal(ts, s[a:b]) and np.array_equal(tl, ln[a:b]) and np.array_equal(tq, q[a:b])


def _engine(lengths, n):
    """an engine whose offsets are those of `lengths` (dummy observations)"""
    from bhmm_amd.engine import Engine
    eng = Engine(0)
    eng.set_observations("gaussian", [np.zeros(int(T)) for T in lengths], n)
    return eng


def _on_device(path):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(path)).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    return t


def _both_ways(eng, path, lengths, n, label=""):
    """the same path from the host and as a device tensor, with and without statistics"""
    ref = _rle(path, lengths, n)
    _same(eng.path_runs(path, stats=True), ref, True, label + " host")
    assert eng.get_option("runs_count") == ref[0][-1]
    dev = _on_device(path)
    _same(eng.path_runs(dev, stats=True), ref, True, label + " device")
    _same(eng.path_runs(dev), ref, False, label + " device, no statistics")
    assert np.array_equal(dev.cpu().numpy(), path)         # read in place, not written
    for got, want in zip(eng.runs_fetch(), ref[1:4]):
        assert np.array_equal(got, want)
    assert eng.get_option("runs_ms") > 0
    return ref


def _path_with_changes(total, changes, n, dtype=np.uint8):
    """a flat path whose state changes exactly at the flat positions `changes` (> 0)"""
    step = np.zeros(total, dtype=np.int64)
    step[[c for c in changes if 0 < c < total]] = 1
    return (np.cumsum(step) % n).astype(dtype)


def _sizes():
    eng = _engine([1], 2)
    S, L = int(eng.get_option("runs_tile")), int(eng.get_option("runs_lane"))
    eng.close()
    assert S > 0 and L > 0 and S % L == 0 and S >= 64 * L + 2
    return S, L


# ---- 1. directed edges ----------------------------------------------------------------------------------
def _edge_positions(S, L, total):
    return sorted({0, 1, L - 1, L, L + 1, 64 * L - 1, 64 * L, 64 * L + 1, S - 1, S, S + 1, 2 * S - 1, 2 * S,
                   total - 1})


@pytest.mark.parametrize("mode", ["changes", "starts", "starts_equal", "mixed"])
@pytest.mark.parametrize("extra", [0, 1, 15])
def test_directed_edges(extra, mode):
    S, L = _sizes()
    total = 3 * S + extra
    assert total % 16 == extra
    pos = _edge_positions(S, L, total)
    n = 5
    if mode == "changes":               # one trajectory, a change of state at every position
        lengths, changes = [total], pos
    elif mode in ("starts", "starts_equal"):   # a trajectory starts at every position
        lengths, changes = np.diff(pos + [total]).tolist(), []
        if mode == "starts":            # ... and the state changes there as well
            changes = pos
    else:                               # starts at every other position, changes at the rest and inside the lanes
        starts = pos[::2]
        lengths = np.diff(starts + [total]).tolist()
        changes = pos[1::2] + [p + 3 for p in pos if p + 3 < total]
    assert sum(lengths) == total and min(lengths) >= 1
    path = _path_with_changes(total, changes, n)
    eng = _engine(lengths, n)
    ref = _both_ways(eng, path, lengths, n, "edges %s total=%d" % (mode, total))
    eng.close()
    if mode == "starts_equal":          # equal states on both sides of every bound: still one run per trajectory
        assert not path.any() and ref[0][-1] == len(lengths)


@pytest.mark.parametrize("K", [1, 2])
def test_run_over_two_whole_tiles(K):
    """A run that begins in tile 0 and ends in tile 3: tiles 1 and 2 hold no change at all."""
    S, L = _sizes()
    total = 4 * S + 1
    changes = [5, S - 1, 3 * S + 1, total - 1]
    lengths = [total] if K == 1 else [3 * S + 1, S]       # K = 2: the long run ends at a trajectory bound
    path = _path_with_changes(total, changes if K == 1 else changes[:2] + changes[3:], 3)
    eng = _engine(lengths, 3)
    ref = _both_ways(eng, path, lengths, 3, "long run K=%d" % K)
    eng.close()
    assert ref[2].max() == 2 * S + 2


# ---- 2. degenerate sets ----------------------------------------------------------------------------------
def test_single_step():
    eng = _engine([1], 4)
    ref = _both_ways(eng, np.array([3], dtype=np.uint8), [1], 4, "K=1 T=1")
    eng.close()
    assert ref[0].tolist() == [0, 1] and ref[4][3].tolist() == [1, 1, 1, 1, 1]


def test_all_trajectories_of_length_one():
    S, L = _sizes()
    K = S + 37                          # more trajectory starts than one tile has steps
    rng = np.random.default_rng(5)
    path = rng.integers(0, 6, K).astype(np.uint8)
    eng = _engine([1] * K, 6)
    ref = _both_ways(eng, path, [1] * K, 6, "all T=1")
    eng.close()
    assert ref[0][-1] == K and not ref[5].any()


def test_empty_trajectories():
    S, L = _sizes()
    lengths = [0, 0, 7, L, 0, 0, S - L - 7, 1, 0, 2 * S + 3, 0]   # first, last, two in a row in the middle
    total = sum(lengths)
    rng = np.random.default_rng(6)
    path = _path_with_changes(total, rng.choice(total, 200, replace=False).tolist(), 4)
    eng = _engine(lengths, 4)
    ref = _both_ways(eng, path, lengths, 4, "empty trajectories")
    eng.close()
    off = ref[0]
    for k, T in enumerate(lengths):
        assert (off[k + 1] == off[k]) == (T == 0)


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_change_at_every_step_and_constant(dtype):
    S, L = _sizes()
    lengths = [S + 3, 0, 2 * L + 1, S - 1]
    total = sum(lengths)
    eng = _engine(lengths, 3)
    every = (np.arange(total) % 3).astype(dtype)
    ref = _both_ways(eng, every, lengths, 3, "change at every step")
    assert ref[0][-1] == total and (ref[2] == 1).all()
    const = np.full(total, 2, dtype=dtype)
    ref = _both_ways(eng, const, lengths, 3, "constant")
    eng.close()
    assert ref[0][-1] == 3              # the non-empty trajectories: equal states across a bound are two runs
    assert ref[2].tolist() == [S + 3, 2 * L + 1, S - 1]


# ---- 3. random -------------------------------------------------------------------------------------------
def _random_path(total, n, p, rng, dtype):
    jump = rng.random(total) < p
    delta = np.where(jump, rng.integers(1, n, total), 0) if n > 1 else np.zeros(total, dtype=np.int64)
    return ((rng.integers(0, n) + np.cumsum(delta)) % n).astype(dtype)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("p", [0.001, 0.05, 0.5])
@pytest.mark.parametrize("dtype,n,Kmax", [(np.uint8, 2, 40), (np.uint8, 8, 40), (np.uint8, 200, 6),
                                          (np.int32, 300, 6)])
def test_random(dtype, n, Kmax, p, seed):
    S, L = _sizes()
    rng = np.random.default_rng(1000 * seed + n + int(1000 * p))
    K = int(rng.integers(1, Kmax + 1))
    lengths = rng.integers(1, 2 * S + 1, K).tolist()
    total = sum(lengths)
    path = _random_path(total, n, p, rng, dtype)
    if n > 256 and total > 3:
        path[[0, total // 2, total - 1]] = [n - 1, 256, n - 1]      # states above 255
    eng = _engine(lengths, n)
    _both_ways(eng, path, lengths, n, "random n=%d p=%g seed=%d K=%d" % (n, p, seed, K))
    eng.close()


# ---- 4. validation ---------------------------------------------------------------------------------------
def test_validation_and_recovery():
    import torch
    from bhmm_amd import _lib
    S, L = _sizes()
    n = 4
    lengths = [S + 5, 3, 2 * L]
    total = sum(lengths)
    eng = _engine(lengths, n)
    good = _path_with_changes(total, [1, L, S, S + 4, total - 1], n)
    with pytest.raises((_lib.BhmmAmdError, ValueError)):
        eng.runs_fetch()                                            # before any runs call
    assert eng._L.bhmm_runs_fetch(eng._h, None, None, None) == _lib.ERR_INVALID
    for where in (0, L + 1, S, total - 1):                          # a state equal to n, host and device
        bad = good.copy()
        bad[where] = n
        with pytest.raises((_lib.BhmmAmdError, ValueError)):
            eng.path_runs(bad, stats=True)
        with pytest.raises((_lib.BhmmAmdError, ValueError)):
            eng.path_runs(_on_device(bad), stats=True)
        with pytest.raises((_lib.BhmmAmdError, ValueError)):
            eng.runs_fetch()                                        # no run is delivered
    bad32 = good.astype(np.int32)
    bad32[7] = -1
    with pytest.raises((_lib.BhmmAmdError, ValueError)):
        eng.path_runs(bad32)
    for size in (total - 1, total + 1):                             # a wrong-size path
        with pytest.raises((_lib.BhmmAmdError, ValueError)):
            eng.path_runs(np.zeros(size, dtype=np.uint8))
        with pytest.raises((_lib.BhmmAmdError, ValueError)):
            eng.path_runs(torch.zeros(size, dtype=torch.uint8, device="cuda:0"))
    shifted = torch.zeros(total + 16, dtype=torch.uint8, device="cuda:0")[1:total + 1]
    assert shifted.data_ptr() % 16 == 1 and shifted.is_contiguous()
    with pytest.raises((_lib.BhmmAmdError, ValueError)):
        eng.path_runs(shifted)                                      # a misaligned device pointer
    off = np.empty(len(lengths) + 1, dtype=np.int64)               # ... refused by the C call as well
    assert eng._L.bhmm_path_runs(eng._h, ctypes.c_void_p(shifted.data_ptr()), 1, 1, _lib.lp(off), None,
                                 None) == _lib.ERR_INVALID
    assert eng._L.bhmm_path_runs(eng._h, None, 1, 1, _lib.lp(off), None, None) == _lib.ERR_INVALID
    assert eng._L.bhmm_path_runs(eng._h, ctypes.c_void_p(good.ctypes.data), 1, 0, None, None,
                                 None) == _lib.ERR_INVALID
    # the engine still works: a valid call right after returns the right runs
    _both_ways(eng, good, lengths, n, "after the refusals")
    # new observations discard the runs
    eng.set_observations("gaussian", [np.zeros(9)], n)
    with pytest.raises((_lib.BhmmAmdError, ValueError)):
        eng.runs_fetch()
    eng.close()


# ---- 5. decoders -----------------------------------------------------------------------------------------
def _rand_model(kind, n, M, rng, stay):
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
        return [rng.normal(0, 3, T) for T in lengths]
    return [rng.integers(0, M, T).astype(np.int32) for T in lengths]


DEC_LENGTHS = [1, 2, 700, 3001, 4500]


@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 12)])
@pytest.mark.parametrize("n", [3, 12, 70])
def test_decoders(n, kind, M):
    from bhmm_amd.engine import Engine
    rng = np.random.default_rng(31 * n + M)
    obs = _rand_obs(kind, M, DEC_LENGTHS, rng)
    model = _rand_model(kind, n, M, rng, stay=8.0)

    def fresh():
        eng = Engine(0)
        eng.set_observations(kind, obs, n, nsymbols=M, chunk=64)
        if n <= 8:                      # the chunked path, more than one chunk per trajectory
            assert eng.num_chunks > len(DEC_LENGTHS) and eng.chunk_len <= 64
        return eng

    def follow(eng):
        """what the existing calls return on this engine now"""
        v = eng.viterbi_u8(*model).copy()
        p = np.concatenate(eng.posterior_decode(*model))
        e = eng.estep(*model)
        return v, p, e.packed.copy(), e.logL_k.copy()

    eng = fresh()
    plain = follow(eng)                 # the same calls on an engine that never compacted a path
    eng.close()
    assert plain[0].dtype == np.uint8 and plain[1].dtype == np.uint8
    for method, which in (("viterbi", 0), ("posterior", 1)):
        eng = fresh()
        res = eng.decode_runs(*model, method=method, stats=True)
        R = eng.get_option("runs_count")
        after = follow(eng)
        _same(res, _rle(after[which], DEC_LENGTHS, n), True, "decode_runs %s n=%d %s" % (method, n, kind))
        assert R == res.count and res.count == len(res.start)
        assert int(res.length.sum()) == sum(DEC_LENGTHS)
        # and without statistics, after the other calls
        _same(eng.decode_runs(*model, method=method), _rle(after[which], DEC_LENGTHS, n), False)
        eng.close()
        for a, b in zip(after, plain):  # calling it changed nothing of what the existing calls return
            assert np.array_equal(a, b), "%s n=%d %s" % (method, n, kind)


def test_decode_runs_refuses_more_than_256_states():
    from bhmm_amd import _lib
    n = 300
    rng = np.random.default_rng(3)
    A, pi, mu, sig = _rand_model("gaussian", n, 0, rng, stay=0.0)
    obs = [rng.normal(0, 3, 50)]
    from bhmm_amd.engine import Engine
    eng = Engine(0)
    eng.set_observations("gaussian", obs, n)
    with pytest.raises(ValueError):
        eng.decode_runs(A, pi, mu, sig)
    Ap, pip, e0, e1 = eng._model_ptrs(A, pi, mu, sig)
    off = np.empty(2, dtype=np.int64)
    for method in (0, 1):
        assert eng._L.bhmm_decode_runs(eng._h, Ap, pip, e0, e1, method, _lib.lp(off), None,
                                       None) == _lib.ERR_INVALID
    # ... decode with the existing call and hand over the int32 path
    path = np.concatenate(eng.viterbi(A, pi, mu, sig))
    assert path.dtype == np.int32
    _same(eng.path_runs(path, stats=True), _rle(path, [50], n), True, "int32 Viterbi path, n=300")
    eng.close()


# ---- 6. estimator and top level --------------------------------------------------------------------------
def _three_state_data(seed, lengths):
    rng = np.random.default_rng(seed)
    A = np.array([[0.95, 0.05, 0.0], [0.03, 0.9, 0.07], [0.0, 0.1, 0.9]])
    mu, sig = np.array([-2.0, 0.5, 3.0]), np.array([0.6, 0.5, 0.9])
    obs = []
    for T in lengths:
        s = np.zeros(T, dtype=int)
        for t in range(1, T):
            s[t] = rng.choice(3, p=A[s[t - 1]])
        obs.append(rng.normal(mu[s], sig[s]))
    return obs, (A, mu, sig)


@pytest.mark.parametrize("lag", [1, 2])
def test_estimator_and_top_level(lag):
    import bhmm_amd
    obs, (A, mu, sig) = _three_state_data(11, [400, 437, 3, 474])
    init = bhmm_amd.gaussian_hmm([0.4, 0.3, 0.3], 0.8 * A + 0.2 / 3, mu + 0.4, sig * 1.3)
    data = bhmm_amd.lag_observations(obs, lag) if lag > 1 else obs
    lengths = [len(o) for o in data]
    assert lag == 1 or len(data) > len(obs) - 1
    est = bhmm_amd.MaximumLikelihoodEstimator(data, 3, initial_model=init, reversible=False, accuracy=1e-4,
                                              maxit=15)
    hmm = est.fit()
    want = {"viterbi": np.concatenate([np.asarray(p) for p in est.compute_viterbi_paths()]),
            "posterior": np.concatenate(est.posterior_decode())}
    for method in ("viterbi", "posterior"):
        off, s, ln, q, dwell, jumps = _rle(want[method], lengths, 3)
        segs, d, j = est.hidden_state_segments(method=method, stats=True)
        assert len(segs) == len(data)
        for k, (ts, tl, tq) in enumerate(segs):
            a, b = off[k], off[k + 1]
            assert np.array_equal(ts, s[a:b]) and np.array_equal(tl, ln[a:b]) and np.array_equal(tq, q[a:b])
        assert np.array_equal(d, dwell) and np.array_equal(j, jumps)
        plain = est.hidden_state_segments(method=method)
        assert all(np.array_equal(x, y) for a, b in zip(plain, segs) for x, y in zip(a, b))
        # the top-level call on the raw observations: it cuts the lagged views itself
        res = bhmm_amd.decode_segments(obs, hmm, lag=lag, method=method, stats=True)
        _same(res, (off, s, ln, q, dwell, jumps), True, "decode_segments %s lag=%d" % (method, lag))
    with pytest.raises(ValueError):
        est.hidden_state_segments(method="gibbs")
