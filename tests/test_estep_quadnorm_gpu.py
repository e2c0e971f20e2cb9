"""Backward launch of the time-split E-step (up to 8 states) with the gamma / xi normaliser applied once
per stored alpha row: the quads (discrete kind) and pairs (Gaussian kind) of the branch-free sweep rebuild
alpha / S instead of alpha, and the discrete kind takes its state counts from the columns of the
workgroup's symbol table.  Every case runs against the CPU oracle with the tolerances of
tests/test_estep_gpu.py: log-likelihood 1e-11 relative, counts 1e-9 relative.
"""
import os

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

M = 64
# (chunk, trajectory lengths): three trajectories each.  A trajectory of T steps is cut into
# ceil(T / chunk) chunks of T // n or T // n + 1 steps (plan.hpp); the two sets together hold chunk
# lengths of every residue mod 8, i.e. every count of single steps in front of the groups of two quads,
# first, inner and last chunks of a trajectory.
SET_A = (200, (807, 861, 917))   # 161/162, 172/173, 183/184 steps: residues 1 2 4 5 7 0
SET_B = (40, (383, 323, 1173))   # 38/39, 35/36, 39/40 steps:       residues 6 7 3 4 7 0


def _chunk_lens(T, chunk):
    n = -(-T // chunk)
    return {T // n + (1 if q < T % n else 0) for q in range(n)}


def _engine():
    from bhmm_amd.engine import Engine
    return Engine(0)


def _model(n, seed, kind="discrete"):
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) + 0.05
    A /= A.sum(axis=1)[:, None]
    pi = rng.random(n) + 0.1
    pi /= pi.sum()
    if kind == "gaussian":
        return A, pi, np.linspace(-4.0, 4.0, n), rng.uniform(0.6, 1.4, n)
    B = rng.random((n, M)) + 0.01
    B /= B.sum(axis=1)[:, None]
    return A, pi, B, None


def _sample(A, pi, B, lengths, seed):
    """Trajectories drawn from the model itself (so that no observed symbol is impossible)."""
    rng = np.random.default_rng(seed)
    cA, cB = np.cumsum(A, axis=1), np.cumsum(B, axis=1)
    obs = []
    for T in lengths:
        u = rng.random((T, 2))
        s = int(np.searchsorted(np.cumsum(pi), u[0, 0]))
        o = np.empty(T, dtype=np.int32)
        for t in range(T):
            if t:
                s = min(int(np.searchsorted(cA[s], u[t, 0])), A.shape[0] - 1)
            o[t] = min(int(np.searchsorted(cB[s], u[t, 1])), B.shape[1] - 1)
        obs.append(o)
    return obs


def _symbol_counts(obs, gammas, n):
    sc = np.zeros((n, M))
    for o, g in zip(obs, gammas):
        np.add.at(sc.T, o, g)
    return sc


def _check(res, ref, obs=None):
    np.testing.assert_allclose(res.logL_k, ref["logL"], rtol=1e-11)
    np.testing.assert_allclose(res.loglik, ref["logL"].sum(), rtol=1e-11)
    np.testing.assert_allclose(res.C, ref["C"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(res.state_counts, ref["state_counts"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(res.gamma0_sum, ref["gamma0_sum"], rtol=1e-9, atol=1e-14)
    if obs is not None:
        np.testing.assert_allclose(res.symbol_counts, _symbol_counts(obs, ref["gammas"], res.C.shape[0]),
                                   rtol=1e-9, atol=1e-12)


def _discrete_invariants(eng, res, model, steps):
    """What the state counts from the symbol table must keep: they are its column sums, every step
    carries unit mass, and the fixed order of every sum makes a second call bit-identical."""
    np.testing.assert_allclose(res.state_counts, res.symbol_counts.sum(axis=1), rtol=1e-13)
    np.testing.assert_allclose(res.state_counts.sum(), steps, rtol=1e-12)
    again = eng.estep(*model)
    assert np.array_equal(res.packed, again.packed)
    assert np.array_equal(res.logL_k, again.logL_k)


def _took_split_launches(eng):
    """The verified two-launch path, on the branch-free kernels."""
    assert eng.get_option("spec_ok") > 0 and eng.get_option("spec_fail") == 0
    assert eng.get_option("careful") == 0


def _run_discrete(n, chunk, lengths, seed):
    A, pi, B, _ = _model(n, seed)
    obs = _sample(A, pi, B, lengths, seed + 1)
    ref = orc.estep("discrete", obs, A, pi, B, want_gamma=True)
    eng = _engine()
    eng.set_observations("discrete", obs, n, nsymbols=M, chunk=chunk)
    res = eng.estep(A, pi, B)
    _took_split_launches(eng)
    _check(res, ref, obs)
    _discrete_invariants(eng, res, (A, pi, B), sum(lengths))
    _took_split_launches(eng)
    eng.close()


def test_sets_hold_every_chunk_length_residue():
    res = set()
    for chunk, lengths in (SET_A, SET_B):
        for T in lengths:
            res |= {l % 8 for l in _chunk_lens(T, chunk)}
    assert res == set(range(8))


@pytest.mark.parametrize("chunk,lengths", [SET_A, SET_B])
def test_every_tail_residue(chunk, lengths):
    _run_discrete(8, chunk, lengths, 11)


@pytest.mark.parametrize("n", [5, 7])
def test_fewer_real_states_in_the_eight_state_kernel(n):
    _run_discrete(n, *SET_B, seed=20 + n)


@pytest.mark.parametrize("chunk,lengths", [SET_A, SET_B])
def test_gaussian_pairs(chunk, lengths):
    A, pi, mu, sig = _model(8, 31, "gaussian")
    rng = np.random.default_rng(32)
    obs = [rng.normal(0.0, 3.0, T) for T in lengths]
    ref = orc.estep("gaussian", obs, A, pi, mu, sig)
    eng = _engine()
    eng.set_observations("gaussian", obs, 8, chunk=chunk)
    res = eng.estep(A, pi, mu, sig)
    _took_split_launches(eng)
    _check(res, ref)
    np.testing.assert_allclose(res.state_counts.sum(), sum(lengths), rtol=1e-12)
    again = eng.estep(A, pi, mu, sig)
    assert np.array_equal(res.packed, again.packed)
    eng.close()


def test_exponents_differ_between_the_records_of_a_chunk():
    """Four states never emit the upper half of the alphabet (1e-30), the other four put most of their
    weight on one symbol each: the emission column of a step lies between 1e-30 and about 1 depending on
    the state, alpha and beta shed powers of two at nearly every rescale, and the exponents of the stored
    alpha rows (ea) and of beta (Eb) differ from record to record inside one chunk.  The reference is
    finite and the engine stays on the branch-free split launches (asserted: verified, not careful)."""
    n = 8
    A, pi, B, _ = _model(n, 41)
    B[:4, M // 2:] = 1e-30
    for i in range(4, n):
        B[i, M // 2 + i] = 8.0
    B /= B.sum(axis=1)[:, None]
    assert B.min() < 1e-29 and B.max() > 0.7
    chunk, lengths = SET_A
    obs = _sample(A, pi, B, lengths, 42)
    ref = orc.estep("discrete", obs, A, pi, B, want_gamma=True)
    assert all(np.all(np.isfinite(ref[k])) for k in ("logL", "C", "state_counts", "gamma0_sum"))
    eng = _engine()
    eng.set_observations("discrete", obs, n, nsymbols=M, chunk=chunk)
    res = eng.estep(A, pi, B)
    _took_split_launches(eng)
    _check(res, ref, obs)
    _discrete_invariants(eng, res, (A, pi, B), sum(lengths))
    eng.close()


@pytest.mark.parametrize("case", ["disc4_M1150_9501_20", "disc5_tiny_B_8001_1411"])
def test_guard_raises_and_the_careful_kernels_answer(case):
    """Saved cases on which the branch-free backward sweep must report instead of answer: a state that
    carries weight alpha_i / S of 2^850 or more (seed 9501 case 20, the wmax guard) and rebuilt rows that
    underflow (seed 8001 case 1411).  The E-step is repeated on the per-step-checked kernels and equals
    the oracle."""
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "cases", case + ".npz"), allow_pickle=True)
    A, pi, B, lens = d["A"], d["pi"], d["par0"], d["lens"]
    obs = [o.astype(np.int32) for o in np.split(d["obs"], np.cumsum(lens)[:-1])]
    ref = orc.estep("discrete", obs, A, pi, B)
    assert np.all(np.isfinite(ref["C"]))
    eng = _engine()
    eng.set_observations("discrete", obs, A.shape[0], nsymbols=B.shape[1], chunk=int(d["chunk"]))
    res = eng.estep(A, pi, B)
    assert eng.get_option("careful") == 1
    print(case, "logL rel", np.max(np.abs(res.logL_k / ref["logL"] - 1.0)),
          "C abs", np.max(np.abs(res.C - ref["C"])), "state counts abs",
          np.max(np.abs(res.state_counts - ref["state_counts"])))
    np.testing.assert_allclose(res.logL_k, ref["logL"], rtol=1e-11)
    np.testing.assert_allclose(res.C, ref["C"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(res.state_counts, ref["state_counts"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(res.state_counts.sum(), sum(int(l) for l in lens), rtol=1e-12)
    eng.close()
