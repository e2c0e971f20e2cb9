"""Cases of tests/test_estep_obs16_gpu.py, and its child process.

The split E-step of the discrete kind (up to 8 states, B^T in LDS, M * N * 8 <= 65536 with N the padded state
count) reads a second copy of the observations in its main loops: 16 bits per step, the byte offset sym * N * 8 of
the symbol's table row, in blocks of four steps.  Every case here runs an E-step against the CPU oracle at the
tolerances of tests/test_estep_gpu.py (log-likelihood 1e-11 relative, counts 1e-9), asserts which copy the sweeps
read (option obs16_used), repeats the call (bitwise equal) and compares with a context forced onto the int32 copy
(option obs16 = 0; bitwise equal).

As a program (BHMM_AMD_POISON=1, read once per process) it runs the edge cases with every fresh allocation and
the guards around the new buffer filled with 0xFF bytes, one line per case: `CASE <name> ok` or `CASE <name> FAIL
<reason>`, then `all cases run`.  Only a failed comparison lets the other cases go on; anything else ends the
process at once, so that nothing more is started on the GPU.

Chunk plans.  A trajectory of T steps is cut into n = ceil(T / chunk) chunks of T // n or T // n + 1 steps; one of
at most `chunk` steps is one chunk.  The sets hold trajectories of 1, 2, 9 and 4100 steps (and a fifth that makes
a short first chunk):
  chunk 24: 4100 -> 167 chunks of 24 and 4 of 23        Lmax 24 (a multiple of 4), three record groups
  chunk 25: 4100 -> 164 chunks of 25                    Lmax 25 (odd)
  chunk 26: 4100 -> 150 chunks of 26 and 8 of 25        Lmax 26
so that len % 8 takes 0, 1, 2, 7 and (len - 1) % 8 takes 7, 0, 1, 6 -- with 9 (1, 0), 2 and 1 from the short
trajectories -- for chunks that start a trajectory (the forward groups start at step 4) and chunks that do not.
"""
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

from oracle import oracle as orc

LENGTHS = (1, 4100, 2, 9, 17)
CHUNKS = (24, 25, 26)


def padded(n):
    return 2 if n <= 2 else 4 if n <= 4 else 8


def packs(n, M):
    """whether the context builds the 16-bit copy: every row offset fits 16 bits, and the tables fit the LDS --
    the library keeps alphabets above about 1180 symbols in global memory whatever the state count"""
    return M * padded(n) * 8 <= 65536 and M <= 1024


def Engine(device):
    from bhmm_amd.engine import Engine as E
    return E(device)


def chunk_lens(T, chunk):
    n = -(-T // chunk)
    return [T // n + (1 if q < T % n else 0) for q in range(n)]


def model(n, M, seed):
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) + 0.05
    A /= A.sum(axis=1)[:, None]
    pi = rng.random(n) + 0.1
    pi /= pi.sum()
    B = rng.random((n, M)) + 0.01
    B /= B.sum(axis=1)[:, None]
    return A, pi, B


def sample(M, lengths, seed):
    """uniform symbols; the last symbol of the alphabet stands at the first, the last and every 37th step"""
    rng = np.random.default_rng(seed)
    obs = [rng.integers(0, M, T).astype(np.int32) for T in lengths]
    for o in obs:
        o[::37] = M - 1
        o[-1] = M - 1
    return obs


def symbol_counts(obs, gammas, n, M):
    sc = np.zeros((n, M))
    for o, g in zip(obs, gammas):
        np.add.at(sc.T, o, g)
    return sc


_REF = {}


def reference(n, M, mdl, obs, key):
    """the oracle's E-step, computed once per (model, observations)"""
    if key not in _REF:
        ref = orc.estep("discrete", obs, *mdl, want_gamma=True)
        ref["symbol_counts"] = symbol_counts(obs, ref["gammas"], n, M)
        del ref["gammas"]
        _REF[key] = ref
    return _REF[key]


def check(res, ref):
    """tolerances of tests/test_estep_gpu.py: log-likelihood 1e-11 relative, counts 1e-9"""
    np.testing.assert_allclose(res.logL_k, ref["logL"], rtol=1e-11)
    np.testing.assert_allclose(res.loglik, ref["logL"].sum(), rtol=1e-11)
    np.testing.assert_allclose(res.C, ref["C"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(res.state_counts, ref["state_counts"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(res.gamma0_sum, ref["gamma0_sum"], rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(res.symbol_counts, ref["symbol_counts"], rtol=1e-9, atol=1e-12)
    assert np.all(np.isfinite(res.packed))


def on_split_launches(eng):
    assert eng.get_option("spec_ok") > 0 and eng.get_option("spec_fail") == 0, "boundaries did not verify"
    assert eng.get_option("careful") == 0, "per-step-checked kernels took over"


def same_bits(a, b, tables_ordered):
    """Every statistic bit for bit.  The symbol counts only where each wavefront adds to a count table of its own.
    With one table per workgroup (8 states: M above about 460) or the global tables of a big alphabet, the atomic
    additions of several wavefronts reach a cell in any order, from call to call of ONE build as well.  A cell of
    these cases sums at most 130 non-negative terms (the last symbol: every 37th of 4100 steps, plus chance hits),
    so two orders differ by at most 129 * 2^-53 = 1.5e-14 of the sum: the bound is 1e-13."""
    assert np.array_equal(a.logL_k, b.logL_k)
    assert np.array_equal(a.C, b.C) and np.array_equal(a.state_counts, b.state_counts)
    assert np.array_equal(a.gamma0_sum, b.gamma0_sum)
    if tables_ordered:
        assert np.array_equal(a.symbol_counts, b.symbol_counts)
        assert np.array_equal(a.packed, b.packed)
    else:
        np.testing.assert_allclose(a.symbol_counts, b.symbol_counts, rtol=1e-13, atol=0)


def tables_ordered(n, M):
    """one count table per wavefront: tables in LDS and (1 + wavefronts) of them well inside it"""
    N = padded(n)
    return M <= 1024 and M * N * 8 * (1 + max(1, N // 2)) <= 128 * 1024


def run(n, M, obs, mdl, ref, load, want16=None):
    """load(eng) hands the observations over.  A context on the 16-bit copy (where the alphabet allows it) twice,
    one forced onto the int32 copy: all against the oracle, all with the same bits."""
    want16 = packs(n, M) if want16 is None else want16
    ordered = tables_ordered(n, M)
    eng = Engine(0)
    load(eng)
    res = eng.estep(*mdl)
    on_split_launches(eng)
    assert bool(eng.get_option("obs16_used")) == want16, (n, M, eng.get_option("obs16_used"))
    check(res, ref)
    again = eng.estep(*mdl)
    assert bool(eng.get_option("obs16_used")) == want16
    same_bits(res, again, ordered)
    eng.close()
    forced = Engine(0)
    forced.set_option("obs16", 0)
    load(forced)
    r32 = forced.estep(*mdl)
    on_split_launches(forced)
    assert forced.get_option("obs16_used") == 0
    check(r32, ref)
    same_bits(res, r32, ordered)
    forced.close()


def case_plan(n, M, chunk):
    mdl = model(n, M, 100 + n)
    obs = sample(M, LENGTHS, 7)
    ref = reference(n, M, mdl, obs, ("plan", n, M))

    def load(eng):
        eng.set_observations("discrete", obs, n, nsymbols=M, chunk=chunk)
        want = [l for T in LENGTHS for l in chunk_lens(T, chunk)]
        assert eng.num_chunks == len(want), (eng.num_chunks, len(want))
    run(n, M, obs, mdl, ref, load)


def case_device(n, M, chunk):
    import torch
    mdl = model(n, M, 100 + n)
    obs = sample(M, LENGTHS, 7)
    ref = reference(n, M, mdl, obs, ("plan", n, M))
    t = torch.from_numpy(np.concatenate(obs)).to("cuda:0")
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)

    def load(eng):
        eng.set_observations_device("discrete", t.data_ptr(), off, n, nsymbols=M, chunk=chunk)
    run(n, M, obs, mdl, ref, load)


def case_lagged(n, M, chunk):
    from bhmm_amd.api import lag_observations
    mdl = model(n, M, 100 + n)
    base = sample(M, (8200, 35, 19), 10)
    lagged = lag_observations(base, 2)
    views = [np.ascontiguousarray(o) for o in lagged]
    ref = reference(n, M, mdl, views, ("lag", n, M))

    def load(eng):
        eng.set_observations_lagged("discrete", lagged.base, lagged.lag, lagged.views, n, nsymbols=M, chunk=chunk)
    run(n, M, views, mdl, ref, load)


def case_replan(n, M):
    """The automatic plan, which the library may re-make once the warm-up is known: the 16-bit copy follows it."""
    mdl = model(n, M, 100 + n)
    obs = sample(M, (40000, 9, 1), 12)
    ref = reference(n, M, mdl, obs, ("auto", n, M))

    def load(eng):
        eng.set_observations("discrete", obs, n, nsymbols=M, chunk=0)
    run(n, M, obs, mdl, ref, load)


# (state counts 8 7 3 2: padded 8 8 4 2) x (M 2, 64) x the three plans
PLAN_CASES = [("n%d_M%d_chunk%d" % (n, M, ch), case_plan, (n, M, ch))
              for n in (8, 7, 3, 2) for M in (2, 64) for ch in CHUNKS]
# the largest alphabet whose offsets fit 16 bits at each padded state count (8 states: the top offset is 65472, in
# LDS; at 4 and 2 states those alphabets are beyond the LDS and stay on the int32 copy, as does 1500), the largest
# that fits the LDS at 4 and 2 states, one symbol above the limit at 8 states
BIG_CASES = [("n%d_M%d_chunk%d" % (n, M, ch), case_plan, (n, M, ch))
             for n, M, ch in ((8, 1024, 24), (7, 1024, 25), (8, 1025, 24), (8, 1500, 26), (3, 2048, 24), (2, 4096, 25),
                              (3, 1024, 26), (2, 1024, 24))]
ROUTE_CASES = [("n8_M64_device", case_device, (8, 64, 24)), ("n3_M64_device", case_device, (3, 64, 25)),
               ("n8_M64_lagged", case_lagged, (8, 64, 25)), ("n2_M64_lagged", case_lagged, (2, 64, 24)),
               ("n8_M64_replan", case_replan, (8, 64)), ("n8_M1024_device", case_device, (8, 1024, 26))]
CASES = PLAN_CASES + BIG_CASES + ROUTE_CASES
# what the child runs under BHMM_AMD_POISON=1: every plan at 8 states, one each at 4 and 2, the top offsets, the routes
EDGE_CASES = [c for c in CASES if c[0].startswith("n8_M64_") or c[0] in
              ("n3_M64_chunk25", "n2_M64_chunk24", "n8_M1024_chunk24", "n8_M1025_chunk24", "n8_M1024_device",
               "n3_M64_device", "n2_M64_lagged")]
NAMES = [c[0] for c in CASES]
EDGE_NAMES = [c[0] for c in EDGE_CASES]

if __name__ == "__main__":
    assert os.environ.get("BHMM_AMD_POISON"), "run with BHMM_AMD_POISON=1"
    import torch
    torch.cuda.init()   # (before the engine's own runtime start, as in the test processes: case_device)
    for name, fn, args in EDGE_CASES:
        try:
            fn(*args)
            print("CASE", name, "ok", flush=True)
        except AssertionError as e:  # a failed comparison: go on with the other cases
            traceback.print_exc(file=sys.stdout)
            print("CASE", name, "FAIL", type(e).__name__, str(e).replace("\n", " | ")[:600], flush=True)
        except BaseException as e:   # anything else (a HIP error comes as RuntimeError): nothing more runs on the GPU
            traceback.print_exc(file=sys.stdout)
            print("CASE", name, "ERROR", type(e).__name__, str(e).replace("\n", " | ")[:600], flush=True)
            print("stopped: no further case was started", flush=True)
            sys.stdout.flush()
            os._exit(3)
    print("all cases run", flush=True)
