"""Child process of tests/test_estep_prefetch_edges_gpu.py (BHMM_AMD_POISON is read once per process).

Runs every case, each against the CPU oracle, and prints one line per case: `CASE <name> ok` or
`CASE <name> FAIL <reason>`, then `all cases run`.  Only a failed comparison (AssertionError) lets the other
cases go on; any other exception -- a HIP error arrives as one -- ends the process at once with a non-zero
status, so that nothing more is started on the GPU, and the missing lines say where.
"""
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

from oracle import oracle as orc

M = 64

# (chunk, trajectory lengths).  A trajectory of T steps is cut into n = ceil(T / chunk) chunks of T // n or
# T // n + 1 steps (plan.hpp), a trajectory of at most `chunk` steps is one chunk; 64 consecutive chunks
# share a record group of Lmax = longest chunk records.
#
# backward main loop (two quads = 8 steps, discrete; two pairs = 4 steps, Gaussian) over len - 1 steps:
#   len - 1 = 3 -> no iteration, 8 / 9 -> one (two), 16 / 17 -> two (four), with and without single steps.
# SET_BWD: chunk lengths 9 | 10 9 | 17 17 | 4 | 1 | 10 | 18 18.  The first chunk of the first trajectory
# (record group 0, lane 0) runs exactly one iteration of the quad loop, whose refill reaches eight records
# before the buffers; the last chunk has Lmax steps and ends the (only, hence last) record group: the
# forward refill of its last group of eight reaches behind the observations.
SET_BWD = (18, (9, 19, 34, 4, 1, 10, 36))
# forward main loop (groups of 2 PF = 8 steps).  A chunk that starts its trajectory takes single steps up
# to step 4 (discrete) or 2 (Gaussian) first, any other chunk starts with the groups.
# SET_FWD_FIRST: first chunks of 11 12 13 20 21 steps (discrete: 7 8 9 16 17 steps in groups and singles,
# i.e. 0 1 1 2 2 iterations), 9 10 steps (Gaussian: 7 8).
SET_FWD_FIRST = (21, (12, 11, 13, 20, 9, 10, 21))
# SET_FWD_INNER: chunk lengths 8 8 | 7 7 | 9 8 | 1 | 9 9 9: chunks that do not start a trajectory with 7 8 9
# steps (0 1 1 iterations); the last chunk again has Lmax steps.
SET_FWD_INNER = (9, (16, 14, 17, 1, 27))
# ... and 15 16 17 steps (1 2 2 iterations): chunk lengths 16 16 | 15 15 | 17 16 | 17 17 17
SET_FWD_INNER2 = (17, (32, 30, 33, 51))
SETS = {"bwd": SET_BWD, "fwd_first": SET_FWD_FIRST, "fwd_inner": SET_FWD_INNER, "fwd_inner2": SET_FWD_INNER2}


def Engine(device):
    from bhmm_amd.engine import Engine as E
    return E(device)


def chunk_lens(T, chunk):
    n = -(-T // chunk)
    return [T // n + (1 if q < T % n else 0) for q in range(n)]


def model(n, seed, kind="discrete"):
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


def sample(kind, mdl, lengths, seed):
    rng = np.random.default_rng(seed)
    if kind == "gaussian":
        return [rng.normal(0.0, 3.0, T) for T in lengths]
    return [rng.integers(0, M, T).astype(np.int32) for T in lengths]   # (B has no zero entry)


def symbol_counts(obs, gammas, n):
    sc = np.zeros((n, M))
    for o, g in zip(obs, gammas):
        np.add.at(sc.T, o, g)
    return sc


def check(res, ref, kind, obs):
    """tolerances of tests/test_estep_gpu.py: log-likelihood 1e-11 relative, counts 1e-9"""
    np.testing.assert_allclose(res.logL_k, ref["logL"], rtol=1e-11)
    np.testing.assert_allclose(res.loglik, ref["logL"].sum(), rtol=1e-11)
    np.testing.assert_allclose(res.C, ref["C"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(res.state_counts, ref["state_counts"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(res.gamma0_sum, ref["gamma0_sum"], rtol=1e-9, atol=1e-14)
    if kind == "discrete":
        np.testing.assert_allclose(res.symbol_counts, symbol_counts(obs, ref["gammas"], res.C.shape[0]),
                                   rtol=1e-9, atol=1e-12)
    assert np.all(np.isfinite(res.packed))


def on_split_launches(eng):
    """the verified two-launch path on the branch-free kernels: the loops under test"""
    assert eng.get_option("spec_ok") > 0 and eng.get_option("spec_fail") == 0, "boundaries did not verify"
    assert eng.get_option("careful") == 0, "per-step-checked kernels took over"


def params(kind, mdl):
    return mdl if kind == "gaussian" else mdl[:3]


def estep_checked(eng, kind, mdl, obs):
    ref = orc.estep(kind, obs, *params(kind, mdl), want_gamma=(kind == "discrete"))
    res = eng.estep(*params(kind, mdl))
    on_split_launches(eng)
    check(res, ref, kind, obs)
    return res


def case_set(kind, n, which):
    chunk, lengths = SETS[which]
    mdl = model(n, 100 + n, kind)
    obs = sample(kind, mdl, lengths, 7)
    eng = Engine(0)
    eng.set_observations(kind, obs, n, nsymbols=M if kind == "discrete" else 0, chunk=chunk)
    want = [l for T in lengths for l in chunk_lens(T, chunk)]
    assert eng.num_chunks == len(want), (eng.num_chunks, want)
    res = estep_checked(eng, kind, mdl, obs)
    again = eng.estep(*params(kind, mdl))
    assert np.array_equal(res.packed, again.packed) and np.array_equal(res.logL_k, again.logL_k)
    eng.close()


def case_two_groups(kind, n):
    """65 chunks of 9 steps: chunk 64 opens a second record group, whose backward refill lands in the
    records of group 0"""
    mdl = model(n, 200 + n, kind)
    obs = sample(kind, mdl, (9 * 65,), 8)
    eng = Engine(0)
    eng.set_observations(kind, obs, n, nsymbols=M if kind == "discrete" else 0, chunk=9)
    assert eng.num_chunks == 65
    estep_checked(eng, kind, mdl, obs)
    eng.close()


def case_carry(kind, n):
    """Consecutive E-steps on one context with slightly different models.  The second one must run on
    carried boundary vectors (asserted: carry_W > 0, carry_ok counts it) and every one must split its
    backward sweep at a capture (asserted: carry_cap > 0) -- the `cap` stretch of the backward main loops
    at these chunk lengths.  Every call matches the oracle.  The same model a second and third time runs
    on full warm-ups both times (carried vectors are only used after a model change) with the same split:
    those two calls are bit-identical.  The call on carried starts differs from them by the boundary
    tolerance by design."""
    lengths = (400, 333, 290)
    m1 = model(n, 300 + n, kind)
    rng = np.random.default_rng(5)
    A2 = m1[0] * (1.0 + 1e-4 * rng.normal(size=m1[0].shape))
    A2 /= A2.sum(axis=1)[:, None]
    m2 = (A2,) + tuple(m1[1:])
    obs = sample(kind, m1, lengths, 9)
    eng = Engine(0)
    eng.set_option("spec_W", 40)
    eng.set_observations(kind, obs, n, nsymbols=M if kind == "discrete" else 0, chunk=64)

    def split_at_a_capture():
        cap = int(eng.get_option("carry_cap"))
        assert cap > 0 and cap % 8 == 0, cap
        return cap

    estep_checked(eng, kind, m1, obs)
    caps = [split_at_a_capture()]
    assert int(eng.get_option("carry_W")) == 0 and eng.get_option("carry_ok") == 0
    r2 = estep_checked(eng, kind, m2, obs)
    carried, ok = int(eng.get_option("carry_W")), eng.get_option("carry_ok")
    caps.append(split_at_a_capture())
    print("carry", kind, "carry_W of the second E-step", carried, "carry_ok", ok, "carry_fail",
          eng.get_option("carry_fail"), flush=True)
    assert carried > 0 and ok >= 1 and eng.get_option("carry_fail") == 0, (carried, ok)
    r3 = estep_checked(eng, kind, m2, obs)
    assert int(eng.get_option("carry_W")) == 0
    caps.append(split_at_a_capture())
    r4 = estep_checked(eng, kind, m2, obs)
    assert int(eng.get_option("carry_W")) == 0
    caps.append(split_at_a_capture())
    print("carry", kind, "caps", caps, "second == third bitwise", bool(np.array_equal(r2.packed, r3.packed)),
          flush=True)
    assert caps[2] == caps[3]
    assert np.array_equal(r3.packed, r4.packed) and np.array_equal(r3.logL_k, r4.logL_k)
    eng.close()


def case_lagged(kind, n):
    from bhmm_amd.api import lag_observations
    mdl = model(n, 400 + n, kind)
    base = sample(kind, mdl, (54, 35, 19), 10)
    lagged = lag_observations(base, 2)
    views = [np.ascontiguousarray(o) for o in lagged]
    eng = Engine(0)
    eng.set_observations_lagged(kind, lagged.base, lagged.lag, lagged.views, n,
                                nsymbols=M if kind == "discrete" else 0, chunk=9)
    estep_checked(eng, kind, mdl, views)
    eng.close()


def case_device(kind, n):
    import torch
    chunk, lengths = SET_BWD
    mdl = model(n, 500 + n, kind)
    obs = sample(kind, mdl, lengths, 11)
    t = torch.from_numpy(np.concatenate(obs)).to("cuda:0")
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    eng = Engine(0)
    eng.set_observations_device(kind, t.data_ptr(), off, n, nsymbols=M if kind == "discrete" else 0, chunk=chunk)
    estep_checked(eng, kind, mdl, obs)
    eng.close()


KINDS = (("discrete", 8), ("gaussian", 8), ("discrete", 2), ("discrete", 4))
CASES = []
for kind, n in KINDS:
    for which in SETS:
        CASES.append(("%s%d_%s" % (kind, n, which), case_set, (kind, n, which)))
    CASES.append(("%s%d_two_groups" % (kind, n), case_two_groups, (kind, n)))
for kind, n in KINDS[:2]:
    CASES.append(("%s%d_carry" % (kind, n), case_carry, (kind, n)))
    CASES.append(("%s%d_lagged" % (kind, n), case_lagged, (kind, n)))
    CASES.append(("%s%d_device" % (kind, n), case_device, (kind, n)))
NAMES = [c[0] for c in CASES]

if __name__ == "__main__":
    assert os.environ.get("BHMM_AMD_POISON"), "run with BHMM_AMD_POISON=1"
    import torch
    torch.cuda.init()   # (before the engine's own runtime start, as in the test processes: case_device)
    for name, fn, args in CASES:
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
