"""Case builders shared by tests/test_viterbi_matrix_cpu.py and tests/test_viterbi_matrix_gpu.py: models, data,
the planner rule and a numpy restatement of the max-product recursion.  Every case is a function of its arguments
alone (its own seed), so the CPU file checks exactly the inputs the GPU file runs.

The only reference of either file is orc.viterbi on orc.pobs_gaussian / orc.pobs_discrete (reference() below,
computed once per case and left unchanged).  The numpy recursion (maxprod_step) is NOT a reference: it places
conditions on the inputs -- "a warm-up of W steps from the uniform vector leaves this boundary more than 1e-6 off" --
for which its 1e-15 is plenty."""
import numpy as np

from oracle import oracle as orc

KINDS = ("gaussian", "discrete", "explicit")
M = 13                      # alphabet of the discrete cases
NUM_SIMD = 1024             # MI355X: 256 compute units of four SIMDs (the plans below are asserted on the GPU)


# ---- the planner ----------------------------------------------------------------------------------------------------
def plan(lengths, L):
    """(trajectory, t0, len) of every segment: plan::plan_segments (csrc/plan.hpp) with mult 1"""
    segs = []
    for k, T in enumerate(lengths):
        ns = -(-T // L) if L > 0 else 1
        prev = 0
        for q in range(1, ns + 1):
            b = T if q == ns else ((q * T) // ns) & ~3
            if b > prev:
                segs.append((k, prev, b - prev))
                prev = b
    return segs


def np_of(n):
    """lanes per segment of k_wide_viterbi_seg (9 .. 64 states)"""
    return 16 if n <= 16 else 32 if n <= 32 else 64


def seglen_wide(total, n, W, seg_per_simd=1, warmups=2):
    """segment length of the 9..64-state pass (plan::vit_wide_seglen, called by wide_seg_viterbi in path_api.hip; the
    two are compared in tests/test_viterbi_plan_cpu.py): enough segments for every lane group of the device, none
    shorter than `warmups` warm-ups"""
    want = seg_per_simd * NUM_SIMD * (64 // np_of(n))
    return max(-(-total // want), warmups * W)


def seglen_gen(total, n, W, seg_per_simd=1):
    """... of the 65..128-state pass (plan::vit_gen_seglen, gen_seg_viterbi in gen_api.hip; one warm-up per segment
    with the margin rule on) and of the row-batched pass for 129..256 states (plan::vit_rows_fill / vit_rows_seglen,
    gen_rows_viterbi; four segments per workgroup, one workgroup per compute unit)"""
    if n <= 128:
        return max(-(-total // (seg_per_simd * NUM_SIMD)), W)
    fill0 = (-(-total // (4 * (NUM_SIMD // 4))) + 7) // 8 * 8
    return max(fill0, W)


# ---- models -----------------------------------------------------------------------------------------------------------
def _emission(n, rng, kind, mu_span, sig_lo, sig_hi, conc):
    if kind == "gaussian":
        return np.linspace(-mu_span, mu_span, n), rng.uniform(sig_lo, sig_hi, n)
    if kind == "discrete":
        return rng.dirichlet(np.ones(M) * conc, n), None
    return None, None


def fast_model(n, rng, kind):
    """forgets within a few dozen steps (the recipe of tests/test_viterbi_margin_gpu.py)"""
    A = rng.random((n, n)) + 0.05
    A += np.eye(n) * 8.0
    A /= A.sum(axis=1)[:, None]
    pi = rng.dirichlet(np.ones(n))
    return (A, pi) + _emission(n, rng, kind, 6.0, 0.5, 1.5, 1.0)


def slow_model(n, rng, kind):
    """diagonal 0.99: the max-product vectors of two starts meet only once one state has pulled ahead of all others by
    the off-diagonal factor (1e-2 / n).  The emissions are as flat as leaves that to a few dozen steps -- more than a
    warm-up of 16, within the reach of twelve fix-up rounds on segments of 32 (flatter ones, tried first, took 200 to
    600 steps and the library, rightly, gave such observations to the serial kernel)"""
    A = rng.random((n, n)) + 0.05
    np.fill_diagonal(A, 0.0)
    A *= 0.01 / A.sum(axis=1)[:, None]
    A[np.arange(n), np.arange(n)] = 0.99
    pi = rng.dirichlet(np.ones(n))
    return (A, pi) + _emission(n, rng, kind, 6.0, 0.7, 1.2, 0.4)


def flat_model(n, rng, kind):
    """diagonal 0.99 and emissions that hardly tell the states apart: no warm-up of a few steps reproduces a vector
    (8 states and fewer, where the slow model above still forgets within two steps at n = 2)"""
    A, pi = slow_model(n, rng, kind)[:2]
    return (A, pi) + _emission(n, rng, kind, 1.0, 1.0, 1.2, 20.0)


def metastable_model(n, rng, kind):
    """lifetimes of 10 .. 100 steps, overlapping emissions (tests/test_viterbi_margin_gpu.py, the mending test): after
    a short warm-up SOME boundaries are further than 1e-12 from their predecessors' vectors, most are not"""
    life = np.exp(np.linspace(np.log(10.0), np.log(100.0), n))
    A = rng.random((n, n)) + 0.05
    np.fill_diagonal(A, 0.0)
    A = A / A.sum(axis=1)[:, None] / life[:, None]
    A[np.arange(n), np.arange(n)] = 1.0 - 1.0 / life
    pi = np.full(n, 1.0 / n)
    if kind == "gaussian":
        return A, pi, np.linspace(-5, 5, n), np.linspace(0.5, 2.0, n)
    if kind == "discrete":
        return A, pi, rng.dirichlet(np.ones(M) * 0.7, n), None
    return A, pi, None, None


def observations(kind, rng, lengths, n, dwell=False, flat=False):
    """gaussian: white noise wider than the means; discrete: uniform symbols; explicit: random positive rows, each
    times its own factor over six decades.  dwell (the slowly forgetting model's explicit rows): one entry per row,
    the same for 20 .. 60 steps on end, is three times larger -- rows of pure noise let no state pull ahead for
    hundreds of steps, more than twelve fix-up rounds cover.  flat (flat_model's data): noise as narrow as the
    means, explicit entries within a factor of two of each other"""
    if kind == "gaussian":
        return [rng.normal(0.0, 1.0 if flat else 4.0, T) for T in lengths]
    if kind == "discrete":
        return [rng.integers(0, M, T).astype(np.int32) for T in lengths]
    obs = [rng.uniform(0.5 if flat else 0.02, 1.0, (T, n)) for T in lengths]
    if dwell:
        for o in obs:
            t = 0
            while t < len(o):
                d = int(rng.integers(20, 61))
                o[t:t + d, int(rng.integers(n))] *= 3.0
                t += d
    return [o * 10.0 ** rng.uniform(-3.0, 3.0, (len(o), 1)) for o in obs]


def pobs_of(kind, obs, model):
    _, _, p0, p1 = model
    if kind == "gaussian":
        return [orc.pobs_gaussian(o, p0, p1) for o in obs]
    if kind == "discrete":
        return [orc.pobs_discrete(o, p0) for o in obs]
    return [np.ascontiguousarray(o, dtype=np.float64) for o in obs]


_references = {}


def reference(key, kind, obs, model):
    """the oracle's paths of a case, computed once per `key` and read-only from then on"""
    if key not in _references:
        A, pi = model[0], model[1]
        paths = [orc.viterbi(A, po, pi) for po in pobs_of(kind, obs, model)]
        for p in paths:
            p.setflags(write=False)
        _references[key] = paths
    return _references[key]


def case(section, n, kind, lengths, model_fn=fast_model, dwell=False, seed=0):
    """model, data and lengths of one case; the seed is a function of the arguments"""
    rng = np.random.default_rng(10007 * section + 31 * n + KINDS.index(kind) + 1000003 * seed)
    model = model_fn(n, rng, kind)
    obs = observations(kind, rng, lengths, n, dwell, flat=model_fn is flat_model)
    return dict(key=(section, n, kind, tuple(lengths), model_fn.__name__, dwell, seed), n=n, kind=kind,
                lengths=tuple(lengths), model=model, obs=obs, nsymbols=M if kind == "discrete" else 0)


def case_reference(c):
    return reference(c["key"], c["kind"], c["obs"], c["model"])


# ---- the max-product recursion, restated ------------------------------------------------------------------------------
def maxprod_step(v, A, p):
    vn = p * (v[:, None] * A).max(axis=0)
    return vn / vn.sum()


def boundary_deviation(A, pobs, pi, starts, W, upto=None):
    """For every segment start t0 > 0 in `starts` (below `upto`): the largest relative difference between the vector
    of step t0 - 1 of the serial recursion and the one reached from the uniform vector W steps earlier (exactly 0
    where the warm-up reaches the trajectory's start: there the pass starts from pi, like the serial run)."""
    n = A.shape[0]
    starts = sorted(t for t in starts if t > 0 and (upto is None or t <= upto))
    if not starts:
        return {}
    want = set(t - 1 for t in starts)
    kept = {}
    v = pi * pobs[0]
    v = v / v.sum()
    if 0 in want:
        kept[0] = v
    for t in range(1, starts[-1]):
        v = maxprod_step(v, A, pobs[t])
        if t in want:
            kept[t] = v
    out = {}
    for t0 in starts:
        tw = t0 - W
        if tw <= 0:
            out[t0] = 0.0
            continue
        u = np.full(n, 1.0 / n)
        for t in range(tw, t0):
            u = maxprod_step(u, A, pobs[t])
        s = kept[t0 - 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(s == u, 0.0, np.abs(u - s) / np.maximum(s, 1e-300))
        out[t0] = float(d.max())
    return out


def case_boundary_deviation(c, L, W, upto=None):
    """boundary_deviation over every trajectory of a case cut into segments of L: {(k, t0): deviation}"""
    A, pi = c["model"][0], c["model"][1]
    pobs = pobs_of(c["kind"], c["obs"], c["model"])
    out = {}
    for k in range(len(c["lengths"])):
        starts = [t0 for kk, t0, _ in plan(c["lengths"], L) if kk == k]
        for t0, d in boundary_deviation(A, pobs[k], pi, starts, W, upto).items():
            out[(k, t0)] = d
    return out


# ---- section 1: 9 .. 64 states -----------------------------------------------------------------------------------------
S1_STATES = (9, 15, 16, 17, 31, 32, 33, 48, 63, 64)
S1_LENGTHS = (9001, 1, 2, 50, 6000, 300)          # 50 < the policy's warm-up of 128
S1B_LENGTHS = (6000, 1, 2, 11, 3000)              # 11 < the forced warm-ups
S1B_W = 16                                        # from {8, 16, 32}: see test_viterbi_matrix_cpu.py


def s1a_case(n, kind):
    return case(1, n, kind, S1_LENGTHS)


def s1b_case(n, kind):
    return case(11, n, kind, S1B_LENGTHS, slow_model, dwell=True)


# ---- section 2: 8 states and fewer ---------------------------------------------------------------------------------------
S2_STATES = (2, 3, 4, 5, 7, 8)
S2_CHUNKS = (16, 64, 300)
S2_LENGTHS = (5000, 1, 2, 257, 63)
S2_MARGIN_W = (8, 12, 16, 20, 24, 26, 28, 30, 32, 36, 40, 48, 64)     # warm-ups under which some boundary carries rounding noise only


def s2_case(n, kind, slow=False):
    return case(22 if slow else 2, n, kind, S2_LENGTHS, flat_model if slow else fast_model)


# ---- section 3: twins ----------------------------------------------------------------------------------------------------
# n -> pairs (i, i') with i' an exact copy of i.  128 states: 63, 64 and 65 are one class of three.  200 states: the two
# candidate ranges of k_gen_viterbi_rows<4, 2> are [0, 104) and [104, 200) (gen_kernels.hpp: (n / 2 rounded up to 8)), so
# 103 | 104 and 0 | 199 are decided where the ranges are merged; 63 | 64 and 127 | 128 lie across wavefronts of targets.
TWINS = {
    64: ((7, 8), (15, 16), (31, 32), (47, 48), (3, 35), (0, 63)),
    20: ((7, 8), (15, 16), (0, 19)),
    12: ((7, 8), (0, 11)),
    8: ((1, 2), (3, 4)),
    4: ((1, 2),),
    128: ((63, 64), (64, 65), (0, 127)),
    200: ((103, 104), (127, 128), (63, 64), (0, 199)),
}
TWIN_KINDS = {64: KINDS, 20: KINDS, 12: KINDS, 8: KINDS, 4: KINDS, 128: ("gaussian", "explicit"),
              200: ("gaussian", "explicit")}
TWIN_LENGTHS = {64: (6000, 700, 1500, 2, 900), 20: (6000, 700, 1500, 2, 900), 12: (6000, 700, 1500, 2, 900),
                8: (5000, 700, 257, 2, 900), 4: (5000, 700, 257, 2, 900), 128: (6000, 700, 2, 900),
                200: (6000, 700, 2, 900)}


def twin_classes(n):
    """class of every state (the lowest index of its class) and the classes with more than one member"""
    cls = np.arange(n)
    for i, j in TWINS[n]:
        lo = min(cls[i], cls[j])
        hi = max(cls[i], cls[j])
        cls[cls == hi] = lo
    twin = sorted(set(int(c) for c in cls if (cls == c).sum() > 1))
    return cls, twin


def twin_case(n, kind):
    """A model built per CLASS and expanded, so that the members of a class have bitwise equal rows and columns of A,
    pi entries and emissions.  The twin classes get the largest self-transition and emissions of their own; the data
    dwell in a class for 10 .. 40 steps, every other dwell in a twin class, and every trajectory ends in one."""
    rng = np.random.default_rng(30011 + 31 * n + KINDS.index(kind))
    cls, twin = twin_classes(n)
    lengths = TWIN_LENGTHS[n]
    A = (rng.random((n, n)) + 0.05)[cls][:, cls]            # A[s, t] = Ac[class(s), class(t)]
    for s in range(n):
        for t in range(n):
            if cls[s] == cls[t]:
                A[s, t] = 12.0 if cls[s] in twin else 4.0
    A /= A.sum(axis=1)[:, None]
    pi = rng.dirichlet(np.ones(n))[cls]
    pi /= pi.sum()
    single = [int(c) for c in sorted(set(cls)) if c not in twin]
    # hidden class of every step
    hidden = []
    for T in lengths:
        h = np.empty(T, dtype=np.int64)
        t, q = 0, 0
        while t < T:
            d = int(rng.integers(10, 41))
            c = twin[int(rng.integers(len(twin)))] if (q % 2 == 0 or not single) else single[int(rng.integers(len(single)))]
            h[t:t + d] = c
            t += d
            q += 1
        h[max(T - 12, 0):] = twin[int(rng.integers(len(twin)))]
        hidden.append(h)
    # emissions: the twin classes apart from each other and from the rest
    mu = np.linspace(-6.0, 6.0, n)
    sig = rng.uniform(0.5, 1.0, n)
    for q, c in enumerate(twin):
        mu[c] = 10.0 + 4.0 * q
        sig[c] = 0.8
    mu, sig = mu[cls], sig[cls]
    if kind == "discrete":
        Mt = len(twin) + 7
        B = rng.dirichlet(np.ones(Mt), n)
        for q, c in enumerate(twin):
            B[c] = 0.2 / (Mt - 1)
            B[c, q] = 0.8
        B = B[cls]
        B /= B.sum(axis=1)[:, None]
        obs = []
        for h in hidden:
            o = np.empty(len(h), dtype=np.int32)
            for t, c in enumerate(h):
                o[t] = rng.choice(Mt, p=B[c])
            obs.append(o)
        model = (A, pi, B, None)
    else:
        obs = [mu[h] + sig[h] * rng.standard_normal(len(h)) for h in hidden]
        model = (A, pi, mu, sig)
        if kind == "explicit":      # the Gaussian rows, each times its own factor: twin columns stay bitwise equal
            obs = [orc.pobs_gaussian(o, mu, sig) * 10.0 ** rng.uniform(-3.0, 3.0, (len(o), 1)) for o in obs]
            model = (A, pi, None, None)
    c = dict(key=("twin", n, kind), n=n, kind=kind, lengths=lengths, model=model, obs=obs)
    c["nsymbols"] = model[2].shape[1] if kind == "discrete" else 0
    return c


# ---- section 4: geometry ---------------------------------------------------------------------------------------------------
S4_STATES = (12, 24, 64, 100, 200)
S4_KINDS = ("gaussian", "discrete")
S4_PHASES = (1, 37, 63, 64, 65)
S4_RELOAD = (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 6000)
# segment counts around multiples of the segments per wavefront (4, 2, 1) and per workgroup (16, 8, 4) of
# k_wide_viterbi_seg, of the eight wavefronts of k_gen_viterbi_seg and of the four rows of k_gen_viterbi_rows
S4_COUNTS = {12: (3, 4, 5, 8, 9, 16, 17), 24: (2, 3, 4, 5, 8, 9), 64: (1, 2, 3, 4, 5), 100: (7, 8, 9),
             200: (3, 4, 5, 7, 8, 9)}
S4_W = {12: 128, 24: 128, 64: 128, 100: 288, 200: 288}      # the policy's first warm-up on fresh observations


def s4_seglen(n, total):
    return seglen_wide(total, n, S4_W[n]) if n <= 64 else seglen_gen(total, n, S4_W[n])


def s4_count_length(n, s):
    """a trajectory length that the planner cuts into exactly s segments"""
    return s * s4_seglen(n, 0) - 2


def s4_case(n, kind, lengths, tag):
    return case(4, n, kind, lengths, seed=tag)


# ---- section 5: the ones rule ----------------------------------------------------------------------------------------------
S5_STATES = (20, 64)
S5_LENGTHS = (37, 4000)       # the long trajectory starts at phase 37 of the 64-step grid
S5_W = 128


def s5_case(n):
    """Gaussian; an observation 60 sigma above every state (a zero density in every state) at: step 0, the last step,
    the first and last step of an interior segment, a step inside a warm-up (t0 - W / 2) and -- 64 states -- steps
    whose count from the start of their segment's run, (gt - (o0 + tw)) & 63, is 0 and 63."""
    c = case(5, n, "gaussian", S5_LENGTHS)
    _, _, mu, sig = c["model"]
    far = float(mu.max() + 60.0 * sig.max() + 60.0 * sig.max())     # >= 60 sigma_i from every mu_i
    T = S5_LENGTHS[1]
    L = seglen_wide(sum(S5_LENGTHS), n, S5_W)
    segs = [(t0, ln) for k, t0, ln in plan(S5_LENGTHS, L) if k == 1]
    assert len(segs) >= 12
    where = {"step 0": 0, "last step": T - 1, "first step of a segment": segs[3][0],
             "last step of a segment": segs[5][0] + segs[5][1] - 1, "inside a warm-up": segs[8][0] - S5_W // 2}
    if n == 64:
        tw = segs[10][0] - S5_W
        where["run step & 63 == 0"] = tw + 192
        tw = segs[12][0] - S5_W
        where["run step & 63 == 63"] = tw + 191
    obs = [o.copy() for o in c["obs"]]
    for t in where.values():
        obs[1][t] = far
    c = dict(c, obs=obs, key=("ones", n), where=where, seglen=L, nseg=len(segs) + 1)
    return c


# ---- section 6: above 64 states ---------------------------------------------------------------------------------------------
S6_CASES = [(n, k) for n in (65, 66, 127, 128, 129, 130, 255, 256) for k in ("gaussian", "explicit")] + \
           [(66, "discrete"), (255, "discrete")]
S6_LENGTHS = (6000, 1, 700, 2)
S6_FORCED = ((66, "gaussian", 32), (130, "gaussian", 128))       # (n, kind, viterbi_W)


def s6_case(n, kind):
    return case(6, n, kind, S6_LENGTHS)


def s6_forced_case(n, kind):
    """65..128 states: the slowly forgetting model (fix-up rounds).  129..256: no rounds exist there, and the mending
    variant runs only when at most half of the boundaries are far -- the metastable model"""
    if n <= 128:
        return case(66, n, kind, S6_LENGTHS, slow_model, dwell=True)
    return case(66, n, kind, S6_LENGTHS, metastable_model)


def s257_case():
    return case(257, 257, "gaussian", (700, 1, 300))
