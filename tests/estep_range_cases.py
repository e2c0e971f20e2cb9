"""Test infrastructure for the number-range tests of the lazily scaled E-step (test_estep_range_cpu.py,
test_estep_range_gpu.py): the trajectories, tuned models and emission rows of tests/score_range_cases.py (imported,
not copied), a restatement of the two forward schedules of the E-step, a full E-step reference in 80-bit arithmetic
shaped like _want(ref) of tests/test_tile_matrix_gpu.py, and the batches the GPU test runs.

The schedules (estep_run), one trajectory from its start, in the arithmetic of the rows handed over:
  wide  k_wide_fwd<.., LAZY> (csrc/wide_kernels.hpp): the exponent of the largest element is measured and taken off
        on steps r % 4 == 3.  It calls wide_emit<.., RESCUE = !LAZY>: a row in the denormal range is multiplied in
        as it stands -- unlike k_score_wide<.., LAZY>, which sc.lazy_run("wide") restates.
  tile  k_tile_fwd (csrc/tile_kernels.hpp): m_step measures the row maxima into sE on u == 2 (pm, row16_max_i32)
        from the values it writes, and on u == 3 takes max(sE) off the values it writes (ldexp(v, -E[r])); s_step
        looks at that E on u == 3, and only where the row is still active (rs < nst[r]).  A vector that is all zero
        measures -(1 << 28).
Neither looks at the exit sum here; that is what the kernels' last line does, and what the tests are about.

Steps are counted from the trajectory's start although the kernels count them from the start of a segment's
warm-up: plan::plan_segments cuts inner boundaries at multiples of four and the warm-up length is a multiple of
eight, so a cut trajectory's last segment starts its warm-up at a multiple of four and every refresh falls on the
same steps either way (assert_warmups_on_four asserts it on _plan for the lengths in use).  After its first
refresh the vector of such a segment is the exact one up to the warm-up's error and a power of two.

The reference (reference) is ld_reference.hidden_longdouble on sc.rows_exact: logL, gamma and C per trajectory; a
batch's gamma0_sum, state_counts, symbol_counts (discrete) or sum_gd / sum_gdd (gaussian) are accumulated from
those in long double.  Trajectories whose exact likelihood is zero -- the discrete one-step tails whose column of B
is zero as doubles -- are left out: the E-step of an impossible trajectory is not what these tests are about.

The batches of a case (batches), each with one benign trajectory of BENIGN_T steps so that the plan cuts something
(the lazily scaled kernels only run on a cut plan); flags[2] is one word for the whole E-step, so one noticed
trajectory sends its whole batch to the per-step-normalising kernels, hence separate batches:
  unnoticed k  tail length k, the restated schedule reports no trouble and the exit sum lies in (0, 2^-900)
  other        every kept trajectory of neither other batch: flagged by a refresh, flushed to an exit sum of zero,
               or back in range at its end although its target is not (a refresh cut the tail in two)
  in range     the targets of sc.IN_RANGE and every control copy
  single step  (single_step_batch) beside the case list: trajectories of one step in the denormal range and nothing
               else that would be noticed"""
import functools

import numpy as np

from tests import score_range_cases as sc
from tests.ld_reference import hidden_longdouble
from tests.test_tile_matrix_gpu import _plan

L = np.longdouble
SEGLEN, WARMUP = 100, 64      # wide_segment_len and spec_W of the GPU test
BENIGN_T = 300
LEFT_OUT_CAP = 0.06
NONE = -(1 << 28)

WIDE_CASES = list(sc.WIDE_CASES)
WIDE_EXPLICIT = [(16, "explicit", 32), (64, "explicit", 32)]   # the discrete case's rows handed over as pobs
TILE_CASES = [(n, kind, M) for n in (33, 64, 65, 96, 112, 128) for kind, M in (("gaussian", 0), ("discrete", 64))]


def kmax_of(route):
    return 4 if route == "tile" else 3


def _built(route, kind, n, M):
    """the case of score_range_cases.py behind (route, kind, n, M): explicit rows are the discrete case's"""
    return sc.build(route, "discrete" if kind == "explicit" else kind, n, M)


# ---- the schedules -----------------------------------------------------------------------------------------------
def estep_run(schedule, A, pi, rows):
    """(logL or None, exit sum, trouble, exit vector) of one trajectory: see the module text.  trouble is what a
    refresh finds (a vector below 2^-900, an all-zero one); logL is None where the exit sum is zero or not finite."""
    dt = rows.dtype.type
    A, pi = A.astype(dt), pi.astype(dt)
    eP, trouble, E2, a = 0, False, NONE, None
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        for r in range(rows.shape[0]):
            a = (pi if r == 0 else a @ A) * rows[r]
            mx = a.max()
            if schedule == "wide":
                if r % 4 == 3:
                    E = sc._exp_of(mx) if mx > 0 else NONE
                    trouble |= E < sc.TROUBLE_EXP
                    if mx > 0:
                        a = np.ldexp(a, -E)
                        eP += E
            elif r % 4 == 3:
                trouble |= E2 < sc.TROUBLE_EXP
                if E2 > NONE:
                    a = np.ldexp(a, -E2)
                    eP += E2
            elif r % 4 == 2:
                E2 = sc._exp_of(mx) if mx > 0 else NONE
        S = a.sum()
        ok = S > 0 and S < np.inf
        ll = float(np.log(S.astype(L) if dt is np.float64 else S) + eP * np.log(L(2))) if ok else None
    return ll, S, bool(trouble), a


def wide_estep(A, pi, rows):
    return estep_run("wide", A, pi, rows)


def tile_estep(A, pi, rows):
    return estep_run("tile", A, pi, rows)


def careful_estep(A, pi, rows):
    """A float64 E-step that normalises every step and takes a row times 2^900 (exactly) where the row, or the sum
    formed with it, lies below 2^-959: what a correct double-precision kernel can reach.  (logL, gamma, C)"""
    T, n = rows.shape
    lift = np.zeros(T, dtype=bool)
    alpha, beta = np.empty((T, n)), np.empty((T, n))
    ll = L(0)
    with np.errstate(under="ignore"):
        for t in range(T):
            pred = pi if t == 0 else alpha[t - 1] @ A
            a = pred * rows[t]
            if not a.sum() >= sc.RESCUE_MIN and np.any(rows[t] != 0):
                lift[t] = True
                a = pred * np.ldexp(rows[t], 900)
                ll -= 900 * np.log(L(2))
            c = a.sum()
            ll += np.log(L(c))
            alpha[t] = a / c
        p = np.where(lift[:, None], np.ldexp(rows, 900), rows)
        beta[T - 1] = 1.0 / n
        C = np.zeros((n, n))
        for t in range(T - 2, -1, -1):
            x = p[t + 1] * beta[t + 1]
            if not (A @ x).sum() >= sc.RESCUE_MIN:
                x = np.ldexp(p[t + 1], 900) * beta[t + 1]
            b = A @ x
            beta[t] = b / b.sum()
            xi = alpha[t][:, None] * A * x[None, :]
            s = xi.sum()
            if not s >= sc.RESCUE_MIN:
                xi = alpha[t][:, None] * A * np.ldexp(x, 900)[None, :]
                s = xi.sum()
            C += xi / s
        g = alpha * beta
        g /= g.sum(axis=1, keepdims=True)
    return float(ll), g, C


# ---- reference and batches ---------------------------------------------------------------------------------------
class Batch:
    """obs: what set_observations takes; model: what estep takes; rows: the double-precision emission rows; ref:
    (logL, gamma, C) per trajectory in 80 bits; want: the batch's reference, shaped like _want(ref)"""


def _traj_ref(kind, model, o):
    ll, _, _, g, C = hidden_longdouble(model[0], sc.rows_exact(kind, model, o), model[1])
    return ll, g, C


def _benign(c):
    rng = np.random.default_rng(104729 + c.n)
    return rng.integers(0, sc.NB, BENIGN_T).astype(np.int32) if c.kind == "discrete" else rng.normal(0, 3, BENIGN_T)


@functools.lru_cache(maxsize=None)
def reference(route, kind, n, M):
    """Everything a case's batches are assembled from: made once, shared, never changed.  kept: the trajectories
    with a positive exact likelihood; ref / ref_ctrl / ref_benign: (logL, gamma, C) in 80 bits; ll, S, trouble: the
    restated schedule in doubles."""
    c = _built(route, kind, n, M)
    r = sc.Case()
    r.c = c
    r.kept = np.isfinite(c.ref)
    r.ref = [_traj_ref(c.kind, c.tuned, o) if k else None for o, k in zip(c.obs, r.kept)]
    r.ref_ctrl = [_traj_ref(c.kind, c.tuned, o) for o in c.ctrl]
    r.benign = _benign(c)
    r.ref_benign = _traj_ref(c.kind, c.tuned, r.benign)
    out = [estep_run(route, c.tuned[0], c.tuned[1], sc.rows_double(c.kind, c.tuned, o)) for o in c.obs]
    r.ll = np.array([np.nan if x[0] is None else x[0] for x in out])
    r.S = np.array([float(x[1]) for x in out])
    r.trouble = np.array([x[2] for x in out])
    r.last = [x[3] for x in out]
    r.unnoticed = r.kept & ~r.trouble & (r.S > 0) & (r.S < sc.RANGE_MIN)
    r.in_range = r.kept & np.isin(c.e, sc.IN_RANGE)
    r.other = r.kept & ~r.unnoticed & ~r.in_range
    return r


def _assemble(kind, c, picks):
    """picks: (observations, (logL, gamma, C)) per trajectory"""
    n = c.n
    A, pi, p0, p1 = c.tuned
    b = Batch()
    raw = [o for o, _ in picks]
    b.ref = [x for _, x in picks]
    b.lengths = [len(o) for o in raw]
    b.rows = [sc.rows_double(c.kind, c.tuned, o) for o in raw]
    b.obs = b.rows if kind == "explicit" else raw
    b.model = (A, pi, None, None) if kind == "explicit" else c.tuned
    g0, cnt, C = np.zeros(n, dtype=L), np.zeros(n, dtype=L), np.zeros((n, n), dtype=L)
    for _, g, Ck in b.ref:
        g0 += g[0].astype(L)
        cnt += g.astype(L).sum(axis=0)
        C += Ck.astype(L)
    f = np.float64
    b.want = dict(logL=np.array([x[0] for x in b.ref]), C=C.astype(f), gamma0=g0.astype(f), counts=cnt.astype(f),
                  gamma=np.concatenate([x[1] for x in b.ref]))
    if kind == "gaussian":
        sd, sdd = np.zeros(n, dtype=L), np.zeros(n, dtype=L)
        for o, (_, g, _) in zip(raw, b.ref):
            d = o.astype(L)[:, None] - p0.astype(L)[None, :]
            sd += (g.astype(L) * d).sum(axis=0)
            sdd += (g.astype(L) * d * d).sum(axis=0)
        b.want.update(sum_gd=sd.astype(f), sum_gdd=sdd.astype(f))
    elif kind == "discrete":
        sym = np.zeros((c.M, n), dtype=L)
        for o, (_, g, _) in zip(raw, b.ref):
            np.add.at(sym, o, g.astype(L))
        b.want.update(symbols=sym.T.astype(f))
    return b


def batch_names(route):
    return ["unnoticed %d" % k for k in range(1, kmax_of(route) + 1)] + ["other", "in range"]


@functools.lru_cache(maxsize=None)
def batch(route, kind, n, M, name):
    r = reference(route, "discrete" if kind == "explicit" else kind, n, M)
    c = r.c
    if name.startswith("unnoticed"):
        sel = r.unnoticed & (c.k == int(name.split()[1]))
    else:
        sel = r.other if name == "other" else r.in_range
    picks = [(c.obs[i], r.ref[i]) for i in np.flatnonzero(sel)]
    if name == "in range":
        picks += list(zip(c.ctrl, r.ref_ctrl))
    picks.append((r.benign, r.ref_benign))
    b = _assemble(kind, c, picks)
    b.index = np.flatnonzero(sel)
    return b


SINGLE_STEP = (-1000, -1023, -1040, -1060)   # none flushes pi o p to zero: nothing else gets the batch flagged


@functools.lru_cache(maxsize=None)
def single_step_batch(route, kind, n, M):
    """Trajectories of ONE step whose row lies at 2^e, e in SINGLE_STEP, and the benign one.  They are not in the
    case list (its one-step trajectories have the targets -890, -910 and -1000), and they are the trajectories the
    backward pass cannot speak for: it has no step to take, so no normaliser of its loop sees pi o p, and with every
    trajectory of the batch of this kind none gets the batch flagged for the others.
    discrete: the reserved symbol of (e, 1); gaussian: the widest state's density is 2^e exactly, as in sc.build."""
    r = reference(route, "discrete" if kind == "explicit" else kind, n, M)
    c = r.c
    if c.kind == "discrete":
        obs = [np.array([sc.reserved_symbol(e, 1)], dtype=np.int32) for e in SINGLE_STEP]
    else:
        mu, sig = c.tuned[2], c.tuned[3]
        cn = 1 / (L(sig[n - 1]) * np.sqrt(2 * L(np.pi)))
        obs = [np.array([float(L(mu[n - 1]) + L(sig[n - 1]) * np.sqrt(-2 * np.log(np.exp2(L(e)) / cn)))])
               for e in SINGLE_STEP]
    picks = [(o, _traj_ref(c.kind, c.tuned, o)) for o in obs] + [(r.benign, r.ref_benign)]
    return _assemble(kind, c, picks)


def assert_warmups_on_four(lengths):
    """the argument of the module text, on the plan these lengths get; returns the number of segments"""
    segs = _plan(lengths, SEGLEN)
    assert WARMUP % 8 == 0
    for k, t0, ln in segs:
        assert max(t0 - WARMUP, 0) % 4 == 0 and (t0 + ln == lengths[k] or (t0 + ln) % 4 == 0), (k, t0, ln)
    return len(segs)
