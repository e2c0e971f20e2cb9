"""Test infrastructure for the number-range tests of bhmm_score (test_score_range_cpu.py, test_score_range_gpu.py):
trajectories whose last k steps are all but impossible under every state of a tuned model, an exact reference in
80-bit arithmetic, and a restatement of the two lazy scaling schedules (k_score_wide<.., LAZY>, k_score_tile) in
the arithmetic of the caller's choice.

A case is one (route, kind, n, M).  Its trajectories are (target e, tail k, length T): T - k benign steps, then k
steps that together scale the forward vector by about 2^e.
  discrete  symbols 0 and 1 are benign (the tuned model gives them about half of every row of B each, so a benign
            step scales the vector by about 1/2); every (e, k) has a reserved symbol whose column of B is
            2^(e / k) times a per-state factor in [0.5, 1] -- as a double, so a column below 2^-1074 is zero.
  gaussian  one state is the widest (sigma = 2) and has the largest mean, so beyond it it outweighs every other;
            a tail observation lies at the distance from its mean at which its density is the wanted factor.
            The factor of the first tail step also takes off what the lazily scaled vector has lost since its
            last refresh, so that the exit sum of a tail that no refresh cuts is 2^e within a bit or two (times
            a random factor in [0.55, 1): a power of two is exact on any grid).  For k = 1 below 2^-959, where
            the row is in the denormal range itself and the lane-group kernel's rescue rule takes over, the
            density is 2^e as it stands.
Every trajectory has a control copy with a benign tail."""
import functools

import numpy as np

L = np.longdouble
TARGETS = (-700, -890, -910, -1000, -1023, -1040, -1060, -1073, -1080, -1200)
IN_RANGE = (-700, -890)                       # the guard must not fire on these
SHORT = tuple(range(1, 12))                   # every residue mod 4, with and without a refresh, from the start
LONG = ((37, 2), (64, 2), (129, 1), (262, 1))  # (length, targets that take it) per tail length
_HOT = (-1060, -1040, -1073, -1023, -1000, -910, -1080, -1200, -890, -700)
NB = 2                                        # benign symbols
TROUBLE_EXP = -900                            # WIDE_TROUBLE_EXP
RANGE_MIN = np.ldexp(1.0, TROUBLE_EXP)
RESCUE_MIN = np.ldexp(1.0, -959)              # the rescue rule of wide_emit


def case_list(kmax):
    """(e, k, T) of every trajectory: each (k, short length) under three targets, each (k, long length) under one
    or two; every target meets every tail length."""
    out = []
    for k in range(1, kmax + 1):
        for c, T in enumerate(t for t in SHORT if t >= k):
            out += [(TARGETS[(3 * c + m + k) % len(TARGETS)], k, T) for m in range(3)]
    i = 0
    for k in range(1, kmax + 1):
        for T, cnt in LONG:
            for _ in range(cnt):
                out.append((_HOT[i % len(_HOT)], k, T))
                i += 1
    return out


def reserved_symbol(e, k):
    return NB + (k - 1) * len(TARGETS) + TARGETS.index(e)


def rand_A(n, rng):
    A = rng.random((n, n)) + 0.05
    return A / A.sum(axis=1)[:, None]


def rand_model(kind, n, M, rng):
    pi = rng.random(n) + 0.1
    pi /= pi.sum()
    if kind == "gaussian":
        return (rand_A(n, rng), pi, np.sort(rng.normal(0, 3, n)), rng.uniform(0.5, 2.0, n))
    B = rng.random((n, M)) + 0.01
    return (rand_A(n, rng), pi, B / B.sum(axis=1)[:, None], None)


# ---- emission rows ---------------------------------------------------------------------------------
def rows_exact(kind, model, obs):
    """(T, n) emission probabilities in 80-bit arithmetic, formed from the parameters.  Gaussian: the log-density,
    then exp; a row whose densities are all zero as doubles is a row of ones (the model's outlier rule).
    Discrete: the entries of B as given."""
    _, _, p0, p1 = model
    if kind == "discrete":
        return p0.astype(L)[:, np.asarray(obs)].T.copy()
    mu, sig = p0.astype(L), p1.astype(L)
    z = (np.asarray(obs, dtype=np.float64).astype(L)[:, None] - mu[None, :]) / sig[None, :]
    p = np.exp(-np.log(sig * np.sqrt(2 * L(np.pi)))[None, :] - z * z / 2)
    with np.errstate(under="ignore"):
        dead = np.all(p.astype(np.float64) == 0.0, axis=1)
    p[dead] = 1
    return p


def rows_double(kind, model, obs):
    """The same rows the way the kernels form them, in doubles (gaussian: cnorm * exp(-z^2 / 2))."""
    _, _, p0, p1 = model
    if kind == "discrete":
        return p0[:, np.asarray(obs)].T.copy()
    with np.errstate(under="ignore", over="ignore"):
        z = (np.asarray(obs, dtype=np.float64)[:, None] - p0[None, :]) / p1[None, :]
        p = 1.0 / (np.sqrt(2.0 * np.pi) * p1)[None, :] * np.exp(-0.5 * z * z)
    p[np.all(p == 0.0, axis=1)] = 1.0
    return p


# ---- the exact recursion ---------------------------------------------------------------------------
def loglik_exact(A, pi, rows):
    """Forward recursion in 80-bit arithmetic, normalised every step; the sum of the logs as a float."""
    A, pi = A.astype(L), pi.astype(L)
    ll = L(0)
    a = None
    for t in range(rows.shape[0]):
        a = (pi if t == 0 else a @ A) * rows[t]
        c = a.sum()
        if not c > 0:
            return -np.inf
        ll += np.log(c)
        a = a / c
    return float(ll)


# ---- the lazy schedules ----------------------------------------------------------------------------
def _exp_of(x):
    return int(np.frexp(x)[1])


def lazy_run(schedule, A, pi, rows):
    """One trajectory, one segment from its start, in the arithmetic of `rows` (double: what the kernels compute;
    long double: what they would without a number range).  Returns (logL or None, exit sum, trouble, exit vector):
    trouble is what the kernels find at a refresh (a vector below 2^-900, an all-zero one), logL is None where
    the exit sum is zero or not finite.  Neither looks at the size of the exit sum otherwise.
      wide  k_score_wide<.., LAZY>: the exponent is measured and taken off on steps r % 4 == 3; a row in the
            denormal range is taken times 2^900 first (the rescue rule)
      tile  k_score_tile: measured after steps r % 4 == 2, taken off on steps r % 4 == 3"""
    dt = rows.dtype.type
    A, pi = A.astype(dt), pi.astype(dt)
    eP, trouble, E2, a = 0, False, 0, None
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        for r in range(rows.shape[0]):
            p = rows[r]
            if schedule == "wide" and np.all(p < RESCUE_MIN) and np.any(p != 0):
                p = np.ldexp(p, 900)
                eP -= 900
            a = (pi if r == 0 else a @ A) * p
            mx = a.max()
            if schedule == "wide":
                if r % 4 == 3:
                    E = _exp_of(mx) if mx > 0 else -(1 << 28)
                    trouble |= E < TROUBLE_EXP
                    if mx > 0:
                        a = np.ldexp(a, -E)
                        eP += E
            else:
                if r % 4 == 3:
                    trouble |= E2 < TROUBLE_EXP
                    if E2 > -(1 << 28):
                        a = np.ldexp(a, -E2)
                        eP += E2
                elif r % 4 == 2:
                    E2 = _exp_of(mx) if mx > 0 else -(1 << 28)
        S = a.sum()
        ok = S > 0 and S < np.inf
        ll = float(np.log(S.astype(L) if dt is np.float64 else S) + eP * np.log(L(2))) if ok else None
    return ll, S, bool(trouble), a


# ---- cases -----------------------------------------------------------------------------------------
class Case:
    pass


@functools.lru_cache(maxsize=None)
def build(route, kind, n, M):
    """The inputs of one case and the exact log-likelihoods of the tuned model: made once, shared, never changed."""
    kmax = 4 if route == "tile" else 3
    rng = np.random.default_rng(7919 * n + 31 * M + kmax)
    c = Case()
    c.route, c.kind, c.n, c.M, c.kmax = route, kind, n, M, kmax
    c.cases = case_list(kmax)
    A = rand_A(n, rng)
    pi = rng.random(n) + 0.1
    pi /= pi.sum()
    if kind == "gaussian":
        mu, sig = np.sort(rng.normal(0, 3, n)), rng.uniform(0.5, 2.0, n)
        w = n - 1   # the widest state has the largest mean too: beyond it, it outweighs every other state
        sig[w] = 2.0
        c.tuned = (A, pi, mu, sig)
    else:
        assert M >= NB + kmax * len(TARGETS)
        B = np.zeros((n, M))
        B[:, :NB] = rng.uniform(0.3, 0.7, (n, NB))
        if M > NB + kmax * len(TARGETS):   # symbols no trajectory uses: two percent of every row
            rest = rng.random((n, M - NB - kmax * len(TARGETS))) + 0.01
            B[:, NB + kmax * len(TARGETS):] = 0.02 * rest / rest.sum(axis=1)[:, None] * B[:, :NB].sum(axis=1)[:, None]
        B /= B.sum(axis=1)[:, None]
        with np.errstate(under="ignore"):
            for k in range(1, kmax + 1):
                for e in TARGETS:   # (far below an ulp of 1: the rows still sum to 1)
                    B[:, reserved_symbol(e, k)] = np.exp2(e / k) * rng.uniform(0.5, 1.0, n)
        c.tuned = (A, pi, B, None)
    c.others = [rand_model(kind, n, M, rng) for _ in range(2)]
    c.obs, c.ctrl = [], []
    for e, k, T in c.cases:
        if kind == "discrete":
            pre = rng.integers(0, NB, T - k).astype(np.int32)
            c.obs.append(np.concatenate([pre, np.full(k, reserved_symbol(e, k), dtype=np.int32)]))
            c.ctrl.append(np.concatenate([pre, rng.integers(0, NB, k).astype(np.int32)]))
            continue
        pre = rng.normal(0, 3, T - k)
        f = np.exp2(L(e) / k)
        if k == 1 and e < -959:
            pw = [f]
        else:
            f *= L(rng.uniform(0.55, 1.0))   # (off the powers of two: an exit sum of 2^e is exact on any grid)
            Aw = A.astype(L)
            pred = L(pi[w]) if T == k else (lazy_run(route, A, pi, rows_exact(kind, c.tuned, pre))[3] @ Aw)[w]
            pw = [f / pred] + [f / Aw[w, w]] * (k - 1)
        cn = 1 / (L(sig[w]) * np.sqrt(2 * L(np.pi)))
        tail = [float(L(mu[w]) + L(sig[w]) * np.sqrt(-2 * np.log(p / cn))) for p in pw]
        c.obs.append(np.concatenate([pre, tail]))
        c.ctrl.append(np.concatenate([pre, rng.normal(0, 3, k)]))
    A_, pi_ = c.tuned[0], c.tuned[1]
    c.ref = np.array([loglik_exact(A_, pi_, rows_exact(kind, c.tuned, o)) for o in c.obs])
    c.ref_ctrl = np.array([loglik_exact(A_, pi_, rows_exact(kind, c.tuned, o)) for o in c.ctrl])
    c.e = np.array([x[0] for x in c.cases])
    c.k = np.array([x[1] for x in c.cases])
    c.T = np.array([x[2] for x in c.cases])
    return c


@functools.lru_cache(maxsize=None)
def restated(route, kind, n, M):
    """lazy_run in doubles over the case's trajectories: (logL or nan, exit sum, trouble) per trajectory."""
    c = build(route, kind, n, M)
    out = [lazy_run(route, c.tuned[0], c.tuned[1], rows_double(kind, c.tuned, o))[:3] for o in c.obs]
    return (np.array([np.nan if x[0] is None else x[0] for x in out]), np.array([float(x[1]) for x in out]),
            np.array([x[2] for x in out]))


WIDE_CASES = [(n, kind, M) for n in (9, 16, 17, 33, 64)
              for kind, M in (("gaussian", 0), ("discrete", 32), ("discrete", 1000))]
TILE_CASES = [(n, kind, M) for n in (65, 96, 112, 128) for kind, M in (("gaussian", 0), ("discrete", 64))]
