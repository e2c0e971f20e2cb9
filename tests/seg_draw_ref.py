"""Plain restatement of the segment-parallel backward draw's protocol (TEST INFRASTRUCTURE): the segment plan of
plan::plan_segments(.., mult = 1), pass 0 / check / fix-up rounds as the comment block above k_wide_sample_seg
(csrc/path_kernels.hpp) states them and seg_draw (csrc/path_api.hip) drives them, and plan::draw_next_warmup.
numpy only; never imports the package.  Every draw is decided with the reference's arithmetic (_hidden.c:283-305:
_normalize by an ascending sum, then the first state whose sequential cumulative sum reaches u) -- np.cumsum adds
in index order, so cumsum(x)[-1] is that ascending sum.  The segments of one pass touch only their own slots
(s_entry, s_exit, their steps of the path), so the emulation steps all of them together, one row per segment."""
import collections

import numpy as np

W_START, W_MAX, MAX_ROUNDS = 64, 4096, 16

Emulation = collections.namedtuple("Emulation", [
    "paths",        # per trajectory, int32; the serial draw's where `accepted`
    "nseg",         # segments of the plan
    "flagged",      # indices of the segments the check after pass 0 flagged (their count: sample_mismatch)
    "rounds",       # the round whose check found nothing; max_rounds + 1: they ran out (sample_rounds)
    "reached",      # fix-up runs that drew their first step without meeting the path (they wrote a new s_exit)
    "met_inside",   # fix-up runs that met the path above their first step
    "min_gap",      # min over every draw performed (warm-ups and abandoned runs too) of min_q |acc_q - u|
    "accepted",     # a check found nothing within max_rounds
    "flags",        # per round (0 = after pass 0), the boolean flag vector its check left
    "reached_segs",  # segments with a fix-up run counted in `reached`
    "no_state",     # a draw of a segment's own steps found no state (the device raises its status word)
])


def plan(lengths, seglen):
    """[(trajectory, t0, len)]: ns = ceil(T / seglen) segments per trajectory, boundaries at (q T // ns) & ~3, the
    last one at T, empty segments skipped."""
    out = []
    for k, T in enumerate(lengths):
        T = int(T)
        if T <= 0:
            continue
        ns = (T + seglen - 1) // seglen if seglen > 0 else 1
        prev = 0
        for q in range(1, ns + 1):
            b = T if q == ns else ((q * T) // ns) & ~3
            if b <= prev:
                continue
            out.append((k, prev, b - prev))
            prev = b
    return out


def next_w(W, mismatch, nseg):
    """plan::draw_next_warmup: the next call's warm-up doubles while more than a tenth of the segments were flagged."""
    return 2 * W if mismatch * 10 > nseg and W < W_MAX else W


def draw(ps, u):
    """One draw (_hidden.c:283-305) on the weights ps with the uniform u: (state or len(ps) if none, decisive gap)."""
    S = np.cumsum(ps)[-1]                 # _normalize, ascending
    acc = np.cumsum(ps / S)
    hit = np.nonzero(acc >= u)[0]
    return (int(hit[0]) if hit.size else len(ps)), float(np.abs(acc - u).min())


def serial(alpha, A, u):
    """The serial backward draw of one trajectory (_hidden.c:330-378) with draw()."""
    T, n = alpha.shape
    path = np.empty(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        ps = alpha[t] if t == T - 1 else alpha[t] * A[:, path[t + 1]]
        path[t] = min(draw(ps, u[t])[0], n - 1)
    return path


def _draw_rows(ps, u):
    """draw() for one row per segment: ps (m, n), u (m,) -> (states (m,), n where none; gaps (m,))."""
    S = np.cumsum(ps, axis=1)[:, -1]
    acc = np.cumsum(ps / S[:, None], axis=1)
    ge = acc >= u[:, None]
    pick = np.where(ge.any(axis=1), ge.argmax(axis=1), ps.shape[1])
    return pick, np.abs(acc - u[:, None]).min(axis=1)


def emulate(alphas, A, us, lengths, W, max_rounds=MAX_ROUNDS, seglen=64, replace_entry=True):
    """Pass 0, the check and the fix-up rounds on the rows `alphas` (per trajectory, (T, n)) and uniforms `us`.
    replace_entry = False is a deliberately WRONG protocol (the check flags but leaves s_entry): tests use it to
    show that the comparison with the serial draw can fail."""
    lengths = [int(T) for T in lengths]
    n = A.shape[0]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    alpha = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1, n) for a in alphas])
    u = np.concatenate([np.asarray(x, dtype=np.float64) for x in us])
    A = np.asarray(A, dtype=np.float64)
    segs = plan(lengths, seglen)
    nseg = len(segs)
    traj = np.array([s[0] for s in segs], dtype=np.int64)
    t0 = np.array([s[1] for s in segs], dtype=np.int64)
    t1 = t0 + np.array([s[2] for s in segs], dtype=np.int64)
    o0, T = off[traj], off[traj + 1] - off[traj]
    path = np.full(off[-1], -1, dtype=np.int32)
    s_entry = np.full(nseg, -1, dtype=np.int64)
    s_exit = np.full(nseg, -1, dtype=np.int64)
    min_gap, no_state = np.inf, False

    def run(idx, ts, nxt, fix):
        """The segments idx from step ts down to their first; returns (last state drawn, met, step it met at)."""
        nonlocal min_gap, no_state
        nxt = nxt.copy()
        met = np.zeros(len(idx), dtype=bool)
        met_t = np.full(len(idx), -1, dtype=np.int64)
        for c in range(int((ts - t0[idx]).max()) + 1):
            t = ts - c
            on = np.nonzero((t >= t0[idx]) & ~met)[0]
            if on.size == 0:
                break
            s, tt = idx[on], t[on]
            a = alpha[o0[s] + tt]
            ps = np.where((tt == T[s] - 1)[:, None], a, a * A[:, nxt[on]].T)      # _hidden.c:349 / :365
            pick, gap = _draw_rows(ps, u[o0[s] + tt])
            min_gap = min(min_gap, float(gap.min()))
            own = tt < t1[s]
            no_state |= bool(((pick >= n) & own).any())
            pick = np.minimum(pick, n - 1)
            nxt[on] = pick
            if not fix:
                above = tt == t1[s]
                s_entry[s[above]] = pick[above]          # the state drawn for the step above the segment
            else:
                m = own & (path[o0[s] + tt] == pick)     # the path already holds it: nothing changes below
                met[on[m]] = True
                met_t[on[m]] = tt[m]
                own = own & ~m
            path[o0[s[own]] + tt[own]] = pick[own]
        return nxt, met, met_t

    def check():
        flag = np.zeros(nseg, dtype=bool)
        for s in range(nseg - 1):
            if traj[s + 1] == traj[s] and s_entry[s] != s_exit[s + 1]:
                flag[s] = True
                if replace_entry:
                    s_entry[s] = s_exit[s + 1]
        return flag

    every = np.arange(nseg)
    s_exit[:], _, _ = run(every, np.minimum(t1 + W, T) - 1, np.zeros(nseg, dtype=np.int64), False)
    flags = [check()]
    reached, met_inside, reached_segs = 0, 0, set()
    rounds = 0
    while flags[-1].any():
        rounds += 1
        if rounds > max_rounds:
            break
        idx = np.nonzero(flags[-1])[0]
        last, met, met_t = run(idx, t1[idx] - 1, s_entry[idx], True)
        s_exit[idx[~met]] = last[~met]
        reached += int((~met).sum())
        reached_segs.update(int(s) for s in idx[~met])
        met_inside += int((met & (met_t > t0[idx])).sum())
        flags.append(check())
    return Emulation([path[off[k]:off[k + 1]].copy() for k in range(len(lengths))], nseg, np.nonzero(flags[0])[0],
                     rounds, reached, met_inside, min_gap, rounds <= max_rounds, flags, reached_segs, no_state)
