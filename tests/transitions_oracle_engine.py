"""Pair posteriors from the CPU oracle, and MarginalsOracleEngine with the posterior_transitions method of
bhmm_amd.engine.Engine (TEST INFRASTRUCTURE), so that bhmm_amd.posterior_transitions, hidden.posterior_transitions
and the estimator's method run without a GPU.  The engine double counts its calls."""
import numpy as np

from oracle import oracle as orc
from tests.marginals_oracle_engine import MarginalsOracleEngine


def jump_mask(n):
    """(n, n, 1): the off-diagonal 0/1 mask whose projection is the jump form"""
    return (1.0 - np.eye(n))[:, :, None]


def pobs_of(kind, o, par0, par1):
    if kind == "gaussian":
        return orc.pobs_gaussian(o, par0, par1)
    if kind == "discrete":
        return orc.pobs_discrete(o, par0)
    return np.asarray(o, dtype=np.float64)


def oracle_rows(kind, obs, model, weights=None):
    """per trajectory (rows, absrows): the projection of xi_t on `weights` ((n, n, Q); None: the jump mask) and on
    |weights| (the relative part of the tolerance), both (T_k - 1, Q).  xi_t of the pair (t, t + 1) from orc.forward
    / orc.backward alone: x_t = alpha_t[:, None] * A * (pobs_(t+1) * beta_(t+1))[None, :], normalised per step, in
    numpy fp64"""
    A, pi, par0, par1 = model
    n = np.shape(A)[0]
    W = jump_mask(n) if weights is None else np.asarray(weights, dtype=np.float64)
    Wf, Wa = W.reshape(n * n, -1), np.abs(W).reshape(n * n, -1)
    out = []
    for o in obs:
        pobs = pobs_of(kind, o, par0, par1)
        alpha = orc.forward(A, pobs, pi)[1]
        pb = pobs * orc.backward(A, pobs)
        T = len(pobs)
        rows, absrows = np.zeros((T - 1, Wf.shape[1])), np.zeros((T - 1, Wf.shape[1]))
        step = max(1, (1 << 22) // (n * n))           # (blocks of steps: xi of a long trajectory is large)
        for t0 in range(0, T - 1, step):
            t1 = min(T - 1, t0 + step)
            x = alpha[t0:t1, :, None] * np.asarray(A, dtype=np.float64)[None, :, :] * pb[t0 + 1:t1 + 1, None, :]
            x /= x.sum(axis=(1, 2), keepdims=True)
            x = x.reshape(t1 - t0, n * n)
            rows[t0:t1], absrows[t0:t1] = x @ Wf, x @ Wa
        out.append((rows, absrows))
    return out


class TransitionsOracleEngine(MarginalsOracleEngine):
    def __init__(self, device=0):
        MarginalsOracleEngine.__init__(self, device)
        self.transition_calls = []

    def close(self):
        pass

    def posterior_transitions(self, A, pi, par0=None, par1=None, weights=None, dtype=np.float64, out=None):
        self.transition_calls.append(tuple(None if x is None else np.array(x) for x in (A, pi, par0, par1)))
        rows = [r for r, _ in oracle_rows(self.kind, self.obs, (A, pi, par0, par1), weights)]
        if weights is None:
            rows = [r[:, 0] for r in rows]
        return [r.astype(dtype) for r in rows]
