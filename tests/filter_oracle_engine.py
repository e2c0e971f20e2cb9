"""OracleEngine with the filter_states method of bhmm_amd.engine.Engine (TEST INFRASTRUCTURE), so that the
estimator's filter_states wiring runs without a GPU.  It counts its calls."""
import numpy as np

from oracle import oracle as orc
from tests.oracle_engine import OracleEngine


def oracle_filter(kind, obs, A, pi, par0, par1):
    """(alpha rows, log c_t) of one trajectory: orc.forward's rows, c_0 = sum pi o p_0, c_t = (alpha_{t-1} A) . p_t"""
    pobs = orc.pobs_gaussian(obs, par0, par1) if kind == 'gaussian' else orc.pobs_discrete(obs, par0)
    alpha = orc.forward(A, pobs, pi)[1]
    c = np.empty(len(pobs))
    c[0] = np.dot(np.asarray(pi, dtype=np.float64), pobs[0])
    c[1:] = np.einsum('tj,tj->t', alpha[:-1] @ np.asarray(A, dtype=np.float64), pobs[1:])
    with np.errstate(divide='ignore'):
        return alpha, np.log(c)


class FilterOracleEngine(OracleEngine):
    def __init__(self, device=0):
        OracleEngine.__init__(self, device)
        self.filter_calls = []

    def filter_states(self, A, pi, par0=None, par1=None, weights=None, dtype=np.float64, probabilities=True,
                      increments=True, out=None, out_increments=None):
        self.filter_calls.append(tuple(None if x is None else np.array(x) for x in (A, pi, par0, par1)))
        res = [oracle_filter(self.kind, o, A, pi, par0, par1) for o in self.obs]
        rows = [a for a, _ in res]
        if weights is not None:
            rows = [a @ np.asarray(weights, dtype=np.float64) for a in rows]
        return ([r.astype(dtype) for r in rows] if probabilities else None,
                [l.astype(dtype) for _, l in res] if increments else None)
