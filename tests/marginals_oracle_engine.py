"""OracleEngine with the posterior_marginals method of bhmm_amd.engine.Engine (TEST INFRASTRUCTURE), so that the
estimator's hidden_state_probabilities / posterior_marginals wiring runs without a GPU.  It counts its calls."""
import numpy as np

from oracle import oracle as orc
from tests.oracle_engine import OracleEngine


class MarginalsOracleEngine(OracleEngine):
    def __init__(self, device=0):
        OracleEngine.__init__(self, device)
        self.marginal_calls = []

    def posterior_marginals(self, A, pi, par0=None, par1=None, weights=None, dtype=np.float64, out=None):
        self.marginal_calls.append(tuple(None if x is None else np.array(x) for x in (A, pi, par0, par1)))
        g = orc.estep(self.kind, self.obs, A, pi, par0, par1, want_gamma=True)['gammas']
        if weights is not None:
            g = [x @ np.asarray(weights, dtype=np.float64) for x in g]
        return [x.astype(dtype) for x in g]
