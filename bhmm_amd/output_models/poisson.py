"""Poisson emission model for counts: D channels, one rate >= 0 per hidden state and channel, the channels
independent given the state:

    log b_i(x) = sum_d [x_d log lambda_id - lambda_id - log(x_d !)]

Inside the batched calls the densities are made on the device from the counts kept there (PoissonEngine,
bhmm_pois_emissions) and this class is not involved; `log_p_obs` / `p_obs` are the numpy restatement of the complete
density for one array of counts, `estimate_from_packed` is the M-step on the moments the device returns
(bhmm_host_pois_mstep).  The generators run in numpy.
"""
import math

import numpy as np

from .. import _lib
from .outputmodel import OutputModel

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def check_observation(o, D=None):
    """One trajectory of counts as a C-contiguous float64 (T, D) array.  Integer or float arrays are taken; a value
    that is negative or not an integer is refused (NaN passes: it makes its trajectory NaN)."""
    o = np.asarray(o)
    if not (np.issubdtype(o.dtype, np.integer) or np.issubdtype(o.dtype, np.floating) or o.dtype == np.bool_):
        raise ValueError("counts must be integer or float arrays, not %s" % o.dtype.name)
    if o.ndim != 2 or (D is not None and o.shape[1] != D):
        raise ValueError("count observations must be (T, %s) arrays, not %r" % ('D' if D is None else D, o.shape))
    x = np.ascontiguousarray(o, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        if np.any(x < 0.0):
            raise ValueError("counts must not be negative")
        if np.any((x != np.floor(x)) & ~np.isnan(x)) or np.any(np.isinf(x)):
            raise ValueError("counts must be integers")
    return x


class PoissonOutputModel(OutputModel):
    def __init__(self, nstates, rates):
        OutputModel.__init__(self, nstates, ignore_outliers=False)
        self._rates = self._checked(rates, None)
        self._D = int(self._rates.shape[1])

    def _checked(self, rates, D):
        r = np.array(rates, dtype=np.float64)
        if r.ndim != 2 or r.shape[0] != self.nstates or r.shape[1] < 1 or (D is not None and r.shape[1] != D):
            raise ValueError('rates must have shape (nstates, D)')
        if r.shape[1] > _lib.MVN_MAX_D:
            raise ValueError('at most %d channels are supported, not %d' % (_lib.MVN_MAX_D, r.shape[1]))
        if not np.all(np.isfinite(r)) or np.any(r < 0.0):
            raise ValueError('rates must be finite and not negative')
        return r

    def __repr__(self):
        return 'PoissonOutputModel(%d, rates=%r)' % (self.nstates, self._rates)

    @property
    def model_type(self):
        return 'poisson'

    @property
    def dimension(self):
        return self._D

    @property
    def rates(self):
        return self._rates

    def parameters(self):
        """(par0, par1) as PoissonEngine takes them: rates (N, D), None."""
        return self._rates, None

    def set_parameters(self, rates, par1=None):
        self._rates = self._checked(np.asarray(rates, dtype=np.float64).reshape(self.nstates, self._D), self._D)

    def sub_output_model(self, states):
        states = np.asarray(states, dtype=np.int64)
        return PoissonOutputModel(len(states), self._rates[states])

    def log_p_obs(self, obs, out=None):
        """(T, N) matrix of the complete log-density, in numpy: a zero count under any rate contributes
        -lambda alone (also under rate 0: the term 0 log 0 is 0), a positive count under rate 0 gives -inf."""
        x = check_observation(obs, self._D)
        T, N = x.shape[0], self.nstates
        with np.errstate(divide='ignore'):
            loglam = np.log(self._rates)
        res = np.empty((T, N))
        cst = -_lgamma(x + 1.0).sum(axis=1) if T else np.zeros(0)
        for i in range(N):
            with np.errstate(invalid='ignore'):
                term = np.where(x == 0.0, 0.0, x * loglam[i][None, :])
            res[:, i] = term.sum(axis=1) - self._rates[i].sum() + cst
        if out is None:
            return res
        out[:T] = res
        return out

    def p_obs(self, obs, out=None):
        """The densities themselves: exp(log_p_obs)."""
        lp = self.log_p_obs(obs, out=out)
        return np.exp(lp, out=lp)

    def estimate_from_statistics(self, S0, S1, S2=None):
        """M-step from the moments about the current rates: S0 (N,) = sum_t gamma, S1 (N, D) = sum_t gamma
        (x - lambda_old); the new rate is max(0, lambda_old + S1 / S0), a state without weight keeps its rates."""
        N, D = self.nstates, self._D
        S0, S1 = np.asarray(S0, dtype=np.float64), np.asarray(S1, dtype=np.float64)
        if S0.shape != (N,) or S1.shape != (N, D):
            raise ValueError('moments must have shapes (%d,) and (%d, %d)' % (N, N, D))
        packed = np.zeros((N, 1 + 2 * D))
        packed[:, 0] = S0
        packed[:, 1:1 + D] = S1
        self.estimate_from_packed(packed.ravel())

    def estimate_from_packed(self, moments):
        """The same from the packed layout of bhmm_mvn_moments with diagonal second moments (which are not read)."""
        N, D = self.nstates, self._D
        moments = _lib.f64(moments)
        if moments.shape != (N * (1 + 2 * D),):
            raise ValueError('packed moments must hold %d doubles' % (N * (1 + 2 * D)))
        new = np.empty((N, D))
        _lib.check(_lib.load().bhmm_host_pois_mstep(N, D, _lib.dp(moments), _lib.dp(_lib.f64(self._rates)),
                                                    _lib.dp(new)))
        self._rates = new

    def generate_observation_from_state(self, state_index, rng=np.random):
        return rng.poisson(self._rates[state_index]).astype(np.int64)

    def generate_observations_from_state(self, state_index, nobs, rng=np.random):
        return rng.poisson(self._rates[state_index], size=(nobs, self._D)).astype(np.int64)

    def generate_observation_trajectory(self, s_t, rng=np.random):
        s_t = np.asarray(s_t)
        out = np.empty((s_t.shape[0], self._D), dtype=np.int64)
        for i in range(self.nstates):
            idx = np.where(s_t == i)[0]
            if idx.size:
                out[idx] = self.generate_observations_from_state(i, idx.size, rng=rng)
        return out
