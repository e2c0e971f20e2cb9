"""Host-side model updates as ONE native call each (include/bhmm_amd.h, section 3): the whole
M-step of an EM iteration (maximum_likelihood.py:284-330) and the parameter draws of a Gibbs
sweep (bayesian_sampling.py:333-373).  Host code of the shared library, no device work; the
numpy functions in _tmatrix.py are the restatements these are tested against.
"""
import ctypes

import numpy as np

from .. import _lib

_KIND = {'gaussian': _lib.EMIT_GAUSSIAN, 'discrete': _lib.EMIT_DISCRETE, 'explicit': _lib.EMIT_EXPLICIT}


def _addr(a):
    """Address of a C-contiguous float64 array as a ctypes pointer, without numpy's `.ctypes`
    helper object (5 us per use; these calls run once per EM iteration / Gibbs sweep)."""
    if a is None:
        return None
    return ctypes.cast(a.__array_interface__['data'][0], _lib.c_double_p)


def _c64(a):
    if isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous:
        return a
    return np.ascontiguousarray(a, dtype=np.float64)


class MStep(object):
    """Persistent argument block of bhmm_mstep for one estimator (buffers and ctypes pointers are
    made once: the call itself must stay in the tens of microseconds)."""

    def __init__(self, kind, n, M=0):
        self._L = _lib.load()
        self._fn = self._L.bhmm_mstep
        self.kind, self.n, self.M = kind, int(n), int(M)
        self._code = _KIND[kind]
        self.T = np.empty((n, n))
        self.pi = np.empty(n)
        if kind == 'gaussian':
            self.par0, self.par1 = np.empty(n), np.empty(n)
        elif kind == 'discrete':
            self.par0, self.par1 = np.empty((n, M)), None
        else:
            self.par0 = self.par1 = None
        self.info = np.zeros(2, dtype=np.int32)
        self.warm = np.zeros(1 + n)       # state of the reversible fixed point, carried along
        self._out = (_addr(self.T), _addr(self.pi), _addr(self.par0), _addr(self.par1),
                     _lib.ip(self.info), _addr(self.warm))

    def __call__(self, packed, T_old, par0_old, par1_old, reversible, stationary, fixed_pi,
                 maxiter, maxerr, mincount):
        """reversible: True / False / None (= 'iff T_old is reversible', what the reference's
        self._hmm.is_reversible evaluates to).  Returns fresh copies (T, pi, par0, par1)."""
        packed = _c64(packed)
        rev = -1 if reversible is None else int(bool(reversible))
        fp = _c64(fixed_pi) if fixed_pi is not None else None
        T_old = _c64(T_old)
        p0o = _c64(par0_old) if par0_old is not None else None
        p1o = _c64(par1_old) if par1_old is not None else None
        _lib.check(self._fn(self._code, self.n, self.M, _addr(packed), _addr(T_old), _addr(p0o),
                            _addr(p1o), rev, int(bool(stationary)), _addr(fp), int(maxiter),
                            float(maxerr), float(mincount), *self._out))
        return (self.T.copy(), self.pi.copy(),
                None if self.par0 is None else self.par0.copy(),
                None if self.par1 is None else self.par1.copy())


class GibbsParameters(object):
    """Persistent argument block of bhmm_gibbs_parameters for one sampler."""

    def __init__(self, kind, n, M=0, prior_C=None, prior_n0=None, prior_B=None, reversible=True,
                 stationary=False, nsteps=1000):
        self._L = _lib.load()
        self._fn = self._L.bhmm_gibbs_parameters
        self.kind, self.n, self.M = kind, int(n), int(M)
        self._code = _KIND[kind]
        self.prior_C = _lib.f64(prior_C) if prior_C is not None else None
        self.prior_n0 = _lib.f64(prior_n0) if prior_n0 is not None else None
        self.prior_B = _lib.f64(prior_B) if prior_B is not None else None
        self.reversible, self.stationary, self.nsteps = bool(reversible), bool(stationary), int(nsteps)
        self.T = np.empty((n, n))
        self.p0 = np.empty(n)
        self.info = np.zeros(1, dtype=np.int32)
        self._priors = (_addr(self.prior_C), _addr(self.prior_n0), _addr(self.prior_B))
        self._out = (_addr(self.T), _addr(self.p0))
        self._info = _lib.ip(self.info)

    def __call__(self, packed_path_stats, par0, par1, seed, sweep):
        """par0 / par1: current emission parameters (copied, then updated in the copies).
        Returns (T, p0, par0_new, par1_new)."""
        packed = _c64(packed_path_stats)
        p0n = np.array(par0, dtype=np.float64) if par0 is not None else None
        p1n = np.array(par1, dtype=np.float64) if par1 is not None else None
        _lib.check(self._fn(self._code, self.n, self.M, _addr(packed), *self._priors,
                            int(self.reversible), int(self.stationary), self.nsteps,
                            int(seed) & 0xFFFFFFFFFFFFFFFF, int(sweep), *self._out, _addr(p0n),
                            _addr(p1n), self._info))
        return self.T.copy(), self.p0.copy(), p0n, p1n


class GibbsParametersMvn(object):
    """Persistent argument block of bhmm_gibbs_parameters_mvn for one sampler (multivariate gaussian emissions)."""

    def __init__(self, n, D, covariance_type='full', prior_C=None, prior_n0=None, reversible=True,
                 stationary=False, nsteps=1000):
        if covariance_type not in ('full', 'diag'):
            raise ValueError("covariance_type must be 'full' or 'diag', not %r" % (covariance_type,))
        self._L = _lib.load()
        self._fn = self._L.bhmm_gibbs_parameters_mvn
        self.n, self.D, self.covariance_type = int(n), int(D), covariance_type
        self._code = _lib.COV_FULL if covariance_type == 'full' else _lib.COV_DIAG
        self.prior_C = _lib.f64(prior_C) if prior_C is not None else None
        self.prior_n0 = _lib.f64(prior_n0) if prior_n0 is not None else None
        self.reversible, self.stationary, self.nsteps = bool(reversible), bool(stationary), int(nsteps)
        self.T = np.empty((n, n))
        self.p0 = np.empty(n)
        self.info = np.zeros(2, dtype=np.int32)   # draws consumed, states whose covariance was kept
        self._priors = (_addr(self.prior_C), _addr(self.prior_n0))
        self._out = (_addr(self.T), _addr(self.p0))
        self._info = _lib.ip(self.info)

    def __call__(self, packed_path_stats, means, covariances, seed, sweep):
        """packed_path_stats: [C n*n | n0 n | packed moments about `means`]; means / covariances: the current
        parameters (copied, then updated in the copies).  Returns (T, p0, means_new, covariances_new)."""
        n, D = self.n, self.D
        packed = _c64(packed_path_stats)
        stride = 1 + D + (D * (D + 1) // 2 if self.covariance_type == 'full' else D)
        if packed.shape != (n * n + n + n * stride,):
            raise ValueError("packed path statistics must hold %d doubles" % (n * n + n + n * stride))
        mu = np.array(means, dtype=np.float64)
        cov = np.array(covariances, dtype=np.float64)
        if mu.shape != (n, D) or cov.shape != ((n, D, D) if self.covariance_type == 'full' else (n, D)):
            raise ValueError("means / covariances do not have the shapes of %d states, %d dimensions, %r"
                             % (n, D, self.covariance_type))
        _lib.check(self._fn(n, D, self._code, _addr(packed), *self._priors, int(self.reversible),
                            int(self.stationary), self.nsteps, int(seed) & 0xFFFFFFFFFFFFFFFF, int(sweep),
                            *self._out, _addr(mu), _addr(cov), self._info))
        return self.T.copy(), self.p0.copy(), mu, cov


class GibbsParametersGmm(object):
    """Persistent argument block of bhmm_gibbs_parameters_gmm for one sampler (gaussian-mixture emissions per state):
    prior_w (n, M) >= 0 is the Dirichlet prior of the mixture weights (None: zeros)."""

    def __init__(self, n, M, D, covariance_type='full', prior_C=None, prior_n0=None, prior_w=None, reversible=True,
                 stationary=False, nsteps=1000):
        if covariance_type not in ('full', 'diag'):
            raise ValueError("covariance_type must be 'full' or 'diag', not %r" % (covariance_type,))
        self._L = _lib.load()
        self._fn = self._L.bhmm_gibbs_parameters_gmm
        self.n, self.M, self.D, self.covariance_type = int(n), int(M), int(D), covariance_type
        self._code = _lib.COV_FULL if covariance_type == 'full' else _lib.COV_DIAG
        self.prior_C = _lib.f64(prior_C) if prior_C is not None else None
        self.prior_n0 = _lib.f64(prior_n0) if prior_n0 is not None else None
        self.prior_w = _lib.f64(prior_w) if prior_w is not None else None
        if self.prior_w is not None and self.prior_w.shape != (self.n, self.M):
            raise ValueError("prior_w must be (%d, %d), not %r" % (self.n, self.M, self.prior_w.shape))
        self.reversible, self.stationary, self.nsteps = bool(reversible), bool(stationary), int(nsteps)
        self.T = np.empty((n, n))
        self.p0 = np.empty(n)
        # draws consumed, components whose covariance was kept, components of weight 0
        self.info = np.zeros(3, dtype=np.int32)
        self._priors = (_addr(self.prior_C), _addr(self.prior_n0), _addr(self.prior_w))
        self._out = (_addr(self.T), _addr(self.p0))
        self._info = _lib.ip(self.info)

    def __call__(self, packed_path_stats, weights, means, covariances, seed, sweep):
        """packed_path_stats: [C n*n | n0 n | the n M packed moment blocks of the labels about `means`]; weights (n, M),
        means (n, M, D), covariances (n, M, D, D) or (n, M, D): the current parameters (copied, then updated in the
        copies).  Returns (T, p0, weights_new, means_new, covariances_new)."""
        n, M, D = self.n, self.M, self.D
        packed = _c64(packed_path_stats)
        stride = 1 + D + (D * (D + 1) // 2 if self.covariance_type == 'full' else D)
        if packed.shape != (n * n + n + n * M * stride,):
            raise ValueError("packed path statistics must hold %d doubles" % (n * n + n + n * M * stride))
        w = np.array(weights, dtype=np.float64)
        mu = np.array(means, dtype=np.float64)
        cov = np.array(covariances, dtype=np.float64)
        if w.shape != (n, M) or mu.shape != (n, M, D) or \
                cov.shape != ((n, M, D, D) if self.covariance_type == 'full' else (n, M, D)):
            raise ValueError("weights / means / covariances do not have the shapes of %d states, %d components, "
                             "%d dimensions, %r" % (n, M, D, self.covariance_type))
        _lib.check(self._fn(n, M, D, self._code, _addr(packed), *self._priors, int(self.reversible),
                            int(self.stationary), self.nsteps, int(seed) & 0xFFFFFFFFFFFFFFFF, int(sweep),
                            *self._out, _addr(w), _addr(mu), _addr(cov), self._info))
        return self.T.copy(), self.p0.copy(), w, mu, cov
