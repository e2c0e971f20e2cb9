"""Multivariate Gaussian emission model: D-dimensional observations, one mean vector and one
covariance -- full (D, D) or diagonal (D,) -- per hidden state.

Inside the batched calls the densities are made on the device from the observations kept there
(MvnEngine, bhmm_mvn_emissions) and this class is not involved; `log_p_obs` / `p_obs` run the same
kernel for one array of observations (bhmm_logpdf_mvn), `estimate_from_statistics` is the M-step on
the moments the device returns (bhmm_host_mvn_mstep).  The generators run in numpy.
"""
import numpy as np

from .. import _lib
from .outputmodel import OutputModel

_COV = {'full': _lib.COV_FULL, 'diag': _lib.COV_DIAG}


def moment_stride(D, covariance_type):
    """Doubles per state of the packed moments (bhmm_mvn_moments): S0 | S1 (D) | S2 (lower triangle or diagonal)."""
    if covariance_type not in _COV:
        raise ValueError("covariance_type must be 'full' or 'diag', not %r" % (covariance_type,))
    return 1 + D + (D * (D + 1) // 2 if covariance_type == 'full' else D)


def pack_moments(S0, S1, S2, covariance_type):
    """(S0 (N,), S1 (N, D), S2 (N, D, D) or (N, D)) -> the packed layout of bhmm_mvn_moments."""
    S0, S1, S2 = (np.asarray(a, dtype=np.float64) for a in (S0, S1, S2))
    N, D = S1.shape
    out = np.empty((N, moment_stride(D, covariance_type)))
    out[:, 0] = S0
    out[:, 1:1 + D] = S1
    if covariance_type == 'full':
        il = np.tril_indices(D)
        out[:, 1 + D:] = S2[:, il[0], il[1]]
    else:
        out[:, 1 + D:] = S2
    return out.ravel()


def unpack_moments(packed, N, D, covariance_type):
    """The inverse of pack_moments; a full S2 comes back symmetric."""
    m = np.asarray(packed, dtype=np.float64).reshape(N, moment_stride(D, covariance_type))
    S0, S1 = m[:, 0].copy(), m[:, 1:1 + D].copy()
    if covariance_type == 'full':
        il = np.tril_indices(D)
        S2 = np.zeros((N, D, D))
        S2[:, il[0], il[1]] = m[:, 1 + D:]
        S2[:, il[1], il[0]] = m[:, 1 + D:]
    else:
        S2 = m[:, 1 + D:].copy()
    return S0, S1, S2


def _scatter_factor(S):
    """Cholesky factor of a scatter matrix, or None where it has none: a pivot that is not above 1e-12 of its
    diagonal entry counts as zero (the rule of the native draw, host_model.cpp)."""
    D = S.shape[0]
    L = np.zeros((D, D))
    for a in range(D):
        for b in range(a + 1):
            s = S[a, b] - np.dot(L[a, :b], L[b, :b])
            if a == b:
                if not np.isfinite(s) or not s > 1e-12 * S[a, a]:
                    return None
                L[a, a] = np.sqrt(s)
            else:
                L[a, b] = s / L[b, b]
    return L


def check_observation(o, D=None):
    """One trajectory as a C-contiguous float64 (T, D) array."""
    o = np.asarray(o, dtype=np.float64)
    if o.ndim != 2 or (D is not None and o.shape[1] != D):
        raise ValueError("multivariate observations must be (T, %s) arrays, not %r"
                         % ('D' if D is None else D, o.shape))
    return np.ascontiguousarray(o)


class MultivariateGaussianOutputModel(OutputModel):
    def __init__(self, nstates, means, covariances, covariance_type='full', min_covar=0.0):
        OutputModel.__init__(self, nstates, ignore_outliers=False)
        if covariance_type not in _COV:
            raise ValueError("covariance_type must be 'full' or 'diag', not %r" % (covariance_type,))
        self._covariance_type = covariance_type
        self._means = np.array(means, dtype=np.float64)
        if self._means.ndim != 2 or self._means.shape[0] != self.nstates or self._means.shape[1] < 1:
            raise ValueError('means must have shape (nstates, D)')
        self._D = int(self._means.shape[1])
        if self._D > _lib.MVN_MAX_D:
            raise ValueError('at most %d dimensions are supported, not %d' % (_lib.MVN_MAX_D, self._D))
        self._covs = np.array(covariances, dtype=np.float64)
        if self._covs.shape != self._cov_shape():
            raise ValueError('covariances must have shape %r for covariance_type=%r, not %r'
                             % (self._cov_shape(), covariance_type, self._covs.shape))
        if not min_covar >= 0.0:
            raise ValueError('min_covar must be >= 0')
        self.min_covar = float(min_covar)

    def _cov_shape(self):
        N, D = self.nstates, self._D
        return (N, D, D) if self._covariance_type == 'full' else (N, D)

    def __repr__(self):
        return 'MultivariateGaussianOutputModel(%d, means=%r, covariances=%r, covariance_type=%r)' % (
            self.nstates, self._means, self._covs, self._covariance_type)

    @property
    def model_type(self):
        return 'mvgaussian'

    @property
    def dimension(self):
        return self._D

    @property
    def covariance_type(self):
        return self._covariance_type

    @property
    def means(self):
        return self._means

    @property
    def covariances(self):
        return self._covs

    def parameters(self):
        """(par0, par1) as MvnEngine takes them: means (N, D), covariances (N, D, D) or (N, D)."""
        return self._means, self._covs

    def set_parameters(self, means, covariances):
        self._means = np.array(means, dtype=np.float64).reshape(self.nstates, self._D)
        self._covs = np.array(covariances, dtype=np.float64).reshape(self._cov_shape())

    def sub_output_model(self, states):
        states = np.asarray(states, dtype=np.int64)
        return MultivariateGaussianOutputModel(len(states), self._means[states], self._covs[states],
                                               covariance_type=self._covariance_type, min_covar=self.min_covar)

    def log_p_obs(self, obs, out=None):
        """(T, N) matrix of log N(x_t; mu_i, Sigma_i), from the kernel the batched calls use."""
        L = _lib.load()
        _lib.require_device()
        obs = check_observation(obs, self._D)
        T, N = obs.shape[0], self.nstates
        direct = out is not None and out.flags.c_contiguous and out.dtype == np.float64 and out.shape == (T, N)
        buf = out if direct else np.empty((T, N))
        if T:
            _lib.check(L.bhmm_logpdf_mvn(_lib.dp(buf), _lib.dp(obs), T, self._D, N, _lib.dp(_lib.f64(self._means)),
                                         _lib.dp(_lib.f64(self._covs)), _COV[self._covariance_type]))
        if out is not None and not direct:
            out[:T] = buf
            return out
        return buf

    def p_obs(self, obs, out=None):
        """The densities themselves: exp(log_p_obs).  They underflow where the log-densities do not; the batched
        calls never form them (they scale every row by its largest entry)."""
        lp = self.log_p_obs(obs, out=out)
        return np.exp(lp, out=lp)

    def estimate_from_statistics(self, S0, S1, S2):
        """M-step from the moments about the current means: S0 (N,) = sum_t gamma, S1 (N, D) = sum_t gamma
        (x - mu_old), S2 (N, D, D) or (N, D) = sum_t gamma (x - mu_old)(x - mu_old)^T (its diagonal).  The new
        mean is mu_old + S1 / S0, the covariance about the NEW mean S2 / S0 - delta delta^T + min_covar I; a
        result that is not positive definite raises RuntimeError (bhmm_host_mvn_mstep)."""
        N, D = self.nstates, self._D
        S0, S1, S2 = (np.asarray(a, dtype=np.float64) for a in (S0, S1, S2))
        if S0.shape != (N,) or S1.shape != (N, D) or S2.shape != self._cov_shape():
            raise ValueError('moments must have shapes (%d,), (%d, %d) and %r' % (N, N, D, self._cov_shape()))
        self.estimate_from_packed(pack_moments(S0, S1, S2, self._covariance_type))

    def estimate_from_packed(self, moments):
        """The same from the packed layout of bhmm_mvn_moments."""
        N, D = self.nstates, self._D
        moments = _lib.f64(moments)
        if moments.shape != (N * moment_stride(D, self._covariance_type),):
            raise ValueError('packed moments must hold %d doubles' % (N * moment_stride(D, self._covariance_type)))
        means, covs = np.empty((N, D)), np.empty(self._cov_shape())
        _lib.check(_lib.load().bhmm_host_mvn_mstep(N, D, _COV[self._covariance_type], _lib.dp(moments),
                                                   _lib.dp(_lib.f64(self._means)), self.min_covar, _lib.dp(means),
                                                   _lib.dp(covs)))
        self._means, self._covs = means, covs

    def sample_from_statistics(self, S0, S1, S2, rng=np.random):
        """Gibbs update from the moments of a hidden path about the current means (the rule
        of bhmm_gibbs_parameters_mvn in numpy, on rng's stream): S0 (N,) counts, S1 (N, D) = sum (x - mu_old),
        S2 (N, D, D) or (N, D) = sum (x - mu_old)(x - mu_old)^T (its diagonal).  Per state with n = S0 > 0:
        mu' = mu + S1 / n + L z / sqrt(n) (z: D standard normals, L the Cholesky factor of the current covariance);
        S = the scatter about mu'; full with n - 1 >= D and S positive definite: Sigma' = (L_S B^-T)(L_S B^-T)^T, B a
        Bartlett factor (sqrt of chi-squares with n - 1 - d degrees of freedom on the diagonal, then the standard
        normals below it, row-major) -- an inverse-Wishart draw; diag with n > 1: S_dd / chi2(n - 1) per dimension.
        At D = 1 this consumes the variates of GaussianOutputModel.sample_from_statistics in its order.  Returns the
        number of states whose covariance was kept because it could not be drawn."""
        N, D = self.nstates, self._D
        S0, S1, S2 = (np.asarray(a, dtype=np.float64) for a in (S0, S1, S2))
        if S0.shape != (N,) or S1.shape != (N, D) or S2.shape != self._cov_shape():
            raise ValueError('moments must have shapes (%d,), (%d, %d) and %r' % (N, N, D, self._cov_shape()))
        full = self._covariance_type == 'full'
        kept = 0
        for i in range(N):
            n = int(round(S0[i]))
            if n <= 0:
                continue
            old_mu = self._means[i].copy()
            L = self._factor(i)
            z = np.array([rng.randn()]) if D == 1 else rng.standard_normal(D)
            self._means[i] = L.dot(z) / np.sqrt(n) + (old_mu + S1[i] / n)
            delta = self._means[i] - old_mu
            if not full:
                if n > 1:
                    for d in range(D):
                        chi2 = rng.chisquare(n - 1)
                        sdd = S2[i, d] - 2.0 * delta[d] * S1[i, d] + n * delta[d] * delta[d]
                        if sdd > 0.0:
                            self._covs[i, d] = sdd / chi2
                        else:
                            kept += 1
                continue
            S = S2[i] - np.outer(delta, S1[i]) - np.outer(S1[i], delta) + n * np.outer(delta, delta)
            LS = _scatter_factor(S) if n - 1 >= D else None
            if LS is None:
                kept += 1
                continue
            B = np.zeros((D, D))
            for d in range(D):
                B[d, d] = np.sqrt(rng.chisquare(n - 1 - d))
            if D > 1:
                B[np.tril_indices(D, -1)] = rng.standard_normal(D * (D - 1) // 2)
            M = np.linalg.solve(B, LS.T).T          # L_S B^-T
            cov = M.dot(M.T)
            self._covs[i] = 0.5 * (cov + cov.T)
        return kept

    def sample(self, observations, prior=None, rng=np.random):
        """The reference's signature (gaussian.py:274-320) on top of sample_from_statistics: observations[k] are the
        (n_k, D) observations assigned to state k."""
        N, D = self.nstates, self._D
        S0, S1 = np.zeros(N), np.zeros((N, D))
        S2 = np.zeros(self._cov_shape())
        for i in range(N):
            o = np.asarray(observations[i], dtype=np.float64).reshape(-1, D)
            d = o - self._means[i]
            S0[i], S1[i] = o.shape[0], d.sum(axis=0)
            S2[i] = d.T.dot(d) if self._covariance_type == 'full' else (d * d).sum(axis=0)
        return self.sample_from_statistics(S0, S1, S2, rng=rng)

    def _factor(self, state_index):
        c = self._covs[state_index]
        return np.linalg.cholesky(c) if self._covariance_type == 'full' else np.diag(np.sqrt(c))

    def generate_observation_from_state(self, state_index, rng=np.random):
        return self._means[state_index] + self._factor(state_index).dot(rng.standard_normal(self._D))

    def generate_observations_from_state(self, state_index, nobs, rng=np.random):
        return self._means[state_index] + rng.standard_normal((nobs, self._D)).dot(self._factor(state_index).T)

    def generate_observation_trajectory(self, s_t, rng=np.random):
        s_t = np.asarray(s_t)
        out = np.empty((s_t.shape[0], self._D))
        for i in range(self.nstates):
            idx = np.where(s_t == i)[0]
            if idx.size:
                out[idx] = self.generate_observations_from_state(i, idx.size, rng=rng)
        return out
