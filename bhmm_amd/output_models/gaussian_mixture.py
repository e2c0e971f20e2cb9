"""Gaussian-mixture emission model: D-dimensional observations, M Gaussian components per hidden state --
mixture weights w_ic, means mu_ic and covariances Sigma_ic, full (D, D) or diagonal (D,) -- the same M for
every state.

Inside the batched calls the mixture densities and the component responsibilities are made on the device
from the observations kept there (GmmEngine, bhmm_gmm_emissions) and this class is not involved; `log_p_obs` /
`p_obs` run the same kernel for one array of observations (bhmm_logpdf_gmm), `estimate_from_statistics` is
the M-step on the per-component moments the device returns: the weights here, means and covariances of all
N M components by bhmm_host_mvn_mstep.  The generators run in numpy.
"""
import numpy as np

from .. import _lib
from .mvgaussian import _COV, check_observation, moment_stride, pack_moments, unpack_moments
from .outputmodel import OutputModel

STARVED = 1e-8     # a component below this share of its state's weight keeps its mean and covariance


def pack_parameters(weights, means, covariances):
    """(weights (N, M), means (N, M, D), covariances (N, M, D, D) or (N, M, D)) -> (par0, par1) as GmmEngine takes
    them: par0 (N, M, 1 + D) with the weight in column 0 and the mean after it, par1 the covariances."""
    w, mu = np.asarray(weights, dtype=np.float64), np.asarray(means, dtype=np.float64)
    par0 = np.empty(mu.shape[:2] + (1 + mu.shape[2],))
    par0[:, :, 0] = w
    par0[:, :, 1:] = mu
    return par0, np.array(covariances, dtype=np.float64)


def unpack_parameters(par0, par1):
    """The inverse of pack_parameters: (weights, means, covariances), copies."""
    par0 = np.asarray(par0, dtype=np.float64)
    return par0[:, :, 0].copy(), par0[:, :, 1:].copy(), np.array(par1, dtype=np.float64)


def unpack_component_moments(packed, N, M, D, covariance_type):
    """The N M blocks of bhmm_gmm_moments -> S0 (N, M), S1 (N, M, D), S2 (N, M, D, D) symmetric or (N, M, D)."""
    S0, S1, S2 = unpack_moments(packed, N * M, D, covariance_type)
    return S0.reshape(N, M), S1.reshape(N, M, D), S2.reshape((N, M) + S2.shape[1:])


def pack_component_moments(S0, S1, S2, covariance_type):
    """The inverse of unpack_component_moments."""
    S0, S1, S2 = (np.asarray(a, dtype=np.float64) for a in (S0, S1, S2))
    N, M, D = S1.shape
    return pack_moments(S0.reshape(N * M), S1.reshape(N * M, D), S2.reshape((N * M,) + S2.shape[2:]),
                        covariance_type)


class GaussianMixtureOutputModel(OutputModel):
    def __init__(self, nstates, weights, means, covariances, covariance_type='full', min_covar=0.0):
        OutputModel.__init__(self, nstates, ignore_outliers=False)
        if covariance_type not in _COV:
            raise ValueError("covariance_type must be 'full' or 'diag', not %r" % (covariance_type,))
        self._covariance_type = covariance_type
        self._means = np.array(means, dtype=np.float64)
        if self._means.ndim != 3 or self._means.shape[0] != self.nstates or self._means.shape[1] < 1 \
                or self._means.shape[2] < 1:
            raise ValueError('means must have shape (nstates, M, D)')
        self._M, self._D = int(self._means.shape[1]), int(self._means.shape[2])
        if self._D > _lib.MVN_MAX_D:
            raise ValueError('at most %d dimensions are supported, not %d' % (_lib.MVN_MAX_D, self._D))
        if self.nstates * self._M > 4096:
            raise ValueError('at most 4096 components in all are supported, not %d x %d' % (self.nstates, self._M))
        self._weights = np.array(weights, dtype=np.float64)
        if self._weights.shape != (self.nstates, self._M):
            raise ValueError('weights must have shape %r, not %r' % ((self.nstates, self._M), self._weights.shape))
        if not np.all(np.isfinite(self._weights)) or np.any(self._weights < 0.0) \
                or np.any(np.abs(self._weights.sum(axis=1) - 1.0) > 1e-8):
            raise ValueError('the mixture weights of every state must be >= 0 and sum to 1')
        self._covs = np.array(covariances, dtype=np.float64)
        if self._covs.shape != self._cov_shape():
            raise ValueError('covariances must have shape %r for covariance_type=%r, not %r'
                             % (self._cov_shape(), covariance_type, self._covs.shape))
        if not min_covar >= 0.0:
            raise ValueError('min_covar must be >= 0')
        self.min_covar = float(min_covar)

    def _cov_shape(self):
        N, M, D = self.nstates, self._M, self._D
        return (N, M, D, D) if self._covariance_type == 'full' else (N, M, D)

    def __repr__(self):
        return 'GaussianMixtureOutputModel(%d, weights=%r, means=%r, covariances=%r, covariance_type=%r)' % (
            self.nstates, self._weights, self._means, self._covs, self._covariance_type)

    @property
    def model_type(self):
        return 'gaussian_mixture'

    @property
    def dimension(self):
        return self._D

    @property
    def ncomponents(self):
        return self._M

    @property
    def covariance_type(self):
        return self._covariance_type

    @property
    def weights(self):
        return self._weights

    @property
    def means(self):
        return self._means

    @property
    def covariances(self):
        return self._covs

    def parameters(self):
        """(par0, par1) as GmmEngine takes them: par0 (N, M, 1 + D) = [weight | mean], par1 the covariances
        (N, M, D, D) or (N, M, D)."""
        return pack_parameters(self._weights, self._means, self._covs)

    def set_parameters(self, par0, par1):
        w, mu, cov = unpack_parameters(np.asarray(par0).reshape(self.nstates, self._M, 1 + self._D), par1)
        self._weights, self._means, self._covs = w, mu, cov.reshape(self._cov_shape())

    def sub_output_model(self, states):
        states = np.asarray(states, dtype=np.int64)
        return GaussianMixtureOutputModel(len(states), self._weights[states], self._means[states], self._covs[states],
                                          covariance_type=self._covariance_type, min_covar=self.min_covar)

    def log_p_obs(self, obs, out=None):
        """(T, N) matrix of log sum_c w_ic N(x_t; mu_ic, Sigma_ic), from the kernel the batched calls use."""
        L = _lib.load()
        _lib.require_device()
        obs = check_observation(obs, self._D)
        T, N = obs.shape[0], self.nstates
        direct = out is not None and out.flags.c_contiguous and out.dtype == np.float64 and out.shape == (T, N)
        buf = out if direct else np.empty((T, N))
        if T:
            _lib.check(L.bhmm_logpdf_gmm(_lib.dp(buf), _lib.dp(obs), T, self._D, N, self._M,
                                         _lib.dp(_lib.f64(self._weights)), _lib.dp(_lib.f64(self._means)),
                                         _lib.dp(_lib.f64(self._covs)), _COV[self._covariance_type]))
        if out is not None and not direct:
            out[:T] = buf
            return out
        return buf

    def p_obs(self, obs, out=None):
        """The densities themselves: exp(log_p_obs) (they underflow where the log-densities do not)."""
        lp = self.log_p_obs(obs, out=out)
        return np.exp(lp, out=lp)

    def estimate_from_statistics(self, S0, S1, S2):
        """M-step from the per-component moments about the current means: S0 (N, M) = sum_t gamma_t(i) r_t(i,c),
        S1 (N, M, D) and S2 (N, M, D, D) or (N, M, D) the same weights on (x - mu_old) and its outer product (its
        diagonal).  w_ic = S0_ic / sum_c S0_ic; mean and covariance of a component as
        MultivariateGaussianOutputModel.estimate_from_statistics.  A starved component -- S0_ic < 1e-8 sum_c S0_ic
        -- keeps its mean and covariance and takes only its new weight (still a generalised M-step: the expected
        log-likelihood does not fall).  A state without any weight, or a covariance that is not positive definite,
        raises RuntimeError (bhmm_host_mvn_mstep)."""
        N, M, D = self.nstates, self._M, self._D
        S0, S1, S2 = (np.asarray(a, dtype=np.float64) for a in (S0, S1, S2))
        if S0.shape != (N, M) or S1.shape != (N, M, D) or S2.shape != self._cov_shape():
            raise ValueError('moments must have shapes %r, %r and %r' % ((N, M), (N, M, D), self._cov_shape()))
        self.estimate_from_packed(pack_component_moments(S0, S1, S2, self._covariance_type))

    def estimate_from_packed(self, moments):
        """The same from the N M packed blocks of bhmm_gmm_moments."""
        N, M, D = self.nstates, self._M, self._D
        ms = moment_stride(D, self._covariance_type)
        moments = np.array(_lib.f64(moments), dtype=np.float64)
        if moments.shape != (N * M * ms,):
            raise ValueError('packed moments must hold %d doubles' % (N * M * ms))
        blocks = moments.reshape(N * M, ms)
        S0 = blocks[:, 0].reshape(N, M).copy()
        tot = S0.sum(axis=1)
        starved = S0 < STARVED * tot[:, None]
        starved[~(tot > 0.0)] = False          # (a state without any weight fails in the native M-step, as it does now)
        # a starved component goes through the native M-step as one unit of weight at its old mean with its old
        # scatter of zero -- whatever comes back for it is replaced by what it had
        flat = starved.ravel()
        blocks[flat, 0] = 1.0
        blocks[flat, 1:] = 0.0
        if self._covariance_type == 'full':
            il = np.tril_indices(D)
            blocks[flat, 1 + D:] = self._covs.reshape(N * M, D, D)[flat][:, il[0], il[1]]
        else:
            blocks[flat, 1 + D:] = self._covs.reshape(N * M, D)[flat]
        means, covs = np.empty((N * M, D)), np.empty((N * M,) + self._cov_shape()[2:])
        _lib.check(_lib.load().bhmm_host_mvn_mstep(N * M, D, _COV[self._covariance_type], _lib.dp(blocks.ravel()),
                                                   _lib.dp(_lib.f64(self._means.reshape(N * M, D))), self.min_covar,
                                                   _lib.dp(means), _lib.dp(covs)))
        means, covs = means.reshape(N, M, D), covs.reshape(self._cov_shape())
        means[starved], covs[starved] = self._means[starved], self._covs[starved]
        self._weights = S0 / tot[:, None]
        self._means, self._covs = means, covs

    def sample_from_statistics(self, S0, S1, S2, rng=np.random, weights_prior=1.0):
        """Gibbs update from the moments of the component labels of a hidden path about the current means (DESIGN.md
        section 26; the rule of bhmm_gibbs_parameters_gmm in numpy, on rng's stream): S0 (N, M) counts, S1 (N, M, D),
        S2 (N, M, D, D) or (N, M, D).  Means and covariances component by component as
        MultivariateGaussianOutputModel.sample_from_statistics draws them per state (an empty component keeps both);
        then per state w_i ~ Dirichlet(weights_prior + S0_i): a component with alpha = 0 takes weight exactly 0, a
        state whose alpha are all 0 keeps its weights, M = 1 draws nothing.  weights_prior: a scalar or (N, M).
        Returns the number of components whose covariance was kept because it could not be drawn."""
        from .mvgaussian import MultivariateGaussianOutputModel
        N, M, D = self.nstates, self._M, self._D
        S0, S1, S2 = (np.asarray(a, dtype=np.float64) for a in (S0, S1, S2))
        if S0.shape != (N, M) or S1.shape != (N, M, D) or S2.shape != self._cov_shape():
            raise ValueError('moments must have shapes %r, %r and %r' % ((N, M), (N, M, D), self._cov_shape()))
        prior = np.broadcast_to(np.asarray(weights_prior, dtype=np.float64), (N, M))
        if not np.all(np.isfinite(prior)) or np.any(prior < 0.0):
            raise ValueError('weights_prior must be >= 0 and finite')
        flat = MultivariateGaussianOutputModel(N * M, self._means.reshape(N * M, D),
                                               self._covs.reshape((N * M,) + self._cov_shape()[2:]),
                                               covariance_type=self._covariance_type)
        kept = flat.sample_from_statistics(S0.reshape(N * M), S1.reshape(N * M, D),
                                           S2.reshape((N * M,) + S2.shape[2:]), rng=rng)
        self._means = flat.means.reshape(N, M, D).copy()
        self._covs = flat.covariances.reshape(self._cov_shape()).copy()
        if M > 1:
            alpha = prior + np.rint(S0)
            w = self._weights.copy()
            for i in range(N):
                pos = alpha[i] > 0.0
                if not pos.any():
                    continue
                w[i] = 0.0
                w[i, pos] = rng.dirichlet(alpha[i, pos])
            self._weights = w
        return kept

    def _factor(self, i, c):
        cv = self._covs[i, c]
        return np.linalg.cholesky(cv) if self._covariance_type == 'full' else np.diag(np.sqrt(cv))

    def _components(self, state_index, nobs, rng):
        w = self._weights[state_index]
        return np.minimum(np.searchsorted(np.cumsum(w), rng.random(nobs) * w.sum(), side='right'), self._M - 1)

    def generate_observations_from_state(self, state_index, nobs, rng=np.random, return_components=False):
        comp = self._components(state_index, nobs, rng)
        out = np.empty((nobs, self._D))
        for c in range(self._M):
            idx = np.where(comp == c)[0]
            if idx.size:
                out[idx] = self._means[state_index, c] + \
                    rng.standard_normal((idx.size, self._D)).dot(self._factor(state_index, c).T)
        return (out, comp) if return_components else out

    def generate_observation_from_state(self, state_index, rng=np.random):
        return self.generate_observations_from_state(state_index, 1, rng=rng)[0]

    def generate_observation_trajectory(self, s_t, rng=np.random):
        s_t = np.asarray(s_t)
        out = np.empty((s_t.shape[0], self._D))
        for i in range(self.nstates):
            idx = np.where(s_t == i)[0]
            if idx.size:
                out[idx] = self.generate_observations_from_state(i, idx.size, rng=rng)
        return out
