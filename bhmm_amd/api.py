"""Functional wrappers with the signatures of bhmm/api.py:309-372 (estimate_hmm) and
:375-470 (bayesian_hmm), plus lag_observations (:70-94) and the model factories (:97-158)."""
import numpy as np

from .estimators.bayesian_sampling import BayesianHMMSampler
from .estimators.maximum_likelihood import MaximumLikelihoodEstimator
from .hmm import HMM, SampledHMM
from .output_models import (DiscreteOutputModel, GaussianMixtureOutputModel, GaussianOutputModel,
                            MultivariateGaussianOutputModel, PoissonOutputModel)


def _guess_output_type(observations):
    """bhmm/api.py:36-66."""
    o1 = np.asarray(observations[0])
    if np.issubdtype(o1.dtype, np.integer) and o1.ndim == 1:
        return 'discrete'
    if np.issubdtype(o1.dtype, np.floating) and o1.ndim == 1:
        return 'gaussian'
    if np.issubdtype(o1.dtype, np.floating) and o1.ndim == 2:
        return 'mvgaussian'
    if np.issubdtype(o1.dtype, np.integer) and o1.ndim == 2:
        return 'poisson'        # (T, D) counts: binned multi-channel photon data
    raise TypeError('Observations is neither 1D- or 2D-sequences of integers nor 1D- or 2D-sequences of floats.')


class LaggedObservations(list):
    """What lag_observations returns: a plain list of sub-sampled trajectories (numpy views, so
    existing code keeps working) that also remembers how it was made -- the original
    trajectories, the lag, and (trajectory, shift) of every entry -- so that the estimators can
    upload the ORIGINAL data once and cut the views on the GPU
    (bhmm_ctx_set_observations_lagged) instead of uploading `lag` host-side copies."""

    def __init__(self, base, lag, stride):
        list.__init__(self)
        self.base = [np.asarray(o) for o in base]
        self.lag = int(lag)
        self.stride = int(stride)
        self.views = []          # (trajectory index, shift) of every entry


def lag_observations(observations, lag, stride=1):
    """Sub-sampled, shifted trajectories (bhmm/api.py:70-94): trajectory k contributes
    obs_k[shift::lag] for shift = 0, stride, 2 stride, ... < lag; pieces with fewer than two
    observations are left out (they carry no transition)."""
    out = LaggedObservations(observations, lag, stride)
    for k, traj in enumerate(out.base):
        for shift in range(0, out.lag, out.stride):
            piece = traj[shift::out.lag]
            if piece.shape[0] > 1:
                out.append(piece)
                out.views.append((k, shift))
    return out


def gaussian_hmm(pi, P, means, sigmas):
    """bhmm/api.py:97-126."""
    nstates = len(means)
    return HMM(pi, P, GaussianOutputModel(nstates, means, sigmas))


def discrete_hmm(pi, P, pout):
    """bhmm/api.py:129-158."""
    return HMM(pi, P, DiscreteOutputModel(pout))


def mvgaussian_hmm(pi, P, means, covariances, covariance_type='full'):
    """An HMM with multivariate gaussian emissions: means (nstates, D), covariances (nstates, D, D), or with
    covariance_type='diag' the variances (nstates, D)."""
    nstates = len(means)
    return HMM(pi, P, MultivariateGaussianOutputModel(nstates, means, covariances, covariance_type=covariance_type))


def gaussian_mixture_hmm(pi, P, weights, means, covariances, covariance_type='full'):
    """An HMM with a mixture of M gaussians per state: weights (nstates, M), means
    (nstates, M, D), covariances (nstates, M, D, D), or with covariance_type='diag' the variances (nstates, M, D)."""
    nstates = len(means)
    return HMM(pi, P, GaussianMixtureOutputModel(nstates, weights, means, covariances,
                                                 covariance_type=covariance_type))


def poisson_hmm(pi, P, rates):
    """An HMM with Poisson count emissions: rates (nstates, D), one rate >= 0 per state and
    channel; the observations are (T_k, D) arrays of counts."""
    nstates = len(rates)
    return HMM(pi, P, PoissonOutputModel(nstates, rates))


def init_poisson_hmm(observations, nstates, lag=1, reversible=True):
    """Initial model for (T_k, D) count observations, deterministic, numpy only: the seeding and Lloyd iterations of
    init_mvgaussian_hmm on the variance-stabilised counts sqrt(x + 3/8), rates from the cluster means of the raw
    counts (a channel that is all zero in a cluster gets 0.5 / its points), refined by a few EM iterations of the
    Poisson mixture, and a transition matrix from the count matrix of the labels at the lag
    (bhmm_amd/init/poisson.py)."""
    from .init.poisson import init_model_poisson
    hmm0 = init_model_poisson(observations, nstates, lag=lag, reversible=reversible)
    hmm0._lag = lag
    return hmm0


def init_gaussian_mixture_hmm(observations, nstates, ncomponents, lag=1, reversible=True, covariance_type='full'):
    """Initial model with `ncomponents` gaussian components per state for (T_k, D) observations, deterministic, numpy
    only: the model of init_mvgaussian_hmm and its hard labels, then inside every state the same farthest-point
    seeding and at most 20 Lloyd iterations on that state's points; a component of fewer than D + 1 points takes the
    state's covariance; weights are the cluster shares, floored at 1e-3 and renormalised
    (bhmm_amd/init/mvgaussian.py)."""
    from .init.mvgaussian import init_model_gaussian_mixture
    hmm0 = init_model_gaussian_mixture(observations, nstates, ncomponents, lag=lag, reversible=reversible,
                                       covariance_type=covariance_type)
    hmm0._lag = lag
    return hmm0


def init_mvgaussian_hmm(observations, nstates, lag=1, reversible=True, covariance_type='full'):
    """Initial model for (T_k, D) observations, deterministic, numpy only: farthest-point seeding and at most 20
    Lloyd iterations on at most 1e5 evenly strided points, mean and covariance of every cluster, and a transition
    matrix from the count matrix of the hard labels at the lag (bhmm_amd/init/mvgaussian.py)."""
    from .init.mvgaussian import init_model_mvgaussian
    hmm0 = init_model_mvgaussian(observations, nstates, lag=lag, reversible=reversible,
                                 covariance_type=covariance_type)
    hmm0._lag = lag
    return hmm0


def init_gaussian_hmm(observations, nstates, lag=1, reversible=True):
    """bhmm/api.py:202-228."""
    from .init.gaussian import init_model_gaussian1d
    if lag > 1:
        observations = lag_observations(observations, lag)
    hmm0 = init_model_gaussian1d(observations, nstates, reversible=reversible)
    hmm0._lag = lag
    return hmm0


def init_discrete_hmm(observations, nstates, lag=1, reversible=True, stationary=True,
                      regularize=True, method='connect-spectral', separate=None):
    """bhmm/api.py:231-306."""
    from .init import discrete as _init
    p0, P, B = _init.init_discrete_hmm(observations, nstates, lag=lag, reversible=reversible,
                                       stationary=stationary, regularize=regularize,
                                       method=method, separate=separate)
    hmm0 = discrete_hmm(p0, P, B)
    hmm0._lag = lag
    return hmm0


def init_hmm(observations, nstates, lag=1, output=None, reversible=True, ncomponents=None):
    """bhmm/api.py:161-199.  output='gaussian_mixture' (never guessed) needs ncomponents."""
    if output is None:
        output = _guess_output_type(observations)
    if output == 'discrete':
        return init_discrete_hmm(observations, nstates, lag=lag, reversible=reversible)
    if output == 'gaussian':
        return init_gaussian_hmm(observations, nstates, lag=lag, reversible=reversible)
    if output == 'mvgaussian':
        return init_mvgaussian_hmm(observations, nstates, lag=lag, reversible=reversible)
    if output == 'poisson':
        return init_poisson_hmm(observations, nstates, lag=lag, reversible=reversible)
    if output == 'gaussian_mixture':
        if ncomponents is None:
            raise ValueError("output='gaussian_mixture' needs ncomponents")
        return init_gaussian_mixture_hmm(observations, nstates, ncomponents, lag=lag, reversible=reversible)
    raise NotImplementedError('output model type ' + str(output) + ' not yet implemented.')


def estimate_hmm(observations, nstates, lag=1, initial_model=None, output=None, reversible=True,
                 stationary=False, p=None, accuracy=1e-3, maxit=1000, maxit_P=100000,
                 mincount_connectivity=1e-2, **engine_kwargs):
    """bhmm/api.py:309-372."""
    if output is None:
        output = _guess_output_type(observations)
    if lag > 1:
        observations = lag_observations(observations, lag)
    est = MaximumLikelihoodEstimator(observations, nstates, initial_model=initial_model,
                                     output=output, reversible=reversible, stationary=stationary,
                                     p=p, accuracy=accuracy, maxit=maxit, maxit_P=maxit_P,
                                     **engine_kwargs)
    est.fit()
    est.hmm._lag = lag
    return est.hmm


def _refuse_poisson(estimated_hmm):
    if estimated_hmm.output_model.model_type == 'poisson':
        raise NotImplementedError('Poisson count emissions have no Gibbs sampler yet (DESIGN.md section 27)')


def bayesian_hmm(observations, estimated_hmm, nsample=100, reversible=True, stationary=False,
                 p0_prior='mixed', transition_matrix_prior='mixed', store_hidden=False,
                 call_back=None, **engine_kwargs):
    """bhmm/api.py:375-470.  Returns a SampledHMM (which also iterates over / indexes the
    sampled models)."""
    _refuse_poisson(estimated_hmm)
    if estimated_hmm.output_model.model_type == 'mvgaussian':
        raise NotImplementedError('multivariate gaussian emissions are sampled by bayesian_mvgaussian_hmm, '
                                  'not by bayesian_hmm yet')
    if estimated_hmm.output_model.model_type == 'gaussian_mixture':
        raise NotImplementedError('the Gibbs sampler for gaussian-mixture emissions is '
                                  'bayesian_gaussian_mixture_hmm')
    sampler = BayesianHMMSampler(observations, estimated_hmm.nstates, initial_model=estimated_hmm,
                                 reversible=reversible, stationary=stationary,
                                 transition_matrix_sampling_steps=1000, p0_prior=p0_prior,
                                 transition_matrix_prior=transition_matrix_prior,
                                 output=estimated_hmm.output_model.model_type, **engine_kwargs)
    sampled = sampler.sample(nsamples=nsample, save_hidden_state_trajectory=store_hidden,
                             call_back=call_back)
    return SampledHMM(estimated_hmm, sampled)


def bayesian_mvgaussian_hmm(observations, estimated_hmm, nsample=100, reversible=True, stationary=False,
                            p0_prior='mixed', transition_matrix_prior='mixed', store_hidden=False,
                            call_back=None, **engine_kwargs):
    """bayesian_hmm for multivariate gaussian emissions: observations are (T_k, D) arrays,
    estimated_hmm a model of output type 'mvgaussian' (estimate_hmm, mvgaussian_hmm).  Every sweep draws the hidden
    paths and takes their moments on the device (MvnEngine.sample_paths_moments), then draws per state a mean vector
    and -- inverse Wishart (full) or one inverse chi-square per dimension (diag) -- a covariance, the transition
    matrix and the initial distribution (bhmm_gibbs_parameters_mvn).  Returns a SampledHMM: means_mean,
    covariances_std, covariances_conf ... summarise the sampled emission parameters.  Sampled models are not
    relabelled (label switching is the user's to watch, as in the reference).  engine_kwargs: device, seed (of the
    chain; one from numpy's global generator if not given), native_parameters."""
    _refuse_poisson(estimated_hmm)
    if estimated_hmm.output_model.model_type == 'gaussian_mixture':
        raise NotImplementedError('the Gibbs sampler for gaussian-mixture emissions is '
                                  'bayesian_gaussian_mixture_hmm')
    if estimated_hmm.output_model.model_type != 'mvgaussian':
        raise ValueError("bayesian_mvgaussian_hmm takes a model with multivariate gaussian emissions, not %r"
                         % (estimated_hmm.output_model.model_type,))
    seed = engine_kwargs.pop('seed', None)
    sampler = BayesianHMMSampler(observations, estimated_hmm.nstates, initial_model=estimated_hmm,
                                 reversible=reversible, stationary=stationary,
                                 transition_matrix_sampling_steps=1000, p0_prior=p0_prior,
                                 transition_matrix_prior=transition_matrix_prior, output='mvgaussian',
                                 **engine_kwargs)
    sampled = sampler.sample(nsamples=nsample, save_hidden_state_trajectory=store_hidden,
                             call_back=call_back, seed=seed)
    return SampledHMM(estimated_hmm, sampled)


def bayesian_gaussian_mixture_hmm(observations, estimated_hmm, nsample=100, reversible=True, stationary=False,
                                  p0_prior='mixed', transition_matrix_prior='mixed', store_hidden=False,
                                  call_back=None, weights_prior=1.0, seed=None, **engine_kwargs):
    """bayesian_hmm for gaussian-mixture emissions per state: observations are (T_k, D) arrays,
    estimated_hmm a model of output type 'gaussian_mixture' (estimate_hmm, gaussian_mixture_hmm).  Every sweep draws
    the hidden paths, a component for every step and the moments of the component labels on the device
    (GmmEngine.sample_paths_components), then mean and covariance of every component as bayesian_mvgaussian_hmm
    draws them per state, the mixture weights of every state from Dirichlet(weights_prior + counts), the transition
    matrix and the initial distribution (bhmm_gibbs_parameters_gmm).  weights_prior: a scalar or an (N, M) array;
    1.0 is the flat Dirichlet, 0 lets a component that was emptied once stay empty for good.  seed: of the chain
    (one from numpy's global generator if not given).  Returns a SampledHMM: weights_mean / _std / _conf (N, M),
    means_* and covariances_* as for the multivariate gaussian kind with the component axis after the state's;
    bhmm_amd.score takes it.  Sampled models are not relabelled: label switching, between states and between the
    components of a state, is the user's to watch.  engine_kwargs: device, native_parameters."""
    _refuse_poisson(estimated_hmm)
    if estimated_hmm.output_model.model_type != 'gaussian_mixture':
        raise ValueError("bayesian_gaussian_mixture_hmm takes a model with gaussian-mixture emissions, not %r"
                         % (estimated_hmm.output_model.model_type,))
    from .estimators.bayesian_sampling import BayesianGaussianMixtureHMMSampler
    sampler = BayesianGaussianMixtureHMMSampler(observations, estimated_hmm.nstates, initial_model=estimated_hmm,
                                                reversible=reversible, stationary=stationary,
                                                transition_matrix_sampling_steps=1000, p0_prior=p0_prior,
                                                transition_matrix_prior=transition_matrix_prior,
                                                weights_prior=weights_prior, **engine_kwargs)
    sampled = sampler.sample(nsamples=nsample, save_hidden_state_trajectory=store_hidden,
                             call_back=call_back, seed=seed)
    return SampledHMM(estimated_hmm, sampled)


def _engine_for(output, device):
    """The engine of an output type: multivariate gaussian models run on an MvnEngine, gaussian mixtures on a
    GmmEngine, Poisson count models on a PoissonEngine."""
    from .engine import Engine, GmmEngine, MvnEngine, PoissonEngine
    if output == 'gaussian_mixture':
        return GmmEngine(device)
    if output == 'poisson':
        return PoissonEngine(device)
    return MvnEngine(device) if output == 'mvgaussian' else Engine(device)


def score(observations, models, lag=1, per_trajectory=False, **engine_kwargs):
    """Log-likelihood of `observations` under each of `models` (one forward pass per model, all
    models of a call on the GPU together, bhmm_score).  `models`: one HMM, a list of HMMs of the same
    output type and number of states, or a SampledHMM (its sampled models).  lag > 1 scores the lagged
    views (lag_observations).  Returns one total per model (an array of shape (S,)), or with
    per_trajectory the (S, K) array of per-trajectory log-likelihoods.  A trajectory of probability zero
    under a model scores -inf.  Gaussian and discrete models of up to 128 states run parallel over time
    (verified against the serial recursion, which more states take; Engine.get_option("score_path") is 3 for 65 to
    128 states).  engine_kwargs: device (default 0)."""
    from .estimators.maximum_likelihood import model_tuple
    if isinstance(models, SampledHMM):
        models = models.sampled_hmms
    elif isinstance(models, HMM):
        models = [models]
    models = list(models)
    if not models:
        raise ValueError("score needs at least one model")
    for m in models:
        if not isinstance(m, HMM):
            raise TypeError("models must be HMM objects (or a SampledHMM)")
    output = models[0].output_model.model_type
    nstates = models[0].nstates
    for m in models[1:]:
        if m.output_model.model_type != output:
            raise ValueError("all models must have the same output type (got %r and %r)"
                             % (output, m.output_model.model_type))
        if m.nstates != nstates:
            raise ValueError("all models must have the same number of states")
    nsymbols = models[0].output_model.nsymbols if output == 'discrete' else 0
    if output == 'discrete':
        for m in models[1:]:
            if m.output_model.nsymbols != nsymbols:
                raise ValueError("all models must have the same number of symbols")
    if len(observations) == 0:
        raise ValueError("no observations")
    device = engine_kwargs.pop('device', 0)
    if engine_kwargs:
        raise TypeError("unexpected keyword arguments: %s" % ", ".join(sorted(engine_kwargs)))
    if lag > 1:
        observations = lag_observations(observations, lag)
    eng = _engine_for(output, device)
    try:
        if output == 'discrete':
            obs = [np.asarray(o) for o in observations]
            eng.set_observations('discrete', obs, nstates, nsymbols=nsymbols)
        else:
            eng.set_observations(output, [np.asarray(o, dtype=np.float64) for o in observations], nstates)
        logL = eng.score([model_tuple(m) for m in models])
    finally:
        eng.close()
    return logL if per_trajectory else logL.sum(axis=1)


def posterior_decode(observations, model, lag=1, confidence=False, **engine_kwargs):
    """Posterior (maximum-posterior-marginal) decoding of `observations` under one HMM
    (bhmm_posterior_decode): per trajectory the state of largest posterior marginal gamma_t(i) at every
    step (the lowest index on exactly equal gamma), as uint8 arrays (int32 above 256 states); with
    `confidence` also max_i gamma_t(i) as float32 arrays, returned as (paths, conf).  lag > 1 decodes the
    lagged views (lag_observations), one result per view.  Gaussian and discrete models of up to 8 states
    are decoded by one fused kernel that stores no gamma; more states run an E-step that stores gamma.
    engine_kwargs: device (default 0)."""
    from .estimators.maximum_likelihood import model_tuple
    if not isinstance(model, HMM):
        raise TypeError("model must be an HMM object")
    if len(observations) == 0:
        raise ValueError("no observations")
    output = model.output_model.model_type
    nstates = model.nstates
    nsymbols = model.output_model.nsymbols if output == 'discrete' else 0
    device = engine_kwargs.pop('device', 0)
    if engine_kwargs:
        raise TypeError("unexpected keyword arguments: %s" % ", ".join(sorted(engine_kwargs)))
    if lag > 1:
        observations = lag_observations(observations, lag)
    eng = _engine_for(output, device)
    try:
        if output == 'discrete':
            obs = [np.asarray(o) for o in observations]
            eng.set_observations('discrete', obs, nstates, nsymbols=nsymbols)
        else:
            eng.set_observations(output, [np.asarray(o, dtype=np.float64) for o in observations], nstates)
        return eng.posterior_decode(*model_tuple(model), confidence=confidence)
    finally:
        eng.close()


def decode_segments(observations, model, lag=1, method='viterbi', stats=False, **engine_kwargs):
    """Dwell segments of `observations` decoded under one HMM (bhmm_decode_runs): the path of method 'viterbi'
    (the most probable path) or 'posterior' (the state of largest posterior marginal per step) collapsed on the
    GPU into runs of equal states -- per run its state, its first step inside the trajectory and its length --
    without the per-step path crossing the link.  Returns a PathRuns (bhmm_amd.engine): offsets (K + 1), start,
    length and state concatenated over the trajectories, trajectory(k) for the three views of one; with `stats`
    also dwell ((nstates, 5): runs, steps, longest run, censored runs, censored steps per state) and jumps
    ((nstates, nstates) run pairs i -> j).  lag > 1 decodes the lagged views (lag_observations), one trajectory
    per view.  Up to 256 states.  engine_kwargs: device (default 0)."""
    from .estimators.maximum_likelihood import model_tuple
    if not isinstance(model, HMM):
        raise TypeError("model must be an HMM object")
    if method not in ('viterbi', 'posterior'):
        raise ValueError("method must be 'viterbi' or 'posterior', not %r" % (method,))
    if len(observations) == 0:
        raise ValueError("no observations")
    output = model.output_model.model_type
    nstates = model.nstates
    nsymbols = model.output_model.nsymbols if output == 'discrete' else 0
    device = engine_kwargs.pop('device', 0)
    if engine_kwargs:
        raise TypeError("unexpected keyword arguments: %s" % ", ".join(sorted(engine_kwargs)))
    if lag > 1:
        observations = lag_observations(observations, lag)
    eng = _engine_for(output, device)
    try:
        if output == 'discrete':
            obs = [np.asarray(o) for o in observations]
            eng.set_observations('discrete', obs, nstates, nsymbols=nsymbols)
        else:
            eng.set_observations(output, [np.asarray(o, dtype=np.float64) for o in observations], nstates)
        return eng.decode_runs(*model_tuple(model), method=method, stats=stats)
    finally:
        eng.close()


def path_logprob(observations, models, paths=None, method='viterbi', lag=1, **engine_kwargs):
    """Joint log-probability log p(s, O | model) of hidden paths of `observations`, per trajectory
    (bhmm_path_logprob, bhmm_decode_logprob): log pi(s_0) + e(s_0, o_0) + sum_t [log A(s_t-1, s_t) + e(s_t, o_t)].
    With `paths` -- one integer array per trajectory, or one flat uint8 / int32 array concatenated like the
    observations -- they are scored under each of `models` (one HMM, a list of HMMs of the same output type and
    number of states, or a SampledHMM) in one pass over paths and observations: an (S, K) array.  With paths=None
    `models` must be ONE HMM: the observations are decoded with `method` ('viterbi': the result is the Viterbi
    score; 'posterior') and the decoded path is scored where it lies on the GPU: a (K,) array.  lag > 1 works on
    the lagged views (lag_observations), one trajectory per view.  Every term is formed in log space; the gaussian
    outlier rule of the recursions is NOT applied (an outlier gives a very negative finite term).  A zero
    probability on a path gives -inf for that trajectory -- a posterior-decoded path can take a jump the model
    forbids --, a NaN observation NaN, an empty trajectory 0.0.  engine_kwargs: device (default 0)."""
    from .estimators.maximum_likelihood import model_tuple
    if isinstance(models, SampledHMM):
        models = models.sampled_hmms
    elif isinstance(models, HMM):
        models = [models]
    elif not isinstance(models, (list, tuple)):
        raise TypeError("models must be an HMM, a list of HMMs or a SampledHMM")
    models = list(models)
    if not models:
        raise ValueError("path_logprob needs at least one model")
    for m in models:
        if not isinstance(m, HMM):
            raise TypeError("models must be HMM objects (or a SampledHMM)")
    if method not in ('viterbi', 'posterior'):
        raise ValueError("method must be 'viterbi' or 'posterior', not %r" % (method,))
    if paths is None and len(models) != 1:
        raise ValueError("without paths exactly one model decodes (got %d)" % len(models))
    output = models[0].output_model.model_type
    nstates = models[0].nstates
    nsymbols = models[0].output_model.nsymbols if output == 'discrete' else 0
    for m in models[1:]:
        if m.output_model.model_type != output:
            raise ValueError("all models must have the same output type (got %r and %r)"
                             % (output, m.output_model.model_type))
        if m.nstates != nstates:
            raise ValueError("all models must have the same number of states")
        if output == 'discrete' and m.output_model.nsymbols != nsymbols:
            raise ValueError("all models must have the same number of symbols")
    if len(observations) == 0:
        raise ValueError("no observations")
    device = engine_kwargs.pop('device', 0)
    if engine_kwargs:
        raise TypeError("unexpected keyword arguments: %s" % ", ".join(sorted(engine_kwargs)))
    if lag > 1:
        observations = lag_observations(observations, lag)
    if paths is not None:
        lengths = [len(o) for o in observations]
        if isinstance(paths, (list, tuple)):
            if len(paths) != len(lengths):
                raise ValueError("expected one path per trajectory (%d), got %d" % (len(lengths), len(paths)))
            pieces = [np.asarray(p) for p in paths]
        else:
            flat = np.asarray(paths)
            if flat.ndim != 1 or flat.shape[0] != sum(lengths):
                raise ValueError("a flat path must hold sum(T_k) = %d states" % sum(lengths))
            pieces = [flat]
        for k, p in enumerate(pieces):
            if p.size and not np.issubdtype(p.dtype, np.integer):
                raise ValueError("paths must hold integers, not %s" % p.dtype.name)
            if isinstance(paths, (list, tuple)) and (p.ndim != 1 or p.shape[0] != lengths[k]):
                raise ValueError("path %d must be 1-d with %d steps, not %r" % (k, lengths[k], p.shape))
        if not isinstance(paths, (list, tuple)):
            if flat.size and (flat.min() < 0 or flat.max() >= nstates):
                raise ValueError("paths holds a state outside [0, %d)" % nstates)
            paths = np.ascontiguousarray(flat, dtype=np.uint8 if flat.dtype == np.uint8 else np.int32)
    eng = _engine_for(output, device)
    try:
        if output == 'discrete':
            obs = [np.asarray(o) for o in observations]
            eng.set_observations('discrete', obs, nstates, nsymbols=nsymbols)
        else:
            eng.set_observations(output, [np.asarray(o, dtype=np.float64) for o in observations], nstates)
        if paths is None:
            return eng.decode_logprob(*model_tuple(models[0]), method=method)
        return eng.path_logprob(paths, [model_tuple(m) for m in models])
    finally:
        eng.close()


def posterior_marginals(observations, model, lag=1, weights=None, dtype=np.float64, **engine_kwargs):
    """Posterior state probabilities of `observations` under one HMM (bhmm_posterior_marginals): per
    trajectory a (T_k, nstates) array of gamma_t(i) -- what the reference's estimator hands out as
    hidden_state_probabilities, for any model and without an EM run -- or with `weights` ((nstates, Q),
    1 <= Q <= 8: set memberships, state means) the (T_k, Q) array gamma @ weights.  dtype float64 or float32.
    The arrays are views into one array.  lag > 1 works on the lagged views (lag_observations), one result
    per view.  Gaussian and discrete models of up to 8 states run one fused kernel that stores no gamma beyond
    the result; more states run an E-step that stores gamma.  engine_kwargs: device (default 0)."""
    from .estimators.maximum_likelihood import model_tuple
    if not isinstance(model, HMM):
        raise TypeError("model must be an HMM object")
    if len(observations) == 0:
        raise ValueError("no observations")
    output = model.output_model.model_type
    nstates = model.nstates
    nsymbols = model.output_model.nsymbols if output == 'discrete' else 0
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("dtype must be float64 or float32")
    if weights is not None:
        w = np.asarray(weights)
        if w.ndim != 2 or w.shape[0] != nstates or not 1 <= w.shape[1] <= 8:
            raise ValueError("weights must be (%d, Q) with 1 <= Q <= 8" % nstates)
    device = engine_kwargs.pop('device', 0)
    if engine_kwargs:
        raise TypeError("unexpected keyword arguments: %s" % ", ".join(sorted(engine_kwargs)))
    if lag > 1:
        observations = lag_observations(observations, lag)
    eng = _engine_for(output, device)
    try:
        if output == 'discrete':
            obs = [np.asarray(o) for o in observations]
            eng.set_observations('discrete', obs, nstates, nsymbols=nsymbols)
        else:
            eng.set_observations(output, [np.asarray(o, dtype=np.float64) for o in observations], nstates)
        return eng.posterior_marginals(*model_tuple(model), weights=weights, dtype=dtype)
    finally:
        eng.close()


def posterior_transitions(observations, model, lag=1, weights=None, dtype=np.float64, **engine_kwargs):
    """Pair posteriors of `observations` under one HMM (bhmm_posterior_transitions): per trajectory the
    probability of a jump at every step, P(s_t != s_t+1 | O), as an array of length T_k - 1 -- where the jumps
    are and how sure the model is of them -- or with `weights` ((nstates, nstates, Q), 1 <= Q <= 8: unit pair
    matrices for the expected A -> B events, any few pair weightings) the (T_k - 1, Q) array
    sum_ij xi_t(i, j) weights[i, j, q].  dtype float64 or float32.  The arrays are views into one array.  lag > 1
    works on the lagged views (lag_observations), one result per view.  Gaussian and discrete models of up to 8
    states run one fused kernel; more states run filter_states and posterior_marginals on the device, each on the path
    it picks itself, and a kernel over their rows.  engine_kwargs: device (default 0)."""
    from .estimators.maximum_likelihood import model_tuple
    if not isinstance(model, HMM):
        raise TypeError("model must be an HMM object")
    if len(observations) == 0:
        raise ValueError("no observations")
    output = model.output_model.model_type
    nstates = model.nstates
    nsymbols = model.output_model.nsymbols if output == 'discrete' else 0
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("dtype must be float64 or float32")
    if weights is not None:
        w = np.asarray(weights)
        if w.ndim != 3 or w.shape[:2] != (nstates, nstates) or not 1 <= w.shape[2] <= 8:
            raise ValueError("weights must be (%d, %d, Q) with 1 <= Q <= 8" % (nstates, nstates))
        if not np.all(np.isfinite(np.asarray(w, dtype=np.float64))):
            raise ValueError("weights has a non-finite entry")
    device = engine_kwargs.pop('device', 0)
    if engine_kwargs:
        raise TypeError("unexpected keyword arguments: %s" % ", ".join(sorted(engine_kwargs)))
    if lag > 1:
        observations = lag_observations(observations, lag)
    eng = _engine_for(output, device)
    try:
        if output == 'discrete':
            obs = [np.asarray(o) for o in observations]
            eng.set_observations('discrete', obs, nstates, nsymbols=nsymbols)
        else:
            eng.set_observations(output, [np.asarray(o, dtype=np.float64) for o in observations], nstates)
        return eng.posterior_transitions(*model_tuple(model), weights=weights, dtype=dtype)
    finally:
        eng.close()


def filter_states(observations, model, lag=1, weights=None, dtype=np.float64, probabilities=True, increments=True,
                  **engine_kwargs):
    """Filtered state probabilities and per-step likelihood of `observations` under one HMM (bhmm_filter):
    (rows, logc) with per trajectory a (T_k, nstates) array of P(s_t = i | o_0 .. o_t) -- or with `weights`
    ((nstates, Q), 1 <= Q <= 8) the (T_k, Q) array of their projection -- and a (T_k,) array of
    log p(o_t | o_0 .. o_{t-1}), whose sum is the log-likelihood; None for the one not asked for.  dtype float64
    or float32.  The arrays are views into one array each.  lag > 1 works on the lagged views
    (lag_observations), one result per view.  Gaussian and discrete models of up to 8 states run parallel over
    time; more states run the serial recursion per trajectory.  engine_kwargs: device (default 0)."""
    from .estimators.maximum_likelihood import model_tuple
    if not isinstance(model, HMM):
        raise TypeError("model must be an HMM object")
    if len(observations) == 0:
        raise ValueError("no observations")
    output = model.output_model.model_type
    nstates = model.nstates
    nsymbols = model.output_model.nsymbols if output == 'discrete' else 0
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("dtype must be float64 or float32")
    if not probabilities and not increments:
        raise ValueError("neither probabilities nor increments asked for")
    if weights is not None:
        w = np.asarray(weights)
        if w.ndim != 2 or w.shape[0] != nstates or not 1 <= w.shape[1] <= 8:
            raise ValueError("weights must be (%d, Q) with 1 <= Q <= 8" % nstates)
    device = engine_kwargs.pop('device', 0)
    if engine_kwargs:
        raise TypeError("unexpected keyword arguments: %s" % ", ".join(sorted(engine_kwargs)))
    if lag > 1:
        observations = lag_observations(observations, lag)
    eng = _engine_for(output, device)
    try:
        if output == 'discrete':
            obs = [np.asarray(o) for o in observations]
            eng.set_observations('discrete', obs, nstates, nsymbols=nsymbols)
        else:
            eng.set_observations(output, [np.asarray(o, dtype=np.float64) for o in observations], nstates)
        return eng.filter_states(*model_tuple(model), weights=weights, dtype=dtype, probabilities=probabilities,
                                 increments=increments)
    finally:
        eng.close()
