"""Initial HMM with multivariate Gaussian emissions.

Deterministic and numpy only: k-means on the pooled observations -- farthest-point seeding from the point
nearest the centroid, at most 20 Lloyd iterations, on at most 1e5 evenly strided points -- then every
observation gets the label of its nearest centre, the clusters give means and covariances, and the hard
labels at the lag give a count matrix from which bhmm_amd.estimators._tmatrix estimates the transition matrix.
States are ordered by their first mean coordinate.
"""
import numpy as np

from ..estimators import _tmatrix
from ..hmm import HMM
from ..output_models import MultivariateGaussianOutputModel

MAX_POINTS = 100000
MAX_LLOYD = 20


def _labels(x, centres):
    # |x - c|^2 up to the term that does not depend on c
    d = -2.0 * x.dot(centres.T) + np.einsum('ij,ij->i', centres, centres)[None, :]
    return np.argmin(d, axis=1)


def kmeans(x, k):
    """Centres (k, D) of the evenly strided subsample of x (T, D): farthest-point seeding, Lloyd iterations."""
    stride = max(1, -(-x.shape[0] // MAX_POINTS))
    pts = x[::stride]
    if pts.shape[0] < k:
        raise ValueError('fewer observations than states')
    first = int(np.argmin(((pts - pts.mean(axis=0)) ** 2).sum(axis=1)))
    centres = [pts[first]]
    dist = ((pts - centres[0]) ** 2).sum(axis=1)
    for _ in range(1, k):
        nxt = int(np.argmax(dist))
        centres.append(pts[nxt])
        dist = np.minimum(dist, ((pts - pts[nxt]) ** 2).sum(axis=1))
    centres = np.array(centres)
    lab = None
    for _ in range(MAX_LLOYD):
        new = _labels(pts, centres)
        if lab is not None and np.array_equal(new, lab):
            break
        lab = new
        for i in range(k):
            sel = pts[lab == i]
            if sel.shape[0]:
                centres[i] = sel.mean(axis=0)
    return centres


def init_model_mvgaussian(observations, nstates, lag=1, reversible=True, covariance_type='full'):
    if covariance_type not in ('full', 'diag'):
        raise ValueError("covariance_type must be 'full' or 'diag', not %r" % (covariance_type,))
    obs = [np.asarray(o, dtype=np.float64) for o in observations]
    if not obs or any(o.ndim != 2 for o in obs) or any(o.shape[1] != obs[0].shape[1] for o in obs):
        raise ValueError('observations must be (T_k, D) arrays of one D')
    x = np.concatenate(obs, axis=0)
    D = x.shape[1]
    centres = kmeans(x, nstates)
    centres = centres[np.argsort(centres[:, 0], kind='stable')]
    lab = _labels(x, centres)
    means = np.empty((nstates, D))
    covs = np.empty((nstates, D, D))
    # a floor on the variances: a cluster of one point, or of points on a line, must still give a density
    floor = 1e-6 * max(float(x.var(axis=0).mean()), np.finfo(np.float64).tiny)
    for i in range(nstates):
        sel = x[lab == i]
        if sel.shape[0] == 0:
            means[i], covs[i] = centres[i], np.eye(D) * x.var(axis=0).mean()
            continue
        means[i] = sel.mean(axis=0)
        d = sel - means[i]
        covs[i] = d.T.dot(d) / sel.shape[0] + floor * np.eye(D)
    if covariance_type == 'diag':
        covs = np.array([np.diag(c) for c in covs])
    C = np.zeros((nstates, nstates))
    pos = 0
    for o in obs:
        l = lab[pos:pos + o.shape[0]]
        pos += o.shape[0]
        if l.shape[0] > lag:
            np.add.at(C, (l[:-lag], l[lag:]), 1.0)
    C += 1e-3   # (a transition never seen among the hard labels is not forbidden: EM could not bring it back)
    P = _tmatrix.estimate_P(C, reversible=reversible, mincount_connectivity=1e-16)
    pi = _tmatrix.stationary_distribution(P, C=C, mincount_connectivity=1e-16)
    om = MultivariateGaussianOutputModel(nstates, means, covs, covariance_type=covariance_type)
    return HMM(pi, P, om)


def _state_components(pts, M, state_mean, state_cov):
    """Weights (M,), means (M, D) and covariances (M, D, D) of M components of one state's points: the farthest-point
    seeding and Lloyd iterations of `kmeans` on them; a component of fewer than D + 1 points takes the state's
    covariance (one without points also the state's mean); weights are the cluster shares, floored at 1e-3 and
    renormalised."""
    D = state_mean.shape[0]
    means = np.tile(state_mean, (M, 1))
    covs = np.tile(state_cov, (M, 1, 1))
    counts = np.zeros(M)
    if pts.shape[0] >= M:
        centres = kmeans(pts, M)
        centres = centres[np.argsort(centres[:, 0], kind='stable')]
        lab = _labels(pts, centres)
        for c in range(M):
            sel = pts[lab == c]
            counts[c] = sel.shape[0]
            if sel.shape[0] == 0:
                means[c] = centres[c]
                continue
            means[c] = sel.mean(axis=0)
            if sel.shape[0] >= D + 1:
                d = sel - means[c]
                # (the floor of the state's covariance is in state_cov; a cluster on a line still needs one)
                covs[c] = d.T.dot(d) / sel.shape[0] + 1e-6 * np.eye(D) * max(np.trace(state_cov) / D,
                                                                             np.finfo(np.float64).tiny)
    elif pts.shape[0]:
        means[:pts.shape[0]] = pts
        counts[:pts.shape[0]] = 1.0
    w = counts / counts.sum() if counts.sum() > 0 else np.full(M, 1.0 / M)
    w = np.maximum(w, 1e-3)
    return w / w.sum(), means, covs


def init_model_gaussian_mixture(observations, nstates, ncomponents, lag=1, reversible=True, covariance_type='full'):
    """Initial HMM with `ncomponents` gaussian components per state, deterministic and numpy
    only: the model of init_model_mvgaussian and its hard labels first, then inside every state the same seeding and
    Lloyd iterations on that state's points."""
    from ..output_models import GaussianMixtureOutputModel
    M = int(ncomponents)
    if M < 1 or nstates * M > 4096:
        raise ValueError('ncomponents must be >= 1 and nstates * ncomponents <= 4096')
    base = init_model_mvgaussian(observations, nstates, lag=lag, reversible=reversible, covariance_type='full')
    om = base.output_model
    x = np.concatenate([np.asarray(o, dtype=np.float64) for o in observations], axis=0)
    D = x.shape[1]
    # the hard labels of init_model_mvgaussian: nearest cluster centre; the cluster means are its centres' successors
    # by one averaging, so the nearest mean is taken
    lab = _labels(x, om.means)
    w = np.empty((nstates, M))
    mu = np.empty((nstates, M, D))
    cov = np.empty((nstates, M, D, D))
    for i in range(nstates):
        w[i], mu[i], cov[i] = _state_components(x[lab == i], M, om.means[i], om.covariances[i])
    if covariance_type == 'diag':
        cov = np.einsum('icaa->ica', cov).copy()
    elif covariance_type != 'full':
        raise ValueError("covariance_type must be 'full' or 'diag', not %r" % (covariance_type,))
    return HMM(base.initial_distribution, base.transition_matrix,
               GaussianMixtureOutputModel(nstates, w, mu, cov, covariance_type=covariance_type))
