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
