"""Initial HMM with Poisson count emissions.

Deterministic and numpy only.  The k-means of init/mvgaussian.py -- farthest-point seeding from the point nearest the
centroid, at most 20 Lloyd iterations, on at most 1e5 evenly strided points -- runs on the variance-stabilised counts
sqrt(x + 3/8) (Anscombe: about unit variance whatever the rate, so that one Euclidean distance serves dark and
bright states alike).  Farthest-point seeding follows outliers, and in the stabilised space a bright state is wider
than two dark states are apart, so it can spend two seeds on one bright state: the same Lloyd iterations are also run
from seeds at the quantiles of the summed stabilised counts, and the clustering of lower inertia is kept.  Every
observation gets the label of its nearest centre; the rates are the cluster means of the RAW counts; a channel whose
counts in a cluster are all zero gets 0.5 / (points in the cluster) instead of a rate of zero, which EM could never
leave.  Hard labels cut the tails off overlapping states -- the low counts of a state of rate 5 fall to a neighbour
of rate 0.3 and raise its mean by a third -- so the rates are then refined by at most 50 EM iterations of the
Poisson MIXTURE (no dynamics) on the same subsample, and the labels are those of the largest responsibility.  The
labels at the lag give a count matrix from which bhmm_amd.estimators._tmatrix estimates the transition matrix.
States are ordered by the first coordinate of their centre.
"""
import numpy as np

from ..estimators import _tmatrix
from ..hmm import HMM
from ..output_models.poisson import PoissonOutputModel, check_observation
from .mvgaussian import MAX_LLOYD, MAX_POINTS, _labels, kmeans

MAX_MIXTURE_EM = 50


def _lloyd(pts, centres):
    centres = centres.copy()
    lab = None
    for _ in range(MAX_LLOYD):
        new = _labels(pts, centres)
        if lab is not None and np.array_equal(new, lab):
            break
        lab = new
        for i in range(centres.shape[0]):
            sel = pts[lab == i]
            if sel.shape[0]:
                centres[i] = sel.mean(axis=0)
    return centres


def _inertia(pts, centres):
    return float(((pts - centres[_labels(pts, centres)]) ** 2).sum())


def _centres(z, k):
    """The centres of `kmeans` or, where they cluster the subsample more tightly, those of the same Lloyd iterations
    from the points at the (2 i + 1) / (2 k) quantiles of the summed coordinates."""
    stride = max(1, -(-z.shape[0] // MAX_POINTS))
    pts = z[::stride]
    a = kmeans(z, k)
    order = np.argsort(pts.sum(axis=1), kind='stable')
    seeds = pts[order[((2 * np.arange(k) + 1) * pts.shape[0]) // (2 * k)]]
    b = _lloyd(pts, seeds)
    return b if _inertia(pts, b) < _inertia(pts, a) else a


def _log_resp(x, rates, weights):
    """log of weight times Poisson density up to the term that does not depend on the component, (T, k)"""
    with np.errstate(divide='ignore'):
        return x.dot(np.log(rates).T) - rates.sum(axis=1)[None, :] + np.log(weights)[None, :]


def _mixture_em(x, rates, weights):
    for _ in range(MAX_MIXTURE_EM):
        a = _log_resp(x, rates, weights)
        r = np.exp(a - a.max(axis=1)[:, None])
        r /= r.sum(axis=1)[:, None]
        n = r.sum(axis=0)
        keep = n <= 1e-8 * x.shape[0]          # (a component nothing belongs to stays where it is)
        new = np.where(keep[:, None], rates, r.T.dot(x) / np.where(keep, 1.0, n)[:, None])
        new = np.maximum(new, 0.5 / np.maximum(n, 1.0)[:, None])   # (the rule for an all-zero channel, softly)
        done = np.allclose(new, rates, rtol=1e-6, atol=0.0)
        rates, weights = new, np.maximum(n / n.sum(), 1e-12)
        if done:
            break
    return rates, weights


def init_model_poisson(observations, nstates, lag=1, reversible=True):
    obs = [check_observation(o) for o in observations]
    if not obs or any(o.shape[1] != obs[0].shape[1] for o in obs):
        raise ValueError('observations must be (T_k, D) arrays of counts of one D')
    x = np.concatenate(obs, axis=0)
    if not np.all(np.isfinite(x)):
        raise ValueError('counts must be finite')
    D = x.shape[1]
    z = np.sqrt(x + 0.375)
    centres = _centres(z, nstates)
    centres = centres[np.argsort(centres[:, 0], kind='stable')]
    lab = _labels(z, centres)
    rates = np.empty((nstates, D))
    weights = np.empty(nstates)
    for i in range(nstates):
        sel = x[lab == i]
        weights[i] = max(sel.shape[0], 1) / float(x.shape[0])
        if sel.shape[0] == 0:
            rates[i] = np.maximum(centres[i] ** 2 - 0.375, 0.5 / x.shape[0])   # (the centre, taken back to counts)
            continue
        rates[i] = sel.mean(axis=0)
        rates[i][rates[i] == 0.0] = 0.5 / sel.shape[0]
    stride = max(1, -(-x.shape[0] // MAX_POINTS))
    rates, weights = _mixture_em(x[::stride], rates, weights / weights.sum())
    lab = np.argmax(_log_resp(x, rates, weights), axis=1)
    C = np.zeros((nstates, nstates))
    pos = 0
    for o in obs:
        l = lab[pos:pos + o.shape[0]]
        pos += o.shape[0]
        if l.shape[0] > lag:
            np.add.at(C, (l[:-lag], l[lag:]), 1.0)
    C += 1e-3   # (a transition never seen among the labels is not forbidden: EM could not bring it back)
    P = _tmatrix.estimate_P(C, reversible=reversible, mincount_connectivity=1e-16)
    pi = _tmatrix.stationary_distribution(P, C=C, mincount_connectivity=1e-16)
    return HMM(pi, P, PoissonOutputModel(nstates, rates))
