"""The component draw of bhmm_gmm_path_components restated in numpy (TEST INFRASTRUCTURE): the
counter-based uniforms of the device (uniform01 of path_kernels.hpp on the key mix64(seed ^ constant), restated as
host_rng_ref.py restates the host generator), the one-pass draw rule on given a_c, and the reference the GPU test holds
the kernel to -- a_tic in long double, the decisions u < e_c / s_c, and which of them lie too close to call."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
DRAW_KEY_CONST = 0xC3A5C85C97CB3127
EPS = np.finfo(np.float64).eps


def mix64(z):
    """SplitMix64 finaliser on a uint64 array (or a Python int)"""
    if isinstance(z, int):
        z &= M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw_key(seed):
    return mix64((int(seed) & M64) ^ DRAW_KEY_CONST)


def uniform01(key, x):
    """[0, 1) from counter x (uint64 array) of stream `key`"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = np.uint64(key) + np.uint64(GOLDEN) * (x + np.uint64(1))
    return (mix64(z) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def stream_positions(lengths, soff=None):
    """g of every step: its index in the concatenation, or soff[k] + t"""
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    if soff is None:
        return np.arange(off[-1], dtype=np.uint64)
    return np.concatenate([np.arange(T, dtype=np.int64) + int(s) for T, s in zip(lengths, soff)]
                          + [np.zeros(0, dtype=np.int64)]).astype(np.uint64)


def draw_rule(a, key, g):
    """The rule in float64: a (T, M) with -inf marking the components that are not visited (weight zero), g (T,) uint64.
    Returns the picks (T,).  One pass: running maximum mx, rescaled sum s, the pick."""
    a = np.asarray(a, dtype=np.float64)
    T, M = a.shape
    mx = np.full(T, -np.inf)
    s = np.zeros(T)
    pick = np.zeros(T, dtype=np.int64)
    seen = np.zeros(T, dtype=bool)
    g = np.asarray(g, dtype=np.uint64)
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(M):
            vis = a[:, c] != -np.inf
            up = vis & (a[:, c] > mx)
            e = np.where(up, 1.0, np.exp(a[:, c] - mx))
            s = np.where(up, s * np.exp(mx - a[:, c]) + 1.0, np.where(vis, s + e, s))
            mx = np.where(up, a[:, c], mx)
            u = uniform01(key, g * np.uint64(M) + np.uint64(c))
            take = vis & (~seen | (u * s < e))
            pick = np.where(take, c, pick)
            seen |= vis
    return pick


def reference_labels(a_ld, bound, path, M, key, g):
    """a_ld (T, M) long double: a_tic of the state the path is in (-inf: weight zero); bound (T, M): the bound on the
    device's error in a_tic.  Returns (labels (T,), undecided (T,)): the draw with p_c = e_c / s_c formed in long double,
    and the steps with a decision |u - p_c| <= p_c (4 max_{c' <= c} B_c' + 16 M eps) -- twice the bound on a difference
    of two a, plus the exps and the sum."""
    T = a_ld.shape[0]
    LD = np.longdouble
    pick = np.zeros(T, dtype=np.int64)
    seen = np.zeros(T, dtype=bool)
    undecided = np.zeros(T, dtype=bool)
    bmax = np.zeros(T)
    g = np.asarray(g, dtype=np.uint64)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for c in range(M):
            vis = a_ld[:, c] != -np.inf
            bmax = np.where(vis, np.maximum(bmax, bound[:, c]), bmax)
            # p_c = e_c / s_c = 1 / sum_{c' <= c, visited} exp(a_c' - a_c)
            diff = np.where((a_ld[:, :c + 1] != -np.inf), a_ld[:, :c + 1] - a_ld[:, c:c + 1], -np.inf)
            p = (LD(1) / np.exp(diff).sum(axis=1)).astype(np.float64)
            u = uniform01(key, g * np.uint64(M) + np.uint64(c))
            later = vis & seen
            close = later & (np.abs(u - p) <= p * (4.0 * bmax + 16 * M * EPS))
            undecided |= close
            take = vis & (~seen | (u < p))
            pick = np.where(take, c, pick)
            seen |= vis
    return np.asarray(path, dtype=np.int64) * M + pick, undecided
