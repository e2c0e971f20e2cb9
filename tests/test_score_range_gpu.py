"""GPU: bhmm_score where a trajectory ends just after the lazily scaled kernels last refreshed their power of two
(k_score_wide<.., LAZY>, 9 to 64 states; k_score_tile, 65 to 128 states).  The last k steps
of a trajectory are all but impossible under every state of a tuned model, so that the forward vector is carried
towards, into and through the denormal range between two refreshes; the per-trajectory log-likelihoods are held
to an exact recursion in 80-bit arithmetic whose emission probabilities are formed in 80 bits too.  Inputs,
reference and the targets are those of tests/score_range_cases.py; test_score_range_cpu.py shows that they reach
the window.

One batch per case holds every target and tail length, with lengths 1 to 11 (every residue mod 4, with and without
a refresh, from the trajectory's start) and 37, 64, 129, 262 (with score_seglen = 64 the tail sits in a last segment
behind verified boundaries); every batch runs again as one segment per trajectory.  Each call takes the tuned
model and two random ones, whose results must be bitwise those of a call without it.  The same inputs go through
the kernels for up to 8 states (both layouts) and through the E-step's log-likelihood (k_wide_fwd<.., LAZY>,
k_tile_fwd), and one case drives the lazily scaled vector to infinity inside a window.

The GPU work of a case is done once and shared by the tests that look at one tail length each."""
import numpy as np
import pytest

from tests import score_range_cases as sc

pytestmark = pytest.mark.gpu

RTOL = 1e-11   # the bound of test_score_wide_gpu.py and test_score_tile_gpu.py
SEGLENS = (64, 100000)


def _engine():
    from bhmm_amd.engine import Engine
    return Engine(0)


_DONE = {}


def _once(key, fn):
    """fn() once per key; a failure is kept and raised again, never run again."""
    if key not in _DONE:
        try:
            _DONE[key] = (fn(), None)
        except BaseException as ex:   # noqa: B902 -- kept for the tests that share the run
            _DONE[key] = (None, ex)
    res, ex = _DONE[key]
    if ex is not None:
        raise ex
    return res


def _hold(tag, got, ref, sel=None):
    """Every finite reference value within RTOL, -inf where the reference is -inf; prints the worst deviation as a
    fraction of the bound."""
    got, ref = np.asarray(got), np.asarray(ref)
    if sel is not None:
        got, ref = got[sel], ref[sel]
    fin = np.isfinite(ref)
    assert fin.any()
    with np.errstate(invalid="ignore", divide="ignore"):
        dev = np.abs(got[fin] - ref[fin]) / (RTOL * np.abs(ref[fin]))
    dev = np.where(np.isnan(dev), np.inf, dev)
    print(tag, "trajectories", len(ref), "minus infinity", int((~fin).sum()), "worst deviation / bound", dev.max())
    assert np.all(got[~fin] == -np.inf)
    assert not np.any(np.isnan(got))
    np.testing.assert_allclose(got[fin], ref[fin], rtol=RTOL)


def _fallbacks(eng, models):
    before = eng.get_option("score_fallbacks")
    out = eng.score(models)
    return out, eng.get_option("score_fallbacks") - before


# ---- the two time-segmented routes ------------------------------------------------------------------
def _run_route(route, n, kind, M, seglen):
    c = sc.build(route, kind, n, M)
    path = 2 if route == "wide" else 3
    models = [c.tuned] + c.others
    r = {}
    eng = _engine()
    eng.set_observations(kind, c.obs, n, nsymbols=M)
    eng.set_option("score_seglen", seglen)
    r["main"], r["main_fb"] = _fallbacks(eng, models)
    r["path"] = eng.get_option("score_path")
    r["segments"] = eng.get_option("score_segments")
    r["alone"] = eng.score(c.others)
    if route == "wide":
        eng.set_option("score_lazy", 0)
        r["every"] = eng.score(models)
        r["every_path"] = eng.get_option("score_path")
        eng.set_option("score_lazy", 1)
    eng.set_observations(kind, c.ctrl, n, nsymbols=M)
    eng.set_option("score_seglen", seglen)
    r["ctrl"], r["ctrl_fb"] = _fallbacks(eng, models)
    # the trajectories on which no refresh of the restated schedule finds anything: only the look at the exit sum
    # stands between them and the caller, and no other trajectory of the batch gets the model flagged for them
    _, S, trouble = sc.restated(route, kind, n, M)
    r["quiet_sel"] = ~trouble & (S > 0) & np.isfinite(S)
    eng.set_observations(kind, [o for o, q in zip(c.obs, r["quiet_sel"]) if q], n, nsymbols=M)
    eng.set_option("score_seglen", seglen)
    r["quiet"], r["quiet_fb"] = _fallbacks(eng, models)
    if route == "wide":   # (the matrix-core route leaves no counter: it takes the serial recursion at once)
        r["fb"] = {}
        for e in sc.TARGETS:
            eng.set_observations(kind, [o for o, x in zip(c.obs, c.e) if x == e], n, nsymbols=M)
            eng.set_option("score_seglen", seglen)
            r["fb"][e] = _fallbacks(eng, [c.tuned])[1]
    eng.close()
    assert path == r["path"]
    return c, r


def _route(route, n, kind, M, seglen):
    return _once((route, n, kind, M, seglen), lambda: _run_route(route, n, kind, M, seglen))


WIDE = [pytest.param(*x, id="%d-%s%d" % x) for x in sc.WIDE_CASES]
TILE = [pytest.param(*x, id="%d-%s%d" % x) for x in sc.TILE_CASES]


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("seglen", SEGLENS)
@pytest.mark.parametrize("n,kind,M", WIDE)
def test_wide_tail(n, kind, M, seglen, k):
    c, r = _route("wide", n, kind, M, seglen)
    tag = "wide n %d %s M %d seglen %d tail %d" % (n, kind, M, seglen, k)
    _hold(tag + " lazy", r["main"][0], c.ref, c.k == k)
    _hold(tag + " every step", r["every"][0], c.ref, c.k == k)
    q = r["quiet_sel"]
    _hold(tag + " lazy, unnoticed at a refresh", r["quiet"][0], c.ref[q], c.k[q] == k)


@pytest.mark.parametrize("seglen", SEGLENS)
@pytest.mark.parametrize("n,kind,M", WIDE)
def test_wide_protocol(n, kind, M, seglen):
    c, r = _route("wide", n, kind, M, seglen)
    assert r["path"] == 2 and r["every_path"] == 2
    assert r["segments"] > len(c.obs) if seglen == 64 else r["segments"] == len(c.obs)
    # a flagged model does not disturb its neighbours
    assert np.array_equal(r["main"][1:], r["alone"])
    np.testing.assert_allclose(r["every"][1:], r["alone"], rtol=RTOL)   # (another kernel: other sums)
    _hold("wide n %d %s M %d seglen %d control" % (n, kind, M, seglen), r["ctrl"][0], c.ref_ctrl)
    # the guard fires below the range and nowhere else
    print("fallbacks: batch", r["main_fb"], "control", r["ctrl_fb"], "per target", r["fb"])
    assert r["main_fb"] > 0 and r["quiet_fb"] > 0
    assert r["ctrl_fb"] == 0
    for e in sc.TARGETS:
        assert (r["fb"][e] == 0) if e in sc.IN_RANGE else (r["fb"][e] > 0), e


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("seglen", SEGLENS)
@pytest.mark.parametrize("n,kind,M", TILE)
def test_tile_tail(n, kind, M, seglen, k):
    c, r = _route("tile", n, kind, M, seglen)
    tag = "tile n %d %s M %d seglen %d tail %d" % (n, kind, M, seglen, k)
    _hold(tag, r["main"][0], c.ref, c.k == k)
    q = r["quiet_sel"]
    _hold(tag + " unnoticed at a refresh", r["quiet"][0], c.ref[q], c.k[q] == k)


@pytest.mark.parametrize("seglen", SEGLENS)
@pytest.mark.parametrize("n,kind,M", TILE)
def test_tile_protocol(n, kind, M, seglen):
    c, r = _route("tile", n, kind, M, seglen)
    assert r["path"] == 3
    assert r["segments"] > len(c.obs) if seglen == 64 else r["segments"] == len(c.obs)
    assert np.array_equal(r["main"][1:], r["alone"])
    _hold("tile n %d %s M %d seglen %d control" % (n, kind, M, seglen), r["ctrl"][0], c.ref_ctrl)
    assert r["ctrl_fb"] == 0


# ---- (a) up to 8 states, both layouts ---------------------------------------------------------------
def _run_small(n, kind, M, layout):
    c = sc.build("wide", kind, n, M)
    eng = _engine()
    eng.set_observations(kind, c.obs, n, nsymbols=M)
    eng.set_option("score_layout", layout)
    out = eng.score([c.tuned] + c.others)
    assert eng.get_option("score_path") == 1
    alone = eng.score(c.others)
    eng.set_observations(kind, c.ctrl, n, nsymbols=M)
    eng.set_option("score_layout", layout)
    ctrl = eng.score([c.tuned])
    eng.close()
    return c, out, alone, ctrl


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("layout", [1, 2])
@pytest.mark.parametrize("kind,M", [("gaussian", 0), ("discrete", 32)])
@pytest.mark.parametrize("n", [3, 8])
def test_small_tail(n, kind, M, layout, k):
    c, out, alone, ctrl = _once(("small", n, kind, M, layout), lambda: _run_small(n, kind, M, layout))
    _hold("n %d %s layout %d tail %d" % (n, kind, layout, k), out[0], c.ref, c.k == k)
    assert np.array_equal(out[1:], alone)
    if k == 1:
        _hold("n %d %s layout %d control" % (n, kind, layout), ctrl[0], c.ref_ctrl)


# ---- (b) the E-step's log-likelihood ----------------------------------------------------------------
def _run_estep(n, kind, M, k):
    """One E-step per tail length (it answers for all of its trajectories or for none), over the trajectories with a
    finite reference (it has no answer for a trajectory of probability zero)."""
    c = sc.build("tile" if n > 64 else "wide", kind, n, M)
    sel = np.isfinite(c.ref) & (c.k == k)
    eng = _engine()
    eng.set_observations(kind, [o for o, f in zip(c.obs, sel) if f], n, nsymbols=M)
    try:
        logL = eng.estep(*c.tuned).logL_k.copy()
    finally:
        eng.close()
    return c, sel, logL


ESTEP = [(n, kind, M, k) for n, kind, M in ((12, "gaussian", 0), (12, "discrete", 32), (64, "gaussian", 0),
                                            (64, "discrete", 32), (100, "gaussian", 0), (100, "discrete", 64))
         for k in range(1, 5 if n > 64 else 4)]


@pytest.mark.parametrize("n,kind,M,k", ESTEP)
def test_estep_logl_tail(n, kind, M, k):
    """k_wide_fwd<.., LAZY> (12, 64 states) and k_tile_fwd (100 states) at their tails: their backward passes flag
    such rows and the E-step is repeated on the kernels that normalise every step -- for 65 to 128 states the
    order-faithful ones, whose E-step form takes a row at the bottom of the double range times 2^900
    (k_gen_forward<.., RESCUE>, k_gen_backward<.., STATS>): without that the batch with the row at 2^-1073 was
    refused, "log-likelihood of trajectory 6 is not finite"."""
    c, sel, logL = _run_estep(n, kind, M, k)
    _hold("estep n %d %s tail %d" % (n, kind, k), logL, c.ref[sel])


# ---- (c) overflow inside a window -------------------------------------------------------------------
@pytest.mark.parametrize("n,path", [(12, 2), (64, 2), (100, 3)])
def test_overflow_inside_a_window(n, path):
    """One state of sigma 1e-100 (a density of 4e99 on its mean) and four consecutive observations on that mean:
    steps 0..3 and 4..7 are one window of the lazy scaling each, 2^1324 inside it; 5..8 straddles a refresh."""
    rng = np.random.default_rng(n)
    A, pi, mu, sig = sc.rand_model("gaussian", n, 0, rng)
    j = n // 2
    sig[j] = 1e-100
    model = (A, pi, mu, sig)
    obs = []
    for T, first in ((4, 0), (12, 0), (12, 4), (13, 5), (70, 64), (9, 5)):
        o = rng.normal(0, 3, T)
        o[first:first + 4] = mu[j]
        obs.append(o)
    ref = np.array([sc.loglik_exact(A, pi, sc.rows_exact("gaussian", model, o)) for o in obs])
    assert np.all(np.isfinite(ref)) and ref.min() > np.log(np.finfo(np.float64).max)   # (beyond a double, each)
    eng = _engine()
    eng.set_observations("gaussian", obs, n)
    for seglen in SEGLENS:
        eng.set_option("score_seglen", seglen)
        out, fb = _fallbacks(eng, [model, sc.rand_model("gaussian", n, 0, rng)])
        assert eng.get_option("score_path") == path
        _hold("overflow n %d seglen %d" % (n, seglen), out[0], ref)
        assert np.all(np.isfinite(out))
        if path == 2:
            assert fb > 0   # the lazily scaled kernel must have counted it out of range
    eng.close()
