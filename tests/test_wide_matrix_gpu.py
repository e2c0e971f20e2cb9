"""GPU parity of the lane-group E-step of 9..64 states (csrc/wide_kernels.hpp: k_wide_fwd / k_wide_bwd, one group of
16, 32 or 64 lanes per segment; WIDE_DISPATCH and wide_launch_* in csrc/wide_api.hip pick the instantiation) over
EVERY instantiation, route and edge, against the float64 CPU oracle (oracle/oracle.py), in the style and under the
bounds of tests/test_tile_matrix_gpu.py (its _plan, _frac, _compare, _collect, _want, _oracle and BOUNDS and the
_model and _observations of tests/test_tile_gpu.py are imported, not copied):

    logL rtol 1e-11; C and state counts rtol 1e-9 / atol 1e-11; gamma0 rtol 1e-9 / atol 1e-13; stored gamma rows
    rtol 1e-8 / atol 1e-13 (every trajectory, every step); sum_gd / sum_gdd rtol 1e-8 / atol 1e-9; symbol counts
    rtol 1e-9 / atol 1e-12; every gamma row sums to 1 within 1e-12.

The family is the only E-step route of 9..32 states, the route of 33..64 states with option tile = 0 and the serial
and "careful" fallback of the matrix-core route of 33..64 states.  Its three routes (wide_estep):

  * lazy segmented: k_wide_fwd / k_wide_bwd<NP, KIND, LAZY = true> on the time-segmented plan (alpha and beta carried
    up to a power of two that is refreshed every fourth step), boundaries from warm-ups of W steps, verified.
  * serial: the per-step-normalising instantiations on plan 0, one segment per trajectory (option wide_segments = 0).
  * careful segmented: the per-step-normalising instantiations on the time-segmented plan, after a lazily scaled
    E-step on these observations raised wide_trouble (a vector fell below 2^-900 between two refreshes).

A wrong route still gives a right result (the serial plan takes over after a failed check), so every E-step checked
here asserts the route that produced it (_assert_route): tile == 0 throughout; the segment count is the one _plan
gives, the segment length and warm-up read back are the ones set.  NP = 16 for up to 16 states, 32 for up to 32, 64
above; n == 64 is the instantiation without padded lanes (FULL).

Segments are not cut at multiples of L: see _plan.  (L, W) = (100, 64) except for the forward pass's own plan: with
the models of _model the largest componentwise deviation between warm-ups of 64 steps started from the uniform and
from a near-one-hot vector is below 1e-15 (the check allows 1e-11).

The bounds are not rounding-limited on these inputs: test_the_bounds_are_not_rounding_limited runs a float64 numpy
E-step that adds the states in the reverse order and stays below a tenth of every bound against the oracle.

Every case prints its worst deviation as a fraction of its bound ("lazy n=17 discrete: C 0.03 of bound")."""
import numpy as np
import pytest

from tests.test_tile_gpu import _model, _observations
from tests.test_tile_matrix_gpu import BOUNDS, _collect, _compare, _frac, _oracle, _plan, _want

gpu = pytest.mark.gpu          # (per test: the checks of the comparison itself at the end of the file need no GPU)

KINDS = ("gaussian", "discrete", "explicit")
ROUTES = ("lazy", "serial", "careful")
L0, W0 = 100, 64
MATRIX_N = (9, 16, 17, 32, 33, 63, 64)
MATRIX_LENGTHS = (601, 1, 250, 2, 333, 3, 5)
MATRIX_M = 23
FAR_AT = 300                   # first step of the stretch that leaves the lazily scaled kernels' range (trajectory 0)


def _readonly(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def _assert_route(eng, route, ntraj, label, L=None, W=None, nseg=None):
    """which kernels produced the last E-step, by the options csrc/wide_api.hip exposes"""
    g = eng.get_option
    assert g("tile") == 0, "%s: on the matrix-core kernels" % label
    assert g("spec_fail") == 0, "%s: spec_fail %d (last deviation %.3g)" % (label, g("spec_fail"), g("spec_last_dev"))
    if route == "serial":
        assert g("wide_segments") == 0, "%s: %d segments on the serial route" % (label, g("wide_segments"))
        return
    assert g("spec_ok") >= 1, "%s: no verified segmented E-step" % label
    if route == "lazy":
        assert g("careful") == 0, "%s: careful" % label
        assert g("wide_trouble") == 0, "%s: wide_trouble %d" % (label, g("wide_trouble"))
    else:
        assert g("careful") == 1, "%s: not careful" % label
        assert g("wide_trouble") != 0, "%s: wide_trouble 0" % label
        assert g("wide_segments") > ntraj, "%s: %d segments for %d trajectories" % (label, g("wide_segments"), ntraj)
    if nseg is not None:
        assert g("wide_segments") == nseg, "%s: %d segments, meant %d" % (label, g("wide_segments"), nseg)
    if L is not None:
        assert (g("wide_segment_len"), g("spec_W")) == (L, W), \
            "%s: L, W = %d, %d, set %d, %d" % (label, g("wide_segment_len"), g("spec_W"), L, W)


def _run(kind, obs, model, n, M, route, label, L=L0, W=W0, ref=None, repeat=False, logl_atol=0.0, options=()):
    """one engine, one E-step with stored gamma on the route asked for, the route assertions and every comparison;
    returns (what was compared, the engine's options read back)"""
    from bhmm_amd.engine import Engine
    A, pi, p0, p1 = model
    if ref is None:
        ref = _oracle(kind, obs, model, n, M)
    label = "%s %s" % (route, label)
    lengths = [len(o) for o in obs]
    nseg = len(_plan(lengths, L))
    assert route == "serial" or nseg > len(obs), "%s: the plan cuts no trajectory" % label
    eng = Engine(0)
    try:
        if n >= 33:
            eng.set_option("tile", 0)
        eng.set_option("wide_segment_len", L)
        eng.set_option("spec_W", W)
        if route == "serial":
            eng.set_option("wide_segments", 0)
        for name, value in options:
            eng.set_option(name, value)
        eng.set_observations(kind, obs, n, nsymbols=M if kind == "discrete" else 0)
        res = eng.estep(A, pi, p0, p1, store_gamma=True)
        _assert_route(eng, route, len(obs), label, L, W, nseg)
        opts = dict(fwd=int(eng.get_option("wide_fwd_segments")), nseg=int(eng.get_option("wide_segments")))
        got = _collect(eng, res, kind)
        _compare(got, _want(ref), label, logl_atol=logl_atol)
        rowsum = float(np.abs(got["gamma"].sum(axis=1) - 1.0).max())
        assert rowsum <= 1e-12, "%s: a gamma row sums to 1 +- %.3g" % (label, rowsum)
        if route == "careful":
            # the per-step-normalising kernels on the same plan, without the lazily scaled attempt before them
            r2 = eng.estep(A, pi, p0, p1, store_gamma=True)
            _assert_route(eng, route, len(obs), label + " (second call)", L, W, nseg)
            assert np.array_equal(r2.packed, res.packed) and np.array_equal(r2.logL_k, res.logL_k), label
            assert np.array_equal(_collect(eng, r2, kind)["gamma"], got["gamma"]), label
        elif repeat:
            r2 = eng.estep(A, pi, p0, p1)       # statistics only: the same numbers, run to run
            _assert_route(eng, route, len(obs), label + " (second call)", L, W, nseg)
            np.testing.assert_allclose(r2.packed, res.packed, rtol=1e-12, atol=1e-12)
            r3 = eng.estep(A, pi, p0, p1)
            _assert_route(eng, route, len(obs), label + " (third call)", L, W, nseg)
            assert np.array_equal(r2.packed, r3.packed) and np.array_equal(r2.logL_k, r3.logL_k), label
    finally:
        eng.close()
    return got, opts


# ---- 1. the instantiation matrix ---------------------------------------------------------------------------------
def _far_stretch(kind, model, obs):
    """Copies of the model and the observations with a stretch from step FAR_AT of trajectory 0 that takes the lazily
    scaled vectors below 2^-900 within one refresh window wherever the window starts (seven or eight steps hold four
    consecutive ones of any alignment), and that the oracle and the per-step-normalising kernels pass through.

    gaussian: sigma of the highest-mean state 1.2, seven observations 41 above that mean (34 sigma: 2^-841 a step,
    every other state further out); discrete: symbol 0 has probability 1e-80 in every state, eight of them in a row;
    explicit: eight rows times 1e-80."""
    A, pi, p0, p1 = model
    obs = [o.copy() for o in obs]
    assert len(obs[0]) > FAR_AT + 8
    if kind == "gaussian":
        p1 = p1.copy()
        p1[np.argmax(p0)] = 1.2
        obs[0][FAR_AT:FAR_AT + 7] = p0.max() + 41.0
    elif kind == "discrete":
        p0 = p0.copy()
        p0[:, 0] = 1e-80
        p0 /= p0.sum(axis=1)[:, None]
        obs[0][FAR_AT:FAR_AT + 8] = 0
    else:
        obs[0][FAR_AT:FAR_AT + 8] *= 1e-80
    return (A, pi, p0, p1), obs


_matrix_cache = {}


def _matrix_input(n, kind, far):
    """(model, observations, oracle result) of the instantiation matrix, made once per (n, kind, far) and left
    unchanged: the lazy and the serial route, and the CPU check of the bounds, share them"""
    key = (n, kind, far)
    if key not in _matrix_cache:
        model = _model(n, np.random.default_rng(6000 + n), kind, MATRIX_M)
        obs = _observations(kind, np.random.default_rng(6100 + 3 * n + KINDS.index(kind)), MATRIX_LENGTHS, n, MATRIX_M)
        if far:
            model, obs = _far_stretch(kind, model, obs)
        ref = _oracle(kind, obs, model, n, MATRIX_M)
        assert all(np.all(np.isfinite(v)) for v in _want(ref).values())
        _readonly(*model)
        _readonly(*obs)
        _matrix_cache[key] = (model, obs, ref)
    return _matrix_cache[key]


@gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", MATRIX_N)
def test_every_instantiation_kind_and_route(n, kind, route):
    """16, 32 and 64 lanes per segment, each with and without padded lanes (64 states: FULL), every emission kind,
    the lazily scaled and the per-step-normalising instantiation, the latter on both of its plans; a ragged batch in
    segments of 100 with warm-ups of 64."""
    model, obs, ref = _matrix_input(n, kind, route == "careful")
    _run(kind, obs, model, n, MATRIX_M, route, "n=%d %s" % (n, kind), ref=ref, repeat=True)


# ---- 2. geometry -------------------------------------------------------------------------------------------------
# one state count per lane-group width (12: four groups per wavefront, 24: two, 40: one, with padded lanes each)
GEO_CASES = [(n, kind) for n in (12, 24, 40) for kind in ("gaussian", "discrete")]
GEO_M = 31
FILL = (2, 3, 4, 5, 7, 8, 9)   # segments of the one trajectory of test_wavefront_fill
_geo_models = {}


def _geo_model(n, kind):
    """one model per (n, kind), shared by the geometry tests and left unchanged"""
    if (n, kind) not in _geo_models:
        m = _model(n, np.random.default_rng(6000 + n), kind, GEO_M)
        _readonly(*m)
        _geo_models[(n, kind)] = m
    return _geo_models[(n, kind)]


def _geo_run(n, kind, lengths, label, seed, route="lazy", L=L0):
    obs = _observations(kind, np.random.default_rng(seed), lengths, n, GEO_M)
    return _run(kind, obs, _geo_model(n, kind), n, GEO_M, route, "n=%d %s %s" % (n, kind, label), L=L)


@gpu
@pytest.mark.parametrize("n,kind", GEO_CASES)
def test_lengths_around_the_group_of_four_and_the_prefetch_ring(n, kind):
    """The lazily scaled vectors are refreshed on every fourth step and the observations (backward: and alpha rows)
    are fetched eight steps ahead, clamped at the segment's ends: trajectories of 1 .. 17 steps next to one of
    3 L + 1, lane groups of 1 .. 17 steps side by side in a wavefront."""
    lengths = (1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 3 * L0 + 1)
    _geo_run(n, kind, lengths, "1..17 and 3L+1", 6200 + n)


@gpu
@pytest.mark.parametrize("n,kind", GEO_CASES)
def test_lengths_around_the_segment_grid(n, kind):
    L, W = L0, W0
    lengths = (L - 1, L, L + 1, 2 * L, 2 * L + 1, L + 2, W - 1, W, W + 1, 2 * W - 8, 2 * W, 2 * W + 8)
    _geo_run(n, kind, lengths, "grid", 6300 + n)


def test_the_segment_grid_lengths_land_where_they_are_meant_to():
    """(no GPU) a second segment that starts from pi, one whose warm-up reaches the trajectory start exactly, one that
    just misses it; and the wavefront-fill lengths give exactly nseg segments"""
    L, W = L0, W0
    lengths = (L - 1, L, L + 1, 2 * L, 2 * L + 1, L + 2, W - 1, W, W + 1, 2 * W - 8, 2 * W, 2 * W + 8)
    segs = _plan(lengths, L)
    second = {k: t0 for k, t0, _ in segs if t0 > 0 and k >= 9}
    assert second == {9: W - 4, 10: W, 11: W + 4}, second
    assert [sum(1 for s in segs if s[0] == k) for k in range(9)] == [1, 1, 2, 2, 3, 2, 1, 1, 1]
    for nseg in FILL:
        assert len(_plan((nseg * L - 2,), L)) == nseg
    assert all(t0 % 4 == 0 for _, t0, _ in _plan(MATRIX_LENGTHS + (3000, 1500, 700), L))


@gpu
@pytest.mark.parametrize("nseg", FILL)
@pytest.mark.parametrize("n,kind", GEO_CASES)
def test_wavefront_fill(n, kind, nseg):
    """One trajectory of exactly nseg segments: the last wavefront holds 1 .. 64 / NP lane groups, and groups past
    the last segment exist at four (nseg 2, 3, 5, 7, 9) and two (3, 5, 7, 9) groups per wavefront."""
    _geo_run(n, kind, (nseg * L0 - 2,), "%d segments" % nseg, 6400 + n + nseg)


@gpu
@pytest.mark.parametrize("order", ["long first", "long last"])
@pytest.mark.parametrize("n,kind", GEO_CASES)
def test_lane_groups_that_differ_inside_a_wavefront(n, kind, order):
    """3000 steps next to fifteen trajectories of 1 .. 15 steps: the step loops of the groups of one wavefront end at
    different steps while the sums, maxima and ballots over a group go on.  Segmented, and on the serial route, where
    one wavefront runs 3000 steps beside 1, 2 and 3."""
    lengths = (3000,) + tuple(range(1, 16))
    if order == "long last":
        lengths = lengths[::-1]
    _geo_run(n, kind, lengths, order, 6500 + n)
    _geo_run(n, kind, lengths, order, 6500 + n, route="serial")


@gpu
@pytest.mark.parametrize("n,kind", GEO_CASES)
def test_results_do_not_depend_on_the_segment_length(n, kind):
    """The same batch in segments of 100, 200, 600 and on the serial route: each run within the bounds of the oracle,
    the runs within twice those bounds of each other."""
    lengths = (1500, 1, 700, 2, 333, 3, 5)
    model = _geo_model(n, kind)
    obs = _observations(kind, np.random.default_rng(6600 + n), lengths, n, GEO_M)
    ref = _oracle(kind, obs, model, n, GEO_M)
    want = _want(ref)
    runs = {}
    for L in (100, 200, 600):
        runs[L], _ = _run(kind, obs, model, n, GEO_M, "lazy", "n=%d %s L=%d" % (n, kind, L), L=L, ref=ref)
    runs[0], _ = _run(kind, obs, model, n, GEO_M, "serial", "n=%d %s" % (n, kind), ref=ref)
    keys = sorted(runs)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            fr = {}
            for key, w in want.items():
                rtol, atol = BOUNDS[key]
                fr[key] = _frac(runs[a][key], runs[b][key], 0.0, 2.0 * (atol + rtol * np.abs(w)))
            print("n=%d %s L=%d against L=%d: " % (n, kind, a, b)
                  + ", ".join("%s %.3g" % kv for kv in fr.items()) + " of twice the bound")
            for key, v in fr.items():
                assert v <= 1.0, (a, b, key, v)


# ---- 3. the forward pass's own plan (64 lanes) -------------------------------------------------------------------
def _forward_plan(lengths, L):
    """segments of the forward pass's own plan: plan::plan_segments (csrc/plan.hpp) with mult 2 -- every piece of
    _plan cut in two at a multiple of four, which a trajectory of fewer than eight steps may not have"""
    n = 0
    for T in lengths:
        ns = 2 * -(-T // L)
        prev = 0
        for q in range(1, ns + 1):
            b = T if q == ns else ((q * T) // ns) & ~3
            if b > prev:
                n, prev = n + 1, b
    return n


SPLIT_LENGTHS = (6001, 2503, 4099, 1, 2)


@gpu
@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [40, 64])
def test_forward_pass_on_its_own_finer_segments(n, kind, split):
    """64 lanes per segment: the forward kernel runs on a plan with every segment cut in two (wide_split), so the
    backward pass meets a change of alpha's rescaling chain inside its segments (tmid) and must not reuse the gamma
    normaliser across it (SPARSE_SUM).  Every quantity, stored gamma included, against the oracle, with the split
    plan and without.

    wide_fwd_segments is twice wide_segments for the trajectories that can be cut: the planner gives the one- and
    the two-step trajectory of this batch one forward segment each (_forward_plan), so 2 * 17 - 2 = 32 here."""
    L, W, M = 1000, 32, 31
    model = _model(n, np.random.default_rng(6000 + n), kind, M)
    obs = _observations(kind, np.random.default_rng(6700 + 3 * n + KINDS.index(kind)), SPLIT_LENGTHS, n, M)
    _, opts = _run(kind, obs, model, n, M, "lazy", "n=%d %s wide_split=%d" % (n, kind, split), L=L, W=W, repeat=True,
                   options=(("wide_split", split),))
    if split:
        nlong = len(_plan(SPLIT_LENGTHS[:3], L))
        assert _forward_plan(SPLIT_LENGTHS[:3], L) == 2 * nlong and _forward_plan(SPLIT_LENGTHS, L) == 2 * nlong + 2
        assert opts["fwd"] == 2 * opts["nseg"] - 2 == _forward_plan(SPLIT_LENGTHS, L), opts
    else:
        assert opts["fwd"] == 0, opts


# ---- 4. model edges that must stay on the lazily scaled path ------------------------------------------------------
EDGE_N = (12, 24)


@gpu
@pytest.mark.parametrize("kind", ["gaussian", "discrete"])
@pytest.mark.parametrize("n", EDGE_N)
def test_zero_column_absorbing_state_and_one_hot_start(n, kind):
    """A state that is never entered (a zero column of A), an absorbing state the data rule out, and pi one-hot on
    state n - 1, the last lane with a state: the model of the test of this name in tests/test_tile_matrix_gpu.py."""
    rng = np.random.default_rng(7000 + n)
    M = 40
    A, pi, p0, p1 = _model(n, rng, kind, M)
    dead, sink = 7, 0
    if kind == "gaussian":
        p1[sink] = 0.3
    else:
        p0[sink, :] = 0.0
        p0[sink, 0] = 1.0
    A[:, dead] = 0.0
    A[sink, :] = 0.0
    A[sink, sink] = 1.0
    A /= A.sum(axis=1)[:, None]
    pi = np.zeros(n)
    pi[n - 1] = 1.0
    obs = _observations(kind, rng, MATRIX_LENGTHS, n, M)
    if kind == "gaussian":
        for k, o in enumerate(obs):
            o[0] = p0[n - 1] + 0.1 * k          # (the only start state must be able to emit the first observation)
    got, _ = _run(kind, obs, (A, pi, p0, p1), n, M, "lazy", "n=%d %s zero column, sink, one-hot pi" % (n, kind))
    assert np.all(got["C"][:, dead] == 0.0) and np.all(got["gamma"][:, dead] == 0.0)
    assert got["gamma0"][n - 1] == pytest.approx(len(MATRIX_LENGTHS), rel=1e-12)


@gpu
@pytest.mark.parametrize("M", [1, 2, 257])
@pytest.mark.parametrize("n", EDGE_N)
def test_discrete_alphabets_and_exact_zeros(n, M):
    """Alphabets of 1, 2 and 257 symbols; 30 % of B exactly zero, every symbol positive under some state and every
    state with a symbol it can emit.  M = 1: logL is exactly 0 and |logL_k| <= T_k (n + 2) 2^-53 stands in for the
    relative bound (tests/test_tile_matrix_gpu.py, module text)."""
    rng = np.random.default_rng(7100 + n + M)
    A, pi, B, _ = _model(n, rng, "discrete", M)
    if M > 1:
        zero = rng.random((n, M)) < 0.3
        zero[rng.integers(0, n, M), np.arange(M)] = False       # every symbol keeps a state
        zero[np.arange(n), rng.integers(0, M, n)] = False       # every state keeps a symbol
        B = np.where(zero, 0.0, B + 1e-3)
        B /= B.sum(axis=1)[:, None]
        # (keeping a symbol per state takes zeros back: at M = 2 most of them, 2 of 48 entries stay zero at n = 24)
        assert (0.25 if M > 2 else 0.04) < (B == 0.0).mean() <= 0.3
        assert np.all(B.max(axis=0) > 0.0) and np.all(B.max(axis=1) > 0.0)
    obs = _observations("discrete", rng, MATRIX_LENGTHS, n, M)
    atol = np.array([T * (n + 2) * 2.0 ** -53 for T in MATRIX_LENGTHS]) if M == 1 else 0.0
    _run("discrete", obs, (A, pi, B, None), n, M, "lazy", "n=%d discrete M=%d" % (n, M), logl_atol=atol)


@gpu
@pytest.mark.parametrize("n", EDGE_N)
def test_explicit_rows_with_sixty_decades_of_scale(n):
    """Every explicit emission row times its own factor, log-uniform in 1e-30 .. 1e+30: four of them between two
    refreshes are at most 2^400 away from 1, inside the 2^-900 of the self-check -- wide_trouble stays 0 (asserted
    with the route)."""
    rng = np.random.default_rng(7300 + n)
    model = _model(n, rng, "explicit")
    obs = [o * 10.0 ** rng.uniform(-30.0, 30.0, (len(o), 1)) for o in _observations("explicit", rng, MATRIX_LENGTHS, n, 0)]
    _run("explicit", obs, model, n, 0, "lazy", "n=%d explicit rows x 1e-30..1e+30" % n)


# ---- 5. the comparison itself, on the CPU -------------------------------------------------------------------------
def _emission_rows(kind, o, p0, p1):
    if kind == "gaussian":
        z = (o[:, None] - p0[None, :]) / p1[None, :]
        p = np.exp(-0.5 * z * z) / (p1[None, :] * np.sqrt(2.0 * np.pi))
        p[np.all(p == 0.0, axis=1)] = 1.0
        return p
    if kind == "discrete":
        return np.ascontiguousarray(p0[:, o].T)
    return o


def _estep_reversed(kind, obs, model, n, M):
    """A plain float64 E-step with a normalisation on every step whose sums over the states run from state n - 1
    down to state 0 (the oracle's run upwards); what _collect returns."""
    A, pi, p0, p1 = model
    Af = np.ascontiguousarray(A[::-1, :])          # forward: sum over i, rows n - 1 .. 0 (add.reduce adds row by row)
    Ab = np.ascontiguousarray(A.T[::-1, :])        # backward: sum over j
    rsum = lambda v: float(np.add.reduce(np.ascontiguousarray(v[::-1])))
    out = dict(logL=np.zeros(len(obs)), C=np.zeros((n, n)), gamma0=np.zeros(n), counts=np.zeros(n), gamma=[])
    if kind == "gaussian":
        out.update(sum_gd=np.zeros(n), sum_gdd=np.zeros(n))
    elif kind == "discrete":
        out.update(symbols=np.zeros((n, M)))
    for k, o in enumerate(obs):
        p = _emission_rows(kind, o, p0, p1)
        T = len(o)
        alpha, beta = np.empty((T, n)), np.empty((T, n))
        ll = 0.0
        for t in range(T):
            a = pi * p[0] if t == 0 else np.add.reduce(alpha[t - 1, ::-1, None] * Af, axis=0) * p[t]
            c = rsum(a)
            alpha[t] = a / c
            ll += np.log(c)
        beta[T - 1] = 1.0 / n
        for t in range(T - 2, -1, -1):
            b = np.add.reduce((p[t + 1] * beta[t + 1])[::-1, None] * Ab, axis=0)
            beta[t] = b / rsum(b)
        g = alpha * beta
        g /= np.add.reduce(g[:, ::-1], axis=1)[:, None]
        if T > 1:
            x = p[1:] * beta[1:]                                   # xi_t[i, j] = alpha_t[i] A[i, j] x_{t+1}[j] / S_t
            S = np.add.reduce((alpha[:-1] * np.add.reduce(x[:, ::-1, None] * Ab[None, :, :], axis=1))[:, ::-1], axis=1)
            out["C"] += A * ((alpha[:-1] / S[:, None]).T @ x)
        out["logL"][k] = ll
        out["gamma0"] += g[0]
        out["counts"] += g.sum(axis=0)
        out["gamma"].append(g)
        if kind == "gaussian":
            d = o[:, None] - p0[None, :]
            out["sum_gd"] += (g * d).sum(axis=0)
            out["sum_gdd"] += (g * d * d).sum(axis=0)
        elif kind == "discrete":
            np.add.at(out["symbols"].T, o, g)
    out["gamma"] = np.concatenate(out["gamma"])
    return out


@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", MATRIX_N)
def test_the_bounds_are_not_rounding_limited(n, kind, far):
    """(no GPU) On the inputs of the instantiation matrix, with and without the stretch that leaves the lazy range, a
    float64 recursion that adds the states in the reverse order stays below A TENTH of every bound against the
    oracle: a kernel that exceeds a bound on these inputs is wrong, not unlucky with its rounding."""
    model, obs, ref = _matrix_input(n, kind, far)
    got = _estep_reversed(kind, obs, model, n, MATRIX_M)
    _compare(got, _want(ref), "reversed order n=%d %s%s" % (n, kind, ", far stretch" if far else ""), scale=0.1)
    assert np.abs(got["gamma"].sum(axis=1) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("kind", KINDS)
def test_the_comparison_notices_one_entry_off_by_twice_its_bound(kind):
    """(no GPU) _compare accepts the oracle's own result; with ONE entry of one quantity moved by twice its bound, or
    replaced by NaN, it fails -- for every quantity in turn, at the entry of largest and of smallest magnitude."""
    n, M = 9, 5
    rng = np.random.default_rng(8000 + KINDS.index(kind))
    model = _model(n, rng, kind, M)
    obs = _observations(kind, rng, (40, 1, 7), n, M)
    want = _want(_oracle(kind, obs, model, n, M))
    assert set(want) == {"logL", "C", "gamma0", "counts", "gamma"} | \
        {"gaussian": {"sum_gd", "sum_gdd"}, "discrete": {"symbols"}, "explicit": set()}[kind]
    same = {key: np.array(w, dtype=np.float64) for key, w in want.items()}
    assert max(_compare(same, want, "%s, the oracle itself" % kind).values()) == 0.0
    for key, w in want.items():
        rtol, atol = BOUNDS[key]
        w = np.asarray(w, dtype=np.float64)
        for where in (np.argmax(np.abs(w)), np.argmin(np.abs(w))):
            idx = np.unravel_index(where, w.shape)
            for sign in (1.0, -1.0):
                got = {k2: np.array(v, dtype=np.float64) for k2, v in want.items()}
                got[key][idx] += sign * 2.0 * (atol + rtol * abs(w[idx]))
                if got[key][idx] == w[idx]:
                    continue                    # (logL of a bound of zero: nothing to move)
                with pytest.raises(AssertionError, match=": %s at " % key):
                    _compare(got, want, "%s, %s off by twice its bound" % (kind, key))
            got = {k2: np.array(v, dtype=np.float64) for k2, v in want.items()}
            got[key][idx] = np.nan
            with pytest.raises(AssertionError, match=": %s at " % key):
                _compare(got, want, "%s, NaN in %s" % (kind, key))
