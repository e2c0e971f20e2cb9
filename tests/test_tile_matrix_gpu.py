"""GPU parity of the row-batched matrix-core E-step over EVERY instantiation and segment edge: csrc/tile_kernels.hpp
(33..64 states through wide_api.hip, 65..128 through tile_gen.hip) and csrc/big_kernels.hpp (129..512), against the
float64 CPU oracle (oracle/oracle.py), by the route and under the bounds of tests/test_tile_gpu.py (its _model,
_observations, _reference and _check are imported, not copied):

    logL rtol 1e-11; C and state counts rtol 1e-9 / atol 1e-11; gamma0 rtol 1e-9 / atol 1e-13; stored gamma rows
    rtol 1e-8 / atol 1e-13 (every trajectory, every step); sum_gd / sum_gdd rtol 1e-8 / atol 1e-9; symbol counts
    rtol 1e-9 / atol 1e-12; every gamma row sums to 1 within 1e-12.

tile_gen_estep and wide_estep hand an E-step to the order-faithful family on any self-check, failed boundary or
calibration outcome, and the result is then still right -- so every E-step checked here also asserts that the
matrix-core kernels produced it: tile == 1 (tile_reason in the message), careful == 0, wide_trouble == 0,
spec_fail == 0 and, where the case is meant to be segmented, wide_segments > number of trajectories.

What the dispatch tables say (and the cases follow):
  * 33..64 states (wide_api.hip, tile_launch_fwd / _bwd): always four column tiles, the last ones partly padded; the
    only second instantiation is n == 64 (no padded states).  33, 48, 49 and 64 are run all the same: the padding of
    the column tiles differs.  This family has NO unsegmented tile plan: one segment per trajectory runs the exact
    serial kernels (tile == 0), which the invariance test below asserts instead of hiding.
  * 65..128 states (tile_gen.hip, TILE_GEN_NT): 5, 6, 7, 8 column tiles for up to 80, 96, 112, 128 states.
  * 129..512 states (big_api.hip, BIG_TPW): 3, 4, 5, 6, 8 column tiles per wavefront for up to 192, 256, 320, 384, 512.

Segments are NOT cut at multiples of the segment length L: plan::plan_segments cuts a trajectory of T steps into
ceil(T / L) pieces of about equal length whose boundaries are multiples of four (_plan below restates the rule).  A
"last segment of two steps" therefore does not exist in this planner; the lengths the geometry tests use are the
ones around the grid (L - 1 .. 2 L + 1, W - 1 .. W + 1) plus 2 W - 8, 2 W and 2 W + 8, whose second segment starts
at W - 4 (starts from pi), W (the warm-up reaches the trajectory start exactly) and W + 4 (it just misses it).

M = 1: the likelihood is exactly 1, logL exactly 0, and a relative bound says nothing.  There every step's
normaliser is a sum of n rounded products of value 1, so |logL_k| <= T_k (n + 2) 2^-53 for kernel and oracle alike;
that bound stands in for rtol 1e-11 in this one case.

Every case prints its worst deviation as a fraction of its bound ("n=321 discrete: C 0.03 of bound")."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_tile_gpu import _check, _model, _observations, _reference

pytestmark = pytest.mark.gpu

KINDS = ("gaussian", "discrete", "explicit")
# (rtol, atol) of tests/test_tile_gpu.py
BOUNDS = dict(logL=(1e-11, 0.0), C=(1e-9, 1e-11), gamma0=(1e-9, 1e-13), counts=(1e-9, 1e-11), gamma=(1e-8, 1e-13),
              sum_gd=(1e-8, 1e-9), sum_gdd=(1e-8, 1e-9), symbols=(1e-9, 1e-12))


def _plan(lengths, L):
    """(trajectory, t0, len) of every segment: plan::plan_segments (csrc/plan.hpp) with mult 1"""
    segs = []
    for k, T in enumerate(lengths):
        ns = -(-T // L) if L > 0 else 1
        prev = 0
        for q in range(1, ns + 1):
            b = T if q == ns else ((q * T) // ns) & ~3
            if b > prev:
                segs.append((k, prev, b - prev))
                prev = b
    return segs


def _frac(got, want, rtol, atol):
    """largest |got - want| / (atol + rtol |want|): at most 1 is what assert_allclose accepts"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(err == 0.0, 0.0, err / (atol + rtol * np.abs(want)))
    return float(np.max(f))          # (a NaN anywhere gives NaN, which fails `<= 1`)


def _emission_reference(kind, obs, ref, p0, n, M):
    if kind == "gaussian":
        sd = sum((g * (o[:, None] - p0[None, :])).sum(axis=0) for o, g in zip(obs, ref["gammas"]))
        sdd = sum((g * (o[:, None] - p0[None, :]) ** 2).sum(axis=0) for o, g in zip(obs, ref["gammas"]))
        return dict(sum_gd=sd, sum_gdd=sdd)
    if kind == "discrete":
        cnt = np.zeros((n, M))
        for o, g in zip(obs, ref["gammas"]):
            orc.update_pout(o, g, cnt)
        return dict(symbols=cnt)
    return {}


def _oracle(kind, obs, model, n, M):
    A, pi, p0, p1 = model
    ref = _reference(kind, obs, A, pi, p0, p1)
    ref.update(_emission_reference(kind, obs, ref, p0, n, M))
    return ref


def _collect(eng, res, kind):
    """everything one E-step is compared by"""
    out = dict(logL=res.logL_k, C=res.C, gamma0=res.gamma0_sum, counts=res.state_counts,
               gamma=np.concatenate([eng.gamma(k) for k in range(len(eng.lengths))]))
    if kind == "gaussian":
        out.update(sum_gd=res.sum_gd, sum_gdd=res.sum_gdd)
    elif kind == "discrete":
        out.update(symbols=res.symbol_counts)
    return out


def _want(ref):
    w = dict(logL=ref["logL"], C=ref["C"], gamma0=ref["gamma0_sum"], counts=ref["state_counts"],
             gamma=np.concatenate(ref["gammas"]))
    for key in ("sum_gd", "sum_gdd", "symbols"):
        if key in ref:
            w[key] = ref[key]
    return w


def _assert_path(eng, ntraj, label, segmented=True):
    g = eng.get_option
    assert g("tile") == 1, "%s: not on the matrix-core kernels, tile_reason %d" % (label, g("tile_reason"))
    assert g("careful") == 0, label
    assert g("wide_trouble") == 0, "%s: wide_trouble %d" % (label, g("wide_trouble"))
    assert g("spec_fail") == 0, "%s: spec_fail %d" % (label, g("spec_fail"))
    if segmented:
        assert g("wide_segments") > ntraj, "%s: %d segments for %d trajectories" % (label, g("wide_segments"), ntraj)


def _compare(got, want, label, scale=1.0, logl_atol=0.0):
    """print the worst deviation of every quantity as a fraction of its bound (scale times the bounds), then assert"""
    fr = {}
    for key, w in want.items():
        rtol, atol = BOUNDS[key]
        if key == "logL":
            atol = logl_atol
        fr[key] = _frac(got[key], w, scale * rtol, scale * np.asarray(atol))
    print("%s: " % label + ", ".join("%s %.3g" % (k, v) for k, v in fr.items()) + " of bound")
    for key, v in fr.items():
        assert v <= 1.0, "%s: %s at %.3g of its bound" % (label, key, v)
    return fr


def _estep_checked(kind, obs, model, n, M, seglen, label, spec_W=None, ref=None, segmented=True, repeat=False,
                   logl_atol=0.0, nseg=None):
    """one engine, one E-step with stored gamma, the path assertions and every comparison; returns (what was
    compared, options read back)"""
    from bhmm_amd.engine import Engine
    A, pi, p0, p1 = model
    if ref is None:
        ref = _oracle(kind, obs, model, n, M)
    eng = Engine(0)
    try:
        eng.set_option("wide_segment_len", seglen)
        if spec_W is not None:
            eng.set_option("spec_W", spec_W)
        eng.set_observations(kind, obs, n, nsymbols=M if kind == "discrete" else 0)
        res = eng.estep(A, pi, p0, p1, store_gamma=True)
        _assert_path(eng, len(obs), label, segmented)
        opts = dict(L=int(eng.get_option("wide_segment_len")), W=int(eng.get_option("spec_W")),
                    nseg=int(eng.get_option("wide_segments")))
        if nseg is not None:
            assert opts["nseg"] == nseg, "%s: %d segments, meant %d" % (label, opts["nseg"], nseg)
        got = _collect(eng, res, kind)
        _compare(got, _want(ref), label, logl_atol=logl_atol)
        if np.all(np.asarray(logl_atol) == 0.0):
            _check(res, ref)                                       # (the same bounds, by the neighbour's own routine)
        rowsum = float(np.abs(got["gamma"].sum(axis=1) - 1.0).max())
        assert rowsum <= 1e-12, "%s: a gamma row sums to 1 +- %.3g" % (label, rowsum)
        if repeat:
            r2 = eng.estep(A, pi, p0, p1)       # statistics only: the same numbers, run to run
            _assert_path(eng, len(obs), label + " (second call)", segmented)
            np.testing.assert_allclose(r2.packed, res.packed, rtol=1e-12, atol=1e-12)
            r3 = eng.estep(A, pi, p0, p1)
            _assert_path(eng, len(obs), label + " (third call)", segmented)
            assert np.array_equal(r2.packed, r3.packed) and np.array_equal(r2.logL_k, r3.logL_k), label
    finally:
        eng.close()
    return got, opts


# ---- 1. the instantiation matrix ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128])
def test_every_instantiation_up_to_128_states(n, kind):
    """Both ends of every column-tile range, every emission kind, a ragged batch cut into segments of 200."""
    rng = np.random.default_rng(4000 + 3 * n + KINDS.index(kind))
    M = 40
    lengths = (1203, 1, 700, 2, 333, 3, 5)
    model = _model(n, rng, kind, M)
    obs = _observations(kind, rng, lengths, n, M)
    _estep_checked(kind, obs, model, n, M, 200, "n=%d %s" % (n, kind), spec_W=96 if n <= 64 else None, repeat=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [129, 192, 193, 256, 257, 320, 321, 384, 385, 512])
def test_every_instantiation_above_128_states(n, kind):
    """Both ends of every range of column tiles per wavefront (3, 4, 5, 6, 8), every emission kind, segments of 100."""
    rng = np.random.default_rng(5000 + 3 * n + KINDS.index(kind))
    M = 23
    lengths = (601, 1, 250, 2)
    model = _model(n, rng, kind, M)
    obs = _observations(kind, rng, lengths, n, M)
    _estep_checked(kind, obs, model, n, M, 100, "n=%d %s" % (n, kind), repeat=True)


# ---- 2. segment and tile geometry ---------------------------------------------------------------------------------
# one state count per kernel layout; the segment length L and the warm-up W are set, read back and asserted, so that
# the lengths built from them land where they are meant to (L / 2 < W <= L: see the module text)
GEO = {40: (160, 96), 100: (100, 64), 200: (100, 64)}
GEO_CASES = [(n, kind) for n in (40, 100, 200) for kind in ("gaussian", "discrete")]
GEO_M = 31
_geo_models = {}


def _geo_model(n, kind):
    """one model per (n, kind), shared by the geometry tests and left unchanged"""
    if (n, kind) not in _geo_models:
        m = _model(n, np.random.default_rng(6000 + n + KINDS.index(kind)), kind, GEO_M)
        for a in m:
            if a is not None:
                a.setflags(write=False)
        _geo_models[(n, kind)] = m
    return _geo_models[(n, kind)]


def _geo_run(n, kind, lengths, label, seed, nseg=None, seglen=None, segmented=True):
    L, W = GEO[n]
    rng = np.random.default_rng(seed)
    obs = _observations(kind, rng, lengths, n, GEO_M)
    if nseg is None and segmented:
        nseg = len(_plan(lengths, L))
    got, opts = _estep_checked(kind, obs, _geo_model(n, kind), n, GEO_M, L if seglen is None else seglen,
                               "n=%d %s %s" % (n, kind, label), spec_W=W, nseg=nseg, segmented=segmented)
    if segmented:
        assert (opts["L"], opts["W"]) == (L, W), opts     # the geometry in force is the one the lengths were built for
    return opts


@pytest.mark.parametrize("n,kind", GEO_CASES)
def test_lengths_around_the_group_of_four_and_the_prefetch_distance(n, kind):
    """Steps run in groups of four, observations are loaded 12 steps ahead and clamped at the row's last step:
    trajectories of 1 .. 17 steps next to one of 3 L + 1."""
    L, _ = GEO[n]
    lengths = (1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 3 * L + 1)
    _geo_run(n, kind, lengths, "1..17 and 3L+1", 6100 + n)


@pytest.mark.parametrize("n,kind", GEO_CASES)
def test_lengths_around_the_segment_grid(n, kind):
    L, W = GEO[n]
    lengths = (L - 1, L, L + 1, 2 * L, 2 * L + 1, L + 2, W - 1, W, W + 1, 2 * W - 8, 2 * W, 2 * W + 8)
    segs = _plan(lengths, L)
    second = {k: t0 for k, t0, _ in segs if t0 > 0 and k >= 9}
    # a second segment that starts from pi, one whose warm-up reaches the trajectory start exactly, one that just misses
    assert second == {9: W - 4, 10: W, 11: W + 4}, second
    assert [sum(1 for s in segs if s[0] == k) for k in range(6)] == [1, 1, 2, 2, 3, 2]
    _geo_run(n, kind, lengths, "grid", 6200 + n)


@pytest.mark.parametrize("nseg", [15, 16, 17, 18, 32, 33, 34])
@pytest.mark.parametrize("n,kind", GEO_CASES)
def test_tile_fill(n, kind, nseg):
    """One trajectory of exactly nseg segments: the tile of the segment that starts (ends) the trajectory has 15 empty
    rows, the others hold nseg - 1 = 14, 15, 16, 17, 31, 32, 33 rows -- a last tile with two, one and no empty row,
    exactly one and two full tiles, and full tiles followed by a tile of a single row."""
    L, _ = GEO[n]
    lengths = (nseg * L - 2,)
    assert len(_plan(lengths, L)) == nseg
    _geo_run(n, kind, lengths, "%d segments" % nseg, 6300 + n + nseg, nseg=nseg)


@pytest.mark.parametrize("order", ["long first", "long last"])
@pytest.mark.parametrize("n,kind", GEO_CASES)
def test_a_tile_whose_sixteen_rows_differ(n, kind, order):
    """3000 steps next to fifteen trajectories of 1 .. 15 steps.  Segmented, the sixteen segments that start a
    trajectory share one tile (L, 15, 14 .. 1 steps); above 64 states also unsegmented, where one tile runs rows of
    3000 and of 1 .. 15 steps (up to 64 states a plan of one segment per trajectory is not a matrix-core plan)."""
    lengths = (3000,) + tuple(range(1, 16))
    if order == "long last":
        lengths = lengths[::-1]
    _geo_run(n, kind, lengths, order, 6400 + n)
    if n > 64:
        _geo_run(n, kind, lengths, order + ", unsegmented", 6400 + n, seglen=3000, segmented=False)


@pytest.mark.parametrize("n,kind", GEO_CASES)
def test_results_do_not_depend_on_the_segment_length(n, kind):
    """The same batch in segments of 100, 200, 600 and unsegmented: each run within the bounds of the oracle, the runs
    within twice those bounds of each other."""
    from bhmm_amd.engine import Engine
    rng = np.random.default_rng(6500 + n)
    lengths = (1500, 1, 700, 2, 333, 3, 5)
    model = _geo_model(n, kind)
    obs = _observations(kind, rng, lengths, n, GEO_M)
    ref = _oracle(kind, obs, model, n, GEO_M)
    want = _want(ref)
    runs = {}
    for seglen in (100, 200, 600):
        label = "n=%d %s L=%d" % (n, kind, seglen)
        runs[seglen], opts = _estep_checked(kind, obs, model, n, GEO_M, seglen, label, ref=ref,
                                            spec_W=96 if n <= 64 else None, nseg=len(_plan(lengths, seglen)))
        assert opts["L"] == seglen
    label = "n=%d %s unsegmented" % (n, kind)
    if n > 64:
        runs[0], _ = _estep_checked(kind, obs, model, n, GEO_M, 1500, label, ref=ref, segmented=False)
    else:
        # 33..64 states: one segment per trajectory is the exact serial recursion of wide_kernels.hpp, not a
        # matrix-core plan -- said here, and the run serves as a second reference
        eng = Engine(0)
        eng.set_option("wide_segment_len", 1500)
        eng.set_observations(kind, obs, n, nsymbols=GEO_M if kind == "discrete" else 0)
        res = eng.estep(*model, store_gamma=True)
        assert eng.get_option("tile") == 0 and eng.get_option("wide_segments") == 0
        runs[0] = _collect(eng, res, kind)
        eng.close()
        _compare(runs[0], want, label + " (serial kernels)")
    keys = sorted(runs)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            fr = {}
            for key, w in want.items():
                rtol, atol = BOUNDS[key]
                d = np.abs(np.asarray(runs[a][key]) - np.asarray(runs[b][key]))
                fr[key] = float(np.max(d / (2.0 * (atol + rtol * np.abs(w)))))
            print("n=%d %s L=%d against L=%d: " % (n, kind, a, b)
                  + ", ".join("%s %.3g" % kv for kv in fr.items()) + " of twice the bound")
            for key, v in fr.items():
                assert v <= 1.0, (a, b, key, v)


# ---- 3. model edges that must stay on the matrix-core path ---------------------------------------------------------
def _edge_shape(n):
    """(lengths, segment length, alphabet) of the instantiation matrix for this state count"""
    return ((1203, 1, 700, 2, 333, 3, 5), 200) if n <= 128 else ((601, 1, 250, 2), 100)


@pytest.mark.parametrize("kind", ["gaussian", "discrete"])
@pytest.mark.parametrize("n", [100, 200])
def test_zero_column_absorbing_state_and_one_hot_start(n, kind):
    """A state that is never entered (a zero column of A), an absorbing state, and pi one-hot on state n - 1, which
    lies in the partly filled last column tile.

    The absorbing state is one the data rule out (gaussian: the narrow state at the low end of the means; discrete: it
    emits symbol 0 only).  k_wide_check compares the boundary vectors element by element, relative to the element, down
    to 1e-280 of the vector's sum -- and beta of an absorbing state is the product of its own densities to the end of
    the trajectory, which no warm-up reproduces.  With a sink the observations fit (first version of this test: the
    state in the middle of the means, a dense row of B) every backward boundary differs by O(1) in that one element,
    spec_fail counts, tile_reason becomes 5 and the order-faithful family computes the (correct) result: such a model
    is not one for which the segmented path holds, whatever the warm-up."""
    rng = np.random.default_rng(7000 + n)
    M = 40
    lengths, seglen = _edge_shape(n)
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
    obs = _observations(kind, rng, lengths, n, M)
    if kind == "gaussian":
        for k, o in enumerate(obs):
            o[0] = p0[n - 1] + 0.1 * k          # (the only start state must be able to emit the first observation)
    got, _ = _estep_checked(kind, obs, (A, pi, p0, p1), n, M, seglen, "n=%d %s zero column, sink, one-hot pi" % (n, kind))
    assert np.all(got["C"][:, dead] == 0.0) and np.all(got["gamma"][:, dead] == 0.0)
    assert got["gamma0"][n - 1] == pytest.approx(len(lengths), rel=1e-12)


@pytest.mark.parametrize("M", [1, 2, 17, 257, 1200])
@pytest.mark.parametrize("n", [100, 200])
def test_discrete_alphabets_and_exact_zeros(n, M):
    """Alphabets of 1 .. 1200 symbols; 30 % of B exactly zero, every symbol positive under some state and every state
    with a symbol it can emit."""
    rng = np.random.default_rng(7100 + n + M)
    lengths, seglen = _edge_shape(n)
    A, pi, B, _ = _model(n, rng, "discrete", M)
    if M > 1:
        zero = rng.random((n, M)) < 0.3
        zero[rng.integers(0, n, M), np.arange(M)] = False       # every symbol keeps a state
        zero[np.arange(n), rng.integers(0, M, n)] = False       # every state keeps a symbol
        B = np.where(zero, 0.0, B + 1e-3)
        B /= B.sum(axis=1)[:, None]
        # (keeping a symbol per state takes zeros back: half of them at M = 2)
        assert 0.1 < (B == 0.0).mean() <= 0.3 and np.all(B.max(axis=0) > 0.0) and np.all(B.max(axis=1) > 0.0)
    obs = _observations("discrete", rng, lengths, n, M)
    # M = 1: logL is exactly 0 -- the absolute rounding bound of the module text stands in for the relative one
    atol = np.array([T * (n + 2) * 2.0 ** -53 for T in lengths]) if M == 1 else 0.0
    _estep_checked("discrete", obs, (A, pi, B, None), n, M, seglen, "n=%d discrete M=%d" % (n, M), logl_atol=atol)


@pytest.mark.parametrize("n", [100, 200])
def test_gaussian_widths_from_narrow_to_wide(n):
    """Sigmas from 0.05 to 5 in one model (densities from 8 down to tiny), observations drawn from the model's own
    mixture so that no row underflows."""
    rng = np.random.default_rng(7200 + n)
    lengths, seglen = _edge_shape(n)
    A, pi, mu, _ = _model(n, rng, "gaussian")
    sig = np.exp(rng.uniform(np.log(0.05), np.log(5.0), n))
    sig[0], sig[n - 1] = 0.05, 5.0
    obs = []
    for T in lengths:
        s = rng.integers(0, n, T)
        obs.append(mu[s] + sig[s] * rng.standard_normal(T))
    _estep_checked("gaussian", obs, (A, pi, mu, sig), n, 0, seglen, "n=%d gaussian sigma 0.05..5" % n)


@pytest.mark.parametrize("n", [100, 200])
def test_explicit_rows_with_sixty_decades_of_scale(n):
    """Every explicit emission row times its own factor, log-uniform in 1e-30 .. 1e+30.  The recursion refreshes its
    exponent every fourth step and a row is out of range below 2^-900: four such factors are at most 2^400 away, so
    wide_trouble stays 0 (asserted with the path) and logL matches the oracle at rtol 1e-11."""
    rng = np.random.default_rng(7300 + n)
    lengths, seglen = _edge_shape(n)
    model = _model(n, rng, "explicit")
    obs = [o * 10.0 ** rng.uniform(-30.0, 30.0, (len(o), 1)) for o in _observations("explicit", rng, lengths, n, 0)]
    _estep_checked("explicit", obs, model, n, 0, seglen, "n=%d explicit rows x 1e-30..1e+30" % n)
