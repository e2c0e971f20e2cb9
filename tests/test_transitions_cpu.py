"""No GPU: bhmm_posterior_transitions exists at every layer (header, exported symbol, code object, ctypes table,
Engine, package, hidden, estimator), the Python layers validate their arguments before any native call, and the
module functions and the estimator's method hand out what an engine returns -- checked on an oracle-backed engine
double, trajectories of one and two steps included."""
import os
import re
import subprocess

import numpy as np
import pytest

import bhmm_amd
from tests.transitions_oracle_engine import TransitionsOracleEngine, jump_mask, oracle_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bhmm_amd.h")


def test_header_declares_and_library_exports():
    from bhmm_amd import _lib
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    m = re.search(r"\bint\s+bhmm_posterior_transitions\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, "include/bhmm_amd.h does not declare bhmm_posterior_transitions"
    assert len([a.strip() for a in m.group(1).split(",")]) == 9
    assert re.search(r"#define\s+BHMM_PAIR_F32\s+1\b", text) and re.search(r"#define\s+BHMM_PAIR_DEVICE\s+2\b", text)
    assert (_lib.PAIR_F32, _lib.PAIR_DEVICE) == (1, 2)
    assert len(_lib.SIGNATURES["bhmm_posterior_transitions"][1]) == 9
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build)"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r"\bT bhmm_posterior_transitions\b", out)
    assert hasattr(_lib.load(), "bhmm_posterior_transitions")
    # the header says in which order the pairs are accumulated, and what becomes of a trajectory of probability zero
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*#define\s+BHMM_PAIR_F32", raw, re.S).group(1)
    assert re.search(r"i the OUTER and j the INNER loop, both in ASCENDING\s+order", comment)
    assert re.search(r"reciprocal", comment) and re.search(r"probability zero is out of contract", comment)


def test_every_instantiation_is_in_the_gfx950_code_object():
    """1..8 states x gaussian / discrete x B^T in LDS / global x double / float x jump / projected = 128"""
    from bhmm_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    names = set(m.decode() for m in re.findall(rb"_ZN4bhmm12k_pair_sweepILi\d[A-Za-z0-9_]*", blob))
    want = set()
    for n in range(1, 9):
        for kind in (0, 1):
            for lds in (0, 1):
                for ot in ("d", "f"):
                    for proj in (0, 1):
                        want.add("_ZN4bhmm12k_pair_sweepILi%dELi%dELb%dE%sLb%dEEEvPKNS_5ModelIXT_EEEiNS_6ChunksEii"
                                 % (n, kind, lds, ot, proj))
    assert len(want) == 128
    missing = [w for w in want if not any(x.startswith(w) for x in names)]
    assert not missing, missing[:4]


def test_python_entry_points_exist():
    from bhmm_amd.engine import Engine
    from bhmm_amd.estimators.maximum_likelihood import MaximumLikelihoodEstimator
    assert callable(Engine.posterior_transitions)
    assert callable(bhmm_amd.posterior_transitions)
    assert callable(bhmm_amd.api.posterior_transitions)
    assert callable(bhmm_amd.hidden.posterior_transitions)
    assert "posterior_transitions" in bhmm_amd.hidden.api.__all__
    assert callable(MaximumLikelihoodEstimator.posterior_transitions)


class _NoNative(object):
    """Stands where the loaded library would: any native call fails the test."""

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def _bare_engine(kind, n, M, lengths):
    from bhmm_amd.engine import Engine
    eng = Engine.__new__(Engine)        # no context: Engine() needs a device
    eng._L = _NoNative()
    eng._h = None
    eng._stage = None
    eng._keep = {}
    eng.device = 0
    eng._adopt(kind, n, M, np.asarray(lengths, dtype=np.int64))
    return eng


def _model(n, M=0):
    A = np.full((n, n), 1.0 / n)
    pi = np.full(n, 1.0 / n)
    if M:
        return A, pi, np.full((n, M), 1.0 / M), None
    return A, pi, np.arange(n, dtype=float), np.ones(n)


def test_engine_validates_before_native_call():
    n = 4
    eng = _bare_engine("gaussian", n, 0, [10, 5])
    A, pi, mu, sig = _model(n)
    with pytest.raises(ValueError):
        eng.posterior_transitions(np.ones((n, n + 1)), pi, mu, sig)                  # wrong A shape
    with pytest.raises(ValueError):
        eng.posterior_transitions(A, pi, mu, None)                                   # gaussian without sigmas
    with pytest.raises(ValueError):
        eng.posterior_transitions(A, pi, mu, sig, weights=np.ones((n, n)))           # wrong rank: 2-d
    with pytest.raises(ValueError):
        eng.posterior_transitions(A, pi, mu, sig, weights=np.ones((n, n, 2, 1)))     # wrong rank: 4-d
    with pytest.raises(ValueError):
        eng.posterior_transitions(A, pi, mu, sig, weights=np.ones((n + 1, n, 2)))    # wrong shape: rows
    with pytest.raises(ValueError):
        eng.posterior_transitions(A, pi, mu, sig, weights=np.ones((n, n - 1, 2)))    # wrong shape: columns
    with pytest.raises(ValueError):
        eng.posterior_transitions(A, pi, mu, sig, weights=np.ones((n, n, 9)))        # Q = 9
    with pytest.raises(ValueError):
        eng.posterior_transitions(A, pi, mu, sig, weights=np.ones((n, n, 0)))        # Q < 1
    W = np.ones((n, n, 2))
    W[1, 2, 0] = np.nan
    with pytest.raises(ValueError):
        eng.posterior_transitions(A, pi, mu, sig, weights=W)                         # a NaN in weights
    for bad in (np.float16, np.int32, np.complex128):
        with pytest.raises(ValueError):
            eng.posterior_transitions(A, pi, mu, sig, dtype=bad)                     # neither float32 nor float64
    with pytest.raises(ValueError):
        eng.posterior_transitions(A, pi, mu, sig, out=np.empty(15, dtype=np.float32))            # dtype of out
    with pytest.raises(ValueError):
        eng.posterior_transitions(A, pi, mu, sig, out=np.empty(14))                              # size of out
    with pytest.raises(ValueError):
        eng.posterior_transitions(A, pi, mu, sig, out=np.empty((15, 2))[:, 0])                   # not contiguous
    with pytest.raises(ValueError):
        eng.posterior_transitions(A, pi, mu, sig, weights=np.ones((n, n, 3)), out=np.empty(15))  # shape of out
    with pytest.raises(ValueError):
        eng.posterior_transitions(A, pi, mu, sig, out=0x1008)            # device address not 16-byte aligned
    # valid arguments reach the native layer (which this engine does not have)
    with pytest.raises(AssertionError):
        eng.posterior_transitions(A, pi, mu, sig, weights=np.ones((n, n, 8)), dtype=np.float32)
    with pytest.raises(AssertionError):
        eng.posterior_transitions(A, pi, mu, sig, out=np.empty(15))
    d = _bare_engine("discrete", n, 6, [7])
    A, pi, B, _ = _model(n, 6)
    with pytest.raises(ValueError):
        d.posterior_transitions(A, pi, B[:, :5])
    unloaded = _bare_engine("gaussian", n, 0, [1])
    unloaded.kind = None
    with pytest.raises(ValueError):
        unloaded.posterior_transitions(*_model(n))


def test_module_level_validation():
    with pytest.raises(TypeError):
        bhmm_amd.posterior_transitions([np.zeros(5)], "not a model")
    A = np.array([[0.9, 0.1], [0.1, 0.9]])
    hmm = bhmm_amd.gaussian_hmm(np.array([0.5, 0.5]), A, np.array([-1.0, 1.0]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError):
        bhmm_amd.posterior_transitions([], hmm)
    with pytest.raises(TypeError):
        bhmm_amd.posterior_transitions([np.zeros(5)], hmm, no_such_option=1)
    with pytest.raises(ValueError):
        bhmm_amd.posterior_transitions([np.zeros(5)], hmm, weights=np.ones((2, 2)))
    with pytest.raises(ValueError):
        bhmm_amd.posterior_transitions([np.zeros(5)], hmm, weights=np.ones((3, 2, 2)))
    with pytest.raises(ValueError):
        bhmm_amd.posterior_transitions([np.zeros(5)], hmm, weights=np.ones((2, 2, 9)))
    with pytest.raises(ValueError):
        bhmm_amd.posterior_transitions([np.zeros(5)], hmm, weights=np.full((2, 2, 1), np.inf))
    with pytest.raises(ValueError):
        bhmm_amd.posterior_transitions([np.zeros(5)], hmm, dtype=np.int64)
    pi = np.array([0.5, 0.5])
    with pytest.raises(ValueError):
        bhmm_amd.hidden.posterior_transitions(A, np.ones((5, 3)), pi)           # pobs columns
    with pytest.raises(ValueError):
        bhmm_amd.hidden.posterior_transitions(A, np.ones((0, 2)), pi)
    with pytest.raises(ValueError):
        bhmm_amd.hidden.posterior_transitions(A, np.ones((5, 2)), pi, weights=np.ones((2, 2, 9)))
    with pytest.raises(ValueError):
        bhmm_amd.hidden.posterior_transitions(A, np.ones((5, 2)), pi, weights=np.full((2, 2, 2), np.nan))
    with pytest.raises(ValueError):
        bhmm_amd.hidden.posterior_transitions(A, np.ones((5, 2)), pi, dtype=np.float16)


def _gauss_problem(seed=0, lengths=(300, 337, 1, 2)):
    rng = np.random.default_rng(seed)
    A = np.array([[0.95, 0.05, 0.0], [0.03, 0.9, 0.07], [0.0, 0.1, 0.9]])
    mu, sig = np.array([-2.0, 0.5, 3.0]), np.array([0.6, 0.5, 0.9])
    obs = []
    for T in lengths:
        s = np.zeros(T, dtype=int)
        for t in range(1, T):
            s[t] = rng.choice(3, p=A[s[t - 1]])
        obs.append(rng.normal(mu[s], sig[s]))
    return obs, (A, np.array([0.4, 0.3, 0.3]), mu, sig)


def _unit_pairs(n, pairs):
    W = np.zeros((n, n, len(pairs)))
    for q, (i, j) in enumerate(pairs):
        W[i, j, q] = 1.0
    return W


def test_module_functions_on_the_oracle_engine(monkeypatch):
    import bhmm_amd.engine
    made = []

    def factory(device=0):
        made.append(TransitionsOracleEngine(device))
        return made[-1]

    monkeypatch.setattr(bhmm_amd.engine, "Engine", factory)
    obs, (A, pi, mu, sig) = _gauss_problem()
    hmm = bhmm_amd.gaussian_hmm(pi, A, mu, sig)
    jump = bhmm_amd.posterior_transitions(obs, hmm)
    W = _unit_pairs(3, [(0, 1), (1, 0), (1, 2), (2, 1), (1, 1)])
    proj = bhmm_amd.posterior_transitions(obs, hmm, weights=W, dtype=np.float32)
    assert len(made) == 2 and len(jump) == len(proj) == len(obs)
    ref_j = oracle_rows("gaussian", obs, (A, pi, mu, sig))
    ref_p = oracle_rows("gaussian", obs, (A, pi, mu, sig), W)
    for k, o in enumerate(obs):
        assert jump[k].shape == (len(o) - 1,) and jump[k].dtype == np.float64
        assert proj[k].shape == (len(o) - 1, 5) and proj[k].dtype == np.float32
        assert np.array_equal(jump[k], ref_j[k][0][:, 0])
        assert np.array_equal(proj[k], ref_p[k][0].astype(np.float32))
        assert np.all((jump[k] >= 0) & (jump[k] <= 1 + 1e-12))
    assert jump[2].size == 0 and jump[3].size == 1           # one step: no pair; two steps: one pair
    # a jump is one of the off-diagonal pairs: with all six of them as columns the rows add up to the jump form
    every = _unit_pairs(3, [(i, j) for i in range(3) for j in range(3) if i != j])
    six = bhmm_amd.posterior_transitions(obs, hmm, weights=every)
    for k in range(len(obs)):
        assert np.allclose(six[k].sum(axis=1), jump[k], rtol=0, atol=1e-14)
        assert np.array_equal(bhmm_amd.posterior_transitions(obs, hmm, weights=jump_mask(3))[k][:, 0], jump[k])
    # lagged views: what the cut trajectories give (pieces shorter than two steps are left out by lag_observations)
    lagged = bhmm_amd.posterior_transitions(obs, hmm, lag=2)
    cut = bhmm_amd.lag_observations(obs, 2)
    ref_l = oracle_rows("gaussian", list(cut), (A, pi, mu, sig))
    assert len(lagged) == len(cut) == 4           # (both views of the trajectories of one and two steps are left out)
    assert all(np.array_equal(a, b[0][:, 0]) for a, b in zip(lagged, ref_l))
    # explicit pobs, one trajectory, lengths 1 and 2 included
    from oracle import oracle as orc
    for T in (1, 2, 50):
        pobs = orc.pobs_gaussian(obs[0][:T], mu, sig)
        r = bhmm_amd.hidden.posterior_transitions(A, pobs, pi)
        assert r.shape == (T - 1,) and r.dtype == np.float64
        p = bhmm_amd.hidden.posterior_transitions(A, pobs, pi, weights=W, dtype=np.float32)
        assert p.shape == (T - 1, 5) and p.dtype == np.float32
        want = oracle_rows("explicit", [pobs], (A, pi, None, None), W)[0][0]
        assert np.array_equal(p, want.astype(np.float32))
        assert np.array_equal(r, oracle_rows("explicit", [pobs], (A, pi, None, None))[0][0][:, 0])
        assert made[-1].kind == "explicit"


def test_estimator_hands_out_the_pairs_of_the_last_estep():
    obs, (A, pi, mu, sig) = _gauss_problem(lengths=(300, 337, 2, 411))
    init = bhmm_amd.gaussian_hmm([0.4, 0.3, 0.3], 0.8 * A + 0.2 / 3, mu + 0.4, sig * 1.3)
    made = []

    def factory(device):
        made.append(TransitionsOracleEngine(device))
        return made[-1]

    est = bhmm_amd.MaximumLikelihoodEstimator(obs, 3, initial_model=init, reversible=False, accuracy=1e-4,
                                              maxit=8, engine_factory=factory)
    with pytest.raises(RuntimeError):
        est.posterior_transitions()                   # no E-step yet
    est.fit()
    eng = made[0]
    jump = est.posterior_transitions()
    used = eng.transition_calls[-1]
    # the model of the LAST E-STEP, which is not the fitted one (the last M-step moved it)
    assert all(np.array_equal(a, b) for a, b in zip(used, est._estep_model))
    assert not np.array_equal(used[0], est.hmm.transition_matrix)
    ref = oracle_rows("gaussian", obs, used)
    assert len(jump) == len(obs)
    for k, o in enumerate(obs):
        assert jump[k].shape == (len(o) - 1,) and np.array_equal(jump[k], ref[k][0][:, 0])
    W = _unit_pairs(3, [(0, 1), (2, 1)])
    proj = est.posterior_transitions(weights=W, dtype=np.float32)
    refp = oracle_rows("gaussian", obs, used, W)
    for k, o in enumerate(obs):
        assert proj[k].shape == (len(o) - 1, 2) and proj[k].dtype == np.float32
        assert np.array_equal(proj[k], refp[k][0].astype(np.float32))
    # summed over time the unit-pair projections are the E-step's transition counts of that model
    from oracle import oracle as orc
    C = orc.estep("gaussian", obs, *used)["C"]
    got = sum(p.astype(np.float64).sum(axis=0) for p in proj)
    assert np.allclose(got, [C[0, 1], C[2, 1]], rtol=1e-5)
