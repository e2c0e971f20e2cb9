"""No GPU: bhmm_filter exists at every layer (header, exported symbol, ctypes table, code object, Engine, package,
hidden, estimator), the Python layers validate their arguments before any native call, and the estimator hands
out the filtered probabilities and increments of the last E-step's model."""
import os
import re
import subprocess

import numpy as np
import pytest

import bhmm_amd
from tests.filter_oracle_engine import FilterOracleEngine, oracle_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bhmm_amd.h")


def test_header_declares_and_library_exports():
    from bhmm_amd import _lib
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    m = re.search(r"\bint\s+bhmm_filter\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, "include/bhmm_amd.h does not declare bhmm_filter"
    assert len([a.strip() for a in m.group(1).split(",")]) == 10
    assert re.search(r"#define\s+BHMM_FILT_F32\s+1\b", text) and re.search(r"#define\s+BHMM_FILT_DEVICE\s+2\b", text)
    assert (_lib.FILT_F32, _lib.FILT_DEVICE) == (1, 2)
    assert len(_lib.SIGNATURES["bhmm_filter"][1]) == 10
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build)"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r"\bT bhmm_filter\b", out)
    assert hasattr(_lib.load(), "bhmm_filter")


def test_every_instantiation_is_in_the_gfx950_code_object():
    """1..8 states x gaussian / discrete x B^T in LDS / global x double / float x rows / projection x with /
    without logc"""
    from bhmm_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    names = set(m.decode() for m in re.findall(rb"_ZN4bhmm14k_filter_sweepILi\d[A-Za-z0-9_]*", blob))
    want = set()
    for n in range(1, 9):
        for kind in (0, 1):
            for lds in (0, 1):
                for ot in ("d", "f"):
                    for proj in (0, 1):
                        for lc in (0, 1):
                            want.add("_ZN4bhmm14k_filter_sweepILi%dELi%dELb%dE%sLb%dELb%dEEEvPKNS_5ModelIXT_EEEiNS_6ChunksEi"
                                     % (n, kind, lds, ot, proj, lc))
    assert len(want) == 256
    missing = [w for w in want if not any(x.startswith(w) for x in names)]
    assert not missing, missing[:4]
    for ot in ("d", "f"):
        for kind in (0, 1, 2):
            assert ("_ZN4bhmm15k_filter_serialILi%dE%sEE" % (kind, ot)).encode() in blob


def test_python_entry_points_exist():
    from bhmm_amd.engine import Engine
    from bhmm_amd.estimators.maximum_likelihood import MaximumLikelihoodEstimator
    assert callable(Engine.filter_states)
    assert callable(bhmm_amd.filter_states)
    assert callable(bhmm_amd.api.filter_states)
    assert callable(bhmm_amd.hidden.filter_states)
    assert "filter_states" in bhmm_amd.hidden.api.__all__
    assert callable(MaximumLikelihoodEstimator.filter_states)


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
        eng.filter_states(np.ones((n, n + 1)), pi, mu, sig)             # wrong A shape
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, None)                              # gaussian without sigmas
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, weights=np.ones((n + 1, 2)))  # bad weights shape: rows
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, weights=np.ones(n))           # bad weights shape: 1-d
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, weights=np.ones((n, 9)))      # Q > 8
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, weights=np.ones((n, 0)))      # Q < 1
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, weights=np.full((n, 2), np.nan))
    for bad in (np.float16, np.int32, np.complex128):
        with pytest.raises(ValueError):
            eng.filter_states(A, pi, mu, sig, dtype=bad)                # neither float32 nor float64
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, probabilities=False, increments=False)    # neither output
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, probabilities=False, out=np.empty((15, n)))   # buffer for no output
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, out=np.empty((15, n), dtype=np.float32))      # dtype of out
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, out=np.empty((14, n)))                        # size of out
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, out=np.empty((15, 2 * n))[:, ::2])            # not contiguous
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, weights=np.ones((n, 3)), out=np.empty((15, n)))
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, out_increments=np.empty(14))                  # size of out_increments
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, out_increments=np.empty(15, dtype=np.float32))
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, out=0x1008, out_increments=0x2000)  # device address not 16-byte aligned
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, out=0x1000, out_increments=0x2008)
    with pytest.raises(ValueError):
        eng.filter_states(A, pi, mu, sig, out=0x1000, out_increments=np.empty(15))      # one here, one there
    # valid arguments reach the native layer (which this engine does not have)
    with pytest.raises(AssertionError):
        eng.filter_states(A, pi, mu, sig, weights=np.ones((n, 8)), dtype=np.float32)
    with pytest.raises(AssertionError):
        eng.filter_states(A, pi, mu, sig, out=np.empty((15, n)), out_increments=np.empty(15))
    with pytest.raises(AssertionError):
        eng.filter_states(A, pi, mu, sig, probabilities=False)
    d = _bare_engine("discrete", n, 6, [7])
    A, pi, B, _ = _model(n, 6)
    with pytest.raises(ValueError):
        d.filter_states(A, pi, B[:, :5])
    unloaded = _bare_engine("gaussian", n, 0, [1])
    unloaded.kind = None
    with pytest.raises(ValueError):
        unloaded.filter_states(*_model(n))


def test_module_level_validation():
    with pytest.raises(TypeError):
        bhmm_amd.filter_states([np.zeros(5)], "not a model")
    A = np.array([[0.9, 0.1], [0.1, 0.9]])
    hmm = bhmm_amd.gaussian_hmm(np.array([0.5, 0.5]), A, np.array([-1.0, 1.0]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError):
        bhmm_amd.filter_states([], hmm)
    with pytest.raises(TypeError):
        bhmm_amd.filter_states([np.zeros(5)], hmm, no_such_option=1)
    with pytest.raises(ValueError):
        bhmm_amd.filter_states([np.zeros(5)], hmm, weights=np.ones((3, 2)))
    with pytest.raises(ValueError):
        bhmm_amd.filter_states([np.zeros(5)], hmm, weights=np.ones((2, 9)))
    with pytest.raises(ValueError):
        bhmm_amd.filter_states([np.zeros(5)], hmm, dtype=np.int64)
    with pytest.raises(ValueError):
        bhmm_amd.filter_states([np.zeros(5)], hmm, probabilities=False, increments=False)
    pi = np.array([0.5, 0.5])
    with pytest.raises(ValueError):
        bhmm_amd.hidden.filter_states(A, np.ones((5, 3)), pi)           # pobs columns
    with pytest.raises(ValueError):
        bhmm_amd.hidden.filter_states(A, np.ones((0, 2)), pi)
    with pytest.raises(ValueError):
        bhmm_amd.hidden.filter_states(A, np.ones((5, 2)), pi, weights=np.ones((2, 9)))
    with pytest.raises(ValueError):
        bhmm_amd.hidden.filter_states(A, np.ones((5, 2)), pi, dtype=np.float16)
    with pytest.raises(ValueError):
        bhmm_amd.hidden.filter_states(A, np.ones((5, 2)), pi, probabilities=False, increments=False)


def _gauss_problem(seed=0, K=4, T=300):
    rng = np.random.default_rng(seed)
    A = np.array([[0.95, 0.05, 0.0], [0.03, 0.9, 0.07], [0.0, 0.1, 0.9]])
    mu, sig = np.array([-2.0, 0.5, 3.0]), np.array([0.6, 0.5, 0.9])
    obs = []
    for k in range(K):
        s = np.zeros(T + 37 * k, dtype=int)
        for t in range(1, len(s)):
            s[t] = rng.choice(3, p=A[s[t - 1]])
        obs.append(rng.normal(mu[s], sig[s]))
    init = bhmm_amd.gaussian_hmm([0.4, 0.3, 0.3], 0.8 * A + 0.2 / 3, mu + 0.4, sig * 1.3)
    return obs, init


def test_estimator_filters_under_the_model_of_the_last_estep():
    obs, init = _gauss_problem()
    made = []

    def factory(device):
        made.append(FilterOracleEngine(device))
        return made[-1]

    est = bhmm_amd.MaximumLikelihoodEstimator(obs, 3, initial_model=init, reversible=False, accuracy=1e-4,
                                              maxit=8, engine_factory=factory)
    with pytest.raises(RuntimeError):
        est.filter_states()                           # no E-step yet
    est.fit()
    eng = made[0]
    rows, logc = est.filter_states()
    A_used, pi_used, par0, par1 = eng.filter_calls[-1]
    assert not np.array_equal(A_used, est.hmm.transition_matrix)     # the last M-step moved the fitted model
    assert all(np.array_equal(a, b) for a, b in zip(est._estep_model, eng.filter_calls[-1]))
    assert len(rows) == len(logc) == len(obs)
    for k, o in enumerate(obs):
        a, l = oracle_filter("gaussian", o, A_used, pi_used, par0, par1)
        assert rows[k].shape == (len(o), 3) and rows[k].dtype == np.float64
        assert logc[k].shape == (len(o),) and logc[k].dtype == np.float64
        assert np.array_equal(rows[k], a) and np.array_equal(logc[k], l)
        assert np.allclose(rows[k].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    # the sum of the increments is the log-likelihood of the last E-step
    assert np.isclose(sum(l.sum() for l in logc), est.likelihoods[-1], rtol=1e-10)
    # projection, dtype and one output alone
    V = np.column_stack([[1.0, 0.0, 1.0], par0])
    p, none = est.filter_states(weights=V, dtype=np.float32, increments=False)
    assert none is None
    for k in range(len(obs)):
        assert p[k].shape == (len(obs[k]), 2) and p[k].dtype == np.float32
        assert np.allclose(p[k], rows[k] @ V, rtol=0, atol=1e-6 * np.abs(V).sum(axis=0).max())
    none, l32 = est.filter_states(dtype=np.float32, probabilities=False)
    assert none is None and all(x.dtype == np.float32 for x in l32)
    with pytest.raises(ValueError):
        est.filter_states(probabilities=False, increments=False)
