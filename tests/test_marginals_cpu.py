"""No GPU: bhmm_posterior_marginals exists at every layer (header, exported symbol, ctypes table, Engine,
package, hidden, estimator), the Python layers validate their arguments before any native call, and the
estimator hands out gamma of the last E-step's model whether or not it was built with store_gamma."""
import os
import re
import subprocess

import numpy as np
import pytest

import bhmm_amd
from oracle import oracle as orc
from tests.marginals_oracle_engine import MarginalsOracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bhmm_amd.h")


def test_header_declares_and_library_exports():
    from bhmm_amd import _lib
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    m = re.search(r"\bint\s+bhmm_posterior_marginals\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, "include/bhmm_amd.h does not declare bhmm_posterior_marginals"
    assert len([a.strip() for a in m.group(1).split(",")]) == 9
    assert re.search(r"#define\s+BHMM_MARG_F32\s+1\b", text) and re.search(r"#define\s+BHMM_MARG_DEVICE\s+2\b", text)
    assert (_lib.MARG_F32, _lib.MARG_DEVICE) == (1, 2)
    assert len(_lib.SIGNATURES["bhmm_posterior_marginals"][1]) == 9
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build)"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r"\bT bhmm_posterior_marginals\b", out)
    assert hasattr(_lib.load(), "bhmm_posterior_marginals")
    # the header says in which order a projection is accumulated
    assert re.search(r"ASCENDING\s+order", raw)


def test_every_instantiation_is_in_the_gfx950_code_object():
    """1..8 states x gaussian / discrete (B^T in LDS / global) x double / float x row / projection"""
    from bhmm_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    names = set(m.decode() for m in re.findall(rb"_ZN4bhmm12k_marg_sweepILi\d[A-Za-z0-9_]*", blob))
    want = set()
    for n in range(1, 9):
        for kind in (0, 1):
            for lds in (0, 1):
                for ot in ("d", "f"):
                    for proj in (0, 1):
                        want.add("_ZN4bhmm12k_marg_sweepILi%dELi%dELb%dE%sLb%dEEEvPKNS_5ModelIXT_EEEiNS_6ChunksEii"
                                 % (n, kind, lds, ot, proj))
    missing = [w for w in want if not any(x.startswith(w) for x in names)]
    assert not missing, missing[:4]


def test_python_entry_points_exist():
    from bhmm_amd.engine import Engine
    from bhmm_amd.estimators.maximum_likelihood import MaximumLikelihoodEstimator
    assert callable(Engine.posterior_marginals)
    assert callable(bhmm_amd.posterior_marginals)
    assert callable(bhmm_amd.api.posterior_marginals)
    assert callable(bhmm_amd.hidden.posterior_marginals)
    assert "posterior_marginals" in bhmm_amd.hidden.api.__all__
    assert callable(MaximumLikelihoodEstimator.posterior_marginals)


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
        eng.posterior_marginals(np.ones((n, n + 1)), pi, mu, sig)             # wrong A shape
    with pytest.raises(ValueError):
        eng.posterior_marginals(A, pi, mu, None)                              # gaussian without sigmas
    with pytest.raises(ValueError):
        eng.posterior_marginals(A, pi, mu, sig, weights=np.ones((n + 1, 2)))  # bad weights shape: rows
    with pytest.raises(ValueError):
        eng.posterior_marginals(A, pi, mu, sig, weights=np.ones(n))           # bad weights shape: 1-d
    with pytest.raises(ValueError):
        eng.posterior_marginals(A, pi, mu, sig, weights=np.ones((n, 9)))      # Q > 8
    with pytest.raises(ValueError):
        eng.posterior_marginals(A, pi, mu, sig, weights=np.ones((n, 0)))      # Q < 1
    with pytest.raises(ValueError):
        eng.posterior_marginals(A, pi, mu, sig, weights=np.full((n, 2), np.nan))
    for bad in (np.float16, np.int32, np.complex128):
        with pytest.raises(ValueError):
            eng.posterior_marginals(A, pi, mu, sig, dtype=bad)                # neither float32 nor float64
    with pytest.raises(ValueError):
        eng.posterior_marginals(A, pi, mu, sig, out=np.empty((15, n), dtype=np.float32))      # dtype of out
    with pytest.raises(ValueError):
        eng.posterior_marginals(A, pi, mu, sig, out=np.empty((14, n)))                        # size of out
    with pytest.raises(ValueError):
        eng.posterior_marginals(A, pi, mu, sig, out=np.empty((15, 2 * n))[:, ::2])            # not contiguous
    with pytest.raises(ValueError):
        eng.posterior_marginals(A, pi, mu, sig, weights=np.ones((n, 3)), out=np.empty((15, n)))
    with pytest.raises(ValueError):
        eng.posterior_marginals(A, pi, mu, sig, out=0x1008)                   # device address not 16-byte aligned
    # valid arguments reach the native layer (which this engine does not have)
    with pytest.raises(AssertionError):
        eng.posterior_marginals(A, pi, mu, sig, weights=np.ones((n, 8)), dtype=np.float32)
    with pytest.raises(AssertionError):
        eng.posterior_marginals(A, pi, mu, sig, out=np.empty((15, n)))
    d = _bare_engine("discrete", n, 6, [7])
    A, pi, B, _ = _model(n, 6)
    with pytest.raises(ValueError):
        d.posterior_marginals(A, pi, B[:, :5])
    unloaded = _bare_engine("gaussian", n, 0, [1])
    unloaded.kind = None
    with pytest.raises(ValueError):
        unloaded.posterior_marginals(*_model(n))


def test_module_level_validation():
    with pytest.raises(TypeError):
        bhmm_amd.posterior_marginals([np.zeros(5)], "not a model")
    A = np.array([[0.9, 0.1], [0.1, 0.9]])
    hmm = bhmm_amd.gaussian_hmm(np.array([0.5, 0.5]), A, np.array([-1.0, 1.0]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError):
        bhmm_amd.posterior_marginals([], hmm)
    with pytest.raises(TypeError):
        bhmm_amd.posterior_marginals([np.zeros(5)], hmm, no_such_option=1)
    with pytest.raises(ValueError):
        bhmm_amd.posterior_marginals([np.zeros(5)], hmm, weights=np.ones((3, 2)))
    with pytest.raises(ValueError):
        bhmm_amd.posterior_marginals([np.zeros(5)], hmm, weights=np.ones((2, 9)))
    with pytest.raises(ValueError):
        bhmm_amd.posterior_marginals([np.zeros(5)], hmm, dtype=np.int64)
    pi = np.array([0.5, 0.5])
    with pytest.raises(ValueError):
        bhmm_amd.hidden.posterior_marginals(A, np.ones((5, 3)), pi)           # pobs columns
    with pytest.raises(ValueError):
        bhmm_amd.hidden.posterior_marginals(A, np.ones((0, 2)), pi)
    with pytest.raises(ValueError):
        bhmm_amd.hidden.posterior_marginals(A, np.ones((5, 2)), pi, weights=np.ones((2, 9)))
    with pytest.raises(ValueError):
        bhmm_amd.hidden.posterior_marginals(A, np.ones((5, 2)), pi, dtype=np.float16)


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


def test_estimator_without_store_gamma_hands_out_gamma_of_the_last_estep():
    obs, init = _gauss_problem()
    made = []

    def factory(device):
        made.append(MarginalsOracleEngine(device))
        return made[-1]

    est = bhmm_amd.MaximumLikelihoodEstimator(obs, 3, initial_model=init, reversible=False, accuracy=1e-4,
                                              maxit=8, engine_factory=factory)
    with pytest.raises(RuntimeError):
        est.posterior_marginals()                     # no E-step yet
    est.fit()
    eng = made[0]
    g = est.hidden_state_probabilities                # (raised RuntimeError before this call existed)
    assert len(g) == len(obs)
    # the oracle's gamma under the model of the LAST E-STEP: what the engine kept from it
    want = eng._gammas
    for k, o in enumerate(obs):
        assert g[k].shape == (len(o), 3) and g[k].dtype == np.float64
        assert np.allclose(g[k].sum(axis=1), 1.0, rtol=0, atol=1e-12)
        assert np.array_equal(g[k], want[k])
    # ... which is NOT the fitted model (the last M-step moved it)
    A_used = eng.marginal_calls[-1][0]
    assert not np.array_equal(A_used, est.hmm.transition_matrix)
    # the same list from an estimator that stores gamma
    est2 = bhmm_amd.MaximumLikelihoodEstimator(obs, 3, initial_model=init, reversible=False, accuracy=1e-4,
                                               maxit=8, store_gamma=True, engine_factory=factory)
    est2.fit()
    for a, b in zip(est2.hidden_state_probabilities, g):
        assert np.array_equal(a, b)
    assert made[1].marginal_calls == []               # store_gamma=True does what it did before
    # the explicit form: projection and dtype
    V = np.column_stack([[1.0, 0.0, 1.0], eng.marginal_calls[-1][2]])        # a set membership, the state means
    p = est.posterior_marginals(weights=V, dtype=np.float32)
    for k in range(len(obs)):
        assert p[k].shape == (len(obs[k]), 2) and p[k].dtype == np.float32
        assert np.allclose(p[k], want[k] @ V, rtol=0, atol=1e-6 * np.abs(V).sum(axis=0).max())
    par0, par1 = eng.marginal_calls[-1][2], eng.marginal_calls[-1][3]
    ref = orc.estep("gaussian", obs, A_used, eng.marginal_calls[-1][1], par0, par1, want_gamma=True)["gammas"]
    assert all(np.array_equal(a, b) for a, b in zip(ref, g))
