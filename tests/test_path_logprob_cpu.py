"""No GPU: the path log-probability entry points exist at every layer (header, exported symbols, ctypes table, Engine,
package, estimator, hidden), and the Python layers validate their arguments before any native call.  What needs a
context (a state outside [0, n) in the path, a misaligned device pointer, the numbers) is covered on the GPU
(tests/test_path_logprob_gpu.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_path_runs_cpu import _FakeTensor, _bare_engine, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bhmm_amd.h")

SYMBOLS = {"bhmm_path_logprob": 10, "bhmm_decode_logprob": 7}


def test_header_declares_and_library_exports():
    from bhmm_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build)"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    L = _lib.load()
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
        assert m, "include/bhmm_amd.h does not declare %s" % name
        assert len(m.group(1).split(",")) == nargs
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert re.search(r"\bT %s\b" % name, out)
        assert hasattr(L, name)


def test_python_entry_points_exist():
    import bhmm_amd
    from bhmm_amd import hidden
    from bhmm_amd.engine import Engine
    from bhmm_amd.estimators.maximum_likelihood import MaximumLikelihoodEstimator
    assert callable(bhmm_amd.path_logprob)
    assert bhmm_amd.path_logprob is bhmm_amd.api.path_logprob
    assert callable(Engine.path_logprob)
    assert callable(Engine.decode_logprob)
    assert callable(MaximumLikelihoodEstimator.hidden_state_logprob)
    assert callable(hidden.path_logprob)
    assert hidden.path_logprob is hidden.api.path_logprob


def test_engine_path_logprob_validates_before_native_call():
    n = 4
    eng = _bare_engine("gaussian", n, 0, [10, 0, 5])
    models = [_model(n)]
    with pytest.raises(ValueError):
        eng.path_logprob(np.zeros(14, dtype=np.uint8), models)           # wrong total length
    with pytest.raises(ValueError):
        eng.path_logprob(np.zeros(16, dtype=np.int32), models)
    with pytest.raises(ValueError):
        eng.path_logprob(np.zeros(15, dtype=np.float64), models)         # a float path
    with pytest.raises(ValueError):
        eng.path_logprob(np.zeros(15, dtype=np.int64), models)           # neither uint8 nor int32
    with pytest.raises(ValueError):
        eng.path_logprob(np.zeros((3, 5), dtype=np.uint8), models)       # not flat
    with pytest.raises(ValueError):
        eng.path_logprob([np.zeros(10, dtype=np.uint8), np.zeros(5, dtype=np.uint8)], models)   # two paths, three trajectories
    with pytest.raises(ValueError):
        eng.path_logprob([np.zeros(10, dtype=np.uint8), np.zeros(0, dtype=np.uint8),
                          np.zeros(4, dtype=np.uint8)], models)          # a trajectory's path too short
    with pytest.raises(ValueError):
        eng.path_logprob([np.zeros(10), np.zeros(0), np.zeros(5)], models)   # float pieces
    with pytest.raises(ValueError):
        eng.path_logprob(_FakeTensor(15, 4096 + 8), models)              # device pointer not aligned to 16 bytes
    with pytest.raises(ValueError):
        eng.path_logprob(_FakeTensor(15, 4096, itemsize=4, floating=True), models)
    good = np.zeros(15, dtype=np.uint8)
    with pytest.raises(ValueError):
        eng.path_logprob(good, [])                                       # no model
    with pytest.raises(ValueError):
        eng.path_logprob(good, [_model(n), _model(n + 1)])               # differing state counts
    A, pi, mu, sig = _model(n)
    with pytest.raises(ValueError):
        eng.path_logprob(good, [(A, pi, mu, None)])                      # gaussian without sigmas
    with pytest.raises(ValueError):
        eng.path_logprob(good, [(A, pi, np.full((n, 3), 1.0 / 3), None)])  # a discrete model on gaussian data
    # valid arguments reach the native layer (which this engine does not have)
    with pytest.raises(AssertionError):
        eng.path_logprob(good, models)
    with pytest.raises(AssertionError):
        eng.path_logprob(np.zeros(15, dtype=np.int32), [_model(n)] * 3)
    with pytest.raises(AssertionError):
        eng.path_logprob([np.zeros(10, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(5, dtype=np.uint8)],
                         models)
    with pytest.raises(AssertionError):
        eng.path_logprob(_FakeTensor(15, 4096), models)
    big = _bare_engine("gaussian", 300, 0, [3])
    with pytest.raises(ValueError):
        big.path_logprob(np.zeros(3, dtype=np.uint8), [_model(300)])     # bytes cannot hold 300 states
    with pytest.raises(AssertionError):
        big.path_logprob(np.zeros(3, dtype=np.int32), [_model(300)])
    unloaded = _bare_engine("gaussian", n, 0, [1])
    unloaded.kind = None
    with pytest.raises(ValueError):
        unloaded.path_logprob(np.zeros(1, dtype=np.uint8), models)


def test_engine_decode_logprob_validates_before_native_call():
    n = 4
    eng = _bare_engine("gaussian", n, 0, [10, 5])
    A, pi, mu, sig = _model(n)
    with pytest.raises(ValueError):
        eng.decode_logprob(A, pi, mu, sig, method="gibbs")               # an unknown method
    with pytest.raises(ValueError):
        eng.decode_logprob(np.ones((n, n + 1)), pi, mu, sig)
    with pytest.raises(ValueError):
        eng.decode_logprob(A, pi, mu, None)
    for method in ("viterbi", "posterior"):
        with pytest.raises(AssertionError):
            eng.decode_logprob(A, pi, mu, sig, method=method)
    big = _bare_engine("gaussian", 300, 0, [3])
    with pytest.raises(ValueError):
        big.decode_logprob(*_model(300))                                 # more than 256 states


def test_module_level_validation():
    import bhmm_amd
    pi, P = np.array([0.5, 0.5]), np.array([[0.9, 0.1], [0.1, 0.9]])
    g2 = bhmm_amd.gaussian_hmm(pi, P, np.array([-1.0, 1.0]), np.array([1.0, 1.0]))
    g3 = bhmm_amd.gaussian_hmm(np.full(3, 1.0 / 3), np.full((3, 3), 1.0 / 3), np.array([-1.0, 0.0, 1.0]), np.ones(3))
    d2 = bhmm_amd.discrete_hmm(pi, P, np.array([[0.5, 0.5], [0.2, 0.8]]))
    obs = [np.zeros(5), np.zeros(3)]
    ok = [np.zeros(5, dtype=np.int32), np.zeros(3, dtype=np.int32)]
    with pytest.raises(TypeError):
        bhmm_amd.path_logprob(obs, "not a model", paths=ok)
    with pytest.raises(TypeError):
        bhmm_amd.path_logprob(obs, [g2, "not a model"], paths=ok)
    with pytest.raises(ValueError):
        bhmm_amd.path_logprob(obs, [], paths=ok)
    with pytest.raises(ValueError):
        bhmm_amd.path_logprob(obs, [g2, g3], paths=ok)                   # differing state counts
    with pytest.raises(ValueError):
        bhmm_amd.path_logprob(obs, [g2, d2], paths=ok)                   # differing output types
    with pytest.raises(ValueError):
        bhmm_amd.path_logprob(obs, [g2, g2])                             # paths=None decodes under ONE model
    with pytest.raises(ValueError):
        bhmm_amd.path_logprob(obs, g2, method="gibbs")                   # an unknown method
    with pytest.raises(ValueError):
        bhmm_amd.path_logprob(obs, g2, paths=ok, method="gibbs")
    with pytest.raises(ValueError):
        bhmm_amd.path_logprob([], g2, paths=[])
    with pytest.raises(ValueError):
        bhmm_amd.path_logprob(obs, g2, paths=np.zeros(7, dtype=np.int32))   # wrong total length
    with pytest.raises(ValueError):
        bhmm_amd.path_logprob(obs, g2, paths=[ok[0]])                    # one path, two trajectories
    with pytest.raises(ValueError):
        bhmm_amd.path_logprob(obs, g2, paths=[ok[0], np.zeros(4, dtype=np.int32)])
    with pytest.raises(ValueError):
        bhmm_amd.path_logprob(obs, g2, paths=np.full(8, 2, dtype=np.int64))  # a state outside [0, 2) in a flat path
    with pytest.raises(ValueError):
        bhmm_amd.path_logprob(obs, g2, paths=np.zeros(8))                # a float path
    with pytest.raises(ValueError):
        bhmm_amd.path_logprob(obs, g2, paths=[np.zeros(5), np.zeros(3)])
    with pytest.raises(TypeError):
        bhmm_amd.path_logprob(obs, g2, paths=ok, no_such_option=1)


def test_hidden_path_logprob_validates_before_native_call():
    from bhmm_amd import hidden
    A, pi = np.array([[0.9, 0.1], [0.1, 0.9]]), np.array([0.5, 0.5])
    pobs = np.full((4, 2), 0.5)
    with pytest.raises(ValueError):
        hidden.path_logprob(A, pobs, pi, np.zeros(3, dtype=np.int32))    # wrong length
    with pytest.raises(ValueError):
        hidden.path_logprob(A, pobs, pi, np.zeros(4))                    # a float path
    with pytest.raises(ValueError):
        hidden.path_logprob(A, pobs, pi, np.array([0, 1, 2, 0]))         # a state outside [0, N)
    with pytest.raises(ValueError):
        hidden.path_logprob(A, pobs[:, :1], pi, np.zeros(4, dtype=np.int32))
    with pytest.raises(ValueError):
        hidden.path_logprob(A, pobs[:0], pi, np.zeros(0, dtype=np.int32))
