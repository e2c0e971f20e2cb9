"""No GPU: the posterior-decoding entry points exist at every layer (header, exported symbol, ctypes table,
Engine, package, hidden, estimator) and the Python layers validate their arguments before any native call.

bhmm_posterior_decode's own refusal of path_u8 with more than 256 states sits behind bhmm_ctx_create, which
needs a device, and Engine.posterior_decode never asks for bytes there (it switches to int32), so that check
is covered on the GPU (tests/test_posterior_gpu.py::test_u8_needs_at_most_256_states)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bhmm_amd.h")


def test_header_declares_and_library_exports():
    from bhmm_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+bhmm_posterior_decode\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, "include/bhmm_amd.h does not declare bhmm_posterior_decode"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 8
    assert "bhmm_posterior_decode" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["bhmm_posterior_decode"][1]) == 8
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build)"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r"\bT bhmm_posterior_decode\b", out)
    assert hasattr(_lib.load(), "bhmm_posterior_decode")


def test_python_entry_points_exist():
    import bhmm_amd
    from bhmm_amd.engine import Engine
    from bhmm_amd.estimators.maximum_likelihood import MaximumLikelihoodEstimator
    assert callable(Engine.posterior_decode)
    assert callable(bhmm_amd.posterior_decode)
    assert callable(bhmm_amd.api.posterior_decode)
    assert callable(bhmm_amd.hidden.posterior_decode)
    assert "posterior_decode" in bhmm_amd.hidden.api.__all__
    assert callable(MaximumLikelihoodEstimator.posterior_decode)


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
        eng.posterior_decode(np.ones((n, n + 1)), pi, mu, sig)           # wrong A shape
    with pytest.raises(ValueError):
        eng.posterior_decode(A, np.ones(n + 1) / (n + 1), mu, sig)       # wrong pi shape
    with pytest.raises(ValueError):
        eng.posterior_decode(A, pi, mu, None)                            # gaussian without sigmas
    with pytest.raises(ValueError):
        eng.posterior_decode(A, pi, mu[:-1], sig[:-1])                   # wrong emission shape
    with pytest.raises(ValueError):
        eng.posterior_decode(A, pi, mu, sig, out=np.empty(15, dtype=np.int32))   # wrong dtype
    with pytest.raises(ValueError):
        eng.posterior_decode(A, pi, mu, sig, out=np.empty(14, dtype=np.uint8))   # wrong size
    with pytest.raises(ValueError):
        eng.posterior_decode(A, pi, mu, sig, out=np.empty(30, dtype=np.uint8)[::2])  # not contiguous
    # valid arguments reach the native layer (which this engine does not have)
    with pytest.raises(AssertionError):
        eng.posterior_decode(A, pi, mu, sig, out=np.empty(15, dtype=np.uint8))
    d = _bare_engine("discrete", n, 6, [7])
    A, pi, B, _ = _model(n, 6)
    with pytest.raises(ValueError):
        d.posterior_decode(A, pi, None)                                  # discrete without B
    with pytest.raises(ValueError):
        d.posterior_decode(A, pi, B[:, :5])
    # more than 256 states: int32 paths
    big = _bare_engine("gaussian", 300, 0, [3])
    A, pi, mu, sig = _model(300)
    with pytest.raises(ValueError):
        big.posterior_decode(A, pi, mu, sig, out=np.empty(3, dtype=np.uint8))
    unloaded = _bare_engine("gaussian", n, 0, [1])
    unloaded.kind = None
    with pytest.raises(ValueError):
        unloaded.posterior_decode(*_model(n))


def test_module_level_validation():
    import bhmm_amd
    with pytest.raises(TypeError):
        bhmm_amd.posterior_decode([np.zeros(5)], "not a model")
    hmm = bhmm_amd.gaussian_hmm(np.array([0.5, 0.5]), np.array([[0.9, 0.1], [0.1, 0.9]]),
                                np.array([-1.0, 1.0]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError):
        bhmm_amd.posterior_decode([], hmm)
    with pytest.raises(TypeError):
        bhmm_amd.posterior_decode([np.zeros(5)], hmm, no_such_option=1)
    A = np.array([[0.9, 0.1], [0.1, 0.9]])
    with pytest.raises(ValueError):
        bhmm_amd.hidden.posterior_decode(A, np.ones((5, 3)), np.array([0.5, 0.5]))   # pobs columns
    with pytest.raises(ValueError):
        bhmm_amd.hidden.posterior_decode(np.ones((2, 3)), np.ones((5, 2)), np.array([0.5, 0.5]))
    with pytest.raises(ValueError):
        bhmm_amd.hidden.posterior_decode(A, np.ones((0, 2)), np.array([0.5, 0.5]))
