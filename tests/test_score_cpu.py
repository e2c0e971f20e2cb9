"""CPU: argument checks of Engine.score / bhmm_amd.score, the stacked model layout of bhmm_score, and
the missing-GPU error (no silent fall-back)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gmodel(n, rng):
    A = rng.random((n, n)) + 0.1
    A /= A.sum(axis=1)[:, None]
    return (A, np.full(n, 1.0 / n), np.arange(n, dtype=float), np.ones(n))


def test_symbol_in_signature_table():
    from bhmm_amd import _lib
    assert "bhmm_score" in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "bhmm_amd.h")) as f:
        assert "int bhmm_score(bhmm_ctx *ctx, int nmodels" in f.read()


def test_stack_layout_gaussian():
    from bhmm_amd.engine import stack_models
    rng = np.random.default_rng(0)
    models = [_gmodel(3, rng) for _ in range(4)]
    A, pi, p0, p1 = stack_models("gaussian", 3, 0, models)
    assert A.shape == (4, 3, 3) and pi.shape == (4, 3) and p0.shape == (4, 3) and p1.shape == (4, 3)
    for a in (A, pi, p0, p1):
        assert a.dtype == np.float64 and a.flags.c_contiguous
    # the flat ABI layout: model s starts at s*N*N in A, s*N in pi / mu / sigma
    flatA = A.reshape(-1)
    for s, m in enumerate(models):
        assert np.array_equal(flatA[s * 9:(s + 1) * 9], m[0].reshape(-1))
        assert np.array_equal(pi.reshape(-1)[s * 3:(s + 1) * 3], m[1])
        assert np.array_equal(p0.reshape(-1)[s * 3:(s + 1) * 3], m[2])
        assert np.array_equal(p1.reshape(-1)[s * 3:(s + 1) * 3], m[3])


def test_stack_layout_discrete():
    from bhmm_amd.engine import stack_models
    rng = np.random.default_rng(1)
    n, M = 2, 5
    models = []
    for _ in range(3):
        A = rng.random((n, n))
        B = rng.random((n, M)).astype(np.float32)      # converted to double
        models.append((A / A.sum(axis=1)[:, None], np.array([0.5, 0.5]), B / B.sum(axis=1)[:, None], None))
    A, pi, p0, p1 = stack_models("discrete", n, M, models)
    assert p1 is None and p0.shape == (3, n, M) and p0.dtype == np.float64
    flat = p0.reshape(-1)
    for s, m in enumerate(models):   # B of model s at s*N*M, row-major
        assert np.array_equal(flat[s * n * M:(s + 1) * n * M], np.asarray(m[2], dtype=np.float64).reshape(-1))


def test_stack_validation():
    from bhmm_amd.engine import stack_models
    rng = np.random.default_rng(2)
    with pytest.raises(ValueError, match="at least one"):
        stack_models("gaussian", 3, 0, [])
    A, pi, mu, sg = _gmodel(3, rng)
    with pytest.raises(ValueError, match="model 1"):
        stack_models("gaussian", 3, 0, [(A, pi, mu, sg), (A[:2, :2], pi, mu, sg)])
    with pytest.raises(ValueError):
        stack_models("gaussian", 3, 0, [(A, pi, mu, None)])
    with pytest.raises(ValueError):
        stack_models("gaussian", 3, 0, [(A, pi, mu[:2], sg)])
    with pytest.raises(ValueError):
        stack_models("discrete", 3, 4, [(A, pi, np.ones((3, 5)) / 5, None)])
    with pytest.raises(ValueError):
        stack_models("gaussian", 3, 0, [(A, pi, mu)])


def test_api_validation():
    import bhmm_amd
    rng = np.random.default_rng(3)
    obs = [rng.normal(size=50)]
    g = bhmm_amd.gaussian_hmm(np.array([0.5, 0.5]), np.array([[0.9, 0.1], [0.2, 0.8]]),
                              np.array([0.0, 1.0]), np.array([1.0, 1.0]))
    d = bhmm_amd.discrete_hmm(np.array([0.5, 0.5]), np.array([[0.9, 0.1], [0.2, 0.8]]),
                              np.array([[0.5, 0.5], [0.1, 0.9]]))
    g3 = bhmm_amd.gaussian_hmm(np.full(3, 1 / 3), np.full((3, 3), 1 / 3), np.zeros(3), np.ones(3))
    with pytest.raises(ValueError, match="at least one"):
        bhmm_amd.score(obs, [])
    with pytest.raises(ValueError, match="output type"):
        bhmm_amd.score(obs, [g, d])
    with pytest.raises(ValueError, match="number of states"):
        bhmm_amd.score(obs, [g, g3])
    with pytest.raises(TypeError):
        bhmm_amd.score(obs, [(1, 2, 3, 4)])
    with pytest.raises(TypeError):
        bhmm_amd.score(obs, g, nonsense=1)


def test_no_gpu_raises():
    """With no device visible bhmm_amd.score raises BhmmAmdError instead of computing anything."""
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import bhmm_amd\n"
        "from bhmm_amd import _lib\n"
        "g = bhmm_amd.gaussian_hmm(np.array([0.5, 0.5]), np.array([[0.9, 0.1], [0.2, 0.8]]),\n"
        "                          np.array([0.0, 1.0]), np.array([1.0, 1.0]))\n"
        "try:\n"
        "    bhmm_amd.score([np.zeros(10)], g)\n"
        "except _lib.BhmmAmdError as e:\n"
        "    print('raised', e.code)\n"
        "    sys.exit(0)\n"
        "print('no error')\n"
        "sys.exit(1)\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "raised 7" in r.stdout


def test_null_context_is_an_error():
    """The C entry point refuses a missing context (no fall-back path that could run without one)."""
    import ctypes
    from bhmm_amd import _lib
    L = _lib.load()
    A = np.array([[1.0]])
    out = np.zeros(1)
    rc = L.bhmm_score(None, 1, _lib.dp(A), _lib.dp(np.ones(1)), _lib.dp(np.zeros(1)), _lib.dp(np.ones(1)),
                      _lib.dp(out))
    assert rc == _lib.ERR_INVALID
    assert b"no observations" in L.bhmm_last_error()
    assert ctypes.sizeof(ctypes.c_double) == 8
