"""No GPU: the dwell-segment entry points exist at every layer (header, exported symbols, ctypes table, Engine,
package, estimator), PathRuns slices its arrays per trajectory, and the Python layers validate their arguments
before any native call.  What needs a context (a state outside [0, n) in the path, bhmm_runs_fetch before any
runs call, a misaligned device pointer) is covered on the GPU (tests/test_path_runs_gpu.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bhmm_amd.h")

SYMBOLS = {"bhmm_path_runs": 7, "bhmm_decode_runs": 9, "bhmm_runs_fetch": 4}


def test_header_declares_and_library_exports():
    from bhmm_amd import _lib
    raw = open(HEADER).read()
    assert re.search(r"#define\s+BHMM_DWELL_COLS\s+5\b", raw)
    assert _lib.DWELL_COLS == 5
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
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
    from bhmm_amd.engine import Engine, PathRuns
    from bhmm_amd.estimators.maximum_likelihood import MaximumLikelihoodEstimator
    assert callable(bhmm_amd.decode_segments)
    assert callable(bhmm_amd.api.decode_segments)
    assert callable(Engine.path_runs)
    assert callable(Engine.decode_runs)
    assert callable(Engine.runs_fetch)
    assert callable(MaximumLikelihoodEstimator.hidden_state_segments)
    assert bhmm_amd.PathRuns is PathRuns


def test_path_runs_object_slices_per_trajectory():
    from bhmm_amd.engine import PathRuns
    # three trajectories: 0 0 1 | (empty) | 2 2 2 0
    off = np.array([0, 2, 2, 4], dtype=np.int64)
    start = np.array([0, 2, 0, 3], dtype=np.int64)
    length = np.array([2, 1, 3, 1], dtype=np.int64)
    state = np.array([0, 1, 2, 0], dtype=np.int32)
    r = PathRuns(off, start, length, state)
    assert len(r) == 3 and r.count == 4
    assert r.dwell is None and r.jumps is None
    s, l, q = r.trajectory(0)
    assert s.tolist() == [0, 2] and l.tolist() == [2, 1] and q.tolist() == [0, 1]
    assert all(x.size == 0 for x in r.trajectory(1))
    s, l, q = r.trajectory(2)
    assert s.tolist() == [0, 3] and l.tolist() == [3, 1] and q.tolist() == [2, 0]
    assert [x.tolist() for x in r.trajectory(-1)] == [x.tolist() for x in r.trajectory(2)]
    # views, not copies
    assert s.base is start and l.base is length and q.base is state
    for k in (3, -4):
        with pytest.raises(IndexError):
            r.trajectory(k)
    dwell, jumps = np.zeros((3, 5), dtype=np.int64), np.zeros((3, 3), dtype=np.int64)
    r = PathRuns(off, start, length, state, dwell, jumps)
    assert r.dwell is dwell and r.jumps is jumps


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


def _model(n):
    return np.full((n, n), 1.0 / n), np.full(n, 1.0 / n), np.arange(n, dtype=float), np.ones(n)


class _FakeTensor(object):
    """What Engine.path_runs asks of a tensor."""

    def __init__(self, numel, ptr, itemsize=1, cuda=True, device=0, contiguous=True, floating=False):
        self._n, self._p, self._s, self.is_cuda, self._c, self._f = numel, ptr, itemsize, cuda, contiguous, floating
        self.device = type("D", (), {"index": device})()

    def numel(self):
        return self._n

    def data_ptr(self):
        return self._p

    def element_size(self):
        return self._s

    def is_contiguous(self):
        return self._c

    def is_floating_point(self):
        return self._f


def test_path_runs_validates_before_native_call():
    eng = _bare_engine("gaussian", 4, 0, [10, 0, 5])
    with pytest.raises(ValueError):
        eng.path_runs(np.zeros(14, dtype=np.uint8))                  # wrong size
    with pytest.raises(ValueError):
        eng.path_runs(np.zeros(16, dtype=np.uint8))
    with pytest.raises(ValueError):
        eng.path_runs(np.zeros(15, dtype=np.int64))                  # wrong dtype
    with pytest.raises(ValueError):
        eng.path_runs(np.zeros(15, dtype=np.float32))
    with pytest.raises(ValueError):
        eng.path_runs(np.zeros(30, dtype=np.uint8)[::2])             # not contiguous
    with pytest.raises(ValueError):
        eng.path_runs(np.zeros((3, 5), dtype=np.uint8))              # not flat
    with pytest.raises(ValueError):
        eng.path_runs([0] * 15)                                      # neither an array nor a tensor
    with pytest.raises(ValueError):
        eng.path_runs(_FakeTensor(15, 4096 + 8))                     # device pointer not aligned to 16 bytes
    with pytest.raises(ValueError):
        eng.path_runs(_FakeTensor(15, 4096, device=1))               # another GPU
    with pytest.raises(ValueError):
        eng.path_runs(_FakeTensor(14, 4096))                         # wrong size
    with pytest.raises(ValueError):
        eng.path_runs(_FakeTensor(15, 4096, itemsize=8))             # int64 tensor
    with pytest.raises(ValueError):
        eng.path_runs(_FakeTensor(15, 4096, itemsize=4, floating=True))
    with pytest.raises(ValueError):
        eng.path_runs(_FakeTensor(15, 4096, contiguous=False))
    # valid arguments reach the native layer (which this engine does not have)
    with pytest.raises(AssertionError):
        eng.path_runs(np.zeros(15, dtype=np.uint8))
    with pytest.raises(AssertionError):
        eng.path_runs(np.zeros(15, dtype=np.int32), stats=True)
    with pytest.raises(AssertionError):
        eng.path_runs(_FakeTensor(15, 4096))
    with pytest.raises(AssertionError):
        eng.path_runs(_FakeTensor(15, 4096 + 8, cuda=False))         # host memory is staged: any alignment
    big = _bare_engine("gaussian", 300, 0, [3])
    with pytest.raises(ValueError):
        big.path_runs(np.zeros(3, dtype=np.uint8))                   # bytes cannot hold 300 states
    with pytest.raises(AssertionError):
        big.path_runs(np.zeros(3, dtype=np.int32))
    unloaded = _bare_engine("gaussian", 4, 0, [1])
    unloaded.kind = None
    with pytest.raises(ValueError):
        unloaded.path_runs(np.zeros(1, dtype=np.uint8))


def test_decode_runs_validates_before_native_call():
    n = 4
    eng = _bare_engine("gaussian", n, 0, [10, 5])
    A, pi, mu, sig = _model(n)
    with pytest.raises(ValueError):
        eng.decode_runs(A, pi, mu, sig, method="gibbs")
    with pytest.raises(ValueError):
        eng.decode_runs(np.ones((n, n + 1)), pi, mu, sig)
    with pytest.raises(ValueError):
        eng.decode_runs(A, pi, mu, None)
    with pytest.raises(ValueError):
        eng.decode_runs(A, pi, mu[:-1], sig[:-1], method="posterior")
    for method in ("viterbi", "posterior"):
        with pytest.raises(AssertionError):
            eng.decode_runs(A, pi, mu, sig, method=method)
    big = _bare_engine("gaussian", 300, 0, [3])
    with pytest.raises(ValueError):
        big.decode_runs(*_model(300))                                # more than 256 states
    unloaded = _bare_engine("gaussian", n, 0, [1])
    unloaded.kind = None
    with pytest.raises(ValueError):
        unloaded.decode_runs(A, pi, mu, sig)


def test_module_level_validation():
    import bhmm_amd
    with pytest.raises(TypeError):
        bhmm_amd.decode_segments([np.zeros(5)], "not a model")
    hmm = bhmm_amd.gaussian_hmm(np.array([0.5, 0.5]), np.array([[0.9, 0.1], [0.1, 0.9]]),
                                np.array([-1.0, 1.0]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError):
        bhmm_amd.decode_segments([], hmm)
    with pytest.raises(ValueError):
        bhmm_amd.decode_segments([np.zeros(5)], hmm, method="gibbs")
    with pytest.raises(TypeError):
        bhmm_amd.decode_segments([np.zeros(5)], hmm, no_such_option=1)
