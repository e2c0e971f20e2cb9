"""GPU: the lazily scaled E-step where a trajectory ends just after the kernels last refreshed their power of two
(k_wide_fwd / k_wide_bwd<.., LAZY>, 9 to 64 states with tile = 0; k_tile_fwd / k_tile_logl / k_tile_bwd, 33 to 128
states).  The last k steps of a trajectory are all but impossible under every state, so
that alpha is carried towards, into and through the denormal range between two refreshes; everything an E-step
returns -- logL, C, gamma0, state counts, every stored gamma row, symbol counts or sum_gd / sum_gdd -- is held to an
E-step in 80-bit arithmetic under the BOUNDS of tests/test_tile_matrix_gpu.py (its _collect, _compare and BOUNDS
are imported), and every gamma row sums to 1 within 1e-12.  Inputs, reference and batches are those of
tests/estep_range_cases.py; test_estep_range_cpu.py shows that they reach the window and that the bounds can be met.

flags[2] is one word per E-step, so the trajectories are run in separate batches, each with a benign trajectory of
300 steps that the plan cuts (wide_segment_len = 100, spec_W = 64):
  unnoticed k, other   results only; wide_trouble, careful, spec_ok and spec_fail are printed -- a rescue inside a
                       kernel is as good as a repeat on the per-step-normalising kernels
  single step          (beside the case list) trajectories of one step at 2^-1000 to 2^-1060 and nothing else: the
                       backward pass takes no step on them, so none of its normalisers speaks for the forward pass;
                       results only
  in range             results, and that the lazily scaled kernels produced them (a guard that fired at 2^-890
                       would cost the route the benchmark runs on); a second E-step on the engine is bitwise equal"""
import numpy as np
import pytest

from tests import estep_range_cases as ec
from tests.test_tile_matrix_gpu import _collect, _compare

pytestmark = pytest.mark.gpu

CASES = [("wide",) + x for x in ec.WIDE_CASES + ec.WIDE_EXPLICIT] + [("tile",) + x for x in ec.TILE_CASES]
PARAMS = [pytest.param(*x, name, id="%s-%d-%s%d-%s" % (x + (name.replace(" ", ""),)))
          for x in CASES for name in ec.batch_names(x[0]) + ["single step"]]


@pytest.mark.parametrize("route,n,kind,M,name", PARAMS)
def test_estep_at_the_end_of_the_range(route, n, kind, M, name):
    from bhmm_amd.engine import Engine
    b = ec.single_step_batch(route, kind, n, M) if name == "single step" else ec.batch(route, kind, n, M, name)
    label = "%s n=%d %s M=%d %s (%d trajectories)" % (route, n, kind, M, name, len(b.obs))
    eng = Engine(0)
    try:
        if route == "wide" and n >= 33:
            eng.set_option("tile", 0)
        eng.set_option("wide_segment_len", ec.SEGLEN)
        eng.set_option("spec_W", ec.WARMUP)
        eng.set_observations(kind, b.obs, n, nsymbols=M if kind == "discrete" else 0)
        res = eng.estep(*b.model, store_gamma=True)
        g = eng.get_option
        opts = {o: int(g(o)) for o in ("tile", "wide_trouble", "careful", "spec_ok", "spec_fail", "wide_segments")}
        print(label + ": " + ", ".join("%s %d" % kv for kv in opts.items()))
        got = _collect(eng, res, kind)
        _compare(got, b.want, label)
        rowsum = float(np.abs(got["gamma"].sum(axis=1) - 1.0).max())
        assert rowsum <= 1e-12, "%s: a gamma row sums to 1 +- %.3g" % (label, rowsum)
        if name == "in range":
            assert opts["wide_trouble"] == 0 and opts["careful"] == 0, label
            assert opts["spec_ok"] >= 1 and opts["spec_fail"] == 0, label
            assert opts["tile"] == (1 if route == "tile" else 0), label
            assert opts["wide_segments"] > len(b.obs), label
            r2 = eng.estep(*b.model, store_gamma=True)
            got2 = _collect(eng, r2, kind)
            for key in got:
                assert np.array_equal(got[key], got2[key]), "%s: %s differs on the second call" % (label, key)
            assert np.array_equal(res.packed, r2.packed), label
            assert g("wide_trouble") == 0 and g("careful") == 0 and g("spec_fail") == 0, label
    finally:
        eng.close()
