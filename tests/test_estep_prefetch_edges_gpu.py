"""The sweeps of the time-split E-step (up to 8 states) refill their prefetch registers unconditionally:
a chunk's last iteration of a main loop loads CI records before its first (backward) or behind its last
(forward) record, which nothing may consume and which must lie inside an allocation for every chunk -- the
first chunk of record group 0, the last chunk of the last group, a second record group, lagged views and
device-resident observations.

Every case runs against the CPU oracle with the tolerances of tests/test_estep_gpu.py (log-likelihood
1e-11 relative, counts 1e-9) in ONE child process with BHMM_AMD_POISON=1 (tests/estep_prefetch_edges_child.py;
the variable is read once per process): the guards, like every fresh allocation, are filled with 0xFF bytes,
so a consumed over-read shows as NaN or a wrong count.  The shapes are a few trajectories of a few hundred
steps at most; the chunk lengths make the backward main loop run exactly 0, 1 and 2 iterations (len - 1 of
3, 8, 9, 16, 17) and the forward one likewise (7 .. 9 and 15 .. 17 steps in groups).  Nothing reads outside
an allocation.

Carried boundaries: the second E-step of the carry cases must run on carried boundary vectors and every one
must split at a capture (asserted in the child: carry_W, carry_ok, carry_cap).  The next call of the same model
never uses carried vectors (they are only used after a model change), so it differs from the one that did by
the boundary tolerance by design; bit identity is asserted between the second and the third call of that model
(same warm-ups, same split at the capture).
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import estep_prefetch_edges_child as child  # noqa: E402  (names and chunk plans only: starts nothing)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def child_output(launcher):
    """(Started through the pre-GPU launcher of tests/conftest.py: this pytest process has initialised the
    GPU by now and must not start programs itself.)"""
    env = dict(os.environ, BHMM_AMD_POISON="1")
    r = launcher.run([[sys.executable, os.path.join(ROOT, "tests", "estep_prefetch_edges_child.py")]],
                     timeout=600, env=env)[0]
    return r


def test_chunk_plans_hold_the_loop_counts():
    """What the sets claim (no GPU work): iteration counts 0, 1, 2 of both main loops, the first chunk of
    the batch with exactly one backward iteration, the last chunk with Lmax steps."""
    chunk, lengths = child.SET_BWD
    lens = [l for T in lengths for l in child.chunk_lens(T, chunk)]
    assert {l - 1 for l in lens} >= {3, 8, 9, 16, 17} and 1 in lens
    assert lens[0] - 1 == 8 and lens[-1] == max(lens)
    chunk, lengths = child.SET_FWD_FIRST
    firsts = [child.chunk_lens(T, chunk) for T in lengths]
    assert all(len(f) == 1 for f in firsts)
    assert {f[0] - 4 for f in firsts} >= {7, 8, 9, 16, 17}      # discrete: groups start at step 4
    assert {f[0] - 2 for f in firsts} >= {7, 8, 9}              # Gaussian: at step 2
    inner = set()
    for chunk, lengths in (child.SET_FWD_INNER, child.SET_FWD_INNER2):
        per = [child.chunk_lens(T, chunk) for T in lengths]
        inner |= {l for p in per for l in p[1:]}
        assert per[-1][-1] == max(l for p in per for l in p)
    assert inner >= {7, 8, 9, 15, 16, 17}


def test_child_ran_every_case(child_output):
    out = child_output["out"]
    assert child_output["rc"] == 0 and "all cases run" in out, out[-6000:]


@pytest.mark.parametrize("name", child.NAMES)
def test_case(child_output, name):
    out = child_output["out"]
    lines = [l for l in out.splitlines() if l.startswith("CASE %s " % name)]
    assert lines, "case did not run: " + out[-3000:]
    assert lines[0] == "CASE %s ok" % name, lines[0] + "\n" + out[-6000:]
