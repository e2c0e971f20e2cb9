"""The split E-step of the discrete kind on 2-byte observation records (k_pack_obs16, Obs16Cursor).

Every case of tests/estep_obs16_child.py (see there for the chunk plans and what a case asserts): state counts 8,
7, 3, 2; alphabets of 2, 64 and 1024 symbols -- the top row offset of 16 bits at 8 states --, one symbol more
(int32 copy), alphabets beyond the LDS (int32 copy, tables in global memory); trajectories of 1, 2, 9 and 4100 steps
in one set under three chunk plans (Lmax 24, 25, 26: every alignment of both main loops, three record groups);
host, device-resident and lagged observations and the automatic plan.  Each is checked against the CPU oracle (log-
likelihood 1e-11 relative, counts 1e-9), repeated (same bits) and compared bit for bit with a context that option
obs16 = 0 keeps on the int32 copy; option obs16_used says which copy the sweeps read.

The edge cases run once more in ONE child process with BHMM_AMD_POISON=1: the new buffer and its guards start out
as 0xFF bytes there, so a refill that is consumed, or a word of a block that the packer did not write, shows as a
wrong count.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import estep_obs16_child as child  # noqa: E402  (importing starts nothing)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plans_cover_the_alignments():
    """What the chunk plans claim (no GPU work)."""
    seen, lmax = set(), {}
    for chunk in child.CHUNKS:
        per = [child.chunk_lens(T, chunk) for T in child.LENGTHS]
        lens = [l for p in per for l in p]
        lmax[chunk] = max(lens)
        seen |= {(l % 8, i == 0) for p in per for i, l in enumerate(p)}
        assert len(lens) > 128                      # three record groups
    assert lmax[24] % 4 == 0 and lmax[25] % 2 == 1
    later = {r for r, first in seen if not first}
    assert later >= {0, 1, 2, 7}                    # (len - 1) % 8 of 7, 0, 1, 6
    assert {r for r, first in seen if first} >= {0, 1, 2}
    assert child.packs(8, 1024) and not child.packs(8, 1025) and child.packs(7, 1024)
    assert not child.packs(3, 2048) and not child.packs(2, 4096)     # (beyond the LDS: tables in global memory)
    assert 1023 * 8 * 8 == 65472                    # the top offset, above 2^15


@pytest.mark.gpu
@pytest.mark.parametrize("name", child.NAMES)
def test_case(name):
    fn, args = next((c[1], c[2]) for c in child.CASES if c[0] == name)
    fn(*args)


@pytest.fixture(scope="module")
def child_output(launcher):
    """(Started through the pre-GPU launcher of tests/conftest.py: this pytest process has initialised the GPU by
    now and must not start programs itself.)"""
    env = dict(os.environ, BHMM_AMD_POISON="1")
    return launcher.run([[sys.executable, os.path.join(ROOT, "tests", "estep_obs16_child.py")]], timeout=600, env=env)[0]


@pytest.mark.gpu
def test_child_ran_every_case(child_output):
    out = child_output["out"]
    assert child_output["rc"] == 0 and "all cases run" in out, out[-6000:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", child.EDGE_NAMES)
def test_poisoned_case(child_output, name):
    out = child_output["out"]
    lines = [l for l in out.splitlines() if l.startswith("CASE %s " % name)]
    assert lines, "case did not run: " + out[-3000:]
    assert lines[0] == "CASE %s ok" % name, lines[0] + "\n" + out[-6000:]
