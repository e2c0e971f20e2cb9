"""No GPU: k_pair_tile (the matrix-core row kernel of the generic path of bhmm_posterior_transitions, DESIGN.md
section 21) is in the gfx950 code object in all its instantiations, the header documents its options, and the
restatement the kernel computes -- P = f A, r = gamma+ / P (0 where P = 0), U_q = f (A o W_q), out_q =
(U_q . r) / (P . r) -- agrees with the oracle's pair rows under the fp64 bound of tests/test_transitions_gpu.py."""
import os
import re

import numpy as np

from oracle import oracle as orc
from tests.test_pair_tile_gpu import ATOL64, RTOL64, _rand_model, _rand_obs, _weights, unentered_model
from tests.transitions_oracle_engine import jump_mask, oracle_rows, pobs_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bhmm_amd.h")


def test_every_instantiation_is_in_the_gfx950_code_object():
    """1 .. 8 column tiles x double / float = 16"""
    from bhmm_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    names = set(m.decode() for m in re.findall(rb"_ZN4bhmm11k_pair_tileILi\d[A-Za-z0-9_]*", blob))
    want = set("_ZN4bhmm11k_pair_tileILi%dE%sEEvPKdS2_S2_ii" % (nt, ot) for nt in range(1, 9) for ot in ("d", "f"))
    assert len(want) == 16
    missing = [w for w in want if not any(x.startswith(w) for x in names)]
    assert not missing, missing[:4]


def test_header_documents_the_options():
    raw = open(HEADER).read()
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*#define\s+BHMM_PAIR_F32", raw, re.S).group(1)
    assert re.search(r"\bpair_rows\b", comment) and re.search(r"\bpair_rows_kernel\b", comment)
    assert re.search(r"k_pair_tile", comment) and re.search(r"fixed\s+tree\s+order", comment)
    # what the comment said before stands
    assert re.search(r"i the OUTER and j the INNER loop, both in ASCENDING\s+order", comment)
    assert re.search(r"reciprocal", comment) and re.search(r"probability zero is out of contract", comment)


def restated_rows(kind, obs, model, weights=None):
    """the rows as k_pair_tile forms them, from filtered rows and posterior rows of the oracle: one matrix per
    column (the jump form: A with its diagonal zeroed), r = 0 where the prediction is 0"""
    A, pi, par0, par1 = model
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    if weights is None:
        Ms = [A * (1.0 - np.eye(n))]
    else:
        Ms = [A * weights[:, :, q] for q in range(weights.shape[2])]
    out = []
    for o in obs:
        pobs = pobs_of(kind, o, par0, par1)
        alpha = orc.forward(A, pobs, pi)[1]
        beta = orc.backward(A, pobs)
        f = alpha / alpha.sum(axis=1, keepdims=True)
        gam = alpha * beta
        gam /= gam.sum(axis=1, keepdims=True)
        P = f[:-1] @ A
        r = np.divide(gam[1:], P, out=np.zeros_like(P), where=P > 0)
        den = (P * r).sum(axis=1)
        out.append(np.stack([((f[:-1] @ M) * r).sum(axis=1) / den for M in Ms], axis=1))
    return out


def _within(refs, rows, W, label):
    scale = np.abs(W).sum(axis=(0, 1))
    worst = 0.0
    for (want, wabs), r in zip(refs, rows):
        assert r.shape == want.shape, label
        if want.size == 0:
            continue
        assert np.all(np.isfinite(r)) and np.all(np.isfinite(want)), label
        worst = max(worst, float((np.abs(r - want) / (scale * ATOL64 + RTOL64 * wabs)).max()))
    print("%s: worst error / bound %.3g" % (label, worst))
    assert worst <= 1.0, label


def test_restatement_agrees_with_the_oracle():
    n = 17
    lengths = [1, 2, 15, 16, 17, 33, 300]
    for label, make in (("random", lambda rng: _rand_model("gaussian", n, 0, rng)), ("unentered", unentered_model)):
        rng = np.random.default_rng(4)
        model = make(rng)
        obs = _rand_obs("gaussian", n, 0, lengths, rng)
        W = _weights(n, 3, rng)
        _within(oracle_rows("gaussian", obs, model), restated_rows("gaussian", obs, model), jump_mask(n),
                label + " jump")
        _within(oracle_rows("gaussian", obs, model, W), restated_rows("gaussian", obs, model, W), W, label + " Q=3")
    # the unentered model does exercise r = 0 where P = 0
    A, pi = unentered_model(np.random.default_rng(4))[:2]
    assert np.all(A[:, 5] == 0.0) and pi[5] == 0.0 and A[3, 3] == 1.0
