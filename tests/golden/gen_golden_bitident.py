#!/usr/bin/env python
"""Generate tests/golden/ref_bitident.npz: the reference's own compiled C kernels (oracle/_ref, built by
`make -C oracle ref` where the reference tree is present) on seeded random inputs, for
tests/test_oracle.py::test_bit_identical_to_compiled_reference.  Never imported by tests.

Per case (N states, T steps, seed): the inputs, and the reference's outputs -- p_obs, alpha and beta as
SHA-1 digests of their float64 bytes (the test asserts bit identity), log-likelihood, transition counts,
Viterbi path, sampled path (libc stream after srand(11)) and update_pout in full.

    python tests/golden/gen_golden_bitident.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle as orc  # noqa: E402  (ctypes access to oracle/_ref only)

CASES = [(2, 50, 1), (3, 1000, 2), (8, 5000, 3), (17, 300, 4)]


def sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    assert orc.ref_available(), "build oracle/_ref first (make -C oracle ref)"
    out = {}
    for N, T, seed in CASES:
        rng = np.random.default_rng(seed)
        A = rng.random((N, N))
        A /= A.sum(axis=1)[:, None]
        pi = rng.dirichlet(np.ones(N))
        mu = np.linspace(-3, 3, N)
        sig = rng.uniform(0.3, 1.5, N)
        obs = rng.normal(0, 3, T)
        o_int = rng.integers(0, 5, T).astype(np.int32)
        pobs = orc.ref_pobs_gaussian(obs, mu, sig)
        logL, alpha = orc.ref_forward(A, pobs, pi)
        beta = orc.ref_backward(A, pobs)
        p = "N%d_T%d_s%d_" % (N, T, seed)
        out.update({p + "A": A, p + "pi": pi, p + "mu": mu, p + "sigma": sig, p + "obs": obs, p + "o_int": o_int,
                    p + "pobs_sha1": sha1(pobs), p + "logL": logL, p + "alpha_sha1": sha1(alpha),
                    p + "beta_sha1": sha1(beta), p + "C": orc.ref_transition_counts(alpha, beta, A, pobs),
                    p + "viterbi": orc.ref_viterbi(A, pobs, pi),
                    p + "sample_path_seed11": orc.ref_sample_path(alpha, A, pobs, seed=11),
                    p + "pout": orc.ref_update_pout(o_int, orc.gamma(alpha, beta), np.zeros((N, 5)))})
    path = os.path.join(HERE, "ref_bitident.npz")
    np.savez_compressed(path, **out)
    print("%-28s %8.1f KB" % ("ref_bitident.npz", os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
