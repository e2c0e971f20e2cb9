#!/usr/bin/env python
"""Gaussian-mixture emissions per state against the only route there was before them -- MvnEngine on the expanded
N M-state model, A'[(i,c),(j,c')] = A_ij w_jc' -- on one GPU and in one process.

N = 8 states, 256 trajectories of 1e5 steps, M in {1, 2, 4} components, D in {2, 8}, full and diagonal covariances.
Per shape, after one warm-up pass, the medians of `--reps` repetitions of:

  rows       k_gmm_rows + k_mvn_shift without and with log responsibilities, HIP events inside bhmm_gmm_emissions
             (option mvn_rows_ms), and their share of the byte bound at the HBM rate of DESIGN.md section 0 (8 TB/s):
             read 8 D, write 8 N + 8 per step, plus 8 N M with responsibilities;
  reload     the explicit re-load that follows (option mvn_reload_ms, a host clock: it ends synchronised);
  estep      the E-step on the loaded rows that leaves gamma on the device, HIP events on the engine's stream;
  weights    k_gmm_weights (option gmm_weights_ms);
  moments    k_mvn_moments + finish over the N M columns (option mvn_moments_ms);
  em_step    one whole MaximumLikelihoodEstimator.em_step, a host clock around it;
  score      one whole GmmEngine.score call of a model whose rows are not loaded, a host clock around it;
  x_*        the expanded route: rows (k_mvn_rows, N M states), reload, E-step, moments and score of MvnEngine on the
             N M-state model.  At M = 1 this is the existing kind itself: x_rows is k_mvn_rows against k_gmm_rows.

One JSON object per shape, printed and appended to profiles/gmm/gmm_time.json.  Options: --only-d D, --only-m M,
--steps T, --traj K, --reps R, --label TEXT, --out FILE, --no-em."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bhmm_amd  # noqa: E402
from bhmm_amd.engine import GmmEngine, MvnEngine  # noqa: E402

HBM_BYTES_PER_S = 8e12


def make_problem(n, M, D, ctype, K, T, seed):
    """model and observations drawn on the device from the model's components (timing data: the hidden path does not
    matter to any of the passes)"""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) * 0.1 + np.eye(n) * 2.0
    A /= A.sum(axis=1)[:, None]
    pi = np.ones(n) / n
    w = rng.dirichlet(np.full(M, 4.0), n)
    mu = rng.normal(size=(n, M, D)) * 3.0
    if ctype == "full":
        cov = np.empty((n, M, D, D))
        for i in range(n):
            for c in range(M):
                B = rng.normal(size=(D, D)) / math.sqrt(D)
                cov[i, c] = B.dot(B.T) + 0.5 * np.eye(D)
        fac = np.linalg.cholesky(cov)
    else:
        cov = rng.uniform(0.5, 2.0, (n, M, D))
        fac = np.array([[np.diag(np.sqrt(c)) for c in cc] for cc in cov])
    total = K * T
    lab = torch.randint(0, n * M, (total,), generator=g, device="cuda:0")
    lab = (lab.view(-1, 64)[:, :1].expand(-1, 64)).reshape(-1) if total % 64 == 0 else lab   # dwell of 64 steps
    X = torch.randn((total, D), generator=g, device="cuda:0", dtype=torch.float64)
    muf, facf = mu.reshape(n * M, D), fac.reshape(n * M, D, D)
    for q in range(n * M):
        idx = lab == q
        X[idx] = torch.from_numpy(muf[q]).cuda() + X[idx] @ torch.from_numpy(facf[q]).cuda().T
    del lab
    off = np.arange(K + 1, dtype=np.int64) * T
    return A, pi, w, mu, cov, X.contiguous(), off


def event_ms(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def med(prefix, ts):
    return {prefix + "_ms": float(np.median(ts)), prefix + "_ms_min": float(min(ts)), prefix + "_ms_max": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only-d", type=int, default=None)
    ap.add_argument("--only-m", type=int, default=None)
    ap.add_argument("--steps", type=int, default=100000)
    ap.add_argument("--traj", type=int, default=256)
    ap.add_argument("--states", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-em", action="store_true", help="leave out the estimator's em_step (it copies the data)")
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmm", "gmm_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gmm_time.py measures on the GPU: none is visible")
    n, K, T = args.states, args.traj, args.steps
    total = K * T
    for D in (2, 8):
        if args.only_d and D != args.only_d:
            continue
        for M in (1, 2, 4):
            if args.only_m and M != args.only_m:
                continue
            for ctype in ("full", "diag"):
                A, pi, w, mu, cov, X, off = make_problem(n, M, D, ctype, K, T, 7 * D + M)
                p0 = np.concatenate([w[:, :, None], mu], axis=2)

                def other(rep):                             # a model whose rows are never the loaded ones
                    q = p0.copy()
                    q[:, :, 1:] += 1e-3 * (1 + rep % 2)
                    return q

                stream = torch.cuda.Stream()
                sobj = stream
                eng = GmmEngine(0, stream=stream.cuda_stream)
                eng.set_observations_device("gaussian_mixture", X.data_ptr(), off, n, dimension=D)
                gam = torch.empty((total, n), dtype=torch.float64, device="cuda:0")
                r0, r1, rl, es, wt, mo, sc = [], [], [], [], [], [], []
                for rep in range(args.reps + 1):
                    eng.emissions(p0, cov, force=True)
                    a = eng.get_option("mvn_rows_ms")
                    eng.emissions(p0, cov, force=True, want_resp=True)
                    b, c = eng.get_option("mvn_rows_ms"), eng.get_option("mvn_reload_ms")
                    e = event_ms(lambda: eng.posterior_marginals(A, pi, p0, cov, out=gam.data_ptr()), sobj)
                    mom = eng.moments(gam, None, ctype)
                    t0 = time.perf_counter()
                    ll = eng.score([(A, pi, other(rep), cov)])
                    s = 1e3 * (time.perf_counter() - t0)
                    if rep:                                 # (the first pass is the warm-up)
                        r0.append(a), r1.append(b), rl.append(c), es.append(e)
                        wt.append(eng.get_option("gmm_weights_ms")), mo.append(eng.get_option("mvn_moments_ms"))
                        sc.append(s)
                eng.close()
                em = []
                if not args.no_em:
                    model = bhmm_amd.gaussian_mixture_hmm(pi, A, w, mu, cov, covariance_type=ctype)
                    Xh = X.cpu().numpy()
                    est = bhmm_amd.MaximumLikelihoodEstimator([Xh[off[k]:off[k + 1]] for k in range(K)], n,
                                                              initial_model=model)
                    del Xh
                    for rep in range(args.reps + 1):
                        t0 = time.perf_counter()
                        est.em_step()
                        if rep:
                            em.append(1e3 * (time.perf_counter() - t0))
                    est._engine.close()
                    del est
                # the expanded route: N M states, one gaussian each
                nx = n * M
                Ax = np.repeat((A[:, :, None] * w[None, :, :]).reshape(n, nx), M, axis=0)
                pix = (pi[:, None] * w).reshape(nx)
                mux, covx = mu.reshape(nx, D), cov.reshape((nx,) + cov.shape[2:])
                mv = MvnEngine(0, stream=stream.cuda_stream)
                mv.set_observations_device("mvgaussian", X.data_ptr(), off, nx, dimension=D)
                gx = torch.empty((total, nx), dtype=torch.float64, device="cuda:0")
                xr, xl, xe, xm, xs = [], [], [], [], []
                for rep in range(args.reps + 1):
                    mv.emissions(mux, covx, force=True)
                    a, c = mv.get_option("mvn_rows_ms"), mv.get_option("mvn_reload_ms")
                    e = event_ms(lambda: mv.posterior_marginals(Ax, pix, mux, covx, out=gx.data_ptr()), sobj)
                    momx = mv.moments(gx, mux, ctype)
                    t0 = time.perf_counter()
                    llx = mv.score([(Ax, pix, mux + 1e-3 * (1 + rep % 2), covx)])
                    s = 1e3 * (time.perf_counter() - t0)
                    if rep:
                        xr.append(a), xl.append(c), xe.append(e), xm.append(mv.get_option("mvn_moments_ms")), xs.append(s)
                mv.close()
                line = dict(build=args.label, states=n, components=M, D=D, covariance_type=ctype, trajectories=K,
                            steps=total, reps=args.reps)
                for name, ts in (("rows", r0), ("rows_resp", r1), ("reload", rl), ("estep", es), ("weights", wt),
                                 ("moments", mo), ("score", sc), ("x_rows", xr), ("x_reload", xl), ("x_estep", xe),
                                 ("x_moments", xm), ("x_score", xs)) + ((("em_step", em),) if em else ()):
                    line.update(med(name, ts))
                line["rows_bound_ms"] = 1e3 * total * (8 * D + 8 * n + 8) / HBM_BYTES_PER_S
                line["rows_resp_bound_ms"] = 1e3 * total * (8 * D + 8 * n + 8 + 8 * n * M) / HBM_BYTES_PER_S
                line["rows_share_of_byte_bound"] = line["rows_bound_ms"] / line["rows_ms"]
                line["rows_resp_share_of_byte_bound"] = line["rows_resp_bound_ms"] / line["rows_resp_ms"]
                line["estep_route_ms"] = line["rows_resp_ms"] + line["reload_ms"] + line["estep_ms"] + \
                    line["weights_ms"] + line["moments_ms"]
                line["x_estep_route_ms"] = line["x_rows_ms"] + line["x_reload_ms"] + line["x_estep_ms"] + \
                    line["x_moments_ms"]
                line["estep_route_speedup_over_expanded"] = line["x_estep_route_ms"] / line["estep_route_ms"]
                line["score_speedup_over_expanded"] = line["x_score_ms"] / line["score_ms"]
                ms = 1 + D + (D * (D + 1) // 2 if ctype == "full" else D)
                line["routes_agree"] = bool(np.allclose(mom.reshape(nx, ms)[:, 0], momx.reshape(nx, ms)[:, 0], rtol=1e-8)
                                            and np.allclose(ll, llx, rtol=1e-10))
                text = json.dumps(line)
                print(text, flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(text + "\n")
                del X, gam, gx
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
