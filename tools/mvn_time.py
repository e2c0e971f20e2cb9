#!/usr/bin/env python
"""Multivariate gaussian emissions against the route a user had before them, on one GPU and in one process
(DESIGN.md section 23).

N = 8 states, 256 trajectories of 1e5 steps, D in {2, 8, 32}, full and diagonal covariances.  Per shape, after one
warm-up pass, `--reps` repetitions of:

  rows      k_mvn_rows + k_mvn_shift, HIP events inside bhmm_mvn_emissions (option mvn_rows_ms), and their share of the
            byte bound: read 8 D, write 8 N + 8 per step, at the HBM rate of DESIGN.md section 0 (8 TB/s);
  reload    the explicit re-load that follows (option mvn_reload_ms: a host clock around work that ends in a
            synchronise);
  estep     the E-step on the loaded rows that leaves gamma on the device (posterior_marginals into a device tensor),
            HIP events on the engine's stream;
  moments   k_mvn_moments + finish (option mvn_moments_ms) and their share of the byte bound: read 8 D + 8 N per step;
  em_step   one whole MaximumLikelihoodEstimator.em_step, a host clock around it (it ends synchronised);
  torch     the route there was before: rows with torch (linalg.solve_triangular, exp) from the same observations on
            the device, handed over with set_observations_device('explicit', ...), the E-step, the moments with
            torch.einsum; HIP events around the torch parts, the same calls for the rest.

One JSON object per shape, printed and appended to profiles/mvn/mvn_time.json.  Options: --only D, --steps T, --traj K,
--reps R, --torch-reps R, --label TEXT, --out FILE."""
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
from bhmm_amd.engine import Engine, MvnEngine  # noqa: E402

HBM_BYTES_PER_S = 8e12


def make_problem(n, D, ctype, K, T, seed):
    """model and observations drawn on the device from a mixture of the model's components (timing data: the hidden
    path does not matter to any of the passes)"""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) * 0.1 + np.eye(n) * 2.0
    A /= A.sum(axis=1)[:, None]
    pi = np.ones(n) / n
    mu = rng.normal(size=(n, D)) * 3.0
    if ctype == "full":
        cov = np.empty((n, D, D))
        for i in range(n):
            B = rng.normal(size=(D, D)) / math.sqrt(D)
            cov[i] = B.dot(B.T) + 0.5 * np.eye(D)
        fac = np.linalg.cholesky(cov)
    else:
        cov = rng.uniform(0.5, 2.0, (n, D))
        fac = np.array([np.diag(np.sqrt(c)) for c in cov])
    total = K * T
    lab = torch.randint(0, n, (total,), generator=g, device="cuda:0")
    lab = (lab.view(-1, 64)[:, :1].expand(-1, 64)).reshape(-1) if total % 64 == 0 else lab   # dwell of 64 steps
    z = torch.randn((total, D), generator=g, device="cuda:0", dtype=torch.float64)
    X = torch.empty_like(z)
    for i in range(n):
        idx = lab == i
        X[idx] = torch.from_numpy(mu[i]).cuda() + z[idx] @ torch.from_numpy(fac[i]).cuda().T
    del z, lab
    off = np.arange(K + 1, dtype=np.int64) * T
    return A, pi, mu, cov, X.contiguous(), off


def torch_rows(X, mu, cov, ctype):
    """the emission rows a user forms today: log-densities, row maximum, exp -- and the shifts"""
    n, D = mu.shape
    mu_d, cov_d = torch.from_numpy(mu).cuda(), torch.from_numpy(cov).cuda()
    l = torch.empty((X.shape[0], n), dtype=torch.float64, device=X.device)
    for i in range(n):
        d = X - mu_d[i]
        if ctype == "full":
            L = torch.linalg.cholesky(cov_d[i])
            z = torch.linalg.solve_triangular(L, d.T, upper=False).T
            logdet = torch.log(torch.diagonal(L)).sum()
        else:
            sd = torch.sqrt(cov_d[i])
            z = d / sd
            logdet = torch.log(sd).sum()
        l[:, i] = -0.5 * (z * z).sum(dim=1) - logdet - 0.5 * D * math.log(2 * math.pi)
    m = l.max(dim=1).values
    return torch.exp(l - m[:, None]).contiguous(), m


def torch_moments(X, gam, mu, ctype):
    mu_d = torch.from_numpy(mu).cuda()
    out = []
    for i in range(mu.shape[0]):
        d = X - mu_d[i]
        w = gam[:, i]
        # (products with the long axis contracted: a column sum of a (total, D) tensor takes seconds)
        S1 = torch.einsum("t,ta->a", w, d)
        S2 = torch.einsum("ta,tb->ab", d * w[:, None], d) if ctype == "full" else torch.einsum("t,ta->a", w, d * d)
        out.append((w.sum(), S1, S2))
    return out


def event_ms(fn, stream=None):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s = stream or torch.cuda.current_stream()
    a.record(s)
    fn()
    b.record(s)
    b.synchronize()
    return a.elapsed_time(b)


def summary(prefix, ts):
    return {prefix + "_ms": float(np.median(ts)), prefix + "_ms_min": float(min(ts)), prefix + "_ms_max": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", type=int, default=None, help="one D")
    ap.add_argument("--steps", type=int, default=100000)
    ap.add_argument("--traj", type=int, default=256)
    ap.add_argument("--states", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=None,
                    help="repetitions of the torch route (default: --reps); its moments take 10 to 30 s per call")
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvn", "mvn_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mvn_time.py measures on the GPU: none is visible")
    n, K, T = args.states, args.traj, args.steps
    for D in (2, 8, 32):
        if args.only and D != args.only:
            continue
        for ctype in ("full", "diag"):
            A, pi, mu, cov, X, off = make_problem(n, D, ctype, K, T, 7 * D)
            total = K * T
            stream = torch.cuda.Stream()
            eng = MvnEngine(0, stream=stream.cuda_stream)
            eng.set_observations_device("mvgaussian", X.data_ptr(), off, n, dimension=D)
            gam = torch.empty((total, n), dtype=torch.float64, device="cuda:0")
            rows_ms, reload_ms, estep_ms, mom_ms = [], [], [], []
            for rep in range(args.reps + 1):
                eng.emissions(mu, cov, force=True)         # (the same parameters again: make the rows anyway)
                e = event_ms(lambda: eng.posterior_marginals(A, pi, mu, cov, out=gam.data_ptr()), stream)
                mom = eng.moments(gam, mu, ctype)
                if rep:                                     # (the first pass is the warm-up)
                    rows_ms.append(eng.get_option("mvn_rows_ms"))
                    reload_ms.append(eng.get_option("mvn_reload_ms"))
                    estep_ms.append(e)
                    mom_ms.append(eng.get_option("mvn_moments_ms"))
            shifts = eng.shifts.copy()
            eng.close()
            # one whole EM iteration through the estimator (its own engine and copy of the observations)
            model = bhmm_amd.mvgaussian_hmm(pi, A, mu, cov, covariance_type=ctype)
            Xh = X.cpu().numpy()
            est = bhmm_amd.MaximumLikelihoodEstimator([Xh[off[k]:off[k + 1]] for k in range(K)], n,
                                                      initial_model=model)
            del Xh
            em_ms = []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                est.em_step()
                if rep:
                    em_ms.append(1e3 * (time.perf_counter() - t0))
            est._engine.close()
            del est
            # the route there was before, on the same observations
            ex = Engine(0, stream=stream.cuda_stream)
            t_rows, t_load, t_estep, t_mom = [], [], [], []
            for rep in range((args.torch_reps or args.reps) + 1):
                res = [None]

                def make():
                    res[0] = torch_rows(X, mu, cov, ctype)

                a = event_ms(make)
                rows_t, m_t = res[0]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ex.set_observations_device("explicit", rows_t.data_ptr(), off, n)
                b = 1e3 * (time.perf_counter() - t0)
                c = event_ms(lambda: ex.posterior_marginals(A, pi, out=gam.data_ptr()), stream)
                stream.synchronize()
                d = event_ms(lambda: res.__setitem__(0, torch_moments(X, gam, mu, ctype)))
                if rep:
                    t_rows.append(a)
                    t_load.append(b)
                    t_estep.append(c)
                    t_mom.append(d)
            S0_t = np.array([float(r[0]) for r in res[0]])
            shifts_t = m_t.view(K, T).sum(dim=1).cpu().numpy()
            ex.close()
            rows_bound = 1e3 * total * (8 * D + 8 * n + 8) / HBM_BYTES_PER_S
            mom_bound = 1e3 * total * (8 * D + 8 * n) / HBM_BYTES_PER_S
            line = dict(build=args.label, states=n, D=D, covariance_type=ctype, trajectories=K, steps=total,
                        reps=args.reps)
            line.update(summary("rows", rows_ms))
            line.update(summary("reload", reload_ms))
            line.update(summary("estep", estep_ms))
            line.update(summary("moments", mom_ms))
            line.update(summary("em_step", em_ms))
            line.update(summary("torch_rows", t_rows))
            line.update(summary("torch_load", t_load))
            line.update(summary("torch_estep", t_estep))
            line.update(summary("torch_moments", t_mom))
            line["rows_bound_ms"] = rows_bound
            line["rows_share_of_byte_bound"] = rows_bound / line["rows_ms"]
            line["moments_bound_ms"] = mom_bound
            line["moments_share_of_byte_bound"] = mom_bound / line["moments_ms"]
            line["rows_speedup_over_torch"] = line["torch_rows_ms"] / line["rows_ms"]
            line["moments_speedup_over_torch"] = line["torch_moments_ms"] / line["moments_ms"]
            ms = 1 + D + (D * (D + 1) // 2 if ctype == "full" else D)
            line["routes_agree"] = bool(np.allclose(mom.reshape(n, ms)[:, 0], S0_t, rtol=1e-9)
                                        and np.allclose(shifts, shifts_t, rtol=1e-10))
            text = json.dumps(line)
            print(text, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
            del X, gam, rows_t, m_t, res
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
