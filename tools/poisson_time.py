#!/usr/bin/env python
"""Poisson count emissions against the route a user had before them and against the diagonal gaussian rows, on one GPU
and in one process.

N = 8 states, 256 trajectories of 1e5 steps, D in {2, 8}.  Per shape, after one warm-up pass, `--reps` repetitions of:

  rows       k_pois_rows + k_mvn_shift, HIP events inside bhmm_pois_emissions (option mvn_rows_ms), and their share of
             the byte bound: read 8 D, write 8 N + 8 per step, at the HBM rate of DESIGN.md section 0 (8 TB/s);
  reload     the explicit re-load that follows (option mvn_reload_ms);
  mvn_rows   k_mvn_rows + k_mvn_shift with diagonal covariances on the same buffer in the same run (means the rates,
             variances the rates floored at 0.1): the same bytes, about three times the arithmetic per channel;
  torch      the same rows made with torch on the device: X @ log(lambda)^T - Lambda, lgamma, max, exp; HIP events;
  em_step    one whole MaximumLikelihoodEstimator.em_step, a host clock around it (it ends synchronised).

One JSON object per shape, printed and appended to profiles/poisson/poisson_time.json.  Options: --only D, --steps T,
--traj K, --reps R, --label TEXT, --out FILE."""
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
from bhmm_amd.engine import MvnEngine, PoissonEngine  # noqa: E402

HBM_BYTES_PER_S = 8e12


def make_problem(n, D, K, T, seed):
    """model and counts drawn on the device (timing data: dwells of 64 steps in a random state)"""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) * 0.1 + np.eye(n) * 2.0
    A /= A.sum(axis=1)[:, None]
    pi = np.ones(n) / n
    rates = np.exp(rng.uniform(np.log(0.2), np.log(30.0), (n, D)))      # dark to bright photon bins
    total = K * T
    lab = torch.randint(0, n, (total,), generator=g, device="cuda:0")
    lab = (lab.view(-1, 64)[:, :1].expand(-1, 64)).reshape(-1) if total % 64 == 0 else lab
    X = torch.poisson(torch.from_numpy(rates).cuda()[lab], generator=g).to(torch.float64).contiguous()
    off = np.arange(K + 1, dtype=np.int64) * T
    torch.cuda.synchronize()    # (the engines copy X on a stream of their own, which does not wait for torch's)
    return A, pi, rates, X, off


def torch_rows(X, rates):
    """the emission rows a user forms today: log-densities without and with the count term, row maximum, exp"""
    r = torch.from_numpy(rates).cuda()
    l = X @ torch.log(r).T - r.sum(dim=1)[None, :]
    c = -torch.lgamma(X + 1.0).sum(dim=1)
    m = l.max(dim=1).values
    return torch.exp(l - m[:, None]).contiguous(), m + c


def host_shift(x, rates):
    """sum_t (m_t + c_t) of one trajectory on the host"""
    l = np.zeros((x.shape[0], rates.shape[0]))
    for d in range(x.shape[1]):
        l += x[:, d, None] * np.log(rates)[None, :, d]
    l -= rates.sum(axis=1)[None, :]
    c = -np.vectorize(math.lgamma, otypes=[np.float64])(x + 1.0).sum(axis=1)
    return math.fsum((l.max(axis=1) + c).tolist())


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
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poisson", "poisson_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("poisson_time.py measures on the GPU: none is visible")
    n, K, T = args.states, args.traj, args.steps
    for D in (2, 8):
        if args.only and D != args.only:
            continue
        A, pi, rates, X, off = make_problem(n, D, K, T, 7 * D)
        total = K * T
        stream = torch.cuda.Stream()
        eng = PoissonEngine(0, stream=stream.cuda_stream)
        eng.set_observations_device("poisson", X.data_ptr(), off, n, dimension=D)
        rows_ms, reload_ms = [], []
        for rep in range(args.reps + 1):
            eng.emissions(rates, force=True)                # (the same rates again: make the rows anyway)
            if rep:                                         # (the first pass is the warm-up)
                rows_ms.append(eng.get_option("mvn_rows_ms"))
                reload_ms.append(eng.get_option("mvn_reload_ms"))
        shifts = eng.shifts.copy()
        eng.close()
        mv = MvnEngine(0, stream=stream.cuda_stream)
        mv.set_observations_device("mvgaussian", X.data_ptr(), off, n, dimension=D)
        mvn_ms = []
        var = np.maximum(rates, 0.1)
        for rep in range(args.reps + 1):
            mv.emissions(rates, var, force=True)
            if rep:
                mvn_ms.append(mv.get_option("mvn_rows_ms"))
        mv.close()
        t_rows = []
        res = [None]
        for rep in range(args.reps + 1):
            a = event_ms(lambda: res.__setitem__(0, torch_rows(X, rates)))
            if rep:
                t_rows.append(a)
        shifts_t = res[0][1].view(K, T).sum(dim=1).cpu().numpy()
        host0 = host_shift(X[:T].cpu().numpy(), rates)
        res[0] = None
        torch.cuda.empty_cache()
        # one whole EM iteration through the estimator (its own engine and copy of the observations)
        model = bhmm_amd.poisson_hmm(pi, A, rates)
        Xh = X.cpu().numpy()
        est = bhmm_amd.MaximumLikelihoodEstimator([Xh[off[k]:off[k + 1]] for k in range(K)], n, initial_model=model)
        del Xh
        em_ms = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            est.em_step()
            if rep:
                em_ms.append(1e3 * (time.perf_counter() - t0))
        est._engine.close()
        del est
        rows_bound = 1e3 * total * (8 * D + 8 * n + 8) / HBM_BYTES_PER_S
        line = dict(build=args.label, states=n, D=D, trajectories=K, steps=total, reps=args.reps)
        line.update(summary("rows", rows_ms))
        line.update(summary("reload", reload_ms))
        line.update(summary("mvn_diag_rows", mvn_ms))
        line.update(summary("torch_rows", t_rows))
        line.update(summary("em_step", em_ms))
        line["rows_bound_ms"] = rows_bound
        line["rows_share_of_byte_bound"] = rows_bound / line["rows_ms"]
        line["rows_over_mvn_diag_rows"] = line["rows_ms"] / line["mvn_diag_rows_ms"]
        line["rows_speedup_over_torch"] = line["torch_rows_ms"] / line["rows_ms"]
        line["routes_agree"] = bool(np.allclose(shifts, shifts_t, rtol=1e-10))
        line["shift_max_rel_diff"] = float(np.max(np.abs(shifts - shifts_t) / np.abs(shifts)))
        # which route is off when they differ: trajectory 0 again on the host (float64 numpy, math.lgamma, math.fsum)
        line["shift0_rel_diff_kernel_host"] = float(abs(shifts[0] - host0) / abs(host0))
        line["shift0_rel_diff_torch_host"] = float(abs(shifts_t[0] - host0) / abs(host0))
        text = json.dumps(line)
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
        del X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
