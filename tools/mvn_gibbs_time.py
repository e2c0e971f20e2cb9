#!/usr/bin/env python
"""The moments of a hidden path for multivariate gaussian emissions against the only route there was before them, and
one whole sweep of the sampler, on one GPU and in one process.

N = 8 states, 256 trajectories of 1e5 steps, D in {2, 8, 32}, full and diagonal covariances: the shapes of
tools/mvn_time.py.  The path is one draw of the sampler under the generating model.  Per shape, after one warm-up pass,
the median of `--reps` repetitions of:

  path_moments  k_mvn_path_moments + finish on the path as an int32 tensor on the device, HIP events inside the call
                (option mvn_path_moments_ms); its share of the byte bound -- 8 D + 4 bytes read per step at the HBM
                rate of DESIGN.md section 0 (8 TB/s) -- and of the fp64 vector peak (78.6 TFLOP/s: D additions and
                D (D + 1) / 2 or D FMAs per step);
  onehot        the route of the parent commit: a (total, N) fp64 one-hot tensor made from the same path with torch
                (HIP events around zeros + scatter_), then bhmm_mvn_moments on it (option mvn_moments_ms);
  sweep         one BayesianHMMSampler._update (emission rows, re-load, path draw, moments, parameter draws), a host
                clock around it (it ends synchronised).

One JSON object per shape, printed and appended to profiles/mvn/mvn_gibbs_time.json.  Options: --only D, --steps T,
--traj K, --states N, --reps R, --no-sweep, --label TEXT, --out FILE."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bhmm_amd  # noqa: E402
from bhmm_amd.engine import MvnEngine  # noqa: E402
from mvn_time import make_problem, event_ms, summary  # noqa: E402

HBM_BYTES_PER_S = 8e12
FP64_VECTOR_FLOPS = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", type=int, default=None, help="one D")
    ap.add_argument("--steps", type=int, default=100000)
    ap.add_argument("--traj", type=int, default=256)
    ap.add_argument("--states", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-sweep", action="store_true", help="leave the whole sweep out (it copies the data to the host)")
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvn", "mvn_gibbs_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mvn_gibbs_time.py measures on the GPU: none is visible")
    n, K, T = args.states, args.traj, args.steps
    for D in (2, 8, 32):
        if args.only and D != args.only:
            continue
        for ctype in ("full", "diag"):
            A, pi, mu, cov, X, off = make_problem(n, D, ctype, K, T, 7 * D)
            total = K * T
            eng = MvnEngine(0)
            eng.set_observations_device("mvgaussian", X.data_ptr(), off, n, dimension=D)
            paths, C, n0, drawn = eng.sample_paths_moments(A, pi, mu, cov, seed=11, want_paths=True)
            path = torch.from_numpy(np.concatenate(paths)).to("cuda:0")
            del paths
            new_ms, hot_ms, soft_ms = [], [], []
            for rep in range(args.reps + 1):
                hard = eng.path_moments(path, mu, ctype)
                res = [None]

                def one_hot():
                    g = torch.zeros((total, n), dtype=torch.float64, device="cuda:0")
                    g.scatter_(1, path.long()[:, None], 1.0)
                    res[0] = g

                h = event_ms(one_hot)
                soft = eng.moments(res[0], mu, ctype)
                if rep:                                     # (the first pass is the warm-up)
                    new_ms.append(eng.get_option("mvn_path_moments_ms"))
                    hot_ms.append(h)
                    soft_ms.append(eng.get_option("mvn_moments_ms"))
            res[0] = None
            eng.close()
            sweep_ms = []
            if not args.no_sweep:
                model = bhmm_amd.mvgaussian_hmm(pi, A, mu, cov, covariance_type=ctype)
                Xh = X.cpu().numpy()
                smp = bhmm_amd.BayesianHMMSampler([Xh[off[k]:off[k + 1]] for k in range(K)], n, initial_model=model,
                                                  output="mvgaussian")
                del Xh
                for rep in range(args.reps + 1):
                    t0 = time.perf_counter()
                    smp._update(seed=3 if rep == 0 else None)
                    if rep:
                        sweep_ms.append(1e3 * (time.perf_counter() - t0))
                smp._engine.close()
                del smp
            nfma = D * (D + 1) // 2 if ctype == "full" else D
            byte_bound = 1e3 * total * (8 * D + 4) / HBM_BYTES_PER_S
            flop_bound = 1e3 * total * (D + 2 * nfma) / FP64_VECTOR_FLOPS
            line = dict(build=args.label, states=n, D=D, covariance_type=ctype, trajectories=K, steps=total,
                        reps=args.reps)
            line.update(summary("path_moments", new_ms))
            line.update(summary("onehot_make", hot_ms))
            line.update(summary("onehot_moments", soft_ms))
            if sweep_ms:
                line.update(summary("sweep", sweep_ms))
            line["onehot_route_ms"] = line["onehot_make_ms"] + line["onehot_moments_ms"]
            line["speedup_over_onehot_route"] = line["onehot_route_ms"] / line["path_moments_ms"]
            line["byte_bound_ms"] = byte_bound
            line["share_of_byte_bound"] = byte_bound / line["path_moments_ms"]
            line["fp64_vector_bound_ms"] = flop_bound
            line["share_of_fp64_vector_peak"] = flop_bound / line["path_moments_ms"]
            # (a sanity flag, not a bound: rounding of `total` terms of order one, and the moments of the draw itself)
            line["routes_agree"] = bool(np.all(np.abs(hard - soft) <= 1e-12 * total + 1e-9 * np.abs(soft))
                                        and np.array_equal(hard, drawn))
            text = json.dumps(line)
            print(text, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
            del X, path
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
