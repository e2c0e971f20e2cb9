#!/usr/bin/env python
"""The component draw of the Gibbs sweep for gaussian-mixture emissions, the moments of its labels, one whole sweep, and
what the sweep avoids, on one GPU and in one process.

N = 8 states, 256 trajectories of 1e5 steps, D in {2, 8}, M in {1, 2, 4}, full and diagonal covariances: the shapes of
tools/gmm_time.py.  The path is one draw of the sampler under the generating model.  Per shape, after one warm-up pass,
the median of `--reps` repetitions of:

  draw          k_gmm_draw_components on the path as an int32 tensor on the device, HIP events inside the call (option
                gmm_draw_ms); its share of the byte bound -- 8 D + 4 bytes read and 4 written per step at the HBM rate
                of DESIGN.md section 0 (8 TB/s);
  moments       k_mvn_path_moments + finish over the N M labels (option mvn_path_moments_ms);
  rows          bhmm_gmm_emissions without and with want_resp (option mvn_rows_ms): the difference and the
                (total, N M) buffer are what the sweep avoids;
  torch         the route over the fetched responsibilities: gather the M columns of the state of every step,
                exponentiate, torch.multinomial (HIP events around the three);
  sweep         one BayesianGaussianMixtureHMMSampler._update (rows, re-load, path draw, component draw, moments,
                parameter draws), a host clock around it (it ends synchronised).

rounds: distinct states per wavefront (64 consecutive steps) of the path, mean and maximum -- the rounds of the draw
kernel's loop.  One JSON object per shape, printed and appended to profiles/gmm/gmm_gibbs_time.json.  Options: --only-d D,
--only-m M, --steps T, --traj K, --states N, --reps R, --no-torch, --no-sweep, --label TEXT, --out FILE."""
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
from bhmm_amd.engine import GmmEngine  # noqa: E402
from gmm_time import HBM_BYTES_PER_S, event_ms, make_problem, med  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only-d", type=int, default=None)
    ap.add_argument("--only-m", type=int, default=None)
    ap.add_argument("--steps", type=int, default=100000)
    ap.add_argument("--traj", type=int, default=256)
    ap.add_argument("--states", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="leave out the torch route (it fetches total N M doubles)")
    ap.add_argument("--no-sweep", action="store_true", help="leave the whole sweep out (it copies the data to the host)")
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmm", "gmm_gibbs_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gmm_gibbs_time.py measures on the GPU: none is visible")
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
                stream = torch.cuda.Stream()
                eng = GmmEngine(0, stream=stream.cuda_stream)
                eng.set_observations_device("gaussian_mixture", X.data_ptr(), off, n, dimension=D)
                paths, _, _, _ = eng.sample_paths(A, pi, p0, cov, seed=11, want_paths=True)
                flat = np.concatenate(paths)
                del paths
                waves = np.sort(flat[:total // 64 * 64].reshape(-1, 64), axis=1)
                rounds = 1 + (np.diff(waves, axis=1) != 0).sum(axis=1)
                del waves
                path = torch.from_numpy(flat).to("cuda:0")
                dr, mo, r0, r1, tq = [], [], [], [], []
                for rep in range(args.reps + 1):
                    eng.draw_components(path, seed=rep, want_labels=False)
                    if rep:                                 # (the first pass is the warm-up)
                        dr.append(eng.get_option("gmm_draw_ms")), mo.append(eng.get_option("mvn_path_moments_ms"))
                for rep in range(args.reps + 1):
                    eng.emissions(p0, cov, force=True)
                    a = eng.get_option("mvn_rows_ms")
                    eng.emissions(p0, cov, force=True, want_resp=True)
                    if rep:
                        r0.append(a), r1.append(eng.get_option("mvn_rows_ms"))
                if not args.no_torch:
                    resp = torch.from_numpy(eng.responsibilities()).to("cuda:0")       # (total, n, M) log r
                    idx = path.long()[:, None, None].expand(-1, 1, M)
                    res = [None]

                    def route():
                        res[0] = torch.multinomial(torch.exp(resp.gather(1, idx)[:, 0, :]), 1)

                    for rep in range(args.reps + 1):
                        t = event_ms(route, torch.cuda.current_stream())
                        if rep:
                            tq.append(t)
                    del resp, idx
                    res[0] = None
                eng.close()
                sweep_ms = []
                if not args.no_sweep:
                    model = bhmm_amd.gaussian_mixture_hmm(pi, A, w, mu, cov, covariance_type=ctype)
                    Xh = X.cpu().numpy()
                    smp = bhmm_amd.BayesianGaussianMixtureHMMSampler([Xh[off[k]:off[k + 1]] for k in range(K)], n,
                                                                     initial_model=model)
                    del Xh
                    for rep in range(args.reps + 1):
                        t0 = time.perf_counter()
                        smp._update(seed=3 if rep == 0 else None)
                        if rep:
                            sweep_ms.append(1e3 * (time.perf_counter() - t0))
                    smp._engine.close()
                    del smp
                byte_bound = 1e3 * total * (8 * D + 4 + 4) / HBM_BYTES_PER_S
                line = dict(build=args.label, states=n, M=M, D=D, covariance_type=ctype, trajectories=K, steps=total,
                            reps=args.reps, rounds_mean=float(rounds.mean()), rounds_max=int(rounds.max()))
                line.update(med("draw", dr))
                line.update(med("moments", mo))
                line.update(med("rows", r0))
                line.update(med("rows_resp", r1))
                line["resp_extra_ms"] = line["rows_resp_ms"] - line["rows_ms"]
                line["resp_buffer_bytes"] = 8 * total * n * M
                if tq:
                    line.update(med("torch_route", tq))
                if sweep_ms:
                    line.update(med("sweep", sweep_ms))
                line["byte_bound_ms"] = byte_bound
                line["share_of_byte_bound"] = byte_bound / line["draw_ms"]
                text = json.dumps(line)
                print(text, flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(text + "\n")
                del X, path
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
