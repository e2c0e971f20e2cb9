#!/usr/bin/env python
"""bhmm_posterior_transitions against the closest existing call and against the route there was before it, on one
GPU and in one process.

For configs[1] (8-state gaussian, 256 x 1e5: the fused path) and for 16 and 64 states (gaussian, 128 x 1e5: the
generic path), the observation sets and models of tools/score_time.py: Engine.posterior_transitions in the jump
form and with a Q = 2 projection (two unit pairs), float32, left on the device; Engine.posterior_marginals with a
Q = 1 projection in the same dtype, left on the device -- the same traffic without the n * n pair work; and the only
route a caller had before this call -- filter_states and posterior_marginals to the host in float64, then numpy
(xi_t(i,j) = f_t(i) A_ij gamma_t+1(j) / pred_j, summed off the diagonal) -- timed on the first --sub trajectories (an
engine of its own on that slice of the same observations; "sub_trajectories" says so, and "route_ms_scaled" is that
time times K / sub).  One JSON object per measurement, printed and appended to profiles/pair/pair_time.json.
Options: --only c1|g16|c3, --reps R, --sub N, --label TEXT (a "build" field in every line), --pair-only (the two
device forms alone: the workload of a profiler pass)."""
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
from score_time import c1_setup, c3_setup, g16_setup  # noqa: E402
from bhmm_amd.engine import Engine  # noqa: E402


def timed_all(fn, reps):
    """ms of each of `reps` calls after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def stats(prefix, ts):
    return {prefix + "_ms": float(np.mean(ts)), prefix + "_ms_min": float(min(ts)), prefix + "_ms_max": float(max(ts))}


def numpy_route(eng, model):
    """what a caller had before: both row sets to the host, then the pair sum in numpy, trajectory by trajectory"""
    A = np.asarray(model[0])
    filt, _ = eng.filter_states(*model, increments=False)
    gam = eng.posterior_marginals(*model)
    out = []
    for f, g in zip(filt, gam):
        pred = f[:-1] @ A
        c = np.divide(g[1:], pred, out=np.zeros_like(pred), where=pred > 0)
        stay = ((f[:-1] * np.diag(A)[None, :]) * c).sum(axis=1)
        out.append(1.0 - stay)                    # (the pairs of a step sum to one)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c1", "g16", "c3"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sub", type=int, default=16, help="trajectories of the host route")
    ap.add_argument("--label", default=None, help="written as \"build\" into every line (e.g. the commit timed)")
    ap.add_argument("--pair-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair", "pair_time.json"))
    args = ap.parse_args()
    for key, setup in (("c1", c1_setup), ("g16", g16_setup), ("c3", c3_setup)):
        if args.only and key != args.only:
            continue
        name, eng, models, obs, steps = setup()
        model = models[0]
        kind, n, M, K = eng.kind, eng.nstates, eng.nsymbols, len(eng.lengths)
        T = int(eng.lengths[0])
        total = K * T
        W2 = np.zeros((n, n, 2))
        W2[0, 1, 0] = W2[1, 0, 1] = 1.0
        V1 = (np.arange(n) < n // 2).astype(float)[:, None]
        line = dict(build=args.label, config=name, steps=steps, reps=args.reps)
        tj = torch.empty(total, dtype=torch.float32, device="cuda:0")
        line.update(stats("pair_jump_f32_dev",
                          timed_all(lambda: eng.posterior_transitions(*model, dtype=np.float32, out=tj), args.reps)))
        del tj
        tq = torch.empty((total, 2), dtype=torch.float32, device="cuda:0")
        line.update(stats("pair_q2_f32_dev", timed_all(
            lambda: eng.posterior_transitions(*model, weights=W2, dtype=np.float32, out=tq), args.reps)))
        del tq
        for o in ("pair_path", "pair_fallbacks"):
            line[o] = eng.get_option(o)
        if not args.pair_only:
            tm = torch.empty((total, 1), dtype=torch.float32, device="cuda:0")
            line.update(stats("marg_q1_f32_dev", timed_all(
                lambda: eng.posterior_marginals(*model, weights=V1, dtype=np.float32, out=tm), args.reps)))
            del tm
            line["marg_path"] = eng.get_option("marg_path")
            sub = min(args.sub, K)
            seng = Engine(0)
            seng.set_observations_device(kind, obs.data_ptr(), np.arange(sub + 1, dtype=np.int64) * T, n, nsymbols=M)
            line["sub_trajectories"] = sub
            line.update(stats("route", timed_all(lambda: numpy_route(seng, model), args.reps)))
            seng.close()
            line["route_ms_scaled"] = line["route_ms"] * K / sub
            line["pair_jump_over_marg_q1"] = line["pair_jump_f32_dev_ms"] / line["marg_q1_f32_dev_ms"]
            line["pair_q2_over_marg_q1"] = line["pair_q2_f32_dev_ms"] / line["marg_q1_f32_dev_ms"]
            line["route_scaled_over_pair_jump"] = line["route_ms_scaled"] / line["pair_jump_f32_dev_ms"]
        text = json.dumps(line)
        print(text, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
        eng.close()
        del obs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
