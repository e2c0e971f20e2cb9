#!/usr/bin/env python
"""Engine.path_logprob / Engine.decode_logprob against the routes there were before them, on one GPU and in one
process.

For configs[1] (8-state gaussian, 256 x 1e5) and configs[2] (8-state discrete, M = 64, 1024 x 1e6), the observation
sets and models of tools/score_time.py, and for a 64-state (128 x 1e5) and a 256-state (128 x 1e4) gaussian set:

  path_logprob    whole calls on the Viterbi path in a device tensor with S = 1 and S = 8 models, and "pathlp_ms"
                  (device time of prepare, tiles and finish);
  decode_logprob  the whole call (method 'viterbi') against (b) the bare decode call, viterbi_u8 into a device tensor;
  (a) old route   viterbi_u8 into a pinned host buffer, then the numpy route over path and observations per
                  trajectory (log A[p[:-1], p[1:]] and the emission terms, summed); at configs[2] the numpy part is
                  timed on --host-traj trajectories and scaled to all of them ("numpy_scaled_from");
  (c) bound       the bytes the pass must read -- 1 B of path + 8 B of gaussian or 4 B of discrete observation per
                  step -- at the HBM rate of DESIGN.md section 0 (8 TB/s): "stream_ms", and its share of pathlp_ms.

One JSON object per (config, S), printed and appended to profiles/pathlp/path_logprob_time.json.  Options: --only
c1|c2|g64|g256, --reps R, --host-traj N, --label TEXT, --out FILE."""
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
from score_time import c1_setup, c2_setup, c3_setup, gen_setup  # noqa: E402

HBM_BYTES_PER_S = 8e12
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


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


def host_logprob(kind, path, obs, offsets, model, ntraj):
    """the numpy route a caller takes today, over the first ntraj trajectories"""
    A, pi, p0, p1 = model
    with np.errstate(divide="ignore"):
        lA, lpi = np.log(A), np.log(pi)
        lB = np.log(p0) if kind == "discrete" else None
    out = np.zeros(ntraj)
    for k in range(ntraj):
        p = path[offsets[k]:offsets[k + 1]].astype(np.intp)
        o = obs[offsets[k]:offsets[k + 1]]
        if p.size == 0:
            continue
        if kind == "discrete":
            e = lB[p, o]
        else:
            e = -0.5 * ((o - p0[p]) / p1[p]) ** 2 - np.log(p1)[p] - LOG_SQRT_2PI
        out[k] = lpi[p[0]] + lA[p[:-1], p[1:]].sum() + e.sum()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c1", "c2", "g64", "g256"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-traj", type=int, default=32, help="trajectories of configs[2] the numpy route is timed on")
    ap.add_argument("--label", default=None, help="written as \"build\" into every line (e.g. the commit timed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pathlp", "path_logprob_time.json"))
    args = ap.parse_args()
    setups = (("c1", c1_setup), ("c2", c2_setup), ("g64", c3_setup), ("g256", lambda: gen_setup(256)))
    for key, setup in setups:
        if args.only and key != args.only:
            continue
        name, eng, models, obs, steps = setup()
        kind, n, K = eng.kind, eng.nstates, len(eng.lengths)
        model = tuple(None if x is None else np.asarray(x, dtype=np.float64) for x in models[0])
        dev = torch.empty(steps, dtype=torch.uint8, device="cuda:0")
        pinned = torch.empty(steps, dtype=torch.uint8, pin_memory=True)
        bare = timed_all(lambda: eng.viterbi_u8(*model, out=dev), args.reps)             # (b)
        dec = timed_all(lambda: eng.decode_logprob(*model, method="viterbi"), args.reps)
        dec_dev_ms = eng.get_option("pathlp_ms")
        to_host = timed_all(lambda: eng.viterbi_u8(*model, out=pinned), args.reps)       # (a), first half
        host_obs = obs.cpu().numpy()
        ntraj = K if key != "c2" else min(K, args.host_traj)
        t0 = time.perf_counter()
        ref = host_logprob(kind, pinned.numpy(), host_obs, eng.offsets, model, ntraj)
        numpy_ms = 1e3 * (time.perf_counter() - t0) * K / ntraj
        del host_obs
        stream_ms = 1e3 * steps * (1 + (8 if kind == "gaussian" else 4)) / HBM_BYTES_PER_S   # (c)
        for S in (1, 8):
            res = [None]

            def call():
                res[0] = eng.path_logprob(dev, models[:S])

            tn, ms = [], []
            call()
            for _ in range(args.reps):
                t0 = time.perf_counter()
                call()
                tn.append(1e3 * (time.perf_counter() - t0))
                ms.append(eng.get_option("pathlp_ms"))
            line = dict(build=args.label, config=name, S=S, steps=steps, trajectories=K, states=n, reps=args.reps,
                        pathlp_tile=eng.get_option("pathlp_tile"), pathlp_lane=eng.get_option("pathlp_lane"),
                        pathlp_table=eng.get_option("pathlp_table"))
            line.update(stats("path_logprob", tn))
            line.update(stats("pathlp", ms))
            line["stream_ms"] = stream_ms
            line["stream_share"] = stream_ms / float(min(ms))
            line.update(stats("decode_logprob", dec))
            line["decode_logprob_pathlp_ms"] = dec_dev_ms
            line.update(stats("bare_decode", bare))
            line.update(stats("decode_host", to_host))
            line["numpy_ms"] = numpy_ms
            line["numpy_scaled_from"] = ntraj
            line["old_route_ms"] = line["decode_host_ms"] + numpy_ms
            line["speedup_decode"] = line["old_route_ms"] / line["decode_logprob_ms"]
            line["link_bytes_new"] = int(8 * K * S)
            line["link_bytes_old"] = int(steps)
            err = np.abs(res[0][0, :ntraj] - ref) / (1.0 + np.abs(ref))
            line["routes_agree"] = bool(np.all(err < 1e-9))
            text = json.dumps(line)
            print(text, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        eng.close()
        del obs, dev, pinned
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
