#!/usr/bin/env python
"""bhmm_posterior_marginals against the route there was before it, on one GPU and in one process (DESIGN.md
section 15).

For configs[1] (8-state gaussian, 256 x 1e5) and configs[2] (8-state discrete, M = 64, 1024 x 1e6), the
observation sets and models of tools/score_time.py: a bare E-step; an E-step that stores gamma; the route a
caller had for gamma of all trajectories -- estep(store_gamma=True) and Engine.gamma(k) for every k, the code
path of the commit before this call existed, which the library still contains; and Engine.posterior_marginals
in four forms: float64 to the host, float32 to the host, float32 left on the device, and a Q = 2 projection
(one set membership, the state index) in float32 left on the device.  At configs[2] gamma is 65 GB in float64:
everything that moves gamma is timed on the first --sub trajectories (an engine of its own on that slice of the
same observations; "sub_trajectories" says so), and the two device forms also on the whole set.  "sweep_gbps_*"
is the bytes of the result over the whole call's time -- a lower bound of the kernel's write bandwidth; the
kernel split comes from a rocprofv3 --kernel-trace --stats pass over --marg-only.  One JSON object per
measurement, printed and appended to profiles/marg/marg_time.json.  Options: --only c1|c2, --reps R, --label
TEXT (a "build" field in every line), --sub N, --marg-only (the device forms alone: the workload of a profiler
pass)."""
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
from score_time import c1_setup, c2_setup  # noqa: E402
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


def gamma_route(eng, model):
    """what a caller had before: an E-step that stores gamma, then one fetch per trajectory"""
    eng.estep(*model, store_gamma=True)
    return [eng.gamma(k) for k in range(len(eng.lengths))]


def device_forms(eng, model, V, reps, line, suffix=""):
    """float32 rows and the Q = 2 projection left on the device"""
    n, total = eng.nstates, int(eng.offsets[-1])
    t32 = torch.empty((total, n), dtype=torch.float32, device="cuda:0")
    ts = timed_all(lambda: eng.posterior_marginals(*model, dtype=np.float32, out=t32), reps)
    line.update(stats("marg_f32_dev" + suffix, ts))
    line["sweep_gbps_f32_dev" + suffix] = total * n * 4 / (1e6 * min(ts))
    del t32
    tq = torch.empty((total, V.shape[1]), dtype=torch.float32, device="cuda:0")
    ts = timed_all(lambda: eng.posterior_marginals(*model, weights=V, dtype=np.float32, out=tq), reps)
    line.update(stats("marg_q2_dev" + suffix, ts))
    del tq
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c1", "c2"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sub", type=int, default=32, help="trajectories of everything that moves gamma at configs[2]")
    ap.add_argument("--label", default=None, help="written as \"build\" into every line (e.g. the commit timed)")
    ap.add_argument("--marg-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marg", "marg_time.json"))
    args = ap.parse_args()
    for key, setup in (("c1", c1_setup), ("c2", c2_setup)):
        if args.only and key != args.only:
            continue
        name, eng, models, obs, steps = setup()
        model = models[0]
        kind, n, M, K = eng.kind, eng.nstates, eng.nsymbols, len(eng.lengths)
        T = int(eng.lengths[0])
        V = np.column_stack([(np.arange(n) < n // 2).astype(float), np.arange(n, dtype=float)])
        line = dict(build=args.label, config=name, steps=steps, reps=args.reps)
        if args.marg_only:
            device_forms(eng, model, V, 1, line)
            eng.close()
            continue
        line.update(stats("estep", timed_all(lambda: eng.estep(*model), args.reps)))
        line["estep_kernel_ms"] = eng.kernel_ms_all().tolist()
        line.update(stats("decode", timed_all(lambda: eng.posterior_decode(*model), args.reps)))
        # what moves gamma: on all trajectories where that is feasible, else on the first --sub
        sub = K if key == "c1" else min(args.sub, K)
        if sub == K:
            geng = eng
        else:
            device_forms(eng, model, V, args.reps, line, "_full")
            geng = Engine(0)
            geng.set_observations_device(kind, obs.data_ptr(), np.arange(sub + 1, dtype=np.int64) * T, n, nsymbols=M)
        line["sub_trajectories"] = sub
        reps = args.reps if sub == K else 1
        line.update(stats("estep_gamma", timed_all(lambda: geng.estep(*model, store_gamma=True), reps)))
        line.update(stats("gamma_route", timed_all(lambda: gamma_route(geng, model), reps)))
        device_forms(geng, model, V, reps, line)
        total = sub * T
        h64 = np.empty((total, n))
        line.update(stats("marg_f64_host", timed_all(lambda: geng.posterior_marginals(*model, out=h64), reps)))
        del h64
        h32 = np.empty((total, n), dtype=np.float32)
        line.update(stats("marg_f32_host",
                          timed_all(lambda: geng.posterior_marginals(*model, dtype=np.float32, out=h32), reps)))
        del h32
        p32 = torch.empty((total, n), dtype=torch.float32).pin_memory()
        line.update(stats("marg_f32_pinned",
                          timed_all(lambda: geng.posterior_marginals(*model, dtype=np.float32, out=p32), reps)))
        del p32
        for o in ("marg_path", "marg_fallbacks", "marg_ws_mb"):
            line[o] = geng.get_option(o)
        line["chunks"], line["chunk_len"] = geng.num_chunks, geng.chunk_len
        line["gamma_route_over_marg_f64_host"] = line["gamma_route_ms"] / line["marg_f64_host_ms"]
        if geng is not eng:
            geng.close()
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
