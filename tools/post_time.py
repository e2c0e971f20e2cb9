#!/usr/bin/env python
"""bhmm_posterior_decode against the routes there were before it, on one GPU and in one process (DESIGN.md
section 14).

For configs[1] (8-state gaussian, 256 x 1e5) and configs[2] (8-state discrete, M = 64, 1024 x 1e6), the
observation sets and models of tools/score_time.py: the whole Engine.posterior_decode call (paths as bytes on
the host) with and without the confidences; beside it the route through the gamma rows --
estep(store_gamma=True), Engine.gamma(k) for every trajectory and argmax / max on the host -- and the bare
E-step.  At configs[2] the gamma route would move 65 GB through the host one trajectory at a time: it is timed on
the first --sub trajectories (an engine of its own on that slice of the same observations) and the line says so
("gamma_route_trajectories"; "gamma_route_ms_scaled" is that time times K / sub).  One JSON object per
measurement, printed and appended to profiles/post/post_time.json.  Options: --only c1|c2, --reps R, --label TEXT
(a "build" field in every line: which library was timed), --sub N, --decode-only (two decode calls alone: the
workload of a rocprofv3 pass)."""
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
    """what a caller had before: the gamma rows through the host, argmax and max there"""
    eng.estep(*model, store_gamma=True)
    paths, conf = [], []
    for k in range(len(eng.lengths)):
        g = eng.gamma(k)
        paths.append(g.argmax(axis=1).astype(np.uint8))
        conf.append(g.max(axis=1).astype(np.float32))
    return paths, conf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c1", "c2"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sub", type=int, default=32, help="trajectories of the gamma route at configs[2]")
    ap.add_argument("--label", default=None, help="written as \"build\" into every line (e.g. the commit timed)")
    ap.add_argument("--decode-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post", "post_time.json"))
    args = ap.parse_args()
    for key, setup in (("c1", c1_setup), ("c2", c2_setup)):
        if args.only and key != args.only:
            continue
        name, eng, models, obs, steps = setup()
        model = models[0]
        kind, n, M, K = eng.kind, eng.nstates, eng.nsymbols, len(eng.lengths)
        T = int(eng.lengths[0])
        out = np.empty(steps, dtype=np.uint8)
        if args.decode_only:
            eng.posterior_decode(*model, out=out)
            eng.posterior_decode(*model, confidence=True, out=out)
            torch.cuda.synchronize()
            eng.close()
            continue
        line = dict(build=args.label, config=name, steps=steps, reps=args.reps)
        line.update(stats("estep", timed_all(lambda: eng.estep(*model), args.reps)))
        line["estep_kernel_ms"] = eng.kernel_ms_all().tolist()
        line.update(stats("decode", timed_all(lambda: eng.posterior_decode(*model, out=out), args.reps)))
        line.update(stats("decode_conf",
                          timed_all(lambda: eng.posterior_decode(*model, confidence=True, out=out), args.reps)))
        for o in ("post_path", "post_fallbacks", "post_ws_mb"):
            line[o] = eng.get_option(o)
        line["chunks"], line["chunk_len"] = eng.num_chunks, eng.chunk_len
        # the gamma route, on all trajectories where that is feasible, else on the first --sub
        sub = K if key == "c1" else min(args.sub, K)
        if sub == K:
            geng = eng
        else:
            geng = Engine(0)
            geng.set_observations_device(kind, obs.data_ptr(), np.arange(sub + 1, dtype=np.int64) * T, n, nsymbols=M)
        reps = args.reps if sub == K else 1
        line.update(stats("estep_gamma", timed_all(lambda: geng.estep(*model, store_gamma=True), reps)))
        tg = timed_all(lambda: gamma_route(geng, model), reps)
        line.update(stats("gamma_route", tg))
        line["gamma_route_trajectories"] = sub
        line["gamma_route_ms_scaled"] = float(np.mean(tg)) * K / sub
        if geng is not eng:
            line.update(stats("decode_sub", timed_all(lambda: geng.posterior_decode(*model), reps)))
            geng.close()
        line["decode_over_estep"] = line["decode_ms"] / line["estep_ms"]
        line["timesteps_per_s"] = steps / (1e-3 * line["decode_ms"])
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
