#!/usr/bin/env python
"""bhmm_filter against its floor, its bigger sibling and the route there was before it, on one GPU and in one
process.

For configs[1] (8-state gaussian, 256 x 1e5) and the first --sub trajectories of configs[2] (8-state discrete,
M = 64, 1e6 steps each; an engine of its own on that slice of the observations of tools/score_time.py), whole
calls of Engine.filter_states in five forms: float64 to the host, float32 to the host, float32 left on the
device, logc alone left on the device and a Q = 1 projection (the state index) left on the device -- against
  (a) Engine.score with one model: the same sweep without per-step output, the floor;
  (b) Engine.posterior_marginals in the same output form: it does strictly more work;
  (c) the route a user had before this call: pobs on the host and hidden.forward per trajectory, timed on the
      first --fwd trajectories and scaled to the set ("forward_route_trajectories" says how many ran).
One JSON object per configuration, printed and appended to profiles/filter/filter_time.json.  Options: --only
c1|c2, --reps R, --sub N, --fwd N, --label TEXT (a "build" field in every line), --filter-only (the device forms
alone: the workload of a rocprofv3 --kernel-trace --stats pass)."""
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


def device_forms(eng, model, V, reps, line, marginals=True):
    n, total = eng.nstates, int(eng.offsets[-1])
    t32 = torch.empty((total, n), dtype=torch.float32, device="cuda:0")
    l32 = torch.empty(total, dtype=torch.float32, device="cuda:0")
    ts = timed_all(lambda: eng.filter_states(*model, dtype=np.float32, out=t32, out_increments=l32), reps)
    line.update(stats("filter_f32_dev", ts))
    line["sweep_gbps_f32_dev"] = total * (n + 1) * 4 / (1e6 * min(ts))
    ts = timed_all(lambda: eng.filter_states(*model, dtype=np.float32, increments=False, out=t32), reps)
    line.update(stats("filter_f32_dev_rows_only", ts))
    if marginals:
        line.update(stats("marg_f32_dev", timed_all(lambda: eng.posterior_marginals(*model, dtype=np.float32, out=t32),
                                                    reps)))
    del t32
    ts = timed_all(lambda: eng.filter_states(*model, dtype=np.float32, probabilities=False, out_increments=l32), reps)
    line.update(stats("filter_logc_dev", ts))
    tq = torch.empty((total, 1), dtype=torch.float32, device="cuda:0")
    ts = timed_all(lambda: eng.filter_states(*model, weights=V, dtype=np.float32, out=tq, out_increments=l32), reps)
    line.update(stats("filter_q1_dev", ts))
    if marginals:
        line.update(stats("marg_q1_dev", timed_all(
            lambda: eng.posterior_marginals(*model, weights=V, dtype=np.float32, out=tq), reps)))
    del tq, l32
    torch.cuda.empty_cache()


def forward_route(kind, obs_host, model, count):
    """what a user had before: the emission table on the host, then hidden.forward, per trajectory"""
    from bhmm_amd import hidden
    from bhmm_amd.output_models import DiscreteOutputModel, GaussianOutputModel
    A, pi, p0, p1 = model
    om = GaussianOutputModel(len(pi), means=p0, sigmas=p1) if kind == "gaussian" else DiscreteOutputModel(p0)
    for k in range(count):
        hidden.forward(A, om.p_obs(obs_host[k]), pi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c1", "c2"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sub", type=int, default=32, help="trajectories of configs[2] that are filtered")
    ap.add_argument("--fwd", type=int, default=2, help="trajectories the hidden.forward route is timed on")
    ap.add_argument("--label", default=None, help="written as \"build\" into every line (e.g. the commit timed)")
    ap.add_argument("--filter-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter", "filter_time.json"))
    args = ap.parse_args()
    for key, setup in (("c1", c1_setup), ("c2", c2_setup)):
        if args.only and key != args.only:
            continue
        name, eng, models, obs, steps = setup()
        model = models[0]
        kind, n, M, K = eng.kind, eng.nstates, eng.nsymbols, len(eng.lengths)
        T = int(eng.lengths[0])
        sub = K if key == "c1" else min(args.sub, K)
        if sub != K:
            eng.close()
            eng = Engine(0)
            eng.set_observations_device(kind, obs.data_ptr(), np.arange(sub + 1, dtype=np.int64) * T, n, nsymbols=M)
        total = sub * T
        V = np.arange(n, dtype=float)[:, None]
        line = dict(build=args.label, config=name, trajectories=sub, steps=total, reps=args.reps)
        if args.filter_only:
            device_forms(eng, model, V, 1, line, marginals=False)
            eng.close()
            continue
        line.update(stats("score_one_model", timed_all(lambda: eng.score([model]), args.reps)))
        device_forms(eng, model, V, args.reps, line)
        h64, l64 = np.empty((total, n)), np.empty(total)
        line.update(stats("filter_f64_host",
                          timed_all(lambda: eng.filter_states(*model, out=h64, out_increments=l64), args.reps)))
        line.update(stats("marg_f64_host", timed_all(lambda: eng.posterior_marginals(*model, out=h64), args.reps)))
        del h64, l64
        h32, l32 = np.empty((total, n), dtype=np.float32), np.empty(total, dtype=np.float32)
        line.update(stats("filter_f32_host", timed_all(
            lambda: eng.filter_states(*model, dtype=np.float32, out=h32, out_increments=l32), args.reps)))
        line.update(stats("marg_f32_host",
                          timed_all(lambda: eng.posterior_marginals(*model, dtype=np.float32, out=h32), args.reps)))
        del h32, l32
        for o in ("filter_path", "filter_fallbacks", "marg_path", "score_path"):
            line[o] = eng.get_option(o)
        line["chunks"], line["chunk_len"] = eng.num_chunks, eng.chunk_len
        fwd = min(args.fwd, sub)
        obs_host = obs[:fwd * T].cpu().numpy().reshape(fwd, T)
        t0 = time.perf_counter()
        forward_route(kind, obs_host, model, fwd)
        line["forward_route_trajectories"] = fwd
        line["forward_route_ms_scaled"] = 1e3 * (time.perf_counter() - t0) * sub / fwd
        line["filter_f32_dev_over_score"] = line["filter_f32_dev_ms"] / line["score_one_model_ms"]
        line["filter_f32_dev_over_marg"] = line["filter_f32_dev_ms"] / line["marg_f32_dev_ms"]
        line["forward_route_over_filter_f64_host"] = line["forward_route_ms_scaled"] / line["filter_f64_host_ms"]
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
