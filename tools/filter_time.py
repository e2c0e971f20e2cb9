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
Blocks c3 | g32 | g16 (the shapes of tools/score_time.py: 128 x 1e5 gaussian at 64, 32 and 16 states) time the
time-parallel path for 9 to 64 states (k_filter_wide, filter_parallel = 1) in four forms -- float64 to the host,
float32 to the device, logc alone to the device, a Q = 1 projection to the device -- against the same build with
filter_parallel = 0 (k_filter_serial, which is also what the commit before this path ran), Engine.score with one
model (the floor) and posterior_marginals in the same form.  Block scan: one long 64-state trajectory of 4096,
16384, 65536 and 262144 steps under filter_parallel 0 and 1 -- the break-even behind FILTER_WIDE_MIN_TOTAL.
Block tile (the matrix-core path for 65 to 128 states, k_filter_tile): 128 states, 128 x 1e4 gaussian (the shape of
tools/score_time.py's g128) and 100 states discrete, M = 64, on the same 128 x 1e4 steps, in the four forms of the
c3 block under filter_tile 1 against 0 (k_filter_serial, which is also what the commit before this path ran), with
Engine.score with one model as the floor; then the scan behind FILTER_TILE_MIN_TOTAL: the first 4096 .. 1.28e6
steps of the 128-state set as trajectories of 1e4 steps (one shorter one for 4096), float32 rows and logc to the
device, filter_tile 1 against 0.
One JSON object per configuration, printed and appended to profiles/filter/filter_time.json.  Options: --only
c1|c2|c3|g32|g16|scan|tile, --reps R, --sub N, --fwd N, --label TEXT (a "build" field in every line), --filter-only (the device forms
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
from score_time import c1_setup, c2_setup, c3_setup, g16_setup, g32_setup, g128_setup  # noqa: E402
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


def wide_forms(eng, model, V, reps, line, prefix):
    """the four forms of the 9..64-state blocks under the engine's current filter_parallel"""
    n, total = eng.nstates, int(eng.offsets[-1])
    h64, l64 = np.empty((total, n)), np.empty(total)
    line.update(stats(prefix + "_f64_host", timed_all(lambda: eng.filter_states(*model, out=h64, out_increments=l64),
                                                      reps)))
    del h64, l64
    t32 = torch.empty((total, n), dtype=torch.float32, device="cuda:0")
    l32 = torch.empty(total, dtype=torch.float32, device="cuda:0")
    line.update(stats(prefix + "_f32_dev", timed_all(
        lambda: eng.filter_states(*model, dtype=np.float32, out=t32, out_increments=l32), reps)))
    del t32
    line.update(stats(prefix + "_logc_dev", timed_all(
        lambda: eng.filter_states(*model, dtype=np.float32, probabilities=False, out_increments=l32), reps)))
    tq = torch.empty((total, 1), dtype=torch.float32, device="cuda:0")
    line.update(stats(prefix + "_q1_dev", timed_all(
        lambda: eng.filter_states(*model, weights=V, dtype=np.float32, out=tq, out_increments=l32), reps)))
    line[prefix + "_path"] = eng.get_option("filter_path")
    line[prefix + "_fallbacks"] = eng.get_option("filter_fallbacks")
    line[prefix + "_segments"] = eng.get_option("filter_segments")
    del tq, l32
    torch.cuda.empty_cache()


def wide_block(args, setup):
    name, eng, models, obs, total = setup()
    model = models[0]
    n = eng.nstates
    V = np.arange(n, dtype=float)[:, None]
    line = dict(build=args.label, config=name, trajectories=len(eng.lengths), steps=total, reps=args.reps)
    eng.set_option("filter_parallel", 1)
    if args.filter_only:
        wide_forms(eng, model, V, 1, line, "wide")
        eng.close()
        return
    wide_forms(eng, model, V, args.reps, line, "wide")
    eng.set_option("filter_parallel", 0)
    wide_forms(eng, model, V, args.reps, line, "serial")
    line.update(stats("score_one_model", timed_all(lambda: eng.score([model]), args.reps)))
    t32 = torch.empty((total, n), dtype=torch.float32, device="cuda:0")
    line.update(stats("marg_f32_dev", timed_all(lambda: eng.posterior_marginals(*model, dtype=np.float32, out=t32),
                                                args.reps)))
    del t32
    tq = torch.empty((total, 1), dtype=torch.float32, device="cuda:0")
    line.update(stats("marg_q1_dev", timed_all(
        lambda: eng.posterior_marginals(*model, weights=V, dtype=np.float32, out=tq), args.reps)))
    del tq
    h64 = np.empty((total, n))
    line.update(stats("marg_f64_host", timed_all(lambda: eng.posterior_marginals(*model, out=h64), args.reps)))
    del h64
    for form in ("f64_host", "f32_dev", "logc_dev", "q1_dev"):
        line["serial_over_wide_" + form] = line["serial_%s_ms" % form] / line["wide_%s_ms" % form]
    line["wide_f32_dev_over_score"] = line["wide_f32_dev_ms"] / line["score_one_model_ms"]
    line["wide_f32_dev_over_marg"] = line["wide_f32_dev_ms"] / line["marg_f32_dev_ms"]
    emit(args, line)
    eng.close()


def scan_block(args):
    """one long 64-state trajectory (a prefix of configs[3]'s observations), float32 rows and logc to the device"""
    name, eng, models, obs, _ = c3_setup()
    model, n = models[0], eng.nstates
    eng.close()
    for total in (4096, 16384, 65536, 262144):
        eng = Engine(0)
        eng.set_observations_device("gaussian", obs.data_ptr(), np.array([0, total], dtype=np.int64), n)
        t32 = torch.empty((total, n), dtype=torch.float32, device="cuda:0")
        l32 = torch.empty(total, dtype=torch.float32, device="cuda:0")
        line = dict(build=args.label, config="scan: 64-state gaussian, one trajectory", steps=total, reps=args.reps)
        for par, key in ((0, "serial"), (1, "wide")):
            eng.set_option("filter_parallel", par)
            line.update(stats(key + "_f32_dev", timed_all(
                lambda: eng.filter_states(*model, dtype=np.float32, out=t32, out_increments=l32), args.reps)))
            line[key + "_path"] = eng.get_option("filter_path")
        line["wide_segments"] = eng.get_option("filter_segments")
        line["serial_over_wide"] = line["serial_f32_dev_ms"] / line["wide_f32_dev_ms"]
        emit(args, line)
        eng.close()
        del t32, l32


def tile_forms_block(args, name, eng, model, total):
    """the four forms under filter_tile 1 and 0, Engine.score with one model as the floor"""
    n = eng.nstates
    V = np.arange(n, dtype=float)[:, None]
    line = dict(build=args.label, config=name, trajectories=len(eng.lengths), steps=total, reps=args.reps)
    eng.set_option("filter_tile", 1)
    if args.filter_only:
        wide_forms(eng, model, V, 1, line, "tile")
        return
    wide_forms(eng, model, V, args.reps, line, "tile")
    line["tile_redone"] = eng.get_option("filter_redone")
    eng.set_option("filter_tile", 0)
    wide_forms(eng, model, V, args.reps, line, "serial")
    line.update(stats("score_one_model", timed_all(lambda: eng.score([model]), args.reps)))
    line["score_path"] = eng.get_option("score_path")
    for form in ("f64_host", "f32_dev", "logc_dev", "q1_dev"):
        line["serial_over_tile_" + form] = line["serial_%s_ms" % form] / line["tile_%s_ms" % form]
    line["tile_logc_dev_over_score"] = line["tile_logc_dev_ms"] / line["score_one_model_ms"]
    line["tile_f32_dev_over_score"] = line["tile_f32_dev_ms"] / line["score_one_model_ms"]
    emit(args, line)


def tile_block(args):
    name, eng, models, obs, total = g128_setup()
    model, n = models[0], eng.nstates
    tile_forms_block(args, name, eng, model, total)
    eng.close()
    # 100 states, discrete, M = 64, the same number of steps
    rng = np.random.default_rng(100)
    K, T, nd, M = 128, 10000, 100, 64
    A = rng.random((nd, nd)) + 0.05 + 5.0 * np.eye(nd)
    A /= A.sum(axis=1)[:, None]
    B = rng.random((nd, M)) + 0.01
    B /= B.sum(axis=1)[:, None]
    sym = torch.randint(0, M, (K * T,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    eng = Engine(0)
    eng.set_observations_device("discrete", sym.data_ptr(), np.arange(K + 1, dtype=np.int64) * T, nd, nsymbols=M)
    tile_forms_block(args, "100-state discrete M = 64, 128 x 1e4", eng, (A, np.full(nd, 1.0 / nd), B, None), K * T)
    eng.close()
    del sym
    if args.filter_only:
        return
    # the break-even behind FILTER_TILE_MIN_TOTAL
    for steps in (4096, 8192, 16384, 32768, 65536, 131072, 320000, 1280000):
        off = np.array(sorted(set(list(range(0, steps, T)) + [steps])), dtype=np.int64)
        eng = Engine(0)
        eng.set_observations_device("gaussian", obs.data_ptr(), off, n)
        t32 = torch.empty((steps, n), dtype=torch.float32, device="cuda:0")
        l32 = torch.empty(steps, dtype=torch.float32, device="cuda:0")
        line = dict(build=args.label, config="tile scan: 128-state gaussian, trajectories of 1e4 steps", steps=steps,
                    trajectories=len(off) - 1, reps=args.reps)
        for opt, key in ((0, "serial"), (1, "tile")):
            eng.set_option("filter_tile", opt)
            line.update(stats(key + "_f32_dev", timed_all(
                lambda: eng.filter_states(*model, dtype=np.float32, out=t32, out_increments=l32), args.reps)))
            line[key + "_path"] = eng.get_option("filter_path")
        line["tile_segments"] = eng.get_option("filter_segments")
        line["serial_over_tile"] = line["serial_f32_dev_ms"] / line["tile_f32_dev_ms"]
        emit(args, line)
        eng.close()
        del t32, l32


def emit(args, line):
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c1", "c2", "c3", "g32", "g16", "scan", "tile"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sub", type=int, default=32, help="trajectories of configs[2] that are filtered")
    ap.add_argument("--fwd", type=int, default=2, help="trajectories the hidden.forward route is timed on")
    ap.add_argument("--label", default=None, help="written as \"build\" into every line (e.g. the commit timed)")
    ap.add_argument("--filter-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter", "filter_time.json"))
    args = ap.parse_args()
    for key, setup in (("c3", c3_setup), ("g32", g32_setup), ("g16", g16_setup)):
        if args.only == key:        # (the 9..64-state blocks run on request only: the serial side takes seconds)
            wide_block(args, setup)
    if args.only == "scan":
        scan_block(args)
    if args.only == "tile":
        tile_block(args)
    if args.only in ("c3", "g32", "g16", "scan", "tile"):
        return
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
        emit(args, line)
        eng.close()
        del obs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
