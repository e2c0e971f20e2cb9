#!/usr/bin/env python
"""The matrix-core path of posterior_decode / posterior_marginals for 65 to 128 states (smooth_tile = 1: k_filter_tile
forward, k_smooth_tile_bwd backward) against the generic route (smooth_tile = 0: an E-step that stores gamma, then a
kernel over the rows -- which is also what the commit before this path ran), on one GPU and in one process
(DESIGN.md section 18).

Shapes: 128 states gaussian at 128 x 1e4 (s128) and 128 x 1e5 (l128), 100 states discrete with 64 symbols at
128 x 1e4 (d100).  Whole calls in four forms: decode (bytes to the host), decode with confidences (bytes and float32
to the host), float32 rows left on the device, a Q = 2 projection (state index and state mean, or state index and
its square) in float32 left on the device.  Each form: one warm-up call per route, then --reps rounds that alternate
the two routes, the host clock around a device synchronise; the mean, the fastest and the slowest call of each.
"wins" is true where the SLOWEST call on the new path is faster than the FASTEST on the generic route -- a
difference larger than the run-to-run spread of either; the automatic rule (smooth_tile_auto,
csrc/smooth_tile_api.hpp) takes the new path only for the forms where every shape measured says so.
--memory (l128 only): the device memory each route holds after one decode call on a fresh engine, as the drop of
the free memory the runtime reports around it (the engine's buffers only grow, so that is its peak).
One JSON object per shape, printed and appended to profiles/smooth/smooth_tile_time.json.  Options: --only
s128|l128|d100, --reps R, --memory, --label TEXT (a "build" field in every line)."""
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
from score_time import gen_setup, metastable_matrix, stationary  # noqa: E402

FORMS = ("decode", "decode_conf", "rows_f32_dev", "q2_f32_dev")


def d100_setup():
    """100 states, 64 symbols, 128 x 1e4 uniform symbols; a random model with a heavy diagonal"""
    from bhmm_amd.engine import Engine
    rng = np.random.default_rng(100)
    n, M, K, T = 100, 64, 128, 10000
    A = rng.random((n, n)) + 0.05 + 5.0 * np.eye(n)
    A /= A.sum(axis=1)[:, None]
    pi = np.full(n, 1.0 / n)
    B = rng.dirichlet(np.ones(M), size=n)
    obs = torch.randint(0, M, (K * T,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    eng = Engine(0)
    eng.set_observations_device("discrete", obs.data_ptr(), np.arange(K + 1, dtype=np.int64) * T, n, nsymbols=M)
    return "100-state discrete (M=64) 128 x 1e4", eng, [(A, pi, B, None)], obs, K * T


def l128_setup():
    """gen_setup(128)'s model on 128 x 1e5 steps drawn the same way"""
    from bhmm_amd.engine import Engine
    n, K, T = 128, 128, 100000
    rng = np.random.default_rng(n)
    A = metastable_matrix(n, rng)
    pi = stationary(A)
    mu, sig = np.linspace(-5, 5, n), np.linspace(0.5, 2.0, n)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(n)
    obs = torch.randn(K * T, dtype=torch.float64, device="cuda:0", generator=g) * 3.0
    torch.cuda.synchronize()
    eng = Engine(0)
    eng.set_observations_device("gaussian", obs.data_ptr(), np.arange(K + 1, dtype=np.int64) * T, n)
    return "128-state gaussian 128 x 1e5", eng, [(0.9 * A + 0.1 / n, pi, mu + 0.05, sig)], obs, K * T


def one_call(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternate(eng, fn, reps):
    """ms of `reps` calls per route, the routes taking turns; one warm-up call each first"""
    ts = {1: [], 0: []}
    for tile in (1, 0):
        eng.set_option("smooth_tile", tile)
        one_call(fn)
    for _ in range(reps):
        for tile in (1, 0):
            eng.set_option("smooth_tile", tile)
            ts[tile].append(one_call(fn))
    return ts


def held_after_decode(setup, tile):
    """MiB of device memory a fresh engine holds after one decode call on the given route"""
    torch.cuda.synchronize()
    name, eng, models, obs, total = setup()
    free0 = torch.cuda.mem_get_info()[0]
    eng.set_option("smooth_tile", tile)
    eng.posterior_decode(*models[0], out=np.empty(total, dtype=np.uint8))
    torch.cuda.synchronize()
    held = (free0 - torch.cuda.mem_get_info()[0]) / 2.0 ** 20
    path = eng.get_option("post_path")
    eng.close()
    del obs
    torch.cuda.empty_cache()
    return held, path


def block(args, setup, memory):
    name, eng, models, obs, total = setup()
    model = models[0]
    n = eng.nstates
    second = model[2] if model[3] is not None else np.arange(n, dtype=float) ** 2
    V = np.column_stack([np.arange(n, dtype=float), second])
    line = dict(build=args.label, config=name, states=n, trajectories=len(eng.lengths), steps=total, reps=args.reps)
    path = np.empty(total, dtype=np.uint8)
    t32 = torch.empty((total, n), dtype=torch.float32, device="cuda:0")
    tq = torch.empty((total, 2), dtype=torch.float32, device="cuda:0")
    calls = {
        "decode": (lambda: eng.posterior_decode(*model, out=path), "post"),
        "decode_conf": (lambda: eng.posterior_decode(*model, confidence=True, out=path), "post"),
        "rows_f32_dev": (lambda: eng.posterior_marginals(*model, dtype=np.float32, out=t32), "marg"),
        "q2_f32_dev": (lambda: eng.posterior_marginals(*model, weights=V, dtype=np.float32, out=tq), "marg"),
    }
    for form in FORMS:
        fn, call = calls[form]
        ts = alternate(eng, fn, args.reps)
        for tile, prefix in ((1, "tile"), (0, "generic")):
            t = ts[tile]
            line["%s_%s_ms" % (prefix, form)] = float(np.mean(t))
            line["%s_%s_ms_min" % (prefix, form)] = float(min(t))
            line["%s_%s_ms_max" % (prefix, form)] = float(max(t))
        line["generic_over_tile_" + form] = line["generic_%s_ms" % form] / line["tile_%s_ms" % form]
        line["wins_" + form] = bool(max(ts[1]) < min(ts[0]))
        # what the routes were, read after the last call of each
        for tile, prefix in ((1, "tile"), (0, "generic")):
            eng.set_option("smooth_tile", tile)
            fn()
            line["%s_%s_path" % (prefix, form)] = eng.get_option(call + "_path")
        line["tile_%s_fallbacks" % form] = eng.get_option(call + "_fallbacks")
    eng.set_option("smooth_tile", 1)
    calls["decode"][0]()
    line["smooth_segments"] = eng.get_option("smooth_segments")
    eng.close()
    del t32, tq, obs
    torch.cuda.empty_cache()
    if memory:
        for tile, prefix in ((1, "tile"), (0, "generic")):
            held, p = held_after_decode(setup, tile)
            line["%s_decode_held_mib" % prefix] = held
            line["%s_decode_held_path" % prefix] = p
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["s128", "l128", "d100"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--memory", action="store_true", help="l128: device memory held by each route after one decode")
    ap.add_argument("--label", default=None, help="written as \"build\" into every line (e.g. the commit timed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth", "smooth_tile_time.json"))
    args = ap.parse_args()
    shapes = (("s128", lambda: gen_setup(128)), ("d100", d100_setup),
              ("l128", l128_setup))
    for key, setup in shapes:
        if args.only in (None, key):
            block(args, setup, args.memory and key == "l128")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
