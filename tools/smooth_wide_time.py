#!/usr/bin/env python
"""The time-segmented path of posterior_decode / posterior_marginals for 9 to 64 states (smooth_wide = 1: k_filter_wide
forward, k_smooth_wide_bwd backward) against the generic route (smooth_wide = 0: an E-step that stores gamma, then a
kernel over the rows -- which is also what the commit before this path ran), on one GPU and in one process
(DESIGN.md section 17).

Shapes: the 128 x 1e5 gaussian sets of tools/score_time.py at 64, 32 and 16 states (c3 | g32 | g16) and 128 x 1e4
gaussian at 64 and 16 states (s64 | s16).  Whole calls in four forms: decode (bytes to the host), decode with
confidences (bytes and float32 to the host), float32 rows left on the device, a Q = 2 projection (state index and
state mean) in float32 left on the device.  Each form: one warm-up call per route, then --reps rounds that
alternate the two routes; the mean, the fastest and the slowest call of each.  "wins" is true where the SLOWEST
call on the new path is faster than the FASTEST on the generic route -- a difference larger than the run-to-run
spread of either; the automatic rule (smooth_wide_auto, csrc/smooth_wide_launch.hpp) takes the new path only for
the lane-group classes and forms where every shape measured says so.
One JSON object per shape, printed and appended to profiles/smooth/smooth_wide_time.json.  Options: --only
c3|g32|g16|s64|s16, --reps R, --label TEXT (a "build" field in every line)."""
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
from score_time import c3_setup, g16_setup, g32_setup, gen_setup  # noqa: E402

FORMS = ("decode", "decode_conf", "rows_f32_dev", "q2_f32_dev")


def one_call(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternate(eng, fn, reps):
    """ms of `reps` calls per route, the routes taking turns; one warm-up call each first"""
    ts = {1: [], 0: []}
    for wide in (1, 0):
        eng.set_option("smooth_wide", wide)
        one_call(fn)
    for _ in range(reps):
        for wide in (1, 0):
            eng.set_option("smooth_wide", wide)
            ts[wide].append(one_call(fn))
    return ts


def block(args, setup):
    name, eng, models, obs, total = setup()
    model = models[0]
    n = eng.nstates
    V = np.column_stack([np.arange(n, dtype=float), model[2]])
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
        for wide, prefix in ((1, "wide"), (0, "generic")):
            t = ts[wide]
            line["%s_%s_ms" % (prefix, form)] = float(np.mean(t))
            line["%s_%s_ms_min" % (prefix, form)] = float(min(t))
            line["%s_%s_ms_max" % (prefix, form)] = float(max(t))
        line["generic_over_wide_" + form] = line["generic_%s_ms" % form] / line["wide_%s_ms" % form]
        line["wins_" + form] = bool(max(ts[1]) < min(ts[0]))
        # what the routes were, read after one call each
        for wide, prefix in ((1, "wide"), (0, "generic")):
            eng.set_option("smooth_wide", wide)
            fn()
            line["%s_%s_path" % (prefix, form)] = eng.get_option(call + "_path")
        eng.set_option("smooth_wide", 1)
        fn()
        line["wide_%s_fallbacks" % form] = eng.get_option(call + "_fallbacks")
    line["smooth_segments"] = eng.get_option("smooth_segments")
    eng.close()
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c3", "g32", "g16", "s64", "s16"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default=None, help="written as \"build\" into every line (e.g. the commit timed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth", "smooth_wide_time.json"))
    args = ap.parse_args()
    shapes = (("c3", c3_setup), ("g32", g32_setup), ("g16", g16_setup), ("s64", lambda: gen_setup(64)),
              ("s16", lambda: gen_setup(16)))
    for key, setup in shapes:
        if args.only in (None, key):
            block(args, setup)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
