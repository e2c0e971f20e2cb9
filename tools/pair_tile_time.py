#!/usr/bin/env python
"""The two row kernels of the generic path of bhmm_posterior_transitions on the same build, on one GPU and in one
process: whole Engine.posterior_transitions calls with the option pair_rows 0 (k_pair_rows)
and 1 (k_pair_tile), float32 left on the device, in the jump form and with Q = 2 and Q = 8 projections, and beside
them the two calls every such call contains, alone, as it makes them: filter_states and posterior_marginals with
full float64 rows left on the device.  Shapes (gaussian, the observation sets and models of tools/score_time.py):
16, 32 and 64 states at 128 x 1e5; 64, 100 and 128 states at 128 x 1e4.  Each figure is the mean (min, max) of
--reps calls after one warm-up call.  One JSON object per shape, printed and appended to
profiles/pair/pair_tile_time.json.  Options: --only KEY[,KEY...] (g16 g32 c3 g64s g100 g128), --reps R,
--label TEXT (a "build" field in every line)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from score_time import c3_setup, g16_setup, g32_setup, gen_setup, timed_all  # noqa: E402

SHAPES = (("g16", g16_setup), ("g32", g32_setup), ("c3", c3_setup), ("g64s", lambda: gen_setup(64)),
          ("g100", lambda: gen_setup(100)), ("g128", lambda: gen_setup(128)))


def stats(prefix, ts):
    return {prefix + "_ms": float(np.mean(ts)), prefix + "_ms_min": float(min(ts)), prefix + "_ms_max": float(max(ts))}


def weights(n, Q):
    """Q unit pairs off the diagonal"""
    W = np.zeros((n, n, Q))
    for q in range(Q):
        W[q % n, (q + 1) % n, q] = 1.0
    return W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--label", default=None, help="written as \"build\" into every line (e.g. the commit timed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair", "pair_tile_time.json"))
    args = ap.parse_args()
    only = args.only.split(",") if args.only else None
    for key, setup in SHAPES:
        if only and key not in only:
            continue
        name, eng, models, obs, steps = setup()
        model = models[0]
        n, total = eng.nstates, len(eng.lengths) * int(eng.lengths[0])
        line = dict(build=args.label, config=name, states=n, steps=steps, reps=args.reps)
        rows = torch.empty((total, n), dtype=torch.float64, device="cuda:0")
        line.update(stats("filter_f64_dev", timed_all(
            lambda: eng.filter_states(*model, increments=False, out=rows), args.reps)))
        line.update(stats("marg_f64_dev", timed_all(lambda: eng.posterior_marginals(*model, out=rows), args.reps)))
        line["filter_path"], line["marg_path"] = eng.get_option("filter_path"), eng.get_option("marg_path")
        del rows
        torch.cuda.empty_cache()
        for form, Q in (("jump", 0), ("q2", 2), ("q8", 8)):
            W = weights(n, Q) if Q else None
            out = torch.empty((total, Q) if Q else (total,), dtype=torch.float32, device="cuda:0")
            for kernel in (1, 0):
                eng.set_option("pair_rows", kernel)
                ts = timed_all(lambda: eng.posterior_transitions(*model, weights=W, dtype=np.float32, out=out),
                               args.reps)
                assert eng.get_option("pair_rows_kernel") == kernel and eng.get_option("pair_path") == 0
                line.update(stats("pair_%s_%s" % (form, "tile" if kernel else "rows"), ts))
            line["pair_%s_rows_over_tile" % form] = line["pair_%s_rows_ms" % form] / line["pair_%s_tile_ms" % form]
            line["pair_%s_tile_share_of_contained_calls" % form] = (
                (line["filter_f64_dev_ms"] + line["marg_f64_dev_ms"]) / line["pair_%s_tile_ms" % form])
            del out
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
