#!/usr/bin/env python
"""bhmm_score against the E-step, on one GPU and in one process.

For configs[2] (8-state discrete, M = 64, 1024 x 1e6) and configs[1] (8-state gaussian, 256 x 1e5):
one Engine.score call with S = 1, 8 and 64 models for each kernel layout (option score_layout), and the same
S models as S E-steps.  Prints one JSON
object per measurement.  Options: --only c2|c1 (one config), --reps R, --score-only (S = 1 and 8 score
calls alone: the workload of a rocprofv3 pass)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import make_c2_model, metastable_matrix, stationary  # noqa: E402
from bhmm_amd.engine import Engine, synth_observations  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def c2_setup():
    rng = np.random.default_rng(3000)
    n, M, K, T = 8, 64, 1024, 1000000
    A = metastable_matrix(n, rng)
    pi = stationary(A)
    B = rng.dirichlet(np.ones(M), size=n)
    obs = torch.empty(K * T, dtype=torch.int32, device="cuda:0")
    synth_observations("discrete", obs.data_ptr(), A, pi, B, None, K, T, seed=17)
    torch.cuda.synchronize()
    eng = Engine(0)
    eng.set_observations_device("discrete", obs.data_ptr(), np.arange(K + 1, dtype=np.int64) * T, n, nsymbols=M)
    models = []
    for s in range(64):  # candidate models around the generating one (EM starts, posterior samples ...)
        w, v = 0.85 + 0.1 * s / 63, 0.75 + 0.2 * ((s * 37) % 64) / 63
        models.append((w * A + (1 - w) / n, pi, v * B + (1 - v) / M, None))
    return "configs[2] 8-state discrete (M=64) 1024 x 1e6", eng, models, obs, K * T


def c1_setup():
    model = make_c2_model()
    n, K, T = 8, 256, 100000
    A, pi = model["A"], model["pi"]
    obs = torch.empty(K * T, dtype=torch.float64, device="cuda:0")
    synth_observations("gaussian", obs.data_ptr(), A, pi, model["mu"], model["sigma"], K, T, seed=11)
    torch.cuda.synchronize()
    eng = Engine(0)
    eng.set_observations_device("gaussian", obs.data_ptr(), np.arange(K + 1, dtype=np.int64) * T, n)
    models = []
    for s in range(64):
        w = 0.85 + 0.1 * s / 63
        models.append((w * A + (1 - w) / n, pi, model["mu"] + 0.2 * ((s * 37) % 64) / 63, model["sigma"]))
    return "configs[1] 8-state gaussian 256 x 1e5", eng, models, obs, K * T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c2", "c1"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--score-only", action="store_true")
    ap.add_argument("--layouts", default="1,2", help="score_layout values to time (1: lane per chunk, 2: N/2 lanes)")
    args = ap.parse_args()
    for key, setup in (("c2", c2_setup), ("c1", c1_setup)):
        if args.only and key != args.only:
            continue
        name, eng, models, obs, steps = setup()
        if args.score_only:
            for layout in [int(x) for x in args.layouts.split(",")]:
                eng.set_option("score_layout", layout)
                for S in (1, 8):
                    eng.score(models[:S])
            torch.cuda.synchronize()
            eng.close()
            continue
        # the E-step of the first model, as the reference point (kernel intervals: prescan, stitch, sweep, ...)
        t_e1 = timed(lambda: eng.estep(*models[0]), args.reps)
        kms = eng.kernel_ms_all().tolist()
        print(json.dumps(dict(config=name, what="E-step, one model", ms=1e3 * t_e1, kernel_ms=kms,
                              spec_W=eng.get_option("spec_W"))), flush=True)
        layouts = [int(x) for x in args.layouts.split(",")]
        for S in (1, 8, 64):
            ms = models[:S]
            t_e = timed(lambda: [eng.estep(*m) for m in ms], max(1, args.reps if S < 64 else 1))
            for layout in layouts:
                eng.set_option("score_layout", layout)
                t_s = timed(lambda: eng.score(ms), args.reps)
                print(json.dumps(dict(config=name, layout=layout, S=S, score_ms=1e3 * t_s,
                                      score_ms_per_model=1e3 * t_s / S, estep_ms=1e3 * t_e,
                                      estep_ms_per_model=1e3 * t_e / S, score_over_estep=t_s / t_e,
                                      timesteps_models_per_s=steps * S / t_s,
                                      score_fallbacks=eng.get_option("score_fallbacks"))), flush=True)
        eng.close()
        del obs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
