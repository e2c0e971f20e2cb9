#!/usr/bin/env python
"""bhmm_score against the E-step, on one GPU and in one process.

For configs[2] (8-state discrete, M = 64, 1024 x 1e6) and configs[1] (8-state gaussian, 256 x 1e5):
one Engine.score call with S = 1, 8 and 64 models for each kernel layout (option score_layout), and the same
S models as S E-steps.  For the 9..64-state setups -- configs[3] (64-state gaussian, 128 x 1e5: the model,
observations and seed of bench.py's configs[3] block) and a 16- and a 32-state gaussian setup of the same size -- the
same per scaling of the segmented kernel (option score_lazy; on a library without the option: as it is).  For the
65..128-state setups g65 and g128 -- the shapes and the model construction of bench.py's secondary_gen (128 x 1e4
gaussian, 65 and 128 states) -- the same once (there is one scaling); these two also append their lines to
profiles/score/score_time.json.  Prints one JSON object per measurement, with the minimum and maximum over the
repetitions.  Options: --only c2|c1|c3|g16|g32|g65|g128 (one config), --reps R, --label TEXT (a "build" field in every line: which library was timed), --score-only (S = 1 and 8 score calls alone: the workload of a rocprofv3 pass)."""
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


def wide_setup(n, seed, name):
    """bench.py's configs[3] block at n states: 128 x 1e5 gaussian, 64 candidate models around the generating one"""
    rng = np.random.default_rng(seed)
    K, T = 128, 100000
    A = metastable_matrix(n, rng)
    pi = stationary(A)
    mu, sig = np.linspace(-5, 5, n), np.linspace(0.5, 2.0, n)
    obs = torch.empty(K * T, dtype=torch.float64, device="cuda:0")
    synth_observations("gaussian", obs.data_ptr(), A, pi, mu, sig, K, T, seed=100 * seed)
    torch.cuda.synchronize()
    eng = Engine(0)
    eng.set_observations_device("gaussian", obs.data_ptr(), np.arange(K + 1, dtype=np.int64) * T, n)
    models = []
    for s in range(64):
        w = 0.85 + 0.1 * s / 63
        models.append((w * A + (1 - w) / n, pi, mu + 0.2 * ((s * 37) % 64) / 63, sig))
    return name, eng, models, obs, K * T


def c3_setup():
    return wide_setup(64, 64, "configs[3] 64-state gaussian 128 x 1e5")


def g16_setup():
    return wide_setup(16, 16, "16-state gaussian 128 x 1e5")


def g32_setup():
    return wide_setup(32, 32, "32-state gaussian 128 x 1e5")


def gen_setup(n):
    """bench.py's secondary_gen at n states: 128 x 1e4 gaussian, 64 candidate models around the generating one"""
    rng = np.random.default_rng(n)
    K, T = 128, 10000
    A = metastable_matrix(n, rng)
    pi = stationary(A)
    mu, sig = np.linspace(-5, 5, n), np.linspace(0.5, 2.0, n)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(n)
    obs = torch.randn(K * T, dtype=torch.float64, device="cuda:0", generator=g) * 3.0
    torch.cuda.synchronize()
    eng = Engine(0)
    eng.set_observations_device("gaussian", obs.data_ptr(), np.arange(K + 1, dtype=np.int64) * T, n)
    models = [(0.9 * A + 0.1 / n, pi, mu + 0.05, sig)]     # secondary_gen's model first
    for s in range(1, 64):
        w = 0.85 + 0.1 * s / 63
        models.append((w * A + (1 - w) / n, pi, mu + 0.2 * ((s * 37) % 64) / 63, sig))
    return "%d-state gaussian 128 x 1e4" % n, eng, models, obs, K * T


def g65_setup():
    return gen_setup(65)


def g128_setup():
    return gen_setup(128)


def opt(eng, name):
    try:
        return eng.get_option(name)
    except ValueError:
        return None


def wide_main(args, setup, one_scaling=False, keep=None):
    name, eng, models, obs, steps = setup()
    lazies = [int(x) for x in args.lazy.split(",")] if opt(eng, "score_lazy") is not None else [None]
    if one_scaling:
        lazies = [None]
    if args.score_only:
        for S in (1, 8):
            eng.score(models[:S])
        torch.cuda.synchronize()
        eng.close()
        return
    for S in (1, 8, 64):
        ms = models[:S]
        reps = args.reps if S < 64 else max(2, args.reps // 2)
        te = timed_all(lambda: [eng.estep(*m) for m in ms], args.reps if S < 64 else 1)
        for lazy in lazies:
            if lazy is not None:
                eng.set_option("score_lazy", lazy)
            ts = timed_all(lambda: eng.score(ms), reps)
            line = json.dumps(dict(build=args.label, config=name, lazy=lazy, S=S, reps=reps, score_ms_per_model=np.mean(ts) / S,
                                   score_ms_per_model_min=min(ts) / S, score_ms_per_model_max=max(ts) / S,
                                   estep_ms_per_model=np.mean(te) / S, estep_ms_per_model_min=min(te) / S,
                                   estep_ms_per_model_max=max(te) / S,
                                   timesteps_models_per_s=steps * S / (1e-3 * np.mean(ts)),
                                   score_path=opt(eng, "score_path"), score_segments=opt(eng, "score_segments"),
                                   score_W_max=opt(eng, "score_W_max"),
                                   score_fallbacks=opt(eng, "score_fallbacks")))
            print(line, flush=True)
            if keep:
                os.makedirs(os.path.dirname(keep), exist_ok=True)
                with open(keep, "a") as f:
                    f.write(line + "\n")
    eng.close()
    del obs
    torch.cuda.empty_cache()


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
    ap.add_argument("--only", choices=["c2", "c1", "c3", "g16", "g32", "g65", "g128"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--score-only", action="store_true")
    ap.add_argument("--layouts", default="1,2", help="score_layout values to time (1: lane per chunk, 2: N/2 lanes)")
    ap.add_argument("--label", default=None, help="written as \"build\" into every line (e.g. the commit timed)")
    ap.add_argument("--lazy", default="1,0", help="score_lazy values to time at 9..64 states (1: refresh every "
                                                   "fourth step, 0: sum every step)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score", "score_time.json"),
                    help="file the g65 / g128 lines are appended to")
    args = ap.parse_args()
    for key, setup in (("c3", c3_setup), ("g16", g16_setup), ("g32", g32_setup)):
        if not args.only or key == args.only:
            wide_main(args, setup)
    for key, setup in (("g65", g65_setup), ("g128", g128_setup)):
        if not args.only or key == args.only:
            wide_main(args, setup, one_scaling=True, keep=args.out)
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
        print(json.dumps(dict(build=args.label, config=name, what="E-step, one model", ms=1e3 * t_e1, kernel_ms=kms,
                              spec_W=eng.get_option("spec_W"))), flush=True)
        layouts = [int(x) for x in args.layouts.split(",")]
        for S in (1, 8, 64):
            ms = models[:S]
            t_e = timed(lambda: [eng.estep(*m) for m in ms], max(1, args.reps if S < 64 else 1))
            for layout in layouts:
                eng.set_option("score_layout", layout)
                t_s = timed(lambda: eng.score(ms), args.reps)
                print(json.dumps(dict(build=args.label, config=name, layout=layout, S=S, score_ms=1e3 * t_s,
                                      score_ms_per_model=1e3 * t_s / S, estep_ms=1e3 * t_e,
                                      estep_ms_per_model=1e3 * t_e / S, score_over_estep=t_s / t_e,
                                      timesteps_models_per_s=steps * S / t_s,
                                      score_fallbacks=eng.get_option("score_fallbacks"))), flush=True)
        eng.close()
        del obs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
