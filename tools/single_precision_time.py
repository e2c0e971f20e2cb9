"""fp32 against fp64 E-steps (BHMM_FLAG_SINGLE) and mixed-precision against fp64 EM, on one GPU.

  python tools/single_precision_time.py [--reps R] [--warmup W] [--c2 K T] [--c1 K T] [--em K T]

E-steps: configs[2] (discrete, 8 states, M = 64) and configs[1] (gaussian, 8 states), the
workloads of bench.py (imported, not changed), with fp64 and fp32 E-steps alternating in one
process on one context; each E-step is timed from launch to the fetched statistics with the device
synchronised before.  Whole EM: MaximumLikelihoodEstimator to convergence on a configs[1]-shaped
problem from the perturbed evaluation model, estep_precision 'mixed' against 'float64'.
Prints one JSON line: times, speedups, f32_used, and the largest deviation of every statistic
between the fp32 and the fp64 E-step (in the units of the accuracy contract of
tests/test_single_precision_gpu.py).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workload generators)


def deviations(r32, r64, kind, K, sigma=None):
    sc = r64.state_counts
    d = {
        "logL_rel": abs(r32.loglik - r64.loglik) / abs(r64.loglik),
        "gamma0_of_K": float(np.max(np.abs(r32.gamma0_sum - r64.gamma0_sum)) / K),
        "C_of_row": float(np.max(np.abs(r32.C - r64.C) / np.maximum(r64.C.sum(axis=1)[:, None], 1e-300))),
        "state_counts_of_total": float(np.max(np.abs(r32.state_counts - sc)) / sc.sum()),
    }
    if r64.logL_k is not None and r32.logL_k is not None:
        d["logL_k_rel"] = float(np.max(np.abs(r32.logL_k - r64.logL_k) / np.abs(r64.logL_k)))
    if kind == "gaussian":
        d["sum_gd_of_sc_sigma"] = float(np.max(np.abs(r32.sum_gd - r64.sum_gd) / (sc * sigma)))
        d["sum_gdd_rel"] = float(np.max(np.abs(r32.sum_gdd - r64.sum_gdd) / np.abs(r64.sum_gdd)))
    else:
        d["symbol_counts_of_state"] = float(np.max(np.abs(r32.symbol_counts - r64.symbol_counts) / sc[:, None]))
    return d


def estep_leg(wl, reps, warmup):
    import torch
    from bhmm_amd.engine import Engine, synth_observations
    K, T = wl.K, wl.T
    dt = torch.float64 if wl.kind == "gaussian" else torch.int32
    obs = torch.empty(K * T, dtype=dt, device="cuda:0")
    A, pi, p0, p1 = wl.gen
    synth_observations(wl.kind, obs.data_ptr(), A, pi, p0, p1, K, T, seed=wl.seed, device=0)
    torch.cuda.synchronize()
    eng = Engine(0)
    eng.set_observations_device(wl.kind, obs.data_ptr(), np.arange(K + 1, dtype=np.int64) * T, wl.n,
                                nsymbols=wl.M)
    A, pi, p0, p1 = wl.margs

    def one(single):
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.estep_launch(A, pi, p0, p1, single=single)
        res = eng.estep_fetch()
        dt_ms = (time.perf_counter() - t) * 1e3
        return res, dt_ms, eng.get_option("f32_used")

    for _ in range(warmup):
        one(False)
        one(True)
    t64, t32, used = [], [], []
    r64 = r32 = None
    for _ in range(reps):
        r64, t, _u = one(False)
        t64.append(t)
        r32, t, u = one(True)
        t32.append(t)
        used.append(u)
    out = {
        "workload": wl.name,
        "fp64_ms_median": float(np.median(t64)), "fp32_ms_median": float(np.median(t32)),
        "fp64_ms": [round(x, 3) for x in t64], "fp32_ms": [round(x, 3) for x in t32],
        "speedup": float(np.median(t64) / np.median(t32)),
        "f32_used": float(min(used)), "f32_fallbacks": eng.get_option("f32_fallbacks"),
        "f32_W": eng.get_option("f32_W"), "spec_W": eng.get_option("spec_W"),
        "deviation": deviations(r32, r64, wl.kind, K, sigma=p1),
    }
    eng.close()
    return out


def em_leg(K, T, accuracy, maxit):
    import torch
    import bhmm_amd
    from bhmm_amd.engine import synth_observations
    from bhmm_amd.estimators.maximum_likelihood import MaximumLikelihoodEstimator
    wl = bench.workload_configs1(K, T)
    obs_d = torch.empty(K * T, dtype=torch.float64, device="cuda:0")
    A, pi, mu, sigma = wl.gen
    synth_observations("gaussian", obs_d.data_ptr(), A, pi, mu, sigma, K, T, seed=wl.seed, device=0)
    obs = list(obs_d.cpu().numpy().reshape(K, T))
    del obs_d
    A0, pi0, mu0, sg0 = wl.margs
    out = {"shape": "configs[1] shape, %d x %d, accuracy %g" % (K, T, accuracy)}
    fits = {}
    for prec in ("float64", "mixed", "float64", "mixed"):   # (second round: warm caches, the one reported)
        init = bhmm_amd.gaussian_hmm(pi0, A0, mu0, sg0)
        est = MaximumLikelihoodEstimator(obs, wl.n, initial_model=init, output="gaussian",
                                         accuracy=accuracy, maxit=maxit, estep_precision=prec)
        torch.cuda.synchronize()
        t = time.perf_counter()
        est.fit()
        fits[prec] = (time.perf_counter() - t, est)
    (t64, e64), (tmx, emx) = fits["float64"], fits["mixed"]
    out.update({
        "float64_s": t64, "mixed_s": tmx, "speedup": t64 / tmx,
        "float64_iterations": len(e64.likelihoods), "mixed_iterations": len(emx.likelihoods),
        "mixed_precisions": "".join("s" if p == "float32" else "d" for p in emx.estep_precisions),
        "likelihood_rel": abs(emx.likelihood - e64.likelihood) / abs(e64.likelihood),
        "max_abs_dT": float(np.max(np.abs(emx.transition_matrix - e64.transition_matrix))),
        "max_abs_dpi": float(np.max(np.abs(emx.initial_probability - e64.initial_probability))),
        "max_abs_dmu": float(np.max(np.abs(emx.output_model.means - e64.output_model.means))),
        "max_abs_dsigma": float(np.max(np.abs(emx.output_model.sigmas - e64.output_model.sigmas))),
    })
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--c2", type=int, nargs=2, default=[1024, 1000000])
    ap.add_argument("--c1", type=int, nargs=2, default=[256, 100000])
    ap.add_argument("--em", type=int, nargs=2, default=[256, 100000])
    ap.add_argument("--em-accuracy", type=float, default=1e-3)
    ap.add_argument("--em-maxit", type=int, default=200)
    a = ap.parse_args()
    res = {"tool": "single_precision_time"}
    res["configs2"] = estep_leg(bench.workload_configs2(*a.c2), a.reps, a.warmup)
    res["configs1"] = estep_leg(bench.workload_configs1(*a.c1), a.reps, a.warmup)
    res["em"] = em_leg(a.em[0], a.em[1], a.em_accuracy, a.em_maxit)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
