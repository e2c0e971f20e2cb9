#!/usr/bin/env python
"""Engine.decode_runs against the route there was before it, on one GPU and in one process.

For configs[1] (8-state gaussian, 256 x 1e5) and configs[2] (8-state discrete, M = 64, 1024 x 1e6), the observation
sets and models of tools/score_time.py, and for both decoders ('viterbi', 'posterior'):

  new route   the whole Engine.decode_runs call with statistics (decode, compaction on the device, run_off and the
              tables to the host, the runs fetched): "runs_ms" (device time of count, scan and scatter), R and the
              bytes that crossed the link;
  old route   viterbi_u8 / posterior_decode into a pinned host buffer, then a numpy run-length encoding with the
              same outputs (per trajectory np.flatnonzero(np.diff(p)), statistics by np.add.at / np.maximum.at):
              "decode_host_ms" and "encode_host_ms";
  floor       two streaming reads of the path at the copy rate measured here (a device-to-device copy of the path
              reads and writes it once): "two_reads_ms", and runs_ms over it.

One JSON object per (config, method), printed and appended to profiles/runs/path_runs_time.json.  Options: --only
c1|c2, --reps R, --host-reps R (the host encoding at configs[2] takes seconds), --label TEXT, --out FILE."""
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


def host_encode(path, offsets, n):
    """the run-length encoding a caller does on the host today, with the outputs of decode_runs(stats=True)"""
    run_off = np.zeros(len(offsets), dtype=np.int64)
    S, L, Q = [], [], []
    dwell, jumps = np.zeros((n, 5), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    for k in range(len(offsets) - 1):
        p = path[offsets[k]:offsets[k + 1]]
        if p.size == 0:
            run_off[k + 1] = run_off[k]
            continue
        s = np.concatenate([[0], np.flatnonzero(np.diff(p)) + 1])
        ln = np.diff(np.concatenate([s, [p.size]]))
        q = p[s].astype(np.int32)
        np.add.at(dwell[:, 0], q, 1)
        np.add.at(dwell[:, 1], q, ln)
        np.maximum.at(dwell[:, 2], q, ln)
        for e in {0, s.size - 1}:
            dwell[q[e], 3] += 1
            dwell[q[e], 4] += ln[e]
        np.add.at(jumps, (q[:-1], q[1:]), 1)
        run_off[k + 1] = run_off[k] + s.size
        S.append(s), L.append(ln), Q.append(q)
    return run_off, np.concatenate(S), np.concatenate(L), np.concatenate(Q), dwell, jumps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c1", "c2"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--label", default=None, help="written as \"build\" into every line (e.g. the commit timed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "runs", "path_runs_time.json"))
    args = ap.parse_args()
    for key, setup in (("c1", c1_setup), ("c2", c2_setup)):
        if args.only and key != args.only:
            continue
        name, eng, models, obs, steps = setup()
        model = models[0]
        n, K = eng.nstates, len(eng.lengths)
        pinned = torch.empty(steps, dtype=torch.uint8, pin_memory=True)
        host = pinned.numpy()
        # the copy rate of this card on a buffer of the path's size: one read and one write of `steps` bytes
        a = torch.empty(steps, dtype=torch.uint8, device="cuda:0")
        b = torch.empty_like(a)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.copy_(a)
        ev0.record()
        for _ in range(5):
            b.copy_(a)
        ev1.record()
        torch.cuda.synchronize()
        copy_ms = ev0.elapsed_time(ev1) / 5
        del a, b
        torch.cuda.empty_cache()
        for method in ("viterbi", "posterior"):
            line = dict(build=args.label, config=name, method=method, steps=steps, trajectories=K, reps=args.reps,
                        runs_tile=eng.get_option("runs_tile"), runs_lane=eng.get_option("runs_lane"))
            res = [None]

            def new_route():
                res[0] = eng.decode_runs(*model, method=method, stats=True)

            ms = []
            tn = []
            new_route()
            torch.cuda.synchronize()
            for _ in range(args.reps):
                t0 = time.perf_counter()
                new_route()
                torch.cuda.synchronize()
                tn.append(1e3 * (time.perf_counter() - t0))
                ms.append(eng.get_option("runs_ms"))
            line.update(stats("decode_runs", tn))
            line.update(stats("runs", ms))
            R = res[0].count
            line["runs_count"] = R
            line["steps_per_run"] = steps / R
            line["link_bytes_new"] = int(8 * (K + 1) + 8 * (5 * n + n * n) + 20 * R)
            line["link_bytes_old"] = int(steps)
            line["copy_ms"] = copy_ms                       # one read + one write of the path
            line["two_reads_ms"] = copy_ms                  # two reads move the same bytes
            line["runs_over_two_reads"] = line["runs_ms"] / copy_ms
            if method == "viterbi":
                decode = lambda: eng.viterbi_u8(*model, out=pinned)          # noqa: E731
            else:
                decode = lambda: eng.posterior_decode(*model, out=host)      # noqa: E731
            line.update(stats("decode_host", timed_all(decode, args.reps)))
            enc = [None]

            def encode():
                enc[0] = host_encode(host, eng.offsets, n)

            te = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                encode()
                te.append(1e3 * (time.perf_counter() - t0))
            line.update(stats("encode_host", te))
            line["old_route_ms"] = line["decode_host_ms"] + line["encode_host_ms"]
            line["speedup"] = line["old_route_ms"] / line["decode_runs_ms"]
            # both routes computed the same thing
            r = res[0]
            same = all(np.array_equal(x, y) for x, y in zip(
                (r.offsets, r.start, r.length, r.state, r.dwell, r.jumps), enc[0]))
            line["routes_agree"] = bool(same)
            text = json.dumps(line)
            print(text, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        eng.close()
        del obs, pinned, host
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
