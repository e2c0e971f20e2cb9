#!/usr/bin/env python
"""bench.py -- E-step throughput of the MI355X forward-backward engine.

Metric (BASELINE.json): timesteps/s of one full E-step (fused emission probabilities +
scaled forward + backward + gamma / xi / emission sufficient statistics), whole job.
One "step" of this benchmark = one E-step over the whole resident batch, from "model handed
to the engine" to "reduced statistics on the host" -- the call sequence of
bhmm/estimators/maximum_likelihood.py:249-265 plus the sums of :271-282.

Workload (`value`, at every N): BASELINE.json configs[2], the shape the metric and the north-star
target are quoted on -- 8-state discrete-output HMM (M = 64 symbols), 1024 trajectories x 1e6 time
steps IN TOTAL.  One MI355X holds it (4.1 GB of observations, 16 GB of workspace); at N GPUs it is
STRONG-scaled: rank r holds trajectories r*1024/N .. of the same global set (drawn on the device by
global index, so every N sees the same data and the summed log-likelihood must reproduce the
committed N = 1 value), and the packed sufficient statistics are all-reduced over RCCL, once per step.

    python bench.py --gpus 1 --steps 200 --warmup 50    # the defaults
    python bench.py --gpus N ...        # WORLD_SIZE unset: starts N ranks itself (torchrun)
    python bench.py ... --dump-outputs DIR   # + the statistics of the last timed step as DIR/<field>.npy
    python bench.py ... --full          # + everything below that is not the headline figure
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run does what `value` needs and nothing more: it draws the data, warms up, times the K steps,
writes --dump-outputs and prints the line.  The line carries, for THAT workload, `roofline` (algorithmic
bytes of SURVEY.md 8(d), 136 B per time step, over the sweep kernels' duration by HIP events of the
timed steps; PMC traffic and issue rate from the offline passes named in `traffic_source`) and
`kernel_ms`, both read off the timed steps themselves.

With --full the run goes on after the headline: a steady-state window behind the timed steps
(`steady_state_ms`), `cpu_baseline` (the reference's own C kernels on one core on a bounded sample of
the same trajectories, plus `all_cores`; rank 0, also at N > 1), at N > 1 the all-reduce alone, and at
N = 1 the PMC traffic and issue rate measured by the run itself (three rocprofv3 passes), plus
`configs1_gaussian` -- BASELINE configs[1] (8-state Gaussian, 256 x 1e5), the headline of rounds 1-4,
with its own roofline and CPU figure so that series continues -- `configs3_64_states`,
`more_than_64_states`, `secondary` (Viterbi and the Gibbs path step at the configs[1] shape, whole EM
iterations and whole Gibbs sweeps, host side included) and `projected_8gpu`.  At N > 1 `secondary`
holds the whole EM iterations / Gibbs sweeps of the estimator classes, sharded.  The --no-* options
below take parts out of a --full run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NSTATES = 8
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
B_ALG_GAUSS = 2 * 8 + 16 * NSTATES   # 144 B / time step, SURVEY.md section 8(d)


# ---------------------------------------------------------------------------------------
# synthetic workload (recipe of bhmm/util/testsystems.py:26-65,159-160 restated)
# ---------------------------------------------------------------------------------------
def metastable_matrix(n, rng, lifetime_min=10.0, lifetime_max=100.0):
    lt = np.linspace(np.log(lifetime_min), np.log(lifetime_max), n)
    diag = 1.0 - 1.0 / np.exp(lt)
    X = rng.random((n, n))
    X = X + X.T
    T = X / X.sum(axis=1)[:, None]
    for i in range(n):
        T[i, i] = 0.0
        T[i, :] *= (1.0 - diag[i]) / T[i, :].sum()
        T[i, i] = 1.0 - T[i, :].sum()
    return T


def stationary(T):
    p = np.full(T.shape[0], 1.0 / T.shape[0])
    for _ in range(20000):
        q = p @ T
        if np.abs(q - p).max() < 1e-15:
            break
        p = q
    return p / p.sum()


def make_c2_model(n=NSTATES, seed=2):
    """Generating model + the (perturbed) model the E-step is evaluated with."""
    rng = np.random.default_rng(1000 * seed)
    A = metastable_matrix(n, rng)
    mu = np.linspace(-5.0, 5.0, n)
    sigma = np.linspace(0.5, 2.0, n)
    pi = stationary(A)
    return dict(A=A, mu=mu, sigma=sigma, pi=pi, A_eval=0.9 * A + 0.1 / n, mu_eval=mu + 0.1)


def synth_hidden(model, K, T, seed):
    """K hidden paths of length T, vectorised over trajectories."""
    rng = np.random.default_rng(seed)
    A, pi = model["A"], model["pi"]
    n = A.shape[0]
    cdf = np.cumsum(A, axis=1)
    cdf[:, -1] = 1.0
    s = np.empty((T, K), dtype=np.int8)
    cur = np.minimum(np.searchsorted(np.cumsum(pi), rng.random(K)), n - 1)
    s[0] = cur
    for t in range(1, T):
        u = rng.random(K)
        cur = (u[:, None] > cdf[cur]).sum(axis=1)
        s[t] = cur
    return np.ascontiguousarray(s.T)


def synth_gaussian(model, K, T, seed):
    s = synth_hidden(model, K, T, seed)
    rng = np.random.default_rng(seed + 7919)
    return model["mu"][s] + model["sigma"][s] * rng.standard_normal((K, T))


def synth_gaussian_device(model, K, T, seed, device):
    """Observations as one trajectory-concatenated fp64 tensor on `device`."""
    import torch
    obs = synth_gaussian(model, K, T, seed)
    return torch.from_numpy(obs.reshape(-1)).to(device)


# ---------------------------------------------------------------------------------------
# CPU baseline: the reference's own C kernels (oracle/_ref, compiled from the reference
# sources) driven through the call sequence of maximum_likelihood.py:249-265.  The reference
# is single-threaded by construction (maximum_likelihood.py:26-27), so ONE core is the
# like-for-like figure; "all_cores" runs the same per-trajectory sequence on a thread per host
# core (ctypes and numpy release the GIL inside the kernels; every thread owns its buffers).
# Falls back to this repo's restatement (oracle/liboracle.so, kind "port").
# ---------------------------------------------------------------------------------------
def _cpu_estep_traj(orc, use_ref, kind, o, A, pi, par0, par1, bufs):
    """p_obs + forward + backward + gamma + xi of ONE trajectory; returns its log-likelihood."""
    pobs, alpha, beta, gamma, C = bufs
    if not use_ref:
        return orc.estep(kind, [o], A, pi, par0, par1)["logL"][0]
    if kind == "gaussian":
        orc.ref_pobs_gaussian(o, par0, par1, out=pobs)
        outl = np.where(pobs.sum(axis=1) == 0)[0]          # outputmodel.py:126-130
        if outl.size:
            pobs[outl, :] = 1.0
    else:
        np.copyto(pobs, par0[:, o].T)                      # discrete.py:150-153
    l, _ = orc.ref_forward(A, pobs, pi, alpha)
    orc.ref_backward(A, pobs, beta)
    orc.ref_gamma(alpha, beta, out=gamma)                  # hidden/api.py:176-186
    orc.ref_transition_counts(alpha, beta, A, pobs, C)
    return l


def cpu_baseline(kind, A, pi, par0, par1, obs_sample, threads=1):
    """obs_sample: (K, T) array.  Returns (dict, list of per-trajectory log-likelihoods)."""
    from oracle import oracle as orc
    A, pi, par0 = (np.ascontiguousarray(x, dtype=np.float64) for x in (A, pi, par0))
    par1 = np.ascontiguousarray(par1, dtype=np.float64) if par1 is not None else None
    K, T = obs_sample.shape
    n = A.shape[0]
    use_ref = orc.ref_available()
    if use_ref:
        orc.ref()

    def work(ks):
        bufs = [np.zeros((T, n)) for _ in range(4)] + [np.zeros((n, n))]
        return [(k, _cpu_estep_traj(orc, use_ref, kind, np.ascontiguousarray(obs_sample[k]), A, pi,
                                    par0, par1, bufs)) for k in ks]

    t0 = time.perf_counter()
    if threads <= 1:
        res = work(range(K))
        dt = time.perf_counter() - t0
        ll = [l for _, l in sorted(res)]
        how = "%.1f s on 1 core" % dt
    else:
        # all host cores: OpenMP over trajectories in C (oracle/omp_driver.c) around the same kernels
        ll, used, which = orc.estep_batch_omp(kind, obs_sample, A, pi, par0, par1, threads=threads)
        dt = time.perf_counter() - t0
        ll = list(ll)
        use_ref = which == "reference"
        how = "%.1f s on %d OpenMP threads (oracle/omp_driver.c)" % (dt, used)
        threads = used
    return dict(value=K * T / dt, unit="timesteps/s", cores=threads,
                kind="reference" if use_ref else "port",
                sample="%d of the workload's trajectories x %d steps, %d-state %s, "
                       "p_obs+forward+backward+gamma+xi per trajectory as in "
                       "maximum_likelihood.py:249-265, %s" % (K, T, n, kind, how)), ll


def host_cores():
    try:
        return len(os.sched_getaffinity(0))
    except AttributeError:
        return os.cpu_count() or 1


# ---------------------------------------------------------------------------------------
# N > 1 without a launcher: start the ranks ourselves.  This parent never touches the GPU.
# ---------------------------------------------------------------------------------------
class OnlyTheResultOnStdout(object):
    """The contract is ONE JSON line on stdout.  RCCL writes a version banner to the C-level stdout of every
    process that creates a communicator (also the one-rank communicator of the 8-GPU projection), so from here
    on file descriptor 1 is stderr; emit() flushes the C buffers there and writes the result to the real stdout."""

    def __init__(self):
        sys.stdout.flush()
        self.real = os.dup(1)
        os.dup2(2, 1)

    def emit(self, line):
        import ctypes
        sys.stdout.flush()
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        os.write(self.real, (line + "\n").encode())


def self_launch(args, argv):
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    p = subprocess.run(cmd, stdout=subprocess.PIPE, env=env)
    line = None
    for ln in p.stdout.decode("utf-8", "replace").splitlines():
        if ln.startswith('{"metric"'):
            line = ln
        else:
            print(ln, file=sys.stderr)
    if line is not None:
        print(line)
    elif p.returncode == 0:
        print("bench.py: the ranks printed no result line", file=sys.stderr)
        return 1
    return p.returncode


def timeit(fn, reps, sync, batches=1):
    """Seconds per call: `reps` calls back to back between two syncs; with batches > 1 the median
    over that many such batches (the secondary measurements: a single host-side hiccup on a shared
    box -- seen: one batch in ~20 at twice the time with unchanged kernel durations -- must not
    stand for the figure)."""
    fn()
    sync()
    out = []
    for _ in range(batches):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        out.append((time.perf_counter() - t0) / reps)
    return float(np.median(out))


# ---------------------------------------------------------------------------------------
# what the measurements need to know about the job
# ---------------------------------------------------------------------------------------
class Ranks(object):
    """What the secondary measurements need to know about the job."""

    def __init__(self, torch, dist, world, rank, local, dev, backend, distributed, stream=None):
        self.torch, self.dist = torch, dist
        self.world, self.rank, self.local, self.dev = world, rank, local, dev
        self.backend, self.distributed, self.stream = backend, distributed, stream

    def fence(self):
        self.torch.cuda.synchronize(self.dev)
        if self.distributed:
            self.dist.barrier()
        self.torch.cuda.synchronize(self.dev)

    def max_over_ranks(self, seconds):
        if not self.distributed:
            return seconds
        t = self.torch.tensor([seconds], dtype=self.torch.float64,
                              device=self.dev if self.backend == "nccl" else "cpu")
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def sum_stats(self, stats_dev_tensor):
        """Packed statistics of all ranks on the host (ONE all-reduce + ONE copy)."""
        if not self.distributed:
            return stats_dev_tensor.cpu().numpy()
        if self.backend == "nccl":
            self.dist.all_reduce(stats_dev_tensor)
            return stats_dev_tensor.cpu().numpy()
        h = stats_dev_tensor.cpu()
        self.dist.all_reduce(h)
        return h.numpy()



# ---------------------------------------------------------------------------------------
# the two E-step workloads of the line
# ---------------------------------------------------------------------------------------
# log-likelihood of the configs[2] evaluation model on the default workload (1024 x 1e6, seed 3000),
# measured at N = 1 (profiles/r03): every N must reproduce it, the trajectories being drawn by
# GLOBAL index.  Other shapes: not recorded.
C2_LOGLIK_N1 = {(1024, 1000000): -4043229364.929859}


class Workload(object):
    """One E-step workload: the generating model (data), the model the E-step is evaluated with,
    the shape, and the algorithmic bytes per time step of SURVEY.md 8(d)."""

    def __init__(self, key, name, kind, n, M, K, T, seed, gen, margs, b_alg, kernel):
        self.key, self.name, self.kind, self.n, self.M = key, name, kind, n, M
        self.K, self.T, self.seed, self.gen, self.margs = K, T, seed, gen, margs
        self.b_alg, self.kernel = b_alg, kernel


def workload_configs2(K, T, n=NSTATES, M=64):
    """BASELINE configs[2]: 8-state discrete-output HMM, M = 64 symbols (M is this
    build's choice, BASELINE leaves it open), 1024 trajectories x 1e6 steps."""
    rng = np.random.default_rng(3000)
    A = metastable_matrix(n, rng)
    pi = stationary(A)
    B = rng.dirichlet(np.ones(M), size=n)
    return Workload("configs2", "configs[2]: 8-state discrete HMM (M=%d), %d traj x %d steps" % (M, K, T),
                    "discrete", n, M, K, T, 3000, (A, pi, B, None),
                    (0.9 * A + 0.1 / n, pi, 0.8 * B + 0.2 / M, None), 2 * 4 + 16 * n,
                    "k_estep_light<8,discrete,spec,P1> + k_estep<8,discrete,spec,P2> (the sweep of one E-step)")


def workload_configs1(K, T):
    """BASELINE configs[1]: 8-state Gaussian HMM, 256 trajectories x 1e5 steps."""
    m = make_c2_model()
    return Workload("configs1", "configs[1]: 8-state Gaussian HMM, %d traj x %d steps" % (K, T),
                    "gaussian", NSTATES, 0, K, T, 2000, (m["A"], m["pi"], m["mu"], m["sigma"]),
                    (m["A_eval"], m["pi"], m["mu_eval"], m["sigma"]), B_ALG_GAUSS,
                    "k_estep_light<8,gauss,spec,P1> + k_estep<8,gauss,spec,P2> (the sweep of one E-step)")


KERNEL_NAMES = ["prescan", "stitch", "fwdbwd", "finalize", "estep_total"]


def dump_outputs(d, res):
    """--dump-outputs: the reduced statistics of the last timed E-step, one float64 .npy per field (a few
    KB in all).  The workload is seeded, so two builds run with the same arguments can be compared field
    by field."""
    os.makedirs(d, exist_ok=True)
    fields = {"loglik": np.array([res.loglik]), "gamma0_sum": res.gamma0_sum, "transition_counts": res.C,
              "state_counts": res.state_counts, "sum_gd": res.sum_gd, "sum_gdd": res.sum_gdd,
              "symbol_counts": res.symbol_counts}
    for name, a in fields.items():
        if a is not None:
            np.save(os.path.join(d, name + ".npy"), np.asarray(a, dtype=np.float64))


class Series(object):
    """This rank's share of a workload on its GPU and the timing protocol of the contract on it."""

    def __init__(self, rk, wl, Kloc, first_traj, chunk=0):
        from bhmm_amd.engine import Engine, synth_observations
        torch = rk.torch
        self.rk, self.wl, self.Kloc = rk, wl, Kloc
        self.obs = torch.empty(Kloc * wl.T, dtype=torch.int32 if wl.kind == "discrete" else torch.float64,
                               device=rk.dev)
        t0 = time.perf_counter()
        # drawn ON THE DEVICE by global trajectory index (bhmm_synth_observations_at): rank r's slice is
        # exactly what one call for the whole set would have drawn for these trajectories
        synth_observations(wl.kind, self.obs.data_ptr(), wl.gen[0], wl.gen[1], wl.gen[2], wl.gen[3], Kloc, wl.T,
                           seed=wl.seed, device=rk.local, first_traj=first_traj)
        torch.cuda.synchronize(rk.dev)
        self.synth_seconds = time.perf_counter() - t0
        # a dedicated (non-default) stream shared by the engine and the collective: the legacy default
        # stream would serialise against every other stream of the process
        self.eng = eng = Engine(rk.local, stream=rk.stream.cuda_stream)
        self.off = np.arange(Kloc + 1, dtype=np.int64) * wl.T
        eng.set_observations_device(wl.kind, self.obs.data_ptr(), self.off, wl.n, nsymbols=wl.M, chunk=chunk)
        self.S = eng.stats_size
        self.stats = torch.zeros(self.S, dtype=torch.float64, device=rk.dev)
        self.host_stats = torch.zeros(self.S, dtype=torch.float64).pin_memory()
        self.host_np = self.host_stats.numpy()          # (same memory)
        self.allreduces = 0

    def one_step(self):
        """Model in -> reduced statistics of ALL ranks on the host."""
        rk, eng, m = self.rk, self.eng, self.wl.margs
        if not rk.distributed:
            # single GPU: the library lands the statistics in pinned host memory itself
            eng.estep_launch(m[0], m[1], m[2], m[3])
            eng.estep_fetch_packed(self.host_np)
            return self.host_stats
        eng.estep_launch(m[0], m[1], m[2], m[3], stats_dev=self.stats.data_ptr())
        self.allreduces += 1
        if rk.backend == "nccl":
            rk.dist.all_reduce(self.stats)                  # RCCL sum of the packed statistics
            self.host_stats.copy_(self.stats, non_blocking=True)
            rk.stream.synchronize()                         # statistics are on the host
        else:
            self.host_stats.copy_(self.stats)
            rk.dist.all_reduce(self.host_stats)
        return self.host_stats

    def run(self, warmup, steps, steady_n):
        rk, eng = self.rk, self.eng
        for _ in range(warmup):
            self.one_step()
        kern_ms = np.zeros(5)
        n0 = self.allreduces
        rk.fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.one_step()                         # returns with the results on the host: events complete
            if rk.distributed:
                eng.sync()                          # (no fetch on this path: read the events here)
            kern_ms += eng.kernel_ms_all()
        rk.fence()
        self.elapsed = rk.max_over_ranks(time.perf_counter() - t0)
        self.last_timed = self.host_np.copy()       # what the last timed step handed its caller
        self.allreduces_per_step = (self.allreduces - n0) / float(max(steps, 1))
        self.kern_ms = kern_ms / max(steps, 1)
        # a second window right behind the requested steps, untimed by the contract: what an EM loop of
        # hundreds of iterations sees once the GPU's power management has settled
        steady = []
        for _ in range(steady_n):
            t1 = time.perf_counter()
            self.one_step()
            steady.append(time.perf_counter() - t1)
        self.steady_ms = 1e3 * float(np.median(steady[len(steady) // 2:])) if steady else None
        self.res = eng.unpack(self.host_np.copy())
        assert np.isfinite(self.res.loglik)
        # sanity of the reduced statistics: every step of every rank carries unit gamma mass
        total = rk.world * self.Kloc * self.wl.T
        np.testing.assert_allclose(self.res.state_counts.sum(), total, rtol=1e-9)
        np.testing.assert_allclose(self.res.C.sum(), total - rk.world * self.Kloc, rtol=1e-9)
        return self

    def logL_k(self):
        """Per-trajectory log-likelihoods of this rank's shard (one more E-step)."""
        m = self.wl.margs
        if not self.rk.distributed:
            return self.eng.estep(m[0], m[1], m[2], m[3]).logL_k
        self.eng.estep_launch(m[0], m[1], m[2], m[3], stats_dev=self.stats.data_ptr())
        return self.eng.estep_fetch_logL()

    def collective_ms(self, reps=20):
        """The all-reduce + copy of the packed statistics alone."""
        rk = self.rk
        if not rk.distributed:
            return None
        rk.fence()
        t0 = time.perf_counter()
        for _ in range(reps):
            rk.sum_stats(self.stats)
        return 1e3 * (time.perf_counter() - t0) / reps

    def close(self):
        self.eng.close()
        self.obs = self.stats = None
        self.rk.torch.cuda.empty_cache()


def load_traffic(args, key):
    """Offline PMC figures of one workload's sweep launches (profiles/traffic_current.json, written
    by tools/profile_r05.sh): HBM bytes per launch pair (separate FETCH_SIZE / WRITE_SIZE passes, the
    gfx950 correction of MI355X_MICROARCH.md applied) and SQ_INSTS_VALU.  Not re-measured by this run."""
    tj = args.traffic_json if os.path.isabs(args.traffic_json) else os.path.join(ROOT, args.traffic_json)
    if not os.path.exists(tj):
        return None
    tdoc = json.load(open(tj))
    ent = tdoc.get("workloads", {}).get(key)
    if ent is None and key == "configs1" and "traffic_bytes_per_launch" in tdoc:
        ent = tdoc                                    # (the rounds 1-4 layout: configs[1] at top level)
    if ent is None:
        return None
    ent = dict(ent)
    ent["file"] = "%s (%s)" % (args.traffic_json, ent.get("source", tdoc.get("source", "source not recorded")))
    return ent


def live_traffic(K, T, timeout=150.0):
    """roofline.traffic measured by THIS run (N = 1 only): two child processes, `rocprofv3 --pmc FETCH_SIZE` and
    `--pmc WRITE_SIZE` (separate passes, MI355X_MICROARCH.md section HBM) over tools/pmc_r05.py --only-configs2 K T --
    this run's workload drawn and run exactly as above, plus the guide's 1 GiB calibration copy.  Bytes =
    1024 (2 FETCH_SIZE + WRITE_SIZE) of the two sweep launches of one E-step (mean of the last three E-steps);
    the factor 2 is checked on the copy.  Returns None when rocprofv3 is not there, a pass fails or runs out of
    time -- the offline figures of profiles/traffic_current.json stay in the line then."""
    import collections
    import csv
    import glob
    import shutil
    import signal
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe) or os.environ.get("ROCP_TOOL_LIBRARIES") or "rocprof" in os.environ.get("LD_PRELOAD", ""):
        return None
    vals = {}
    t_all = time.perf_counter()
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="bhmm_pmc_", dir="/tmp")
        cmd = [exe, "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.join(ROOT, "tools", "pmc_r05.py"), "--only-configs2", str(K), str(T)]
        try:
            p = subprocess.Popen(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL,
                                 stderr=subprocess.DEVNULL, start_new_session=True)
            try:
                rc = p.wait(timeout)
            except subprocess.TimeoutExpired:
                os.killpg(p.pid, signal.SIGKILL)
                p.wait()
                return None
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if rc != 0 or not files:
                return None
            per = collections.defaultdict(list)
            for r in csv.DictReader(open(files[0])):
                if r["Counter_Name"] == ctr:
                    per[r["Kernel_Name"]].append(float(r["Counter_Value"]))
            vals[ctr] = {k: sum(v[-3:]) / len(v[-3:]) for k, v in per.items()}
        except Exception:
            return None
        finally:
            shutil.rmtree(d, ignore_errors=True)

    def pick(ctr, a, b):
        hit = [v for k, v in vals[ctr].items() if a in k and b in k]
        return hit[0] if hit else None
    kb = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        p1 = pick(ctr, "k_estep_light<8, 1, true", ", 2>")
        p2 = pick(ctr, "k_estep<8, 1, true", ", 3>")
        cp = pick(ctr, "opyBuffer", "")
        if p1 is None or p2 is None:
            return None
        kb[ctr] = (p1, p2, cp)
    traffic = 1024.0 * (2.0 * (kb["FETCH_SIZE"][0] + kb["FETCH_SIZE"][1]) + kb["WRITE_SIZE"][0] + kb["WRITE_SIZE"][1])
    # third pass: vector instructions and the shader clock of the two sweep launches (for issue_frac); optional
    issue = None
    d = tempfile.mkdtemp(prefix="bhmm_pmc_", dir="/tmp")
    try:
        cmd = [exe, "--pmc", "GRBM_GUI_ACTIVE", "SQ_INSTS_VALU", "--kernel-trace", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.join(ROOT, "tools", "pmc_r05.py"), "--only-configs2", str(K), str(T)]
        p = subprocess.Popen(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL,
                             stderr=subprocess.DEVNULL, start_new_session=True)
        try:
            rc = p.wait(timeout)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)
            p.wait()
            rc = -1
        cf = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
        kf = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if rc == 0 and cf and kf:
            dur = {r["Dispatch_Id"]: int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in csv.DictReader(open(kf[0]))}
            rows = collections.defaultdict(dict)
            names = {}
            for r in csv.DictReader(open(cf[0])):
                rows[r["Dispatch_Id"]][r["Counter_Name"]] = float(r["Counter_Value"])
                names[r["Dispatch_Id"]] = r["Kernel_Name"]
            ph = {}
            for key, a, b in (("P1", "k_estep_light<8, 1, true", ", 2>"), ("P2", "k_estep<8, 1, true", ", 3>")):
                ds = [i for i, nm in names.items() if a in nm and b in nm and i in dur][-3:]
                if ds:
                    ns = sum(dur[i] for i in ds) / len(ds)
                    clk = sum(rows[i].get("GRBM_GUI_ACTIVE", 0.0) for i in ds) / len(ds) / ns
                    ph[key] = (sum(rows[i].get("SQ_INSTS_VALU", 0.0) for i in ds) / len(ds), clk / 8.0 if clk > 4.0 else clk, ns / 1e3)
            if len(ph) == 2 and min(ph["P1"][1], ph["P2"][1]) > 0.5:
                i1, i2 = ph["P1"][0], ph["P2"][0]
                issue = {"valu_wave_insts_per_launch": i1 + i2,
                         # one vector instruction per SIMD and four cycles at the clock the counters saw
                         "issue_ceiling_insts_per_us_per_simd": (i1 + i2) / (i1 / (250.0 * ph["P1"][1]) + i2 / (250.0 * ph["P2"][1])),
                         "under_counters": {"P1_us": ph["P1"][2], "P2_us": ph["P2"][2],
                                            "P1_clock_GHz": ph["P1"][1], "P2_clock_GHz": ph["P2"][1]}}
    except Exception:
        issue = None
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return {"traffic": traffic, "issue": issue,
            "source": "this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE (one pass each, child processes) over "
                      "tools/pmc_r05.py --only-configs2; bytes = 1024 (2 FETCH_SIZE + WRITE_SIZE), P1 + P2 of one E-step; "
                      "issue_frac from a third pass (GRBM_GUI_ACTIVE, SQ_INSTS_VALU) when it succeeds",
            "kb_per_launch": {"P1": {"FETCH_SIZE": kb["FETCH_SIZE"][0], "WRITE_SIZE": kb["WRITE_SIZE"][0]},
                              "P2": {"FETCH_SIZE": kb["FETCH_SIZE"][1], "WRITE_SIZE": kb["WRITE_SIZE"][1]}},
            "calibration_1GiB_copy_kb": {"FETCH_SIZE": kb["FETCH_SIZE"][2], "WRITE_SIZE": kb["WRITE_SIZE"][2],
                                         "expected": "FETCH 524288 (half of the bytes read), WRITE 1048576"},
            "seconds": time.perf_counter() - t_all}


def roofline_block(wl, ser, args, steps_per_s_per_gpu):
    """algorithmic bytes of this rank's launch pair over its duration by HIP events
    (recorded on the launch stream inside the library), against the 8 TB/s HBM peak."""
    Kloc, T, eng = ser.Kloc, wl.T, ser.eng
    sweep_ms = float(ser.kern_ms[2])
    alg = wl.b_alg * Kloc * T
    achieved = alg / (sweep_ms * 1e-3) / 1e9
    ent = load_traffic(args, wl.key)
    traffic = valu = rate = src = None
    if ent is not None and eng.get_option("spec_ok") > 0 and eng.get_option("spec_fail") == 0:
        shape = ent.get("shape")
        if shape is None or (int(shape[1]) == T and int(shape[0]) % Kloc == 0 and int(shape[0]) >= Kloc):
            # measured at N = 1 on the whole set; a shard of it moves that fraction of the bytes
            share = 1.0 if shape is None else Kloc / float(shape[0])
            traffic = ent["traffic_bytes_per_launch"] * share
            if ent.get("valu_wave_insts_per_launch"):
                valu = ent["valu_wave_insts_per_launch"] * share
            rate = ent.get("issue_ceiling_insts_per_us_per_simd")
            src = ent["file"] + ("" if share == 1.0 else " x %g (this rank's share of the trajectories)" % share)
    return {"bound": "hbm", "kernel": wl.kernel,
            "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic, "traffic_is_live": False,
            # the other ceilings, named: HBM bytes the counters saw / time / peak, and vector
            # instructions issued / what this part issues on 1024 SIMDs in that time
            "hbm_counter_frac": None if traffic is None else traffic / (sweep_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "issue_frac": None if not (valu and rate) else valu / (rate * 1024 * sweep_ms * 1e3),
            "traffic_source": src,
            "alg_bytes_per_launch": alg, "alg_bytes_per_timestep": wl.b_alg,
            "sweep_kernel_ms": sweep_ms, "per": "GPU (rank 0's two sweep launches of one E-step)",
            "whole_estep_frac": wl.b_alg * steps_per_s_per_gpu / 1e9 / HBM_PEAK_GBS}


def cpu_legs(wl, ser, ncpu, all_cores=True):
    """Rank 0: the reference's C kernels on `ncpu` of this rank's trajectories on one core, and (when
    the host has the memory: every thread materialises pobs, alpha, beta, gamma like the reference)
    on one OpenMP thread per core.  Asserts GPU/CPU parity of the log-likelihoods in the same run."""
    T, n = wl.T, wl.n
    ncpu = max(1, min(ncpu, ser.Kloc))
    m = wl.margs
    sample = ser.obs[: ncpu * T].cpu().numpy().reshape(ncpu, T)
    cb, ll = cpu_baseline(wl.kind, m[0], m[1], m[2], m[3], sample, threads=1)
    gpu_ll = ser.logL_k()[:ncpu]
    rel = float(np.max(np.abs((gpu_ll - np.array(ll)) / np.array(ll))))
    assert rel < 1e-9, "%s: GPU/CPU log-likelihood mismatch %g" % (wl.key, rel)
    cb["loglik_rel_diff_vs_gpu"] = rel
    nc = host_cores()
    if all_cores and nc > 1:
        per_thread = 4 * T * n * 8 + 64                  # bytes: pobs, alpha, beta, gamma (omp_driver.c)
        try:
            import psutil
            avail = psutil.virtual_memory().available
        except Exception:
            avail = 16 << 30
        threads = int(max(1, min(nc, ser.Kloc, (avail // 3) // per_thread)))
        if threads > 1:
            ktot = int(min(ser.Kloc, max(threads, min(ser.Kloc, int(2.5e8 // T)))))   # ~10-15 s of work
            big = ser.obs[: ktot * T].cpu().numpy().reshape(ktot, T)
            cba, lla = cpu_baseline(wl.kind, m[0], m[1], m[2], m[3], big, threads=threads)
            k = min(ncpu, ktot)
            assert np.allclose(lla[:k], ll[:k], rtol=1e-13)
            cb["all_cores"] = {k_: cba[k_] for k_ in ("value", "unit", "cores", "sample")}
    return cb


def secondary_whole_iterations(rk, model, args):
    """What a user of the estimator classes pays per iteration, host side included: whole EM
    iterations (MaximumLikelihoodEstimator.em_step: E-step + all-reduce + native M-step,
    maximum_likelihood.py:383-399) and whole Gibbs sweeps (BayesianHMMSampler.sample: sharded path
    step + all-reduce + parameter draws + model update + the per-sample model copy,
    bayesian_sampling.py:206-281) on the configs[1] / configs[4] shape.  Every rank holds the same
    global set of trajectories (drawn on the device by global index) and the classes shard it."""
    import bhmm_amd
    from bhmm_amd.engine import synth_observations
    from bhmm_amd.estimators import _tmatrix
    torch, dev, local = rk.torch, rk.dev, rk.local
    n, K, T = NSTATES, args.c1_ntraj, args.c1_length
    buf = torch.empty(K * T, dtype=torch.float64, device=dev)
    synth_observations("gaussian", buf.data_ptr(), model["A"], model["pi"], model["mu"],
                       model["sigma"], K, T, seed=2000, device=local, first_traj=0)
    host = buf.cpu().numpy().reshape(K, T)
    del buf
    torch.cuda.empty_cache()
    obs = [host[k] for k in range(K)]
    pi, A_eval = model["pi"], model["A_eval"]
    A_rev = _tmatrix.mle_reversible(pi[:, None] * A_eval, maxerr=1e-14)   # a reversible start
    res = []
    for rev in (True, False):
        init = bhmm_amd.gaussian_hmm(pi, A_rev if rev else A_eval, model["mu_eval"], model["sigma"])
        est = bhmm_amd.MaximumLikelihoodEstimator(obs, n, initial_model=init, reversible=rev,
                                                  device=local)
        for _ in range(max(5, args.em_iterations)):      # (also brings the GPU out of its idle clocks)
            est.em_step()
        rk.fence()
        lls, sweep_ms, carried = [], [], []
        eng = est._engine
        t0 = time.perf_counter()
        for _ in range(args.em_iterations):
            lls.append(est.em_step())
            if est.local_trajectories and hasattr(eng, "kernel_ms"):
                sweep_ms.append(eng.kernel_ms(2))
                carried.append(int(eng.get_option("carry_W")))
        rk.fence()
        dt = rk.max_over_ranks(time.perf_counter() - t0) / args.em_iterations
        assert np.all(np.diff(lls) > -1e-6 * abs(lls[0])), "EM log-likelihood decreased"
        res.append({"config": "configs[1] shape, WHOLE EM iteration (E-step%s + native M-step, model "
                              "updated every iteration), %s transition matrix, %d x %d over %d GPU(s)"
                              % (" + all-reduce" if rk.distributed else "",
                                 "reversible" if rev else "non-reversible", K, T, rk.world),
                    "n_gpus": rk.world, "ms_per_iteration": 1e3 * dt,
                    "timesteps_per_s": K * T / dt, "iterations": args.em_iterations,
                    "loglik_first_last": [lls[0], lls[-1]],
                    "sweep_kernel_ms_mean": float(np.mean(sweep_ms)) if sweep_ms else None,
                    "warmup_steps_used": {"full": eng.get_option("spec_W"),
                                          "carried_min_median_max": [int(np.min(carried)),
                                                                     int(np.median(carried)),
                                                                     int(np.max(carried))],
                                          "note": "0 = full warm-up from the uniform vector; > 0 = "
                                                  "warm-up of that many steps from the previous "
                                                  "E-step's boundary vectors (verified like every "
                                                  "warm-up)"} if carried else None,
                    "spec": {k: eng.get_option(k) for k in ("spec_W", "spec_ok", "spec_fail",
                                                            "carry_ok", "carry_fail")}
                    if hasattr(eng, "get_option") and est.local_trajectories else None})
        eng.close()
        del est
    for rev, nsteps in ((False, 1000), (True, 1000), (True, 30)):
        init = bhmm_amd.gaussian_hmm(pi, A_rev if rev else A_eval, model["mu_eval"], model["sigma"])
        smp = bhmm_amd.BayesianHMMSampler(obs, n, initial_model=init, reversible=rev,
                                          transition_matrix_sampling_steps=nsteps, device=local)
        smp.sample(max(3, args.chain_sweeps), seed=1)
        rk.fence()
        t0 = time.perf_counter()
        models = smp.sample(args.chain_sweeps)
        rk.fence()
        dt = rk.max_over_ranks(time.perf_counter() - t0) / args.chain_sweeps
        assert len(models) == args.chain_sweeps
        res.append({"config": "configs[4] chain, WHOLE Gibbs sweep (path step%s + parameter draws + "
                              "model update + model copy), %s, 8-state Gaussian, %d x %d over %d GPU(s)"
                              % (" + all-reduce" if rk.distributed else "",
                                 ("reversible, %d full sweeps of the transition-matrix sampler per "
                                  "Gibbs sweep%s" % (nsteps, " (the reference's default)"
                                                     if nsteps == 1000 else "")) if rev
                                 else "non-reversible (Dirichlet rows)", K, T, rk.world),
                    "n_gpus": rk.world, "ms_per_sweep": 1e3 * dt, "timesteps_per_s": K * T / dt,
                    "sweeps": args.chain_sweeps, "samples_100_seconds": 100 * dt})
        smp._engine.close()
        del smp, models
    torch.cuda.empty_cache()
    return res


def projected_8gpu(torch, dev, local, stream, args, n1_ms, n1_secondary, model):
    """A PROJECTION of the 8-GPU job from ONE GPU -- not a measurement (the pool has one-GPU boxes; RCCL has
    never run with more than one rank here).  What rank 0 of an 8-rank job does is run for real: the shard of
    trajectories 0 .. K/8 - 1 of the SAME global set (drawn by global index), through the distributed code path
    -- statistics into the device buffer, RCCL all-reduce (one rank: the call, its launch and its
    synchronisation, not the xGMI hops), one copy to the host -- and timed with the contract's protocol.  The
    8-rank all-reduce of 4.7 KB over xGMI is latency-bound; what it adds to the 1-rank call is NOT in here.
    The distributed form of the host sums at maximum_likelihood.py:271-282."""
    import copy
    import socket
    import torch.distributed as dist
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    out = {"what": "projection from one GPU, not a measurement: rank 0's shard of an 8-rank job run for real "
                   "(1/8 of the trajectories, drawn by global index) with a ONE-rank RCCL all-reduce and the "
                   "copy to the host inside every step; the latency of the 8-rank all-reduce over xGMI is not in it"}
    try:
        rk1 = Ranks(torch, dist, 1, 0, local, dev, "nccl", True, stream)
        wl = workload_configs2(args.ntraj, args.length)
        Ksh = max(1, args.ntraj // 8)
        ser = Series(rk1, wl, Ksh, 0, chunk=args.chunk)
        ser.run(args.warmup, args.steps, 0)
        shard_ms = 1e3 * ser.elapsed / args.steps
        coll_ms = ser.collective_ms()
        out.update({"shard": "%d traj x %d steps (of %d), chunks %d of %d steps, warm-up %d"
                             % (Ksh, wl.T, args.ntraj, ser.eng.num_chunks, ser.eng.chunk_len,
                                int(ser.eng.get_option("spec_W"))),
                    "shard_ms": shard_ms, "shard_kernels_ms": float(ser.kern_ms[4]),
                    "allreduce_plus_copy_ms": coll_ms,
                    "host_gap_ms": shard_ms - float(ser.kern_ms[4]),
                    "n1_ms_per_step": n1_ms,
                    "projected_speedup_vs_n1": n1_ms / shard_ms,
                    "projected_value_timesteps_per_s": args.ntraj * wl.T / (1e-3 * shard_ms),
                    "roofline_frac_of_the_shard": wl.b_alg * Ksh * wl.T / (1e-3 * float(ser.kern_ms[2])) / 1e9
                                                  / HBM_PEAK_GBS})
        ser.close()
        del ser
        if n1_secondary is not None:
            # whole EM iterations / Gibbs sweeps (configs[4] chain): 1/8 of the trajectories through the sharded
            # estimator classes, collectives forced on
            os.environ["BHMM_AMD_FORCE_COMM"] = "1"
            a8 = copy.copy(args)
            a8.c1_ntraj = max(1, args.c1_ntraj // 8)
            sh = secondary_whole_iterations(rk1, model, a8)
            del os.environ["BHMM_AMD_FORCE_COMM"]
            rows = []
            for full, part in zip(n1_secondary, sh):
                key = "ms_per_sweep" if "ms_per_sweep" in part else "ms_per_iteration"
                rows.append({"config": full["config"].split(", 8-state")[0].split(", %d x" % args.c1_ntraj)[0],
                             "n1_ms": full[key], "shard_ms": part[key],
                             "projected_speedup_vs_n1": full[key] / part[key]})
            out["whole_iterations_and_sweeps"] = rows
    finally:
        dist.destroy_process_group()
    return out


def draw_watch_rates(eng, sweep, nsweeps):
    """Over `nsweeps` path steps with different seeds: how many draws fell within 64 x the deviation the
    boundary check of the forward pass measured (csrc/draw_verify.hpp), how many of them were decided again on
    the windowed serial recursion, how many calls were repeated on the exact alpha rows."""
    ev = ck = rd = 0
    dev = 0.0
    for sd in range(nsweeps):
        sweep(1000 + sd)
        ev += int(eng.get_option("draw_events"))
        ck += int(eng.get_option("draw_checked"))
        rd += int(eng.get_option("draw_redone"))
        dev = max(dev, eng.get_option("draw_alpha_dev"))
    return {"sweeps": nsweeps, "watched": ev, "decided_again": ck, "calls_repeated_on_exact_rows": rd,
            "largest_boundary_deviation": dev}


def secondary_c2_paths(torch, dev, local, eng, model, K, T, args):
    """Viterbi (bit-exact, one byte per step, device-resident result) and the Gibbs hidden-path
    sweep on the headline workload's engine (configs[1] shape; configs[4] is this sweep x 100)."""
    margs = (model["A_eval"], model["pi"], model["mu_eval"], model["sigma"])
    res = []
    pdev = torch.empty(K * T, dtype=torch.uint8, device=dev)
    t0 = time.perf_counter()
    eng.viterbi_u8(*margs, out=pdev)
    eng.sync()
    first_ms = 1e3 * (time.perf_counter() - t0)       # (the E-step's warm-up length; what a single call after EM pays)
    for _ in range(8):                                # the pass searches its own, shorter warm-up over the next calls
        eng.viterbi_u8(*margs, out=pdev)
    dt = timeit(lambda: eng.viterbi_u8(*margs, out=pdev), 2, eng.sync, batches=5)
    ppin = torch.empty(K * T, dtype=torch.uint8).pin_memory()
    dth = timeit(lambda: eng.viterbi_u8(*margs, out=ppin), 2, eng.sync, batches=5)
    assert torch.equal(pdev.cpu(), ppin)
    b_alg = 8 + 2 * 4 * 8 + 4       # obs + int32 back-pointers written and read + path
    res.append({"config": "Viterbi at the configs[1] shape (8-state Gaussian, %d x %d), paths as "
                          "uint8" % (K, T),
                "ms_device_result": 1e3 * dt, "ms_pinned_host_result": 1e3 * dth, "ms_first_call": first_ms,
                "warmup_steps": {"settled": eng.get_option("viterbi_W"), "e_step": eng.get_option("spec_W")},
                "timesteps_per_s": K * T / dt, "chunked": eng.get_option("viterbi_chunked"),
                "roofline": {"bound": "hbm", "alg_bytes_per_timestep": b_alg,
                             "frac": b_alg * K * T / dt / 1e9 / HBM_PEAK_GBS}})
    sbuf = torch.zeros(eng.path_stats_size, dtype=torch.float64, device=dev)
    dt = timeit(lambda: eng.sample_paths_dev(*margs, sbuf.data_ptr(), seed=1), 5, eng.sync, batches=5)
    C, n0, _ = eng.unpack_path_stats(sbuf.cpu().numpy())
    assert C.sum() == K * (T - 1) and n0.sum() == K
    watch = draw_watch_rates(eng, lambda sd: eng.sample_paths_dev(*margs, sbuf.data_ptr(), seed=sd), 100)
    b_alg = 2 * 8 + 16 * 8 + 4                           # Gibbs path sweep
    res.append({"config": "configs[4] sweep: Gibbs hidden-path step (forward + backward sampling + "
                          "path statistics), 8-state Gaussian, %d x %d, one GPU" % (K, T),
                "ms": 1e3 * dt, "timesteps_per_s": K * T / dt,
                "path_steps_100_seconds": 100 * dt,
                "note": "the hidden-path step alone; the whole sweep incl. parameter draws is the "
                        "'WHOLE Gibbs sweep' entries below",
                "draws_next_to_a_cumulative_sum_edge": watch,
                "roofline": {"bound": "hbm", "alg_bytes_per_timestep": b_alg,
                             "frac": b_alg * K * T / dt / 1e9 / HBM_PEAK_GBS}})
    return res


def secondary_c4(torch, dev, local, args):
    """configs[3]: 64-state Gaussian, 128 x 1e5 (fp64-throughput bound)."""
    from bhmm_amd.engine import Engine, synth_observations
    rng = np.random.default_rng(64)
    n, K, T = 64, 128, 100000
    A = metastable_matrix(n, rng)
    pi = stationary(A)
    mu, sig = np.linspace(-5, 5, n), np.linspace(0.5, 2.0, n)
    obs = torch.empty(K * T, dtype=torch.float64, device=dev)
    synth_observations("gaussian", obs.data_ptr(), A, pi, mu, sig, K, T, seed=6400, device=local)
    eng = Engine(local)
    eng.set_observations_device("gaussian", obs.data_ptr(), np.arange(K + 1, dtype=np.int64) * T, n)
    margs = (0.9 * A + 0.1 / n, pi, mu + 0.05, sig)
    for _ in range(3):                 # lets the segment plan settle on a warm-up that verifies
        eng.estep(*margs)
    dt = timeit(lambda: eng.estep(*margs), 3, eng.sync)
    r = eng.estep(*margs)
    np.testing.assert_allclose(r.state_counts.sum(), K * T, rtol=1e-9)
    flops = 2.0 * 3 * n * n                              # forward, backward, xi: n*n FMAs each
    out = {"config": "configs[3]: 64-state Gaussian HMM, %d x %d, one full E-step" % (K, T),
           "ms": 1e3 * dt, "timesteps_per_s": K * T / dt,
           "roofline": {"bound": "fp64", "alg_flop_per_timestep": flops,
                        "achieved": flops * K * T / dt / 1e12, "peak": 78.6, "unit": "TFLOP/s",
                        "frac": flops * K * T / dt / 1e12 / 78.6},
           "segments": eng.get_option("wide_segments"),
           "kernels": "k_tile_fwd / k_tile_bwd (row-batched v_mfma_f64_16x16x4, 16 segments per workgroup)"
                      if eng.get_option("tile") else "k_wide_fwd / k_wide_bwd (one segment per wavefront)",
           "kernel_ms": {"forward": eng.kernel_ms(0), "backward_and_statistics": eng.kernel_ms(2)},
           "self_checks_fired": int(eng.get_option("wide_trouble")),
           "spec": {k: eng.get_option(k) for k in ("spec_W", "spec_ok", "spec_fail", "spec_last_dev")}}
    # the other two passes of the path on this shape: both run over time segments (round 4) and are
    # exact by construction: Viterbi is accepted only with bitwise-identical boundary vectors; the draw is the
    # serial draw GIVEN its alpha rows, which come from the segmented forward pass verified to 1e-11
    pdev = torch.empty(K * T, dtype=torch.uint8, device=dev)
    for _ in range(5):                 # (the Viterbi pass searches its own warm-up over the first calls)
        eng.viterbi_u8(*margs, out=pdev)
    dv = timeit(lambda: eng.viterbi_u8(*margs, out=pdev), 3, eng.sync)
    out["viterbi"] = {"ms": 1e3 * dv, "timesteps_per_s": K * T / dv,
                      "over_time_segments": bool(eng.get_option("viterbi_chunked")),
                      "segments": eng.get_option("viterbi_segments"), "warmup": eng.get_option("viterbi_W"),
                      "boundaries_not_bit_identical_after_first_pass": eng.get_option("viterbi_mismatch"),
                      "boundaries_further_than_1e-12": eng.get_option("viterbi_far"),
                      "fixup_rounds": eng.get_option("viterbi_rounds"),
                      "accepted_by_path_margins": bool(eng.get_option("viterbi_margin_used")),
                      "close_decisions_on_the_path": eng.get_option("viterbi_margin_close"),
                      "note": "paths as one byte per step into a device buffer"}
    for _ in range(3):
        eng.sample_paths(*margs, seed=1, want_paths=False)
    dg = timeit(lambda: eng.sample_paths(*margs, seed=1, want_paths=False), 3, eng.sync)
    out["gibbs_path_step"] = {"ms": 1e3 * dg, "timesteps_per_s": K * T / dg,
                              "over_time_segments": bool(eng.get_option("sample_segmented")),
                              "forward_pass_segmented": bool(eng.get_option("sample_forward_segmented")),
                              "segments": eng.get_option("sample_segments"), "warmup": eng.get_option("sample_W"),
                              "segments_drawn_again": eng.get_option("sample_mismatch"),
                              "fixup_rounds": eng.get_option("sample_rounds"),
                              "note": "forward filter + backward draw + path statistics, counts on the device"}
    out["gibbs_path_step"]["draws_next_to_a_cumulative_sum_edge"] = draw_watch_rates(
        eng, lambda sd: eng.sample_paths(*margs, seed=sd, want_paths=False), 20)
    eng.close()
    # whole EM iterations on this shape (E-step + native M-step, the model changes every iteration)
    import bhmm_amd
    host = obs.cpu().numpy().reshape(K, T)
    init = bhmm_amd.gaussian_hmm(pi, margs[0], margs[2], sig)
    est = bhmm_amd.MaximumLikelihoodEstimator([host[k] for k in range(K)], n, initial_model=init,
                                              reversible=False, device=local)
    for _ in range(4):
        est.em_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    iters = 8
    lls = [est.em_step() for _ in range(iters)]
    torch.cuda.synchronize()
    de = (time.perf_counter() - t0) / iters
    e2 = est._engine
    out["whole_em_iteration"] = {"ms": 1e3 * de, "timesteps_per_s": K * T / de, "iterations": iters,
                                 "loglik_first_last": [lls[0], lls[-1]],
                                 "tile_kernels": bool(e2.get_option("tile")),
                                 "spec": {k: e2.get_option(k) for k in ("spec_W", "spec_ok", "spec_fail")},
                                 "note": "MaximumLikelihoodEstimator.em_step, non-reversible, host side included"}
    e2.close()
    del est
    return out


def secondary_gen(torch, dev, local, args):
    """More than 64 states (the any-N family): E-step on the row-batched matrix-core kernels -- up to 128
    states with A's blocks in registers (csrc/tile_gen.hip), 129 .. 512 with A streamed from L2
    (csrc/big_kernels.hpp, round 5)."""
    from bhmm_amd.engine import Engine
    out = []
    for n, K, T in ((65, 128, 10000), (128, 128, 10000), (256, 128, 4000)):
        rng = np.random.default_rng(n)
        A = metastable_matrix(n, rng)
        pi = stationary(A)
        mu, sig = np.linspace(-5, 5, n), np.linspace(0.5, 2.0, n)
        g = torch.Generator(device=dev)
        g.manual_seed(n)
        obs = torch.randn(K * T, dtype=torch.float64, device=dev, generator=g) * 3.0
        eng = Engine(local)
        eng.set_observations_device("gaussian", obs.data_ptr(), np.arange(K + 1, dtype=np.int64) * T, n)
        margs = (0.9 * A + 0.1 / n, pi, mu + 0.05, sig)
        for _ in range(3):
            eng.estep(*margs)
        dt = timeit(lambda: eng.estep(*margs), 3, eng.sync)
        r = eng.estep(*margs)
        np.testing.assert_allclose(r.state_counts.sum(), K * T, rtol=1e-9)
        flops = 2.0 * 3 * n * n
        out.append({"config": "%d-state Gaussian HMM, %d x %d, one full E-step" % (n, K, T),
                    "ms": 1e3 * dt, "timesteps_per_s": K * T / dt,
                    "roofline": {"bound": "fp64", "achieved": flops * K * T / dt / 1e12, "peak": 78.6,
                                 "unit": "TFLOP/s", "frac": flops * K * T / dt / 1e12 / 78.6},
                    "tile_kernels": bool(eng.get_option("tile")), "segments": eng.get_option("wide_segments"),
                    "self_checks_fired": int(eng.get_option("wide_trouble")),
                    "tile_reason": int(eng.get_option("tile_reason")),
                    "spec": {k: eng.get_option(k) for k in ("spec_W", "spec_ok", "spec_fail", "spec_last_dev")}})
        pdev = torch.empty(K * T, dtype=torch.uint8, device=dev)
        eng.viterbi_u8(*margs, out=pdev)
        dv = timeit(lambda: eng.viterbi_u8(*margs, out=pdev), 2, eng.sync)
        eng.sample_paths(*margs, seed=1, want_paths=False)
        dg = timeit(lambda: eng.sample_paths(*margs, seed=1, want_paths=False), 2, eng.sync)
        out[-1]["viterbi"] = {"ms": 1e3 * dv, "over_time_segments": bool(eng.get_option("viterbi_chunked")),
                              "segments": eng.get_option("viterbi_segments"), "warmup": eng.get_option("viterbi_W"),
                              "fixup_rounds": eng.get_option("viterbi_rounds"),
                              "accepted_by_path_margins": bool(eng.get_option("viterbi_margin_used"))}
        out[-1]["gibbs_path_step"] = {"ms": 1e3 * dg, "over_time_segments": bool(eng.get_option("sample_segmented")),
                                      "forward_pass_segmented": bool(eng.get_option("sample_forward_segmented")),
                                      "fixup_rounds": eng.get_option("sample_rounds")}
        eng.close()
        del obs, pdev
    return out


# ---------------------------------------------------------------------------------------
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--ntraj", type=int, default=1024, help="trajectories of the headline workload, IN TOTAL")
    ap.add_argument("--length", type=int, default=1000000)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also the steady-state window, the CPU baselines, the live counter "
                         "passes, the other configurations and the 8-GPU projection (several minutes); the "
                         "--no-* options below take parts out of it")
    ap.add_argument("--cpu-traj", type=int, default=48,
                    help="trajectories in the 1-core CPU baseline of the headline (~10 s at 1e6 steps each)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-secondary", action="store_true")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="keep the offline counter figures (profiles/traffic_current.json) instead of two rocprofv3 "
                         "--pmc passes in child processes (N = 1 only, about half a minute)")
    ap.add_argument("--no-steady", action="store_true",
                    help="skip the extra steady-state window (profiling runs: the kernel statistics then "
                         "cover exactly the warm-up and timed launches)")
    ap.add_argument("--c1-ntraj", type=int, default=256, help="configs[1] (N = 1 secondary): trajectories")
    ap.add_argument("--c1-length", type=int, default=100000)
    ap.add_argument("--c1-steps", type=int, default=200)
    ap.add_argument("--c1-warmup", type=int, default=50)
    ap.add_argument("--c1-cpu-traj", type=int, default=100)
    ap.add_argument("--traffic-json", default="profiles/traffic_current.json",
                    help="offline PMC measurements quoted as roofline.traffic (tools/profile_r05.sh)")
    ap.add_argument("--chain-sweeps", type=int, default=20, help="Gibbs sweeps timed per chain variant")
    ap.add_argument("--em-iterations", type=int, default=30, help="whole EM iterations timed")
    ap.add_argument("--no-projection", action="store_true", help="skip the labelled 8-GPU projection (N = 1 only)")
    ap.add_argument("--only", default="", help="profiling aid: 'c3' runs the configs[3] block alone (E-step, "
                                               "Viterbi, Gibbs path step -- exactly the calls of the full run), 'shard' the "
                                               "E-step part of the 8-GPU projection, and prints it")
    ap.add_argument("--oversubscribe", action="store_true",
                    help="TEST AID for boxes with fewer GPUs than ranks: ranks share GPUs "
                         "(local rank modulo device count) and the all-reduce runs over gloo")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write the reduced statistics of the last one (configs[2]) as "
                         "DIR/<field>.npy, float64 (rank 0; not with --only)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    launched = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    if args.gpus > 1 and not launched:
        # never exec / re-exec from a process that touched the GPU: this parent has not
        sys.exit(self_launch(args, sys.argv[1:]))

    result = OnlyTheResultOnStdout()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, "--gpus %d but WORLD_SIZE=%d" % (args.gpus, world)
    distributed = launched

    K, T = args.ntraj, args.length
    assert K % world == 0, "%d trajectories do not split evenly over %d ranks" % (K, world)
    Kloc = K // world

    import torch
    import torch.distributed as dist

    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    ndev = torch.cuda.device_count()
    if args.oversubscribe:
        local = local % max(ndev, 1)
    assert local < ndev, "rank %d wants GPU %d but only %d visible" % (rank, local, ndev)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    backend = "gloo" if args.oversubscribe else "nccl"
    if distributed:
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    rk = Ranks(torch, dist, world, rank, local, dev, backend, distributed, stream)

    if args.only == "c3":
        result.emit(json.dumps({"configs3_64_states": secondary_c4(torch, dev, local, args)}))
        return
    if args.only == "gen":
        result.emit(json.dumps({"more_than_64_states": secondary_gen(torch, dev, local, args)}))
        return
    if args.only == "shard":   # the E-step part of the 8-GPU projection alone (rank 0's shard, 1-rank RCCL all-reduce)
        result.emit(json.dumps({"projected_8gpu": projected_8gpu(torch, dev, local, stream, args, float("nan"), None, None)}))
        return

    # ---- the headline: configs[2], strong-scaled --------------------------------------------------
    # (the CPU legs run AFTER the GPU timing: tens of seconds of host work between drawing the data
    # and the timed loop would let the GPU fall back to its idle clocks right before the warm-up steps)
    wl = workload_configs2(K, T)
    ser = Series(rk, wl, Kloc, rank * Kloc, chunk=args.chunk)
    ser.run(args.warmup, args.steps, 40 if args.full and not args.no_steady else 0)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ser.eng.unpack(ser.last_timed))
    elapsed = ser.elapsed
    res = ser.res
    want = C2_LOGLIK_N1.get((K, T))
    if want is not None:
        assert abs(res.loglik - want) <= 1e-12 * abs(want), \
            "configs[2]: log-likelihood %r differs from the committed N = 1 value %r" % (res.loglik, want)
    # every rank must hold the same reduced statistics (one all-reduce, nothing rank-dependent after it)
    same = True
    if distributed:
        mine = torch.from_numpy(ser.host_np.copy())
        if backend == "nccl":
            mine = mine.to(dev)
        lo, hi = mine.clone(), mine.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        same = bool(torch.equal(lo, hi))
        assert same, "the ranks hold different reduced statistics"
    coll_ms = ser.collective_ms() if args.full else None
    cb = None
    if args.full and not args.no_cpu:
        if rank == 0:
            # at N > 1 a smaller sample: the other ranks wait at the next barrier meanwhile
            cb = cpu_legs(wl, ser, args.cpu_traj if world == 1 else min(args.cpu_traj, 8), all_cores=(world == 1))
        rk.fence()

    out = None
    if rank == 0:
        value = K * T * args.steps / elapsed
        eng = ser.eng
        out = {
            "metric": "timesteps/sec forward-backward (whole node), N=8 states",
            "value": value, "unit": "timesteps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
            "steady_state_ms": ser.steady_ms,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": "%s in total, %d per GPU, one full E-step" % (wl.name, Kloc),
                       "trajectories_total": K, "trajectories_per_gpu": Kloc, "timesteps_per_trajectory": T,
                       "first_trajectory_of_rank": "rank r holds trajectories r*%d .. (r+1)*%d-1 of ONE global set" % (Kloc, Kloc),
                       "symbols": wl.M, "chunk_len": eng.chunk_len, "chunks": eng.num_chunks,
                       "speculative_boundaries": {k: eng.get_option(k) for k in
                                                  ("spec_enabled", "spec_W", "spec_ok", "spec_fail",
                                                   "spec_last_dev", "careful")},
                       "collective": ("RCCL all-reduce" if backend == "nccl" else
                                      "gloo all-reduce (--oversubscribe test aid: ranks share GPUs)")
                                     if distributed else "none (one process)",
                       "allreduces_per_step": ser.allreduces_per_step,
                       "parallelism": "trajectories sharded over %d GPU(s), all-reduce of "
                                      "%d statistics" % (world, ser.S)},
            "roofline": roofline_block(wl, ser, args, value / world),
            "kernel_ms": {KERNEL_NAMES[i]: float(ser.kern_ms[i]) for i in range(5)},
            "dominant_kernel": KERNEL_NAMES[int(np.argmax(ser.kern_ms[:4]))],
            "loglik": res.loglik, "loglik_matches_n1": None if want is None else True,
            "statistics_identical_on_all_ranks": same if distributed else None,
            "allreduce_plus_copy_ms": coll_ms,
            "synth_seconds": ser.synth_seconds,
            "timing_note": "ms_per_step covers exactly the requested steps, max over ranks, between barriers; "
                           "steady_state_ms (--full) is the median of the last 20 steps of an extra 40-step window "
                           "right behind them (DESIGN.md section 7)",
        }
        if cb is not None:
            out["cpu_baseline"] = cb
            out["speedup_vs_1core"] = value / cb["value"]
            # the target is quoted on ONE GPU (BASELINE.json north_star): checked there, not a statement elsewhere
            out["target_50x_met"] = bool(out["speedup_vs_1core"] >= 50.0) if world == 1 else None
            if world == 1:
                assert out["target_50x_met"], "north-star target (>= 50x the reference CPU path) missed"
    ser.close()
    del ser

    if args.full and rank == 0 and world == 1 and out is not None and \
            not (args.no_live_traffic or args.no_secondary or args.only):
        # roofline.traffic of THIS run (the engine above is closed: its 20 GB are free for the child processes)
        lt = live_traffic(K, T)
        if lt is not None:
            rf = out["roofline"]
            rf["traffic_offline"] = {"traffic": rf["traffic"], "source": rf["traffic_source"]}
            rf["traffic"], rf["traffic_is_live"], rf["traffic_source"] = lt["traffic"], True, lt["source"]
            rf["hbm_counter_frac"] = lt["traffic"] / (rf["sweep_kernel_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
            rf["traffic_live_detail"] = {k: lt[k] for k in ("kb_per_launch", "calibration_1GiB_copy_kb", "seconds")}
            if lt.get("issue"):
                iss = lt["issue"]
                rf["issue_frac_offline"] = rf["issue_frac"]
                rf["issue_frac"] = iss["valu_wave_insts_per_launch"] / (iss["issue_ceiling_insts_per_us_per_simd"] * 1024 *
                                                                       rf["sweep_kernel_ms"] * 1e3)
                rf["traffic_live_detail"]["issue"] = iss

    if args.full and not args.no_secondary:
        # the secondary measurements run on ALL ranks (their collectives need everyone)
        sec = []
        c1 = c4 = gen = None
        model = make_c2_model()
        if world == 1:
            # configs[1]: the headline of rounds 1-4, same protocol, its own roofline and CPU figure
            w1 = workload_configs1(args.c1_ntraj, args.c1_length)
            s1 = Series(rk, w1, w1.K, 0)
            s1.run(args.c1_warmup, args.c1_steps, 0 if args.no_steady else 100)
            v1 = w1.K * w1.T * args.c1_steps / s1.elapsed
            c1 = {"config": w1.name + ", one full E-step, one GPU", "value": v1, "unit": "timesteps/s",
                  "steps": args.c1_steps, "warmup": args.c1_warmup, "ms_per_step": 1e3 * s1.elapsed / args.c1_steps,
                  "steady_state_ms": s1.steady_ms, "roofline": roofline_block(w1, s1, args, v1),
                  "kernel_ms": {KERNEL_NAMES[i]: float(s1.kern_ms[i]) for i in range(5)},
                  "chunk_len": s1.eng.chunk_len, "chunks": s1.eng.num_chunks,
                  "speculative_boundaries": {k: s1.eng.get_option(k) for k in
                                             ("spec_W", "spec_ok", "spec_fail", "spec_last_dev", "careful")},
                  "note": "the `value` of BENCH_r01..r04 (there with the driver's --warmup 5 --steps 20 "
                          "right after start-up: 0.96-1.02 ms)"}
            if not args.no_cpu:
                c1["cpu_baseline"] = cpu_legs(w1, s1, args.c1_cpu_traj)
                c1["speedup_vs_1core"] = v1 / c1["cpu_baseline"]["value"]
            sec = secondary_c2_paths(torch, dev, local, s1.eng, model, w1.K, w1.T, args)
            s1.close()
            del s1
            c4 = secondary_c4(torch, dev, local, args)
            sec.append(c4)
            gen = secondary_gen(torch, dev, local, args)
            sec.extend(gen)
        whole = secondary_whole_iterations(rk, model, args)
        sec.extend(whole)
        if out is not None and world == 1 and not args.no_projection:
            try:
                out["projected_8gpu"] = projected_8gpu(torch, dev, local, stream, args, out["ms_per_step"], whole, model)
            except Exception as e:      # (a box on which a one-rank RCCL communicator cannot be made: the line stands)
                out["projected_8gpu"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if out is not None:
            out["secondary"] = sec
            if c1 is not None:
                out["configs1_gaussian"] = c1
            if c4 is not None:
                out["configs3_64_states"] = {k: c4[k] for k in ("config", "ms", "timesteps_per_s", "roofline",
                                                                "kernels", "kernel_ms", "segments", "spec", "viterbi",
                                                                "gibbs_path_step", "whole_em_iteration",
                                                                "self_checks_fired") if k in c4}
            if gen:
                out["more_than_64_states"] = [{k: g[k] for k in ("config", "ms", "roofline", "tile_kernels", "self_checks_fired",
                                                                 "viterbi", "gibbs_path_step") if k in g}
                                              for g in gen]
    if distributed:
        dist.destroy_process_group()
    if out is not None:
        result.emit(json.dumps(out))


if __name__ == "__main__":
    main()
