"""Device-resident batch engine: the host-side handle of one `bhmm_ctx` (include/bhmm_amd.h).

One Engine holds a set of observation trajectories on one GPU (uploaded once -- they are
constant across EM iterations / Gibbs sweeps, maximum_likelihood.py:101) and runs the whole
per-iteration loop over trajectories of the reference
(maximum_likelihood.py:383-385, bayesian_sampling.py:288-290) as one call.
"""
import ctypes

import numpy as np

from . import _lib


class EStepResult(object):
    """Reduced sufficient statistics of one E-step (what maximum_likelihood.py:271-282 and the
    emission `estimate` methods consume)."""

    def __init__(self, kind, n, M, packed, logL_k, dimension=0, covariance_type=None):
        self.kind = kind
        self.packed = packed
        self.logL_k = logL_k
        o = 0
        self.loglik = float(packed[o]); o += 1
        self.gamma0_sum = packed[o:o + n].copy(); o += n
        self.C = packed[o:o + n * n].reshape(n, n).copy(); o += n * n
        self.state_counts = packed[o:o + n].copy(); o += n
        self.sum_gd = self.sum_gdd = self.symbol_counts = None
        if kind == 'gaussian':
            self.sum_gd = packed[o:o + n].copy(); o += n
            self.sum_gdd = packed[o:o + n].copy(); o += n
        elif kind == 'discrete':
            self.symbol_counts = packed[o:o + n * M].reshape(n, M).copy(); o += n * M
        # multivariate gaussian: the moments about the means of the E-step's model (bhmm_mvn_moments) -- S0 (n,),
        # S1 (n, D), S2 (n, D, D) symmetric or (n, D) -- and the packed block they came in
        self.moments = self.S0 = self.S1 = self.S2 = None
        if kind == 'mvgaussian':
            from .output_models.mvgaussian import moment_stride, unpack_moments
            size = n * moment_stride(dimension, covariance_type)
            self.moments = packed[o:o + size].copy(); o += size
            self.S0, self.S1, self.S2 = unpack_moments(self.moments, n, dimension, covariance_type)
        # gaussian mixture (M components per state): the per-component moments of bhmm_gmm_moments -- S0 (n, M), S1
        # (n, M, D), S2 (n, M, D, D) symmetric or (n, M, D)
        if kind == 'gaussian_mixture':
            from .output_models.gaussian_mixture import unpack_component_moments
            from .output_models.mvgaussian import moment_stride
            size = n * M * moment_stride(dimension, covariance_type)
            self.moments = packed[o:o + size].copy(); o += size
            self.S0, self.S1, self.S2 = unpack_component_moments(self.moments, n, M, dimension, covariance_type)
        # poisson counts: the moments of bhmm_mvn_moments with diagonal second moments about the rates of the
        # E-step's model -- S0 (n,), S1 (n, D); S2 (n, D) comes along and is not used by the M-step
        if kind == 'poisson':
            from .output_models.mvgaussian import moment_stride, unpack_moments
            size = n * moment_stride(dimension, 'diag')
            self.moments = packed[o:o + size].copy(); o += size
            self.S0, self.S1, self.S2 = unpack_moments(self.moments, n, dimension, 'diag')


class PathRuns(object):
    """Dwell segments (runs) of a decoded path (Engine.path_runs, Engine.decode_runs): a run is a maximal stretch
    of equal states inside one trajectory.  offsets (K + 1, int64): the runs of trajectory k are
    offsets[k]:offsets[k + 1] of start (int64, step index inside the trajectory), length (int64) and state (int32),
    which are concatenated over the trajectories; an empty trajectory has none.  With statistics, dwell is
    (nstates, 5) int64 -- per state the number of runs, the steps in them, the longest run, the runs that touch the
    first or the last step of their trajectory (censored) and the steps in those -- and jumps (nstates, nstates)
    int64 the number of adjacent run pairs i -> j inside one trajectory (zero diagonal); else both are None."""

    DWELL_COLUMNS = ('runs', 'steps', 'longest', 'censored_runs', 'censored_steps')

    def __init__(self, offsets, start, length, state, dwell=None, jumps=None):
        self.offsets = offsets
        self.start = start
        self.length = length
        self.state = state
        self.dwell = dwell
        self.jumps = jumps

    def __len__(self):
        return len(self.offsets) - 1

    @property
    def count(self):
        """Number of runs."""
        return int(self.offsets[-1])

    def trajectory(self, k):
        """(start, length, state) of the runs of trajectory k: three views."""
        K = len(self.offsets) - 1
        k = int(k)
        if not -K <= k < K:
            raise IndexError("trajectory %d of %d" % (k, K))
        k %= K
        a, b = int(self.offsets[k]), int(self.offsets[k + 1])
        return self.start[a:b], self.length[a:b], self.state[a:b]


_METHODS = {'viterbi': 0, 'posterior': 1}


_KINDS = {'gaussian': _lib.EMIT_GAUSSIAN, 'discrete': _lib.EMIT_DISCRETE,
          'explicit': _lib.EMIT_EXPLICIT}


class Engine(object):
    def __init__(self, device=0, stream=None):
        self._L = _lib.load()
        _lib.require_device()
        h = ctypes.c_void_p()
        _lib.check(self._L.bhmm_ctx_create(ctypes.byref(h), int(device),
                                           ctypes.c_void_p(stream) if stream else None))
        self._h = h
        self.device = int(device)
        self.kind = None
        self._stage = None
        self._keep = {}
        self._fetch = None
        self._kms = None
        self.nstates = 0
        self.nsymbols = 0
        self.lengths = None

    def close(self):
        if getattr(self, "_h", None):
            self._L.bhmm_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data ---------------------------------------------------------------------------
    def set_observations(self, kind, observations, nstates, nsymbols=0, chunk=0):
        """observations: list of 1-d arrays (gaussian: float, discrete: int) or, for kind
        'explicit', list of (T_k, nstates) pobs matrices."""
        code = _KINDS[kind]
        lengths = np.array([len(o) for o in observations], dtype=np.int64)
        off = np.zeros(len(observations) + 1, dtype=np.int64)
        off[1:] = np.cumsum(lengths)
        if kind == 'gaussian':
            flat = np.ascontiguousarray(np.concatenate([np.asarray(o, dtype=np.float64)
                                                        for o in observations]))
        elif kind == 'discrete':
            flat = np.ascontiguousarray(np.concatenate([np.asarray(o).astype(np.int32)
                                                        for o in observations]))
            if flat.size and (flat.min() < 0 or flat.max() >= nsymbols):
                raise ValueError("discrete observation outside [0, nsymbols)")
        else:
            flat = np.ascontiguousarray(np.concatenate(
                [np.asarray(o, dtype=np.float64).reshape(-1, nstates) for o in observations]))
        _lib.check(self._L.bhmm_ctx_set_observations(
            self._h, code, flat.ctypes.data_as(ctypes.c_void_p), _lib.lp(off), len(observations),
            int(nstates), int(nsymbols), int(chunk), 0))
        self._adopt(kind, nstates, nsymbols, lengths)

    def set_observations_lagged(self, kind, observations, lag, views, nstates, nsymbols=0, chunk=0):
        """Lagged views (bhmm/api.py:70-94) cut on the device: `observations` are the ORIGINAL
        trajectories (uploaded once), `views` a list of (trajectory index, shift); context
        trajectory v becomes observations[k][shift::lag]."""
        code = _KINDS[kind]
        lens = np.array([len(o) for o in observations], dtype=np.int64)
        off = np.zeros(len(observations) + 1, dtype=np.int64)
        off[1:] = np.cumsum(lens)
        if kind == 'gaussian':
            flat = np.ascontiguousarray(np.concatenate([np.asarray(o, dtype=np.float64)
                                                        for o in observations]))
        elif kind == 'discrete':
            flat = np.ascontiguousarray(np.concatenate([np.asarray(o).astype(np.int32)
                                                        for o in observations]))
            # only what the views touch has to be a symbol (stride > 1 skips shifts)
            for k, s in views:
                piece = np.asarray(observations[k])[int(s)::int(lag)]
                if piece.size and (piece.min() < 0 or piece.max() >= nsymbols):
                    raise ValueError("discrete observation outside [0, nsymbols)")
        else:
            flat = np.ascontiguousarray(np.concatenate(
                [np.asarray(o, dtype=np.float64).reshape(-1, nstates) for o in observations]))
        vt = np.ascontiguousarray([k for k, _ in views], dtype=np.int32)
        vs = np.ascontiguousarray([s for _, s in views], dtype=np.int32)
        _lib.check(self._L.bhmm_ctx_set_observations_lagged(
            self._h, code, flat.ctypes.data_as(ctypes.c_void_p), _lib.lp(off), len(observations),
            int(lag), _lib.ip(vt), _lib.ip(vs), len(views), int(nstates), int(nsymbols), int(chunk), 0))
        vlen = np.array([max(0, -(-(int(lens[k]) - int(s)) // int(lag))) for k, s in views],
                        dtype=np.int64)
        self._adopt(kind, nstates, nsymbols, vlen)

    def set_observations_device(self, kind, dev_ptr, offsets, nstates, nsymbols=0, chunk=0):
        """Same, for a trajectory-concatenated buffer already resident on this GPU
        (dev_ptr: integer device address, e.g. torch.Tensor.data_ptr())."""
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        _lib.check(self._L.bhmm_ctx_set_observations(
            self._h, _KINDS[kind], ctypes.c_void_p(int(dev_ptr)), _lib.lp(off), len(off) - 1,
            int(nstates), int(nsymbols), int(chunk), 1))
        self._adopt(kind, nstates, nsymbols, np.diff(off))

    def _adopt(self, kind, nstates, nsymbols, lengths):
        self.kind = kind
        self.nstates = int(nstates)
        self.nsymbols = int(nsymbols)
        self.lengths = lengths
        self.offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        self._stage = None
        self._fetch = None

    @property
    def _ctx_kind(self):
        """The kind of what the CONTEXT holds, which is what this class's methods go by: the kind the caller loaded,
        unless a subclass loads the context with something else (MvnEngine: explicit rows)."""
        return self.kind

    @property
    def stats_size(self):
        return self._ctx_stats_size()

    def _ctx_stats_size(self):
        """doubles of the context's own packed statistics vector"""
        return self._L.bhmm_ctx_stats_size(self._h)

    @property
    def total_steps(self):
        return self._L.bhmm_ctx_total_steps(self._h)

    @property
    def num_chunks(self):
        return self._L.bhmm_ctx_num_chunks(self._h)

    @property
    def chunk_len(self):
        return self._L.bhmm_ctx_chunk_len(self._h)

    @property
    def stream(self):
        return self._L.bhmm_ctx_stream(self._h)

    def set_option(self, name, value):
        _lib.check(self._L.bhmm_ctx_set_option(self._h, name.encode(), float(value)))

    def get_option(self, name):
        v = ctypes.c_double(0.0)
        _lib.check(self._L.bhmm_ctx_get_option(self._h, name.encode(), ctypes.byref(v)))
        return v.value

    def sync(self):
        _lib.check(self._L.bhmm_ctx_sync(self._h))

    def kernel_ms(self, which):
        return self._L.bhmm_ctx_last_kernel_ms(self._h, which)

    def kernel_ms_all(self):
        """The five HIP-event intervals of the last E-step (prescan, stitch, sweep, finalise, whole)
        in an array owned by the engine (overwritten by the next call)."""
        k = self._kms
        if k is None:
            buf = np.zeros(5)
            k = self._kms = (buf, _lib.dp(buf))
        _lib.check(self._L.bhmm_ctx_last_kernel_ms_all(self._h, k[1]))
        return k[0]

    # -- E-step --------------------------------------------------------------------------
    _STAGE_LIMIT = 1 << 16   # elements: larger emission tables are passed as they are

    def _model_ptrs(self, A, pi, par0, par1):
        """ctypes pointers (A, pi, par0, par1) for one call.  The model is copied into arrays owned
        by the engine whose pointers are made once per set of observations: building four ctypes
        pointers from numpy arrays costs ~13 us per call, a sixtieth of an E-step of configs[1]."""
        n = self.nstates
        if np.shape(A) != (n, n) or np.shape(pi) != (n,):
            raise ValueError("model shape does not match nstates=%d" % n)
        st = self._stage
        if st is None:
            st = self._stage = {}
        out = []
        for key, a in (("A", A), ("pi", pi), ("p0", par0), ("p1", par1)):
            if a is None:
                out.append(None)
                continue
            shp = np.shape(a)
            ent = st.get(key)
            if ent is None or ent[0].shape != shp:
                if int(np.prod(shp, dtype=np.int64)) > self._STAGE_LIMIT:
                    a = _lib.f64(a)
                    self._keep[key] = a             # alive until the call returns
                    out.append(_lib.dp(a))
                    continue
                buf = np.empty(shp, dtype=np.float64)
                ent = st[key] = (buf, _lib.dp(buf))
            np.copyto(ent[0], a)
            out.append(ent[1])
        return out

    def estep_launch(self, A, pi, par0=None, par1=None, stats_dev=None, store_gamma=False, single=False):
        """Enqueue one E-step.  stats_dev: optional device address receiving the packed
        statistics (e.g. a torch tensor that is all-reduced across ranks afterwards).  single: the
        caller accepts single-precision accuracy (BHMM_FLAG_SINGLE; get_option('f32_used') tells
        whether the fp32 kernels ran or the call went to the fp64 path)."""
        A, pi, p0, p1 = self._model_ptrs(A, pi, par0, par1)
        flags = (_lib.FLAG_STORE_GAMMA if store_gamma else 0) | (_lib.FLAG_SINGLE if single else 0)
        _lib.check(self._L.bhmm_estep(self._h, A, pi, p0, p1,
                                      ctypes.c_void_p(int(stats_dev)) if stats_dev else None,
                                      flags))

    def estep_fetch(self):
        S = self._ctx_stats_size()
        packed = np.empty(S)
        logL_k = np.empty(len(self.lengths))
        _lib.check(self._L.bhmm_estep_fetch(self._h, _lib.dp(packed), _lib.dp(logL_k)))
        return EStepResult(self._ctx_kind, self.nstates, self.nsymbols, packed, logL_k)

    def estep_fetch_packed(self, out=None):
        """Wait for the last E-step and return only its packed statistics vector (layout:
        include/bhmm_amd.h, bhmm_ctx_stats_size) -- no per-field copies, no logL_k."""
        if out is None:
            out = np.empty(self._ctx_stats_size())
        f = self._fetch
        if f is None or f[0] is not out:            # the pointer of a re-used `out` is made once
            f = self._fetch = (out, _lib.dp(out))
        _lib.check(self._L.bhmm_estep_fetch(self._h, f[1], None))
        return out

    def estep_fetch_logL(self):
        """Per-trajectory log-likelihoods of the last E-step only (waits for it).  Used when the
        packed statistics stay on the device for an all-reduce."""
        logL_k = np.empty(len(self.lengths))
        _lib.check(self._L.bhmm_estep_fetch(self._h, None, _lib.dp(logL_k)))
        return logL_k

    def estep(self, A, pi, par0=None, par1=None, store_gamma=False, single=False):
        self.estep_launch(A, pi, par0, par1, store_gamma=store_gamma, single=single)
        return self.estep_fetch()

    def unpack(self, packed, logL_k=None):
        return EStepResult(self._ctx_kind, self.nstates, self.nsymbols, np.asarray(packed), logL_k)

    def gamma(self, k):
        T = int(self.lengths[k])
        g = np.empty((T, self.nstates))
        _lib.check(self._L.bhmm_get_gamma(self._h, int(k), _lib.dp(g)))
        return g

    # -- scoring -------------------------------------------------------------------------
    def score(self, models):
        """Log-likelihood of every loaded trajectory under each model (bhmm_score): `models` is a
        list of (A, pi, par0, par1) tuples as for estep.  Returns an (S, K) array; a trajectory of
        probability zero under a model scores -inf there.  Forward pass only; leaves the state that
        later E-steps, Viterbi and sampling calls use untouched.  Gaussian and discrete models run parallel
        over time: up to 8 states over the chunk plan, 9 to 64 states over a segment plan of its own (option
        score_seglen; get_option("score_path") is 2 there, "score_segments" the plan's size), 65 to 128 states
        the same on the matrix cores (score_path 3) -- up to 128 states run parallel over time; more than 128
        states and explicit pobs take the exact serial recursion (score_path 0)."""
        if self._ctx_kind is None:
            raise ValueError("no observations loaded")
        A, pi, p0, p1 = stack_models(self._ctx_kind, self.nstates, self.nsymbols, models)
        logL = np.empty((len(models), len(self.lengths)))
        _lib.check(self._L.bhmm_score(self._h, len(models), _lib.dp(A), _lib.dp(pi), _lib.dp(p0), _lib.dp(p1),
                                      _lib.dp(logL)))
        return logL

    def _check_model(self, A, pi, par0, par1):
        """Shapes of one model against the loaded observations, before any native call."""
        if self._ctx_kind is None:
            raise ValueError("no observations loaded")
        n, M = self.nstates, self.nsymbols
        if np.shape(A) != (n, n) or np.shape(pi) != (n,):
            raise ValueError("A must be (%d, %d) and pi (%d,)" % (n, n, n))
        if self._ctx_kind == 'gaussian':
            if par0 is None or par1 is None:
                raise ValueError("gaussian emissions need means and sigmas")
            if np.shape(par0) != (n,) or np.shape(par1) != (n,):
                raise ValueError("means and sigmas must be (%d,)" % n)
        elif self._ctx_kind == 'discrete':
            if par0 is None:
                raise ValueError("discrete emissions need B")
            if np.shape(par0) != (n, M):
                raise ValueError("B must be (%d, %d)" % (n, M))

    # -- posterior decoding ----------------------------------------------------------------
    def posterior_decode(self, A, pi, par0=None, par1=None, confidence=False, out=None):
        """Posterior (maximum-posterior-marginal) decoding (bhmm_posterior_decode): for every step the
        state of largest gamma_t(i) -- the lowest index on exactly equal gamma -- and, with `confidence`,
        that largest gamma.  Returns a list of per-trajectory uint8 views (int32 above 256 states) like
        viterbi, or (paths, conf) with per-trajectory float32 views.  out: None, or a C-contiguous numpy
        array of sum(T_k) elements of that path dtype which receives the concatenated paths (the views
        then point into it).  Up to 8 states (gaussian, discrete) one fused kernel decodes without storing
        gamma and leaves the state of E-step, Viterbi, sampling and scoring calls untouched
        (get_option("post_path") == 1; options post_W, post_ws_mb, read-only post_fallbacks).  9 to 64
        states (gaussian, discrete) can run over time segments instead -- k_filter_wide forward,
        k_smooth_wide_bwd backward, a workspace of at most smooth_ws_mb MiB, no gamma stored, no other
        call's state touched (post_path 2): set_option("smooth_wide", 1); the default -1 takes it only
        where it was measured faster than the E-step route (no class: it wins at 128 x 1e5 steps, loses at 128 x 1e4, so -1 acts as 0); options smooth_seglen, smooth_W, smooth_ws_mb, read-only smooth_segments and
        smooth_wide_min_total.  65 to 128 states (gaussian, discrete) can run on the fp64 matrix cores
        -- k_filter_tile forward, k_smooth_tile_bwd backward, the same workspace budget, no gamma stored,
        no other call's state touched (post_path 3): set_option("smooth_tile", 1); the default -1 takes it
        only for the call forms measured faster than the E-step route in every shape (DESIGN.md section
        18); one segment outside the kernels' number range (probability zero, an outlier, a NaN
        observation) sends the whole call to the E-step route; the same options, read-only
        smooth_tile_min_total.  Everything else (9 states and more otherwise, explicit pobs) runs an
        E-step that stores gamma and counts as one (post_path 0)."""
        if self._ctx_kind is None:
            raise ValueError("no observations loaded")
        n = self.nstates
        self._check_model(A, pi, par0, par1)
        total = int(self.offsets[-1])
        dtype = np.uint8 if n <= 256 else np.int32
        if out is None:
            out = np.empty(total, dtype=dtype)
        elif (not isinstance(out, np.ndarray) or out.dtype != dtype or out.ndim != 1 or out.size != total
              or not out.flags.c_contiguous):
            raise ValueError("out must be a C-contiguous %s array of sum(T_k) = %d elements"
                             % (np.dtype(dtype).name, total))
        conf = np.empty(total, dtype=np.float32) if confidence else None
        A, pi, p0, p1 = self._model_ptrs(A, pi, par0, par1)
        _lib.check(self._L.bhmm_posterior_decode(
            self._h, A, pi, p0, p1, ctypes.c_void_p(out.ctypes.data), 1 if dtype == np.uint8 else 0,
            ctypes.c_void_p(conf.ctypes.data) if confidence else None))
        K = len(self.lengths)
        paths = [out[self.offsets[k]:self.offsets[k + 1]] for k in range(K)]
        if not confidence:
            return paths
        return paths, [conf[self.offsets[k]:self.offsets[k + 1]] for k in range(K)]

    # -- posterior state probabilities ---------------------------------------------------
    def posterior_marginals(self, A, pi, par0=None, par1=None, weights=None, dtype=np.float64, out=None):
        """Posterior state probabilities gamma_t(i) of every step of every loaded trajectory under one model
        (bhmm_posterior_marginals).  Returns a list of per-trajectory views (T_k, Q') into ONE array of
        sum(T_k) rows: Q' = nstates, or with `weights` (an (nstates, Q) matrix, 1 <= Q <= 8) Q' = Q and the
        rows are gamma_t @ weights, accumulated over the states in ascending order in fp64.  dtype: float64
        or float32 (the rounded float64 result).  out: None (a numpy array is allocated), a C-contiguous numpy
        array of that dtype and sum(T_k) * Q' elements, an object with data_ptr() / is_cuda (a torch tensor: on
        this engine's GPU the kernels write it directly and nothing crosses the link, pinned host memory is
        copied at link rate), or an integer device address on this engine's GPU, aligned to 16 bytes (as
        estep_launch takes stats_dev; then None is returned).  Rows left on the device are complete in the
        order of the engine's stream (sync()).  Up to 8 states (gaussian, discrete) one fused kernel leaves
        the state of every other call untouched (get_option("marg_path") == 1; options marg_W, marg_ws_mb,
        read-only marg_fallbacks).  9 to 64 states (gaussian, discrete) can run over time segments instead
        (marg_path 2, as posterior_decode: set_option("smooth_wide", 1); the default -1 takes it only
        where it was measured faster at every size, no class); there a projection is summed over the states by a fixed tree over the lanes, not in
        ascending order.  65 to 128 states (gaussian, discrete) can run on the fp64 matrix cores (marg_path 3,
        as posterior_decode: set_option("smooth_tile", 1)); a projection is summed by a fixed tree over
        sixteen lanes there.  Everything else (9 states and more otherwise, explicit pobs) runs an E-step that
        stores gamma and counts as one (marg_path 0)."""
        self._check_model(A, pi, par0, par1)
        n = self.nstates
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("dtype must be float64 or float32, not %s" % dtype.name)
        V, Q = None, 0
        if weights is not None:
            V = np.ascontiguousarray(weights, dtype=np.float64)
            if V.ndim != 2 or V.shape[0] != n or not 1 <= V.shape[1] <= 8:
                raise ValueError("weights must be (%d, Q) with 1 <= Q <= 8, not %r" % (n, np.shape(weights)))
            if not np.all(np.isfinite(V)):
                raise ValueError("weights has a non-finite entry")
            Q = V.shape[1]
        Qp = Q if Q else n
        total = int(self.offsets[-1])
        flags = _lib.MARG_F32 if dtype == np.float32 else 0
        rows = None
        if out is None:
            out = np.empty((total, Qp), dtype=dtype)
        if isinstance(out, np.ndarray):
            if out.dtype != dtype or out.size != total * Qp or not out.flags.c_contiguous:
                raise ValueError("out must be a C-contiguous %s array of sum(T_k) * %d = %d elements"
                                 % (dtype.name, Qp, total * Qp))
            ptr, rows = out.ctypes.data, out.reshape(total, Qp)
        elif hasattr(out, 'data_ptr'):
            if out.numel() != total * Qp or out.element_size() != dtype.itemsize or not out.is_contiguous() \
                    or not out.is_floating_point():
                raise ValueError("out must be a contiguous %s tensor of sum(T_k) * %d = %d elements"
                                 % (dtype.name, Qp, total * Qp))
            if out.is_cuda:
                if out.device.index != self.device:
                    raise ValueError("out lives on another GPU than this engine")
                flags |= _lib.MARG_DEVICE
            ptr, rows = out.data_ptr(), out.view(total, Qp)
        else:
            ptr = int(out)
            flags |= _lib.MARG_DEVICE
        if (flags & _lib.MARG_DEVICE) and ptr % 16:
            raise ValueError("a device buffer must be aligned to 16 bytes")
        A, pi, p0, p1 = self._model_ptrs(A, pi, par0, par1)
        _lib.check(self._L.bhmm_posterior_marginals(self._h, A, pi, p0, p1, _lib.dp(V), Q,
                                                    ctypes.c_void_p(int(ptr)), flags))
        if rows is None:
            return None
        return [rows[self.offsets[k]:self.offsets[k + 1]] for k in range(len(self.lengths))]

    # -- pair posteriors -------------------------------------------------------------------
    def posterior_transitions(self, A, pi, par0=None, par1=None, weights=None, dtype=np.float64, out=None):
        """Pair posteriors xi_t(i, j) = P(s_t = i, s_t+1 = j | O) of every transition t -> t+1 of every loaded
        trajectory under one model (bhmm_posterior_transitions), in one of two forms.  weights=None, the jump
        form: a list of 1-d arrays of length T_k - 1, P(s_t != s_t+1 | O) -- the soft counterpart of the run
        boundaries decode_runs returns.  weights of shape (nstates, nstates, Q), 1 <= Q <= 8, the projected
        form: a list of (T_k - 1, Q) arrays, sum_ij xi_t(i, j) weights[i, j, q], accumulated with i the outer
        and j the inner loop in ascending order in fp64 (the jump form is bitwise the projection on the
        off-diagonal 0/1 mask).  The arrays are views into ONE array of sum(T_k) rows in which the last row of
        every trajectory is zero; the views leave that row out.  dtype: float64 or float32 (the rounded float64
        result).  out: as for posterior_marginals -- None, a C-contiguous numpy array of that dtype and
        sum(T_k) * Q' elements (Q' = 1 or Q), an object with data_ptr() / is_cuda (a torch tensor), or an
        integer device address on this engine's GPU aligned to 16 bytes (then None is returned).  Rows left on
        the device are complete in the order of the engine's stream (sync()).  Up to 8 states (gaussian,
        discrete) one fused kernel leaves the state of every other call untouched (get_option("pair_path") == 1;
        options pair_W, pair_ws_mb, pair_fused, read-only pair_fallbacks).  Everything else (9 states and more,
        explicit pobs, pair_fused 0) runs filter_states and posterior_marginals on the device and one kernel
        over their rows (pair_path 0), and counts as those two calls.  That row kernel is k_pair_rows (one thread
        per step, the order above) or, up to 128 states, k_pair_tile on the fp64 matrix cores (16 steps a tile;
        it sums in a fixed tree order, is repeatable bitwise and is held to the same bound against the oracle, not
        to bitwise equality with k_pair_rows): set_option("pair_rows", 0 / 1) forces one or the other (1: every
        kind up to 128 states), the default -1 takes k_pair_tile at 9 to 128 states, where it was measured
        faster in every shape; get_option("pair_rows_kernel") says which one the last generic pass ran."""
        self._check_model(A, pi, par0, par1)
        n = self.nstates
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("dtype must be float64 or float32, not %s" % dtype.name)
        W, Q = None, 0
        if weights is not None:
            W = np.ascontiguousarray(weights, dtype=np.float64)
            if W.ndim != 3 or W.shape[0] != n or W.shape[1] != n or not 1 <= W.shape[2] <= 8:
                raise ValueError("weights must be (%d, %d, Q) with 1 <= Q <= 8, not %r" % (n, n, np.shape(weights)))
            if not np.all(np.isfinite(W)):
                raise ValueError("weights has a non-finite entry")
            Q = W.shape[2]
        Qp = Q if Q else 1
        total = int(self.offsets[-1])
        flags = _lib.PAIR_F32 if dtype == np.float32 else 0
        rows = None
        if out is None:
            out = np.empty((total, Qp), dtype=dtype)
        if isinstance(out, np.ndarray):
            if out.dtype != dtype or out.size != total * Qp or not out.flags.c_contiguous:
                raise ValueError("out must be a C-contiguous %s array of sum(T_k) * %d = %d elements"
                                 % (dtype.name, Qp, total * Qp))
            ptr, rows = out.ctypes.data, out.reshape(total, Qp)
        elif hasattr(out, 'data_ptr'):
            if out.numel() != total * Qp or out.element_size() != dtype.itemsize or not out.is_contiguous() \
                    or not out.is_floating_point():
                raise ValueError("out must be a contiguous %s tensor of sum(T_k) * %d = %d elements"
                                 % (dtype.name, Qp, total * Qp))
            if out.is_cuda:
                if out.device.index != self.device:
                    raise ValueError("out lives on another GPU than this engine")
                flags |= _lib.PAIR_DEVICE
            ptr, rows = out.data_ptr(), out.view(total, Qp)
        else:
            ptr = int(out)
            flags |= _lib.PAIR_DEVICE
        if (flags & _lib.PAIR_DEVICE) and ptr % 16:
            raise ValueError("a device buffer must be aligned to 16 bytes")
        A, pi, p0, p1 = self._model_ptrs(A, pi, par0, par1)
        _lib.check(self._L.bhmm_posterior_transitions(self._h, A, pi, p0, p1, _lib.dp(W), Q,
                                                      ctypes.c_void_p(int(ptr)), flags))
        if rows is None:
            return None
        views = [rows[self.offsets[k]:max(self.offsets[k + 1] - 1, self.offsets[k])] for k in range(len(self.lengths))]
        return views if Q else [v[:, 0] for v in views]

    # -- filtered state probabilities ----------------------------------------------------
    def _filter_out(self, out, what, total, width, dtype):
        """(address, 2-d view or None, on this engine's GPU) of one output of filter_states"""
        if out is None:
            out = np.empty((total, width) if what == 'out' else total, dtype=dtype)
        shape = (total, width) if what == 'out' else (total,)
        if isinstance(out, np.ndarray):
            if out.dtype != dtype or out.size != total * width or not out.flags.c_contiguous:
                raise ValueError("%s must be a C-contiguous %s array of %d elements" % (what, dtype.name, total * width))
            return out.ctypes.data, out.reshape(shape), False
        if hasattr(out, 'data_ptr'):
            if out.numel() != total * width or out.element_size() != dtype.itemsize or not out.is_contiguous() \
                    or not out.is_floating_point():
                raise ValueError("%s must be a contiguous %s tensor of %d elements" % (what, dtype.name, total * width))
            if out.is_cuda and out.device.index != self.device:
                raise ValueError("%s lives on another GPU than this engine" % what)
            return out.data_ptr(), out.view(*shape), bool(out.is_cuda)
        return int(out), None, True

    def filter_states(self, A, pi, par0=None, par1=None, weights=None, dtype=np.float64, probabilities=True,
                      increments=True, out=None, out_increments=None):
        """Filtered state probabilities P(s_t = i | o_0 .. o_t) of every step of every loaded trajectory under one
        model, and the one-step predictive log-densities log p(o_t | o_0 .. o_{t-1}) whose sum is the
        log-likelihood (bhmm_filter).  Returns (rows, logc): rows a list of per-trajectory views (T_k, Q') into
        ONE array of sum(T_k) rows -- Q' = nstates, or with `weights` (an (nstates, Q) matrix, 1 <= Q <= 8)
        Q' = Q and the rows are alpha^_t @ weights, accumulated over the states in ascending order in fp64 --
        and logc a list of per-trajectory views (T_k,) into one array; None for the one not asked for
        (probabilities / increments; at least one).  logc[k][0] = log sum_i pi_i p_0(i).  From the first step of
        probability zero on, the rows of a trajectory are zero and its logc -inf.  dtype: float64 or float32
        (the rounded float64 result), for both.  out / out_increments: None (numpy arrays are allocated), a
        C-contiguous numpy array of that dtype, an object with data_ptr() / is_cuda (a torch tensor), or an
        integer device address on this engine's GPU aligned to 16 bytes (then None stands in the result); both
        on the host or both on this engine's GPU.  Results left on the device are complete in the order of the
        engine's stream (sync()).  Up to 8 states (gaussian, discrete) one chunk-parallel forward sweep with
        verified boundaries (get_option("filter_path") == 1; option filter_W, read-only filter_fallbacks); 9
        states and more and explicit pobs run the serial recursion, one workgroup per trajectory (filter_path
        0).  No other call's state is touched."""
        self._check_model(A, pi, par0, par1)
        n = self.nstates
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("dtype must be float64 or float32, not %s" % dtype.name)
        if not probabilities and not increments:
            raise ValueError("neither probabilities nor increments asked for")
        if (not probabilities and out is not None) or (not increments and out_increments is not None):
            raise ValueError("a buffer was passed for an output that is not asked for")
        V, Q = None, 0
        if weights is not None:
            V = np.ascontiguousarray(weights, dtype=np.float64)
            if V.ndim != 2 or V.shape[0] != n or not 1 <= V.shape[1] <= 8:
                raise ValueError("weights must be (%d, Q) with 1 <= Q <= 8, not %r" % (n, np.shape(weights)))
            if not np.all(np.isfinite(V)):
                raise ValueError("weights has a non-finite entry")
            Q = V.shape[1]
        Qp = Q if Q else n
        total = int(self.offsets[-1])
        rptr = lptr = 0
        rows = logc = None
        where = []
        if probabilities:
            rptr, rows, dev = self._filter_out(out, 'out', total, Qp, dtype)
            where.append(dev)
        if increments:
            lptr, logc, dev = self._filter_out(out_increments, 'out_increments', total, 1, dtype)
            where.append(dev)
        if len(set(where)) > 1:
            raise ValueError("out and out_increments must both be on the host or both on this engine's GPU")
        flags = _lib.FILT_F32 if dtype == np.float32 else 0
        if where[0]:
            flags |= _lib.FILT_DEVICE
            if rptr % 16 or lptr % 16:
                raise ValueError("a device buffer must be aligned to 16 bytes")
        A, pi, p0, p1 = self._model_ptrs(A, pi, par0, par1)
        _lib.check(self._L.bhmm_filter(self._h, A, pi, p0, p1, _lib.dp(V) if probabilities else None,
                                       Q if probabilities else 0, ctypes.c_void_p(int(rptr)) if probabilities else None,
                                       ctypes.c_void_p(int(lptr)) if increments else None, flags))
        K = len(self.lengths)
        if rows is not None:
            rows = [rows[self.offsets[k]:self.offsets[k + 1]] for k in range(K)]
        if logc is not None:
            logc = [logc[self.offsets[k]:self.offsets[k + 1]] for k in range(K)]
        return rows, logc

    # -- paths ---------------------------------------------------------------------------
    def viterbi(self, A, pi, par0=None, par1=None):
        A, pi, p0, p1 = self._model_ptrs(A, pi, par0, par1)
        paths = np.empty(int(self.offsets[-1]), dtype=np.int32)
        _lib.check(self._L.bhmm_viterbi_batch(self._h, A, pi, p0, p1, _lib.ip(paths)))
        return [paths[self.offsets[k]:self.offsets[k + 1]] for k in range(len(self.lengths))]

    def viterbi_u8(self, A, pi, par0=None, par1=None, out=None):
        """Viterbi paths as one byte per step.  out: None (a numpy uint8 array is allocated), a
        numpy uint8 array, or any object with data_ptr()/is_cuda (a torch uint8 tensor: on this
        engine's GPU the kernels write it directly, pinned host memory is copied at link rate).
        Returns `out` (concatenated over trajectories like the observations)."""
        A, pi, p0, p1 = self._model_ptrs(A, pi, par0, par1)
        total = int(self.offsets[-1])
        on_dev = 0
        if out is None:
            out = np.empty(total, dtype=np.uint8)
        if isinstance(out, np.ndarray):
            if out.dtype != np.uint8 or out.size < total or not out.flags.c_contiguous:
                raise ValueError("out must be a contiguous uint8 array of sum(T_k) elements")
            ptr = out.ctypes.data
        else:
            if out.numel() < total or out.element_size() != 1 or not out.is_contiguous():
                raise ValueError("out must be a contiguous uint8 tensor of sum(T_k) elements")
            on_dev = 1 if out.is_cuda else 0
            if on_dev and out.device.index != self.device:
                raise ValueError("out lives on another GPU than this engine")
            ptr = out.data_ptr()
        _lib.check(self._L.bhmm_viterbi_batch_u8(self._h, A, pi, p0, p1, ctypes.c_void_p(int(ptr)), on_dev))
        return out

    # -- dwell segments of a path ----------------------------------------------------------
    def _runs_result(self, call, stats):
        """Run one of the two runs calls (call(run_off, dwell, jumps) -> status) and fetch its runs."""
        n, K = self.nstates, len(self.lengths)
        off = np.empty(K + 1, dtype=np.int64)
        dwell = np.zeros((n, _lib.DWELL_COLS), dtype=np.int64) if stats else None
        jumps = np.zeros((n, n), dtype=np.int64) if stats else None
        _lib.check(call(_lib.lp(off), _lib.lp(dwell), _lib.lp(jumps)))
        R = int(off[K])
        start, length = np.empty(R, dtype=np.int64), np.empty(R, dtype=np.int64)
        state = np.empty(R, dtype=np.int32)
        _lib.check(self._L.bhmm_runs_fetch(self._h, _lib.lp(start), _lib.lp(length), _lib.ip(state)))
        return PathRuns(off, start, length, state, dwell, jumps)

    def path_runs(self, paths, stats=False):
        """Dwell segments of a GIVEN path, compacted on the device (bhmm_path_runs): `paths` holds one state per
        step of every loaded trajectory, concatenated like the observations -- what viterbi_u8 and
        posterior_decode(out=...) write.  A C-contiguous numpy uint8 or int32 array of sum(T_k) elements (staged on
        the device), or an object with data_ptr() / is_cuda of one or four bytes per element (a torch uint8 / int32
        tensor: on this engine's GPU it is read in place and must be aligned to 16 bytes; host memory is staged).
        uint8 needs nstates <= 256.  A state outside [0, nstates) raises ValueError.  Returns a PathRuns; with
        `stats` its dwell and jumps tables are filled.  Only the runs cross the link (get_option("runs_count"),
        "runs_ms": device time of the compaction; read-only "runs_tile", "runs_lane")."""
        ptr, u8, on_dev = self._path_arg(paths)
        return self._runs_result(
            lambda off, dwell, jumps: self._L.bhmm_path_runs(self._h, ctypes.c_void_p(int(ptr)), 1 if u8 else 0,
                                                             on_dev, off, dwell, jumps), stats)

    def _path_arg(self, paths, loaded=None):
        """(address, one byte per step, on this engine's GPU) of a flat path, validated against the loaded
        trajectories before any native call (path_runs, path_logprob; loaded: the caller's own answer to "are there
        observations", where that is not the context's kind)."""
        if not (self._ctx_kind is not None if loaded is None else loaded):
            raise ValueError("no observations loaded")
        total = int(self.offsets[-1])
        on_dev = 0
        if isinstance(paths, np.ndarray):
            if paths.dtype not in (np.dtype(np.uint8), np.dtype(np.int32)):
                raise ValueError("paths must be uint8 or int32, not %s" % paths.dtype.name)
            if paths.ndim != 1 or paths.size != total or not paths.flags.c_contiguous:
                raise ValueError("paths must be a C-contiguous array of sum(T_k) = %d elements" % total)
            u8 = paths.dtype == np.uint8
            ptr = paths.ctypes.data
        elif hasattr(paths, 'data_ptr'):
            if paths.element_size() not in (1, 4) or paths.is_floating_point():
                raise ValueError("paths must be a uint8 or int32 tensor")
            if paths.numel() != total or not paths.is_contiguous():
                raise ValueError("paths must be a contiguous tensor of sum(T_k) = %d elements" % total)
            u8 = paths.element_size() == 1
            ptr = paths.data_ptr()
            if paths.is_cuda:
                if paths.device.index != self.device:
                    raise ValueError("paths lives on another GPU than this engine")
                if ptr % 16:
                    raise ValueError("a device path must be aligned to 16 bytes")
                on_dev = 1
        else:
            raise ValueError("paths must be a numpy array or an object with data_ptr() / is_cuda")
        if u8 and self.nstates > 256:
            raise ValueError("one byte per step holds at most 256 states (pass an int32 path)")
        return ptr, u8, on_dev

    # -- joint log-probability of a path -----------------------------------------------------
    def path_logprob(self, paths, models):
        """Joint log-probability log p(s, O | model) of GIVEN hidden paths under each model (bhmm_path_logprob), per
        trajectory: log pi(s_0) + e(s_0, o_0) + sum_t [log A(s_t-1, s_t) + e(s_t, o_t)] -- the "Viterbi score" when s
        is the Viterbi path.  `paths` as path_runs takes them -- a C-contiguous numpy uint8 or int32 array of
        sum(T_k) states concatenated like the observations (staged on the device), or an object with data_ptr() /
        is_cuda (a torch uint8 / int32 tensor: on this engine's GPU it is read in place and must be aligned to 16
        bytes) -- or a list / tuple of one integer array per trajectory.  `models` as score takes them: a list of
        (A, pi, par0, par1) tuples.  Returns an (S, K) float64 array.  Every term is formed in log space: the
        gaussian density is never exponentiated and the outlier rule of the recursions (an emission row that
        underflowed to all zeros counts as all ones) is deliberately NOT applied -- an outlier gives a very negative
        finite term.  A zero probability on the path gives -inf for that trajectory (never NaN, no other trajectory
        changes), a NaN observation NaN for its own trajectory, an empty trajectory 0.0; a state outside
        [0, nstates) raises ValueError.  Path and observations are read once for all models; no floating-point
        atomics, so the result is bitwise the same from call to call, for a host and a device path, for uint8 and
        int32, and for a model alone and inside a stack (read-only options "pathlp_tile", "pathlp_lane",
        "pathlp_table": 1 if the log-transition table sat in LDS, "pathlp_ms": device time)."""
        if self._ctx_kind is None:
            raise ValueError("no observations loaded")
        if isinstance(paths, (list, tuple)):
            paths = self._concat_paths(paths)
        ptr, u8, on_dev = self._path_arg(paths)
        A, pi, p0, p1 = stack_models(self._ctx_kind, self.nstates, self.nsymbols, models)
        S = A.shape[0]
        logp = np.empty((S, len(self.lengths)))
        _lib.check(self._L.bhmm_path_logprob(self._h, ctypes.c_void_p(int(ptr)), 1 if u8 else 0, on_dev, S, _lib.dp(A),
                                             _lib.dp(pi), _lib.dp(p0), _lib.dp(p1), _lib.dp(logp)))
        return logp

    def _concat_paths(self, paths):
        """One flat uint8 (every piece uint8) or int32 array from one integer array per loaded trajectory."""
        if len(paths) != len(self.lengths):
            raise ValueError("expected one path per trajectory (%d), got %d" % (len(self.lengths), len(paths)))
        pieces = [np.asarray(p) for p in paths]
        for k, p in enumerate(pieces):
            if p.ndim != 1 or p.shape[0] != int(self.lengths[k]):
                raise ValueError("path %d must be 1-d with %d steps, not %r" % (k, int(self.lengths[k]), p.shape))
            if p.size and not np.issubdtype(p.dtype, np.integer):
                raise ValueError("path %d must hold integers, not %s" % (k, p.dtype.name))
        dtype = np.uint8 if all(p.dtype == np.uint8 for p in pieces if p.size) else np.int32
        flat = np.empty(int(self.offsets[-1]), dtype=dtype)
        for k, p in enumerate(pieces):
            if p.size and dtype == np.int32 and (p.min() < np.iinfo(np.int32).min or p.max() > np.iinfo(np.int32).max):
                raise ValueError("path %d holds a state outside int32" % k)
            flat[self.offsets[k]:self.offsets[k + 1]] = p
        return flat

    def decode_logprob(self, A, pi, par0=None, par1=None, method='viterbi'):
        """Decode every loaded trajectory under one model and return the joint log-probability of the decoded path
        under that model (bhmm_decode_logprob), a (K,) float64 array: method 'viterbi' runs what viterbi_u8 runs
        into a device buffer (the result is the Viterbi score), 'posterior' what posterior_decode runs up to its
        copy to the host -- the same kernels, options and side effects on the engine -- and the path is scored on
        the device: only K numbers cross the link.  A posterior-decoded path can take a jump the model forbids: its
        trajectory scores -inf.  Terms as for path_logprob (log space, no outlier rule).  Up to 256 states (more:
        decode with viterbi / posterior_decode and call path_logprob on the int32 path)."""
        if method not in _METHODS:
            raise ValueError("method must be 'viterbi' or 'posterior', not %r" % (method,))
        self._check_model(A, pi, par0, par1)
        if self.nstates > 256:
            raise ValueError("decode_logprob handles up to 256 states (decode, then path_logprob on the int32 path)")
        A, pi, p0, p1 = self._model_ptrs(A, pi, par0, par1)
        logp = np.empty(len(self.lengths))
        _lib.check(self._L.bhmm_decode_logprob(self._h, A, pi, p0, p1, _METHODS[method], _lib.dp(logp)))
        return logp

    def decode_runs(self, A, pi, par0=None, par1=None, method='viterbi', stats=False):
        """Decode every loaded trajectory under one model and return the dwell segments of the decoded path
        (bhmm_decode_runs): method 'viterbi' runs what viterbi_u8 runs into a device buffer, 'posterior' what
        posterior_decode runs up to its copy to the host -- the same kernels, options and side effects on the
        engine -- and the path is compacted on the device: it never crosses the link.  Up to 256 states (more:
        decode with viterbi / posterior_decode and call path_runs on the int32 path).  Returns a PathRuns; with
        `stats` its dwell and jumps tables are filled."""
        if method not in _METHODS:
            raise ValueError("method must be 'viterbi' or 'posterior', not %r" % (method,))
        self._check_model(A, pi, par0, par1)
        if self.nstates > 256:
            raise ValueError("decode_runs handles up to 256 states (decode, then path_runs on the int32 path)")
        A, pi, p0, p1 = self._model_ptrs(A, pi, par0, par1)
        return self._runs_result(
            lambda off, dwell, jumps: self._L.bhmm_decode_runs(self._h, A, pi, p0, p1, _METHODS[method], off, dwell,
                                                               jumps), stats)

    def runs_fetch(self):
        """(start, length, state) of the runs the last path_runs / decode_runs call on these observations left on
        the device (bhmm_runs_fetch); ValueError before any."""
        _lib.check(self._L.bhmm_runs_fetch(self._h, None, None, None))   # (no runs: raises)
        R = int(self.get_option("runs_count"))
        start, length = np.empty(R, dtype=np.int64), np.empty(R, dtype=np.int64)
        state = np.empty(R, dtype=np.int32)
        _lib.check(self._L.bhmm_runs_fetch(self._h, _lib.lp(start), _lib.lp(length), _lib.ip(state)))
        return start, length, state

    def set_stream_offsets(self, soff):
        """Position of each loaded trajectory in the device random stream (include/bhmm_amd.h):
        a sharded caller passes the offsets in the unsharded concatenation, None resets."""
        if soff is None:
            _lib.check(self._L.bhmm_ctx_set_stream_offsets(self._h, None))
            return
        soff = np.ascontiguousarray(soff, dtype=np.int64)
        if soff.shape != (len(self.lengths),):
            raise ValueError("one stream offset per loaded trajectory")
        _lib.check(self._L.bhmm_ctx_set_stream_offsets(self._h, _lib.lp(soff)))

    @property
    def path_stats_size(self):
        return self._L.bhmm_ctx_path_stats_size(self._h)

    def sample_paths_dev(self, A, pi, par0, par1, stats_dev, u=None, seed=0, want_paths=False):
        """Gibbs hidden-path step with the packed path statistics left in the device buffer
        `stats_dev` (integer address, path_stats_size doubles).  Returns paths or None."""
        A, pi, p0, p1 = self._model_ptrs(A, pi, par0, par1)
        total = int(self.offsets[-1])
        paths = np.empty(total, dtype=np.int32) if want_paths else None
        uu = _lib.f64(np.concatenate(u)) if u is not None else None
        _lib.check(self._L.bhmm_sample_paths_dev(self._h, A, pi, p0, p1, _lib.dp(uu), ctypes.c_uint64(int(seed)),
                                                 _lib.ip(paths), ctypes.c_void_p(int(stats_dev))))
        if not want_paths:
            return None
        return [paths[self.offsets[k]:self.offsets[k + 1]] for k in range(len(self.lengths))]

    def unpack_path_stats(self, packed):
        """[counts n*n | n0 n | emission block] -> (C int64 (n,n), n0 int64 (n,), emis)."""
        n, M = self.nstates, self.nsymbols
        packed = np.asarray(packed, dtype=np.float64)
        C = np.rint(packed[:n * n]).astype(np.int64).reshape(n, n)
        n0 = np.rint(packed[n * n:n * n + n]).astype(np.int64)
        rest = packed[n * n + n:]
        if self._ctx_kind == 'gaussian':
            emis = rest[:3 * n].reshape(3, n).copy()
        elif self._ctx_kind == 'discrete':
            emis = rest[:n * M].reshape(n, M).copy()
        else:
            emis = None
        return C, n0, emis

    def sample_paths(self, A, pi, par0=None, par1=None, u=None, seed=0, want_paths=True):
        """Gibbs hidden-path step.  Returns (paths or None, C int64 (n,n), n0 int64 (n,), emis)."""
        A, pi, p0, p1 = self._model_ptrs(A, pi, par0, par1)
        n = self.nstates
        total = int(self.offsets[-1])
        paths = np.empty(total, dtype=np.int32) if want_paths else None
        C = np.zeros((n, n), dtype=np.int64)
        n0 = np.zeros(n, dtype=np.int64)
        if self._ctx_kind == 'gaussian':
            emis = np.zeros((3, n))
        elif self._ctx_kind == 'discrete':
            emis = np.zeros((n, self.nsymbols))
        else:
            emis = None
        uu = _lib.f64(np.concatenate(u)) if u is not None else None
        _lib.check(self._L.bhmm_sample_paths(self._h, A, pi, p0, p1, _lib.dp(uu), ctypes.c_uint64(int(seed)),
                                             _lib.ip(paths), _lib.lp(C), _lib.lp(n0),
                                             _lib.dp(emis)))
        plist = None
        if want_paths:
            plist = [paths[self.offsets[k]:self.offsets[k + 1]] for k in range(len(self.lengths))]
        return plist, C, n0, emis


class MvnEngine(Engine):
    """Engine for multivariate gaussian emissions (kind 'mvgaussian'): the observations are
    (T_k, D) arrays, a model is (A, pi, means (n, D), covariances (n, D, D) or (n, D) variances).  The recursions run
    on explicit emission rows: a model-taking method first makes the rows exp(l_ti - m_t) on the device from the
    observations kept there (bhmm_mvn_emissions; not again while the parameters are the ones the loaded rows were
    made from), calls the base method without emission parameters and adds what the scaling took out -- shift_k =
    sum_t m_t to every per-trajectory log-likelihood and path log-probability, m_t to the filter increments.  An
    E-step also returns the moments of the M-step (bhmm_mvn_moments) from the posterior rows left on the device."""

    def __init__(self, device=0, stream=None):
        Engine.__init__(self, device, stream)
        self.dimension = 0
        self._loaded = None        # (means, covariances) the rows on the device were made from
        self._shift = self._m_t = None
        self._gamma_dev = None
        self._moments = None
        self._cov_last = None

    @property
    def _ctx_kind(self):
        """explicit rows once emissions have been made, nothing a model call can use before"""
        return 'explicit' if self._shift is not None else None

    # -- data ---------------------------------------------------------------------------
    def _set(self, ptr, off, nstates, D, chunk, on_device):
        if not 1 <= int(D) <= _lib.MVN_MAX_D:
            raise ValueError("1 <= D <= %d dimensions are supported, not %d" % (_lib.MVN_MAX_D, D))
        self.dimension = 0
        _lib.check(self._L.bhmm_ctx_set_observations_mvn(self._h, ctypes.c_void_p(int(ptr)), _lib.lp(off), len(off) - 1,
                                                         int(D), int(nstates), int(chunk), on_device))
        self._adopt('mvgaussian', nstates, 0, np.diff(off))
        self.dimension = int(D)
        self._loaded = self._shift = self._m_t = self._moments = self._cov_last = None

    def set_observations(self, kind, observations, nstates, nsymbols=0, chunk=0):
        """observations: list of (T_k, D) float arrays, 1 <= D <= 64."""
        if kind != 'mvgaussian':
            raise ValueError("an MvnEngine holds observations of kind 'mvgaussian', not %r" % (kind,))
        from .output_models.mvgaussian import check_observation
        obs = [check_observation(o) for o in observations]
        if not obs:
            raise ValueError("no observations")
        D = obs[0].shape[1]
        if any(o.shape[1] != D for o in obs):
            raise ValueError("every trajectory must have the same number of columns")
        off = np.zeros(len(obs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([o.shape[0] for o in obs])
        flat = np.ascontiguousarray(np.concatenate(obs, axis=0))
        self._set(flat.ctypes.data, off, nstates, D, chunk, 0)

    def set_observations_device(self, kind, dev_ptr, offsets, nstates, nsymbols=0, chunk=0, dimension=None):
        """The same for a (sum T_k, D) row-major float64 buffer already on this GPU (integer device address)."""
        if kind != 'mvgaussian' or dimension is None:
            raise ValueError("an MvnEngine takes kind 'mvgaussian' and the dimension of the observations")
        self._set(dev_ptr, np.ascontiguousarray(offsets, dtype=np.int64), nstates, dimension, chunk, 1)

    def set_observations_lagged(self, *args, **kwargs):
        raise NotImplementedError("lagged views are cut on the host for multivariate observations")

    @property
    def stats_size(self):
        """The explicit kind's vector followed by the moment block of the last covariance type (full before any)."""
        from .output_models.mvgaussian import moment_stride
        return self._ctx_stats_size() + self.nstates * moment_stride(self.dimension, self._cov_last or 'full')

    # -- emissions ------------------------------------------------------------------------
    def _params(self, par0, par1):
        """(means (n, D), covariances, covariance type) of one model, shapes checked."""
        if self.dimension == 0:
            raise ValueError("no observations loaded")
        if par0 is None or par1 is None:
            raise ValueError("multivariate gaussian emissions need means and covariances")
        n, D = self.nstates, self.dimension
        mu, cov = _lib.f64(par0), _lib.f64(par1)
        if mu.shape != (n, D):
            raise ValueError("means must be (%d, %d), not %r" % (n, D, mu.shape))
        if cov.shape == (n, D, D):
            return mu, cov, 'full'
        if cov.shape == (n, D):
            return mu, cov, 'diag'
        raise ValueError("covariances must be (%d, %d, %d) or (%d, %d), not %r" % (n, D, D, n, D, cov.shape))

    def emissions(self, par0, par1, force=False):
        """Make the emission rows of (means, covariances) the context's observations, unless the loaded ones were
        made from the same parameters (force: make them anyway).  Returns the covariance type."""
        mu, cov, ctype = self._params(par0, par1)
        ld = self._loaded
        if not force and ld is not None and ld[0].shape == mu.shape and ld[1].shape == cov.shape \
                and np.array_equal(ld[0], mu) and np.array_equal(ld[1], cov):
            return ctype
        self._loaded = self._shift = self._m_t = self._moments = None   # (the re-load ends the last E-step too)
        _lib.check(self._L.bhmm_mvn_emissions(self._h, _lib.dp(mu), _lib.dp(cov),
                                              _lib.COV_FULL if ctype == 'full' else _lib.COV_DIAG))
        self._stage = None
        self._fetch = None
        shift = np.empty(len(self.lengths))
        _lib.check(self._L.bhmm_mvn_fetch_scale(self._h, _lib.dp(shift), None))
        self._shift = shift
        self._loaded = (mu.copy(), cov.copy())
        return ctype

    @property
    def shifts(self):
        """shift_k = sum_t m_t of the loaded emission rows, per trajectory."""
        if self._shift is None:
            raise ValueError("no emissions made yet")
        return self._shift

    def step_scales(self):
        """m_t = max_i l_ti of the loaded emission rows, concatenated over the trajectories."""
        if self._shift is None:
            raise ValueError("no emissions made yet")
        if self._m_t is None:
            m = np.empty(int(self.offsets[-1]))
            _lib.check(self._L.bhmm_mvn_fetch_scale(self._h, None, _lib.dp(m)))
            self._m_t = m
        return self._m_t

    def emission_rows(self):
        """The loaded emission rows exp(l_ti - m_t), (sum T_k, nstates), copied to the host (tests, diagnostics)."""
        if self._shift is None:
            raise ValueError("no emissions made yet")
        rows = np.empty((int(self.offsets[-1]), self.nstates))
        _lib.check(self._L.bhmm_mvn_fetch_rows(self._h, _lib.dp(rows)))
        return rows

    def moments(self, gamma_dev, means, covariance_type='full'):
        """Packed moments of the M-step (bhmm_mvn_moments) from posterior rows on this GPU: gamma_dev is the
        integer device address of (sum T_k, nstates) float64 rows, or an object with data_ptr()."""
        from .output_models.mvgaussian import moment_stride
        mu = _lib.f64(means)
        if mu.shape != (self.nstates, self.dimension):
            raise ValueError("means must be (%d, %d)" % (self.nstates, self.dimension))
        ptr = gamma_dev.data_ptr() if hasattr(gamma_dev, 'data_ptr') else int(gamma_dev)
        out = np.empty(self.nstates * moment_stride(self.dimension, covariance_type))
        _lib.check(self._L.bhmm_mvn_moments(self._h, ctypes.c_void_p(ptr), _lib.dp(mu),
                                            _lib.COV_FULL if covariance_type == 'full' else _lib.COV_DIAG,
                                            _lib.dp(out)))
        return out

    def _moments_args(self, means, covariance_type):
        from .output_models.mvgaussian import moment_stride
        if self.dimension == 0:
            raise ValueError("no observations loaded")
        mu = _lib.f64(means)
        if mu.shape != (self.nstates, self.dimension):
            raise ValueError("means must be (%d, %d)" % (self.nstates, self.dimension))
        out = np.empty(self.nstates * moment_stride(self.dimension, covariance_type))
        return mu, _lib.COV_FULL if covariance_type == 'full' else _lib.COV_DIAG, out

    def path_moments(self, paths, means, covariance_type='full'):
        """Packed moments of a hidden path about `means` (bhmm_mvn_path_moments), in the layout of `moments`: per
        state the count S0, S1 = sum (x_t - mu_i) and S2 = sum (x_t - mu_i)(x_t - mu_i)^T (lower triangle or
        diagonal) over the steps with s_t = i.  `paths` as path_logprob takes them: a flat uint8 / int32 numpy array,
        a list of one integer array per trajectory, or a uint8 / int32 tensor (read in place on this engine's GPU).
        Needs no emissions.  The arithmetic per step does not grow with the number of states; a state that never
        occurs gives exact zeros, a state outside [0, nstates) raises ValueError; bitwise the same from call to
        call and for every form of the same path (read-only option "mvn_path_moments_ms": device time)."""
        mu, ctype, out = self._moments_args(means, covariance_type)
        if isinstance(paths, (list, tuple)):
            paths = self._concat_paths(paths)
        ptr, u8, on_dev = self._path_arg(paths, loaded=True)
        _lib.check(self._L.bhmm_mvn_path_moments(self._h, ctypes.c_void_p(int(ptr)), 1 if u8 else 0, on_dev,
                                                 _lib.dp(mu), ctype, _lib.dp(out)))
        return out

    def sample_paths_moments(self, A, pi, means, covariances, u=None, seed=0, want_paths=False):
        """Gibbs hidden-path step under (A, pi, means, covariances) followed by the packed moments of the drawn path
        about `means` (bhmm_mvn_sample_paths).  Returns (paths or None, C int64 (n, n), n0 int64 (n,), moments);
        paths, C and n0 are those of sample_paths for the same arguments.  The path stays on the device unless
        want_paths."""
        ctype = self.emissions(means, covariances)
        mu, code, out = self._moments_args(means, ctype)
        A, pi, _, _ = self._model_ptrs(A, pi, None, None)
        n = self.nstates
        total = int(self.offsets[-1])
        paths = np.empty(total, dtype=np.int32) if want_paths else None
        C = np.zeros((n, n), dtype=np.int64)
        n0 = np.zeros(n, dtype=np.int64)
        uu = _lib.f64(np.concatenate(u)) if u is not None else None
        _lib.check(self._L.bhmm_mvn_sample_paths(self._h, A, pi, _lib.dp(uu), ctypes.c_uint64(int(seed)),
                                                 _lib.ip(paths), _lib.lp(C), _lib.lp(n0), _lib.dp(mu), code,
                                                 _lib.dp(out)))
        plist = None
        if want_paths:
            plist = [paths[self.offsets[k]:self.offsets[k + 1]] for k in range(len(self.lengths))]
        return plist, C, n0, out

    # -- E-step --------------------------------------------------------------------------
    def estep_launch(self, A, pi, par0=None, par1=None, stats_dev=None, store_gamma=False, single=False):
        """One E-step: emission rows, then ONE pass of the recursions that leaves the posterior rows on the device
        (posterior_marginals, which on explicit rows is an E-step that stores gamma: its packed statistics stay in
        the context for estep_fetch), then the moments from those rows.  Synchronous."""
        if stats_dev is not None:
            raise NotImplementedError("multivariate gaussian E-steps keep their statistics in the context")
        if single:
            raise NotImplementedError("multivariate gaussian E-steps run in float64")
        ctype = self.emissions(par0, par1)
        import torch
        total = int(self.offsets[-1])
        g = self._gamma_dev
        if g is None or g.numel() != total * self.nstates or g.device.index != self.device:
            g = self._gamma_dev = torch.empty(total * self.nstates, dtype=torch.float64,
                                              device='cuda:%d' % self.device)
        Engine.posterior_marginals(self, A, pi, out=g.data_ptr())
        self._moments = self.moments(g.data_ptr(), self._loaded[0], ctype)
        self._cov_last = ctype

    def _shifted(self, packed):
        packed[0] += self._shift.sum()
        return np.concatenate([packed, self._moments])

    def estep_fetch(self):
        if self._moments is None:
            raise ValueError("no E-step has run on these observations")
        res = Engine.estep_fetch(self)
        return EStepResult('mvgaussian', self.nstates, 0, self._shifted(res.packed), res.logL_k + self._shift,
                           self.dimension, self._cov_last)

    def estep_fetch_packed(self, out=None):
        """The explicit kind's packed vector, its log-likelihood with the shifts added, followed by the packed
        moments of bhmm_mvn_moments."""
        if self._moments is None:
            raise ValueError("no E-step has run on these observations")
        packed = Engine.estep_fetch_packed(self)
        packed = self._shifted(packed)
        if out is None:
            return packed
        out[:] = packed
        return out

    def estep_fetch_logL(self):
        return Engine.estep_fetch_logL(self) + self._shift

    def estep(self, A, pi, par0=None, par1=None, store_gamma=False, single=False):
        self.estep_launch(A, pi, par0, par1, store_gamma=store_gamma, single=single)
        return self.estep_fetch()

    def unpack(self, packed, logL_k=None):
        return EStepResult('mvgaussian', self.nstates, 0, np.asarray(packed), logL_k, self.dimension,
                           self._cov_last or 'full')

    # -- everything else: emissions, the base call on explicit rows, the shifts --------------
    def score(self, models):
        """(S, K) log-likelihoods; one emission pass per model."""
        models = list(models)
        if not models:
            raise ValueError("score needs at least one model")
        out = np.empty((len(models), len(self.lengths)))
        for s, m in enumerate(models):
            if len(m) != 4:
                raise ValueError("model %d: expected an (A, pi, means, covariances) tuple" % s)
            self.emissions(m[2], m[3])
            out[s] = Engine.score(self, [(m[0], m[1], None, None)])[0] + self._shift
        return out

    def posterior_decode(self, A, pi, par0=None, par1=None, confidence=False, out=None):
        self.emissions(par0, par1)
        return Engine.posterior_decode(self, A, pi, confidence=confidence, out=out)

    def posterior_marginals(self, A, pi, par0=None, par1=None, weights=None, dtype=np.float64, out=None):
        self.emissions(par0, par1)
        return Engine.posterior_marginals(self, A, pi, weights=weights, dtype=dtype, out=out)

    def posterior_transitions(self, A, pi, par0=None, par1=None, weights=None, dtype=np.float64, out=None):
        self.emissions(par0, par1)
        return Engine.posterior_transitions(self, A, pi, weights=weights, dtype=dtype, out=out)

    def filter_states(self, A, pi, par0=None, par1=None, weights=None, dtype=np.float64, probabilities=True,
                      increments=True, out=None, out_increments=None):
        """As Engine.filter_states; m_t is added to the increments, so they are those of the true densities and sum
        to the log-likelihood.  Increments left at a raw device address are not supported (pass a tensor)."""
        if increments and out_increments is not None and not isinstance(out_increments, np.ndarray) \
                and not hasattr(out_increments, 'data_ptr'):
            raise NotImplementedError("increments at a raw device address: pass a numpy array or a tensor")
        self.emissions(par0, par1)
        rows, logc = Engine.filter_states(self, A, pi, weights=weights, dtype=dtype, probabilities=probabilities,
                                          increments=increments, out=out, out_increments=out_increments)
        if logc is not None:
            m = self.step_scales()
            on_tensor = out_increments is not None and hasattr(out_increments, 'data_ptr')
            if on_tensor:
                import torch
                self.sync()
            for k, l in enumerate(logc):
                mk = m[self.offsets[k]:self.offsets[k + 1]]
                if on_tensor:
                    l += torch.from_numpy(mk).to(device=l.device, dtype=l.dtype)
                else:
                    l += mk.astype(l.dtype)
        return rows, logc

    def viterbi(self, A, pi, par0=None, par1=None):
        self.emissions(par0, par1)
        return Engine.viterbi(self, A, pi)

    def viterbi_u8(self, A, pi, par0=None, par1=None, out=None):
        self.emissions(par0, par1)
        return Engine.viterbi_u8(self, A, pi, out=out)

    def path_logprob(self, paths, models):
        """(S, K) joint log-probabilities of given paths; one emission pass per model."""
        models = list(models)
        if not models:
            raise ValueError("path_logprob needs at least one model")
        out = np.empty((len(models), len(self.lengths)))
        for s, m in enumerate(models):
            if len(m) != 4:
                raise ValueError("model %d: expected an (A, pi, means, covariances) tuple" % s)
            self.emissions(m[2], m[3])
            out[s] = Engine.path_logprob(self, paths, [(m[0], m[1], None, None)])[0] + self._shift
        return out

    def decode_logprob(self, A, pi, par0=None, par1=None, method='viterbi'):
        self.emissions(par0, par1)
        return Engine.decode_logprob(self, A, pi, method=method) + self._shift

    def decode_runs(self, A, pi, par0=None, par1=None, method='viterbi', stats=False):
        self.emissions(par0, par1)
        return Engine.decode_runs(self, A, pi, method=method, stats=stats)

    def sample_paths_dev(self, A, pi, par0, par1, stats_dev, u=None, seed=0, want_paths=False):
        self.emissions(par0, par1)
        return Engine.sample_paths_dev(self, A, pi, None, None, stats_dev, u=u, seed=seed, want_paths=want_paths)

    def sample_paths(self, A, pi, par0=None, par1=None, u=None, seed=0, want_paths=True):
        self.emissions(par0, par1)
        return Engine.sample_paths(self, A, pi, u=u, seed=seed, want_paths=want_paths)


class GmmEngine(MvnEngine):
    """Engine for gaussian-mixture emissions per state (kind 'gaussian_mixture'): observations
    as for MvnEngine, a model is (A, pi, par0, par1) with par0 (n, M, 1 + D) -- column 0 the mixture weight, the rest
    the mean of component (i, c) -- and par1 (n, M, D, D) covariances or (n, M, D) variances.  Everything runs as in
    MvnEngine on the explicit rows of the mixture densities (bhmm_gmm_emissions); an E-step makes those rows with the
    log responsibilities of the components, runs ONE pass of the recursions that leaves gamma on the device, and
    takes the per-component moments from gamma and the responsibilities (bhmm_gmm_moments)."""

    def __init__(self, device=0, stream=None):
        MvnEngine.__init__(self, device, stream)
        self.ncomponents = 0       # of the last emissions
        self._resp = False         # the context holds log responsibilities of the loaded rows

    def _set(self, ptr, off, nstates, D, chunk, on_device):
        MvnEngine._set(self, ptr, off, nstates, D, chunk, on_device)
        self.kind = 'gaussian_mixture'
        self._resp = False

    def set_observations(self, kind, observations, nstates, nsymbols=0, chunk=0):
        """observations: list of (T_k, D) float arrays, 1 <= D <= 64."""
        if kind != 'gaussian_mixture':
            raise ValueError("a GmmEngine holds observations of kind 'gaussian_mixture', not %r" % (kind,))
        MvnEngine.set_observations(self, 'mvgaussian', observations, nstates, chunk=chunk)

    def set_observations_device(self, kind, dev_ptr, offsets, nstates, nsymbols=0, chunk=0, dimension=None):
        if kind != 'gaussian_mixture':
            raise ValueError("a GmmEngine holds observations of kind 'gaussian_mixture', not %r" % (kind,))
        MvnEngine.set_observations_device(self, 'mvgaussian', dev_ptr, offsets, nstates, chunk=chunk,
                                          dimension=dimension)

    def set_observations_lagged(self, *args, **kwargs):
        raise NotImplementedError("lagged views are cut on the host for multivariate observations")

    @property
    def stats_size(self):
        """The explicit kind's vector followed by the n M moment blocks of the last covariance type (full before
        any)."""
        from .output_models.mvgaussian import moment_stride
        return self._ctx_stats_size() + self.nstates * max(self.ncomponents, 1) * \
            moment_stride(self.dimension, self._cov_last or 'full')

    def _params(self, par0, par1):
        """(par0 (n, M, 1 + D), covariances, covariance type) of one model, shapes checked."""
        if self.dimension == 0:
            raise ValueError("no observations loaded")
        if par0 is None or par1 is None:
            raise ValueError("gaussian-mixture emissions need par0 = [weights | means] and covariances")
        n, D = self.nstates, self.dimension
        p0, cov = _lib.f64(par0), _lib.f64(par1)
        if p0.ndim != 3 or p0.shape[0] != n or p0.shape[1] < 1 or p0.shape[2] != 1 + D:
            raise ValueError("par0 must be (%d, M, %d): the weight and the mean of every component, not %r"
                             % (n, 1 + D, p0.shape))
        M = p0.shape[1]
        if n * M > 4096:
            raise ValueError("at most 4096 components in all are supported, not %d x %d" % (n, M))
        if cov.shape == (n, M, D, D):
            return p0, cov, 'full'
        if cov.shape == (n, M, D):
            return p0, cov, 'diag'
        raise ValueError("covariances must be (%d, %d, %d, %d) or (%d, %d, %d), not %r"
                         % (n, M, D, D, n, M, D, cov.shape))

    def emissions(self, par0, par1, force=False, want_resp=False):
        """Make the mixture rows of (par0, par1) the context's observations, unless the loaded ones were made from
        the same parameters (force: make them anyway; want_resp: with the log responsibilities of the components,
        which are made again when the loaded rows came without them or a moments call has used them up).  Returns
        the covariance type."""
        p0, cov, ctype = self._params(par0, par1)
        ld = self._loaded
        if not force and ld is not None and ld[0].shape == p0.shape and ld[1].shape == cov.shape \
                and np.array_equal(ld[0], p0) and np.array_equal(ld[1], cov) and (self._resp or not want_resp):
            return ctype
        self._loaded = self._shift = self._m_t = self._moments = None   # (the re-load ends the last E-step too)
        self._resp = False
        M = p0.shape[1]
        w = np.ascontiguousarray(p0[:, :, 0])
        mu = np.ascontiguousarray(p0[:, :, 1:])
        _lib.check(self._L.bhmm_gmm_emissions(self._h, int(M), _lib.dp(w), _lib.dp(mu), _lib.dp(cov),
                                              _lib.COV_FULL if ctype == 'full' else _lib.COV_DIAG,
                                              1 if want_resp else 0))
        self._stage = None
        self._fetch = None
        shift = np.empty(len(self.lengths))
        _lib.check(self._L.bhmm_mvn_fetch_scale(self._h, _lib.dp(shift), None))
        self._shift = shift
        self._loaded = (p0.copy(), cov.copy())
        self.ncomponents = int(M)
        self._resp = bool(want_resp)
        return ctype

    def responsibilities(self):
        """The (sum T_k, n, M) buffer of the context, copied to the host (bhmm_gmm_fetch_resp; tests, diagnostics):
        log r_t(i,c) after emissions with want_resp, the weights gamma_t(i) r_t(i,c) after `moments`."""
        out = np.empty((int(self.offsets[-1]), self.nstates, self.ncomponents))
        _lib.check(self._L.bhmm_gmm_fetch_resp(self._h, _lib.dp(out)))
        return out

    def moments(self, gamma_dev, means=None, covariance_type='full'):
        """Packed per-component moments of the M-step (bhmm_gmm_moments) from posterior rows on this GPU: gamma_dev
        is the integer device address of (sum T_k, nstates) float64 rows, or an object with data_ptr(); means
        (n, M, D) to take them about (default: those of the loaded emissions).  Uses up the log responsibilities."""
        from .output_models.mvgaussian import moment_stride
        if self._loaded is None:
            raise ValueError("no emissions made yet")
        n, M, D = self.nstates, self.ncomponents, self.dimension
        mu = _lib.f64(self._loaded[0][:, :, 1:] if means is None else means)
        if mu.shape != (n, M, D):
            raise ValueError("means must be (%d, %d, %d)" % (n, M, D))
        mu = np.ascontiguousarray(mu)
        ptr = gamma_dev.data_ptr() if hasattr(gamma_dev, 'data_ptr') else int(gamma_dev)
        out = np.empty(n * M * moment_stride(D, covariance_type))
        self._resp = False
        _lib.check(self._L.bhmm_gmm_moments(self._h, ctypes.c_void_p(ptr), _lib.dp(mu),
                                            _lib.COV_FULL if covariance_type == 'full' else _lib.COV_DIAG,
                                            _lib.dp(out)))
        return out

    def path_moments(self, *args, **kwargs):
        raise NotImplementedError("a hidden path has no moments per state under gaussian-mixture emissions: "
                                  "draw_components gives those of its components")

    def sample_paths_moments(self, *args, **kwargs):
        raise NotImplementedError("the Gibbs sweep of gaussian-mixture emissions is sample_paths_components")

    # -- the components of a hidden path ------------------------------
    def _component_moments(self):
        from .output_models.mvgaussian import moment_stride
        if self._loaded is None:
            raise ValueError("no emissions made yet")
        ctype = 'full' if self._loaded[1].ndim == 4 else 'diag'
        return np.empty(self.nstates * self.ncomponents * moment_stride(self.dimension, ctype))

    def draw_components(self, paths, seed=0, want_labels=True):
        """For every step of a given hidden path a component c_t ~ r_t(s_t, .) under the loaded emissions
        (bhmm_gmm_path_components), and the packed moments of the labels s_t M + c_t about the component means of
        those emissions, in the layout of `moments`.  `paths` as path_logprob takes them.  Returns (labels or None,
        moments): labels a flat int32 array.  Only the M densities of the state a step is in are formed, and no
        responsibilities are kept or needed.  A state outside [0, nstates) raises ValueError.  Labels and moments
        are a function of (observations, path, parameters, seed, stream offsets) alone: bitwise the same from call
        to call and for every form of the same path.  Stream offsets (set_stream_offsets, after the emissions: a
        re-load forgets them) place the trajectories in the random stream as they do for the path draw (read-only
        option "gmm_draw_ms": device time of the draw)."""
        out = self._component_moments()
        if isinstance(paths, (list, tuple)):
            paths = self._concat_paths(paths)
        ptr, u8, on_dev = self._path_arg(paths, loaded=True)
        labels = np.empty(int(self.offsets[-1]), dtype=np.int32) if want_labels else None
        _lib.check(self._L.bhmm_gmm_path_components(self._h, ctypes.c_void_p(int(ptr)), 1 if u8 else 0, on_dev,
                                                    ctypes.c_uint64(int(seed)), _lib.ip(labels), _lib.dp(out)))
        return labels, out

    def sample_paths_components(self, A, pi, par0, par1, u=None, seed=0, want_paths=False, want_labels=False):
        """Gibbs hidden-path step under (A, pi, par0, par1) followed by the component draw of draw_components on
        the drawn path, where it lies on the device, and the moments of the labels (bhmm_gmm_sample_paths).  Makes
        the emissions first when the loaded ones are not those of (par0, par1).  Returns (paths or None, labels or
        None, C int64 (n, n), n0 int64 (n,), moments); paths, C and n0 are those of sample_paths for the same
        arguments; paths and labels are lists of one int32 array per trajectory and cross the link only when
        asked for."""
        self.emissions(par0, par1)
        out = self._component_moments()
        A, pi, _, _ = self._model_ptrs(A, pi, None, None)
        n = self.nstates
        total = int(self.offsets[-1])
        paths = np.empty(total, dtype=np.int32) if want_paths else None
        labels = np.empty(total, dtype=np.int32) if want_labels else None
        C = np.zeros((n, n), dtype=np.int64)
        n0 = np.zeros(n, dtype=np.int64)
        uu = _lib.f64(np.concatenate(u)) if u is not None else None
        _lib.check(self._L.bhmm_gmm_sample_paths(self._h, A, pi, _lib.dp(uu), ctypes.c_uint64(int(seed)),
                                                 _lib.ip(paths), _lib.ip(labels), _lib.lp(C), _lib.lp(n0),
                                                 _lib.dp(out)))

        def split(flat):
            if flat is None:
                return None
            return [flat[self.offsets[k]:self.offsets[k + 1]] for k in range(len(self.lengths))]
        return split(paths), split(labels), C, n0, out

    # -- E-step --------------------------------------------------------------------------
    def estep_launch(self, A, pi, par0=None, par1=None, stats_dev=None, store_gamma=False, single=False):
        """One E-step: mixture rows with log responsibilities, ONE pass of the recursions that leaves the posterior
        rows on the device (Engine.posterior_marginals), the per-component moments from both.  Synchronous."""
        if stats_dev is not None:
            raise NotImplementedError("gaussian-mixture E-steps keep their statistics in the context")
        if single:
            raise NotImplementedError("gaussian-mixture E-steps run in float64")
        ctype = self.emissions(par0, par1, want_resp=True)
        import torch
        total = int(self.offsets[-1])
        g = self._gamma_dev
        if g is None or g.numel() != total * self.nstates or g.device.index != self.device:
            g = self._gamma_dev = torch.empty(total * self.nstates, dtype=torch.float64,
                                              device='cuda:%d' % self.device)
        Engine.posterior_marginals(self, A, pi, out=g.data_ptr())
        self._moments = self.moments(g.data_ptr(), None, ctype)
        self._cov_last = ctype

    def estep_fetch(self):
        if self._moments is None:
            raise ValueError("no E-step has run on these observations")
        res = Engine.estep_fetch(self)
        return EStepResult('gaussian_mixture', self.nstates, self.ncomponents, self._shifted(res.packed),
                           res.logL_k + self._shift, self.dimension, self._cov_last)

    def unpack(self, packed, logL_k=None):
        return EStepResult('gaussian_mixture', self.nstates, self.ncomponents, np.asarray(packed), logL_k,
                           self.dimension, self._cov_last or 'full')


class PoissonEngine(MvnEngine):
    """Engine for Poisson count emissions (kind 'poisson'): the observations are (T_k, D) arrays
    of counts (integer or float dtype; held as float64 on the device), a model is (A, pi, rates (n, D), None).
    Everything runs as in MvnEngine on the explicit rows bhmm_pois_emissions makes; the step scales are m_t + c_t with
    c_t = -sum_d log(x_td !), so every log-likelihood, path log-probability and filter increment is that of the
    complete density.  An E-step makes the rows, runs ONE pass of the recursions that leaves gamma on the device and
    takes the moments about the loaded rates (bhmm_mvn_moments with diagonal second moments, which go unused)."""

    def _set(self, ptr, off, nstates, D, chunk, on_device):
        MvnEngine._set(self, ptr, off, nstates, D, chunk, on_device)
        self.kind = 'poisson'

    def set_observations(self, kind, observations, nstates, nsymbols=0, chunk=0):
        """observations: list of (T_k, D) arrays of counts, 1 <= D <= 64; a negative or fractional value is refused."""
        if kind != 'poisson':
            raise ValueError("a PoissonEngine holds observations of kind 'poisson', not %r" % (kind,))
        from .output_models.poisson import check_observation
        MvnEngine.set_observations(self, 'mvgaussian', [check_observation(o) for o in observations], nstates,
                                   chunk=chunk)

    def set_observations_device(self, kind, dev_ptr, offsets, nstates, nsymbols=0, chunk=0, dimension=None):
        """The same for a (sum T_k, D) row-major float64 buffer of counts already on this GPU; its values are checked
        by the kernel that makes the rows (ValueError from the first model call)."""
        if kind != 'poisson':
            raise ValueError("a PoissonEngine holds observations of kind 'poisson', not %r" % (kind,))
        MvnEngine.set_observations_device(self, 'mvgaussian', dev_ptr, offsets, nstates, chunk=chunk,
                                          dimension=dimension)

    def set_observations_lagged(self, *args, **kwargs):
        raise NotImplementedError("lagged views are cut on the host for multivariate observations")

    @property
    def stats_size(self):
        """The explicit kind's vector followed by the moment block (diagonal second moments)."""
        from .output_models.mvgaussian import moment_stride
        return self._ctx_stats_size() + self.nstates * moment_stride(self.dimension, 'diag')

    def _params(self, par0, par1):
        """rates (n, D) of one model, checked (before anything loaded is given up)."""
        if self.dimension == 0:
            raise ValueError("no observations loaded")
        if par0 is None:
            raise ValueError("poisson emissions need rates")
        if par1 is not None:
            raise ValueError("poisson emissions take par0 = rates and par1 = None")
        n, D = self.nstates, self.dimension
        rates = _lib.f64(par0)
        if rates.shape != (n, D):
            raise ValueError("rates must be (%d, %d), not %r" % (n, D, rates.shape))
        if not np.all(np.isfinite(rates)) or np.any(rates < 0.0):
            raise ValueError("rates must be finite and not negative")
        return rates

    def emissions(self, par0, par1=None, force=False):
        """Make the emission rows of `rates` the context's observations, unless the loaded ones were made from the
        same rates (force: make them anyway).  Returns 'diag', the layout of the moments."""
        rates = self._params(par0, par1)
        ld = self._loaded
        if not force and ld is not None and np.array_equal(ld[0], rates):
            return 'diag'
        self._loaded = self._shift = self._m_t = self._moments = None   # (the re-load ends the last E-step too)
        _lib.check(self._L.bhmm_pois_emissions(self._h, _lib.dp(rates)))
        self._stage = None
        self._fetch = None
        shift = np.empty(len(self.lengths))
        _lib.check(self._L.bhmm_mvn_fetch_scale(self._h, _lib.dp(shift), None))
        self._shift = shift
        self._loaded = (rates.copy(), None)
        return 'diag'

    def sample_paths_moments(self, *args, **kwargs):
        raise NotImplementedError("Poisson count emissions have no Gibbs sweep yet")

    # -- E-step --------------------------------------------------------------------------
    def estep_launch(self, A, pi, par0=None, par1=None, stats_dev=None, store_gamma=False, single=False):
        """One E-step: rows, ONE pass of the recursions that leaves the posterior rows on the device
        (Engine.posterior_marginals), the moments from them about the loaded rates.  Synchronous."""
        if stats_dev is not None:
            raise NotImplementedError("poisson E-steps keep their statistics in the context")
        if single:
            raise NotImplementedError("poisson E-steps run in float64")
        self.emissions(par0, par1)
        import torch
        total = int(self.offsets[-1])
        g = self._gamma_dev
        if g is None or g.numel() != total * self.nstates or g.device.index != self.device:
            g = self._gamma_dev = torch.empty(total * self.nstates, dtype=torch.float64,
                                              device='cuda:%d' % self.device)
        Engine.posterior_marginals(self, A, pi, out=g.data_ptr())
        self._moments = self.moments(g.data_ptr(), self._loaded[0], 'diag')
        self._cov_last = 'diag'

    def estep_fetch(self):
        if self._moments is None:
            raise ValueError("no E-step has run on these observations")
        res = Engine.estep_fetch(self)
        return EStepResult('poisson', self.nstates, 0, self._shifted(res.packed), res.logL_k + self._shift,
                           self.dimension)

    def unpack(self, packed, logL_k=None):
        return EStepResult('poisson', self.nstates, 0, np.asarray(packed), logL_k, self.dimension)


def stack_models(kind, nstates, nsymbols, models):
    """The stacked model arrays of bhmm_score (include/bhmm_amd.h): A (S, n, n), pi (S, n), par0 (S, n) means /
    (S, n, M) emission matrices / None, par1 (S, n) sigmas / None, each C-contiguous float64."""
    models = list(models)
    if not models:
        raise ValueError("score needs at least one model")
    n, M = int(nstates), int(nsymbols)
    A, pi, p0, p1 = [], [], [], []
    for i, m in enumerate(models):
        if len(m) != 4:
            raise ValueError("model %d: expected an (A, pi, par0, par1) tuple" % i)
        a, p, e0, e1 = m
        a = np.asarray(a, dtype=np.float64)
        p = np.asarray(p, dtype=np.float64)
        if a.shape != (n, n) or p.shape != (n,):
            raise ValueError("model %d: A must be (%d, %d) and pi (%d,)" % (i, n, n, n))
        A.append(a)
        pi.append(p)
        if kind == 'gaussian':
            if e0 is None or e1 is None:
                raise ValueError("model %d: gaussian emissions need means and sigmas" % i)
            e0, e1 = np.asarray(e0, dtype=np.float64), np.asarray(e1, dtype=np.float64)
            if e0.shape != (n,) or e1.shape != (n,):
                raise ValueError("model %d: means and sigmas must be (%d,)" % (i, n))
            p0.append(e0)
            p1.append(e1)
        elif kind == 'discrete':
            if e0 is None:
                raise ValueError("model %d: discrete emissions need B" % i)
            e0 = np.asarray(e0, dtype=np.float64)
            if e0.shape != (n, M):
                raise ValueError("model %d: B must be (%d, %d)" % (i, n, M))
            p0.append(e0)
    st = lambda xs: np.ascontiguousarray(np.stack(xs)) if xs else None  # noqa: E731
    return st(A), st(pi), st(p0), st(p1)


class NativeComm(object):
    """The library's own communicator (include/bhmm_amd.h, section 2b): RCCL behind the C ABI, for
    callers that do not bring torch.distributed -- one all-reduce of the packed statistics per EM
    iteration / Gibbs sweep (maximum_likelihood.py:271-282 in distributed form).  Rank 0 calls
    NativeComm.unique_id() and hands the 128 bytes to the other ranks; every rank then constructs
    NativeComm(device, nranks, rank, uid) (a collective)."""

    def __init__(self, device, nranks=1, rank=0, uid=None):
        self._L = _lib.load()
        if uid is None:
            if nranks != 1:
                raise ValueError("more than one rank: pass the unique id of rank 0")
            uid = NativeComm.unique_id()
        self._uid = ctypes.create_string_buffer(bytes(uid), 128)
        self._h = ctypes.c_void_p()
        _lib.check(self._L.bhmm_comm_init_rank(ctypes.byref(self._h), int(device), int(nranks), int(rank),
                                               ctypes.cast(self._uid, ctypes.c_void_p)))
        self.nranks, self.rank, self.device = int(nranks), int(rank), int(device)

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        _lib.check(_lib.load().bhmm_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p)))
        return buf.raw

    def allreduce_stats(self, engine, dev_ptr, count):
        """In-place sum over the ranks of `count` doubles at device address dev_ptr, enqueued on the
        engine's stream (no host synchronisation)."""
        _lib.check(self._L.bhmm_ctx_allreduce_stats(engine._h, self._h, ctypes.c_void_p(int(dev_ptr)),
                                                    ctypes.c_int64(int(count))))

    def close(self):
        if self._h:
            self._L.bhmm_comm_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def synth_observations(kind, obs_dev, A, pi, par0, par1, K, T, seed, device=0, stream=None,
                       states_dev=None, first_traj=0):
    """Draw K synthetic trajectories of T steps on the GPU into the device buffer at address
    `obs_dev` (K*T doubles for 'gaussian', int32 for 'discrete'); see bhmm_synth_observations in
    include/bhmm_amd.h.  states_dev: optional device address of K*T bytes for the hidden paths.
    first_traj: index of this call's first trajectory in a larger (sharded) set -- the slice is then
    exactly what one call for the whole set would have drawn for these trajectories."""
    L = _lib.load()
    _lib.require_device()
    A = _lib.f64(A)
    n = A.shape[0]
    p0 = _lib.f64(par0)
    p1 = _lib.f64(par1) if par1 is not None else None
    M = p0.shape[1] if kind == 'discrete' else 0
    _lib.check(L.bhmm_synth_observations_at(
        ctypes.c_void_p(int(obs_dev)), ctypes.c_void_p(int(states_dev)) if states_dev else None,
        int(device), ctypes.c_void_p(stream) if stream else None, _KINDS[kind], _lib.dp(A),
        _lib.dp(_lib.f64(pi)), _lib.dp(p0), _lib.dp(p1), int(n), int(M), int(K), int(T),
        ctypes.c_uint64(int(seed)), int(first_traj)))
