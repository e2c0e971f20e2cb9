"""Mixed-precision EM over two ranks (gloo, CPU test double): one rank's single-precision E-steps
verify, the other's always fall back to fp64.  What ran differs between the ranks, so the
stopping rule must not depend on it: both ranks have to stop at the same iteration with the same
results (a rank-local rule would leave one rank waiting in an all-reduce -- the collective's
timeout turns that into a failure here instead of a hang)."""
import datetime
import os
import socket
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _make_engine_class():
    from oracle_engine import OracleEngine

    class RankEngine(OracleEngine):
        """single=True: rank 0 'runs fp32' (f32_used = 1), rank 1 'falls back' (exact fp64 statistics,
        f32_used = 0).  Rank 0's fp32 log-likelihood is exact on the first call (so the initial gap, and
        with it the switch threshold, is the EM accuracy) and 1.0 too high afterwards: at the switch the
        fp64 likelihood then lies below the previous (fp32) one, which a rule comparing across
        precisions would take for convergence -- on rank 1 only, where both iterations 'ran' fp64."""
        bias = 1.0

        def __init__(self, device=0):
            super(RankEngine, self).__init__(device)
            import torch.distributed as dist
            self.rank = dist.get_rank()
            self.used = 0.0

        def estep(self, A, pi, par0=None, par1=None, store_gamma=False, **kw):
            res = super(RankEngine, self).estep(A, pi, par0, par1, store_gamma=store_gamma)
            self.used = 1.0 if (kw.get('single') and self.rank == 0) else 0.0
            if self.used:
                self.nsingle = getattr(self, 'nsingle', 0) + 1
                packed = res.packed.copy()
                packed[0] += self.bias if self.nsingle > 1 else 0.0
                res = self.unpack(packed, res.logL_k)
            return res

        def get_option(self, name):
            assert name == 'f32_used'
            return self.used
    return RankEngine


def _worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch.distributed as dist
    import bhmm_amd
    from test_host_logic import _gauss_problem
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    obs, init = _gauss_problem(seed=3, K=6, T=400)
    est = bhmm_amd.MaximumLikelihoodEstimator(obs, 3, initial_model=init, reversible=False, accuracy=1e-6,
                                              maxit=200, engine_factory=_make_engine_class(),
                                              estep_precision='mixed')
    est.fit()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), L=est.likelihoods,
             prec=np.array(est.estep_precisions), A=est.transition_matrix)
    dist.destroy_process_group()


def test_two_rank_mixed_stops_together():
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, _free_port(), d), nprocs=2, join=True)
        r0 = np.load(os.path.join(d, "rank0.npz"))
        r1 = np.load(os.path.join(d, "rank1.npz"))
    assert len(r0["L"]) == len(r1["L"])
    np.testing.assert_array_equal(r0["L"], r1["L"])
    np.testing.assert_array_equal(r0["A"], r1["A"])
    # what ran differs (rank 1 always fell back), the iterations do not
    assert 'float32' in list(r0["prec"]) and 'float32' not in list(r1["prec"])
    assert list(r0["prec"][-2:]) == ['float64', 'float64']
