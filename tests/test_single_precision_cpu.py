"""Single-precision E-step (BHMM_FLAG_SINGLE), host side on CPU: the flag constant, the
estimator's `estep_precision` keyword, and the control logic of the mixed-precision EM loop,
driven by a test double of the engine that records which E-steps asked for single precision."""
import os
import re

import numpy as np
import pytest

import bhmm_amd
from bhmm_amd import _lib
from bhmm_amd.estimators.maximum_likelihood import MaximumLikelihoodEstimator
from oracle_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the double adds to the log-likelihood of a "single-precision" E-step: an fp32 result that is
# off by more than the EM accuracy, so that a convergence test across precisions would misfire
SINGLE_BIAS = 1e-3


class RecordingEngine(OracleEngine):
    """OracleEngine that accepts `single=` and records, per E-step, whether the keyword was
    given at all and whether it asked for single precision."""

    def __init__(self, device=0):
        super(RecordingEngine, self).__init__(device)
        self.calls = []

    def estep(self, A, pi, par0=None, par1=None, store_gamma=False, **kw):
        self.calls.append(kw.get('single', None))
        res = super(RecordingEngine, self).estep(A, pi, par0, par1, store_gamma=store_gamma)
        if kw.get('single'):
            packed = res.packed.copy()
            packed[0] += SINGLE_BIAS
            res = self.unpack(packed, res.logL_k)
        return res


def _two_state_discrete(T=3000, seed=1):
    rng = np.random.default_rng(seed)
    A = np.array([[0.95, 0.05], [0.1, 0.9]])
    B = np.array([[0.7, 0.2, 0.1], [0.1, 0.3, 0.6]])
    s, obs = 0, np.empty(T, dtype=np.int64)
    for t in range(T):
        obs[t] = rng.choice(3, p=B[s])
        s = rng.choice(2, p=A[s])
    init = bhmm_amd.discrete_hmm([0.5, 0.5], np.array([[0.8, 0.2], [0.3, 0.7]]),
                                 np.array([[0.5, 0.3, 0.2], [0.2, 0.3, 0.5]]))
    return [obs[:T // 2], obs[T // 2:]], init


def _fit(precision, engines, accuracy=1e-6):
    obs, init = _two_state_discrete()

    def factory(device):
        e = RecordingEngine(device)
        engines.append(e)
        return e
    kw = {} if precision is None else {'estep_precision': precision}
    est = MaximumLikelihoodEstimator(obs, 2, initial_model=init, output='discrete', accuracy=accuracy,
                                     maxit=500, engine_factory=factory, **kw)
    est.fit()
    return est


def test_flag_single_matches_header():
    with open(os.path.join(ROOT, 'include', 'bhmm_amd.h')) as f:
        m = re.search(r'#define\s+BHMM_FLAG_SINGLE\s+(\d+)', f.read())
    assert m is not None
    assert int(m.group(1)) == _lib.FLAG_SINGLE
    assert _lib.FLAG_SINGLE & _lib.FLAG_STORE_GAMMA == 0


@pytest.mark.parametrize('bad', ['float16', 'double', '', None, 32])
def test_estep_precision_validation(bad):
    obs, init = _two_state_discrete(T=100)
    with pytest.raises(ValueError):
        MaximumLikelihoodEstimator(obs, 2, initial_model=init, output='discrete',
                                   engine_factory=OracleEngine, estep_precision=bad)


def test_default_never_passes_single():
    for precision in (None, 'float64'):
        engines = []
        est = _fit(precision, engines)
        assert all(c is None for c in engines[0].calls)          # the keyword is not even given
        assert est.estep_precisions == ['float64'] * len(est.likelihoods)


def test_float32_asks_every_estep():
    engines = []
    est = _fit('float32', engines)
    calls = engines[0].calls
    assert len(calls) == len(est.likelihoods) and all(c is True for c in calls)
    # the double has no get_option: what was asked for is recorded
    assert est.estep_precisions == ['float32'] * len(est.likelihoods)


def test_mixed_control_logic():
    engines = []
    est = _fit('mixed', engines)
    calls = engines[0].calls
    prec = est.estep_precisions
    n = len(est.likelihoods)
    assert len(prec) == n
    # iteration 0: one fp32 and one fp64 E-step on the initial model; the M-step takes the fp64 one
    assert calls[0] is True and calls[1] is None
    assert prec[0] == 'float64'
    # then fp32 first, fp64 from the switch on, never back
    rest = calls[2:]
    k = rest.index(None)
    assert k >= 1 and all(c is True for c in rest[:k]) and all(c is None for c in rest[k:])
    assert 'float32' in prec
    first64 = prec.index('float64', 1)
    assert all(p == 'float32' for p in prec[1:first64]) and all(p == 'float64' for p in prec[first64:])
    # convergence on consecutive fp64 likelihoods only: the last two iterations ran fp64 and the
    # stopping rule holds between them
    assert prec[-2:] == ['float64', 'float64']
    assert est.likelihoods[-1] - est.likelihoods[-2] < 1e-6
    # the returned likelihood / counts / model are fp64 ones: the same as a plain fp64 fit
    engines64 = []
    ref = _fit('float64', engines64)
    assert abs(est.likelihood - ref.likelihood) <= 1e-6 * abs(ref.likelihood)
    np.testing.assert_allclose(est.transition_matrix, ref.transition_matrix, atol=1e-4)
    np.testing.assert_allclose(est.output_model.output_probabilities,
                               ref.output_model.output_probabilities, atol=1e-4)


def test_mixed_switch_threshold_uses_initial_gap():
    """The switch happens at the first fp32 increase below max(accuracy, 10 |L32 - L64|): with the
    double's bias of 1e-3 the fp32 phase ends once an iteration gains less than 1e-2."""
    engines = []
    est = _fit('mixed', engines, accuracy=1e-8)
    prec = est.estep_precisions
    first64 = prec.index('float64', 1)
    L = est.likelihoods
    # every fp32 iteration after the first gained at least 1e-2 over its predecessor (as seen in fp32)
    for it in range(1, first64):
        assert L[it] - L[it - 1] >= 10 * SINGLE_BIAS - 1e-12
