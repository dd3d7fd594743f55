"""CPU: the host side of the test-set evaluation -- the noise reordering of DGP_Base.evaluate, LogLikelihoodLogger's batching
and divisor (conv_gp/utils/tensorboard.py:15-42), and the C-ABI declarations of the two new entry points."""
import re

import numpy as np

from deepcgp_amd import device as dev
from deepcgp_amd.dgp import batched_noise
from deepcgp_amd.models import LogLikelihoodLogger, TestLogDensityLogger


def test_batched_noise_on_ragged_batches():
    S, N, D, bs = 3, 7, 4, 3
    z = np.arange(S * N * D, dtype=np.float64).reshape(S, N, D)
    flat = batched_noise([z, None], N, S, bs)
    assert flat[1] is None
    assert flat[0].shape == (S * N * D,)
    off = 0
    for lo in range(0, N, bs):              # batch b: its [S, n_b, D] table, then the next batch's
        n = min(bs, N - lo)
        table = flat[0][off:off + S * n * D].reshape(S, n, D)
        assert np.array_equal(table, z[:, lo:lo + n])
        off += S * n * D
    assert off == flat[0].size
    # one batch of the whole set is the [S, N, D] table itself; images one at a time are image-major
    assert np.array_equal(batched_noise([z], N, S, N)[0], z.reshape(-1))
    assert np.array_equal(batched_noise([z], N, S, 1)[0], z.transpose(1, 0, 2).reshape(-1))
    assert batched_noise(None, N, S, bs) is None


class _StubModel:
    """Records the ELBO calls of a logger; the ELBO of a batch is a function of its rows and seed."""

    def __init__(self, n):
        self.X = np.arange(n, dtype=np.float64).reshape(n, 1) * 0.5
        self.Y = np.arange(n, dtype=np.int32) % 10
        self.calls, self.pending, self.next = [], {}, 0
        self.max_in_flight = 0

    def value(self, X, seed):
        return float(X.sum()) + 1000.0 * seed

    def enqueue_log_likelihood(self, X, Y, zs=None, seed=0, scale=None):
        assert len(X) == len(Y) and scale is None
        self.calls.append((float(X[0, 0]) * 2, len(X), seed))
        t = self.next
        self.next += 1
        self.pending[t] = self.value(X, seed)
        self.max_in_flight = max(self.max_in_flight, len(self.pending))
        return t

    def collect_log_likelihood(self, t):
        assert t == min(self.pending), "tickets are collected in order"
        return self.pending.pop(t)


def test_log_likelihood_logger_batching_and_divisor():
    for n, batches in ((150, 3), (64, 1), (5000, 79), (6000, 79), (1, 1)):
        m = _StubModel(n)
        got = LogLikelihoodLogger()(m, seed=7)
        assert [c[2] for c in m.calls] == [7 + i for i in range(batches)]
        assert [c[0] for c in m.calls] == [64 * i for i in range(batches)]
        assert m.max_in_flight <= 4 and not m.pending
        want = 0.0
        for i in range(batches):                # the reference's slices of model.X and its divisor
            want += m.value(m.X[i * 64:(i + 1) * 64], 7 + i)
        assert got == want / (batches * 64)
    m = _StubModel(150)
    LogLikelihoodLogger()(m)
    assert [c[1] for c in m.calls] == [64, 64, 22]   # a short last batch, still divided by 3 * 64
    assert LogLikelihoodLogger.title == "train_log_likelihood"
    assert TestLogDensityLogger.title == "test_log_likelihood"


def test_logdensity_logger_uses_accuracy_logger_defaults():
    seen = {}

    class M:
        def evaluate(self, X, Y, S, batch_size, seed):
            seen.update(S=S, batch_size=batch_size, seed=seed, n=len(X))
            return {"mean_log_density": -1.25}
    X, Y = np.zeros((40, 3)), np.zeros(40, np.int32)
    assert TestLogDensityLogger(X, Y)(M(), seed=3) == -1.25
    assert seen == dict(S=5, batch_size=32, seed=3, n=40)


def _declaration(src, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_evaluate_declarations_parse():
    with open(dev.HEADER_PATH) as fh:
        src = fh.read()
    declared = dev.declared_symbols()
    for name, nargs in (("dcgp_model_predict_density", 9), ("dcgp_model_evaluate", 12)):
        assert name in declared
        args = _declaration(src, name)
        assert len(args) == nargs == len(dev._SIGS[name]), (name, args)
        assert args[0].startswith("dcgp_model*")
    assert "const int32_t* y" in _declaration(src, "dcgp_model_evaluate")
    assert "double* out_host" in _declaration(src, "dcgp_model_evaluate")
