"""GPU: ``--keep-optimizer`` -- a run that is interrupted after a period and resumed in a NEW PROCESS from its checkpoint and sidecar is the
run that was not interrupted: the same checkpoint arrays, the same sidecar and the same log.csv values, bit for bit, under Adam (with device
augmentation and clipping on, across a learning-rate decay boundary) and under NatGrad; and without the flag it is not."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

from deepcgp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--data", "unused", "-M", "6,6", "--feature-maps", "2", "--filter-sizes", "3,3", "--strides", "1,1", "--batch-size", "4", "--num-samples", "2",
        "--test-every", "3", "--lr-decay-steps", "4"]
EXTRA = {"Adam": ["--optimizer", "Adam", "--augment-shift", "1", "--augment-flip", "--clip-norm", "5"], "NatGrad": ["--optimizer", "NatGrad"]}
# the resumed period, in a process of its own: argv = the arrays' file, then the flags
RUNNER = """
import sys
import numpy as np
from deepcgp_amd.experiment import ArrayExperiment, read_args
z = np.load(sys.argv[1])
exp = ArrayExperiment(read_args(sys.argv[2:]), z["Xtr"], z["Ytr"], z["Xte"], z["Yte"])
assert exp.global_step == 3
try:
    exp.train_step()
finally:
    exp.conclude()
exp.model.close()
"""


def _arrays():
    X, Y = syn.make_batch((8, 8, 1), 52, seed=11)
    X = X.reshape(52, 8, 8, 1)
    return dict(Xtr=X[:40], Ytr=Y[:40], Xte=X[40:], Yte=Y[40:])


def _run(name, flags, periods, log_dir, data):
    from deepcgp_amd.experiment import ArrayExperiment, read_args
    np.random.seed(0)          # (the inducing patches of a fresh model are cut with the global generator)
    exp = ArrayExperiment(read_args(["--name", name, "--log-dir", log_dir] + BASE + flags), data["Xtr"], data["Ytr"], data["Xte"], data["Yte"])
    try:
        for _ in range(periods):
            exp.train_step()
    finally:
        exp.conclude()
    exp.model.close()
    return exp


def _rows(log_dir, name):
    with open(os.path.join(log_dir, name, "log.csv"), newline="") as f:
        rows = list(csv.reader(f))
    return rows[0][1:], [r[1:] for r in rows[1:]]          # (without the entry counter, which starts again with a run)


def _checkpoint(log_dir, name):
    return np.load(os.path.join(log_dir, name + ".npy"), allow_pickle=True).item()


def _same_checkpoint(a, b):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("optimizer", ["Adam", "NatGrad"])
def test_resumed_run_is_the_uninterrupted_run(ctx, tmp_path, optimizer):
    log_dir = str(tmp_path)
    data = _arrays()
    np.savez(os.path.join(log_dir, "arrays.npz"), **data)
    flags = EXTRA[optimizer] + ["--keep-optimizer"]
    _run("whole", flags, 2, log_dir, data)
    _run("first", flags, 1, log_dir, data)
    assert os.path.exists(os.path.join(log_dir, "first.opt.npz"))
    argv = ["--name", "second", "--log-dir", log_dir, "--load-model", "first"] + BASE + flags
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", RUNNER, os.path.join(log_dir, "arrays.npz")] + argv, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    whole, second = _checkpoint(log_dir, "whole"), _checkpoint(log_dir, "second")
    assert whole["global_step"] == 6 and second["global_step"] == 6
    _same_checkpoint(whole, second)
    with np.load(os.path.join(log_dir, "whole.opt.npz")) as a, np.load(os.path.join(log_dir, "second.opt.npz")) as b:
        assert set(a.files) == set(b.files) and int(a["opt/t"]) == 6
        for k in a.files:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    head_w, rows_w = _rows(log_dir, "whole")
    head_f, rows_f = _rows(log_dir, "first")
    head_s, rows_s = _rows(log_dir, "second")
    print(head_w, rows_w, rows_f, rows_s)
    want_head = ["global_step", "test_accuracy", "train_log_likelihood"] + (["grad_norm"] if optimizer == "Adam" else [])
    assert head_w == head_f == head_s == want_head
    assert len(rows_w) == 2 and rows_f == rows_w[:1] and rows_s == rows_w[1:]          # the printed values, character for character
    assert rows_w[0] != rows_w[1]


def test_resume_without_the_state_goes_elsewhere(ctx, tmp_path):
    """The same Adam resume without --keep-optimizer: zero moments, t = 1 and the first minibatches again -- another q_mu."""
    log_dir = str(tmp_path)
    data = _arrays()
    flags = EXTRA["Adam"] + ["--keep-optimizer"]
    _run("whole", flags, 2, log_dir, data)
    _run("first", flags, 1, log_dir, data)
    _run("kept", flags + ["--load-model", "first"], 1, log_dir, data)
    _run("lost", EXTRA["Adam"] + ["--load-model", "first"], 1, log_dir, data)
    assert not os.path.exists(os.path.join(log_dir, "lost.opt.npz"))
    whole, kept, lost = (_checkpoint(log_dir, n) for n in ("whole", "kept", "lost"))
    _same_checkpoint(whole, kept)
    assert lost["global_step"] == 6
    assert not np.array_equal(lost["DGP/layers/0/q_mu"], whole["DGP/layers/0/q_mu"])
    assert not np.array_equal(lost["DGP/layers/1/q_mu"], whole["DGP/layers/1/q_mu"])
