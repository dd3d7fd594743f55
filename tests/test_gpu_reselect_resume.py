"""GPU: ``--reselect-every 1 --keep-optimizer`` -- a run that re-selects its inducing patches at the start of its second period is the same run
whether that period follows the first in one process or starts a NEW PROCESS from the first period's checkpoint and sidecar: the same checkpoint
arrays, the same sidecar (moments, step count, prior patches) and the same log.csv values, bit for bit.  The helpers are those of
tests/test_gpu_resume.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_resume as tr

pytestmark = pytest.mark.gpu

FLAGS = ["--optimizer", "Adam", "--reselect-every", "1", "--reselect-images", "30", "--keep-optimizer"]


def test_resumed_run_reselects_as_the_uninterrupted_run(ctx, tmp_path):
    log_dir = str(tmp_path)
    data = tr._arrays()
    np.savez(os.path.join(log_dir, "arrays.npz"), **data)
    tr._run("whole", FLAGS, 2, log_dir, data)
    tr._run("first", FLAGS, 1, log_dir, data)
    argv = ["--name", "second", "--log-dir", log_dir, "--load-model", "first"] + tr.BASE + FLAGS
    env = dict(os.environ, PYTHONPATH=tr.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", tr.RUNNER, os.path.join(log_dir, "arrays.npz")] + argv, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.count("re-selected") == 2, out.stdout          # both layers, at step 3
    whole, first, second = (tr._checkpoint(log_dir, n) for n in ("whole", "first", "second"))
    assert whole["global_step"] == 6 and second["global_step"] == 6
    tr._same_checkpoint(whole, second)
    with np.load(os.path.join(log_dir, "whole.opt.npz")) as a, np.load(os.path.join(log_dir, "second.opt.npz")) as b, \
            np.load(os.path.join(log_dir, "first.opt.npz")) as f:
        assert set(a.files) == set(b.files) == set(f.files) and int(a["opt/t"]) == 6          # the sidecar keeps its key set
        for k in a.files:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        assert not np.array_equal(a["prior/0/Z"], f["prior/0/Z"])                              # the prior's patches were chosen again
    assert set(whole) == set(first)                                                            # ... and the checkpoint its key set
    head_w, rows_w = tr._rows(log_dir, "whole")
    head_s, rows_s = tr._rows(log_dir, "second")
    assert head_w == head_s == ["global_step", "test_accuracy", "train_log_likelihood"]        # the same loggers
    assert len(rows_w) == 2 and rows_s == rows_w[1:]


def test_without_the_flag_nothing_is_reselected(ctx, tmp_path):
    log_dir = str(tmp_path)
    data = tr._arrays()
    tr._run("plain", ["--optimizer", "Adam", "--keep-optimizer"], 2, log_dir, data)
    tr._run("again", ["--optimizer", "Adam", "--keep-optimizer", "--reselect-every", "0"], 2, log_dir, data)
    tr._same_checkpoint(tr._checkpoint(log_dir, "plain"), tr._checkpoint(log_dir, "again"))
    tr._run("every", FLAGS, 2, log_dir, data)
    assert not np.array_equal(tr._checkpoint(log_dir, "plain")["DGP/layers/0/feature/Z"], tr._checkpoint(log_dir, "every")["DGP/layers/0/feature/Z"])
