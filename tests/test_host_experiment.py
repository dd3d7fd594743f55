"""The experiment driver's host side (deepcgp_amd/experiment.py, deepcgp_amd/utils/) without a GPU: the log's file format, the options.toml
writer, the index and learning-rate tables of a run, ``Experiment.train_step``'s control flow on a stub model, the flat shims, and the two
entry points of the run in include/dcgp.h (tests/test_host_cpu.py's symbol-table test then checks that the library exports them)."""
import argparse
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd import utils
from deepcgp_amd.experiment import Experiment, read_args, standardise
from deepcgp_amd.models import index_table, learning_rate, lr_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Const(utils.Logger):
    def __init__(self, title, values):
        self.title, self.values = title, list(values)

    def __call__(self, model):
        return self.values.pop(0)


def test_log_file_format_and_returned_line(tmp_path):
    log = utils.Log(str(tmp_path / "results"), "run", [_Const("global_step", [20, 40]), _Const("test_accuracy", [0.25, 0.5])])
    assert log.write_entry(None) == "Entry: 0; global_step: 20; test_accuracy: 0.25"
    assert log.write_entry(None) == "Entry: 1; global_step: 40; test_accuracy: 0.5"
    log.close()
    path = tmp_path / "results" / "run" / "log.csv"
    assert path.read_text().splitlines() == ["Entry,global_step,test_accuracy", "0,20,0.25", "1,40,0.5"]
    # a restarted run appends: a second header, entries counted from 0 again (conv_gp/utils/log.py:96-106 opens with 'at')
    log = utils.Log(str(tmp_path / "results"), "run", [_Const("global_step", [60]), _Const("test_accuracy", [0.75])])
    log.write_entry(None)
    log.close()
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows == [["Entry", "global_step", "test_accuracy"], ["0", "20", "0.25"], ["1", "40", "0.5"],
                    ["Entry", "global_step", "test_accuracy"], ["0", "60", "0.75"]]


def test_step_and_rate_loggers():
    class M:
        global_step = 140
    assert utils.GlobalStepLogger().title == "global_step" and utils.GlobalStepLogger()(M()) == 140
    assert utils.GlobalStepLogger()(object()) == 0
    lr = utils.LearningRateLogger(lambda: 0.001)
    assert lr.title == "lr" and lr(M()) == 0.001
    from deepcgp_amd import models
    assert utils.AccuracyLogger is models.AccuracyLogger and utils.LogLikelihoodLogger is models.LogLikelihoodLogger
    assert utils.TestLogDensityLogger is models.TestLogDensityLogger


def test_options_toml_on_every_flag_type(tmp_path):
    flags = argparse.Namespace(name="run \"7\"\\x", log_dir="a/b", empty="", load_model=None, white=False, identity_mean=True, batch_size=32,
                               negative=-5, lr=0.01, gamma=1e-3, big=1e22, whole=2.0, tiny=-2.5e-7, tab="a\tb\nc", uni="é\x01")
    log = utils.Log(str(tmp_path), "run", [])
    log.write_flags(flags)
    log.close()
    text = (tmp_path / "run" / "options.toml").read_text()
    lines = text.splitlines()
    assert 'empty = ""' in lines and "white = false" in lines and "identity_mean = true" in lines and "batch_size = 32" in lines
    assert "whole = 2.0" in lines and "lr = 0.01" in lines and "negative = -5" in lines
    assert not any(l.startswith("load_model") for l in lines) and "# load_model is not set" in lines
    assert all(" = " in l or l.startswith("#") for l in lines)           # flat key = value lines
    with pytest.raises(TypeError):
        utils.toml_lines({"a": [1, 2]})
    try:
        import tomli
    except ImportError:
        return
    want = {k: v for k, v in vars(flags).items() if v is not None}
    assert tomli.loads(text) == want
    assert tomli.loads("\n".join(utils.toml_lines({"x": float("inf"), "y": float("-inf")}))) == {"x": float("inf"), "y": float("-inf")}
    assert np.isnan(tomli.loads("\n".join(utils.toml_lines({"x": float("nan")})))["x"])


def test_index_table_equals_successive_choice_calls():
    a, b = np.random.default_rng(3), np.random.default_rng(3)
    table = index_table(a, 23, 5, 7)
    assert table.shape == (7, 5) and table.dtype == np.int32
    for i in range(7):
        assert np.array_equal(table[i], b.choice(23, size=5, replace=False))
    assert np.array_equal(a.choice(23, size=5, replace=False), b.choice(23, size=5, replace=False))     # the generator is where the loop leaves it
    assert index_table(a, 23, 5, 0).shape == (0, 5)


def test_lr_table_equals_learning_rate_step_by_step():
    t = lr_table(0.01, 97, 7, 100)
    assert t.dtype == np.float64 and list(t) == [learning_rate(0.01, 97 + i, 100) for i in range(7)]
    assert list(t[:3]) == [0.01] * 3 and list(t[3:]) == [0.01 * 0.1 ** 1] * 4


def test_standardise_is_the_standard_scaler():
    from sklearn import preprocessing
    rng = np.random.default_rng(0)
    A, B = rng.standard_normal((30, 4, 3, 2)) * 3 + 1, rng.standard_normal((7, 4, 3, 2))
    A[:, 0, 0, 0] = 2.5                                   # a constant pixel
    a, b = standardise(A, B)
    sc = preprocessing.StandardScaler()
    assert a.shape == A.shape and b.shape == B.shape
    np.testing.assert_allclose(a.reshape(30, -1), sc.fit_transform(A.reshape(30, -1)), rtol=0, atol=1e-13)
    np.testing.assert_allclose(b.reshape(7, -1), sc.transform(B.reshape(7, -1)), rtol=0, atol=1e-13)


class _StubModel:
    """Records what the driver asks of a model."""
    minibatch_size = 4
    parameters = []

    def __init__(self):
        self.X = np.zeros((10, 3))
        self.calls = []

    def train_run(self, idx, lr, seed=0):
        self.calls.append(("train_run", np.array(idx), np.array(lr), seed, getattr(self, "global_step", None)))
        return np.arange(len(idx), dtype=np.float64)

    def pull_parameters(self):
        self.calls.append(("pull",))


class _StubExperiment(Experiment):
    def _load_data(self):
        self.X_train = self.Y_train = self.X_test = self.Y_test = None

    def _setup_model(self):
        self.model = _StubModel()
        self.global_step = 95
        self.model.global_step = 95

    def _setup_logger(self):
        self.log = utils.Log(self.flags.log_dir, self.flags.name, [utils.GlobalStepLogger(), utils.LearningRateLogger(self.learning_rate)])
        self.log.write_flags(self.flags)


def test_train_step_control_flow_on_a_stub_model(tmp_path, capsys):
    flags = read_args(["--name", "stub", "--data", "none.npz", "--log-dir", str(tmp_path), "--test-every", "6", "--lr-decay-steps", "100",
                       "--batch-size", "4"])
    flags.seed = 9
    exp = _StubExperiment(flags)
    assert exp._model_path() == os.path.join(str(tmp_path), "stub.npy") and exp._model_path("other") == os.path.join(str(tmp_path), "other.npy")
    exp.train_step()
    exp.train_step()
    exp.conclude()
    runs = [c for c in exp.model.calls if c[0] == "train_run"]
    assert len(runs) == 2 and [c[0] for c in exp.model.calls] == ["train_run", "pull"] * 2      # one run per period, then the pull for the checkpoint
    rng = np.random.default_rng(9)
    for k, (_, idx, lr, seed, gs) in enumerate(runs):
        start = 95 + 6 * k
        assert idx.shape == (6, 4) and np.array_equal(idx, index_table(rng, 10, 4, 6))            # the generator goes on across periods
        assert list(lr) == [learning_rate(0.01, start + i, 100) for i in range(6)]
        assert seed == 9 + start and gs == start
    assert 0.001 in list(runs[0][2]) and 0.01 in list(runs[0][2])                                  # (the first period crosses a decay boundary)
    assert exp.global_step == 107 and exp.model.global_step == 107 and isinstance(exp.global_step, int)
    out = capsys.readouterr().out.splitlines()
    assert out == ["Entry: 0; global_step: 101; lr: %s" % learning_rate(0.01, 101, 100), "Entry: 1; global_step: 107; lr: %s" % learning_rate(0.01, 107, 100)]
    saved = np.load(os.path.join(str(tmp_path), "stub.npy"), allow_pickle=True).item()
    assert saved == {"global_step": 107}
    assert (tmp_path / "stub" / "log.csv").read_text().splitlines()[0] == "Entry,global_step,lr"
    with pytest.raises(NotImplementedError):
        Experiment(flags)                                                                           # _load_data is abstract
    flags.optimizer = "LBFGS"
    with pytest.raises(ValueError):
        _StubExperiment(flags)


def test_data_flag_is_the_drivers_own():
    from deepcgp_amd.arguments import FLAGS, default_parser
    assert "--data" not in [f[0] for f in FLAGS]
    assert read_args(["--name", "x", "--data", "d.npz"]).data == "d.npz"
    with pytest.raises(SystemExit):
        read_args(["--name", "x"])
    assert not hasattr(default_parser().parse_args(["--name", "x"]), "data")


def test_flat_shims_import():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r);"
            "import utils; from experiment import Experiment; import deepcgp_amd.experiment as E; import deepcgp_amd.utils as U;"
            "assert Experiment is E.Experiment and utils.Log is U.Log and utils.GlobalStepLogger is U.GlobalStepLogger;"
            "assert utils.AccuracyLogger is U.AccuracyLogger and utils.LearningRateLogger is U.LearningRateLogger; print('ok')"
            % (ROOT, os.path.join(ROOT, "deepcgp_amd", "flat")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_header_declares_the_run():
    declared = dev.declared_symbols()
    assert "dcgp_model_set_dataset" in declared and "dcgp_model_train_run_adam" in declared
    assert "dcgp_model_set_dataset" in dev._SIGS and "dcgp_model_train_run_adam" in dev._SIGS
    assert issubclass(dev.NotPositiveDefinite, np.linalg.LinAlgError) and issubclass(dev.NotPositiveDefinite, dev.DcgpError)
