"""--keep-optimizer and --clip-norm without a GPU: the flags and their options.toml lines, ``parse_clip_norm``, the flat shim, the driver's
logger list, the sidecar's round trip (a PCG64 state's 128-bit integers included) and its refusals, the header's new entry points, and a
default-flags period on a stub model that writes nothing new."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd import utils
from deepcgp_amd.arguments import default_parser, parse_clip_norm
from deepcgp_amd.experiment import Experiment, read_args
from deepcgp_amd.models import load_optimizer_state, restore_optimizer_state, save_optimizer_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_defaults_and_their_option_lines(tmp_path):
    fl = default_parser().parse_args(["--name", "run"])
    assert fl.keep_optimizer is False and fl.clip_norm == 0.0 and isinstance(fl.clip_norm, float)
    log = utils.Log(str(tmp_path), "run", [])
    log.write_flags(fl)
    log.close()
    lines = (tmp_path / "run" / "options.toml").read_text().splitlines()
    assert "keep_optimizer = false" in lines and "clip_norm = 0.0" in lines, lines
    fl = default_parser().parse_args(["--name", "run", "--keep-optimizer", "--clip-norm", "2.5"])
    assert fl.keep_optimizer is True and fl.clip_norm == 2.5


def test_parse_clip_norm():
    assert parse_clip_norm(argparse.Namespace()) == 0.0                       # a namespace from before the flag
    assert parse_clip_norm(argparse.Namespace(clip_norm=None)) == 0.0
    assert parse_clip_norm(argparse.Namespace(clip_norm=3)) == 3.0
    assert parse_clip_norm(argparse.Namespace(clip_norm=float("inf"))) == float("inf")
    for bad in (-1.0, -1e-300, float("nan")):
        with pytest.raises(ValueError, match="--clip-norm"):
            parse_clip_norm(argparse.Namespace(clip_norm=bad))


def test_flat_shim_exports_the_helper():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r);"
            "import arguments, utils; import deepcgp_amd.arguments as A; import deepcgp_amd.utils as U;"
            "assert arguments.parse_clip_norm is A.parse_clip_norm and utils.GradNormLogger is U.GradNormLogger; print('ok')"
            % (ROOT, os.path.join(ROOT, "deepcgp_amd", "flat")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def _logger_list(tmp_path, name, *extra):
    """``_setup_logger`` on an experiment that has its flags and test set and nothing else."""
    exp = Experiment.__new__(Experiment)
    exp.flags = default_parser().parse_args(["--name", name, "--log-dir", str(tmp_path)] + list(extra))
    exp.test_views = None
    exp.X_test, exp.Y_test = np.zeros((6, 8, 8, 1)), np.arange(6).reshape(-1, 1)
    exp._setup_logger()
    exp.log.close()
    return exp, exp.log.loggers


def test_driver_logger_list(tmp_path):
    _, plain = _logger_list(tmp_path, "plain")
    assert [type(l) for l in plain] == [utils.GlobalStepLogger, utils.AccuracyLogger, utils.LogLikelihoodLogger]
    exp, clipped = _logger_list(tmp_path, "clipped", "--clip-norm", "5")
    assert [type(l) for l in clipped] == [utils.GlobalStepLogger, utils.AccuracyLogger, utils.LogLikelihoodLogger, utils.GradNormLogger]
    assert clipped[-1].title == "grad_norm" and np.isnan(clipped[-1](None))          # no period yet
    exp._period_norms = np.array([1.0, 2.0, 6.0])
    assert clipped[-1](None) == 3.0
    old = argparse.Namespace(**{k: v for k, v in vars(exp.flags).items() if k not in ("clip_norm", "keep_optimizer")})
    exp.flags = old                                                                   # a namespace from before the flags
    exp._setup_logger()
    exp.log.close()
    assert len(exp.log.loggers) == 3


class _FakeModel:
    """Holds a state dict the way DGP_Base does."""
    layers = []

    def __init__(self, state):
        self.state = state

    def optimizer_state(self):
        return self.state


def _fake_state(rng):
    return {"t": 7, "layers/0/Z/m": rng.standard_normal((5, 9)), "layers/0/Z/v": rng.random((5, 9)), "layers/0/hyper/m": rng.standard_normal(3),
            "layers/0/hyper/v": rng.random(3), "likelihood/m": np.array([1e-300]), "likelihood/v": np.array([np.nextafter(1.0, 2.0)])}


def test_sidecar_round_trip(tmp_path):
    gen = np.random.default_rng(12345)
    gen.random(11)
    state = _fake_state(np.random.default_rng(0))
    path = str(tmp_path / "run.opt.npz")
    save_optimizer_state(_FakeModel(state), path, 140, rng=gen)
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    want_draws = gen.random(5)
    with np.load(path, allow_pickle=False) as z:                                       # nothing in it needs pickle
        assert int(z["format"]) == 1 and int(z["global_step"]) == 140
        assert {k for k in z.files if k.startswith("opt/")} == {"opt/" + k for k in state}
    side = load_optimizer_state(path)
    assert side["global_step"] == 140 and side["prior"] == {} and set(side["state"]) == set(state)
    assert side["state"]["t"] == 7 and isinstance(side["state"]["t"], int)
    for k, v in state.items():
        np.testing.assert_array_equal(side["state"][k], v, err_msg=k)
    # PCG64: state and inc are 128-bit integers -- they come back as the integers they were
    inner = side["rng"]["state"]
    assert side["rng"]["bit_generator"] == "PCG64" and isinstance(inner["state"], int) and inner["inc"] > 2 ** 64
    again = np.random.default_rng(0)
    again.bit_generator.state = side["rng"]
    assert np.array_equal(again.random(5), want_draws)
    big = {"bit_generator": "PCG64", "state": {"state": 2 ** 128 - 1, "inc": 2 ** 127 + 1}, "has_uint32": 0, "uinteger": 0}
    assert json.loads(json.dumps(big)) == big
    # without a generator there is no generator state
    save_optimizer_state(_FakeModel(state), path, 141)
    assert load_optimizer_state(path)["rng"] is None and load_optimizer_state(path)["global_step"] == 141


def test_sidecar_refusals(tmp_path):
    path = str(tmp_path / "run.opt.npz")
    with pytest.raises(ValueError, match="run.opt.npz"):
        load_optimizer_state(path)                                                     # missing
    save_optimizer_state(_FakeModel(_fake_state(np.random.default_rng(1))), path, 20)
    with pytest.raises(ValueError, match="run.opt.npz.*20.*25|run.opt.npz"):
        restore_optimizer_state(_FakeModel({}), path, 25)                              # another global_step than the checkpoint's
    np.savez(open(path, "wb"), format=np.array(2), global_step=np.array(20))
    with pytest.raises(ValueError, match="run.opt.npz"):
        load_optimizer_state(path)                                                     # another format


def test_header_declares_the_entry_points():
    declared = dev.declared_symbols()
    for name in ("dcgp_model_get_adam_state", "dcgp_model_set_adam_state", "dcgp_model_get_adam_t", "dcgp_model_set_adam_t",
                 "dcgp_model_set_grad_clip", "dcgp_model_grad_norms"):
        assert name in declared and name in dev._SIGS, name


class _StubModel:
    """A model from before the feature: ``train_run(idx, lr, seed)`` and ``pull_parameters``, nothing else."""
    minibatch_size = 4
    parameters = []

    def __init__(self):
        self.X = np.zeros((10, 3))
        self.calls = []

    def train_run(self, idx, lr, seed=0):
        self.calls.append("train_run")
        return np.arange(len(idx), dtype=np.float64)

    def pull_parameters(self):
        self.calls.append("pull")


class _StubExperiment(Experiment):
    def _load_data(self):
        self.X_train = self.Y_train = self.X_test = self.Y_test = None

    def _setup_model(self):
        self.model = _StubModel()
        self.global_step = 0

    def _setup_logger(self):
        self.log = utils.Log(self.flags.log_dir, self.flags.name, [utils.GlobalStepLogger()])
        self.log.write_flags(self.flags)


def test_default_flags_call_nothing_new_and_write_nothing_new(tmp_path):
    flags = read_args(["--name", "stub", "--data", "none.npz", "--log-dir", str(tmp_path), "--test-every", "3", "--batch-size", "4"])
    exp = _StubExperiment(flags)
    exp.train_step()
    exp.conclude()
    assert exp.model.calls == ["train_run", "pull"]
    assert sorted(os.listdir(str(tmp_path))) == ["stub", "stub.npy"]
    assert np.load(os.path.join(str(tmp_path), "stub.npy"), allow_pickle=True).item() == {"global_step": 3}
    # --keep-optimizer --load-model without a sidecar: refused, naming the file
    flags = read_args(["--name", "next", "--data", "none.npz", "--log-dir", str(tmp_path), "--load-model", "stub", "--keep-optimizer"])
    with pytest.raises(ValueError, match="stub.opt.npz"):
        _StubExperiment(flags)
    with pytest.raises(ValueError, match="--clip-norm"):
        _StubExperiment(read_args(["--name", "bad", "--data", "none.npz", "--log-dir", str(tmp_path), "--clip-norm", "-2"]))
