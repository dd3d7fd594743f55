"""Test-time augmentation without a GPU: the view lists (``augment.views``), the NumPy mirror of the view gather (``augment.apply_views``)
against ``augment.apply`` view by view, the gather's index arithmetic (csrc/augment_map.h: view_row, view_draw and the row map, compiled with the
host C++ compiler, tests/view_map_check.cc) against the mirror, the validation, the flags, options.toml, the driver's logger list and the
declared symbols.  Every comparison of images is ``np.array_equal``: the transform only moves values."""
import argparse
import os
import shutil
import subprocess

import numpy as np
import pytest

from deepcgp_amd import augment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(v):
    return [tuple(int(a) for a in r) for r in v]


# ---- view lists --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 4])
def test_cross_and_grid(t):
    c = augment.views(t)
    assert c.shape == (5, 3) and c.dtype == np.int32
    assert set(_rows(c)) == {(0, 0, 0), (t, 0, 0), (-t, 0, 0), (0, t, 0), (0, -t, 0)}
    cf = augment.views(t, True)
    assert cf.shape == (10, 3)
    assert np.array_equal(cf[:5], c) and np.array_equal(cf[5:, :2], c[:, :2]) and np.all(cf[5:, 2] == 1)     # the unflipped views first
    g = augment.views(t, pattern="grid")
    assert g.shape == ((2 * t + 1) ** 2, 3)
    assert set(_rows(g)) == {(dy, dx, 0) for dy in range(-t, t + 1) for dx in range(-t, t + 1)}
    gf = augment.views(t, True, "grid")
    assert gf.shape == (2 * (2 * t + 1) ** 2, 3) and np.array_equal(gf[:len(g)], g) and np.all(gf[len(g):, 2] == 1)
    for v in (c, cf, g, gf):
        assert _rows(v)[0] == (0, 0, 0)                                   # the identity first
        assert len(set(_rows(v))) == len(v)                               # no duplicates


def test_degenerate_lists():
    for pattern in ("cross", "grid"):
        assert _rows(augment.views(0, False, pattern)) == [(0, 0, 0)]
        assert _rows(augment.views(0, True, pattern)) == [(0, 0, 0), (0, 0, 1)]
    assert _rows(augment.views()) == [(0, 0, 0)]
    with pytest.raises(ValueError, match="max_shift"):
        augment.views(-1)
    with pytest.raises(ValueError, match="pattern"):
        augment.views(1, pattern="ring")


# ---- the mirror --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,C", [(3, 9, 7, 3), (4, 5, 13, 2), (1, 6, 4, 2)])
def test_apply_views_is_apply_view_by_view(N, H, W, C):
    rng = np.random.default_rng(H * 100 + W)
    X = rng.standard_normal((N, H, W, C))
    keep = X.copy()
    m = min(H, W)
    v = np.array([(0, 0, 0), (-2, 3, 1), (H - 1, 0, 0), (0, -(W - 1), 1), (1, 1, 0), (0, 0, 1)], np.int32)      # one row, one column left
    got = augment.apply_views(X, v)
    assert got.shape == (len(v) * N, H, W, C) and got.dtype == X.dtype
    for k, (dy, dx, f) in enumerate(_rows(v)):
        assert np.array_equal(got[k * N:(k + 1) * N], augment.apply(X, dy, dx, f)), (dy, dx, f)       # view-major: view k at rows k N ...
    assert np.array_equal(got[:N], X) and np.array_equal(got[5 * N:], X[:, :, ::-1])
    assert np.array_equal(X, keep)
    for t, flip, pattern in ((2, True, "cross"), (1, False, "grid")):
        vv = augment.views(t, flip, pattern)
        assert augment.apply_views(X, vv).shape[0] == len(vv) * N


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("view_map") / "view_map_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "deepcgp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "view_map_check.cc"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("n,H,W,C", [(3, 9, 7, 3), (1, 5, 13, 1), (4, 4, 6, 2)])
def test_gather_index_arithmetic_is_the_mirror(check_exe, n, H, W, C):
    """The header's arithmetic, walked as the kernel walks it, on a batch whose values are their own indices: what it reads is what
    ``apply_views`` writes (fill -1 -> the mirror's fill of a batch shifted up by one)."""
    m = min(H, W)
    v = np.array([(0, 0, 0), (-2, 3, 1), (H - 1, 0, 0), (0, -(W - 1), 1), (-(m - 1), m - 1, 0), (1, -1, 1)], np.int32)
    r = subprocess.run([check_exe, "map", str(n), str(H), str(W), str(C)] + [str(a) for a in v.reshape(-1)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = np.array([line.split() for line in r.stdout.splitlines()], np.int64)
    assert got.shape == (len(v) * n, H * W * C)
    src = np.arange(1, n * H * W * C + 1).reshape(n, H, W, C)           # index + 1: the mirror's zero fill stays apart from index 0
    want = augment.apply_views(src, v).reshape(len(v) * n, -1) - 1
    assert np.array_equal(got, want)
    assert (got >= 0).any(axis=1).all()                                 # |dy| < H, |dx| < W: something of every image survives
    assert (got[2 * n] >= 0).sum() == W * C and (got[3 * n] >= 0).sum() == H * C      # the extreme shifts: one row, one column


def test_table_check_of_the_header(check_exe):
    def say(per_axis, H, W, *views):
        r = subprocess.run([check_exe, "table", str(per_axis), str(H), str(W)] + [str(a) for v in views for a in v], capture_output=True, text=True)
        assert r.returncode == 0
        return r.stdout.strip()
    # an evaluation's views: the training-time bound, min(H, W), whatever the axis
    assert say(0, 9, 7, (0, 0, 0), (6, -6, 1)) == "ok"
    for bad in ((7, 0, 0), (0, -7, 0), (-8, 0, 1)):
        assert "min(H, W)" in say(0, 9, 7, (0, 0, 0), bad)
    # the gather alone: per axis
    assert say(1, 9, 7, (0, 0, 0), (8, -6, 1), (-8, 6, 0)) == "ok"
    for bad in ((9, 0, 0), (-9, 0, 0), (0, 7, 1), (0, -7, 0)):
        assert "no pixel" in say(1, 9, 7, (0, 0, 0), bad)
    for per_axis in (0, 1):
        for bad in ((0, 0, 2), (0, 0, -1)):
            assert "flip" in say(per_axis, 9, 7, bad)


# ---- validation --------------------------------------------------------------------------------------------------------------------------
def test_validation():
    X = np.zeros((2, 9, 7, 3))
    ok = augment.check_views([(0, 0, 0), (6, -6, 1)], 9, 7)
    assert ok.dtype == np.int32 and ok.shape == (2, 3) and ok.flags["C_CONTIGUOUS"]
    assert np.array_equal(augment.check_views(np.array([[1.0, -2.0, 1.0]]), 9, 7), [[1, -2, 1]])
    for bad, what in (([(7, 0, 0)], "min"), ([(0, -7, 0)], "min"), ([(0, 8, 1)], "min"),      # a shift >= min(H, W), either sign, either axis
                      ([(0, 0, 2)], "flip"), ([(0, 0, -1)], "flip"),
                      ([(0, 0)], "V, 3"), ([0, 0, 0], "V, 3"), (np.zeros((2, 2, 3), int), "V, 3"),
                      (np.zeros((0, 3), int), "empty"), ([], "V, 3|empty"),
                      ([(0.5, 0, 0)], "integers")):
        with pytest.raises(ValueError, match=what):
            augment.check_views(bad, 9, 7)
        if what != "min":
            with pytest.raises(ValueError):
                augment.apply_views(X, bad)
    # the mirror of the gather alone takes any shift that leaves a pixel: |dy| < H, |dx| < W
    assert augment.apply_views(X, [(8, -6, 1), (7, 0, 0)]).shape == (4, 9, 7, 3)
    for bad in ([(9, 0, 0)], [(-9, 0, 1)], [(0, 7, 0)], [(0, -7, 0)]):
        with pytest.raises(ValueError, match="no pixel"):
            augment.apply_views(X, bad)
    with pytest.raises(ValueError, match="N, H, W, C"):
        augment.apply_views(np.zeros((2, 63)), [(0, 0, 0)])


def test_dense_head_only_model_has_no_views():
    """``evaluate(views=...)`` on a head-only ``--last-kernel rbf`` model, and bad views on a model with images, raise before the device model
    exists."""
    from deepcgp_amd.models import build_from_spec
    import live_specs as ls
    spec = ls.live_spec(hwc=(6, 6, 1), convs=[], head=(3, 1), M=8, c=0.5, a=0.3, head_kernel="rbf")
    m = build_from_spec(spec, np.zeros((4, 36)), np.zeros(4, np.int32))
    for call in (lambda: m.evaluate(m.X, m.Y, S=2, views=augment.views(1)),
                 lambda: m.evaluate_uncertainty(m.X, m.Y, S=2, views=augment.views(1)),
                 lambda: m.predict_density(m.X, m.Y, 2, views=augment.views(1)),
                 lambda: m.predict_uncertainty(m.X, 2, views=augment.views(1))):
        with pytest.raises(ValueError, match="dense head"):
            call()
    assert m._model is None
    conv = build_from_spec(ls.live_spec(hwc=(9, 7, 3), convs=[], head=(2, 1), M=5, c=1.0, a=0.1), np.zeros((4, 189)), np.zeros(4, np.int32))
    for bad, what in (([(7, 0, 0)], "min"), ([(0, 0, 2)], "flip"), ([(0, 0)], "V, 3"), (np.zeros((0, 3), int), "empty")):
        with pytest.raises(ValueError, match=what):
            conv.evaluate(conv.X, conv.Y, S=2, views=bad)
    # S * V * K + K above the multi-class tails' 8192 LDS slots (the uncertainty tail keeps 48 more): the smallest S that is too many
    K, V = conv.layers[-1].num_outputs, 5
    S_eval, S_unc = (8192 - K) // (V * K) + 1, (8192 - K - 48) // (V * K) + 1
    with pytest.raises(ValueError, match="LDS"):
        conv.evaluate(conv.X, conv.Y, S=S_eval, views=augment.views(1))
    with pytest.raises(ValueError, match="LDS"):
        conv.predict_density(conv.X, conv.Y, S_eval, views=augment.views(1))
    for call in (lambda: conv.evaluate_uncertainty(conv.X, conv.Y, S=S_unc, views=augment.views(1)),
                 lambda: conv.predict_uncertainty(conv.X, S_unc, views=augment.views(1))):
        with pytest.raises(ValueError, match="LDS"):
            call()
    assert conv._model is None


# ---- flags, options.toml, the driver's loggers ----------------------------------------------------------------------------------------------
def _flags(*extra):
    from deepcgp_amd.arguments import default_parser
    return default_parser().parse_args(["--name", "t"] + list(extra))


def test_flags_and_options_toml(tmp_path):
    from deepcgp_amd import utils
    from deepcgp_amd.arguments import parse_test_views
    from deepcgp_amd.flat import arguments as flat_arguments
    assert flat_arguments.parse_test_views is parse_test_views
    fl = _flags()
    assert (fl.test_shift, fl.test_flip, fl.test_views) == (0, False, "cross")
    assert parse_test_views(fl) is None
    assert parse_test_views(argparse.Namespace()) is None                   # flags from before the feature
    assert np.array_equal(parse_test_views(_flags("--test-shift", "2")), augment.views(2))
    assert np.array_equal(parse_test_views(_flags("--test-flip")), [(0, 0, 0), (0, 0, 1)])
    assert np.array_equal(parse_test_views(_flags("--test-shift", "1", "--test-views", "grid")), augment.views(1, False, "grid"))
    assert np.array_equal(parse_test_views(_flags("--test-shift", "3", "--test-flip", "--test-views", "grid")), augment.views(3, True, "grid"))
    assert parse_test_views(_flags("--test-views", "grid")) is None         # a pattern alone asks for no view
    with pytest.raises(ValueError, match="--test-views"):
        parse_test_views(_flags("--test-views", "ring"))
    with pytest.raises(ValueError, match="--test-views"):
        parse_test_views(_flags("--test-shift", "1", "--test-views", "ring"))
    with pytest.raises(ValueError, match="--test-shift"):
        parse_test_views(_flags("--test-shift", "-1"))
    log = utils.Log(str(tmp_path), "run", [])
    log.write_flags(_flags("--test-shift", "2", "--test-flip", "--test-views", "grid"))
    log.close()
    lines = (tmp_path / "run" / "options.toml").read_text().splitlines()
    assert "test_shift = 2" in lines and "test_flip = true" in lines and 'test_views = "grid"' in lines, lines
    log = utils.Log(str(tmp_path), "plain", [])
    log.write_flags(_flags())
    log.close()
    lines = (tmp_path / "plain" / "options.toml").read_text().splitlines()
    assert "test_shift = 0" in lines and "test_flip = false" in lines and 'test_views = "cross"' in lines, lines


def _logger_list(tmp_path, name, *extra):
    """The driver's ``_setup_logger`` on an experiment that has its flags and test set and nothing else (no model is touched)."""
    from deepcgp_amd.arguments import parse_test_views
    from deepcgp_amd.experiment import Experiment
    exp = Experiment.__new__(Experiment)
    exp.flags = _flags("--log-dir", str(tmp_path), *extra)
    exp.flags.name = name
    exp.test_views = parse_test_views(exp.flags)
    exp.X_test, exp.Y_test = np.zeros((6, 8, 8, 1)), np.arange(6).reshape(-1, 1)
    exp._setup_logger()
    exp.log.close()
    return exp.log.loggers


def test_driver_logger_list(tmp_path):
    from deepcgp_amd import utils
    from deepcgp_amd.models import AccuracyLogger, LogLikelihoodLogger, TTAAccuracyLogger
    plain = _logger_list(tmp_path, "plain")
    assert [type(l) for l in plain] == [utils.GlobalStepLogger, AccuracyLogger, LogLikelihoodLogger]      # today's list, exactly
    tta = _logger_list(tmp_path, "tta", "--test-shift", "1", "--test-flip")
    assert [type(l) for l in tta] == [utils.GlobalStepLogger, TTAAccuracyLogger, LogLikelihoodLogger]
    assert [l.title for l in tta] == [l.title for l in plain] and TTAAccuracyLogger.title == "test_accuracy"
    lg = tta[1]
    assert np.array_equal(lg.views, augment.views(1, True)) and (lg.batch_size, lg.num_samples) == (32, 5)
    assert lg.X_test.shape == (6, 64) and lg.Y_test.shape == (6,)
    assert utils.TTAAccuracyLogger is TTAAccuracyLogger


class _Recorder:
    gaussian = student_t = poisson = False

    def __init__(self):
        self.calls = []

    def evaluate(self, X, Y, **kw):
        self.calls.append(("evaluate", kw))
        return {"accuracy": 0.25, "mean_log_density": -1.5}

    def evaluate_uncertainty(self, X, Y, **kw):
        self.calls.append(("evaluate_uncertainty", kw))
        return {"ece": 0.1}


def test_loggers_hand_their_views_on():
    from deepcgp_amd.models import TestLogDensityLogger, TTAAccuracyLogger, UncertaintyLogger
    X, Y, v = np.zeros((4, 9)), np.arange(4), augment.views(1, True)
    m = _Recorder()
    assert TTAAccuracyLogger(X, Y, v, batch_size=3, num_samples=2)(m, seed=7) == 0.25
    assert TestLogDensityLogger(X, Y, batch_size=3, num_samples=2, views=v)(m, seed=7) == -1.5
    assert UncertaintyLogger(X, Y, S=2, batch_size=3, views=v)(m, seed=7) == {"ece": 0.1}
    assert TestLogDensityLogger(X, Y)(m) == -1.5 and UncertaintyLogger(X, Y)(m) == {"ece": 0.1}
    names = [c[0] for c in m.calls]
    assert names == ["evaluate", "evaluate", "evaluate_uncertainty", "evaluate", "evaluate_uncertainty"]
    for _, kw in m.calls[:3]:
        assert kw["views"] is v or np.array_equal(kw["views"], v)
        assert kw["seed"] == 7 and kw["batch_size"] == 3 and kw["S"] == 2
    for _, kw in m.calls[3:]:
        assert "views" not in kw                  # without views the loggers make the call they always made
    g = _Recorder()
    g.gaussian = True
    g._lik_name = lambda: "Gaussian"
    with pytest.raises(ValueError, match="classification"):
        TTAAccuracyLogger(X, Y, v)(g)


def test_batched_noise_with_views():
    """[S, V, N, D] -> per batch [S, V n_b, D], row v n_b + i; V = None is the layout it always had."""
    from deepcgp_amd.dgp import batched_noise
    S, V, N, D, bs = 2, 3, 5, 4, 2
    z = np.arange(S * V * N * D, dtype=np.float64).reshape(S, V, N, D)
    flat, none = batched_noise([z, None], N, S, bs, [D, 7], V)
    assert none is None and flat.shape == (z.size,)
    at = 0
    for lo in range(0, N, bs):
        n = min(bs, N - lo)
        tab = flat[at:at + S * V * n * D].reshape(S, V * n, D)
        for s in range(S):
            for v in range(V):
                for i in range(n):
                    assert np.array_equal(tab[s, v * n + i], z[s, v, lo + i])
        at += S * V * n * D
    assert at == z.size
    z1 = z[:, 0]
    assert np.array_equal(batched_noise([z1], N, S, bs, [D], 1)[0], batched_noise([z1], N, S, bs, [D])[0])       # one view: the same table
    with pytest.raises(ValueError, match=r"\[S, V, N, D\]"):
        batched_noise([z1], N, S, bs, [D], V)


# ---- symbols -----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    from deepcgp_amd import device as dev
    declared = dev.declared_symbols()
    for name in ("dcgp_model_set_eval_views", "dcgp_view_images"):
        assert name in declared and name in dev._SIGS
