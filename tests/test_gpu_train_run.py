"""A training run on the device (``DGP_Base.attach_dataset`` / ``train_run``, dcgp_model_set_dataset / dcgp_model_train_run_adam, csrc/train_run.hip)
against the per-step loop it replaces, and the experiment driver over it (deepcgp_amd/experiment.py).

The contract is identity, not closeness: step i of a run IS ``train_step(X[idx[i]], Y[idx[i]], lr[i], seed=seed + i)`` on a batch that a
gather kernel wrote from the resident set, so every comparison here is ``np.array_equal`` -- on the ELBO history, on every entry of
``model.parameters`` and, through one more identical step on both models, on the Adam moments and the step count.  No tolerance appears.

Models come from ``live_specs.live_spec`` (every gradient group live, so every parameter moves); the image pool is
``synthetic.make_batch(hwc, 23, seed)``, the labels come from a seeded generator, batch 5, S = 2.  The index table holds rows 0 and 22 (the ends
of the pool), one step repeats the previous step's batch exactly (the single set of batch buffers is rewritten with the same rows), and the
learning-rate table crosses a decay boundary inside the run.  Row lengths: 196, 338, 144, 189, 784.

On an MI355X every case below passes with every comparison exact; a case takes well under a second."""
import copy
import csv
import functools
import os

import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.likelihoods import Gaussian
from deepcgp_amd.models import build_from_spec, learning_rate, train
import live_specs as ls

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

POOL, BATCH, S, SEED0 = 23, 5, 2, 11
LR0, STEP0, DECAY = 0.01, 2, 5      # learning_rate(LR0, STEP0 + i, DECAY): 0.01 for i < 3, 0.001 from i = 3 on

GEOMETRIES = {
    "small3_M20": dict(ls.CASES_M256["small3_M20"]),                                        # 3 layers, rows of 196
    "odd_M33": dict(ls.CASES_M256["odd_M33"]),                                              # rows of 338, R = 13
    "head_only_M24": dict(hwc=(12, 12, 1), convs=[], head=(3, 1), M=24, c=0.5, a=0.3),      # the model opens with the head: rows of 144
    "g973_M5": dict(hwc=(9, 7, 3), convs=[(4, 2, 3)], head=(2, 1), M=5, c=1.0, a=0.1),      # rows of 189 = 9 x 7 x 3
    "ch_M384": dict(ls.CASES["ch_M384"]),                                                   # M > 256: the sweep + GEMM route's workspaces
}
STEPS = {"ch_M384": 3}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(spec, X pool, labels, float targets [POOL, R]) of a geometry, built once per process and never written to."""
    k = dict(GEOMETRIES[name])
    k.pop("N", None)
    spec = ls.live_spec(S=S, **k)
    X, _ = syn.make_batch(k["hwc"], POOL, seed=7)
    rng = np.random.default_rng(99)
    Y = rng.integers(0, 10, POOL).astype(np.int32)
    Yf = rng.standard_normal((POOL, spec["head"]["R"]))
    return spec, X, Y, Yf


def _model(name, dedup=True, gaussian=False):
    spec, X, Y, Yf = _case(name)
    m = build_from_spec(copy.deepcopy(spec), X.copy(), Yf.copy() if gaussian else Y.copy(), likelihood=Gaussian(0.7) if gaussian else None)
    m.dedup_layer0 = dedup
    m._build()
    return m


def _tables(steps):
    """idx [steps, BATCH] and lr [steps]: rows 0 and 22 in step 0, step 3 (step 2 of a 3-step run) repeats its predecessor's batch."""
    rng = np.random.default_rng(5)
    idx = np.stack([rng.choice(POOL, BATCH, replace=False) for _ in range(steps)]).astype(np.int64)
    idx[0] = [0, 22, 5, 11, 17]
    rep = min(3, steps - 1)
    idx[rep] = idx[rep - 1]
    lrs = np.array([learning_rate(LR0, STEP0 + i, DECAY) for i in range(steps)])
    assert len(set(lrs)) == 2 or steps <= 3, lrs
    return idx, lrs


def _values(model):
    model.pull_parameters()
    return [(p.pathname, np.array(p.value)) for p in model.parameters]


def _assert_same(a, b, what, equal_nan=False):
    assert [n for n, _ in a] == [n for n, _ in b]
    for (name, va), (_, vb) in zip(a, b):
        assert np.array_equal(va, vb, equal_nan=equal_nan), (what, name, float(np.nanmax(np.abs(va - vb))))


def _loop(model, idx, lrs, seed0):
    """The per-step loop a run replaces: host gather, one ``train_step`` per step."""
    hist = []
    for i in range(len(idx)):
        hist.append(model.train_step(model.X[idx[i]], model.Y[idx[i]], lrs[i], seed=seed0 + i))
    return np.array(hist)


def _run_equals_loop(name, dedup=True, gaussian=False, prepare=None):
    steps = STEPS.get(name, 6)
    idx, lrs = _tables(steps)
    a, b = _model(name, dedup, gaussian), _model(name, dedup, gaussian)
    for m in (a, b):
        if prepare:
            prepare(m)
    start = _values(a)
    ha = _loop(a, idx, lrs, SEED0)
    b.attach_dataset()
    hb = b.train_run(idx, lrs, seed=SEED0)
    print("%s dedup=%d gaussian=%d: loop %s\n   run %s" % (name, dedup, gaussian, ha, hb))
    assert hb.shape == (steps,) and np.all(np.isfinite(ha))
    assert np.array_equal(ha, hb)
    va, vb = _values(a), _values(b)
    _assert_same(va, vb, "after the run")
    # one more identical step on both: its ELBO and result depend on both moment buffers and on the step count of the bias correction
    ea = a.train_step(a.X[idx[1]], a.Y[idx[1]], 0.004, seed=77)
    eb = b.train_step(b.X[idx[1]], b.Y[idx[1]], 0.004, seed=77)
    assert ea == eb, (ea, eb)
    _assert_same(_values(a), _values(b), "one step after the run")
    b.detach_dataset()
    return a, b, start, va


@pytest.mark.parametrize("name,dedup", [("small3_M20", True), ("small3_M20", False), ("odd_M33", True), ("head_only_M24", True), ("g973_M5", True),
                                        ("ch_M384", True)])
def test_run_equals_loop_bit_for_bit(ctx, name, dedup):
    a, b, start, end = _run_equals_loop(name, dedup)
    moved = [n for (n, v0), (_, v1) in zip(start, end) if not np.array_equal(v0, v1)]
    assert len(moved) >= len(start) - 1, (sorted(set(n for n, _ in start) - set(moved)))     # (RobustMax epsilon is no trainable value)
    a.close(), b.close()


def test_run_equals_loop_with_float_targets(ctx):
    """Gaussian(0.7), targets [23, R]: the likelihood variance and its moments move identically."""
    a, b, start, end = _run_equals_loop("small3_M20", gaussian=True)
    v0 = dict(start)["DGP/likelihood/likelihood/variance"]
    v1 = dict(end)["DGP/likelihood/likelihood/variance"]
    print("likelihood variance %.17g -> %.17g" % (v0, v1))
    assert v0 == 0.7 and v1 != v0
    a.close(), b.close()


def test_frozen_groups_stay_bitwise(ctx):
    last = len(_case("small3_M20")[0]["convs"])

    def freeze(m):
        m.set_trainable(0, "Z", False)
        m.set_trainable(last, "hyper", False)
    a, b, start, end = _run_equals_loop("small3_M20", prepare=freeze)
    s, e = dict(start), dict(end)
    frozen = ["DGP/layers/0/feature/Z", "DGP/layers/%d/kern/base_kernel/variance" % last, "DGP/layers/%d/kern/base_kernel/lengthscales" % last]
    for name in frozen:
        assert np.array_equal(s[name], e[name]), name
    for name in s:
        if name not in frozen and "invlink" not in name:
            assert not np.array_equal(s[name], e[name]), (name, "did not move")
    a.close(), b.close()


def test_nan_in_Z_fails_step_0_like_the_loop(ctx):
    """(a) a NaN in layer 0's Z: both routes raise numpy.linalg.LinAlgError (device.NotPositiveDefinite) at step 0 and leave parameters, moments and
    step count as they were -- shown by restoring Z and taking one step on both and on a model that never failed."""
    idx, lrs = _tables(6)
    a, b, c = _model("small3_M20"), _model("small3_M20"), _model("small3_M20")
    keep = np.array(a.layers[0].feature.Z)
    for m in (a, b):
        bad = keep.copy()
        bad[3, 2] = np.nan
        m.layers[0].feature.Z = bad
        m.sync_parameters()
    before = _values(a)
    with pytest.raises(np.linalg.LinAlgError) as ea:
        a.train_step(a.X[idx[0]], a.Y[idx[0]], lrs[0], seed=SEED0)
    b.attach_dataset()
    with pytest.raises(np.linalg.LinAlgError) as eb:
        b.train_run(idx, lrs, seed=SEED0)
    assert type(eb.value) is type(ea.value) is dev.NotPositiveDefinite
    assert eb.value.step == 0 and len(eb.value.history) == 0 and "step 0" in str(eb.value), str(eb.value)
    assert eb.value.column == ea.value.column
    _assert_same(_values(a), before, "loop, after the failure", equal_nan=True)
    _assert_same(_values(b), before, "run, after the failure", equal_nan=True)
    for m in (a, b):
        m.layers[0].feature.Z = keep.copy()
        m.sync_parameters()
    es = [m.train_step(m.X[idx[1]], m.Y[idx[1]], 0.01, seed=5) for m in (a, b, c)]
    assert es[0] == es[1] == es[2], es
    vc = _values(c)
    _assert_same(_values(a), vc, "loop, first good step")
    _assert_same(_values(b), vc, "run, first good step")
    a.close(), b.close(), c.close()


def test_nan_pixel_fails_where_the_loop_fails(ctx):
    """(b) one pool image holds a NaN pixel and the index table selects it at step 2 of 5: the loop is run to its exception, the run must raise the
    same type at the same step with the same history before it and the same parameters after it."""
    steps = 5
    idx, lrs = _tables(6)
    idx, lrs = idx[:steps], lrs[:steps]
    poisoned = 9
    idx[idx == poisoned] = 10                      # nowhere ...
    idx[2] = [poisoned, 1, 2, 3, 4]                # ... but in step 2
    a, b = _model("small3_M20"), _model("small3_M20")
    for m in (a, b):
        m.X[poisoned, 17] = np.nan
    hist, failed = [], None
    try:
        for i in range(steps):
            hist.append(a.train_step(a.X[idx[i]], a.Y[idx[i]], lrs[i], seed=SEED0 + i))
    except Exception as e:      # noqa: BLE001  (whatever the loop raises is what the run must raise)
        failed = e
    print("the loop failed at step %d with %r; history %s" % (len(hist), failed, hist))
    assert failed is not None and 2 <= len(hist) < steps, (failed, hist)
    b.attach_dataset()
    with pytest.raises(type(failed)) as eb:
        b.train_run(idx, lrs, seed=SEED0)
    assert type(eb.value) is type(failed)
    assert eb.value.step == len(hist), (eb.value.step, len(hist))
    assert np.array_equal(eb.value.history, np.array(hist), equal_nan=True), (eb.value.history, hist)
    _assert_same(_values(a), _values(b), "after the failure", equal_nan=True)
    a.close(), b.close()


@pytest.mark.parametrize("with_callback", [False, True])
def test_models_train_is_unchanged(ctx, with_callback):
    """train(model, 7, seed=3) against the Adam branch it had before the run existed, written out by hand: the same default_rng(3).choice calls,
    then train_step."""
    steps, seed, decay = 7, 3, 4
    a, b = _model("small3_M20"), _model("small3_M20")
    for m in (a, b):
        m.minibatch_size = BATCH
    rng = np.random.default_rng(seed)
    seen_a, seen_b, hist_a = [], [], []
    a.dedup_layer0 = True
    for i in range(steps):
        ix = rng.choice(POOL, size=BATCH, replace=False)
        e = a.train_step(a.X[ix], a.Y[ix], learning_rate(0.01, i, decay), seed=seed + i)
        hist_a.append(e)
        seen_a.append((i + 1, e))
    hist_b = train(b, steps, seed=seed, lr_decay_steps=decay, callback=(lambda step, e: seen_b.append((step, e))) if with_callback else None)
    assert hist_b == hist_a, (hist_a, hist_b)
    assert isinstance(hist_b, list) and all(type(e) is float for e in hist_b)
    if with_callback:
        assert seen_b == seen_a
    _assert_same(_values(a), _values(b), "after train()")
    assert b._dataset is None          # attached for the call only
    a.close(), b.close()


def test_guards_raise_before_any_launch(ctx):
    idx, lrs = _tables(6)
    m = _model("small3_M20")
    with pytest.raises(ValueError):
        m.train_run(idx, lrs)                           # no dataset attached
    L = dev.lib()
    elbo, done, info = np.zeros(6), dev.C.c_int(7), dev.C.c_int(0)
    i32 = np.ascontiguousarray(idx, np.int32)

    def raw(table, rates):
        return L.dcgp_model_train_run_adam(m._model, table.ctypes.data, 6, BATCH, 10.0, rates.ctypes.data, 0, 1, 0.9, 0.999, 1e-8, elbo.ctypes.data,
                                           dev.C.byref(done), dev.C.byref(info))
    assert raw(i32, lrs) == dev.ERR_ARG and done.value == 0     # ... says the library as well
    m.attach_dataset()
    before = _values(m)
    for bad in (POOL, -1):
        t = idx.copy()
        t[4, 3] = bad
        with pytest.raises(ValueError):
            m.train_run(t, lrs)
        assert raw(np.ascontiguousarray(t, np.int32), lrs) == dev.ERR_ARG and done.value == 0      # the library's own check, in front of every launch
    with pytest.raises(ValueError):
        m.train_run(idx, lrs[:5])                       # a table of the wrong length
    with pytest.raises(ValueError):
        m.train_run(idx, -0.01)
    zero = lrs.copy()
    zero[5] = 0.0
    assert raw(i32, zero) == dev.ERR_ARG and done.value == 0
    with pytest.raises(ValueError):
        m.train_run(idx.astype(np.float64), lrs)
    with pytest.raises(ValueError):
        m.attach_dataset(m.X[:, :100], m.Y)             # rows of another length
    _assert_same(_values(m), before, "after the refused calls")
    assert not np.any(elbo)
    hist = m.train_run(idx, lrs, seed=SEED0)            # the model still trains
    assert hist.shape == (6,) and np.all(np.isfinite(hist))
    m.detach_dataset()
    with pytest.raises(ValueError):
        m.train_run(idx, lrs)
    m.close()


def test_driver_end_to_end(ctx, tmp_path):
    """ArrayExperiment on 200 + 60 digits: two periods of 20 steps; log.csv, options.toml, and the checkpoint through --load-model."""
    from sklearn.datasets import load_digits
    from deepcgp_amd.experiment import ArrayExperiment, read_args, standardise
    from deepcgp_amd.utils import AccuracyLogger
    d = load_digits()
    Xtr, Xte = standardise(d.images[:200], d.images[200:260])
    Ytr, Yte = d.target[:200], d.target[200:260]
    args = ["--data", "unused", "--log-dir", str(tmp_path), "-M", "16,16", "--feature-maps", "2", "--filter-sizes", "3,3", "--strides", "1,1",
            "--batch-size", "16", "--num-samples", "2", "--test-every", "20", "--test-size", "60"]
    np.random.seed(0)
    exp = ArrayExperiment(read_args(["--name", "run"] + args), Xtr, Ytr, Xte, Yte)
    assert exp.global_step == 0 and exp.X_test.shape == (60, 8, 8, 1)
    try:
        exp.train_step()
        exp.train_step()
    finally:
        exp.conclude()
    assert exp.global_step == 40 and np.all(np.isfinite(exp.last_elbos)) and len(exp.last_elbos) == 20
    with open(os.path.join(str(tmp_path), "run", "log.csv"), newline="") as f:
        rows = list(csv.reader(f))
    print(rows)
    assert rows[0] == ["Entry", "global_step", "test_accuracy", "train_log_likelihood"] and len(rows) == 3
    assert [r[0] for r in rows[1:]] == ["0", "1"] and [r[1] for r in rows[1:]] == ["20", "40"]
    assert all(0.0 <= float(r[2]) <= 1.0 and np.isfinite(float(r[3])) for r in rows[1:])
    try:
        import tomli
    except ImportError:
        tomli = None
    if tomli is not None:
        with open(os.path.join(str(tmp_path), "run", "options.toml"), "rb") as f:
            opts = tomli.load(f)
        want = {k: v for k, v in vars(exp.flags).items() if v is not None}
        assert opts == want, (opts, want)
    # the checkpoint, through --load-model: the same predictions, and the step count goes on
    again = ArrayExperiment(read_args(["--name", "run2", "--load-model", "run"] + args), Xtr, Ytr, Xte, Yte)
    try:
        assert again.global_step == 40 and again.model.global_step == 40
        assert np.array_equal(again.X_test, exp.X_test) and np.array_equal(again.Y_test, exp.Y_test)
        acc = AccuracyLogger(again.X_test.reshape(60, -1), again.Y_test)(again.model)
        print("logged accuracy %s, reloaded %r" % (rows[2][2], acc))
        assert acc == float(rows[2][2])
        flat = again.X_test.reshape(60, -1)          # (an accuracy is a coarse number: the class probabilities themselves, to the bit)
        assert np.array_equal(again.model.predict_proba(flat[:32], 5, seed=0), exp.model.predict_proba(flat[:32], 5, seed=0))
    finally:
        again.conclude()
    exp.model.close(), again.model.close()
