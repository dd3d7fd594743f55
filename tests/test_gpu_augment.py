"""Training-time augmentation on the device (``DGP_Base.set_augmentation`` / ``augment``, dcgp_model_set_augmentation / dcgp_augment_images,
csrc/augment.hip) against its NumPy mirror (deepcgp_amd/augment.py), and an augmenting ``train_run`` against the per-step loop on
mirror-augmented batches.

The transform only moves values and the draws are integers, so the contract is identity: every comparison of images, ELBOs and parameters is
``np.array_equal``.  No tolerance appears.

Models, pool, batch, S and the tables have the shape of tests/test_gpu_train_run.py's: ``live_specs.live_spec`` models (every gradient group
live), a pool of 23 images from ``synthetic.make_batch``, batch 5, S = 2, 6 steps, one step repeating its predecessor's batch; max_shift 2 with
the flip on."""
import copy
import csv
import functools
import os

import numpy as np
import pytest

from deepcgp_amd import augment
from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.augment import Augmentation
from deepcgp_amd.likelihoods import Gaussian
from deepcgp_amd.models import build_from_spec, learning_rate
import live_specs as ls
import padding_ref as pr
import stack_specs as ss

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

POOL, BATCH, S, SEED0, STEPS = 23, 5, 2, 11, 6
LR0, STEP0, DECAY = 0.01, 2, 5
AUG = Augmentation(2, True)

GEOMETRIES = {
    "small3_M20": dict(ls.CASES_M256["small3_M20"]),                                        # 3 layers, rows of 196
    "odd_M33": dict(ls.CASES_M256["odd_M33"]),                                              # rows of 338 = 13 x 13 x 2
    "head_only_M24": dict(hwc=(12, 12, 1), convs=[], head=(3, 1), M=24, c=0.5, a=0.3),      # the model opens with the head: rows of 144
    "g973_M5": dict(hwc=(9, 7, 3), convs=[(4, 2, 3)], head=(2, 1), M=5, c=1.0, a=0.1),      # rows of 189 = 9 x 7 x 3
    "padded_res3": dict(pr.STACKS["res3"]),                                                 # the first layer pads its 10 x 10 x 1 input by 1
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(spec, (H, W, C), X pool, labels, float targets [POOL, R]) of a geometry, built once per process and never written to."""
    k = dict(GEOMETRIES[name])
    k.pop("N", None)
    spec = ss.stack_spec(**k) if name.startswith("padded") else ls.live_spec(S=S, **k)
    X, _ = syn.make_batch(k["hwc"], POOL, seed=7)
    rng = np.random.default_rng(99)
    Y = rng.integers(0, 10, POOL).astype(np.int32)
    Yf = rng.standard_normal((POOL, spec["head"]["R"]))
    return spec, tuple(k["hwc"]), X, Y, Yf


def _model(name, dedup=True, gaussian=False):
    spec, _, X, Y, Yf = _case(name)
    m = build_from_spec(copy.deepcopy(spec), X.copy(), Yf.copy() if gaussian else Y.copy(), likelihood=Gaussian(0.7) if gaussian else None)
    m.dedup_layer0 = dedup
    m._build()
    return m


def _tables(steps=STEPS):
    """idx [steps, BATCH] and lr [steps]: rows 0 and 22 in step 0, step 3 repeats its predecessor's batch."""
    rng = np.random.default_rng(5)
    idx = np.stack([rng.choice(POOL, BATCH, replace=False) for _ in range(steps)]).astype(np.int64)
    idx[0] = [0, 22, 5, 11, 17]
    idx[3] = idx[2]
    lrs = np.array([learning_rate(LR0, STEP0 + i, DECAY) for i in range(steps)])
    return idx, lrs


def _values(model):
    model.pull_parameters()
    return [(p.pathname, np.array(p.value)) for p in model.parameters]


def _assert_same(a, b, what):
    assert [n for n, _ in a] == [n for n, _ in b]
    for (name, va), (_, vb) in zip(a, b):
        assert np.array_equal(va, vb), (what, name, float(np.nanmax(np.abs(va - vb))))


def _mirror_batch(X_rows, hwc, seed, aug):
    """What the device is to write for these rows at this step seed: the NumPy mirror, flat rows again."""
    n = X_rows.shape[0]
    out = augment.apply(X_rows.reshape((n,) + hwc), *augment.draw(seed, n, aug.max_shift, aug.hflip))
    return out.reshape(n, -1)


def _loop(model, hwc, idx, lrs, seed0, aug=None):
    """The per-step loop a run replaces, fed host-augmented batches."""
    hist, batches = [], []
    for i in range(len(idx)):
        Xb = model.X[idx[i]] if not aug else _mirror_batch(model.X[idx[i]], hwc, seed0 + i, aug)
        batches.append(Xb)
        hist.append(model.train_step(Xb, model.Y[idx[i]], lrs[i], seed=seed0 + i))
    return np.array(hist), batches


# ---- 6: the stand-alone call -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C", [(9, 7, 3), (13, 13, 2), (12, 12, 1), (5, 4, 1)])
def test_device_augment_is_the_mirror(ctx, H, W, C):
    """``model.augment`` and the raw entry point on a NaN-filled destination (an unwritten fill value would show) against
    ``augment.apply(X, *augment.draw(seed, N, t, hflip))``: N = 5 and 70, t in {0, 1, 3, min(H, W) - 1}, flip on and off, two seeds."""
    spec = ls.live_spec(S=S, hwc=(H, W, C), convs=[], head=(2, 1), M=5, c=0.5, a=0.3)
    rng = np.random.default_rng(H * 100 + W)
    pool = rng.standard_normal((70, H * W * C))
    m = build_from_spec(spec, pool[:4].copy(), np.zeros(4, np.int32))
    m._build()
    L = dev.lib()
    seen_shift = seen_flip = False
    for N in (5, 70):
        X = pool[:N]
        dX = ctx.to_device(X)
        for t in (0, 1, 3, min(H, W) - 1):
            for hflip in (False, True):
                for seed in (3, 2 ** 32 + 12345):
                    dy, dx, flip = augment.draw(seed, N, t, hflip)
                    want = augment.apply(X.reshape(N, H, W, C), dy, dx, flip)
                    seen_shift |= bool(dy.any() and dx.any())
                    seen_flip |= bool(flip.any())
                    out = ctx.to_device(np.full((N, H, W, C), np.nan))
                    ctx._check(L.dcgp_augment_images(ctx.handle, dX.ptr, N, H, W, C, t, int(hflip), seed, out.ptr))
                    got = out.numpy()
                    assert not np.isnan(got).any(), (N, t, hflip, seed)
                    assert np.array_equal(got, want), (N, t, hflip, seed)
                    m.set_augmentation(Augmentation(t, hflip))
                    for shaped in (X, X.reshape(N, H, W, C)):
                        mine = m.augment(shaped, seed)
                        assert mine.shape == shaped.shape and np.array_equal(mine.reshape(want.shape), want), (N, t, hflip, seed)
                    if t == 0 and not hflip:
                        assert np.array_equal(got, X.reshape(N, H, W, C))
    assert seen_shift and seen_flip
    assert np.array_equal(dX.numpy(), pool[:70])                     # the source is read only
    # refused before any launch: a shift that can leave nothing of the image, a negative one, an aliased destination
    out = ctx.empty((70, H, W, C))
    for bad in (min(H, W), -1):
        assert L.dcgp_augment_images(ctx.handle, dX.ptr, 70, H, W, C, bad, 1, 0, out.ptr) == dev.ERR_ARG
    assert L.dcgp_augment_images(ctx.handle, dX.ptr, 70, H, W, C, 1, 1, 0, dX.ptr) == dev.ERR_ARG
    m.close()


# ---- 7: an augmenting run is the loop on mirror-augmented batches ------------------------------------------------------------------------
def _augmented_run_equals_loop(name, dedup=True, gaussian=False):
    idx, lrs = _tables()
    hwc = _case(name)[1]
    a, b = _model(name, dedup, gaussian), _model(name, dedup, gaussian)
    start = _values(a)
    ha, batches = _loop(a, hwc, idx, lrs, SEED0, AUG)
    # steps 2 and 3 train on the same rows: each step draws afresh, so the two augmented batches differ -- and both differ from the rows
    assert np.array_equal(idx[2], idx[3]) and not np.array_equal(batches[2], batches[3])
    assert not np.array_equal(batches[2], a.X[idx[2]])
    b.attach_dataset()
    b.set_augmentation(AUG)
    assert b.augmentation is AUG
    hb = b.train_run(idx, lrs, seed=SEED0)
    print("%s dedup=%d gaussian=%d: loop %s\n   run %s" % (name, dedup, gaussian, ha, hb))
    assert hb.shape == (STEPS,) and np.all(np.isfinite(ha))
    assert np.array_equal(ha, hb)
    va, vb = _values(a), _values(b)
    _assert_same(va, vb, "after the augmented run")
    assert any(not np.array_equal(v0, v1) for (_, v0), (_, v1) in zip(start, va))
    # one more identical (unaugmented) step on both: its result depends on both moment buffers and on the step count
    ea = a.train_step(a.X[idx[1]], a.Y[idx[1]], 0.004, seed=77)
    eb = b.train_step(b.X[idx[1]], b.Y[idx[1]], 0.004, seed=77)
    assert ea == eb, (ea, eb)
    _assert_same(_values(a), _values(b), "one step after the augmented run")
    b.detach_dataset()
    a.close(), b.close()


@pytest.mark.parametrize("name,dedup", [("g973_M5", True), ("odd_M33", True), ("head_only_M24", True), ("small3_M20", True), ("small3_M20", False),
                                        ("padded_res3", True)])
def test_augmented_run_equals_loop_bit_for_bit(ctx, name, dedup):
    _augmented_run_equals_loop(name, dedup)


def test_augmented_run_equals_loop_with_float_targets(ctx):
    """Gaussian(0.7), targets [23, R]: the targets are gathered untouched beside the augmented images."""
    _augmented_run_equals_loop("small3_M20", gaussian=True)


def test_augmentation_changes_the_run(ctx):
    """(The comparison above would also hold if neither side augmented: the augmented history is not the plain one.)"""
    idx, lrs = _tables()
    a, b = _model("g973_M5"), _model("g973_M5")
    for m in (a, b):
        m.attach_dataset()
    b.set_augmentation(AUG)
    ha, hb = a.train_run(idx, lrs, seed=SEED0), b.train_run(idx, lrs, seed=SEED0)
    assert not np.array_equal(ha, hb)
    a.close(), b.close()


# ---- 8: off means off --------------------------------------------------------------------------------------------------------------------
def test_off_means_off(ctx):
    """One augmented run, then ``set_augmentation(None)``: the next run is that of a model that never had an augmentation set.  (That model
    reaches the same state by one ``train_step`` on the mirror-augmented batch, which the tests above show to be the augmented run's step.)"""
    idx, lrs = _tables()
    hwc = _case("small3_M20")[1]
    was_on, never, plain, zero = (_model("small3_M20") for _ in range(4))
    for m in (was_on, never, plain, zero):
        m.attach_dataset()
    was_on.set_augmentation(Augmentation(2, True))
    was_on.train_run(idx[:1], lrs[:1], seed=SEED0 + 50)
    was_on.set_augmentation(None)
    assert was_on.augmentation is None
    never.train_step(_mirror_batch(never.X[idx[0]], hwc, SEED0 + 50, Augmentation(2, True)), never.Y[idx[0]], lrs[0], seed=SEED0 + 50)
    _assert_same(_values(was_on), _values(never), "before the plain runs")
    h_on, h_never = was_on.train_run(idx, lrs, seed=SEED0), never.train_run(idx, lrs, seed=SEED0)
    assert np.array_equal(h_on, h_never)
    _assert_same(_values(was_on), _values(never), "after the plain runs")
    # t = 0 without flip is likewise the plain run
    zero.set_augmentation(Augmentation(0, False))
    assert zero.augmentation is None
    assert np.array_equal(zero.train_run(idx, lrs, seed=SEED0), plain.train_run(idx, lrs, seed=SEED0))
    _assert_same(_values(zero), _values(plain), "t = 0, no flip")
    for m in (was_on, never, plain, zero):
        m.close()


# ---- 9: errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_raise_before_any_launch(ctx):
    idx, lrs = _tables()
    m = _model("g973_M5")                       # 9 x 7 x 3: min(H, W) = 7
    m.attach_dataset()
    before = _values(m)
    L = dev.lib()
    for bad in (7, 8):
        with pytest.raises(ValueError, match="max_shift"):
            m.set_augmentation(Augmentation(bad, True))
        assert L.dcgp_model_set_augmentation(m._model, 9, 7, 3, bad, 1) == dev.ERR_ARG      # ... says the library as well
    with pytest.raises(ValueError):
        m.set_augmentation(Augmentation(-1))
    neg = Augmentation(1, True)
    neg.max_shift = -1                           # past the value object's own check
    with pytest.raises(ValueError, match="max_shift"):
        m.set_augmentation(neg)
    assert L.dcgp_model_set_augmentation(m._model, 9, 7, 3, -1, 0) == dev.ERR_ARG
    assert L.dcgp_model_set_augmentation(m._model, 7, 9, 2, 1, 0) == dev.ERR_ARG            # 126 values: not the model's 189
    assert m.augmentation is None
    # steps enqueued and not yet collected
    ticket = m.enqueue_log_likelihood(m.X[idx[0]], m.Y[idx[0]], seed=1)
    with pytest.raises(ValueError, match="collected"):
        m.set_augmentation(AUG)
    assert m.augmentation is None
    assert np.isfinite(m.collect_log_likelihood(ticket))
    _assert_same(_values(m), before, "after the refused calls")
    # nothing of the refused calls stuck: the run is the plain run ...
    ref = _model("g973_M5")
    ref.attach_dataset()
    assert np.array_equal(m.train_run(idx[:2], lrs[:2], seed=SEED0), ref.train_run(idx[:2], lrs[:2], seed=SEED0))
    # ... and the model still trains, augmented too
    m.set_augmentation(AUG)
    hist = m.train_run(idx, lrs, seed=SEED0)
    assert hist.shape == (STEPS,) and np.all(np.isfinite(hist))
    m.close(), ref.close()


# ---- 10: the driver ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer", ["Adam", "SGD"])
def test_driver_with_the_flags(ctx, tmp_path, optimizer):
    """ArrayExperiment on 200 + 60 digits with --augment-shift 1 --augment-flip, two periods of 20 steps: finite log rows, the flags in
    options.toml, and a second experiment with the same seed reproduces the ELBOs exactly."""
    from sklearn.datasets import load_digits
    from deepcgp_amd.experiment import ArrayExperiment, read_args, standardise
    d = load_digits()
    Xtr, Xte = standardise(d.images[:200], d.images[200:260])
    Ytr, Yte = d.target[:200], d.target[200:260]
    args = ["--data", "unused", "--log-dir", str(tmp_path), "-M", "16,16", "--feature-maps", "2", "--filter-sizes", "3,3", "--strides", "1,1",
            "--batch-size", "16", "--num-samples", "2", "--test-every", "20", "--test-size", "60", "--optimizer", optimizer, "--lr", "0.001",
            "--augment-shift", "1", "--augment-flip"]
    elbos = []
    for name in ("run", "again"):
        np.random.seed(0)
        exp = ArrayExperiment(read_args(["--name", name] + args), Xtr, Ytr, Xte, Yte)
        assert (exp.augmentation.max_shift, exp.augmentation.hflip) == (1, True)
        if optimizer == "Adam":
            assert exp.model.augmentation is exp.augmentation
        try:
            exp.train_step()
            first = np.array(exp.last_elbos)
            exp.train_step()
        finally:
            exp.conclude()
        assert exp.global_step == 40 and len(exp.last_elbos) == 20 and np.all(np.isfinite(exp.last_elbos))
        elbos.append(np.concatenate([first, np.array(exp.last_elbos)]))
        with open(os.path.join(str(tmp_path), name, "log.csv"), newline="") as f:
            rows = list(csv.reader(f))
        print(optimizer, rows)
        assert len(rows) == 3 and all(np.isfinite(float(v)) for r in rows[1:] for v in r)
        lines = open(os.path.join(str(tmp_path), name, "options.toml")).read().splitlines()
        assert "augment_shift = 1" in lines and "augment_flip = true" in lines
        exp.model.close()
    assert np.array_equal(elbos[0], elbos[1])
