"""Training-time augmentation without a GPU: the index map and the draw of csrc/augment_map.h (compiled with the host C++ compiler,
tests/augment_map_check.cc) against an independent NumPy formulation -- np.flip on the W axis, np.pad by t, a slice -- and against
deepcgp_amd/augment.py, the NumPy mirror; the mirror's ``apply`` against the same formulation; the flags, options.toml, and the host branches
of ``models.train`` on a stub model.  Every comparison is ``np.array_equal``: the transform only moves values."""
import argparse
import os
import shutil
import subprocess

import numpy as np
import pytest

from deepcgp_amd import augment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(9, 7, 3), (13, 13, 2), (12, 12, 1), (5, 4, 1)]     # odd W: a pixel on the flip axis; H != W: a swapped axis shows
SEEDS = [0, 1, 11, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63 + 5, 2 ** 64 - 1]


def shifts(H, W):
    return [0, 1, 3, min(H, W) - 1]         # the last one leaves a single surviving row or column


def reference(img, dy, dx, flip, t, fill):
    """One image [H, W, C] by np.flip, np.pad and a slice: out[y][x] = F[y - dy][x - dx] is the padded F at [y - dy + t][x - dx + t]."""
    H, W, _ = img.shape
    F = np.flip(img, axis=1) if flip else img
    P = np.pad(F, ((t, t), (t, t), (0, 0)), constant_values=fill)
    return P[t - dy:t - dy + H, t - dx:t - dx + W]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("augment_map") / "augment_map_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "deepcgp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "augment_map_check.cc"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("H,W,C", GEOMETRIES)
def test_index_map_is_flip_pad_slice(check_exe, H, W, C):
    """Every destination index, every (dy, dx) of [-t, t]^2 for every t of the list, both flips."""
    tmax = max(shifts(H, W))
    r = subprocess.run([check_exe, "map"] + [str(v) for v in (H, W, C, tmax)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = {}
    for line in r.stdout.splitlines():
        v = np.array(line.split(), np.int64)
        got[tuple(v[:3])] = v[3:]
    assert len(got) == (2 * tmax + 1) ** 2 * 2
    src = np.arange(H * W * C).reshape(H, W, C)
    checked = 0
    for t in shifts(H, W):
        for dy in range(-t, t + 1):
            for dx in range(-t, t + 1):
                for flip in (0, 1):
                    want = reference(src, dy, dx, flip, t, -1)
                    assert got[(dy, dx, flip)].shape == (H * W * C,)
                    assert np.array_equal(got[(dy, dx, flip)], want.reshape(-1)), (t, dy, dx, flip)
                    checked += 1
    assert checked >= len(got)
    # t = min(H, W) - 1: something of the image always survives, and at the extreme shift along the short axis exactly one line of it
    t = tmax
    assert all((m >= 0).any() for m in got.values())
    if H <= W:
        assert (got[(t, 0, 0)] >= 0).sum() == W * C
    if W <= H:
        assert (got[(0, t, 1)] >= 0).sum() == H * C


@pytest.mark.parametrize("t", [0, 1, 4])
@pytest.mark.parametrize("hflip", [0, 1])
def test_the_header_draws_what_the_mirror_draws(check_exe, t, hflip):
    n = 70
    r = subprocess.run([check_exe, "draw", str(t), str(hflip), str(n)] + [str(s) for s in SEEDS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(SEEDS)
    for seed, line in zip(SEEDS, lines):
        got = np.array(line.split(), np.int64).reshape(n, 3)
        dy, dx, flip = augment.draw(seed, n, t, bool(hflip))
        assert dy.shape == dx.shape == flip.shape == (n,) and dy.dtype.kind == dx.dtype.kind == flip.dtype.kind == "i"
        assert np.array_equal(got[:, 0], dy) and np.array_equal(got[:, 1], dx) and np.array_equal(got[:, 2], flip), seed
        assert np.abs(dy).max() <= t and np.abs(dx).max() <= t and set(flip) <= {0, 1}
        if not hflip:
            assert not flip.any()
        if t == 0:
            assert not dy.any() and not dx.any()


def test_philox_mirror_is_the_published_generator():
    """Random123's known-answer vectors of Philox4x32-10 (counter, key -> output): the mirror, and through the test above the header, are
    the generator the name says, not merely equal to each other."""
    got = augment.philox4x32_10(0, 0, 0, 0, 0)
    assert [int(w) for w in got] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    got = augment.philox4x32_10(0xffffffffffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)
    assert [int(w) for w in got] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    got = augment.philox4x32_10((0x299f31d0 << 32) | 0xa4093822, 0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344)
    assert [int(w) for w in got] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


@pytest.mark.parametrize("H,W,C", GEOMETRIES)
def test_apply_is_flip_pad_slice(H, W, C):
    rng = np.random.default_rng(H * 100 + W)
    for t in shifts(H, W):
        combos = [(dy, dx, f) for dy in range(-t, t + 1) for dx in range(-t, t + 1) for f in (0, 1)]
        X = rng.standard_normal((len(combos), H, W, C))
        dy, dx, flip = (np.array(v) for v in zip(*combos))
        got = augment.apply(X, dy, dx, flip)
        assert got.shape == X.shape and got.dtype == X.dtype
        for b, (y, x, f) in enumerate(combos):
            assert np.array_equal(got[b], reference(X[b], y, x, f, t, 0.0)), (t, y, x, f)
    X = rng.standard_normal((3, H, W, C))
    keep = X.copy()
    same = augment.apply(X, np.zeros(3, int), np.zeros(3, int), np.zeros(3, int))
    assert np.array_equal(same, X) and same is not X and np.array_equal(X, keep)


def test_draws_are_usable():
    """seed 0, t = 2, 4096 positions: each of the five values of dy and of dx has frequency 0.2 with standard deviation
    sqrt(0.2 * 0.8 / 4096) = 0.006; the band [0.15, 0.25] is eight of those.  The flip frequency (sd 0.008) lies in [0.45, 0.55]."""
    n, t = 4096, 2
    dy, dx, flip = augment.draw(0, n, t, True)
    for name, d in (("dy", dy), ("dx", dx)):
        freq = [(d == v).mean() for v in range(-t, t + 1)]
        print(name, freq)
        assert all(0.15 <= f <= 0.25 for f in freq) and abs(sum(freq) - 1.0) < 1e-12
    print("flip", flip.mean())
    assert 0.45 <= flip.mean() <= 0.55
    assert not np.array_equal(dy, dx)
    for s in (0, 7, 2 ** 32 - 1, 2 ** 40):
        a, b = augment.draw(s, n, t, True), augment.draw(s + 1, n, t, True)
        assert all(not np.array_equal(u, v) for u, v in zip(a, b)), s
    # a position's draw does not depend on how many positions are drawn
    assert all(np.array_equal(u[:70], v) for u, v in zip(augment.draw(5, 4096, t, True), augment.draw(5, 70, t, True)))


def test_augmentation_value_object():
    A = augment.Augmentation
    assert not A() and not A(0, False) and A(1) and A(0, True) and A(4, True)
    assert (A().max_shift, A().hflip) == (0, False) and (A(4, True).max_shift, A(4, True).hflip) == (4, True)
    with pytest.raises(ValueError):
        A(-1)
    with pytest.raises(ValueError):
        augment.draw(0, 4, -1, False)


def _flags(*extra):
    from deepcgp_amd.arguments import default_parser
    return default_parser().parse_args(["--name", "t"] + list(extra))


def test_flags_and_options_toml(tmp_path):
    from deepcgp_amd import utils
    from deepcgp_amd.arguments import parse_augmentation
    fl = _flags()
    assert fl.augment_shift == 0 and fl.augment_flip is False and not parse_augmentation(fl)
    assert not parse_augmentation(argparse.Namespace())                     # flags from before the feature
    a = parse_augmentation(_flags("--augment-shift", "4", "--augment-flip"))
    assert a and (a.max_shift, a.hflip) == (4, True)
    a = parse_augmentation(_flags("--augment-flip"))
    assert a and (a.max_shift, a.hflip) == (0, True)
    with pytest.raises(ValueError, match="--augment-shift"):
        parse_augmentation(_flags("--augment-shift", "-1"))
    log = utils.Log(str(tmp_path), "run", [])
    log.write_flags(_flags("--augment-shift", "4", "--augment-flip"))
    log.close()
    lines = (tmp_path / "run" / "options.toml").read_text().splitlines()
    assert "augment_shift = 4" in lines and "augment_flip = true" in lines, lines
    back = {}
    for l in lines:                          # flat key = value lines (tests/test_host_experiment.py pins the format)
        if l.startswith("augment_"):
            k, v = l.split(" = ")
            back[k] = {"true": True, "false": False}.get(v, v)
    b = parse_augmentation(argparse.Namespace(augment_shift=int(back["augment_shift"]), augment_flip=back["augment_flip"]))
    assert (b.max_shift, b.hflip) == (4, True)
    try:
        import tomli
    except ImportError:
        return
    b = parse_augmentation(argparse.Namespace(**tomli.loads("\n".join(lines))))
    assert (b.max_shift, b.hflip) == (4, True)


def test_dense_head_only_model_has_no_image_geometry():
    """A head-only ``--last-kernel rbf`` model takes feature vectors: set_augmentation says so before it touches the device."""
    from deepcgp_amd.models import build_from_spec
    import live_specs as ls
    spec = ls.live_spec(hwc=(6, 6, 1), convs=[], head=(3, 1), M=8, c=0.5, a=0.3, head_kernel="rbf")
    m = build_from_spec(spec, np.zeros((4, 36)), np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="dense head"):
        m.set_augmentation(augment.Augmentation(1, True))
    assert m._model is None and m.augmentation is None
    m.set_augmentation(None)                 # nothing to switch off, nothing built
    assert m._model is None
    # a model with images knows its shift's upper bound without the device as well
    # (a patch head alone: a conv layer's constructor already factors its prior on the device)
    conv = build_from_spec(ls.live_spec(hwc=(9, 7, 3), convs=[], head=(2, 1), M=5, c=1.0, a=0.1), np.zeros((4, 189)), np.zeros(4, np.int32))
    assert conv._image_geometry() == (9, 7, 3)
    for bad in (7, 8, 100):
        with pytest.raises(ValueError, match="max_shift"):
            conv._checked_augmentation(augment.Augmentation(bad))
    assert conv._checked_augmentation(augment.Augmentation(6, True)) == (9, 7, 3, 6, 1)
    assert conv._model is None


class _StubModel:
    """Records what ``models.train`` asks of a model."""
    minibatch_size = 4
    dedup_layer0 = False
    layers = [None, None]

    def __init__(self, augmentation=None):
        self.X = np.arange(30.0).reshape(10, 3)
        self.Y = np.arange(10)
        self.augmentation = augmentation
        self.calls = []
        self._ctx = object()

    def _build(self):
        pass

    def set_trainable(self, *a):
        pass

    def set_augmentation(self, aug):
        self.calls.append(("set_augmentation", aug))
        self.augmentation = aug if aug else None

    def augment(self, X, seed):
        self.calls.append(("augment", np.array(X), seed))
        return -np.asarray(X)

    def compute_gradients(self, X, Y, seed=0, fetch=True):
        self.calls.append(("grad", np.array(X), np.array(Y), seed))
        return 1.5, None

    def natgrad_step(self, gamma):
        self.calls.append(("natgrad",))

    def sgd_step(self, lr):
        self.calls.append(("sgd",))

    def adam_step(self, lr):
        self.calls.append(("adam",))

    def pull_parameters(self):
        self.calls.append(("pull",))


@pytest.mark.parametrize("optimizer", ["SGD", "NatGrad"])
def test_host_branches_of_train_augment_with_seed_plus_step(optimizer):
    from deepcgp_amd.models import train
    aug, earlier = augment.Augmentation(2, True), augment.Augmentation(1)
    m = _StubModel(earlier)
    hist = train(m, 3, global_step=40, seed=9, optimizer=optimizer, augment=aug)
    assert hist == [1.5] * 3
    rng = np.random.default_rng(9)
    sets = [c for c in m.calls if c[0] == "set_augmentation"]
    assert [c[1] for c in sets] == [aug, earlier] and m.augmentation is earlier          # set for the span, restored behind it
    assert m.calls[0][0] == "set_augmentation" and [c[0] for c in m.calls[-2:]] == ["set_augmentation", "pull"]
    augs, grads = [c for c in m.calls if c[0] == "augment"], [c for c in m.calls if c[0] == "grad"]
    assert len(augs) == 3 and len(grads) == (6 if optimizer == "NatGrad" else 3)
    per = len(grads) // 3
    for i in range(3):
        idx = rng.choice(10, size=4, replace=False)
        assert np.array_equal(augs[i][1], m.X[idx]) and augs[i][2] == 9 + 40 + i
        for g in grads[per * i:per * (i + 1)]:                                            # every gradient of the step sees the augmented batch
            assert np.array_equal(g[1], -m.X[idx]) and np.array_equal(g[2], m.Y[idx]) and g[3] == 9 + 40 + i
    # no augmentation anywhere: the branch never asks for one
    m = _StubModel()
    train(m, 2, seed=9, optimizer=optimizer)
    assert not [c for c in m.calls if c[0] in ("augment", "set_augmentation")]
    rng = np.random.default_rng(9)
    for g in [c for c in m.calls if c[0] == "grad"][::per]:
        assert np.array_equal(g[1], m.X[rng.choice(10, size=4, replace=False)])
    # augment=None leaves what the model has set in force
    m = _StubModel(earlier)
    train(m, 2, seed=9, optimizer=optimizer)
    assert len([c for c in m.calls if c[0] == "augment"]) == 2 and not [c for c in m.calls if c[0] == "set_augmentation"]


def test_header_declares_the_entries():
    from deepcgp_amd import device as dev
    declared = dev.declared_symbols()
    for name in ("dcgp_model_set_augmentation", "dcgp_augment_images"):
        assert name in declared and name in dev._SIGS
