"""Dilation without a GPU: the index map of csrc/dilate_map.h against NumPy slicing ``x[:, a::d, b::d]`` and its inverse, FullView's dilated
geometry and refusals, the host split around the patch extraction (``view.split`` / ``view.merge``) against ``torch.nn.functional.unfold(...,
dilation=d)``, --dilations, ``ModelBuilder.spec()`` carrying ``dil``, the options.toml record, and the reference helper checking itself
(tests/dilation_ref.py).  ``extract_patches`` itself calls the device: tests/test_gpu_dilation.py compares it with ``unfold``."""
import argparse
import os
import shutil
import subprocess

import numpy as np
import pytest

import dilation_ref as dr
import stack_specs as ss
import torch_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (H, W, C, f, d) of the issue's identity check; d^2 P' / P is 1 where d divides both sides, 1.19 for 17 x 17 d3, 1.6 for 9 x 7 d2
SHAPES = [(10, 10, 1, 3, 2), (9, 7, 3, 3, 2), (17, 17, 1, 3, 3), (12, 12, 2, 3, 2), (28, 28, 1, 5, 2), (11, 8, 2, 2, 3)]


@pytest.fixture(scope="module")
def dilate_map_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("dilate_map") / "dilate_map_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "deepcgp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "dilate_map_check.cc"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("H,W,C,d", [(9, 7, 3, 2), (17, 17, 1, 3), (11, 8, 2, 3), (6, 5, 2, 1), (1, 1, 1, 3), (10, 10, 1, 2)])
def test_index_map_is_numpy_slicing_and_its_inverse(dilate_map_exe, H, W, C, d):
    """Every index of the phase batch and every index of the image batch, two images.  (1 x 1 d3: the output image of 7 x 7 f3 d3, one pixel in
    phase (0, 0) and eight sub-images of fill.)"""
    rows = 2
    r = subprocess.run([dilate_map_exe] + [str(v) for v in (rows, H, W, C, d)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fwd, inv = [np.array(l.split(), np.int64) for l in r.stdout.splitlines()]
    src = np.arange(rows * H * W * C).reshape(rows, H, W, C)
    Hs, Ws = -(-H // d), -(-W // d)
    want = -np.ones((rows, d, d, Hs, Ws, C), np.int64)
    for a in range(d):
        for b in range(d):
            t = src[:, a::d, b::d]
            want[:, a, b, :t.shape[1], :t.shape[2]] = t
    assert fwd.size == rows * d * d * Hs * Ws * C and np.array_equal(fwd, want.reshape(-1))
    # the inverse: every image index once, at the place the forward map reads it from
    assert inv.size == src.size and np.array_equal(fwd[inv], np.arange(src.size))
    assert np.count_nonzero(fwd >= 0) == src.size
    # the kernels' own reading: s2b fills with zeros, b2s(s2b(x)) == x, and b2s never reads a fill entry
    x = np.random.default_rng(0).standard_normal(src.size)
    sub = np.where(fwd < 0, 0.0, x[np.maximum(fwd, 0)])
    assert np.array_equal(sub.reshape(rows * d * d, Hs, Ws, C), dr.s2b(x.reshape(src.shape), d))
    poisoned = np.where(fwd < 0, np.nan, sub)
    assert np.array_equal(poisoned[inv], x)
    if d == 1:
        assert np.array_equal(fwd, np.arange(src.size)) and np.array_equal(inv, fwd)


def test_full_view_geometry_and_refusals():
    from deepcgp_amd.views import FullView
    for H, W, C, f, d in SHAPES + [(7, 7, 1, 3, 3)]:
        for p in (0, 2):
            v = FullView((H, W), f, C, 1, padding=p, dilation=d)
            ho, wo = H + 2 * p - d * (f - 1), W + 2 * p - d * (f - 1)
            assert v.dilation == d and v.padded_size == [H + 2 * p, W + 2 * p]
            assert (v.out_image_height, v.out_image_width, v.patch_count, v.patch_length) == (ho, wo, ho * wo, f * f * C)
            assert v.phase_size == [-(-(H + 2 * p) // d), -(-(W + 2 * p) // d)]
            assert -(-ho // d) == v.phase_size[0] - f + 1 and -(-wo // d) == v.phase_size[1] - f + 1      # ceil(Ho / d) = Hs - f + 1 exactly
            assert v.as_maps(np.zeros((3, ho * wo, 4))).shape == (3, ho, wo, 4)
    v0 = FullView((8, 8), 3, 1)
    assert v0.dilation == 1 and v0.phase_size == [8, 8] and v0.patch_count == 36
    x = np.zeros((1, 8, 8, 1))
    assert v0.split(x) is x and v0.merge(x, 8, 8) is x
    assert FullView((7, 7), 3, 1, dilation=3).patch_count == 1      # the window fits exactly once
    for bad in (dict(dilation=0), dict(dilation=-1), dict(dilation=1.5), dict(dilation=2, stride=2), dict(dilation=4)):
        with pytest.raises(ValueError):
            FullView((7, 7), 3, 1, **bad)                            # d = 4: a span of 9 on 7 pixels
    assert FullView((7, 7), 3, 1, dilation=4, padding=1).patch_count == 1


@pytest.mark.parametrize("H,W,C,f,d", SHAPES)
def test_host_split_around_the_patch_extraction_is_unfold(H, W, C, f, d):
    """What ``FullView._extract`` does around dcgp_extract_patches -- split, ordinary patches of the sub-images, merge in image order --
    with NumPy patches in the device call's place: patch for patch the dilated patches of ``unfold``, same values."""
    torch = pytest.importorskip("torch")
    from deepcgp_amd.views import FullView
    x = np.random.default_rng(H * W).standard_normal((2, H, W, C))
    v = FullView((H, W), f, C, 1, dilation=d)
    sub = v.split(x)
    assert np.array_equal(sub, dr.s2b(x, d)) and np.array_equal(v.merge(sub, H, W), x)
    pat = v.merge(dr.numpy_patches(sub, f), v.out_image_height, v.out_image_width).reshape(2, v.patch_count, v.patch_length)
    want = dr.torch_patches(torch.tensor(x), f, 1, d).numpy()
    assert np.array_equal(pat, want)
    # the reference helper checks itself: b2s(patches(s2b(x))) == unfold(x, dilation = d)
    got = dr.b2s(dr.numpy_patches(dr.s2b(x, d), f), d, v.out_image_height, v.out_image_width).reshape(want.shape)
    assert np.array_equal(got, want) and np.array_equal(dr.numpy_patches(x, f, d).reshape(want.shape), want)
    Hs, Ws = v.phase_size
    ratio = d * d * (Hs - f + 1) * (Ws - f + 1) / v.patch_count
    print("%d x %d x %d f%d d%d: d^2 P' / P = %.3f" % (H, W, C, f, d, ratio))
    assert ratio >= 1.0 and (ratio == 1.0) == (H % d == 0 and W % d == 0)


def _flags(*extra):
    from deepcgp_amd.arguments import default_parser
    return default_parser().parse_args(["--name", "t", "-M", "5,6,7", "--feature-maps", "2,2", "--filter-sizes", "3,3,3", "--strides", "1,1,1",
                                        "--num-samples", "2", "--batch-size", "4"] + list(extra))


def test_dilations_flag_and_its_errors():
    from deepcgp_amd.arguments import default_parser, parse_dilations
    from deepcgp_amd.models import ModelBuilder
    assert default_parser().parse_args(["--name", "x"]).dilations == ""
    assert parse_dilations(_flags(), 2) == [1, 1]
    assert parse_dilations(_flags("--dilations", "2,1"), 2) == [2, 1]
    assert ModelBuilder(_flags("--dilations", "1,2"), np.zeros((4, 12, 12, 1)), np.zeros(4)).dilations() == [1, 2]
    for bad in ("2", "2,1,1", "2,0", "2,-1", "2,x", "2,,1", "1.5,1"):
        with pytest.raises(ValueError, match="--dilations"):
            parse_dilations(_flags("--dilations", bad), 2)
    with pytest.raises(ValueError, match="--dilations.*--strides"):
        parse_dilations(_flags("--dilations", "1,2", "--strides", "1,2,1"), 2)
    assert parse_dilations(_flags("--dilations", "2,1", "--strides", "1,2,1"), 2) == [2, 1]      # the strided layer is not the dilated one
    with pytest.raises(ValueError, match="--dilations"):
        ModelBuilder(_flags("--dilations", "2"), np.zeros((4, 12, 12, 1)), np.zeros(4)).spec()


def test_model_builder_spec_carries_dil_and_chains_the_dilated_geometry(monkeypatch):
    """(Lloyd's iterations run on the device: here the first M rows of the patch sample stand in for the centres.)  14 x 14 x 1 -> f3 d2 p2
    (resolution kept) -> 14 x 14 x 2 -> f3 d3 -> 8 x 8 x 2 -> head f3 (P = 36).  The initialisation images go through the dilated identity
    convolution: output Hp - d (f - 1), centre tap at d * (f // 2)."""
    from deepcgp_amd import kernels
    from deepcgp_amd.models import ModelBuilder, filter_conv, identity_conv
    monkeypatch.setattr(kernels, "kmeans", lambda sample, k, **kw: np.array(sample[:k]))
    rng = np.random.default_rng(0)
    np.random.seed(0)
    X = rng.standard_normal((30, 14, 14, 1))
    spec = ModelBuilder(_flags("--dilations", "2,3", "--paddings", "2,0,0", "--identity-mean"), X, rng.integers(0, 10, (30, 1))).spec()
    got = [(c["H"], c["W"], c["C"], c["pad"], c["dil"]) for c in spec["convs"]] + [tuple(spec["head"][k] for k in ("H", "W", "C"))]
    assert got == [(14, 14, 1, 2, 2), (14, 14, 2, 0, 3), (8, 8, 2)], got
    assert "dil" not in spec["head"]
    from deepcgp_amd.views import FullView      # (the views build_layers_from_spec makes; the layers themselves need the device)
    views = [FullView((c["H"], c["W"]), c["f"], c["C"], c["s"], padding=c["pad"], dilation=c["dil"]) for c in spec["convs"]]
    assert [(v.dilation, v.out_image_height, v.phase_size) for v in views] == [(2, 14, [9, 9]), (3, 8, [5, 5])]
    h = spec["head"]
    assert FullView((h["H"], h["W"], h["C"]), h["f"], h["C"], h["s"]).patch_count == 36
    assert [c["Z"].shape for c in spec["convs"]] == [(5, 9), (6, 18)]
    spec0 = ModelBuilder(_flags(), X, np.zeros((30, 1))).spec()
    assert [c["dil"] for c in spec0["convs"]] == [1, 1] and [c["H"] for c in spec0["convs"]] == [14, 12]
    # the propagation helpers: the centre tap of the dilated window / the filter's taps d apart
    x = rng.standard_normal((5, 9, 7, 2))
    np.random.seed(1)
    a = identity_conv(x, 3, 2, 3, 1, count=5, dilation=2)
    np.random.seed(1)
    pick = x[np.random.choice(np.arange(5), size=5)]
    assert a.shape == (5, 5, 3, 3) and np.array_equal(a[..., 0], pick[:, 2:7, 2:5, :].sum(-1))
    Wf = rng.standard_normal((3, 3, 2, 4))
    np.random.seed(1)
    b = filter_conv(x, Wf, 1, count=5, dilation=2)
    want = dr.numpy_patches(pick, 3, 2) @ Wf.reshape(18, 4)
    assert b.shape == (5, 5, 3, 4) and np.allclose(b, want, rtol=0, atol=1e-12)


def test_inducing_candidates_are_dilated_windows():
    """``draw_patches(..., dilation=d)``: every candidate is a dilated window of one of the images -- on images whose pixel value encodes its
    position the taps sit d apart; and the draws of dilation 1 are the draws of before."""
    from deepcgp_amd.models import draw_patches
    H, W = 9, 8
    X = (np.arange(H)[:, None] * 100 + np.arange(W)[None, :]).astype(np.float64)[None, :, :, None].repeat(3, 0)
    got = draw_patches(X, 50, 3, np.random.RandomState(0), dilation=2).reshape(50, 3, 3)
    assert np.all(got[:, 1, 0] - got[:, 0, 0] == 200) and np.all(got[:, 0, 1] - got[:, 0, 0] == 2)
    assert got.max() <= (H - 1) * 100 + W - 1
    assert np.array_equal(draw_patches(X, 50, 3, np.random.RandomState(0), dilation=1), draw_patches(X, 50, 3, np.random.RandomState(0)))


def test_options_toml_records_the_flag(tmp_path):
    from deepcgp_amd import utils
    from deepcgp_amd.arguments import parse_dilations
    for i, (extra, want) in enumerate(((("--dilations", "2,1"), 'dilations = "2,1"'), ((), 'dilations = ""'))):
        log = utils.Log(str(tmp_path), "run%d" % i, [])
        log.write_flags(_flags(*extra))
        log.close()
        lines = (tmp_path / ("run%d" % i) / "options.toml").read_text().splitlines()
        assert want in lines, lines
        try:
            import tomli
        except ImportError:
            continue
        back = argparse.Namespace(**tomli.loads("\n".join(lines)))
        assert parse_dilations(back, 2) == parse_dilations(_flags(*extra), 2)


@pytest.mark.parametrize("name", ["dil2", "dil2_odd", "dil3_pad", "two_dilated"])
def test_torch_forward_of_the_stacks_is_live_and_has_the_dilated_sizes(name):
    """The torch reference on the table's stacks: finite parts, every layer's output of the dilated view's size, and every gradient group live
    (tests/live_specs.py's measures) -- so that a dead group cannot pass the GPU comparison vacuously."""
    pytest.importorskip("torch")
    import live_specs as ls
    spec, X, Y, zs = dr.make_stack(name)
    ref = tr.reference(spec, X, Y, zs)
    assert all(np.isfinite(ref["parts"]))
    assert [m.shape[-1] for m in ref["means"]] == [o for _, o in ss.output_dims(spec)]
    ls.assert_live(name, ref["want"])
