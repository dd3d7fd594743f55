"""Zero padding without a GPU: the index map of csrc/pad_map.h against np.pad, FullView's padded geometry, --paddings, the geometry chain of
ModelBuilder.spec(), the options.toml round trip, and the padded oracle (an unmodified oracle layer on the padded view behind np.pad,
tests/padding_ref.py) against the torch forward with F.pad."""
import argparse
import os
import shutil
import subprocess

import numpy as np
import pytest

import padding_ref as pr
import stack_specs as ss
import torch_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pad_map_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pad_map") / "pad_map_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "deepcgp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "pad_map_check.cc"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("H,W,C,p", [(9, 7, 3, 1), (9, 7, 3, 2), (5, 5, 2, 1), (4, 4, 1, 3)])
def test_index_map_is_np_pad_and_its_adjoint(pad_map_exe, H, W, C, p):
    """Every index of the padded batch and every index of the source batch, two images."""
    rows = 2
    r = subprocess.run([pad_map_exe] + [str(v) for v in (rows, H, W, C, p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fwd, adj = [np.array(l.split(), np.int64) for l in r.stdout.splitlines()]
    src = np.arange(rows * H * W * C).reshape(rows, H, W, C)
    want = np.pad(src, ((0, 0), (p, p), (p, p), (0, 0)), constant_values=-1)
    assert np.array_equal(fwd, want.reshape(-1))
    # the adjoint: crop(y)[j] = y[adj[j]] is y's interior ...
    y = np.random.default_rng(0).standard_normal(want.shape)
    assert np.array_equal(y.reshape(-1)[adj], y[:, p:-p, p:-p, :].reshape(-1))
    # ... and <pad(x), y> == <x, crop(y)> with the kernels' own reading of the map
    x = np.random.default_rng(1).standard_normal(src.size)
    padded = np.where(fwd < 0, 0.0, x[np.maximum(fwd, 0)])
    assert np.array_equal(padded.reshape(want.shape), np.pad(x.reshape(src.shape), ((0, 0), (p, p), (p, p), (0, 0))))
    assert abs(padded @ y.reshape(-1) - x @ y.reshape(-1)[adj]) <= 1e-12 * np.abs(x).sum() * np.abs(y).max()


def test_full_view_geometry():
    from deepcgp_amd.views import FullView
    for H, W, f, s, p in [(9, 7, 4, 2, 2), (10, 10, 3, 2, 1), (28, 28, 5, 2, 2), (4, 4, 5, 1, 1), (7, 5, 4, 3, 1)]:
        assert (H + 2 * p - f) % s != 0 or (H, f) == (4, 5)
        v = FullView((H, W), f, 2, s, padding=p)
        ho, wo = (H + 2 * p - f) // s + 1, (W + 2 * p - f) // s + 1
        assert v.input_size == [H, W] and v.padding == p and v.padded_size == [H + 2 * p, W + 2 * p]
        assert (v.out_image_height, v.out_image_width, v.patch_count, v.patch_length) == (ho, wo, ho * wo, f * f * 2)
        assert v.as_maps(np.zeros((3, ho * wo, 4))).shape == (3, ho, wo, 4)
        x = np.random.default_rng(0).standard_normal((2, H, W, 2))
        assert np.array_equal(v.pad(x), np.pad(x, ((0, 0), (p, p), (p, p), (0, 0))))
    v0 = FullView((8, 8), 3, 1)
    assert v0.padding == 0 and v0.padded_size == [8, 8] and v0.patch_count == 36
    x = np.zeros((1, 8, 8, 1))
    assert v0.pad(x) is x
    with pytest.raises(ValueError):
        FullView((4, 4), 7, 1, padding=1)       # 6 x 6 padded: the filter still does not fit
    with pytest.raises(ValueError):
        FullView((4, 4), 3, 1, padding=-1)


def _flags(*extra):
    from deepcgp_amd.arguments import default_parser
    return default_parser().parse_args(["--name", "t", "-M", "5,6,7", "--feature-maps", "2,2", "--filter-sizes", "3,3,3", "--strides", "1,2,1",
                                        "--num-samples", "2", "--batch-size", "4"] + list(extra))


def test_paddings_flag_and_its_errors():
    from deepcgp_amd.arguments import default_parser, parse_paddings
    from deepcgp_amd.models import ModelBuilder
    assert default_parser().parse_args(["--name", "x"]).paddings == ""
    assert parse_paddings(_flags(), 3) == [0, 0, 0]
    assert parse_paddings(_flags("--paddings", "1,0,2"), 3) == [1, 0, 2]
    assert ModelBuilder(_flags("--paddings", "1,1,0"), np.zeros((4, 10, 10, 1)), np.zeros(4)).paddings() == [1, 1, 0]
    for bad in ("1,1", "1,1,1,1", "1,-1,0", "1,x,0", "1,,0"):
        with pytest.raises(ValueError, match="--paddings"):
            parse_paddings(_flags("--paddings", bad), 3)
    with pytest.raises(ValueError, match="--paddings"):
        parse_paddings(_flags("--paddings", "1,0,1", "--last-kernel", "rbf"), 3)
    assert parse_paddings(_flags("--paddings", "1,1,0", "--last-kernel", "rbf"), 3) == [1, 1, 0]
    with pytest.raises(ValueError, match="--paddings"):
        ModelBuilder(_flags("--paddings", "1,1"), np.zeros((4, 10, 10, 1)), np.zeros(4)).spec()


def test_model_builder_spec_chains_the_padded_geometry(monkeypatch):
    """(Lloyd's iterations run on the device: here the first M rows of the patch sample stand in for the centres.)  10 x 10 x 1 -> f3 s1 p1 -> 10 x 10 x 2 -> f3 s2 p1 -> 5 x 5 x 2 -> head f3 p1 (P = 25): H, W stay unpadded, ``pad`` carries the border,
    the inducing patches have the patch length of their layer, and the layers built from the spec have the chained views."""
    from deepcgp_amd import kernels
    from deepcgp_amd.models import ModelBuilder, build_layers_from_spec
    monkeypatch.setattr(kernels, "kmeans", lambda sample, k, **kw: np.array(sample[:k]))
    rng = np.random.default_rng(0)
    np.random.seed(0)
    X = rng.standard_normal((30, 10, 10, 1))
    spec = ModelBuilder(_flags("--paddings", "1,1,1", "--identity-mean"), X, rng.integers(0, 10, (30, 1))).spec()
    got = [(c["H"], c["W"], c["C"], c["pad"]) for c in spec["convs"]] + [tuple(spec["head"][k] for k in ("H", "W", "C", "pad"))]
    assert got == [(10, 10, 1, 1), (10, 10, 2, 1), (5, 5, 2, 1)], got
    sizes, P = ss.chain((10, 10, 1), [(3, 1, 2, 1, 1), (3, 2, 2, 1, 1)], (3, 1, 1))
    assert sizes == [g[:3] for g in got] and P == 25
    assert [c["Z"].shape for c in spec["convs"]] == [(5, 9), (6, 18)] and spec["head"]["Z"].shape == (7, 18)
    from deepcgp_amd.views import FullView
    views = [FullView((e["H"], e["W"]), e["f"], e["C"], e["s"], padding=e["pad"]) for e in spec["convs"] + [spec["head"]]]
    assert [(v.padding, v.out_image_height, v.out_image_width) for v in views] == [(1, 10, 10), (1, 5, 5), (1, 5, 5)]
    assert spec["head"]["w"] is None and all(c["mean_function"] == "conv2d" for c in spec["convs"])
    # without the flag: the spec of before (pad 0 everywhere, the VALID chain 12 -> 10 -> 4)
    X12 = rng.standard_normal((30, 12, 12, 1))
    spec0 = ModelBuilder(_flags(), X12, np.zeros((30, 1))).spec()
    assert [(c["H"], c["pad"]) for c in spec0["convs"]] + [(spec0["head"]["H"], spec0["head"]["pad"])] == [(12, 0), (10, 0), (4, 0)]
    with pytest.raises(ValueError, match="--paddings"):
        build_layers_from_spec(dict(spec0, head=dict(spec0["head"], kernel="rbf", pad=1)))


def test_border_patches_are_among_the_initial_inducing_patches():
    """Inducing patches are drawn from the zero-padded images: on constant-one images every unpadded patch is all ones, a patch with a zero in
    it can only come from the border."""
    from deepcgp_amd.models import draw_patches, zero_pad
    X = np.ones((6, 6, 6, 1))
    np.random.seed(3)
    assert draw_patches(zero_pad(X, 0), 200, 3).min() == 1.0
    assert draw_patches(zero_pad(X, 1), 200, 3).min() == 0.0
    assert zero_pad(X, 0) is X and zero_pad(X, 2).shape == (6, 10, 10, 1)


def test_options_toml_records_the_flag(tmp_path):
    from deepcgp_amd import utils
    for i, (extra, want) in enumerate(((("--paddings", "1,1,0"), 'paddings = "1,1,0"'), ((), 'paddings = ""'))):
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
        from deepcgp_amd.arguments import parse_paddings
        assert parse_paddings(back, 3) == parse_paddings(_flags(*extra), 3)


@pytest.mark.parametrize("name", ["res3", "res3_white", "wide_pad"])
def test_padded_oracle_matches_the_torch_forward(name):
    """The wrapper oracle (np.pad in front of an unmodified oracle layer on the padded view) against the torch forward with F.pad: ELBO, data
    term and KL to the 1e-9 of tests/test_oracle_autograd.py; every padded layer's output has the padded view's size."""
    torch = pytest.importorskip("torch")
    spec, X, Y, zs = pr.make_stack(name)
    ref = pr.oracle_model(spec, X, Y)
    with torch.no_grad():
        out = tr.forward(spec, X, Y, zs)
    got = (ref.compute_log_likelihood(X, Y, zs=zs), ref.data_term(X, Y, zs=zs), ref.KL())
    for what, g, w in zip(("elbo", "data", "kl"), got, (out["elbo"].item(), out["data"].sum().item(), out["kl"].item())):
        print("%s %-4s oracle %.12g torch %.12g rel %.3e" % (name, what, g, w, abs(g - w) / abs(w)))
        assert np.isfinite(g) and abs(g - w) <= 1e-9 * abs(w), (name, what, g, w)
    _, Fm, _ = ref.propagate(X, S=spec["S"], zs=zs)
    assert [m.shape[-1] for m in Fm] == [o for _, o in ss.output_dims(spec)]
    # the layer-0 identity on the CPU: the VALID model of the same parameters on np.pad(X) gives layer 0's outputs
    c0 = spec["convs"][0]
    phys = pr.physical(spec)
    from oracle_build import oracle_layers
    m0, v0 = oracle_layers(phys)[0].conditional_ND(pr.pad_images(X, (c0["H"], c0["W"], c0["C"]), c0["pad"]))
    assert np.array_equal(m0, Fm[0][0])


def test_patch_kernels_pad_on_the_host():
    """The patch kernels hand the device the images the window sees: shapes and the zero border (the operator calls themselves need the device)."""
    from deepcgp_amd.kernels import RBF, ConvKernel
    from deepcgp_amd.views import FullView
    k = ConvKernel(RBF(18, 1.0, 1.0), FullView((5, 5, 2), 3, 2, 1, padding=1))
    Xp = k._padded_X(np.ones((2, 50)))
    assert k.patch_count == 25 and Xp.shape == (2, 7, 7, 2) and Xp[:, 0].max() == 0.0 and Xp[:, 1:-1, 1:-1].min() == 1.0
    k0 = ConvKernel(RBF(18, 1.0, 1.0), FullView((5, 5, 2), 3, 2, 1))
    assert k0.patch_count == 9 and k0._padded_X(np.ones((2, 50))).shape == (2, 5, 5, 2)
