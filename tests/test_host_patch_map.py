"""CPU: the per-patch evidence entries are declared and bound, the tests' NumPy restatement sums to the oracle's head mean, FullView.as_maps,
and the argument errors that are raised before a device is needed."""
import re

import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.kernels import RBF, ArcCosine, AdditivePatchKernel, ConvKernel, InducingPoints
from deepcgp_amd.layers import SVGP_Layer
from deepcgp_amd.views import FullView
from oracle.dgp import SVGP_Layer as OSVGP
from oracle.gpflow_ref import RBF as ORBF
from oracle.kernels import AdditivePatchKernel as OAdd, ConvKernel as OConv
from oracle.views import FullView as OView
from patch_map_ref import head_patch_mean, patch_mean, patches

NEW = ("dcgp_convkernel_patch_mean", "dcgp_model_patch_evidence")
JITTER = 1e-3


def test_new_entries_in_sigs():
    with open(dev.HEADER_PATH) as fh:
        text = fh.read()
    for name in NEW:
        assert name in dev.declared_symbols()
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, text)
        assert m, name
        assert len(dev._SIGS[name]) == len(m.group(1).split(",")), name


@pytest.mark.parametrize("additive", [False, True])
@pytest.mark.parametrize("white", [False, True])
def test_restated_maps_sum_to_oracle_head_mean(white, additive):
    hwc = (9, 8, 2)
    spec = syn.make_spec(hwc, [], (3, 2), 12, seed=4, white=white, head_q_sqrt_scale=0.5, head_outputs=5)
    h = spec["head"]
    h["w"] = 0.5 + np.random.default_rng(1).random(h["w"].size)
    view = OView((h["H"], h["W"], h["C"]), h["f"], h["C"], h["s"])
    kern = (OAdd if additive else OConv)(ORBF(view.patch_length, h["variance"], h["ls"]), view, patch_weights=h["w"])
    layer = OSVGP(kern, h["R"], h["Z"], None, white=white, q_mu=h["q_mu"], q_sqrt=h["q_sqrt"])
    X, _ = syn.make_batch(hwc, 6, seed=4)
    om, _ = layer.conditional_ND(X)
    c = head_patch_mean(h, X, JITTER)
    assert c.shape == (6, view.patch_count, 5)
    assert np.max(np.abs(c.sum(1) - om)) <= 1e-10 * np.max(np.sum(np.abs(c), 1))
    # and, with beta the identity, to the oracle's Kzx itself
    kz = patch_mean(X, (9, 8, 2, 3, 2), h["Z"], h["variance"], h["ls"], h["w"], np.eye(12)).sum(1)
    want = kern.Kzx(h["Z"], X).T
    assert np.max(np.abs(kz - want)) <= 1e-12 * np.max(np.abs(want))


def test_restated_patch_order():
    geom = (5, 4, 2, 3, 1)
    X = np.arange(2 * 5 * 4 * 2, dtype=np.float64).reshape(2, 5, 4, 2)
    pt = patches(X, geom)
    assert pt.shape == (2, 6, 18)
    assert np.array_equal(pt[1, 3], X[1, 1:4, 1:4, :].reshape(-1))   # patch (row 1, column 1), elements in (kh, kw, c) order


def test_as_maps():
    v = FullView((9, 8, 2), 3, 2, 2)
    assert (v.out_image_height, v.out_image_width, v.patch_count) == (4, 3, 12)
    a = np.arange(5 * 12 * 7, dtype=np.float64).reshape(5, 12, 7)
    m = v.as_maps(a)
    assert m.shape == (5, 4, 3, 7)
    assert np.array_equal(m[2, 3, 1], a[2, 3 * 3 + 1])
    assert v.as_maps(np.zeros((2, 5, 12, 1))).shape == (2, 5, 4, 3, 1)
    assert v.as_maps(np.zeros((12, 3))).shape == (4, 3, 3)
    for bad in (np.zeros((5, 11, 7)), np.zeros(12)):
        with pytest.raises(ValueError):
            v.as_maps(bad)


def test_argument_errors_before_the_device():
    view = FullView((7, 6, 2), 3, 2, 2)
    X = np.zeros((3, 7 * 6 * 2))
    Z = np.zeros((4, view.patch_length))
    with pytest.raises(NotImplementedError):
        ConvKernel(ArcCosine(view.patch_length, order=0), view).patch_mean(Z, X, np.zeros((4, 2)))
    with pytest.raises(NotImplementedError):
        AdditivePatchKernel(RBF(view.patch_length, 1.0, np.ones(view.patch_length), ARD=True), view).patch_mean(Z, X, np.zeros((4, 2)))
    kern = ConvKernel(RBF(view.patch_length, 1.0, 1.0), view)
    with pytest.raises(ValueError):
        kern.patch_mean(Z, X, np.zeros((5, 2)))          # beta rows != M
    with pytest.raises(ValueError):
        kern.patch_mean(Z, X, np.zeros((4, 0)))          # R < 1
    with pytest.raises(ValueError):
        kern.patch_mean(Z[:, :-1], X, np.zeros((4, 2)))  # patch length
    assert kern.patch_mean(Z, X[:0], np.zeros((4, 2))).shape == (0, view.patch_count, 2)
    # a dense RBF-ARD head has no patches
    dense = SVGP_Layer(RBF(8, 1.0, np.ones(8), ARD=True), 3, InducingPoints(np.zeros((4, 8))), white=True)
    with pytest.raises((TypeError, NotImplementedError)):
        dense.patch_contributions(np.zeros((2, 8)))
