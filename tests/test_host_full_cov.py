"""CPU: the full-covariance entry points are declared and bound, and the tests' NumPy restatements of ConvKernel.K,
AdditivePatchKernel.K and the head's full-cov conditional agree with the oracle where they overlap."""
import re

import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from full_cov_ref import head_full_cov, patch_K, rbf
from oracle.gpflow_ref import RBF as ORBF
from oracle.kernels import AdditivePatchKernel as OAdd, ConvKernel as OConv
from oracle.dgp import SVGP_Layer as OSVGP
from oracle.views import FullView

NEW = ("dcgp_convkernel_k", "dcgp_svgp_conditional_full_cov", "dcgp_reparam_full_cov")
JITTER = 1e-3


def test_new_entries_in_sigs():
    with open(dev.HEADER_PATH) as fh:
        text = fh.read()
    for name in NEW:
        assert name in dev.declared_symbols()
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, text)
        assert m, name
        assert len(dev._SIGS[name]) == len(m.group(1).split(",")), name


@pytest.mark.parametrize("geom", [(7, 6, 2, 3, 2), (11, 11, 3, 5, 1)])
def test_restated_K_diag_vs_oracle(geom):
    H, W, C, f, s = geom
    view = FullView((H, W), f, C, s)
    rng = np.random.default_rng(0)
    w = 0.5 + rng.random(view.patch_count)
    X = rng.standard_normal((5, H, W, C))
    base = ORBF(view.patch_length, 2.0, 3.0)
    conv = OConv(base, FullView((H, W, C), f, C, s), patch_weights=w)
    K = patch_K(view, X, None, 2.0, 3.0, w, False)
    assert np.allclose(np.diag(K), conv.Kdiag(X.reshape(5, -1)), rtol=1e-12, atol=0)
    assert np.allclose(K, K.T, rtol=1e-13, atol=0)
    add = OAdd(base, FullView((H, W, C), f, C, s), patch_weights=w)
    Ka = patch_K(view, X, None, 2.0, 3.0, w, True)
    assert np.allclose(np.diag(Ka), add.Kdiag(X.reshape(5, -1)), rtol=1e-12, atol=0)


@pytest.mark.parametrize("white", [False, True])
def test_restated_conditional_diag_vs_oracle(white):
    hwc = (8, 8, 2)
    spec = syn.make_spec(hwc, [], (3, 1), 12, seed=4, white=white, head_q_sqrt_scale=0.5)
    h = spec["head"]
    h["w"] = 0.5 + np.random.default_rng(1).random(h["w"].size)
    view = FullView((h["H"], h["W"], h["C"]), h["f"], h["C"], h["s"])
    kern = OConv(ORBF(view.patch_length, h["variance"], h["ls"]), view, patch_weights=h["w"])
    layer = OSVGP(kern, h["R"], h["Z"], None, white=white, q_mu=h["q_mu"], q_sqrt=h["q_sqrt"])
    X, _ = syn.make_batch(hwc, 6, seed=4)
    om, ov = layer.conditional_ND(X)
    pview = FullView((h["H"], h["W"]), h["f"], h["C"], h["s"])
    Ku = rbf(h["Z"], h["Z"], h["variance"], h["ls"]) + JITTER * np.eye(h["M"])
    Kff = patch_K(pview, X.reshape(6, *hwc), None, h["variance"], h["ls"], h["w"], False)
    m, v = head_full_cov(kern.Kzx(h["Z"], X), Ku, Kff, h["q_mu"], h["q_sqrt"], white)
    assert np.max(np.abs(m - om)) <= 1e-12 * np.max(np.abs(om))
    assert np.max(np.abs(np.diagonal(v, axis1=0, axis2=1).T - ov)) <= 1e-12 * np.max(np.abs(ov))
