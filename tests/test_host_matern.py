"""Matern-3/2 and Matern-5/2 base kernels of the conv layers, the part that needs no GPU: the closed forms of the reference
(tests/matern_ref.py), the host classes' constructor errors, the --base-kernel flag, make_spec's untouched rbf / acos specs, and the
liveness of the torch reference on the cases tests/test_gpu_matern.py runs on the device."""
import math

import numpy as np
import pytest

import matern_ref as mr
import torch_ref as tr

GPU_CASES = ("small3_M20", "small3_white_M20", "odd_M33", "mnist3_M72", "ch_M200", "ch_M384")


@pytest.mark.parametrize("cls,nu2", [(mr.Matern32, 3), (mr.Matern52, 5)])
def test_closed_forms(cls, nu2):
    """k(x, x) = variance (1 - O(1e-12)); the value at r = 1; positive definite with the 1e-3 jitter on 64 random patches; autograd of the
    torch Gram against dk/drho within 1e-12."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    v, l = 1.7, 2.3
    k = cls(25, variance=v, lengthscales=l)
    Z = rng.standard_normal((64, 25))
    K = k.K(Z)
    d = np.diag(K)
    assert np.all(d < v) and np.all(v - d < 1e-11 * v), (v - d).max()      # a = sqrt(nu2 1e-12): 1 - k / v = a^2 / 2 | a^2 / 6 + O(a^3)
    assert np.all(k.Kdiag(Z) == v)
    x = np.zeros((1, 25))
    y = x.copy()
    y[0, 3] = l                                                             # |x - y| / l = 1
    a = math.sqrt(nu2)
    want = v * (1 + a) * math.exp(-a) if nu2 == 3 else v * (1 + a + 5.0 / 3.0) * math.exp(-a)
    assert abs(k.K(x, y)[0, 0] - want) <= 1e-11 * v                         # (the 1e-12 under the root moves r by 5e-13)
    assert np.linalg.eigvalsh(K + 1e-3 * np.eye(64)).min() > 0
    np.linalg.cholesky(K + 1e-3 * np.eye(64))
    assert np.allclose(K, K.T, rtol=0, atol=0)
    # the torch Gram equals the NumPy class, and its derivative with respect to rho is the closed form
    A, B = torch.tensor(Z[:7]), torch.tensor(Z[5:16])
    Kt = mr.torch_gram(A, B, torch.tensor(v, dtype=torch.float64), torch.tensor(l, dtype=torch.float64), nu2)
    assert np.abs(Kt.numpy() - k.K(Z[:7], Z[5:16])).max() <= 1e-14 * v
    # rho >= 1e-6: autograd differentiates (1 + a) exp(-a) as exp(-a) - (1 + a) exp(-a), a difference of nearly equal terms that keeps
    # eps / a of relative precision -- 1.3e-13 at rho = 1e-6, but 6e-11 at rho = 1e-12, which is autograd's rounding, not the formula's
    rho = torch.tensor(np.concatenate([[1e-6, 1e-4, 1e-2], rng.random(20) * 9.0]), requires_grad=True)
    at = math.sqrt(nu2) * torch.sqrt(rho)
    kt = v * ((1 + at) if nu2 == 3 else (1 + at + at * at / 3)) * torch.exp(-at)
    (g,) = torch.autograd.grad(kt.sum(), rho)
    assert np.abs(g.numpy() - mr.dk_drho(rho.detach().numpy(), v, nu2)).max() <= 1e-12 * v
    assert np.all(np.isfinite(mr.dk_drho(np.array([0.0]), v, nu2)))         # finite at r = 0


def test_constructor_errors_and_descriptions():
    from deepcgp_amd.kernels import Matern32, Matern52, ConvKernel
    from deepcgp_amd.flat import kernels as flat_kernels
    from deepcgp_amd.views import FullView
    k3, k5 = Matern32(9, variance=2.0, lengthscales=3.0), Matern52(9, 2.0, 3.0)
    assert k3._describe() == [2.0, 2.0, 3.0, 0.0] and k5._describe() == [3.0, 2.0, 3.0, 0.0]
    assert isinstance(k3.lengthscales, float) and k3.variance == 2.0 and np.all(k5.Kdiag(np.zeros((4, 9))) == 2.0)
    assert flat_kernels.Matern32 is Matern32 and flat_kernels.Matern52 is Matern52
    for cls in (Matern32, Matern52):
        with pytest.raises(NotImplementedError):
            cls(4, ARD=True)
        with pytest.raises(ValueError):
            cls(4, variance=0.0)
        with pytest.raises(ValueError):
            cls(4, lengthscales=-1.0)
        with pytest.raises(ValueError):
            cls(4, lengthscales=[1.0, 2.0, 3.0, 4.0])
        with pytest.raises(NotImplementedError):          # the heads stay RBF-based
            ConvKernel(cls(9), FullView((6, 6), 3, 1, 1))


def test_base_kernel_flag():
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.kernels import Matern32, Matern52, RBF
    from deepcgp_amd.models import ModelBuilder, build_layers_from_spec
    from deepcgp_amd.layers import ConvLayer
    rng = np.random.default_rng(0)
    X = rng.standard_normal((6, 10, 10, 1))
    Z = [rng.standard_normal((4, 9)), rng.standard_normal((5, 9 * 2))]

    class B(ModelBuilder):        # inducing patches without the device's k-means
        def spec(self):
            import deepcgp_amd.models as M
            real = M.PatchInducingFeatures.from_images
            M.PatchInducingFeatures.from_images = classmethod(lambda cls, imgs, m, f: cls(Z[0] if imgs.shape[3] == 1 else Z[1]))
            try:
                return ModelBuilder.spec(self)
            finally:
                M.PatchInducingFeatures.from_images = real
    for name, cls in (("matern32", Matern32), ("matern52", Matern52)):
        fl = default_parser().parse_args(['--name', 't', '-M', '4,5', '--feature-maps', '2', '--filter-sizes', '3,3', '--strides', '1,1',
                                          '--base-kernel', name])
        spec = B(fl, X, np.zeros((6, 1))).spec()
        c = spec["convs"][0]
        assert c["base"] == name and c["variance"] == 5.0 and c["ls"] == 5.0 and spec["head"]["ls"] == 5.0

        class Stub(ConvLayer):    # (no device: skip the prior factorisation and the initial q_sqrt)
            def _build_prior_cholesky(self):
                pass
        import deepcgp_amd.models as M
        real = M.ConvLayer
        M.ConvLayer = Stub
        try:
            spec["convs"][0].update(q_mu=np.zeros((4, 2)), q_sqrt=np.tile(np.eye(4), (2, 1, 1)))
            spec["head"].update(q_mu=np.zeros((5, 10)), q_sqrt=np.tile(np.eye(5), (10, 1, 1)), white=True)
            layers = build_layers_from_spec(spec)
        finally:
            M.ConvLayer = real
        bk = layers[0].base_kernel
        assert type(bk) is cls and bk.variance == 5.0 and bk.lengthscales == 5.0
        assert type(layers[1].kern.base_kernel) is RBF
    fl.base_kernel = "matern12"
    with pytest.raises(ValueError):
        B(fl, X, np.zeros((6, 1))).spec()
    with pytest.raises(ValueError):
        build_layers_from_spec({"convs": [dict(spec["convs"][0], base="matern12")], "head": spec["head"]})


def test_make_spec_records_the_base_and_leaves_rbf_and_acos_alone():
    """The rbf and acos specs are the arrays their formulas give from the same seed, bit for bit; a Matern spec differs from the rbf one
    only in `base` and in the conv layers' q_sqrt, which comes from the Matern K_uu."""
    from deepcgp_amd import synthetic as syn
    args = ((12, 12, 1), [(3, 1, 2)], (3, 1))
    kw = dict(M=6, S=2, seed=4, conv_q_sqrt_scale=0.3, variance=2.0, ls=1.5)
    rbf, acos = syn.make_spec(*args, **kw), syn.make_spec(*args, base_kernel="acos", **kw)
    rng = np.random.default_rng(4)
    imgs = syn._blur_images(rng, 64, 12, 12, 1)
    Z = syn._cut_patches(rng, imgs, 6, 3)
    q_mu = rng.standard_normal((6, 2))
    assert np.array_equal(rbf["convs"][0]["Z"], Z) and np.array_equal(acos["convs"][0]["Z"], Z)
    assert np.array_equal(rbf["convs"][0]["q_mu"], q_mu) and np.array_equal(acos["convs"][0]["q_mu"], q_mu)
    A = Z / 1.5
    d = np.sum(A * A, 1)[:, None] + np.sum(A * A, 1)[None, :] - 2.0 * A @ A.T
    Lr = np.linalg.cholesky(2.0 * np.exp(-0.5 * d) + 1e-3 * np.eye(6))
    assert np.array_equal(rbf["convs"][0]["q_sqrt"], np.tile(Lr[None], [2, 1, 1]) * 0.3)
    den = np.sqrt(1.0 * np.sum(Z * Z, 1) + 1.0)
    theta = np.arccos(1e-15 + (1.0 - 2e-15) * (1.0 * (Z @ Z.T) + 1.0) / den[:, None] / den[None, :])
    La = np.linalg.cholesky(1.0 * (np.pi - theta) / np.pi + 1e-3 * np.eye(6))
    assert np.array_equal(acos["convs"][0]["q_sqrt"], np.tile(La[None], [2, 1, 1]) * 0.3)
    assert rbf["convs"][0]["base"] == "rbf" and acos["convs"][0]["base"] == "acos"
    for name, cls in (("matern32", mr.Matern32), ("matern52", mr.Matern52)):
        m = syn.make_spec(*args, base_kernel=name, **kw)
        assert m["convs"][0]["base"] == name
        Lm = np.linalg.cholesky(cls(9, 2.0, 1.5).K(Z) + 1e-3 * np.eye(6))
        assert np.abs(m["convs"][0]["q_sqrt"] - np.tile(Lm[None], [2, 1, 1]) * 0.3).max() <= 1e-12
        for key in ("Z", "Z0", "q_mu", "variance", "ls"):
            assert np.array_equal(m["convs"][0][key], rbf["convs"][0][key]), key
        for key, val in rbf["head"].items():
            assert np.array_equal(m["head"][key], val), key


@pytest.mark.parametrize("base", ["matern32", "matern52"])
def test_the_helper_is_the_textbook_forward_with_another_gram(base, monkeypatch):
    """tests/torch_ref.py's forward (with tests/matern_ref.py's Gram function) against a stand-in written here: tests/test_oracle_autograd.py's _torch_elbo with its conv layers'
    Gram function replaced (the head keeps the RBF).  Value and one gradient group."""
    torch = pytest.importorskip("torch")
    import test_oracle_autograd as toa
    spec, X, Y, zs = mr.matern_case("small3_M20", base)
    _stand_in(monkeypatch, toa, spec, mr.NU2[base])
    e_s, leaves = toa._torch_elbo(spec, X, Y, zs)
    (g_s,) = torch.autograd.grad(e_s, [leaves[0]["lengthscales"]])
    ref = tr.reference(spec, X, Y, zs)
    e_h, want = ref["parts"][0], ref["want"]
    assert abs(e_h - e_s.item()) <= 1e-13 * abs(e_h)
    assert abs(want[0]["lengthscales"] - g_s.item()) <= 1e-11 * abs(g_s.item())


def _stand_in(monkeypatch, toa, spec, nu2):
    """_torch_elbo asks its Gram function for K_uu, K_uf and (unwhitened) the prior's K_p of each conv layer in turn, then for the head's
    matrices: the first 3 (2) calls per conv layer get the Matern form, the rest the RBF (mnist3's second conv layer and its head both
    have 250-entry patches, so the patch length cannot tell them apart)."""
    import torch
    left = [sum(2 if c["white"] else 3 for c in spec["convs"])]
    orig = toa._rbf

    def gram(A, B, variance, l):
        if left[0] <= 0:
            return orig(A, B, variance, l)
        left[0] -= 1
        r = torch.sqrt(torch.cdist(A / l, B / l, compute_mode="donot_use_mm_for_euclid_dist") ** 2 + 1e-12)
        a = math.sqrt(nu2) * r
        return variance * ((1 + a + a * a / 3) if nu2 == 5 else (1 + a)) * torch.exp(-a)
    monkeypatch.setattr(toa, "_rbf", gram)


@pytest.mark.parametrize("base", ["matern32", "matern52"])
@pytest.mark.parametrize("case", GPU_CASES)
def test_reference_gradients_are_live(case, base, monkeypatch):
    """live_specs.assert_live on the reference alone (the stand-in above, not the helper), for every case of tests/test_gpu_matern.py."""
    pytest.importorskip("torch")
    import live_specs as ls
    import test_oracle_autograd as toa
    spec, X, Y, zs = mr.matern_case(case, base)
    _stand_in(monkeypatch, toa, spec, mr.NU2[base])
    _, want = ls.torch_reference(spec, X, Y, zs)
    rows = ls.liveness(want)
    print(case, base, "min group max %.3e  largest left-out share %.3f" % (min(r[2] for r in rows),
                                                                           max(r[4] for r in rows if r[1] in ls.CAPPED_GROUPS)))
    ls.assert_live(case, want)
