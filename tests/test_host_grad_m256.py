"""Liveness of the M <= 256 gradient cases and of the model variants (tests/live_specs.py, CASES_M256), on the CPU: torch autograd of the
textbook forward alone.

tests/test_gpu_grad_m256.py compares the device's reverse pass on the route a training step at M <= 256 takes with this reference, group by
group and entry by entry, relative to the reference -- which says nothing where the reference is (almost) zero.  So every case keeps the
condition of tests/test_host_grad_large_m.py: |want|max >= 1e-3 in every group, the median of |want| over Z, q_mu and patch_weights at least
1e-6 of the group's maximum, and at most half of the entries of Z, q_mu, patch_weights and tril(q_sqrt) below the entry-wise floor.
``test_specs_of_the_group_wise_tests_are_not_live`` records why the cases are not the specs the gradient tests of tests/test_gpu_model.py
build."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from deepcgp_amd import synthetic as syn          # noqa: E402
import live_specs as ls                           # noqa: E402


@pytest.mark.parametrize("case", list(ls.CASES_M256))
def test_every_gradient_group_is_live(case):
    spec, X, Y, zs = ls.make_case(case)
    k = ls.CASES_M256[case]
    assert spec["head"]["M"] == k["M"] <= 256 and all(c["M"] == k["M"] for c in spec["convs"])
    assert spec["S"] == k.get("S", 2)
    e, want = ls.torch_reference(spec, X, Y, zs)
    assert np.isfinite(e)
    for row in ls.liveness(want):
        print("%s L%d %-14s max %.3e  median/max %.3e  below the entry floor %.4f" % ((case,) + row))
    ls.assert_live(case, want)
    for groups in want:        # the reference's own q_sqrt gradient: nothing above the diagonal
        assert not np.triu(groups["q_sqrt"], 1).any()


def test_the_two_syrk_cases_have_the_columns_for_it():
    """ch_M256 / ch_M200 are the cases that must reach syrk_kscale_kernel (K >= 8192 columns, M > 128) and the strip kernel (4096) by default."""
    for case in ("ch_M256", "ch_M200"):
        k = ls.CASES_M256[case]
        f, s, _ = k["convs"][0]
        P = ((k["hwc"][0] - f) // s + 1) * ((k["hwc"][1] - f) // s + 1)
        assert k["N"] * k["S"] * P >= 8192 and k["M"] > 128, (case, k["N"] * k["S"] * P)


@pytest.mark.parametrize("which", ["cfg2_mnist_CH_M256", "three_layers_M20_white"])
def test_specs_of_the_group_wise_tests_are_not_live(which):
    """Why tests/test_gpu_grad_m256.py does not take the specs of the group-wise gradient tests.
    cfg2_mnist_CH_M256 (test_full_size_cfg2_gradient_vs_torch_autograd), cut to 4 images: make_config's conv q_sqrt = 1e-5 chol(K_uu) puts the
    KL's 1 / L_ii (1e6) on the diagonal of the q_sqrt gradient, so nearly every entry of the lower triangle -- every one that carries the data
    term -- is below 1e-6 of the maximum: the LEFT_OUT_CAP condition fails.
    The whitened three-layer spec of test_gradients_match_oracle: Z, q_sqrt, variance and lengthscales of the conv layers have maxima of
    1e-11 .. 1e-6: LIVE_MAX fails.  If either starts to fail here, that spec has become live and the new module can take it directly."""
    if which == "cfg2_mnist_CH_M256":
        N = 4
        spec, X, Y = syn.make_config(which, S=2)
        X, Y = X[:N], Y[:N]
        zs = syn.make_noise(spec, N, seed=6)
    else:
        N = 3
        spec = syn.make_spec((14, 14, 1), [(3, 1, 3), (4, 2, 2)], (3, 1), 20, S=2, num_data=500, seed=9, white=True, conv_q_sqrt_scale=0.3,
                             variance=2.0, ls=1.5)
        spec["head"]["w"] = 0.5 + np.random.default_rng(9).random(spec["head"]["w"].shape)
        X, Y = syn.make_batch((14, 14, 1), N, seed=9)
        zs = syn.make_noise(spec, N, seed=9)
    _, want = ls.torch_reference(spec, X, Y, zs)
    rows = {(li, name): (top, med, out) for li, name, top, med, out in ls.liveness(want)}
    for key, row in rows.items():
        print("%s L%d %-14s max %.3e  median/max %.3e  below the entry floor %.4f" % ((which,) + key + row))
    with pytest.raises(AssertionError):
        ls.assert_live(which, want)
    if which == "cfg2_mnist_CH_M256":
        assert rows[(0, "q_sqrt")][2] > ls.LEFT_OUT_CAP
    else:
        assert min(rows[(li, name)][0] for li in (0, 1) for name in ("Z", "q_sqrt", "lengthscales")) < ls.LIVE_MAX
