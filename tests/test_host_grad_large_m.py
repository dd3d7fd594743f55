"""Liveness of the large-M gradient cases (tests/live_specs.py), on the CPU: torch autograd of the textbook forward alone.

tests/test_gpu_grad_large_m.py compares the device's reverse pass with this reference group by group and entry by entry, relative to the
reference -- which says nothing where the reference is (almost) zero.  So every case must keep every parameter group of every layer live:
|want|max >= 1e-3, the median of |want| over Z, q_mu and patch_weights at least 1e-6 of the group's maximum, and at most half of the entries of
Z, q_mu, patch_weights and tril(q_sqrt) below the entry-wise floor.  A change of deepcgp_amd/synthetic.py (or of live_specs.py) that makes a
case degenerate fails here, without a GPU.  ``test_make_config_three_layer_specs_are_degenerate`` records why the cases are not the
BASELINE specs themselves."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from deepcgp_amd import synthetic as syn          # noqa: E402
import live_specs as ls                           # noqa: E402


@pytest.mark.parametrize("case", list(ls.CASES))
def test_every_gradient_group_is_live(case):
    spec, X, Y, zs = ls.make_case(case)
    k = ls.CASES[case]
    assert spec["head"]["M"] == k["M"] > 256 and all(c["M"] == k["M"] for c in spec["convs"])
    e, want = ls.torch_reference(spec, X, Y, zs)
    assert np.isfinite(e)
    for row in ls.liveness(want):
        print("%s L%d %-14s max %.3e  median/max %.3e  below the entry floor %.4f" % ((case,) + row))
    ls.assert_live(case, want)
    for groups in want:        # the reference's own q_sqrt gradient: nothing above the diagonal
        assert not np.triu(groups["q_sqrt"], 1).any()


@pytest.mark.parametrize("name,N", [("cfg3_mnist_3layer_M256", 4), ("cfg4_cifar_3layer_M384", 2)])
def test_make_config_three_layer_specs_are_degenerate(name, N):
    """The three-layer BASELINE specs as make_config builds them fail the liveness condition (conv dZ of 1e-30: K_uf of the second layer
    underflows) -- the reason the gradient tests at M > 256 build their specs through live_spec.  If this starts to fail, the BASELINE
    specs have become live and the large-M module can take them directly."""
    spec, X, Y = syn.make_config(name, S=2)
    X, Y = X[:N], Y[:N]
    _, want = ls.torch_reference(spec, X, Y, syn.make_noise(spec, N, seed=6))
    with pytest.raises(AssertionError):
        ls.assert_live(name, want)
    assert np.abs(want[0]["Z"]).max() < 1e-20 and np.abs(want[1]["Z"]).max() < 1e-20
