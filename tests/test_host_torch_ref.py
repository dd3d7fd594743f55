"""No GPU: tests/torch_ref.py's one forward against the per-feature copies it replaced.

tests/golden/torch_ref_parent.npz (made by tests/golden/make_torch_ref_parent.py from the helper files of the commit before the copies were
deleted) holds, for one or two small cases of each family, the ELBO parts and every gradient array of that family's old ``torch_reference``.
``torch_ref.reference`` on today's case of the same name reproduces each to tests/test_host_compose.py's RULE_RTOL (1e-12: "the same
operations"), gradients relative to the group's largest entry.  On the CPU that made the fixture every value came out equal to the bit; the
tolerance is for another CPU and another BLAS."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import acos_ref                                  # noqa: E402
import conv_mean_ref                             # noqa: E402
import dilation_ref                              # noqa: E402
import matern_ref                                # noqa: E402
import mixing_ref                                # noqa: E402
import padding_ref                               # noqa: E402
import torch_ref as tr                           # noqa: E402
from test_host_compose import RULE_RTOL          # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "torch_ref_parent.npz")

CASES = {
    "padding_ref/res3": lambda: padding_ref.make_stack("res3"),
    "padding_ref/wide_pad": lambda: padding_ref.make_stack("wide_pad"),
    "conv_mean_ref/ch_res": lambda: conv_mean_ref.make_case("ch_res"),
    "conv_mean_ref/even_s2-acos": lambda: conv_mean_ref.make_case("even_s2", base="acos"),
    "mixing_ref/deep": lambda: mixing_ref.make_case("deep"),
    "mixing_ref/pad_lin": lambda: mixing_ref.make_case("pad_lin"),
    "dilation_ref/dil3_pad": lambda: dilation_ref.make_stack("dil3_pad"),
    "dilation_ref/dil2_odd": lambda: dilation_ref.make_stack("dil2_odd"),
    "matern_ref/small3_M12-matern52": lambda: matern_ref.matern_case("small3_M12", "matern52"),
    "acos_ref/small3_M12": lambda: acos_ref.acos_case("small3_M12"),
}


def test_the_fixture_holds_exactly_these_cases():
    with np.load(GOLDEN) as z:
        assert {"/".join(k.split("/")[:2]) for k in z.files} == set(CASES)


@pytest.mark.parametrize("cid", list(CASES))
def test_reference_reproduces_the_copy_it_replaced(cid):
    with np.load(GOLDEN) as z:
        gold = {k[len(cid) + 1:]: z[k] for k in z.files if k.startswith(cid + "/")}
    ref = tr.reference(*CASES[cid]())
    parts = gold.pop("parts")      # (ELBO, data term, KL); the Matern and ArcCosine copies returned the ELBO alone
    assert len(parts) in (1, 3)
    for what, g, w in zip(("elbo", "data", "kl"), ref["parts"], parts):
        print("%s %-4s %.15e parent %.15e rel %.3e" % (cid, what, g, w, abs(g - w) / abs(w)))
        assert abs(g - w) <= RULE_RTOL * abs(w), (cid, what, g, w)
    got = {"want/%d/%s" % (li, name): g for li, groups in enumerate(ref["want"]) for name, g in groups.items()}
    assert set(got) == set(gold), (cid, sorted(set(got) ^ set(gold)))
    for k, w in gold.items():
        assert got[k].shape == w.shape, (cid, k)
        err, top = np.abs(got[k] - w).max(), np.abs(w).max()
        print("%s %-24s %.3e of |parent|max %.3e" % (cid, k, err / top, top))
        assert top > 0 and err <= RULE_RTOL * top, (cid, k, err, top)
