"""Generates tests/golden/torch_ref_parent.npz: what the per-feature torch forwards computed before tests/torch_ref.py replaced them.

Until commit PARENT each of tests/padding_ref.py, conv_mean_ref.py, mixing_ref.py, dilation_ref.py, matern_ref.py and acos_ref.py carried its
own copy of the torch forward with a ``torch_reference`` on top.  This script reads those files FROM THAT COMMIT (``git archive``, into a
temporary directory that goes first on sys.path), runs each family's old ``torch_reference`` on the cases below and writes the ELBO parts and
every gradient array.  It never imports tests/torch_ref.py: tests/test_host_torch_ref.py holds the one forward to these numbers.  Needs the
repository's history; run from the repo root:

    python tests/golden/make_torch_ref_parent.py
"""
import io
import os
import subprocess
import sys
import tarfile
import tempfile

import numpy as np

PARENT = "cd61efd17967b63857ad463a67803be285331e28"      # "Pin the device-drawn layer noise to a host Philox reference"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (family, case id, how the old helper makes the case): tests/test_host_torch_ref.py builds the same cases from today's helpers
CASES = [
    ("padding_ref", "res3", lambda m: m.make_stack("res3")),
    ("padding_ref", "wide_pad", lambda m: m.make_stack("wide_pad")),
    ("conv_mean_ref", "ch_res", lambda m: m.make_case("ch_res")),
    ("conv_mean_ref", "even_s2-acos", lambda m: m.make_case("even_s2", base="acos")),
    ("mixing_ref", "deep", lambda m: m.make_case("deep")),
    ("mixing_ref", "pad_lin", lambda m: m.make_case("pad_lin")),
    ("dilation_ref", "dil3_pad", lambda m: m.make_stack("dil3_pad")),
    ("dilation_ref", "dil2_odd", lambda m: m.make_stack("dil2_odd")),
    ("matern_ref", "small3_M12-matern52", lambda m: m.matern_case("small3_M12", "matern52")),
    ("acos_ref", "small3_M12", lambda m: m.acos_case("small3_M12")),
]


def old_reference(module, case):
    """((ELBO[, data term, KL]), want) from the four return shapes the old copies had."""
    r = module.torch_reference(*case)
    if isinstance(r, dict):
        return r["parts"], r["want"]
    parts, want = r
    return (parts if isinstance(parts, tuple) else (parts,)), want


def main():
    import importlib
    tar = subprocess.run(["git", "archive", PARENT, "tests"], cwd=ROOT, check=True, capture_output=True).stdout
    with tempfile.TemporaryDirectory() as tmp:
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        sys.path[:0] = [os.path.join(tmp, "tests"), ROOT]
        out = {}
        for family, cid, make in CASES:
            module = importlib.import_module(family)
            assert module.__file__.startswith(tmp), module.__file__
            parts, want = old_reference(module, make(module))
            out["%s/%s/parts" % (family, cid)] = np.array(parts, np.float64)
            for li, groups in enumerate(want):
                for name, g in groups.items():
                    out["%s/%s/want/%d/%s" % (family, cid, li, name)] = np.asarray(g, np.float64)
        assert "torch_ref" not in sys.modules
    path = os.path.join(ROOT, "tests", "golden", "torch_ref_parent.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
