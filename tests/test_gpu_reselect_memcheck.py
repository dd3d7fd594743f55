"""GPU: dcgp_cross_gram, dcgp_inducing_transfer and ``DGP_Base.reselect_inducing`` under poisoned and guarded device allocations, the pattern of
tests/test_gpu_greedy_memcheck.py: each scenario of tests/reselect_memcheck_child.py runs twice in fresh processes, clean and with
DCGP_POISON_WS=1 DCGP_GUARD_WS=4096.  Both runs must be finite, leave every guard whole -- the transfer's scratch (the padded Gram matrices and
their factors, the products, the batch of new covariances) and the outputs it takes from the caller -- and hash the same.  A product that read
the padding of a factor nobody wrote, an assembly that left part of a padded S' unwritten in front of the factorisation, or a commit that wrote on
a failed call would read NaNs under poison, or change the untouched output buffers, and change the hash."""
import os
import subprocess
import sys
import time

import pytest

import reselect_memcheck_child as child

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"DCGP_POISON_WS": "1", "DCGP_GUARD_WS": "4096"}
SWITCHES = ("DCGP_POISON_WS", "DCGP_POISON_ONLY", "DCGP_GUARD_WS")
# As tests/test_gpu_memcheck.py sizes its own: three times the slowest child, rounded up; the seconds measured stand in the MEMCHECK line the
# test prints (measured: 0.8 s for `transfer`, 1.0 s for `model`, which builds and trains two small models; doubled for a busy host).
CHILD_TIMEOUT = 6


def _env(extra):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra)
    return env


def _child(name, extra):
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join("tests", "reselect_memcheck_child.py"), name], cwd=ROOT, env=_env(extra), capture_output=True,
                       text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (name, extra, r.returncode, r.stderr[-3000:])
    want = "MODES guard %s poison %d" % (extra.get("DCGP_GUARD_WS", "0"), int("DCGP_POISON_WS" in extra))
    assert want in r.stdout.splitlines(), (name, want, r.stdout[-300:])            # the child ran under the modes it was meant to
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1].split()
    return line[1], int(line[2]), int(line[3]), r.stderr, time.perf_counter() - t0


@pytest.mark.parametrize("name", child.SCENARIOS)
def test_reselect_is_unchanged_under_poison_and_leaves_every_guard_whole(ctx, name):
    clean = _child(name, {})
    hard = _child(name, MODES)
    print("MEMCHECK reselect %s clean %s (%.1f s) guarded %s (%.1f s) n_bad %d" % (name, clean[0][:16], clean[4], hard[0][:16], hard[4], hard[1]))
    assert clean[2] == 1, (name, "clean run not finite", clean[3][-2000:])
    assert hard[2] == 1, (name, "not finite under poison", hard[3][-2000:])
    assert clean[1] == 0, (name, "guard mode off reported violations", clean[3][-2000:])
    assert hard[1] == 0, (name, "writes past the end of a buffer", hard[3][-3000:])
    assert clean[0] == hard[0], (name, "results differ under poisoned and guarded allocations", hard[3][-2000:])
