"""GPU: every feature family under poisoned and guarded device allocations (csrc/ctx.hip: dev_alloc / dev_free; csrc/dev_guard.h).

Each scenario of tests/memcheck_scenarios.py runs twice, in fresh processes one after the other: in a clean environment, then with
DCGP_POISON_WS=1 (every fresh device allocation of the library filled with NaNs) and DCGP_GUARD_WS=4096 (4096 bytes of 0xFF behind the requested
size of every allocation, checked when it is freed and by ``Context.check_guards``).  A kernel that reads memory nobody wrote -- a padded row, the
tail of a tile, a C it was told to overwrite -- changes the hash of the results or makes them non-finite; a kernel that writes past the end of a
buffer, the outputs the operator entries take from the caller included, breaks a guard, and the report names the buffer and the offset.  The bar
is equality of the two hashes: these paths are deterministic (the bitwise-reproducibility tests of the suite), so no tolerance appears and no
call's result is left out of the hash.

The first run of the file on an MI355X found nothing: every scenario came out bit-identical and with every guard whole (the seconds its children
took stand beside CHILD_TIMEOUT)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import memcheck_scenarios as ms

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"DCGP_POISON_WS": "1", "DCGP_GUARD_WS": "4096"}
SWITCHES = ("DCGP_POISON_WS", "DCGP_POISON_ONLY", "DCGP_GUARD_WS")
# Seconds of the slower of the two children of each scenario on an MI355X, the largest of three runs of this file (about 0.6 s of each is the
# interpreter, NumPy and the ctx):
#   compose:narrow_R1-gaussian1-matern52-filter-all 1.0    compose:wide_R-gaussian3-rbf-none-alternate 0.8
#   compose:ch_72_264-poisson1-acos-conv2d-none 1.0        compose:small3_20_40_24-bernoulli1-matern32-filter-all 1.0
#   compose:ch_264_72-softmax3-rbf-conv2d-all 1.0          compose:even_s2-multiclass3-rbf-filter-none 0.9
#   compose:valid2-studentt3-matern52-conv2d-alternate 0.8  compose:ch_res-softmax3-acos-filter-alternate 0.9
#   ard 0.9   mixed 0.8   evaluate 1.1   train_run 1.0   operators 1.7 (0.7 of it the 242 GEMM cases' host data; ~2.0 since the riding chain's cases, ~2.2 with the wide heads of the per-output likelihoods)
CHILD_TIMEOUT = 6       # seconds: three times the slowest (1.7 s), rounded up
# Parent commit 99bdb54, cfg2_mnist_CH_M256 after one ELBO: what dcgp_workspace_query gives with both switches unset
PARENT_WORKSPACE_BYTES, PARENT_WORKSPACE_COUNT = 14074368, 12


def _env(extra):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra)
    return env


def _child(name, extra):
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join("tests", "memcheck_scenarios.py"), name], cwd=ROOT, env=_env(extra), capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (name, extra, r.returncode, r.stderr[-3000:])
    want = "MODES guard %s poison %d" % (extra.get("DCGP_GUARD_WS", "0"), int("DCGP_POISON_WS" in extra))
    assert want in r.stdout.splitlines(), (name, want, r.stdout[-300:])            # the child ran under the modes it was meant to
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1].split()
    return line[1], int(line[2]), int(line[3]), r.stderr, time.perf_counter() - t0


@pytest.mark.parametrize("name", ms.names())
def test_scenario_is_unchanged_under_poison_and_leaves_every_guard_whole(ctx, name):
    clean = _child(name, {})
    hard = _child(name, MODES)
    print("MEMCHECK %s clean %s (%.1f s) guarded %s (%.1f s) n_bad %d" % (name, clean[0][:16], clean[4], hard[0][:16], hard[4], hard[1]))
    assert clean[2] == 1, (name, "clean run not finite", clean[3][-2000:])
    assert hard[2] == 1, (name, "not finite under poison", hard[3][-2000:])
    assert clean[1] == 0, (name, "guard mode off reported violations", clean[3][-2000:])
    assert hard[1] == 0, (name, "writes past the end of a buffer", hard[3][-3000:])
    assert clean[0] == hard[0], (name, "results differ under poisoned and guarded allocations", hard[3][-2000:])


GUARD_CHECKER = r'''
import sys
import numpy as np
sys.path.insert(0, ".")
from deepcgp_amd import device as dev
ctx = dev.get_context()
assert ctx.guard_bytes() == 4096
buf = ctx.empty((100,), np.uint8)
assert buf.nbytes == 100
assert ctx.check_guards() == (0, "")
ctx.touch_guard(buf, 0)
n, report = ctx.check_guards()
assert n == 1 and report == "dcgp_malloc (100 B) +0", (n, report)
assert ctx.check_guards() == (0, "")                  # reported once
ctx.touch_guard(buf, 155)                             # the last byte of what a round-up of 100 to 256 would have left as slack
n, report = ctx.check_guards()
assert n == 1 and report == "dcgp_malloc (100 B) +155", (n, report)
assert ctx.check_guards() == (0, "")
assert np.array_equal(buf.set(np.arange(100)).numpy(), np.arange(100))      # the buffer itself is untouched by all this
assert ctx.check_guards() == (0, "")
ctx.touch_guard(buf, 4095)
buf.free()                                            # the free's own check finds it and the ctx remembers
n, report = ctx.check_guards()
assert n == 1 and report == "dcgp_malloc (100 B) +4095 at free", (n, report)
assert ctx.check_guards() == (0, "")
other = ctx.empty((100,), np.uint8)
for bad in (4096, -1):
    try:
        ctx.touch_guard(other, bad)
    except dev.DcgpError as e:
        assert e.code == dev.ERR_ARG, e
    else:
        raise AssertionError("offset %d was not refused" % bad)
rc = dev.lib().dcgp_debug_touch_guard(ctx.handle, other.ptr + 8, 0)        # not the base of a registered allocation
assert rc == dev.ERR_ARG, rc
assert ctx.check_guards() == (0, "")
print("CHECKER OK")
'''


def test_guard_checker_sees_a_touched_guard(ctx):
    r = subprocess.run([sys.executable, "-c", GUARD_CHECKER], cwd=ROOT, env=_env({"DCGP_GUARD_WS": "4096"}), capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    assert r.returncode == 0 and "CHECKER OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_modes_off_change_nothing(ctx, monkeypatch):
    """Both switches unset: no guard, no registry, and the workspaces of the flagship model are the parent commit's to the byte."""
    if any(k in os.environ for k in SWITCHES):
        pytest.fail("the suite itself runs with %s set: this test is about the switches being off" % [k for k in SWITCHES if k in os.environ])
    from deepcgp_amd import device as dev
    from deepcgp_amd import synthetic as syn
    from deepcgp_amd.models import build_from_spec
    assert ctx.guard_bytes() == 0
    assert ctx.check_guards() == (0, "")
    probe = ctx.empty((100,), np.uint8)
    with pytest.raises(dev.DcgpError) as e:
        ctx.touch_guard(probe, 0)
    assert e.value.code == dev.ERR_ARG
    # a ctx of its own, so that what other tests left in the shared one does not count: the model takes the process-wide default ctx
    fresh = dev.Context(ctx.device)
    monkeypatch.setattr(dev, "_default_ctx", fresh)
    try:
        assert fresh.workspace_bytes() == (0, 0) and fresh.guard_bytes() == 0
        spec, X, Y = syn.make_config("cfg2_mnist_CH_M256")
        model = build_from_spec(spec, X, Y)
        elbo = model.compute_log_likelihood(X, Y, seed=5)
        got = fresh.workspace_bytes()
        model.close()
    finally:
        monkeypatch.undo()
        fresh.close()
    print("MEMCHECK workspaces %r, parent commit %r" % (got, (PARENT_WORKSPACE_BYTES, PARENT_WORKSPACE_COUNT)))
    assert np.isfinite(elbo)
    assert got == (PARENT_WORKSPACE_BYTES, PARENT_WORKSPACE_COUNT)
