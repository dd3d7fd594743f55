"""GPU: dilated stacks under poisoned and guarded device allocations, the pattern of tests/test_gpu_memcheck.py: each scenario of
tests/dilation_memcheck_child.py runs twice in fresh processes, clean and with DCGP_POISON_WS=1 DCGP_GUARD_WS=4096 (the project's own allocator
switches, csrc/ctx.hip).  Both runs must be finite, leave every guard whole -- the split batch, the phase-layout outputs and gradients, the split
noise -- and hash the same.  Both stacks have phantom outputs (``d`` divides neither side of 9 x 7; 17 % 3 != 0): a phantom column that reached a
sum, a fill entry of a reused workspace that a call did not rewrite, or a batch-to-space pass that read one would read NaNs under poison and
change the hash."""
import os
import subprocess
import sys
import time

import pytest

import dilation_memcheck_child as child

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"DCGP_POISON_WS": "1", "DCGP_GUARD_WS": "4096"}
SWITCHES = ("DCGP_POISON_WS", "DCGP_POISON_ONLY", "DCGP_GUARD_WS")
# As tests/test_gpu_memcheck.py sizes its own: three times the slowest child, rounded up.  Seconds of the slower of the two children of each
# scenario on an MI355X (about 0.6 s of each is the interpreter, NumPy and the ctx); the seconds measured stand in the MEMCHECK line the test prints:
#   dil2_odd 0.8   dil3_pad 0.8
# Three times the slowest is 2.4 s, most of it start-up; the limit is the 6 s of tests/test_gpu_memcheck.py and tests/test_gpu_greedy_memcheck.py,
# whose children are of the same kind: one cold import on a busy machine must not read as a hang.
CHILD_TIMEOUT = 6


def _env(extra):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra)
    return env


def _child(name, extra):
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join("tests", "dilation_memcheck_child.py"), name], cwd=ROOT, env=_env(extra), capture_output=True,
                       text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (name, extra, r.returncode, r.stderr[-3000:])
    want = "MODES guard %s poison %d" % (extra.get("DCGP_GUARD_WS", "0"), int("DCGP_POISON_WS" in extra))
    assert want in r.stdout.splitlines(), (name, want, r.stdout[-300:])            # the child ran under the modes it was meant to
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1].split()
    return line[1], int(line[2]), int(line[3]), r.stderr, time.perf_counter() - t0


@pytest.mark.parametrize("name", child.SCENARIOS)
def test_dilated_stacks_are_unchanged_under_poison_and_leave_every_guard_whole(ctx, name):
    clean = _child(name, {})
    hard = _child(name, MODES)
    print("MEMCHECK dilation %s clean %s (%.1f s) guarded %s (%.1f s) n_bad %d" % (name, clean[0][:16], clean[4], hard[0][:16], hard[4], hard[1]))
    assert clean[2] == 1, (name, "clean run not finite", clean[3][-2000:])
    assert hard[2] == 1, (name, "not finite under poison", hard[3][-2000:])
    assert clean[1] == 0, (name, "guard mode off reported violations", clean[3][-2000:])
    assert hard[1] == 0, (name, "writes past the end of a buffer", hard[3][-3000:])
    assert clean[0] == hard[0], (name, "results differ under poisoned and guarded allocations", hard[3][-2000:])
