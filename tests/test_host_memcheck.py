"""The guarded device allocator without a GPU: csrc/dev_guard.h (the registry of live allocations and the scan of a guard) through the stand-alone
program tests/dev_guard_check.cc, built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer; the cover of feature
combinations tests/memcheck_scenarios.py runs on the device; and the rule that the library takes and returns device memory in one place."""
import os
import re
import shutil
import subprocess

import compose_cases as cc
import memcheck_scenarios as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepcgp_amd", "csrc")


def test_registry_and_guard_scan_under_the_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dev_guard_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "dev_guard_check.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert re.fullmatch(r"OK \d+\n", r.stdout), r.stdout
    assert r.stderr == "", r.stderr          # the sanitizers report nothing


def test_dev_guard_header_has_no_hip_in_it():
    with open(os.path.join(CSRC, "dev_guard.h")) as fh:
        text = fh.read()
    assert not re.search(r"\bhip[A-Z_]|__device__|__global__", text)
    includes = re.findall(r"#include\s+(\S+)", text)
    assert includes and all(re.fullmatch(r"<[a-z]+>", i) for i in includes), includes      # the standard library alone


def test_compose_cover_holds_every_level_of_every_factor():
    ids = ms.compose_cover()
    assert ids == ms.compose_cover() and len(set(ids)) == len(ids) and set(ids) <= set(cc.IDS)
    for factor, levels in cc.FACTORS.items():
        seen = {cc.BY_ID[cid][factor] for cid in ids}
        assert seen == set(levels), (factor, sorted(set(levels) - seen))
    # what the cover is for: the M > 256 routes in either position, a conv layer of width 1, the padded stacks
    stacks = {cc.BY_ID[cid]["stack"] for cid in ids}
    assert {"ch_264_72", "ch_72_264", "narrow_R1"} <= stacks
    assert any(c[3] for s in stacks for c in cc.STACKS[s]["convs"])
    assert len(ids) <= 10, ids
    names = ms.names()
    assert names[:len(ids)] == ["compose:" + cid for cid in ids] and names[len(ids):] == ["ard", "mixed", "evaluate", "train_run", "operators"]


def test_gemm_selection_is_the_ragged_part_of_the_table():
    import gemm_cases as gc
    picked = ms.ragged_gemm_cases()
    assert {c["layout"] for c in picked} == set(gc.LAYOUTS)
    assert {c["expect"]["tile"] for c in picked if "tile" in c["expect"]} == set(gc.TILES)
    assert any(c["expect"].get("split") for c in picked) and any(not c["expect"].get("split", True) for c in picked)
    assert set().union(*(gc.epilogues(c) for c in picked)) == set(gc.EPILOGUES)
    for c in gc.CASES:
        tile = c["expect"].get("tile", 32)
        assert (c in picked) == bool(c["M"] % tile or c["N"] % tile), c["name"]


def test_device_memory_is_taken_and_returned_in_one_place():
    """No hipMalloc( / hipFree( under csrc/ outside dev_alloc_cap / dev_free of ctx.hip (comments aside)."""
    found = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h")):
            continue
        with open(os.path.join(CSRC, name)) as fh:
            for no, line in enumerate(fh, 1):
                code = line.split("//", 1)[0]
                if re.search(r"\bhip(Malloc|Free)\(", code):
                    found.append((name, no, code.strip()))
    assert [f[0] for f in found] == ["ctx.hip", "ctx.hip"], found
    assert "hipMalloc(p, total)" in found[0][2] and found[1][2] == "hipFree(p);", found
    with open(os.path.join(CSRC, "ctx.hip")) as fh:
        text = fh.read()
    alloc = text[text.index("static hipError_t dev_alloc_cap("):text.index("hipError_t dev_alloc(dcgp_ctx")]
    free = text[text.index("void dev_free(dcgp_ctx"):text.index("void* ws_get(")]
    assert "hipMalloc(p, total)" in alloc and "hipFree(p);" in free
    # the copied poison blocks are gone: dcgp_poison is consulted by the allocator alone
    uses = [name for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h"))
            and "dcgp_poison(" in open(os.path.join(CSRC, name)).read()]
    assert uses == ["common.h", "ctx.hip"], uses
