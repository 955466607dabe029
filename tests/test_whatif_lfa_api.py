"""Post-failure loop-free alternates (openr_spf_whatif_lfa*): the public surface, without a GPU.

The C-ABI symbols and Python bindings, and the wave-uniformity of every kernel in
spf_wlfa.hip (compiles only), analysed as tests/test_lfa_api.py analyses spf_lfa.hip.
"""
import os
import re
import subprocess

import pytest

from openr_amd import engine
from uniformity_ir import COLLECTIVE, analyse, kernel, no_collective_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "openr_spf.h")
SRC = os.path.join(ROOT, "openr_amd", "csrc", "spf_wlfa.hip")
WLFA_CALLS = ("openr_spf_whatif_lfa", "openr_spf_whatif_lfa_device")


def test_whatif_lfa_calls_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(openr_spf_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (openr_spf_\w+)", out.stdout))
    for name in WLFA_CALLS:
        assert name in declared, name
        assert name in engine.EXPORTS, name
        assert name in exported, name
        assert hasattr(lib, name)
    for m in ("whatif_lfa", "whatif_lfa_device"):
        assert callable(getattr(engine.SpfEngine, m))
    assert re.search(r"\}\s*openr_spf_whatif_lfa_t\s*;", text)
    assert [f for f, _ in engine.WhatifLfa._fields_] == ["ptr", "group", "metric", "nh", "alt", "cap", "nh_bytes"]
    struct = re.search(r"typedef struct \{([^}]*)\}\s*openr_spf_whatif_lfa_t\s*;", text).group(1)
    assert re.findall(r"(\w+);", struct) == ["ptr", "group", "metric", "nh", "alt", "cap", "nh_bytes"]
    assert lib.openr_spf_abi_version() == 1  # additive: the ABI version stays
    assert "spf_wlfa.hip" in lib.openr_spf_build_id().decode()  # the build id covers the new file


# --- wave uniformity of the kernels ---------------------------------------------------------
@pytest.fixture(scope="module")
def analysis():
    """The kernels of spf_wlfa.hip (tests/uniformity_ir.py)."""
    return analyse(SRC, "wlfa")


def test_every_kernel_is_analysed(analysis):
    names = sorted(re.search(r"\d+(wlfa_[a-z_]+?)(ILb[01]E)?E", k).group(1) + (
        "<%s>" % k[k.index("ILb") + 3] if "ILb" in k else "") for k in analysis)
    assert names == ["wlfa_base", "wlfa_kernel<0>", "wlfa_kernel<1>", "wlfa_mark"], names


@pytest.mark.parametrize("emit, n_loops", [(False, 23), (True, 23)], ids=["count", "emit"])
def test_wlfa_kernel_barriers_outside_divergent_loops(analysis, emit, n_loops):
    """wlfa_kernel has no wave collective. Its barriers sit in the work-list loop (block
    stride; the count is read at a uniform address), the candidate-chunk loop (the candidate
    count is read from LDS at a uniform address) and the slice loop (the source's row length),
    all workgroup-uniform. The loops with per-lane trip counts are the staging loops (the
    hash and bitmap reset, the delta entries and their inverse-map walk, a slice's slots and
    edges), the set scans, the hash probes, the delta scans and the member loops of a lane's
    group; the compiler keeps several copies of the probe and member loops."""
    blocks, cycles = kernel(analysis, "wlfa_kernelILb%d" % int(emit))
    assert len(cycles) == n_loops, cycles
    no_collective_in(blocks, cycles)
    barrier_blocks = [lb for lb, b in blocks.items() if "s.barrier" in b]
    assert barrier_blocks  # the barriers exist, outside every divergent-exit loop
    in_cycles = {lb for _, labels in cycles for lb in labels}
    assert not in_cycles & set(barrier_blocks)
    assert all(depth >= 2 for depth, _ in cycles), cycles  # never the work-list loop (1)
    others = [m.group(0) for b in blocks.values() for m in COLLECTIVE.finditer(b) if "s.barrier" not in m.group(0)]
    assert not others, others


def test_wlfa_base_barriers_in_the_uniform_source_loop(analysis):
    """wlfa_base: the group loop of a thread is the one divergent-exit loop; the three barriers
    of a source sit in the source loop (block stride)."""
    blocks, cycles = kernel(analysis, "wlfa_base")
    assert len(cycles) == 1, cycles
    no_collective_in(blocks, cycles)
    assert any("s.barrier" in b for b in blocks.values())
    assert all(depth >= 2 for depth, _ in cycles), cycles


def test_wlfa_mark_has_no_collective(analysis):
    """wlfa_mark: per-thread loops only (the units, a source's edges, a set's links), no
    barrier and no wave collective anywhere."""
    blocks, cycles = kernel(analysis, "wlfa_mark")
    assert len(cycles) == 3, cycles
    assert not any(COLLECTIVE.search(b) for b in blocks.values())
