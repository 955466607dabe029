"""Loop-free alternates (openr_spf_lfa_routes*): the public surface, without a GPU.

The C-ABI symbols and Python bindings, and the wave-uniformity of every kernel in
spf_lfa.hip (compiles only), analysed as tests/test_routes_api.py analyses spf_routes.hip.
"""
import os
import re
import subprocess

import pytest

from openr_amd import engine
from uniformity_ir import COLLECTIVE, analyse, kernel, no_collective_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "openr_spf.h")
SRC = os.path.join(ROOT, "openr_amd", "csrc", "spf_lfa.hip")
LFA_CALLS = ("openr_spf_lfa_routes", "openr_spf_lfa_routes_device")


def test_lfa_calls_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(openr_spf_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (openr_spf_\w+)", out.stdout))
    for name in LFA_CALLS:
        assert name in declared, name
        assert name in engine.EXPORTS, name
        assert name in exported, name
        assert hasattr(lib, name)
    for m in ("lfa_routes", "lfa_routes_device"):
        assert callable(getattr(engine.SpfEngine, m))
    assert re.search(r"\}\s*openr_spf_lfa_entries_t\s*;", text)
    assert [f for f, _ in engine.LfaEntries._fields_] == ["ptr", "nbr", "metric", "cap"]
    assert lib.openr_spf_abi_version() == 1  # additive: the ABI version stays
    assert "spf_lfa.hip" in lib.openr_spf_build_id().decode()  # the build id covers the new file


# --- wave uniformity of the kernels ---------------------------------------------------------
@pytest.fixture(scope="module")
def analysis():
    """The kernels of spf_lfa.hip (tests/uniformity_ir.py)."""
    return analyse(SRC, "lfa")


def test_every_kernel_is_analysed(analysis):
    names = sorted(re.search(r"\d+(lfa_[a-z_]+?)(ILb[01]E)?E", k).group(1) + (
        "<%s>" % k[k.index("ILb") + 3] if "ILb" in k else "") for k in analysis)
    assert names == ["lfa_nbr_table", "lfa_ptr_shift", "lfa_reduce_large<0>", "lfa_reduce_large<1>",
                     "lfa_reduce_small<0>", "lfa_reduce_small<1>", "lfa_rows_compact", "lfa_rows_count",
                     "lfa_rows_mark"], names


@pytest.mark.parametrize("emit, n_loops", [(False, 3), (True, 9)], ids=["count", "emit"])
def test_lfa_reduce_small_barriers_outside_divergent_loops(analysis, emit, n_loops):
    """lfa_reduce_small has no wave collective; its two barriers per slice of the neighbour
    table sit in the slice loop, which, like the tile loop around it, is workgroup-uniform
    (blockIdx stride; the trip count is the source's row length, read at a uniform address).
    The loops with per-lane trip counts are the staging loop of a slice and the member loop
    of a lane's group: the compiler keeps 2 copies of the member loop in the count pass and
    one per neighbour of a byte (8) in the emit pass, where the 8-neighbour loop is unrolled."""
    blocks, cycles = kernel(analysis, "lfa_reduce_smallILb%d" % int(emit))
    assert len(cycles) == n_loops, cycles
    assert all(depth >= 3 for depth, _ in cycles), cycles  # never the tile loop (1) or the slice loop (2)
    no_collective_in(blocks, cycles)
    barrier_blocks = [lb for lb, b in blocks.items() if "s.barrier" in b]
    assert barrier_blocks  # the barriers exist, outside every divergent-exit loop
    in_cycles = {lb for _, labels in cycles for lb in labels}
    assert not in_cycles & set(barrier_blocks)
    others = [m.group(0) for b in blocks.values() for m in COLLECTIVE.finditer(b) if "s.barrier" not in m.group(0)]
    assert not others, others


@pytest.mark.parametrize("emit", [False, True], ids=["count", "emit"])
def test_lfa_reduce_large_collectives_outside_divergent_loops(analysis, emit):
    """lfa_reduce_large reduces across the wave (shuffles) once per neighbour: its item loop
    (wave id through readfirstlane), its byte loop and the loop over a byte's 8 neighbours
    have uniform exits; only the member loop, whose trip count is per lane, has a divergent
    one, and the reduction sits after it."""
    blocks, cycles = kernel(analysis, "lfa_reduce_largeILb%d" % int(emit))
    assert len(cycles) == 1, cycles
    assert all(depth >= 4 for depth, _ in cycles), cycles
    no_collective_in(blocks, cycles)
    assert any("ds.bpermute" in b for b in blocks.values())  # the shuffles exist: the check is not vacuous
    assert not any("s.barrier" in b for b in blocks.values())


@pytest.mark.parametrize("name, n_loops", [("lfa_rows_mark", 1), ("lfa_rows_count", 1), ("lfa_rows_compact", 2),
                                           ("lfa_nbr_table", 1), ("lfa_ptr_shift", 1)])
def test_helper_kernels_have_no_collective(analysis, name, n_loops):
    """The row-list, table and pointer kernels: per-thread loops only (mark / table: a
    source's edges inside the uniform source loop; compact: the words and a word's set
    bits), no barrier and no wave collective anywhere."""
    blocks, cycles = kernel(analysis, name)
    assert len(cycles) == n_loops, cycles
    assert not any(COLLECTIVE.search(b) for b in blocks.values())
