"""Route-level calls (openr_spf_routes*, openr_spf_whatif_routes*): the public surface, without a GPU.

The C-ABI symbols, the Python helpers that build group tables, and the wave-uniformity of
the kernels in spf_routes.hip (compiles only).
"""
import os
import re
import subprocess

import pytest

from openr_amd import engine
from openr_amd import topology as T
from uniformity_ir import COLLECTIVE, analyse, kernel, no_collective_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "openr_spf.h")
SRC = os.path.join(ROOT, "openr_amd", "csrc", "spf_routes.hip")
ROUTE_CALLS = ("openr_spf_routes", "openr_spf_routes_device", "openr_spf_whatif_routes",
               "openr_spf_whatif_routes_device")


def test_route_calls_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(openr_spf_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (openr_spf_\w+)", out.stdout))
    for name in ROUTE_CALLS:
        assert name in declared, name
        assert name in engine.EXPORTS, name
        assert name in exported, name
        assert hasattr(lib, name)
    for m in ("routes", "routes_device", "whatif_routes", "whatif_routes_device"):
        assert callable(getattr(engine.SpfEngine, m))
    for t in ("openr_spf_groups_t", "openr_spf_whatif_routes_t"):
        assert re.search(r"\}\s*" + t + r"\s*;", text), t
    assert lib.openr_spf_abi_version() == 1  # additive: the ABI version stays
    assert "spf_routes.hip" in lib.openr_spf_build_id().decode()  # the build id covers the new file


def test_prefix_groups_validates_sorts_and_dedupes():
    g = T.grid(3)
    assert T.prefix_groups(g, [[3, 1, 3], [], (8,), range(9)]) == [[1, 3], [], [8], list(range(9))]
    with pytest.raises(ValueError):
        T.prefix_groups(g, [[0, 1], [g.num_nodes]])
    with pytest.raises(ValueError):
        T.prefix_groups(g, [[-1]])


def test_loopback_groups():
    g = T.grid(3)
    assert T.loopback_groups(g) == [[v] for v in range(9)]
    assert T.prefix_groups(g, T.loopback_groups(g)) == T.loopback_groups(g)


# --- wave uniformity of the kernels ---------------------------------------------------------
@pytest.fixture(scope="module")
def analysis():
    """The kernels of spf_routes.hip (tests/uniformity_ir.py)."""
    return analyse(SRC, "routes")


def test_routes_reduce_collectives_outside_divergent_loops(analysis):
    """routes_reduce_large reduces across the wave (shuffles): its item loop (wave id through
    readfirstlane) and its next-hop byte loop have uniform exits, and only the three member
    loops, whose trip counts are per lane, have divergent ones."""
    blocks, cycles = kernel(analysis, "routes_reduce_large")
    # 1 the minimum over a lane's members, 2 the count of members at the minimum,
    # 3 the OR of one next-hop byte over a lane's members at the minimum
    assert len(cycles) == 3, cycles
    assert all(depth >= 2 for depth, _ in cycles), cycles  # never the item loop (depth 1)
    no_collective_in(blocks, cycles)
    assert any("ds.bpermute" in b for b in blocks.values())  # the shuffles exist: the check is not vacuous
    # the lane-per-group kernel: 1 the grid-stride item loop, 2 a group's members, 3 the OR over
    # the members at the minimum; it has no collective at all
    blocks, cycles = kernel(analysis, "routes_reduce_small")
    assert len(cycles) == 3, cycles
    assert not any(COLLECTIVE.search(b) for b in blocks.values())


@pytest.mark.parametrize("emit, n_loops", [(False, 15), (True, 17)], ids=["count", "emit"])
def test_whatif_routes_barriers_outside_divergent_loops(analysis, emit, n_loops):
    """whatif_routes_kernel has no wave collective; its three barriers per unit sit in the unit
    loop, which is block-uniform (blockIdx stride, counts from memory). Every other loop has
    a per-lane trip count."""
    blocks, cycles = kernel(analysis, "whatif_routes_kernelILb%d" % int(emit))
    # count pass (15):
    #   1-2   zeroing the LDS overlay and the LDS bitmap
    #   3-4   phase 1: the unit's entries, and the groups of an entry's node (inverse map)
    #   5-8   phase 2, candidate list: the candidates, a candidate's members (minimum), the
    #         next-hop bytes compared with the base route, the members OR-ed into one byte
    #   9-13  phase 2, bitmap scan: the bitmap words, the set bits of a word, then the same
    #         three loops as 6-8
    #   14-15 phase 3: the unit's entries, and the groups of an entry's node (clearing)
    # emit pass (17): in both phase-2 branches also the members OR-ed into each next-hop byte
    #   written out (the loop over the bytes themselves runs to nh_bytes: a uniform exit)
    assert len(cycles) == n_loops, cycles
    no_collective_in(blocks, cycles)
    barrier_blocks = [lb for lb, b in blocks.items() if "s.barrier" in b]
    assert barrier_blocks  # the barriers exist, outside every divergent-exit loop
    in_cycles = {lb for _, labels in cycles for lb in labels}
    assert not in_cycles & set(barrier_blocks)
    others = [m.group(0) for b in blocks.values() for m in COLLECTIVE.finditer(b) if "s.barrier" not in m.group(0)]
    assert not others, others
