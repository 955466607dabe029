"""Drain what-if sweep (openr_spf_whatif_drain*): the public surface, without a GPU.

The C-ABI symbols and Python bindings, topology.drain_events, and the wave-uniformity of the
kernels in spf_drain.hip (compiles only), analysed as tests/test_whatif_lfa_api.py analyses
spf_wlfa.hip.
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
SRC = os.path.join(ROOT, "openr_amd", "csrc", "spf_drain.hip")
DRAIN_CALLS = ("openr_spf_whatif_drain", "openr_spf_whatif_drain_device", "openr_spf_whatif_drain_routes",
               "openr_spf_whatif_drain_routes_device")


def test_drain_calls_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(openr_spf_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (openr_spf_\w+)", out.stdout))
    for name in DRAIN_CALLS:
        assert name in declared, name
        assert name in engine.EXPORTS, name
        assert name in exported, name
        assert hasattr(lib, name)
    for m in ("whatif_drain", "whatif_drain_device", "whatif_drain_routes", "whatif_drain_routes_device"):
        assert callable(getattr(engine.SpfEngine, m))
    fields = ["n_events", "node_ptr", "nodes", "link_ptr", "links"]
    assert [f for f, _ in engine.DrainEvents._fields_] == fields
    struct = re.search(r"typedef struct \{([^}]*)\}\s*openr_spf_drain_events_t\s*;", text).group(1)
    assert re.findall(r"(\w+);", struct) == fields
    assert lib.openr_spf_abi_version() == 1  # additive: the ABI version stays
    assert "spf_drain.hip" in lib.openr_spf_build_id().decode()  # the build id covers the new file


def test_drain_events_sorts_dedups_and_validates():
    g = T.grid(4)  # V = 16, L = 24
    assert g.num_nodes == 16 and g.num_links == 24
    nodes, links = T.drain_events(g, [[5, 1, 5, 3], [], [15]])
    assert nodes == [[1, 3, 5], [], [15]] and links is None
    nodes, links = T.drain_events(g, [[2, 2], [0]], [[23, 0, 23], []])
    assert nodes == [[2], [0]] and links == [[0, 23], []]
    with pytest.raises(ValueError):
        T.drain_events(g, [[16]])  # node >= V
    with pytest.raises(ValueError):
        T.drain_events(g, [[0]], [[24]])  # link >= L
    with pytest.raises(ValueError):
        T.drain_events(g, [[-1]])
    with pytest.raises(ValueError):
        T.drain_events(g, [[0]], [[-2]])
    with pytest.raises(ValueError):
        T.drain_events(g, [[0], [1]], [[0]])  # one link set for two events


# --- wave uniformity of the kernels ---------------------------------------------------------
@pytest.fixture(scope="module")
def analysis():
    """The kernels of spf_drain.hip (tests/uniformity_ir.py)."""
    return analyse(SRC, "drain")


def test_every_kernel_is_analysed(analysis):
    names = sorted(re.search(r"\d+(drain_[a-z]+)E", k).group(1) for k in analysis)
    assert names == ["drain_filter", "drain_repair"], names


def test_drain_repair_barriers_outside_divergent_loops(analysis):
    """drain_repair has no wave collective. Its barriers sit in the unit loop and in the round
    loops (A closure, distance rounds, D closure, Kahn rounds), whose counts every thread reads
    from LDS at a uniform address between two barriers. The loops with per-lane trip counts
    are the strided loops over lists, bitmap words and slots with their bit, row and byte
    loops inside; the compiler keeps several copies of the walks (one per callback). One of
    them, the slot-index fill before the unit loop, is at depth 1; none of the others is the
    unit loop or a round loop."""
    blocks, cycles = kernel(analysis, "drain_repair")
    assert len(cycles) == N_REPAIR_LOOPS, cycles
    no_collective_in(blocks, cycles)
    barrier_blocks = [lb for lb, b in blocks.items() if "s.barrier" in b]
    assert barrier_blocks  # the barriers exist, outside every divergent-exit loop
    in_cycles = {lb for _, labels in cycles for lb in labels}
    assert not in_cycles & set(barrier_blocks)
    assert [len(labels) for depth, labels in cycles if depth < 2] == [1], cycles  # the fill loop alone
    others = [m.group(0) for b in blocks.values() for m in COLLECTIVE.finditer(b) if "s.barrier" not in m.group(0)]
    assert not others, others


def test_drain_filter_collectives_outside_divergent_loops(analysis):
    """drain_filter: the loops over an event's nodes, a node's row and an event's links have
    per-lane trip counts; the ballot, the lane read and the shuffle of the append sit in the
    unit loop (block stride), outside them. No barrier."""
    blocks, cycles = kernel(analysis, "drain_filter")
    assert len(cycles) == 3, cycles
    no_collective_in(blocks, cycles)
    assert all(depth >= 2 for depth, _ in cycles), cycles
    assert any("ballot" in b for b in blocks.values())
    assert not any("s.barrier" in b for b in blocks.values())


N_REPAIR_LOOPS = 37
