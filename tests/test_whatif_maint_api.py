"""Maintenance what-if sweep (openr_spf_whatif_maint*): the public surface, without a GPU.

The C-ABI symbols and Python bindings, topology.maint_events, the corner cases the random
recipe of tests/test_gpu_whatif_maint.py holds, and the wave-uniformity of the kernels in
spf_maint.hip (compiles only), analysed as tests/test_whatif_metric_api.py analyses
spf_metric.hip.
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
SRC = os.path.join(ROOT, "openr_amd", "csrc", "spf_maint.hip")
MAINT_CALLS = ("openr_spf_whatif_maint", "openr_spf_whatif_maint_device", "openr_spf_whatif_maint_routes",
               "openr_spf_whatif_maint_routes_device")


def test_maint_calls_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(openr_spf_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (openr_spf_\w+)", out.stdout))
    for name in MAINT_CALLS:
        assert name in declared, name
        assert name in engine.EXPORTS, name
        assert name in exported, name
        assert hasattr(lib, name)
        # the argument list of the restore call of the same form, the events struct apart
        twin = getattr(lib, name.replace("maint", "restore")).argtypes
        assert len(getattr(lib, name).argtypes) == len(twin)
    for m in ("whatif_maint", "whatif_maint_device", "whatif_maint_routes", "whatif_maint_routes_device"):
        assert callable(getattr(engine.SpfEngine, m))
    fields = ["n_events", "node_ptr", "nodes", "link_ptr", "links", "edge_ptr", "edges", "metrics"]
    assert [f for f, _ in engine.MaintEvents._fields_] == fields
    assert engine.MaintEvents._fields_ == engine.RestoreEvents._fields_
    struct = re.search(r"typedef struct \{([^}]*)\}\s*openr_spf_maint_events_t\s*;", text).group(1)
    assert re.findall(r"(\w+);", struct) == fields
    assert lib.openr_spf_abi_version() == 1  # additive: the ABI version stays
    assert "spf_maint.hip" in lib.openr_spf_build_id().decode()  # the build id covers the new file


def test_maint_events_sorts_merges_and_validates():
    g = T.grid(4)  # V = 16, L = 24, E = 48, every metric 1
    nodes, links, edges, metrics = T.maint_events(g, [[7, 2, 7], [], [15]], [[5, 5, 1], [23], []],
                                                  [[7, 2, 40], [], [47]], [[3, 9, 1], [], [2**31 - 1]])
    assert nodes == [[2, 7], [], [15]] and links == [[1, 5], [23], []]
    assert edges == [[2, 7, 40], [], [47]] and metrics == [[9, 3, 1], [], [2**31 - 1]]
    # an edge listed twice keeps the larger metric, wherever it stands
    _, _, edges, metrics = T.maint_events(g, edge_sets=[[5, 1, 5, 1]], metric_sets=[[4, 8, 6, 2]])
    assert edges == [[1, 5]] and metrics == [[8, 6]]
    # the parts are those of drain_events and metric_events
    assert T.maint_events(g, [[3, 1, 3]], [[4, 0]])[:2] == T.drain_events(g, [[3, 1, 3]], [[4, 0]])
    assert T.maint_events(g, edge_sets=[[9, 4]], metric_sets=[[2, 5]])[2:] == T.metric_events(g, [[9, 4]], [[2, 5]])
    # a kind that is not given stays None
    assert T.maint_events(g, node_sets=[[3, 1]]) == ([[1, 3]], None, None, None)
    assert T.maint_events(g, link_sets=[[3, 1]]) == (None, [[1, 3]], None, None)
    assert T.maint_events(g) == (None, None, None, None)
    g9 = g.patched(list(range(48)), [9] * 48, [], [], [], [])
    for kw in ({"edge_sets": [[48]], "metric_sets": [[5]]},  # edge >= E
               {"edge_sets": [[-1]], "metric_sets": [[5]]},
               {"edge_sets": [[0]], "metric_sets": [[8]]},  # a decrease: a restore event
               {"edge_sets": [[0]], "metric_sets": [[2**31]]},  # above 2^31 - 1
               {"edge_sets": [[0, 1]], "metric_sets": [[9]]},  # an event's lists differ in length
               {"edge_sets": [[0], [1]], "metric_sets": [[9]]},  # one metric list for two events
               {"edge_sets": [[0]]},  # edges without metrics
               {"node_sets": [[16]]}, {"node_sets": [[-1]]}, {"link_sets": [[24]]},  # ids out of range
               {"node_sets": [[0]], "link_sets": [[0], [1]]},  # one node set for two events
               {"node_sets": [[0]], "edge_sets": [[0], [1]], "metric_sets": [[9], [9]]}):
        with pytest.raises(ValueError):
            T.maint_events(g9, **kw)


def test_random_recipe_holds_every_corner_case():
    """Empty events, raises on a drained node's row (the node a source or not), on a removed
    link, on a down edge and on an overloaded node's row, and already-overloaded nodes in N_i all
    occur in the random recipe of the GPU module: no hand-made event is needed."""
    import test_gpu_whatif_maint as M

    held = [M.corner_cases(*M.mixed_case(seed)) for seed in (0, 1, 2)]
    assert tuple(sum(col) for col in zip(*held)) == M.MIXED_CORNERS == (2, 23, 3, 4, 44, 17, 79), held
    for seed in (0, 1, 2):
        _, ev, _ = M.mixed_case(seed)
        assert sum(1 for n, l, e in zip(*ev[:3]) if n and l and e) == M.MIXED_UNION["all_three_kinds"][seed]


# --- wave uniformity of the kernels ---------------------------------------------------------
@pytest.fixture(scope="module")
def analysis():
    """The kernels of spf_maint.hip (tests/uniformity_ir.py)."""
    return analyse(SRC, "maint")


def test_every_kernel_is_analysed(analysis):
    names = sorted(re.search(r"\d+(maint_[a-z]+)E", k).group(1) for k in analysis)
    assert names == ["maint_filter", "maint_repair"], names


def test_maint_repair_barriers_outside_divergent_loops(analysis):
    """maint_repair has no wave collective. Its barriers sit in the unit loop and in the round
    loops (A closure, distance rounds, D closure, Kahn rounds), whose counts every thread reads
    from LDS at a uniform address between two barriers. The loops with per-lane trip counts
    are the strided loops over lists, bitmap words and slots with their bit, row and byte
    loops and the binary search of the event's slice inside; the compiler keeps several copies
    of the walks (one per callback). One of them, the slot-index fill before the unit loop, is
    at depth 1; none of the others is the unit loop or a round loop."""
    blocks, cycles = kernel(analysis, "maint_repair")
    assert len(cycles) == N_REPAIR_LOOPS, cycles
    no_collective_in(blocks, cycles)
    barrier_blocks = [lb for lb, b in blocks.items() if "s.barrier" in b]
    assert barrier_blocks  # the barriers exist, outside every divergent-exit loop
    in_cycles = {lb for _, labels in cycles for lb in labels}
    assert not in_cycles & set(barrier_blocks)
    assert [len(labels) for depth, labels in cycles if depth < 2] == [1], cycles  # the fill loop alone
    others = [m.group(0) for b in blocks.values() for m in COLLECTIVE.finditer(b) if "s.barrier" not in m.group(0)]
    assert not others, others


def test_maint_filter_collectives_outside_divergent_loops(analysis):
    """maint_filter: the loops over an event's nodes, a row, its links and its entries have
    per-lane trip counts; the ballot, the lane read and the shuffle of the append sit in the
    unit loop (block stride), outside them. No barrier."""
    blocks, cycles = kernel(analysis, "maint_filter")
    assert len(cycles) == N_FILTER_LOOPS, cycles
    no_collective_in(blocks, cycles)
    assert all(depth >= 2 for depth, _ in cycles), cycles
    assert any("ballot" in b for b in blocks.values())
    assert not any("s.barrier" in b for b in blocks.values())


N_REPAIR_LOOPS = 48
N_FILTER_LOOPS = 4
