"""Restore what-if sweep (openr_spf_whatif_restore*): the public surface, without a GPU.

The C-ABI symbols and Python bindings, topology.restore_events, the no-op kinds the random
recipe of tests/test_gpu_whatif_restore.py holds, and the wave-uniformity of the kernels in
spf_restore.hip (compiles only), analysed as tests/test_whatif_metric_api.py analyses
spf_metric.hip.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from openr_amd import engine
from openr_amd import topology as T
from uniformity_ir import COLLECTIVE, analyse, kernel, no_collective_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "openr_spf.h")
SRC = os.path.join(ROOT, "openr_amd", "csrc", "spf_restore.hip")
RESTORE_CALLS = ("openr_spf_whatif_restore", "openr_spf_whatif_restore_device", "openr_spf_whatif_restore_routes",
                 "openr_spf_whatif_restore_routes_device")


def test_restore_calls_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(openr_spf_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (openr_spf_\w+)", out.stdout))
    for name in RESTORE_CALLS:
        assert name in declared, name
        assert name in engine.EXPORTS, name
        assert name in exported, name
        assert hasattr(lib, name)
    for m in ("whatif_restore", "whatif_restore_device", "whatif_restore_routes", "whatif_restore_routes_device"):
        assert callable(getattr(engine.SpfEngine, m))
    fields = ["n_events", "node_ptr", "nodes", "link_ptr", "links", "edge_ptr", "edges", "metrics"]
    assert [f for f, _ in engine.RestoreEvents._fields_] == fields
    struct = re.search(r"typedef struct \{([^}]*)\}\s*openr_spf_restore_events_t\s*;", text).group(1)
    assert re.findall(r"(\w+);", struct) == fields
    assert lib.openr_spf_abi_version() == 1  # additive: the ABI version stays
    assert "spf_restore.hip" in lib.openr_spf_build_id().decode()  # the build id covers the new file


def test_restore_events_sorts_merges_and_validates():
    g = T.grid(4)  # V = 16, L = 24, E = 48, every metric 1
    g = g.patched(list(range(48)), [9] * 48, [], [], [], [])
    nodes, links, edges, metrics = T.restore_events(g, [[7, 2, 7], [], [15]], [[5, 5, 1], [23], []],
                                                    [[7, 2, 40], [], [47]], [[3, 9, 1], [], [9]])
    assert nodes == [[2, 7], [], [15]] and links == [[1, 5], [23], []]
    assert edges == [[2, 7, 40], [], [47]] and metrics == [[9, 3, 1], [], [9]]
    # an edge listed twice keeps the lower metric, wherever it stands
    _, _, edges, metrics = T.restore_events(g, edge_sets=[[5, 1, 5, 1]], metric_sets=[[4, 8, 6, 2]])
    assert edges == [[1, 5]] and metrics == [[2, 4]]
    # a kind that is not given stays None
    assert T.restore_events(g, node_sets=[[3, 1]]) == ([[1, 3]], None, None, None)
    assert T.restore_events(g, link_sets=[[3, 1]]) == (None, [[1, 3]], None, None)
    for kw in ({"edge_sets": [[48]], "metric_sets": [[5]]},  # edge >= E
               {"edge_sets": [[-1]], "metric_sets": [[5]]},
               {"edge_sets": [[0]], "metric_sets": [[10]]},  # a raise
               {"edge_sets": [[0]], "metric_sets": [[0]]},  # a metric of 0
               {"edge_sets": [[0, 1]], "metric_sets": [[5]]},  # an event's lists differ in length
               {"edge_sets": [[0], [1]], "metric_sets": [[5]]},  # one metric list for two events
               {"edge_sets": [[0]]},  # edges without metrics
               {"node_sets": [[16]]}, {"node_sets": [[-1]]}, {"link_sets": [[24]]},  # ids out of range
               {"node_sets": [[0]], "link_sets": [[0], [1]]}):  # one node set for two events
        with pytest.raises(ValueError):
            T.restore_events(g, **kw)


def test_random_recipe_holds_every_noop_kind():
    """Empty events, nodes that are not overloaded, links already up, zero lowers and lowers on
    an edge that stays down all occur in the random recipe of the GPU module: no hand-made
    event is needed."""
    import test_gpu_whatif_restore as R

    held = np.array([R.noop_kinds(*R.mixed_case(seed)) for seed in (0, 1, 2)])
    assert held.tolist() == [[0, 42, 92, 5, 16], [1, 50, 77, 113, 18], [0, 61, 76, 12, 14]], held
    assert (held.sum(axis=0) > 0).all()


# --- wave uniformity of the kernels ---------------------------------------------------------
@pytest.fixture(scope="module")
def analysis():
    """The kernels of spf_restore.hip (tests/uniformity_ir.py)."""
    return analyse(SRC, "restore")


def test_every_kernel_is_analysed(analysis):
    names = sorted(re.search(r"\d+(restore_[a-z]+)E", k).group(1) for k in analysis)
    assert names == ["restore_filter", "restore_repair"], names


def test_restore_repair_barriers_outside_divergent_loops(analysis):
    """restore_repair has no wave collective. Its barriers sit in the unit loop and in the round
    loops (frontier rounds, D closure, Kahn rounds), whose counts every thread reads from LDS
    at a uniform address between two barriers. The loops with per-lane trip counts are the
    strided loops over lists, bitmap words and slots with their bit, row and byte loops and
    the binary search of the event's slice inside; the compiler keeps several copies of the
    walks (one per callback). One of them, the slot-index fill before the unit loop, is at
    depth 1; none of the others is the unit loop or a round loop."""
    blocks, cycles = kernel(analysis, "restore_repair")
    assert len(cycles) == N_REPAIR_LOOPS, cycles
    no_collective_in(blocks, cycles)
    barrier_blocks = [lb for lb, b in blocks.items() if "s.barrier" in b]
    assert barrier_blocks  # the barriers exist, outside every divergent-exit loop
    in_cycles = {lb for _, labels in cycles for lb in labels}
    assert not in_cycles & set(barrier_blocks)
    assert [len(labels) for depth, labels in cycles if depth < 2] == [1], cycles  # the fill loop alone
    others = [m.group(0) for b in blocks.values() for m in COLLECTIVE.finditer(b) if "s.barrier" not in m.group(0)]
    assert not others, others


def test_restore_filter_collectives_outside_divergent_loops(analysis):
    """restore_filter: the loops over an event's entries, a row, the listed-id scans and the
    binary search have per-lane trip counts; the ballot, the lane read and the shuffle of the
    append sit in the unit loop (block stride), outside them. No barrier."""
    blocks, cycles = kernel(analysis, "restore_filter")
    assert len(cycles) == N_FILTER_LOOPS, cycles
    no_collective_in(blocks, cycles)
    assert all(depth >= 2 for depth, _ in cycles), cycles
    assert any("ballot" in b for b in blocks.values())
    assert not any("s.barrier" in b for b in blocks.values())


N_REPAIR_LOOPS = 52
N_FILTER_LOOPS = 19
