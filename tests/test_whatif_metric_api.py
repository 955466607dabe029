"""Metric what-if sweep (openr_spf_whatif_metric*): the public surface, without a GPU.

The C-ABI symbols and Python bindings, topology.metric_events / soft_drain_events, and the
wave-uniformity of the kernels in spf_metric.hip (compiles only), analysed as
tests/test_whatif_drain_api.py analyses spf_drain.hip.
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
SRC = os.path.join(ROOT, "openr_amd", "csrc", "spf_metric.hip")
METRIC_CALLS = ("openr_spf_whatif_metric", "openr_spf_whatif_metric_device", "openr_spf_whatif_metric_routes",
                "openr_spf_whatif_metric_routes_device")


def test_metric_calls_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(openr_spf_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (openr_spf_\w+)", out.stdout))
    for name in METRIC_CALLS:
        assert name in declared, name
        assert name in engine.EXPORTS, name
        assert name in exported, name
        assert hasattr(lib, name)
    for m in ("whatif_metric", "whatif_metric_device", "whatif_metric_routes", "whatif_metric_routes_device"):
        assert callable(getattr(engine.SpfEngine, m))
    fields = ["n_events", "edge_ptr", "edges", "metrics"]
    assert [f for f, _ in engine.MetricEvents._fields_] == fields
    struct = re.search(r"typedef struct \{([^}]*)\}\s*openr_spf_metric_events_t\s*;", text).group(1)
    assert re.findall(r"(\w+);", struct) == fields
    assert lib.openr_spf_abi_version() == 1  # additive: the ABI version stays
    assert "spf_metric.hip" in lib.openr_spf_build_id().decode()  # the build id covers the new file


def test_metric_events_sorts_merges_and_validates():
    g = T.grid(4)  # V = 16, L = 24, E = 48, every metric 1
    assert g.num_nodes == 16 and g.num_dir_edges == 48 and set(g.metric.tolist()) == {1}
    edges, metrics = T.metric_events(g, [[7, 2, 40], [], [47]], [[3, 9, 1], [], [2**31 - 1]])
    assert edges == [[2, 7, 40], [], [47]] and metrics == [[9, 3, 1], [], [2**31 - 1]]
    # an edge listed twice keeps the larger metric, wherever it stands
    edges, metrics = T.metric_events(g, [[5, 1, 5, 1]], [[4, 8, 6, 2]])
    assert edges == [[1, 5]] and metrics == [[8, 6]]
    with pytest.raises(ValueError):
        T.metric_events(g, [[48]], [[5]])  # edge >= E
    with pytest.raises(ValueError):
        T.metric_events(g, [[-1]], [[5]])
    with pytest.raises(ValueError):
        T.metric_events(g, [[0]], [[0]])  # below the current metric
    with pytest.raises(ValueError):
        T.metric_events(g, [[0]], [[2**31]])  # above 2^31 - 1
    with pytest.raises(ValueError):
        T.metric_events(g, [[0, 1]], [[5]])  # an event's lists differ in length
    with pytest.raises(ValueError):
        T.metric_events(g, [[0], [1]], [[5]])  # one metric list for two events


def test_soft_drain_events_cover_rows_and_reverse_edges():
    g = T.grid(4)
    edges, metrics = T.soft_drain_events(g, [[5], [], [0, 1]], 10)
    assert edges == [list(g.row(5)), [], list(g.row(0)) + list(g.row(1))]
    assert metrics == [[11] * len(e) for e in edges]
    both, mb = T.soft_drain_events(g, [[5], [0, 1]], 3, both_directions=True)
    owner = g.edge_owner()
    for nodes, ev, mv in zip(([5], [0, 1]), both, mb):
        assert ev == sorted(set(ev)) and mv == [4] * len(ev)
        links = {int(g.link_id[e]) for u in nodes for e in g.row(u)}
        # both directed edges of every link at the event's nodes, nothing else
        assert sorted(ev) == sorted(e for e in range(48) if int(g.link_id[e]) in links)
        assert {int(owner[e]) for e in ev} >= set(nodes)
    # nodes 0 and 1 are neighbours: the link between them is covered from both rows, once each way
    assert len(both[1]) == 2 * len({int(g.link_id[e]) for u in (0, 1) for e in g.row(u)})
    with pytest.raises(ValueError):
        T.soft_drain_events(g, [[16]], 1)
    with pytest.raises(ValueError):
        T.soft_drain_events(g, [[0]], -1)


# --- wave uniformity of the kernels ---------------------------------------------------------
@pytest.fixture(scope="module")
def analysis():
    """The kernels of spf_metric.hip (tests/uniformity_ir.py)."""
    return analyse(SRC, "metric")


def test_every_kernel_is_analysed(analysis):
    names = sorted(re.search(r"\d+(metric_[a-z]+)E", k).group(1) for k in analysis)
    assert names == ["metric_filter", "metric_repair"], names


def test_metric_repair_barriers_outside_divergent_loops(analysis):
    """metric_repair has no wave collective. Its barriers sit in the unit loop and in the round
    loops (A closure, distance rounds, D closure, Kahn rounds), whose counts every thread reads
    from LDS at a uniform address between two barriers. The loops with per-lane trip counts
    are the strided loops over lists, bitmap words and slots with their bit, row and byte
    loops and the binary search of the event's slice inside; the compiler keeps several copies
    of the walks (one per callback). One of them, the slot-index fill before the unit loop, is
    at depth 1; none of the others is the unit loop or a round loop."""
    blocks, cycles = kernel(analysis, "metric_repair")
    assert len(cycles) == N_REPAIR_LOOPS, cycles
    no_collective_in(blocks, cycles)
    barrier_blocks = [lb for lb, b in blocks.items() if "s.barrier" in b]
    assert barrier_blocks  # the barriers exist, outside every divergent-exit loop
    in_cycles = {lb for _, labels in cycles for lb in labels}
    assert not in_cycles & set(barrier_blocks)
    assert [len(labels) for depth, labels in cycles if depth < 2] == [1], cycles  # the fill loop alone
    others = [m.group(0) for b in blocks.values() for m in COLLECTIVE.finditer(b) if "s.barrier" not in m.group(0)]
    assert not others, others


def test_metric_filter_collectives_outside_divergent_loops(analysis):
    """metric_filter: the loop over an event's entries has a per-lane trip count; the ballot,
    the lane read and the shuffle of the append sit in the unit loop (block stride), outside
    it. No barrier."""
    blocks, cycles = kernel(analysis, "metric_filter")
    assert len(cycles) == N_FILTER_LOOPS, cycles
    no_collective_in(blocks, cycles)
    assert all(depth >= 2 for depth, _ in cycles), cycles
    assert any("ballot" in b for b in blocks.values())
    assert not any("s.barrier" in b for b in blocks.values())


N_REPAIR_LOOPS = 32
N_FILTER_LOOPS = 1
