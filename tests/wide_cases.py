"""Scaled copies of the suite's graphs and events, for the distance tiers of the what-if and
event sweeps (tests/test_gpu_dist_tiers.py).

Multiplying every metric of a graph (down edges included) and of an event by one integer
K >= 1 keeps every comparison between two path costs, so every tie, next-hop set and changed
set stays and every finite distance is multiplied by K. The library picks its distance width
from V * w_max alone (w_max: the largest usable metric), so K moves a recipe between the
tiers without changing what its answer looks like:

    what-if repairs   u16 when V * w_max < 0xFFFF, else u32, else u64
    fringe / rounds   u64 when V * w_max >= 0xFFFFFFFF, else u32
    LDS-graph variant only when w_max <= 65535

The factors are derived here on the CPU; each test re-asserts the inequalities it relies on
before it touches the engine.
"""
import dataclasses

import numpy as np

METRIC_MAX = 2**31 - 1  # the API's largest metric
U16_LIMIT = 0xFFFF  # V * w_max below it: u16 what-if rows
U32_LIMIT = 0xFFFFFFFF  # V * w_max below it: u32 rows everywhere
LDS_GRAPH_W_MAX = 65535  # the LDS-graph record holds metrics up to it

# on the 120-node graphs with metrics <= 64
K_LDS = 211  # w_max = 13 504 <= 65 535 (LDS graph eligible), V * w_max = 1 620 480: u32
K_MID = 1031  # w_max = 65 984 > 65 535 (not eligible), V * w_max = 7 918 080: u32
# on long_line_graph(5): V = 220, w_max = 297, the farthest node from source 0 at 46 973
K_TOP = 65732  # V * w_max = 4 294 928 880 < 0xFFFFFFFF: u32, distances with bit 31 set
LINE_FARTHEST = 46973


def k_wide(m_max):
    """The largest odd K with K * m_max <= 2^31 - 1: no low bit of a scaled metric is
    systematically zero and the top metric sits at the API's limit."""
    k = METRIC_MAX // int(m_max)
    return k if k & 1 else k - 1


assert k_wide(64) == 33554431 and k_wide(104) == 20648881
assert 120 * 64 * K_LDS >= U16_LIMIT and 64 * K_LDS <= LDS_GRAPH_W_MAX
assert 120 * 64 * K_MID < U32_LIMIT and 64 * K_MID > LDS_GRAPH_W_MAX
assert 220 * 297 * K_TOP == 4294928880 < U32_LIMIT <= 220 * 297 * (K_TOP + 1) == 4294994220
assert 2**31 < LINE_FARTHEST * K_TOP == 3087629236 < 2**32


def scaled(g, K):
    """A copy of a CsrGraph with every metric multiplied by K, down edges included."""
    K = int(K)
    assert K >= 1 and int(g.metric.max(initial=0)) * K <= METRIC_MAX
    m = g.metric * np.uint64(K)
    return dataclasses.replace(g, metric=m)


def scale_metric_sets(metric_sets, K):
    """The metric lists of metric, restore and maint events (one list per event, or None)."""
    if metric_sets is None:
        return None
    return [[int(m) * int(K) for m in ms] for ms in metric_sets]


def scale_events(ev, K):
    """(node_sets, link_sets, edge_sets, metric_sets) with the metric lists multiplied by K;
    also takes the Events dataclasses of the restore and event-LFA modules (a `metrics` field)."""
    if dataclasses.is_dataclass(ev):
        return dataclasses.replace(ev, metrics=tuple(tuple(int(m) * int(K) for m in ms) for ms in ev.metrics))
    nodes, links, edges, metrics = ev
    return nodes, links, edges, scale_metric_sets(metrics, K)


def m_max_of(g, *metric_sets):
    """The largest metric a graph or the given event metric lists mention."""
    top = int(g.metric.max(initial=1))
    for sets in metric_sets:
        for ms in sets or ():
            for m in ms:
                top = max(top, int(m))
    return top


def w_max_of(g):
    """The largest usable metric: over the up edges, as the library counts it."""
    up = g.edge_up != 0
    return int(g.metric[up].max()) if up.any() else 1


def tier_of(g, unit_cost=False):
    """("u16" | "u32" | "u64", LDS-graph eligible) of a what-if launch on g."""
    w = 1 if unit_cost else w_max_of(g)
    span = g.num_nodes * w
    return ("u16" if span < U16_LIMIT else "u32" if span < U32_LIMIT else "u64"), w_max_of(g) <= LDS_GRAPH_W_MAX
