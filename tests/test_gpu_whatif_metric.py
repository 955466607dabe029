"""Metric what-if sweep on the GPU (openr_spf_whatif_metric*) vs the CPU oracle.

A metric event raises the metrics of a list of directed edges; unit (i, j) is the oracle's
runSpf(source j, true) on the graph patched with the event's metrics, diffed against the
no-event run. The module runs on both parametrisations of tests/test_gpu_whatif_drain.py, so
the base rows the repair reads come from every kernel family (code / lvl BFS, fringe, rounds
with its in-degree rows). The oracle-side tables were computed on the CPU with the oracle
alone and are asserted before the engine is compared, so a vacuous recipe cannot pass.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from openr_amd import topology as T
from openr_amd.engine import E2BIG, EINVAL, ENOTSUP, USE_LINK_METRIC, MetricEvents, SpfEngine, SpfError, _p
import test_gpu_whatif_drain as drain_tests
from oracle import Oracle
from test_gpu_routes_resolve import reduce_routes, tables
from test_gpu_whatif_sets import check_delta, small_graph

pytestmark = pytest.mark.gpu

U64_MAX = np.uint64(2**64 - 1)
SOURCES = list(range(0, 120, 4))


@pytest.fixture(scope="module", autouse=True, params=[("code", "fringe"), ("lvl", "rounds")],
                ids=["code-fringe", "lvl-rounds"])
def bfs_family(request):
    keys = ("OPENR_SPF_BFS_FAMILY", "OPENR_SPF_GENERAL")
    old = {k: os.environ.get(k) for k in keys}
    for k, v in zip(keys, request.param):
        os.environ[k] = v
    yield request.param
    for k in keys:
        if old[k] is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = old[k]


@pytest.fixture(scope="module")
def eng():
    e = SpfEngine()
    yield e
    e.close()


# --- oracle side: computed once per (graph, events, sources), shared by both
# --- parametrisations of the module and never modified
_EXPECT = {}
_ROWS = {}


@dataclasses.dataclass(frozen=True)
class Expect:
    changed: np.ndarray  # [n_events, n_sources]
    ptr: np.ndarray  # [units + 1] u64
    node: np.ndarray  # every unit's changed nodes ascending, concatenated
    dist: np.ndarray  # their distance in the event run
    nh: np.ndarray  # [entries, oracle nh_bytes]
    same_dist: np.ndarray  # per entry: the node's distance is the base distance (next hops changed)
    base_dist: np.ndarray  # [n_sources, V] no-event distances


def oracle_rows(key, g, edge_sets, metric_sets, sources):
    """(base dist [S, V], base nh, event dist [n_events * S, V], event nh) of every unit."""
    if key not in _ROWS:
        o = Oracle(g)
        base = [o.run_spf(int(s), True) for s in sources]
        runs = []
        for edges, metrics in zip(edge_sets, metric_sets):
            if not len(edges):
                runs += base
                continue
            oe = Oracle(g.patched([int(e) for e in edges], [int(m) for m in metrics], [], [], [], []))
            runs += [oe.run_spf(int(s), True) for s in sources]
        rows = (np.stack([r.dist for r in base]), np.stack([r.nh for r in base]),
                np.stack([r.dist for r in runs]), np.stack([r.nh for r in runs]))
        for a in rows:
            a.setflags(write=False)
        _ROWS[key] = rows
    return _ROWS[key]


def oracle_metric(key, g, edge_sets, metric_sets, sources):
    """Expected changed counts and delta rows of every unit (event i, source j)."""
    if key in _EXPECT:
        return _EXPECT[key]
    bd, bh, fd, fh = oracle_rows(key, g, edge_sets, metric_sets, sources)
    n, S = len(edge_sets), len(sources)
    bdu, bhu = np.tile(bd, (n, 1)), np.tile(bh, (n, 1, 1))
    # a raise shrinks no distance and disconnects nothing
    assert (fd >= bdu).all()
    assert ((fd == U64_MAX) == (bdu == U64_MAX)).all()
    ch = (fd != bdu) | np.any(fh != bhu, axis=2)  # [units, V]
    counts = ch.sum(axis=1).astype(np.uint32)
    ptr = np.zeros(ch.shape[0] + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(counts, dtype=np.uint64)
    uu, vv = np.nonzero(ch)  # row-major: units ascending, nodes ascending inside a unit
    e = Expect(counts.reshape(n, S), ptr, vv.astype(np.uint32), fd[uu, vv], fh[uu, vv], fd[uu, vv] == bdu[uu, vv], bd)
    for a in dataclasses.astuple(e):
        a.setflags(write=False)
    _EXPECT[key] = e
    return e


def facts_of(exp):
    return {
        "unchanged": int((exp.changed == 0).sum()),
        "over64": int((exp.changed > 64).sum()),
        "nh_only": int(exp.same_dist.sum()),
        "total": int(exp.ptr[-1]),
        "max": int(exp.changed.max()),
    }


# --- 1. advertised-adjacency soft drains -----------------------------------------------------
ROW_FACTS = {  # oracle side, seeds 0 / 1 / 2
    "unchanged": (1798, 1893, 1876),
    "over64": (58, 48, 58),
    "nh_only": (276, 7119, 2584),
    "total": (15635, 14584, 15143),
    "max": (119, 118, 119),
}


def row_case(seed, increment=5, both=False):
    g = small_graph(seed)
    assert g.num_nodes == 120 and g.num_links == 330 and g.num_dir_edges == 660
    edge_sets, metric_sets = T.soft_drain_events(g, [[v] for v in range(120)], increment, both_directions=both)
    return g, edge_sets, metric_sets, SOURCES


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_adjacency_soft_drains_match_oracle(eng, bfs_family, seed):
    g, edge_sets, metric_sets, sources = row_case(seed)
    for v in range(120):  # event v is the CSR row of v, +5
        assert edge_sets[v] == list(g.row(v))
        assert metric_sets[v] == [int(g.metric[e]) + 5 for e in g.row(v)]
    exp = oracle_metric(("row", seed), g, edge_sets, metric_sets, sources)
    assert exp.changed.size == 3600
    assert facts_of(exp) == {k: v[seed] for k, v in ROW_FACTS.items()}, facts_of(exp)
    eng.set_graph(g)
    changed, solved = eng.whatif_metric(edge_sets, metric_sets, sources, want_delta=False)
    ks = eng.last_kernels()
    assert "metric_filter" in ks and "metric_repair" in ks, ks
    np.testing.assert_array_equal(changed, exp.changed)
    assert len(sources) <= solved < changed.size + len(sources)
    assert solved >= int((exp.changed != 0).sum()) + len(sources)
    c2, ptr, node, dist, nh, solved2 = eng.whatif_metric(edge_sets, metric_sets, sources)
    assert solved2 == solved
    check_delta(exp, c2, ptr, node, dist, nh)


# --- 2. both directions ------------------------------------------------------------------------
BOTH_FACTS = {"unchanged": (0, 30, 0), "over64": (60, 49, 58), "total": (19205, 18124, 18713)}


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_both_directions_match_oracle(eng, bfs_family, seed):
    g, edge_sets, metric_sets, sources = row_case(seed, 1, True)
    exp = oracle_metric(("both", seed, 1), g, edge_sets, metric_sets, sources)
    assert exp.changed.size == 3600
    f = facts_of(exp)
    assert {k: f[k] for k in BOTH_FACTS} == {k: v[seed] for k, v in BOTH_FACTS.items()}, f
    eng.set_graph(g)
    got = eng.whatif_metric(edge_sets, metric_sets, sources)
    check_delta(exp, *got[:5])
    if seed:
        return
    # the set of changed nodes does not depend on the size of a uniform raise; the distances do
    _, edge_k, metric_k, _ = row_case(0, 1000, True)
    assert edge_k == edge_sets
    exp_k = oracle_metric(("both", 0, 1000), g, edge_k, metric_k, sources)
    np.testing.assert_array_equal(exp_k.changed, exp.changed)
    np.testing.assert_array_equal(exp_k.node, exp.node)
    assert (exp_k.dist != exp.dist).any()
    got_k = eng.whatif_metric(edge_k, metric_k, sources)
    check_delta(exp_k, *got_k[:5])
    np.testing.assert_array_equal(got_k[0], got[0])
    assert (got_k[3] != got[3]).any()


# --- 3. random edge raises -------------------------------------------------------------------------
RANDOM_FACTS = {
    "unchanged": (974, 915, 1024),
    "over64": (10, 3, 11),
    "nh_only": (110, 2927, 1158),
    "total": (5320, 4646, 4553),
    "max": (119, 86, 107),
}


def random_case(seed):
    """60 events of 0..8 distinct edges, each raised by 0..19 (the issue's recipe), sorted by edge."""
    g = small_graph(seed)
    rng = np.random.default_rng(90 + seed)
    edge_sets, metric_sets = [], []
    for k in rng.integers(0, 9, 60):
        ed = rng.choice(660, int(k), replace=False)
        new = g.metric[ed].astype(np.int64) + rng.integers(0, 20, int(k))
        edge_sets.append(ed.tolist())
        metric_sets.append(new.tolist())
    edge_sets, metric_sets = T.metric_events(g, edge_sets, metric_sets)
    return g, edge_sets, metric_sets, SOURCES


def recipe_holds(g, edge_sets, metric_sets):
    """What the events of a graph exercise: (zero raises, empty events, entries on a down edge,
    entries on a row of an overloaded node)."""
    owner = g.edge_owner()
    zero = empty = down = ovl = 0
    for edges, metrics in zip(edge_sets, metric_sets):
        empty += not edges
        for e, m in zip(edges, metrics):
            zero += m == int(g.metric[e])
            down += not g.edge_up[e]
            ovl += bool(g.node_overloaded[owner[e]])
    return zero, empty, down, ovl


def test_random_recipe_holds_every_case():
    held = np.sum([recipe_holds(*random_case(seed)[:3]) for seed in (0, 1, 2)], axis=0)
    assert (held > 0).all(), held  # zero raises, empty events, down edges, overloaded rows: no hand-made event needed


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_edge_raises_match_oracle(eng, bfs_family, seed):
    g, edge_sets, metric_sets, sources = random_case(seed)
    exp = oracle_metric(("random", seed), g, edge_sets, metric_sets, sources)
    assert exp.changed.size == 1800
    assert facts_of(exp) == {k: v[seed] for k, v in RANDOM_FACTS.items()}, facts_of(exp)
    eng.set_graph(g)
    got = eng.whatif_metric(edge_sets, metric_sets, sources)
    check_delta(exp, *got[:5])
    empty = [i for i, e in enumerate(edge_sets) if not e]
    assert not got[0][empty].any()
    assert len(sources) <= got[5] < exp.changed.size + len(sources)
    assert got[5] >= int((exp.changed != 0).sum()) + len(sources)
    # every entry a zero raise: an all-zero row, and no unit of it counts as solved
    i = next(q for q in range(60) if len(edge_sets[q]) >= 2)
    same = [[int(g.metric[e]) for e in edge_sets[i]]]
    changed, solved = eng.whatif_metric([edge_sets[i]], same, sources, want_delta=False)
    assert not changed.any() and solved == len(sources)


# --- 4. against the engine's own old way ---------------------------------------------------------
def test_equals_patch_solve_diff(eng, bfs_family):
    g, edge_sets, metric_sets, sources = row_case(0)
    exp = oracle_metric(("row", 0), g, edge_sets, metric_sets, sources)
    events = [3, 17, 40, 77, 118]
    assert all(exp.changed[i].any() for i in events)
    eng.set_graph(g)
    got = eng.whatif_metric([edge_sets[i] for i in events], [metric_sets[i] for i in events], sources)
    bd, bh, _ = eng.solve(sources)
    for k, i in enumerate(events):
        eng.patch(edges=edge_sets[i], metrics=metric_sets[i], track=False)
        fd, fh, _ = eng.solve(sources)
        eng.patch(edges=edge_sets[i], metrics=[int(g.metric[e]) for e in edge_sets[i]], track=False)
        ch = (fd != bd) | np.any(fh != bh, axis=2)
        np.testing.assert_array_equal(got[0][k], ch.sum(axis=1))
        for j in range(len(sources)):
            a, e = int(got[1][k * len(sources) + j]), int(got[1][k * len(sources) + j + 1])
            vv = np.nonzero(ch[j])[0]
            np.testing.assert_array_equal(got[2][a:e], vv)
            np.testing.assert_array_equal(got[3][a:e], fd[j, vv])
            np.testing.assert_array_equal(got[4][a:e], fh[j, vv])
    d2, h2, _ = eng.solve(sources)  # patched back
    np.testing.assert_array_equal(d2, bd)
    np.testing.assert_array_equal(h2, bh)


# --- 5. other graph families ------------------------------------------------------------------------
def test_grid_both_directions(eng, bfs_family):
    g = T.grid(8)
    sources = list(range(0, 64, 5))
    edge_sets, metric_sets = T.soft_drain_events(g, [[v] for v in range(64)], 1, both_directions=True)
    exp = oracle_metric(("grid8",), g, edge_sets, metric_sets, sources)
    f = facts_of(exp)
    assert exp.changed.size == 832
    assert f == {"unchanged": 0, "over64": 0, "nh_only": 1907, "total": 3913, "max": 63}, f
    eng.set_graph(g)
    got = eng.whatif_metric(edge_sets, metric_sets, sources)
    check_delta(exp, *got[:5])
    # 64 nodes: the default slots hold any unit, nothing is re-run
    assert not any("overflow" in k for k in eng.last_kernels()), eng.last_kernels()


def test_fabric_both_directions(eng, bfs_family):
    g = T.fabric(344)
    sources = list(range(0, 344, 23))
    edge_sets, metric_sets = T.soft_drain_events(g, [[v] for v in range(0, 344, 7)], 1, both_directions=True)
    exp = oracle_metric(("fabric344",), g, edge_sets, metric_sets, sources)
    f = facts_of(exp)
    assert exp.changed.size == 750
    assert (f["unchanged"], f["total"], f["max"]) == (0, 2716, 343), f
    assert int((exp.changed > 128).sum()) == 4
    assert g.nh_bytes() == 11  # the wide next-hop classes: three words per set, the last one partial
    eng.set_graph(g)
    got = eng.whatif_metric(edge_sets, metric_sets, sources)
    check_delta(exp, *got[:5])
    assert "metric_repair<overflow>" in eng.last_kernels()  # 343 nodes outgrow the default slots


# --- 6. capacity crossed --------------------------------------------------------------------------
def test_capacity_crossed(monkeypatch, bfs_family):
    monkeypatch.setenv("OPENR_SPF_METRIC_SLOTS", "16")
    g, edge_sets, metric_sets, sources = row_case(0)
    exp = oracle_metric(("row", 0), g, edge_sets, metric_sets, sources)
    assert int((exp.changed > 16).sum()) > 0
    e = SpfEngine()
    try:
        e.set_graph(g)
        got = e.whatif_metric(edge_sets, metric_sets, sources)
        ks = e.last_kernels()
    finally:
        e.close()
    check_delta(exp, *got[:5])
    assert "metric_repair<overflow>" in ks and "metric_repair" in ks, ks


# --- 7. device form and cap ------------------------------------------------------------------------
def test_device_form_and_cap(eng, bfs_family):
    import torch

    g, edge_sets, metric_sets, sources = random_case(0)
    eng.set_graph(g)
    changed, ptr, node, dist, nh, solved = eng.whatif_metric(edge_sets, metric_sets, sources)
    exp = oracle_metric(("random", 0), g, edge_sets, metric_sets, sources)
    check_delta(exp, changed, ptr, node, dist, nh)
    total, nb, units = int(ptr[-1]), eng.nh_bytes, len(edge_sets) * len(sources)
    assert total == int(changed.sum()) and total > 0
    dev = torch.device("cuda", 0)
    p = np.zeros(len(edge_sets) + 1, dtype=np.int32)
    p[1:] = np.cumsum([len(x) for x in edge_sets])
    d_ep = torch.from_numpy(p).to(dev)
    d_ee = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.int32) for x in edge_sets])).to(dev)
    d_mm = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.int32) for x in metric_sets])).to(dev)
    d_s = torch.from_numpy(np.asarray(sources, dtype=np.int32)).to(dev)
    d_c = torch.full((len(edge_sets), len(sources)), -1, dtype=torch.int32, device=dev)
    d_ptr = torch.zeros(units + 1, dtype=torch.int64, device=dev)
    d_node = torch.zeros(total, dtype=torch.int32, device=dev)
    d_dist = torch.zeros(total, dtype=torch.int64, device=dev)
    d_nh = torch.zeros((total, nb), dtype=torch.uint8, device=dev)
    args = (d_ep.data_ptr(), d_ee.data_ptr(), d_mm.data_ptr(), len(edge_sets), d_ee.numel(), d_s.data_ptr(),
            len(sources), d_c.data_ptr(), d_ptr.data_ptr())
    got, s_dev = eng.whatif_metric_device(*args, d_node.data_ptr(), d_dist.data_ptr(), d_nh.data_ptr(), total, nb)
    assert got == total and s_dev == solved
    np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint32), changed)
    pp = d_ptr.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(pp, ptr)
    pn = d_node.cpu().numpy().view(np.uint32)
    pd = d_dist.cpu().numpy().view(np.uint64)
    ph = d_nh.cpu().numpy()
    for u in range(units):  # the device form keeps the kernel's order: sort each unit by node
        a, e = int(pp[u]), int(pp[u + 1])
        k = np.argsort(pn[a:e], kind="stable")
        np.testing.assert_array_equal(pn[a:e][k], node[a:e])
        np.testing.assert_array_equal(pd[a:e][k], dist[a:e])
        np.testing.assert_array_equal(ph[a:e][k], nh[a:e])
    # cap 0: counts and ptr only (no entry buffers)
    d_c.fill_(-1)
    d_ptr.zero_()
    got0, _ = eng.whatif_metric_device(*args, 0, 0, 0, 0, nb, allow_overflow=True)
    assert got0 == total
    np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint32), changed)
    np.testing.assert_array_equal(d_ptr.cpu().numpy().view(np.uint64), ptr)
    # cap below the total: E2BIG, counts and ptr still filled
    d_c.fill_(-1)
    d_ptr.zero_()
    with pytest.raises(SpfError) as ei:
        eng.whatif_metric_device(*args, d_node.data_ptr(), d_dist.data_ptr(), d_nh.data_ptr(), total - 1, nb)
    assert ei.value.code == E2BIG
    np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint32), changed)
    np.testing.assert_array_equal(d_ptr.cpu().numpy().view(np.uint64), ptr)


def test_two_device_slots(bfs_family):
    """The host forms split the events in contiguous blocks across the context's devices and
    rebase the edge CSR for each block: a context over the same ordinal twice (the suite's
    pattern for the split on a 1-GPU box) gives the oracle's answer, counts, delta and routes."""
    g, edge_sets, metric_sets, sources = random_case(0)
    exp = oracle_metric(("random", 0), g, edge_sets, metric_sets, sources)
    _, dense = tables(0)
    want = expected_routes(("random", 0), g, edge_sets, metric_sets, sources, dense)
    two = SpfEngine([0, 0])
    try:
        two.set_graph(g)
        got = two.whatif_metric(edge_sets, metric_sets, sources)
        check_delta(exp, *got[:5])
        c, _ = two.whatif_metric(edge_sets, metric_sets, sources, want_delta=False)
        np.testing.assert_array_equal(c, exp.changed)
        r = two.whatif_metric_routes(edge_sets, metric_sets, sources, dense)
        for k in (0, 1, 2, 3):
            np.testing.assert_array_equal(r[k], want[k])
    finally:
        two.close()


# --- 7b. both event sweeps on one engine -------------------------------------------------------------
def head_of(exp, n_events, n_src):
    """The first n_events events of an oracle table."""
    units = n_events * n_src
    end = int(exp.ptr[units])
    return dataclasses.replace(exp, changed=exp.changed[:n_events], ptr=exp.ptr[: units + 1], node=exp.node[:end],
                               dist=exp.dist[:end], nh=exp.nh[:end], same_dist=exp.same_dist[:end])


def test_drain_metric_drain_on_one_engine(eng, bfs_family):
    """The drain and the metric sweep run one repair body and one driver: drain -> metric ->
    drain on one engine and one graph, each against its module's oracle table; the second
    drain result is the first, so the counters and the slot index are at rest between sweeps
    of different kinds."""
    n = 30
    g, edge_sets, metric_sets, sources = row_case(0)
    _, events, drain_sources = drain_tests.single_case(0)
    assert drain_sources == sources
    want_d = head_of(drain_tests.oracle_drain(("single", 0), g, events, None, sources), n, len(sources))
    want_m = head_of(oracle_metric(("row", 0), g, edge_sets, metric_sets, sources), n, len(sources))
    assert want_d.changed.any() and want_m.changed.any()
    assert not np.array_equal(want_d.changed, want_m.changed)  # the two kinds answer differently
    eng.set_graph(g)
    first = eng.whatif_drain(events[:n], sources)
    assert "drain_filter" in eng.last_kernels() and "drain_repair" in eng.last_kernels(), eng.last_kernels()
    check_delta(want_d, *first[:5])
    got = eng.whatif_metric(edge_sets[:n], metric_sets[:n], sources)
    assert "metric_filter" in eng.last_kernels() and "metric_repair" in eng.last_kernels(), eng.last_kernels()
    check_delta(want_m, *got[:5])
    second = eng.whatif_drain(events[:n], sources)
    assert "drain_repair" in eng.last_kernels(), eng.last_kernels()
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)


# --- 8. routes --------------------------------------------------------------------------------------
def expected_routes(key, g, edge_sets, metric_sets, sources, groups):
    """(changed_routes [n_events, S], ptr, group, metric, nh, n_best, same_metric count) from
    the oracle rows through test_gpu_routes_resolve.reduce_routes."""
    bd, bh, fd, fh = oracle_rows(key, g, edge_sets, metric_sets, sources)
    n = len(edge_sets)
    bm, bnh, _ = reduce_routes(bd, bh, groups)
    fm, fnh, fnb = reduce_routes(fd, fh, groups)
    bmu, bnhu = np.tile(bm, (n, 1)), np.tile(bnh, (n, 1, 1))
    ch = (fm != bmu) | np.any(fnh != bnhu, axis=2)
    counts = ch.sum(axis=1).astype(np.uint32)
    ptr = np.zeros(ch.shape[0] + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(counts, dtype=np.uint64)
    uu, kk = np.nonzero(ch)
    same_metric = int((ch & (fm == bmu)).sum())
    return counts.reshape(n, len(sources)), ptr, kk.astype(np.uint32), fm[uu, kk], fnh[uu, kk], fnb[uu, kk], same_metric


@pytest.mark.parametrize("seed", [0, 1])
def test_metric_routes_match_oracle(eng, bfs_family, seed):
    g, edge_sets, metric_sets, sources = random_case(seed)
    _, dense = tables(seed)
    want = expected_routes(("random", seed), g, edge_sets, metric_sets, sources, dense)
    assert want[0].any() and want[6] > 0  # some changed route keeps its metric
    eng.set_graph(g)
    changed, ptr, group, metric, nh, n_best, solved = eng.whatif_metric_routes(edge_sets, metric_sets, sources, dense)
    np.testing.assert_array_equal(changed, want[0])
    np.testing.assert_array_equal(ptr, want[1])
    np.testing.assert_array_equal(group, want[2])
    np.testing.assert_array_equal(metric, want[3])
    np.testing.assert_array_equal(nh[:, : want[4].shape[1]], want[4])
    assert not nh[:, want[4].shape[1]:].any()
    np.testing.assert_array_equal(n_best, want[5])
    assert solved >= len(sources)


def test_no_loopback_route_is_lost(eng, bfs_family):
    """Adjacency soft drains over the loopback table: a metric raise disconnects nothing."""
    g, edge_sets, metric_sets, sources = row_case(0)
    loop = T.loopback_groups(g)
    want = expected_routes(("row", 0), g, edge_sets, metric_sets, sources, loop)
    assert want[0].any() and not (want[3] == U64_MAX).any()
    eng.set_graph(g)
    changed, ptr, group, metric, nh, n_best, _ = eng.whatif_metric_routes(edge_sets, metric_sets, sources, loop)
    np.testing.assert_array_equal(changed, want[0])
    np.testing.assert_array_equal(ptr, want[1])
    np.testing.assert_array_equal(group, want[2])
    np.testing.assert_array_equal(metric, want[3])
    assert not (metric == U64_MAX).any()


# --- 9. errors and empty inputs --------------------------------------------------------------------
def test_errors_and_empty_inputs(eng, bfs_family):
    g = small_graph(2)
    V, E = g.num_nodes, g.num_dir_edges
    w = [int(x) for x in g.metric]
    eng.set_graph(g)
    lower = next(e for e in range(E) if w[e] > 1)
    for call in (lambda: eng.whatif_metric([[0, E]], [[w[0], 5]], [0]),  # an edge >= E
                 lambda: eng.whatif_metric([[3, 2]], [[w[3], w[2]]], [0]),  # a slice that does not ascend
                 lambda: eng.whatif_metric([[2, 2]], [[w[2], w[2] + 1]], [0]),  # ... not strictly
                 lambda: eng.whatif_metric([[lower]], [[w[lower] - 1]], [0]),  # a metric below the current one
                 lambda: eng.whatif_metric([[0]], [[2**31]], [0]),  # ... above 2^31 - 1
                 lambda: eng.whatif_metric([[0]], [[w[0]]], [V]),  # a source >= V
                 lambda: eng.whatif_metric_routes([[E]], [[5]], [0], [[0]]),
                 lambda: eng.whatif_metric_routes([[lower]], [[w[lower] - 1]], [0], [[0]])):
        with pytest.raises(SpfError) as ei:
            call()
        assert ei.value.code == EINVAL
    # a non-ascending and a null edge_ptr (raw calls)
    ep = np.array([0, 2, 1], dtype=np.uint32)
    ee = np.array([0, 1, 2], dtype=np.uint32)
    mm = np.array([w[0], w[1], w[2]], dtype=np.uint32)
    src = np.array([0], dtype=np.uint32)
    out = np.zeros((2, 1), dtype=np.uint32)
    ev = MetricEvents(2, _p(ep), _p(ee), _p(mm))
    rc = eng._lib.openr_spf_whatif_metric(eng._ctx, ctypes.byref(ev), _p(src), 1, USE_LINK_METRIC, _p(out), None, None)
    assert rc == EINVAL
    ev = MetricEvents(2, None, _p(ee), _p(mm))
    rc = eng._lib.openr_spf_whatif_metric(eng._ctx, ctypes.byref(ev), _p(src), 1, USE_LINK_METRIC, _p(out), None, None)
    assert rc == EINVAL
    # more than 2^32 - 1 units: refused before anything is read past the event CSR
    big = np.zeros(65537, dtype=np.uint32)
    ev = MetricEvents(65536, _p(big), _p(ee), _p(mm))
    srcs = np.zeros(65536, dtype=np.uint32)
    rc = eng._lib.openr_spf_whatif_metric(eng._ctx, ctypes.byref(ev), _p(srcs), 65536, USE_LINK_METRIC, _p(out), None,
                                          None)
    assert rc == EINVAL
    # zero events or zero sources: empty results, ptr == [0]
    got = eng.whatif_metric([], [], [0, 1])
    assert got[0].shape == (0, 2) and got[1].tolist() == [0] and len(got[2]) == 0 and got[5] == 0
    got = eng.whatif_metric([[0]], [[w[0] + 1]], [])
    assert got[0].shape == (1, 0) and got[1].tolist() == [0] and got[5] == 0
    got = eng.whatif_metric_routes([], [], [0], [[0]])
    assert got[0].shape == (0, 1) and got[1].tolist() == [0]
    # the hop-count form is served without a kernel: metrics do not enter runSpf(src, false)
    edge_sets, metric_sets = T.soft_drain_events(g, [[v] for v in range(0, V, 3)], 7)
    sources = list(range(0, V, 12))
    assert eng.whatif_metric(edge_sets, metric_sets, sources, want_delta=False)[0].any()
    got = eng.whatif_metric(edge_sets, metric_sets, sources, use_link_metric=False)
    assert got[0].shape == (len(edge_sets), len(sources)) and not got[0].any()
    assert not got[1].any() and len(got[1]) == got[0].size + 1 and len(got[2]) == 0 and got[5] == 0
    assert eng.last_kernels() == []
    r = eng.whatif_metric_routes(edge_sets, metric_sets, sources, T.loopback_groups(g), use_link_metric=False)
    assert not r[0].any() and not r[1].any() and r[6] == 0 and eng.last_kernels() == []
    # one usable metric set to 0: the base SPF needs the exact-order kernel under link metric
    m = g.metric.copy()
    m[int(np.nonzero(g.edge_up != 0)[0][10])] = 0
    gz = dataclasses.replace(g, metric=m)
    eng.set_graph(gz)
    with pytest.raises(SpfError) as ei:
        eng.whatif_metric([[1]], [[int(m[1]) + 1]], [0])
    assert ei.value.code == ENOTSUP
