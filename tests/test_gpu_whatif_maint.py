"""Maintenance what-if sweep on the GPU (openr_spf_whatif_maint*) vs the CPU oracle.

A maintenance event overloads a set of nodes, takes a set of links out of service and raises
the metrics of a list of directed edges, all at once; unit (i, j) is the oracle's
runSpf(source j, useLinkMetric) on the graph patched with all three, diffed against the
no-event run. The module runs on both parametrisations of tests/test_gpu_whatif_drain.py, so
the base rows the repair reads come from every kernel family. The oracle-side tables were
computed on the CPU with the oracle alone and are asserted before the engine is compared, so a
vacuous recipe cannot pass; among them is the number of units whose answer differs from both
the drain-only and the metric-only run of the same event, which is what shows that the union
rule is under test.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from openr_amd import topology as T
from openr_amd.engine import E2BIG, EINVAL, ENOTSUP, USE_LINK_METRIC, MaintEvents, SpfEngine, SpfError, _p
import test_gpu_whatif_drain as drain_tests
import test_gpu_whatif_metric as metric_tests
from oracle import Oracle
from test_gpu_routes_resolve import reduce_routes, tables
from test_gpu_whatif_sets import check_delta, small_graph

pytestmark = pytest.mark.gpu

U64_MAX = np.uint64(2**64 - 1)
SOURCES = list(range(0, 120, 4))
Expect = drain_tests.Expect


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


# --- oracle side: computed once per (graph, events, sources, metric form), shared by both
# --- parametrisations of the module and never modified
_EXPECT = {}
_ROWS = {}


def oracle_rows(key, g, ev, sources, use_metric=True):
    """(base dist [S, V], base nh, event dist [n_events * S, V], event nh) of every unit; ev =
    (node_sets, link_sets, edge_sets, metric_sets), a kind None: none of it."""
    k = (key, bool(use_metric))
    if k not in _ROWS:
        o = Oracle(g)
        base = [o.run_spf(int(s), use_metric) for s in sources]
        n = len(next(x for x in ev if x is not None))
        runs = []
        for i in range(n):
            nodes, links, edges, metrics = ([int(v) for v in x[i]] if x is not None else [] for x in ev)
            if not (nodes or links or edges):
                runs += base
                continue
            oe = Oracle(g.patched(edges, metrics, links, [0] * len(links), nodes, [1] * len(nodes)))
            runs += [oe.run_spf(int(s), use_metric) for s in sources]
        rows = (np.stack([r.dist for r in base]), np.stack([r.nh for r in base]),
                np.stack([r.dist for r in runs]), np.stack([r.nh for r in runs]))
        for a in rows:
            a.setflags(write=False)
        _ROWS[k] = rows
    return _ROWS[k]


def oracle_maint(key, g, ev, sources, use_metric=True):
    """Expected changed counts and delta rows of every unit (event i, source j)."""
    k = (key, bool(use_metric))
    if k in _EXPECT:
        return _EXPECT[k]
    bd, bh, fd, fh = oracle_rows(key, g, ev, sources, use_metric)
    n, S = fd.shape[0] // len(sources), len(sources)
    bdu, bhu = np.tile(bd, (n, 1)), np.tile(bh, (n, 1, 1))
    assert (fd >= bdu).all()  # no distance shrinks
    ch = (fd != bdu) | np.any(fh != bhu, axis=2)  # [units, V]
    counts = ch.sum(axis=1).astype(np.uint32)
    ptr = np.zeros(ch.shape[0] + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(counts, dtype=np.uint64)
    uu, vv = np.nonzero(ch)  # row-major: units ascending, nodes ascending inside a unit
    e = Expect(counts.reshape(n, S), ptr, vv.astype(np.uint32), fd[uu, vv], fh[uu, vv], fd[uu, vv] == bdu[uu, vv], bd)
    for a in dataclasses.astuple(e):
        a.setflags(write=False)
    _EXPECT[k] = e
    return e


def units_differing(a, b):
    """Units whose rows (dist or next hops) differ between two oracle_rows results."""
    return (a[2] != b[2]).any(axis=1) | (a[3] != b[3]).any(axis=(1, 2))


def facts_of(exp):
    return {
        "unchanged": int((exp.changed == 0).sum()),
        "over64": int((exp.changed > 64).sum()),
        "unreachable": int((exp.dist == U64_MAX).sum()),
        "nh_only": int(exp.same_dist.sum()),
        "total": int(exp.ptr[-1]),
        "max": int(exp.changed.max()),
    }


def head_of(ev, n):
    return tuple(x[:n] if x is not None else None for x in ev)


# --- 1. mixed events ---------------------------------------------------------------------------
MIXED_FACTS = {  # oracle side, seeds 0 / 1 / 2
    "unchanged": (64, 154, 197),
    "over64": (90, 78, 61),
    "unreachable": (769, 179, 205),
    "nh_only": (451, 12373, 4402),
    "total": (29815, 26640, 24826),
    "max": (119, 118, 119),
}
MIXED_UNION = {  # units differing from the drain-only run of (N, K), the metric-only run, both
    "vs_drain": (1586, 1380, 1349),
    "vs_metric": (1351, 1309, 1108),
    "vs_both": (1201, 1043, 854),
    "all_three_kinds": (25, 27, 24),
}
# over the three seeds: empty events; events with a raise on a drained node's row, (of those)
# the node being a source too; with a raise on a removed link; on a down edge; with an
# already-overloaded node in N_i; with a raise on an overloaded node's row
MIXED_CORNERS = (2, 23, 3, 4, 44, 17, 79)


def mixed_case(seed):
    """60 events of 0..3 hard-drained nodes, 0..2 links out of service and 0..3 nodes soft-drained
    in both directions (the issue's recipe)."""
    g = small_graph(seed)
    assert g.num_nodes == 120 and g.num_links == 330 and g.num_dir_edges == 660
    rng = np.random.default_rng(90 + seed)
    node_sets = [sorted(rng.choice(120, int(k), replace=False).tolist()) for k in rng.integers(0, 4, 60)]
    link_sets = [sorted(rng.choice(330, int(k), replace=False).tolist()) for k in rng.integers(0, 3, 60)]
    soft = [sorted(rng.choice(120, int(k), replace=False).tolist()) for k in rng.integers(0, 4, 60)]
    edge_sets, metric_sets = T.soft_drain_events(g, soft, {0: 40, 1: 1, 2: 5}[seed], both_directions=True)
    return g, (node_sets, link_sets, edge_sets, metric_sets), SOURCES


def corner_cases(g, ev, sources):
    """What the events of a graph hold, as events counted: MIXED_CORNERS' order."""
    owner = g.edge_owner()
    ovl = {int(v) for v in np.nonzero(g.node_overloaded)[0]}
    empty = drained_row = drained_src = on_link = on_down = ovl_node = ovl_row = 0
    for nodes, links, edges, metrics in zip(*ev):
        assert all(m > int(g.metric[e]) for e, m in zip(edges, metrics))  # every entry is a raise
        empty += not (nodes or links or edges)
        hit = {int(owner[e]) for e in edges} & set(nodes)
        drained_row += bool(hit)
        drained_src += bool(hit & set(sources))
        on_link += bool({int(g.link_id[e]) for e in edges} & set(links))
        on_down += any(not g.edge_up[e] for e in edges)
        ovl_node += bool(ovl & set(nodes))
        ovl_row += bool(ovl & {int(owner[e]) for e in edges})
    return empty, drained_row, drained_src, on_link, on_down, ovl_node, ovl_row


def test_recipe_holds_every_corner_case():
    held = np.sum([corner_cases(*mixed_case(seed)) for seed in (0, 1, 2)], axis=0)
    assert tuple(int(x) for x in held) == MIXED_CORNERS, held


def mixed_union_facts(seed):
    g, ev, sources = mixed_case(seed)
    rows = oracle_rows(("mixed", seed), g, ev, sources)
    drain = oracle_rows(("mixed-drain", seed), g, (ev[0], ev[1], None, None), sources)
    metric = oracle_rows(("mixed-metric", seed), g, (None, None, ev[2], ev[3]), sources)
    vd, vm = units_differing(rows, drain), units_differing(rows, metric)
    return {
        "vs_drain": int(vd.sum()),
        "vs_metric": int(vm.sum()),
        "vs_both": int((vd & vm).sum()),
        "all_three_kinds": sum(1 for n, l, e in zip(*ev[:3]) if n and l and e),
    }


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mixed_events_match_oracle(eng, bfs_family, seed):
    g, ev, sources = mixed_case(seed)
    exp = oracle_maint(("mixed", seed), g, ev, sources)
    assert exp.changed.size == 1800
    assert facts_of(exp) == {k: v[seed] for k, v in MIXED_FACTS.items()}, facts_of(exp)
    union = mixed_union_facts(seed)
    assert union == {k: v[seed] for k, v in MIXED_UNION.items()}, union
    eng.set_graph(g)
    changed, solved = eng.whatif_maint(*ev, sources, want_delta=False)
    ks = eng.last_kernels()
    assert "maint_filter" in ks and "maint_repair" in ks, ks
    np.testing.assert_array_equal(changed, exp.changed)
    assert int((exp.changed != 0).sum()) + len(sources) <= solved < changed.size + len(sources)
    got = eng.whatif_maint(*ev, sources)
    assert got[5] == solved
    check_delta(exp, *got[:5])
    empty = [i for i in range(60) if not (ev[0][i] or ev[1][i] or ev[2][i])]
    assert not got[0][empty].any()
    # every node and link listed twice: the identical result (an edge slice stays strictly ascending)
    twice = eng.whatif_maint([x + x for x in ev[0]], [x + x for x in ev[1]], ev[2], ev[3], sources)
    for a, b in zip(got, twice):
        np.testing.assert_array_equal(a, b)


# --- 2. reductions ---------------------------------------------------------------------------------
def test_reduces_to_drain_and_metric(eng, bfs_family):
    g, ev, sources = mixed_case(0)
    eng.set_graph(g)
    as_drain = eng.whatif_maint(ev[0], ev[1], None, None, sources)
    assert "maint_repair" in eng.last_kernels()
    drain = eng.whatif_drain(ev[0], sources, link_sets=ev[1])
    assert as_drain[0].any()
    for a, b in zip(as_drain, drain):
        np.testing.assert_array_equal(a, b)
    as_metric = eng.whatif_maint(None, None, ev[2], ev[3], sources)
    assert "maint_repair" in eng.last_kernels()
    metric = eng.whatif_metric(ev[2], ev[3], sources)
    assert as_metric[0].any() and not np.array_equal(as_metric[0], as_drain[0])
    for a, b in zip(as_metric, metric):
        np.testing.assert_array_equal(a, b)


# --- 3. hop count and a wider nh_bytes ---------------------------------------------------------------
HOPS_UNCHANGED = (29, 32, 39)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_hop_count_ignores_metrics(eng, bfs_family, seed):
    g, ev, sources = mixed_case(seed)
    ev, sources = head_of(ev, 20), sources[:6]
    rows = oracle_rows(("hops", seed), g, ev, sources, False)
    drain = oracle_rows(("hops-drain", seed), g, (ev[0], ev[1], None, None), sources, False)
    assert not units_differing(rows, drain).any()  # metrics do not enter runSpf(src, false)
    exp = oracle_maint(("hops", seed), g, ev, sources, False)
    assert exp.changed.size == 120 and int((exp.changed == 0).sum()) == HOPS_UNCHANGED[seed]
    eng.set_graph(g)
    got = eng.whatif_maint(*ev, sources, use_link_metric=False, nh_bytes=eng.nh_bytes + 5)
    assert got[4].shape[1] == eng.nh_bytes + 5
    check_delta(exp, *got[:5])
    ks = eng.last_kernels()
    assert "maint_filter" in ks and "maint_repair" in ks, ks


# --- 4. against the engine's own old way -----------------------------------------------------------
def test_equals_patch_solve_diff(eng, bfs_family):
    g, ev, sources = mixed_case(0)
    exp = oracle_maint(("mixed", 0), g, ev, sources)
    events = [i for i in range(60) if ev[0][i] and ev[1][i] and ev[2][i] and exp.changed[i].any()][:5]
    assert len(events) == 5
    eng.set_graph(g)
    got = eng.whatif_maint(*(tuple(x[i] for i in events) for x in ev), sources)
    bd, bh, _ = eng.solve(sources)
    for k, i in enumerate(events):
        nodes, links, edges, metrics = (x[i] for x in ev)
        was_ovl = [int(g.node_overloaded[v]) for v in nodes]
        was_up = link_state(g, links)
        eng.patch(edges=edges, metrics=metrics, links=links, link_up=[0] * len(links), nodes=nodes,
                  node_overloaded=[1] * len(nodes), track=False)
        fd, fh, _ = eng.solve(sources)
        eng.patch(edges=edges, metrics=[int(g.metric[e]) for e in edges], links=links, link_up=was_up, nodes=nodes,
                  node_overloaded=was_ovl, track=False)
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


def link_state(g, links):
    """1 for a link both of whose directed edges are up, else 0."""
    return [int(all(g.edge_up[e] for e in np.nonzero(g.link_id == l)[0])) for l in links]


# --- 5. other graph families ------------------------------------------------------------------------
GRID_FACTS = {"unchanged": 0, "over64": 0, "unreachable": 0, "nh_only": 2951, "total": 5444, "max": 63}
FABRIC_FACTS = {"unchanged": 0, "over64": 8, "unreachable": 846, "nh_only": 186, "total": 3296, "max": 343}


def grid_case():
    g = T.grid(8)
    edge_sets, metric_sets = T.soft_drain_events(g, [[(v + 1) % 64] for v in range(64)], 1, both_directions=True)
    return g, ([[v] for v in range(64)], None, edge_sets, metric_sets), list(range(0, 64, 5))


def fabric_case():
    g = T.fabric(344)
    edge_sets, metric_sets = T.soft_drain_events(g, [[7 * k + 3] for k in range(49)], 1, both_directions=True)
    return g, ([[7 * k] for k in range(49)], None, edge_sets, metric_sets), list(range(0, 344, 23))


def test_grid_overload_next_to_soft_drain(eng, bfs_family):
    g, ev, sources = grid_case()
    exp = oracle_maint(("grid8",), g, ev, sources)
    assert exp.changed.size == 832
    assert facts_of(exp) == GRID_FACTS, facts_of(exp)
    eng.set_graph(g)
    got = eng.whatif_maint(*ev, sources)
    check_delta(exp, *got[:5])
    # 64 nodes: the default slots hold any unit, nothing is re-run
    assert "maint_repair" in eng.last_kernels() and not any("overflow" in k for k in eng.last_kernels())


def test_fabric_overload_next_to_soft_drain(eng, bfs_family):
    g, ev, sources = fabric_case()
    exp = oracle_maint(("fabric344",), g, ev, sources)
    assert exp.changed.size == 735
    assert facts_of(exp) == FABRIC_FACTS, facts_of(exp)
    assert int((exp.changed > 256).sum()) == 4  # units that outgrow the default slots
    assert g.nh_bytes() == 11  # the wide next-hop classes: three words per set, the last one partial
    eng.set_graph(g)
    got = eng.whatif_maint(*ev, sources)
    check_delta(exp, *got[:5])
    assert "maint_repair<overflow>" in eng.last_kernels()


# --- 6. capacity crossed --------------------------------------------------------------------------
def test_capacity_crossed(monkeypatch, bfs_family):
    monkeypatch.setenv("OPENR_SPF_MAINT_SLOTS", "16")
    g, ev, sources = mixed_case(0)
    exp = oracle_maint(("mixed", 0), g, ev, sources)
    assert int((exp.changed > 16).sum()) > 0 and int(((exp.changed > 0) & (exp.changed < 8)).sum()) > 0
    e = SpfEngine()
    try:
        e.set_graph(g)
        got = e.whatif_maint(*ev, sources)
        ks = e.last_kernels()
    finally:
        e.close()
    check_delta(exp, *got[:5])
    assert "maint_repair<overflow>" in ks and "maint_repair" in ks, ks


# --- 7. device form and cap ------------------------------------------------------------------------
def test_device_form_and_cap(eng, bfs_family):
    import torch

    g, ev, sources = mixed_case(0)
    eng.set_graph(g)
    changed, ptr, node, dist, nh, solved = eng.whatif_maint(*ev, sources)
    check_delta(oracle_maint(("mixed", 0), g, ev, sources), changed, ptr, node, dist, nh)
    total, nb, units = int(ptr[-1]), eng.nh_bytes, 60 * len(sources)
    assert total == int(changed.sum()) and total > 0
    dev = torch.device("cuda", 0)

    def csr(sets):
        p = np.zeros(len(sets) + 1, dtype=np.int32)
        p[1:] = np.cumsum([len(x) for x in sets])
        return torch.from_numpy(p).to(dev)

    def flat(sets):
        return torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.int32) for x in sets])).to(dev)

    d_np, d_lp, d_ep = (csr(x) for x in ev[:3])
    d_nn, d_ll, d_ee, d_mm = (flat(x) for x in ev)
    d_s = torch.from_numpy(np.asarray(sources, dtype=np.int32)).to(dev)
    d_c = torch.full((60, len(sources)), -1, dtype=torch.int32, device=dev)
    d_ptr = torch.zeros(units + 1, dtype=torch.int64, device=dev)
    d_node = torch.zeros(total, dtype=torch.int32, device=dev)
    d_dist = torch.zeros(total, dtype=torch.int64, device=dev)
    d_nh = torch.zeros((total, nb), dtype=torch.uint8, device=dev)
    args = (d_np.data_ptr(), d_nn.data_ptr(), d_lp.data_ptr(), d_ll.data_ptr(), d_ep.data_ptr(), d_ee.data_ptr(),
            d_mm.data_ptr(), 60, d_nn.numel(), d_ll.numel(), d_ee.numel(), d_s.data_ptr(), len(sources),
            d_c.data_ptr(), d_ptr.data_ptr())
    got, s_dev = eng.whatif_maint_device(*args, d_node.data_ptr(), d_dist.data_ptr(), d_nh.data_ptr(), total, nb)
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
    got0, s0 = eng.whatif_maint_device(*args, 0, 0, 0, 0, nb, allow_overflow=True)
    assert got0 == total and s0 == solved
    np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint32), changed)
    np.testing.assert_array_equal(d_ptr.cpu().numpy().view(np.uint64), ptr)
    # cap below the total: E2BIG, counts and ptr still filled
    d_c.fill_(-1)
    d_ptr.zero_()
    with pytest.raises(SpfError) as ei:
        eng.whatif_maint_device(*args, d_node.data_ptr(), d_dist.data_ptr(), d_nh.data_ptr(), total - 1, nb)
    assert ei.value.code == E2BIG
    np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint32), changed)
    np.testing.assert_array_equal(d_ptr.cpu().numpy().view(np.uint64), ptr)


# --- 8. two device slots ---------------------------------------------------------------------------
def test_two_device_slots(bfs_family):
    """The host forms split the events in contiguous blocks across the context's devices and
    rebase the three CSRs for each block: a context over the same ordinal twice gives the
    oracle's answer, counts, delta and routes."""
    g, ev, sources = mixed_case(0)
    exp = oracle_maint(("mixed", 0), g, ev, sources)
    _, dense = tables(0)
    want = expected_routes(("mixed", 0), g, ev, sources, dense)
    two = SpfEngine([0, 0])
    try:
        two.set_graph(g)
        got = two.whatif_maint(*ev, sources)
        check_delta(exp, *got[:5])
        c, _ = two.whatif_maint(*ev, sources, want_delta=False)
        np.testing.assert_array_equal(c, exp.changed)
        r = two.whatif_maint_routes(*ev, sources, dense)
        for k in (0, 1, 2, 3):
            np.testing.assert_array_equal(r[k], want[k])
    finally:
        two.close()


# --- 9. kinds interleaved on one engine ------------------------------------------------------------
def test_drain_maint_metric_maint_on_one_engine(eng, bfs_family):
    """drain -> maint -> metric -> maint on one engine and one graph: the drain and the metric
    result against their own modules' oracle tables, the two maint results identical, so the
    counters and the slot index are at rest between sweeps of different kinds."""
    n = 30
    g, ev, sources = mixed_case(0)
    _, edge_sets, metric_sets, msources = metric_tests.row_case(0)
    _, events, dsources = drain_tests.single_case(0)
    assert dsources == sources and msources == sources
    want_d = metric_tests.head_of(drain_tests.oracle_drain(("single", 0), g, events, None, sources), n, len(sources))
    want_m = metric_tests.head_of(metric_tests.oracle_metric(("row", 0), g, edge_sets, metric_sets, sources), n,
                                  len(sources))
    want = metric_tests.head_of(oracle_maint(("mixed", 0), g, ev, sources), n, len(sources))
    assert want_d.changed.any() and want_m.changed.any() and want.changed.any()
    ev = head_of(ev, n)
    eng.set_graph(g)
    check_delta(want_d, *eng.whatif_drain(events[:n], sources)[:5])
    assert "drain_repair" in eng.last_kernels(), eng.last_kernels()
    first = eng.whatif_maint(*ev, sources)
    assert "maint_filter" in eng.last_kernels() and "maint_repair" in eng.last_kernels(), eng.last_kernels()
    check_delta(want, *first[:5])
    check_delta(want_m, *eng.whatif_metric(edge_sets[:n], metric_sets[:n], sources)[:5])
    assert "metric_repair" in eng.last_kernels(), eng.last_kernels()
    second = eng.whatif_maint(*ev, sources)
    assert "maint_repair" in eng.last_kernels(), eng.last_kernels()
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)


# --- 10. routes -------------------------------------------------------------------------------------
def expected_routes(key, g, ev, sources, groups):
    """(changed_routes [n_events, S], ptr, group, metric, nh, n_best, base metric of every entry)
    from the oracle rows through test_gpu_routes_resolve.reduce_routes."""
    bd, bh, fd, fh = oracle_rows(key, g, ev, sources)
    n = fd.shape[0] // len(sources)
    bm, bnh, _ = reduce_routes(bd, bh, groups)
    fm, fnh, fnb = reduce_routes(fd, fh, groups)
    bmu, bnhu = np.tile(bm, (n, 1)), np.tile(bnh, (n, 1, 1))
    ch = (fm != bmu) | np.any(fnh != bnhu, axis=2)
    counts = ch.sum(axis=1).astype(np.uint32)
    ptr = np.zeros(ch.shape[0] + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(counts, dtype=np.uint64)
    uu, kk = np.nonzero(ch)
    return counts.reshape(n, len(sources)), ptr, kk.astype(np.uint32), fm[uu, kk], fnh[uu, kk], fnb[uu, kk], bmu[uu, kk]


@pytest.mark.parametrize("seed", [0, 1])
def test_maint_routes_match_oracle(eng, bfs_family, seed):
    g, ev, sources = mixed_case(seed)
    _, dense = tables(seed)
    want = expected_routes(("mixed", seed), g, ev, sources, dense)
    assert want[0].any()
    # some routes turn unreachable through K_i: more than the same events lose without their links
    lost = int(((want[3] == U64_MAX) & (want[6] != U64_MAX)).sum())
    nodes_only = expected_routes(("mixed-nodes", seed), g, (ev[0], None, ev[2], ev[3]), sources, dense)
    lost_nodes_only = int(((nodes_only[3] == U64_MAX) & (nodes_only[6] != U64_MAX)).sum())
    assert (lost, lost_nodes_only) == ((915, 730), (179, 119))[seed], (lost, lost_nodes_only)
    eng.set_graph(g)
    changed, ptr, group, metric, nh, n_best, solved = eng.whatif_maint_routes(*ev, sources, dense)
    np.testing.assert_array_equal(changed, want[0])
    np.testing.assert_array_equal(ptr, want[1])
    np.testing.assert_array_equal(group, want[2])
    np.testing.assert_array_equal(metric, want[3])
    np.testing.assert_array_equal(nh[:, : want[4].shape[1]], want[4])
    assert not nh[:, want[4].shape[1]:].any()
    np.testing.assert_array_equal(n_best, want[5])
    assert solved >= len(sources)


def test_drained_loopback_stays_reachable(eng, bfs_family):
    """Over the loopback table, without the links: where an event drains one node alone, that
    node's loopback keeps a finite metric wherever the base reached it (a drain is not a
    failure; behind a second drained node it can be cut off)."""
    g, ev, sources = mixed_case(0)
    ev = (ev[0], None, ev[2], ev[3])
    loop = T.loopback_groups(g)
    want = expected_routes(("mixed-nodes", 0), g, ev, sources, loop)
    assert want[0].any()
    drained = 0
    for u in range(want[0].size):
        a, e = int(want[1][u]), int(want[1][u + 1])
        for k in range(a, e):
            if [int(want[2][k])] == ev[0][u // len(sources)] and want[6][k] != U64_MAX:
                assert want[3][k] != U64_MAX
                drained += 1
    assert drained > 0
    eng.set_graph(g)
    changed, ptr, group, metric, nh, n_best, _ = eng.whatif_maint_routes(*ev, sources, loop)
    np.testing.assert_array_equal(changed, want[0])
    np.testing.assert_array_equal(ptr, want[1])
    np.testing.assert_array_equal(group, want[2])
    np.testing.assert_array_equal(metric, want[3])


# --- 11. errors and empty inputs --------------------------------------------------------------------
def test_errors_and_empty_inputs(eng, bfs_family):
    g = small_graph(2)
    V, L, E = g.num_nodes, g.num_links, g.num_dir_edges
    w = [int(x) for x in g.metric]
    eng.set_graph(g)
    lower = next(e for e in range(E) if w[e] > 1)
    for call in (lambda: eng.whatif_maint([[V]], None, None, None, [0]),  # a node >= V
                 lambda: eng.whatif_maint([[0]], [[L]], None, None, [0]),  # a link >= L
                 lambda: eng.whatif_maint([[0]], None, [[0, E]], [[w[0], 5]], [0]),  # an edge >= E
                 lambda: eng.whatif_maint(None, None, [[3, 2]], [[w[3], w[2]]], [0]),  # a slice that does not ascend
                 lambda: eng.whatif_maint(None, None, [[2, 2]], [[w[2], w[2] + 1]], [0]),  # ... not strictly
                 lambda: eng.whatif_maint([[1]], [[1]], [[lower]], [[w[lower] - 1]], [0]),  # a decrease
                 lambda: eng.whatif_maint(None, None, [[0]], [[2**31]], [0]),  # a metric above 2^31 - 1
                 lambda: eng.whatif_maint([[0]], None, None, None, [V]),  # a source >= V
                 lambda: eng.whatif_maint_routes([[V]], None, None, None, [0], [[0]]),
                 lambda: eng.whatif_maint_routes([[0]], None, [[lower]], [[w[lower] - 1]], [0], [[0]])):
        with pytest.raises(SpfError) as ei:
            call()
        assert ei.value.code == EINVAL
    # non-ascending and null ptr arrays (raw calls)
    up = np.array([0, 1, 2], dtype=np.uint32)
    down = np.array([0, 2, 1], dtype=np.uint32)
    ids = np.array([0, 1, 2], dtype=np.uint32)
    mm = np.array([w[0], w[1], w[2]], dtype=np.uint32)
    src = np.array([0], dtype=np.uint32)
    out = np.zeros((2, 1), dtype=np.uint32)

    def raw(ev, srcs=src, n=1):
        return eng._lib.openr_spf_whatif_maint(eng._ctx, ctypes.byref(ev), _p(srcs), n, USE_LINK_METRIC, _p(out), None,
                                               None)

    assert raw(MaintEvents(2, _p(up), _p(ids), None, None, None, None, None)) == 0
    assert raw(MaintEvents(2, None, _p(ids), None, None, None, None, None)) == EINVAL  # null node_ptr
    assert raw(MaintEvents(2, _p(down), _p(ids), None, None, None, None, None)) == EINVAL
    assert raw(MaintEvents(2, _p(up), _p(ids), _p(down), _p(ids), None, None, None)) == EINVAL
    assert raw(MaintEvents(2, _p(up), _p(ids), None, None, _p(down), _p(ids), _p(mm))) == EINVAL
    # more than 2^32 - 1 units: refused before anything is read past the event CSRs
    big = np.zeros(65537, dtype=np.uint32)
    srcs = np.zeros(65536, dtype=np.uint32)
    assert raw(MaintEvents(65536, _p(big), _p(ids), None, None, None, None, None), srcs, 65536) == EINVAL
    # zero events or zero sources: empty results, ptr == [0]
    got = eng.whatif_maint([], [], [], [], [0, 1])
    assert got[0].shape == (0, 2) and got[1].tolist() == [0] and len(got[2]) == 0 and got[5] == 0
    got = eng.whatif_maint([[1]], [[0]], [[0]], [[w[0] + 1]], [])
    assert got[0].shape == (1, 0) and got[1].tolist() == [0] and got[5] == 0
    got = eng.whatif_maint_routes([], None, None, None, [0], [[0]])
    assert got[0].shape == (0, 1) and got[1].tolist() == [0]
    # one usable metric set to 0: the base SPF needs the exact-order kernel under link metric;
    # the hop-count form of that graph is served
    m = g.metric.copy()
    m[int(np.nonzero(g.edge_up != 0)[0][10])] = 0
    gz = dataclasses.replace(g, metric=m)
    eng.set_graph(gz)
    with pytest.raises(SpfError) as ei:
        eng.whatif_maint([[1]], None, [[1]], [[int(m[1]) + 1]], [0])
    assert ei.value.code == ENOTSUP
    ev = ([[v] for v in range(0, V, 9)], None, None, None)
    sources = list(range(0, V, 12))
    exp = oracle_maint(("zero-metric-hops",), gz, ev, sources, False)
    assert exp.changed.any()
    check_delta(exp, *eng.whatif_maint(*ev, sources, use_link_metric=False)[:5])
