"""The u16 / u32 / u64 distance tiers of the what-if and event sweeps vs the CPU oracle.

The library picks a distance width from the graph alone (V * w_max; tests/wide_cases.py has the
rules), and every other module of the suite stays at metrics of at most 64 on 120 to 1000
nodes: the u16 tier. Here the suite's own recipes run again with every metric multiplied by
one integer K. Scaling keeps every tie, next-hop set and changed set and multiplies every
finite distance by K, which is used twice: as an oracle-side fact that each test asserts
before it touches the engine (so a vacuous recipe cannot pass), and as a second, oracle-free
check on the engine. Every engine result is compared with the oracle on the scaled graph entry
for entry, and the tier that ran is read from the launch trace (openr_spf_last_kernels).

The oracle side is computed once per (recipe, K), shared by both parametrisations of the
module and never modified.
"""
import dataclasses
import os

import numpy as np
import pytest

import test_gpu_event_lfa as elfa_tests
import test_gpu_lfa as lfa_tests
import test_gpu_whatif_drain as drain_tests
import test_gpu_whatif_lfa as wlfa_tests
import test_gpu_whatif_maint as maint_tests
import test_gpu_whatif_metric as metric_tests
import test_gpu_whatif_restore as restore_tests
import test_gpu_whatif_sets as sets_tests
import wide_cases as W
from openr_amd import topology as T
from openr_amd.engine import SpfEngine
from openr_amd.spf_result import tight_in_edges
from oracle import Oracle
from test_gpu_parity import check_delta_rows, long_line_graph, random_graph, whatif_oracle
from test_gpu_routes_resolve import tables
from test_gpu_whatif_sets import check_delta, oracle_sets, small_graph

pytestmark = pytest.mark.gpu

U64_MAX = np.uint64(2**64 - 1)
K64 = W.k_wide(64)


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


# --- shared helpers -------------------------------------------------------------------------------
def typed(bfs_family, width):
    """The general-metric kernel of the parametrisation with its distance type, as the launch
    trace names it after the plain entry."""
    return f"{bfs_family[1]}_kernel<{width}>"


def finite_max(dist):
    d = np.asarray(dist)
    return int(d[d != U64_MAX].max())


def times(dist, K):
    """K x the finite entries, the unreachable ones kept."""
    d = np.asarray(dist, dtype=np.uint64)
    return np.where(d == U64_MAX, U64_MAX, d * np.uint64(K))


def assert_scaled(exp1, expK, K):
    """The oracle-side fact: the delta at K is the delta at 1 with its finite distances x K."""
    np.testing.assert_array_equal(expK.changed, exp1.changed)
    np.testing.assert_array_equal(expK.ptr, exp1.ptr)
    np.testing.assert_array_equal(expK.node, exp1.node)
    np.testing.assert_array_equal(expK.nh, exp1.nh)
    np.testing.assert_array_equal(expK.dist, times(exp1.dist, K))
    assert exp1.changed.any() and (exp1.dist != U64_MAX).any()


def assert_wide(exp):
    """Some finite distance of the delta needs more than 32 bits."""
    assert finite_max(exp.dist) > 2**32, finite_max(exp.dist)


def assert_u64_tier(g):
    assert g.num_nodes * W.w_max_of(g) >= W.U32_LIMIT and int(g.metric.max()) <= W.METRIC_MAX


def link_expect(key, g, links, sources, use_metric=True):
    """The single-link sweep's expectation: oracle_sets over singleton sets (unit (i, j) fails
    links[i] for sources[j]), cached under the key."""
    return oracle_sets(("tiers", key), g, [[int(l)] for l in links], sources, use_metric)


# --- a. link what-if, four tiers of one graph -----------------------------------------------------
TIER_KS = {"K1": 1, "K_LDS": W.K_LDS, "K_MID": W.K_MID, "K_WIDE": K64}
TIER_OF_K = {"K1": "u16", "K_LDS": "u32", "K_MID": "u32", "K_WIDE": "u64"}
TIER_SOURCES = list(range(0, 120, 6))
_TIER_GRAPHS = {}
_ENGINE_UNIT = {}


def tier_graph(kname):
    if kname not in _TIER_GRAPHS:
        g1 = random_graph(300, 120, 300, 64, p_ovl=0.05, p_down=0.05, p_par=0.1)
        assert g1.num_nodes == 120 and int(g1.metric.max()) == 64 and W.w_max_of(g1) == 64
        _TIER_GRAPHS[kname] = W.scaled(g1, TIER_KS[kname])
    return _TIER_GRAPHS[kname]


def tier_case(kname):
    """(graph, links, expectation) at a K, the oracle-side facts asserted."""
    K, g = TIER_KS[kname], tier_graph(kname)
    links = list(range(g.num_links))
    tier, lds_ok = W.tier_of(g)
    assert tier == TIER_OF_K[kname] and lds_ok == (kname in ("K1", "K_LDS"))
    assert W.w_max_of(g) == 64 * K
    exp1 = link_expect(("link", "K1"), tier_graph("K1"), links, TIER_SOURCES)
    exp = link_expect(("link", kname), g, links, TIER_SOURCES)
    assert_scaled(exp1, exp, K)
    assert (exp.dist == U64_MAX).any() and (exp.same_dist & (exp.dist != U64_MAX)).any()
    if kname == "K_WIDE":
        assert_u64_tier(g)
        assert_wide(exp)
    else:
        assert finite_max(exp.dist) < 2**32
    return g, links, exp


@pytest.fixture(params=["group", "group-lds", "group-cap1", "incr", "solve"])
def tier_mode(request, monkeypatch):
    """The what-if modes of test_gpu_parity.whatif_mode that differ in the distance type's code."""
    mode = request.param
    if mode == "group-lds":
        monkeypatch.setenv("OPENR_SPF_WHATIF_LDSG", "1")
    if mode == "group-cap1":
        monkeypatch.setenv("OPENR_SPF_WHATIF_CAP", "1")
    monkeypatch.setenv("OPENR_SPF_WHATIF", mode.split("-")[0])
    return mode


def engine_unit_delta(eng, bfs_family, mode, links):
    """The engine's own K = 1 delta in a mode (computed once per parametrisation and mode)."""
    key = (bfs_family, mode)
    if key not in _ENGINE_UNIT:
        eng.set_graph(tier_graph("K1"))
        _ENGINE_UNIT[key] = eng.whatif_delta(links, TIER_SOURCES, True)[:5]
    return _ENGINE_UNIT[key]


@pytest.mark.parametrize("kname", list(TIER_KS))
def test_link_whatif_tiers(eng, bfs_family, tier_mode, kname):
    K = TIER_KS[kname]
    g, links, exp = tier_case(kname)
    tier, lds_ok = W.tier_of(g)
    width = "u64" if tier == "u64" else "u32"  # the general-metric kernels have no u16 rows
    unit = engine_unit_delta(eng, bfs_family, tier_mode, links)
    eng.set_graph(g)
    changed, solved = eng.whatif(links, TIER_SOURCES, True)
    ks = eng.last_kernels()
    np.testing.assert_array_equal(changed, exp.changed)
    assert len(TIER_SOURCES) <= solved < changed.size + len(TIER_SOURCES)
    got = eng.whatif_delta(links, TIER_SOURCES, True)
    ks_delta = eng.last_kernels()
    check_delta(exp, *got[:5])
    # the tier that ran
    for trace in (ks, ks_delta):
        assert typed(bfs_family, width) in trace, trace  # the base solve
        assert not any(k.endswith("<u32>" if width == "u64" else "<u64>") for k in trace), trace
    if tier_mode.startswith("group"):
        want = f"whatif_group<{tier}{',lds' if tier_mode == 'group-lds' and lds_ok else ''}>"
        assert {k for k in ks if k.startswith("whatif_group")} == {want}, ks
        assert {k for k in ks_delta if k.startswith("whatif_group")} == {want}, ks_delta
    else:
        assert not any(k.startswith("whatif_group") for k in ks + ks_delta)
    if tier_mode == "incr":  # the counts-only call; the delta call re-solves
        assert f"whatif_incr<{width}>" in ks and not any(k.startswith("whatif_incr") for k in ks_delta), (ks, ks_delta)
    else:
        assert not any(k.startswith("whatif_incr") for k in ks + ks_delta)
    if tier_mode in ("group-cap1", "solve"):  # the re-solves beside the base solve
        assert ks.count(typed(bfs_family, width)) >= 2 and ks_delta.count(typed(bfs_family, width)) >= 2, (ks, ks_delta)
    # oracle-free: the engine's own K = 1 answer, scaled
    for a, b in zip(got[:3], unit[:3]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got[3], times(unit[3], K))
    np.testing.assert_array_equal(got[4], unit[4])


@pytest.mark.parametrize("kname", list(TIER_KS))
def test_link_whatif_hop_count_ignores_the_scale(eng, bfs_family, kname):
    """Hop count: every edge costs 1 whatever its metric, so the repair runs on u16 rows at every K."""
    g = tier_graph(kname)
    links, sources = list(range(0, g.num_links, 5)), TIER_SOURCES[:7]
    assert W.tier_of(g, unit_cost=True)[0] == "u16"
    eng.set_graph(g)
    c, p, n, d, h, _ = eng.whatif_delta(links, sources, False, nh_bytes=eng.nh_bytes + 5)
    ks = eng.last_kernels()
    np.testing.assert_array_equal(c, whatif_oracle(g, links, sources, False))
    check_delta_rows(g, links, sources, False, c, p, n, d, h)
    assert "whatif_group<u16>" in ks and not any("<u32>" in k or "<u64>" in k for k in ks), ks


# --- b. the u32 tier's top bit and the u32 / u64 threshold --------------------------------------
_LINE = {}


def line_case(K):
    """long_line_graph(5) x K: (graph, all-sources oracle runs, sweep sources, sweep expectation)."""
    if K not in _LINE:
        g1 = long_line_graph(5)
        assert g1.num_nodes == 220 and W.w_max_of(g1) == 297 and int(g1.metric.max()) == 297
        g = W.scaled(g1, K)
        o = Oracle(g)
        runs = [o.run_spf(s, True) for s in range(g.num_nodes)]
        for r in runs:
            r.dist.setflags(write=False)
            r.nh.setflags(write=False)
        _LINE[K] = (g, runs)
    g, runs = _LINE[K]
    links, sources = list(range(g.num_links)), list(range(0, g.num_nodes, 11))
    assert len(sources) == 20
    exp1 = link_expect(("line", 1), long_line_graph(5), links, sources)
    exp = link_expect(("line", K), g, links, sources)
    assert_scaled(exp1, exp, K)
    return g, runs, links, sources, exp


@pytest.mark.parametrize("K", [W.K_TOP, W.K_TOP + 1], ids=["K_TOP", "K_TOP+1"])
def test_top_bit_and_u64_threshold(eng, bfs_family, monkeypatch, K):
    g, runs, links, sources, exp = line_case(K)
    span = g.num_nodes * W.w_max_of(g)
    far = finite_max(runs[0].dist)
    assert far == W.LINE_FARTHEST * K
    if K == W.K_TOP:
        assert span == 4294928880 < W.U32_LIMIT and far == 3087629236 and 2**31 < far < 2**32
        assert 2**31 < finite_max(exp.dist) < 2**32
        width = "u32"
    else:
        assert span == 4294994220 >= W.U32_LIMIT
        width = "u64"
    # all-sources solves: the plain form and the tight-edge form (pathLinks in the reference's order)
    eng.set_graph(g)
    srcs = list(range(g.num_nodes))
    want_d, want_h = np.stack([r.dist for r in runs]), np.stack([r.nh for r in runs])
    dist, nh, _ = eng.solve(srcs, True)
    ks = eng.last_kernels()
    np.testing.assert_array_equal(dist, want_d)
    np.testing.assert_array_equal(nh, want_h)
    assert typed(bfs_family, width) in ks and bfs_family[1] + "_kernel" in ks, ks
    dist2, nh2, tight = eng.solve(srcs, True, want_tight=True)
    assert typed(bfs_family, width) in eng.last_kernels()
    np.testing.assert_array_equal(dist2, want_d)
    np.testing.assert_array_equal(nh2, want_h)
    for s in sources:
        pe = tight_in_edges(g, dist2[s], tight[s])
        for v in np.nonzero(runs[s].reachable())[0].tolist():
            assert pe.get(v, []) == runs[s].pl_edge[runs[s].pl_ptr[v]:runs[s].pl_ptr[v + 1]].tolist(), (s, v)
    # the link sweep: one dirty slot per wave (nearly every affected unit re-solved), then the default
    for cap in ("1", None):
        if cap:
            monkeypatch.setenv("OPENR_SPF_WHATIF_CAP", cap)
        else:
            monkeypatch.delenv("OPENR_SPF_WHATIF_CAP")
        changed, _ = eng.whatif(links, sources, True)
        ks = eng.last_kernels()
        np.testing.assert_array_equal(changed, exp.changed)
        assert f"whatif_group<{width}>" in ks and typed(bfs_family, width) in ks, ks
        assert not any(k.endswith("<u32>" if width == "u64" else "<u64>") for k in ks), ks
        if cap:
            assert ks.count(typed(bfs_family, width)) >= 2, ks  # the seeded re-solves
        check_delta(exp, *eng.whatif_delta(links, sources, True)[:5])


# --- c. the u16 / u32 threshold -----------------------------------------------------------------
_PLAIN_LINES = {}


def plain_line(V, w):
    if (V, w) not in _PLAIN_LINES:
        names = [f"p{i:04d}" for i in range(V)]
        links = np.array([(i, i + 1) for i in range(V - 1)])
        m = np.full(V - 1, w, dtype=np.uint64)
        _PLAIN_LINES[(V, w)] = T.csr_from_links(names, links, m, m, np.zeros(V, np.uint8), np.ones(V - 1, np.uint8))
    return _PLAIN_LINES[(V, w)]


@pytest.mark.parametrize("V,w,tier", [(254, 258, "u16"), (255, 257, "u32")])
def test_u16_u32_threshold(eng, bfs_family, V, w, tier):
    g = plain_line(V, w)
    assert g.num_nodes == V and g.num_links == V - 1 and W.w_max_of(g) == w
    assert (V * w < W.U16_LIMIT) == (tier == "u16") and V * w == {254: 65532, 255: 65535}[V]
    assert W.tier_of(g)[0] == tier
    links, sources = list(range(g.num_links)), list(range(0, V, 13))
    assert len(sources) == 20
    exp = link_expect(("plain-line", V, w), g, links, sources)
    o = Oracle(g)
    assert finite_max(o.run_spf(0, True).dist) == (V - 1) * w < 0xFFFF  # the longest base distance fits u16
    assert exp.changed.any() and (exp.dist == U64_MAX).all()  # every link is a bridge: a failure only cuts nodes off
    eng.set_graph(g)
    dist, nh, _ = eng.solve(sources, True)
    for i, s in enumerate(sources):
        r = o.run_spf(s, True)
        np.testing.assert_array_equal(dist[i], r.dist)
        np.testing.assert_array_equal(nh[i], r.nh)
    changed, _ = eng.whatif(links, sources, True)
    ks = eng.last_kernels()
    np.testing.assert_array_equal(changed, exp.changed)
    assert {k for k in ks if k.startswith("whatif_group")} == {f"whatif_group<{tier}>"}, ks
    check_delta(exp, *eng.whatif_delta(links, sources, True)[:5])
    assert f"whatif_group<{tier}>" in eng.last_kernels()


# --- d. the set sweep and the event sweeps at K_WIDE ----------------------------------------------
def test_set_sweep_wide(eng, bfs_family):
    g1, sets, sources = sets_tests.srlg_case(0)
    sources = sources[:20]
    g = W.scaled(g1, K64)
    assert_u64_tier(g)
    exp1 = oracle_sets(("tiers", "srlg", 1), g1, sets, sources)
    exp = oracle_sets(("tiers", "srlg", K64), g, sets, sources)
    assert_scaled(exp1, exp, K64)
    assert_wide(exp)
    eng.set_graph(g)
    changed, solved = eng.whatif_sets(sets, sources, True)
    ks = eng.last_kernels()
    np.testing.assert_array_equal(changed, exp.changed)
    assert ks.count(typed(bfs_family, "u64")) >= 2 and not any(k.endswith("<u32>") for k in ks), ks
    got = eng.whatif_sets_delta(sets, sources, True)
    check_delta(exp, *got[:5])
    assert got[5] == solved and typed(bfs_family, "u64") in eng.last_kernels()


def event_base_is_wide(eng, bfs_family):
    ks = eng.last_kernels()
    assert typed(bfs_family, "u64") in ks and not any(k.endswith("<u32>") for k in ks), ks
    return ks


def test_drain_sweep_wide(eng, bfs_family):
    g1, node_sets, link_sets, sources = drain_tests.multi_case(0)
    node_sets, link_sets, sources = node_sets[:20], link_sets[:20], sources[:10]
    g = W.scaled(g1, K64)
    assert_u64_tier(g)
    exp1 = drain_tests.oracle_drain(("tiers-multi", 1), g1, node_sets, link_sets, sources)
    exp = drain_tests.oracle_drain(("tiers-multi", K64), g, node_sets, link_sets, sources)
    assert_scaled(exp1, exp, K64)
    assert_wide(exp)
    eng.set_graph(g)
    got = eng.whatif_drain(node_sets, sources, link_sets=link_sets)
    ks = event_base_is_wide(eng, bfs_family)
    assert "drain_filter" in ks and "drain_repair" in ks, ks
    check_delta(exp, *got[:5])


def test_metric_sweep_wide(eng, bfs_family):
    g1, edge_sets, metric_sets, sources = metric_tests.row_case(0)
    K = W.k_wide(W.m_max_of(g1, metric_sets))
    assert K == W.k_wide(69)  # the recipe raises every metric by 5
    edge_sets, metric_sets, sources = edge_sets[:20], metric_sets[:20], sources[:10]
    g, metric_k = W.scaled(g1, K), W.scale_metric_sets(metric_sets, K)
    assert_u64_tier(g)
    assert max(max(ms) for ms in metric_k if ms) <= W.METRIC_MAX
    exp1 = metric_tests.oracle_metric(("tiers-row", 1), g1, edge_sets, metric_sets, sources)
    exp = metric_tests.oracle_metric(("tiers-row", K), g, edge_sets, metric_k, sources)
    assert_scaled(exp1, exp, K)
    assert_wide(exp)
    eng.set_graph(g)
    got = eng.whatif_metric(edge_sets, metric_k, sources)
    ks = event_base_is_wide(eng, bfs_family)
    assert "metric_filter" in ks and "metric_repair" in ks, ks
    check_delta(exp, *got[:5])


def restore_wide_case():
    g1, ev1 = restore_tests.mixed_case(0)
    K = W.k_wide(W.m_max_of(g1, ev1.metrics))
    ev1 = ev1.take(range(20))
    return g1, ev1, K, W.scaled(g1, K), W.scale_events(ev1, K)


def test_restore_sweep_wide(eng, bfs_family):
    g1, ev1, K, g, ev = restore_wide_case()
    sources = restore_tests.SOURCES[:10]
    assert_u64_tier(g)
    exp1 = restore_tests.oracle_restore(("tiers-mixed", 1), g1, ev1, sources)
    exp = restore_tests.oracle_restore(("tiers-mixed", K), g, ev, sources)
    assert_scaled(exp1, exp, K)
    np.testing.assert_array_equal(exp.flagged, exp1.flagged)
    assert_wide(exp)
    assert exp.new_reach.any()
    eng.set_graph(g)
    got = eng.whatif_restore(*ev.args(), sources)
    ks = event_base_is_wide(eng, bfs_family)
    assert "restore_filter" in ks and "restore_repair" in ks, ks
    check_delta(exp, *got[:5])
    restore_tests.check_solved(exp, got[5], len(sources))


def maint_wide_case():
    g1, ev1, sources = maint_tests.mixed_case(0)
    K = W.k_wide(W.m_max_of(g1, ev1[3]))
    assert K == W.k_wide(104) == 20648881  # metrics up to 64, raised by 40
    ev1, sources = maint_tests.head_of(ev1, 20), sources[:10]
    return g1, ev1, sources, K, W.scaled(g1, K), W.scale_events(ev1, K)


@pytest.mark.parametrize("slots", [None, "16"], ids=["default-slots", "16-slots"])
def test_maint_sweep_wide(bfs_family, monkeypatch, slots):
    """With 16 slots the overflow re-run (one slot per node) runs wide too."""
    if slots:
        monkeypatch.setenv("OPENR_SPF_MAINT_SLOTS", slots)
    g1, ev1, sources, K, g, ev = maint_wide_case()
    assert_u64_tier(g)
    exp1 = maint_tests.oracle_maint(("tiers-mixed", 1), g1, ev1, sources)
    exp = maint_tests.oracle_maint(("tiers-mixed", K), g, ev, sources)
    assert_scaled(exp1, exp, K)
    assert_wide(exp)
    assert int((exp.changed > 16).sum()) > 0 and int(((exp.changed > 0) & (exp.changed < 8)).sum()) > 0
    e = SpfEngine()
    try:
        e.set_graph(g)
        got = e.whatif_maint(*ev, sources)
        ks = event_base_is_wide(e, bfs_family)
    finally:
        e.close()
    check_delta(exp, *got[:5])
    assert "maint_filter" in ks and "maint_repair" in ks, ks
    assert ("maint_repair<overflow>" in ks) == bool(slots), ks


# --- e. routes and loop-free alternates at K_WIDE -----------------------------------------------
def test_maint_routes_wide(eng, bfs_family):
    g1, ev1, sources, K, g, ev = maint_wide_case()
    _, dense = tables(0)
    want1 = maint_tests.expected_routes(("tiers-mixed", 1), g1, ev1, sources, dense)
    want = maint_tests.expected_routes(("tiers-mixed", K), g, ev, sources, dense)
    for k in (0, 1, 2, 4, 5):
        np.testing.assert_array_equal(want[k], want1[k])
    np.testing.assert_array_equal(want[3], times(want1[3], K))
    assert want[0].any() and finite_max(want[3]) > 2**32
    eng.set_graph(g)
    changed, ptr, group, metric, nh, n_best, solved = eng.whatif_maint_routes(*ev, sources, dense)
    event_base_is_wide(eng, bfs_family)
    np.testing.assert_array_equal(changed, want[0])
    np.testing.assert_array_equal(ptr, want[1])
    np.testing.assert_array_equal(group, want[2])
    np.testing.assert_array_equal(metric, want[3])
    np.testing.assert_array_equal(nh[:, : want[4].shape[1]], want[4])
    assert not nh[:, want[4].shape[1]:].any()
    np.testing.assert_array_equal(n_best, want[5])
    assert finite_max(metric) > 2**32 and solved >= len(sources)


def test_lfa_routes_wide(eng, bfs_family):
    g1 = small_graph(0)
    g = W.scaled(g1, K64)
    assert_u64_tier(g)
    _, dense = tables(0)
    exp1 = lfa_tests.expect((("tiers-small", 1), "dense"), g1, lfa_tests.SOURCES, dense)
    exp = lfa_tests.expect((("tiers-small", K64), "dense"), g, lfa_tests.SOURCES, dense)
    for name in ("nh", "alt", "n_alt", "ptr", "nbr"):
        np.testing.assert_array_equal(getattr(exp, name), getattr(exp1, name))
    np.testing.assert_array_equal(exp.metric, times(exp1.metric, K64))
    np.testing.assert_array_equal(exp.alt_metric, times(exp1.alt_metric, K64))
    assert finite_max(exp.metric) > 2**32 and finite_max(exp.alt_metric) > 2**32
    assert exp.facts["lfa_only"] > 0 and exp.facts["no_alt"] > 0
    eng.set_graph(g)
    got = eng.lfa_routes(lfa_tests.SOURCES, dense, True)
    ks = event_base_is_wide(eng, bfs_family)
    assert "lfa_rows" in ks and "lfa_reduce_emit" in ks, ks
    lfa_tests.check(exp, got)
    assert finite_max(got[0]) > 2**32 and finite_max(got[6]) > 2**32


def test_whatif_lfa_wide(eng, bfs_family):
    g1 = small_graph(0)
    g = W.scaled(g1, K64)
    sets = T.node_failure_sets(g1, range(0, 120, 6))
    assert len(sets) == 20 and sets == T.node_failure_sets(g, range(0, 120, 6))
    _, dense = tables(0)
    exp1 = wlfa_tests.oracle_whatif_lfa((("tiers-node", 1), "dense"), g1, sets, lfa_tests.SOURCES, dense)
    exp = wlfa_tests.oracle_whatif_lfa((("tiers-node", K64), "dense"), g, sets, lfa_tests.SOURCES, dense)
    for name in ("changed", "unprotected", "lost_backup", "ptr", "group", "nh", "alt"):
        np.testing.assert_array_equal(getattr(exp, name), getattr(exp1, name))
    np.testing.assert_array_equal(exp.metric, times(exp1.metric, K64))
    assert finite_max(exp.metric) > 2**32
    assert exp.facts["alt_only"] > 0 and exp.facts["route"] > 0 and exp.facts["lost"] > 0, exp.facts
    eng.set_graph(g)
    got = eng.whatif_lfa(sets, lfa_tests.SOURCES, dense, True)
    ks = event_base_is_wide(eng, bfs_family)
    assert "wlfa_mark" in ks and "wlfa_emit" in ks, ks
    wlfa_tests.check(exp, got)
    assert finite_max(got[3]) > 2**32


def test_restore_event_lfa_wide(eng, bfs_family):
    """The restore family's mixed recipe (undrains, link-ups and lowered metrics in one event):
    its metric lists are scaled with the graph."""
    g1, ev1 = elfa_tests.CASES["mixed"](0)
    K = W.k_wide(W.m_max_of(g1, ev1.metrics))
    assert K == W.k_wide(114)  # metrics up to 64, 15 rows soft-drained by 50
    ev1 = ev1.take(range(20))
    g, ev = W.scaled(g1, K), W.scale_events(ev1, K)
    assert_u64_tier(g)
    _, dense = tables(0)
    exp1 = elfa_tests.oracle_event_lfa(("tiers-restore-mixed", 1), g1, ev1, lfa_tests.SOURCES, dense)
    exp = elfa_tests.oracle_event_lfa(("tiers-restore-mixed", K), g, ev, lfa_tests.SOURCES, dense)
    for name in ("changed", "unprotected", "lost_backup", "ptr", "group", "nh", "alt"):
        np.testing.assert_array_equal(getattr(exp, name), getattr(exp1, name))
    np.testing.assert_array_equal(exp.metric, times(exp1.metric, K))
    assert finite_max(exp.metric) > 2**32
    assert exp.facts["sum"] > 0 and exp.facts["alt_only"] > 0 and exp.facts["tome_moves"] > 0, exp.facts
    eng.set_graph(g)
    got = ev.lfa(eng, lfa_tests.SOURCES, dense, True)
    ks = event_base_is_wide(eng, bfs_family)
    assert "elfa_mark" in ks and "elfa_emit" in ks and "restore_repair" in ks, ks
    wlfa_tests.check(exp, got)
    assert finite_max(got[3]) > 2**32


# --- f. patches that move w_max across both thresholds, on one engine ---------------------------
HEAVY = W.METRIC_MAX
_HEAVY = {}


def heavy_case():
    """tier_graph("K1") with one bridge link at metric 2^31 - 1 in both directions, down: (graph,
    link, its two directed edges, sources). The bridge is a leaf's only link, and the leaf is
    among the sources: every path to it and every path from it crosses the heavy link."""
    if not _HEAVY:
        g1 = tier_graph("K1")
        o = Oracle(g1)
        base = o.run_spf(0, True)
        link, cut = next((l, c) for l in range(g1.num_links)
                         for c in [np.nonzero((o.run_spf(0, True, [l]).dist == U64_MAX) & (base.dist != U64_MAX))[0]]
                         if len(c))
        edges = [int(e) for e in np.nonzero(g1.link_id == link)[0]]
        assert len(edges) == 2 and all(g1.edge_up[e] for e in edges) and len(cut) == 1
        leaf = int(cut[0])
        assert len(g1.distinct_neighbors(leaf)) == 1 and not g1.node_overloaded[g1.distinct_neighbors(leaf)[0]]
        sources = sorted(set(range(0, 120, 12)) | {leaf})
        _HEAVY["case"] = (g1.patched(edges, [HEAVY, HEAVY], [link], [0], [], []), link, edges, sources, leaf)
    return _HEAVY["case"]


def sweep_and_solve(e, bfs_family, key, tier, sources):
    """The link sweep and a solve on the engine's current graph against the oracle on e.g (the
    host copy the patches were applied to), and the tier both ran at."""
    g = e.g
    assert W.tier_of(g)[0] == tier
    width = "u64" if tier == "u64" else "u32"
    links = list(range(g.num_links))
    exp = link_expect(("patch", key), g, links, sources)
    assert exp.changed.any()
    got = e.whatif_delta(links, sources, True)
    ks = e.last_kernels()
    check_delta(exp, *got[:5])
    assert {k for k in ks if k.startswith("whatif_group")} == {f"whatif_group<{tier}>"}, ks
    assert typed(bfs_family, width) in ks and not any(k.endswith("<u32>" if width == "u64" else "<u64>") for k in ks), ks
    changed, _ = e.whatif(links, sources, True)
    np.testing.assert_array_equal(changed, exp.changed)
    o = Oracle(g)
    dist, nh, _ = e.solve(sources, True)
    ks = e.last_kernels()
    assert typed(bfs_family, width) in ks, ks
    for i, s in enumerate(sources):
        r = o.run_spf(s, True)
        np.testing.assert_array_equal(dist[i], r.dist)
        np.testing.assert_array_equal(nh[i], r.nh)
    return exp


def refresh_and_check(e, srcs, rows):
    """Rows solved before the patch, refreshed: a fresh solve's rows (sweep_and_solve holds the
    fresh solve against the oracle)."""
    dist, nh, tight = rows
    e.refresh(srcs, dist, nh, tight)
    fd, fn, ft = e.solve(srcs, True, want_tight=True)
    np.testing.assert_array_equal(dist, fd)
    np.testing.assert_array_equal(nh, fn)
    np.testing.assert_array_equal(tight, ft)


def test_patches_move_the_tier(bfs_family):
    """The multiset of usable metrics follows a link through down -> up -> cheaper -> down -> up:
    the what-if launch and the general-metric kernels pick their width from it after every
    patch, and rows of the narrower graph refresh to the wider one."""
    g, link, edges, sources, leaf = heavy_case()
    assert W.tier_of(g) == ("u16", True) and int(g.metric.max()) == HEAVY
    srcs = list(range(g.num_nodes))
    e = SpfEngine()
    try:
        e.set_graph(g)
        rows = e.solve(srcs, True, want_tight=True)
        # 1. the heavy link is down: its metric does not count
        first = sweep_and_solve(e, bfs_family, "down", "u16", sources)
        # ... a restore event brings it up out of the u16-tier base. One link of 2^31 - 1 cannot
        # put a shortest path above 2^32 (a path crosses it once, the rest is below 120 * 64):
        # the distances behind the bridge have bit 31 set
        ev = restore_tests.events_of(link_sets=[[link]])
        exp = restore_tests.oracle_restore(("tiers-heavy-up",), g, ev, sources)
        assert 2**31 <= finite_max(exp.dist) < 2**31 + 120 * 64
        j = sources.index(leaf)  # the leaf's base row reaches nothing; the event row reaches the graph
        assert exp.changed[0, j] >= 100 and int(exp.new_reach.sum()) >= 100 + len(sources) - 1
        got = e.whatif_restore(*ev.args(), sources)
        ks = e.last_kernels()
        assert "restore_repair" in ks and typed(bfs_family, "u32") in ks, ks
        check_delta(exp, *got[:5])
        # 2. up: V * w_max >= 2^32
        e.patch(links=[link], link_up=[1])
        assert W.w_max_of(e.g) == HEAVY
        refresh_and_check(e, srcs, rows)
        up = sweep_and_solve(e, bfs_family, "up-heavy", "u64", sources)
        assert finite_max(up.dist) >= 2**31
        # 3. both directions at 600: 120 * 600 = 72 000
        e.patch(edges=edges, metrics=[600, 600])
        assert W.w_max_of(e.g) == 600
        refresh_and_check(e, srcs, rows)
        at600 = sweep_and_solve(e, bfs_family, "up-600", "u32", sources)
        # 4. down again
        e.patch(links=[link], link_up=[0])
        assert W.w_max_of(e.g) == 64
        refresh_and_check(e, srcs, rows)
        again = sweep_and_solve(e, bfs_family, "down-600", "u16", sources)
        for a, b in zip(dataclasses.astuple(first), dataclasses.astuple(again)):
            np.testing.assert_array_equal(a, b)
        # 5. up again: the link's 600 counts again
        e.patch(links=[link], link_up=[1])
        assert W.w_max_of(e.g) == 600
        refresh_and_check(e, srcs, rows)
        again = sweep_and_solve(e, bfs_family, "up-600", "u32", sources)
        assert again is at600
    finally:
        e.close()
