"""Route-level results on the GPU (openr_spf_routes*, openr_spf_whatif_routes*) vs the CPU oracle.

A route belongs to a prefix group (the nodes that advertise the prefix): its metric is the
minimum distance over the members, its next hops the union over the members at that
minimum (getMinCostNodes + the shortest-path half of getNextHopsWithMetric). Expected
values are oracle runs of runSpf(source, useLinkMetric, set) reduced in numpy by that
rule; the what-if expectation is the diff of the reduced failure run against the reduced
no-failure run. The module runs on both what-if re-solve routes, as
test_gpu_whatif_sets.py does.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from openr_amd import topology as T
from openr_amd.engine import E2BIG, EINVAL, ENOTSUP, USE_LINK_METRIC, SpfEngine, SpfError, SpfGroups, _p
from oracle import Oracle
from test_gpu_parity import random_graph

pytestmark = pytest.mark.gpu

U64_MAX = np.uint64(2**64 - 1)
SOURCES = list(range(0, 120, 8))


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


# --- oracle side: computed once per key, shared by both parametrisations, never modified
_GRAPHS = {}
_ROWS = {}
_EXPECT = {}


def small_graph(seed):
    if seed not in _GRAPHS:
        g = random_graph(400 + seed, 120, 300, {0: 64, 1: 1, 2: 7}[seed], p_ovl=0.05, p_down=0.05, p_par=0.1)
        assert g.num_nodes == 120 and g.num_links == 330 and g.nh_bytes() == 2
        _GRAPHS[seed] = g
    return _GRAPHS[seed]


def tables(seed):
    """(sparse, dense) group tables of a seed: 40 random groups of 2-6 nodes, the empty group
    and the all-nodes group; dense = the 120 loopbacks first, then those 42."""
    rng = np.random.default_rng(7 + seed)
    groups = []
    for _ in range(40):
        k = int(rng.integers(2, 7))
        groups.append(sorted(int(v) for v in rng.choice(120, k, replace=False)))
    sparse = groups + [[], list(range(120))]
    dense = [[v] for v in range(120)] + sparse
    assert len(sparse) == 42 and len(dense) == 162
    assert sum(len(x) for x in dense) == {0: 395, 1: 406, 2: 398}[seed]
    return sparse, dense


def reduce_routes(dist, nh, groups):
    """The route rule on rows dist [R, V] / nh [R, V, nb]: (metric [R, G], nh [R, G, nb], n_best [R, G])."""
    R, nb, G = dist.shape[0], nh.shape[2], len(groups)
    metric = np.full((R, G), U64_MAX, dtype=np.uint64)
    rnh = np.zeros((R, G, nb), dtype=np.uint8)
    n_best = np.zeros((R, G), dtype=np.uint32)
    for k, grp in enumerate(groups):
        if not grp:
            continue
        sub = dist[:, grp]
        mn = sub.min(axis=1)
        at = (sub == mn[:, None]) & (mn != U64_MAX)[:, None]
        metric[:, k] = mn
        n_best[:, k] = at.sum(axis=1)
        rnh[:, k] = np.bitwise_or.reduce(np.where(at[:, :, None], nh[:, grp], np.uint8(0)), axis=1)
    return metric, rnh, n_best


def oracle_rows(key, g, sets, sources, use_metric):
    """(base dist [S, V], base nh, failure dist [n_sets * S, V], failure nh) of every unit."""
    k = (key, bool(use_metric))
    if k not in _ROWS:
        o = Oracle(g)
        base = [o.run_spf(int(s), use_metric) for s in sources]
        runs = [o.run_spf(int(s), use_metric, [int(l) for l in st]) if st else base[j]
                for st in sets for j, s in enumerate(sources)]
        rows = (np.stack([r.dist for r in base]), np.stack([r.nh for r in base]),
                np.stack([r.dist for r in runs]), np.stack([r.nh for r in runs]))
        for a in rows:
            a.setflags(write=False)
        _ROWS[k] = rows
    return _ROWS[k]


@dataclasses.dataclass(frozen=True)
class Expect:
    changed: np.ndarray  # [n_sets, n_sources] routes changed
    ptr: np.ndarray
    group: np.ndarray  # every unit's changed groups ascending, concatenated
    metric: np.ndarray
    nh: np.ndarray
    n_best: np.ndarray
    facts: dict


def oracle_routes(key, g, sets, sources, groups, use_metric=True):
    k = (key, bool(use_metric))
    if k in _EXPECT:
        return _EXPECT[k]
    bd, bh, fd, fh = oracle_rows(key[0], g, sets, sources, use_metric)
    S, G = len(sources), len(groups)
    bm, bnh, bnb = reduce_routes(bd, bh, groups)
    fm, fnh, fnb = reduce_routes(fd, fh, groups)
    bm_u, bnh_u, bnb_u = (np.tile(x, (len(sets),) + (1,) * (x.ndim - 1)) for x in (bm, bnh, bnb))
    ch = (fm != bm_u) | np.any(fnh != bnh_u, axis=2)  # [units, G]
    node_ch = (fd != np.tile(bd, (len(sets), 1))) | np.any(fh != np.tile(bh, (len(sets), 1, 1)), axis=2)
    member_ch = np.zeros_like(ch)
    for q, grp in enumerate(groups):
        if grp:
            member_ch[:, q] = node_ch[:, grp].any(axis=1)
    assert not (ch & ~member_ch).any()  # a route changes only through its members
    counts = ch.sum(axis=1).astype(np.uint32)
    ptr = np.zeros(ch.shape[0] + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(counts, dtype=np.uint64)
    uu, kk = np.nonzero(ch)  # row-major: units ascending, groups ascending inside a unit
    # the all-nodes group holds every changed node and the source (metric 0, no next hop, never
    # changes): it is left out of the changed-member-but-unchanged-route count
    partial = np.array([len(grp) < g.num_nodes for grp in groups])
    facts = {
        "sum": int(counts.sum()),
        "max_per_unit": int(counts.max()) if counts.size else 0,
        "lost": int((ch & (fm == U64_MAX)).sum()),
        "same_metric": int((ch & (fm == bm_u)).sum()),
        "nbest_only": int((~ch & (fnb != bnb_u)).sum()),
        "member_not_route": int((member_ch & ~ch)[:, partial].sum()),
        "base_multi": int((bnb > 1).sum()),
        "nodes_not_routes": int((node_ch.any(axis=1) & (counts == 0)).sum()),
    }
    e = Expect(counts.reshape(len(sets), S), ptr, kk.astype(np.uint32), fm[uu, kk], fnh[uu, kk], fnb[uu, kk], facts)
    for a in (e.changed, e.ptr, e.group, e.metric, e.nh, e.n_best):
        a.setflags(write=False)
    assert G == ch.shape[1]
    _EXPECT[k] = e
    return e


def check_routes(exp, changed, ptr, group, metric, nh, n_best):
    """changed_routes and the host CSR entry for entry: groups ascending, the new route."""
    np.testing.assert_array_equal(changed, exp.changed)
    np.testing.assert_array_equal(ptr, exp.ptr)
    np.testing.assert_array_equal(group, exp.group)
    np.testing.assert_array_equal(metric, exp.metric)
    want = np.zeros((exp.nh.shape[0], nh.shape[1]), dtype=np.uint8)
    want[:, : exp.nh.shape[1]] = exp.nh
    np.testing.assert_array_equal(nh, want)
    np.testing.assert_array_equal(n_best, exp.n_best)


# --- 1. routes of every source ---------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("use_metric", [True, False], ids=["metric", "hops"])
def test_routes_match_oracle(eng, seed, use_metric):
    g = small_graph(seed)
    _, dense = tables(seed)
    o = Oracle(g)
    dist, nh = o.all_sources(list(range(120)), use_metric)
    wm, wnh, wnb = reduce_routes(dist, nh, dense)
    assert (wm == U64_MAX).any() and (wnb > 1).any() and (wm[:, :120].diagonal() == 0).all()
    eng.set_graph(g)
    metric, rnh, n_best = eng.routes(list(range(120)), dense, use_metric)
    assert "routes_reduce" in eng.last_kernels()
    np.testing.assert_array_equal(metric, wm)
    np.testing.assert_array_equal(rnh, wnh)
    np.testing.assert_array_equal(n_best, wnb)
    assert not rnh[np.arange(120), np.arange(120)].any()  # a group holding the source: metric 0, no next hop
    m2, h2, b2 = eng.routes(list(range(120)), dense, use_metric, want_nh=False, want_n_best=False)
    assert h2 is None and b2 is None
    np.testing.assert_array_equal(m2, wm)
    m3, h3, b3 = eng.routes(list(range(120)), dense, use_metric, nh_bytes=eng.nh_bytes + 3)
    np.testing.assert_array_equal(m3, wm)
    np.testing.assert_array_equal(h3[:, :, :2], wnh)
    assert not h3[:, :, 2:].any()
    np.testing.assert_array_equal(b3, wnb)


# --- 2. the sweep, host form -----------------------------------------------------------
DENSE_FACTS = {
    "sum": (11907, 11478, 11644), "max_per_unit": (159, 158, 159), "lost": (4206, 4146, 4196),
    "same_metric": (238, 4848, 1811), "nbest_only": (17, 446, 249), "member_not_route": (5740, 5702, 5702),
    "base_multi": (8, 245, 85),
}
DENSE_HOPS_SUM = (11684, 11478, 11838)
SPARSE_FACTS = {"sum": (2452, 2487, 2416), "max_per_unit": (40, 40, 40), "nodes_not_routes": (1175, 1195, 1234)}


def sweep_case(seed, table, use_metric):
    g = small_graph(seed)
    sets = T.node_failure_sets(g)
    sparse, dense = tables(seed)
    groups = dense if table == "dense" else sparse
    exp = oracle_routes((("node", seed), table), g, sets, SOURCES, groups, use_metric)
    assert exp.changed.size == 1800
    # what the inputs exercise, on the oracle's side
    if table == "dense" and use_metric:
        for name, want in DENSE_FACTS.items():
            assert exp.facts[name] == want[seed], (name, exp.facts)
    elif table == "dense":
        assert exp.facts["sum"] == DENSE_HOPS_SUM[seed], exp.facts
    elif use_metric:
        for name, want in SPARSE_FACTS.items():
            assert exp.facts[name] == want[seed], (name, exp.facts)
    return g, sets, groups, exp


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("table", ["dense", "sparse"])
@pytest.mark.parametrize("use_metric", [True, False], ids=["metric", "hops"])
def test_whatif_routes_match_oracle(eng, bfs_family, seed, table, use_metric):
    g, sets, groups, exp = sweep_case(seed, table, use_metric)
    eng.set_graph(g)
    got = eng.whatif_routes(sets, SOURCES, groups, use_metric)
    ks = eng.last_kernels()
    assert "whatif_routes_count" in ks and "whatif_routes_emit" in ks, ks
    check_routes(exp, *got[:6])
    _, solved = eng.whatif_sets(sets, SOURCES, use_metric)
    assert got[6] == solved
    # a wider nh_bytes: zero past the graph's width
    wide = eng.whatif_routes(sets[:30], SOURCES, groups, use_metric, nh_bytes=eng.nh_bytes + 5)
    n30 = int(exp.ptr[30 * len(SOURCES)])
    assert wide[4].shape == (n30, eng.nh_bytes + 5) and not wide[4][:, 2:].any()
    np.testing.assert_array_equal(wide[4][:, :2], exp.nh[:n30])
    np.testing.assert_array_equal(wide[2], exp.group[:n30])


def test_singletons_and_empty_set(eng, bfs_family):
    """Singleton link sets are single-link failures; a set listing its link twice is the same
    set; an empty set changes no route."""
    g = small_graph(0)
    _, dense = tables(0)
    links = [l for l in range(g.num_links) if g.edge_up[np.nonzero(g.link_id == l)[0][0]]][:40]
    sets = [[l] for l in links] + [[]]
    exp = oracle_routes((("single", 0), "dense"), g, sets, SOURCES, dense, True)
    assert exp.facts["sum"] > 0 and not exp.changed[-1].any()
    eng.set_graph(g)
    got = eng.whatif_routes(sets, SOURCES, dense, True)
    check_routes(exp, *got[:6])
    twice = eng.whatif_routes([[l, l] for l in links] + [[]], SOURCES, dense, True)
    for a, b in zip(got[:6], twice[:6]):
        np.testing.assert_array_equal(a, b)
    _, solved = eng.whatif_sets(sets, SOURCES, True)
    assert got[6] == solved


def test_two_device_slots_and_split_calls(eng, bfs_family):
    """The host forms split sources (routes) and sets (whatif_routes) in blocks across the
    context's devices: a context over the same ordinal twice (the suite's pattern for the
    split on a 1-GPU box) gives the oracle's answer, and a caller-side split of the sets in
    two halves concatenates to the whole call."""
    g, sets, groups, exp = sweep_case(1, "dense", True)
    two = SpfEngine([0, 0])
    try:
        two.set_graph(g)
        got = two.whatif_routes(sets, SOURCES, groups, True)
        check_routes(exp, *got[:6])
        eng.set_graph(g)
        for a, b in zip(two.routes(list(range(120)), groups, True), eng.routes(list(range(120)), groups, True)):
            np.testing.assert_array_equal(a, b)
    finally:
        two.close()
    h = len(sets) // 2 + 7
    lo, hi = eng.whatif_routes(sets[:h], SOURCES, groups, True), eng.whatif_routes(sets[h:], SOURCES, groups, True)
    np.testing.assert_array_equal(np.concatenate([lo[0], hi[0]]), exp.changed)
    np.testing.assert_array_equal(np.concatenate([lo[1], hi[1][1:] + lo[1][-1]]), exp.ptr)
    for k, want in ((2, exp.group), (3, exp.metric), (5, exp.n_best)):
        np.testing.assert_array_equal(np.concatenate([lo[k], hi[k]]), want)


# --- 3. device form and cap -------------------------------------------------------------
def test_device_form_and_cap(eng, bfs_family):
    import torch

    g, sets, groups, exp = sweep_case(2, "dense", True)
    eng.set_graph(g)
    nb, units, total = eng.nh_bytes, exp.changed.size, exp.facts["sum"]
    dev = torch.device("cuda", 0)

    def csr(lists):
        p = np.zeros(len(lists) + 1, dtype=np.int32)
        p[1:] = np.cumsum([len(x) for x in lists])
        return torch.from_numpy(p).to(dev), torch.from_numpy(np.concatenate(
            [np.asarray(x, dtype=np.int32) for x in lists])).to(dev)

    d_sp, d_sl = csr(sets)
    d_gp, d_gn = csr(groups)
    d_s = torch.from_numpy(np.asarray(SOURCES, dtype=np.int32)).to(dev)
    d_c = torch.full((len(sets), len(SOURCES)), -1, dtype=torch.int32, device=dev)
    d_ptr = torch.zeros(units + 1, dtype=torch.int64, device=dev)
    d_group = torch.zeros(total, dtype=torch.int32, device=dev)
    d_metric = torch.zeros(total, dtype=torch.int64, device=dev)
    d_nh = torch.zeros((total, nb), dtype=torch.uint8, device=dev)
    d_nb = torch.zeros(total, dtype=torch.int32, device=dev)
    head = (d_sp.data_ptr(), d_sl.data_ptr(), len(sets), d_sl.numel(), d_s.data_ptr(), len(SOURCES), d_gp.data_ptr(),
            d_gn.data_ptr(), len(groups), d_gn.numel(), d_c.data_ptr(), d_ptr.data_ptr())
    bufs = (d_group.data_ptr(), d_metric.data_ptr(), d_nh.data_ptr(), d_nb.data_ptr())
    _, solved = eng.whatif_sets(sets, SOURCES, True)

    def counts_ok():
        np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint32), exp.changed)
        np.testing.assert_array_equal(d_ptr.cpu().numpy().view(np.uint64), exp.ptr)

    got, s_dev = eng.whatif_routes_device(*head, *bufs, total, nb)
    assert got == total and s_dev == solved
    counts_ok()
    pg = d_group.cpu().numpy().view(np.uint32)
    pm = d_metric.cpu().numpy().view(np.uint64)
    ph, pb = d_nh.cpu().numpy(), d_nb.cpu().numpy().view(np.uint32)
    for u in range(units):  # the device form keeps the kernel's order: sort each unit by group
        a, e = int(exp.ptr[u]), int(exp.ptr[u + 1])
        k = np.argsort(pg[a:e], kind="stable")
        np.testing.assert_array_equal(pg[a:e][k], exp.group[a:e])
        np.testing.assert_array_equal(pm[a:e][k], exp.metric[a:e])
        np.testing.assert_array_equal(ph[a:e][k], exp.nh[a:e])
        np.testing.assert_array_equal(pb[a:e][k], exp.n_best[a:e])
    # cap = total - 1: E2BIG with counts and ptr filled; cap 0: the same without entry buffers
    for cap, b in ((total - 1, bufs), (0, (0, 0, 0, 0))):
        d_c.fill_(-1)
        d_ptr.zero_()
        with pytest.raises(SpfError) as ei:
            eng.whatif_routes_device(*head, *b, cap, nb)
        assert ei.value.code == E2BIG
        counts_ok()
    got0, _ = eng.whatif_routes_device(*head, 0, 0, 0, 0, 0, nb, allow_overflow=True)
    assert got0 == total
    # the host form under cap = total - 1: E2BIG, ptr and changed_routes filled (raw call)
    sp, sl = d_sp.cpu().numpy().view(np.uint32), d_sl.cpu().numpy().view(np.uint32)
    gp, gn = d_gp.cpu().numpy().view(np.uint32), d_gn.cpu().numpy().view(np.uint32)
    src = np.asarray(SOURCES, dtype=np.uint32)
    from openr_amd.engine import WhatifRoutes

    h_c = np.full(exp.changed.shape, 0xFFFFFFFF, dtype=np.uint32)
    h_ptr = np.zeros(units + 1, dtype=np.uint64)
    h_g, h_m, h_b = np.zeros(total, np.uint32), np.zeros(total, np.uint64), np.zeros(total, np.uint32)
    h_nh = np.zeros((total, nb), np.uint8)
    gs = SpfGroups(len(groups), _p(gp), _p(gn))
    d = WhatifRoutes(_p(h_ptr), _p(h_g), _p(h_m), _p(h_nh), _p(h_b), total - 1, nb)
    rc = eng._lib.openr_spf_whatif_routes(eng._ctx, _p(sp), _p(sl), len(sets), _p(src), len(src), USE_LINK_METRIC,
                                          ctypes.byref(gs), _p(h_c), ctypes.byref(d), None)
    assert rc == E2BIG
    np.testing.assert_array_equal(h_c, exp.changed)
    np.testing.assert_array_equal(h_ptr, exp.ptr)
    # routes_device on the same table
    d_rm = torch.zeros((len(SOURCES), len(groups)), dtype=torch.int64, device=dev)
    d_rh = torch.zeros((len(SOURCES), len(groups), nb), dtype=torch.uint8, device=dev)
    d_rb = torch.zeros((len(SOURCES), len(groups)), dtype=torch.int32, device=dev)
    eng.routes_device(d_s.data_ptr(), len(SOURCES), d_gp.data_ptr(), d_gn.data_ptr(), len(groups), d_gn.numel(),
                      d_rm.data_ptr(), d_rh.data_ptr(), nb, d_rb.data_ptr())
    torch.cuda.synchronize()
    wm, wh, wb = eng.routes(SOURCES, groups, True)
    np.testing.assert_array_equal(d_rm.cpu().numpy().view(np.uint64), wm)
    np.testing.assert_array_equal(d_rh.cpu().numpy(), wh)
    np.testing.assert_array_equal(d_rb.cpu().numpy().view(np.uint32), wb)


# --- 4. every fixed capacity crossed -----------------------------------------------------
KNOBS = {
    "overlay-global": {"OPENR_SPF_ROUTES_LDS_NODES": "64"},  # V = 120 > 64: overlay in global scratch
    "bitmap-global": {"OPENR_SPF_ROUTES_LDS_GROUPS": "100"},  # G = 162 > 100: bitmap in global scratch
    "list-overflow": {"OPENR_SPF_ROUTES_CAND_CAP": "8"},  # units with more than 8 candidates scan the bitmap
    "no-list": {"OPENR_SPF_ROUTES_CAND_CAP": "0"},
    "delta-rerun": {"OPENR_SPF_ROUTES_DELTA_CAP": "100"},  # the node delta overflows its first estimate
    "wave-groups": {"OPENR_SPF_ROUTES_SMALL_MAX": "3"},  # groups of 4-6 nodes take the wave path
    "all-global": {"OPENR_SPF_ROUTES_LDS_NODES": "0", "OPENR_SPF_ROUTES_LDS_GROUPS": "0",
                   "OPENR_SPF_ROUTES_CAND_CAP": "3"},
}


@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_capacities_crossed(eng, monkeypatch, knob):
    g, sets, groups, exp = sweep_case(0, "dense", True)
    assert exp.facts["max_per_unit"] > 8  # candidate lists of 8 overflow; smaller units still use the list
    for k, v in KNOBS[knob].items():
        monkeypatch.setenv(k, v)
    eng.set_graph(g)
    got = eng.whatif_routes(sets, SOURCES, groups, True)
    check_routes(exp, *got[:6])


def test_routes_chunked_and_wave_boundary(eng, monkeypatch):
    g = small_graph(2)
    _, dense = tables(2)
    eng.set_graph(g)
    want = eng.routes(list(range(120)), dense, True)
    for env in ({"OPENR_SPF_ROUTES_CHUNK": "7"}, {"OPENR_SPF_ROUTES_SMALL_MAX": "3"},
                {"OPENR_SPF_ROUTES_SMALL_MAX": "0"}, {"OPENR_SPF_ROUTES_SMALL_MAX": "200"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            got = eng.routes(list(range(120)), dense, True)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)


# --- 5. wide next hops (exact-order plan) --------------------------------------------------
def test_wide_next_hops(eng):
    n = 300
    adj = {0: list(range(1, n + 1))}
    for i in range(1, n + 1):
        adj[i] = [0, (i - 2) % n + 1, i % n + 1]
    g = T.from_adj_map(adj)
    assert g.nh_bytes() == 38
    hub = g.id("0")
    spokes = [g.id(str(i)) for i in (5, 77, 78, 200, 299)]
    groups = T.loopback_groups(g) + T.prefix_groups(g, [[g.id("5"), g.id("77"), g.id("200")],
                                                        [g.id("78"), g.id("79")], [g.id(str(i)) for i in range(1, 41)]])
    sets = T.node_failure_sets(g, spokes)
    exp = oracle_routes((("hub",), "wide"), g, sets, [hub], groups, True)
    assert exp.facts["sum"] >= 10 and exp.facts["lost"] == 5 and exp.facts["same_metric"] >= 4
    eng.set_graph(g)
    assert eng.nh_bytes == 38
    o = Oracle(g)
    r = o.run_spf(hub, True)
    wm, wh, wb = reduce_routes(r.dist[None], r.nh[None], groups)
    metric, nh, n_best = eng.routes([hub], groups, True)
    assert "spf_exact_kernel" in eng.last_kernels()
    np.testing.assert_array_equal(metric, wm)
    np.testing.assert_array_equal(nh, wh)
    np.testing.assert_array_equal(n_best, wb)
    assert int(wb[0, -1]) == 40 and int(np.unpackbits(wh[0, -1]).sum()) == 40
    got = eng.whatif_routes(sets, [hub], groups, True)
    check_routes(exp, *got[:6])


# --- 6. errors and empty inputs -------------------------------------------------------------
def test_errors_and_empty_inputs(eng):
    g0 = small_graph(2)
    eng.set_graph(g0)
    V = g0.num_nodes
    sets = T.node_failure_sets(g0, [3, 4])
    for groups in ([[0, V]], [[5, 5]], [[7, 2]]):
        for call in (lambda: eng.routes([0], groups), lambda: eng.whatif_routes(sets, [0], groups, cap=4)):
            with pytest.raises(SpfError) as ei:
                call()
            assert ei.value.code == EINVAL
    gp = np.array([0, 2, 1], dtype=np.uint32)  # a descending group_ptr
    gn = np.array([0, 1, 2], dtype=np.uint32)
    src = np.array([0], dtype=np.uint32)
    gs = SpfGroups(2, _p(gp), _p(gn))
    out = np.zeros((1, 2), dtype=np.uint64)
    assert eng._lib.openr_spf_routes(eng._ctx, _p(src), 1, USE_LINK_METRIC, ctypes.byref(gs), _p(out), None, 2,
                                     None) == EINVAL
    # empty sources, sets or tables: zeros
    m, h, b = eng.routes([], [[0], [1]])
    assert m.shape == (0, 2) and h.shape == (0, 2, eng.nh_bytes) and b.shape == (0, 2)
    m, h, b = eng.routes([0, 1], [])
    assert m.shape == (2, 0)
    got = eng.whatif_routes([], [0, 1], [[0]])
    assert got[0].shape == (0, 2) and got[1].tolist() == [0] and len(got[2]) == 0 and got[6] == 0
    got = eng.whatif_routes(sets, [], [[0]])
    assert got[0].shape == (2, 0) and got[1].tolist() == [0] and got[6] == 0
    got = eng.whatif_routes(sets, [0, 1], [])
    assert not got[0].any() and not got[1].any() and len(got[2]) == 0
    # a zero metric: link metric form is refused, hop-count form runs
    m = g0.metric.copy()
    m[int(np.nonzero(g0.edge_up != 0)[0][10])] = 0
    g = dataclasses.replace(g0, metric=m)
    eng.set_graph(g)
    _, dense = tables(2)
    for call in (lambda: eng.routes([0], dense, True), lambda: eng.whatif_routes(sets, [0], dense, True)):
        with pytest.raises(SpfError) as ei:
            call()
        assert ei.value.code == ENOTSUP
    o = Oracle(g)
    r = o.run_spf(0, False)
    wm, wh, wb = reduce_routes(r.dist[None], r.nh[None], dense)
    metric, nh, n_best = eng.routes([0], dense, False)
    np.testing.assert_array_equal(metric, wm)
    np.testing.assert_array_equal(nh, wh)
    np.testing.assert_array_equal(n_best, wb)
    exp = oracle_routes((("zero-metric",), "dense"), g, sets, [0, 8], dense, False)
    check_routes(exp, *eng.whatif_routes(sets, [0, 8], dense, False)[:6])
