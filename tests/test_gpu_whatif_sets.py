"""Link-set what-if sweep on the GPU (openr_spf_whatif_sets*) vs the CPU oracle.

A unit (i, j) fails every link of set i at once for source j: node failures (all of a
router's links) and shared-risk link groups. Expected values are oracle runs of
runSpf(source, useLinkMetric, set) diffed against the no-failure run, the way
whatif_oracle / check_delta_rows of test_gpu_parity.py do it for one link. The module runs
on both what-if re-solve routes: the rounds kernel's seeded start with the fused compare
and delta (lvl-rounds), and plain ignore-set solves + rows_compare (code-fringe; the BFS
families and the exact-order kernel take that route under either setting).
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from openr_amd import topology as T
from openr_amd.engine import E2BIG, EINVAL, SpfEngine, SpfError
from oracle import Oracle
from test_gpu_parity import random_graph

pytestmark = pytest.mark.gpu

U64_MAX = np.uint64(2**64 - 1)


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


# --- oracle side: computed once per (graph, sets, sources, metric form), shared by both
# --- parametrisations of the module and never modified
_GRAPHS = {}
_EXPECT = {}


def small_graph(seed):
    """The three graphs of the module: V = 120, L = 330 with overloads, down and parallel links."""
    if seed not in _GRAPHS:
        max_metric = {0: 64, 1: 1, 2: 7}[seed]
        _GRAPHS[seed] = random_graph(400 + seed, 120, 300, max_metric, p_ovl=0.05, p_down=0.05, p_par=0.1)
    return _GRAPHS[seed]


@dataclasses.dataclass(frozen=True)
class Expect:
    changed: np.ndarray  # [n_sets, n_sources]
    ptr: np.ndarray  # [units + 1] u64
    node: np.ndarray  # every unit's changed nodes ascending, concatenated
    dist: np.ndarray  # their distance in the failure run
    nh: np.ndarray  # [entries, oracle nh_bytes]
    same_dist: np.ndarray  # per entry: the node's distance is the base distance (next hops changed)


def oracle_sets(key, g, sets, sources, use_metric=True):
    """Expected changed counts and delta rows of every unit (set i, source j)."""
    k = (key, bool(use_metric))
    if k in _EXPECT:
        return _EXPECT[k]
    o = Oracle(g)
    base = [o.run_spf(int(s), use_metric) for s in sources]
    changed = np.zeros((len(sets), len(sources)), dtype=np.uint32)
    nodes, dists, nhs, same = [], [], [], []
    for i, st in enumerate(sets):
        for j, s in enumerate(sources):
            r = o.run_spf(int(s), use_metric, [int(l) for l in st])
            b = base[j]
            ch = np.nonzero((r.dist != b.dist) | np.any(r.nh != b.nh, axis=1))[0]
            changed[i, j] = len(ch)
            nodes.append(ch.astype(np.uint32))
            dists.append(r.dist[ch])
            nhs.append(r.nh[ch])
            same.append(r.dist[ch] == b.dist[ch])
    ptr = np.zeros(changed.size + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(changed.reshape(-1), dtype=np.uint64)
    e = Expect(changed, ptr, np.concatenate(nodes) if nodes else np.zeros(0, np.uint32),
               np.concatenate(dists) if dists else np.zeros(0, np.uint64),
               np.concatenate(nhs) if nhs else np.zeros((0, o.nh_bytes), np.uint8),
               np.concatenate(same) if same else np.zeros(0, bool))
    for a in dataclasses.astuple(e):
        a.setflags(write=False)
    _EXPECT[k] = e
    return e


def check_delta(exp, changed, ptr, node, dist, nh):
    """changed and the host delta CSR, entry for entry: nodes ascending, new dist, nh bytes
    (zero past the graph's width)."""
    np.testing.assert_array_equal(changed, exp.changed)
    np.testing.assert_array_equal(ptr, exp.ptr)
    np.testing.assert_array_equal(node, exp.node)
    np.testing.assert_array_equal(dist, exp.dist)
    want = np.zeros((exp.nh.shape[0], nh.shape[1]), dtype=np.uint8)
    want[:, : exp.nh.shape[1]] = exp.nh
    np.testing.assert_array_equal(nh, want)


def route_kernels(eng, bfs_family, uniform):
    """The re-solve kernel the module's parametrisation selects shows in the launch trace."""
    ks = eng.last_kernels()
    want = "bfs_" if uniform else "fringe_kernel" if bfs_family[1] == "fringe" else "rounds_kernel"
    assert ks and all(k.startswith(want) for k in ks), ks


# --- 1. node failures: counts and delta rows -----------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_node_failures_match_oracle(eng, bfs_family, seed):
    g = small_graph(seed)
    assert g.num_nodes == 120 and g.num_links == 330
    sets = T.node_failure_sets(g)
    assert 12 <= max(len(s) for s in sets) <= 15
    sources = list(range(0, g.num_nodes, 4))
    exp = oracle_sets(("node", seed), g, sets, sources)
    assert exp.changed.size == 3600
    # what the inputs exercise, on the oracle's side
    assert (exp.dist == U64_MAX).any()  # units that cut nodes off
    assert 49 <= int((exp.changed > 64).sum()) <= 60  # units changing more than a wave's worth of nodes
    assert (exp.same_dist & (exp.dist != U64_MAX)).any()  # next hops change, the distance does not
    assert int((exp.changed == 0).sum()) == (30 if seed == 1 else 0)  # isolated nodes (seed 1)
    eng.set_graph(g)
    changed, solved = eng.whatif_sets(sets, sources, True)
    route_kernels(eng, bfs_family, uniform=(seed == 1))
    np.testing.assert_array_equal(changed, exp.changed)
    assert len(sources) <= solved <= changed.size + len(sources)
    assert solved >= int((exp.changed != 0).sum()) + len(sources)
    c2, ptr, node, dist, nh, solved2 = eng.whatif_sets_delta(sets, sources, True)
    assert solved2 == solved
    check_delta(exp, c2, ptr, node, dist, nh)
    assert (dist == U64_MAX).any() and (c2 > 64).any()


# --- 2. shared-risk groups with empty sets; the filter ------------------------------------
def srlg_case(seed):
    g = small_graph(seed)
    rng = np.random.default_rng(50 + seed)
    sizes = rng.integers(0, 6, 80)
    sets = T.srlg_sets(g, [rng.choice(g.num_links, int(k), replace=False).tolist() for k in sizes])
    return g, sets, list(range(0, g.num_nodes, 4))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_srlg_sets_and_filter(eng, bfs_family, seed):
    g, sets, sources = srlg_case(seed)
    empty = [i for i, s in enumerate(sets) if not s]
    assert empty and max(len(s) for s in sets) == 5
    exp = oracle_sets(("srlg", seed), g, sets, sources)
    n_units = len(sets) * len(sources)
    assert n_units == 2400
    assert int((exp.changed == 0).sum()) == {0: 875, 1: 1012, 2: 1047}[seed]
    eng.set_graph(g)
    changed, ptr, node, dist, nh, solved = eng.whatif_sets_delta(sets, sources, True)
    check_delta(exp, changed, ptr, node, dist, nh)
    # only units whose set holds a base-tight link are solved, plus the base solves
    assert len(sources) <= solved < n_units + len(sources)
    assert solved >= int((exp.changed != 0).sum()) + len(sources)
    assert not changed[empty].any()
    c1, solved1 = eng.whatif_sets(sets, sources, True)
    np.testing.assert_array_equal(c1, exp.changed)
    assert solved1 == solved


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_srlg_sets_hop_count_and_wider_nh(eng, seed):
    g, sets, sources = srlg_case(seed)
    sets, sources = sets[:20], sources[:6]
    exp = oracle_sets(("srlg-hops", seed), g, sets, sources, use_metric=False)
    assert 36 <= int((exp.changed == 0).sum()) <= 41 and exp.changed.size == 120
    eng.set_graph(g)
    got = eng.whatif_sets_delta(sets, sources, False, nh_bytes=eng.nh_bytes + 5)
    assert got[4].shape[1] == eng.nh_bytes + 5
    check_delta(exp, *got[:5])


# --- 3. uniform-cost level family -----------------------------------------------------
def test_grid_node_failures(eng, bfs_family):
    g = T.grid(8)
    sets = T.node_failure_sets(g)
    sources = list(range(0, 64, 5))
    exp = oracle_sets(("grid8",), g, sets, sources)
    assert exp.changed.size == 832
    assert (exp.changed != 0).all()  # every unit cuts its node off (or, at the source, all others)
    assert int((exp.dist == U64_MAX).sum()) >= 832
    eng.set_graph(g)
    got = eng.whatif_sets_delta(sets, sources, True)
    route_kernels(eng, bfs_family, uniform=True)
    check_delta(exp, *got[:5])
    assert got[5] == 832 + len(sources)  # no unit is filtered


# --- 4. exact-order plan --------------------------------------------------------------
def test_exact_order_plan(eng):
    """One usable metric set to 0: the graph leaves the fast kernels' domain, every solve runs
    on the exact-order kernel and the filter keeps every unit whose set holds a link of the
    graph (the pop order depends on every relaxation)."""
    g0 = small_graph(2)
    m = g0.metric.copy()
    e0 = int(np.nonzero(g0.edge_up != 0)[0][10])
    m[e0] = 0
    g = dataclasses.replace(g0, metric=m)
    sets = T.node_failure_sets(g)
    sources = list(range(0, g.num_nodes, 15))
    assert len(sources) == 8
    exp = oracle_sets(("exact",), g, sets, sources)
    eng.set_graph(g)
    got = eng.whatif_sets_delta(sets, sources, True)
    assert "spf_exact_kernel" in eng.last_kernels()
    check_delta(exp, *got[:5])
    assert got[5] == len(sources) * (1 + sum(1 for s in sets if s))
    c, _ = eng.whatif_sets(sets, sources, True)
    np.testing.assert_array_equal(c, exp.changed)


# --- 5. singletons equal the single-link calls ----------------------------------------
def test_singletons_equal_single_link_calls(eng):
    g = small_graph(0)
    eng.set_graph(g)
    links = list(range(g.num_links))
    sets = [[l] for l in links]
    sources = list(range(0, g.num_nodes, 4))
    c1, s1 = eng.whatif(links, sources, True)
    c2, s2 = eng.whatif_sets(sets, sources, True)
    np.testing.assert_array_equal(c2, c1)
    assert s2 == s1
    d1 = eng.whatif_delta(links, sources, True)
    d2 = eng.whatif_sets_delta(sets, sources, True)
    for a, b in zip(d1[:5], d2[:5]):
        np.testing.assert_array_equal(b, a)
    assert d2[5] == d1[5]


# --- 6. device forms and cap ----------------------------------------------------------
def test_device_forms_and_cap(eng):
    import torch

    g = T.wan(1000, 3000, 64, seed=1)
    eng.set_graph(g)
    rng = np.random.default_rng(13)
    nodes = np.sort(rng.choice(g.num_nodes, 12, replace=False))
    sources = np.sort(rng.choice(g.num_nodes, 10, replace=False)).astype(np.uint32)
    sets = T.node_failure_sets(g, nodes)
    changed, ptr, node, dist, nh, solved = eng.whatif_sets_delta(sets, sources, True)
    exp = oracle_sets(("wan",), g, sets, sources)
    check_delta(exp, changed, ptr, node, dist, nh)
    total = int(ptr[-1])
    assert total == int(changed.sum()) and total > 0
    nb, units = eng.nh_bytes, len(sets) * len(sources)
    sp = np.zeros(len(sets) + 1, dtype=np.int32)
    sp[1:] = np.cumsum([len(s) for s in sets])
    sl = np.concatenate([np.asarray(s, dtype=np.int32) for s in sets])
    dev = torch.device("cuda", 0)
    d_sp, d_sl = torch.from_numpy(sp).to(dev), torch.from_numpy(sl).to(dev)
    d_s = torch.from_numpy(sources.astype(np.int32)).to(dev)
    d_c = torch.full((len(sets), len(sources)), -1, dtype=torch.int32, device=dev)
    s_dev = eng.whatif_sets_device(d_sp.data_ptr(), d_sl.data_ptr(), len(sets), len(sl), d_s.data_ptr(), len(sources),
                                   d_c.data_ptr(), True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint32), changed)
    assert s_dev == solved
    d_ptr = torch.zeros(units + 1, dtype=torch.int64, device=dev)
    d_node = torch.zeros(total, dtype=torch.int32, device=dev)
    d_dist = torch.zeros(total, dtype=torch.int64, device=dev)
    d_nh = torch.zeros((total, nb), dtype=torch.uint8, device=dev)
    args = (d_sp.data_ptr(), d_sl.data_ptr(), len(sets), len(sl), d_s.data_ptr(), len(sources), d_c.data_ptr(),
            d_ptr.data_ptr(), d_node.data_ptr(), d_dist.data_ptr(), d_nh.data_ptr())
    d_c.fill_(-1)
    got, _ = eng.whatif_sets_delta_device(*args, total, nb)
    assert got == total
    np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint32), changed)
    p = d_ptr.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(p, ptr)
    pn = d_node.cpu().numpy().view(np.uint32)
    pd = d_dist.cpu().numpy().view(np.uint64)
    ph = d_nh.cpu().numpy()
    for u in range(units):  # the device form keeps discovery order: sort each unit by node
        a, e = int(p[u]), int(p[u + 1])
        k = np.argsort(pn[a:e], kind="stable")
        np.testing.assert_array_equal(pn[a:e][k], node[a:e])
        np.testing.assert_array_equal(pd[a:e][k], dist[a:e])
        np.testing.assert_array_equal(ph[a:e][k], nh[a:e])
    # cap below the total: E2BIG, counts and ptr still filled
    d_c.fill_(-1)
    d_ptr.zero_()
    with pytest.raises(SpfError) as ei:
        eng.whatif_sets_delta_device(*args, total - 1, nb)
    assert ei.value.code == E2BIG
    np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint32), changed)
    np.testing.assert_array_equal(d_ptr.cpu().numpy().view(np.uint64), ptr)
    # the host form under the same cap: E2BIG with ptr and changed filled (raw call)
    src = np.ascontiguousarray(sources, dtype=np.uint32)
    hp, hl = sp.astype(np.uint32), sl.astype(np.uint32)
    h_c = np.full((len(sets), len(sources)), 0xFFFFFFFF, dtype=np.uint32)
    h_ptr = np.zeros(units + 1, dtype=np.uint64)
    h_node, h_dist = np.zeros(total, np.uint32), np.zeros(total, np.uint64)
    h_nh = np.zeros((total, nb), np.uint8)
    from openr_amd.engine import USE_LINK_METRIC, WhatifDelta, _p

    d = WhatifDelta(_p(h_ptr), _p(h_node), _p(h_dist), _p(h_nh), total - 1, nb)
    rc = eng._lib.openr_spf_whatif_sets_delta(eng._ctx, _p(hp), _p(hl), len(sets), _p(src), len(src), USE_LINK_METRIC,
                                              _p(h_c), ctypes.byref(d), None)
    assert rc == E2BIG
    np.testing.assert_array_equal(h_c, changed)
    np.testing.assert_array_equal(h_ptr, ptr)
    # cap 0: counts and ptr only (no entry buffers)
    d_c.fill_(-1)
    d_ptr.zero_()
    got0, _ = eng.whatif_sets_delta_device(*args[:8], 0, 0, 0, 0, nb, allow_overflow=True)
    assert got0 == total
    np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint32), changed)
    np.testing.assert_array_equal(d_ptr.cpu().numpy().view(np.uint64), ptr)


# --- 7. edge cases --------------------------------------------------------------------
def test_edge_cases(eng):
    from openr_amd.engine import USE_LINK_METRIC, _p

    g = small_graph(0)
    o = Oracle(g)
    eng.set_graph(g)
    V, L = g.num_nodes, g.num_links
    # no sets, or no sources
    c, solved = eng.whatif_sets([], [0, 1], True)
    assert c.shape == (0, 2) and solved == 0
    c, solved = eng.whatif_sets([[0], [1, 2]], [], True)
    assert c.shape == (2, 0) and solved == 0
    got = eng.whatif_sets_delta([], [0, 1], True)
    assert got[0].shape == (0, 2) and got[1].tolist() == [0] and len(got[2]) == 0 and got[5] == 0
    got = eng.whatif_sets_delta([[0]], [], True)
    assert got[0].shape == (1, 0) and got[1].tolist() == [0] and got[5] == 0
    # a link id == L, a source == V, a descending set_ptr
    for call in (lambda: eng.whatif_sets([[0, L]], [0], True), lambda: eng.whatif_sets_delta([[L]], [0], True, cap=4),
                 lambda: eng.whatif_sets([[0]], [V], True)):
        with pytest.raises(SpfError) as ei:
            call()
        assert ei.value.code == EINVAL
    sp = np.array([0, 2, 1], dtype=np.uint32)
    sl = np.array([0, 1, 2], dtype=np.uint32)
    src = np.array([0], dtype=np.uint32)
    out = np.zeros((2, 1), dtype=np.uint32)
    rc = eng._lib.openr_spf_whatif_sets(eng._ctx, _p(sp), _p(sl), 2, _p(src), 1, USE_LINK_METRIC, _p(out), None)
    assert rc == EINVAL
    # a set listing one link three times equals the singleton
    sources = list(range(0, V, 4))
    base = [o.run_spf(s, True) for s in sources]
    pick = [l for l in range(L) if g.edge_up[np.nonzero(g.link_id == l)[0][0]]][:40]
    a = eng.whatif_sets_delta([[l, l, l] for l in pick], sources, True)
    b = eng.whatif_sets_delta([[l] for l in pick], sources, True)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert a[0].any()
    # a set holding every link: every reachable non-source node is cut off
    c, ptr, node, dist, nh, solved = eng.whatif_sets_delta([list(range(L))], sources, True)
    for j, s in enumerate(sources):
        reach = np.nonzero((base[j].dist != U64_MAX) & (np.arange(V) != s))[0]
        np.testing.assert_array_equal(node[int(ptr[j]) : int(ptr[j + 1])], reach)
        assert c[0, j] == len(reach)
    assert (dist == U64_MAX).all() and not nh.any()
    # a source whose own node is the failed one: it reaches nothing but itself
    nodes = sources[:10]
    c, ptr, node, dist, nh, _ = eng.whatif_sets_delta(T.node_failure_sets(g, nodes), nodes, True)
    for k, s in enumerate(nodes):
        u = k * len(nodes) + k
        j = sources.index(s)
        reach = np.nonzero((base[j].dist != U64_MAX) & (np.arange(V) != s))[0]
        np.testing.assert_array_equal(node[int(ptr[u]) : int(ptr[u + 1])], reach)
        assert (dist[int(ptr[u]) : int(ptr[u + 1])] == U64_MAX).all()


# --- 8. the split across devices, on one device ------------------------------------------
def test_permuted_and_split_calls_agree(eng, bfs_family):
    """The host form rebases set_ptr for each device's block of sets: a caller-side split in
    two halves (the second half's links start mid-array in the whole call) and a permutation
    of the sets must give the same per-set answers."""
    g, sets, sources = srlg_case(0)
    exp = oracle_sets(("srlg", 0), g, sets, sources)
    eng.set_graph(g)
    whole = eng.whatif_sets_delta(sets, sources, True)
    check_delta(exp, *whole[:5])
    h = len(sets) // 2
    lo, hi = eng.whatif_sets_delta(sets[:h], sources, True), eng.whatif_sets_delta(sets[h:], sources, True)
    np.testing.assert_array_equal(np.concatenate([lo[0], hi[0]]), whole[0])
    np.testing.assert_array_equal(np.concatenate([lo[1], hi[1][1:] + lo[1][-1]]), whole[1])
    for k in (2, 3, 4):
        np.testing.assert_array_equal(np.concatenate([lo[k], hi[k]]), whole[k])
    assert lo[5] + hi[5] == whole[5] + len(sources)  # the base solves run once per call
    perm = np.random.default_rng(8).permutation(len(sets))
    pc, pptr, pnode, pdist, pnh, psolved = eng.whatif_sets_delta([sets[i] for i in perm], sources, True)
    assert psolved == whole[5]
    np.testing.assert_array_equal(pc, whole[0][perm])
    ns = len(sources)
    for k, i in enumerate(perm):
        for j in range(ns):
            a, e = int(pptr[k * ns + j]), int(pptr[k * ns + j + 1])
            a0, e0 = int(whole[1][i * ns + j]), int(whole[1][i * ns + j + 1])
            np.testing.assert_array_equal(pnode[a:e], whole[2][a0:e0])
            np.testing.assert_array_equal(pdist[a:e], whole[3][a0:e0])
            np.testing.assert_array_equal(pnh[a:e], whole[4][a0:e0])
