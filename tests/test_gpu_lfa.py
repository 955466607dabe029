"""Loop-free alternates on the GPU (openr_spf_lfa_routes*) vs the CPU oracle.

The expectation is the reference rule, getNextHopsWithMetric(me, group, perDestination = false,
one area) with computeLfaPaths_ on (Decision.cpp:1124-1207), applied in Python by lfa_expect to
oracle.Oracle.run_spf rows of every needed node (the sources and their up neighbours). The
module runs under both BFS families / general-metric kernels, as test_gpu_routes_resolve.py does.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from openr_amd import topology as T
from openr_amd.engine import E2BIG, EINVAL, ENOTSUP, USE_LINK_METRIC, LfaEntries, SpfEngine, SpfError, SpfGroups, _p
from oracle import Oracle
from test_gpu_routes_resolve import small_graph, tables

pytestmark = pytest.mark.gpu

U64_MAX = 2**64 - 1
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
_ROWS = {}
_EXPECT = {}


def up_neighbors(g, s):
    """Distinct neighbours of s with at least one up link, in no particular order."""
    return {int(g.col[e]) for e in g.row(s) if g.edge_up[e]}


def closure(g, sources):
    """The rows a batch needs: the distinct nodes among the sources and their up neighbours."""
    need = set(int(s) for s in sources)
    for s in sources:
        need |= up_neighbors(g, int(s))
    return need


def oracle_rows(key, g, nodes, use_metric):
    """({node: dist row}, {node: nh row}) of Oracle.run_spf for every node asked so far."""
    dist, nh = _ROWS.setdefault((key, bool(use_metric)), ({}, {}))
    o = None
    for v in sorted(nodes):
        if v not in dist:
            o = o or Oracle(g)
            r = o.run_spf(int(v), use_metric)
            dist[v], nh[v] = r.dist.copy(), r.nh.copy()
            dist[v].setflags(write=False)
            nh[v].setflags(write=False)
    return dist, nh


@dataclasses.dataclass(frozen=True)
class Expect:
    metric: np.ndarray  # [n, G]
    nh: np.ndarray  # [n, G, nb]
    alt: np.ndarray  # [n, G, nb]
    n_alt: np.ndarray  # [n, G]
    ptr: np.ndarray  # [n * G + 1]
    nbr: np.ndarray
    alt_metric: np.ndarray
    facts: dict


def lfa_expect(dist_rows, nh_rows, g, sources, groups):
    """The rule of the header on oracle rows, in Python integers (no u64 wrap anywhere)."""
    n, G, nb = len(sources), len(groups), g.nh_bytes()
    metric = np.full((n, G), U64_MAX, dtype=np.uint64)
    nh = np.zeros((n, G, nb), dtype=np.uint8)
    alt = np.zeros((n, G, nb), dtype=np.uint8)
    n_alt = np.zeros((n, G), dtype=np.uint32)
    nbr, am = [], []
    facts = {"ovl_tested": 0, "down_only": 0, "self_group_alt": 0, "lfa_only": 0, "no_alt": 0, "reached": 0,
             "nh_not_in_alt": 0}
    for i, s in enumerate(int(x) for x in sources):
        ds, hs = dist_rows[s], nh_rows[s]
        nbrs = g.distinct_neighbors(s)
        up = up_neighbors(g, s)
        facts["down_only"] += sum(1 for x in nbrs if x not in up)
        facts["ovl_tested"] += sum(1 for x in up if g.node_overloaded[x])
        for k, grp in enumerate(groups):
            reached = [int(ds[d]) for d in grp if int(ds[d]) != U64_MAX]
            if not reached:
                continue  # the reference continues before the LFA loop
            mn = min(reached)
            metric[i, k] = mn
            for d in grp:
                if int(ds[d]) == mn:
                    nh[i, k] |= hs[d]
            for b, x in enumerate(nbrs):
                if x not in up:
                    continue
                dn = dist_rows[x]
                to_me = int(dn[s])
                q = [int(dn[d]) for d in grp if int(dn[d]) != U64_MAX and int(dn[d]) < mn + to_me]
                if not q:
                    continue
                alt[i, k, b >> 3] |= np.uint8(1 << (b & 7))
                n_alt[i, k] += 1
                best = min(q)
                if (nh[i, k, b >> 3] >> (b & 7)) & 1:
                    best = min(best, mn - int(ds[x]))
                nbr.append(b)
                am.append(best)
            only = bool((alt[i, k] & ~nh[i, k]).any())
            facts["reached"] += 1
            facts["lfa_only"] += only
            facts["no_alt"] += not only
            facts["nh_not_in_alt"] += bool((nh[i, k] & ~alt[i, k]).any())
            facts["self_group_alt"] += s in grp and bool(alt[i, k].any())
    ptr = np.zeros(n * G + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(n_alt.reshape(-1), dtype=np.uint64)
    e = Expect(metric, nh, alt, n_alt, ptr, np.asarray(nbr, dtype=np.uint32), np.asarray(am, dtype=np.uint64), facts)
    for a in (e.metric, e.nh, e.alt, e.n_alt, e.ptr, e.nbr, e.alt_metric):
        a.setflags(write=False)
    return e


def expect(key, g, sources, groups, use_metric=True):
    k = (key, tuple(int(s) for s in sources), bool(use_metric))
    if k not in _EXPECT:
        dist, nh = oracle_rows(key[0], g, closure(g, sources), use_metric)
        _EXPECT[k] = lfa_expect(dist, nh, g, sources, groups)
    return _EXPECT[k]


def check(exp, got):
    metric, nh, alt, n_alt, ptr, nbr, am = got[:7]
    w = exp.nh.shape[2]
    np.testing.assert_array_equal(metric, exp.metric)
    np.testing.assert_array_equal(nh[:, :, :w], exp.nh)
    np.testing.assert_array_equal(alt[:, :, :w], exp.alt)
    assert not nh[:, :, w:].any() and not alt[:, :, w:].any()  # zero past the graph's width
    np.testing.assert_array_equal(n_alt, exp.n_alt)
    if ptr is not None:
        np.testing.assert_array_equal(ptr, exp.ptr)
        np.testing.assert_array_equal(nbr, exp.nbr)
        np.testing.assert_array_equal(am, exp.alt_metric)


# --- 1. parity ---------------------------------------------------------------------------
# loopback groups under link metrics, the source's own loopback left out: (LFA-only routes,
# routes with no alternate beyond nh, reached pairs) per seed
LOOPBACK_FACTS = {0: (1690, 95, 1785), 1: (1399, 371, 1770), 2: (1691, 94, 1785)}


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("use_metric", [True, False], ids=["metric", "hops"])
def test_parity(eng, bfs_family, seed, use_metric):
    g = small_graph(seed)
    _, dense = tables(seed)
    exp = expect((("small", seed), "dense"), g, SOURCES, dense, use_metric)
    # what the inputs exercise, on the oracle's side
    f = exp.facts
    assert f["nh_not_in_alt"] == 0  # nh is a subset of alt on every reached route
    assert f["lfa_only"] > 0 and f["no_alt"] > 0
    assert f["ovl_tested"] > 0 and f["down_only"] > 0
    assert f["self_group_alt"] > 0  # the all-nodes group holds every source; a neighbour is 0 from itself
    assert (exp.metric == np.uint64(U64_MAX)).any() and not exp.alt[exp.metric == np.uint64(U64_MAX)].any()
    if use_metric:
        lo_only = (exp.alt[:, :120] & ~exp.nh[:, :120]).any(axis=2)
        other = np.ones((len(SOURCES), 120), dtype=bool)
        other[np.arange(len(SOURCES)), SOURCES] = False
        reached = (exp.metric[:, :120] != np.uint64(U64_MAX)) & other
        assert (int((lo_only & reached).sum()), int((~lo_only & reached).sum()),
                int(reached.sum())) == LOOPBACK_FACTS[seed]
    eng.set_graph(g)
    got = eng.lfa_routes(SOURCES, dense, use_metric)
    ks = eng.last_kernels()
    assert "lfa_rows" in ks and "lfa_reduce_count" in ks and "lfa_reduce_emit" in ks and "routes_reduce" in ks, ks
    check(exp, got)
    assert got[7] == len(closure(g, SOURCES))
    rm, rh, _ = eng.routes(SOURCES, dense, use_metric)
    np.testing.assert_array_equal(got[0], rm)
    np.testing.assert_array_equal(got[1], rh)
    # no entries: one pass, the same counts
    one = eng.lfa_routes(SOURCES, dense, use_metric, want_entries=False)
    assert "lfa_reduce_emit" not in eng.last_kernels() and one[4] is None
    check(exp, one)


# --- 2. all sources ----------------------------------------------------------------------
def test_all_sources(eng, bfs_family):
    """Every row is both a source's row and a neighbour's row."""
    g = small_graph(0)
    _, dense = tables(0)
    G = len(dense)
    eng.set_graph(g)
    every = eng.lfa_routes(list(range(120)), dense, True)
    some = eng.lfa_routes(SOURCES, dense, True)
    assert every[7] == 120 and some[7] == len(closure(g, SOURCES))
    check(expect((("small", 0), "dense"), g, SOURCES, dense, True), some)
    for a, b in zip(every[:4], some[:4]):
        np.testing.assert_array_equal(a[SOURCES], b)
    for j, s in enumerate(SOURCES):
        ea, ee = int(every[4][s * G]), int(every[4][(s + 1) * G])
        sa, se = int(some[4][j * G]), int(some[4][(j + 1) * G])
        np.testing.assert_array_equal(every[4][s * G:(s + 1) * G + 1] - every[4][s * G],
                                      some[4][j * G:(j + 1) * G + 1] - some[4][j * G])
        np.testing.assert_array_equal(every[5][ea:ee], some[5][sa:se])
        np.testing.assert_array_equal(every[6][ea:ee], some[6][sa:se])


def test_two_device_slots(bfs_family):
    """The host form splits the sources in contiguous blocks across the context's devices and
    appends each block's entries at the running total: a context over the same ordinal twice
    (the suite's pattern for the split on a 1-GPU box) gives the oracle's answer."""
    g = small_graph(1)
    _, dense = tables(1)
    exp = expect((("small", 1), "dense"), g, SOURCES, dense, True)
    two = SpfEngine([0, 0])
    try:
        two.set_graph(g)
        got = two.lfa_routes(SOURCES, dense, True)
        check(exp, got)
        h = (len(SOURCES) + 1) // 2
        assert got[7] == len(closure(g, SOURCES[:h])) + len(closure(g, SOURCES[h:]))
    finally:
        two.close()


# --- 3. capacities and fallbacks crossed ---------------------------------------------------
KNOBS = {
    "wave-groups": {"OPENR_SPF_ROUTES_SMALL_MAX": "1"},  # every non-singleton group on the wave path
    "lane-groups": {"OPENR_SPF_ROUTES_SMALL_MAX": "200"},  # none on it, the all-nodes group included
    "chunked": {"OPENR_SPF_ROUTES_CHUNK": "4"},  # 4 chunks of sources, each with its own closure
    "slices": {"OPENR_SPF_LFA_SLICE": "8"},  # a neighbour table of more than 8 entries takes several slices
}


@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_capacities_crossed(eng, monkeypatch, knob):
    g = small_graph(2)
    _, dense = tables(2)
    exp = expect((("small", 2), "dense"), g, SOURCES, dense, True)
    assert max(len(g.row(s)) for s in SOURCES) > 8
    for k, v in KNOBS[knob].items():
        monkeypatch.setenv(k, v)
    eng.set_graph(g)
    got = eng.lfa_routes(SOURCES, dense, True)
    check(exp, got)
    want = len(closure(g, SOURCES))
    if knob == "chunked":  # a row two chunks need is solved in both
        want = sum(len(closure(g, SOURCES[c:c + 4])) for c in range(0, len(SOURCES), 4))
    assert got[7] == want


def test_duplicate_sources(eng):
    g = small_graph(1)
    _, dense = tables(1)
    srcs = [0, 8, 0, 16, 8]
    exp = expect((("small", 1), "dense"), g, srcs, dense, True)
    eng.set_graph(g)
    check(exp, eng.lfa_routes(srcs, dense, True))


def test_source_without_up_neighbor(eng):
    g0 = small_graph(0)
    x = 16
    down = set(g0.link_id[g0.row_ptr[x]:g0.row_ptr[x + 1]].tolist())
    up = g0.edge_up.copy()
    up[np.isin(g0.link_id, sorted(down))] = 0
    g = dataclasses.replace(g0, edge_up=up)
    assert not up_neighbors(g, x) and g.distinct_neighbors(x)
    _, dense = tables(0)
    srcs = [x, 8, 24]
    exp = expect((("isolated", 0), "dense"), g, srcs, dense, True)
    assert int((exp.metric[0] != np.uint64(U64_MAX)).sum()) >= 2 and not exp.alt[0].any()  # its loopback, all-nodes
    assert exp.alt[1].any()
    eng.set_graph(g)
    got = eng.lfa_routes(srcs, dense, True)
    check(exp, got)
    assert got[7] == len(closure(g, srcs))
    check(lfa_expect(*oracle_rows(("isolated", 0), g, {x}, True), g, [x], dense), eng.lfa_routes([x], dense, True))


# --- 4. wide next-hop sets -------------------------------------------------------------------
def wide_graph():
    n = 75  # hub 0 with 75 spokes; spokes 1..40 form a ring, the others hang off the hub alone
    adj = {0: [(i, 1 + i % 3) for i in range(1, n + 1)]}
    for i in range(1, n + 1):
        adj[i] = [(0, 1 + i % 3)]
        if i <= 40:
            adj[i] += [((i - 2) % 40 + 1, 1), (i % 40 + 1, 1)]
    return T.from_adj_map(adj)


def test_wide_next_hops(eng, monkeypatch):
    g = wide_graph()
    assert g.nh_bytes() == 10
    hub = g.id("0")
    srcs = [hub, g.id("5"), g.id("60")]
    groups = T.loopback_groups(g) + T.prefix_groups(g, [
        [g.id("5"), g.id("33"), g.id("70")], [g.id(str(i)) for i in range(1, 31)], range(g.num_nodes), []])
    exp = expect((("wide",), "wide"), g, srcs, groups, True)
    assert len(g.distinct_neighbors(hub)) == 75 and int(exp.n_alt[0].max()) >= 70  # bits past 64 are set
    assert exp.facts["lfa_only"] > 0 and exp.facts["no_alt"] > 0 and exp.facts["nh_not_in_alt"] == 0
    monkeypatch.setenv("OPENR_SPF_LFA_SLICE", "16")  # the hub's table: five slices
    eng.set_graph(g)
    assert eng.nh_bytes == 10
    got = eng.lfa_routes(srcs, groups, True, nh_bytes=13)
    assert got[1].shape[2] == 13 and got[2].shape[2] == 13
    check(exp, got)
    monkeypatch.setenv("OPENR_SPF_ROUTES_SMALL_MAX", "2")
    check(exp, eng.lfa_routes(srcs, groups, True, nh_bytes=13))


# --- 5. entries and cap ------------------------------------------------------------------
def test_entries_and_cap(eng):
    g = small_graph(1)
    _, dense = tables(1)
    exp = expect((("small", 1), "dense"), g, SOURCES, dense, True)
    total = int(exp.ptr[-1])
    assert total == int(exp.n_alt.sum()) and total > 0
    eng.set_graph(g)
    check(exp, eng.lfa_routes(SOURCES, dense, True, cap=total))
    gp = np.zeros(len(dense) + 1, dtype=np.uint32)
    gp[1:] = np.cumsum([len(x) for x in dense])
    gn = np.concatenate([np.asarray(x, dtype=np.uint32) for x in dense])
    gs = SpfGroups(len(dense), _p(gp), _p(gn))
    src = np.asarray(SOURCES, dtype=np.uint32)
    n, G, nb = len(SOURCES), len(dense), eng.nh_bytes

    def raw(cap, with_entries=True):
        metric = np.full((n, G), 7, dtype=np.uint64)
        nh = np.full((n, G, nb), 0xEE, dtype=np.uint8)
        alt = np.full((n, G, nb), 0xEE, dtype=np.uint8)
        n_alt = np.full((n, G), 0xFFFFFFFF, dtype=np.uint32)
        ptr = np.full(n * G + 1, 5, dtype=np.uint64)
        nbr = np.zeros(max(cap, 1), dtype=np.uint32)
        am = np.zeros(max(cap, 1), dtype=np.uint64)
        ent = LfaEntries(_p(ptr), _p(nbr), _p(am), cap)
        rc = eng._lib.openr_spf_lfa_routes(eng._ctx, _p(src), n, USE_LINK_METRIC, ctypes.byref(gs), _p(metric),
                                           _p(nh), _p(alt), nb, _p(n_alt), ctypes.byref(ent) if with_entries else None,
                                           None)
        return rc, (metric, nh, alt, n_alt, ptr if with_entries else None, nbr, am)

    rc, got = raw(total - 1)
    assert rc == E2BIG
    check(exp, got[:4] + (None, None, None))
    np.testing.assert_array_equal(got[4], exp.ptr)
    rc0, got0 = raw(0)
    assert rc0 == E2BIG
    np.testing.assert_array_equal(got0[4], exp.ptr)
    rcn, gotn = raw(0, with_entries=False)
    assert rcn == 0
    for a, b in zip(got0[:4], gotn[:4]):
        np.testing.assert_array_equal(a, b)
    check(exp, gotn[:4] + (None, None, None))


# --- 6. device form ------------------------------------------------------------------------
def test_device_form(eng, bfs_family):
    import torch

    g = small_graph(2)
    V = g.num_nodes
    _, dense = tables(2)
    # a malformed table: a member >= V inside a group, and a last group whose slice runs past
    # n_group_nodes; the device form clamps the slice and counts the bad member as unreached
    bad = dense + [[3, 50, V + 5], [7, 9, 11, 60]]
    good = dense + [[3, 50], [7, 9, 11, 60]]
    gp = np.zeros(len(bad) + 1, dtype=np.int32)
    gp[1:] = np.cumsum([len(x) for x in bad])
    gn = np.concatenate([np.asarray(x, dtype=np.int32) for x in bad])
    gp[-1] += 50
    exp = expect((("small", 2), "malformed"), g, SOURCES, good, True)
    total = int(exp.ptr[-1])
    eng.set_graph(g)
    n, G, nb, guard = len(SOURCES), len(bad), eng.nh_bytes + 1, 64
    dev = torch.device("cuda", 0)
    d_gp, d_gn = torch.from_numpy(gp).to(dev), torch.from_numpy(gn).to(dev)
    d_s = torch.from_numpy(np.asarray(SOURCES, dtype=np.int32)).to(dev)

    def guarded(count, dtype, fill):
        t = torch.full((count + 2 * guard,), fill, dtype=dtype, device=dev)
        return t, t.data_ptr() + guard * t.element_size(), fill

    def body(buf, view):
        t, _, fill = buf
        assert bool((t[:guard] == fill).all()) and bool((t[-guard:] == fill).all())  # nothing outside [n][G]
        return t[guard:-guard].cpu().numpy().view(view)

    stream = torch.cuda.Stream(device=dev)

    def run(cap, want_entries=True):
        bufs = {"metric": guarded(n * G, torch.int64, -3), "nh": guarded(n * G * nb, torch.uint8, 0xEE),
                "alt": guarded(n * G * nb, torch.uint8, 0xEE), "n_alt": guarded(n * G, torch.int32, -3),
                "ptr": guarded(n * G + 1, torch.int64, -3), "nbr": guarded(max(cap, 1), torch.int32, -3),
                "am": guarded(max(cap, 1), torch.int64, -3)}
        ent = (bufs["ptr"][1], bufs["nbr"][1], bufs["am"][1]) if want_entries else (0, 0, 0)
        code = 0
        try:
            tot, solved = eng.lfa_routes_device(d_s.data_ptr(), n, d_gp.data_ptr(), d_gn.data_ptr(), G, d_gn.numel(),
                                                bufs["metric"][1], bufs["nh"][1], bufs["alt"][1], nb,
                                                bufs["n_alt"][1], *ent, cap, stream=stream.cuda_stream)
        except SpfError as e:
            code = e.code
            tot, solved = eng.lfa_routes_device(d_s.data_ptr(), n, d_gp.data_ptr(), d_gn.data_ptr(), G, d_gn.numel(),
                                                bufs["metric"][1], bufs["nh"][1], bufs["alt"][1], nb,
                                                bufs["n_alt"][1], *ent, cap, stream=stream.cuda_stream,
                                                allow_overflow=True)
        stream.synchronize()
        out = (body(bufs["metric"], np.uint64).reshape(n, G), body(bufs["nh"], np.uint8).reshape(n, G, nb),
               body(bufs["alt"], np.uint8).reshape(n, G, nb), body(bufs["n_alt"], np.uint32).reshape(n, G),
               body(bufs["ptr"], np.uint64), body(bufs["nbr"], np.uint32), body(bufs["am"], np.uint64))
        return code, tot, solved, out

    code, tot, solved, out = run(total)
    assert code == 0 and tot == total and solved == len(closure(g, SOURCES))
    check(exp, out[:5] + (out[5][:total], out[6][:total]))
    for u in range(n * G):  # bits ascending inside every unit
        assert (np.diff(out[5][int(exp.ptr[u]):int(exp.ptr[u + 1])].astype(np.int64)) > 0).all()
    # the two malformed groups: the bad member and the entries past n_group_nodes count for nothing
    assert out[3][:, -2:].sum() > 0
    # cap below the total: E2BIG, counts and ptr filled
    code1, tot1, _, out1 = run(total - 1)
    assert code1 == E2BIG and tot1 == total
    check(exp, out1[:4] + (None, None, None))
    np.testing.assert_array_equal(out1[4], exp.ptr)
    # no entry request: one pass, ptr and the entry buffers untouched
    code2, tot2, _, out2 = run(0, want_entries=False)
    assert code2 == 0 and tot2 == 0
    check(exp, out2[:4] + (None, None, None))
    assert (out2[4] == np.uint64(2**64 - 3)).all()


# --- 7. errors --------------------------------------------------------------------------------
def test_errors(eng):
    g0 = small_graph(2)
    eng.set_graph(g0)
    V = g0.num_nodes
    for groups in ([[7, 2]], [[0, V]], [[5, 5]]):
        with pytest.raises(SpfError) as ei:
            eng.lfa_routes([0], groups)
        assert ei.value.code == EINVAL
    with pytest.raises(SpfError) as ei:
        eng.lfa_routes([0], [[1]], nh_bytes=eng.nh_bytes - 1)
    assert ei.value.code == EINVAL
    with pytest.raises(SpfError) as ei:
        eng.lfa_routes([V], [[1]])
    assert ei.value.code == EINVAL
    # empty inputs
    got = eng.lfa_routes([], [[0], [1]])
    assert got[0].shape == (0, 2) and got[4].tolist() == [0] and got[7] == 0
    got = eng.lfa_routes([0, 1], [])
    assert got[0].shape == (2, 0) and got[4].tolist() == [0]
    # a zero metric: the link-metric form is refused, the hop-count form runs
    m = g0.metric.copy()
    m[int(np.nonzero(g0.edge_up != 0)[0][10])] = 0
    g = dataclasses.replace(g0, metric=m)
    eng.set_graph(g)
    _, dense = tables(2)
    with pytest.raises(SpfError) as ei:
        eng.lfa_routes([0], dense, True)
    assert ei.value.code == ENOTSUP
    exp = expect((("zero-metric",), "dense"), g, [0, 8], dense, False)
    check(exp, eng.lfa_routes([0, 8], dense, False))
