"""Post-failure loop-free alternates on the GPU (openr_spf_whatif_lfa*) vs the CPU oracle.

The expectation is the contract taken literally: for every failure set, the oracle's
run_spf(v, use_metric, set) rows of every node of the base closure (the sources and their up
neighbours) go through test_gpu_lfa.lfa_expect on the graph with the set's links cleared, and
the result is diffed against lfa_expect on the unfailed graph. Everything is compared bit for
bit. The module runs under both BFS families / general-metric kernels, as test_gpu_lfa.py does.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from openr_amd import topology as T
from openr_amd.engine import E2BIG, EINVAL, ENOTSUP, USE_LINK_METRIC, SpfEngine, SpfError, SpfGroups, WhatifLfa, _p
from oracle import Oracle
from test_gpu_lfa import SOURCES, closure, lfa_expect, up_neighbors, wide_graph
from test_gpu_routes_resolve import DENSE_FACTS, small_graph, tables

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


# --- oracle side: computed once per key, shared by both parametrisations, never modified
_EXPECT = {}


@dataclasses.dataclass(frozen=True)
class Expect:
    changed: np.ndarray  # [n_sets, n_sources]
    unprotected: np.ndarray  # [n_sets, n_sources]
    lost_backup: np.ndarray  # [n_sets, n_sources]
    ptr: np.ndarray  # [units + 1]
    group: np.ndarray  # every unit's changed groups ascending, concatenated
    metric: np.ndarray
    nh: np.ndarray  # [entries, nb]
    alt: np.ndarray  # [entries, nb]
    base: tuple  # (metric [S, G], nh [S, G, nb], alt [S, G, nb]) of the unfailed graph
    facts: dict


def popcount(a):
    return np.unpackbits(a, axis=-1).sum(axis=-1)


def failed_graph(g, links):
    up = g.edge_up.copy()
    if len(links):
        up[np.isin(g.link_id, sorted(set(int(l) for l in links)))] = 0
    return dataclasses.replace(g, edge_up=up)


def oracle_whatif_lfa(key, g, sets, sources, groups, use_metric=True):
    k = (key, bool(use_metric))
    if k in _EXPECT:
        return _EXPECT[k]
    o = Oracle(g)
    need = sorted(closure(g, sources))
    brow = {v: o.run_spf(v, use_metric) for v in need}
    bd, bh = {v: r.dist for v, r in brow.items()}, {v: r.nh for v, r in brow.items()}
    base = lfa_expect(bd, bh, g, sources, groups)
    b_live = (base.metric != U64_MAX) & base.nh.any(axis=2)
    b_pc = popcount(base.nh | base.alt)
    S, G = len(sources), len(groups)
    changed = np.zeros((len(sets), S), dtype=np.uint32)
    unprot = np.zeros((len(sets), S), dtype=np.uint32)
    lost = np.zeros((len(sets), S), dtype=np.uint32)
    eg, em, eh, ea = [], [], [], []
    facts = {"alt_only": 0, "route": 0, "nbr_shrinks": 0, "tome_moves": 0, "changed_units": 0, "src_delta_empty": 0}
    for i, st in enumerate(sets):
        if st:
            rows = {v: o.run_spf(v, use_metric, [int(l) for l in st]) for v in need}
            fd, fh = {v: r.dist for v, r in rows.items()}, {v: r.nh for v, r in rows.items()}
            gf = failed_graph(g, st)
            f = lfa_expect(fd, fh, gf, sources, groups)
        else:
            fd, fh, gf, f = bd, bh, g, base
        route = (f.metric != base.metric) | (f.nh != base.nh).any(axis=2)
        ch = route | (f.alt != base.alt).any(axis=2)  # [S, G]
        live = (f.metric != U64_MAX) & f.nh.any(axis=2)
        one = live & (popcount(f.nh | f.alt) == 1)
        changed[i] = ch.sum(axis=1)
        unprot[i] = one.sum(axis=1)
        lost[i] = (b_live & (b_pc >= 2) & one).sum(axis=1)
        jj, kk = np.nonzero(ch)  # row-major: sources ascending, groups ascending inside a unit
        eg.append(kk.astype(np.uint32))
        em.append(f.metric[jj, kk])
        eh.append(f.nh[jj, kk])
        ea.append(f.alt[jj, kk])
        facts["alt_only"] += int((ch & ~route).sum())
        facts["route"] += int(route.sum())
        for j, s in enumerate(int(x) for x in sources):
            now, was = up_neighbors(gf, s), up_neighbors(g, s)
            facts["nbr_shrinks"] += now != was
            facts["tome_moves"] += any(int(fd[x][s]) != int(bd[x][s]) for x in now)
            if ch[j].any():
                facts["changed_units"] += 1
                facts["src_delta_empty"] += bool(np.array_equal(fd[s], bd[s]) and np.array_equal(fh[s], bh[s]))
    ptr = np.zeros(changed.size + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(changed.reshape(-1), dtype=np.uint64)
    nb = base.nh.shape[2]
    facts.update(sum=int(changed.sum()), lost=int(lost.sum()), unprotected=int(unprot.sum()),
                 max_per_unit=int(changed.max()) if changed.size else 0)
    e = Expect(changed, unprot, lost, ptr, np.concatenate(eg) if eg else np.zeros(0, np.uint32),
               np.concatenate(em) if em else np.zeros(0, np.uint64),
               np.concatenate(eh) if eh else np.zeros((0, nb), np.uint8),
               np.concatenate(ea) if ea else np.zeros((0, nb), np.uint8), (base.metric, base.nh, base.alt), facts)
    for a in (e.changed, e.unprotected, e.lost_backup, e.ptr, e.group, e.metric, e.nh, e.alt):
        a.setflags(write=False)
    _EXPECT[k] = e
    return e


def check(exp, got, counts=True):
    """The host form entry for entry: groups ascending inside a unit, the new entry."""
    changed, ptr, group, metric, nh, alt, unprot, lost = got[:8]
    np.testing.assert_array_equal(changed, exp.changed)
    np.testing.assert_array_equal(ptr, exp.ptr)
    np.testing.assert_array_equal(group, exp.group)
    np.testing.assert_array_equal(metric, exp.metric)
    w = exp.nh.shape[1]
    np.testing.assert_array_equal(nh[:, :w], exp.nh)
    np.testing.assert_array_equal(alt[:, :w], exp.alt)
    assert not nh[:, w:].any() and not alt[:, w:].any()  # zero past the graph's width
    if counts:
        np.testing.assert_array_equal(unprot, exp.unprotected)
        np.testing.assert_array_equal(lost, exp.lost_backup)


# --- 1. node failures ----------------------------------------------------------------------
NODE_FACTS = {"sum": 23496, "alt_only": 11589, "route": DENSE_FACTS["sum"][0], "lost": 1273, "unprotected": 15654,
              "nbr_shrinks": 89, "tome_moves": 11, "max_per_unit": 160}


def node_case(seed, use_metric):
    g = small_graph(seed)
    sets = T.node_failure_sets(g) if seed == 0 else T.node_failure_sets(g, range(0, 120, 3))
    _, dense = tables(seed)
    exp = oracle_whatif_lfa((("node", seed), "dense"), g, sets, SOURCES, dense, use_metric)
    return g, sets, dense, exp


def test_node_failures_seed0(eng, bfs_family):
    g, sets, dense, exp = node_case(0, True)
    assert exp.changed.size == 1800 and NODE_FACTS["route"] == 11907
    for name, want in NODE_FACTS.items():
        assert exp.facts[name] == want, (name, exp.facts)
    assert exp.facts["src_delta_empty"] == 0  # a node failure that moves an entry moves the source's row
    eng.set_graph(g)
    got = eng.whatif_lfa(sets, SOURCES, dense, True)
    ks = eng.last_kernels()
    assert "wlfa_mark" in ks and "wlfa_count" in ks and "wlfa_emit" in ks, ks
    check(exp, got)
    extras = sorted(closure(g, SOURCES) - set(SOURCES))
    assert got[8] == eng.whatif_sets(sets, SOURCES + extras, True)[1]
    # cap below the total: E2BIG from the host form too
    with pytest.raises(SpfError) as ei:
        eng.whatif_lfa(sets, SOURCES, dense, True, cap=exp.facts["sum"] - 1, want_counts=False)
    assert ei.value.code == E2BIG and "wlfa_emit" not in eng.last_kernels()


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("use_metric", [True, False], ids=["metric", "hops"])
def test_node_failures_other_seeds(eng, bfs_family, seed, use_metric):
    g, sets, dense, exp = node_case(seed, use_metric)
    assert exp.changed.size == 40 * len(SOURCES)
    for name in ("sum", "alt_only", "route", "lost", "unprotected", "nbr_shrinks", "max_per_unit"):
        assert exp.facts[name] > 0, (name, exp.facts)
    if seed != 1 and use_metric:  # 0 where every link costs the same: seed 1's unit metrics, every hop form
        assert exp.facts["tome_moves"] > 0, exp.facts
    eng.set_graph(g)
    check(exp, eng.whatif_lfa(sets, SOURCES, dense, use_metric))


# --- 2. singleton link sets -------------------------------------------------------------------
LINK_FACTS = {"sum": 6006, "alt_only": 3570, "changed_units": 637, "src_delta_empty": 144, "lost": 252}


def link_case():
    g = small_graph(0)
    _, dense = tables(0)
    links = [l for l in range(g.num_links) if g.edge_up[np.nonzero(g.link_id == l)[0][0]]][:80]
    sets = [[l] for l in links] + [[]]
    return g, links, sets, dense, oracle_whatif_lfa((("single", 0), "dense"), g, sets, SOURCES, dense, True)


def test_singleton_link_sets(eng, bfs_family):
    g, links, sets, dense, exp = link_case()
    assert exp.changed.size == 1215
    for name, want in LINK_FACTS.items():
        assert exp.facts[name] == want, (name, exp.facts)
    assert not exp.changed[-1].any()  # the empty set changes nothing
    eng.set_graph(g)
    got = eng.whatif_lfa(sets, SOURCES, dense, True)
    check(exp, got)
    np.testing.assert_array_equal(got[6][-1], exp.unprotected[-1])
    twice = eng.whatif_lfa([[l, l] for l in links] + [[]], SOURCES, dense, True)
    for a, b in zip(got[:8], twice[:8]):
        np.testing.assert_array_equal(a, b)


# --- 3. cross-check per set -------------------------------------------------------------------
def test_cross_check_against_set_graph(eng, bfs_family):
    """Consistency, not the reference: the base entries with a unit's entries applied equal
    lfa_routes on the graph with the set's links down."""
    g, sets, dense, exp = node_case(0, True)
    eng.set_graph(g)
    pick = [3, 16, 41, 77, 118]  # 16 is a source: it loses every neighbour
    got = eng.whatif_lfa([sets[i] for i in pick], SOURCES, dense, True)
    bm, bh, ba = eng.lfa_routes(SOURCES, dense, True, want_entries=False)[:3]
    S = len(SOURCES)
    for x, i in enumerate(pick):
        m, h, a = bm.copy(), bh.copy(), ba.copy()
        for j in range(S):
            lo, hi = int(got[1][x * S + j]), int(got[1][x * S + j + 1])
            m[j, got[2][lo:hi]] = got[3][lo:hi]
            h[j, got[2][lo:hi]] = got[4][lo:hi]
            a[j, got[2][lo:hi]] = got[5][lo:hi]
        eng.set_graph(failed_graph(g, sets[i]))
        fm, fh, fa = eng.lfa_routes(SOURCES, dense, True, want_entries=False)[:3]
        np.testing.assert_array_equal(m, fm)
        np.testing.assert_array_equal(h, fh)
        np.testing.assert_array_equal(a, fa)


# --- 4. two device slots, a caller-side split of the sets ---------------------------------
def test_two_device_slots_and_split_calls(eng, bfs_family):
    g, sets, dense, exp = node_case(1, True)
    two = SpfEngine([0, 0])
    try:
        two.set_graph(g)
        check(exp, two.whatif_lfa(sets, SOURCES, dense, True))
    finally:
        two.close()
    eng.set_graph(g)
    h = len(sets) // 2 + 3
    lo, hi = eng.whatif_lfa(sets[:h], SOURCES, dense, True), eng.whatif_lfa(sets[h:], SOURCES, dense, True)
    np.testing.assert_array_equal(np.concatenate([lo[0], hi[0]]), exp.changed)
    np.testing.assert_array_equal(np.concatenate([lo[1], hi[1][1:] + lo[1][-1]]), exp.ptr)
    for k, want in ((2, exp.group), (3, exp.metric), (4, exp.nh), (5, exp.alt)):
        np.testing.assert_array_equal(np.concatenate([lo[k], hi[k]]), want)
    for k, want in ((6, exp.unprotected), (7, exp.lost_backup)):
        np.testing.assert_array_equal(np.concatenate([lo[k], hi[k]]), want)


# --- 5. device form -----------------------------------------------------------------------
def test_device_form(eng, bfs_family):
    import torch

    g = small_graph(2)
    V, L = g.num_nodes, g.num_links
    _, dense = tables(2)
    # a malformed table (a member >= V, a last slice past n_group_nodes) and a link id >= L in
    # a set: the device form clamps the slices, the bad member is unreached, the bad link is none
    bad = dense + [[3, 50, V + 5], [7, 9, 11, 60]]
    good = dense + [[3, 50], [7, 9, 11, 60]]
    sets = T.node_failure_sets(g, range(0, 120, 3))
    bad_sets = [list(st) for st in sets]
    bad_sets[5] = bad_sets[5] + [L + 9]
    exp = oracle_whatif_lfa((("node", 2), "malformed"), g, sets, SOURCES, good, True)
    total = int(exp.ptr[-1])
    assert total > 0 and int(exp.changed[5].sum()) > 0
    eng.set_graph(g)
    S, G, nb, guard = len(SOURCES), len(bad), eng.nh_bytes + 1, 64
    units = len(sets) * S
    dev = torch.device("cuda", 0)

    def csr(lists, extra=0):
        p = np.zeros(len(lists) + 1, dtype=np.int32)
        p[1:] = np.cumsum([len(x) for x in lists])
        n = np.concatenate([np.asarray(x, dtype=np.int32) for x in lists])
        p[-1] += extra
        return torch.from_numpy(p).to(dev), torch.from_numpy(n).to(dev)

    d_sp, d_sl = csr(bad_sets)
    d_gp, d_gn = csr(bad, extra=50)
    d_s = torch.from_numpy(np.asarray(SOURCES, dtype=np.int32)).to(dev)
    extras = sorted(closure(g, SOURCES) - set(SOURCES))
    solved_want = eng.whatif_sets(sets, SOURCES + extras, True)[1]

    def guarded(count, dtype, fill):
        t = torch.full((count + 2 * guard,), fill, dtype=dtype, device=dev)
        return t, t.data_ptr() + guard * t.element_size(), fill

    def body(buf, view):
        t, _, fill = buf
        assert bool((t[:guard] == fill).all()) and bool((t[-guard:] == fill).all())  # nothing outside
        return t[guard:-guard].cpu().numpy().view(view)

    stream = torch.cuda.Stream(device=dev)

    def run(cap, want_entries=True):
        bufs = {"changed": guarded(units, torch.int32, -3), "unprot": guarded(units, torch.int32, -3),
                "lost": guarded(units, torch.int32, -3), "ptr": guarded(units + 1, torch.int64, -3),
                "group": guarded(max(cap, 1), torch.int32, -3), "metric": guarded(max(cap, 1), torch.int64, -3),
                "nh": guarded(max(cap, 1) * nb, torch.uint8, 0xEE), "alt": guarded(max(cap, 1) * nb, torch.uint8, 0xEE)}
        ent = [bufs[k][1] for k in ("ptr", "group", "metric", "nh", "alt")] if want_entries else [0] * 5
        args = (d_sp.data_ptr(), d_sl.data_ptr(), len(sets), d_sl.numel(), d_s.data_ptr(), S, d_gp.data_ptr(),
                d_gn.data_ptr(), G, d_gn.numel(), bufs["changed"][1], bufs["unprot"][1], bufs["lost"][1], *ent, cap, nb)
        code = 0
        try:
            tot, solved = eng.whatif_lfa_device(*args, stream=stream.cuda_stream)
        except SpfError as e:
            code = e.code
            tot, solved = eng.whatif_lfa_device(*args, stream=stream.cuda_stream, allow_overflow=True)
        stream.synchronize()
        out = {k: body(bufs[k], v) for k, v in (("changed", np.uint32), ("unprot", np.uint32), ("lost", np.uint32),
                                                ("ptr", np.uint64), ("group", np.uint32), ("metric", np.uint64),
                                                ("nh", np.uint8), ("alt", np.uint8))}
        return code, tot, solved, out

    def counts_ok(out):
        np.testing.assert_array_equal(out["changed"].reshape(exp.changed.shape), exp.changed)
        np.testing.assert_array_equal(out["unprot"].reshape(exp.changed.shape), exp.unprotected)
        np.testing.assert_array_equal(out["lost"].reshape(exp.changed.shape), exp.lost_backup)

    code, tot, solved, out = run(total)
    assert code == 0 and tot == total and solved == solved_want
    counts_ok(out)
    np.testing.assert_array_equal(out["ptr"], exp.ptr)
    ph, pa = out["nh"].reshape(-1, nb), out["alt"].reshape(-1, nb)
    w = exp.nh.shape[1]
    for u in range(units):  # the device form keeps the kernel's order: sort each unit by group
        a, e = int(exp.ptr[u]), int(exp.ptr[u + 1])
        k = np.argsort(out["group"][a:e], kind="stable")
        np.testing.assert_array_equal(out["group"][a:e][k], exp.group[a:e])
        np.testing.assert_array_equal(out["metric"][a:e][k], exp.metric[a:e])
        np.testing.assert_array_equal(ph[a:e][k][:, :w], exp.nh[a:e])
        np.testing.assert_array_equal(pa[a:e][k][:, :w], exp.alt[a:e])
        assert not ph[a:e, w:].any() and not pa[a:e, w:].any()
    assert (exp.group >= len(dense)).any()  # the two malformed groups change somewhere
    # cap below the total: E2BIG, counts and ptr filled, no entry written
    code1, tot1, _, out1 = run(total - 1)
    assert code1 == E2BIG and tot1 == total
    counts_ok(out1)
    np.testing.assert_array_equal(out1["ptr"], exp.ptr)
    assert (out1["group"] == np.uint32(2**32 - 3)).all()
    # counts only: ptr and the entry buffers untouched
    code2, tot2, _, out2 = run(0, want_entries=False)
    assert code2 == 0 and tot2 == total
    counts_ok(out2)
    assert (out2["ptr"] == np.uint64(2**64 - 3)).all()


# --- 6. every fixed capacity crossed -------------------------------------------------------
KNOBS = {
    "hash-small": {"OPENR_SPF_WLFA_HASH_SLOTS": "64"},  # units with more than 32 delta entries scan
    "no-hash": {"OPENR_SPF_WLFA_HASH_SLOTS": "0"},
    "list-overflow": {"OPENR_SPF_WLFA_CAND_CAP": "8"},
    "no-list": {"OPENR_SPF_WLFA_CAND_CAP": "0"},
    "bitmap-global": {"OPENR_SPF_WLFA_LDS_GROUPS": "100"},  # G = 162 > 100
    "slot-slices": {"OPENR_SPF_WLFA_SLOTS": "8"},  # a source with more than 8 edges takes several slices
    "all-low": {"OPENR_SPF_WLFA_HASH_SLOTS": "16", "OPENR_SPF_WLFA_CAND_CAP": "3", "OPENR_SPF_WLFA_LDS_GROUPS": "0",
                "OPENR_SPF_WLFA_SLOTS": "8"},
    "wave-groups": {"OPENR_SPF_ROUTES_SMALL_MAX": "1"},
    "lane-groups": {"OPENR_SPF_ROUTES_SMALL_MAX": "200"},
    "delta-rerun": {"OPENR_SPF_ROUTES_DELTA_CAP": "100"},  # the node delta overflows its first estimate
}


@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_capacities_crossed(eng, monkeypatch, knob):
    g, sets, dense, exp = node_case(0, True)
    assert exp.facts["max_per_unit"] > 8 and max(len(g.row(s)) for s in SOURCES) > 8
    for k, v in KNOBS[knob].items():
        monkeypatch.setenv(k, v)
    eng.set_graph(g)
    runs0 = eng.stats().spf_runs
    got = eng.whatif_lfa(sets, SOURCES, dense, True, cap=int(exp.ptr[-1]))
    check(exp, got)
    assert eng.stats().spf_runs - runs0 == got[8]  # a rerun of the sweep is counted once
    monkeypatch.undo()
    extras = sorted(closure(g, SOURCES) - set(SOURCES))
    assert got[8] == eng.whatif_sets(sets, SOURCES + extras, True)[1]


# --- 7. wide next hops ------------------------------------------------------------------------
def test_wide_next_hops(eng, monkeypatch):
    g = wide_graph()
    assert g.nh_bytes() == 10
    hub = g.id("0")
    srcs = [hub, g.id("5"), g.id("60")]
    groups = T.loopback_groups(g) + T.prefix_groups(g, [
        [g.id("5"), g.id("33"), g.id("70")], [g.id(str(i)) for i in range(1, 31)], range(g.num_nodes), []])
    sets = T.node_failure_sets(g, [g.id("6"), g.id("33"), g.id("70"), g.id("75"), hub])
    exp = oracle_whatif_lfa((("wide",), "wide"), g, sets, srcs, groups, True)
    assert exp.facts["sum"] > 0 and exp.facts["alt_only"] > 0 and exp.facts["nbr_shrinks"] > 0
    assert exp.nh[:, 8:].any() or exp.alt[:, 8:].any()  # bits past 64 change
    monkeypatch.setenv("OPENR_SPF_WLFA_SLOTS", "16")  # the hub's neighbours: five slices
    eng.set_graph(g)
    got = eng.whatif_lfa(sets, srcs, groups, True, nh_bytes=13)
    assert got[4].shape[1] == 13 and got[5].shape[1] == 13
    check(exp, got)
    monkeypatch.delenv("OPENR_SPF_WLFA_SLOTS")
    check(exp, eng.whatif_lfa(sets, srcs, groups, True, nh_bytes=13))


# --- 8. errors and empty inputs -----------------------------------------------------------------
def test_errors_and_empty_inputs(eng):
    g0 = small_graph(2)
    eng.set_graph(g0)
    V, L = g0.num_nodes, g0.num_links
    sets = T.node_failure_sets(g0, [3, 4])
    for groups in ([[0, V]], [[5, 5]], [[7, 2]]):
        with pytest.raises(SpfError) as ei:
            eng.whatif_lfa(sets, [0], groups)
        assert ei.value.code == EINVAL
    for bad in ([[L]], [[0, L + 3]]):
        with pytest.raises(SpfError) as ei:
            eng.whatif_lfa(bad, [0], [[1]])
        assert ei.value.code == EINVAL
    sp = np.array([0, 2, 1], dtype=np.uint32)  # a descending set_ptr
    sl = np.array([0, 1, 2], dtype=np.uint32)
    gp, gn = np.array([0, 1], dtype=np.uint32), np.array([1], dtype=np.uint32)
    src = np.array([0], dtype=np.uint32)
    ch = np.zeros((2, 1), dtype=np.uint32)
    gs = SpfGroups(1, _p(gp), _p(gn))
    assert eng._lib.openr_spf_whatif_lfa(eng._ctx, _p(sp), _p(sl), 2, _p(src), 1, USE_LINK_METRIC, ctypes.byref(gs),
                                         _p(ch), None, None, None, None) == EINVAL
    with pytest.raises(SpfError) as ei:
        eng.whatif_lfa(sets, [0], [[1]], nh_bytes=eng.nh_bytes - 1)
    assert ei.value.code == EINVAL
    ptr = np.zeros(3, dtype=np.uint64)
    d = WhatifLfa(_p(ptr), None, None, None, None, 0, eng.nh_bytes - 1)
    sp2 = np.array([0, 1, 2], dtype=np.uint32)
    assert eng._lib.openr_spf_whatif_lfa(eng._ctx, _p(sp2), _p(sl), 2, _p(src), 1, USE_LINK_METRIC, ctypes.byref(gs),
                                         _p(ch), None, None, ctypes.byref(d), None) == EINVAL
    with pytest.raises(SpfError) as ei:
        eng.whatif_lfa(sets, [V], [[1]])
    assert ei.value.code == EINVAL
    # empty inputs
    got = eng.whatif_lfa([], [0, 1], [[0]])
    assert got[0].shape == (0, 2) and got[1].tolist() == [0] and len(got[2]) == 0 and got[8] == 0
    got = eng.whatif_lfa(sets, [], [[0]])
    assert got[0].shape == (2, 0) and got[1].tolist() == [0] and got[8] == 0
    got = eng.whatif_lfa(sets, [0, 1], [])  # units without groups: ptr [units + 1], all zero
    assert not got[0].any() and not got[1].any() and len(got[2]) == 0 and not got[6].any() and not got[7].any()
    # a zero metric: the link-metric form is refused, the hop-count form runs and matches
    m = g0.metric.copy()
    m[int(np.nonzero(g0.edge_up != 0)[0][10])] = 0
    g = dataclasses.replace(g0, metric=m)
    eng.set_graph(g)
    _, dense = tables(2)
    with pytest.raises(SpfError) as ei:
        eng.whatif_lfa(sets, [0], dense, True)
    assert ei.value.code == ENOTSUP
    exp = oracle_whatif_lfa((("zero-metric",), "dense"), g, sets, [0, 8], dense, False)
    check(exp, eng.whatif_lfa(sets, [0, 8], dense, False))


def test_source_without_up_neighbor(eng):
    """A source behind down links only tests no neighbour: alt' is empty in every unit."""
    g0 = small_graph(0)
    x = 16
    g = failed_graph(g0, g0.link_id[g0.row_ptr[x]:g0.row_ptr[x + 1]].tolist())
    assert not up_neighbors(g, x) and g.distinct_neighbors(x)
    _, dense = tables(0)
    srcs = [x, 8, 24]
    sets = T.node_failure_sets(g, [8, 9, 40, 77])
    exp = oracle_whatif_lfa((("isolated", 0), "dense"), g, sets, srcs, dense, True)
    assert not exp.base[2][0].any() and exp.base[2][1].any()
    assert not exp.changed[:, 0].any() and exp.changed[:, 1:].any()  # x reaches itself only, before and after
    eng.set_graph(g)
    check(exp, eng.whatif_lfa(sets, srcs, dense, True))
