"""KSP2 (openr_spf_ksp2) on the edges of its branches vs the CPU oracle, edge for edge.

The KSP2 path branches on properties of the graph: uniform cost or not and which cost, the
distance tier of the general-metric second SPF, the repair kernel's three capacity exits, the
node count (repair off at powers of two, the tag budget of the level rows) and the tracer's
output limits (tokens, hops, arena entries on the DFS stack). test_gpu_parity.py reaches those
branches through environment switches on graphs of metric 1 or 1..9 with at most 400 nodes;
here every branch is put on both sides of its bound by the graph itself.

Every expectation is Oracle.kth_paths(s, d, 1 | 2), computed once per (recipe, cost) and
shared by both parametrisations of the module. Each construction's shape (how many first
paths, how long the second one) is asserted on the oracle side before the engine runs, so a
vacuous recipe cannot pass.

Whether the repair kernel kept a pair or handed it to the forward solve is read from the
`ksp_repair kept=<n> forward=<m>` line the KSP2 driver prints under OPENR_SPF_PROF=1.

What the constructions had to respect:
  * P disjoint chains of H hops put all their P * (H - 1) inner nodes and d into the affected
    set, far over its cap of 127, whatever the number of ignored links. The bound of 256
    ignored links is reached with P parallel links per hop (H affected nodes); the chains run
    too and are expected on the forward side.
  * No shortest path of a random graph comes near V * w_max / 2, which a u32-tier distance
    with bit 31 set needs; second paths the long way round a ring of 220 nodes do.
  * copy_row16_tagged never runs at any cost: ksp_use_d16() is false for every launch.
  * The affected-set bound is checked through the kept / forward counts only: one node over
    the cap leaves the repair's queue slot 127 unwritten, so a library that took such a pair
    would read an arbitrary node id there.
"""
import dataclasses
import functools
import os
import re

import numpy as np
import pytest

import wide_cases as W
from openr_amd import topology as T
from openr_amd.engine import E2BIG, SpfEngine, SpfError, decode_paths
from oracle import Oracle
from test_gpu_parity import (check_ksp2_against_oracle, fabric_with_faults, hub_graph, random_graph,
                             skip_edge_graphs)

pytestmark = pytest.mark.gpu

BAD = 0xFFFFFFFF


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
_WANT = {}


def want(key, g, pairs):
    """((k1 paths, k2 paths), ...) of the oracle for the pairs, computed once per key."""
    if key not in _WANT:
        o = Oracle(g)
        _WANT[key] = tuple((o.kth_paths(s, d, 1), o.kth_paths(s, d, 2)) for s, d in pairs)
    return _WANT[key]


def ksp2_equals(eng, g, pairs, exp, tok_cap=256):
    """The engine's answer for the pairs, held against the oracle's edge for edge."""
    eng.set_graph(g)
    got = eng.ksp2([p[0] for p in pairs], [p[1] for p in pairs], tok_cap)
    assert len(got) == len(exp) == len(pairs)
    for (s, d), (k1, k2), (w1, w2) in zip(pairs, got, exp):
        assert k1 == w1, ("k1", s, d)
        assert k2 == w2, ("k2", s, d)
    return got


def with_cost(g1, c):
    """A unit-cost graph with every metric (down edges included) set to c."""
    assert (g1.metric == 1).all()
    return dataclasses.replace(g1, metric=np.full_like(g1.metric, c))


def links_of(g, paths):
    return sorted({int(g.link_id[e]) for p in paths for e in p})


def traced_distances(g, pairs, exp):
    """The distances the tracer compares on the way to each dest: the base distance of every
    pair with a first path, the second SPF's of every pair with a second path."""
    o = Oracle(g)
    base, second = [], []
    for (s, d), (k1, k2) in zip(pairs, exp):
        if k1:
            base.append(int(o.run_spf(s, True).dist[d]))
            assert base[-1] == sum(int(g.metric[e]) for e in k1[0])
        if k2:
            second.append(int(o.run_spf(s, True, links_of(g, k1)).dist[d]))
            assert second[-1] == sum(int(g.metric[e]) for e in k2[0])
    return base, second


def named(V):
    """Node names whose order is not the id order (the pathLinks order goes by name)."""
    return [f"n{(i * 7919) % 10007:05d}-{i}" for i in range(V)]


BLOB = 40


def unit_graph(V, links, blob=False):
    """Unit-cost graph of the links. `blob`: 40 more nodes, a random connected multigraph
    that hangs on node 0 by one link, so that calls on the graph have ordinary pairs whose
    second SPF is worth solving; no shortest path between the first V nodes enters it."""
    links = list(links)
    if blob:
        rng = np.random.default_rng(V)
        links += [(0, V)] + [(V + int(rng.integers(0, i)), V + i) for i in range(1, BLOB)]
        links += [tuple(int(x) for x in V + rng.choice(BLOB, 2, replace=False)) for _ in range(50)]
        V += BLOB
    assert V & (V - 1), V  # never a power of two: the repair kernel is off there
    m = np.ones(len(links), dtype=np.uint64)
    return T.csr_from_links(named(V), np.array(links), m, m)


def ordinary_pairs(g, seed, n, without):
    """n pairs of a unit_graph with its blob: every other one inside the blob."""
    rng = np.random.default_rng(seed)
    V = g.num_nodes
    out = []
    while len(out) < n:
        lo = V - BLOB if len(out) & 1 else 0
        p = (int(rng.integers(lo, V)), int(rng.integers(lo, V)))
        if p != without:
            out.append(p)
    return out


# --- 1. uniform cost 1, 7 and 2^31 - 1 ------------------------------------------------------------
COSTS = {"c1": 1, "c7": 7, "cmax": W.METRIC_MAX}


@functools.lru_cache(maxsize=None)
def uniform_recipes():
    """((name, unit-cost graph, pairs, 2^32 expected at cmax), ...)."""
    rng = np.random.default_rng(41)
    out = []
    # one pod: only pairs with a fabric switch (ids 288 .. 295) at one end have second paths
    gf, ovl = fabric_with_faults(8)
    fsw = range(288, 296)
    assert all(gf.names[f].startswith("2-") for f in fsw)
    pairs = [(f, int(d)) for f in fsw for d in rng.integers(0, gf.num_nodes, 10)]
    pairs += [(int(s), f) for f in fsw for s in rng.integers(0, gf.num_nodes, 6)]
    pairs += [(int(a), int(b)) for a, b in rng.integers(0, gf.num_nodes, (60, 2))]
    pairs += [(int(rng.integers(0, gf.num_nodes)), int(x)) for x in ovl[:6]]
    pairs += [(int(x), int(rng.integers(0, gf.num_nodes))) for x in ovl[:6]] + [(9, 9)]
    out.append(("fabric-faults", gf, tuple(pairs), True))
    # two pods with the same kinds of faults: second paths between random pairs
    g2 = T.fabric(288 + 2 * 56)
    down = rng.choice(g2.num_links, 60, replace=False)
    sinks = rng.choice(g2.num_nodes, 12, replace=False)
    g2 = g2.patched([], [], down, [0] * len(down), sinks, [1] * len(sinks))
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, g2.num_nodes, (150, 2))]
    out.append(("fabric-2-pods-faults", g2, tuple(pairs), True))
    gr = random_graph(97, 120, 260, 1, p_ovl=0.08, p_down=0.08, p_par=0.2)
    out.append(("random", gr, tuple((s, d) for s in range(0, gr.num_nodes, 17) for d in range(gr.num_nodes)), True))
    gh = hub_graph(23, V=220, L=500)
    pairs = [(h, int(d)) for h in range(3) for d in rng.integers(0, gh.num_nodes, 30)]
    pairs += [(int(s), h) for h in range(3) for s in rng.integers(0, gh.num_nodes, 20)]
    out.append(("hubs", gh, tuple(pairs), True))
    for i, gs in enumerate(skip_edge_graphs()):
        out.append((f"skip-{i}", gs, tuple((s, d) for s in range(gs.num_nodes) for d in range(gs.num_nodes)), False))
    return tuple(out)


@pytest.fixture(params=[{}, {"OPENR_SPF_KSP_REPAIR": "0"}, {"OPENR_SPF_KSP_TL": "0"}, {"OPENR_SPF_KSP_TAG": "0"}],
                ids=["default", "forward", "record-rows", "untagged"])
def ksp_mode(request, monkeypatch):
    for k, v in request.param.items():
        monkeypatch.setenv(k, v)
    return request.param


@pytest.mark.parametrize("cname", list(COSTS))
def test_uniform_cost(eng, bfs_family, ksp_mode, cname):
    """Scaling a uniform cost keeps every tie: the paths at c are the paths at 1. With c != 1
    the repair's level division, the trace's level x cost distances and the cost-tight tests
    of the pathLinks lists and of the repair run with a real factor; at 2^31 - 1 the traced
    distances pass 2^32 from the third hop on."""
    c = COSTS[cname]
    for name, g1, pairs, wide in uniform_recipes():
        g = with_cost(g1, c)
        exp1 = want(("uniform", name, 1), g1, pairs)
        exp = want(("uniform", name, c), g, pairs)
        assert exp == exp1
        assert any(k2 for _, k2 in exp) and any(not k2 for _, k2 in exp) and any(k1 for k1, _ in exp)
        if wide:
            assert any(len(k1) > 1 for k1, _ in exp)
        if wide and c == W.METRIC_MAX:
            base, second = traced_distances(g, pairs[:40], exp[:40])
            assert max(base) > 2**32 and max(second) > 2**32, (max(base), max(second))
        ksp2_equals(eng, g, pairs, exp)
        ks = eng.last_kernels()
        repair = bfs_family[0] == "code" and not ksp_mode  # tagged level rows and the lists: code family
        assert ("ksp_repair_kernel" in ks) == repair, (name, ks)
        assert not any(k.startswith(("fringe_kernel", "rounds_kernel")) for k in ks), ks  # uniform cost: BFS plans


# --- 2. weighted graphs: the u32 and u64 tiers of the second SPF --------------------------------
def typed(bfs_family, width):
    return f"{bfs_family[1]}_kernel<{width}>"


def ring_graph(V=220, chords=6, w_lo=250, w_hi=297):
    """long_line_graph's sizes (V * w_hi just under 0xFFFF) closed to a ring: a pair's second
    path goes round the other way, more than half of V * w_max for pairs close together."""
    rng = np.random.default_rng(59)
    links = [(i, (i + 1) % V) for i in range(V)]
    while len(links) < V + chords:
        a = int(rng.integers(0, V - 6))
        links.append((a, a + int(rng.integers(2, 6))))
    m_uv = rng.integers(w_lo, w_hi + 1, len(links)).astype(np.uint64)
    m_vu = rng.integers(w_lo, w_hi + 1, len(links)).astype(np.uint64)
    return T.csr_from_links([f"r{i:04d}" for i in range(V)], np.array(links), m_uv, m_vu)


@functools.lru_cache(maxsize=None)
def weighted_case(kind, kname):
    """(graph, pairs, K). "random": metrics up to 64 on 120 nodes; no shortest path of such a
    graph comes near V * w_max / 2, so its u32 tier stays below bit 31. "ring": second paths
    the long way round a ring of the long line's sizes (wide_cases.K_TOP), which do."""
    if kind == "random":
        g1 = random_graph(300, 120, 300, 64, p_ovl=0.05, p_down=0.05, p_par=0.1)
        assert g1.num_nodes == 120 and W.w_max_of(g1) == 64 == int(g1.metric.max())
        K = {"K1": 1, "K_U32": W.K_MID, "K_U64": W.k_wide(64)}[kname]
        rng = np.random.default_rng(43)
        pairs = [(int(a), int(b)) for a, b in rng.integers(0, 120, (150, 2))] + [(3, 3)]
    else:
        g1 = ring_graph()
        assert g1.num_nodes == 220 and W.w_max_of(g1) == 297 == int(g1.metric.max())  # wide_cases.K_TOP's graph sizes
        K = {"K1": 1, "K_U32": W.K_TOP, "K_U64": W.K_TOP + 1}[kname]
        rng = np.random.default_rng(47)
        pairs = [(0, 9), (9, 0), (100, 130)] + [(int(a), int(b)) for a, b in rng.integers(0, 220, (60, 2))] + [(3, 3)]
    return g1, W.scaled(g1, K), tuple(pairs), K


@pytest.mark.parametrize("kname", ["K1", "K_U32", "K_U64"])
@pytest.mark.parametrize("kind", ["random", "ring"])
def test_weighted_tiers(eng, bfs_family, kind, kname):
    """General metrics: the second SPF is the fringe or the rounds kernel with per-pair ignore
    sets and a target bound, and the tracer compares dist[u] + w with dist[v] in the row's own
    width. Paths do not move with K; the tier that ran is read from the launch trace."""
    g1, g, pairs, K = weighted_case(kind, kname)
    span = g.num_nodes * W.w_max_of(g)
    assert W.w_max_of(g) == W.w_max_of(g1) * K <= W.METRIC_MAX
    width = "u64" if kname == "K_U64" else "u32"
    assert (span >= W.U32_LIMIT) == (width == "u64"), span
    exp1 = want(("weighted", kind, 1), g1, pairs)
    exp = want(("weighted", kind, K), g, pairs)
    assert exp == exp1
    assert sum(1 for _, k2 in exp if k2) >= 20 and any(not k1 for k1, _ in exp)
    base, second = traced_distances(g, pairs, exp)
    if kname == "K_U64" and kind == "ring":  # one step over the threshold: the ring's distances in u64 rows
        assert 2**31 < max(second) < 2**32
    elif kname == "K_U64":
        assert max(base) > 2**32 and max(second) > 2**32
    elif kname == "K_U32" and kind == "ring":
        assert 2**31 < max(second) < 2**32 and sum(1 for x in second if x > 2**31) >= 20  # bit 31 set, u32 rows
    elif kname == "K_U32":
        assert 2**16 < max(second) < 2**31
    ksp2_equals(eng, g, pairs, exp)
    ks = eng.last_kernels()
    assert ks.count(typed(bfs_family, width)) >= 2, ks  # the base solve and the second SPFs
    assert not any(k.endswith("<u32>" if width == "u64" else "<u64>") for k in ks), ks
    assert "ksp_repair_kernel" not in ks


# --- 3. the repair kernel's hand-backs, each on both sides of its bound -------------------------
def chain(links, nodes, copies=1):
    for a, b in zip(nodes, nodes[1:]):
        links.extend([(a, b)] * copies)


@functools.lru_cache(maxsize=None)
def ignored_links_graph(P, H, parallel):
    """s and d joined over H hops P times, plus one chain of H + 2 hops: P first paths, P * H
    ignored links, one second path. `parallel`: the P paths share their H - 1 inner nodes over
    P parallel links per hop, so the affected set is those nodes and d (H nodes); else they are
    P disjoint chains, whose every inner node is affected (P * (H - 1) + 1 nodes)."""
    links, nxt = [], 2
    if parallel:
        chain(links, [0] + list(range(nxt, nxt + H - 1)) + [1], P)
        nxt += H - 1
    else:
        for _ in range(P):
            chain(links, [0] + list(range(nxt, nxt + H - 1)) + [1])
            nxt += H - 1
    chain(links, [0] + list(range(nxt, nxt + H + 1)) + [1])
    return unit_graph(nxt + H + 1, links, blob=True), (0, 1)


@functools.lru_cache(maxsize=None)
def affected_cap_graph(n):
    """s - hub, a detour s - a - b - hub, n leaves on the hub, leaf 1 - leaf 0. For (s, leaf 0)
    the first path s - hub - leaf 0 takes the hub's only pathLink: the hub and every leaf are
    affected (n + 1 nodes); the second path is s - a - b - hub - leaf 1 - leaf 0."""
    s, hub, a, b, leaf = 0, 1, 2, 3, 4
    links = [(s, hub), (s, a), (a, b), (b, hub)] + [(hub, leaf + i) for i in range(n)] + [(leaf + 1, leaf)]
    return unit_graph(4 + n, links, blob=True), (s, leaf)


@functools.lru_cache(maxsize=None)
def count_byte_graph(m):
    """s - m mids - y, then y - z, y - w, w - z. For (s, z), y has m base pathLinks and loses
    one (the first path's mid): the repair counts it in a byte that holds up to 127."""
    s, y, z, w, mid = 0, 1, 2, 3, 4
    links = [(y, z), (y, w), (w, z)]
    for i in range(m):
        links += [(s, mid + i), (mid + i, y)]
    return unit_graph(4 + m, links, blob=True), (s, z)


@functools.lru_cache(maxsize=None)
def funnel_graph(m):
    """s - a - m mids - y - z with the detours s - p - q - a and y - w - z. For (s, z) the first
    path takes a's only pathLink: a, every mid, y (all m of its pathLinks lost, one count
    each), w and z are affected: m + 4 nodes."""
    s, a, y, z, w, p, q, mid = 0, 1, 2, 3, 4, 5, 6, 7
    links = [(s, a), (s, p), (p, q), (q, a), (y, z), (y, w), (w, z)]
    for i in range(m):
        links += [(a, mid + i), (mid + i, y)]
    return unit_graph(7 + m, links, blob=True), (s, z)


# name: (builder, kept by the repair kernel, k = 1 path count, k = 1 hops, k = 2 hops, affected nodes)
HANDBACKS = {
    # kRpHash / 2 = 256 ignored links at most
    "ignored-256": (lambda: ignored_links_graph(16, 16, True), True, 16, 16, 18, 16),
    "ignored-272": (lambda: ignored_links_graph(16, 17, True), False, 16, 17, 19, 17),
    "ignored-255": (lambda: ignored_links_graph(15, 17, True), True, 15, 17, 19, 17),
    # the same counts over disjoint chains: the affected set (241 / 257 / 241 nodes) passes its cap
    # whatever the link count
    "chains-256": (lambda: ignored_links_graph(16, 16, False), False, 16, 16, 18, 241),
    "chains-272": (lambda: ignored_links_graph(16, 17, False), False, 16, 17, 19, 257),
    "chains-255": (lambda: ignored_links_graph(15, 17, False), False, 15, 17, 19, 241),
    # kRpMaxCap = 127 affected nodes at most
    "affected-127": (lambda: affected_cap_graph(126), True, 1, 2, 5, 127),
    "affected-128": (lambda: affected_cap_graph(127), False, 1, 2, 5, 128),
    # a node's base pathLinks are counted in a byte: 127 at most
    "pathlinks-127": (lambda: count_byte_graph(127), True, 1, 3, 4, 2),
    "pathlinks-128": (lambda: count_byte_graph(128), False, 1, 3, 4, 2),
    # 123 counted losses at one node, 127 affected nodes
    "funnel-123": (lambda: funnel_graph(123), True, 1, 4, 7, 127),
}


def affected_set(g, s, ignore):
    """The nodes whose distance from s grows or is lost when the links are ignored."""
    o = Oracle(g)
    a, b = o.run_spf(s, True).dist, o.run_spf(s, True, ignore).dist
    return int((a != b).sum())


def repair_line(capfd):
    m = re.findall(r"^ksp_repair kept=(\d+) forward=(\d+)$", capfd.readouterr().err, re.M)
    assert len(m) == 1, m
    return int(m[0][0]), int(m[0][1])


@pytest.mark.parametrize("c", [1, 7], ids=["c1", "c7"])
@pytest.mark.parametrize("case", list(HANDBACKS))
def test_repair_handbacks(eng, bfs_family, monkeypatch, capfd, case, c):
    """The boundary pair among ordinary pairs of its graph in one call (one chunk: repaired and
    forward rows side by side), and the same call without it: the difference of the two
    `ksp_repair` lines is the way the boundary pair went."""
    build, kept, n1, h1, h2, n_aff = HANDBACKS[case]
    g1, pair = build()
    g = with_cost(g1, c)
    assert g.num_nodes & (g.num_nodes - 1)
    others = ordinary_pairs(g, 53, 36, pair)
    pairs = others[:18] + [pair] + others[18:]
    exp = want(("handback", case, c), g, tuple(pairs))
    k1, k2 = exp[18]
    assert [len(p) for p in k1] == [h1] * n1 and [len(p) for p in k2] == [h2]
    assert affected_set(g, pair[0], links_of(g, k1)) == n_aff
    assert sum(1 for _, b in exp if b) >= 10
    exp_others = exp[:18] + exp[19:]
    tok_cap = 512  # 16 paths of 17 hops are 289 tokens
    monkeypatch.setenv("OPENR_SPF_PROF", "1")
    capfd.readouterr()
    ksp2_equals(eng, g, others, exp_others, tok_cap)
    without = repair_line(capfd)
    ksp2_equals(eng, g, pairs, exp, tok_cap)
    ks = eng.last_kernels()
    both = repair_line(capfd)
    if bfs_family[0] == "code":
        assert "ksp_repair_kernel" in ks, ks
        assert sum(without) > 0
        assert (both[0] - without[0], both[1] - without[1]) == ((1, 0) if kept else (0, 1)), (without, both)
    else:  # u64 level rows: no tags, no repair
        assert "ksp_repair_kernel" not in ks and without == both == (0, 0)


# --- 4. gates on V --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gate_case(V):
    g = random_graph(5, V, int(1.6 * V), 1, 0.03, 0.03, 0.05)
    assert g.num_nodes == V
    rng = np.random.default_rng(V)
    return g, tuple((int(a), int(b)) for a, b in rng.integers(0, V, (70, 2)))


@pytest.mark.parametrize("V", [255, 256, 257])
def test_repair_is_off_at_a_power_of_two(eng, bfs_family, V):
    """V = 2^n leaves no level value free for the repair's "no level" mark: the forward solve runs."""
    g, pairs = gate_case(V)
    got = check_ksp2_against_oracle(eng, g, list(pairs))
    ks = eng.last_kernels()
    assert sum(1 for _, k2 in got if k2) >= 20
    assert ("ksp_repair_kernel" in ks) == (bfs_family[0] == "code" and V != 256), ks


@pytest.mark.parametrize("V,chunk", [(8200, "7"), (16400, None)], ids=["3-tags-10-chunks", "no-tag-bits"])
def test_tag_budget(eng, bfs_family, monkeypatch, V, chunk):
    """14 level bits leave 3 tags: ten chunks of 7 pairs zero the level rows three more times.
    15 level bits leave none: the rows are written untagged."""
    if chunk:
        monkeypatch.setenv("OPENR_SPF_KSP_CHUNK", chunk)
    g, pairs = gate_case(V)
    got = check_ksp2_against_oracle(eng, g, list(pairs))
    ks = eng.last_kernels()
    assert sum(1 for _, k2 in got if k2) >= 20
    assert ("ksp_repair_kernel" in ks) == (bfs_family[0] == "code" and V == 8200), ks


# --- 5. output limits -----------------------------------------------------------------------------
def tokens_needed(paths):
    return 1 + sum(1 + len(p) for p in paths)


def rows_equal(tok, exp_paths):
    return decode_paths(tok) == exp_paths


def test_token_limit(eng, bfs_family):
    """A row holds its paths at exactly the tokens they need and is marked at one fewer, each
    of a pair's two rows on its own; a marked k = 1 row marks the pair's k = 2 row."""
    g, (s, leaf) = affected_cap_graph(21)
    hub = 1
    pairs = [(s, leaf)] + [(s, leaf + j) for j in range(2, 11)] + [(s, hub), (s, s)]
    exp = want(("tokens",), g, tuple(pairs))
    need = [(tokens_needed(k1), tokens_needed(k2)) for k1, k2 in exp]
    # leaf 0: 2 hops, then 5; the other leaves have one link and no second path; the hub: 1 hop, then 3
    assert need[0] == (4, 7) and need[1:10] == [(4, 1)] * 9 and need[10] == (3, 5) and need[11] == (1, 1)
    eng.set_graph(g)
    src, dst = [p[0] for p in pairs], [p[1] for p in pairs]
    # exact fit of the largest row
    t1, t2 = eng.ksp2_tokens(src, dst, 7)
    for i, (k1, k2) in enumerate(exp):
        assert rows_equal(t1[i], k1) and rows_equal(t2[i], k2), i
    # one token fewer: that row alone
    with pytest.raises(SpfError) as ei:
        eng.ksp2_tokens(src, dst, 6)
    assert ei.value.code == E2BIG and "DFS stack" in str(ei.value) and "tokens" in str(ei.value)
    t1, t2 = eng.ksp2_tokens(src, dst, 6, allow_overflow=True)
    assert t2[0, 0] == BAD and rows_equal(t1[0], exp[0][0])
    for i in range(1, len(pairs)):
        assert rows_equal(t1[i], exp[i][0]) and rows_equal(t2[i], exp[i][1]), i
    # the k = 1 rows of the leaves fit exactly; of the k = 2 rows the two with paths do not fit
    t1, t2 = eng.ksp2_tokens(src, dst, 4, allow_overflow=True)
    for i in range(len(pairs)):
        assert rows_equal(t1[i], exp[i][0]), i
        assert t2[i, 0] == BAD if i in (0, 10) else rows_equal(t2[i], []), i
    # ... and one fewer: the k = 1 row is marked, and with it the k = 2 row (include/openr_spf.h)
    t1, t2 = eng.ksp2_tokens(src, dst, 3, allow_overflow=True)
    for i in range(10):
        assert t1[i, 0] == BAD and t2[i, 0] == BAD, i
    assert rows_equal(t1[10], exp[10][0]) and t2[10, 0] == BAD
    assert t1[11, 0] == 0 and t2[11, 0] == 0


def test_hop_limit(eng, bfs_family):
    """255 hops are traced, 256 are marked, in either direction of a 300-node line."""
    V = 300
    g = unit_graph(V, [(i, i + 1) for i in range(V - 1)])
    pairs = [(0, 255), (0, 256), (299, 44), (299, 43), (5, 200), (7, 7)]
    exp = want(("line300",), g, tuple(pairs))
    assert [[len(p) for p in k1] for k1, _ in exp] == [[255], [256], [255], [256], [195], []]
    assert not any(k2 for _, k2 in exp)
    eng.set_graph(g)
    src, dst = [p[0] for p in pairs], [p[1] for p in pairs]
    with pytest.raises(SpfError) as ei:
        eng.ksp2_tokens(src, dst, 300)
    assert ei.value.code == E2BIG and "255 hops" in str(ei.value)
    t1, t2 = eng.ksp2_tokens(src, dst, 300, allow_overflow=True)
    for i in (0, 2, 4, 5):
        assert rows_equal(t1[i], exp[i][0]) and t2[i, 0] == 0, i
    for i in (1, 3):
        assert t1[i, 0] == BAD and t2[i, 0] == BAD, i


@functools.lru_cache(maxsize=None)
def layered_graph(layers, last):
    """s, `layers` layers of 32 nodes with every link between consecutive layers, d on `last`
    nodes of the last layer. The trace's DFS stack holds `last` pathLinks of d, 32 of every
    layer node but the first layer's, and 1 of that: last + 32 * (layers - 1) + 1."""
    W_ = 32
    node = lambda l, i: 2 + l * W_ + i
    links = [(0, node(0, i)) for i in range(W_)]
    for l in range(layers - 1):
        links += [(node(l, i), node(l + 1, j)) for i in range(W_) for j in range(W_)]
    links += [(node(layers - 1, i), 1) for i in range(last)]
    return unit_graph(2 + layers * W_, links)


@pytest.mark.parametrize("layers,last,entries", [(31, 32, 993), (32, 31, 1024), (32, 32, 1025)],
                         ids=["993", "1024-exact", "1025-marked"])
def test_arena_limit(eng, bfs_family, layers, last, entries):
    """The third reason for a marked row: more than 1024 pathLinks on the DFS stack. The count
    is the same from d back to s, but for the layer next to d: it holds `last` of them."""
    g = layered_graph(layers, last)
    assert last + 32 * (layers - 1) + 1 == entries and g.num_nodes == 2 + 32 * layers
    pairs = [(0, 1), (0, 2 + 32 * (layers - 1)), (2, 1), (1, 0), (40, 2 + 32 * 5 + 3)]
    exp = want(("layered", layers, last), g, tuple(pairs))
    assert [len(p) for p in exp[0][0]] == [layers + 1] * last and exp[0][1] == []
    assert [len(p) for p in exp[3][0]] == [layers + 1] * last and exp[3][1] == []
    assert all(k1 for k1, _ in exp) and [len(p) for p in exp[4][1]] == [8] * 32
    tok_cap = 1 + 32 * (1 + 33) + 11  # the 32 paths of 33 hops and some room
    eng.set_graph(g)
    src, dst = [p[0] for p in pairs], [p[1] for p in pairs]
    if entries <= 1024:
        got = ksp2_equals(eng, g, pairs, exp, tok_cap)
        assert len(got[0][0]) == last
        return
    with pytest.raises(SpfError) as ei:
        eng.ksp2_tokens(src, dst, tok_cap)
    assert ei.value.code == E2BIG and "1024 pathLinks on the DFS stack" in str(ei.value)
    t1, t2 = eng.ksp2_tokens(src, dst, tok_cap, allow_overflow=True)
    for i in (0, 3):  # (s, d) and (d, s); include/openr_spf.h: a marked k = 1 row marks the k = 2 row
        assert t1[i, 0] == BAD and t2[i, 0] == BAD, i
    for i in (1, 2, 4):
        assert rows_equal(t1[i], exp[i][0]) and rows_equal(t2[i], exp[i][1]), i
