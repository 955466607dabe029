"""GPU parity: the HIP engine (through the C-ABI) vs the CPU oracle, bit-exact.

Compared per solve: u64 distances, next-hop bitsets (= NodeSpfResult::nextHops),
and pathLinks rebuilt from the tight-edge mask in the reference's order
(settle order of the predecessor, then linksFromNode order). KSP paths are
compared edge-for-edge. Full-size configs are checked through size-independent
properties (grid Manhattan distances, next-hop closure) plus oracle samples.
"""
import numpy as np
import pytest

import golden_cases as G
from openr_amd import topology as T
from openr_amd.engine import E2BIG, EINVAL, ENOTSUP, SpfEngine, SpfError
from openr_amd.spf_result import get_kth_paths, materialize, tight_in_edges
from oracle import Oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True, params=[("code", "fringe"), ("lvl", "rounds")],
                ids=["code-fringe", "lvl-rounds"])
def bfs_family(request):
    """Every parity test runs on both uniform-cost kernel families (spf_bfs.hip and
    spf_bfs_lvl.hip) and both general-metric kernels (spf_fringe.hip, spf_rounds.hip);
    production picks per graph by sampled depth (spf_capi.hip)."""
    import os

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


def check_against_oracle(eng, g, sources, use_metric=True, ignore=None, check_pathlinks=True):
    """Both engine paths vs the oracle: the plain solve (dist + next hops; the
    specialised non-generic kernel variants) and, with check_pathlinks, the tight-edge
    solve (generic variants, pathLinks rebuilt in the reference's order)."""
    eng.set_graph(g)
    o = Oracle(g)
    assert eng.nh_bytes == o.nh_bytes
    runs = [o.run_spf(int(s), use_metric, ignore[i] if ignore else None) for i, s in enumerate(sources)]
    dist, nh, _ = eng.solve(sources, use_metric, want_nh=True, want_tight=False, ignore=ignore)
    for i, s in enumerate(sources):
        np.testing.assert_array_equal(dist[i], runs[i].dist, err_msg=f"dist src={s}")
        np.testing.assert_array_equal(nh[i], runs[i].nh, err_msg=f"nh src={s}")
    if check_pathlinks:
        dist2, nh2, tight = eng.solve(sources, use_metric, want_nh=True, want_tight=True, ignore=ignore)
        np.testing.assert_array_equal(dist2, dist)
        np.testing.assert_array_equal(nh2, nh)
        for i, s in enumerate(sources):
            run = runs[i]
            pe = tight_in_edges(g, dist[i], tight[i])
            for v in np.nonzero(run.reachable())[0].tolist():
                want = run.pl_edge[run.pl_ptr[v] : run.pl_ptr[v + 1]].tolist()
                assert pe.get(v, []) == want, f"pathLinks src={s} v={v}"
    return dist, nh


# --- reference test topologies ------------------------------------------------
@pytest.mark.parametrize("case", G.load()["cases"], ids=lambda c: c["name"])
def test_reference_cases_all_sources(eng, case):
    g = G.build(case)
    for use_metric in (True, False):
        check_against_oracle(eng, g, list(range(g.num_nodes)), use_metric)


@pytest.mark.parametrize("case", G.spf_cases(), ids=lambda c: c["name"])
def test_reference_spf_expectations_on_gpu(eng, case):
    g = G.build(case)
    eng.set_graph(g)
    for exp in case["spf"]:
        s = g.id(exp["src"])
        dist, nh, tight = eng.solve([s], True, want_tight=True)
        res = materialize(g, s, dist[0], nh[0], eng.neighbor_map(s), tight[0])
        if exp.get("unreachable"):
            assert exp["dst"] not in res
        else:
            assert res[exp["dst"]].metric == exp["metric"]
            assert res[exp["dst"]].next_hops == set(exp["nh"])


@pytest.mark.parametrize("case", G.kth_cases(), ids=lambda c: c["name"])
def test_kth_paths_match_oracle(eng, case):
    g = G.build(case)
    eng.set_graph(g)
    o = Oracle(g)
    for exp in case["kth"]:
        s, d = g.id(exp["src"]), g.id(exp["dst"])
        got = get_kth_paths(eng, s, d, exp["k"])
        assert got == o.kth_paths(s, d, exp["k"])
        assert len(got) == exp["num_paths"]


def test_kth_paths_all_pairs_small(eng):
    case = [c for c in G.load()["cases"] if c["name"].startswith("DecisionTest.ParallelAdjRing")][0]
    g = G.build(case)
    eng.set_graph(g)
    o = Oracle(g)
    for s in range(g.num_nodes):
        for d in range(g.num_nodes):
            for k in (1, 2, 3):
                assert get_kth_paths(eng, s, d, k) == o.kth_paths(s, d, k), (s, d, k)


# --- grids --------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 6, 8, 10, 12, 14, 16, 32])
def test_grid_all_sources(eng, n):
    g = T.build_csr(T.grid_dbs(n, test_form=True))
    V = n * n
    dist, _ = check_against_oracle(eng, g, list(range(V)), True, check_pathlinks=(n <= 16))
    a = np.arange(V)
    manhattan = np.abs(a[:, None] % n - a[None, :] % n) + np.abs(a[:, None] // n - a[None, :] // n)
    assert np.array_equal(dist.astype(np.int64), manhattan)


def test_grid100_all_sources_properties(eng):
    """G100 (BASELINE config): all 10k sources; distances = Manhattan; next hops valid."""
    n = 100
    g = T.grid_fast(n)
    eng.set_graph(g)
    V = n * n
    a = np.arange(V)
    owner = g.edge_owner()
    for lo in range(0, V, 2500):
        srcs = np.arange(lo, min(V, lo + 2500))
        dist, nh, _ = eng.solve(srcs, True)
        manhattan = np.abs(srcs[:, None] % n - a[None, :] % n) + np.abs(srcs[:, None] // n - a[None, :] // n)
        assert np.array_equal(dist.astype(np.int64), manhattan)
        bits = np.unpackbits(nh[..., 0], axis=-1, bitorder="little").reshape(len(srcs), V, 8).sum(-1)
        self_mask = srcs[:, None] == a[None, :]
        assert bits[self_mask].max() == 0
        assert bits[~self_mask].min() >= 1 and bits[~self_mask].max() <= 2
    o = Oracle(g)
    sample = [0, 99, 4950, 5050, 9900, 9999, 1234, 7777]
    check_against_oracle(eng, g, sample, True, check_pathlinks=True)
    _ = o


# --- fabrics / WAN -------------------------------------------------------------
@pytest.mark.parametrize("block", ["512", "256"])
@pytest.mark.parametrize("faithful", [False, True])
def test_fabric_small_all_sources(eng, monkeypatch, faithful, block):
    """All sources of a 3-pod fabric; the code family's high-degree classes on 512-thread
    workgroups (default) and on the 256-thread shape (OPENR_SPF_BFS_BLOCK=256)."""
    monkeypatch.setenv("OPENR_SPF_BFS_BLOCK", block)
    g = T.fabric(288 + 3 * 56, faithful=faithful)  # 3 pods, max degree 84
    check_against_oracle(eng, g, list(range(g.num_nodes)), True, check_pathlinks=False)
    check_against_oracle(eng, g, list(range(0, g.num_nodes, 37)), True, check_pathlinks=True)


@pytest.mark.parametrize("rows", ["1", "7"])
def test_sliced_class_in_chunks(eng, monkeypatch, rows):
    """The code family's sliced class (degree-84 SSWs / FSWs) run in chunks of a few solves
    with one chunk's slice scratch (OPENR_SPF_SLICE_ROWS forces the chunk size the launcher
    otherwise derives from its 512 MiB budget): every row as the oracle's, with
    duplicate sliced sources and a partial last chunk."""
    monkeypatch.setenv("OPENR_SPF_BFS_FAMILY", "code")
    monkeypatch.setenv("OPENR_SPF_WIDE", "0")  # the sliced pass (the wide pass has no scratch)
    monkeypatch.setenv("OPENR_SPF_SLICE_ROWS", rows)
    g = T.fabric(288 + 3 * 56)
    srcs = list(range(g.num_nodes)) + list(range(0, 60, 3))
    check_against_oracle(eng, g, srcs, True, check_pathlinks=False)


@pytest.mark.parametrize("wide", ["1", "2", "0"])
def test_fabric_5000_sample(eng, monkeypatch, bfs_family, wide):
    """Degree-84 sources: the wide pass (512 / 256 threads) and the sliced pass (code
    family; the lvl family has its own 32-bit slices)."""
    monkeypatch.setenv("OPENR_SPF_WIDE", wide)
    g = T.fabric(5000)
    assert g.num_nodes == 4992 and g.num_links == 56448
    check_against_oracle(eng, g, [0, 287, 288, 289, 1000, 4991, 2500], True, check_pathlinks=True)
    eng.solve([0, 300, 1000], True)  # two degree-84 sources (an SSW, an FSW) and an RSW
    assert ("bfs_wide_kernel" in eng.last_kernels()) == (wide != "0" and bfs_family[0] == "code")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_wan_weighted(eng, seed):
    g = T.wan(256, 768, 64, seed=seed, parallel_fraction=0.02)
    check_against_oracle(eng, g, list(range(g.num_nodes)), True, check_pathlinks=False)
    check_against_oracle(eng, g, list(range(0, 256, 17)), True, check_pathlinks=True)
    check_against_oracle(eng, g, list(range(0, 256, 5)), False, check_pathlinks=True)


# --- randomized graphs with overload / down links / parallel links -------------
def random_graph(seed, V, L, max_metric, p_ovl=0.1, p_down=0.05, p_par=0.1):
    rng = np.random.default_rng(seed)
    names = [f"n{rng.integers(0, 10**6)}-{i}" for i in range(V)]  # name order != id order
    links = []
    for i in range(1, V):
        links.append((int(rng.integers(0, i)), i))  # spanning tree
    while len(links) < L:
        a, b = rng.integers(0, V, 2)
        if a != b:
            links.append((int(a), int(b)))
    for _ in range(int(p_par * L)):
        links.append(links[int(rng.integers(0, len(links)))])
    m_uv = rng.integers(1, max_metric + 1, len(links)).astype(np.uint64)
    m_vu = rng.integers(1, max_metric + 1, len(links)).astype(np.uint64)
    up = (rng.random(len(links)) >= p_down).astype(np.uint8)
    ovl = (rng.random(V) < p_ovl).astype(np.uint8)
    return T.csr_from_links(names, np.array(links), m_uv, m_vu, ovl, up)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("max_metric", [1, 3, 50])
def test_random_graphs(eng, seed, max_metric):
    g = random_graph(seed, 60 + 40 * seed, 150 + 90 * seed, max_metric)
    srcs = list(range(g.num_nodes))
    check_against_oracle(eng, g, srcs, True)
    check_against_oracle(eng, g, srcs, False)


@pytest.mark.parametrize("block", ["64", "128", "256"])
def test_rounds_kernel_block_sizes(eng, monkeypatch, block):
    """The rounds kernel (spf_rounds.hip) at each workgroup size it picks from: one
    wavefront per solve (barrier-free rounds) and 2 / 4 wavefronts sharing a solve's
    frontier with a workgroup barrier per round (small batches). Weighted WAN with
    parallel links, random graphs with overloads / down links, ignore sets, pathLinks."""
    monkeypatch.setenv("OPENR_SPF_GENERAL", "rounds")
    monkeypatch.setenv("OPENR_SPF_ROUNDS_BLOCK", block)
    g = T.wan(256, 768, 64, seed=3, parallel_fraction=0.05)
    check_against_oracle(eng, g, list(range(g.num_nodes)), True, check_pathlinks=False)
    check_against_oracle(eng, g, list(range(0, 256, 9)), True, check_pathlinks=True)
    rng = np.random.default_rng(int(block))
    srcs = list(range(0, 256, 4))
    ign = [sorted(rng.choice(g.num_links, 3, replace=False).tolist()) for _ in srcs]
    check_against_oracle(eng, g, srcs, True, ignore=ign, check_pathlinks=True)
    for seed in (1, 2):
        r = random_graph(500 + seed, 150, 420, 40, p_ovl=0.1, p_down=0.05, p_par=0.1)
        check_against_oracle(eng, r, list(range(r.num_nodes)), True)


def test_uniform_nonunit_cost(eng):
    g = random_graph(11, 120, 300, 1)
    g.metric[:] = 7  # BFS kernel with cost 7
    check_against_oracle(eng, g, list(range(g.num_nodes)), True)


@pytest.mark.parametrize("seed", range(4))
def test_ignore_sets(eng, seed):
    g = random_graph(100 + seed, 150, 400, 9 if seed % 2 else 1)
    rng = np.random.default_rng(seed)
    srcs = rng.integers(0, g.num_nodes, 64).tolist()
    ignore = [sorted(set(rng.integers(0, g.num_links, int(rng.integers(0, 12))).tolist())) for _ in srcs]
    check_against_oracle(eng, g, srcs, True, ignore=ignore)


def test_whatif_single_link_sweep(eng):
    """Per-link-failure sweep from one source (runSpf(src, true, {link}))."""
    g = T.wan(128, 384, 64, seed=5)
    srcs = [3] * g.num_links
    ignore = [[l] for l in range(g.num_links)]
    check_against_oracle(eng, g, srcs, True, ignore=ignore, check_pathlinks=False)


def test_large_metrics_use_u64_distances(eng):
    V = 40
    names = [str(i) for i in range(V)]
    links = np.array([(i, i + 1) for i in range(V - 1)] + [(0, V - 1)])
    m = np.full(len(links), 0x7FFFFFFF, dtype=np.uint64)
    m[-1] = 0x7FFFFFF0  # asymmetric closing edge -> not uniform, general kernel
    g = T.csr_from_links(names, links, m, m)
    dist, _ = check_against_oracle(eng, g, list(range(V)), True)
    assert int(dist.max()) > 0xFFFFFFFF


@pytest.mark.parametrize("full", ["0", "1"])
def test_deep_bfs_u8_overflow_rerun(eng, monkeypatch, full):
    """BFS deeper than 253 levels: a u8-level ring pass flags it and the full-order pass
    re-runs it from the list (or the full-order variant runs alone)."""
    monkeypatch.setenv("OPENR_SPF_BFS_FULL", full)
    V = 700
    names = [f"p{i:04d}" for i in range(V)]
    links = np.array([(i, i + 1) for i in range(V - 1)])
    g = T.csr_from_links(names, links)
    dist, _ = check_against_oracle(eng, g, [0, 1, 350, 699, 100, 0], True, check_pathlinks=True)
    assert int(dist[0, V - 1]) == V - 1
    srcs = [0, 699, 5]
    ignore = [[10], [], [600]]
    check_against_oracle(eng, g, srcs, True, ignore=ignore)


@pytest.mark.parametrize("case", ["grid", "depth", "half", "overload-down"])
def test_wave_pass(eng, monkeypatch, capfd, case):
    """The wave pass (one wavefront per solve, delta-coded rows staged in LDS; picked for
    small batches of graphs whose rows have <= 4 edges within 127 ids of their node),
    forced on and checked against the oracle, including both re-run paths: a chain
    deeper than 253 levels and a forced tiny queue half. OPENR_SPF_PROF makes the pass
    report itself on stderr (proof that it ran)."""
    monkeypatch.setenv("OPENR_SPF_BFS_FAMILY", "lvl")
    monkeypatch.setenv("OPENR_SPF_BFS_WAVE", "1")
    monkeypatch.setenv("OPENR_SPF_PROF", "1")
    n = 40
    names = [f"g{r:02d}-{c:02d}" for r in range(n) for c in range(n)]
    links = [(r * n + c, r * n + c + 1) for r in range(n) for c in range(n - 1)]
    links += [(r * n + c, (r + 1) * n + c) for r in range(n - 1) for c in range(n)]
    ovl = up = None
    srcs = list(range(0, n * n, 7))
    if case == "depth":
        tail = 300
        names += [f"z{i:03d}" for i in range(tail)]
        links += [(n * n + i, n * n + i + 1) for i in range(tail - 1)]
        srcs = [0, n * n - 1, n * n, n * n + tail - 1, n * n + 150, 20 * n + 20]
    if case == "half":
        monkeypatch.setenv("OPENR_SPF_WAVE_QHALF", "16")
    if case == "overload-down":
        rng = np.random.default_rng(3)
        ovl = (rng.random(n * n) < 0.05).astype(np.uint8)
        up = (rng.random(len(links)) > 0.05).astype(np.uint8)
    g = T.csr_from_links(names, np.array(links), overloaded=ovl, link_up=up)
    dist, _ = check_against_oracle(eng, g, srcs, True, check_pathlinks=False)
    if case == "depth":
        assert int(dist[2, n * n + 299]) == 299
    assert "bfs_wave:" in capfd.readouterr().err


def test_wave_pass_not_applicable(eng, monkeypatch, capfd):
    """A neighbour more than 127 ids away (here: a 200 x 200 grid, rows +-200) leaves the
    wave pass off even when forced; the lean / generic passes serve the graph."""
    monkeypatch.setenv("OPENR_SPF_BFS_FAMILY", "lvl")
    monkeypatch.setenv("OPENR_SPF_BFS_WAVE", "1")
    monkeypatch.setenv("OPENR_SPF_PROF", "1")
    g = T.grid_fast(200)
    check_against_oracle(eng, g, [0, 199, 20100, 39999], True, check_pathlinks=False)
    assert "bfs_wave:" not in capfd.readouterr().err


def test_lean_pass_depth_overflow(eng, monkeypatch, capfd, bfs_family):
    """The lean ELL pass (graphs with <= 4 edges per row too big for the full-order queue,
    sampled depth under the u8 limit): a 70 x 70 grid plus a separate 300-node chain whose
    nodes no depth sample starts from. Chain sources run deeper than 253 levels: the lean
    pass flags them at level 254 and the u16 full-order pass re-runs them. (With
    OPENR_SPF_PROF the lean pass reports itself on stderr: proof that it ran.)"""
    monkeypatch.setenv("OPENR_SPF_PROF", "1")
    monkeypatch.setenv("OPENR_SPF_BFS_WAVE", "0")  # small batch: the wave pass would take it
    n, tail = 70, 300
    names = [f"g{r:02d}-{c:02d}" for r in range(n) for c in range(n)] + [f"z{i:03d}" for i in range(tail)]
    links = [(r * n + c, r * n + c + 1) for r in range(n) for c in range(n - 1)]
    links += [(r * n + c, (r + 1) * n + c) for r in range(n - 1) for c in range(n)]
    links += [(n * n + i, n * n + i + 1) for i in range(tail - 1)]
    g = T.csr_from_links(names, np.array(links))
    srcs = [0, n * n - 1, n * n, n * n + tail - 1, n * n + 10, 35 * n + 35]
    dist, _ = check_against_oracle(eng, g, srcs, True, check_pathlinks=False)
    assert int(dist[2, n * n + tail - 1]) == tail - 1
    assert ("bfs_ell:" in capfd.readouterr().err) == (bfs_family[0] == "lvl")


def test_lean_pass_half_overflow(eng, monkeypatch, capfd, bfs_family):
    """A level wider than a queue half in the lean pass (forced onto a graph whose sampled
    width would otherwise keep it on the generic ring): the solve is flagged and re-run."""
    monkeypatch.setenv("OPENR_SPF_LEAN_FORCE", "1")
    monkeypatch.setenv("OPENR_SPF_PROF", "1")
    monkeypatch.setenv("OPENR_SPF_BFS_WAVE", "0")
    chain, depth = 100, 11
    names = [f"c{i:03d}" for i in range(chain)] + [f"t{i:05d}" for i in range(1, 2 ** (depth + 1) - 1)]
    links = [(i, i + 1) for i in range(chain - 1)]
    tid = lambda i: chain - 1 if i == 0 else chain - 1 + i  # heap index -> node id (root = last chain node)
    links += [(tid(i), tid(c)) for i in range(2 ** depth - 1) for c in (2 * i + 1, 2 * i + 2)]
    g = T.csr_from_links(names, np.array(links))
    check_against_oracle(eng, g, [0, 50, chain - 1, chain + 5, len(names) - 1], True, check_pathlinks=False)
    assert ("bfs_ell:" in capfd.readouterr().err) == (bfs_family[0] == "lvl")


def test_ring_overflow_rerun_list(eng, monkeypatch):
    """A ring too small for the frontier (forced: levels of ~1000 nodes on a random
    expander) flags every solve; the full-order pass re-runs them from the list."""
    g = random_graph(5, 3000, 6000, 1, p_ovl=0.02)
    srcs = list(range(0, g.num_nodes, 11))
    eng.set_graph(g)
    d1, n1, _ = eng.solve(srcs, True)
    monkeypatch.setenv("OPENR_SPF_RING_CAP", "256")
    check_against_oracle(eng, g, srcs, True, check_pathlinks=False)
    d2, n2, _ = eng.solve(srcs, True)
    assert np.array_equal(d1, d2) and np.array_equal(n1, n2)
    monkeypatch.setenv("OPENR_SPF_WIDE", "0")  # the sliced pass: its (solve, slice) units ring
    hub = hub_graph(4)  # sliced classes: every (solve, slice) unit is listed on its own
    check_against_oracle(eng, hub, list(range(hub.num_nodes)), True, check_pathlinks=False)


# --- edge cases -------------------------------------------------------------
def test_single_node_and_isolated(eng):
    g = T.build_csr([T.AdjacencyDatabase("a", []), T.AdjacencyDatabase("b", [])])
    eng.set_graph(g)
    dist, nh, _ = eng.solve([0, 1], True)
    assert dist.tolist() == [[0, 2**64 - 1], [2**64 - 1, 0]]
    assert nh.max() == 0


def test_duplicate_sources_in_batch(eng):
    g = T.grid_fast(7)
    eng.set_graph(g)
    dist, nh, _ = eng.solve([5, 5, 5, 10], True)
    assert np.array_equal(dist[0], dist[1]) and np.array_equal(nh[0], nh[2])


def test_empty_batch(eng):
    g = T.grid_fast(3)
    eng.set_graph(g)
    dist, nh, _ = eng.solve([], True)
    assert dist.shape == (0, 9)


def test_nh_bytes_too_small(eng):
    g = T.fabric(288 + 56)
    eng.set_graph(g)
    with pytest.raises(SpfError) as ei:
        eng.solve([0], True, nh_bytes=1)
    assert ei.value.code == EINVAL


def test_wider_nh_output_zero_padded(eng):
    g = T.grid_fast(5)
    eng.set_graph(g)
    d1, nh1, _ = eng.solve(range(25), True)
    d2, nh2, _ = eng.solve(range(25), True, nh_bytes=4)
    assert np.array_equal(d1, d2)
    assert np.array_equal(nh2[..., 0], nh1[..., 0]) and nh2[..., 1:].max() == 0


def test_spf_runs_counter(eng):
    g = T.grid_fast(4)
    eng.set_graph(g)
    before = eng.stats().spf_runs
    eng.solve(range(16), True)
    assert eng.stats().spf_runs - before == 16


def hub_graph(seed, V=300, L=700, hub_deg=(40, 75, 130)):
    """Random unit-metric graph plus hubs of distinct degree 40 / 75 / 130: every source
    class (nibble .. 32-bit sliced next-hop sets, 2-5 slices) is present in one batch."""
    g0 = random_graph(seed, V, L, 1, p_ovl=0.05, p_down=0.03, p_par=0.05)
    rng = np.random.default_rng(seed + 1000)
    links = []
    src_of = g0.edge_owner()
    for e in range(g0.num_dir_edges):  # keep the random graph's links (one direction each)
        u, v = int(src_of[e]), int(g0.col[e])
        if u < v:
            links.append((u, v))
    for h, d in enumerate(hub_deg):
        for v in rng.choice(np.arange(len(hub_deg), V), d, replace=False):
            links.append((h, int(v)))
    links = np.array(links)
    m = np.ones(len(links), dtype=np.uint64)
    ovl = np.zeros(V, dtype=np.uint8)
    ovl[rng.integers(len(hub_deg), V, 6)] = 1
    names = [f"h{rng.integers(0, 10**6)}-{i}" for i in range(V)]
    return T.csr_from_links(names, links, m, m, ovl)


@pytest.mark.parametrize("wide", ["1", "0"])
@pytest.mark.parametrize("seed", [0, 1])
def test_source_classes_and_sliced_next_hops(eng, monkeypatch, seed, wide):
    """Every source class in one batch; sets wider than 29 bits through the wide pass (2-5
    words per node) or the sliced pass (OPENR_SPF_WIDE=0); with an ignore set always the
    sliced pass."""
    monkeypatch.setenv("OPENR_SPF_WIDE", wide)
    g = hub_graph(seed)
    assert g.max_distinct_degree() > 128  # 5 slices of 32 next-hop bits for the largest hub
    srcs = list(range(g.num_nodes))
    check_against_oracle(eng, g, srcs, True)
    check_against_oracle(eng, g, srcs, False)
    rng = np.random.default_rng(seed)
    sub = [0, 1, 2] + rng.integers(3, g.num_nodes, 40).tolist()
    ignore = [sorted(set(rng.integers(0, g.num_links, int(rng.integers(0, 20))).tolist())) for _ in sub]
    check_against_oracle(eng, g, sub, True, ignore=ignore)


@pytest.mark.parametrize("wide", ["1", "0"])
def test_sliced_next_hops_wide_stride(eng, bfs_family, monkeypatch, wide):
    """Sliced next-hop sets (code family: the wide pass's word streams or 29-bit chunks
    merged into bytes; lvl family: 32-bit slices) into a caller stride wider than the set:
    the set's bytes as the oracle's, every byte past them zero."""
    monkeypatch.setenv("OPENR_SPF_WIDE", wide)
    g = hub_graph(4)
    eng.set_graph(g)
    o = Oracle(g)
    nb = eng.nh_bytes
    srcs = list(range(0, g.num_nodes, 3))
    dist, nh, _ = eng.solve(srcs, True, nh_bytes=nb + 5)
    assert nh.shape[-1] == nb + 5
    for i, s in enumerate(srcs):
        run = o.run_spf(int(s), True, None)
        np.testing.assert_array_equal(dist[i], run.dist, err_msg=f"dist src={s}")
        np.testing.assert_array_equal(nh[i][:, :nb], run.nh, err_msg=f"nh src={s}")
    assert not nh[:, :, nb:].any()


def test_source_classes_device_partition(eng):
    """solve_device partitions on the GPU: same results as the host-buffer solve."""
    import torch

    g = hub_graph(3)
    eng.set_graph(g)
    srcs = np.random.default_rng(3).permutation(g.num_nodes).astype(np.int32)
    dist_h, nh_h, _ = eng.solve(srcs.astype(np.uint32), True)
    dev = torch.device("cuda", 0)
    d_src = torch.from_numpy(srcs).to(dev)
    d_dist = torch.empty((len(srcs), g.num_nodes), dtype=torch.int64, device=dev)
    d_nh = torch.empty((len(srcs), g.num_nodes, eng.nh_bytes), dtype=torch.uint8, device=dev)
    eng.solve_device(d_src.data_ptr(), len(srcs), d_dist.data_ptr(), d_nh.data_ptr(), eng.nh_bytes, True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_dist.cpu().numpy().view(np.uint64), dist_h)
    np.testing.assert_array_equal(d_nh.cpu().numpy(), nh_h)


# --- per-link-failure what-if sweep (openr_spf_whatif) -----------------------
def whatif_oracle(g, links, sources, use_metric=True):
    """changed[i, j] = nodes whose dist or next-hop set differ between runSpf(s) and
    runSpf(s, {links[i]}) on the oracle."""
    o = Oracle(g)
    base = {s: o.run_spf(int(s), use_metric) for s in sources}
    out = np.zeros((len(links), len(sources)), dtype=np.uint32)
    for i, l in enumerate(links):
        for j, s in enumerate(sources):
            r = o.run_spf(int(s), use_metric, [int(l)])
            b = base[s]
            out[i, j] = int(np.count_nonzero((r.dist != b.dist) | np.any(r.nh != b.nh, axis=1)))
    return out


@pytest.fixture(params=["group", "group-lds", "group-d32", "group-cap", "group-cap1", "group-items", "incr", "solve"])
def whatif_mode(request, monkeypatch):
    """What-if units repaired from LDS-staged base rows per (source, link chunk) workgroup
    (default: graph read from global memory, u16 distances when they fit; or the graph
    staged in LDS too; or u32 distances forced where u16 would fit; no mode reaches u64, the
    graph's V * w_max alone does: tests/test_gpu_dist_tiers.py), per-unit incremental repair, or full
    re-solves. group-cap: 3 dirty slots per wave, so most units are re-solved; group-cap1:
    1 slot, so nearly every affected unit takes the seeded re-solve (the rounds kernel
    starting from the base rows); group-items: 1 item per workgroup and 60 % of each
    source's links in the queue's tail as third-size chunks (the split's bounds)."""
    mode = request.param
    if mode == "group-items":
        monkeypatch.setenv("OPENR_SPF_WHATIF_IPW", "1")
        monkeypatch.setenv("OPENR_SPF_WHATIF_TAILFRAC", "60")
        monkeypatch.setenv("OPENR_SPF_WHATIF_TAILDIV", "3")
    if mode == "group-lds":
        monkeypatch.setenv("OPENR_SPF_WHATIF_LDSG", "1")
    if mode == "group-d32":
        monkeypatch.setenv("OPENR_SPF_WHATIF_D32", "1")
    if mode in ("group-cap", "group-cap1"):
        monkeypatch.setenv("OPENR_SPF_WHATIF_CAP", "3" if mode == "group-cap" else "1")
    monkeypatch.setenv("OPENR_SPF_WHATIF", mode.split("-")[0])
    return request.param


def long_line_graph(seed, V=220, chords=24, w_lo=250, w_hi=297):
    """A line of V nodes plus a few short chords, metrics up to w_hi with V * w_hi just under
    0xFFFF: shortest distances reach ~60 000, the top of the rounds kernel's packed u16 rows."""
    rng = np.random.default_rng(seed)
    names = [f"l{i:04d}" for i in range(V)]
    links = [(i, i + 1) for i in range(V - 1)]
    while len(links) < V - 1 + chords:
        a = int(rng.integers(0, V - 6))
        links.append((a, a + int(rng.integers(2, 6))))  # short detours: distances stay long
    m_uv = rng.integers(w_lo, w_hi + 1, len(links)).astype(np.uint64)
    m_vu = rng.integers(w_lo, w_hi + 1, len(links)).astype(np.uint64)
    up = np.ones(len(links), np.uint8)
    ovl = np.zeros(V, np.uint8)
    return T.csr_from_links(names, np.array(links), m_uv, m_vu, ovl, up)


def test_rounds_long_distances(eng, monkeypatch):
    """Distances near 0xFFFF (V * w_max = 65 340; the what-if repair's u16 rows hold them):
    all-sources solves with pathLinks, ignore sets, and a what-if sweep whose affected units
    all take the seeded re-solve (1 dirty slot), against the oracle."""
    monkeypatch.setenv("OPENR_SPF_GENERAL", "rounds")
    g = long_line_graph(5)
    assert g.num_nodes * int(g.metric.max()) < 0xFFFF
    o = Oracle(g)
    assert max(int(d) for d in o.run_spf(0, True).dist if d != np.iinfo(np.uint64).max) > 40000
    check_against_oracle(eng, g, list(range(g.num_nodes)), True)
    rng = np.random.default_rng(7)
    srcs = list(range(0, g.num_nodes, 5))
    ign = [sorted(rng.choice(g.num_links, 2, replace=False).tolist()) for _ in srcs]
    check_against_oracle(eng, g, srcs, True, ignore=ign)
    monkeypatch.setenv("OPENR_SPF_WHATIF_CAP", "1")
    eng.set_graph(g)
    links = list(range(g.num_links))
    sources = list(range(0, g.num_nodes, 11))
    changed, _ = eng.whatif(links, sources, True)
    np.testing.assert_array_equal(changed, whatif_oracle(g, links, sources, True))


@pytest.mark.parametrize("seed,max_metric", [(0, 64), (1, 1), (2, 7)])
def test_whatif_sweep_matches_oracle(eng, seed, max_metric, whatif_mode):
    g = random_graph(300 + seed, 120, 300, max_metric, p_ovl=0.05, p_down=0.05, p_par=0.1)
    eng.set_graph(g)
    links = list(range(g.num_links))
    sources = list(range(0, g.num_nodes, 3))
    changed, solved = eng.whatif(links, sources, True)
    want = whatif_oracle(g, links, sources, True)
    np.testing.assert_array_equal(changed, want)
    # only units whose link is on a shortest path are solved, plus the base solves
    assert len(sources) <= solved < len(links) * len(sources) + len(sources)
    c2, _ = eng.whatif(links[::5], sources[:7], False)
    np.testing.assert_array_equal(c2, whatif_oracle(g, links[::5], sources[:7], False))


def test_whatif_wan_sample_and_device_form(eng, whatif_mode):
    import torch

    g = T.wan(1000, 3000, 64, seed=1)
    eng.set_graph(g)
    rng = np.random.default_rng(11)
    links = np.sort(rng.choice(g.num_links, 40, replace=False)).astype(np.uint32)
    sources = np.sort(rng.choice(g.num_nodes, 12, replace=False)).astype(np.uint32)
    changed, _ = eng.whatif(links, sources, True)
    np.testing.assert_array_equal(changed, whatif_oracle(g, links, sources, True))
    dev = torch.device("cuda", 0)
    d_l = torch.from_numpy(links.astype(np.int32)).to(dev)
    d_s = torch.from_numpy(sources.astype(np.int32)).to(dev)
    d_c = torch.full((len(links), len(sources)), -1, dtype=torch.int32, device=dev)
    eng.whatif_device(d_l.data_ptr(), len(links), d_s.data_ptr(), len(sources), d_c.data_ptr(), True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint32), changed)


def check_delta_rows(g, links, sources, use_metric, changed, ptr, node, dist, nh):
    """Every unit's delta entries against explicit oracle rows: the nodes whose distance
    or next-hop set differ between runSpf(s) and runSpf(s, {link}), ascending, with the
    re-solve's distance and next-hop bytes."""
    o = Oracle(g)
    base = {int(s): o.run_spf(int(s), use_metric) for s in sources}
    nb = nh.shape[1]
    for i, l in enumerate(links):
        for j, s in enumerate(sources):
            u = i * len(sources) + j
            r = o.run_spf(int(s), use_metric, [int(l)])
            b = base[int(s)]
            ch = np.nonzero((r.dist != b.dist) | np.any(r.nh != b.nh, axis=1))[0]
            a, e = int(ptr[u]), int(ptr[u + 1])
            assert e - a == len(ch) == changed[i, j], (l, s)
            np.testing.assert_array_equal(node[a:e], ch)
            np.testing.assert_array_equal(dist[a:e], r.dist[ch])
            want = np.zeros((len(ch), nb), dtype=np.uint8)
            want[:, : min(nb, r.nh.shape[1])] = r.nh[ch, :nb]
            np.testing.assert_array_equal(nh[a:e], want)


@pytest.mark.parametrize("seed,max_metric", [(0, 64), (1, 1)])
def test_whatif_delta_matches_oracle_rows(eng, seed, max_metric, whatif_mode):
    """openr_spf_whatif_delta on random graphs with overloads, down and parallel links:
    per unit, the changed nodes with their new distance (UINT64_MAX when the failure cuts
    them off) and next-hop bytes, entry for entry against oracle re-solves, in every
    what-if mode (repair overlays, seeded re-solves, full re-solves + row compare), with
    link metrics and hop counts, and with next-hop entries wider than the graph's."""
    g = random_graph(310 + seed, 110, 240, max_metric, p_ovl=0.05, p_down=0.05, p_par=0.1)
    eng.set_graph(g)
    links = list(range(g.num_links))
    sources = list(range(0, g.num_nodes, 5))
    changed, ptr, node, dist, nh, _ = eng.whatif_delta(links, sources, True)
    np.testing.assert_array_equal(changed, whatif_oracle(g, links, sources, True))
    check_delta_rows(g, links, sources, True, changed, ptr, node, dist, nh)
    assert (dist == np.uint64(2**64 - 1)).any()  # some failures cut nodes off (tree links)
    c2, p2, n2, d2, h2, _ = eng.whatif_delta(links[::4], sources[:6], False, nh_bytes=eng.nh_bytes + 5)
    check_delta_rows(g, links[::4], sources[:6], False, c2, p2, n2, d2, h2)


def test_whatif_delta_device_form_and_cap(eng, whatif_mode):
    """The device form's CSR (entries in the repair's order) holds the host form's entries
    (node ids ascending); a cap below the total returns E2BIG with changed and ptr filled."""
    import torch

    g = T.wan(1000, 3000, 64, seed=1)
    eng.set_graph(g)
    rng = np.random.default_rng(12)
    links = np.sort(rng.choice(g.num_links, 60, replace=False)).astype(np.uint32)
    sources = np.sort(rng.choice(g.num_nodes, 10, replace=False)).astype(np.uint32)
    changed, ptr, node, dist, nh, _ = eng.whatif_delta(links, sources, True)
    total = int(ptr[-1])
    assert total == int(changed.sum())
    nb = eng.nh_bytes
    units = len(links) * len(sources)
    dev = torch.device("cuda", 0)
    d_l = torch.from_numpy(links.astype(np.int32)).to(dev)
    d_s = torch.from_numpy(sources.astype(np.int32)).to(dev)
    d_c = torch.zeros((len(links), len(sources)), dtype=torch.int32, device=dev)
    d_ptr = torch.zeros(units + 1, dtype=torch.int64, device=dev)
    d_node = torch.zeros(total, dtype=torch.int32, device=dev)
    d_dist = torch.zeros(total, dtype=torch.int64, device=dev)
    d_nh = torch.zeros((total, nb), dtype=torch.uint8, device=dev)
    got, _ = eng.whatif_delta_device(d_l.data_ptr(), len(links), d_s.data_ptr(), len(sources), d_c.data_ptr(),
                                     d_ptr.data_ptr(), d_node.data_ptr(), d_dist.data_ptr(), d_nh.data_ptr(), total, nb)
    assert got == total
    np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint32), changed)
    p = d_ptr.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(p, ptr)
    pn = d_node.cpu().numpy().view(np.uint32)
    pd = d_dist.cpu().numpy().view(np.uint64)
    ph = d_nh.cpu().numpy()
    for u in range(units):
        a, e = int(p[u]), int(p[u + 1])
        k = np.argsort(pn[a:e], kind="stable")
        np.testing.assert_array_equal(pn[a:e][k], node[a:e])
        np.testing.assert_array_equal(pd[a:e][k], dist[a:e])
        np.testing.assert_array_equal(ph[a:e][k], nh[a:e])
    # cap below the total: E2BIG, counts and ptr still right
    d_c.zero_()
    d_ptr.zero_()
    got2, _ = eng.whatif_delta_device(d_l.data_ptr(), len(links), d_s.data_ptr(), len(sources), d_c.data_ptr(),
                                      d_ptr.data_ptr(), d_node.data_ptr(), d_dist.data_ptr(), d_nh.data_ptr(),
                                      total // 2, nb, allow_overflow=True)
    assert got2 == total
    np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint32), changed)
    np.testing.assert_array_equal(d_ptr.cpu().numpy().view(np.uint64), ptr)
    with pytest.raises(SpfError) as ei:
        eng.whatif_delta(links, sources, True, cap=total - 1)
    assert ei.value.code == E2BIG


def test_whatif_edge_cases(eng, whatif_mode):
    g = T.grid_fast(6)
    eng.set_graph(g)
    c, solved = eng.whatif([], [0, 1], True)
    assert c.shape == (0, 2) and solved == 0
    c, solved = eng.whatif([0, 1], [], True)
    assert c.shape == (2, 0)
    with pytest.raises(SpfError) as ei:
        eng.whatif([g.num_links], [0], True)
    assert ei.value.code == EINVAL
    with pytest.raises(SpfError):
        eng.whatif([0], [g.num_nodes], True)
    # a grid edge failure: exact counts against the oracle, all links x all sources
    links = list(range(g.num_links))
    srcs = list(range(g.num_nodes))
    c, _ = eng.whatif(links, srcs, True)
    np.testing.assert_array_equal(c, whatif_oracle(g, links, srcs, True))


# --- KSP2 traced on the device (openr_spf_ksp2) ------------------------------
def check_ksp2_against_oracle(eng, g, pairs):
    eng.set_graph(g)
    o = Oracle(g)
    src = [p[0] for p in pairs]
    dst = [p[1] for p in pairs]
    got = eng.ksp2(src, dst)
    for (s, d), (k1, k2) in zip(pairs, got):
        assert k1 == o.kth_paths(s, d, 1), ("k1", s, d)
        assert k2 == o.kth_paths(s, d, 2), ("k2", s, d)
    return got


@pytest.fixture(params=["default", "0", "3"])
def ksp_probe(request, monkeypatch):
    """KSP DFS reachability probe: default threshold, before every frame, after 3."""
    if request.param != "default":
        monkeypatch.setenv("OPENR_SPF_KSP_PROBE", request.param)
    return request.param


@pytest.mark.parametrize("case", G.load()["cases"], ids=lambda c: c["name"])
def test_ksp2_device_reference_cases_all_pairs(eng, case, ksp_probe):
    g = G.build(case)
    pairs = [(s, d) for s in range(g.num_nodes) for d in range(g.num_nodes)]
    got = check_ksp2_against_oracle(eng, g, pairs)
    for exp in case.get("kth", []):  # the reference tests' own expectations
        s, d = g.id(exp["src"]), g.id(exp["dst"])
        if exp["k"] in (1, 2):
            assert len(got[pairs.index((s, d))][exp["k"] - 1]) == exp["num_paths"]


@pytest.mark.parametrize("seed,max_metric", [(0, 1), (1, 9), (2, 1)])
def test_ksp2_device_random_graphs(eng, seed, max_metric, ksp_probe):
    g = random_graph(400 + seed, 70, 160, max_metric, p_ovl=0.08, p_down=0.05, p_par=0.15)
    rng = np.random.default_rng(seed)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, g.num_nodes, (400, 2))] + [(3, 3)]
    check_ksp2_against_oracle(eng, g, pairs)


def test_ksp2_device_fabric_sample(eng, ksp_probe):
    g = T.fabric(288 + 56)
    rng = np.random.default_rng(5)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, g.num_nodes, (300, 2))]
    got = check_ksp2_against_oracle(eng, g, pairs)
    assert any(len(k1) > 1 for k1, _ in got)  # ECMP: several edge-disjoint first paths


def fabric_with_faults(seed, n_ovl=12, n_down=60):
    """The fabric with overloaded switches (sinks) and down links."""
    g = T.fabric(288 + 56)
    rng = np.random.default_rng(seed)
    nodes = rng.choice(g.num_nodes, n_ovl, replace=False)
    links = rng.choice(g.num_links, n_down, replace=False)
    return g.patched([], [], links, [0] * len(links), nodes, [1] * len(nodes)), nodes


@pytest.mark.parametrize("seed", [0, 1])
def test_fabric_faults_all_sources_and_ksp2(eng, seed):
    """Last-level skip (every node reached) and the KSP2 second SPF's target pull tests
    next to sinks and down links: all-sources rows and traced paths vs the oracle,
    with pairs whose target neighbours an overloaded switch."""
    g, ovl = fabric_with_faults(seed)
    rng = np.random.default_rng(100 + seed)
    check_against_oracle(eng, g, rng.integers(0, g.num_nodes, 96).tolist() + [int(x) for x in ovl[:4]])
    nbrs = [int(g.col[e]) for x in ovl[:6] for e in range(g.row_ptr[x], g.row_ptr[x + 1])][::7]
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, g.num_nodes, (160, 2))]
    pairs += [(int(rng.integers(0, g.num_nodes)), d) for d in nbrs] + [(int(s), (int(s) + 1) % g.num_nodes) for s in ovl[:6]]
    check_ksp2_against_oracle(eng, g, pairs)


@pytest.mark.parametrize("seed", [0, 1])
def test_distance_only_solves(eng, seed):
    """No next-hop output: the code family solves every source in one 8-bit-field class
    without next-hop bits (no slices). Distances must match the full solve and the
    oracle, with and without ignore sets, for sources of every degree."""
    for g in (hub_graph(30 + seed, V=220, L=500), T.fabric(288 + 56)):
        eng.set_graph(g)
        o = Oracle(g)
        rng = np.random.default_rng(seed)
        srcs = list(range(3)) + rng.integers(0, g.num_nodes, 60).tolist()
        ignore = [sorted(set(rng.integers(0, g.num_links, int(rng.integers(0, 16))).tolist())) for _ in srcs]
        for ig in (None, ignore):
            d_only, nh, _ = eng.solve(srcs, True, want_nh=False, ignore=ig)
            assert nh is None
            d_full, _, _ = eng.solve(srcs, True, want_nh=True, ignore=ig)
            np.testing.assert_array_equal(d_only, d_full)
            for i, s in enumerate(srcs):
                np.testing.assert_array_equal(d_only[i], o.run_spf(int(s), True, ig[i] if ig else None).dist)


@pytest.mark.parametrize("seed", [0, 1])
def test_ksp2_device_hub_graphs(eng, seed, ksp_probe):
    """Rows of 40 / 75 / 130 in-edges: the register rank (<= 64, <= 128 in-edges) and the
    LDS rank (> 128) of pathLinks, with the hubs as sources, destinations and transit."""
    g = hub_graph(20 + seed, V=220, L=500)
    rng = np.random.default_rng(seed)
    pairs = [(h, int(d)) for h in range(3) for d in rng.integers(0, g.num_nodes, 40)]
    pairs += [(int(s), h) for h in range(3) for s in rng.integers(0, g.num_nodes, 40)]
    pairs += [(int(a), int(b)) for a, b in rng.integers(3, g.num_nodes, (200, 2))]
    check_ksp2_against_oracle(eng, g, pairs)


def test_ksp2_device_form_and_overflow(eng):
    import torch

    g = T.grid_fast(9)
    eng.set_graph(g)
    V = g.num_nodes
    srcs = np.array([0, 40, 80], dtype=np.uint32)
    prow = np.repeat(np.arange(3, dtype=np.uint32), V)
    pdst = np.tile(np.arange(V, dtype=np.uint32), 3)
    t1h, t2h = eng.ksp2_tokens(srcs[prow], pdst, 128)
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)
    d1 = torch.zeros((len(pdst), 128), dtype=torch.int32, device=dev)
    d2 = torch.zeros_like(d1)
    keep = [to(srcs), to(prow), to(pdst)]  # alive until the stream is synchronized
    eng.ksp2_device(keep[0].data_ptr(), 3, keep[1].data_ptr(), keep[2].data_ptr(), len(pdst), 128, d1.data_ptr(),
                    d2.data_ptr())
    torch.cuda.synchronize()
    from openr_amd.engine import decode_paths

    for dev_t, host_t in ((d1, t1h), (d2, t2h)):  # tokens past a row's used prefix are unspecified
        dt = dev_t.cpu().numpy().view(np.uint32)
        assert [decode_paths(r) for r in dt] == [decode_paths(r) for r in host_t]
    # a token row too small for the corner-to-corner paths: flagged, the call fails loudly
    with pytest.raises(SpfError) as ei:
        eng.ksp2_tokens([0], [V - 1], 8)
    assert ei.value.code == E2BIG
    t1, _ = eng.ksp2_tokens([0, 0], [V - 1, 1], 8, allow_overflow=True)
    assert t1[0, 0] == 0xFFFFFFFF and t1[1, 0] == 1


def test_whatif_overloads_parallel_links_hubs(eng, whatif_mode):
    """What-if on graphs with overloaded nodes, down links, parallel links and wide
    next-hop sets (multi-byte rows), all links x all sources."""
    g = hub_graph(7, V=160, L=320, hub_deg=(30, 45))
    eng.set_graph(g)
    links = list(range(g.num_links))
    srcs = list(range(0, g.num_nodes, 4))
    for use_metric in (True, False):
        changed, _ = eng.whatif(links, srcs, use_metric)
        np.testing.assert_array_equal(changed, whatif_oracle(g, links, srcs, use_metric))


@pytest.mark.parametrize("tier", [{"OPENR_SPF_KSP_SMALL_FRAMES": "2", "OPENR_SPF_KSP_SMALL_ARENA": "8"},
                                  {"OPENR_SPF_KSP_SMALL_FRAMES": "3"}, {"OPENR_SPF_KSP_TIER": "0"}],
                         ids=["tiny", "frames3", "full-only"])
def test_ksp2_device_capacity_tiers(eng, tier, monkeypatch):
    """The tracer runs a small-capacity tier (DFS frames / arena sized from the graph's
    depth, for occupancy) and re-runs the pairs it cannot hold in the full tier. Forcing
    tiny small-tier capacities sends most pairs through the re-run list; results must
    not change (k = 1 re-runs also rewrite the pair's ignore set for the second SPF)."""
    for k, v in tier.items():
        monkeypatch.setenv(k, v)
    g = random_graph(411, 70, 160, 9, p_ovl=0.08, p_down=0.05, p_par=0.15)
    rng = np.random.default_rng(7)
    check_ksp2_against_oracle(eng, g, [(int(a), int(b)) for a, b in rng.integers(0, g.num_nodes, (300, 2))])
    g = T.fabric(288 + 56)
    check_ksp2_against_oracle(eng, g, [(int(a), int(b)) for a, b in rng.integers(0, g.num_nodes, (200, 2))])
    g = hub_graph(21, V=220, L=500)
    check_ksp2_against_oracle(eng, g, [(h, int(d)) for h in range(3) for d in rng.integers(0, g.num_nodes, 30)])


@pytest.mark.parametrize("tag", ["1", "0"], ids=["tagged", "filled"])
def test_ksp2_tagged_rows_across_chunks(eng, monkeypatch, tag):
    """KSP2 second-SPF level rows (code family, uniform cost): tagged — a solve writes only
    the nodes it settles (it stops at the pair's target) as tag << shift | level, and an
    entry with another chunk's tag reads as unreached — or filled (unreached = 0xFFFF).
    Chunks of 7 pairs: on the 300-node graph (9 level bits, tags 1..127) the tags wrap and
    the rows are zeroed again mid-call; results equal the oracle either way."""
    monkeypatch.setenv("OPENR_SPF_KSP_TAG", tag)
    monkeypatch.setenv("OPENR_SPF_KSP_CHUNK", "7")
    g = random_graph(9, 300, 620, 1, p_ovl=0.05, p_down=0.05, p_par=0.1)
    rng = np.random.default_rng(11)
    check_ksp2_against_oracle(eng, g, [(int(a), int(b)) for a, b in rng.integers(0, g.num_nodes, (1400, 2))])
    g = T.fabric(288 + 56)
    check_ksp2_against_oracle(eng, g, [(int(a), int(b)) for a, b in rng.integers(0, g.num_nodes, (300, 2))])


def skip_edge_graphs():
    """Small graphs where ksp_select_pairs' row-length test is tight: the k = 1
    paths of a pair use every link of src or of dst exactly when the row has no down link
    and no self-loop. Two parallel links a=b (both up, or one down), an overloaded
    destination behind parallel links, and a diamond whose middle node is overloaded."""
    out = []
    # 0 = 1 parallel pair, 1 - 2 - 3 chain with a parallel pair 2 = 3, 0 - 4 - 3 detour
    links = np.array([(0, 1), (0, 1), (1, 2), (2, 3), (2, 3), (0, 4), (4, 3), (1, 4)])
    m = np.ones(len(links), dtype=np.uint64)
    for up in ([1] * 8, [1, 0, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 0, 1, 1, 1]):
        for ovl in ([0] * 5, [0, 0, 0, 1, 0], [0, 0, 1, 0, 0]):
            out.append(T.csr_from_links([f"n{i}" for i in range(5)], links, m, m,
                                        np.array(ovl, dtype=np.uint8), np.array(up, dtype=np.uint8)))
    return out


@pytest.mark.parametrize("skip", ["1", "0"], ids=["skip", "solve-all"])
def test_ksp2_skip_parallel_down_and_overloaded_endpoints(eng, monkeypatch, skip):
    """ksp_select_pairs' skip on and off against the oracle where its row-length test
    decides: parallel links between one pair, a parallel link down (the row is longer
    than the links a path can use, so the pair is kept), overloaded destinations and
    transit nodes. Every ordered pair of every graph."""
    monkeypatch.setenv("OPENR_SPF_KSP_SKIP", skip)
    for g in skip_edge_graphs():
        V = g.num_nodes
        check_ksp2_against_oracle(eng, g, [(s, d) for s in range(V) for d in range(V)])


@pytest.mark.parametrize("pack", ["1", "0"], ids=["arena-packed", "arena-wide"])
@pytest.mark.parametrize("pull", ["1", "0"], ids=["pull-batched", "pull-per-wave"])
@pytest.mark.parametrize("resume", ["1", "0"], ids=["resume", "regather"])
@pytest.mark.parametrize("skip", ["1", "0"], ids=["skip", "solve-all"])
def test_ksp2_empty_second_paths_skipped(eng, monkeypatch, skip, resume, pull, pack):
    """Pairs whose k = 2 answer is empty by construction (no k = 1 path, or k = 1 paths
    that use every link of the source or of the destination) skip the second SPF and the
    k = 2 trace (ksp_select_pairs). Two-pod fabric: every RSW -> RSW pair is such a pair
    (8 edge-disjoint paths over the 8 uplinks); leaves and self-loop-free hubs of a
    random graph with parallel links, down links and sinks; both forms vs the oracle.
    Also with and without the tracer resuming dest's frame between a pair's paths, and
    with the second SPF's pull test (2) batched over the block or one neighbour per wave,
    and with the tracer's arena entries packed (tail | link in one word) or not."""
    monkeypatch.setenv("OPENR_SPF_KSP_SKIP", skip)
    monkeypatch.setenv("OPENR_SPF_KSP_RESUME", resume)  # trace_one resumes dest's frame
    monkeypatch.setenv("OPENR_SPF_KSP_PULL", pull)  # the second SPF's target pull test (2) form
    monkeypatch.setenv("OPENR_SPF_KSP_PACK", pack)  # tracer arena: tail and link in one word
    g = T.fabric(288 + 2 * 56)
    V = g.num_nodes
    rsw = [u for u in range(V) if g.names[u].startswith("3-")]
    pairs = [(s, d) for s in rsw[::9] for d in range(V)]
    got = check_ksp2_against_oracle(eng, g, pairs)
    assert sum(1 for (s, d), (k1, k2) in zip(pairs, got) if d in rsw and s != d and len(k1) == 8 and not k2) > 0
    gf, ovl = fabric_with_faults(3)
    rng = np.random.default_rng(17)
    check_ksp2_against_oracle(eng, gf, [(int(a), int(b)) for a, b in rng.integers(0, gf.num_nodes, (400, 2))])
    gr = random_graph(77, 90, 140, 1, p_ovl=0.08, p_down=0.08, p_par=0.2)
    check_ksp2_against_oracle(eng, gr, [(s, d) for s in range(0, gr.num_nodes, 3) for d in range(gr.num_nodes)])


@pytest.mark.parametrize("tier", [{}, {"OPENR_SPF_KSP_SMALL_FRAMES": "3", "OPENR_SPF_KSP_SMALL_ARENA": "8"}],
                         ids=["tiers", "tiny-small-tier"])
@pytest.mark.parametrize("tl", [("1", "1"), ("1", "0"), ("0", "0")], ids=["path-lists-k12", "path-lists-k1", "record-rows"])
def test_ksp2_k1_path_lists(eng, monkeypatch, tl, tier):
    """The k = 1 trace's frames read the source's pathLinks as lists built once per base
    row (launch_ksp_path_lists: tight in-edges in rank order, the tail's sink rule and the
    edge's up flag applied) instead of gathering record rows and their tails' distances.
    Against the oracle with the lists on and off: the fabric with sinks and down links,
    hub rows of 130 in-edges (lists longer than a wavefront), a uniform-cost random
    multigraph with parallel links, and a weighted one (no lists: not uniform cost); also
    with a tiny small tier, so list gathers overflow the arena and re-run in the full tier.
    The k = 2 trace reads the same lists for nodes its pair's row leaves at their base
    distance (OPENR_SPF_KSP_TL2), else the record rows."""
    monkeypatch.setenv("OPENR_SPF_KSP_TL", tl[0])
    monkeypatch.setenv("OPENR_SPF_KSP_TL2", tl[1])
    for k, v in tier.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(29)
    gf, ovl = fabric_with_faults(6)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, gf.num_nodes, (300, 2))]
    pairs += [(int(x), int(rng.integers(0, gf.num_nodes))) for x in ovl] + [(3, 3)]
    check_ksp2_against_oracle(eng, gf, pairs)
    gh = hub_graph(22, V=220, L=500)
    check_ksp2_against_oracle(eng, gh, [(int(s), h) for h in range(3) for s in rng.integers(0, gh.num_nodes, 40)])
    for mm in (1, 9):
        gr = random_graph(93 + mm, 100, 220, mm, p_ovl=0.08, p_down=0.08, p_par=0.2)
        check_ksp2_against_oracle(eng, gr, [(s, d) for s in range(0, gr.num_nodes, 9) for d in range(gr.num_nodes)])


@pytest.mark.parametrize("mode", [{}, {"OPENR_SPF_KSP_REPAIR": "0"}, {"OPENR_SPF_KSP_REPAIR_G": "4"},
                                  {"OPENR_SPF_KSP_REPAIR_G": "64"}, {"OPENR_SPF_KSP_SKIP": "0"},
                                  {"OPENR_SPF_KSP_TL2": "0"}, {"OPENR_SPF_KSP_CHUNK": "7"},
                                  {"OPENR_SPF_KSP_REPAIR_CAP": "0"}, {"OPENR_SPF_KSP_REPAIR_CAP": "6"}],
                         ids=["repair", "forward", "g4", "g64", "solve-all", "k2-record-rows", "chunks-of-7",
                              "cap0-all-forward", "cap6-mixed"])
def test_ksp2_second_spf_repair(eng, monkeypatch, mode, bfs_family):
    """The KSP2 second SPF as a repair of the base SPF (launch_ksp_repair): the nodes whose
    every base pathLink is ignored or comes from such a node get new levels (a BFS over
    them seeded by their unaffected neighbours, up to dest's level); the k = 2 trace reads
    every other node's distance from the base row. Against the oracle on the fabric (RSW,
    FSW and SSW endpoints, src == dest), the fabric with sinks and down links, a
    uniform-cost random multigraph with parallel links, the small parallel / down /
    overloaded graphs and hub rows; with the forward solve, other lanes-per-node widths,
    every pair solved, the k = 2 record-row gather, chunks of 7 pairs (tags wrap), and
    affected-set caps of 0 and 6 nodes (pairs over the cap are solved forward, and the
    trace reads each pair's row in its own form)."""
    for k, v in mode.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(31)
    g = T.fabric(288 + 2 * 56)
    V = g.num_nodes
    pairs = [(int(s), d) for s in rng.integers(0, V, 5) for d in range(0, V, 3)] + [(5, 5)]
    pairs += [(s, int(d)) for s in range(0, 16 * 2 + 16, 7) for d in rng.integers(0, V, 30)]  # SSW / FSW sources
    check_ksp2_against_oracle(eng, g, pairs)
    if mode.get("OPENR_SPF_KSP_REPAIR") != "0" and bfs_family[0] == "code":  # tagged rows: code family only
        assert "ksp_repair_kernel" in eng.last_kernels()
    gf, ovl = fabric_with_faults(8)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, gf.num_nodes, (300, 2))]
    pairs += [(int(rng.integers(0, gf.num_nodes)), int(x)) for x in ovl] + [(int(x), int(rng.integers(0, gf.num_nodes))) for x in ovl]
    check_ksp2_against_oracle(eng, gf, pairs)
    gr = random_graph(97, 120, 260, 1, p_ovl=0.08, p_down=0.08, p_par=0.2)
    check_ksp2_against_oracle(eng, gr, [(s, d) for s in range(0, gr.num_nodes, 7) for d in range(gr.num_nodes)])
    for gs in skip_edge_graphs()[:5]:
        check_ksp2_against_oracle(eng, gs, [(s, d) for s in range(gs.num_nodes) for d in range(gs.num_nodes)])
    gh = hub_graph(23, V=220, L=500)
    check_ksp2_against_oracle(eng, gh, [(h, int(d)) for h in range(3) for d in rng.integers(0, gh.num_nodes, 30)])
