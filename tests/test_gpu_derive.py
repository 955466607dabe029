"""Split all-sources batches (spf_derive.hip) against the oracle.

For uniform cost the row of a source follows from the rows of its neighbours, so of a batch
that holds those rows only a link-covering set of sources is solved by a BFS pass and the
rest (an independent set: the checkerboard of a grid) is derived by `nh_derive_kernel`.
Every row, u64 distances and next-hop bytes, is compared with `oracle.Oracle`; the same
batches with OPENR_SPF_DERIVE=0 must give byte-identical arrays.

The shapes are the smallest at which each path runs: 12 x 12 and 11 x 11 grids (even and
odd V: with an odd V every other distance row is only 8-byte aligned and the next-hop rows
start at every byte alignment) on the lean and on the wave pass, attribute variants
(overloaded nodes, down links, two components, cost 7, parallel links), partial batches, a
batch of more than 16 384 entries (a second step of the one-workgroup scan), and the two
overflow routes to the u16 re-run (depth above 253, a level wider than its queue half).
"""
import numpy as np
import pytest

from openr_amd import topology as T
from openr_amd.engine import SpfEngine
from oracle import Oracle

pytestmark = pytest.mark.gpu

DERIVE = "nh_derive_kernel"
BFS = ("bfs_ell_kernel", "bfs_wave_kernel")


@pytest.fixture(scope="module")
def eng():
    e = SpfEngine()
    yield e
    e.close()


@pytest.fixture(autouse=True)
def lvl_family(monkeypatch):
    # small grids are shallow: put them on the level family's lean pass (test_gpu_lean_rows.py)
    monkeypatch.setenv("OPENR_SPF_BFS_FAMILY", "lvl")
    monkeypatch.setenv("OPENR_SPF_BFS_WAVE", "0")
    monkeypatch.setenv("OPENR_SPF_RING_CAP", "512")
    monkeypatch.setenv("OPENR_SPF_DERIVE", "1")


def grid_links(rows, cols):
    links = [(r * cols + c, r * cols + c + 1) for r in range(rows) for c in range(cols - 1)]
    links += [(r * cols + c, (r + 1) * cols + c) for r in range(rows - 1) for c in range(cols)]
    return [f"g{r:02d}-{c:02d}" for r in range(rows) for c in range(cols)], links


def grid_graph(rows, cols, extra=(), **kw):
    names, links = grid_links(rows, cols)
    return T.csr_from_links(names, np.array(links + list(extra)), **kw)


def colouring(g):
    """The engine's derive colouring: greedy in node-id order over the link structure."""
    V = g.num_nodes
    der = np.zeros(V, dtype=bool)
    for u in range(V):
        nbrs = {int(v) for v in g.col[g.row_ptr[u]:g.row_ptr[u + 1]] if int(v) != u}
        der[u] = len(nbrs) <= 4 and not any(der[v] for v in nbrs)
    return der


def expected_derived(g, srcs):
    """Batch entries the split derives: the node is derivable and every neighbour behind an
    up link that is not overloaded is a source of the batch."""
    der, present = colouring(g), set(int(s) for s in srcs)
    out = []
    for s in (int(x) for x in srcs):
        ok = bool(der[s])
        for e in range(int(g.row_ptr[s]), int(g.row_ptr[s + 1])):
            v = int(g.col[e])
            if ok and g.edge_up[e] and v != s and not g.node_overloaded[v]:
                ok = v in present
        out.append(ok)
    return np.array(out, dtype=bool)


def check_rows(dist, nh, odist, onh):
    bad = np.nonzero(np.any(dist != odist, axis=1))[0]
    assert bad.size == 0, f"dist differs for batch rows {bad[:8].tolist()}"
    bad = np.nonzero(np.any(nh != onh, axis=(1, 2)))[0]
    assert bad.size == 0, f"next hops differ for batch rows {bad[:8].tolist()}"


def solve_split(eng, g, srcs, use_metric=True, oracle_rows=None):
    """Solve with the split forced, compare with the oracle; returns (dist, nh, kernels, derived)."""
    srcs = np.asarray(srcs, dtype=np.uint32)
    dist, nh, _ = eng.solve(srcs, use_metric)
    ran = eng.last_kernels()
    derived = eng.last_derived()
    if oracle_rows is None:
        oracle_rows = Oracle(g).all_sources(srcs, use_metric, nthreads=16)
    check_rows(dist, nh, *oracle_rows)
    return dist, nh, ran, derived


# --- grids --------------------------------------------------------------------------------
@pytest.mark.parametrize("use_metric", [True, False], ids=["metric", "hops"])
@pytest.mark.parametrize("bfs_pass", ["lean", "wave"])
@pytest.mark.parametrize("n", [12, 11])
def test_grid_all_sources(eng, monkeypatch, n, bfs_pass, use_metric):
    if bfs_pass == "wave":
        monkeypatch.setenv("OPENR_SPF_BFS_WAVE", "1")
    names, links = grid_links(n, n)
    g = T.csr_from_links(names, np.array(links), metric_uv=np.full(len(links), 3, dtype=np.uint64))
    eng.set_graph(g)
    srcs = np.arange(g.num_nodes, dtype=np.uint32)
    dist, nh, ran, derived = solve_split(eng, g, srcs, use_metric)
    assert DERIVE in ran and f"bfs_{'ell' if bfs_pass == 'lean' else 'wave'}_kernel" in ran, ran
    assert derived == (n * n + 1) // 2  # the checkerboard
    assert int(dist[0, g.num_nodes - 1]) == 2 * (n - 1) * (3 if use_metric else 1)
    monkeypatch.setenv("OPENR_SPF_DERIVE", "0")
    dist0, nh0, _ = eng.solve(srcs, use_metric)
    assert DERIVE not in eng.last_kernels() and eng.last_derived() == 0
    assert dist.tobytes() == dist0.tobytes() and nh.tobytes() == nh0.tobytes()


def test_wider_next_hop_rows(eng):
    """nh_bytes = 3: a derived row's bytes past the first are zero, as a solved row's."""
    g = grid_graph(11, 11)
    eng.set_graph(g)
    srcs = np.arange(g.num_nodes, dtype=np.uint32)
    dist, nh, _ = eng.solve(srcs, True, nh_bytes=3)
    assert DERIVE in eng.last_kernels()
    odist, onh = Oracle(g).all_sources(srcs, True, nthreads=16)
    assert np.array_equal(dist, odist) and np.array_equal(nh[:, :, :1], onh)
    assert not nh[:, :, 1:].any()


def test_more_entries_than_one_scan_step(eng):
    """17 001 entries (the 144 sources repeated): the scan takes two steps, duplicates of a
    node map to one of its entries, and every workgroup of the derive pass takes several units."""
    g = grid_graph(12, 12)
    eng.set_graph(g)
    idx = np.arange(17001) % 144
    odist, onh = Oracle(g).all_sources(np.arange(144, dtype=np.uint32), True, nthreads=16)
    _, _, ran, derived = solve_split(eng, g, idx.astype(np.uint32), oracle_rows=(odist[idx], onh[idx]))
    assert DERIVE in ran, ran
    assert derived == int(expected_derived(g, idx).sum()) == int(colouring(g)[idx].sum())


# --- attributes ---------------------------------------------------------------------------
def attribute_graph(kind):
    names, links = grid_links(12, 12)
    rng = np.random.default_rng({"overload": 1, "down": 2, "split": 3, "parallel7": 4}[kind])
    L = len(links)
    ovl = np.zeros(144, dtype=np.uint8)
    up = np.ones(L, dtype=np.uint8)
    metric = np.ones(L, dtype=np.uint64)
    if kind == "overload":
        ovl[rng.choice(144, 14, replace=False)] = 1
    elif kind == "down":
        up[rng.choice(L, L * 12 // 100, replace=False)] = 0
    elif kind == "split":  # columns 0-7 and 8-11 fall apart, plus a few overloaded nodes
        for i, (u, v) in enumerate(links):
            if u % 12 == 7 and v == u + 1:
                up[i] = 0
        ovl[rng.choice(144, 6, replace=False)] = 1
    else:  # ten parallel links between neighbouring border nodes (rows keep <= 4 edges), cost 7
        top = [(c, c + 1) for c in range(0, 10, 2)]
        left = [(r * 12, (r + 1) * 12) for r in range(1, 11, 2)]
        links = links + top + left
        metric = np.full(len(links), 7, dtype=np.uint64)
        up = np.ones(len(links), dtype=np.uint8)
        up[rng.choice(L, 6, replace=False)] = 0
    return T.csr_from_links(names, np.array(links), metric_uv=metric, overloaded=ovl, link_up=up)


@pytest.mark.parametrize("kind", ["overload", "down", "split", "parallel7"])
def test_attributes_and_patches(eng, kind):
    g = attribute_graph(kind)
    assert int(np.diff(g.row_ptr).max()) <= 4
    eng.set_graph(g)
    srcs = np.arange(144, dtype=np.uint32)
    dist, _, ran, derived = solve_split(eng, g, srcs)
    assert DERIVE in ran and any(k in ran for k in BFS), ran
    assert derived == int(expected_derived(g, srcs).sum()) > 0
    if kind == "split":
        assert dist[0, 11] == np.uint64(2**64 - 1)
    if kind == "parallel7":
        assert int(dist[0, 1]) == 7
    # attribute patches keep the colouring: toggle an overload bit, take a link down
    node = 40
    eng.patch(nodes=[node], node_overloaded=[0 if g.node_overloaded[node] else 1])
    _, _, ran, _ = solve_split(eng, eng.g, srcs)
    assert DERIVE in ran, ran
    link = int(np.nonzero(eng.g.edge_up)[0][5])
    eng.patch(links=[int(eng.g.link_id[link])], link_up=[0])
    _, _, ran, derived = solve_split(eng, eng.g, srcs)
    assert DERIVE in ran and derived == int(expected_derived(eng.g, srcs).sum()), ran


# --- partial batches ----------------------------------------------------------------------
def test_partial_batches(eng):
    g = grid_graph(12, 12)
    eng.set_graph(g)
    der = colouring(g)
    assert der.sum() == 72 and der[0] and not der[1] and not der[12] and der[13]
    rng = np.random.default_rng(7)
    block = np.arange(30, 90)
    subset = rng.choice(144, 100, replace=True)
    for srcs in (block, subset):
        want = expected_derived(g, srcs)
        assert 0 < want.sum() < der[srcs].sum()  # some derivable entries lack a neighbour
        _, _, ran, derived = solve_split(eng, g, srcs)
        assert DERIVE in ran and derived == int(want.sum()), (ran, derived)
    # derivable nodes only: none has its neighbours in the batch, every entry is solved
    only = np.nonzero(der)[0]
    _, _, ran, derived = solve_split(eng, g, only)
    assert derived == 0 and any(k in ran for k in BFS), ran


# --- fallbacks ----------------------------------------------------------------------------
def test_ladder_deeper_than_u8_levels(eng, monkeypatch):
    """2 x 300 ladder (node = 2 * rung + side, so ids differ by at most 2), all sources: most
    solves pass level 253, leave no level row and go to the u16 re-run, and so does every
    derived source that needs one of them."""
    monkeypatch.delenv("OPENR_SPF_RING_CAP")
    monkeypatch.setenv("OPENR_SPF_BFS_WAVE", "1")
    names = [f"l{i:03d}{s}" for i in range(300) for s in "ab"]
    links = [(2 * i, 2 * i + 1) for i in range(300)]
    links += [(2 * i + s, 2 * i + 2 + s) for i in range(299) for s in (0, 1)]
    g = T.csr_from_links(names, np.array(links))
    eng.set_graph(g)
    srcs = np.arange(600, dtype=np.uint32)
    dist, _, ran, derived = solve_split(eng, g, srcs)
    assert DERIVE in ran and any("rerun" in k for k in ran), ran
    assert derived == 300 and int(dist[0, 599]) == 300


def test_levels_wider_than_the_queue_halves(eng, monkeypatch):
    """20 x 20 grid, queue halves of 32 entries: sources near the centre reach levels of up
    to 40 nodes and are re-run, corner sources (at most 20) are not; the derived sources
    next to an overflowed one follow it to the re-run, the others are derived."""
    monkeypatch.setenv("OPENR_SPF_LEAN_FORCE", "1")
    monkeypatch.setenv("OPENR_SPF_RING_CAP", "64")
    g = grid_graph(20, 20)
    eng.set_graph(g)
    srcs = np.arange(400, dtype=np.uint32)
    dist, _, ran, derived = solve_split(eng, g, srcs)
    assert DERIVE in ran and "bfs_ell_kernel" in ran and any("rerun" in k for k in ran), ran
    assert derived == 200
    widest = [int(np.bincount(dist[s].astype(np.int64)).max()) for s in (0, 210)]
    assert widest[0] <= 32 < widest[1], widest


# --- not legal ----------------------------------------------------------------------------
def test_requests_the_split_does_not_serve(eng):
    """A distance-only solve, u8 level rows and refresh_device run what they ran before."""
    import torch

    g = grid_graph(12, 12)
    eng.set_graph(g)
    srcs = np.arange(144, dtype=np.uint32)
    o = Oracle(g)
    odist, onh = o.all_sources(srcs, True, nthreads=16)
    dist, nh, _ = eng.solve(srcs, True, want_nh=False)
    assert nh is None and DERIVE not in eng.last_kernels() and eng.last_derived() == 0
    assert np.array_equal(dist, odist)

    dev = torch.device("cuda", 0)
    d_src = torch.from_numpy(srcs.astype(np.int32)).to(dev)
    rows = torch.zeros(144 * 144, dtype=torch.uint8, device=dev)
    d_nh = torch.zeros(144 * 144, dtype=torch.uint8, device=dev)
    eng.solve_device(d_src.data_ptr(), 144, rows.data_ptr(), d_nh.data_ptr(), 1, True, level_bytes=1)
    assert eng.take_status() == 0 and DERIVE not in eng.last_kernels()
    assert np.array_equal(rows.cpu().numpy().reshape(144, 144), odist.astype(np.uint8))
    assert np.array_equal(d_nh.cpu().numpy().reshape(144, 144, 1), onh)

    # resident rows (solved split), a patch, then the in-place refresh of the affected rows
    d_dist = torch.zeros(144 * 144, dtype=torch.int64, device=dev)
    eng.solve_device(d_src.data_ptr(), 144, d_dist.data_ptr(), d_nh.data_ptr(), 1, True)
    assert DERIVE in eng.last_kernels()
    eng.solve_device(d_src.data_ptr(), 1, rows.data_ptr(), 0, 1, True, level_bytes=1)  # starts a new trace
    eng.patch(nodes=[66], node_overloaded=[1])
    assert eng.refresh_device(d_src.data_ptr(), 144, d_dist.data_ptr(), d_nh.data_ptr(), 1, True) > 0
    torch.cuda.synchronize()
    assert DERIVE not in eng.last_kernels()
    pdist, pnh = Oracle(eng.g).all_sources(srcs, True, nthreads=16)
    assert np.array_equal(d_dist.cpu().numpy().view(np.uint64).reshape(144, 144), pdist)
    assert np.array_equal(d_nh.cpu().numpy().reshape(144, 144, 1), pnh)
