"""Row write-out and the hand-over between solves of the lean level pass, against the oracle.

`bfs_ell_kernel` (spf_bfs_lvl.hip) writes a solve's rows from LDS with batched reads (two
nodes per lane and 16-byte store for the u64 distances, one next-hop dword per lane), then
claims its next unit and re-initialises LDS for it.
What can go wrong there shows only at these shapes, none of which needs a large graph:
several units per workgroup on both block sizes (state left by the previous unit, the
claim), an overflowed unit followed by a normal one, rows whose length is 0..3 mod 4 or odd
(so every other row base is only 8-byte aligned), output pointers offset by 8 and by 1 byte,
a distance-only solve, the u8 level-row form, unreached nodes, and uniform costs on both
sides of 2^24 (below it the level x cost product is a 24-bit multiply).

Every row, u64 distances and next-hop bytes, is compared with `oracle.Oracle`. Small graphs
are put on the lean pass with OPENR_SPF_RING_CAP, as in test_gpu_lean_narrow.py.
"""
import re

import numpy as np
import pytest

from openr_amd import topology as T
from openr_amd.engine import SpfEngine
from oracle import Oracle

pytestmark = pytest.mark.gpu

INF = np.uint64(2**64 - 1)


@pytest.fixture(scope="module")
def eng():
    e = SpfEngine()
    yield e
    e.close()


@pytest.fixture(autouse=True)
def lean_pass(monkeypatch):
    monkeypatch.setenv("OPENR_SPF_BFS_FAMILY", "lvl")
    monkeypatch.setenv("OPENR_SPF_BFS_WAVE", "0")
    monkeypatch.setenv("OPENR_SPF_RING_CAP", "512")


def grid_links(rows, cols):
    links = [(r * cols + c, r * cols + c + 1) for r in range(rows) for c in range(cols - 1)]
    links += [(r * cols + c, (r + 1) * cols + c) for r in range(rows - 1) for c in range(cols)]
    return [f"g{r:02d}-{c:02d}" for r in range(rows) for c in range(cols)], links


def grid_graph(rows, cols, **kw):
    names, links = grid_links(rows, cols)
    return T.csr_from_links(names, np.array(links), **kw)


def chain_graph(V):
    return T.csr_from_links([f"p{i:03d}" for i in range(V)], np.array([(i, i + 1) for i in range(V - 1)]))


def check_rows(dist, nh, odist, onh, srcs):
    bad = np.nonzero(np.any(dist != odist, axis=1))[0]
    assert bad.size == 0, f"dist differs for batch rows {bad[:8].tolist()} (sources {np.asarray(srcs)[bad[:8]].tolist()})"
    if nh is not None:
        bad = np.nonzero(np.any(nh != onh, axis=(1, 2)))[0]
        assert bad.size == 0, f"next hops differ for batch rows {bad[:8].tolist()}"


def solve_vs_oracle(eng, g, sources, use_metric=True):
    eng.set_graph(g)
    o = Oracle(g)
    assert eng.nh_bytes == o.nh_bytes
    srcs = np.asarray(sources, dtype=np.uint32)
    dist, nh, _ = eng.solve(srcs, use_metric)
    ran = eng.last_kernels()
    assert "bfs_ell_kernel" in ran, ran
    odist, onh = o.all_sources(srcs, use_metric, nthreads=16)
    check_rows(dist, nh, odist, onh, srcs)
    return dist, nh, ran


def num_cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# --- several units per workgroup, both block sizes -----------------------------------
@pytest.mark.parametrize("block", [256, 128])
def test_several_units_per_workgroup(eng, monkeypatch, capfd, block):
    """12 x 12 grid, its 144 sources repeated: 2 * (8 * CUs) + 5 solves on 256-thread
    workgroups, 3 * (16 * CUs) + 5 on 128-thread ones, so every workgroup runs several units
    and claims the later ones dynamically. Once with the profiling variant, whose stderr line
    carries the block size and the grid, and once with the production kernel."""
    cus = num_cus()
    n = 2 * (8 * cus) + 5 if block == 256 else 3 * (16 * cus) + 5
    g = grid_graph(12, 12)
    eng.set_graph(g)
    idx = np.arange(n) % 144
    srcs = idx.astype(np.uint32)
    odist, onh = Oracle(g).all_sources(np.arange(144, dtype=np.uint32), True, nthreads=16)
    for prof in ("1", "0"):
        monkeypatch.setenv("OPENR_SPF_PROF", prof)
        capfd.readouterr()
        dist, nh, _ = eng.solve(srcs, True)
        assert "bfs_ell_kernel" in eng.last_kernels()
        if prof == "1":
            line = [l for l in capfd.readouterr().err.splitlines() if l.startswith("bfs_ell:")]
            assert line, "no bfs_ell: line"
            m = re.search(r"block=(\d+) grid=(\d+) n=(\d+)", line[-1])
            assert int(m.group(1)) == block, line[-1]
            assert int(m.group(3)) == n and n > int(m.group(2)), line[-1]
        check_rows(dist, nh, odist[idx], onh[idx], srcs)


# --- an overflowed unit followed by a normal one in the same workgroup ---------------------
def test_overflowed_then_normal_units(eng, monkeypatch):
    """40 x 40 grid, queue halves of 64 entries: centre sources reach levels of 78 nodes, are
    listed and re-run by the u16 pass; corner sources (levels of at most 40) are not. The two
    kinds alternate in the batch, repeated past twice the resident workgroups, so a workgroup
    takes a normal unit after one that left without writing rows."""
    monkeypatch.setenv("OPENR_SPF_LEAN_FORCE", "1")
    monkeypatch.setenv("OPENR_SPF_RING_CAP", "128")
    g = grid_graph(40, 40)
    centre = [20 * 40 + 20, 19 * 40 + 20, 20 * 40 + 19, 19 * 40 + 19]
    corner = [0, 39, 39 * 40, 40 * 40 - 1]
    distinct = np.array([x for pair in zip(centre, corner) for x in pair], dtype=np.uint32)  # centre, corner, ...
    n = 2 * (8 * num_cus()) + 7
    idx = np.arange(n) % len(distinct)
    eng.set_graph(g)
    dist, nh, _ = eng.solve(distinct[idx], True)
    ran = eng.last_kernels()
    assert "bfs_ell_kernel" in ran and any("rerun" in k for k in ran), ran
    odist, onh = Oracle(g).all_sources(distinct, True, nthreads=16)
    widest = [int(np.bincount(d.astype(np.int64)).max()) for d in odist]
    assert widest[0] == 78 and widest[1] == 40, widest
    check_rows(dist, nh, odist[idx], onh[idx], distinct[idx])


# --- row shapes ---------------------------------------------------------------------------
SHAPES = {
    "grid12x12": lambda: grid_graph(12, 12),  # V = 144: V % 4 == 0
    "grid11x11": lambda: grid_graph(11, 11),  # V = 121: V % 4 == 1, odd
    "grid9x14": lambda: grid_graph(9, 14),    # V = 126: V % 4 == 2
    "chain203": lambda: chain_graph(203),     # V = 203: V % 4 == 3, odd
}


@pytest.fixture(scope="module")
def shape_refs():
    """Graph and oracle rows (every source) of each shape, computed once."""
    refs = {}
    for name, make in SHAPES.items():
        g = make()
        srcs = np.arange(g.num_nodes, dtype=np.uint32)
        refs[name] = (g, srcs) + tuple(Oracle(g).all_sources(srcs, True, nthreads=16))
    return refs


@pytest.mark.parametrize("shape", list(SHAPES))
def test_row_shapes_host_rows(eng, shape_refs, shape):
    """Every source: with an odd V every other distance row starts 8 bytes off a 16-byte
    boundary, and the next-hop rows start at every byte alignment."""
    g, srcs, odist, onh = shape_refs[shape]
    assert g.num_nodes % 4 == {"grid12x12": 0, "grid11x11": 1, "grid9x14": 2, "chain203": 3}[shape]
    eng.set_graph(g)
    dist, nh, _ = eng.solve(srcs, True)
    assert "bfs_ell_kernel" in eng.last_kernels()
    check_rows(dist, nh, odist, onh, srcs)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_row_shapes_device_forms(eng, shape_refs, shape):
    """solve_device: output pointers offset by 8 bytes (distances) and 1 byte (next hops)
    into over-allocated tensors; a distance-only solve (d_nh = 0, as update_main does); the
    u8 level-row form, aligned and offset by 1 byte."""
    import torch

    g, srcs, odist, onh = shape_refs[shape]
    eng.set_graph(g)
    n, V, nb = len(srcs), g.num_nodes, eng.nh_bytes
    dev = torch.device("cuda", 0)
    d_src = torch.from_numpy(srcs.astype(np.int32)).to(dev)

    def dist_of(buf, off):
        return buf[off:off + n * V * 8].cpu().numpy().copy().view(np.uint64).reshape(n, V)

    def nh_of(buf, off):
        return buf[off:off + n * V * nb].cpu().numpy().reshape(n, V, nb)

    # offset pointers; the bytes around the rows stay untouched
    d_dist = torch.full((n * V * 8 + 32,), 0xA5, dtype=torch.uint8, device=dev)
    d_nh = torch.full((n * V * nb + 32,), 0xA5, dtype=torch.uint8, device=dev)
    eng.solve_device(d_src.data_ptr(), n, d_dist.data_ptr() + 8, d_nh.data_ptr() + 1, nb, True)
    torch.cuda.synchronize()
    assert "bfs_ell_kernel" in eng.last_kernels()
    check_rows(dist_of(d_dist, 8), nh_of(d_nh, 1), odist, onh, srcs)
    for buf, lo, hi in ((d_dist, 8, 8 + n * V * 8), (d_nh, 1, 1 + n * V * nb)):
        edge = torch.cat([buf[:lo], buf[hi:]]).cpu().numpy()
        assert (edge == 0xA5).all(), "bytes outside the rows were written"

    # distance-only
    d_dist.fill_(0xA5)
    eng.solve_device(d_src.data_ptr(), n, d_dist.data_ptr(), 0, nb, True)
    torch.cuda.synchronize()
    assert "bfs_ell_kernel" in eng.last_kernels()
    check_rows(dist_of(d_dist, 0), None, odist, onh, srcs)

    # u8 level rows (unit cost: distance = level; none of these graphs is deeper than 254)
    exp = np.where(odist == INF, 0xFF, np.minimum(odist, 0xFE)).astype(np.uint8)
    for off in (0, 1):
        rows = torch.full((n * V + 32,), 0xA5, dtype=torch.uint8, device=dev)
        d_nh.fill_(0xA5)
        eng.solve_device(d_src.data_ptr(), n, rows.data_ptr() + off, d_nh.data_ptr(), nb, True, level_bytes=1)
        assert eng.take_status() == 0
        assert "bfs_ell_kernel" in eng.last_kernels()
        got = rows.cpu().numpy()
        np.testing.assert_array_equal(got[off:off + n * V].reshape(n, V), exp)
        assert (got[:off] == 0xA5).all() and (got[off + n * V:] == 0xA5).all()
        np.testing.assert_array_equal(nh_of(d_nh, 0), onh)


# --- unreached nodes -------------------------------------------------------------------------
def test_unreached_nodes(eng):
    """Two components (a 10 x 10 and a 5 x 7 grid), a down link that cuts a corner node's
    second edge off and an overloaded node behind which a leaf hangs: UINT64_MAX distances and
    zero next-hop bytes exactly where the oracle has them."""
    na, la = grid_links(10, 10)
    nb_, lb = grid_links(5, 7)
    names = na + [f"h{x[1:]}" for x in nb_] + ["leaf"]
    links = la + [(u + 100, v + 100) for u, v in lb] + [(99, 135)]  # leaf behind node 99
    up = np.ones(len(links), dtype=np.uint8)
    up[links.index((0, 1))] = 0
    ovl = np.zeros(len(names), dtype=np.uint8)
    ovl[99] = 1  # transit through 99 is barred: the leaf is unreached from everywhere else
    g = T.csr_from_links(names, np.array(links), overloaded=ovl, link_up=up)
    srcs = np.arange(g.num_nodes, dtype=np.uint32)
    dist, nh, _ = solve_vs_oracle(eng, g, srcs)
    un = dist == INF
    assert un[0, 100:].all() and un[0, 135] and not un[0, :100].any()
    assert not un[99, 135] and un[135, :99].all()
    assert (nh[un] == 0).all()


# --- uniform cost ------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", [1, 2**24 - 1, 2**24, 2**31 - 1])
def test_uniform_cost(eng, cost):
    """One metric on every link: 1, both sides of 2^24 (below it the product is a 24-bit
    multiply) and 2^31 - 1, the largest metric set_graph takes on this path (metrics are
    u64 in the graph, u32 on the device, and a usable link above 2^31 - 1 leaves the BFS
    families). With the metric, and as hop count on the same graph."""
    names, links = grid_links(11, 11)
    g = T.csr_from_links(names, np.array(links), metric_uv=np.full(len(links), cost, dtype=np.uint64))
    srcs = np.arange(0, 121, 5, dtype=np.uint32)
    dist, _, _ = solve_vs_oracle(eng, g, srcs, True)
    assert int(dist[0, 120]) == 20 * cost
    hops, _, _ = solve_vs_oracle(eng, g, srcs, False)
    assert int(hops[0, 120]) == 20
