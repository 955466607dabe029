"""The lean level pass's narrow mode (bfs_ell_kernel, spf_bfs_lvl.hip) against the oracle.

A level of at most 64 nodes is expanded by wave 0 alone, and so is every following level
while the count stays in [1, 64]: no shared append counter and no barrier inside such a
run; the other waves wait at the one barrier that ends it. These tests drive the mode
switches (never wide; narrow, wide, narrow; a flip at every level; the threshold 64 itself)
and every exit of a narrow run (count 0, every node reached, a level wider than its queue
half), on both block sizes and both row encodings. Every row (distances and next-hop
bytes) is compared with the CPU oracle.

All graphs keep every row to at most 4 edges, the lean pass's precondition. Graphs small
enough for the full-order queue are put on the lean pass with OPENR_SPF_RING_CAP.
"""
import re

import numpy as np
import pytest

from openr_amd import topology as T
from openr_amd.engine import SpfEngine
from oracle import Oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = SpfEngine()
    yield e
    e.close()


@pytest.fixture(autouse=True)
def lean_pass(monkeypatch):
    monkeypatch.setenv("OPENR_SPF_BFS_FAMILY", "lvl")
    monkeypatch.setenv("OPENR_SPF_BFS_WAVE", "0")


def solve_vs_oracle(eng, g, sources):
    """Engine rows == oracle rows for every source; the lean pass must have run."""
    eng.set_graph(g)
    o = Oracle(g)
    assert eng.nh_bytes == o.nh_bytes
    srcs = np.asarray(sources, dtype=np.uint32)
    dist, nh, _ = eng.solve(srcs, True)
    ran = eng.last_kernels()
    assert "bfs_ell_kernel" in ran, ran
    odist, onh = o.all_sources(srcs, True, nthreads=16)
    bad = np.nonzero(np.any(dist != odist, axis=1))[0]
    assert bad.size == 0, f"dist differs for sources {srcs[bad[:8]].tolist()}"
    bad = np.nonzero(np.any(nh != onh, axis=(1, 2)))[0]
    assert bad.size == 0, f"next hops differ for sources {srcs[bad[:8]].tolist()}"
    return dist, ran


def level_widths(dist_row):
    """Nodes per BFS level of one solve (unit cost: distance = level), level 0 first."""
    d = dist_row[dist_row != np.uint64(2**64 - 1)].astype(np.int64)
    return np.bincount(d)


def grid_links(n):
    links = [(r * n + c, r * n + c + 1) for r in range(n) for c in range(n - 1)]
    links += [(r * n + c, (r + 1) * n + c) for r in range(n - 1) for c in range(n)]
    return [f"g{r:02d}-{c:02d}" for r in range(n) for c in range(n)], links


# 70 x 70: corner, mid-edge and centre (levels up to 140 wide), and every 113th node
GRID70_SRCS = sorted({0, 69, 35, 35 * 70, 35 * 70 + 35, 70 * 70 - 1} | set(range(0, 70 * 70, 113)))


# --- 1. never wide ---------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 40])
def test_never_wide_grid(eng, monkeypatch, n):
    """Every 7th source of a small grid. 32 x 32: no level is wider than 62, so every solve
    is one narrow run from level 1 to its end. 40 x 40: the same from the corners and edges
    (levels up to 40 wide); sources near the centre reach 78 and widen for a few levels."""
    monkeypatch.setenv("OPENR_SPF_RING_CAP", "512")
    names, links = grid_links(n)
    g = T.csr_from_links(names, np.array(links))
    dist, _ = solve_vs_oracle(eng, g, list(range(0, n * n, 7)))
    widest = [int(level_widths(d).max()) for d in dist]
    assert max(widest) <= 64 if n == 32 else (widest[0] == 40 and max(widest) == 78)


def test_never_wide_chain200(eng, monkeypatch):
    """200-node chain from both ends and the middle: levels of one or two nodes."""
    monkeypatch.setenv("OPENR_SPF_RING_CAP", "512")
    V = 200
    g = T.csr_from_links([f"p{i:03d}" for i in range(V)], np.array([(i, i + 1) for i in range(V - 1)]))
    dist, _ = solve_vs_oracle(eng, g, [0, V - 1, V // 2])
    assert int(dist[0, V - 1]) == V - 1


# --- 2. narrow, wide, narrow -------------------------------------------------------
@pytest.mark.parametrize("delta", ["1", "0"], ids=["delta-rows", "ellv-rows"])
def test_narrow_wide_narrow_grid70(eng, monkeypatch, delta):
    """70 x 70 grid: a solve starts narrow, widens past 64 (up to 140 from a corner) and
    ends narrow; with the 4-byte delta rows and with the 16-byte ellv rows."""
    monkeypatch.setenv("OPENR_SPF_LEAN_DELTA", delta)
    names, links = grid_links(70)
    g = T.csr_from_links(names, np.array(links))
    dist, ran = solve_vs_oracle(eng, g, GRID70_SRCS)
    w = level_widths(dist[GRID70_SRCS.index(35 * 70 + 35)])
    assert w[1] <= 64 and w.max() > 128 and w[-1] <= 64


# --- 3. a mode flip at every level, and the threshold -------------------------------
def layered_graph(a, layers=13, chain=30):
    """A chain of `chain` nodes, a fan-out from its last node (1, 3, 9, 27 nodes, then the
    a nodes of layer 0: every fan level is reached at once), then layers of alternating
    sizes a, 2a, a, ...: node k of a 2a-layer links to node k // 2 of both neighbouring
    a-layers. Degree <= 4, neighbour ids within 127. From the chain, the levels past the
    fan are a, 2a, a, ... wide."""
    sizes = [1, 3, 9, 27] + [a if i % 2 == 0 else 2 * a for i in range(layers)]
    base = np.concatenate([[0], np.cumsum(sizes)]) + (chain - 1)  # the fan's root is the chain's last node
    links = [(i, i + 1) for i in range(chain - 1)]
    for lv in range(4):  # fan: spread the children evenly, parents in order
        p, c = sizes[lv], sizes[lv + 1]
        links += [(int(base[lv]) + k * p // c, int(base[lv + 1]) + k) for k in range(c)]
    for lv in range(4, 4 + layers - 1):
        lo, hi = int(base[lv]), int(base[lv + 1])
        if sizes[lv] < sizes[lv + 1]:  # a-layer -> 2a-layer
            links += [(lo + k // 2, hi + k) for k in range(sizes[lv + 1])]
        else:
            links += [(lo + k, hi + k // 2) for k in range(sizes[lv])]
    V = int(base[-1])
    g = T.csr_from_links([f"n{i:04d}" for i in range(V)], np.array(links))
    return g, [int(b) for b in base]


@pytest.mark.parametrize("a", [32, 33])
def test_mode_flips_every_level(eng, monkeypatch, a):
    """a = 32: levels 32 / 64 wide, and 64 must stay narrow. a = 33: levels 33 / 66 wide,
    so the mode switches at every level (narrow runs of one level between wide levels)."""
    monkeypatch.setenv("OPENR_SPF_RING_CAP", "512")
    g, base = layered_graph(a)
    deg = np.diff(g.row_ptr)
    assert deg.max() <= 4
    srcs = [0, 29, base[4] + a // 2, base[5] + a, base[-2] + 1]  # chain ends, an a-layer, a 2a-layer, the last layer
    dist, _ = solve_vs_oracle(eng, g, srcs)
    w = level_widths(dist[0])
    assert w[33:33 + 13].tolist() == [a if i % 2 == 0 else 2 * a for i in range(13)], w.tolist()


# --- 4. overloads and down links ------------------------------------------------------
def test_overloads_and_down_links_grid70(eng):
    """5 % overloaded nodes and 5 % links down: parts of the grid are cut off, so a narrow
    run ends on an empty level before every node is reached; overloaded sources included."""
    names, links = grid_links(70)
    rng = np.random.default_rng(3)
    ovl = (rng.random(70 * 70) < 0.05).astype(np.uint8)
    up = (rng.random(len(links)) > 0.05).astype(np.uint8)
    g = T.csr_from_links(names, np.array(links), overloaded=ovl, link_up=up)
    srcs = sorted(set(GRID70_SRCS) | set(np.nonzero(ovl)[0][:6].tolist()))
    assert ovl[srcs].sum() >= 6
    dist, _ = solve_vs_oracle(eng, g, srcs)
    assert (dist == np.uint64(2**64 - 1)).any()  # unreachable nodes exist


# --- 5. overflow raised inside a narrow run ---------------------------------------------
def test_half_overflow_inside_narrow_run(eng, monkeypatch):
    """A ternary tree of depth 6 under a 20-node chain, queue halves of 32 entries: from
    the chain, the 27-node level (narrow) appends 81 entries. The solve is listed and the
    u16 full-order pass re-runs it."""
    monkeypatch.setenv("OPENR_SPF_RING_CAP", "64")
    monkeypatch.setenv("OPENR_SPF_LEAN_FORCE", "1")
    chain, depth = 20, 6
    ntree = (3 ** (depth + 1) - 1) // 2  # heap-indexed; its root is the chain's last node
    tid = lambda i: chain - 1 + i
    names = [f"n{i:04d}" for i in range(chain - 1 + ntree)]
    links = [(i, i + 1) for i in range(chain - 1)]
    links += [(tid(i), tid(3 * i + c)) for i in range((3 ** depth - 1) // 2) for c in (1, 2, 3)]
    g = T.csr_from_links(names, np.array(links))
    assert np.diff(g.row_ptr).max() <= 4
    dist, ran = solve_vs_oracle(eng, g, [0, 10, chain - 1, tid(5), tid(100), len(names) - 1])
    assert level_widths(dist[0])[chain - 1:].tolist() == [3 ** k for k in range(depth + 1)]
    assert any("rerun" in k for k in ran), ran


# --- 6. the 128-thread instantiation at small size ----------------------------------------
def test_block128_grid70_padded_batch(eng, monkeypatch, capfd):
    """The two-wave workgroups of a batch that fills the GPU more than twice over (6 200
    sources past 2 x 256 CUs x 12 workgroups), on the 70 x 70 grid: the sources of case 2
    repeated. Distinct sources against the oracle; duplicates equal their first copy."""
    monkeypatch.setenv("OPENR_SPF_PROF", "1")
    names, links = grid_links(70)
    g = T.csr_from_links(names, np.array(links))
    m, n = len(GRID70_SRCS), 6200
    srcs = np.resize(np.asarray(GRID70_SRCS, dtype=np.uint32), n)
    eng.set_graph(g)
    capfd.readouterr()
    dist, nh, _ = eng.solve(srcs, True)
    assert "bfs_ell_kernel" in eng.last_kernels()
    line = [l for l in capfd.readouterr().err.splitlines() if l.startswith("bfs_ell:")]
    assert line, "no bfs_ell: line"
    if "block=128" not in line[-1]:
        pytest.skip(f"this GPU runs {n} sources on {line[-1].split('|')[0]}")
    odist, onh = Oracle(g).all_sources(srcs[:m], True, nthreads=16)
    assert np.array_equal(dist[:m], odist) and np.array_equal(nh[:m], onh)
    first = np.arange(n) % m
    assert np.array_equal(dist, dist[first]) and np.array_equal(nh, nh[first])


# --- 7. the benchmarked shape ran the narrow mode -------------------------------------------
def test_profile_counts_grid100(eng, monkeypatch, capfd):
    """G100, all 10 000 sources: the profiling variant's counts. Summed over all sources
    the Manhattan rings give 148.0 expanded levels per solve, 69.4 of them at most 64 wide,
    in exactly two runs per solve (one at the start, one at the end). The rows of this
    launch are checked by test_config3_grid100_all_sources."""
    monkeypatch.setenv("OPENR_SPF_PROF", "1")
    eng.set_graph(T.grid_fast(100))
    capfd.readouterr()
    eng.solve(np.arange(10000, dtype=np.uint32), True, want_nh=True)
    assert "bfs_ell_kernel" in eng.last_kernels()
    line = [l for l in capfd.readouterr().err.splitlines() if l.startswith("bfs_ell:")]
    assert line, "no bfs_ell: line"
    print(line[-1])
    f = lambda key: float(re.search(re.escape(key) + r"\s*=?\s*([0-9.]+)", line[-1]).group(1))
    assert f("levels/solve") == 148.0
    assert abs(f("narrow levels/solve") - 69.4) <= 0.1
    assert f("narrow runs/solve") == 2.0
