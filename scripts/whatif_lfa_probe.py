"""Post-failure loop-free alternates on the config-4 WAN, six legs in one process (tuning aid):

(a) openr_spf_whatif_lfa_device, counts only: all 1 000 node-failure sets x all 1 000 sources,
    a dense group table (the 1 000 loopbacks plus 200 random groups of 2-6 nodes);
(b) the same with entries;
(c) openr_spf_whatif_routes_device on the same inputs (the route pass of DESIGN.md 5.9);
(d) the node sweep alone: openr_spf_whatif_sets_delta_device (every node is a source here, so
    the closure the LFA call sweeps is the source list itself; the LFA pass's share of (a) / (b)
    and the route pass's share of (c) are the differences to this leg);
(e) host: the node delta of leg (d) copied out and the rule applied in numpy, for a subsample
    of `host_sets` evenly spaced sets (all sources); its counts are checked against (a)'s;
(f) per set: set_graph(failed graph) + lfa_routes_device, for the same subsample.

After a warm-up the device legs (a)-(d) alternate; every step is timed with a host clock
around a device synchronise.

    python scripts/whatif_lfa_probe.py [steps] [host_sets]
"""
import dataclasses
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openr_amd import topology as T  # noqa: E402
from openr_amd.engine import SpfEngine  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
host_sets = int(sys.argv[2]) if len(sys.argv) > 2 else 10
U64_MAX = np.uint64(2**64 - 1)
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
g = T.wan(1000, 3000, 64, seed=1)
eng = SpfEngine([0])
eng.set_graph(g)
V, nb = g.num_nodes, eng.nh_bytes
sets = T.node_failure_sets(g)
n_sets = len(sets)
rng = np.random.default_rng(7)
groups = T.loopback_groups(g) + T.prefix_groups(
    g, [rng.choice(V, int(rng.integers(2, 7)), replace=False).tolist() for _ in range(200)])
G = len(groups)


def csr(lists):
    p = np.zeros(len(lists) + 1, dtype=np.int64)
    p[1:] = np.cumsum([len(x) for x in lists])
    return p, np.concatenate([np.asarray(x, dtype=np.int64) for x in lists])


sp, sl = csr(sets)
gp, gn = csr(groups)
d_sp, d_sl = (torch.from_numpy(a.astype(np.int32)).to(dev) for a in (sp, sl))
d_gp, d_gn = (torch.from_numpy(a.astype(np.int32)).to(dev) for a in (gp, gn))
srcs = torch.arange(V, dtype=torch.int32, device=dev)
units = n_sets * V
s = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(s)
sets_args = (d_sp.data_ptr(), d_sl.data_ptr(), n_sets, int(sl.shape[0]), srcs.data_ptr(), V)
grp_args = (d_gp.data_ptr(), d_gn.data_ptr(), G, int(gn.shape[0]))


def i32(*shape):
    return torch.empty(shape, dtype=torch.int32, device=dev)


def i64(*shape):
    return torch.empty(shape, dtype=torch.int64, device=dev)


def u8(*shape):
    return torch.empty(shape, dtype=torch.uint8, device=dev)


# sizes from count-only passes
l_changed, l_unprot, l_lost, l_ptr = i32(n_sets, V), i32(n_sets, V), i32(n_sets, V), i64(units + 1)
l_total, _ = eng.whatif_lfa_device(*sets_args, *grp_args, l_changed.data_ptr(), l_unprot.data_ptr(), l_lost.data_ptr(),
                                   nh_bytes=nb, stream=s.cuda_stream)
r_changed, r_ptr = i32(n_sets, V), i64(units + 1)
r_total, _ = eng.whatif_routes_device(*sets_args, *grp_args, r_changed.data_ptr(), r_ptr.data_ptr(), 0, 0, 0, 0, 0, nb,
                                      True, stream=s.cuda_stream, allow_overflow=True)
n_changed, n_ptr = i32(n_sets, V), i64(units + 1)
n_total, _ = eng.whatif_sets_delta_device(*sets_args, n_changed.data_ptr(), n_ptr.data_ptr(), 0, 0, 0, 0, nb, True,
                                          stream=s.cuda_stream, allow_overflow=True)
l_group, l_metric = i32(max(l_total, 1)), i64(max(l_total, 1))
l_nh, l_alt = u8(max(l_total, 1), nb), u8(max(l_total, 1), nb)
r_group, r_metric, r_nh, r_nbest = i32(max(r_total, 1)), i64(max(r_total, 1)), u8(max(r_total, 1), nb), i32(max(r_total, 1))
n_node, n_dist, n_nh = i32(max(n_total, 1)), i64(max(n_total, 1)), u8(max(n_total, 1), nb)
kernels = [None]


def leg_lfa_counts():
    eng.whatif_lfa_device(*sets_args, *grp_args, l_changed.data_ptr(), l_unprot.data_ptr(), l_lost.data_ptr(),
                          nh_bytes=nb, stream=s.cuda_stream)


def leg_lfa_entries():
    eng.whatif_lfa_device(*sets_args, *grp_args, l_changed.data_ptr(), l_unprot.data_ptr(), l_lost.data_ptr(),
                          l_ptr.data_ptr(), l_group.data_ptr(), l_metric.data_ptr(), l_nh.data_ptr(), l_alt.data_ptr(),
                          l_total, nb, stream=s.cuda_stream)
    kernels[0] = sorted(set(eng.last_kernels()))


def leg_routes():
    eng.whatif_routes_device(*sets_args, *grp_args, r_changed.data_ptr(), r_ptr.data_ptr(), r_group.data_ptr(),
                             r_metric.data_ptr(), r_nh.data_ptr(), r_nbest.data_ptr(), r_total, nb, True,
                             stream=s.cuda_stream)


def leg_nodes():
    eng.whatif_sets_delta_device(*sets_args, n_changed.data_ptr(), n_ptr.data_ptr(), n_node.data_ptr(),
                                 n_dist.data_ptr(), n_nh.data_ptr(), n_total, nb, True, stream=s.cuda_stream)


# every (source, distinct neighbour) pair: source, neighbour, next-hop bit, the links between them
pair_s, pair_n, pair_b, pair_links = [], [], [], []
for u in range(V):
    nbrs = g.distinct_neighbors(u)
    for b, x in enumerate(nbrs):
        pair_s.append(u)
        pair_n.append(x)
        pair_b.append(b)
        pair_links.append({int(g.link_id[e]) for e in g.row(u) if int(g.col[e]) == x and g.edge_up[e]})
pair_s, pair_n, pair_b = (np.asarray(a, dtype=np.int64) for a in (pair_s, pair_n, pair_b))
starts = gp[:-1]


def lfa_rule(dist, nh, failed):
    """(metric [V, G], nh [V, G, nb], alt [V, G, nb]) of every source on rows dist [V, V] /
    nh [V, V, nb] with the links of `failed` down."""
    gmin = np.minimum.reduceat(dist[:, gn], starts, axis=1)  # [row, G]: no group of the table is empty
    at = (dist[:, gn] == np.repeat(gmin, np.diff(gp), axis=1)) & (np.repeat(gmin, np.diff(gp), axis=1) != U64_MAX)
    rnh = np.bitwise_or.reduceat(np.where(at[:, :, None], nh[:, gn], np.uint8(0)), starts, axis=1)
    tested = np.array([bool(ls - failed) for ls in pair_links])
    es, en, eb = pair_s[tested], pair_n[tested], pair_b[tested]
    bound = gmin[es] + dist[en, es][:, None]
    ok = (gmin[es] != U64_MAX) & (gmin[en] != U64_MAX) & (gmin[en] < bound)  # [pair, G]
    alt = np.zeros((V, G, nb), dtype=np.uint8)
    for b in np.unique(eb):  # one pair per source and bit
        m = eb == b
        alt[es[m], :, b >> 3] |= ok[m].astype(np.uint8) << np.uint8(b & 7)
    return gmin, rnh, alt


def popcount(a):
    return np.unpackbits(a, axis=-1).sum(axis=-1)


def leg_host(pick, split):
    """Leg (e) for the sets of `pick`: (changed, unprotected, lost_backup) [len(pick), V]."""
    t0 = time.perf_counter()
    leg_nodes()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ptr = n_ptr.cpu().numpy()
    node = n_node.cpu().numpy().astype(np.int64)
    dist = n_dist.cpu().numpy().view(np.uint64)
    nh = n_nh.cpu().numpy()
    t2 = time.perf_counter()
    bdist, bnh, _ = eng.solve(list(range(V)), True)
    bm, bh, ba = lfa_rule(bdist, bnh, set())
    b_live, b_pc = (bm != U64_MAX) & bh.any(axis=2), popcount(bh | ba)
    out = np.zeros((3, len(pick), V), dtype=np.int64)
    for x, i in enumerate(pick):
        fd, fh = bdist.copy(), bnh.copy()
        a, e = int(ptr[i * V]), int(ptr[(i + 1) * V])
        rows = np.repeat(np.arange(V), np.diff(ptr[i * V:(i + 1) * V + 1]))
        fd[rows, node[a:e]] = dist[a:e]
        fh[rows, node[a:e]] = nh[a:e]
        fm, fnh, fa = lfa_rule(fd, fh, set(sets[i]))
        ch = (fm != bm) | (fnh != bh).any(axis=2) | (fa != ba).any(axis=2)
        one = (fm != U64_MAX) & fnh.any(axis=2) & (popcount(fnh | fa) == 1)
        out[0, x], out[1, x], out[2, x] = ch.sum(axis=1), one.sum(axis=1), (b_live & (b_pc >= 2) & one).sum(axis=1)
    t3 = time.perf_counter()
    split.append((t1 - t0, t2 - t1, t3 - t2))
    return out


def leg_set_graph(pick):
    """Leg (f): one mirror rebuild and one lfa_routes_device per set; seconds in all."""
    m, h, a = i64(V, G), u8(V, G, nb), u8(V, G, nb)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in pick:
        up = g.edge_up.copy()
        up[np.isin(g.link_id, sets[i])] = 0
        eng.set_graph(dataclasses.replace(g, edge_up=up))
        eng.lfa_routes_device(srcs.data_ptr(), V, *grp_args, m.data_ptr(), h.data_ptr(), a.data_ptr(), nb,
                              stream=s.cuda_stream)
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    eng.set_graph(g)
    return dt


legs = (("whatif_lfa_device, counts only", leg_lfa_counts), ("whatif_lfa_device, entries", leg_lfa_entries),
        ("whatif_routes_device", leg_routes), ("whatif_sets_delta_device (node sweep alone)", leg_nodes))
times = {name: [] for name, _ in legs}
for name, f in legs:  # warm-up
    f()
    torch.cuda.synchronize()
for _ in range(steps):
    for name, f in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        times[name].append(time.perf_counter() - t0)
print(f"WAN V={V} L={g.num_links}: {n_sets} node-failure sets x {V} sources = {units} units; {G} groups "
      f"({int(gn.shape[0])} members); kernels: {kernels[0]}")
med = {}
for name, _ in legs:
    t = np.array(times[name]) * 1e3
    med[name] = float(np.median(t))
    print(f"{name}: median {np.median(t):.1f} ms per step (min {t.min():.1f}, max {t.max():.1f}, {steps} steps)")
a, b, c, d = (med[name] for name, _ in legs)
print(f"LFA pass (difference of the medians to the node sweep): counts only {a - d:.1f} ms, entries {b - d:.1f} ms; "
      f"route pass {c - d:.1f} ms; LFA pass / route pass = {(a - d) / max(c - d, 1e-9):.1f}x (counts), "
      f"{(b - d) / max(c - d, 1e-9):.1f}x (entries)")
lc = l_changed.cpu().numpy().astype(np.int64)
print(f"changed nodes {n_total} (mean {n_total / units:.2f} per unit); changed routes {r_total} "
      f"(mean {r_total / units:.2f}); changed LFA entries {l_total} (mean {l_total / units:.2f}); "
      f"unprotected {int(l_unprot.sum())}; lost_backup {int(l_lost.sum())}; units with a changed entry "
      f"{int((lc > 0).sum())}", flush=True)
pick = [int(x) for x in np.linspace(0, n_sets - 1, host_sets).round()] if host_sets else []
if pick:
    split = []
    hc = leg_host(pick, split)
    same = all(bool((hc[k] == t.cpu().numpy()[pick]).all()) for k, t in enumerate((l_changed, l_unprot, l_lost)))
    sw, cp, rs = split[-1]
    print(f"host leg, {len(pick)} evenly spaced sets of {n_sets} x all sources: node sweep (all sets) {1e3 * sw:.1f} ms "
          f"+ copy to host {1e3 * cp:.1f} ms + numpy rule {1e3 * rs:.1f} ms ({1e3 * rs / len(pick):.1f} ms per set, "
          f"{rs / len(pick) * n_sets:.1f} s for all sets at that rate); changed / unprotected / lost_backup equal "
          f"the device's: {same}", flush=True)
    dt = leg_set_graph(pick)
    print(f"set_graph + lfa_routes_device per set, the same {len(pick)} sets: {1e3 * dt / len(pick):.1f} ms per set "
          f"({dt / len(pick) * n_sets:.1f} s for all sets at that rate)", flush=True)
eng.close()
