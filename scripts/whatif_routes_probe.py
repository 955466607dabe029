"""Route-level node-failure sweep on the config-4 WAN, three legs in one process (tuning aid):

(a) openr_spf_whatif_routes_device: all 1 000 node-failure sets x all 1 000 sources, a dense
    group table (the 1 000 loopbacks plus 200 random groups of 2-6 nodes);
(b) the node sweep it contains, alone: openr_spf_whatif_sets_delta_device (the route pass's
    share of (a) is the difference);
(c) the only way to the same answer without (a): leg (b), its delta copied to the host, and
    the routes resolved there in numpy (base routes from openr_spf_solve rows, candidates
    through the inverse map, segment minimum / OR), in chunks of sets.

After a warm-up the device legs alternate; every step is timed with a host clock around a
device synchronise. Leg (c) runs `host_steps` times and its counts are checked against (a).

    python scripts/whatif_routes_probe.py [steps] [host_steps] [sets per host chunk]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openr_amd import topology as T  # noqa: E402
from openr_amd.engine import SpfEngine  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
host_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1
host_chunk = int(sys.argv[3]) if len(sys.argv) > 3 else 100
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

# sizes from count-only passes
r_changed = torch.empty((n_sets, V), dtype=torch.int32, device=dev)
r_ptr = torch.empty(units + 1, dtype=torch.int64, device=dev)
r_total, _ = eng.whatif_routes_device(*sets_args, d_gp.data_ptr(), d_gn.data_ptr(), G, int(gn.shape[0]),
                                      r_changed.data_ptr(), r_ptr.data_ptr(), 0, 0, 0, 0, 0, nb, True,
                                      stream=s.cuda_stream, allow_overflow=True)
n_changed = torch.empty((n_sets, V), dtype=torch.int32, device=dev)
n_ptr = torch.empty(units + 1, dtype=torch.int64, device=dev)
n_total, _ = eng.whatif_sets_delta_device(*sets_args, n_changed.data_ptr(), n_ptr.data_ptr(), 0, 0, 0, 0, nb, True,
                                          stream=s.cuda_stream, allow_overflow=True)
r_group = torch.empty(max(r_total, 1), dtype=torch.int32, device=dev)
r_metric = torch.empty(max(r_total, 1), dtype=torch.int64, device=dev)
r_nh = torch.empty((max(r_total, 1), nb), dtype=torch.uint8, device=dev)
r_nbest = torch.empty(max(r_total, 1), dtype=torch.int32, device=dev)
n_node = torch.empty(max(n_total, 1), dtype=torch.int32, device=dev)
n_dist = torch.empty(max(n_total, 1), dtype=torch.int64, device=dev)
n_nh = torch.empty((max(n_total, 1), nb), dtype=torch.uint8, device=dev)
kernels = [None]


def leg_routes():
    eng.whatif_routes_device(*sets_args, d_gp.data_ptr(), d_gn.data_ptr(), G, int(gn.shape[0]), r_changed.data_ptr(),
                             r_ptr.data_ptr(), r_group.data_ptr(), r_metric.data_ptr(), r_nh.data_ptr(),
                             r_nbest.data_ptr(), r_total, nb, True, stream=s.cuda_stream)
    kernels[0] = sorted(set(eng.last_kernels()))


def leg_nodes():
    eng.whatif_sets_delta_device(*sets_args, n_changed.data_ptr(), n_ptr.data_ptr(), n_node.data_ptr(),
                                 n_dist.data_ptr(), n_nh.data_ptr(), n_total, nb, True, stream=s.cuda_stream)


def reduce_rows(dist, nh):
    """The route rule on full rows: (metric [R, G], nh [R, G, nb])."""
    metric = np.full((dist.shape[0], G), U64_MAX, dtype=np.uint64)
    rnh = np.zeros((dist.shape[0], G, nb), dtype=np.uint8)
    for k, grp in enumerate(groups):
        sub = dist[:, grp]
        mn = sub.min(axis=1)
        at = (sub == mn[:, None]) & (mn != U64_MAX)[:, None]
        metric[:, k] = mn
        rnh[:, k] = np.bitwise_or.reduce(np.where(at[:, :, None], nh[:, grp], np.uint8(0)), axis=1)
    return metric, rnh


inv_order = np.argsort(gn, kind="stable")  # inverse map node -> groups
inv = np.repeat(np.arange(G), np.diff(gp))[inv_order]
ip = np.zeros(V + 1, dtype=np.int64)
ip[1:] = np.cumsum(np.bincount(gn, minlength=V))


def seg_expand(starts, sizes):
    """Indices starts[i] .. starts[i] + sizes[i] of every segment, and each one's segment id."""
    seg = np.repeat(np.arange(sizes.shape[0]), sizes)
    return starts[seg] + np.arange(seg.shape[0]) - np.repeat(np.cumsum(sizes) - sizes, sizes), seg


def leg_host(split):
    """Leg (c); fills split with the seconds of its phases; returns changed routes per unit."""
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
    bm, bh = reduce_rows(bdist, bnh)
    counts = np.zeros(units, dtype=np.int64)
    for i0 in range(0, n_sets, host_chunk):
        u0, u1 = i0 * V, min(n_sets, i0 + host_chunk) * V
        a, e = int(ptr[u0]), int(ptr[u1])
        if a == e:
            continue
        en, ed, eh = node[a:e], dist[a:e], nh[a:e]
        eu = np.repeat(np.arange(u0, u1), np.diff(ptr[u0 : u1 + 1]))
        # candidates: the (unit, group) pairs with a changed member
        at_inv, pe = seg_expand(ip[en], ip[en + 1] - ip[en])
        key = np.unique(eu[pe] * G + inv[at_inv])
        cu, ck = key // G, key % G
        at_gn, mc = seg_expand(gp[ck], gp[ck + 1] - gp[ck])
        mv, mu = gn[at_gn], cu[mc]
        # member values: the unit's delta entry where there is one, else the base row
        ekey = eu * V + en
        order = np.argsort(ekey, kind="stable")
        q = mu * V + mv
        pos = np.minimum(np.searchsorted(ekey[order], q), ekey.shape[0] - 1)
        hit = ekey[order][pos] == q
        ent = order[pos]
        d = np.where(hit, ed[ent], bdist[mu % V, mv])
        starts = np.cumsum(gp[ck + 1] - gp[ck]) - (gp[ck + 1] - gp[ck])
        mn = np.minimum.reduceat(d, starts)
        best = (d == mn[mc]) & (mn[mc] != U64_MAX)
        h = np.where((hit & best)[:, None], eh[ent], np.where(best[:, None], bnh[mu % V, mv], np.uint8(0)))
        rnh = np.bitwise_or.reduceat(h, starts, axis=0)
        ch = (mn != bm[cu % V, ck]) | (rnh != bh[cu % V, ck]).any(axis=1)
        counts += np.bincount(cu[ch], minlength=units)
    t3 = time.perf_counter()
    split.append((t1 - t0, t2 - t1, t3 - t2))
    return counts


legs = (("whatif_routes_device", leg_routes), ("whatif_sets_delta_device (node sweep alone)", leg_nodes))
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
a, b = (med[name] for name, _ in legs)
print(f"route pass (difference of the medians): {a - b:.1f} ms = {100.0 * (a - b) / b:.1f}% over the node sweep")
print(f"changed nodes {n_total} (mean {n_total / units:.2f} per unit); changed routes {r_total} "
      f"(mean {r_total / units:.2f} per unit)", flush=True)
split = []
for k in range(host_steps):
    counts = leg_host(split)
    same = bool((counts == r_changed.cpu().numpy().reshape(-1)).all())
    sw, cp, rs = split[-1]
    print(f"host resolve step {k}: {1e3 * (sw + cp + rs):.1f} ms = node sweep {1e3 * sw:.1f} + copy to host "
          f"{1e3 * cp:.1f} + numpy resolve {1e3 * rs:.1f}; counts equal the device's: {same}", flush=True)
eng.close()
