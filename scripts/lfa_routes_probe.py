"""All-sources loop-free alternates, three legs in one process (tuning aid), on two topologies:

WAN     1 000 nodes / 3 000 links, all 1 000 sources, the DESIGN 5.9 table of 1 200 groups
        (the 1 000 loopbacks plus 200 random groups of 2-6 nodes);
fabric  all 4 992 sources x the 4 992 loopback groups.

(a) openr_spf_lfa_routes_device, counts only (one pass) and with entries (count, scan, emit);
(b) openr_spf_routes_device of the same sources and groups: the shortest-path half alone.
    (a) - (b) is the LFA pass with the solves of the rows that are no source; it is set
    against the pass's read volume, sum over sources of up-degree x members x 8 B;
(c) the same rows copied to the host (openr_spf_solve) and resolved in numpy by the rule of
    openr_spf_lfa_routes, its counts checked against the device's.

After a warm-up the device legs alternate; every step is timed with a host clock around a
device synchronise; medians with min-max over `steps` (>= 7) steps.

    python scripts/lfa_routes_probe.py [steps] [wan|fabric|both] [host_steps]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openr_amd import topology as T  # noqa: E402
from openr_amd.engine import SpfEngine  # noqa: E402

steps = max(7, int(sys.argv[1])) if len(sys.argv) > 1 else 7
which = sys.argv[2] if len(sys.argv) > 2 else "both"
host_steps = int(sys.argv[3]) if len(sys.argv) > 3 else 1
U64_MAX = np.uint64(2**64 - 1)
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)


def host_resolve(eng, g, groups, gp, gn):
    """Leg (c): n_alt [V, G] from host rows. Returns (counts, seconds of solve + copy, of numpy)."""
    V, G = g.num_nodes, len(groups)
    t0 = time.perf_counter()
    dist, _, _ = eng.solve(list(range(V)), True, want_nh=False)
    t1 = time.perf_counter()
    sizes = np.diff(gp)
    full = np.nonzero(sizes)[0]  # reduceat needs non-empty segments
    starts = gp[full]
    seg = np.repeat(np.arange(full.shape[0]), sizes[full])
    n_alt = np.zeros((V, G), dtype=np.uint32)
    for s in range(V):
        metric = np.full(G, U64_MAX, dtype=np.uint64)
        metric[full] = np.minimum.reduceat(dist[s][gn], starts)
        reached = metric[full] != U64_MAX
        e0, e1 = int(g.row_ptr[s]), int(g.row_ptr[s + 1])
        for x in np.unique(g.col[e0:e1][g.edge_up[e0:e1] != 0]):
            dn = dist[x]
            bound = np.where(reached, metric[full] + dn[s], np.uint64(0))  # unreached: nothing qualifies
            q = dn[gn] < bound[seg]
            n_alt[s, full] += np.logical_or.reduceat(q, starts).astype(np.uint32)
    return n_alt, t1 - t0, time.perf_counter() - t1


def probe(name, g, groups):
    eng = SpfEngine([0])
    eng.set_graph(g)
    V, nb, G = g.num_nodes, eng.nh_bytes, len(groups)
    gp = np.zeros(G + 1, dtype=np.int64)
    gp[1:] = np.cumsum([len(x) for x in groups])
    gn = np.concatenate([np.asarray(x, dtype=np.int64) for x in groups])
    d_gp, d_gn = (torch.from_numpy(a.astype(np.int32)).to(dev) for a in (gp, gn))
    srcs = torch.arange(V, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    head = (srcs.data_ptr(), V, d_gp.data_ptr(), d_gn.data_ptr(), G, int(gn.shape[0]))
    metric = torch.empty((V, G), dtype=torch.int64, device=dev)
    nh = torch.empty((V, G, nb), dtype=torch.uint8, device=dev)
    alt = torch.empty((V, G, nb), dtype=torch.uint8, device=dev)
    n_alt = torch.empty((V, G), dtype=torch.int32, device=dev)
    ptr = torch.empty(V * G + 1, dtype=torch.int64, device=dev)
    r_metric = torch.empty((V, G), dtype=torch.int64, device=dev)
    r_nh = torch.empty((V, G, nb), dtype=torch.uint8, device=dev)
    out = (metric.data_ptr(), nh.data_ptr(), alt.data_ptr(), nb, n_alt.data_ptr())
    total, solved = eng.lfa_routes_device(*head, *out, ptr.data_ptr(), 0, 0, 0, stream=s.cuda_stream,
                                          allow_overflow=True)
    e_nbr = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    e_am = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    kernels = [None]

    def leg_counts():
        eng.lfa_routes_device(*head, *out, stream=s.cuda_stream)

    def leg_entries():
        eng.lfa_routes_device(*head, *out, ptr.data_ptr(), e_nbr.data_ptr(), e_am.data_ptr(), total,
                              stream=s.cuda_stream)
        kernels[0] = sorted(set(eng.last_kernels()))

    def leg_routes():
        eng.routes_device(*head, r_metric.data_ptr(), r_nh.data_ptr(), nb, stream=s.cuda_stream)

    legs = (("lfa_routes_device, counts only", leg_counts), ("lfa_routes_device, with entries", leg_entries),
            ("routes_device (shortest-path half alone)", leg_routes))
    times = {nm: [] for nm, _ in legs}
    for _, f in legs:  # warm-up
        f()
        torch.cuda.synchronize()
    for _ in range(steps):
        for nm, f in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[nm].append(time.perf_counter() - t0)
    assert bool((metric == r_metric).all()) and bool((nh == r_nh).all())
    up = np.array([len(np.unique(g.col[g.row_ptr[v]:g.row_ptr[v + 1]][g.edge_up[g.row_ptr[v]:g.row_ptr[v + 1]] != 0]))
                   for v in range(V)])
    volume = float(up.sum()) * float(gn.shape[0]) * 8.0
    print(f"{name}: V={V} L={g.num_links} nh_bytes={nb}; {V} sources x {G} groups ({int(gn.shape[0])} members); "
          f"rows solved {solved}; alternates {total} (mean {total / (V * G):.2f} per route); kernels: {kernels[0]}")
    med = {}
    for nm, _ in legs:
        t = np.array(times[nm]) * 1e3
        med[nm] = float(np.median(t))
        print(f"  {nm}: median {np.median(t):.2f} ms per step (min {t.min():.2f}, max {t.max():.2f}, {steps} steps)")
    a1, a2, b = (med[nm] for nm, _ in legs)
    print(f"  LFA pass (counts - routes, difference of the medians): {a1 - b:.2f} ms; its reads, sum of up-degree x "
          f"members x 8 B = {volume / 1e9:.3f} GB -> {volume / 1e9 / max(a1 - b, 1e-6) * 1e3:.0f} GB/s; "
          f"entries cost {a2 - a1:.2f} ms more", flush=True)
    dev_counts = n_alt.cpu().numpy().view(np.uint32)
    for k in range(host_steps):
        counts, t_rows, t_np = host_resolve(eng, g, groups, gp, gn)
        print(f"  host resolve step {k}: {1e3 * (t_rows + t_np):.1f} ms = solve and copy to host {1e3 * t_rows:.1f} + "
              f"numpy resolve {1e3 * t_np:.1f}; counts equal the device's: {bool((counts == dev_counts).all())}",
              flush=True)
    eng.close()


if which in ("wan", "both"):
    g = T.wan(1000, 3000, 64, seed=1)
    rng = np.random.default_rng(7)
    probe("WAN", g, T.loopback_groups(g) + T.prefix_groups(
        g, [rng.choice(g.num_nodes, int(rng.integers(2, 7)), replace=False).tolist() for _ in range(200)]))
if which in ("fabric", "both"):
    g = T.fabric(5000)
    probe("fabric", g, T.loopback_groups(g))
