"""Loop-free alternates under maintenance events on the config-4 WAN (tuning aid): 1 000 nodes,
3 000 links, all 1 000 sources, the 1 200-group table of the route probes. The events are
those of scripts/whatif_maint_probe.py: event r overloads router r and soft-drains the
advertised adjacencies of router (r + 1) mod 1 000 by +1000.

The legs, alternating in one process after a warm-up:

(a) openr_spf_whatif_maint_lfa_device, counts only (d_ptr NULL);
(b) the same with every changed entry written out;
(c) openr_spf_whatif_maint_routes_device on the same inputs;
(e) the way to (a)'s answer without the sweep, on 9 evenly spaced events: patch_graph (the
    event's overload bit and metrics), lfa_routes_device of every source, a compare against the
    base entries on the device, patch_graph (back). Its counts are checked against (a), its
    time extrapolated.

Every step is timed with a host clock around a device synchronise; medians with min-max.

    python scripts/whatif_maint_lfa_probe.py [steps]
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
RAISE = 1000
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
g = T.wan(1000, 3000, 64, seed=1)
V = g.num_nodes
rng = np.random.default_rng(7)
groups = T.loopback_groups(g) + T.prefix_groups(
    g, [rng.choice(V, int(rng.integers(2, 7)), replace=False).tolist() for _ in range(200)])
G = len(groups)
nodes = [[v] for v in range(V)]
edges, metrics = T.soft_drain_events(g, [[(v + 1) % V] for v in range(V)], RAISE)
n_ev = V


def csr(*lists):
    p = np.zeros(len(lists[0]) + 1, dtype=np.int64)
    p[1:] = np.cumsum([len(x) for x in lists[0]])
    out = [torch.from_numpy(p.astype(np.int32)).to(dev)]
    for ls in lists:
        flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in ls] + [np.zeros(0, dtype=np.int64)])
        out.append(torch.from_numpy(np.concatenate([flat, np.zeros(1, np.int64)]).astype(np.int32)).to(dev))
    return out


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def line(t):
    t = np.array(t) * 1e3
    return f"median {np.median(t):.2f} ms (min {t.min():.2f}, max {t.max():.2f})"


eng = SpfEngine([0])
eng.set_graph(g)
nb = eng.nh_bytes
d_np, d_nn = csr(nodes)
d_ep, d_ee, d_mm = csr(edges, metrics)
d_gp, d_gn = csr(groups)
srcs = torch.arange(V, dtype=torch.int32, device=dev)
units = n_ev * V
s = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(s)
ev_args = (d_np.data_ptr(), d_nn.data_ptr(), 0, 0, d_ep.data_ptr(), d_ee.data_ptr(), d_mm.data_ptr(), n_ev,
           d_nn.numel() - 1, 0, d_ee.numel() - 1)
src_args = (srcs.data_ptr(), V)
grp_args = (d_gp.data_ptr(), d_gn.data_ptr(), G, d_gn.numel() - 1)
changed = torch.empty((n_ev, V), dtype=torch.int32, device=dev)
unprot = torch.empty((n_ev, V), dtype=torch.int32, device=dev)
lost = torch.empty((n_ev, V), dtype=torch.int32, device=dev)
ptr = torch.empty(units + 1, dtype=torch.int64, device=dev)
total, solved = eng.whatif_maint_lfa_device(*ev_args, *src_args, *grp_args, changed.data_ptr(), unprot.data_ptr(),
                                            lost.data_ptr(), nh_bytes=nb, stream=s.cuda_stream)
kernels = eng.last_kernels()
a_changed = changed.cpu().numpy().copy()
a_lost = int(lost.sum().item())
e_group = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
e_metric = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
e_nh = torch.empty((max(total, 1), nb), dtype=torch.uint8, device=dev)
e_alt = torch.empty((max(total, 1), nb), dtype=torch.uint8, device=dev)
r_changed = torch.empty((n_ev, V), dtype=torch.int32, device=dev)
r_ptr = torch.empty(units + 1, dtype=torch.int64, device=dev)
r_total, _ = eng.whatif_maint_routes_device(*ev_args, *src_args, *grp_args, r_changed.data_ptr(), r_ptr.data_ptr(), 0, 0,
                                            0, 0, 0, nb, stream=s.cuda_stream, allow_overflow=True)
r_group = torch.empty(max(r_total, 1), dtype=torch.int32, device=dev)
r_metric = torch.empty(max(r_total, 1), dtype=torch.int64, device=dev)
r_nh = torch.empty((max(r_total, 1), nb), dtype=torch.uint8, device=dev)
r_nbest = torch.empty(max(r_total, 1), dtype=torch.int32, device=dev)


def leg_counts():
    eng.whatif_maint_lfa_device(*ev_args, *src_args, *grp_args, changed.data_ptr(), unprot.data_ptr(), lost.data_ptr(),
                                nh_bytes=nb, stream=s.cuda_stream)


def leg_entries():
    eng.whatif_maint_lfa_device(*ev_args, *src_args, *grp_args, changed.data_ptr(), unprot.data_ptr(), lost.data_ptr(),
                                ptr.data_ptr(), e_group.data_ptr(), e_metric.data_ptr(), e_nh.data_ptr(),
                                e_alt.data_ptr(), total, nb, stream=s.cuda_stream)


def leg_routes():
    eng.whatif_maint_routes_device(*ev_args, *src_args, *grp_args, r_changed.data_ptr(), r_ptr.data_ptr(),
                                   r_group.data_ptr(), r_metric.data_ptr(), r_nh.data_ptr(), r_nbest.data_ptr(), r_total,
                                   nb, stream=s.cuda_stream)


legs = (("(a) lfa pass, counts only", leg_counts), ("(b) lfa pass with the entries", leg_entries),
        ("(c) the sweep resolved to routes", leg_routes))
times = {name: [] for name, _ in legs}
for _, f in legs:  # warm-up
    timed(f)
for _ in range(steps):
    for name, f in legs:
        times[name].append(timed(f))
print(f"[maint] WAN V={V} L={g.num_links}: {n_ev} events x {V} sources = {units} units, "
      f"{int((a_changed != 0).sum())} with a changed entry; changed entries {total} (max {int(a_changed.max())} "
      f"per unit), lost_backup {a_lost}; changed routes {r_total}; {G} groups; solved {solved}; kernels of (a): "
      f"{kernels}")
for name, _ in legs:
    print(f"[maint] {name}: {line(times[name])} per step, {steps} steps")
ma, mc = (float(np.median(times[legs[k][0]])) * 1e3 for k in (0, 2))
print(f"[maint] (a) / (c) = {ma / mc:.2f}; (a) per event {ma / n_ev:.4f} ms", flush=True)

# (e) the old way on 9 evenly spaced events
b_metric = torch.empty((V, G), dtype=torch.int64, device=dev)
b_nh = torch.empty((V, G, nb), dtype=torch.uint8, device=dev)
b_alt = torch.empty((V, G, nb), dtype=torch.uint8, device=dev)
o_metric, o_nh, o_alt = torch.empty_like(b_metric), torch.empty_like(b_nh), torch.empty_like(b_alt)


def lfa_routes(m, h, a):
    eng.lfa_routes_device(srcs.data_ptr(), V, d_gp.data_ptr(), d_gn.data_ptr(), G, d_gn.numel() - 1, m.data_ptr(),
                          h.data_ptr(), a.data_ptr(), nb)


lfa_routes(b_metric, b_nh, b_alt)
torch.cuda.synchronize()
picks = [int(x) for x in np.linspace(0, n_ev - 1, 9).astype(np.int64)]
old, same = [], True
for _ in range(2):  # the first round warms the patch path up
    old = []
    for x in picks:
        nd, ed = nodes[x], edges[x]
        was = [int(g.metric[e]) for e in ed]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.patch(edges=ed, metrics=metrics[x], links=[], link_up=[], nodes=nd, node_overloaded=[1] * len(nd),
                  track=False)
        lfa_routes(o_metric, o_nh, o_alt)
        torch.cuda.synchronize()
        cnt = ((o_metric != b_metric) | (o_nh != b_nh).any(dim=2) | (o_alt != b_alt).any(dim=2)).sum(dim=1)
        eng.patch(edges=ed, metrics=was, links=[], link_up=[], nodes=nd,
                  node_overloaded=[int(g.node_overloaded[v]) for v in nd], track=False)
        torch.cuda.synchronize()
        old.append(time.perf_counter() - t0)
        same = same and bool((cnt.cpu().numpy() == a_changed[x]).all())
o = np.array(old) * 1e3
print(f"[maint] (e) patch + lfa_routes of {V} sources + compare + patch back: median {np.median(o):.2f} ms per "
      f"event (min {o.min():.2f}, max {o.max():.2f}, 9 events); extrapolated to {n_ev} events "
      f"{np.median(o) * n_ev:.0f} ms = {np.median(o) * n_ev / ma:.1f}x leg (a); counts equal the pass's: {same}",
      flush=True)
eng.close()
