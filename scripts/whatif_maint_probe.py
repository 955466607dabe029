"""Maintenance sweep on the config-4 WAN, six legs in one process (tuning aid): 1 000 events x
all 1 000 sources; event r overloads router r and soft-drains the advertised adjacencies of
router (r + 1) mod 1 000 (every metric of its row + 1000, above any path cost in that graph).

(a) openr_spf_whatif_maint_device, counts only (cap 0);
(b) the same with the node delta;
(c) openr_spf_whatif_maint_routes_device over the 1 200-group table of the route probes (the
    1 000 loopbacks plus 200 random groups of 2-6 nodes);
(d) for context: openr_spf_whatif_drain_device of the N parts alone, counts only;
(e) for context: openr_spf_whatif_metric_device of the R parts alone, counts only;
(f) the way to (a)'s answer without the sweep, on 10 evenly spaced events: patch_graph (the
    event's overload bit and metrics), solve_device of every source, a row compare against the
    base rows on the device, patch_graph back. Its counts are checked against (a) and its
    time is extrapolated to all events.

After a warm-up legs (a)-(e) alternate; every step is timed with a host clock around a
device synchronise; medians with min-max are printed.

    python scripts/whatif_maint_probe.py [steps] [legs, e.g. ab]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openr_amd import topology as T  # noqa: E402
from openr_amd.engine import SpfEngine  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
which = sys.argv[2] if len(sys.argv) > 2 else "abcdef"
RAISE = 1000
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
g = T.wan(1000, 3000, 64, seed=1)
eng = SpfEngine([0])
eng.set_graph(g)
V, nb = g.num_nodes, eng.nh_bytes
node_sets = [[v] for v in range(V)]
edge_sets, metric_sets = T.soft_drain_events(g, [[(v + 1) % V] for v in range(V)], RAISE)
rng = np.random.default_rng(7)
groups = T.loopback_groups(g) + T.prefix_groups(
    g, [rng.choice(V, int(rng.integers(2, 7)), replace=False).tolist() for _ in range(200)])
G = len(groups)


def csr(lists, values=None):
    p = np.zeros(len(lists) + 1, dtype=np.int64)
    p[1:] = np.cumsum([len(x) for x in lists])
    out = [torch.from_numpy(p.astype(np.int32)).to(dev)]
    for ls in (lists, values) if values is not None else (lists,):
        flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in ls])
        out.append(torch.from_numpy(flat.astype(np.int32)).to(dev))
    return out


d_ep, d_ee, d_mm = csr(edge_sets, metric_sets)
d_np, d_nn = csr(node_sets)
d_gp, d_gn = csr(groups)
srcs = torch.arange(V, dtype=torch.int32, device=dev)
units = V * V
s = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(s)
maint_args = (d_np.data_ptr(), d_nn.data_ptr(), 0, 0, d_ep.data_ptr(), d_ee.data_ptr(), d_mm.data_ptr(), V, V, 0,
              d_ee.numel(), srcs.data_ptr(), V)
drain_args = (d_np.data_ptr(), d_nn.data_ptr(), 0, 0, V, V, 0, srcs.data_ptr(), V)
metric_args = (d_ep.data_ptr(), d_ee.data_ptr(), d_mm.data_ptr(), V, d_ee.numel(), srcs.data_ptr(), V)
grp_args = (d_gp.data_ptr(), d_gn.data_ptr(), G, d_gn.numel())

changed = torch.empty((V, V), dtype=torch.int32, device=dev)
ptr = torch.empty(units + 1, dtype=torch.int64, device=dev)
n_total, solved = eng.whatif_maint_device(*maint_args, changed.data_ptr(), ptr.data_ptr(), 0, 0, 0, 0, nb,
                                          stream=s.cuda_stream, allow_overflow=True)
affected = solved - V
a_changed = changed.cpu().numpy().copy()
r_changed = torch.empty((V, V), dtype=torch.int32, device=dev)
r_ptr = torch.empty(units + 1, dtype=torch.int64, device=dev)
r_total, _ = eng.whatif_maint_routes_device(*maint_args, *grp_args, r_changed.data_ptr(), r_ptr.data_ptr(), 0, 0, 0, 0,
                                            0, nb, stream=s.cuda_stream, allow_overflow=True)
x_changed = torch.empty((V, V), dtype=torch.int32, device=dev)
x_ptr = torch.empty(units + 1, dtype=torch.int64, device=dev)
d_total, d_solved = eng.whatif_drain_device(*drain_args, x_changed.data_ptr(), x_ptr.data_ptr(), 0, 0, 0, 0, nb,
                                            stream=s.cuda_stream, allow_overflow=True)
d_changed = x_changed.cpu().numpy().copy()
m_total, m_solved = eng.whatif_metric_device(*metric_args, x_changed.data_ptr(), x_ptr.data_ptr(), 0, 0, 0, 0, nb,
                                             stream=s.cuda_stream, allow_overflow=True)
m_changed = x_changed.cpu().numpy().copy()
neither = int(((a_changed != d_changed) & (a_changed != m_changed)).sum())
e_node = torch.empty(max(n_total, 1), dtype=torch.int32, device=dev)
e_dist = torch.empty(max(n_total, 1), dtype=torch.int64, device=dev)
e_nh = torch.empty((max(n_total, 1), nb), dtype=torch.uint8, device=dev)
r_group = torch.empty(max(r_total, 1), dtype=torch.int32, device=dev)
r_metric = torch.empty(max(r_total, 1), dtype=torch.int64, device=dev)
r_nh = torch.empty((max(r_total, 1), nb), dtype=torch.uint8, device=dev)
r_nbest = torch.empty(max(r_total, 1), dtype=torch.int32, device=dev)
kernels = {}


def leg_counts():
    eng.whatif_maint_device(*maint_args, changed.data_ptr(), ptr.data_ptr(), 0, 0, 0, 0, nb, stream=s.cuda_stream,
                            allow_overflow=True)
    kernels["a"] = eng.last_kernels()


def leg_delta():
    eng.whatif_maint_device(*maint_args, changed.data_ptr(), ptr.data_ptr(), e_node.data_ptr(), e_dist.data_ptr(),
                            e_nh.data_ptr(), n_total, nb, stream=s.cuda_stream)


def leg_routes():
    eng.whatif_maint_routes_device(*maint_args, *grp_args, r_changed.data_ptr(), r_ptr.data_ptr(), r_group.data_ptr(),
                                   r_metric.data_ptr(), r_nh.data_ptr(), r_nbest.data_ptr(), r_total, nb,
                                   stream=s.cuda_stream)


def leg_drain():
    eng.whatif_drain_device(*drain_args, x_changed.data_ptr(), x_ptr.data_ptr(), 0, 0, 0, 0, nb, stream=s.cuda_stream,
                            allow_overflow=True)


def leg_metric():
    eng.whatif_metric_device(*metric_args, x_changed.data_ptr(), x_ptr.data_ptr(), 0, 0, 0, 0, nb,
                             stream=s.cuda_stream, allow_overflow=True)


legs = [(k, name, f) for k, name, f in (
    ("a", "(a) maintenance sweep, counts only", leg_counts),
    ("b", "(b) maintenance sweep with the delta", leg_delta),
    ("c", "(c) maintenance sweep resolved to routes", leg_routes),
    ("d", "(d) drain sweep of the N parts alone, counts only (context)", leg_drain),
    ("e", "(e) metric sweep of the R parts alone, counts only (context)", leg_metric)) if k in which]
times = {name: [] for _, name, _ in legs}
for _, name, f in legs:  # warm-up
    f()
    torch.cuda.synchronize()
for _ in range(steps):
    for _, name, f in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        times[name].append(time.perf_counter() - t0)
print(f"WAN V={V} L={g.num_links}: {V} events (router r overloaded, row of r+1 soft-drained by +{RAISE}) x {V} sources "
      f"= {units} units, {affected} affected ({100.0 * affected / units:.1f}%); changed nodes {n_total} (mean "
      f"{n_total / max(affected, 1):.2f} per affected unit, max {int(a_changed.max())}); changed routes {r_total}; {G} "
      f"groups; drain part alone: {d_solved - V} affected, {d_total} changed nodes; metric part alone: {m_solved - V} "
      f"affected, {m_total} changed nodes; units whose count equals neither part's: {neither}; kernels of (a): "
      f"{kernels.get('a')}")
med = {}
for k, name, _ in legs:
    t = np.array(times[name]) * 1e3
    med[k] = float(np.median(t))
    print(f"{name}: median {np.median(t):.2f} ms per step (min {t.min():.2f}, max {t.max():.2f}, {steps} steps)")
if "a" in med:
    print(f"(a) per affected unit: {1e3 * med['a'] / max(affected, 1):.3f} us ({affected} units)", flush=True)

if "f" in which:  # the old way on 10 evenly spaced events
    b_dist = torch.empty((V, V), dtype=torch.int64, device=dev)
    b_nh = torch.empty((V, V, nb), dtype=torch.uint8, device=dev)
    o_dist, o_nh = torch.empty_like(b_dist), torch.empty_like(b_nh)
    eng.solve_device(srcs.data_ptr(), V, b_dist.data_ptr(), b_nh.data_ptr(), nb, True)
    torch.cuda.synchronize()
    picks = [int(x) for x in np.linspace(0, V - 1, 10).astype(np.int64)]
    old, same = [], True
    for rep in range(2):  # the first round warms the patch path up
        old = []
        for x in picks:
            was = [int(g.metric[e]) for e in edge_sets[x]]
            was_ovl = [int(g.node_overloaded[v]) for v in node_sets[x]]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.patch(edges=edge_sets[x], metrics=metric_sets[x], nodes=node_sets[x],
                      node_overloaded=[1] * len(node_sets[x]), track=False)
            eng.solve_device(srcs.data_ptr(), V, o_dist.data_ptr(), o_nh.data_ptr(), nb, True)  # the engine's stream, as the patch
            torch.cuda.synchronize()
            cnt = ((o_dist != b_dist) | (o_nh != b_nh).any(dim=2)).sum(dim=1)
            eng.patch(edges=edge_sets[x], metrics=was, nodes=node_sets[x], node_overloaded=was_ovl, track=False)
            torch.cuda.synchronize()
            old.append(time.perf_counter() - t0)
            same = same and bool((cnt.cpu().numpy() == a_changed[x]).all())
    o = np.array(old) * 1e3
    ratio = f" = {np.median(o) * V / med['a']:.1f}x leg (a)" if "a" in med else ""
    print(f"(f) patch + solve of {V} sources + row compare + patch back: median {np.median(o):.2f} ms per event "
          f"(min {o.min():.2f}, max {o.max():.2f}, 10 events); extrapolated to {V} events {np.median(o) * V:.0f} ms"
          f"{ratio}; counts equal the sweep's: {same}")
eng.close()
