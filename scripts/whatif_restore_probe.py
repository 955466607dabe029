"""Restore sweep on the config-4 WAN after a maintenance window (tuning aid): the WAN with
every 10th node overloaded (100), every 30th link down (100) and the rows of 100 other nodes
soft-drained by +1000; 300 restore events (each node undrained, each link put up, each row
back to its metrics) x all 1 000 sources.

(a) openr_spf_whatif_restore_device, counts only (cap 0);
(b) the same with the node delta;
(c) openr_spf_whatif_restore_routes_device over the 1 200-group table of the route probes;
(e) the way to (a)'s answer without the sweep, on 9 evenly spaced events: patch_graph (the
    event), solve_device of every source, a row compare against the base rows on the device,
    patch_graph (back). Its counts are checked against (a), its time extrapolated.

With `tune` the narrow launch's slot count (OPENR_SPF_RESTORE_SLOTS 64 / 128 / 256) x threads
per unit (OPENR_SPF_RESTORE_BLOCK 64 / 128 / 256) alternate on legs (a) and (b) instead; the
library reads both knobs at every call. Every step is timed with a host clock around a device
synchronise; medians with min-max are printed.

    python scripts/whatif_restore_probe.py [steps] [tune]
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
tune = "tune" in sys.argv[2:]
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
g0 = T.wan(1000, 3000, 64, seed=1)
V = g0.num_nodes
drained, soft_rows, down = list(range(0, V, 10)), list(range(5, V, 10)), list(range(0, g0.num_links, 30))
soft = [e for v in soft_rows for e in g0.row(v)]
g = g0.patched(soft, [int(g0.metric[e]) + 1000 for e in soft], down, [0] * len(down), drained, [1] * len(drained))
eng = SpfEngine([0])
eng.set_graph(g)
nb = eng.nh_bytes
node_sets = [[v] for v in drained] + [[]] * (len(down) + len(soft_rows))
link_sets = [[]] * len(drained) + [[l] for l in down] + [[]] * len(soft_rows)
edge_sets = [[]] * (len(drained) + len(down)) + [list(g0.row(v)) for v in soft_rows]
metric_sets = [[int(g0.metric[e]) for e in es] for es in edge_sets]
n_ev = len(node_sets)
rng = np.random.default_rng(7)
groups = T.loopback_groups(g) + T.prefix_groups(
    g, [rng.choice(V, int(rng.integers(2, 7)), replace=False).tolist() for _ in range(200)])
G = len(groups)


def csr(*lists):
    p = np.zeros(len(lists[0]) + 1, dtype=np.int64)
    p[1:] = np.cumsum([len(x) for x in lists[0]])
    out = [torch.from_numpy(p.astype(np.int32)).to(dev)]
    for ls in lists:
        flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in ls])
        out.append(torch.from_numpy(flat.astype(np.int32)).to(dev))
    return out


d_np, d_nn = csr(node_sets)
d_lp, d_ll = csr(link_sets)
d_ep, d_ee, d_mm = csr(edge_sets, metric_sets)
d_gp, d_gn = csr(groups)
srcs = torch.arange(V, dtype=torch.int32, device=dev)
units = n_ev * V
s = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(s)
ev_args = (d_np.data_ptr(), d_nn.data_ptr(), d_lp.data_ptr(), d_ll.data_ptr(), d_ep.data_ptr(), d_ee.data_ptr(),
           d_mm.data_ptr(), n_ev, d_nn.numel(), d_ll.numel(), d_ee.numel(), srcs.data_ptr(), V)
grp_args = (d_gp.data_ptr(), d_gn.data_ptr(), G, d_gn.numel())
changed = torch.empty((n_ev, V), dtype=torch.int32, device=dev)
ptr = torch.empty(units + 1, dtype=torch.int64, device=dev)
n_total, solved = eng.whatif_restore_device(*ev_args, changed.data_ptr(), ptr.data_ptr(), 0, 0, 0, 0, nb,
                                            stream=s.cuda_stream, allow_overflow=True)
affected = solved - V
a_changed = changed.cpu().numpy().copy()
e_node = torch.empty(max(n_total, 1), dtype=torch.int32, device=dev)
e_dist = torch.empty(max(n_total, 1), dtype=torch.int64, device=dev)
e_nh = torch.empty((max(n_total, 1), nb), dtype=torch.uint8, device=dev)
kernels = {}


def leg_counts():
    eng.whatif_restore_device(*ev_args, changed.data_ptr(), ptr.data_ptr(), 0, 0, 0, 0, nb, stream=s.cuda_stream,
                              allow_overflow=True)
    kernels["a"] = eng.last_kernels()


def leg_delta():
    eng.whatif_restore_device(*ev_args, changed.data_ptr(), ptr.data_ptr(), e_node.data_ptr(), e_dist.data_ptr(),
                              e_nh.data_ptr(), n_total, nb, stream=s.cuda_stream)


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def line(t):
    t = np.array(t) * 1e3
    return f"median {np.median(t):.2f} ms (min {t.min():.2f}, max {t.max():.2f})"


head = (f"WAN V={V} L={g.num_links}: {n_ev} restore events ({len(drained)} undrains, {len(down)} link-ups, "
        f"{len(soft_rows)} rows lowered by 1000) x {V} sources = {units} units, {affected} affected "
        f"({100.0 * affected / units:.1f}%), {int((a_changed != 0).sum())} with a change; changed nodes {n_total} "
        f"(mean {n_total / max(affected, 1):.2f} per affected unit, max {int(a_changed.max())}, "
        f"{int((a_changed > 128).sum())} units above 128, {int((a_changed > 256).sum())} above 256)")

if tune:
    configs = [(sl, bl) for sl in (64, 128, 256) for bl in (64, 128, 256)]
    times = {(c, leg): [] for c in configs for leg in "ab"}
    reran = {}

    def run(cfg, leg):
        os.environ["OPENR_SPF_RESTORE_SLOTS"], os.environ["OPENR_SPF_RESTORE_BLOCK"] = str(cfg[0]), str(cfg[1])
        dt = timed(leg_counts if leg == "a" else leg_delta)
        reran[cfg] = "restore_repair<overflow>" in eng.last_kernels()
        return dt

    for cfg in configs:  # warm-up, and every configuration gives the same counts
        for leg in "ab":
            run(cfg, leg)
            assert (changed.cpu().numpy() == a_changed).all(), cfg
    for _ in range(steps):
        for cfg in configs:
            for leg in "ab":
                times[(cfg, leg)].append(run(cfg, leg))
    print(head + f"; {steps} steps per configuration, alternating")
    for cfg in configs:
        row = "; ".join(f"({leg}) {line(times[(cfg, leg)])}" for leg in "ab")
        print(f"slots {cfg[0]:3d}, {cfg[1]:3d} threads per unit: {row}; re-run launch: {reran[cfg]}")
    eng.close()
    sys.exit(0)

r_changed = torch.empty((n_ev, V), dtype=torch.int32, device=dev)
r_ptr = torch.empty(units + 1, dtype=torch.int64, device=dev)
r_total, _ = eng.whatif_restore_routes_device(*ev_args, *grp_args, r_changed.data_ptr(), r_ptr.data_ptr(), 0, 0, 0, 0,
                                              0, nb, stream=s.cuda_stream, allow_overflow=True)
r_group = torch.empty(max(r_total, 1), dtype=torch.int32, device=dev)
r_metric = torch.empty(max(r_total, 1), dtype=torch.int64, device=dev)
r_nh = torch.empty((max(r_total, 1), nb), dtype=torch.uint8, device=dev)
r_nbest = torch.empty(max(r_total, 1), dtype=torch.int32, device=dev)


def leg_routes():
    eng.whatif_restore_routes_device(*ev_args, *grp_args, r_changed.data_ptr(), r_ptr.data_ptr(), r_group.data_ptr(),
                                     r_metric.data_ptr(), r_nh.data_ptr(), r_nbest.data_ptr(), r_total, nb,
                                     stream=s.cuda_stream)


legs = (("(a) restore sweep, counts only", leg_counts), ("(b) restore sweep with the delta", leg_delta),
        ("(c) restore sweep resolved to routes", leg_routes))
times = {name: [] for name, _ in legs}
for name, f in legs:  # warm-up
    timed(f)
for _ in range(steps):
    for name, f in legs:
        times[name].append(timed(f))
print(head + f"; changed routes {r_total}; {G} groups; kernels of (a): {kernels['a']}")
for name, _ in legs:
    print(f"{name}: {line(times[name])} per step, {steps} steps")
ma = float(np.median(times[legs[0][0]])) * 1e3
print(f"(a) per affected unit: {1e3 * ma / max(affected, 1):.3f} us ({affected} units); per event {ma / n_ev:.4f} ms",
      flush=True)

# (e) the old way on 9 evenly spaced events
b_dist = torch.empty((V, V), dtype=torch.int64, device=dev)
b_nh = torch.empty((V, V, nb), dtype=torch.uint8, device=dev)
o_dist, o_nh = torch.empty_like(b_dist), torch.empty_like(b_nh)
eng.solve_device(srcs.data_ptr(), V, b_dist.data_ptr(), b_nh.data_ptr(), nb, True)
torch.cuda.synchronize()
picks = [int(x) for x in np.linspace(0, n_ev - 1, 9).astype(np.int64)]
old, same = [], True
for rep in range(2):  # the first round warms the patch path up
    old = []
    for x in picks:
        nodes, links, edges = node_sets[x], link_sets[x], edge_sets[x]
        was = [int(g.metric[e]) for e in edges]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.patch(edges=edges, metrics=metric_sets[x], links=links, link_up=[1] * len(links), nodes=nodes,
                  node_overloaded=[0] * len(nodes), track=False)
        eng.solve_device(srcs.data_ptr(), V, o_dist.data_ptr(), o_nh.data_ptr(), nb, True)  # the engine's stream, as the patch
        torch.cuda.synchronize()
        cnt = ((o_dist != b_dist) | (o_nh != b_nh).any(dim=2)).sum(dim=1)
        eng.patch(edges=edges, metrics=was, links=links, link_up=[0] * len(links), nodes=nodes,
                  node_overloaded=[1] * len(nodes), track=False)
        torch.cuda.synchronize()
        old.append(time.perf_counter() - t0)
        same = same and bool((cnt.cpu().numpy() == a_changed[x]).all())
o = np.array(old) * 1e3
print(f"(e) patch + solve of {V} sources + row compare + patch back: median {np.median(o):.2f} ms per event "
      f"(min {o.min():.2f}, max {o.max():.2f}, 9 events); extrapolated to {n_ev} events {np.median(o) * n_ev:.0f} ms = "
      f"{np.median(o) * n_ev / ma:.1f}x leg (a); counts equal the sweep's: {same}")
eng.close()
