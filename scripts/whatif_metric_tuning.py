"""Metric sweep tuning on the config-4 WAN (tuning aid): the narrow launch's slot count
(OPENR_SPF_METRIC_SLOTS 64 / 128 / 256) x threads per unit (OPENR_SPF_METRIC_BLOCK 64 / 128)
on the workload of scripts/whatif_metric_probe.py, legs (a) counts only and (b) with the
node delta. The library reads both knobs at every call, so the configurations alternate in
one process after a warm-up; medians with min-max are printed, and whether the narrow launch
overflowed into the re-run.

    python scripts/whatif_metric_tuning.py [steps]
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
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
g = T.wan(1000, 3000, 64, seed=1)
eng = SpfEngine([0])
eng.set_graph(g)
V, nb = g.num_nodes, eng.nh_bytes
edge_sets, metric_sets = T.soft_drain_events(g, [[v] for v in range(V)], 1000)
p = np.zeros(V + 1, dtype=np.int64)
p[1:] = np.cumsum([len(x) for x in edge_sets])
d_ep = torch.from_numpy(p.astype(np.int32)).to(dev)
d_ee = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.int32) for x in edge_sets])).to(dev)
d_mm = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.int32) for x in metric_sets])).to(dev)
srcs = torch.arange(V, dtype=torch.int32, device=dev)
s = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(s)
args = (d_ep.data_ptr(), d_ee.data_ptr(), d_mm.data_ptr(), V, d_ee.numel(), srcs.data_ptr(), V)
changed = torch.empty((V, V), dtype=torch.int32, device=dev)
ptr = torch.empty(V * V + 1, dtype=torch.int64, device=dev)
n_total, solved = eng.whatif_metric_device(*args, changed.data_ptr(), ptr.data_ptr(), 0, 0, 0, 0, nb,
                                           stream=s.cuda_stream, allow_overflow=True)
want = changed.cpu().numpy().copy()
e_node = torch.empty(max(n_total, 1), dtype=torch.int32, device=dev)
e_dist = torch.empty(max(n_total, 1), dtype=torch.int64, device=dev)
e_nh = torch.empty((max(n_total, 1), nb), dtype=torch.uint8, device=dev)
configs = [(sl, bl) for sl in (64, 128, 256) for bl in (64, 128)]
times = {(c, leg): [] for c in configs for leg in "ab"}
reran = {}


def run(cfg, leg):
    os.environ["OPENR_SPF_METRIC_SLOTS"], os.environ["OPENR_SPF_METRIC_BLOCK"] = str(cfg[0]), str(cfg[1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if leg == "a":
        eng.whatif_metric_device(*args, changed.data_ptr(), ptr.data_ptr(), 0, 0, 0, 0, nb, stream=s.cuda_stream,
                                 allow_overflow=True)
    else:
        eng.whatif_metric_device(*args, changed.data_ptr(), ptr.data_ptr(), e_node.data_ptr(), e_dist.data_ptr(),
                                 e_nh.data_ptr(), n_total, nb, stream=s.cuda_stream)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    reran[cfg] = "metric_repair<overflow>" in eng.last_kernels()
    return dt


for cfg in configs:  # warm-up, and every configuration gives the same counts
    for leg in "ab":
        run(cfg, leg)
        assert (changed.cpu().numpy() == want).all(), cfg
for _ in range(steps):
    for cfg in configs:
        for leg in "ab":
            times[(cfg, leg)].append(run(cfg, leg))
print(f"WAN V={V}: {V} adjacency soft drains (+1000) x {V} sources, {solved - V} affected units, {n_total} changed "
      f"nodes (max {int(want.max())} in a unit); {steps} steps per configuration, alternating")
for cfg in configs:
    row = []
    for leg in "ab":
        t = np.array(times[(cfg, leg)]) * 1e3
        row.append(f"({leg}) median {np.median(t):.2f} ms (min {t.min():.2f}, max {t.max():.2f})")
    print(f"slots {cfg[0]:3d}, {cfg[1]:3d} threads per unit: {'; '.join(row)}; re-run launch: {reran[cfg]}")
eng.close()
