"""Node-failure sweep on the config-4 WAN, two ways in one process (tuning aid):

(a) openr_spf_whatif_sets_device: all 1 000 node-failure sets x all 1 000 sources;
(b) the route without it: openr_spf_solve_device with the same ignore sets over every unit,
    in chunks of sets that fit memory, full rows written and no diff against the base rows
    at all (a lower bound on diffing them oneself).

After a warm-up of each the legs alternate; every step is timed with a host clock around a
device synchronise. Prints both per-step times, the affected-unit count and the mean
changed nodes per unit.

    python scripts/whatif_sets_probe.py [steps] [sets per chunk of leg (b)]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openr_amd import topology as T  # noqa: E402
from openr_amd.engine import SpfEngine  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
sets_per_chunk = int(sys.argv[2]) if len(sys.argv) > 2 else 100
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
g = T.wan(1000, 3000, 64, seed=1)
eng = SpfEngine([0])
eng.set_graph(g)
V, nb = g.num_nodes, eng.nh_bytes
sets = T.node_failure_sets(g)
n_sets = len(sets)
sizes = np.array([len(s) for s in sets], dtype=np.int64)
sp = np.zeros(n_sets + 1, dtype=np.int64)
sp[1:] = np.cumsum(sizes)
sl = np.concatenate([np.asarray(s, dtype=np.int64) for s in sets])
d_sp = torch.from_numpy(sp.astype(np.int32)).to(dev)
d_sl = torch.from_numpy(sl.astype(np.int32)).to(dev)
srcs = torch.arange(V, dtype=torch.int32, device=dev)
changed = torch.empty((n_sets, V), dtype=torch.int32, device=dev)
s = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(s)

# leg (b): per chunk of sets, unit (i, j) = (source j, ignore set i): its sources, the CSR
# pointer and each set's links once per source (solve_device takes one slice per solve)
chunks = []
for i0 in range(0, n_sets, sets_per_chunk):
    i1 = min(n_sets, i0 + sets_per_chunk)
    per_unit = np.repeat(sizes[i0:i1], V)
    ptr = np.zeros(per_unit.shape[0] + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(per_unit)
    links = np.concatenate([np.tile(sl[sp[i] : sp[i + 1]], V) for i in range(i0, i1)] or [np.zeros(0, np.int64)])
    chunks.append((torch.arange(V, dtype=torch.int32, device=dev).repeat(i1 - i0),
                   torch.from_numpy(ptr.astype(np.int32)).to(dev),
                   torch.from_numpy(np.ascontiguousarray(links).astype(np.int32)).to(dev) if len(links)
                   else torch.zeros(1, dtype=torch.int32, device=dev)))
rows = sets_per_chunk * V
dist = torch.empty((rows, V), dtype=torch.int64, device=dev)
nh = torch.empty((rows, V, nb), dtype=torch.uint8, device=dev)
solved, kernels = [0], [None]


def leg_sets():
    solved[0] = eng.whatif_sets_device(d_sp.data_ptr(), d_sl.data_ptr(), n_sets, int(sl.shape[0]), srcs.data_ptr(), V,
                                       changed.data_ptr(), True, stream=s.cuda_stream)
    kernels[0] = sorted(set(eng.last_kernels()))


def leg_solve():
    for c_src, c_ptr, c_links in chunks:
        eng.solve_device(c_src.data_ptr(), int(c_src.shape[0]), dist.data_ptr(), nh.data_ptr(), nb, True,
                         stream=s.cuda_stream, d_ignore_ptr=c_ptr.data_ptr(), d_ignore_links=c_links.data_ptr())


legs = (("whatif_sets_device", leg_sets), ("solve_device, every unit, no diff", leg_solve))
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
units = n_sets * V
total = int(changed.sum(dtype=torch.int64).item())
affected = solved[0] - V
nonzero = int((changed != 0).sum().item())
print(f"WAN V={V} L={g.num_links}: {n_sets} node-failure sets (mean {sizes.mean():.2f} links, max {sizes.max()}) x "
      f"{V} sources = {units} units; sweep kernels: {kernels[0]}")
for name, _ in legs:
    t = np.array(times[name]) * 1e3
    print(f"{name}: median {np.median(t):.1f} ms per step (min {t.min():.1f}, max {t.max():.1f}, {steps} steps)")
print(f"affected units {affected} of {units}; units with changes {nonzero}; changed nodes {total}: "
      f"mean {total / units:.2f} per unit, {total / max(affected, 1):.2f} per affected unit", flush=True)
eng.close()
