// spf_metric.hip — metric what-if sweep (openr_spf_whatif_metric*): soft-drain events, the
// metrics of some directed edges raised, repaired on the device from the base SPF.
//
// A metric event i is a list of directed CSR edges with a new metric each (ids strictly
// ascending inside the event). Unit (i, j) is LinkState::runSpf(sources[j], true) on the
// graph in which those edges carry the new metrics, compared with the no-event SPF of
// sources[j]. Only raises are served: with R = the event's entries whose edge is up and
// whose new metric is above the current one (and at most 2^31 - 1),
//     w'(e) = new metric  if e in R,  else w(e);   no edge goes away, none gets cheaper.
// An entry on a down edge, a zero raise, and an entry on a row of an overloaded node other
// than the source change nothing (the last because such a row is never expanded: none of
// its edges is tight or relaxed). dist and nh depend on tight edges only, so a unit none of
// whose raised edges is tight in the base SPF changes nothing (metric_filter). The others
// are repaired by one workgroup each (metric_repair), which reads the source's base rows
// from global memory and keeps only the unit's dirty nodes in LDS slots:
//   A  = nodes that lose every base-tight in-edge. A raised base-tight edge is a lost tight
//        edge (its tail kept its distance, the edge got dearer); an A node's own base-tight
//        out-edges are lost too, and the closure continues. Exactly the nodes whose
//        distance grows: a node outside A keeps a live base-tight in-edge from a tail
//        outside A (induction on the base distance), a node of A has every shortest path
//        raised or through A. Outside A no node gains a tight in-edge, because distances
//        only grow and edges only get dearer.
//   seeds = nodes that lost at least one base-tight in-edge.
//   dist(A) = best dist(u) + w'(e) over all usable in-edges from tails that may expand,
//        raised edges included at their new metric (overlay for tails in A, base row
//        otherwise), relaxed inside A until nothing improves. Sums fit u64.
//   D  = closure of the seeds under new-tight out-edges (tested with w'): the only nodes
//        whose next-hop set can differ. Next hops of D by a Kahn pass restricted to D.
// R is an E-bit LDS bitmap; the new metric of a raised edge is a binary search of the
// event's slice in global memory, run only when the bit is set. An in-edge record (erec)
// carries the id of its directed edge, so the key is at hand wherever a weight is read.
// A unit that needs more slots than the launch has is listed for a second launch of the
// same kernel with one slot per node.
//
// The slot machinery (claim / lose, the two-walk rounds, the Kahn pass, the compare and the
// pool write) follows spf_drain.hip, which stays as it is; DESIGN.md 5.13 names the copy.
//
// Uniformity: barriers sit only in the unit loop and in round loops whose counts are read
// from LDS at a uniform address between two barriers (uread); loops with per-lane trip
// counts, the binary search included, hold no barrier and no wave collective. The filter's
// ballot sits outside its lane-dependent loop.
#include <algorithm>

#include "spf_bfs_common.h"
#include "spf_kernels.h"

namespace openr_spf {

namespace {

constexpr uint32_t kColMask = ~(kEdgeDown | kNodeSink);
constexpr uint32_t kNoSlot = 0xFFFFu;
constexpr uint32_t kMaxMetric = 0x7FFFFFFFu;
constexpr unsigned long long kInf = ~0ull;

// entry k of an event really raises a usable edge
__device__ __forceinline__ bool raises(const DevGraph& g, uint32_t e, uint32_t m) {
  return e < g.E && !(g.adj[e] & kEdgeDown) && m > g.w[e] && m <= kMaxMetric;
}

// One thread per unit, threads in source-major order (t = j * n_events + i), as
// drain_filter: neighbouring list entries share a source's base rows.
__global__ __launch_bounds__(256) void metric_filter(const DevGraph g, const MetricPass p) {
  const uint64_t total = (uint64_t)p.n_events * p.n_src;
  const uint32_t tw = (g.E + 63u) / 64u;
  for (uint64_t t0 = (uint64_t)blockIdx.x * 256u; t0 < total; t0 += (uint64_t)gridDim.x * 256u) {
    const uint64_t t = t0 + threadIdx.x;
    bool hit = false;
    uint64_t u = 0;
    if (t < total) {
      const uint32_t j = (uint32_t)(t / p.n_events);
      const uint32_t i = (uint32_t)(t - (uint64_t)j * p.n_events);
      u = (uint64_t)i * p.n_src + j;
      p.changed[u] = 0;
      const uint64_t* trow = p.base_tight + (size_t)j * tw;
      const uint32_t b = min(p.edge_ptr[i], p.n_edges);  // a slice never reaches past edges
      const uint32_t e = min(max(p.edge_ptr[i + 1], b), p.n_edges);
      for (uint32_t k = b; k < e && !hit; ++k) {
        const uint32_t ed = p.edges[k];
        if (raises(g, ed, p.metrics[k])) hit = ((trow[ed >> 6] >> (ed & 63u)) & 1ull) != 0;
      }
    }
    const unsigned long long m = __ballot(hit);
    if (!m) continue;
    const uint32_t lane = __lane_id();
    const uint32_t leader = (uint32_t)(__ffsll((long long)m) - 1);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(p.wcount, (uint32_t)__popcll(m));
    base = __shfl(base, (int)leader);
    if (hit) p.wunit[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)u;
  }
}

// LDS of one workgroup: node-indexed bitmaps, the edge-indexed bitmap of the raised edges
// and the u16 slot index; everything else is per slot (S of them).
struct MetricLayout {
  uint32_t ctl, abm, sbm, rbm, sidx, dist, node, cnt, nh, alist, q, total;
};

__host__ __device__ inline MetricLayout metric_layout(uint32_t V, uint32_t E, uint32_t S, uint32_t nbw) {
  MetricLayout l;
  uint32_t off = 0;
  auto take = [&](uint32_t bytes) {
    const uint32_t o = off;
    off += (bytes + 15u) & ~15u;
    return o;
  };
  const uint32_t vw = (V + 31u) / 32u, ew = (E + 31u) / 32u;
  l.ctl = take(64);
  l.abm = take(4u * vw);  // A
  l.sbm = take(4u * vw);  // nodes that asked for a slot
  l.rbm = take(4u * ew);  // R: the event's raised edges
  l.sidx = take(2u * V);  // node -> slot, kNoSlot
  l.dist = take(8u * S);  // new distance of the slot's node
  l.node = take(4u * S);
  l.cnt = take(4u * S);   // live tight in-degree (A closure), then in-degree inside D (Kahn)
  l.nh = take(4u * S * nbw);
  l.alist = take(2u * S);  // slots of the A nodes, in joining order
  l.q = take(2u * S);      // Kahn queue of slots, then the changed slots
  l.total = off;
  return l;
}

// ctl words
enum : uint32_t { kN = 0, kOvf, kNA, kFlag, kQT, kCh, kPoolLo, kPoolHi, kNext };

__global__ __launch_bounds__(256) void metric_repair(const DevGraph g, const MetricPass p, const uint32_t* list,
                                                     uint32_t count, uint32_t S, uint32_t* ovf_list,
                                                     uint32_t* ovf_count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t V = g.V, vw = (V + 31u) / 32u, tw = (g.E + 63u) / 64u, ew = (g.E + 31u) / 32u;
  const uint32_t nb = p.nb, nbw = (nb + 3u) / 4u;
  const MetricLayout lay = metric_layout(V, g.E, S, nbw);
  uint32_t* const ctl = reinterpret_cast<uint32_t*>(smem + lay.ctl);
  uint32_t* const abm = reinterpret_cast<uint32_t*>(smem + lay.abm);
  uint32_t* const sbm = reinterpret_cast<uint32_t*>(smem + lay.sbm);
  uint32_t* const rbm = reinterpret_cast<uint32_t*>(smem + lay.rbm);
  uint16_t* const sidx = reinterpret_cast<uint16_t*>(smem + lay.sidx);
  unsigned long long* const dist = reinterpret_cast<unsigned long long*>(smem + lay.dist);
  uint32_t* const node = reinterpret_cast<uint32_t*>(smem + lay.node);
  uint32_t* const cnt = reinterpret_cast<uint32_t*>(smem + lay.cnt);
  uint32_t* const nhw = reinterpret_cast<uint32_t*>(smem + lay.nh);
  uint16_t* const alist = reinterpret_cast<uint16_t*>(smem + lay.alist);
  uint16_t* const qq = reinterpret_cast<uint16_t*>(smem + lay.q);
  const uint32_t tid = threadIdx.x, B = blockDim.x;
  const WhatifDelta& dl = p.delta;

  // a control word every thread reads between two barriers: workgroup-uniform, and the next
  // write to it comes after the second barrier
  auto uread = [&](uint32_t i) {
    __syncthreads();
    const uint32_t v = ctl[i];
    __syncthreads();
    return v;
  };
  auto in_bm = [](const uint32_t* bm, uint32_t x) { return ((bm[x >> 5] >> (x & 31u)) & 1u) != 0; };

  for (uint32_t v = tid; v < V; v += B) sidx[v] = (uint16_t)kNoSlot;  // units put it back as they leave
  if (tid == 0) ctl[kNext] = blockIdx.x;
  uint32_t k = uread(kNext);
  while (k < count) {
    const uint32_t unit = list[k];
    const uint32_t i = unit / p.n_src, j = unit - i * p.n_src;
    const uint32_t src = p.sources[j];
    const unsigned long long* bd = reinterpret_cast<const unsigned long long*>(p.base_dist) + (size_t)j * V;
    const uint8_t* bh = p.base_nh + (size_t)j * V * nb;
    const uint64_t* bt = p.base_tight + (size_t)j * tw;
    const uint16_t* btin = p.base_tin ? p.base_tin + (size_t)j * V : nullptr;
    const uint32_t eb = min(p.edge_ptr[i], p.n_edges);  // the event's slice, clamped
    const uint32_t ee = min(max(p.edge_ptr[i + 1], eb), p.n_edges);
    auto tight = [&](uint32_t e) { return ((bt[e >> 6] >> (e & 63u)) & 1ull) != 0; };
    auto in_a = [&](uint32_t u) { return in_bm(abm, u); };
    auto expands = [&](uint32_t u) { return u == src || !g.ovl[u]; };
    // w'(e), `old` being w(e): the slice is searched only for a raised edge. A slice that
    // does not ascend may miss its entry or find another one; the edge then keeps `old`.
    auto wnew = [&](uint32_t e, uint32_t old) {
      if (!in_bm(rbm, e)) return old;
      uint32_t lo = eb, hi = ee;
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (p.edges[mid] < e) lo = mid + 1u;
        else hi = mid;
      }
      if (lo >= ee || p.edges[lo] != e) return old;
      const uint32_t m = p.metrics[lo];
      return m > old && m <= kMaxMetric ? m : old;
    };

    // 0. reset the unit's bitmaps and counters
    for (uint32_t w = tid; w < vw; w += B) {
      abm[w] = 0;
      sbm[w] = 0;
    }
    for (uint32_t w = tid; w < ew; w += B) rbm[w] = 0;
    if (tid < kNext) ctl[tid] = 0;
    __syncthreads();

    // 1. R as a bitmap
    for (uint32_t t = eb + tid; t < ee; t += B) {
      const uint32_t e = p.edges[t];
      if (raises(g, e, p.metrics[t])) atomicOr(&rbm[e >> 5], 1u << (e & 31u));
    }
    __syncthreads();

    // first asker of a node takes a slot for it; the node starts at its base distance
    auto claim = [&](uint32_t v, bool with_tin) {
      const uint32_t bit = 1u << (v & 31u);
      if (atomicOr(&sbm[v >> 5], bit) & bit) return;
      const uint32_t s = atomicAdd(&ctl[kN], 1u);
      if (s >= S) {
        ctl[kOvf] = 1u;
        return;
      }
      uint32_t tin = 0;
      if (with_tin) {
        if (btin) {
          tin = btin[v];
        } else {
          const uint2 r = g.row2[v];
          for (uint32_t e = r.x; e < r.y; ++e) tin += tight(g.erec[e].w) ? 1u : 0u;
        }
      }
      node[s] = v;
      cnt[s] = tin;
      dist[s] = bd[v];
      sidx[v] = (uint16_t)s;
    };
    // a lost base-tight edge into v: v joins A with its last one
    auto lose = [&](uint32_t v) {
      const uint32_t s = sidx[v];
      if (s == kNoSlot) return;
      if (atomicSub(&cnt[s], 1u) != 1u) return;
      atomicOr(&abm[v >> 5], 1u << (v & 31u));
      const uint32_t a = atomicAdd(&ctl[kNA], 1u);
      if (a < S) alist[a] = (uint16_t)s;
    };
    // heads of the base-tight edges the event itself raises, each edge once
    auto walk_event = [&](auto&& fn) {
      for (uint32_t w = tid; w < ew; w += B) {
        for (uint32_t bits = rbm[w]; bits; bits &= bits - 1u) {
          const uint32_t e = w * 32u + (uint32_t)(__ffs((int)bits) - 1);
          if (tight(e)) fn(g.adj[e] & kColMask);
        }
      }
    };
    // heads of the base-tight out-edges the A nodes alist[lo, hi) lose and the event left
    auto walk_a = [&](uint32_t lo, uint32_t hi, auto&& fn) {
      for (uint32_t t = lo + tid; t < hi; t += B) {
        const uint2 r = g.row2[node[alist[t]]];
        for (uint32_t e = r.x; e < r.y; ++e)
          if (tight(e) && !in_bm(rbm, e)) fn(g.adj[e] & kColMask);
      }
    };

    // 2. A and the seeds. Each round walks its edges twice: slots first, then the counts
    walk_event([&](uint32_t v) { claim(v, true); });
    uint32_t ovf = uread(kOvf);
    if (!ovf) walk_event(lose);
    uint32_t lo = 0, hi = uread(kNA);
    while (!ovf && hi > lo) {
      walk_a(lo, hi, [&](uint32_t v) { claim(v, true); });
      ovf = uread(kOvf);
      if (!ovf) walk_a(lo, hi, lose);
      lo = hi;
      hi = min(uread(kNA), S);
    }
    const uint32_t na = hi;

    // 3. distances of A: from outside A first, then rounds inside A until nothing improves.
    //    Every usable in-edge counts, a raised one at its new metric.
    if (!ovf && na) {
      for (uint32_t t = tid; t < na; t += B) dist[alist[t]] = kInf;
      uint32_t again = 1u;
      for (uint32_t round = 0; again; ++round) {
        __syncthreads();  // the reset above / the flag read below precede this round's writes
        for (uint32_t t = tid; t < na; t += B) {
          const uint32_t s = alist[t], v = node[s];
          unsigned long long best = dist[s];
          const uint2 r = g.row2[v];
          for (uint32_t e = r.x; e < r.y; ++e) {
            const uint4 rec = g.erec[e];  // in-edge u -> v seen from v's row; rec.w is its edge id
            if (rec.x & kEdgeDown) continue;
            const uint32_t u = rec.x & kColMask;
            const bool ua = in_a(u);
            if (round && !ua) continue;  // tails outside A were taken in round 0
            if (u != src && (rec.x & kNodeSink)) continue;
            const unsigned long long du = ua ? dist[sidx[u]] : bd[u];
            if (du == kInf) continue;
            const unsigned long long c = du + (unsigned long long)wnew(rec.w, rec.y);
            if (c < best) best = c;
          }
          if (best < dist[s]) {
            dist[s] = best;
            ctl[kFlag] = 1u;
          }
        }
        again = uread(kFlag);
        if (tid == 0) ctl[kFlag] = 0;
      }
    }

    // 4. D: the seeds, then every head of a new-tight edge out of D
    uint32_t ns = ovf ? 0u : min(uread(kN), S);
    lo = 0;
    while (!ovf && ns > lo) {
      for (uint32_t t = lo + tid; t < ns; t += B) {
        const uint32_t u = node[t];
        const unsigned long long du = dist[t];
        if (du == kInf || !expands(u)) continue;
        const uint2 r = g.row2[u];
        for (uint32_t e = r.x; e < r.y; ++e) {
          const uint32_t a = g.adj[e];
          if (a & kEdgeDown) continue;
          const uint32_t y = a & kColMask;
          // only A nodes moved; a slot being filled by another thread is never read here
          const unsigned long long dy = in_a(y) ? dist[sidx[y]] : bd[y];
          if (du + (unsigned long long)wnew(e, g.w[e]) == dy) claim(y, false);
        }
      }
      ovf = uread(kOvf);
      lo = ns;
      ns = min(uread(kN), S);
    }

    // 5. next hops of D: in-degree inside D and the sets entering from outside D, then
    //    Kahn rounds pushing each finished set over the new-tight edges inside D
    if (!ovf && ns) {
      for (uint32_t t = tid; t < ns * nbw; t += B) nhw[t] = 0;
      __syncthreads();
      for (uint32_t t = tid; t < ns; t += B) {
        const uint32_t v = node[t];
        const unsigned long long dv = dist[t];
        uint32_t c = 0;
        if (dv != kInf) {
          const uint2 r = g.row2[v];
          for (uint32_t e = r.x; e < r.y; ++e) {
            const uint4 rec = g.erec[e];
            if (rec.x & kEdgeDown) continue;
            const uint32_t u = rec.x & kColMask;
            if (u != src && (rec.x & kNodeSink)) continue;
            const uint32_t su = sidx[u];
            const unsigned long long du = su != kNoSlot ? dist[su] : bd[u];
            if (du == kInf || du + (unsigned long long)wnew(rec.w, rec.y) != dv) continue;
            if (su != kNoSlot) {
              ++c;
            } else if (u == src) {
              const uint32_t bit = g.nbr[rec.w];
              if (bit < nb * 8u) nhw[t * nbw + (bit >> 5)] |= 1u << (bit & 31u);
            } else {
              const uint8_t* h = bh + (size_t)u * nb;
              for (uint32_t b = 0; b < nb; ++b) nhw[t * nbw + (b >> 2)] |= (uint32_t)h[b] << (8u * (b & 3u));
            }
          }
        }
        cnt[t] = c;
        if (c == 0) {
          const uint32_t at = atomicAdd(&ctl[kQT], 1u);
          if (at < S) qq[at] = (uint16_t)t;
        }
      }
      lo = 0;
      hi = min(uread(kQT), S);
      while (hi > lo) {
        for (uint32_t t = lo + tid; t < hi; t += B) {
          const uint32_t s = qq[t], v = node[s];
          const unsigned long long dv = dist[s];
          if (dv == kInf || !expands(v)) continue;
          const uint2 r = g.row2[v];
          for (uint32_t e = r.x; e < r.y; ++e) {
            const uint32_t a = g.adj[e];
            if (a & kEdgeDown) continue;
            const uint32_t sy = sidx[a & kColMask];
            if (sy == kNoSlot || dv + (unsigned long long)wnew(e, g.w[e]) != dist[sy]) continue;
            if (v == src) {
              const uint32_t bit = g.nbr[e];
              if (bit < nb * 8u) atomicOr(&nhw[sy * nbw + (bit >> 5)], 1u << (bit & 31u));
            } else {
              for (uint32_t w = 0; w < nbw; ++w) {
                const uint32_t x = nhw[s * nbw + w];
                if (x) atomicOr(&nhw[sy * nbw + w], x);
              }
            }
            if (atomicSub(&cnt[sy], 1u) == 1u) {
              const uint32_t at = atomicAdd(&ctl[kQT], 1u);
              if (at < S) qq[at] = (uint16_t)sy;
            }
          }
        }
        lo = hi;
        hi = min(uread(kQT), S);
      }

      // 6. compare D with the base row; the changed slots, then the unit's delta
      for (uint32_t t = tid; t < ns; t += B) {
        const uint32_t v = node[t];
        bool diff = dist[t] != bd[v];
        const uint8_t* h = bh + (size_t)v * nb;
        for (uint32_t b = 0; b < nb && !diff; ++b) diff = ((nhw[t * nbw + (b >> 2)] >> (8u * (b & 3u))) & 0xFFu) != h[b];
        if (diff) qq[atomicAdd(&ctl[kCh], 1u)] = (uint16_t)t;  // the Kahn queue is done: at most ns entries
      }
      const uint32_t total = uread(kCh);
      if (tid == 0) {
        p.changed[unit] = total;
        if (dl.node && total) {  // one pool reservation per unit (WhatifDelta)
          const unsigned long long b = atomicAdd(dl.used, (unsigned long long)total);
          dl.off[unit] = dl.base_of(b);
          ctl[kPoolLo] = (uint32_t)b;
          ctl[kPoolHi] = (uint32_t)(b >> 32);
        }
      }
      if (dl.node && total) {
        __syncthreads();
        const unsigned long long base = ((unsigned long long)ctl[kPoolHi] << 32) | ctl[kPoolLo];
        for (uint32_t t = tid; t < total; t += B) {
          const unsigned long long pos = base + t;
          if (pos >= dl.cap) continue;
          const uint32_t s = qq[t];
          dl.node[pos] = node[s];
          dl.dist[pos] = dist[s];
          uint8_t* o = dl.nh + (size_t)pos * dl.nhb;
          for (uint32_t b = 0; b < dl.nhb; ++b)
            o[b] = b < nb ? (uint8_t)(nhw[s * nbw + (b >> 2)] >> (8u * (b & 3u))) : (uint8_t)0;
        }
      }
    }
    if (ovf && tid == 0 && ovf_list) ovf_list[atomicAdd(ovf_count, 1u)] = unit;  // the launch with a slot per node

    // the slot index back to empty, the next unit
    const uint32_t used = min(uread(kN), S);
    for (uint32_t t = tid; t < used; t += B) sidx[node[t]] = (uint16_t)kNoSlot;
    if (tid == 0) ctl[kNext] = gridDim.x + atomicAdd(&p.ctr[0], 1u);
    k = uread(kNext);
  }
  bfs::retire_workgroup(p.ctr, nullptr);
}

uint32_t grid_for(uint64_t items, uint32_t per_block, int num_cus) {
  const uint64_t want = (items + per_block - 1) / per_block;
  const uint64_t cap = (uint64_t)num_cus * 8u;
  return (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
}

}  // namespace

uint32_t metric_slots() { return bfs::env_u32("OPENR_SPF_METRIC_SLOTS", kMetricSlots, 1u, 65534u); }

uint32_t metric_lds_bytes(uint32_t V, uint32_t E, uint32_t S, uint32_t nb) {
  if (S >= kNoSlot) return 0;
  const uint64_t per_slot = 8u + 4u + 4u + 4u * (uint64_t)((nb + 3u) / 4u) + 2u + 2u;
  if ((uint64_t)V * 2u + (uint64_t)E / 8u + (uint64_t)S * per_slot > kMaxLds) return 0;  // before the u32 layout sums
  const uint32_t t = metric_layout(V, E, S, (nb + 3u) / 4u).total;
  return t <= kMaxLds ? t : 0;
}

hipError_t launch_metric_filter(const DevGraph& g, const MetricPass& p, int num_cus, hipStream_t s) {
  hipError_t err = hipMemsetAsync(p.wcount, 0, 2 * sizeof(uint32_t), s);  // affected units, overflowed units
  if (err != hipSuccess) return err;
  const uint64_t total = (uint64_t)p.n_events * p.n_src;
  if (!total) return hipSuccess;
  note_launch("metric_filter");
  hipLaunchKernelGGL(metric_filter, dim3(grid_for(total, 256u, num_cus)), dim3(256), 0, s, g, p);
  return hipGetLastError();
}

hipError_t launch_metric_repair(const DevGraph& g, const MetricPass& p, uint32_t count, bool rerun, int num_cus,
                                hipStream_t s) {
  if (!count) return hipSuccess;
  const uint32_t S = rerun ? g.V : std::min(metric_slots(), g.V);
  // OPENR_SPF_METRIC_BLOCK (tuning only): threads per unit of the narrow launch, 64 / 128 / 256
  uint32_t block = rerun ? kMetricBlockWide : bfs::env_u32("OPENR_SPF_METRIC_BLOCK", kMetricBlock, 64u, 256u);
  if (block != 64u && block != 128u && block != 256u) block = kMetricBlock;
  const uint32_t lds = metric_lds_bytes(g.V, g.E, S, p.nb);
  if (!lds) return hipErrorInvalidValue;  // the caller checks metric_lds_bytes first
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(metric_repair),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return err;
  note_launch(rerun ? "metric_repair<overflow>" : "metric_repair");
  hipLaunchKernelGGL(metric_repair, dim3(blocks_for(count, lds, num_cus, block)), dim3(block), lds, s, g, p,
                     rerun ? p.ovf_unit : p.wunit, count, S, rerun ? nullptr : p.ovf_unit, p.wcount + 1);
  return hipGetLastError();
}

}  // namespace openr_spf
