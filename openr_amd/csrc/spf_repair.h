// spf_repair.h — the slot repair shared by the event what-if sweeps (spf_drain.hip,
// spf_metric.hip): the filter skeleton, the repair body and their launchers.
//
// An event changes a set of directed edges for one source's SPF: it takes them away (drain)
// or makes them dearer (metric). dist and nh depend on tight edges only, so a unit none of
// whose hit edges is tight in the base SPF changes nothing (filter_units). The others are
// repaired by one workgroup each (repair_units), which reads the source's base rows from
// global memory and keeps only the unit's dirty nodes in LDS slots: A (the nodes that lose
// every base-tight in-edge), the seeds, dist(A), D and the Kahn pass over D, as the event
// files' headers define them. A unit that needs more slots than the launch has is listed for
// a second launch of the same kernel with one slot per node.
// The restore sweep (spf_restore.hip) goes the other way, edges appear or get cheaper: it keeps
// its own repair body and shares filter_units, the layout, the ctl words and the launchers.
//
// What an event is enters through a policy struct `Event`, built once per workgroup from
// (g, p, smem, layout), with plain force-inlined members:
//   static layout(g, S, nbw)      the LDS layout: repair::layout plus the event's own bytes
//   begin(i, src)                 per unit: the event's slice, the source
//   reset_word(w), reset(tid, B)  step 0: its node-indexed bitmap word, its other bitmaps
//   build(tid, B)                 step 1: its LDS state from the event's slice
//   walk_event(tid, B, tight, fn) fn(head) for every base-tight edge the event itself hits, once
//   row_lost(u), out_lost(e)      walk_a: an A node's row / tight out-edge the event already hit
//   in_usable(link, tail)         steps 3, 5: the in-edge exists under the event
//   out_usable(e)                 steps 4, 5: the out-edge exists under the event
//   w_in(rec), w_out(e)           the edge's weight under the event (erec record / edge id)
//   expands(u)                    u relays under the event
//
// Uniformity: barriers sit only in the unit loop and in round loops whose counts are read
// from LDS at a uniform address between two barriers (uread); loops with per-lane trip
// counts hold no barrier and no wave collective, the policy's members included. The filter's
// ballot sits outside the per-unit hit test.
#pragma once

#include <algorithm>

#include "spf_bfs_common.h"
#include "spf_kernels.h"

namespace openr_spf {
namespace repair {

constexpr uint32_t kColMask = ~(kEdgeDown | kNodeSink);
constexpr uint32_t kNoSlot = 0xFFFFu;
constexpr unsigned long long kInf = ~0ull;

__device__ __forceinline__ bool in_bm(const uint32_t* bm, uint32_t x) { return ((bm[x >> 5] >> (x & 31u)) & 1u) != 0; }

// One thread per unit, threads in source-major order (t = j * n_events + i), as
// whatif_set_filter: neighbouring list entries share a source's base rows. changed[u] = 0 for
// every unit; the units hit(i, j) names are appended to wunit, one atomic per wave.
template <class Pass, class Hit>
__device__ __forceinline__ void filter_units(const Pass& p, Hit&& hit_of) {
  const uint64_t total = (uint64_t)p.n_events * p.n_src;
  for (uint64_t t0 = (uint64_t)blockIdx.x * 256u; t0 < total; t0 += (uint64_t)gridDim.x * 256u) {
    const uint64_t t = t0 + threadIdx.x;
    bool hit = false;
    uint64_t u = 0;
    if (t < total) {
      const uint32_t j = (uint32_t)(t / p.n_events);
      const uint32_t i = (uint32_t)(t - (uint64_t)j * p.n_events);
      u = (uint64_t)i * p.n_src + j;
      p.changed[u] = 0;
      hit = hit_of(i, j);
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

// LDS of one workgroup: node-indexed bitmaps and the u16 slot index; everything else is per
// slot (S of them). The event's own state sits at ev0 (pre bytes) and ev1 (post bytes).
struct Layout {
  uint32_t ctl, ev0, abm, sbm, ev1, sidx, dist, node, cnt, nh, alist, q, total;
};

constexpr uint32_t take(uint32_t& off, uint32_t bytes) {
  const uint32_t o = off;
  off += (bytes + 15u) & ~15u;
  return o;
}

__host__ __device__ constexpr Layout layout(uint32_t V, uint32_t S, uint32_t nbw, uint32_t pre, uint32_t post) {
  Layout l{};
  uint32_t off = 0;
  const uint32_t vw = (V + 31u) / 32u;
  l.ctl = take(off, 64);
  l.ev0 = take(off, pre);
  l.abm = take(off, 4u * vw);  // A
  l.sbm = take(off, 4u * vw);  // nodes that asked for a slot
  l.ev1 = take(off, post);
  l.sidx = take(off, 2u * V);  // node -> slot, kNoSlot
  l.dist = take(off, 8u * S);  // new distance of the slot's node
  l.node = take(off, 4u * S);
  l.cnt = take(off, 4u * S);   // live tight in-degree (A closure), then in-degree inside D (Kahn)
  l.nh = take(off, 4u * S * nbw);
  l.alist = take(off, 2u * S);  // slots of the A nodes, in joining order
  l.q = take(off, 2u * S);      // Kahn queue of slots, then the changed slots
  l.total = off;
  return l;
}

// LDS of a unit with S slots and event_bits of event bitmaps laid out by layout_of(S, nbw);
// 0 when it does not fit kMaxLds (or S outgrows the u16 index)
template <class LayoutOf>
inline uint32_t lds_bytes(uint32_t V, uint64_t event_bits, uint32_t S, uint32_t nb, LayoutOf&& layout_of) {
  if (S >= kNoSlot) return 0;
  const uint64_t per_slot = 8u + 4u + 4u + 4u * (uint64_t)((nb + 3u) / 4u) + 2u + 2u;
  if ((uint64_t)V * 2u + event_bits / 8u + (uint64_t)S * per_slot > kMaxLds) return 0;  // before the u32 layout sums
  const uint32_t t = layout_of(S, (nb + 3u) / 4u).total;
  return t <= kMaxLds ? t : 0;
}

// ctl words
enum : uint32_t { kN = 0, kOvf, kNA, kFlag, kQT, kCh, kPoolLo, kPoolHi, kNext };

// Repairs list[0, count): changed[] and the delta of every listed unit; a unit that outgrows
// the S slots is appended to ovf_list (null: S = V, nothing overflows).
template <class Event, class Pass>
__device__ __forceinline__ void repair_units(const DevGraph& g, const Pass& p, const uint32_t* list, uint32_t count,
                                             uint32_t S, uint32_t* ovf_list, uint32_t* ovf_count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t V = g.V, vw = (V + 31u) / 32u, tw = (g.E + 63u) / 64u;
  const uint32_t nb = p.nb, nbw = (nb + 3u) / 4u;
  const Layout lay = Event::layout(g, S, nbw);
  uint32_t* const ctl = reinterpret_cast<uint32_t*>(smem + lay.ctl);
  uint32_t* const abm = reinterpret_cast<uint32_t*>(smem + lay.abm);
  uint32_t* const sbm = reinterpret_cast<uint32_t*>(smem + lay.sbm);
  uint16_t* const sidx = reinterpret_cast<uint16_t*>(smem + lay.sidx);
  unsigned long long* const dist = reinterpret_cast<unsigned long long*>(smem + lay.dist);
  uint32_t* const node = reinterpret_cast<uint32_t*>(smem + lay.node);
  uint32_t* const cnt = reinterpret_cast<uint32_t*>(smem + lay.cnt);
  uint32_t* const nhw = reinterpret_cast<uint32_t*>(smem + lay.nh);
  uint16_t* const alist = reinterpret_cast<uint16_t*>(smem + lay.alist);
  uint16_t* const qq = reinterpret_cast<uint16_t*>(smem + lay.q);
  const uint32_t tid = threadIdx.x, B = blockDim.x;
  const WhatifDelta& dl = p.delta;
  Event ev(g, p, smem, lay);

  // a control word every thread reads between two barriers: workgroup-uniform, and the next
  // write to it comes after the second barrier
  auto uread = [&](uint32_t i) {
    __syncthreads();
    const uint32_t v = ctl[i];
    __syncthreads();
    return v;
  };

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
    ev.begin(i, src);
    auto tight = [&](uint32_t e) { return ((bt[e >> 6] >> (e & 63u)) & 1ull) != 0; };
    auto in_a = [&](uint32_t u) { return in_bm(abm, u); };

    // 0. reset the unit's bitmaps and counters
    for (uint32_t w = tid; w < vw; w += B) {
      ev.reset_word(w);
      abm[w] = 0;
      sbm[w] = 0;
    }
    ev.reset(tid, B);
    if (tid < kNext) ctl[tid] = 0;
    __syncthreads();

    // 1. the event's state (an id listed twice sets one bit)
    ev.build(tid, B);
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
    // heads of the base-tight out-edges the A nodes alist[lo, hi) lose and the event left
    auto walk_a = [&](uint32_t lo, uint32_t hi, auto&& fn) {
      for (uint32_t t = lo + tid; t < hi; t += B) {
        const uint32_t u = node[alist[t]];
        if (ev.row_lost(u)) continue;
        const uint2 r = g.row2[u];
        for (uint32_t e = r.x; e < r.y; ++e)
          if (tight(e) && !ev.out_lost(e)) fn(g.adj[e] & kColMask);
      }
    };

    // 2. A and the seeds. Each round walks its edges twice: slots first, then the counts
    ev.walk_event(tid, B, tight, [&](uint32_t v) { claim(v, true); });
    uint32_t ovf = uread(kOvf);
    if (!ovf) ev.walk_event(tid, B, tight, lose);
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
    //    Every in-edge the event leaves usable counts, at its weight under the event.
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
            if (!ev.in_usable(rec.z, u) || (u != src && (rec.x & kNodeSink))) continue;
            const unsigned long long du = ua ? dist[sidx[u]] : bd[u];
            if (du == kInf) continue;
            const unsigned long long c = du + ev.w_in(rec);
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
        if (du == kInf || !ev.expands(u)) continue;
        const uint2 r = g.row2[u];
        for (uint32_t e = r.x; e < r.y; ++e) {
          const uint32_t a = g.adj[e];
          if ((a & kEdgeDown) || !ev.out_usable(e)) continue;
          const uint32_t y = a & kColMask;
          // only A nodes moved; a slot being filled by another thread is never read here
          const unsigned long long dy = in_a(y) ? dist[sidx[y]] : bd[y];
          if (du + ev.w_out(e) == dy) claim(y, false);
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
            if (!ev.in_usable(rec.z, u) || (u != src && (rec.x & kNodeSink))) continue;
            const uint32_t su = sidx[u];
            const unsigned long long du = su != kNoSlot ? dist[su] : bd[u];
            if (du == kInf || du + ev.w_in(rec) != dv) continue;
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
          if (dv == kInf || !ev.expands(v)) continue;
          const uint2 r = g.row2[v];
          for (uint32_t e = r.x; e < r.y; ++e) {
            const uint32_t a = g.adj[e];
            if ((a & kEdgeDown) || !ev.out_usable(e)) continue;
            const uint32_t sy = sidx[a & kColMask];
            if (sy == kNoSlot || dv + ev.w_out(e) != dist[sy]) continue;
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

// What differs between the launcher pairs of two event kinds.
struct Kind {
  const char* filter_name;
  const char* repair_name;
  const char* rerun_name;
  const char* block_env;  // tuning only: threads per unit of the narrow launch, 64 / 128 / 256
  uint32_t block, block_wide;
  uint32_t (*slots)();
  uint32_t (*lds)(const DevGraph& g, uint32_t S, uint32_t nb);  // LDS of a unit with S slots on g, 0: no fit
};

template <class Pass>
hipError_t launch_filter(void (*kernel)(DevGraph, Pass), const Kind& kind, const DevGraph& g, const Pass& p,
                         int num_cus, hipStream_t s) {
  hipError_t err = hipMemsetAsync(p.wcount, 0, 2 * sizeof(uint32_t), s);  // affected units, overflowed units
  if (err != hipSuccess) return err;
  const uint64_t total = (uint64_t)p.n_events * p.n_src;
  if (!total) return hipSuccess;
  note_launch(kind.filter_name);
  hipLaunchKernelGGL(kernel, dim3(grid_for(total, 256u, num_cus)), dim3(256), 0, s, g, p);
  return hipGetLastError();
}

template <class Pass>
hipError_t launch_repair(void (*kernel)(DevGraph, Pass, const uint32_t*, uint32_t, uint32_t, uint32_t*, uint32_t*),
                         const Kind& kind, const DevGraph& g, const Pass& p, uint32_t count, bool rerun, int num_cus,
                         hipStream_t s) {
  if (!count) return hipSuccess;
  const uint32_t S = rerun ? g.V : std::min(kind.slots(), g.V);
  uint32_t block = rerun ? kind.block_wide : bfs::env_u32(kind.block_env, kind.block, 64u, 256u);
  if (block != 64u && block != 128u && block != 256u) block = kind.block;
  const uint32_t lds = kind.lds(g, S, p.nb);
  if (!lds) return hipErrorInvalidValue;  // the caller checks the LDS size first
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return err;
  note_launch(rerun ? kind.rerun_name : kind.repair_name);
  hipLaunchKernelGGL(kernel, dim3(blocks_for(count, lds, num_cus, block)), dim3(block), lds, s, g, p,
                     rerun ? p.ovf_unit : p.wunit, count, S, rerun ? nullptr : p.ovf_unit, p.wcount + 1);
  return hipGetLastError();
}

}  // namespace repair
}  // namespace openr_spf
