// spf_restore.hip — restore what-if sweep (openr_spf_whatif_restore*): undrain, link-up and
// metric-lower events, repaired on the device from the base SPF.
//
// A restore event i is a node set N_i (the overload bit is cleared), a link set K_i (the links
// are put back in service: Link::isUp() becomes true, both directions) and a list of directed
// CSR edges with a new, lower metric each (ids strictly ascending inside the event). Unit
// (i, j) is LinkState::runSpf(sources[j], useLinkMetric) on the graph patched that way,
// compared with the no-event SPF of sources[j]. With
//     N = the event's nodes that are overloaded (and are not the source),
//     K = its links that are down and whose two directed edges would carry a metric in
//         [1, 2^31 - 1] after the event (any metric under hop count),
//     R = its entries with 1 <= new metric < current one (empty under hop count),
// the graph of the unit is
//     e is up         iff  edge_up[e]  or  link(e) in K
//     u may expand    iff  u == src  or  u is not overloaded  or  u in N
//     w'(e)           =    the new metric if e in R, else w(e); 1 under hop count
// ("reached, never expanded", LinkState.cpp:831-838). Edges only appear or get cheaper. The
// *improved* edges I of the unit are the edges u -> v that are up and whose tail expands after
// the event and that were not usable for src before, or are in R. They are enumerated from the
// event's slices alone: the rows of N, the two edges of every link of K, the entries of R.
//
// restore_filter: a unit is affected iff some improved edge u -> v has base_dist[u] finite and
// base_dist[v] infinite or base_dist[u] + w'(e) <= base_dist[v]. The test reads the base
// distance rows (an edge that did not exist has no tight bit) and is <=: an equality adds a
// tight in-edge and can change next hops. Any other unit keeps every distance (no path over an
// improved edge beats a base one, by induction on the first improved edge of the path) and
// every tight in-set, hence every next hop.
//
// restore_repair, one workgroup per affected unit, dirty nodes in LDS slots (repair::layout):
//   seeds = heads of the improved edges that pass the filter test; each starts at its base
//        distance and takes min(base_dist[u] + w'(e)) over those edges.
//   B  = the nodes whose distance shrinks: label-correcting rounds over a frontier list (the
//        slots improved in the previous round). A round walks the frontier's usable out-edges
//        twice, claiming slots in the first walk and relaxing in the second, with a barrier
//        between: a slot's index is published before its distance is set, so a one-walk form
//        could read a half-filled slot. The minimum is an LDS atomic min on the 64-bit word.
//        Weights are >= 1 and distances integers, so the rounds end.
//   D  = seeds and B, closed under out-edges that are tight in the new distances: the only
//        nodes whose next-hop set can differ. A node outside D keeps its distance, and all its
//        new-tight tails are outside D (else it would be in D), so they keep their distances
//        and sets; a node outside B never loses a tight in-edge (a tight tail that got closer
//        would have pulled it into B) and one outside the seeds gains none from I, so its
//        tight in-set and its next hops are the base ones.
//   Next hops of D by a Kahn pass restricted to D, the compare with the base row, changed[]
//        and the delta as repair::repair_units steps 5-6. That body is repeated here rather
//        than shared: the packed flags of erec / adj (kEdgeDown, kNodeSink) describe the
//        unmodified graph and are overridden by K and N below, and sharing would change the
//        shape the drain and metric kernels compile to.
//
// Uniformity: barriers sit only in the unit loop and in round loops whose counts are read from
// LDS at a uniform address between two barriers; the loops over an event's entries, bitmap
// words, bits, rows and the binary search have per-lane trip counts and hold no barrier and no
// wave collective. The filter's ballot sits outside the per-unit test (repair::filter_units).
#include "spf_repair.h"
#include "spf_restore_event.h"

namespace openr_spf {

namespace {

using repair::in_bm;
using repair::kColMask;
using repair::kInf;
using repair::kNoSlot;
using restore::Slices;

constexpr uint32_t words(uint32_t bits) { return (bits + 31u) / 32u; }
constexpr uint32_t pad16(uint32_t bytes) { return (bytes + 15u) & ~15u; }

// The repair's LDS with N (V bits) in front of the shared bitmaps, K (L bits) and R (E bits)
// behind them.
__host__ __device__ constexpr repair::Layout restore_layout(uint32_t V, uint32_t L, uint32_t E, uint32_t S,
                                                            uint32_t nbw) {
  return repair::layout(V, S, nbw, 4u * words(V), pad16(4u * words(L)) + 4u * words(E));
}
// the WAN (V = 1000, L = 3000, E = 6000, 2 next-hop bytes): DESIGN.md 5.14
static_assert(restore_layout(1000, 3000, 6000, 128, 1).total == 6656, "restore LDS layout moved");
static_assert(restore_layout(1000, 3000, 6000, 256, 1).total == 9728, "restore LDS layout moved");

// the filter test of one improved edge u -> v at cost c = base_dist[u] + w'(e)
__device__ __forceinline__ bool reaches(unsigned long long du, unsigned long long w, unsigned long long dv) {
  return du != kInf && (dv == kInf || du + w <= dv);
}

struct RestoreEvent {
  const DevGraph& g;
  Slices sl;
  uint32_t* const nbm;  // N: undrained nodes
  uint32_t* const kbm;  // K: links that come up
  uint32_t* const rbm;  // R: lowered edges
  const uint32_t vw, lw, ew;
  const bool unit_cost;
  uint32_t src = 0;

  static __device__ __forceinline__ repair::Layout layout(const DevGraph& g, uint32_t S, uint32_t nbw) {
    return restore_layout(g.V, g.L, g.E, S, nbw);
  }
  __device__ __forceinline__ RestoreEvent(const DevGraph& g_, const RestorePass& p_, unsigned char* smem,
                                          const repair::Layout& lay)
      : g(g_), sl(g_, p_), nbm(reinterpret_cast<uint32_t*>(smem + lay.ev0)),
        kbm(reinterpret_cast<uint32_t*>(smem + lay.ev1)),
        rbm(reinterpret_cast<uint32_t*>(smem + lay.ev1 + pad16(4u * words(g_.L)))), vw(words(g_.V)),
        lw(p_.link_ptr ? words(g_.L) : 0u), ew(p_.edge_ptr && !p_.unit_cost ? words(g_.E) : 0u),
        unit_cost(p_.unit_cost != 0) {}
  __device__ __forceinline__ void begin(uint32_t i, uint32_t src_) {
    src = src_;
    sl.begin(i, src_);
  }
  __device__ __forceinline__ bool in_n(uint32_t u) const { return in_bm(nbm, u); }
  __device__ __forceinline__ bool in_k(uint32_t l) const { return lw && in_bm(kbm, l); }
  __device__ __forceinline__ bool in_r(uint32_t e) const { return ew && in_bm(rbm, e); }

  __device__ __forceinline__ void reset_word(uint32_t w) const { nbm[w] = 0; }
  __device__ __forceinline__ void reset(uint32_t tid, uint32_t B) const {
    for (uint32_t w = tid; w < lw; w += B) kbm[w] = 0;
    for (uint32_t w = tid; w < ew; w += B) rbm[w] = 0;
  }
  // N, K and R as bitmaps (an id listed twice sets one bit)
  __device__ __forceinline__ void build(uint32_t tid, uint32_t B) const {
    const RestorePass& p = sl.p;
    for (uint32_t t = sl.nb + tid; t < sl.ne; t += B) {
      const uint32_t x = p.nodes[t];
      if (sl.undrains(x)) atomicOr(&nbm[x >> 5], 1u << (x & 31u));
    }
    for (uint32_t t = sl.lb + tid; t < sl.le; t += B) {
      const uint32_t l = p.links[t];
      if (sl.comes_up(l)) atomicOr(&kbm[l >> 5], 1u << (l & 31u));
    }
    for (uint32_t t = sl.eb + tid; t < sl.ee; t += B) {
      const uint32_t e = p.edges[t], m = p.metrics[t];
      if (e < g.E && m >= 1u && m < g.w[e]) atomicOr(&rbm[e >> 5], 1u << (e & 31u));
    }
  }
  // the graph under the event; the packed flags of adj / erec describe the unmodified one
  __device__ __forceinline__ bool expands(uint32_t u) const { return u == src || !g.ovl[u] || in_n(u); }
  __device__ __forceinline__ bool out_up(uint32_t e, uint32_t a) const { return !(a & kEdgeDown) || in_k(g.lid[e]); }
  // in-edge record of v's row: the edge rec.w = u -> v exists and u relays over it
  __device__ __forceinline__ bool in_usable(const uint4& rec, uint32_t u) const {
    if ((rec.x & kEdgeDown) && !in_k(rec.z)) return false;
    return u == src || !(rec.x & kNodeSink) || in_n(u);
  }
  __device__ __forceinline__ unsigned long long w_of(uint32_t e, uint32_t old) const {
    if (unit_cost) return 1ull;
    return (unsigned long long)(in_r(e) ? sl.wnew(e, old) : old);
  }
  __device__ __forceinline__ unsigned long long w_in(const uint4& rec) const { return w_of(rec.w, rec.y); }
  __device__ __forceinline__ unsigned long long w_out(uint32_t e) const { return w_of(e, g.w[e]); }

  // fn(v, c) for every improved edge u -> v that passes the filter test, c = base_dist[u] +
  // w'(e): the rows of N, the edges of K, the entries of R. An edge may come up twice.
  template <class Fn>
  __device__ __forceinline__ void walk_improved(uint32_t tid, uint32_t B, const unsigned long long* bd, Fn&& fn) const {
    auto edge = [&](uint32_t u, uint32_t e, uint32_t a) {
      const unsigned long long du = bd[u], w = w_out(e);
      const uint32_t v = a & kColMask;
      if (reaches(du, w, bd[v])) fn(v, du + w);
    };
    for (uint32_t w = tid; w < vw; w += B) {
      for (uint32_t bits = nbm[w]; bits; bits &= bits - 1u) {
        const uint32_t x = w * 32u + (uint32_t)(__ffs((int)bits) - 1);
        const uint2 r = g.row2[x];
        for (uint32_t e = r.x; e < r.y; ++e) {
          const uint32_t a = g.adj[e];
          if (out_up(e, a)) edge(x, e, a);
        }
      }
    }
    for (uint32_t w = tid; w < lw; w += B) {
      for (uint32_t bits = kbm[w]; bits; bits &= bits - 1u) {
        const uint32_t l = w * 32u + (uint32_t)(__ffs((int)bits) - 1);
        const uint2 de = g.ledge[l];
        const uint32_t a0 = g.adj[de.x], a1 = g.adj[de.y];  // de.x = c1 -> c0
        const uint32_t c0 = a0 & kColMask, c1 = a1 & kColMask;
        if (expands(c1)) edge(c1, de.x, a0);
        if (expands(c0)) edge(c0, de.y, a1);
      }
    }
    for (uint32_t w = tid; w < ew; w += B) {
      for (uint32_t bits = rbm[w]; bits; bits &= bits - 1u) {
        const uint32_t e = w * 32u + (uint32_t)(__ffs((int)bits) - 1);
        const uint32_t a = g.adj[e], u = g.adj[g.rev[e]] & kColMask;
        if (out_up(e, a) && expands(u)) edge(u, e, a);
      }
    }
  }
};

// A unit is hit iff an improved edge reaches its head at or below the head's base distance.
__global__ __launch_bounds__(256) void restore_filter(const DevGraph g, const RestorePass p) {
  Slices sl(g, p);
  repair::filter_units(p, [&](uint32_t i, uint32_t j) {
    bool hit = false;
    const uint32_t src = p.sources[j];
    const unsigned long long* bd = reinterpret_cast<const unsigned long long*>(p.base_dist) + (size_t)j * g.V;
    sl.begin(i, src);
    auto weight = [&](uint32_t e) { return sl.unit_cost ? 1ull : (unsigned long long)sl.wnew(e, g.w[e]); };
    auto up = [&](uint32_t e, uint32_t a) {
      if (!(a & kEdgeDown)) return true;
      const uint32_t l = g.lid[e];
      return sl.link_listed(l) && sl.comes_up(l);
    };
    auto expands = [&](uint32_t u) { return u == src || !g.ovl[u] || sl.node_listed(u); };
    for (uint32_t k = sl.nb; k < sl.ne && !hit; ++k) {
      const uint32_t x = p.nodes[k];
      if (!sl.undrains(x) || bd[x] == kInf) continue;
      const uint2 r = g.row2[x];
      for (uint32_t e = r.x; e < r.y && !hit; ++e) {
        const uint32_t a = g.adj[e];
        if (up(e, a)) hit = reaches(bd[x], weight(e), bd[a & kColMask]);
      }
    }
    for (uint32_t k = sl.lb; k < sl.le && !hit; ++k) {
      const uint32_t l = p.links[k];
      if (!sl.comes_up(l)) continue;
      const uint2 de = g.ledge[l];
      const uint32_t c0 = g.adj[de.x] & kColMask, c1 = g.adj[de.y] & kColMask;  // de.x = c1 -> c0
      if (expands(c1)) hit = reaches(bd[c1], weight(de.x), bd[c0]);
      if (!hit && expands(c0)) hit = reaches(bd[c0], weight(de.y), bd[c1]);
    }
    for (uint32_t k = sl.eb; k < sl.ee && !hit; ++k) {
      const uint32_t e = p.edges[k];
      if (e >= g.E) continue;
      const uint32_t old = g.w[e], m = sl.wnew(e, old);
      if (m >= old) continue;
      const uint32_t a = g.adj[e], u = g.adj[g.rev[e]] & kColMask;
      if (up(e, a) && expands(u)) hit = reaches(bd[u], m, bd[a & kColMask]);
    }
    return hit;
  });
}

// Repairs list[0, count): changed[] and the delta of every listed unit; a unit that outgrows
// the S slots is appended to ovf_list (null: S = V, nothing overflows).
__global__ __launch_bounds__(256) void restore_repair(const DevGraph g, const RestorePass p, const uint32_t* list,
                                                      uint32_t count, uint32_t S, uint32_t* ovf_list,
                                                      uint32_t* ovf_count) {
  using namespace repair;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t V = g.V, vw = words(V);
  const uint32_t nb = p.nb, nbw = (nb + 3u) / 4u;
  const Layout lay = RestoreEvent::layout(g, S, nbw);
  uint32_t* const ctl = reinterpret_cast<uint32_t*>(smem + lay.ctl);
  uint32_t* const fbm = reinterpret_cast<uint32_t*>(smem + lay.abm);  // nodes on the next frontier
  uint32_t* const sbm = reinterpret_cast<uint32_t*>(smem + lay.sbm);
  uint16_t* const sidx = reinterpret_cast<uint16_t*>(smem + lay.sidx);
  unsigned long long* const dist = reinterpret_cast<unsigned long long*>(smem + lay.dist);
  uint32_t* const node = reinterpret_cast<uint32_t*>(smem + lay.node);
  uint32_t* const cnt = reinterpret_cast<uint32_t*>(smem + lay.cnt);
  uint32_t* const nhw = reinterpret_cast<uint32_t*>(smem + lay.nh);
  uint16_t* const fa = reinterpret_cast<uint16_t*>(smem + lay.alist);  // frontier lists of slots, by turns
  uint16_t* const qq = reinterpret_cast<uint16_t*>(smem + lay.q);      // ... then the Kahn queue, the changed slots
  const uint32_t tid = threadIdx.x, B = blockDim.x;
  const WhatifDelta& dl = p.delta;
  RestoreEvent ev(g, p, smem, lay);

  // a control word every thread reads between two barriers: workgroup-uniform, and the next
  // write to it comes after the second barrier
  auto uread = [&](uint32_t i) {
    __syncthreads();
    const uint32_t v = ctl[i];
    __syncthreads();
    return v;
  };
  auto dload = [&](uint32_t s) { return __hip_atomic_load(&dist[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };

  for (uint32_t v = tid; v < V; v += B) sidx[v] = (uint16_t)kNoSlot;  // units put it back as they leave
  if (tid == 0) ctl[kNext] = blockIdx.x;
  uint32_t k = uread(kNext);
  while (k < count) {
    const uint32_t unit = list[k];
    const uint32_t i = unit / p.n_src, j = unit - i * p.n_src;
    const uint32_t src = p.sources[j];
    const unsigned long long* bd = reinterpret_cast<const unsigned long long*>(p.base_dist) + (size_t)j * V;
    const uint8_t* bh = p.base_nh + (size_t)j * V * nb;
    ev.begin(i, src);

    // 0. reset the unit's bitmaps and counters
    for (uint32_t w = tid; w < vw; w += B) {
      ev.reset_word(w);
      fbm[w] = 0;
      sbm[w] = 0;
    }
    ev.reset(tid, B);
    if (tid < kNext) ctl[tid] = 0;
    __syncthreads();

    // 1. the event's state
    ev.build(tid, B);
    __syncthreads();

    // first asker of a node takes a slot for it; the node starts at its base distance. The
    // index is published last, and readers of the same walk never trust a slot this young.
    auto claim = [&](uint32_t v) {
      const uint32_t bit = 1u << (v & 31u);
      if (atomicOr(&sbm[v >> 5], bit) & bit) return;
      const uint32_t s = atomicAdd(&ctl[kN], 1u);
      if (s >= S) {
        ctl[kOvf] = 1u;
        return;
      }
      node[s] = v;
      cnt[s] = 0;
      dist[s] = bd[v];
      sidx[v] = (uint16_t)s;
    };
    // distance of y as a walk sees it: slots below `ns` were filled before the walk began
    auto dist_of = [&](uint32_t y, uint32_t ns) {
      const uint32_t sy = sidx[y];
      return sy != kNoSlot && sy < ns ? dload(sy) : bd[y];
    };

    // 2. the seeds: slots first, then the minimum over the improved edges that reach them
    ev.walk_improved(tid, B, bd, [&](uint32_t v, unsigned long long) { claim(v); });
    uint32_t ovf = uread(kOvf);
    if (!ovf) ev.walk_improved(tid, B, bd, [&](uint32_t v, unsigned long long c) { atomicMin(&dist[sidx[v]], c); });
    uint32_t ns = ovf ? 0u : min(uread(kN), S);
    for (uint32_t t = tid; t < ns; t += B)  // the first frontier: the seeds that got closer
      if (dist[t] < bd[node[t]]) fa[atomicAdd(&ctl[kNA], 1u)] = (uint16_t)t;

    // 3. B: label-correcting rounds over the frontier. Each round walks the frontier's
    //    out-edges twice, slots first and the relaxation second.
    uint16_t* cur = fa;
    uint16_t* nxt = qq;
    uint32_t nf = uread(kNA);
    while (!ovf && nf) {
      if (tid == 0) ctl[kNA] = 0;  // the next frontier is counted after the barrier below
      for (uint32_t t = tid; t < nf; t += B) {
        const uint32_t s = cur[t], u = node[s];
        atomicAnd(&fbm[u >> 5], ~(1u << (u & 31u)));
        if (!ev.expands(u)) continue;
        const unsigned long long du = dist[s];  // no slot moves during this walk
        const uint2 r = g.row2[u];
        for (uint32_t e = r.x; e < r.y; ++e) {
          const uint32_t a = g.adj[e];
          if (!ev.out_up(e, a)) continue;
          const uint32_t y = a & kColMask;
          if (du + ev.w_out(e) < dist_of(y, ns)) claim(y);
        }
      }
      __syncthreads();
      ovf = ctl[kOvf];
      ns = min(ctl[kN], S);
      __syncthreads();
      if (ovf) break;
      for (uint32_t t = tid; t < nf; t += B) {
        const uint32_t s = cur[t], u = node[s];
        if (!ev.expands(u)) continue;
        const unsigned long long du = dload(s);  // may be improved meanwhile: u is then on the next frontier
        const uint2 r = g.row2[u];
        for (uint32_t e = r.x; e < r.y; ++e) {
          const uint32_t a = g.adj[e];
          if (!ev.out_up(e, a)) continue;
          const uint32_t y = a & kColMask, sy = sidx[y];
          if (sy == kNoSlot) continue;
          const unsigned long long c = du + ev.w_out(e);
          if (c >= dload(sy) || c >= atomicMin(&dist[sy], c)) continue;
          const uint32_t bit = 1u << (y & 31u);
          if (!(atomicOr(&fbm[y >> 5], bit) & bit)) nxt[atomicAdd(&ctl[kNA], 1u)] = (uint16_t)sy;  // <= ns entries
        }
      }
      nf = uread(kNA);
      uint16_t* const x = cur;
      cur = nxt;
      nxt = x;
    }

    // 4. D: the seeds and B, then every head of a new-tight edge out of D
    uint32_t lo = 0;
    while (!ovf && ns > lo) {
      for (uint32_t t = lo + tid; t < ns; t += B) {
        const uint32_t u = node[t];
        const unsigned long long du = dist[t];
        if (du == kInf || !ev.expands(u)) continue;
        const uint2 r = g.row2[u];
        for (uint32_t e = r.x; e < r.y; ++e) {
          const uint32_t a = g.adj[e];
          if (!ev.out_up(e, a)) continue;
          const uint32_t y = a & kColMask;
          if (du + ev.w_out(e) == dist_of(y, ns)) claim(y);
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
            const uint4 rec = g.erec[e];  // in-edge u -> v seen from v's row; rec.w is its edge id
            const uint32_t u = rec.x & kColMask;
            if (!ev.in_usable(rec, u)) continue;
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
      uint32_t hi = min(uread(kQT), S);
      while (hi > lo) {
        for (uint32_t t = lo + tid; t < hi; t += B) {
          const uint32_t s = qq[t], v = node[s];
          const unsigned long long dv = dist[s];
          if (dv == kInf || !ev.expands(v)) continue;
          const uint2 r = g.row2[v];
          for (uint32_t e = r.x; e < r.y; ++e) {
            const uint32_t a = g.adj[e];
            if (!ev.out_up(e, a)) continue;
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

constexpr repair::Kind kRestore = {
    "restore_filter", "restore_repair",  "restore_repair<overflow>", "OPENR_SPF_RESTORE_BLOCK",
    kRestoreBlock,    kRestoreBlockWide, restore_slots,
    [](const DevGraph& g, uint32_t S, uint32_t nb) { return restore_lds_bytes(g.V, g.L, g.E, S, nb); }};

}  // namespace

uint32_t restore_slots() { return bfs::env_u32("OPENR_SPF_RESTORE_SLOTS", kRestoreSlots, 1u, 65534u); }

uint32_t restore_lds_bytes(uint32_t V, uint32_t L, uint32_t E, uint32_t S, uint32_t nb) {
  return repair::lds_bytes(V, (uint64_t)V + L + E, S, nb,
                           [&](uint32_t s, uint32_t nbw) { return restore_layout(V, L, E, s, nbw); });
}

hipError_t launch_restore_filter(const DevGraph& g, const RestorePass& p, int num_cus, hipStream_t s) {
  return repair::launch_filter(restore_filter, kRestore, g, p, num_cus, s);
}

hipError_t launch_restore_repair(const DevGraph& g, const RestorePass& p, uint32_t count, bool rerun, int num_cus,
                                 hipStream_t s) {
  return repair::launch_repair(restore_repair, kRestore, g, p, count, rerun, num_cus, s);
}

}  // namespace openr_spf
