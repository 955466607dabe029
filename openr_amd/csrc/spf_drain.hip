// spf_drain.hip — drain what-if sweep (openr_spf_whatif_drain*): node-overload and
// link-drain events repaired on the device from the base SPF.
//
// A drain event i is a node set N_i (the nodes get the overload bit) and a link set K_i
// (overloaded links: Link::isUp() is false, unusable in both directions). Unit (i, j) is
// LinkState::runSpf(sources[j], useLinkMetric, K_i) on the graph with node_overloaded = 1
// for every node of N_i, compared with the no-event SPF of sources[j]. A drained node is
// reached but never expanded unless it is the source ("reached, never expanded",
// LinkState.cpp:831-838), so with X = N_i minus the source minus the nodes that are
// overloaded already, the event removes a *directed* edge set:
//     e = u -> v is removed  iff  link(e) in K_i  or  u in X
//     u may expand           iff  u == src  or  (u is not overloaded and u is not in X)
// dist and nh depend on tight edges only, so a unit none of whose removed edges is tight in
// the base SPF changes nothing (drain_filter). The others are repaired by one workgroup
// each (drain_repair: the slot repair of spf_repair.h under the DrainEvent policy below):
//   A  = nodes that lose every base-tight in-edge (closure: an A node's own base-tight
//        out-edges are lost too). Exactly the nodes whose distance grows; every other node
//        keeps a live tight in-edge whose tail keeps its distance by induction on the base
//        distance, and gains no tight in-edge because an A node's distance only grows.
//   seeds = nodes that lost at least one base-tight in-edge.
//   dist(A) = best entry over non-removed in-edges from tails that may expand (overlay for
//        tails in A, base row otherwise), relaxed inside A until nothing improves.
//   D  = closure of the seeds under new-tight out-edges: the only nodes whose next-hop set
//        can differ (a node outside D has the same tight in-edges from tails whose sets
//        are unchanged). Next hops of D by a Kahn pass restricted to D.
//
// Uniformity: the policy's loops (over an event's nodes and links, bitmap words, bits and
// rows) have per-lane trip counts and hold no barrier and no wave collective.
#include "spf_repair.h"

namespace openr_spf {

namespace {

using repair::in_bm;
using repair::kColMask;

// The repair's LDS with X (V bits) in front of the shared bitmaps and K (L bits) behind them.
__host__ __device__ constexpr repair::Layout drain_layout(uint32_t V, uint32_t L, uint32_t S, uint32_t nbw) {
  return repair::layout(V, S, nbw, 4u * ((V + 31u) / 32u), 4u * ((L + 31u) / 32u));
}
// the WAN (V = 1000, L = 3000, 2 next-hop bytes) at the default slots: DESIGN.md 5.12
static_assert(drain_layout(1000, 3000, 128, 1).total == 5904, "drain LDS layout moved");

struct DrainEvent {
  const DevGraph& g;
  const DrainPass& p;
  uint32_t* const xbm;  // X: drained nodes that stop expanding
  uint32_t* const kbm;  // K: drained links
  const uint32_t vw, lw;
  const bool unit_cost;
  uint32_t i = 0, src = 0;

  static __device__ __forceinline__ repair::Layout layout(const DevGraph& g, uint32_t S, uint32_t nbw) {
    return drain_layout(g.V, g.L, S, nbw);
  }
  __device__ __forceinline__ DrainEvent(const DevGraph& g_, const DrainPass& p_, unsigned char* smem,
                                        const repair::Layout& lay)
      : g(g_), p(p_), xbm(reinterpret_cast<uint32_t*>(smem + lay.ev0)),
        kbm(reinterpret_cast<uint32_t*>(smem + lay.ev1)), vw((g_.V + 31u) / 32u),
        lw(p_.link_ptr ? (g_.L + 31u) / 32u : 0u), unit_cost(p_.unit_cost != 0) {}
  __device__ __forceinline__ void begin(uint32_t i_, uint32_t src_) {
    i = i_;
    src = src_;
  }
  __device__ __forceinline__ bool in_x(uint32_t u) const { return in_bm(xbm, u); }
  __device__ __forceinline__ bool in_k(uint32_t l) const { return lw && in_bm(kbm, l); }

  __device__ __forceinline__ void reset_word(uint32_t w) const { xbm[w] = 0; }
  __device__ __forceinline__ void reset(uint32_t tid, uint32_t B) const {
    for (uint32_t w = tid; w < lw; w += B) kbm[w] = 0;
  }
  // X and K as bitmaps (a node or link listed twice sets one bit)
  __device__ __forceinline__ void build(uint32_t tid, uint32_t B) const {
    const uint32_t b = min(p.node_ptr[i], p.n_nodes);  // a slice never reaches past nodes
    const uint32_t e = min(max(p.node_ptr[i + 1], b), p.n_nodes);
    for (uint32_t t = b + tid; t < e; t += B) {
      const uint32_t x = p.nodes[t];
      if (x < g.V && x != src && !g.ovl[x]) atomicOr(&xbm[x >> 5], 1u << (x & 31u));
    }
    if (lw) {
      const uint32_t lb = min(p.link_ptr[i], p.n_links);
      const uint32_t le = min(max(p.link_ptr[i + 1], lb), p.n_links);
      for (uint32_t t = lb + tid; t < le; t += B) {
        const uint32_t l = p.links[t];
        if (l < g.L && g.ledge[l].x != UINT32_MAX) atomicOr(&kbm[l >> 5], 1u << (l & 31u));
      }
    }
  }
  // heads of the base-tight edges the event itself removes, each edge once: the rows of X,
  // then the edges of K whose tail is not in X
  template <class Tight, class Fn>
  __device__ __forceinline__ void walk_event(uint32_t tid, uint32_t B, Tight&& tight, Fn&& fn) const {
    for (uint32_t w = tid; w < vw; w += B) {
      for (uint32_t bits = xbm[w]; bits; bits &= bits - 1u) {
        const uint32_t x = w * 32u + (uint32_t)(__ffs((int)bits) - 1);
        const uint2 r = g.row2[x];
        for (uint32_t e = r.x; e < r.y; ++e)
          if (tight(e)) fn(g.adj[e] & kColMask);
      }
    }
    for (uint32_t w = tid; w < lw; w += B) {
      for (uint32_t bits = kbm[w]; bits; bits &= bits - 1u) {
        const uint32_t l = w * 32u + (uint32_t)(__ffs((int)bits) - 1);
        const uint2 ee = g.ledge[l];
        const uint32_t c0 = g.adj[ee.x] & kColMask, c1 = g.adj[ee.y] & kColMask;  // ee.x = c1 -> c0
        if (tight(ee.x) && !in_x(c1)) fn(c0);
        if (tight(ee.y) && !in_x(c0)) fn(c1);
      }
    }
  }
  __device__ __forceinline__ bool row_lost(uint32_t u) const { return in_x(u); }  // its row went with the event
  __device__ __forceinline__ bool out_lost(uint32_t e) const { return in_k(g.lid[e]); }
  __device__ __forceinline__ bool in_usable(uint32_t link, uint32_t tail) const { return !(in_k(link) || in_x(tail)); }
  __device__ __forceinline__ bool out_usable(uint32_t e) const { return !in_k(g.lid[e]); }
  __device__ __forceinline__ unsigned long long w_in(const uint4& rec) const {
    return unit_cost ? 1ull : (unsigned long long)rec.y;
  }
  __device__ __forceinline__ unsigned long long w_out(uint32_t e) const {
    return unit_cost ? 1ull : (unsigned long long)g.w[e];
  }
  __device__ __forceinline__ bool expands(uint32_t u) const { return u == src || (!g.ovl[u] && !in_x(u)); }
};

// A unit is hit iff a tight edge sits in a drained node's row or on a drained link.
__global__ __launch_bounds__(256) void drain_filter(const DevGraph g, const DrainPass p) {
  const uint32_t tw = (g.E + 63u) / 64u;
  repair::filter_units(p, [&](uint32_t i, uint32_t j) {
    bool hit = false;
    const uint32_t src = p.sources[j];
    const uint64_t* trow = p.base_tight + (size_t)j * tw;
    auto tight = [&](uint32_t e) { return ((trow[e >> 6] >> (e & 63u)) & 1ull) != 0; };
    const uint32_t b = min(p.node_ptr[i], p.n_nodes);  // a slice never reaches past nodes
    const uint32_t e = min(max(p.node_ptr[i + 1], b), p.n_nodes);
    for (uint32_t k = b; k < e && !hit; ++k) {
      const uint32_t x = p.nodes[k];
      if (x >= g.V || x == src || g.ovl[x]) continue;
      const uint2 r = g.row2[x];
      for (uint32_t ee = r.x; ee < r.y && !hit; ++ee) hit = tight(ee);
    }
    if (p.link_ptr) {
      const uint32_t lb = min(p.link_ptr[i], p.n_links);
      const uint32_t le = min(max(p.link_ptr[i + 1], lb), p.n_links);
      for (uint32_t k = lb; k < le && !hit; ++k) {
        const uint32_t l = p.links[k];
        if (l >= g.L) continue;
        const uint2 ee = g.ledge[l];
        if (ee.x == UINT32_MAX) continue;
        hit = tight(ee.x) || tight(ee.y);
      }
    }
    return hit;
  });
}

__global__ __launch_bounds__(256) void drain_repair(const DevGraph g, const DrainPass p, const uint32_t* list,
                                                    uint32_t count, uint32_t S, uint32_t* ovf_list,
                                                    uint32_t* ovf_count) {
  repair::repair_units<DrainEvent>(g, p, list, count, S, ovf_list, ovf_count);
}

constexpr repair::Kind kDrain = {
    "drain_filter", "drain_repair",  "drain_repair<overflow>", "OPENR_SPF_DRAIN_BLOCK",
    kDrainBlock,    kDrainBlockWide, drain_slots,
    [](const DevGraph& g, uint32_t S, uint32_t nb) { return drain_lds_bytes(g.V, g.L, S, nb); }};

}  // namespace

uint32_t drain_slots() { return bfs::env_u32("OPENR_SPF_DRAIN_SLOTS", kDrainSlots, 1u, 65534u); }

uint32_t drain_lds_bytes(uint32_t V, uint32_t L, uint32_t S, uint32_t nb) {
  return repair::lds_bytes(V, L, S, nb, [&](uint32_t s, uint32_t nbw) { return drain_layout(V, L, s, nbw); });
}

hipError_t launch_drain_filter(const DevGraph& g, const DrainPass& p, int num_cus, hipStream_t s) {
  return repair::launch_filter(drain_filter, kDrain, g, p, num_cus, s);
}

hipError_t launch_drain_repair(const DevGraph& g, const DrainPass& p, uint32_t count, bool rerun, int num_cus,
                               hipStream_t s) {
  return repair::launch_repair(drain_repair, kDrain, g, p, count, rerun, num_cus, s);
}

}  // namespace openr_spf
