// spf_maint.hip — maintenance what-if sweep (openr_spf_whatif_maint*): events that mix node
// overloads, links out of service and metric raises, repaired on the device from the base SPF.
//
// A maintenance event i is three lists, each possibly empty: a node set N_i (the nodes get the
// overload bit), a link set K_i (Link::isUp() is false, unusable in both directions) and a list
// of directed CSR edges with a new, higher metric each (ids strictly ascending inside the
// event). Unit (i, j) is LinkState::runSpf(sources[j], useLinkMetric, K_i) on the graph with
// node_overloaded = 1 for every node of N_i and the new metrics in place, compared with the
// no-event SPF of sources[j]. It is the union of the drain rule (spf_drain.hip) and the metric
// rule (spf_metric.hip). With X = N_i minus the source minus the nodes that are overloaded
// already:
//     e = u -> v is removed  iff  link(e) in K_i  or  u in X
//     u may expand           iff  u == src  or  (u is not overloaded and u is not in X)
//     R = the event's entries whose edge is up and whose new metric is in (w(e), 2^31 - 1]
//     w'(e) = new metric  if e in R,  else w(e)
// Without OPENR_SPF_USE_LINK_METRIC every weight is 1 and the metric entries are ignored; the
// kernels still run for N_i and K_i. A base-tight edge is lost iff it is removed or raised.
// Both changes only worsen: distances only grow, edges only disappear or get dearer. That is
// all the drain's and the metric sweep's argument uses, so it holds for their union:
//   A  = nodes that lose every base-tight in-edge (closure: an A node's own base-tight
//        out-edges are lost too). Exactly the nodes whose distance grows: a node outside A
//        keeps a live, unraised base-tight in-edge from a tail outside A (induction on the base
//        distance), and gains no tight in-edge because no distance shrinks and no edge gets
//        cheaper.
//   seeds = nodes that lost at least one base-tight in-edge.
//   dist(A) = best dist(u) + w'(e) over non-removed in-edges from tails that may expand
//        (overlay for tails in A, base row otherwise), relaxed inside A until nothing improves.
//   D  = closure of the seeds under new-tight out-edges (usable under the removed set, tested
//        with w'): the only nodes whose next-hop set can differ. Next hops of D by a Kahn pass
//        restricted to D. Next-hop bit positions are those of the unmodified graph.
// Entries that change nothing: a raise on a removed edge, on a down edge or on a row of an
// overloaded node other than the source (such a row is never expanded); a zero raise; a node
// that is overloaded already or is the unit's source (the source's row stays, and raises on
// it act); an unused link id; duplicates, which count once. An empty event changes nothing.
//
// The unit's LDS holds X (V bits) in front of the shared bitmaps, K (L bits) and R (E bits)
// behind them. The new metric of a raised edge is a binary search of the event's slice in
// global memory, run only when the R bit is set (MetricEvent::wnew). walk_event reports every
// lost base-tight edge once: the rows of X, then the edges of K whose tail is not in X, then
// the edges of R whose tail is not in X and whose link is not in K. Those exclusions are tested
// when R is walked, not when it is built: build fills the three bitmaps side by side and the
// policy holds no barrier.
//
// Loop-free alternates under a maintenance event (openr_spf_whatif_maint_lfa*) run this sweep
// over the closure of the sources and hand its rows to the drain pass of spf_elfa.hip: the LFA
// loop never reads the metric of a link s-n, so the raises act through these rows alone.
// Not covered: events that mix worsening with restoring changes, exact-order base plans, the
// C++ LinkState mirror.
//
// Uniformity: the policy's loops (over an event's nodes, links and entries, bitmap words, bits
// and rows, the binary search) have per-lane trip counts and hold no barrier and no wave
// collective.
#include "spf_repair.h"

namespace openr_spf {

namespace {

using repair::in_bm;
using repair::kColMask;

constexpr uint32_t kMaxMetric = 0x7FFFFFFFu;

// entry k of an event really raises a usable edge
__device__ __forceinline__ bool raises(const DevGraph& g, uint32_t e, uint32_t m) {
  return e < g.E && !(g.adj[e] & kEdgeDown) && m > g.w[e] && m <= kMaxMetric;
}

constexpr uint32_t words(uint32_t bits) { return (bits + 31u) / 32u; }
// K's bytes in the block behind the shared bitmaps: R starts 16-byte aligned after them
constexpr uint32_t k_bytes(uint32_t L) { return (4u * words(L) + 15u) & ~15u; }

// The repair's LDS with X (V bits) in front of the shared bitmaps, K (L bits) and R (E bits) behind them.
__host__ __device__ constexpr repair::Layout maint_layout(uint32_t V, uint32_t L, uint32_t E, uint32_t S,
                                                          uint32_t nbw) {
  return repair::layout(V, S, nbw, 4u * words(V), k_bytes(L) + 4u * words(E));
}
// the WAN (V = 1000, L = 3000, E = 6000, 2 next-hop bytes) at the drain's and at the default slots: DESIGN.md 5.16
static_assert(maint_layout(1000, 3000, 6000, 128, 1).total == 6656, "maint LDS layout moved");
static_assert(maint_layout(1000, 3000, 6000, 256, 1).total == 9728, "maint LDS layout moved");

struct MaintEvent {
  const DevGraph& g;
  const MaintPass& p;
  uint32_t* const xbm;  // X: drained nodes that stop expanding
  uint32_t* const kbm;  // K: links out of service
  uint32_t* const rbm;  // R: raised edges
  const uint32_t vw, lw, ew;  // lw / ew = 0: the event kind is absent (or, for R, unit cost)
  const bool unit_cost;
  uint32_t i = 0, src = 0;
  uint32_t eb = 0, ee = 0;  // the event's edge slice, clamped

  static __device__ __forceinline__ repair::Layout layout(const DevGraph& g, uint32_t S, uint32_t nbw) {
    return maint_layout(g.V, g.L, g.E, S, nbw);
  }
  __device__ __forceinline__ MaintEvent(const DevGraph& g_, const MaintPass& p_, unsigned char* smem,
                                        const repair::Layout& lay)
      : g(g_), p(p_), xbm(reinterpret_cast<uint32_t*>(smem + lay.ev0)),
        kbm(reinterpret_cast<uint32_t*>(smem + lay.ev1)),
        rbm(reinterpret_cast<uint32_t*>(smem + lay.ev1 + k_bytes(g_.L))), vw(words(g_.V)),
        lw(p_.link_ptr ? words(g_.L) : 0u), ew(p_.edge_ptr && !p_.unit_cost ? words(g_.E) : 0u),
        unit_cost(p_.unit_cost != 0) {}
  __device__ __forceinline__ void begin(uint32_t i_, uint32_t src_) {
    i = i_;
    src = src_;
    if (ew) {
      eb = min(p.edge_ptr[i], p.n_edges);  // a slice never reaches past edges
      ee = min(max(p.edge_ptr[i + 1], eb), p.n_edges);
    }
  }
  __device__ __forceinline__ bool in_x(uint32_t u) const { return in_bm(xbm, u); }
  __device__ __forceinline__ bool in_k(uint32_t l) const { return lw && in_bm(kbm, l); }
  __device__ __forceinline__ bool in_r(uint32_t e) const { return ew && in_bm(rbm, e); }
  // w'(e), `old` being w(e): the slice is searched only for a raised edge. A slice that
  // does not ascend may miss its entry or find another one; the edge then keeps `old`.
  __device__ __forceinline__ uint32_t wnew(uint32_t e, uint32_t old) const {
    if (!in_r(e)) return old;
    uint32_t lo = eb, hi = ee;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (p.edges[mid] < e) lo = mid + 1u;
      else hi = mid;
    }
    if (lo >= ee || p.edges[lo] != e) return old;
    const uint32_t m = p.metrics[lo];
    return m > old && m <= kMaxMetric ? m : old;
  }

  __device__ __forceinline__ void reset_word(uint32_t w) const { xbm[w] = 0; }
  __device__ __forceinline__ void reset(uint32_t tid, uint32_t B) const {
    for (uint32_t w = tid; w < lw; w += B) kbm[w] = 0;
    for (uint32_t w = tid; w < ew; w += B) rbm[w] = 0;
  }
  // X, K and R as bitmaps (an id listed twice sets one bit). R takes every valid raise: the
  // ones on removed edges are left out where R is walked and never read elsewhere.
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
    for (uint32_t t = eb + tid; t < ee; t += B) {  // ew == 0: an empty slice
      const uint32_t ed = p.edges[t];
      if (raises(g, ed, p.metrics[t])) atomicOr(&rbm[ed >> 5], 1u << (ed & 31u));
    }
  }
  // heads of the base-tight edges the event itself removes or raises, each edge once: the rows
  // of X, the edges of K whose tail is not in X, the edges of R whose tail is not in X and whose
  // link is not in K
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
        const uint2 de = g.ledge[l];
        const uint32_t c0 = g.adj[de.x] & kColMask, c1 = g.adj[de.y] & kColMask;  // de.x = c1 -> c0
        if (tight(de.x) && !in_x(c1)) fn(c0);
        if (tight(de.y) && !in_x(c0)) fn(c1);
      }
    }
    for (uint32_t w = tid; w < ew; w += B) {
      for (uint32_t bits = rbm[w]; bits; bits &= bits - 1u) {
        const uint32_t e = w * 32u + (uint32_t)(__ffs((int)bits) - 1);
        if (!tight(e) || in_k(g.lid[e])) continue;
        if (!in_x(g.adj[g.rev[e]] & kColMask)) fn(g.adj[e] & kColMask);  // the tail: the reverse edge's column
      }
    }
  }
  __device__ __forceinline__ bool row_lost(uint32_t u) const { return in_x(u); }  // its row went with the event
  __device__ __forceinline__ bool out_lost(uint32_t e) const { return in_k(g.lid[e]) || in_r(e); }
  __device__ __forceinline__ bool in_usable(uint32_t link, uint32_t tail) const { return !(in_k(link) || in_x(tail)); }
  __device__ __forceinline__ bool out_usable(uint32_t e) const { return !in_k(g.lid[e]); }
  __device__ __forceinline__ unsigned long long w_in(const uint4& rec) const {
    return unit_cost ? 1ull : (unsigned long long)wnew(rec.w, rec.y);  // rec.w is the in-edge's id
  }
  __device__ __forceinline__ unsigned long long w_out(uint32_t e) const {
    return unit_cost ? 1ull : (unsigned long long)wnew(e, g.w[e]);
  }
  __device__ __forceinline__ bool expands(uint32_t u) const { return u == src || (!g.ovl[u] && !in_x(u)); }
};

// A unit is hit iff a tight edge sits in an X row, on a K link, or is validly raised. (A tight
// raised edge whose tail is in X or whose link is in K hits through those; a row of an
// overloaded node other than the source holds no tight edge.)
__global__ __launch_bounds__(256) void maint_filter(const DevGraph g, const MaintPass p) {
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
        const uint2 de = g.ledge[l];
        if (de.x == UINT32_MAX) continue;
        hit = tight(de.x) || tight(de.y);
      }
    }
    if (p.edge_ptr && !p.unit_cost) {
      const uint32_t rb = min(p.edge_ptr[i], p.n_edges);
      const uint32_t re = min(max(p.edge_ptr[i + 1], rb), p.n_edges);
      for (uint32_t k = rb; k < re && !hit; ++k) {
        const uint32_t ed = p.edges[k];
        if (raises(g, ed, p.metrics[k])) hit = tight(ed);
      }
    }
    return hit;
  });
}

__global__ __launch_bounds__(256) void maint_repair(const DevGraph g, const MaintPass p, const uint32_t* list,
                                                    uint32_t count, uint32_t S, uint32_t* ovf_list,
                                                    uint32_t* ovf_count) {
  repair::repair_units<MaintEvent>(g, p, list, count, S, ovf_list, ovf_count);
}

constexpr repair::Kind kMaint = {
    "maint_filter", "maint_repair",  "maint_repair<overflow>", "OPENR_SPF_MAINT_BLOCK",
    kMaintBlock,    kMaintBlockWide, maint_slots,
    [](const DevGraph& g, uint32_t S, uint32_t nb) { return maint_lds_bytes(g.V, g.L, g.E, S, nb); }};

}  // namespace

uint32_t maint_slots() { return bfs::env_u32("OPENR_SPF_MAINT_SLOTS", kMaintSlots, 1u, 65534u); }

uint32_t maint_lds_bytes(uint32_t V, uint32_t L, uint32_t E, uint32_t S, uint32_t nb) {
  return repair::lds_bytes(V, (uint64_t)V + L + E, S, nb,
                           [&](uint32_t s, uint32_t nbw) { return maint_layout(V, L, E, s, nbw); });
}

hipError_t launch_maint_filter(const DevGraph& g, const MaintPass& p, int num_cus, hipStream_t s) {
  return repair::launch_filter(maint_filter, kMaint, g, p, num_cus, s);
}

hipError_t launch_maint_repair(const DevGraph& g, const MaintPass& p, uint32_t count, bool rerun, int num_cus,
                               hipStream_t s) {
  return repair::launch_repair(maint_repair, kMaint, g, p, count, rerun, num_cus, s);
}

}  // namespace openr_spf
