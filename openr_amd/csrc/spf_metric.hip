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
// are repaired by one workgroup each (metric_repair: the slot repair of spf_repair.h under
// the MetricEvent policy below):
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
//
// Uniformity: the policy's loops (over an event's entries, bitmap words and bits, the binary
// search) have per-lane trip counts and hold no barrier and no wave collective.
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

// The repair's LDS with R (E bits) behind the shared bitmaps.
__host__ __device__ constexpr repair::Layout metric_layout(uint32_t V, uint32_t E, uint32_t S, uint32_t nbw) {
  return repair::layout(V, S, nbw, 0u, 4u * ((E + 31u) / 32u));
}
// the WAN (V = 1000, E = 6000, 2 next-hop bytes) at the drain's and at the default slots: DESIGN.md 5.13
static_assert(metric_layout(1000, 6000, 128, 1).total == 6144, "metric LDS layout moved");
static_assert(metric_layout(1000, 6000, 256, 1).total == 9216, "metric LDS layout moved");

struct MetricEvent {
  const DevGraph& g;
  const MetricPass& p;
  uint32_t* const rbm;  // R: the event's raised edges
  const uint32_t ew;
  uint32_t eb = 0, ee = 0;  // the event's slice, clamped
  uint32_t src = 0;

  static __device__ __forceinline__ repair::Layout layout(const DevGraph& g, uint32_t S, uint32_t nbw) {
    return metric_layout(g.V, g.E, S, nbw);
  }
  __device__ __forceinline__ MetricEvent(const DevGraph& g_, const MetricPass& p_, unsigned char* smem,
                                         const repair::Layout& lay)
      : g(g_), p(p_), rbm(reinterpret_cast<uint32_t*>(smem + lay.ev1)), ew((g_.E + 31u) / 32u) {}
  __device__ __forceinline__ void begin(uint32_t i, uint32_t src_) {
    src = src_;
    eb = min(p.edge_ptr[i], p.n_edges);
    ee = min(max(p.edge_ptr[i + 1], eb), p.n_edges);
  }
  // w'(e), `old` being w(e): the slice is searched only for a raised edge. A slice that
  // does not ascend may miss its entry or find another one; the edge then keeps `old`.
  __device__ __forceinline__ uint32_t wnew(uint32_t e, uint32_t old) const {
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
  }

  __device__ __forceinline__ void reset_word(uint32_t) const {}
  __device__ __forceinline__ void reset(uint32_t tid, uint32_t B) const {
    for (uint32_t w = tid; w < ew; w += B) rbm[w] = 0;
  }
  // R as a bitmap
  __device__ __forceinline__ void build(uint32_t tid, uint32_t B) const {
    for (uint32_t t = eb + tid; t < ee; t += B) {
      const uint32_t e = p.edges[t];
      if (raises(g, e, p.metrics[t])) atomicOr(&rbm[e >> 5], 1u << (e & 31u));
    }
  }
  // heads of the base-tight edges the event itself raises, each edge once
  template <class Tight, class Fn>
  __device__ __forceinline__ void walk_event(uint32_t tid, uint32_t B, Tight&& tight, Fn&& fn) const {
    for (uint32_t w = tid; w < ew; w += B) {
      for (uint32_t bits = rbm[w]; bits; bits &= bits - 1u) {
        const uint32_t e = w * 32u + (uint32_t)(__ffs((int)bits) - 1);
        if (tight(e)) fn(g.adj[e] & kColMask);
      }
    }
  }
  // no edge goes away: every row and every edge stays usable, a raised one at its new metric
  __device__ __forceinline__ bool row_lost(uint32_t) const { return false; }
  __device__ __forceinline__ bool out_lost(uint32_t e) const { return in_bm(rbm, e); }
  __device__ __forceinline__ bool in_usable(uint32_t, uint32_t) const { return true; }
  __device__ __forceinline__ bool out_usable(uint32_t) const { return true; }
  __device__ __forceinline__ unsigned long long w_in(const uint4& rec) const {
    return (unsigned long long)wnew(rec.w, rec.y);  // rec.w is the in-edge's id
  }
  __device__ __forceinline__ unsigned long long w_out(uint32_t e) const { return (unsigned long long)wnew(e, g.w[e]); }
  __device__ __forceinline__ bool expands(uint32_t u) const { return u == src || !g.ovl[u]; }
};

// A unit is hit iff one of its entries raises a tight edge.
__global__ __launch_bounds__(256) void metric_filter(const DevGraph g, const MetricPass p) {
  const uint32_t tw = (g.E + 63u) / 64u;
  repair::filter_units(p, [&](uint32_t i, uint32_t j) {
    bool hit = false;
    const uint64_t* trow = p.base_tight + (size_t)j * tw;
    const uint32_t b = min(p.edge_ptr[i], p.n_edges);  // a slice never reaches past edges
    const uint32_t e = min(max(p.edge_ptr[i + 1], b), p.n_edges);
    for (uint32_t k = b; k < e && !hit; ++k) {
      const uint32_t ed = p.edges[k];
      if (raises(g, ed, p.metrics[k])) hit = ((trow[ed >> 6] >> (ed & 63u)) & 1ull) != 0;
    }
    return hit;
  });
}

__global__ __launch_bounds__(256) void metric_repair(const DevGraph g, const MetricPass p, const uint32_t* list,
                                                     uint32_t count, uint32_t S, uint32_t* ovf_list,
                                                     uint32_t* ovf_count) {
  repair::repair_units<MetricEvent>(g, p, list, count, S, ovf_list, ovf_count);
}

constexpr repair::Kind kMetric = {
    "metric_filter", "metric_repair",  "metric_repair<overflow>", "OPENR_SPF_METRIC_BLOCK",
    kMetricBlock,    kMetricBlockWide, metric_slots,
    [](const DevGraph& g, uint32_t S, uint32_t nb) { return metric_lds_bytes(g.V, g.E, S, nb); }};

}  // namespace

uint32_t metric_slots() { return bfs::env_u32("OPENR_SPF_METRIC_SLOTS", kMetricSlots, 1u, 65534u); }

uint32_t metric_lds_bytes(uint32_t V, uint32_t E, uint32_t S, uint32_t nb) {
  return repair::lds_bytes(V, E, S, nb, [&](uint32_t s, uint32_t nbw) { return metric_layout(V, E, s, nbw); });
}

hipError_t launch_metric_filter(const DevGraph& g, const MetricPass& p, int num_cus, hipStream_t s) {
  return repair::launch_filter(metric_filter, kMetric, g, p, num_cus, s);
}

hipError_t launch_metric_repair(const DevGraph& g, const MetricPass& p, uint32_t count, bool rerun, int num_cus,
                                hipStream_t s) {
  return repair::launch_repair(metric_repair, kMetric, g, p, count, rerun, num_cus, s);
}

}  // namespace openr_spf
