// spf_restore_event.h — what a restore event's three slices say about a single id: the one
// definition of "this node undrains", "this link comes up" and "this edge is lowered to" that
// the restore sweep (spf_restore.hip: filter and repair) and the loop-free-alternate pass over
// restore events (spf_elfa.hip) share, so that an *effective* link cannot mean two things.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_kernels.h"

namespace openr_spf {
namespace restore {

constexpr uint32_t kMaxMetric = 0x7FFFFFFFu;

// Event i's three slices in global memory, clamped to their arrays, and what they say about a
// single id. The filter has nothing else; the repair asks them while it builds its bitmaps.
struct Slices {
  const DevGraph& g;
  const RestorePass& p;
  const bool unit_cost;
  uint32_t nb = 0, ne = 0, lb = 0, le = 0, eb = 0, ee = 0;
  uint32_t src = 0;

  __device__ __forceinline__ Slices(const DevGraph& g_, const RestorePass& p_)
      : g(g_), p(p_), unit_cost(p_.unit_cost != 0) {}
  __device__ __forceinline__ void begin(uint32_t i, uint32_t src_) {
    src = src_;
    nb = min(p.node_ptr[i], p.n_nodes);
    ne = min(max(p.node_ptr[i + 1], nb), p.n_nodes);
    lb = le = eb = ee = 0;
    if (p.link_ptr) {
      lb = min(p.link_ptr[i], p.n_links);
      le = min(max(p.link_ptr[i + 1], lb), p.n_links);
    }
    if (p.edge_ptr && !unit_cost) {  // metrics do not enter the hop-count form
      eb = min(p.edge_ptr[i], p.n_edges);
      ee = min(max(p.edge_ptr[i + 1], eb), p.n_edges);
    }
  }
  // the metric e carries after the event, `old` being w(e). A slice that does not ascend may
  // miss its entry or find another one; the edge then keeps `old`.
  __device__ __forceinline__ uint32_t wnew(uint32_t e, uint32_t old) const {
    uint32_t lo = eb, hi = ee;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (p.edges[mid] < e) lo = mid + 1u;
      else hi = mid;
    }
    if (lo >= ee || p.edges[lo] != e) return old;
    const uint32_t m = p.metrics[lo];
    return m >= 1u && m < old ? m : old;
  }
  // x undrains: listed, overloaded and not the source (which expands anyway)
  __device__ __forceinline__ bool undrains(uint32_t x) const { return x < g.V && x != src && g.ovl[x] != 0; }
  // l comes up: a used id, down today, and both its edges fit the fast plans afterwards
  __device__ __forceinline__ bool comes_up(uint32_t l) const {
    if (l >= g.L) return false;
    const uint2 de = g.ledge[l];
    if (de.x == UINT32_MAX || !(g.adj[de.x] & kEdgeDown)) return false;
    if (unit_cost) return true;
    const uint32_t w0 = wnew(de.x, g.w[de.x]), w1 = wnew(de.y, g.w[de.y]);
    return w0 >= 1u && w0 <= kMaxMetric && w1 >= 1u && w1 <= kMaxMetric;
  }
  __device__ __forceinline__ bool node_listed(uint32_t x) const {
    bool in = false;
    for (uint32_t k = nb; k < ne && !in; ++k) in = p.nodes[k] == x;
    return in;
  }
  __device__ __forceinline__ bool link_listed(uint32_t l) const {
    bool in = false;
    for (uint32_t k = lb; k < le && !in; ++k) in = p.links[k] == l;
    return in;
  }
};

}  // namespace restore
}  // namespace openr_spf
