// spf_routes.hip — route-level results: best-path selection over prefix groups and the
// route-level what-if pass (openr_spf_routes*, openr_spf_whatif_routes*). The other half of
// next-hop selection, loop-free alternates (Decision.cpp:1169-1204), is spf_lfa.hip
// (openr_spf_lfa_routes*), which runs on the routes this file reduces.
//
// A prefix is advertised by a group of nodes (anycast). Its route at a source is
//   metric = min dist[v] over the members in the SpfResult,
//   nh     = OR of nh[v] over the members at that minimum,
//   n_best = members at the minimum
// (SpfSolver::getMinCostNodes and the shortest-path half of getNextHopsWithMetric,
// Decision.cpp:1094-1167). Groups are a CSR (gptr, gnodes), node ids ascending inside a
// group. Malformed device-form input reads nothing out of bounds: group slices are clamped
// to the M entries of gnodes and a member >= V counts as unreached.
//
// routes_reduce_small / _large: routes of every (row, group) from row-major dist / nh rows.
//   A lane owns a group of at most `small_max` members (loopbacks are singletons: 64 routes
//   per wave); a wave owns each larger group (listed by routes_list_large).
// whatif_routes_kernel: one 64-thread workgroup per what-if unit with a non-empty node
//   delta. The unit's delta entries are overlaid on the source's base row through a
//   node -> entry index array, the groups with a changed member become the candidates
//   (inverse map node -> groups), each candidate's route is recomputed and compared with
//   the base route. A count pass, a scan and an emit pass.
//
// Wave collectives (shuffles) sit only in routes_reduce_large, inside loops whose trip
// counts come from readfirstlane'd wave ids and kernel arguments; whatif_routes_kernel has
// none, and its barriers sit in the block-uniform unit loop (tests/test_routes_api.py).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "spf_device.h"
#include "spf_kernels.h"

namespace openr_spf {
namespace {

constexpr unsigned long long kUnreached = ~0ull;

struct GroupRange {
  uint32_t b, e;
};
__device__ __forceinline__ GroupRange group_range(const uint32_t* gptr, uint32_t k, uint32_t M) {
  const uint32_t e = min(gptr[k + 1], M);
  return {min(gptr[k], e), e};
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = min(x, (unsigned long long)__shfl_xor((long long)x, o));
  return x;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o);
  return x;
}
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x |= (uint32_t)__shfl_xor((int)x, o);
  return x;
}

// large[0 .. *n_large) = the groups with more than small_max members (any order)
__global__ __launch_bounds__(256) void routes_list_large(uint32_t G, uint32_t M, const uint32_t* gptr,
                                                         uint32_t small_max, uint32_t* large, uint32_t* n_large) {
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < G; k += gridDim.x * 256u) {
    const GroupRange r = group_range(gptr, k, M);
    if (r.e - r.b > small_max) large[atomicAdd(n_large, 1u)] = k;
  }
}

// One lane per (row, group) with at most small_max members. Consecutive lanes take
// consecutive groups of one row: a table's loopback groups read the row coalesced.
__global__ __launch_bounds__(256) void routes_reduce_small(uint32_t n, uint32_t V, uint32_t G, uint32_t M,
                                                           const uint32_t* gptr, const uint32_t* gnodes,
                                                           const unsigned long long* dist, const uint8_t* nh,
                                                           uint32_t nb, unsigned long long* metric, uint8_t* onh,
                                                           uint32_t onb, uint32_t* nbest, uint32_t small_max) {
  const size_t items = (size_t)n * G;
  for (size_t it = (size_t)blockIdx.x * 256u + threadIdx.x; it < items; it += (size_t)gridDim.x * 256u) {
    const size_t r = it / G;
    const uint32_t k = (uint32_t)(it % G);
    const GroupRange gr = group_range(gptr, k, M);
    if (gr.e - gr.b > small_max) continue;  // routes_reduce_large's
    const unsigned long long* dr = dist + r * V;
    unsigned long long mn = kUnreached;
    uint32_t cnt = 0, first = gr.e;
    for (uint32_t m = gr.b; m < gr.e; ++m) {
      const uint32_t v = gnodes[m];
      const unsigned long long d = v < V ? dr[v] : kUnreached;
      if (d < mn) {
        mn = d;
        cnt = 1;
        first = m;
      } else if (d == mn && d != kUnreached) {
        ++cnt;
      }
    }
    metric[it] = mn;
    if (nbest) nbest[it] = cnt;
    if (!onh) continue;
    uint8_t* o = onh + it * onb;
    const uint8_t* hr = nh + r * V * nb;
    for (uint32_t q = 0; q < onb; ++q) {
      uint32_t x = 0;
      if (q < nb && cnt) {
        x = hr[(size_t)gnodes[first] * nb + q];
        for (uint32_t m = first + 1u; cnt > 1u && m < gr.e; ++m) {
          const uint32_t v = gnodes[m];
          if (v < V && dr[v] == mn) x |= hr[(size_t)v * nb + q];
        }
      }
      o[q] = (uint8_t)x;
    }
  }
}

// One wave per (row, large group): lanes stride the members, the minimum, the count and
// each next-hop byte are reduced across the wave. The item loop and the byte loop are
// wave-uniform (wave id through readfirstlane, counts from memory and arguments); the
// member loops have per-lane trip counts and hold no collective.
__global__ __launch_bounds__(256) void routes_reduce_large(uint32_t n, uint32_t V, uint32_t G, uint32_t M,
                                                           const uint32_t* gptr, const uint32_t* gnodes,
                                                           const unsigned long long* dist, const uint8_t* nh,
                                                           uint32_t nb, unsigned long long* metric, uint8_t* onh,
                                                           uint32_t onb, uint32_t* nbest, const uint32_t* large,
                                                           const uint32_t* n_large) {
  const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nl = min(*n_large, G);
  const size_t items = (size_t)n * nl;
  for (size_t wi = (size_t)blockIdx.x * 4u + wave; wi < items; wi += (size_t)gridDim.x * 4u) {
    const size_t r = wi / nl;
    const uint32_t k = min(large[wi % nl], G - 1u);
    const GroupRange gr = group_range(gptr, k, M);
    const unsigned long long* dr = dist + r * V;
    unsigned long long mn = kUnreached;
    for (uint32_t m = gr.b + lane; m < gr.e; m += 64u) {
      const uint32_t v = gnodes[m];
      if (v < V) mn = min(mn, dr[v]);
    }
    mn = wave_min_u64(mn);
    uint32_t cnt = 0;
    if (mn != kUnreached)
      for (uint32_t m = gr.b + lane; m < gr.e; m += 64u) {
        const uint32_t v = gnodes[m];
        cnt += (v < V && dr[v] == mn) ? 1u : 0u;
      }
    cnt = wave_sum_u32(cnt);
    const size_t it = r * G + k;
    if (lane == 0) {
      metric[it] = mn;
      if (nbest) nbest[it] = cnt;
    }
    if (!onh) continue;
    const uint8_t* hr = nh + r * V * nb;
    for (uint32_t q = 0; q < onb; ++q) {
      uint32_t x = 0;
      if (q < nb && mn != kUnreached)
        for (uint32_t m = gr.b + lane; m < gr.e; m += 64u) {
          const uint32_t v = gnodes[m];
          if (v < V && dr[v] == mn) x |= hr[(size_t)v * nb + q];
        }
      x = wave_or_u32(x);
      if (lane == 0) onh[it * onb + q] = (uint8_t)x;
    }
  }
}

// Inverse map node -> groups: member counts per node, then (after the scan into iptr) the
// group ids of each node (any order).
__global__ __launch_bounds__(256) void routes_inv_count(uint32_t M, uint32_t V, const uint32_t* gnodes,
                                                        uint32_t* cnt) {
  for (uint32_t m = blockIdx.x * 256u + threadIdx.x; m < M; m += gridDim.x * 256u) {
    const uint32_t v = gnodes[m];
    if (v < V) atomicAdd(&cnt[v], 1u);
  }
}

__global__ __launch_bounds__(256) void routes_inv_fill(uint32_t G, uint32_t M, uint32_t V, const uint32_t* gptr,
                                                       const uint32_t* gnodes, const unsigned long long* iptr,
                                                       uint32_t* cur, uint32_t* inv) {
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < G; k += gridDim.x * 256u) {
    const GroupRange gr = group_range(gptr, k, M);
    for (uint32_t m = gr.b; m < gr.e; ++m) {
      const uint32_t v = gnodes[m];
      if (v >= V) continue;
      const unsigned long long slot = iptr[v] + atomicAdd(&cur[v], 1u);
      if (slot < iptr[v + 1]) inv[slot] = k;
    }
  }
}

// Route of group k in unit u's post-failure row: member values from the unit's delta entry
// where the overlay has one (ovl[v] = entry index + 1), from the base row otherwise.
struct UnitRow {
  const uint32_t* ovl;
  const unsigned long long* ndist;  // the unit's delta entries
  const uint8_t* nnh;
  const unsigned long long* bdist;  // the source's base row
  const uint8_t* bnh;
  uint32_t V, nb;
  __device__ unsigned long long dist(uint32_t v) const {
    if (v >= V) return kUnreached;
    const uint32_t i = ovl[v];
    return i ? ndist[i - 1u] : bdist[v];
  }
  __device__ uint32_t nh_byte(uint32_t v, uint32_t q) const {
    const uint32_t i = ovl[v];
    return i ? nnh[(size_t)(i - 1u) * nb + q] : bnh[(size_t)v * nb + q];
  }
};

template <bool EMIT>
__device__ __forceinline__ void eval_candidate(const RoutesSweep& p, const UnitRow& row, size_t u, uint32_t j,
                                               uint32_t k, uint32_t* n_found) {
  const GroupRange gr = group_range(p.gptr, k, p.M);
  unsigned long long mn = kUnreached;
  uint32_t cnt = 0, first = gr.e;
  for (uint32_t m = gr.b; m < gr.e; ++m) {
    const unsigned long long d = row.dist(p.gnodes[m]);
    if (d < mn) {
      mn = d;
      cnt = 1;
      first = m;
    } else if (d == mn && d != kUnreached) {
      ++cnt;
    }
  }
  // next-hop byte q of the new route (first / cnt: the members at the minimum start there)
  auto nh_byte = [&](uint32_t q) -> uint32_t {
    if (!cnt) return 0u;
    uint32_t x = row.nh_byte(p.gnodes[first], q);
    for (uint32_t m = first + 1u; cnt > 1u && m < gr.e; ++m) {
      const uint32_t v = p.gnodes[m];
      if (row.dist(v) == mn) x |= row.nh_byte(v, q);
    }
    return x;
  };
  const size_t bi = (size_t)j * p.G + k;
  bool diff = mn != p.bmetric[bi];
  for (uint32_t q = 0; !diff && q < p.nb; ++q) diff = nh_byte(q) != p.bmnh[bi * p.nb + q];
  if (!diff) return;
  const uint32_t slot = atomicAdd(n_found, 1u);
  if (!EMIT) return;
  const unsigned long long o = p.optr[u] + slot;
  if (o >= p.optr[u + 1]) return;
  p.ogroup[o] = k;
  p.ometric[o] = mn;
  if (p.onbest) p.onbest[o] = cnt;
  uint8_t* oh = p.onh + o * p.onb;
  for (uint32_t q = 0; q < p.onb; ++q) oh[q] = (uint8_t)(q < p.nb ? nh_byte(q) : 0u);
}

// One 64-thread workgroup per unit with a non-empty node delta (block-stride, so the unit
// loop and its barriers are uniform). LDS: [0] candidates, [1] changed routes, the
// candidate list, then the overlay and the candidate bitmap when they fit (else a slice
// of global scratch per workgroup; both are zero at rest and cleared from the unit's own
// entries). A candidate list that overflows falls back to a scan of the bitmap.
template <bool EMIT>
__global__ __launch_bounds__(64) void whatif_routes_kernel(RoutesSweep p) {
  extern __shared__ uint32_t lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t bmw = (p.G + 31u) / 32u;
  uint32_t* ctr = lds;
  uint32_t* cand = lds + 2;
  uint32_t* l_ovl = cand + p.cand_cap;
  uint32_t* l_bm = l_ovl + (p.ovl_lds ? p.V : 0u);
  uint32_t* ovl = p.ovl_lds ? l_ovl : p.g_ovl + (size_t)blockIdx.x * p.V;
  uint32_t* bm = p.bm_lds ? l_bm : p.g_bm + (size_t)blockIdx.x * bmw;
  if (p.ovl_lds)
    for (uint32_t i = lane; i < p.V; i += 64u) l_ovl[i] = 0u;
  if (p.bm_lds)
    for (uint32_t i = lane; i < bmw; i += 64u) l_bm[i] = 0u;
  if (lane < 2u) ctr[lane] = 0u;
  __syncthreads();
  for (size_t u = blockIdx.x; u < p.units; u += gridDim.x) {
    const unsigned long long e0 = p.nptr[u], e1 = p.nptr[u + 1];
    if (e0 >= e1) continue;  // no node changed: no route can (the count pass's changed[] is pre-zeroed)
    if (EMIT && p.optr[u] == p.optr[u + 1]) continue;
    const uint32_t j = (uint32_t)(u % p.n_src);
    // 1. overlay the unit's entries on the base row; groups with a changed member are candidates
    for (unsigned long long t = e0 + lane; t < e1; t += 64u) {
      const uint32_t v = p.nnode[t];
      if (v >= p.V) continue;
      ovl[v] = (uint32_t)(t - e0) + 1u;
      for (unsigned long long i = p.iptr[v]; i < p.iptr[v + 1]; ++i) {
        const uint32_t k = p.inv[i];
        if (k >= p.G) continue;
        const uint32_t bit = 1u << (k & 31u);
        if (atomicOr(&bm[k >> 5], bit) & bit) continue;
        const uint32_t slot = atomicAdd(&ctr[0], 1u);
        if (slot < p.cand_cap) cand[slot] = k;
      }
    }
    __syncthreads();
    // 2. recompute every candidate's route and compare it with the base route
    UnitRow row{ovl, p.ndist + e0, p.nnh + e0 * p.nb, p.bdist + (size_t)j * p.V, p.bnh + (size_t)j * p.V * p.nb,
                p.V, p.nb};
    const uint32_t nc = ctr[0];
    if (nc <= p.cand_cap) {
      for (uint32_t c = lane; c < nc; c += 64u) eval_candidate<EMIT>(p, row, u, j, cand[c], &ctr[1]);
    } else {  // the list overflowed: every set bit of the bitmap
      for (uint32_t w = lane; w < bmw; w += 64u) {
        uint32_t bits = bm[w];
        while (bits) {
          const uint32_t k = w * 32u + (uint32_t)__builtin_ctz(bits);
          bits &= bits - 1u;
          eval_candidate<EMIT>(p, row, u, j, k, &ctr[1]);
        }
      }
    }
    __syncthreads();
    // 3. clear the overlay and the bitmap from the same entries
    for (unsigned long long t = e0 + lane; t < e1; t += 64u) {
      const uint32_t v = p.nnode[t];
      if (v >= p.V) continue;
      ovl[v] = 0u;
      for (unsigned long long i = p.iptr[v]; i < p.iptr[v + 1]; ++i) {
        const uint32_t k = p.inv[i];
        if (k < p.G) bm[k >> 5] = 0u;
      }
    }
    if (lane == 0) {
      if (!EMIT) p.changed[u] = ctr[1];
      ctr[0] = 0u;
      ctr[1] = 0u;
    }
    __syncthreads();
  }
}

}  // namespace

uint32_t routes_reduce_scratch_words(uint32_t G) { return G + 1u; }

uint32_t routes_small_max() {
  // groups above this size get a wave; OPENR_SPF_ROUTES_SMALL_MAX (tests) moves the boundary
  if (const char* e = std::getenv("OPENR_SPF_ROUTES_SMALL_MAX")) return (uint32_t)std::strtoul(e, nullptr, 10);
  return 16u;
}

hipError_t launch_routes_reduce(uint32_t n, uint32_t V, uint32_t G, uint32_t M, const uint32_t* gptr,
                                const uint32_t* gnodes, const uint64_t* dist, const uint8_t* nh, uint32_t nb,
                                uint64_t* metric, uint8_t* onh, uint32_t onb, uint32_t* nbest, uint32_t* scratch,
                                int num_cus, hipStream_t s) {
  if (!n || !G) return hipSuccess;
  const uint32_t small_max = routes_small_max();
  uint32_t* n_large = scratch + G;
  hipError_t err = hipMemsetAsync(n_large, 0, sizeof(uint32_t), s);
  if (err != hipSuccess) return err;
  const uint64_t items = (uint64_t)n * G;
  const uint32_t cap = (uint32_t)num_cus * 8u;
  auto grid = [cap](uint64_t blocks) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, cap)); };
  const unsigned long long* d = reinterpret_cast<const unsigned long long*>(dist);
  unsigned long long* mt = reinterpret_cast<unsigned long long*>(metric);
  hipLaunchKernelGGL(routes_list_large, dim3(grid((G + 255u) / 256u)), dim3(256), 0, s, G, M, gptr, small_max,
                     scratch, n_large);
  hipLaunchKernelGGL(routes_reduce_small, dim3(grid((items + 255u) / 256u)), dim3(256), 0, s, n, V, G, M, gptr,
                     gnodes, d, nh, nb, mt, onh, onb, nbest, small_max);
  hipLaunchKernelGGL(routes_reduce_large, dim3(grid((items + 3u) / 4u)), dim3(256), 0, s, n, V, G, M, gptr, gnodes,
                     d, nh, nb, mt, onh, onb, nbest, scratch, n_large);
  note_launch("routes_reduce");
  return hipGetLastError();
}

hipError_t launch_routes_inverse(uint32_t V, uint32_t G, uint32_t M, const uint32_t* gptr, const uint32_t* gnodes,
                                 uint32_t* cnt, uint32_t* cur, unsigned long long* tsum, unsigned long long* iptr,
                                 uint32_t* inv, int num_cus, hipStream_t s) {
  hipError_t err = hipMemsetAsync(cnt, 0, (size_t)V * sizeof(uint32_t), s);
  if (err == hipSuccess) err = hipMemsetAsync(cur, 0, (size_t)V * sizeof(uint32_t), s);
  if (err != hipSuccess) return err;
  const uint32_t cap = (uint32_t)num_cus * 8u;
  if (M)
    hipLaunchKernelGGL(routes_inv_count, dim3(std::max(1u, std::min((M + 255u) / 256u, cap))), dim3(256), 0, s, M, V,
                       gnodes, cnt);
  if ((err = launch_delta_scan(cnt, V, tsum, iptr, s)) != hipSuccess) return err;
  if (M && G)
    hipLaunchKernelGGL(routes_inv_fill, dim3(std::max(1u, std::min((G + 255u) / 256u, cap))), dim3(256), 0, s, G, M,
                       V, gptr, gnodes, iptr, cur, inv);
  return hipGetLastError();
}

RoutesSweepLayout whatif_routes_layout(uint32_t V, uint32_t G, size_t units, int num_cus) {
  auto knob = [](const char* name, uint32_t dflt) {
    const char* e = std::getenv(name);
    return e ? (uint32_t)std::strtoul(e, nullptr, 10) : dflt;
  };
  RoutesSweepLayout l;
  // the overlay lives in LDS up to OPENR_SPF_ROUTES_LDS_NODES nodes, the candidate
  // bitmap up to OPENR_SPF_ROUTES_LDS_GROUPS groups, the candidate list holds
  // OPENR_SPF_ROUTES_CAND_CAP groups (defaults: 48 KiB of LDS at most)
  l.ovl_lds = V <= std::min(knob("OPENR_SPF_ROUTES_LDS_NODES", 8192u), 8192u);
  l.bm_lds = G <= std::min(knob("OPENR_SPF_ROUTES_LDS_GROUPS", 65536u), 65536u);
  l.cand_cap = std::min(knob("OPENR_SPF_ROUTES_CAND_CAP", 1024u), 1024u);
  const uint32_t bmw = (G + 31u) / 32u;
  l.lds_bytes = 4u * (2u + l.cand_cap + (l.ovl_lds ? V : 0u) + (l.bm_lds ? bmw : 0u));
  l.grid = blocks_for((uint32_t)std::min<size_t>(units, 0xFFFFFFFFu), l.lds_bytes, num_cus, 64u);
  l.ovl_words = l.ovl_lds ? 0u : (size_t)l.grid * V;
  l.bm_words = l.bm_lds ? 0u : (size_t)l.grid * bmw;
  return l;
}

hipError_t launch_whatif_routes(const RoutesSweep& p, const RoutesSweepLayout& l, bool emit, hipStream_t s) {
  if (!p.units || !p.G) return hipSuccess;
  hipError_t err = hipSuccess;
  if (!emit) {  // global overlay / bitmap slices start zeroed; every unit leaves them zeroed
    if (l.ovl_words) err = hipMemsetAsync(p.g_ovl, 0, l.ovl_words * sizeof(uint32_t), s);
    if (err == hipSuccess && l.bm_words) err = hipMemsetAsync(p.g_bm, 0, l.bm_words * sizeof(uint32_t), s);
    if (err != hipSuccess) return err;
  }
  if (emit)
    hipLaunchKernelGGL(whatif_routes_kernel<true>, dim3(l.grid), dim3(64), l.lds_bytes, s, p);
  else
    hipLaunchKernelGGL(whatif_routes_kernel<false>, dim3(l.grid), dim3(64), l.lds_bytes, s, p);
  note_launch(emit ? "whatif_routes_emit" : "whatif_routes_count");
  return hipGetLastError();
}

}  // namespace openr_spf
