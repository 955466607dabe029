// spf_lfa.hip — loop-free alternates (RFC 5286) over prefix groups: the LFA half of
// SpfSolver::getNextHopsWithMetric (Decision.cpp:1169-1204) for a batch of sources
// (openr_spf_lfa_routes*). spf_routes.hip holds the shortest-path half.
//
// The rule is getNextHopsWithMetric(me, group, perDestination = false, one area) with
// computeLfaPaths_ on, applied literally to the rows openr_spf_solve gives. For source s and
// group k, with (metric, nh) the route openr_spf_routes returns:
//   - metric == UINT64_MAX (no member reached, an empty group): alt is empty; the reference
//     `continue`s before the LFA loop, and metric + toMe is never formed (it would wrap).
//   - otherwise every distinct neighbour n of s with at least one up link s-n is tested
//     (next-hop bit b = its index in openr_spf_neighbor_map), with toMe = dist_n(s). Every
//     member d of the group is tested, not only the members at the minimum: d qualifies when
//     dist_n(d) != UINT64_MAX and dist_n(d) < metric + toMe. Bit b of alt is set iff some
//     member qualifies.
//   - alt_metric(b) is what the reference keeps under key (n, ""): the minimum of dist_n(d)
//     over the qualifying members, and of metric - dist_s(n) as well when b is in nh.
//   The RIB's next hops are nh | alt; the LFA-only ones alt & ~nh. A neighbour behind down
//   links only is never tested; an overloaded neighbour is (its own SPF expands it as the
//   source); a group that holds s has metric 0 and no nh, and its other members can still
//   qualify a neighbour.
//
// lfa_rows_mark / _count / _compact: the rows a batch needs are the distinct nodes among the
//   sources and their up neighbours. The sources are marked in one V-bit map and their up
//   neighbours in another; the words of (neighbours & ~sources) are counted, scanned
//   (launch_delta_scan) and compacted into the list of extra nodes to solve, distances only.
//   rowidx[v] = the distance row of node v: a source's own position in the batch, or
//   n + its rank in the list.
// lfa_nbr_table: per source, entry b of its row of the table (at the CSR offset of the
//   source's edges, so duplicate sources share it) = (distance row of neighbour b, toMe,
//   dist_s(n)); the row index is kNoRow for a neighbour with no up link.
// lfa_reduce_small: one workgroup per (source, tile of 256 groups). A lane owns a group of at
//   most small_max members; the source's table is staged in LDS a slice at a time, and the
//   neighbour loop is the outer, workgroup-uniform loop, so consecutive lanes (consecutive
//   groups: a table's loopbacks) read each neighbour's row coalesced. alt is built a byte at a
//   time, 8 neighbours per byte; no next-hop width is assumed.
// lfa_reduce_large: one wave per (source, larger group), lanes stride the members and the
//   wave reduces the minimum of the qualifying distances per neighbour.
// Both come as a count pass (alt, popcount(alt)) and an emit pass that walks the neighbours
// in the same order and writes (bit, alt_metric) from ptr[unit] on, bits ascending.
//
// Barriers and wave collectives sit only in loops whose trip counts are workgroup- or
// wave-uniform (block / readfirstlane'd wave ids, values read at uniform addresses); the
// member loops have per-lane trip counts and hold none (tests/test_lfa_api.py). Malformed
// device-form input reads nothing out of bounds: group slices are clamped to the M entries
// of gnodes, a member >= V counts as unreached, a source >= V has no neighbour.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "spf_device.h"
#include "spf_kernels.h"

namespace openr_spf {
namespace {

constexpr unsigned long long kUnreached = ~0ull;
constexpr uint32_t kNoRow = 0xFFFFFFFFu;

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

// One workgroup per source: its own bit in srcbm, its up neighbours' bits in need.
__global__ __launch_bounds__(256) void lfa_rows_mark(const uint32_t* sources, uint32_t n, uint32_t V,
                                                     const uint2* row2, const uint32_t* adj, uint32_t* need,
                                                     uint32_t* srcbm, uint32_t* rowidx) {
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t s = sources[i];
    if (s >= V) continue;
    const uint2 r = row2[s];
    if (threadIdx.x == 0) {
      atomicOr(&srcbm[s >> 5], 1u << (s & 31u));
      rowidx[s] = i;  // duplicates of s hold equal rows: any of them
    }
    for (uint32_t e = r.x + threadIdx.x; e < r.y; e += 256u) {
      const uint32_t v = adj[e];
      if (v < V) atomicOr(&need[v >> 5], 1u << (v & 31u));  // kEdgeDown set: v >= V
    }
  }
}

__global__ __launch_bounds__(256) void lfa_rows_count(uint32_t words, const uint32_t* need, const uint32_t* srcbm,
                                                      uint32_t* cnt) {
  for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w < words; w += gridDim.x * 256u)
    cnt[w] = (uint32_t)__popc(need[w] & ~srcbm[w]);
}

// list[wptr[w] ..) = the nodes of word w that are needed and are no source, ascending
__global__ __launch_bounds__(256) void lfa_rows_compact(uint32_t words, uint32_t V, const uint32_t* need,
                                                        const uint32_t* srcbm, const unsigned long long* wptr,
                                                        uint32_t base, uint32_t* list, uint32_t* rowidx) {
  for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w < words; w += gridDim.x * 256u) {
    uint32_t x = need[w] & ~srcbm[w];
    unsigned long long at = wptr[w];
    while (x) {
      const uint32_t v = w * 32u + (uint32_t)__builtin_ctz(x);
      x &= x - 1u;
      if (v >= V || at >= V) break;
      list[at] = v;
      rowidx[v] = base + (uint32_t)at;
      ++at;
    }
  }
}

// One workgroup per source: the table row of its distinct neighbours (trow starts at kNoRow).
// Parallel up links of one neighbour write equal values.
__global__ __launch_bounds__(256) void lfa_nbr_table(const uint32_t* sources, uint32_t n, uint32_t V,
                                                     const uint2* row2, const uint32_t* adj, const uint16_t* nbr,
                                                     const uint32_t* rowidx, const unsigned long long* dist,
                                                     uint32_t* trow, unsigned long long* ttome,
                                                     unsigned long long* tfrom) {
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t s = sources[i];
    if (s >= V) continue;
    const uint2 r = row2[s];
    const unsigned long long* srow = dist + (size_t)i * V;
    for (uint32_t e = r.x + threadIdx.x; e < r.y; e += 256u) {
      const uint32_t v = adj[e];
      if (v >= V) continue;  // down
      const uint32_t slot = r.x + nbr[e];
      if (slot >= r.y) continue;
      const uint32_t ri = rowidx[v];
      trow[slot] = ri;
      ttome[slot] = dist[(size_t)ri * V + s];
      tfrom[slot] = srow[v];
    }
  }
}

__global__ __launch_bounds__(256) void lfa_ptr_shift(unsigned long long* ptr, size_t n, unsigned long long carry) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) ptr[i] += carry;
}

// minimum of dist_n(d) over the members d of [b, e) (stride `step`) that qualify
__device__ __forceinline__ unsigned long long lfa_members(const LfaPass& p, const unsigned long long* nrow,
                                                          uint32_t b, uint32_t e, uint32_t step,
                                                          unsigned long long bound) {
  unsigned long long mn = kUnreached;
  for (uint32_t m = b; m < e; m += step) {
    const uint32_t v = p.gnodes[m];
    const unsigned long long d = v < p.V ? nrow[v] : kUnreached;
    if (d < bound) mn = min(mn, d);  // bound <= UINT64_MAX: an unreached member never qualifies
  }
  return mn;
}

template <bool EMIT>
__global__ __launch_bounds__(256) void lfa_reduce_small(LfaPass p) {
  extern __shared__ unsigned long long lfa_lds[];
  unsigned long long* l_tome = lfa_lds;
  unsigned long long* l_from = lfa_lds + p.slice;
  uint32_t* l_row = reinterpret_cast<uint32_t*>(lfa_lds + 2u * p.slice);
  const uint32_t tiles_g = (p.G + 255u) / 256u;
  const size_t tiles = (size_t)p.n * tiles_g;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint32_t i = (uint32_t)(t / tiles_g);
    const uint32_t k = (uint32_t)(t % tiles_g) * 256u + threadIdx.x;
    const uint32_t s = p.sources[i];
    const uint2 r = s < p.V ? p.row2[s] : make_uint2(0u, 0u);
    const uint32_t nbits = r.y - r.x;  // >= the distinct degree; entries past it are kNoRow
    const size_t it = (size_t)i * p.G + min(k, p.G - 1u);
    GroupRange gr{0u, 0u};
    bool mine = false;  // this lane writes the unit's outputs
    unsigned long long metric = kUnreached;
    if (k < p.G) {
      gr = group_range(p.gptr, k, p.M);
      mine = gr.e - gr.b <= p.small_max;  // else lfa_reduce_large's
      if (mine) metric = p.metric[it];
    }
    if (metric == kUnreached) gr.e = gr.b;  // no member loop: alt stays empty
    uint32_t cnt = 0;
    unsigned long long pos = 0, end = 0;
    if (EMIT && mine) {
      pos = p.optr[it];
      end = p.optr[it + 1];
    }
    for (uint32_t b0 = 0; b0 < nbits; b0 += p.slice) {
      __syncthreads();  // the previous slice is consumed
      for (uint32_t j = threadIdx.x; j < p.slice; j += 256u) {
        const bool ok = b0 + j < nbits;
        l_row[j] = ok ? p.trow[r.x + b0 + j] : kNoRow;
        l_tome[j] = ok ? p.ttome[r.x + b0 + j] : 0ull;
        l_from[j] = ok ? p.tfrom[r.x + b0 + j] : 0ull;
      }
      __syncthreads();
      const uint32_t sn = min(p.slice, nbits - b0);
      for (uint32_t j0 = 0; j0 < sn; j0 += 8u) {  // p.slice is a multiple of 8
        uint32_t byte = 0;
        for (uint32_t t8 = 0; t8 < 8u; ++t8) {
          const uint32_t ri = l_row[j0 + t8];
          if (ri == kNoRow || gr.e == gr.b) continue;
          const unsigned long long mn =
              lfa_members(p, p.dist + (size_t)ri * p.V, gr.b, gr.e, 1u, metric + l_tome[j0 + t8]);
          if (mn == kUnreached) continue;
          byte |= 1u << t8;
          ++cnt;
          if (EMIT) {
            const uint32_t b = b0 + j0 + t8, q = b >> 3;
            unsigned long long am = mn;
            if (q < p.onb && ((p.nh[it * p.onb + q] >> (b & 7u)) & 1u)) am = min(am, metric - l_from[j0 + t8]);
            if (pos < end) {
              p.onbr[pos] = b;
              p.ometric[pos] = am;
            }
            ++pos;
          }
        }
        const uint32_t q = (b0 + j0) >> 3;
        if (!EMIT && mine && p.alt && q < p.onb) p.alt[it * p.onb + q] = (uint8_t)byte;
      }
    }
    if (!EMIT && mine) {
      if (p.alt)
        for (uint32_t q = min(p.onb, (nbits + 7u) >> 3); q < p.onb; ++q) p.alt[it * p.onb + q] = 0;
      if (p.nalt) p.nalt[it] = cnt;
    }
  }
}

// One wave per (source, large group). The item loop, the byte loop and the loop over a
// byte's 8 neighbours are wave-uniform; the reduction sits outside the member loop and
// outside every condition.
template <bool EMIT>
__global__ __launch_bounds__(256) void lfa_reduce_large(LfaPass p) {
  const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nl = min(*p.n_large, p.G);
  const size_t items = (size_t)p.n * nl;
  for (size_t wi = (size_t)blockIdx.x * 4u + wave; wi < items; wi += (size_t)gridDim.x * 4u) {
    const uint32_t i = (uint32_t)(wi / nl);
    const uint32_t k = min(p.large[wi % nl], p.G - 1u);
    const GroupRange gr = group_range(p.gptr, k, p.M);
    const uint32_t s = p.sources[i];
    const uint2 r = s < p.V ? p.row2[s] : make_uint2(0u, 0u);
    const uint32_t nbits = r.y - r.x;
    const size_t it = (size_t)i * p.G + k;
    const unsigned long long metric = p.metric[it];
    const uint32_t nbytes = metric != kUnreached ? (nbits + 7u) >> 3 : 0u;
    uint32_t cnt = 0;
    unsigned long long pos = 0, end = 0;
    if (EMIT) {
      pos = p.optr[it];
      end = p.optr[it + 1];
    }
    for (uint32_t q = 0; q < nbytes; ++q) {
      uint32_t byte = 0;
      for (uint32_t t8 = 0; t8 < 8u; ++t8) {
        const uint32_t b = q * 8u + t8;
        const uint32_t ri = b < nbits ? p.trow[r.x + b] : kNoRow;
        unsigned long long mn = kUnreached;
        if (ri != kNoRow)
          mn = lfa_members(p, p.dist + (size_t)ri * p.V, gr.b + lane, gr.e, 64u, metric + p.ttome[r.x + b]);
        mn = wave_min_u64(mn);
        if (mn == kUnreached) continue;
        byte |= 1u << t8;
        ++cnt;
        if (EMIT) {
          unsigned long long am = mn;
          if (q < p.onb && ((p.nh[it * p.onb + q] >> t8) & 1u)) am = min(am, metric - p.tfrom[r.x + b]);
          if (lane == 0 && pos < end) {
            p.onbr[pos] = b;
            p.ometric[pos] = am;
          }
          ++pos;
        }
      }
      if (!EMIT && lane == 0 && p.alt && q < p.onb) p.alt[it * p.onb + q] = (uint8_t)byte;
    }
    if (!EMIT && lane == 0) {
      if (p.alt)
        for (uint32_t q = min(p.onb, nbytes); q < p.onb; ++q) p.alt[it * p.onb + q] = 0;
      if (p.nalt) p.nalt[it] = cnt;
    }
  }
}

uint32_t capped_grid(uint64_t blocks, int num_cus, uint32_t per_cu) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)num_cus * per_cu));
}

}  // namespace

uint32_t lfa_slice() {
  // neighbours of a source staged in LDS at a time (20 B each); OPENR_SPF_LFA_SLICE (tests)
  uint32_t s = 256u;
  if (const char* e = std::getenv("OPENR_SPF_LFA_SLICE")) s = (uint32_t)std::strtoul(e, nullptr, 10);
  s = std::max(8u, std::min(s, 2048u));
  return (s + 7u) & ~7u;
}

hipError_t launch_lfa_rows(const DevGraph& g, const uint32_t* sources, uint32_t n, uint32_t* need, uint32_t* srcbm,
                           uint32_t* cnt, unsigned long long* tsum, unsigned long long* wptr, uint32_t* list,
                           uint32_t* rowidx, int num_cus, hipStream_t s) {
  const uint32_t words = (g.V + 31u) / 32u;
  hipError_t err = hipMemsetAsync(need, 0, (size_t)words * sizeof(uint32_t), s);
  if (err == hipSuccess) err = hipMemsetAsync(srcbm, 0, (size_t)words * sizeof(uint32_t), s);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(lfa_rows_mark, dim3(capped_grid(n, num_cus, 16u)), dim3(256), 0, s, sources, n, g.V, g.row2,
                     g.adj, need, srcbm, rowidx);
  const uint32_t wg = capped_grid((words + 255u) / 256u, num_cus, 8u);
  hipLaunchKernelGGL(lfa_rows_count, dim3(wg), dim3(256), 0, s, words, need, srcbm, cnt);
  if ((err = launch_delta_scan(cnt, words, tsum, wptr, s)) != hipSuccess) return err;
  hipLaunchKernelGGL(lfa_rows_compact, dim3(wg), dim3(256), 0, s, words, g.V, need, srcbm, wptr, n, list, rowidx);
  note_launch("lfa_rows");
  return hipGetLastError();
}

hipError_t launch_lfa_table(const DevGraph& g, const uint32_t* sources, uint32_t n, const uint32_t* rowidx,
                            const uint64_t* dist, uint32_t* trow, unsigned long long* ttome,
                            unsigned long long* tfrom, int num_cus, hipStream_t s) {
  hipError_t err = hipMemsetAsync(trow, 0xFF, std::max<size_t>(g.E, 1) * sizeof(uint32_t), s);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(lfa_nbr_table, dim3(capped_grid(n, num_cus, 16u)), dim3(256), 0, s, sources, n, g.V, g.row2,
                     g.adj, g.nbr, rowidx, reinterpret_cast<const unsigned long long*>(dist), trow, ttome, tfrom);
  return hipGetLastError();
}

hipError_t launch_lfa_reduce(const LfaPass& pass, bool emit, int num_cus, hipStream_t s) {
  if (!pass.n || !pass.G) return hipSuccess;
  LfaPass p = pass;
  p.small_max = routes_small_max();
  p.slice = lfa_slice();
  const uint32_t lds = p.slice * 20u;
  const uint64_t tiles = (uint64_t)p.n * ((p.G + 255u) / 256u);
  const uint32_t gs = capped_grid(tiles, num_cus, 16u);
  const uint32_t gl = capped_grid(((uint64_t)p.n * p.G + 3u) / 4u, num_cus, 8u);
  if (emit) {
    hipLaunchKernelGGL(lfa_reduce_small<true>, dim3(gs), dim3(256), lds, s, p);
    hipLaunchKernelGGL(lfa_reduce_large<true>, dim3(gl), dim3(256), 0, s, p);
  } else {
    hipLaunchKernelGGL(lfa_reduce_small<false>, dim3(gs), dim3(256), lds, s, p);
    hipLaunchKernelGGL(lfa_reduce_large<false>, dim3(gl), dim3(256), 0, s, p);
  }
  note_launch(emit ? "lfa_reduce_emit" : "lfa_reduce_count");
  return hipGetLastError();
}

hipError_t launch_lfa_ptr_shift(unsigned long long* ptr, size_t n, unsigned long long carry, int num_cus,
                                hipStream_t s) {
  if (!n || !carry) return hipSuccess;
  hipLaunchKernelGGL(lfa_ptr_shift, dim3(capped_grid((n + 255u) / 256u, num_cus, 8u)), dim3(256), 0, s, ptr, n, carry);
  return hipGetLastError();
}

}  // namespace openr_spf
