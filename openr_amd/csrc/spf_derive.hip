// spf_derive.hip — rows of independent sources derived from their neighbours' rows.
//
// Uniform cost c (LinkState::runSpf closed form, as spf_bfs_lvl.hip): for a source s with
// distinct neighbours n_0 .. n_{k-1} (bit i as DevGraph::nbr), n_i usable when some link
// s - n_i is up and n_i != s,
//   cand_i(v) = 1                 if v == n_i (an overloaded n_i counts here),
//             = lvl_{n_i}(v) + 1  if n_i is not overloaded and lvl_{n_i}(v) is set,
//             = unset             otherwise (every unusable n_i included);
//   lvl_s(s) = 0, lvl_s(v) = min_i cand_i(v) (unset if every candidate is);
//   dist = lvl * c, UINT64_MAX when unset;
//   bit i of nh_s(v) is set iff v != s and cand_i(v) == lvl_s(v), which must be set.
// lvl_{n_i} is the row of n_i solved as a source (a source expands even when overloaded,
// which is why an overloaded n_i contributes itself only); s's own overload bit does not
// matter. So in a batch that holds the rows of every needed neighbour, s needs no BFS.
//
// Per call: mark (member[node] = sid), classify (derived iff the node is in the graph's
// derive colouring and every needed neighbour is a source of the batch), a one-workgroup
// scan into two ascending lists, the BFS launch over the solved list (its units also leave
// their u8 level rows, spf_bfs_lvl.hip), then nh_derive_kernel over the derived list.
#include <algorithm>

#include "spf_bfs_common.h"
#include "spf_kernels.h"

namespace openr_spf {

namespace {
using namespace bfs;

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kUnset = 0xFFFFu;  // a candidate level (set ones are <= 255)

__global__ __launch_bounds__(256) void derive_mark_kernel(const uint32_t* sources, uint32_t n, uint32_t V,
                                                          uint32_t* member) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const uint32_t s = sources[i];
    if (s < V) member[s] = i;  // duplicates: any of them (their rows are equal)
  }
}

// member is never cleared: an entry counts only when it names a sid of this batch with
// that source.
__device__ __forceinline__ bool in_batch(const uint32_t* member, const uint32_t* sources, uint32_t n, uint32_t v,
                                         uint32_t* sid) {
  const uint32_t m = member[v];
  *sid = m;
  return m < n && sources[m] == v;
}

// Also leaves a derivable entry's neighbour table (DeriveArgs::nbrs), so nh_derive_kernel
// starts a unit from one 32-byte read instead of the walk over the source's CSR row.
__global__ __launch_bounds__(256) void derive_classify_kernel(DevGraph g, const uint32_t* sources, uint32_t n,
                                                              const uint32_t* member, uint8_t* flags, uint32_t* nbrs) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const uint32_t s = sources[i];
    bool d = s < g.V && g.derivable[s];
    if (d) {
      uint32_t* t = nbrs + (size_t)i * (2u * kDeriveMaxNbrs);
      for (uint32_t q = 0; q < 2u * kDeriveMaxNbrs; q += 4u)
        *reinterpret_cast<uint4*>(t + q) = make_uint4(kNone, kNone, kNone, kNone);
      const uint2 rs = g.row2[s];
      for (uint32_t e = rs.x; e < rs.y && d; ++e) {
        const uint32_t av = g.adj[e], v = av & ~kEdgeDown, b = g.nbr[e];
        if ((av & kEdgeDown) || v == s || b >= kDeriveMaxNbrs) continue;  // parallel links: the same values again
        t[b] = v;
        uint32_t m;
        if (!g.ovl[v] && (d = in_batch(member, sources, n, v, &m))) t[kDeriveMaxNbrs + b] = m;
      }
    }
    flags[i] = d ? 1u : 0u;
  }
}

// One workgroup: the two lists in ascending sid order. A thread takes 16 consecutive
// entries (one 16-byte load of their flags), so a step covers 16 384 of them.
constexpr uint32_t kScanBlock = 1024, kScanPer = 16;
__global__ __launch_bounds__(kScanBlock) void derive_scan_kernel(const uint8_t* flags, uint32_t n, uint32_t cls,
                                                                 uint32_t* perm, uint32_t* part, uint32_t* count) {
  __shared__ uint32_t s_wave[kScanBlock / 64u];
  __shared__ uint32_t s_base[2];
  const uint32_t tid = threadIdx.x, lane = __lane_id(), wave = tid >> 6;
  if (tid == 0) s_base[0] = s_base[1] = 0;
  __syncthreads();
  for (uint32_t c0 = 0; c0 < n; c0 += kScanBlock * kScanPer) {
    const uint32_t i0 = c0 + tid * kScanPer;
    uint32_t bits = 0, have = 0;  // derived entries / entries of this thread
    if (i0 < n) {
      const uint4 f = *reinterpret_cast<const uint4*>(flags + i0);  // the buffer holds n + 16 bytes
      const uint32_t w[4] = {f.x, f.y, f.z, f.w};
      have = std::min<uint32_t>(kScanPer, n - i0);
      for (uint32_t k = 0; k < have; ++k) bits |= ((w[k >> 2] >> (8u * (k & 3u))) & 1u) << k;
    }
    const uint32_t nd = (uint32_t)__popc(bits), mine = nd | ((have - nd) << 16);  // derived | solved
    uint32_t inc = mine;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = inc - mine, total = 0;
    for (uint32_t w = 0; w < kScanBlock / 64u; ++w) {
      if (w < wave) before += s_wave[w];
      total += s_wave[w];
    }
    uint32_t pd = s_base[0] + (before & 0xFFFFu), ps = s_base[1] + (before >> 16);
    for (uint32_t k = 0; k < have; ++k) {
      if ((bits >> k) & 1u) perm[n + pd++] = i0 + k;
      else perm[ps++] = i0 + k;
    }
    __syncthreads();
    if (tid == 0) {
      s_base[0] += total & 0xFFFFu;
      s_base[1] += total >> 16;
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[cls] = s_base[1];
    part[kMaxClasses + cls] = 0;
    *count = s_base[0];
  }
}

// The rows of one derived source (all lanes of its workgroup). Lane t takes the node pairs
// (off + 2p, off + 2p + 1) for p = t, t + 256, ...: one 2-byte load per neighbour row, one
// 16-byte store of the two distances (the write-out's layout: a wave's store covers 1 KB of
// the row), and where nh_bytes == 1 the next-hop bytes of eight nodes gathered into one
// 8-byte store. kDerivePairs pairs per lane and step, their loads issued together: the pass
// is bound by the latency of those loads otherwise (G100: 0.187 ms at one pair per step).
// AL16 = false (off = 1): the distance row is only 8-byte aligned (odd V); the nodes
// outside the pairs go out alone.
constexpr uint32_t kDerivePairs = 4;
template <bool NT, bool AL16>
__device__ __forceinline__ void derive_rows(const uint32_t* s_node, const uint32_t* s_row, const DeriveArgs& dv,
                                            uint32_t src, uint32_t V, uint64_t cost, uint64_t* drow, uint8_t* nrow,
                                            uint32_t nb) {
  constexpr uint32_t U = kDerivePairs, NBRS = kDeriveMaxNbrs, off = AL16 ? 0u : 1u;
  const uint32_t tid = threadIdx.x, lane = __lane_id();
  uint32_t nn[NBRS];
  const uint8_t* lr[NBRS];
#pragma unroll
  for (uint32_t i = 0; i < NBRS; ++i) {
    nn[i] = s_node[i];
    const uint32_t r = s_row[i];
    lr[i] = r != kNone ? dv.rows + (size_t)r * dv.stride : nullptr;
  }
  // candidates of a node pair: v0's | v1's << 16 (kUnset: none) from the pair's level bytes
  auto cands = [&](uint32_t i, uint32_t w, uint32_t v0) -> uint32_t {
    if (nn[i] == kNone) return kUnset | (kUnset << 16);  // uniform
    auto one = [](uint32_t l, bool self) { return self ? 1u : l == 0xFFu ? kUnset : l + 1u; };
    return one(w & 0xFFu, v0 == nn[i]) | (one(w >> 8, v0 + 1u == nn[i]) << 16);
  };
  // one node: its level (kUnset: not reached) and next-hop bits
  auto finish = [&](uint32_t v, const uint32_t (&c)[NBRS], uint32_t sh, uint32_t& m, uint32_t& bits) {
    m = kUnset;
    bits = 0;
#pragma unroll
    for (uint32_t i = 0; i < NBRS; ++i) m = min(m, (c[i] >> sh) & 0xFFFFu);
#pragma unroll
    for (uint32_t i = 0; i < NBRS; ++i) bits |= (((c[i] >> sh) & 0xFFFFu) == m ? 1u : 0u) << i;
    if (m == kUnset) bits = 0;
    if (v == src) {
      m = 0;
      bits = 0;
    }
  };
  auto dist_of = [cost](uint32_t m) -> uint64_t { return m == kUnset ? ~(uint64_t)0 : (uint64_t)m * cost; };
  auto nh_out = [&](uint32_t v, uint32_t bits) {
    uint8_t* o = nrow + (size_t)v * nb;
    o[0] = (uint8_t)bits;
    for (uint32_t q = 1; q < nb; ++q) o[q] = 0;
  };
  const uint32_t np = (V - off) / 2u;  // V >= 1
  const bool nh8 = nb == 1u && ((uint32_t)reinterpret_cast<uintptr_t>(nrow + off) & 7u) == 0u;  // uniform
  for (uint32_t base = 0; base < np; base += 256u * U) {  // uniform: every lane takes part in the gathers
    uint32_t w[U][NBRS];
#pragma unroll
    for (uint32_t k = 0; k < U; ++k) {
      const uint32_t p = base + 256u * k + tid;
      const bool live = p < np;
      const uint32_t v0 = off + 2u * (live ? p : 0u);
#pragma unroll
      for (uint32_t i = 0; i < NBRS; ++i) {
        w[k][i] = 0xFFFFu;
        if (lr[i] && live)
          w[k][i] = AL16 ? (uint32_t) * reinterpret_cast<const uint16_t*>(lr[i] + v0)
                         : (uint32_t)lr[i][v0] | ((uint32_t)lr[i][v0 + 1u] << 8);
      }
    }
    // every load of the step is issued before the first is used
#pragma unroll
    for (uint32_t k = 0; k < U; ++k)
#pragma unroll
      for (uint32_t i = 0; i < NBRS; ++i) asm volatile("" : "+v"(w[k][i]));
#pragma unroll
    for (uint32_t k = 0; k < U; ++k) {
      if (base + 256u * k >= np) break;  // uniform
      const uint32_t p = base + 256u * k + tid;
      const bool live = p < np;
      const uint32_t v0 = off + 2u * (live ? p : 0u);
      uint32_t c[NBRS], m0, m1, b0, b1;
#pragma unroll
      for (uint32_t i = 0; i < NBRS; ++i) c[i] = cands(i, w[k][i], v0);
      finish(v0, c, 0u, m0, b0);
      finish(v0 + 1u, c, 16u, m1, b1);
      if (live) store_row<NT>(reinterpret_cast<u64x2*>(drow + v0), u64x2{dist_of(m0), dist_of(m1)});
      if (nh8) {
        const uint32_t h = live ? b0 | (b1 << 8) : 0u;
        const uint32_t x = h | ((uint32_t)__shfl_down(h, 1u) << 16);
        const uint32_t y = (uint32_t)__shfl_down(x, 2u);
        if ((p | 3u) < np) {  // the four pairs of this lane's group are all inside the row
          if ((lane & 3u) == 0u) store_row<NT>(reinterpret_cast<u32x2*>(nrow + v0), u32x2{x, y});
        } else if (live) {
          nrow[v0] = (uint8_t)b0;
          nrow[v0 + 1u] = (uint8_t)b1;
        }
      } else if (live) {
        nh_out(v0, b0);
        nh_out(v0 + 1u, b1);
      }
    }
  }
  if (tid == 0) {
    auto single = [&](uint32_t v) {
      uint32_t c[NBRS], m, bits;
#pragma unroll
      for (uint32_t i = 0; i < NBRS; ++i) c[i] = cands(i, lr[i] ? (uint32_t)lr[i][v] | 0xFF00u : 0xFFFFu, v);
      finish(v, c, 0u, m, bits);
      store_row<NT>(&drow[v], dist_of(m));
      nh_out(v, bits);
    };
    if (off) single(0u);
    if (off + 2u * np < V) single(off + 2u * np);
  }
}

// One workgroup per derived source at a time: its neighbours from its CSR row, their level
// rows (a missing one sends the unit to the re-run), then the sweep over the nodes.
template <bool NT>
__global__ __launch_bounds__(256) void nh_derive_kernel(DevGraph g, SolveArgs a, uint64_t cost, uint32_t* ovf_count) {
  __shared__ uint32_t s_node[kDeriveMaxNbrs];  // neighbour i when usable, else kNone
  __shared__ uint32_t s_row[kDeriveMaxNbrs];   // sid of its level row; kNone: it contributes itself only
  __shared__ uint32_t s_fail;
  const uint32_t V = g.V, tid = threadIdx.x;
  const uint32_t first = a.part[kMaxClasses + a.cls];
  const uint32_t nd = min(*a.dv.count, a.n);
  const uint32_t nb = a.nh_bytes;
  if (tid == 0) s_fail = 0;
  __syncthreads();
  for (uint32_t j = blockIdx.x; j < nd; j += gridDim.x) {
    const uint32_t k = a.n + j;  // class-local index (the re-run list's unit)
    const uint32_t sid = a.perm[first + k];
    const uint32_t src = a.sources[sid];  // < V: classified
    if (tid < 2u * kDeriveMaxNbrs) {
      const uint32_t x = a.dv.nbrs[(size_t)sid * (2u * kDeriveMaxNbrs) + tid];
      (tid < kDeriveMaxNbrs ? s_node[tid] : s_row[tid - kDeriveMaxNbrs]) = x;
      // a neighbour whose solve overflowed left no row: this unit goes to the re-run with it
      if (tid >= kDeriveMaxNbrs && x != kNone && (x >= a.n || a.dv.valid[x] != a.dv.epoch)) s_fail = 1;
    }
    __syncthreads();
    if (s_fail) {
      if (tid == 0) a.ovf_list[atomicAdd(ovf_count, 1u)] = k;
    } else {
      const size_t orow = out_row_of(a, sid);
      uint64_t* drow = a.dist + orow * V;
      uint8_t* nrow = a.nh + orow * V * nb;
      if (((uint32_t)reinterpret_cast<uintptr_t>(drow) & 15u) == 0u)  // uniform
        derive_rows<NT, true>(s_node, s_row, a.dv, src, V, cost, drow, nrow, nb);
      else
        derive_rows<NT, false>(s_node, s_row, a.dv, src, V, cost, drow, nrow, nb);
    }
    __syncthreads();  // every lane is done with this unit's s_node / s_row / s_fail
    if (tid == 0) s_fail = 0;
  }
}
}  // namespace

hipError_t launch_derive_split(const DevGraph& g, const uint32_t* sources, uint32_t n, uint32_t cls, uint32_t* member,
                               uint8_t* flags, uint32_t* nbrs, uint32_t* perm, uint32_t* part, uint32_t* count,
                               int num_cus, hipStream_t s) {
  const uint32_t grid = grid_for(n, 256u, num_cus);
  note_launch("derive_mark_kernel");
  hipLaunchKernelGGL(derive_mark_kernel, dim3(grid), dim3(256), 0, s, sources, n, g.V, member);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  note_launch("derive_classify_kernel");
  hipLaunchKernelGGL(derive_classify_kernel, dim3(grid), dim3(256), 0, s, g, sources, n, (const uint32_t*)member,
                     flags, nbrs);
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  note_launch("derive_scan_kernel");
  hipLaunchKernelGGL(derive_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, (const uint8_t*)flags, n, cls, perm, part,
                     count);
  return hipGetLastError();
}

hipError_t launch_nh_derive(const DevGraph& g, const SolveArgs& a, uint64_t cost, uint32_t* ovf_count, int num_cus,
                            hipStream_t s) {
  if (!a.dv.rows || !a.dv.count || !a.perm || !a.part || !a.dist || !a.nh || !a.nh_bytes) return hipErrorInvalidValue;
  const uint32_t grid = std::max<uint32_t>(1u, std::min<uint32_t>(a.n, (uint32_t)num_cus * 8u));
  note_launch("nh_derive_kernel");
  hipLaunchKernelGGL(nh_derive_kernel<kNtLvlRows>, dim3(grid), dim3(256), 0, s, g, a, cost, ovf_count);
  return hipGetLastError();
}

}  // namespace openr_spf
