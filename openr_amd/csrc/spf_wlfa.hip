// spf_wlfa.hip — post-failure loop-free alternates: the LFA rule of spf_lfa.hip resolved per
// failure set of a link-set what-if sweep (openr_spf_whatif_lfa*).
//
// For failure set i, source j (node s) and group k the answer is the LFA RIB entry
// (metric', nh', alt') of openr_spf_lfa_routes on the graph with every link of set i down,
// where it differs from the no-failure entry of (s, k). Nothing is re-solved here: the sweep
// over sets x (the sources, then their up neighbours that are no source: launch_lfa_rows)
// left every closure node's base rows resident and every unit's node delta in CSR form, and
// post-failure row values are "the delta entry where there is one, the base row otherwise".
//
// wlfa_base: per source, the number of live groups with exactly one next hop in nh | alt (the
//   `unprotected` count of every unit the failure does not touch).
// wlfa_mark: one thread per unit (i, j). The unit can differ from its base only if the
//   source's node delta is non-empty, an up neighbour's is, or set i holds an up link of row
//   s (the tested status of a neighbour can flip with no node moving). Affected units are
//   appended to a work list; every unit gets changed = 0, lost_backup = 0 and the source's
//   base unprotected count.
// wlfa_kernel<EMIT>: one 256-thread workgroup per affected unit (block stride over the list).
//   1. the deltas of the source (slot 0) and of every base-up neighbour (slot b + 1) go into
//      one LDS hash table keyed slot * V + node -> delta entry; every group with a member in
//      any of them is a candidate (bitmap + list through the inverse map node -> groups).
//      Every group is a candidate when s itself is in a neighbour's delta (toMe moved) or an
//      up link of s is in the set (a superset of "a tested status flipped").
//      The rule is complete: alt' bit b is a function of metric', toMe_b, dist'_b(members) and
//      the tested status only, and metric' / nh' of the source's row at the members.
//   2. a lane owns a candidate: metric' over the members, then nh' and alt' one byte at a
//      time (8 neighbours per byte, no width assumed), the neighbour slots staged in LDS a
//      slice at a time; each byte is compared with the base entry. A neighbour with an empty
//      delta under an unchanged metric keeps its base bit.
//   3. count pass: changed / unprotected / lost_backup of the unit. Emit pass: the entry is
//      allocated when the first differing field is met and the bytes before it are copied
//      from the base entry (they were equal).
// Fixed sizes and their exact fallbacks: a unit whose deltas outgrow half the
// hash slots (or whose keys do not fit 32 bits) looks values up by scanning the delta slices;
// a candidate list that overflows falls back to a scan of the bitmap; the bitmap lives in
// global scratch past OPENR_SPF_WLFA_LDS_GROUPS; neighbour slots past one slice are staged
// slice by slice. No limit changes a result.
//
// Barriers sit only in loops whose trip counts are workgroup-uniform (the work list, the
// candidate chunks, the slices); member, probe and scan loops have per-lane trip counts and
// hold neither a barrier nor a wave collective (tests/test_whatif_lfa_api.py). Malformed
// device-form input reads nothing out of bounds: set and group slices are clamped, a link id
// >= L matches no edge, a member >= V counts as unreached, a source >= V is never affected.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "spf_device.h"
#include "spf_kernels.h"

namespace openr_spf {
namespace {

constexpr unsigned long long kUnreached = ~0ull;
constexpr unsigned long long kNone = ~0ull;
constexpr uint32_t kNoRow = 0xFFFFFFFFu;
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
// ctr[] of a workgroup
enum : uint32_t { kCand = 0, kFound = 1, kAll = 2, kNewUnp = 3, kOldUnp = 4, kEntries = 5, kLost = 6, kCtrs = 8 };

struct Range {
  uint32_t b, e;
};
__device__ __forceinline__ Range clamped(const uint32_t* ptr, uint32_t k, uint32_t n) {
  const uint32_t e = min(ptr[k + 1], n);
  return {min(ptr[k], e), e};
}

__device__ __forceinline__ bool in_set(const WlfaPass& p, Range sr, uint32_t link) {
  for (uint32_t t = sr.b; t < sr.e; ++t)
    if (p.set_links[t] == link) return true;
  return false;
}

// 0: not live (no member reached or no next hop), 1: live with one next hop in nh | alt, 2: more
__device__ __forceinline__ uint32_t route_class(unsigned long long metric, const uint8_t* nh, const uint8_t* alt,
                                                uint32_t nb) {
  uint32_t pc = 0, any = 0;
  for (uint32_t q = 0; q < nb; ++q) {
    any |= nh[q];
    pc += (uint32_t)__popc((uint32_t)(nh[q] | alt[q]));
  }
  if (metric == kUnreached || !any) return 0u;
  return pc == 1u ? 1u : 2u;
}

__global__ __launch_bounds__(256) void wlfa_base(WlfaPass p) {
  __shared__ uint32_t cnt;
  for (uint32_t j = blockIdx.x; j < p.n_src; j += gridDim.x) {
    if (threadIdx.x == 0) cnt = 0u;
    __syncthreads();
    uint32_t c = 0;
    for (uint32_t k = threadIdx.x; k < p.G; k += 256u) {
      const size_t bi = (size_t)j * p.G + k;
      c += route_class(p.bmetric[bi], p.bmnh + bi * p.nb, p.balt + bi * p.nb, p.nb) == 1u ? 1u : 0u;
    }
    if (c) atomicAdd(&cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) p.bunprot[j] = cnt;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void wlfa_mark(WlfaPass p) {
  const size_t units = (size_t)p.n_sets * p.n_src;
  for (size_t u = (size_t)blockIdx.x * 256u + threadIdx.x; u < units; u += (size_t)gridDim.x * 256u) {
    const uint32_t i = (uint32_t)(u / p.n_src), j = (uint32_t)(u % p.n_src);
    const uint32_t s = p.sources[j];
    bool aff = false;
    if (s < p.V) {
      const size_t ub = (size_t)i * p.n_rows;
      aff = p.nchanged[ub + j] != 0u;
      const uint2 r = p.row2[s];
      const Range sr = clamped(p.set_ptr, i, p.n_set_links);
      for (uint32_t e = r.x; e < r.y && !aff; ++e) {
        const uint32_t v = p.adj[e];
        if (v >= p.V) continue;  // down
        const uint32_t ri = p.rowidx[v];
        aff = (ri < p.n_rows && p.nchanged[ub + ri] != 0u) || in_set(p, sr, p.lid[e]);
      }
    }
    p.changed[u] = 0u;
    if (p.lost) p.lost[u] = 0u;
    if (p.unprot) p.unprot[u] = p.bunprot[j];
    if (aff) p.alist[atomicAdd(p.acount, 1u)] = (uint32_t)u;
  }
}

// The unit's staged deltas: slot * V + node -> entry (offset from the set's first entry).
struct Deltas {
  const uint32_t* hk;
  const uint32_t* hv;
  const uint32_t* nnode;
  unsigned long long blk0;
  uint32_t H, shift, V;
  bool hash_on;
  // entry of (slot, v) among the slot's delta entries [e0, e0 + len), or kNone
  __device__ __forceinline__ unsigned long long find(uint32_t slot, uint32_t v, unsigned long long e0,
                                                     uint32_t len) const {
    if (!len) return kNone;
    if (hash_on) {
      const uint32_t key = slot * V + v;
      uint32_t h = (key * 0x9E3779B1u) >> shift;
      for (;;) {
        const uint32_t kk = hk[h];
        if (kk == key) return blk0 + hv[h];
        if (kk == kEmpty) return kNone;
        h = (h + 1u) & (H - 1u);
      }
    }
    for (unsigned long long t = e0; t < e0 + len; ++t)
      if (nnode[t] == v) return t;
    return kNone;
  }
};

__device__ __forceinline__ void hash_put(uint32_t* hk, uint32_t* hv, uint32_t H, uint32_t shift, uint32_t key,
                                         uint32_t val) {
  uint32_t h = (key * 0x9E3779B1u) >> shift;
  for (;;) {  // the table is at most half full: a free slot exists
    const uint32_t prev = atomicCAS(&hk[h], kEmpty, key);
    if (prev == kEmpty || prev == key) {
      hv[h] = val;
      return;
    }
    h = (h + 1u) & (H - 1u);
  }
}

template <bool EMIT>
__global__ __launch_bounds__(256) void wlfa_kernel(WlfaPass p) {
  extern __shared__ unsigned long long wlfa_lds[];
  const uint32_t tid = threadIdx.x, SL = p.slots, H = p.hash_slots;
  unsigned long long* l_e0 = wlfa_lds;
  unsigned long long* l_tome = l_e0 + SL;
  uint32_t* l_len = reinterpret_cast<uint32_t*>(l_tome + SL);
  uint32_t* l_row = l_len + SL;
  uint32_t* l_tst = l_row + SL;
  uint32_t* ctr = l_tst + SL;
  uint32_t* cand = ctr + kCtrs;
  uint32_t* hk = cand + p.cand_cap;
  uint32_t* hv = hk + H;
  uint32_t* l_bm = hv + H;
  const uint32_t bmw = (p.G + 31u) / 32u;
  uint32_t* bm = p.bm_lds ? l_bm : p.g_bm + (size_t)blockIdx.x * bmw;
  const uint32_t n_aff = *p.acount;
  for (uint32_t a = blockIdx.x; a < n_aff; a += gridDim.x) {
    const size_t u = p.alist[a];
    if (EMIT && p.optr[u] == p.optr[u + 1]) continue;
    const uint32_t i = (uint32_t)(u / p.n_src), j = (uint32_t)(u % p.n_src);
    const uint32_t s = p.sources[j];  // < V: wlfa_mark lists no other unit
    const uint2 r = p.row2[s];
    const uint32_t nbits = r.y - r.x;  // >= the distinct degree; table entries past it are kNoRow
    const size_t ub = (size_t)i * p.n_rows;
    const Range sr = clamped(p.set_ptr, i, p.n_set_links);
    const unsigned long long blk0 = p.nptr[ub];
    const unsigned long long s0 = p.nptr[ub + j];
    const uint32_t slen = (uint32_t)min(p.nptr[ub + j + 1] - s0, 0xFFFFFFFFull);
    // 0. reset
    for (uint32_t x = tid; x < H; x += 256u) hk[x] = kEmpty;
    for (uint32_t x = tid; x < bmw; x += 256u) bm[x] = 0u;
    if (tid < kCtrs) ctr[tid] = 0u;
    __syncthreads();
    // 1. entries of the neighbours' deltas (the hash holds them only when it stays half empty)
    const bool key_fits = ((unsigned long long)nbits + 1ull) * p.V < 0xFFFFFFFFull &&
                          p.nptr[ub + p.n_rows] - blk0 < 0xFFFFFFFFull;
    for (uint32_t b = tid; key_fits && b < nbits; b += 256u) {  // key_fits: the sum stays below 2^32
      const uint32_t ri = p.trow[r.x + b];
      if (ri >= p.n_rows) continue;
      const uint32_t len = (uint32_t)(p.nptr[ub + ri + 1] - p.nptr[ub + ri]);
      if (len) atomicAdd(&ctr[kEntries], len);
    }
    __syncthreads();
    const bool hash_on = H != 0u && key_fits && 2ull * ((unsigned long long)ctr[kEntries] + slen) <= H;
    // 2. stage the deltas, mark the candidates
    for (uint32_t slot = 0; slot <= nbits; ++slot) {
      unsigned long long e0 = s0, e1 = s0 + slen;
      if (slot) {
        const uint32_t ri = p.trow[r.x + slot - 1u];
        if (ri >= p.n_rows) continue;
        e0 = p.nptr[ub + ri];
        e1 = p.nptr[ub + ri + 1];
      }
      for (unsigned long long t = e0 + tid; t < e1; t += 256u) {
        const uint32_t v = p.nnode[t];
        if (v >= p.V) continue;
        if (slot && v == s) ctr[kAll] = 1u;  // toMe of this neighbour moved
        if (hash_on) hash_put(hk, hv, H, p.hash_shift, slot * p.V + v, (uint32_t)(t - blk0));
        for (unsigned long long x = p.iptr[v]; x < p.iptr[v + 1]; ++x) {
          const uint32_t k = p.inv[x];
          if (k >= p.G) continue;
          const uint32_t bit = 1u << (k & 31u);
          if (atomicOr(&bm[k >> 5], bit) & bit) continue;
          const uint32_t c = atomicAdd(&ctr[kCand], 1u);
          if (c < p.cand_cap) cand[c] = k;
        }
      }
    }
    // an up link of s in the set: a tested status may flip, every group is a candidate
    for (uint32_t e = r.x + tid; e < r.y; e += 256u)
      if (p.adj[e] < p.V && in_set(p, sr, p.lid[e])) ctr[kAll] = 1u;
    __syncthreads();
    // 3. the candidates, 256 at a time
    const Deltas dl{hk, hv, p.nnode, blk0, H, p.hash_shift, p.V, hash_on};
    const bool all = ctr[kAll] != 0u;
    const bool use_list = !all && ctr[kCand] <= p.cand_cap;
    const uint32_t N = use_list ? ctr[kCand] : p.G;
    const unsigned long long* srow = p.bdist + (size_t)j * p.V;
    const uint8_t* shrow = p.bnh + (size_t)j * p.V * p.nb;
    const uint32_t nbytes = min(p.nb, (nbits + 7u) >> 3);
    const uint32_t nslots = nbytes * 8u;
    const unsigned long long oend = EMIT ? p.optr[u + 1] : 0ull;
    for (uint32_t c0 = 0; c0 < N; c0 += 256u) {
      const uint32_t idx = c0 + tid;
      bool act = idx < N;
      uint32_t k = 0;
      if (act) {
        k = use_list ? cand[idx] : idx;
        if (!use_list && !all) act = ((bm[k >> 5] >> (k & 31u)) & 1u) != 0u;
      }
      const size_t bi = (size_t)j * p.G + k;
      Range gr{0u, 0u};
      unsigned long long mn = kUnreached, bmet = kUnreached;
      if (act) {
        gr = clamped(p.gptr, k, p.M);
        bmet = p.bmetric[bi];
        for (uint32_t m = gr.b; m < gr.e; ++m) {
          const uint32_t v = p.gnodes[m];
          if (v >= p.V) continue;
          const unsigned long long t = dl.find(0u, v, s0, slen);
          mn = min(mn, t != kNone ? p.ndist[t] : srow[v]);
        }
      }
      const bool same_metric = mn == bmet;
      bool diff = act && !same_metric;
      bool have = false;  // emit pass: the entry is allocated
      unsigned long long o = 0;
      if (EMIT && diff) {
        have = true;
        o = p.optr[u] + atomicAdd(&ctr[kFound], 1u);
      }
      uint32_t pc = 0, nhany = 0;
      for (uint32_t b0 = 0; b0 < nslots; b0 += SL) {
        if (c0 == 0u || nslots > SL) {  // one slice: staged once per unit
          __syncthreads();  // the previous slice is consumed
          for (uint32_t x = tid; x < SL; x += 256u) {
            const uint32_t b = b0 + x;
            uint32_t ri = b < nbits ? p.trow[r.x + b] : kNoRow;
            if (ri >= p.n_rows) ri = kNoRow;
            unsigned long long e0 = 0, tome = 0;
            uint32_t len = 0;
            if (ri != kNoRow) {
              e0 = p.nptr[ub + ri];
              len = (uint32_t)min(p.nptr[ub + ri + 1] - e0, 0xFFFFFFFFull);
              tome = p.ttome[r.x + b];
              const unsigned long long t = dl.find(b + 1u, s, e0, len);
              if (t != kNone) tome = p.ndist[t];
            }
            l_row[x] = ri;
            l_e0[x] = e0;
            l_len[x] = len;
            l_tome[x] = tome;
            l_tst[x] = 0u;
          }
          __syncthreads();
          // tested after the failure: an up link s-n that is not in the set
          for (uint32_t e = r.x + tid; e < r.y; e += 256u) {
            const uint32_t sl = p.nbr[e];
            if (p.adj[e] < p.V && sl >= b0 && sl - b0 < SL && !in_set(p, sr, p.lid[e])) l_tst[sl - b0] = 1u;
          }
          __syncthreads();
        }
        if (!act) continue;
        const uint32_t sn = min(SL, nslots - b0);
        for (uint32_t j0 = 0; j0 < sn; j0 += 8u) {  // SL is a multiple of 8
          const uint32_t q = (b0 + j0) >> 3;
          const uint32_t bn = p.bmnh[bi * p.nb + q], ba = p.balt[bi * p.nb + q];
          uint32_t nhq = 0, aq = 0;
          if (mn != kUnreached) {
            for (uint32_t m = gr.b; m < gr.e; ++m) {
              const uint32_t v = p.gnodes[m];
              if (v >= p.V) continue;
              const unsigned long long t = dl.find(0u, v, s0, slen);
              if (t != kNone) {
                if (p.ndist[t] == mn) nhq |= p.nnh[t * p.nb + q];
              } else if (srow[v] == mn) {
                nhq |= shrow[(size_t)v * p.nb + q];
              }
            }
            for (uint32_t t8 = 0; t8 < 8u; ++t8) {
              const uint32_t x = j0 + t8, ri = l_row[x];
              if (ri == kNoRow || !l_tst[x]) continue;
              const uint32_t len = l_len[x];
              if (same_metric && !len) {  // nothing this bit depends on moved
                aq |= ba & (1u << t8);
                continue;
              }
              const unsigned long long e0 = l_e0[x], bound = mn + l_tome[x];
              const unsigned long long* nrow = p.bdist + (size_t)ri * p.V;
              for (uint32_t m = gr.b; m < gr.e; ++m) {
                const uint32_t v = p.gnodes[m];
                if (v >= p.V) continue;
                const unsigned long long t = dl.find(b0 + x + 1u, v, e0, len);
                if ((t != kNone ? p.ndist[t] : nrow[v]) < bound) {  // an unreached member never qualifies
                  aq |= 1u << t8;
                  break;
                }
              }
            }
          }
          pc += (uint32_t)__popc(nhq | aq);
          nhany |= nhq;
          const bool dq = nhq != bn || aq != ba;
          diff |= dq;
          if (!EMIT) continue;
          if (dq && !have) {
            have = true;
            o = p.optr[u] + atomicAdd(&ctr[kFound], 1u);
            if (o < oend)
              for (uint32_t q2 = 0; q2 < q; ++q2) {  // the bytes before the first difference equal the base's
                p.onh[o * p.onb + q2] = p.bmnh[bi * p.nb + q2];
                p.oalt[o * p.onb + q2] = p.balt[bi * p.nb + q2];
              }
          }
          if (have && o < oend && q < p.onb) {
            p.onh[o * p.onb + q] = (uint8_t)nhq;
            p.oalt[o * p.onb + q] = (uint8_t)aq;
          }
        }
      }
      if (!act || !diff) continue;
      if (EMIT) {
        if (o >= oend) continue;
        p.ogroup[o] = k;
        p.ometric[o] = mn;
        for (uint32_t q = nbytes; q < p.onb; ++q) {
          p.onh[o * p.onb + q] = 0;
          p.oalt[o * p.onb + q] = 0;
        }
      } else {
        atomicAdd(&ctr[kFound], 1u);
        const uint32_t now = (mn == kUnreached || !nhany) ? 0u : (pc == 1u ? 1u : 2u);
        const uint32_t was = route_class(bmet, p.bmnh + bi * p.nb, p.balt + bi * p.nb, p.nb);
        if (now == 1u) atomicAdd(&ctr[kNewUnp], 1u);
        if (was == 1u) atomicAdd(&ctr[kOldUnp], 1u);
        if (was == 2u && now == 1u) atomicAdd(&ctr[kLost], 1u);
      }
    }
    __syncthreads();
    if (!EMIT && tid == 0u) {
      p.changed[u] = ctr[kFound];
      if (p.unprot) p.unprot[u] = p.bunprot[j] + ctr[kNewUnp] - ctr[kOldUnp];
      if (p.lost) p.lost[u] = ctr[kLost];
    }
    __syncthreads();
  }
}

uint32_t knob(const char* name, uint32_t dflt) {
  const char* e = std::getenv(name);
  return e ? (uint32_t)std::strtoul(e, nullptr, 10) : dflt;
}

}  // namespace

WlfaLayout whatif_lfa_layout(uint32_t G, size_t units, int num_cus) {
  WlfaLayout l;
  // OPENR_SPF_WLFA_HASH_SLOTS (a power of two, 0: every lookup scans the delta),
  // OPENR_SPF_WLFA_CAND_CAP, OPENR_SPF_WLFA_LDS_GROUPS (the bitmap in LDS up to that many
  // groups), OPENR_SPF_WLFA_SLOTS (neighbour slots staged at a time). Defaults: 22 KiB of LDS
  // (55 KiB with every knob at its maximum).
  uint32_t h = std::min(knob("OPENR_SPF_WLFA_HASH_SLOTS", 2048u), 4096u);
  uint32_t pw = 0;
  while ((2u << pw) <= h) ++pw;  // the largest power of two <= h
  l.hash_slots = h < 16u ? 0u : 1u << pw;
  l.hash_shift = l.hash_slots ? 32u - pw : 0u;
  l.cand_cap = std::min(knob("OPENR_SPF_WLFA_CAND_CAP", 1024u), 1024u);
  l.bm_lds = G <= std::min(knob("OPENR_SPF_WLFA_LDS_GROUPS", 32768u), 32768u);
  l.slots = (std::max(8u, std::min(knob("OPENR_SPF_WLFA_SLOTS", 64u), 512u)) + 7u) & ~7u;
  const uint32_t bmw = (G + 31u) / 32u;
  l.lds_bytes = 28u * l.slots + 4u * (kCtrs + l.cand_cap + 2u * l.hash_slots + (l.bm_lds ? bmw : 0u));
  l.grid = blocks_for((uint32_t)std::min<size_t>(units, 0xFFFFFFFFu), l.lds_bytes, num_cus, 256u);
  l.bm_words = l.bm_lds ? 0u : (size_t)l.grid * bmw;
  return l;
}

hipError_t launch_wlfa_mark(const WlfaPass& p, int num_cus, hipStream_t s) {
  const size_t units = (size_t)p.n_sets * p.n_src;
  if (!units) return hipSuccess;
  hipError_t err = hipMemsetAsync(p.acount, 0, sizeof(uint32_t), s);
  if (err != hipSuccess) return err;
  const uint32_t cap = (uint32_t)num_cus * 8u;
  hipLaunchKernelGGL(wlfa_base, dim3(std::max(1u, std::min(p.n_src, cap))), dim3(256), 0, s, p);
  hipLaunchKernelGGL(wlfa_mark, dim3((uint32_t)std::max<size_t>(1, std::min<size_t>((units + 255u) / 256u, cap))),
                     dim3(256), 0, s, p);
  note_launch("wlfa_mark");
  return hipGetLastError();
}

hipError_t launch_wlfa(const WlfaPass& pass, const WlfaLayout& l, bool emit, hipStream_t s) {
  if (!pass.n_sets || !pass.n_src || !pass.G) return hipSuccess;
  WlfaPass p = pass;
  p.hash_slots = l.hash_slots;
  p.hash_shift = l.hash_shift;
  p.cand_cap = l.cand_cap;
  p.bm_lds = l.bm_lds;
  p.slots = l.slots;
  if (emit)
    hipLaunchKernelGGL(wlfa_kernel<true>, dim3(l.grid), dim3(256), l.lds_bytes, s, p);
  else
    hipLaunchKernelGGL(wlfa_kernel<false>, dim3(l.grid), dim3(256), l.lds_bytes, s, p);
  note_launch(emit ? "wlfa_emit" : "wlfa_count");
  return hipGetLastError();
}

}  // namespace openr_spf
