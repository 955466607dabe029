// spf_elfa.hip — loop-free alternates under drain, metric, restore and maintenance events
// (openr_spf_whatif_drain_lfa*, _metric_lfa*, _restore_lfa*, _maint_lfa*): the LFA rule of spf_lfa.hip
// resolved per event of an event sweep, as spf_wlfa.hip resolves it per failure set.
//
// For event i, source j (node s) and group k the answer is the LFA RIB entry (metric', nh',
// alt') of openr_spf_lfa_routes on the graph patched by event i, where it differs from the
// no-event entry of (s, k). The reference's LFA loop (getNextHopsWithMetric,
// Decision.cpp:1169-1204) walks linksFromNode(me), skips a link only when it is not up
// (:1171-1174), never looks at a neighbour's overload bit, and takes the neighbour's rows
// from the SPF *from* the neighbour, in which the neighbour expands because it is the source.
// Unit (i, row n) of the family's node sweep is that row already ("a drained node that is the
// unit's source still expands"), so nothing is re-solved here: the sweep over events x closure
// left every closure node's base rows resident and every unit's node delta in CSR form, and a
// post-event row value is "the delta entry where there is one, the base row otherwise".
//
// What an event does to the *tested* status of a neighbour n of s (the Event policies below):
//   drain    n is tested iff some link s-n is up and not in K_i. The nodes N_i change no
//            tested status: a drained neighbour is tested. A status can only be lost.
//   metric   tested status never changes.
//   restore  n is tested iff some link s-n is up or is an effective link of K_i: down today,
//            and accepted by the restore sweep's own test (restore::Slices::comes_up, shared
//            with restore_filter / restore_repair). A status can only be gained, and the
//            closure holds every neighbour of a source for that reason (launch_elfa_rows,
//            launch_elfa_table: the table of neighbours with a closure row).
//   maintenance (kElfaMaint, openr_spf_whatif_maint_lfa*): the drain policy, unchanged. The
//            loop never reads the metric of a link s-n, so a raise changes no tested status: a
//            raise on s -> n shows in the source's delta, a raise on n -> s as node s in the
//            delta of unit (i, n) (toMe moved), both rows of the maintenance sweep. The launchers
//            send the family to the drain instantiations; no kernel is added for it.
//
// elfa_base: per source, the base `unprotected` count (as wlfa_base).
// elfa_mark<FAM>: a thread per unit. A unit can differ from its base only if the source's
//   node delta is non-empty, a closure neighbour's is, or a tested status can flip (drain: an
//   up link of s in K_i; restore: a down link of s that is an effective link of K_i). The
//   affected units of a workgroup are counted in LDS and appended with one global atomic per
//   workgroup and round.
// elfa_kernel<FAM, EMIT>: one 256-thread workgroup per affected unit, the structure of
//   wlfa_kernel: the deltas of the source (slot 0) and of every neighbour with a closure row
//   (slot b + 1) in one LDS hash, candidates through the inverse map, every group a candidate
//   when s is in a neighbour's delta (toMe moved) or a tested status can flip; a lane owns a
//   candidate and builds nh' and alt' a byte at a time against the base entry. The shortcut
//   "a neighbour with an empty delta under an unchanged metric keeps its base bit" holds only
//   for a neighbour that was tested at the base: one that a restore makes tested has a base
//   bit of 0 because it was never tested, and is evaluated over the members.
// The fixed sizes, their knobs and their exact fallbacks are whatif_lfa_layout's.
//
// Barriers sit only in loops whose trip counts are workgroup-uniform (the work list, the
// candidate chunks, the slices, the mark pass's rounds); member, probe, scan, set and event
// slice loops have per-lane trip counts and hold neither a barrier nor a wave collective
// (tests/test_event_lfa_api.py). Malformed device-form input reads nothing out of bounds:
// every slice is clamped, a link id >= L matches no edge, a member >= V counts as unreached,
// a source >= V is never affected.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "spf_device.h"
#include "spf_kernels.h"
#include "spf_restore_event.h"

namespace openr_spf {
namespace {

constexpr unsigned long long kUnreached = ~0ull;
constexpr unsigned long long kNone = ~0ull;
constexpr uint32_t kNoRow = 0xFFFFFFFFu;
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kColBits = ~(kEdgeDown | kNodeSink);
// l_tst[] of a staged neighbour
constexpr uint32_t kTested = 1u, kWasTested = 2u;
// ctr[] of a workgroup (whatif_lfa_layout reserves 8 words)
enum : uint32_t { kCand = 0, kFound = 1, kAll = 2, kNewUnp = 3, kOldUnp = 4, kEntries = 5, kLost = 6, kCtrs = 8 };

struct Range {
  uint32_t b, e;
};
__device__ __forceinline__ Range clamped(const uint32_t* ptr, uint32_t k, uint32_t n) {
  const uint32_t e = min(ptr[k + 1], n);
  return {min(ptr[k], e), e};
}

// What event i does to the tested status of the neighbour behind edge e of row s.
template <int FAM>
struct Event;

template <>
struct Event<kElfaDrain> {
  const WlfaPass& p;
  Range sr{0u, 0u};
  __device__ __forceinline__ Event(const DevGraph&, const ElfaPass& ep) : p(ep.w) {}
  __device__ __forceinline__ void begin(uint32_t i, uint32_t) {
    sr = p.set_ptr ? clamped(p.set_ptr, i, p.n_set_links) : Range{0u, 0u};
  }
  __device__ __forceinline__ bool drained(uint32_t e) const {
    const uint32_t link = p.lid[e];
    for (uint32_t t = sr.b; t < sr.e; ++t)
      if (p.set_links[t] == link) return true;
    return false;
  }
  __device__ __forceinline__ bool tested(uint32_t e) const { return p.adj[e] < p.V && !drained(e); }
  __device__ __forceinline__ bool flips(uint32_t e) const { return p.adj[e] < p.V && drained(e); }
};

template <>
struct Event<kElfaMetric> {
  const WlfaPass& p;
  __device__ __forceinline__ Event(const DevGraph&, const ElfaPass& ep) : p(ep.w) {}
  __device__ __forceinline__ void begin(uint32_t, uint32_t) {}
  __device__ __forceinline__ bool tested(uint32_t e) const { return p.adj[e] < p.V; }
  __device__ __forceinline__ bool flips(uint32_t) const { return false; }
};

template <>
struct Event<kElfaRestore> {
  const WlfaPass& p;
  restore::Slices sl;
  __device__ __forceinline__ Event(const DevGraph& g, const ElfaPass& ep) : p(ep.w), sl(g, ep.ev) {}
  __device__ __forceinline__ void begin(uint32_t i, uint32_t s) { sl.begin(i, s); }
  // a down link of K_i that the restore sweep puts back
  __device__ __forceinline__ bool flips(uint32_t e) const {
    if (p.adj[e] < p.V) return false;
    const uint32_t link = p.lid[e];
    return sl.link_listed(link) && sl.comes_up(link);
  }
  __device__ __forceinline__ bool tested(uint32_t e) const { return p.adj[e] < p.V || flips(e); }
};

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

__global__ __launch_bounds__(256) void elfa_base(WlfaPass p) {
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

// The rounds of a workgroup are uniform (every thread runs `rounds` of them, a thread past the
// last unit idles), so the barriers around the LDS count are reached by all.
template <int FAM>
__global__ __launch_bounds__(256) void elfa_mark(const DevGraph g, const ElfaPass ep) {
  __shared__ uint32_t l_cnt, l_base;
  const WlfaPass& p = ep.w;
  Event<FAM> ev(g, ep);
  const size_t units = (size_t)p.n_sets * p.n_src;
  const size_t stride = (size_t)gridDim.x * 256u;
  const size_t rounds = (units + stride - 1u) / stride;
  for (size_t rd = 0; rd < rounds; ++rd) {
    const size_t u = rd * stride + (size_t)blockIdx.x * 256u + threadIdx.x;
    if (threadIdx.x == 0) l_cnt = 0u;
    __syncthreads();
    bool aff = false;
    if (u < units) {
      const uint32_t i = (uint32_t)(u / p.n_src), j = (uint32_t)(u % p.n_src);
      const uint32_t s = p.sources[j];
      if (s < p.V && !ep.idle) {
        const size_t ub = (size_t)i * p.n_rows;
        aff = p.nchanged[ub + j] != 0u;
        const uint2 r = p.row2[s];
        ev.begin(i, s);
        for (uint32_t e = r.x; e < r.y && !aff; ++e) {
          const uint32_t a = p.adj[e];
          if (FAM != kElfaRestore && a >= p.V) continue;  // down: no closure row
          const uint32_t v = a & kColBits;
          const uint32_t ri = v < p.V ? p.rowidx[v] : kNoRow;
          aff = (ri < p.n_rows && p.nchanged[ub + ri] != 0u) || ev.flips(e);
        }
      }
      p.changed[u] = 0u;
      if (p.lost) p.lost[u] = 0u;
      if (p.unprot) p.unprot[u] = p.bunprot[j];
    }
    uint32_t rank = 0;
    if (aff) rank = atomicAdd(&l_cnt, 1u);
    __syncthreads();
    if (threadIdx.x == 0 && l_cnt) l_base = atomicAdd(p.acount, l_cnt);
    __syncthreads();
    if (aff) p.alist[l_base + rank] = (uint32_t)u;
  }
}

// The unit's staged deltas: slot * V + node -> entry (offset from the event's first entry).
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

template <int FAM, bool EMIT>
__global__ __launch_bounds__(256) void elfa_kernel(const DevGraph g, const ElfaPass ep) {
  extern __shared__ unsigned long long elfa_lds[];
  const WlfaPass& p = ep.w;
  Event<FAM> ev(g, ep);
  const uint32_t tid = threadIdx.x, SL = p.slots, H = p.hash_slots;
  unsigned long long* l_e0 = elfa_lds;
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
    const uint32_t s = p.sources[j];  // < V: elfa_mark lists no other unit
    const uint2 r = p.row2[s];
    const uint32_t nbits = r.y - r.x;  // >= the distinct degree; table entries past it are kNoRow
    const size_t ub = (size_t)i * p.n_rows;
    ev.begin(i, s);
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
    // a tested status may flip: every group is a candidate
    for (uint32_t e = r.x + tid; e < r.y; e += 256u)
      if (ev.flips(e)) ctr[kAll] = 1u;
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
          // tested after the event, and whether it was tested before it (an up link s-n)
          for (uint32_t e = r.x + tid; e < r.y; e += 256u) {
            const uint32_t sl = p.nbr[e];
            if (sl >= b0 && sl - b0 < SL && ev.tested(e))
              atomicOr(&l_tst[sl - b0], p.adj[e] < p.V ? (kTested | kWasTested) : kTested);
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
              const uint32_t x = j0 + t8, ri = l_row[x], tst = l_tst[x];
              if (ri == kNoRow || !(tst & kTested)) continue;
              const uint32_t len = l_len[x];
              // nothing this bit depends on moved; a neighbour that was not tested at the
              // base has no base bit to keep
              if (same_metric && !len && (tst & kWasTested)) {
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

// One workgroup per source: its own bit in srcbm, every neighbour's bit in need.
__global__ __launch_bounds__(256) void elfa_rows_mark(const uint32_t* sources, uint32_t n, uint32_t V,
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
      const uint32_t v = adj[e] & kColBits;
      if (v < V) atomicOr(&need[v >> 5], 1u << (v & 31u));
    }
  }
}

__global__ __launch_bounds__(256) void elfa_rows_count(uint32_t words, const uint32_t* need, const uint32_t* srcbm,
                                                       uint32_t* cnt) {
  for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w < words; w += gridDim.x * 256u)
    cnt[w] = (uint32_t)__popc(need[w] & ~srcbm[w]);
}

// list[wptr[w] ..) = the nodes of word w that are needed and are no source, ascending
__global__ __launch_bounds__(256) void elfa_rows_compact(uint32_t words, uint32_t V, const uint32_t* need,
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

// One workgroup per source: the table row of its distinct neighbours, down links included
// (trow starts at kNoRow). Parallel links of one neighbour write equal values.
__global__ __launch_bounds__(256) void elfa_nbr_table(const uint32_t* sources, uint32_t n, uint32_t V,
                                                      const uint2* row2, const uint32_t* adj, const uint16_t* nbr,
                                                      const uint32_t* rowidx, const unsigned long long* dist,
                                                      uint32_t* trow, unsigned long long* ttome) {
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t s = sources[i];
    if (s >= V) continue;
    const uint2 r = row2[s];
    for (uint32_t e = r.x + threadIdx.x; e < r.y; e += 256u) {
      const uint32_t v = adj[e] & kColBits;
      const uint32_t slot = r.x + nbr[e];
      if (v >= V || slot >= r.y) continue;
      const uint32_t ri = rowidx[v];
      trow[slot] = ri;
      ttome[slot] = dist[(size_t)ri * V + s];
    }
  }
}

uint32_t capped_grid(uint64_t blocks, int num_cus, uint32_t per_cu) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)num_cus * per_cu));
}

}  // namespace

hipError_t launch_elfa_rows(const DevGraph& g, const uint32_t* sources, uint32_t n, uint32_t* need, uint32_t* srcbm,
                            uint32_t* cnt, unsigned long long* tsum, unsigned long long* wptr, uint32_t* list,
                            uint32_t* rowidx, int num_cus, hipStream_t s) {
  const uint32_t words = (g.V + 31u) / 32u;
  hipError_t err = hipMemsetAsync(need, 0, (size_t)words * sizeof(uint32_t), s);
  if (err == hipSuccess) err = hipMemsetAsync(srcbm, 0, (size_t)words * sizeof(uint32_t), s);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(elfa_rows_mark, dim3(capped_grid(n, num_cus, 16u)), dim3(256), 0, s, sources, n, g.V, g.row2,
                     g.adj, need, srcbm, rowidx);
  const uint32_t wg = capped_grid((words + 255u) / 256u, num_cus, 8u);
  hipLaunchKernelGGL(elfa_rows_count, dim3(wg), dim3(256), 0, s, words, need, srcbm, cnt);
  if ((err = launch_delta_scan(cnt, words, tsum, wptr, s)) != hipSuccess) return err;
  hipLaunchKernelGGL(elfa_rows_compact, dim3(wg), dim3(256), 0, s, words, g.V, need, srcbm, wptr, n, list, rowidx);
  note_launch("elfa_rows");
  return hipGetLastError();
}

hipError_t launch_elfa_table(const DevGraph& g, const uint32_t* sources, uint32_t n, const uint32_t* rowidx,
                             const uint64_t* dist, uint32_t* trow, unsigned long long* ttome, int num_cus,
                             hipStream_t s) {
  hipError_t err = hipMemsetAsync(trow, 0xFF, std::max<size_t>(g.E, 1) * sizeof(uint32_t), s);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(elfa_nbr_table, dim3(capped_grid(n, num_cus, 16u)), dim3(256), 0, s, sources, n, g.V, g.row2,
                     g.adj, g.nbr, rowidx, reinterpret_cast<const unsigned long long*>(dist), trow, ttome);
  return hipGetLastError();
}

hipError_t launch_elfa_mark(const DevGraph& g, const ElfaPass& p, int fam, int num_cus, hipStream_t s) {
  const size_t units = (size_t)p.w.n_sets * p.w.n_src;
  if (!units) return hipSuccess;
  hipError_t err = hipMemsetAsync(p.w.acount, 0, sizeof(uint32_t), s);
  if (err != hipSuccess) return err;
  const uint32_t cap = (uint32_t)num_cus * 8u;
  hipLaunchKernelGGL(elfa_base, dim3(std::max(1u, std::min(p.w.n_src, cap))), dim3(256), 0, s, p.w);
  const dim3 grid(capped_grid((units + 255u) / 256u, num_cus, 8u));
  if (fam == kElfaDrain || fam == kElfaMaint)  // a maintenance event's N_i and K_i are a drain's
    hipLaunchKernelGGL(elfa_mark<kElfaDrain>, grid, dim3(256), 0, s, g, p);
  else if (fam == kElfaMetric)
    hipLaunchKernelGGL(elfa_mark<kElfaMetric>, grid, dim3(256), 0, s, g, p);
  else if (fam == kElfaRestore)
    hipLaunchKernelGGL(elfa_mark<kElfaRestore>, grid, dim3(256), 0, s, g, p);
  else
    return hipErrorInvalidValue;
  note_launch("elfa_mark");
  return hipGetLastError();
}

hipError_t launch_elfa(const DevGraph& g, const ElfaPass& pass, const WlfaLayout& l, int fam, bool emit,
                       hipStream_t s) {
  if (!pass.w.n_sets || !pass.w.n_src || !pass.w.G) return hipSuccess;
  ElfaPass p = pass;
  p.w.hash_slots = l.hash_slots;
  p.w.hash_shift = l.hash_shift;
  p.w.cand_cap = l.cand_cap;
  p.w.bm_lds = l.bm_lds;
  p.w.slots = l.slots;
  const dim3 grid(l.grid), block(256);
#define OPENR_ELFA_LAUNCH(F)                                                             \
  do {                                                                                   \
    if (emit)                                                                            \
      hipLaunchKernelGGL((elfa_kernel<F, true>), grid, block, l.lds_bytes, s, g, p);     \
    else                                                                                 \
      hipLaunchKernelGGL((elfa_kernel<F, false>), grid, block, l.lds_bytes, s, g, p);    \
  } while (0)
  bool known = true;
  if (fam == kElfaDrain || fam == kElfaMaint)  // a maintenance event's N_i and K_i are a drain's
    OPENR_ELFA_LAUNCH(kElfaDrain);
  else if (fam == kElfaMetric)
    OPENR_ELFA_LAUNCH(kElfaMetric);
  else if (fam == kElfaRestore)
    OPENR_ELFA_LAUNCH(kElfaRestore);
  else
    known = false;
#undef OPENR_ELFA_LAUNCH
  if (!known) return hipErrorInvalidValue;
  note_launch(emit ? "elfa_emit" : "elfa_count");
  return hipGetLastError();
}

}  // namespace openr_spf
