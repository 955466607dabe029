// spf_capi.hip — host side of the C-ABI declared in include/openr_spf.h.
//
// Owns the per-device CSR replicas (one DevGraph per GPU of the context), picks the
// kernel for a solve (uniform-cost BFS or settle-safe buckets), splits a batch of
// sources across the context's devices and moves results. There is deliberately no
// CPU path: every solve runs on the GPU or fails with an error code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/openr_spf.h"
#include "spf_kernels.h"

using namespace openr_spf;

namespace {

thread_local std::string g_last_error;
thread_local std::string g_launch_trace;  // "kernel;kernel;..." of the last solve call

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return fail(OPENR_SPF_EIO, "%s failed: %s", #expr, hipGetErrorString(_e));       \
  } while (0)

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct Device {
  int ordinal = 0;
  int num_cus = 256;
  hipStream_t stream = nullptr;
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  DevGraph g;
  // scratch for host-buffer solves
  DevBuf<uint32_t> src, ign_ptr, ign_links;
  DevBuf<uint64_t> dist, tight;
  DevBuf<uint8_t> nh;
  DevBuf<uint32_t> ovf;  // re-run list of the BFS ring variants ([n * slices])
  // small multi-class batches: the classes run concurrently, one stream each (forked from
  // and joined back into the caller's stream), each with its own re-run list
  DevBuf<uint32_t> slicetmp;  // code-family sliced class: [n][nsl][V] next-hop chunks
  DevBuf<uint32_t> work;  // dynamic-scheduling counters (kWorkWords)
  DevBuf<uint32_t> status;  // sticky OPENR_SPF_STATUS_* bits of device-form calls
  DevBuf<uint32_t> perm, part;  // source-class partition of a batch
  // split batches (spf_derive.hip): node -> sid, the classify flags and neighbour table, the solved / derived
  // lists ([2n]), their class partition (+ the derived count at [2 * kMaxClasses]), the
  // solved units' level rows and the epoch stamps that tell which call left them
  DevBuf<uint32_t> dv_member, dv_nbrs, dv_perm, dv_part, dv_valid;
  DevBuf<uint8_t> dv_flags, dv_rows;
  uint32_t dv_epoch = 0;
  bool dv_last = false;  // the last solve call on this device split its batch
  // what-if sweep: base SPF rows, the affected-unit work list, chunk result rows
  DevBuf<uint64_t> base_dist, base_tight, wdist;
  DevBuf<uint8_t> base_nh, wnh;
  DevBuf<uint32_t> wsrc, wlink, wunit, wcount, wiota, win_links, win_src, wchanged;
  DevBuf<uint32_t> wbeg, wend;  // link-set sweep: each listed unit's slice of the set CSR
  DevBuf<uint32_t> wchanged_t;  // grouped repair: results source-major, transposed into the caller's rows
  // host forms, the units' CSRs (upload_whatif_units): node (win_ptr / win_nodes), link (win_lptr /
  // win_links; single links: win_links alone), edge (win_eptr / win_edges / win_metrics)
  DevBuf<uint32_t> win_ptr, win_nodes, win_lptr, win_eptr, win_edges, win_metrics;
  DevBuf<uint16_t> base_tin;  // what-if base SPF: tight in-degree rows (rounds plan)
  size_t wiota_n = 0;  // wiota[0, wiota_n) holds 0, 1, 2, ... (kept across calls)
  // KSP2: base rows, chunk rows, per-chunk ignore slots / sources / pointers, status
  DevBuf<uint64_t> kbase, krows;
  DevBuf<uint16_t> krows16;  // KSP2 second SPFs on the code family: u16 level rows
  uint32_t ktag = 0;         // tagged krows16: tag of the last chunk (0 = rows zeroed)
  size_t ktag_rows = 0;      // entries of krows16 zeroed for tagging
  DevBuf<uint32_t> kign, kend, ksrc, kptr, kstatus, kin_src, kin_row, kin_dst, ktok1, ktok2, kq;
  DevBuf<uint32_t> kretry;  // KSP small-tier overflows: [0,1] counts (k = 1, k = 2), lists after
  DevBuf<uint32_t> kkeep, kpart;  // KSP pairs that need a second SPF; its count as a class partition
  DevBuf<uint32_t> ktloff;  // KSP2 k = 1: per base row, pathLinks list offsets [V + 1]
  DevBuf<uint2> ktlent;     // ... and entries [E] (launch_ksp_path_lists)
  // what-if delta output of the host form (openr_spf_whatif_delta): per-unit pool offsets,
  // the pool (node, distance, next-hop bytes) and its cursor
  DevBuf<uint32_t> dl_off, dl_node;
  DevBuf<unsigned long long> dl_dist, dl_used, dl_tsum;
  DevBuf<uint8_t> dl_nh;
  // ... and the host form's device-side CSR before it is copied out
  DevBuf<unsigned long long> dlo_ptr, dlo_dist;
  DevBuf<uint32_t> dlo_node;
  DevBuf<uint8_t> dlo_nh;
  // route-level calls (spf_routes.hip): the sweep's node delta in CSR form, the base routes,
  // the inverse map node -> groups, the per-workgroup overlay / bitmap slices when they are
  // not in LDS, and the host forms' group table and outputs before they are copied out
  DevBuf<unsigned long long> rt_nptr, rt_ndist, rt_bmetric, rt_iptr, rt_tsum, rt_optr, rt_ometric;
  DevBuf<uint32_t> rt_nchanged, rt_nnode, rt_inv, rt_icnt, rt_icur, rt_large, rt_ovl, rt_bm;
  DevBuf<uint32_t> rt_gptr, rt_gnodes, rt_ochanged, rt_ogroup, rt_onbest;
  DevBuf<uint8_t> rt_nnh, rt_bnh, rt_onh;
  // loop-free alternates (spf_lfa.hip): the needed-row bitmaps, their scan and list, the
  // node -> row index, the neighbour table, and the host form's outputs before they are
  // copied out (metric / nh share rt_ometric / rt_onh with the routes calls)
  DevBuf<uint32_t> lf_need, lf_srcbm, lf_cnt, lf_list, lf_rowidx, lf_trow, lf_nalt, lf_onbr;
  DevBuf<unsigned long long> lf_wptr, lf_tsum, lf_ttome, lf_tfrom, lf_optr, lf_oam;
  DevBuf<uint8_t> lf_nh, lf_alt;
  // post-failure alternates (spf_wlfa.hip): the closure list the sweep runs over, the base
  // alternates and unprotected counts, the affected-unit list, the bitmap slices when they
  // are not in LDS, and the host form's outputs before they are copied out (the node delta,
  // base routes and inverse map share the rt_ buffers, the closure the lf_ ones)
  DevBuf<uint32_t> wl_clos, wl_bunprot, wl_alist, wl_acount, wl_bm, wl_ochanged, wl_ounprot, wl_olost, wl_ogroup;
  DevBuf<unsigned long long> wl_optr, wl_ometric;
  DevBuf<uint8_t> wl_balt, wl_onh, wl_oalt;
  // alternates under restore events (spf_elfa.hip): the table of every neighbour with a
  // closure row, down links included (the base alternates keep lf_trow / lf_ttome)
  DevBuf<uint32_t> el_trow;
  DevBuf<unsigned long long> el_ttome;
  // incremental updates: patch records, the last patch's delta edges, refresh work list,
  // host-form refresh rows
  DevBuf<PatchRec> precs;
  DevBuf<DeltaEdge> delta;
  DevBuf<uint32_t> alist, asrc, acount, alist2, asrc2;  // refresh: listed rows (first / exact stage)
  // exact-order kernel: per-solve slots when a slot does not fit LDS; pop-order rows
  DevBuf<uint8_t> exscratch;
  DevBuf<uint32_t> order;
};

// Launch counters live zeroed: each kernel's last workgroup resets what it used.
hipError_t reserve_counters(Device& d) {
  if (d.work.p) return hipSuccess;
  hipError_t e = d.work.reserve(kWorkWords);
  if (e == hipSuccess) e = hipMemset(d.work.p, 0, kWorkWords * sizeof(uint32_t));
  return e;
}

void free_graph(DevGraph& g) {
  void* ptrs[] = {g.row, g.row2, g.row2t, g.ovl_bits, g.ellt,    g.ellv,  g.adj,  g.w,    g.win, g.rev,
                   g.lid, g.nbr,  g.ovl,   g.cls,      g.cls_lvl, g.ledge, g.rank, g.erec, g.w64, g.elld, g.erecs,
                   g.derivable};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  g = DevGraph{};
}

}  // namespace

namespace openr_spf {
void note_launch(const char* kernel) {
  if (g_launch_trace.size() < 4096) {
    g_launch_trace += kernel;
    g_launch_trace += ';';
  }
}
void clear_launch_trace() { g_launch_trace.clear(); }
}  // namespace openr_spf

struct openr_spf_ctx {
  std::vector<Device> devs;
  bool has_graph = false;
  uint32_t V = 0, E = 0, L = 0;
  std::vector<uint32_t> row_ptr, col;
  uint32_t nh_bits = 0;         // max distinct degree
  uint32_t w_min = 0, w_max = 0;
  bool metric_ok = true;        // every usable metric in [1, 2^31-1]
  uint32_t group_lanes = 4;
  int family = kFamCode;        // BFS kernel family picked for this graph (FrontierEstimate)
  uint32_t est_depth = 0;       // sampled BFS hop depth (general-metric kernel choice)
  uint32_t cls_mask[kNumFamilies] = {0, 0};  // source classes present among the nodes, per family
  uint32_t nsl[kNumFamilies] = {1, 1};       // next-hop slices of each family's sliced class
  uint32_t nsl_max() const { return std::max(nsl[0], nsl[1]); }
  openr_spf_stats_t stats{};
  // host copy of the mutable attributes and of the device arrays derived from them, so
  // openr_spf_patch_graph can recompute and re-upload single elements
  std::vector<uint64_t> metric;
  std::vector<uint8_t> edge_up, ovl;
  std::vector<uint32_t> adj, w, win, rev, lid, owner, ovl_bits;
  std::vector<uint2> ledge, row2t;
  std::vector<uint4> erec, ellt;
  std::vector<uint32_t> erec_pos;  // directed edge -> its position in DevGraph::erecs
  // delta edges of the most recent patch (openr_spf_refresh); invalid after set_graph
  std::vector<DeltaEdge> delta;
  bool delta_valid = false;
  // the rows before or after the last patch came from a graph with zero / wrapped
  // metrics: the delta filter's tight-edge reasoning does not hold, refresh every row
  bool delta_all = false;
  // no refresh since the last patch: the next patch merges into delta (rows may still be
  // those of the graph before the earlier patch), keeping each edge's oldest state
  bool refreshed = true;
  std::unordered_map<uint32_t, uint32_t> delta_index;  // directed edge -> delta slot
  // metrics of the usable edges as a multiset (w_min / w_max after a patch without an O(E)
  // scan) and the number of usable edges whose metric is 0 or above 2^31-1
  std::map<uint32_t, uint32_t> wcount;
  uint64_t n_bad_metric = 0;
  // per-patch marks (stamp == patch_epoch: set during this patch), so a patch costs
  // O(touched edges) rather than O(E)
  std::vector<uint32_t> seen_e, dirty_e, dirty_v;
  uint32_t patch_epoch = 0;
  void count_metric(uint32_t e, int dir) {  // e's contribution while it is usable
    if (adj[e] & kEdgeDown) return;
    const uint64_t m = metric[e];
    if (m == 0 || m > 0x7FFFFFFFull) {
      n_bad_metric += dir > 0 ? 1 : (uint64_t)-1;
      return;
    }
    if (dir > 0) ++wcount[(uint32_t)m];
    else if (auto it = wcount.find((uint32_t)m); it != wcount.end() && --it->second == 0) wcount.erase(it);
  }
};

namespace {

constexpr uint32_t kDeepGraphLevels = 24;
constexpr uint32_t kRoundsMaxDepth = 48;  // hop depth below which general metrics use the rounds kernel

struct Plan {
  bool exact = false;   // spf_exact.hip: the reference's heap process (metrics / sizes outside the fast kernels)
  bool use_metric = true;
  bool bfs = true;
  bool rounds = false;  // general metrics: distance rounds + Kahn (shallow graphs), else fringe
  int family = kFamCode;
  uint64_t cost = 1;
  uint32_t delta = 1;
  bool dist64 = false;
  int nh_mode = kNhByte;
};

// Tuning / test override (benchmarks and parity tests only): OPENR_SPF_BFS_FAMILY=code|lvl.
int family_override(int dflt) {
  const char* e = std::getenv("OPENR_SPF_BFS_FAMILY");
  if (!e) return dflt;
  if (!std::strcmp(e, "code")) return kFamCode;
  if (!std::strcmp(e, "lvl")) return kFamLvl;
  return dflt;
}

// Frontier shape of a graph, sampled on the host at set_graph (O(samples * (V + E))):
// BFS from evenly spaced sources plus the widest row, overloaded nodes as sinks
// (LinkState.cpp:831-838). depth picks the kernel family — the lvl kernels win on deep
// graphs (grid G100: ~150 levels of ~70 nodes; 1.07 vs 1.92 ms), the code kernels on
// shallow ones (fabric: 5 levels; 1.44 vs 1.95 ms) — and width2 (max |level L| +
// |level L+1|) sizes the frontier ring (width1 = max |level L|: the lean pass's halves).
struct FrontierEstimate {
  uint32_t depth = 0, width2 = 0, width1 = 0;
  int family() const { return depth >= kDeepGraphLevels ? kFamLvl : kFamCode; }
};

FrontierEstimate estimate_frontier(uint32_t V, const uint32_t* row_ptr, const uint32_t* adj, const uint8_t* ovl) {
  FrontierEstimate est;
  if (V == 0) return est;
  std::vector<uint32_t> srcs;
  const uint32_t ns = std::min<uint32_t>(V, 8u);
  for (uint32_t i = 0; i < ns; ++i) srcs.push_back((uint32_t)((uint64_t)i * V / ns));
  uint32_t widest = 0;
  for (uint32_t u = 1; u < V; ++u)
    if (row_ptr[u + 1] - row_ptr[u] > row_ptr[widest + 1] - row_ptr[widest]) widest = u;
  srcs.push_back(widest);
  std::vector<uint32_t> lvl(V), q, width;
  q.reserve(V);
  for (uint32_t src : srcs) {
    std::fill(lvl.begin(), lvl.end(), UINT32_MAX);
    q.clear();
    width.assign(1, 1);
    q.push_back(src);
    lvl[src] = 0;
    for (size_t i = 0; i < q.size(); ++i) {
      const uint32_t u = q[i];
      if (u != src && ovl[u]) continue;  // reached, never expanded
      for (uint32_t e = row_ptr[u]; e < row_ptr[u + 1]; ++e) {
        if (adj[e] & kEdgeDown) continue;
        const uint32_t v = adj[e];
        if (lvl[v] != UINT32_MAX) continue;
        lvl[v] = lvl[u] + 1u;
        if (lvl[v] >= width.size()) width.push_back(0);
        ++width[lvl[v]];
        q.push_back(v);
      }
    }
    est.depth = std::max<uint32_t>(est.depth, (uint32_t)width.size() - 1u);
    for (size_t l = 0; l + 1 < width.size(); ++l) est.width2 = std::max<uint32_t>(est.width2, width[l] + width[l + 1]);
    for (uint32_t w : width) est.width1 = std::max(est.width1, w);
  }
  return est;
}

// Bytes of exact-order slots (global memory) a device may hold at once.
constexpr uint64_t kExactScratchBytes = uint64_t(2) << 30;

int make_plan(const openr_spf_ctx* ctx, uint32_t flags, bool has_ign, Plan* p) {
  const bool use_metric = (flags & OPENR_SPF_USE_LINK_METRIC) != 0;
  p->use_metric = use_metric;
  // Outside the fast kernels' domain the exact-order kernel replays the reference's heap
  // process instead of refusing the graph: zero or wrapped-negative usable metrics (pop
  // order history-dependent), next-hop sets wider than 256, graphs larger
  // than the LDS-resident layouts, and pop-order output requests.
  auto exact = [p, ctx]() -> int {
    // one exact-order slot per solve, addressed with u32 offsets (spf_exact.hip ex_layout)
    const uint64_t slot = exact_slot_bytes(ctx->V, ctx->E, ctx->L, ctx->nh_bits);
    if (slot > 0xFFFFFFFFull || slot > kExactScratchBytes)
      return fail(OPENR_SPF_E2BIG, "graph too large for the exact-order kernel (%llu bytes per solve)",
                  (unsigned long long)slot);
    p->exact = true;
    return OPENR_SPF_OK;
  };
  if ((flags & OPENR_SPF_EMIT_ORDER) || std::getenv("OPENR_SPF_FORCE_EXACT")) return exact();
  if (use_metric && !ctx->metric_ok) return exact();
  p->nh_mode = nh_mode_for_bits(ctx->nh_bits);
  if (p->nh_mode < 0) return exact();
  if (!use_metric || ctx->w_min == ctx->w_max) {
    p->bfs = true;
    p->cost = use_metric ? std::max<uint32_t>(ctx->w_min, 1u) : 1u;
    p->family = family_override(ctx->family);
    for (int c = 0; c < num_classes(p->family); ++c)
      if ((ctx->cls_mask[p->family] >> c) & 1u)
        if (!bfs_lds_bytes(p->family, ctx->V, ctx->L, has_ign, c)) return exact();
  } else {
    p->bfs = false;
    p->delta = ctx->w_min;
    p->dist64 = (uint64_t)ctx->V * ctx->w_max >= 0xFFFFFFFFull;
    // shallow graphs (sampled hop depth): rounds scale with hops, the fringe with distinct
    // distances (OPENR_SPF_GENERAL=fringe|rounds overrides)
    p->rounds = ctx->est_depth < kRoundsMaxDepth && ctx->devs[0].g.max_deg < 65535u;  // u16 in-degrees
    if (const char* e = std::getenv("OPENR_SPF_GENERAL")) {
      if (!std::strcmp(e, "fringe")) p->rounds = false;
      if (!std::strcmp(e, "rounds")) p->rounds = ctx->devs[0].g.max_deg < 65535u;
    }
    if (p->rounds && !rounds_lds_bytes(ctx->V, ctx->L, has_ign, p->nh_mode, p->dist64)) p->rounds = false;
    if (!fringe_lds_bytes(ctx->V, ctx->L, has_ign, p->nh_mode, p->dist64)) return exact();
  }
  return OPENR_SPF_OK;
}


// Split batches (spf_derive.hip): of a single-class lvl-family batch that asks for plain u64
// distance and next-hop rows, only the sources that cover every link are solved; the rest
// are derived from their neighbours' level rows. OPENR_SPF_DERIVE: 0 never, 1 wherever it
// is legal, unset: batches above kDeriveAutoPerCu sources per CU. A batch of at most one
// round of solves per CU cannot gain (its solved half takes the same one round): the wave
// pass holds 8 solves per CU, and G100 on 256 CUs loses at 1 250 sources (0.150 -> 0.185 ms)
// and gains from 2 500 on (0.255 -> 0.198 ms).
// On success either a is unchanged (no split) or a.perm / a.part / a.dv describe the split.
constexpr uint32_t kDeriveAutoPerCu = 8;
constexpr uint64_t kDeriveRowsBudget = 1ull << 30;  // level-row scratch a device may hold
hipError_t split_batch(Device& d, SolveArgs& a, int fam, int group_lanes, hipStream_t s) {
  const char* env = std::getenv("OPENR_SPF_DERIVE");
  const uint32_t knob = !env ? 2u : env[0] == '0' ? 0u : env[0] == '1' ? 1u : 2u;
  if (knob == 0u || (knob == 2u && (uint64_t)a.n <= (uint64_t)kDeriveAutoPerCu * (uint64_t)std::max(d.num_cus, 1)))
    return hipSuccess;
  if (fam != kFamLvl || !a.dist || !a.nh || a.tight || a.ign_ptr || a.lvl_rows || a.lvl16 || a.target || a.seed_dist ||
      a.out_row || a.order || a.n < 2u || prof_enabled())
    return hipSuccess;
  if (!bfs_lvl_fast_pass(d.g, a, group_lanes, d.num_cus)) return hipSuccess;
  const uint32_t stride = (d.g.V + 15u) & ~15u;
  if ((uint64_t)a.n * stride > kDeriveRowsBudget) return hipSuccess;
  hipError_t err = d.dv_member.reserve(std::max<uint32_t>(d.g.V, 1u));
  if (err == hipSuccess) err = d.dv_flags.reserve((size_t)a.n + 16u);
  if (err == hipSuccess) err = d.dv_nbrs.reserve(2u * kDeriveMaxNbrs * (size_t)a.n);
  if (err == hipSuccess) err = d.dv_perm.reserve(2u * (size_t)a.n);
  if (err == hipSuccess) err = d.dv_part.reserve(2u * kMaxClasses + 1u);
  if (err == hipSuccess) err = d.dv_rows.reserve((size_t)a.n * stride);
  if (err == hipSuccess && (a.n > d.dv_valid.cap || d.dv_epoch == 0xFFFFFFFFu)) {
    // stamps of no epoch: a fresh (or wrapped) buffer is zeroed, epochs start at 1
    err = d.dv_valid.reserve(a.n);
    if (err == hipSuccess) err = hipMemsetAsync(d.dv_valid.p, 0, d.dv_valid.cap * sizeof(uint32_t), s);
    d.dv_epoch = 0;
  }
  if (err != hipSuccess) return err;
  uint32_t* count = d.dv_part.p + 2u * kMaxClasses;
  err = launch_derive_split(d.g, a.sources, a.n, a.cls, d.dv_member.p, d.dv_flags.p, d.dv_nbrs.p, d.dv_perm.p, d.dv_part.p, count,
                            d.num_cus, s);
  if (err != hipSuccess) return err;
  a.perm = d.dv_perm.p;
  a.part = d.dv_part.p;
  a.dv.rows = d.dv_rows.p;
  a.dv.stride = stride;
  a.dv.epoch = ++d.dv_epoch;
  a.dv.valid = d.dv_valid.p;
  a.dv.nbrs = d.dv_nbrs.p;
  a.dv.count = count;
  d.dv_last = true;
  return hipSuccess;
}

// Uniform-cost solves run per source class (next-hop width): one class -> one launch;
// several -> a device-side partition of the batch, then one launch per class, the
// widest first.
hipError_t launch(const openr_spf_ctx* ctx, Device& d, const Plan& p, SolveArgs a, hipStream_t s,
                  bool may_derive = false) {
  LaunchInfo info;
  d.dv_last = false;
  if (p.exact) {  // writes every dist / nh / tight word itself
    const uint64_t slot = exact_slot_bytes(d.g.V, d.g.E, d.g.L, ctx->nh_bits);
    uint64_t bytes = 0;
    if (slot > kMaxLds || std::getenv("OPENR_SPF_EXACT_GLOBAL")) {
      const uint64_t slots = std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)a.n, (uint64_t)d.num_cus * 8u,
                                                                        kExactScratchBytes / std::max<uint64_t>(slot, 1)}));
      bytes = slots * slot;
      hipError_t err = d.exscratch.reserve(bytes);
      if (err != hipSuccess) return err;
    }
    hipError_t err = reserve_counters(d);
    if (err != hipSuccess) return err;
    return launch_exact(d.g, a, d.g.w64, p.use_metric, ctx->nh_bits, d.exscratch.p, bytes, a.order,
                        d.work.p + kExactCtr, d.num_cus, s);
  }
  if (a.tight && !a.out_row) {
    hipError_t err = hipMemsetAsync(a.tight, 0, (size_t)a.n * ((d.g.E + 63u) / 64u) * 8u, s);
    if (err != hipSuccess) return err;
  }
  if (!p.bfs) {
    if (p.rounds) return launch_rounds(d.g, a, p.dist64, p.nh_mode, d.num_cus, s, &info);
    return launch_fringe(d.g, a, p.delta, p.dist64, p.nh_mode, d.num_cus, s, &info);
  }
  const int gl = (int)ctx->group_lanes;
  // a caller's list of the batch (KSP2 second SPFs: the pairs ksp_select_pairs kept) is
  // honoured by the single-class distance-only launch; every other launch partitions
  const uint32_t* list = a.perm;
  const uint32_t* list_part = a.part;
  a.perm = nullptr;
  a.part = nullptr;
  const int fam = p.family;
  uint32_t mask = ctx->cls_mask[fam];
  a.nsl = ctx->nsl[fam];
  a.dist_only = 0;
  if (fam == kFamCode && !a.nh && !a.tight) {  // distances only (KSP2 SPFs): 8-bit fields, no slices
    a.dist_only = 1;
    // OPENR_SPF_KSP_PULL=0: the target's pull test (2) one neighbour per wave (A/B, tests)
    if (const char* e = std::getenv("OPENR_SPF_KSP_PULL"))
      if (std::atoi(e) == 0) a.dist_only |= 2u;
    a.nsl = 1;
    mask = 1u << kCls8;
  }
  a.k0 = a.krows = 0;
  if (fam == kFamCode && ((mask >> kClsSliced) & 1u) && a.nh) {
    // slice scratch for at most a budget's worth of sliced solves at a time (the class runs
    // in chunks of krows): 512 MiB, OPENR_SPF_SLICE_ROWS (tests) forces a chunk size
    const uint64_t per_row = (uint64_t)a.nsl * d.g.V * sizeof(uint32_t);
    const uint64_t budget_rows = std::max<uint64_t>(1, (512ull << 20) / std::max<uint64_t>(per_row, 1));
    const uint32_t forced = (uint32_t)std::strtoul(std::getenv("OPENR_SPF_SLICE_ROWS") ? std::getenv("OPENR_SPF_SLICE_ROWS") : "0", nullptr, 10);
    const uint32_t rows = (uint32_t)std::min<uint64_t>(std::max(a.n, 1u), forced ? forced : budget_rows);
    hipError_t err = d.slicetmp.reserve((size_t)rows * a.nsl * d.g.V);
    if (err != hipSuccess) return err;
    a.slice_tmp = d.slicetmp.p;
    a.krows = rows;
  }
  if (__builtin_popcount(mask) == 1) {
    a.cls = (uint32_t)__builtin_ctz(mask);
    if (a.dist_only && list) {  // part[cls] = listed count, part[kMaxClasses + cls] = 0
      a.perm = list;
      a.part = list_part;
    }
    if (may_derive && !list) {
      hipError_t err = split_batch(d, a, fam, gl, s);
      if (err != hipSuccess) return err;
    }
    return launch_bfs(fam, d.g, a, p.cost, gl, d.num_cus, s, &info);
  }
  hipError_t err = d.perm.reserve(std::max<uint32_t>(a.n, 1u));
  if (err == hipSuccess) err = d.part.reserve(3u * kMaxClasses);
  if (err == hipSuccess) err = launch_partition(a.sources, a.n, fam == kFamLvl ? d.g.cls_lvl : d.g.cls, d.g.V, d.part.p,
                                                 d.perm.p, s);
  if (err != hipSuccess) return err;
  a.perm = d.perm.p;
  a.part = d.part.p;
  // classes one after another on the caller's stream (side-by-side class streams were
  // measured slower: the fork / join cost more than the overlap saved, round 3)
  const int nc = num_classes(fam);
  for (int c = nc - 1; c >= 0; --c) {
    if (!((mask >> c) & 1u)) continue;
    a.cls = (uint32_t)c;
    err = launch_bfs(fam, d.g, a, p.cost, gl, d.num_cus, s, &info);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

int check_solve_args(const openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n, uint64_t* dist,
                     uint8_t* nh, uint32_t nh_bytes) {
  if (!ctx) return fail(OPENR_SPF_EINVAL, "null context");
  if (!ctx->has_graph) return fail(OPENR_SPF_EINVAL, "no graph set (openr_spf_set_graph)");
  if (n && (!sources || !dist)) return fail(OPENR_SPF_EINVAL, "null sources or dist");
  const uint32_t need = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  if (nh && nh_bytes < need) return fail(OPENR_SPF_EINVAL, "nh_bytes %u < required %u", nh_bytes, need);
  return OPENR_SPF_OK;
}

int solve_host(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n, uint32_t flags,
               const uint32_t* ignore_ptr, const uint32_t* ignore_links, uint64_t* dist, uint8_t* nh,
               uint32_t nh_bytes, uint64_t* tight, uint32_t* order = nullptr) {
  clear_launch_trace();
  if (order) flags |= OPENR_SPF_EMIT_ORDER;
  int rc = check_solve_args(ctx, sources, n, dist, nh, nh_bytes);
  if (rc) return rc;
  for (uint32_t i = 0; i < n; ++i)
    if (sources[i] >= ctx->V) return fail(OPENR_SPF_EINVAL, "source %u out of range (V=%u)", sources[i], ctx->V);
  if (ignore_ptr) {
    if (ignore_ptr[0] != 0) return fail(OPENR_SPF_EINVAL, "ignore_ptr[0] must be 0");
    for (uint32_t i = 0; i < n; ++i)
      if (ignore_ptr[i + 1] < ignore_ptr[i]) return fail(OPENR_SPF_EINVAL, "ignore_ptr not monotone");
    if (ignore_ptr[n] && !ignore_links) return fail(OPENR_SPF_EINVAL, "null ignore_links");
  }
  Plan plan;
  rc = make_plan(ctx, flags, ignore_ptr != nullptr, &plan);
  if (rc) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t V = ctx->V, tw = (ctx->E + 63u) / 64u;
  const uint32_t nd = (uint32_t)ctx->devs.size();
  const uint32_t per = (n + nd - 1) / std::max<uint32_t>(nd, 1);
  std::vector<uint32_t> rebased;
  for (uint32_t di = 0; di < nd; ++di) {
    Device& d = ctx->devs[di];
    const uint32_t b = std::min(n, di * per), e = std::min(n, b + per), m = e - b;
    if (!m) continue;
    HIP_TRY(hipSetDevice(d.ordinal));
    HIP_TRY(d.src.reserve(m));
    HIP_TRY(d.dist.reserve((size_t)m * V));
    if (nh) HIP_TRY(d.nh.reserve((size_t)m * V * nh_bytes));
    if (tight) HIP_TRY(d.tight.reserve((size_t)m * tw));
    if (order) HIP_TRY(d.order.reserve((size_t)m * V));
    HIP_TRY(hipMemcpyAsync(d.src.p, sources + b, m * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    SolveArgs a{};
    a.sources = d.src.p;
    a.n = m;
    if (ignore_ptr) {
      const uint32_t lb = ignore_ptr[b], le = ignore_ptr[e];
      rebased.resize(m + 1);
      for (uint32_t i = 0; i <= m; ++i) rebased[i] = ignore_ptr[b + i] - lb;
      HIP_TRY(d.ign_ptr.reserve(m + 1));
      HIP_TRY(d.ign_links.reserve(std::max<uint32_t>(le - lb, 1u)));
      HIP_TRY(hipMemcpy(d.ign_ptr.p, rebased.data(), (m + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
      if (le > lb)
        HIP_TRY(hipMemcpyAsync(d.ign_links.p, ignore_links + lb, (le - lb) * sizeof(uint32_t),
                               hipMemcpyHostToDevice, d.stream));
      a.ign_ptr = d.ign_ptr.p;
      a.ign_links = d.ign_links.p;
    }
    a.dist = d.dist.p;
    a.nh = nh ? d.nh.p : nullptr;
    a.nh_bytes = nh_bytes;
    a.tight = tight ? d.tight.p : nullptr;
    a.order = order ? d.order.p : nullptr;
    a.nh_bits = ctx->nh_bits;
    HIP_TRY(d.ovf.reserve((size_t)m * ctx->nsl_max()));
    a.ovf_list = d.ovf.p;
    HIP_TRY(reserve_counters(d));
    a.work = d.work.p;
    HIP_TRY(hipEventRecord(d.ev_begin, d.stream));
    HIP_TRY(launch(ctx, d, plan, a, d.stream, true));
    HIP_TRY(hipEventRecord(d.ev_end, d.stream));
    HIP_TRY(hipMemcpyAsync(dist + (size_t)b * V, d.dist.p, (size_t)m * V * sizeof(uint64_t),
                           hipMemcpyDeviceToHost, d.stream));
    if (nh)
      HIP_TRY(hipMemcpyAsync(nh + (size_t)b * V * nh_bytes, d.nh.p, (size_t)m * V * nh_bytes,
                             hipMemcpyDeviceToHost, d.stream));
    if (tight)
      HIP_TRY(hipMemcpyAsync(tight + (size_t)b * tw, d.tight.p, (size_t)m * tw * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, d.stream));
    if (order)
      HIP_TRY(hipMemcpyAsync(order + (size_t)b * V, d.order.p, (size_t)m * V * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, d.stream));
  }
  double kms = 0.0;
  for (uint32_t di = 0; di < nd; ++di) {
    Device& d = ctx->devs[di];
    const uint32_t b = std::min(n, di * per), e = std::min(n, b + per);
    if (e <= b) continue;
    HIP_TRY(hipSetDevice(d.ordinal));
    HIP_TRY(hipStreamSynchronize(d.stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, d.ev_begin, d.ev_end));
    kms = std::max(kms, (double)ms);
  }
  ctx->stats.spf_runs += n;
  ctx->stats.batches += 1;
  ctx->stats.last_kernel_ms = kms;
  ctx->stats.last_batch_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return OPENR_SPF_OK;
}

// Identity array 0, 1, ..., n-1 in d.wiota (one-link ignore sets: solve k ignores exactly
// links[k]); built once and kept while it is long enough.
hipError_t ensure_iota(Device& d, size_t n, hipStream_t s) {
  if (n <= d.wiota_n) return hipSuccess;
  if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
  d.wiota_n = 0;
  hipError_t e = d.wiota.reserve(n);
  if (e == hipSuccess) e = launch_iota(d.wiota.p, (uint32_t)n, d.num_cus, s);
  if (e == hipSuccess) d.wiota_n = n;
  return e;
}

// Bytes of chunk result rows a what-if sweep may hold on a device at once.
constexpr size_t kWhatifChunkBytes = size_t(1) << 30;

#define OPENR_TRY(x)              \
  do {                            \
    err = (x);                    \
    if (err != hipSuccess) return err; \
  } while (0)

// OPENR_SPF_PROF tuning aid: the phase split of `nres` seeded re-solves (SolveArgs::prof_solve:
// ten u64 per solve, 100 MHz wall clock) and how many ran side by side.
void print_resolve_prof(const std::vector<unsigned long long>& h, uint32_t nres) {
  if (!nres) return;
  unsigned long long t0 = ~0ull, t1 = 0;
  double ph[7] = {0}, na = 0, rd = 0, rk = 0, tot = 0;
  for (uint32_t k = 0; k < nres; ++k) {
    const unsigned long long* x = &h[10 * (size_t)k];
    t0 = std::min(t0, x[0]);
    t1 = std::max(t1, x[7]);
    for (int q = 0; q < 7; ++q) ph[q] += (double)(x[q + 1] - x[q]) / 100.0;
    tot += (double)(x[7] - x[0]) / 100.0;
    na += (double)x[8];
    rd += (double)(x[9] & 0xFFFFFFFFull);
    rk += (double)(x[9] >> 32);
  }
  std::fprintf(stderr,
               "[whatif resolve] n=%u span=%.1fus mean solve %.1fus: seed-a %.1f seed-A %.1f seed-c %.1f "
               "dist %.1f indeg %.1f kahn %.1f compare %.1f | |A| %.1f, rounds: A+c+dist %.1f, kahn %.1f, "
               "concurrency %.0f\n",
               nres, (t1 - t0) / 100.0, tot / nres, ph[0] / nres, ph[1] / nres, ph[2] / nres, ph[3] / nres,
               ph[4] / nres, ph[5] / nres, ph[6] / nres, na / nres, rd / nres, rk / nres,
               tot / ((t1 - t0) / 100.0));
  // duration spread, its correlation with |A|, and the solves running over the span
  std::vector<double> dur(nres), asz(nres);
  for (uint32_t k = 0; k < nres; ++k) {
    dur[k] = (double)(h[10 * (size_t)k + 7] - h[10 * (size_t)k]) / 100.0;
    asz[k] = (double)h[10 * (size_t)k + 8];
  }
  std::vector<double> srt = dur;
  std::sort(srt.begin(), srt.end());
  const double md = tot / nres, ma = na / nres;
  double sxy = 0, sxx = 0, syy = 0;
  for (uint32_t k = 0; k < nres; ++k) {
    sxy += (dur[k] - md) * (asz[k] - ma);
    sxx += (dur[k] - md) * (dur[k] - md);
    syy += (asz[k] - ma) * (asz[k] - ma);
  }
  std::fprintf(stderr, "  duration p10 %.1f p50 %.1f p90 %.1f max %.1f us; corr(duration, |A|) %.2f; running at",
               srt[nres / 10], srt[nres / 2], srt[nres * 9 / 10], srt.back(),
               sxx > 0 && syy > 0 ? sxy / std::sqrt(sxx * syy) : 0.0);
  for (int q : {10, 25, 50, 75, 90, 95}) {
    const unsigned long long tq = t0 + (t1 - t0) * q / 100;
    uint32_t live = 0;
    for (uint32_t k = 0; k < nres; ++k) live += (h[10 * (size_t)k] <= tq && h[10 * (size_t)k + 7] > tq) ? 1u : 0u;
    std::fprintf(stderr, " %d%%:%u", q, live);
  }
  std::fprintf(stderr, "\n");
}

// Base SPF of a what-if sweep (single links or link sets): every source's no-failure rows
// into d.base_dist / base_nh / base_tight, and on the rounds plan each row's tight
// in-degrees into d.base_tin for the seeded re-solves (*base_tin says whether).
hipError_t whatif_base_solve(openr_spf_ctx* ctx, Device& d, const Plan& base_plan, const uint32_t* d_sources,
                             uint32_t n_src, hipStream_t s, bool* base_tin) {
  const uint32_t V = ctx->V, tw = (ctx->E + 63u) / 64u;
  const uint32_t nb = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  hipError_t err;
  OPENR_TRY(d.base_dist.reserve((size_t)n_src * V));
  OPENR_TRY(d.base_nh.reserve((size_t)n_src * V * nb));
  OPENR_TRY(d.base_tight.reserve((size_t)n_src * tw));
  OPENR_TRY(reserve_counters(d));
  SolveArgs a{};
  a.sources = d_sources;
  a.n = n_src;
  a.dist = d.base_dist.p;
  a.nh = d.base_nh.p;
  a.nh_bytes = nb;
  a.tight = d.base_tight.p;
  a.nh_bits = ctx->nh_bits;
  OPENR_TRY(d.ovf.reserve((size_t)n_src * ctx->nsl_max()));
  a.ovf_list = d.ovf.p;
  a.work = d.work.p;
  // the rounds kernel also leaves each base row's tight in-degrees for the seeded re-solves
  *base_tin = base_plan.rounds && !base_plan.exact && !base_plan.bfs;
  if (*base_tin) {
    OPENR_TRY(d.base_tin.reserve((size_t)n_src * V));
    a.tin_out = d.base_tin.p;
  }
  return launch(ctx, d, base_plan, a, s);
}

// Re-solve the `count` units listed from `base` on in wsrc / wunit and compare each row with
// its source's base row. set_links == nullptr: unit k ignores the single link wlink[k];
// else it ignores set_links[wbeg[k], wend[k]) (link sets: the list points into the caller's
// CSR, nothing is copied).
hipError_t whatif_resolve_units(openr_spf_ctx* ctx, Device& d, const Plan& ign_plan, uint32_t count, uint32_t base,
                                const uint32_t* set_links, uint32_t n_src, bool base_tin, uint32_t* d_changed,
                                const WhatifDelta& dl, hipStream_t s) {
  const uint32_t V = ctx->V;
  const uint32_t nb = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  hipError_t e2;
  const size_t row = (size_t)V * (8u + nb);
  const uint32_t chunk = (uint32_t)std::min<size_t>(count, std::max<size_t>(1, kWhatifChunkBytes / row));
  if ((e2 = d.wdist.reserve((size_t)chunk * V)) != hipSuccess) return e2;
  if ((e2 = d.wnh.reserve((size_t)chunk * V * nb)) != hipSuccess) return e2;
  if (!set_links && (e2 = ensure_iota(d, (size_t)chunk + 1u, s)) != hipSuccess) return e2;
  if ((e2 = d.ovf.reserve((size_t)chunk * ctx->nsl_max())) != hipSuccess) return e2;
  std::vector<unsigned long long> prof_rec;
  for (uint32_t off0 = 0; off0 < count; off0 += chunk) {
    const uint32_t m = std::min(chunk, count - off0), off = base + off0;
    SolveArgs b{};
    b.sources = d.wsrc.p + off;
    b.n = m;
    if (set_links) {  // solve k ignores set_links[wbeg[off + k], wend[off + k])
      b.ign_ptr = d.wbeg.p + off;
      b.ign_end = d.wend.p + off;
      b.ign_links = set_links;
    } else {
      b.ign_ptr = d.wiota.p;  // solve k ignores exactly wlink[off + k]
      b.ign_links = d.wlink.p + off;
    }
    b.dist = d.wdist.p;
    b.nh = d.wnh.p;
    b.nh_bytes = nb;
    b.nh_bits = ctx->nh_bits;
    b.ovf_list = d.ovf.p;
    b.work = d.work.p;
    // the rounds kernel starts each unit from its source's base rows (only the nodes the
    // failed links push back are re-solved); other kernels solve from scratch
    b.seed_dist = d.base_dist.p;
    b.seed_tight = d.base_tight.p;
    b.seed_unit = d.wunit.p + off;
    b.seed_nsrc = n_src;
    b.seed_tin = base_tin ? d.base_tin.p : nullptr;
    // ... and compares each solve with the base rows itself (no rows through HBM)
    const bool fused = ign_plan.rounds && !ign_plan.exact && !ign_plan.bfs;
    if (fused) {
      b.seed_nh = d.base_nh.p;
      b.seed_changed = d_changed;
      b.delta = dl;
    }
    // OPENR_SPF_PROF (tuning aid, link-set sweeps): the seeded re-solves' phase records
    const bool prof = fused && set_links && prof_enabled();
    if (prof) {
      const size_t bytes = 10 * (size_t)m * sizeof(unsigned long long);
      if ((e2 = hipMallocAsync(reinterpret_cast<void**>(&b.prof_solve), bytes, s)) != hipSuccess) return e2;
      if ((e2 = hipMemsetAsync(b.prof_solve, 0, bytes, s)) != hipSuccess) return e2;
    }
    if ((e2 = launch(ctx, d, ign_plan, b, s)) != hipSuccess) return e2;
    if (prof) {
      const size_t at = prof_rec.size();
      prof_rec.resize(at + 10 * (size_t)m);
      if ((e2 = hipMemcpyAsync(prof_rec.data() + at, b.prof_solve, 10 * (size_t)m * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, s)) != hipSuccess)
        return e2;
      if ((e2 = hipStreamSynchronize(s)) != hipSuccess) return e2;
      if ((e2 = hipFreeAsync(b.prof_solve, s)) != hipSuccess) return e2;
    }
    if (!fused && (e2 = launch_rows_compare(m, V, nb, d.wdist.p, d.wnh.p, d.base_dist.p, d.base_nh.p, d.wunit.p + off, n_src,
                                  d_changed, dl, d.num_cus, s)) != hipSuccess)
      return e2;
  }
  if (!prof_rec.empty()) print_resolve_prof(prof_rec, (uint32_t)(prof_rec.size() / 10));
  return hipSuccess;
}

// Per-link-failure what-if sweep on one device (spf_sweep.hip has the unit semantics):
// base SPF with tight edges -> filter of the affected units -> chunks of single-link
// ignore-set solves through the ordinary launcher -> row comparison against the base.
// Reads the affected-unit count back (one stream sync) to size the chunks.
hipError_t whatif_on_device(openr_spf_ctx* ctx, Device& d, const Plan& base_plan, const Plan& ign_plan,
                            const uint32_t* d_links, uint32_t n_links, const uint32_t* d_sources, uint32_t n_src,
                            uint32_t* d_changed, hipStream_t s, uint32_t* solved, bool use_link_metric,
                            const WhatifDelta& dl = WhatifDelta{}) {
  const uint32_t V = ctx->V;
  const uint32_t nb = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  *solved = 0;
  if (!n_src || !n_links) return hipSuccess;
  hipError_t err;
  bool base_tin = false;
  OPENR_TRY(whatif_base_solve(ctx, d, base_plan, d_sources, n_src, s, &base_tin));
  auto resolve_units = [&](uint32_t count, uint32_t base) -> hipError_t {
    return whatif_resolve_units(ctx, d, ign_plan, count, base, nullptr, n_src, base_tin, d_changed, dl, s);
  };
  const char* mode = std::getenv("OPENR_SPF_WHATIF");
  const bool dist64 = use_link_metric && (uint64_t)V * ctx->w_max >= 0xFFFFFFFFull;
  // exact-order plans (metrics / widths outside the fast kernels): filter + re-solve; with
  // zero or wrapped metrics the pop order depends on every relaxation, so every unit whose
  // link is up is re-solved (no tight-edge filter)
  const bool exact = base_plan.exact || ign_plan.exact;
  if (!exact && (!mode || !std::strcmp(mode, "group"))) {
    // default: grouped repair (base rows staged once per (source, link chunk), fused filter)
    // (a unit with more dirty nodes than a wave's slots is re-solved after the launch)
    if (whatif_group_lds_bytes(V, ctx->E, nb, dist64, d.g.max_deg)) {
      const size_t units = (size_t)n_links * n_src;
      OPENR_TRY(d.wcount.reserve(3));
      OPENR_TRY(d.wsrc.reserve(units));
      OPENR_TRY(d.wlink.reserve(units));
      OPENR_TRY(d.wunit.reserve(units));
      OPENR_TRY(d.wchanged_t.reserve(units));
      OPENR_TRY(hipEventRecord(d.ev_begin, s));  // the repair kernel's own time -> stats.last_kernel_ms
      OPENR_TRY(launch_whatif_group(d.g, d_links, n_links, d_sources, n_src, d.base_dist.p, d.base_nh.p,
                                    d.base_tight.p, base_tin ? d.base_tin.p : nullptr, nb, !use_link_metric, dist64, ctx->w_max, ctx->nh_bits,
                                    d_changed, d.wchanged_t.p, d.wcount.p, d.wsrc.p, d.wlink.p, d.wunit.p,
                                    d.work.p + kIncrCtr, dl, d.num_cus, s));
      OPENR_TRY(hipEventRecord(d.ev_end, s));
      // Units past the slots are large (WAN: ~6 500 of 1.02 M affected units, ~150 dirty
      // nodes on average): re-solved, each starting from its source's base rows (the
      // rounds kernel's seeded start). On the rounds plan one launch covers them, its
      // count read on the device (wcount[1]): no host round trip between the kernels.
      const bool fused = ign_plan.rounds && !ign_plan.exact && !ign_plan.bfs;
      if (fused) {
        OPENR_TRY(ensure_iota(d, units + 1u, s));
        SolveArgs b{};
        b.sources = d.wsrc.p;
        b.n = (uint32_t)std::min<size_t>(units, 0xFFFFFFFEu);
        b.n_dev = d.wcount.p + 1;
        // two waves per solve: WAN re-solves (6 835 units, 256-thread base SPF) 64 / 128 / 256
        // threads: span 1.02 / 0.83 / 1.00 ms (more solves resident, rounds still split)
        b.n_block = 128u;
        b.ign_ptr = d.wiota.p;  // solve k ignores exactly wlink[k]
        b.ign_links = d.wlink.p;
        b.nh_bytes = nb;
        b.nh_bits = ctx->nh_bits;
        b.work = d.work.p;
        b.seed_dist = d.base_dist.p;
        b.seed_tight = d.base_tight.p;
        b.seed_unit = d.wunit.p;
        b.seed_nsrc = n_src;
        b.seed_tin = base_tin ? d.base_tin.p : nullptr;
        b.seed_nh = d.base_nh.p;
        b.seed_changed = d_changed;
        b.delta = dl;
        if (prof_enabled()) {
          OPENR_TRY(hipMallocAsync(reinterpret_cast<void**>(&b.prof_solve), 10 * units * sizeof(unsigned long long), s));
          OPENR_TRY(hipMemsetAsync(b.prof_solve, 0, 10 * units * sizeof(unsigned long long), s));
        }
        OPENR_TRY(launch(ctx, d, ign_plan, b, s));
        if (b.prof_solve) {  // tuning aid: the re-solves' phases (100 MHz wall clock) and the tail
          uint32_t nres = 0;
          OPENR_TRY(hipMemcpyAsync(&nres, d.wcount.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
          OPENR_TRY(hipStreamSynchronize(s));
          std::vector<unsigned long long> h(10 * (size_t)nres);
          OPENR_TRY(hipMemcpy(h.data(), b.prof_solve, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
          OPENR_TRY(hipFreeAsync(b.prof_solve, s));
          print_resolve_prof(h, nres);
        }
      }
      uint32_t cnt[2] = {0, 0};  // affected units, units past the slots
      OPENR_TRY(hipMemcpyAsync(cnt, d.wcount.p, sizeof(cnt), hipMemcpyDeviceToHost, s));
      OPENR_TRY(hipStreamSynchronize(s));
      float ms = 0.f;
      OPENR_TRY(hipEventElapsedTime(&ms, d.ev_begin, d.ev_end));
      ctx->stats.last_kernel_ms = ms;
      if (!fused && cnt[1]) OPENR_TRY(resolve_units(cnt[1], 0));
      *solved = cnt[0];
      return hipSuccess;
    }
  }
  const size_t units = (size_t)n_links * n_src;
  OPENR_TRY(d.wsrc.reserve(units));
  OPENR_TRY(d.wlink.reserve(units));
  OPENR_TRY(d.wunit.reserve(units));
  OPENR_TRY(d.wcount.reserve(1));
  const uint64_t* filter_tight = (exact && !ctx->metric_ok && use_link_metric) ? nullptr : d.base_tight.p;
  OPENR_TRY(launch_whatif_filter(d.g, d_links, n_links, d_sources, n_src, filter_tight, d_changed, d.wsrc.p,
                                 d.wlink.p, d.wunit.p, d.wcount.p, d.num_cus, s));
  uint32_t count = 0;
  OPENR_TRY(hipMemcpyAsync(&count, d.wcount.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  OPENR_TRY(hipStreamSynchronize(s));
  *solved = count;
  if (!count) return hipSuccess;
  // OPENR_SPF_WHATIF=incr: one wavefront per affected unit repairs it from the base rows it
  // re-reads (A set, distances inside A, dirty next hops); =solve re-solves every unit
  if (!exact && !dl.node && !(mode && !std::strcmp(mode, "solve")) && whatif_incr_lds_bytes(V, nb, dist64)) {
    return launch_whatif_incr(d.g, d.wsrc.p, d.wlink.p, d.wunit.p, count, n_src, d.base_dist.p, d.base_nh.p, nb,
                              !use_link_metric, dist64, d_changed, d.work.p + kIncrCtr, d.num_cus, s);
  }
  return resolve_units(count, 0);
}

// Link-set what-if sweep on one device (openr_spf_whatif_sets; whatif_set_filter in
// spf_sweep.hip has the unit semantics): unit (i, j) fails every link of set i =
// d_set_links[d_set_ptr[i], d_set_ptr[i + 1]) for d_sources[j]. Base SPF with tight edges ->
// set filter (source-major work list that points each affected unit at its set) -> the
// count read back (one stream sync) -> chunked re-solves with the unit's set as ignore set:
// on the rounds plan seeded from the base rows with the compare and the delta fused, on
// every other plan (BFS families, fringe, exact order) plain solves + rows_compare.
// Neither the grouped nor the incremental repair is set-aware: every affected unit is
// re-solved.
hipError_t whatif_sets_on_device(openr_spf_ctx* ctx, Device& d, const Plan& base_plan, const Plan& ign_plan,
                                 const uint32_t* d_set_ptr, const uint32_t* d_set_links, uint32_t n_sets,
                                 uint32_t n_set_links, const uint32_t* d_sources, uint32_t n_src, uint32_t* d_changed,
                                 hipStream_t s,
                                 uint32_t* solved, bool use_link_metric, const WhatifDelta& dl = WhatifDelta{}) {
  *solved = 0;
  if (!n_src || !n_sets) return hipSuccess;
  const size_t units = (size_t)n_sets * n_src;
  if (units > 0xFFFFFFFFull) return hipErrorInvalidValue;  // unit ids are u32
  hipError_t err;
  bool base_tin = false;
  OPENR_TRY(whatif_base_solve(ctx, d, base_plan, d_sources, n_src, s, &base_tin));
  OPENR_TRY(d.wsrc.reserve(units));
  OPENR_TRY(d.wunit.reserve(units));
  OPENR_TRY(d.wbeg.reserve(units));
  OPENR_TRY(d.wend.reserve(units));
  OPENR_TRY(d.wcount.reserve(1));
  // zero or wrapped metrics on an exact-order plan: the pop order depends on every
  // relaxation, so every unit whose set holds a link of the graph is re-solved
  const bool exact = base_plan.exact || ign_plan.exact;
  const uint64_t* filter_tight = (exact && !ctx->metric_ok && use_link_metric) ? nullptr : d.base_tight.p;
  OPENR_TRY(launch_whatif_set_filter(d.g, d_set_ptr, d_set_links, n_sets, n_set_links, d_sources, n_src, filter_tight, d_changed,
                                     d.wsrc.p, d.wunit.p, d.wbeg.p, d.wend.p, d.wcount.p, d.num_cus, s));
  uint32_t count = 0;
  OPENR_TRY(hipMemcpyAsync(&count, d.wcount.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  OPENR_TRY(hipStreamSynchronize(s));
  *solved = count;
  if (!count) return hipSuccess;
  return whatif_resolve_units(ctx, d, ign_plan, count, 0, d_set_links, n_src, base_tin, d_changed, dl, s);
}
#undef OPENR_TRY

// Bytes of second-SPF distance rows a KSP2 batch may hold on a device at once.
constexpr size_t kKspChunkBytes = size_t(8) << 30;  // second-SPF rows + ignore slots per chunk

// getKthPaths(src, dest, 1) and (.., 2) for a batch of pairs on one device: the base SPF
// of every listed source (the reference's memoized getSpfResult), then per chunk of
// pairs: k = 1 trace on the base rows (its links become the pair's ignore set), the
// second SPF with that ignore set (runSpf(src, true, ignore)), the k = 2 trace.
// Sets *overflow when a pair's paths exceed tok_cap tokens or kKspMaxDepth - 1 hops, or its
// trace kKspArena pathLinks on the DFS stack.
hipError_t ksp2_on_device(openr_spf_ctx* ctx, Device& d, const Plan& base_plan, const Plan& ign_plan,
                          const uint32_t* d_sources, uint32_t n_src, const uint32_t* d_prow, const uint32_t* d_pdst,
                          uint32_t n_pairs, uint32_t tok_cap, uint32_t* d_tok1, uint32_t* d_tok2, hipStream_t s,
                          bool* overflow) {
  const uint32_t V = ctx->V;
  *overflow = false;
  if (!n_pairs) return hipSuccess;
  hipError_t err;
#define OPENR_TRY(x)                   \
  do {                                 \
    err = (x);                         \
    if (err != hipSuccess) return err; \
  } while (0)
  OPENR_TRY(reserve_counters(d));
  OPENR_TRY(d.kbase.reserve((size_t)n_src * V));
  OPENR_TRY(d.kstatus.reserve(1));
  OPENR_TRY(hipMemsetAsync(d.kstatus.p, 0, sizeof(uint32_t), s));
  SolveArgs a{};
  a.sources = d_sources;
  a.n = n_src;
  a.dist = d.kbase.p;
  a.nh_bits = ctx->nh_bits;
  OPENR_TRY(d.ovf.reserve((size_t)n_src * ctx->nsl_max()));
  a.ovf_list = d.ovf.p;
  a.work = d.work.p;
  OPENR_TRY(launch(ctx, d, base_plan, a, s));
  // uniform cost: the base rows' pathLinks as lists, read by the k = 1 trace's frames
  // (a list read instead of a record row plus its tails' distances); up to 16 GiB
  const uint32_t* tl_off = nullptr;
  const uint2* tl_ent = nullptr;
  if (base_plan.bfs && base_plan.cost && ksp_path_lists_ok(d.g) &&
      (size_t)n_src * d.g.E * sizeof(uint2) <= (size_t(16) << 30)) {
    if (d.ktloff.reserve((size_t)n_src * (V + 1u)) == hipSuccess &&
        d.ktlent.reserve((size_t)n_src * d.g.E) == hipSuccess) {
      OPENR_TRY(launch_ksp_path_lists(d.g, d_sources, n_src, d.kbase.p, d.ktloff.p, d.ktlent.p, d.num_cus, s));
      tl_off = d.ktloff.p;
      tl_ent = d.ktlent.p;
    } else {
      (void)hipGetLastError();  // no room: the trace gathers from the records
    }
  }
  // the k = 2 trace also reads them where its pair's row keeps the base distance (same
  // uniform cost in both solves); OPENR_SPF_KSP_TL2=0: record rows only (A/B, tests)
  const char* tl2_env = std::getenv("OPENR_SPF_KSP_TL2");
  const uint32_t* tl2_off = tl_off && ign_plan.bfs && ign_plan.cost == base_plan.cost &&
                                    !(tl2_env && std::atoi(tl2_env) == 0)
                                ? tl_off
                                : nullptr;
  const uint32_t ign_cap = tok_cap;  // the k = 1 paths' links fit their tokens (slot; ends in kend)
  // the second SPF as a repair of the base rows (launch_ksp_repair): needs the k = 2 lists'
  // conditions, tagged rows, and a level mask no real level reaches; OPENR_SPF_KSP_REPAIR=0:
  // the forward, target-bounded solve (A/B, tests)
  // uniform-cost second SPFs on the code family are distance-only: u16 level rows, tagged
  // (SolveArgs::lvl_tag: a solve writes only the nodes it settles — it stops at the pair's
  // target — and the trace reads other entries as unreached) when levels leave >= 2 tag bits
  const bool rows16 = ign_plan.bfs && ign_plan.family == kFamCode;
  uint32_t lshift = 1;
  while ((1u << lshift) < V) ++lshift;  // levels < V <= 2^lshift
  const uint32_t tag_max = lshift <= 14u ? (1u << (16u - lshift)) - 1u : 0u;
  const char* tag_env = std::getenv("OPENR_SPF_KSP_TAG");  // 0: untagged rows, unreached fill (A/B)
  const bool tagged = rows16 && tag_max && !(tag_env && std::atoi(tag_env) == 0);
  const size_t row_bytes = (size_t)V * (rows16 ? 2u : 8u);
  // pairs whose k = 2 answer is empty by construction skip the second SPF and the k = 2
  // trace (ksp_select_pairs); the code family's single-class distance-only launch takes
  // the kept list. OPENR_SPF_KSP_SKIP=0: every pair solved and traced (A/B, tests).
  const char* skip_env = std::getenv("OPENR_SPF_KSP_SKIP");
  const bool skip = rows16 && !(skip_env && std::atoi(skip_env) == 0);
  const char* rep_env = std::getenv("OPENR_SPF_KSP_REPAIR");
  const bool repair = tagged && tl_off && ign_plan.bfs && ign_plan.cost == base_plan.cost && (1u << lshift) > V && ksp_repair_lds_bytes(V, d.g.L) != 0u &&
                      !(rep_env && std::atoi(rep_env) == 0);
  // pairs per chunk from a byte budget for the chunk's rows and ignore slots: 8 GiB of the
  // 288 GB, capped at half the device memory free at the call, and halved again
  // when a reservation still fails. Fabric, 512 sources x all destinations, ms per step by
  // budget: 2 GiB (~150 k pairs) 254.3, 4 GiB 248.3, 8 GiB 246.8, 16 GiB 246.4; by pairs:
  // 65 536 271.6, 32 768 297.0, 16 384 351.0, 8 192 470.8. Per-chunk launches and kernel
  // tails dominate, not the rows' cache locality. (Two pipeline lanes alternating chunks
  // over two streams measured slower, 264.7 vs 254.2 ms: each chunk's kernels already fill
  // the GPU; removed in round 4.)
  size_t chunk_budget = kKspChunkBytes;
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
      chunk_budget = std::min(chunk_budget, std::max<size_t>(free_b / 2u, size_t(64) << 20));
  }
  uint32_t chunk =
      (uint32_t)std::min<size_t>(n_pairs, std::max<size_t>(1, chunk_budget / (row_bytes + 4u * ign_cap)));
  if (const char* e = std::getenv("OPENR_SPF_KSP_CHUNK"))  // pairs per chunk (tests: many chunks, tag wrap)
    if (std::atoi(e) > 0) chunk = std::min<uint32_t>(chunk, (uint32_t)std::atoi(e));
  auto reserve_chunk = [&](uint32_t c) -> hipError_t {
    hipError_t e2;
    if ((e2 = d.kptr.reserve((size_t)c + 1u)) != hipSuccess) return e2;
    if (rows16) {
      if ((e2 = d.krows16.reserve((size_t)c * V)) != hipSuccess) return e2;
    } else if ((e2 = d.krows.reserve((size_t)c * V)) != hipSuccess) {
      return e2;
    }
    if ((e2 = d.kign.reserve((size_t)c * ign_cap)) != hipSuccess) return e2;
    if ((e2 = d.kend.reserve(c)) != hipSuccess) return e2;
    if ((e2 = d.kq.reserve((size_t)ksp_max_grid(d.g, d.num_cus) * (V + (V + 31u) / 32u))) != hipSuccess) return e2;
    if ((e2 = d.ksrc.reserve(c)) != hipSuccess) return e2;
    if ((e2 = d.ovf.reserve((size_t)c * ctx->nsl_max())) != hipSuccess) return e2;
    if (skip && (e2 = d.kkeep.reserve(c)) != hipSuccess) return e2;
    if ((e2 = d.kpart.reserve(4u * kMaxClasses)) != hipSuccess) return e2;
    return d.kretry.reserve(8u + 4u * (size_t)c);
  };
  for (;;) {
    err = reserve_chunk(chunk);
    if (err != hipErrorOutOfMemory || chunk == 1) break;
    (void)hipGetLastError();  // clear the failed allocation
    chunk = (chunk + 1u) / 2u;
  }
  if (err != hipSuccess) return err;
  OPENR_TRY(launch_strided_iota(d.kptr.p, chunk + 1u, ign_cap, d.num_cus, s));
  if (tagged && d.ktag_rows < (size_t)chunk * V) {  // fresh or grown buffer: no valid tag in it
    OPENR_TRY(hipMemsetAsync(d.krows16.p, 0, (size_t)chunk * V * sizeof(uint16_t), s));
    d.ktag_rows = (size_t)chunk * V;
    d.ktag = 0;
  }
  // OPENR_SPF_PROF=1: per-kind trace counters printed to stderr (tuning only)
  const uint32_t nst = ksp_stats_count();
  unsigned long long* kst = nullptr;
  if (prof_enabled()) {
    // ... and, after them, the pairs the repair kernel kept / handed to the forward solve
    OPENR_TRY(hipMallocAsync(reinterpret_cast<void**>(&kst), (2 * nst + 2) * sizeof(unsigned long long), s));
    OPENR_TRY(hipMemsetAsync(kst, 0, (2 * nst + 2) * sizeof(unsigned long long), s));
  }
  for (uint32_t first = 0; first < n_pairs; first += chunk) {
    const uint32_t m = std::min(chunk, n_pairs - first);
    hipStream_t ls = s;
    uint32_t* rcount = d.kretry.p;  // [0] k = 1, [1] k = 2; [2..5] work counters of the 4 launches
    uint32_t* wctr = d.kretry.p + 2;
    uint32_t* rlist1 = d.kretry.p + 8;
    uint32_t* rlist2 = rlist1 + chunk;
    uint32_t* rlist3 = rlist2 + chunk;  // repaired second SPFs handed to the forward solve
    uint32_t* rmode = rlist3 + chunk;   // per pair: 0 repaired row, 1 forward row
    uint32_t* rpart3 = d.kpart.p + 2u * kMaxClasses;  // rlist3's count as the kCls8 partition
    OPENR_TRY(hipMemsetAsync(rcount, 0, 8u * sizeof(uint32_t), ls));
    // small tier (occupancy), then the full tier over the pairs it could not hold
    OPENR_TRY(launch_ksp_trace(1, d.g, d_sources, d_prow, d_pdst, first, m, d.kbase.p, d.kign.p, d.kend.p, ign_cap,
                               d_tok1, tok_cap, d.kstatus.p, d.kq.p, d.num_cus, ls, kst, nullptr, nullptr, rlist1,
                               rcount, wctr, nullptr, base_plan.bfs ? base_plan.cost : 0u, 0u, tl_off, tl_ent,
                               d.kbase.p));
    OPENR_TRY(launch_ksp_trace(1, d.g, d_sources, d_prow, d_pdst, first, m, d.kbase.p, d.kign.p, d.kend.p, ign_cap,
                               d_tok1, tok_cap, d.kstatus.p, d.kq.p, d.num_cus, ls, kst, rlist1, rcount, nullptr,
                               nullptr, wctr + 1, nullptr, base_plan.bfs ? base_plan.cost : 0u, 0u, tl_off, tl_ent,
                               d.kbase.p));
    const uint32_t* keep = nullptr;  // chunk-local pairs left for the second SPF (skip)
    const uint32_t* keep_count = nullptr;
    if (skip || repair) OPENR_TRY(hipMemsetAsync(d.kpart.p, 0, 4u * kMaxClasses * sizeof(uint32_t), ls));
    if (skip) {
      OPENR_TRY(launch_ksp_select_pairs(d.g, d_sources, d_prow, d_pdst, first, m, d_tok1, d_tok2, tok_cap, d.ksrc.p,
                                        d.kkeep.p, d.kpart.p + kCls8, d.num_cus, ls));
      keep = d.kkeep.p;
      keep_count = d.kpart.p + kCls8;
    } else {
      OPENR_TRY(launch_gather_sources(d_sources, d_prow, first, m, d.ksrc.p, d.num_cus, ls));
    }
    SolveArgs b{};
    b.sources = d.ksrc.p;
    b.n = m;
    b.perm = keep;  // launch(): the distance-only class runs over keep[0 .. *keep_count)
    b.part = skip ? d.kpart.p : nullptr;
    b.ign_ptr = d.kptr.p;  // pair k ignores kign[k * ign_cap, kend[k])
    b.ign_end = d.kend.p;
    b.ign_links = d.kign.p;
    b.dist = rows16 ? nullptr : d.krows.p;
    b.lvl16 = rows16 ? d.krows16.p : nullptr;
    uint32_t& tag = d.ktag;  // the tag of the last chunk written into this lane's rows (0: rows all zero)
    if (tagged) {
      if (tag == tag_max) {  // every tag used since the rows were zeroed: zero them again
        OPENR_TRY(hipMemsetAsync(d.krows16.p, 0, d.ktag_rows * sizeof(uint16_t), ls));
        tag = 0;
      }
      b.lvl_tag = ++tag;
      b.lvl_shift = lshift;
    }
    b.nh_bits = ctx->nh_bits;
    b.ovf_list = d.ovf.p;
    b.work = d.work.p;
    b.target = d_pdst + first;  // the k = 2 trace reads nodes no farther than dest
    if (repair) {
      OPENR_TRY(launch_ksp_repair(d.g, b.sources, d_prow + first, b.target, keep, keep_count, m, b.ign_ptr, b.ign_end,
                                  b.ign_links, d.kbase.p, tl_off, base_plan.cost, b.lvl16, b.lvl_tag << b.lvl_shift,
                                  (1u << b.lvl_shift) - 1u, rmode, rlist3, rpart3 + kCls8, d.kretry.p + 6,
                                  d.num_cus, ls));
      if (kst) OPENR_TRY(launch_ksp_repair_count(rmode, keep, keep_count, m, kst + 2 * nst, d.num_cus, ls));
      b.perm = rlist3;  // the pairs it handed back: the forward solve
      b.part = rpart3;
    }
    OPENR_TRY(launch(ctx, d, ign_plan, b, ls));
    const uint64_t* r2 = rows16 ? nullptr : d.krows.p;
    const uint16_t* r16 = rows16 ? d.krows16.p : nullptr;
    OPENR_TRY(launch_ksp_trace(2, d.g, d_sources, d_prow, d_pdst, first, m, r2, d.kign.p, d.kend.p, ign_cap, d_tok2,
                               tok_cap, d.kstatus.p, d.kq.p, d.num_cus, ls, kst ? kst + nst : nullptr, keep, keep_count,
                               rlist2, rcount + 1, wctr + 2, r16, ign_plan.bfs ? ign_plan.cost : 0u,
                               tagged ? (b.lvl_tag << 8 | lshift) : 0u, tl2_off, tl_ent, d.kbase.p,
                               repair ? rmode : nullptr));
    OPENR_TRY(launch_ksp_trace(2, d.g, d_sources, d_prow, d_pdst, first, m, r2, d.kign.p, d.kend.p, ign_cap, d_tok2,
                               tok_cap, d.kstatus.p, d.kq.p, d.num_cus, ls, kst ? kst + nst : nullptr, rlist2,
                               rcount + 1, nullptr, nullptr, wctr + 3, r16, ign_plan.bfs ? ign_plan.cost : 0u,
                               tagged ? (b.lvl_tag << 8 | lshift) : 0u, tl2_off, tl_ent, d.kbase.p,
                               repair ? rmode : nullptr));
  }
  if (kst) {
    std::vector<unsigned long long> h(2 * nst + 2);
    OPENR_TRY(hipMemcpyAsync(h.data(), kst, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    OPENR_TRY(hipStreamSynchronize(s));
    OPENR_TRY(hipFree(kst));
    for (int k = 0; k < 2; ++k) {
      std::fprintf(stderr, "ksp_stats k=%d", k + 1);
      for (uint32_t i = 0; i < nst; ++i) std::fprintf(stderr, " %llu", h[k * nst + i]);
      std::fprintf(stderr, "\n");
    }
    // second SPFs by the way they were solved, summed over the chunks (both 0: no repair launch)
    std::fprintf(stderr, "ksp_repair kept=%llu forward=%llu\n", h[2 * nst], h[2 * nst + 1]);
  }
  uint32_t status = 0;
  OPENR_TRY(hipMemcpyAsync(&status, d.kstatus.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  OPENR_TRY(hipStreamSynchronize(s));
  *overflow = status != 0;
#undef OPENR_TRY
  return hipSuccess;
}

// The first check of the what-if, event, route and LFA calls.
int check_ctx(const openr_spf_ctx* ctx) {
  if (!ctx) return fail(OPENR_SPF_EINVAL, "null context");
  if (!ctx->has_graph) return fail(OPENR_SPF_EINVAL, "no graph set (openr_spf_set_graph)");
  return OPENR_SPF_OK;
}

int check_device_index(const openr_spf_ctx* ctx, int device_index) {
  if (device_index < 0 || device_index >= (int)ctx->devs.size())
    return fail(OPENR_SPF_EINVAL, "device_index %d out of range", device_index);
  return OPENR_SPF_OK;
}

int whatif_plans(openr_spf_ctx* ctx, uint32_t flags, Plan* base_plan, Plan* ign_plan) {
  int rc = make_plan(ctx, flags, false, base_plan);
  if (rc) return rc;
  return make_plan(ctx, flags, true, ign_plan);
}

// The failure units of a what-if sweep on one device: n single links (links), or n link
// sets in CSR form (set_ptr != nullptr: set i = set_links[set_ptr[i], set_ptr[i + 1])).
// Or n drain events (node_ptr != nullptr: event i overloads nodes[node_ptr[i], node_ptr[i + 1])
// and takes set_links[set_ptr[i], set_ptr[i + 1]) out of service; set_ptr null: no links).
struct WhatifUnits {
  const uint32_t* links = nullptr;
  const uint32_t* set_ptr = nullptr;
  const uint32_t* set_links = nullptr;
  uint32_t n_set_links = 0;  // entries of set_links (the filter clamps every slice to them)
  uint32_t n = 0;
  const uint32_t* node_ptr = nullptr;
  const uint32_t* nodes = nullptr;
  uint32_t n_nodes = 0;  // entries of nodes
  // metric events (edge_ptr != nullptr): event i gives edges[k] the metric metrics[k] for k in
  // [edge_ptr[i], edge_ptr[i + 1])
  const uint32_t* edge_ptr = nullptr;
  const uint32_t* edges = nullptr;
  const uint32_t* metrics = nullptr;
  uint32_t n_edges = 0;  // entries of edges / metrics
  // restore events: the three CSRs above together (node_ptr set; set_ptr / edge_ptr nullable),
  // the nodes undrained, the links put back, the metrics lowered
  bool restore = false;
  // maintenance events: the three CSRs together as well, the nodes overloaded, the links taken
  // out of service, the metrics raised
  bool maint = false;
};

// Event sweep on one device (openr_spf_whatif_drain / _metric / _restore; spf_drain.hip,
// spf_metric.hip and spf_restore.hip have the unit semantics): base SPF with tight edges ->
// the filter (source-major list of the units the event can change: a hit base-tight edge, or
// for a restore an improved edge that reaches its head) -> the count read back (one stream sync) -> the repair,
// one workgroup per listed unit on the base rows -> the units that outgrew its slots (a
// second 4-byte read) through the same kernel with a slot per node. `p` arrives with its
// event CSR filled; the common part is filled here. The caller has checked the plan and the
// LDS sizes (check_repair_sweep).
template <class Pass>
hipError_t whatif_repair_on_device(openr_spf_ctx* ctx, Device& d, const Plan& base_plan, Pass& p, uint32_t n_events,
                                   uint32_t ctr, hipError_t (*filter)(const DevGraph&, const Pass&, int, hipStream_t),
                                   hipError_t (*repair)(const DevGraph&, const Pass&, uint32_t, bool, int, hipStream_t),
                                   const uint32_t* d_sources, uint32_t n_src, uint32_t* d_changed, hipStream_t s,
                                   uint32_t* solved, const WhatifDelta& dl) {
  *solved = 0;
  if (!n_src || !n_events) return hipSuccess;
  const size_t units = (size_t)n_events * n_src;
  if (units > 0xFFFFFFFFull || base_plan.exact) return hipErrorInvalidValue;
  hipError_t err;
#define OPENR_TRY(x)                   \
  do {                                 \
    if ((err = (x)) != hipSuccess) return err; \
  } while (0)
  bool base_tin = false;
  OPENR_TRY(whatif_base_solve(ctx, d, base_plan, d_sources, n_src, s, &base_tin));
  OPENR_TRY(d.wunit.reserve(units));
  OPENR_TRY(d.wsrc.reserve(units));
  OPENR_TRY(d.wcount.reserve(3));
  p.n_events = n_events;
  p.n_src = n_src;
  p.nb = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  p.sources = d_sources;
  p.base_dist = d.base_dist.p;
  p.base_nh = d.base_nh.p;
  p.base_tight = d.base_tight.p;
  p.base_tin = base_tin ? d.base_tin.p : nullptr;
  p.changed = d_changed;
  p.wunit = d.wunit.p;
  p.ovf_unit = d.wsrc.p;
  p.wcount = d.wcount.p;
  p.ctr = d.work.p + ctr;
  p.delta = dl;
  OPENR_TRY(filter(d.g, p, d.num_cus, s));
  uint32_t count = 0;
  OPENR_TRY(hipMemcpyAsync(&count, d.wcount.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  OPENR_TRY(hipStreamSynchronize(s));
  *solved = count;
  if (!count) return hipSuccess;
  OPENR_TRY(repair(d.g, p, count, false, d.num_cus, s));
  uint32_t over = 0;
  OPENR_TRY(hipMemcpyAsync(&over, d.wcount.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  OPENR_TRY(hipStreamSynchronize(s));
  if (over) OPENR_TRY(repair(d.g, p, over, true, d.num_cus, s));
#undef OPENR_TRY
  return hipSuccess;
}

// The event CSRs of `un` into a pass struct, each where the struct has it: the node and link
// CSRs (with unit_cost) of a drain, restore or maintenance pass ...
template <class Pass>
void fill_node_link_csrs(Pass& p, const WhatifUnits& un, bool use_link_metric) {
  p.n_nodes = un.n_nodes;
  p.n_links = un.n_set_links;
  p.unit_cost = use_link_metric ? 0u : 1u;
  p.node_ptr = un.node_ptr;
  p.nodes = un.nodes;
  p.link_ptr = un.set_ptr;
  p.links = un.set_links;
}

// ... and the edge CSR of a metric, restore or maintenance pass.
template <class Pass>
void fill_edge_csr(Pass& p, const WhatifUnits& un) {
  p.n_edges = un.n_edges;
  p.edge_ptr = un.edge_ptr;
  p.edges = un.edges;
  p.metrics = un.metrics;
}

hipError_t whatif_drain_on_device(openr_spf_ctx* ctx, Device& d, const Plan& base_plan, const WhatifUnits& un,
                                  const uint32_t* d_sources, uint32_t n_src, uint32_t* d_changed, hipStream_t s,
                                  uint32_t* solved, bool use_link_metric, const WhatifDelta& dl) {
  DrainPass p{};
  fill_node_link_csrs(p, un, use_link_metric);
  return whatif_repair_on_device(ctx, d, base_plan, p, un.n, kDrainCtr, launch_drain_filter, launch_drain_repair,
                                 d_sources, n_src, d_changed, s, solved, dl);
}

// The caller serves the hop-count form itself: metrics do not enter it.
hipError_t whatif_metric_on_device(openr_spf_ctx* ctx, Device& d, const Plan& base_plan, const WhatifUnits& un,
                                   const uint32_t* d_sources, uint32_t n_src, uint32_t* d_changed, hipStream_t s,
                                   uint32_t* solved, bool use_link_metric, const WhatifDelta& dl) {
  *solved = 0;
  if (n_src && un.n && !use_link_metric) return hipErrorInvalidValue;
  MetricPass p{};
  fill_edge_csr(p, un);
  return whatif_repair_on_device(ctx, d, base_plan, p, un.n, kMetricCtr, launch_metric_filter, launch_metric_repair,
                                 d_sources, n_src, d_changed, s, solved, dl);
}

hipError_t whatif_restore_on_device(openr_spf_ctx* ctx, Device& d, const Plan& base_plan, const WhatifUnits& un,
                                    const uint32_t* d_sources, uint32_t n_src, uint32_t* d_changed, hipStream_t s,
                                    uint32_t* solved, bool use_link_metric, const WhatifDelta& dl) {
  RestorePass p{};
  fill_node_link_csrs(p, un, use_link_metric);
  fill_edge_csr(p, un);
  return whatif_repair_on_device(ctx, d, base_plan, p, un.n, kRestoreCtr, launch_restore_filter,
                                 launch_restore_repair, d_sources, n_src, d_changed, s, solved, dl);
}

hipError_t whatif_maint_on_device(openr_spf_ctx* ctx, Device& d, const Plan& base_plan, const WhatifUnits& un,
                                  const uint32_t* d_sources, uint32_t n_src, uint32_t* d_changed, hipStream_t s,
                                  uint32_t* solved, bool use_link_metric, const WhatifDelta& dl) {
  MaintPass p{};
  fill_node_link_csrs(p, un, use_link_metric);
  fill_edge_csr(p, un);
  return whatif_repair_on_device(ctx, d, base_plan, p, un.n, kMaintCtr, launch_maint_filter, launch_maint_repair,
                                 d_sources, n_src, d_changed, s, solved, dl);
}

// Plan and capacity checks of the drain and metric calls (`word`): the repair reads base_tight
// rows, which the exact-order kernel's history-dependent pop order does not give a meaning the
// rule can use. lds(V, dim, S, nb) is the kind's LDS size, dim its L or E (`dim_name`).
template <class Lds>
int check_repair_sweep(const openr_spf_ctx* ctx, uint32_t flags, uint64_t n_events, uint64_t n_sources,
                       const char* word, Lds&& lds, uint32_t slots, char dim_name, uint32_t dim) {
  if (n_events * n_sources > 0xFFFFFFFFull) return fail(OPENR_SPF_EINVAL, "more than 2^32 - 1 units");
  Plan bp;
  int rc = make_plan(ctx, flags, false, &bp);
  if (rc) return rc;
  if (bp.exact)
    return fail(OPENR_SPF_ENOTSUP, "%s sweep needs a base plan outside the exact-order kernel (usable metrics in "
                                   "[1, 2^31-1] under link metric, next-hop sets <= 256 bits)", word);
  const uint32_t nb = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  if (!lds(ctx->V, dim, std::min(slots, ctx->V), nb) || !lds(ctx->V, dim, ctx->V, nb))
    return fail(OPENR_SPF_E2BIG, "a %s unit's state does not fit LDS (V=%u, %c=%u)", word, ctx->V, dim_name, dim);
  return OPENR_SPF_OK;
}

int check_drain(const openr_spf_ctx* ctx, uint32_t flags, uint64_t n_events, uint64_t n_sources) {
  return check_repair_sweep(ctx, flags, n_events, n_sources, "drain", drain_lds_bytes, drain_slots(), 'L', ctx->L);
}

int check_metric(const openr_spf_ctx* ctx, uint32_t flags, uint64_t n_events, uint64_t n_sources) {
  return check_repair_sweep(ctx, flags, n_events, n_sources, "metric", metric_lds_bytes, metric_slots(), 'E', ctx->E);
}

int check_restore(const openr_spf_ctx* ctx, uint32_t flags, uint64_t n_events, uint64_t n_sources) {
  const uint32_t L = ctx->L;
  return check_repair_sweep(
      ctx, flags, n_events, n_sources, "restore",
      [L](uint32_t V, uint32_t E, uint32_t S, uint32_t nb) { return restore_lds_bytes(V, L, E, S, nb); },
      restore_slots(), 'E', ctx->E);
}

int check_maint(const openr_spf_ctx* ctx, uint32_t flags, uint64_t n_events, uint64_t n_sources) {
  const uint32_t L = ctx->L;
  return check_repair_sweep(
      ctx, flags, n_events, n_sources, "maintenance",
      [L](uint32_t V, uint32_t E, uint32_t S, uint32_t nb) { return maint_lds_bytes(V, L, E, S, nb); },
      maint_slots(), 'E', ctx->E);
}

hipError_t whatif_units_on_device(openr_spf_ctx* ctx, Device& d, const Plan& bp, const Plan& ip, const WhatifUnits& un,
                                  const uint32_t* d_sources, uint32_t n_src, uint32_t* d_changed, hipStream_t s,
                                  uint32_t* solved, bool use_link_metric, const WhatifDelta& dl = WhatifDelta{}) {
  if (un.restore)
    return whatif_restore_on_device(ctx, d, bp, un, d_sources, n_src, d_changed, s, solved, use_link_metric, dl);
  if (un.maint)
    return whatif_maint_on_device(ctx, d, bp, un, d_sources, n_src, d_changed, s, solved, use_link_metric, dl);
  if (un.edge_ptr)
    return whatif_metric_on_device(ctx, d, bp, un, d_sources, n_src, d_changed, s, solved, use_link_metric, dl);
  if (un.node_ptr)
    return whatif_drain_on_device(ctx, d, bp, un, d_sources, n_src, d_changed, s, solved, use_link_metric, dl);
  if (un.set_ptr)
    return whatif_sets_on_device(ctx, d, bp, ip, un.set_ptr, un.set_links, un.n, un.n_set_links, d_sources, n_src, d_changed, s,
                                 solved, use_link_metric, dl);
  return whatif_on_device(ctx, d, bp, ip, un.links, un.n, d_sources, n_src, d_changed, s, solved, use_link_metric, dl);
}

// openr_spf_whatif[_sets]_delta[_device] on one device: the sweep with the delta into library
// scratch (per-unit slots, WhatifDelta), the exclusive scan of changed into d_ptr, then
// (when the total fits `cap`) every unit's entries gathered into the caller's CSR arrays.
// Synchronizes s. *total = sum(changed); OPENR_SPF_E2BIG when it exceeds cap.
int whatif_delta_on_device(openr_spf_ctx* ctx, Device& d, const WhatifUnits& un, const uint32_t* d_sources, uint32_t n_src, uint32_t flags, uint32_t* d_changed,
                           uint64_t* d_ptr, uint32_t* d_node, unsigned long long* d_dist, uint8_t* d_nh, uint64_t cap,
                           uint32_t nhb, hipStream_t s, uint64_t* total, uint64_t* solved_out,
                           uint64_t* pool_need = nullptr) {
  const uint32_t nb = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  if (nhb < nb) return fail(OPENR_SPF_EINVAL, "nh_bytes %u below the graph's next-hop width %u", nhb, nb);
  Plan bp, ip;
  int rc = whatif_plans(ctx, flags, &bp, &ip);
  if (rc) return rc;
  const size_t units = (size_t)un.n * n_src;
  *total = 0;
  *solved_out = 0;
  unsigned long long* ptr = reinterpret_cast<unsigned long long*>(d_ptr);
  if (!units) {
    HIP_TRY(hipMemsetAsync(ptr, 0, sizeof(unsigned long long), s));
    HIP_TRY(hipStreamSynchronize(s));
    return OPENR_SPF_OK;
  }
  // scratch pool: room for the caller's cap twice over (gaps of the waves' slot blocks,
  // grp_repair) plus one block per resident wave, at most 2^32 - 1 slots
  const uint64_t want = std::min<uint64_t>(2u * cap + (uint64_t)d.num_cus * 32u * 256u + 1024u, 0xFFFFFFFFull);
  HIP_TRY(d.dl_off.reserve(units));
  HIP_TRY(d.dl_node.reserve(want));
  HIP_TRY(d.dl_dist.reserve(want));
  HIP_TRY(d.dl_nh.reserve(want * nhb));
  HIP_TRY(d.dl_used.reserve(1));
  HIP_TRY(d.dl_tsum.reserve(units / 4096u + 1u));
  HIP_TRY(hipMemsetAsync(d.dl_used.p, 0, sizeof(unsigned long long), s));
  WhatifDelta dl;
  dl.off = d.dl_off.p;
  dl.node = d.dl_node.p;
  dl.dist = d.dl_dist.p;
  dl.nh = d.dl_nh.p;
  dl.cap = (uint32_t)want;
  dl.nhb = nhb;
  dl.used = d.dl_used.p;
  // drain / metric / restore / maintenance sweep, counts and ptr only: the repair writes no entries
  if ((un.node_ptr || un.edge_ptr || un.maint) && !cap) dl.node = nullptr;
  uint32_t solved = 0;
  HIP_TRY(whatif_units_on_device(ctx, d, bp, ip, un, d_sources, n_src, d_changed, s, &solved,
                                 (flags & OPENR_SPF_USE_LINK_METRIC) != 0, dl));
  HIP_TRY(launch_delta_scan(d_changed, units, d.dl_tsum.p, ptr, s));
  unsigned long long tu[2] = {0, 0};  // total entries, pool slots used
  HIP_TRY(hipMemcpyAsync(&tu[0], ptr + units, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&tu[1], d.dl_used.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *total = tu[0];
  *solved_out = (uint64_t)solved + n_src;
  if (pool_need) *pool_need = tu[1];  // scratch slots the sweep asked for (the route pass sizes its rerun from it)
  ctx->stats.spf_runs += *solved_out;
  ctx->stats.batches += 1;
  if (tu[1] > want)
    return fail(OPENR_SPF_E2BIG, "delta needs %llu entries (%llu pool slots; scratch %llu for cap %llu)", tu[0], tu[1],
                (unsigned long long)want, (unsigned long long)cap);
  if (tu[0] > cap) return fail(OPENR_SPF_E2BIG, "delta needs %llu entries, cap %llu", tu[0], (unsigned long long)cap);
  HIP_TRY(launch_delta_gather(d_changed, units, d.dl_off.p, ptr, dl, d_node, d_dist, d_nh, d.num_cus, s));
  HIP_TRY(hipStreamSynchronize(s));
  return OPENR_SPF_OK;
}

// One CSR of host units: ptr ascends over the n slices, the values are there when a slice is
// not empty (vals_given: every array the CSR needs), every value is below `bound`. `what`
// names the values in the messages.
int check_host_csr(const char* what, const uint32_t* ptr, uint32_t n, const uint32_t* vals, bool vals_given,
                   uint32_t bound) {
  for (uint32_t i = 0; i < n; ++i)
    if (ptr[i + 1] < ptr[i]) return fail(OPENR_SPF_EINVAL, "%s_ptr does not ascend at %u", what, i);
  if (ptr[n] > ptr[0] && !vals_given) return fail(OPENR_SPF_EINVAL, "null %s values", what);
  for (uint32_t k = ptr[0]; k < ptr[n]; ++k)
    if (vals[k] >= bound) return fail(OPENR_SPF_EINVAL, "%s %u out of range (%u of them)", what, vals[k], bound);
  return OPENR_SPF_OK;
}

// The rules of an edge CSR beyond check_host_csr: ids strictly ascending inside an event, and
// every new metric on the side of the current one that the kind allows. A restore event
// lowers, into [1, current]; a metric or maintenance event raises, into [current, 2^31-1].
int check_host_edges(const openr_spf_ctx* ctx, const WhatifUnits& hu) {
  for (uint32_t i = 0; i < hu.n; ++i)
    for (uint32_t k = hu.edge_ptr[i]; k < hu.edge_ptr[i + 1]; ++k) {
      const uint32_t e = hu.edges[k], m = hu.metrics[k];
      if (k > hu.edge_ptr[i] && e <= hu.edges[k - 1])
        return fail(OPENR_SPF_EINVAL, "event %u: edge ids are not strictly ascending", i);
      const uint64_t cur = ctx->metric[e];
      if (hu.restore ? (m > cur || m < 1u) : (m < cur || m > 0x7FFFFFFFu))
        return fail(OPENR_SPF_EINVAL,
                    "event %u: metric %u of edge %u is %s (a restore event lowers, openr_spf_whatif_restore; a metric "
                    "or maintenance event raises)",
                    i, m, e, hu.restore ? "above the current one or below 1" : "below the current one or above 2^31-1");
    }
  return OPENR_SPF_OK;
}

// Argument checks of the host what-if forms (hu in host memory). EINVAL only.
int check_whatif_host(const openr_spf_ctx* ctx, const WhatifUnits& hu, const uint32_t* sources, uint32_t n_sources,
                      const uint32_t* changed) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if ((hu.n && !hu.links && !hu.set_ptr && !hu.node_ptr && !hu.edge_ptr) || (n_sources && !sources) ||
      (hu.n && n_sources && !changed))
    return fail(OPENR_SPF_EINVAL, "null links, sources or changed");
  for (uint32_t i = 0; i < n_sources; ++i)
    if (sources[i] >= ctx->V) return fail(OPENR_SPF_EINVAL, "source %u out of range (V=%u)", sources[i], ctx->V);
  if (!hu.n) return OPENR_SPF_OK;
  if ((hu.restore || hu.maint) && !hu.node_ptr) return fail(OPENR_SPF_EINVAL, "null node_ptr");
  if (!hu.set_ptr && !hu.node_ptr && !hu.edge_ptr) {  // single links
    for (uint32_t i = 0; i < hu.n; ++i)
      if (hu.links[i] >= ctx->L) return fail(OPENR_SPF_EINVAL, "link %u out of range (L=%u)", hu.links[i], ctx->L);
    return OPENR_SPF_OK;
  }
  // sets: the link CSR; drain events: node and link CSR; metric events: the edge CSR; restore and
  // maintenance events: all three (the link and the edge CSR nullable wherever a node CSR leads)
  if (hu.node_ptr) rc = check_host_csr("node", hu.node_ptr, hu.n, hu.nodes, hu.nodes != nullptr, ctx->V);
  if (!rc && hu.set_ptr) rc = check_host_csr("link", hu.set_ptr, hu.n, hu.set_links, hu.set_links != nullptr, ctx->L);
  if (!rc && hu.edge_ptr) {
    rc = check_host_csr("edge", hu.edge_ptr, hu.n, hu.edges, hu.edges && hu.metrics, ctx->E);
    if (!rc) rc = check_host_edges(ctx, hu);
  }
  return rc;
}

// Units [b, b + m) of hu into the device's input buffers on its stream (*un: the device view).
// Single links are copied as they are. A CSR goes through `block`: its ptr rebased to the
// block's slice, the slice of its values behind it. Every CSR has buffers of its own (node:
// win_ptr / win_nodes, link: win_lptr / win_links, edge: win_eptr / win_edges / win_metrics).
int upload_whatif_units(Device& d, const WhatifUnits& hu, uint32_t b, uint32_t m, std::vector<uint32_t>* rebased,
                        WhatifUnits* un) {
  *un = WhatifUnits{};
  un->n = m;
  un->restore = hu.restore;
  un->maint = hu.maint;
  if (!hu.set_ptr && !hu.node_ptr && !hu.edge_ptr) {  // no rebase, so nothing to wait for
    HIP_TRY(d.win_links.reserve(m));
    HIP_TRY(hipMemcpyAsync(d.win_links.p, hu.links + b, m * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    un->links = d.win_links.p;
    return OPENR_SPF_OK;
  }
  auto block = [&](const uint32_t* ptr, const uint32_t* vals, const uint32_t* vals2, DevBuf<uint32_t>& dptr,
                   DevBuf<uint32_t>& dvals, DevBuf<uint32_t>* dvals2, uint32_t* count) -> int {
    const uint32_t b0 = ptr[b], e0 = ptr[b + m];
    rebased->resize(m + 1);
    for (uint32_t i = 0; i <= m; ++i) (*rebased)[i] = ptr[b + i] - b0;
    HIP_TRY(dptr.reserve(m + 1));
    HIP_TRY(dvals.reserve(std::max<uint32_t>(e0 - b0, 1u)));
    if (dvals2) HIP_TRY(dvals2->reserve(std::max<uint32_t>(e0 - b0, 1u)));
    HIP_TRY(hipMemcpyAsync(dptr.p, rebased->data(), (m + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    if (e0 > b0) {
      HIP_TRY(hipMemcpyAsync(dvals.p, vals + b0, (e0 - b0) * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
      if (dvals2)
        HIP_TRY(hipMemcpyAsync(dvals2->p, vals2 + b0, (e0 - b0) * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    }
    HIP_TRY(hipStreamSynchronize(d.stream));  // `rebased` is reused for the next CSR and the next device's block
    *count = e0 - b0;
    return OPENR_SPF_OK;
  };
  int rc;
  if (hu.node_ptr) {
    if ((rc = block(hu.node_ptr, hu.nodes, nullptr, d.win_ptr, d.win_nodes, nullptr, &un->n_nodes))) return rc;
    un->node_ptr = d.win_ptr.p;
    un->nodes = d.win_nodes.p;
  }
  if (hu.set_ptr) {
    if ((rc = block(hu.set_ptr, hu.set_links, nullptr, d.win_lptr, d.win_links, nullptr, &un->n_set_links))) return rc;
    un->set_ptr = d.win_lptr.p;
    un->set_links = d.win_links.p;
  }
  if (hu.edge_ptr) {
    if ((rc = block(hu.edge_ptr, hu.edges, hu.metrics, d.win_eptr, d.win_edges, &d.win_metrics, &un->n_edges))) return rc;
    un->edge_ptr = d.win_eptr.p;
    un->edges = d.win_edges.p;
    un->metrics = d.win_metrics.p;
  }
  return OPENR_SPF_OK;
}


// openr_spf_whatif / openr_spf_whatif_sets: units split in contiguous blocks across the devices
int whatif_host(openr_spf_ctx* ctx, const WhatifUnits& hu, const uint32_t* sources, uint32_t n_sources,
                uint32_t flags, uint32_t* changed, uint64_t* out_solved) {
  const uint32_t n_links = hu.n;
  int rc = check_whatif_host(ctx, hu, sources, n_sources, changed);
  if (rc) return rc;
  Plan bp, ip;
  rc = whatif_plans(ctx, flags, &bp, &ip);
  if (rc) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  // links (or sets) are split in contiguous blocks across the context's devices
  std::vector<uint32_t> rebased;
  const uint32_t nd = (uint32_t)ctx->devs.size();
  const uint32_t per = (n_links + nd - 1) / std::max<uint32_t>(nd, 1);
  uint64_t solved_total = 0;
  for (uint32_t di = 0; di < nd; ++di) {
    Device& d = ctx->devs[di];
    const uint32_t b = std::min(n_links, di * per), e = std::min(n_links, b + per), m = e - b;
    if (!m || !n_sources) continue;
    HIP_TRY(hipSetDevice(d.ordinal));
    WhatifUnits un;
    if ((rc = upload_whatif_units(d, hu, b, m, &rebased, &un)) != OPENR_SPF_OK) return rc;
    HIP_TRY(d.win_src.reserve(n_sources));
    HIP_TRY(d.wchanged.reserve((size_t)m * n_sources));
    HIP_TRY(hipMemcpyAsync(d.win_src.p, sources, n_sources * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    uint32_t solved = 0;
    HIP_TRY(whatif_units_on_device(ctx, d, bp, ip, un, d.win_src.p, n_sources, d.wchanged.p, d.stream, &solved,
                                   (flags & OPENR_SPF_USE_LINK_METRIC) != 0));
    HIP_TRY(hipMemcpyAsync(changed + (size_t)b * n_sources, d.wchanged.p, (size_t)m * n_sources * sizeof(uint32_t),
                           hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    solved_total += solved + n_sources;
  }
  ctx->stats.spf_runs += solved_total;
  ctx->stats.batches += 1;
  ctx->stats.last_batch_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (out_solved) *out_solved = solved_total;
  return OPENR_SPF_OK;
}

// openr_spf_whatif_delta / openr_spf_whatif_sets_delta
int whatif_delta_host(openr_spf_ctx* ctx, const WhatifUnits& hu, const uint32_t* sources, uint32_t n_sources,
                      uint32_t flags, uint32_t* changed, openr_spf_whatif_delta_t* delta, uint64_t* out_solved) {
  const uint32_t n_links = hu.n;
  if (!ctx) return fail(OPENR_SPF_EINVAL, "null context");
  if (!ctx->has_graph) return fail(OPENR_SPF_EINVAL, "no graph set (openr_spf_set_graph)");
  if (!delta || !delta->ptr) return fail(OPENR_SPF_EINVAL, "null delta or delta->ptr");
  int rc0 = check_whatif_host(ctx, hu, sources, n_sources, changed);
  if (rc0) return rc0;
  if (delta->cap && (!delta->node || !delta->dist || !delta->nh))
    return fail(OPENR_SPF_EINVAL, "null delta->node, dist or nh");
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t nhb = delta->nh_bytes;
  // links (or sets) split in contiguous blocks across the devices (openr_spf_whatif); each
  // device's CSR is appended to the caller's at the running total
  std::vector<uint32_t> rebased;
  const uint32_t nd = (uint32_t)ctx->devs.size();
  const uint32_t per = (n_links + nd - 1) / std::max<uint32_t>(nd, 1);
  uint64_t solved_total = 0, at = 0;
  bool over = false;
  delta->ptr[0] = 0;
  std::vector<uint64_t> ptr;
  std::vector<uint32_t> idx;
  for (uint32_t di = 0; di < nd; ++di) {
    Device& d = ctx->devs[di];
    const uint32_t b = std::min(n_links, di * per), e = std::min(n_links, b + per), m = e - b;
    if (!m || !n_sources) continue;
    const size_t mu = (size_t)m * n_sources;
    HIP_TRY(hipSetDevice(d.ordinal));
    WhatifUnits un;
    if ((rc0 = upload_whatif_units(d, hu, b, m, &rebased, &un)) != OPENR_SPF_OK) return rc0;
    HIP_TRY(d.win_src.reserve(n_sources));
    HIP_TRY(d.wchanged.reserve(mu));
    HIP_TRY(d.dlo_ptr.reserve(mu + 1));
    HIP_TRY(hipMemcpyAsync(d.win_src.p, sources, n_sources * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    // the device's entries land in library buffers sized to the room left in the caller's
    const uint64_t room = delta->cap > at ? delta->cap - at : 0;
    HIP_TRY(d.dlo_node.reserve(std::max<uint64_t>(room, 1)));
    HIP_TRY(d.dlo_dist.reserve(std::max<uint64_t>(room, 1)));
    HIP_TRY(d.dlo_nh.reserve(std::max<uint64_t>(room * nhb, 1)));
    uint64_t total = 0, solved = 0;
    int rc = whatif_delta_on_device(ctx, d, un, d.win_src.p, n_sources, flags, d.wchanged.p,
                                    reinterpret_cast<uint64_t*>(d.dlo_ptr.p), d.dlo_node.p, d.dlo_dist.p, d.dlo_nh.p,
                                    room, nhb, d.stream, &total, &solved);
    if (rc && rc != OPENR_SPF_E2BIG) return rc;
    over |= rc == OPENR_SPF_E2BIG;
    solved_total += solved;
    ptr.resize(mu + 1);
    HIP_TRY(hipMemcpyAsync(changed + (size_t)b * n_sources, d.wchanged.p, mu * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           d.stream));
    HIP_TRY(hipMemcpyAsync(ptr.data(), d.dlo_ptr.p, (mu + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
    const bool fits = !over && total <= room;
    if (fits && total) {
      HIP_TRY(hipMemcpyAsync(delta->node + at, d.dlo_node.p, total * 4u, hipMemcpyDeviceToHost, d.stream));
      HIP_TRY(hipMemcpyAsync(delta->dist + at, d.dlo_dist.p, total * 8u, hipMemcpyDeviceToHost, d.stream));
      HIP_TRY(hipMemcpyAsync(delta->nh + at * nhb, d.dlo_nh.p, total * nhb, hipMemcpyDeviceToHost, d.stream));
    }
    HIP_TRY(hipStreamSynchronize(d.stream));
    for (size_t u = 0; u < mu; ++u) {
      const size_t gu = (size_t)b * n_sources + u;
      delta->ptr[gu + 1] = at + ptr[u + 1];
      const uint32_t c = (uint32_t)(ptr[u + 1] - ptr[u]);
      if (!fits || c < 2) continue;
      // each unit's nodes ascending (the device keeps the repair's order)
      const uint64_t o = at + ptr[u];
      bool sorted = true;
      for (uint32_t k = 1; k < c && sorted; ++k) sorted = delta->node[o + k - 1] < delta->node[o + k];
      if (sorted) continue;
      idx.resize(c);
      for (uint32_t k = 0; k < c; ++k) idx[k] = k;
      std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return delta->node[o + x] < delta->node[o + y]; });
      std::vector<uint32_t> tn(c);
      std::vector<uint64_t> td(c);
      std::vector<uint8_t> th((size_t)c * nhb);
      for (uint32_t k = 0; k < c; ++k) {
        tn[k] = delta->node[o + idx[k]];
        td[k] = delta->dist[o + idx[k]];
        std::memcpy(&th[(size_t)k * nhb], delta->nh + (o + idx[k]) * nhb, nhb);
      }
      std::memcpy(delta->node + o, tn.data(), c * 4u);
      std::memcpy(delta->dist + o, td.data(), c * 8u);
      std::memcpy(delta->nh + o * nhb, th.data(), (size_t)c * nhb);
    }
    at += total;
  }
  ctx->stats.last_batch_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (out_solved) *out_solved = solved_total;
  if (over || at > delta->cap)
    return fail(OPENR_SPF_E2BIG, "delta needs %llu entries, cap %llu (ptr and changed are filled, entries are not)",
                (unsigned long long)at, (unsigned long long)delta->cap);
  return OPENR_SPF_OK;
}


// openr_spf_whatif_device / openr_spf_whatif_sets_device (un in device memory)
int whatif_device_form(openr_spf_ctx* ctx, int device_index, const WhatifUnits& un, const uint32_t* d_sources,
                       uint32_t n_sources, uint32_t flags, uint32_t* d_changed, void* stream, uint64_t* out_solved) {
  int rc = check_ctx(ctx);
  if (rc || (rc = check_device_index(ctx, device_index))) return rc;
  if ((un.n && !un.links && !un.set_ptr && !un.node_ptr && !un.edge_ptr) || (n_sources && !d_sources) ||
      (un.n && n_sources && !d_changed))
    return fail(OPENR_SPF_EINVAL, "null links, sources or changed");
  Plan bp, ip;
  if ((rc = whatif_plans(ctx, flags, &bp, &ip))) return rc;
  Device& d = ctx->devs[device_index];
  HIP_TRY(hipSetDevice(d.ordinal));
  hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : d.stream;
  uint32_t solved = 0;
  HIP_TRY(whatif_units_on_device(ctx, d, bp, ip, un, d_sources, n_sources, d_changed, s, &solved,
                                 (flags & OPENR_SPF_USE_LINK_METRIC) != 0));
  const uint64_t total = un.n && n_sources ? (uint64_t)solved + n_sources : 0u;
  ctx->stats.spf_runs += total;
  ctx->stats.batches += 1;
  if (out_solved) *out_solved = total;
  return OPENR_SPF_OK;
}

// openr_spf_whatif_delta_device / openr_spf_whatif_sets_delta_device
int whatif_delta_device_form(openr_spf_ctx* ctx, int device_index, const WhatifUnits& un, const uint32_t* d_sources,
                             uint32_t n_sources, uint32_t flags, uint32_t* d_changed, uint64_t* d_ptr,
                             uint32_t* d_node, uint64_t* d_dist, uint8_t* d_nh, uint64_t cap, uint32_t nh_bytes,
                             void* stream, uint64_t* out_total, uint64_t* out_solved) {
  int rc = check_ctx(ctx);
  if (rc || (rc = check_device_index(ctx, device_index))) return rc;
  if ((un.n && !un.links && !un.set_ptr && !un.node_ptr && !un.edge_ptr) || (n_sources && !d_sources) ||
      (un.n && n_sources && !d_changed) || !d_ptr)
    return fail(OPENR_SPF_EINVAL, "null links, sources, changed or ptr");
  if (cap && (!d_node || !d_dist || !d_nh)) return fail(OPENR_SPF_EINVAL, "null delta buffer");
  Device& d = ctx->devs[device_index];
  HIP_TRY(hipSetDevice(d.ordinal));
  hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : d.stream;
  uint64_t total = 0, solved = 0;
  rc = whatif_delta_on_device(ctx, d, un, d_sources, n_sources, flags, d_changed, d_ptr, d_node,
                                        reinterpret_cast<unsigned long long*>(d_dist), d_nh, cap, nh_bytes, s, &total,
                                        &solved);
  if (out_total) *out_total = total;
  if (out_solved) *out_solved = solved;
  return rc;
}

WhatifUnits host_sets(const uint32_t* set_ptr, const uint32_t* set_links, uint32_t n_sets) {
  WhatifUnits hu;
  hu.set_ptr = n_sets ? set_ptr : nullptr;
  hu.set_links = set_links;
  hu.n = n_sets;
  return hu;
}

WhatifUnits device_sets(const uint32_t* d_set_ptr, const uint32_t* d_set_links, uint32_t n_sets, uint32_t n_set_links) {
  WhatifUnits un;
  un.set_ptr = n_sets ? d_set_ptr : nullptr;
  un.set_links = d_set_links;
  un.n_set_links = n_set_links;
  un.n = n_sets;
  return un;
}

// Drain events as what-if units (host or device memory; n_nodes / n_links: the device form's
// slice lengths).
WhatifUnits drain_units(const uint32_t* node_ptr, const uint32_t* nodes, const uint32_t* link_ptr,
                        const uint32_t* links, uint32_t n_events, uint32_t n_nodes, uint32_t n_links) {
  WhatifUnits un;
  un.node_ptr = n_events ? node_ptr : nullptr;
  un.nodes = nodes;
  un.n_nodes = n_nodes;
  un.set_ptr = n_events ? link_ptr : nullptr;
  un.set_links = links;
  un.n_set_links = n_links;
  un.n = n_events;
  return un;
}

// Metric events as what-if units (host or device memory; n_edges: the device form's slice length).
WhatifUnits metric_units(const uint32_t* edge_ptr, const uint32_t* edges, const uint32_t* metrics, uint32_t n_events,
                         uint32_t n_edges) {
  WhatifUnits un;
  un.edge_ptr = n_events ? edge_ptr : nullptr;
  un.edges = edges;
  un.metrics = metrics;
  un.n_edges = n_edges;
  un.n = n_events;
  return un;
}

// Restore events as what-if units (host or device memory; the counts: the device form's slice lengths).
WhatifUnits restore_units(const uint32_t* node_ptr, const uint32_t* nodes, const uint32_t* link_ptr,
                          const uint32_t* links, const uint32_t* edge_ptr, const uint32_t* edges,
                          const uint32_t* metrics, uint32_t n_events, uint32_t n_nodes, uint32_t n_links,
                          uint32_t n_edges) {
  WhatifUnits un = drain_units(node_ptr, nodes, link_ptr, links, n_events, n_nodes, n_links);
  un.edge_ptr = n_events ? edge_ptr : nullptr;
  un.edges = edges;
  un.metrics = metrics;
  un.n_edges = n_edges;
  un.restore = true;
  return un;
}

// Maintenance events as what-if units: the CSRs of restore_units, read as overloads, link-downs and raises.
WhatifUnits maint_units(const uint32_t* node_ptr, const uint32_t* nodes, const uint32_t* link_ptr,
                        const uint32_t* links, const uint32_t* edge_ptr, const uint32_t* edges,
                        const uint32_t* metrics, uint32_t n_events, uint32_t n_nodes, uint32_t n_links,
                        uint32_t n_edges) {
  WhatifUnits un = restore_units(node_ptr, nodes, link_ptr, links, edge_ptr, edges, metrics, n_events, n_nodes,
                                 n_links, n_edges);
  un.restore = false;
  un.maint = true;
  return un;
}

// The events struct of a host form as what-if units, one overload per family.
WhatifUnits host_units(const openr_spf_drain_events_t* ev) {
  return drain_units(ev->node_ptr, ev->nodes, ev->link_ptr, ev->links, ev->n_events, 0u, 0u);
}
WhatifUnits host_units(const openr_spf_metric_events_t* ev) {
  return metric_units(ev->edge_ptr, ev->edges, ev->metrics, ev->n_events, 0u);
}
WhatifUnits host_units(const openr_spf_restore_events_t* ev) {
  return restore_units(ev->node_ptr, ev->nodes, ev->link_ptr, ev->links, ev->edge_ptr, ev->edges, ev->metrics,
                       ev->n_events, 0u, 0u, 0u);
}
WhatifUnits host_units(const openr_spf_maint_events_t* ev) {
  return maint_units(ev->node_ptr, ev->nodes, ev->link_ptr, ev->links, ev->edge_ptr, ev->edges, ev->metrics,
                     ev->n_events, 0u, 0u, 0u);
}

// The plan and capacity check of an event family (ElfaFamily names the four).
int check_family(const openr_spf_ctx* ctx, int fam, uint32_t flags, uint64_t n_events, uint64_t n_sources) {
  switch (fam) {
    case kElfaDrain: return check_drain(ctx, flags, n_events, n_sources);
    case kElfaMetric: return check_metric(ctx, flags, n_events, n_sources);
    case kElfaRestore: return check_restore(ctx, flags, n_events, n_sources);
    default: return check_maint(ctx, flags, n_events, n_sources);
  }
}

// The hop-count form of a metric sweep: metrics do not enter runSpf(src, false), so every
// count is 0, ptr is all zero and no kernel is launched (metric_hops_host / _device). The LFA
// forms do not take this exit: their pass still counts the unprotected groups.
bool metric_hops(int fam, uint32_t flags) { return fam == kElfaMetric && !(flags & OPENR_SPF_USE_LINK_METRIC); }

// Events built from the pointers and counts of a device form: an event pointer is null where
// its count is not. The CSR that makes the units events is the node CSR, or a metric event's
// edge CSR; the link CSR, and the edge CSR next to a node CSR, may be null.
bool event_pointer_missing(const WhatifUnits& un) {
  if (!un.n) return false;
  if (!un.node_ptr && (un.restore || un.maint || !un.edge_ptr)) return true;
  return (un.n_nodes && !un.nodes) || (un.set_ptr && un.n_set_links && !un.set_links) ||
         (un.edge_ptr && un.n_edges && (!un.edges || !un.metrics));
}

// Under link metric, the links of a restore event whose restored edges would leave the fast
// plans: an edge comes up with its current metric, or with the event's own entry for it.
int check_restored_links(const openr_spf_ctx* ctx, const WhatifUnits& hu, uint32_t flags) {
  if (!(flags & OPENR_SPF_USE_LINK_METRIC) || !hu.set_ptr) return OPENR_SPF_OK;
  for (uint32_t i = 0; i < hu.n; ++i)
    for (uint32_t k = hu.set_ptr[i]; k < hu.set_ptr[i + 1]; ++k) {
      const uint2 de = ctx->ledge[hu.set_links[k]];
      if (de.x == UINT32_MAX) continue;  // unused id
      for (const uint32_t e : {de.x, de.y}) {
        uint64_t m = ctx->metric[e];
        if (hu.edge_ptr) {  // the event's own entry for e, if any
          const uint32_t* b = hu.edges + hu.edge_ptr[i];
          const uint32_t* en = hu.edges + hu.edge_ptr[i + 1];
          const uint32_t* it = std::lower_bound(b, en, e);
          if (it != en && *it == e) m = hu.metrics[it - hu.edges];
        }
        if (m == 0 || m > 0x7FFFFFFFull)
          return fail(OPENR_SPF_ENOTSUP,
                      "event %u: link %u would come up with metric %llu on edge %u, outside [1, 2^31-1] (the base "
                      "plans after the event would need the exact-order kernel)",
                      i, hu.set_links[k], (unsigned long long)m, e);
      }
    }
  return OPENR_SPF_OK;
}

// The checks of an event call's host forms, in the order every family keeps: EINVAL first (the
// struct here, then sources, changed and the values in check_whatif_host), then the family's
// ENOTSUP / E2BIG, then a restore's links (ENOTSUP). *hu: the events as units.
template <class Events>
int check_events_host(const openr_spf_ctx* ctx, int fam, const Events* ev, const uint32_t* sources,
                      uint32_t n_sources, uint32_t flags, const uint32_t* changed, WhatifUnits* hu) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!ev) return fail(OPENR_SPF_EINVAL, "null events");
  *hu = host_units(ev);
  if (hu->n && !(fam == kElfaMetric ? hu->edge_ptr : hu->node_ptr))
    return fail(OPENR_SPF_EINVAL, "null %s", fam == kElfaMetric ? "edge_ptr" : "node_ptr");
  if ((rc = check_whatif_host(ctx, *hu, sources, n_sources, changed)) != OPENR_SPF_OK) return rc;
  if ((rc = check_family(ctx, fam, flags, hu->n, n_sources)) != OPENR_SPF_OK) return rc;
  return fam == kElfaRestore ? check_restored_links(ctx, *hu, flags) : OPENR_SPF_OK;
}

// ---- route-level calls (spf_routes.hip) ---------------------------------------------------

// A group table in device memory: group k = nodes[ptr[k], ptr[k + 1]), m entries in nodes.
struct DevGroups {
  const uint32_t* ptr = nullptr;
  const uint32_t* nodes = nullptr;
  uint32_t n = 0, m = 0;
};

// The rule "metric = min over members with dist != UINT64_MAX" reads UINT64_MAX as "not in
// the SpfResult"; with zero or wrapped metrics a reached node can carry it (openr_spf.h).
int check_routes_metric(const openr_spf_ctx* ctx, uint32_t flags) {
  if ((flags & OPENR_SPF_USE_LINK_METRIC) && !ctx->metric_ok)
    return fail(OPENR_SPF_ENOTSUP, "routes need usable metrics in [1, 2^31-1] under link metric (hop-count form is allowed)");
  return OPENR_SPF_OK;
}

// Group-table checks of the host forms (the device forms do not check).
int check_groups_host(const openr_spf_ctx* ctx, const openr_spf_groups_t* g) {
  if (!g) return fail(OPENR_SPF_EINVAL, "null groups");
  if (!g->n_groups) return OPENR_SPF_OK;
  if (!g->group_ptr) return fail(OPENR_SPF_EINVAL, "null group_ptr");
  for (uint32_t k = 0; k < g->n_groups; ++k)
    if (g->group_ptr[k + 1] < g->group_ptr[k])
      return fail(OPENR_SPF_EINVAL, "group_ptr does not ascend at group %u", k);
  if (g->group_ptr[g->n_groups] && !g->group_nodes) return fail(OPENR_SPF_EINVAL, "null group_nodes");
  for (uint32_t k = 0; k < g->n_groups; ++k)
    for (uint32_t m = g->group_ptr[k]; m < g->group_ptr[k + 1]; ++m) {
      if (g->group_nodes[m] >= ctx->V)
        return fail(OPENR_SPF_EINVAL, "group %u: node %u out of range (V=%u)", k, g->group_nodes[m], ctx->V);
      if (m > g->group_ptr[k] && g->group_nodes[m] <= g->group_nodes[m - 1])
        return fail(OPENR_SPF_EINVAL, "group %u is not strictly ascending", k);
    }
  return OPENR_SPF_OK;
}

int upload_groups(Device& d, const openr_spf_groups_t* g, DevGroups* out) {
  *out = DevGroups{};
  out->n = g->n_groups;
  if (!g->n_groups) return OPENR_SPF_OK;
  out->m = g->group_ptr[g->n_groups];
  HIP_TRY(d.rt_gptr.reserve((size_t)out->n + 1u));
  HIP_TRY(d.rt_gnodes.reserve(std::max<uint32_t>(out->m, 1u)));
  HIP_TRY(hipMemcpyAsync(d.rt_gptr.p, g->group_ptr, ((size_t)out->n + 1u) * sizeof(uint32_t), hipMemcpyHostToDevice,
                         d.stream));
  if (out->m)
    HIP_TRY(hipMemcpyAsync(d.rt_gnodes.p, g->group_nodes, (size_t)out->m * sizeof(uint32_t), hipMemcpyHostToDevice,
                           d.stream));
  out->ptr = d.rt_gptr.p;
  out->nodes = d.rt_gnodes.p;
  return OPENR_SPF_OK;
}

// openr_spf_routes[_device] on one device: the sources solved through the ordinary launcher
// into library scratch (the what-if base rows' buffers), a chunk of rows at a time when
// n x V rows exceed the what-if chunk budget, each chunk reduced to its routes. Enqueues
// only; OPENR_SPF_ROUTES_CHUNK (tests) forces a chunk size in rows.
int routes_on_device(openr_spf_ctx* ctx, Device& d, const uint32_t* d_sources, uint32_t n, uint32_t flags,
                     const DevGroups& gr, uint64_t* d_metric, uint8_t* d_nh, uint32_t nhb, uint32_t* d_nbest,
                     hipStream_t s) {
  if (!n || !gr.n) return OPENR_SPF_OK;
  Plan plan;
  int rc = make_plan(ctx, flags & OPENR_SPF_USE_LINK_METRIC, false, &plan);
  if (rc) return rc;
  const uint32_t V = ctx->V;
  const uint32_t nb = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  uint32_t chunk = (uint32_t)std::min<size_t>(n, std::max<size_t>(1, kWhatifChunkBytes / ((size_t)V * (8u + nb))));
  if (const char* e = std::getenv("OPENR_SPF_ROUTES_CHUNK"))
    if (std::atoi(e) > 0) chunk = std::min<uint32_t>(chunk, (uint32_t)std::atoi(e));
  HIP_TRY(d.base_dist.reserve((size_t)chunk * V));
  HIP_TRY(d.base_nh.reserve((size_t)chunk * V * nb));
  HIP_TRY(d.ovf.reserve((size_t)chunk * ctx->nsl_max()));
  HIP_TRY(d.rt_large.reserve(routes_reduce_scratch_words(gr.n)));
  HIP_TRY(reserve_counters(d));
  for (uint32_t c0 = 0; c0 < n; c0 += chunk) {
    const uint32_t m = std::min(chunk, n - c0);
    SolveArgs a{};
    a.sources = d_sources + c0;
    a.n = m;
    a.dist = d.base_dist.p;
    a.nh = d.base_nh.p;
    a.nh_bytes = nb;
    a.nh_bits = ctx->nh_bits;
    a.ovf_list = d.ovf.p;
    a.work = d.work.p;
    HIP_TRY(launch(ctx, d, plan, a, s));
    const size_t o = (size_t)c0 * gr.n;
    HIP_TRY(launch_routes_reduce(m, V, gr.n, gr.m, gr.ptr, gr.nodes, d.base_dist.p, d.base_nh.p, nb, d_metric + o,
                                 d_nh ? d_nh + o * nhb : nullptr, nhb, d_nbest ? d_nbest + o : nullptr, d.rt_large.p,
                                 d.num_cus, s));
  }
  ctx->stats.spf_runs += n;
  ctx->stats.batches += 1;
  return OPENR_SPF_OK;
}

// openr_spf_whatif_routes[_device] on one device. The link-set sweep runs with the node
// delta in device form into library scratch (whatif_delta_on_device: base rows stay
// resident in base_dist / base_nh); then the base routes of every source, the inverse map
// node -> groups, the count pass, the scan of the counts into d_ptr, the cap check and the
// emit pass. The node delta's capacity is the library's own: an estimate first, and on
// overflow the sweep is rerun with the total it reported, so OPENR_SPF_E2BIG only ever
// means sum(changed_routes) > cap. Synchronizes s.
int whatif_routes_on_device(openr_spf_ctx* ctx, Device& d, const WhatifUnits& un, const uint32_t* d_sources,
                            uint32_t n_src, uint32_t flags, const DevGroups& gr, uint32_t* d_changed, uint64_t* d_ptr,
                            uint32_t* d_group, uint64_t* d_metric, uint8_t* d_nh, uint32_t* d_nbest, uint64_t cap,
                            uint32_t nhb, hipStream_t s, uint64_t* total, uint64_t* solved_out) {
  const uint32_t V = ctx->V, G = gr.n;
  const uint32_t nb = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  if (nhb < nb) return fail(OPENR_SPF_EINVAL, "nh_bytes %u below the graph's next-hop width %u", nhb, nb);
  *total = 0;
  *solved_out = 0;
  const size_t units = (size_t)un.n * n_src;
  unsigned long long* ptr = reinterpret_cast<unsigned long long*>(d_ptr);
  if (!units) {
    HIP_TRY(hipMemsetAsync(ptr, 0, sizeof(unsigned long long), s));
    HIP_TRY(hipStreamSynchronize(s));
    return OPENR_SPF_OK;
  }
  // 1. the node sweep; a unit changes ~6 nodes on a WAN and V at the most
  HIP_TRY(d.rt_nchanged.reserve(units));
  HIP_TRY(d.rt_nptr.reserve(units + 1u));
  uint64_t ncap = std::min<uint64_t>((uint64_t)units * V, std::max<uint64_t>((uint64_t)units * 16u, 1u << 20));
  if (const char* e = std::getenv("OPENR_SPF_ROUTES_DELTA_CAP"))  // tests: start below the total (the rerun)
    ncap = std::strtoull(e, nullptr, 10);
  uint64_t ntotal = 0;
  for (int attempt = 0;; ++attempt) {
    HIP_TRY(d.rt_nnode.reserve(std::max<uint64_t>(ncap, 1)));
    HIP_TRY(d.rt_ndist.reserve(std::max<uint64_t>(ncap, 1)));
    HIP_TRY(d.rt_nnh.reserve(std::max<uint64_t>(ncap * nb, 1)));
    const openr_spf_stats_t stats0 = ctx->stats;
    uint64_t pool = 0;
    const int rc = whatif_delta_on_device(ctx, d, un, d_sources, n_src, flags, d.rt_nchanged.p,
                                          reinterpret_cast<uint64_t*>(d.rt_nptr.p), d.rt_nnode.p, d.rt_ndist.p,
                                          d.rt_nnh.p, ncap, nb, s, &ntotal, solved_out, &pool);
    if (rc == OPENR_SPF_OK) break;
    if (rc != OPENR_SPF_E2BIG) return rc;
    if (attempt == 2 || ntotal > (uint64_t)units * V)
      return fail(OPENR_SPF_ENOMEM, "node delta of %llu entries did not fit library scratch",
                  (unsigned long long)ntotal);
    ctx->stats = stats0;  // the rerun counts once
    ncap = std::max<uint64_t>(ntotal, pool / 2u + 1u);
  }
  // 2. base routes, inverse map
  HIP_TRY(hipMemsetAsync(d_changed, 0, units * sizeof(uint32_t), s));
  const size_t bg = (size_t)n_src * G;
  HIP_TRY(d.rt_bmetric.reserve(std::max<size_t>(bg, 1)));
  HIP_TRY(d.rt_bnh.reserve(std::max<size_t>(bg * nb, 1)));
  HIP_TRY(d.rt_large.reserve(routes_reduce_scratch_words(G)));
  HIP_TRY(launch_routes_reduce(n_src, V, G, gr.m, gr.ptr, gr.nodes, d.base_dist.p, d.base_nh.p, nb,
                               reinterpret_cast<uint64_t*>(d.rt_bmetric.p), d.rt_bnh.p, nb, nullptr, d.rt_large.p,
                               d.num_cus, s));
  HIP_TRY(d.rt_icnt.reserve(V));
  HIP_TRY(d.rt_icur.reserve(V));
  HIP_TRY(d.rt_iptr.reserve((size_t)V + 1u));
  HIP_TRY(d.rt_inv.reserve(std::max<uint32_t>(gr.m, 1u)));
  HIP_TRY(d.rt_tsum.reserve(std::max<size_t>(units, V) / 4096u + 1u));
  HIP_TRY(launch_routes_inverse(V, G, gr.m, gr.ptr, gr.nodes, d.rt_icnt.p, d.rt_icur.p, d.rt_tsum.p, d.rt_iptr.p,
                                d.rt_inv.p, d.num_cus, s));
  // 3. count pass, scan, cap check, emit pass
  const RoutesSweepLayout lay = whatif_routes_layout(V, G, units, d.num_cus);
  HIP_TRY(d.rt_ovl.reserve(std::max<size_t>(lay.ovl_words, 1)));
  HIP_TRY(d.rt_bm.reserve(std::max<size_t>(lay.bm_words, 1)));
  RoutesSweep p{};
  p.V = V;
  p.G = G;
  p.M = gr.m;
  p.n_src = n_src;
  p.nb = nb;
  p.onb = nhb;
  p.units = units;
  p.gptr = gr.ptr;
  p.gnodes = gr.nodes;
  p.iptr = d.rt_iptr.p;
  p.inv = d.rt_inv.p;
  p.nptr = d.rt_nptr.p;
  p.nnode = d.rt_nnode.p;
  p.ndist = d.rt_ndist.p;
  p.nnh = d.rt_nnh.p;
  p.bdist = reinterpret_cast<const unsigned long long*>(d.base_dist.p);
  p.bnh = d.base_nh.p;
  p.bmetric = d.rt_bmetric.p;
  p.bmnh = d.rt_bnh.p;
  p.changed = d_changed;
  p.optr = ptr;
  p.ogroup = d_group;
  p.ometric = reinterpret_cast<unsigned long long*>(d_metric);
  p.onh = d_nh;
  p.onbest = d_nbest;
  p.ovl_lds = lay.ovl_lds;
  p.bm_lds = lay.bm_lds;
  p.cand_cap = lay.cand_cap;
  p.g_ovl = d.rt_ovl.p;
  p.g_bm = d.rt_bm.p;
  HIP_TRY(launch_whatif_routes(p, lay, false, s));
  HIP_TRY(launch_delta_scan(d_changed, units, d.rt_tsum.p, ptr, s));
  unsigned long long tot = 0;
  HIP_TRY(hipMemcpyAsync(&tot, ptr + units, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *total = tot;
  if (tot > cap)
    return fail(OPENR_SPF_E2BIG, "%llu routes changed, cap %llu (ptr and changed_routes are filled, entries are not)",
                tot, (unsigned long long)cap);
  if (tot) {
    HIP_TRY(launch_whatif_routes(p, lay, true, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return OPENR_SPF_OK;
}

// openr_spf_routes: sources split in contiguous blocks across the devices
int routes_host(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n, uint32_t flags, const openr_spf_groups_t* g,
                uint64_t* metric, uint8_t* nh, uint32_t nh_bytes, uint32_t* n_best) {
  clear_launch_trace();
  if (!ctx) return fail(OPENR_SPF_EINVAL, "null context");
  if (!ctx->has_graph) return fail(OPENR_SPF_EINVAL, "no graph set (openr_spf_set_graph)");
  int rc = check_groups_host(ctx, g);
  if (rc) return rc;
  if (n && !sources) return fail(OPENR_SPF_EINVAL, "null sources");
  if (n && g->n_groups && !metric) return fail(OPENR_SPF_EINVAL, "null metric");
  const uint32_t need = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  if (nh && nh_bytes < need) return fail(OPENR_SPF_EINVAL, "nh_bytes %u < required %u", nh_bytes, need);
  for (uint32_t i = 0; i < n; ++i)
    if (sources[i] >= ctx->V) return fail(OPENR_SPF_EINVAL, "source %u out of range (V=%u)", sources[i], ctx->V);
  if ((rc = check_routes_metric(ctx, flags)) != OPENR_SPF_OK) return rc;
  const uint32_t G = g->n_groups;
  if (!n || !G) return OPENR_SPF_OK;
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t nd = (uint32_t)ctx->devs.size();
  const uint32_t per = (n + nd - 1) / std::max<uint32_t>(nd, 1);
  for (uint32_t di = 0; di < nd; ++di) {
    Device& d = ctx->devs[di];
    const uint32_t b = std::min(n, di * per), e = std::min(n, b + per), m = e - b;
    if (!m) continue;
    const size_t mg = (size_t)m * G;
    HIP_TRY(hipSetDevice(d.ordinal));
    DevGroups gr;
    if ((rc = upload_groups(d, g, &gr)) != OPENR_SPF_OK) return rc;
    HIP_TRY(d.src.reserve(m));
    HIP_TRY(d.rt_ometric.reserve(mg));
    if (nh) HIP_TRY(d.rt_onh.reserve(mg * nh_bytes));
    if (n_best) HIP_TRY(d.rt_onbest.reserve(mg));
    HIP_TRY(hipMemcpyAsync(d.src.p, sources + b, m * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    if ((rc = routes_on_device(ctx, d, d.src.p, m, flags, gr, reinterpret_cast<uint64_t*>(d.rt_ometric.p),
                               nh ? d.rt_onh.p : nullptr, nh_bytes, n_best ? d.rt_onbest.p : nullptr, d.stream)) !=
        OPENR_SPF_OK)
      return rc;
    const size_t o = (size_t)b * G;
    HIP_TRY(hipMemcpyAsync(metric + o, d.rt_ometric.p, mg * sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
    if (nh) HIP_TRY(hipMemcpyAsync(nh + o * nh_bytes, d.rt_onh.p, mg * nh_bytes, hipMemcpyDeviceToHost, d.stream));
    if (n_best)
      HIP_TRY(hipMemcpyAsync(n_best + o, d.rt_onbest.p, mg * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
  }
  for (uint32_t di = 0; di < nd; ++di) {
    if (std::min(n, di * per) >= n) continue;
    HIP_TRY(hipSetDevice(ctx->devs[di].ordinal));
    HIP_TRY(hipStreamSynchronize(ctx->devs[di].stream));
  }
  ctx->stats.last_batch_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return OPENR_SPF_OK;
}

// openr_spf_whatif_routes: sets split in contiguous blocks across the devices, each device's
// CSR appended to the caller's at the running total, each unit's entries sorted by group id
int whatif_routes_host(openr_spf_ctx* ctx, const WhatifUnits& hu, const uint32_t* sources, uint32_t n_sources,
                       uint32_t flags, const openr_spf_groups_t* g, uint32_t* changed,
                       openr_spf_whatif_routes_t* delta, uint64_t* out_solved) {
  clear_launch_trace();
  const uint32_t n_sets = hu.n;
  if (!ctx) return fail(OPENR_SPF_EINVAL, "null context");
  if (!ctx->has_graph) return fail(OPENR_SPF_EINVAL, "no graph set (openr_spf_set_graph)");
  int rc = check_whatif_host(ctx, hu, sources, n_sources, changed);
  if (rc) return rc;
  if ((rc = check_groups_host(ctx, g)) != OPENR_SPF_OK) return rc;
  if (delta && !delta->ptr) return fail(OPENR_SPF_EINVAL, "null delta->ptr");
  if (delta && delta->cap && (!delta->group || !delta->metric || !delta->nh))
    return fail(OPENR_SPF_EINVAL, "null delta->group, metric or nh");
  if ((rc = check_routes_metric(ctx, flags)) != OPENR_SPF_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t need = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  const uint32_t nhb = delta ? delta->nh_bytes : need;
  const uint64_t cap = delta ? delta->cap : 0u;
  const bool want_nbest = delta && delta->n_best;
  std::vector<uint32_t> rebased, idx;
  std::vector<uint64_t> ptr;
  const uint32_t nd = (uint32_t)ctx->devs.size();
  const uint32_t per = (n_sets + nd - 1) / std::max<uint32_t>(nd, 1);
  uint64_t solved_total = 0, at = 0;
  bool over = false;
  if (delta) delta->ptr[0] = 0;
  if (out_solved) *out_solved = 0;
  for (uint32_t di = 0; di < nd; ++di) {
    Device& d = ctx->devs[di];
    const uint32_t b = std::min(n_sets, di * per), e = std::min(n_sets, b + per), m = e - b;
    if (!m || !n_sources) continue;
    const size_t mu = (size_t)m * n_sources;
    HIP_TRY(hipSetDevice(d.ordinal));
    WhatifUnits un;
    if ((rc = upload_whatif_units(d, hu, b, m, &rebased, &un)) != OPENR_SPF_OK) return rc;
    DevGroups gr;
    if ((rc = upload_groups(d, g, &gr)) != OPENR_SPF_OK) return rc;
    HIP_TRY(d.win_src.reserve(n_sources));
    HIP_TRY(d.rt_ochanged.reserve(mu));
    HIP_TRY(d.rt_optr.reserve(mu + 1));
    HIP_TRY(hipMemcpyAsync(d.win_src.p, sources, n_sources * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    // the device's entries land in library buffers sized to the room left in the caller's
    const uint64_t room = cap > at ? cap - at : 0;
    HIP_TRY(d.rt_ogroup.reserve(std::max<uint64_t>(room, 1)));
    HIP_TRY(d.rt_ometric.reserve(std::max<uint64_t>(room, 1)));
    HIP_TRY(d.rt_onh.reserve(std::max<uint64_t>(room * nhb, 1)));
    if (want_nbest) HIP_TRY(d.rt_onbest.reserve(std::max<uint64_t>(room, 1)));
    uint64_t total = 0, solved = 0;
    rc = whatif_routes_on_device(ctx, d, un, d.win_src.p, n_sources, flags, gr, d.rt_ochanged.p,
                                 reinterpret_cast<uint64_t*>(d.rt_optr.p), d.rt_ogroup.p,
                                 reinterpret_cast<uint64_t*>(d.rt_ometric.p), d.rt_onh.p,
                                 want_nbest ? d.rt_onbest.p : nullptr, room, nhb, d.stream, &total, &solved);
    if (rc && rc != OPENR_SPF_E2BIG) return rc;
    over |= rc == OPENR_SPF_E2BIG;
    solved_total += solved;
    ptr.resize(mu + 1);
    HIP_TRY(hipMemcpyAsync(changed + (size_t)b * n_sources, d.rt_ochanged.p, mu * sizeof(uint32_t),
                           hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipMemcpyAsync(ptr.data(), d.rt_optr.p, (mu + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
    const bool fits = delta && !over && total <= room;
    if (fits && total) {
      HIP_TRY(hipMemcpyAsync(delta->group + at, d.rt_ogroup.p, total * 4u, hipMemcpyDeviceToHost, d.stream));
      HIP_TRY(hipMemcpyAsync(delta->metric + at, d.rt_ometric.p, total * 8u, hipMemcpyDeviceToHost, d.stream));
      HIP_TRY(hipMemcpyAsync(delta->nh + at * nhb, d.rt_onh.p, total * nhb, hipMemcpyDeviceToHost, d.stream));
      if (want_nbest)
        HIP_TRY(hipMemcpyAsync(delta->n_best + at, d.rt_onbest.p, total * 4u, hipMemcpyDeviceToHost, d.stream));
    }
    HIP_TRY(hipStreamSynchronize(d.stream));
    for (size_t u = 0; delta && u < mu; ++u) {
      const size_t gu = (size_t)b * n_sources + u;
      delta->ptr[gu + 1] = at + ptr[u + 1];
      const uint32_t c = (uint32_t)(ptr[u + 1] - ptr[u]);
      if (!fits || c < 2) continue;
      // each unit's groups ascending (the device keeps the kernel's order)
      const uint64_t o = at + ptr[u];
      idx.resize(c);
      for (uint32_t k = 0; k < c; ++k) idx[k] = k;
      std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return delta->group[o + x] < delta->group[o + y]; });
      std::vector<uint32_t> tg(c), tb(c);
      std::vector<uint64_t> tm(c);
      std::vector<uint8_t> th((size_t)c * nhb);
      for (uint32_t k = 0; k < c; ++k) {
        tg[k] = delta->group[o + idx[k]];
        tm[k] = delta->metric[o + idx[k]];
        if (want_nbest) tb[k] = delta->n_best[o + idx[k]];
        std::memcpy(&th[(size_t)k * nhb], delta->nh + (o + idx[k]) * nhb, nhb);
      }
      std::memcpy(delta->group + o, tg.data(), c * 4u);
      std::memcpy(delta->metric + o, tm.data(), c * 8u);
      if (want_nbest) std::memcpy(delta->n_best + o, tb.data(), c * 4u);
      std::memcpy(delta->nh + o * nhb, th.data(), (size_t)c * nhb);
    }
    at += total;
  }
  ctx->stats.last_batch_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (out_solved) *out_solved = solved_total;
  if (delta && (over || at > cap))
    return fail(OPENR_SPF_E2BIG, "%llu routes changed, cap %llu (ptr and changed_routes are filled, entries are not)",
                (unsigned long long)at, (unsigned long long)cap);
  return OPENR_SPF_OK;
}

// ---- loop-free alternates (spf_lfa.hip) -----------------------------------------------------

// Outputs of openr_spf_lfa_routes[_device] in device memory. nh / alt hold nhb bytes per
// route; nh, alt and n_alt may be null; the entry arrays are written when `entries` is set
// (ptr [n * G + 1] then non-null; nbr / alt_metric hold cap entries).
struct LfaOut {
  uint64_t* metric = nullptr;
  uint8_t* nh = nullptr;
  uint8_t* alt = nullptr;
  uint32_t nhb = 0;
  uint32_t* n_alt = nullptr;
  bool entries = false;
  uint64_t* ptr = nullptr;
  uint32_t* nbr = nullptr;
  uint64_t* alt_metric = nullptr;
  uint64_t cap = 0;
};

// openr_spf_lfa_routes[_device] on one device, a chunk of sources at a time. Per chunk: the
// needed rows (launch_lfa_rows; one synchronization for their count, which sizes the second
// solve), the sources solved with next hops and the other needed nodes with distances only
// through the ordinary launcher into library scratch, routes_reduce over the sources' rows,
// the neighbour table and the count pass; with entries the scan of the counts into ptr
// (moved behind the chunks before it), one more synchronization for the total, the cap check
// and the emit pass. All sources are one chunk when V distance rows and their next-hop rows
// fit the what-if chunk budget; else a chunk holds as many sources as fit with the widest
// neighbour closure, each chunk has its own closure, and a row two chunks need is solved in
// both. OPENR_SPF_ROUTES_CHUNK (tests) forces a chunk size in sources. *solved = rows solved:
// every source of the batch (a duplicate is solved again, as openr_spf_routes does) plus
// every chunk's other needed nodes.
int lfa_on_device(openr_spf_ctx* ctx, Device& d, const uint32_t* d_sources, uint32_t n, uint32_t flags,
                  const DevGroups& gr, const LfaOut& out, hipStream_t s, uint64_t* total, uint64_t* solved_out) {
  const uint32_t V = ctx->V, G = gr.n;
  const uint32_t nb = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  if (out.nhb < nb) return fail(OPENR_SPF_EINVAL, "nh_bytes %u below the graph's next-hop width %u", out.nhb, nb);
  *total = 0;
  *solved_out = 0;
  unsigned long long* ptr = reinterpret_cast<unsigned long long*>(out.ptr);
  if (!n || !G) {
    if (out.entries) {
      HIP_TRY(hipMemsetAsync(ptr, 0, sizeof(unsigned long long), s));
      HIP_TRY(hipStreamSynchronize(s));
    }
    return OPENR_SPF_OK;
  }
  Plan plan;
  int rc = make_plan(ctx, flags & OPENR_SPF_USE_LINK_METRIC, false, &plan);
  if (rc) return rc;
  const size_t row_bytes = (size_t)V * 8u, nh_row_bytes = (size_t)V * nb;
  uint32_t chunk = n;
  if ((size_t)V * row_bytes + (size_t)n * nh_row_bytes > kWhatifChunkBytes)
    chunk = (uint32_t)std::min<size_t>(
        n, std::max<size_t>(1, kWhatifChunkBytes / (row_bytes * ((size_t)ctx->nh_bits + 1u) + nh_row_bytes)));
  if (const char* e = std::getenv("OPENR_SPF_ROUTES_CHUNK"))
    if (std::atoi(e) > 0) chunk = std::min<uint32_t>(chunk, (uint32_t)std::atoi(e));
  const uint32_t words = (V + 31u) / 32u;
  const size_t E1 = std::max<uint32_t>(ctx->E, 1u);
  HIP_TRY(d.lf_need.reserve(words));
  HIP_TRY(d.lf_srcbm.reserve(words));
  HIP_TRY(d.lf_cnt.reserve(words));
  HIP_TRY(d.lf_wptr.reserve((size_t)words + 1u));
  HIP_TRY(d.lf_tsum.reserve(std::max<size_t>(words, (size_t)chunk * G) / 4096u + 1u));
  HIP_TRY(d.lf_list.reserve(V));
  HIP_TRY(d.lf_rowidx.reserve(V));
  HIP_TRY(d.lf_trow.reserve(E1));
  HIP_TRY(d.lf_ttome.reserve(E1));
  HIP_TRY(d.lf_tfrom.reserve(E1));
  HIP_TRY(d.base_nh.reserve((size_t)chunk * nh_row_bytes));
  HIP_TRY(d.ovf.reserve((size_t)std::max(chunk, V) * ctx->nsl_max()));
  HIP_TRY(d.rt_large.reserve(routes_reduce_scratch_words(G)));
  HIP_TRY(reserve_counters(d));
  // the emit pass reads nh and the scan reads n_alt: library scratch where the caller passed none
  uint8_t* nh_out = out.nh;
  uint32_t* nalt_out = out.n_alt;
  const bool own_nh = out.entries && !nh_out, own_nalt = out.entries && !nalt_out;  // one chunk's worth
  if (own_nh) {
    HIP_TRY(d.lf_nh.reserve((size_t)chunk * G * out.nhb));
    nh_out = d.lf_nh.p;
  }
  if (own_nalt) {
    HIP_TRY(d.lf_nalt.reserve((size_t)chunk * G));
    nalt_out = d.lf_nalt.p;
  }
  unsigned long long carry = 0;
  uint64_t solved = 0;
  bool over = false;
  for (uint32_t c0 = 0; c0 < n; c0 += chunk) {
    const uint32_t m = std::min(chunk, n - c0);
    const uint32_t* src = d_sources + c0;
    const size_t o = (size_t)c0 * G, mg = (size_t)m * G;
    // 1. the rows the chunk needs
    HIP_TRY(launch_lfa_rows(d.g, src, m, d.lf_need.p, d.lf_srcbm.p, d.lf_cnt.p, d.lf_tsum.p, d.lf_wptr.p,
                            d.lf_list.p, d.lf_rowidx.p, d.num_cus, s));
    unsigned long long extra64 = 0;
    HIP_TRY(hipMemcpyAsync(&extra64, d.lf_wptr.p + words, sizeof(extra64), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t extra = (uint32_t)std::min<unsigned long long>(extra64, V);
    // 2. the solves: rows [0, m) the sources (distances and next hops), [m, m + extra) the rest
    HIP_TRY(d.base_dist.reserve(((size_t)m + extra) * V));
    SolveArgs a{};
    a.sources = src;
    a.n = m;
    a.dist = d.base_dist.p;
    a.nh = d.base_nh.p;
    a.nh_bytes = nb;
    a.nh_bits = ctx->nh_bits;
    a.ovf_list = d.ovf.p;
    a.work = d.work.p;
    HIP_TRY(launch(ctx, d, plan, a, s));
    if (extra) {
      SolveArgs b{};
      b.sources = d.lf_list.p;
      b.n = extra;
      b.dist = d.base_dist.p + (size_t)m * V;
      b.nh_bytes = nb;
      b.nh_bits = ctx->nh_bits;
      b.ovf_list = d.ovf.p;
      b.work = d.work.p;
      HIP_TRY(launch(ctx, d, plan, b, s));
    }
    solved += (uint64_t)m + extra;
    // 3. the shortest-path half, the neighbour table, the count pass
    uint8_t* c_nh = nh_out ? (own_nh ? nh_out : nh_out + o * out.nhb) : nullptr;
    uint32_t* c_nalt = nalt_out ? (own_nalt ? nalt_out : nalt_out + o) : nullptr;
    HIP_TRY(launch_routes_reduce(m, V, G, gr.m, gr.ptr, gr.nodes, d.base_dist.p, d.base_nh.p, nb, out.metric + o,
                                 c_nh, out.nhb, nullptr, d.rt_large.p, d.num_cus, s));
    HIP_TRY(launch_lfa_table(d.g, src, m, d.lf_rowidx.p, d.base_dist.p, d.lf_trow.p, d.lf_ttome.p, d.lf_tfrom.p,
                             d.num_cus, s));
    LfaPass p{};
    p.n = m;
    p.V = V;
    p.G = G;
    p.M = gr.m;
    p.onb = out.nhb;
    p.sources = src;
    p.row2 = d.g.row2;
    p.gptr = gr.ptr;
    p.gnodes = gr.nodes;
    p.dist = reinterpret_cast<const unsigned long long*>(d.base_dist.p);
    p.trow = d.lf_trow.p;
    p.ttome = d.lf_ttome.p;
    p.tfrom = d.lf_tfrom.p;
    p.metric = reinterpret_cast<const unsigned long long*>(out.metric + o);
    p.nh = c_nh;
    p.alt = out.alt ? out.alt + o * out.nhb : nullptr;
    p.nalt = c_nalt;
    p.large = d.rt_large.p;
    p.n_large = d.rt_large.p + G;
    HIP_TRY(launch_lfa_reduce(p, false, d.num_cus, s));
    if (!out.entries) continue;
    // 4. this chunk's slice of ptr, the total so far, the cap check, the emit pass
    HIP_TRY(launch_delta_scan(c_nalt, mg, d.lf_tsum.p, ptr + o, s));
    unsigned long long tot = 0;
    HIP_TRY(hipMemcpyAsync(&tot, ptr + o + mg, sizeof(tot), hipMemcpyDeviceToHost, s));
    HIP_TRY(launch_lfa_ptr_shift(ptr + o, mg + 1u, carry, d.num_cus, s));
    HIP_TRY(hipStreamSynchronize(s));
    carry += tot;
    over |= carry > out.cap;
    if (over || !tot) continue;
    p.optr = ptr + o;
    p.onbr = out.nbr;
    p.ometric = reinterpret_cast<unsigned long long*>(out.alt_metric);
    HIP_TRY(launch_lfa_reduce(p, true, d.num_cus, s));
  }
  *total = carry;
  *solved_out = solved;
  ctx->stats.spf_runs += solved;
  ctx->stats.batches += 1;
  if (over)
    return fail(OPENR_SPF_E2BIG, "%llu alternates, cap %llu (ptr, n_alt, metric, nh and alt are filled, entries are not)",
                carry, (unsigned long long)out.cap);
  return OPENR_SPF_OK;
}

// openr_spf_lfa_routes: sources split in contiguous blocks across the devices, each device's
// entries appended to the caller's at the running total
int lfa_host(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n, uint32_t flags, const openr_spf_groups_t* g,
             uint64_t* metric, uint8_t* nh, uint8_t* alt, uint32_t nh_bytes, uint32_t* n_alt,
             openr_spf_lfa_entries_t* ent, uint64_t* out_solved) {
  clear_launch_trace();
  if (out_solved) *out_solved = 0;
  if (!ctx) return fail(OPENR_SPF_EINVAL, "null context");
  if (!ctx->has_graph) return fail(OPENR_SPF_EINVAL, "no graph set (openr_spf_set_graph)");
  int rc = check_groups_host(ctx, g);
  if (rc) return rc;
  if (n && !sources) return fail(OPENR_SPF_EINVAL, "null sources");
  if (n && g->n_groups && !metric) return fail(OPENR_SPF_EINVAL, "null metric");
  const uint32_t need = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  if (nh_bytes < need) return fail(OPENR_SPF_EINVAL, "nh_bytes %u < required %u", nh_bytes, need);
  for (uint32_t i = 0; i < n; ++i)
    if (sources[i] >= ctx->V) return fail(OPENR_SPF_EINVAL, "source %u out of range (V=%u)", sources[i], ctx->V);
  if (ent && !ent->ptr) return fail(OPENR_SPF_EINVAL, "null entries->ptr");
  if (ent && ent->cap && (!ent->nbr || !ent->metric)) return fail(OPENR_SPF_EINVAL, "null entries->nbr or metric");
  if ((rc = check_routes_metric(ctx, flags)) != OPENR_SPF_OK) return rc;
  const uint32_t G = g->n_groups;
  if (ent) ent->ptr[0] = 0;
  if (!n || !G) return OPENR_SPF_OK;
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t cap = ent ? ent->cap : 0u;
  const uint32_t nd = (uint32_t)ctx->devs.size();
  const uint32_t per = (n + nd - 1) / std::max<uint32_t>(nd, 1);
  uint64_t solved_total = 0, at = 0;
  bool over = false;
  std::vector<uint64_t> ptr;
  for (uint32_t di = 0; di < nd; ++di) {
    Device& d = ctx->devs[di];
    const uint32_t b = std::min(n, di * per), e = std::min(n, b + per), m = e - b;
    if (!m) continue;
    const size_t mg = (size_t)m * G, o = (size_t)b * G;
    HIP_TRY(hipSetDevice(d.ordinal));
    DevGroups gr;
    if ((rc = upload_groups(d, g, &gr)) != OPENR_SPF_OK) return rc;
    const uint64_t room = cap > at ? cap - at : 0;
    HIP_TRY(d.src.reserve(m));
    HIP_TRY(d.rt_ometric.reserve(mg));
    HIP_TRY(d.rt_onh.reserve(mg * nh_bytes));
    HIP_TRY(d.lf_alt.reserve(mg * nh_bytes));
    HIP_TRY(d.lf_nalt.reserve(mg));
    if (ent) {
      HIP_TRY(d.lf_optr.reserve(mg + 1u));
      HIP_TRY(d.lf_onbr.reserve(std::max<uint64_t>(room, 1)));
      HIP_TRY(d.lf_oam.reserve(std::max<uint64_t>(room, 1)));
    }
    HIP_TRY(hipMemcpyAsync(d.src.p, sources + b, m * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    LfaOut out;
    out.metric = reinterpret_cast<uint64_t*>(d.rt_ometric.p);
    out.nh = d.rt_onh.p;
    out.alt = d.lf_alt.p;
    out.nhb = nh_bytes;
    out.n_alt = d.lf_nalt.p;
    out.entries = ent != nullptr;
    out.ptr = reinterpret_cast<uint64_t*>(d.lf_optr.p);
    out.nbr = d.lf_onbr.p;
    out.alt_metric = reinterpret_cast<uint64_t*>(d.lf_oam.p);
    out.cap = room;
    uint64_t total = 0, solved = 0;
    rc = lfa_on_device(ctx, d, d.src.p, m, flags, gr, out, d.stream, &total, &solved);
    if (rc && rc != OPENR_SPF_E2BIG) return rc;
    over |= rc == OPENR_SPF_E2BIG;
    solved_total += solved;
    HIP_TRY(hipMemcpyAsync(metric + o, d.rt_ometric.p, mg * sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
    if (nh) HIP_TRY(hipMemcpyAsync(nh + o * nh_bytes, d.rt_onh.p, mg * nh_bytes, hipMemcpyDeviceToHost, d.stream));
    if (alt) HIP_TRY(hipMemcpyAsync(alt + o * nh_bytes, d.lf_alt.p, mg * nh_bytes, hipMemcpyDeviceToHost, d.stream));
    if (n_alt) HIP_TRY(hipMemcpyAsync(n_alt + o, d.lf_nalt.p, mg * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
    if (ent) {
      ptr.resize(mg + 1);
      HIP_TRY(hipMemcpyAsync(ptr.data(), d.lf_optr.p, (mg + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
      if (!over && total) {
        HIP_TRY(hipMemcpyAsync(ent->nbr + at, d.lf_onbr.p, total * 4u, hipMemcpyDeviceToHost, d.stream));
        HIP_TRY(hipMemcpyAsync(ent->metric + at, d.lf_oam.p, total * 8u, hipMemcpyDeviceToHost, d.stream));
      }
    }
    HIP_TRY(hipStreamSynchronize(d.stream));
    for (size_t u = 0; ent && u < mg; ++u) ent->ptr[o + u + 1] = at + ptr[u + 1];
    at += total;
  }
  ctx->stats.last_batch_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (out_solved) *out_solved = solved_total;
  if (ent && (over || at > cap))
    return fail(OPENR_SPF_E2BIG, "%llu alternates, cap %llu (ptr, n_alt, metric, nh and alt are filled, entries are not)",
                (unsigned long long)at, (unsigned long long)cap);
  return OPENR_SPF_OK;
}

// ---- post-failure loop-free alternates (spf_wlfa.hip) ----------------------------------------

// Outputs of openr_spf_whatif_lfa[_device] in device memory. unprot, lost and ptr may be null
// (ptr null: counts only, the scan goes to library scratch).
struct WlfaOut {
  uint32_t* changed = nullptr;
  uint32_t* unprot = nullptr;
  uint32_t* lost = nullptr;
  uint64_t* ptr = nullptr;
  uint32_t* group = nullptr;
  uint64_t* metric = nullptr;
  uint8_t* nh = nullptr;
  uint8_t* alt = nullptr;
  uint64_t cap = 0;
  uint32_t nhb = 0;
};

// openr_spf_whatif_lfa[_device] on one device: the closure list of the sources
// (launch_lfa_rows; one synchronization for its length), the link-set sweep over sets x
// closure with the node delta into library scratch (base rows of every closure node stay
// resident; the capacity is estimated and the sweep rerun on overflow, as in
// whatif_routes_on_device), the base routes and base alternates of the sources, the inverse
// map, the mark pass, the count pass, the scan of the counts, the cap check and the emit
// pass. OPENR_SPF_E2BIG only ever means sum(changed) > cap. Synchronizes s.
// fam >= 0 (ElfaFamily; openr_spf_whatif_drain_lfa / _metric_lfa / _restore_lfa): `un` holds
// events of that family, the node sweep is the family's repair sweep and the passes are those
// of spf_elfa.hip. A restore widens the closure to every neighbour of a source and gives the
// pass a table of its own over it; the hop-count form of a metric sweep solves the base rows
// only (nothing moves: every unit gets its source's base unprotected count). kElfaMaint: the
// node sweep is the maintenance sweep (whatif_units_on_device goes by the unit kind), closure,
// table and pass are the drain's; its hop-count form is not idle (N_i and K_i still act).
int whatif_lfa_on_device(openr_spf_ctx* ctx, Device& d, const WhatifUnits& un, const uint32_t* d_sources,
                         uint32_t n_src, uint32_t flags, const DevGroups& gr, const WlfaOut& out, hipStream_t s,
                         uint64_t* total, uint64_t* solved_out, int fam = -1) {
  const bool idle = fam == kElfaMetric && !(flags & OPENR_SPF_USE_LINK_METRIC);
  const uint32_t V = ctx->V, G = gr.n;
  const uint32_t nb = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  if (out.nhb < nb) return fail(OPENR_SPF_EINVAL, "nh_bytes %u below the graph's next-hop width %u", out.nhb, nb);
  *total = 0;
  *solved_out = 0;
  const size_t units = (size_t)un.n * n_src;
  if (!units || !G) {
    if (units) {
      HIP_TRY(hipMemsetAsync(out.changed, 0, units * sizeof(uint32_t), s));
      if (out.unprot) HIP_TRY(hipMemsetAsync(out.unprot, 0, units * sizeof(uint32_t), s));
      if (out.lost) HIP_TRY(hipMemsetAsync(out.lost, 0, units * sizeof(uint32_t), s));
    }
    if (out.ptr) HIP_TRY(hipMemsetAsync(out.ptr, 0, (units + 1u) * sizeof(uint64_t), s));
    HIP_TRY(hipStreamSynchronize(s));
    return OPENR_SPF_OK;
  }
  // 1. the rows the sources need: themselves, then their up neighbours that are no source
  const uint32_t words = (V + 31u) / 32u;
  const size_t E1 = std::max<uint32_t>(ctx->E, 1u);
  HIP_TRY(d.lf_need.reserve(words));
  HIP_TRY(d.lf_srcbm.reserve(words));
  HIP_TRY(d.lf_cnt.reserve(words));
  HIP_TRY(d.lf_wptr.reserve((size_t)words + 1u));
  HIP_TRY(d.lf_tsum.reserve(words / 4096u + 1u));
  HIP_TRY(d.lf_list.reserve(V));
  HIP_TRY(d.lf_rowidx.reserve(V));
  HIP_TRY(d.lf_trow.reserve(E1));
  HIP_TRY(d.lf_ttome.reserve(E1));
  HIP_TRY(d.lf_tfrom.reserve(E1));
  HIP_TRY((fam == kElfaRestore ? launch_elfa_rows : launch_lfa_rows)(d.g, d_sources, n_src, d.lf_need.p, d.lf_srcbm.p,
                                                                     d.lf_cnt.p, d.lf_tsum.p, d.lf_wptr.p,
                                                                     d.lf_list.p, d.lf_rowidx.p, d.num_cus, s));
  unsigned long long extra64 = 0;
  HIP_TRY(hipMemcpyAsync(&extra64, d.lf_wptr.p + words, sizeof(extra64), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const uint32_t extra = (uint32_t)std::min<unsigned long long>(extra64, V);
  if ((uint64_t)n_src + extra > 0xFFFFFFFFull) return fail(OPENR_SPF_EINVAL, "too many sources");
  const uint32_t n_rows = n_src + extra;
  HIP_TRY(d.wl_clos.reserve(n_rows));
  HIP_TRY(hipMemcpyAsync(d.wl_clos.p, d_sources, (size_t)n_src * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  if (extra)
    HIP_TRY(hipMemcpyAsync(d.wl_clos.p + n_src, d.lf_list.p, (size_t)extra * sizeof(uint32_t),
                           hipMemcpyDeviceToDevice, s));
  // 2. the node sweep over sets x closure
  const size_t nunits = (size_t)un.n * n_rows;
  HIP_TRY(d.rt_nchanged.reserve(nunits));
  HIP_TRY(d.rt_nptr.reserve(nunits + 1u));
  uint64_t ncap = std::min<uint64_t>((uint64_t)nunits * V, std::max<uint64_t>((uint64_t)nunits * 16u, 1u << 20));
  if (const char* e = std::getenv("OPENR_SPF_ROUTES_DELTA_CAP"))  // tests: start below the total (the rerun)
    ncap = std::strtoull(e, nullptr, 10);
  uint64_t ntotal = 0;
  if (idle) {  // the base rows of the closure, no sweep
    Plan bp;
    const int rc = make_plan(ctx, flags, false, &bp);
    if (rc) return rc;
    bool tin = false;
    HIP_TRY(whatif_base_solve(ctx, d, bp, d.wl_clos.p, n_rows, s, &tin));
    *solved_out = n_rows;
    ctx->stats.spf_runs += n_rows;
    ctx->stats.batches += 1;
  }
  for (int attempt = 0; !idle; ++attempt) {
    HIP_TRY(d.rt_nnode.reserve(std::max<uint64_t>(ncap, 1)));
    HIP_TRY(d.rt_ndist.reserve(std::max<uint64_t>(ncap, 1)));
    HIP_TRY(d.rt_nnh.reserve(std::max<uint64_t>(ncap * nb, 1)));
    const openr_spf_stats_t stats0 = ctx->stats;
    uint64_t pool = 0;
    const int rc = whatif_delta_on_device(ctx, d, un, d.wl_clos.p, n_rows, flags, d.rt_nchanged.p,
                                          reinterpret_cast<uint64_t*>(d.rt_nptr.p), d.rt_nnode.p, d.rt_ndist.p,
                                          d.rt_nnh.p, ncap, nb, s, &ntotal, solved_out, &pool);
    if (rc == OPENR_SPF_OK) break;
    if (rc != OPENR_SPF_E2BIG) return rc;
    if (attempt == 2 || ntotal > (uint64_t)nunits * V)
      return fail(OPENR_SPF_ENOMEM, "node delta of %llu entries did not fit library scratch",
                  (unsigned long long)ntotal);
    ctx->stats = stats0;  // the rerun counts once
    ncap = std::max<uint64_t>(ntotal, pool / 2u + 1u);
  }
  // 3. base routes of the sources (rows [0, n_src) of the closure)
  const size_t bg = (size_t)n_src * G;
  HIP_TRY(d.rt_bmetric.reserve(bg));
  HIP_TRY(d.rt_bnh.reserve(bg * nb));
  HIP_TRY(d.rt_large.reserve(routes_reduce_scratch_words(G)));
  HIP_TRY(launch_routes_reduce(n_src, V, G, gr.m, gr.ptr, gr.nodes, d.base_dist.p, d.base_nh.p, nb,
                               reinterpret_cast<uint64_t*>(d.rt_bmetric.p), d.rt_bnh.p, nb, nullptr, d.rt_large.p,
                               d.num_cus, s));
  // 4. base alternates
  HIP_TRY(d.wl_balt.reserve(bg * nb));
  HIP_TRY(launch_lfa_table(d.g, d_sources, n_src, d.lf_rowidx.p, d.base_dist.p, d.lf_trow.p, d.lf_ttome.p,
                           d.lf_tfrom.p, d.num_cus, s));
  LfaPass lp{};
  lp.n = n_src;
  lp.V = V;
  lp.G = G;
  lp.M = gr.m;
  lp.onb = nb;
  lp.sources = d_sources;
  lp.row2 = d.g.row2;
  lp.gptr = gr.ptr;
  lp.gnodes = gr.nodes;
  lp.dist = reinterpret_cast<const unsigned long long*>(d.base_dist.p);
  lp.trow = d.lf_trow.p;
  lp.ttome = d.lf_ttome.p;
  lp.tfrom = d.lf_tfrom.p;
  lp.metric = d.rt_bmetric.p;
  lp.nh = d.rt_bnh.p;
  lp.alt = d.wl_balt.p;
  lp.large = d.rt_large.p;
  lp.n_large = d.rt_large.p + G;
  HIP_TRY(launch_lfa_reduce(lp, false, d.num_cus, s));
  // 5. inverse map node -> groups
  HIP_TRY(d.rt_icnt.reserve(V));
  HIP_TRY(d.rt_icur.reserve(V));
  HIP_TRY(d.rt_iptr.reserve((size_t)V + 1u));
  HIP_TRY(d.rt_inv.reserve(std::max<uint32_t>(gr.m, 1u)));
  HIP_TRY(d.rt_tsum.reserve(std::max<size_t>(units, V) / 4096u + 1u));
  HIP_TRY(launch_routes_inverse(V, G, gr.m, gr.ptr, gr.nodes, d.rt_icnt.p, d.rt_icur.p, d.rt_tsum.p, d.rt_iptr.p,
                                d.rt_inv.p, d.num_cus, s));
  // 6. mark pass; 7. count pass, scan, cap check, emit pass
  const WlfaLayout lay = whatif_lfa_layout(G, units, d.num_cus);
  HIP_TRY(d.wl_bm.reserve(std::max<size_t>(lay.bm_words, 1)));
  HIP_TRY(d.wl_bunprot.reserve(n_src));
  HIP_TRY(d.wl_alist.reserve(units));
  HIP_TRY(d.wl_acount.reserve(1));
  unsigned long long* ptr = reinterpret_cast<unsigned long long*>(out.ptr);
  if (!ptr) {
    HIP_TRY(d.wl_optr.reserve(units + 1u));
    ptr = d.wl_optr.p;
  }
  WlfaPass p{};
  p.V = V;
  p.G = G;
  p.M = gr.m;
  p.n_src = n_src;
  p.n_rows = n_rows;
  p.n_sets = un.n;
  p.n_set_links = un.n_set_links;
  p.nb = nb;
  p.onb = out.nhb;
  p.set_ptr = un.set_ptr;
  p.set_links = un.set_links;
  p.sources = d_sources;
  p.row2 = d.g.row2;
  p.adj = d.g.adj;
  p.lid = d.g.lid;
  p.nbr = d.g.nbr;
  p.rowidx = d.lf_rowidx.p;
  p.gptr = gr.ptr;
  p.gnodes = gr.nodes;
  p.iptr = d.rt_iptr.p;
  p.inv = d.rt_inv.p;
  p.nchanged = d.rt_nchanged.p;
  p.nptr = d.rt_nptr.p;
  p.nnode = d.rt_nnode.p;
  p.ndist = d.rt_ndist.p;
  p.nnh = d.rt_nnh.p;
  p.bdist = reinterpret_cast<const unsigned long long*>(d.base_dist.p);
  p.bnh = d.base_nh.p;
  p.trow = d.lf_trow.p;
  p.ttome = d.lf_ttome.p;
  p.bmetric = d.rt_bmetric.p;
  p.bmnh = d.rt_bnh.p;
  p.balt = d.wl_balt.p;
  p.bunprot = d.wl_bunprot.p;
  p.alist = d.wl_alist.p;
  p.acount = d.wl_acount.p;
  p.changed = out.changed;
  p.unprot = out.unprot;
  p.lost = out.lost;
  p.optr = ptr;
  p.ogroup = out.group;
  p.ometric = reinterpret_cast<unsigned long long*>(out.metric);
  p.onh = out.nh;
  p.oalt = out.alt;
  p.g_bm = d.wl_bm.p;
  ElfaPass ep{};
  if (fam >= 0) {
    if (fam == kElfaRestore) {  // the table over every neighbour with a closure row
      HIP_TRY(d.el_trow.reserve(E1));
      HIP_TRY(d.el_ttome.reserve(E1));
      HIP_TRY(launch_elfa_table(d.g, d_sources, n_src, d.lf_rowidx.p, d.base_dist.p, d.el_trow.p, d.el_ttome.p,
                                d.num_cus, s));
      p.trow = d.el_trow.p;
      p.ttome = d.el_ttome.p;
      ep.ev.n_nodes = un.n_nodes;
      ep.ev.n_links = un.n_set_links;
      ep.ev.n_edges = un.n_edges;
      ep.ev.unit_cost = (flags & OPENR_SPF_USE_LINK_METRIC) ? 0u : 1u;
      ep.ev.node_ptr = un.node_ptr;
      ep.ev.nodes = un.nodes;
      ep.ev.link_ptr = un.set_ptr;
      ep.ev.links = un.set_links;
      ep.ev.edge_ptr = un.edge_ptr;
      ep.ev.edges = un.edges;
      ep.ev.metrics = un.metrics;
    }
    ep.w = p;
    ep.idle = idle ? 1u : 0u;
    HIP_TRY(launch_elfa_mark(d.g, ep, fam, d.num_cus, s));
    if (idle) {
      if (out.ptr) HIP_TRY(hipMemsetAsync(out.ptr, 0, (units + 1u) * sizeof(uint64_t), s));
      HIP_TRY(hipStreamSynchronize(s));
      return OPENR_SPF_OK;
    }
    HIP_TRY(launch_elfa(d.g, ep, lay, fam, false, s));
  } else {
    HIP_TRY(launch_wlfa_mark(p, d.num_cus, s));
    HIP_TRY(launch_wlfa(p, lay, false, s));
  }
  HIP_TRY(launch_delta_scan(out.changed, units, d.rt_tsum.p, ptr, s));
  unsigned long long tot = 0;
  HIP_TRY(hipMemcpyAsync(&tot, ptr + units, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *total = tot;
  if (!out.ptr) return OPENR_SPF_OK;  // counts only
  if (tot > out.cap)
    return fail(OPENR_SPF_E2BIG, "%llu entries changed, cap %llu (ptr and the counts are filled, entries are not)", tot,
                (unsigned long long)out.cap);
  if (tot) {
    if (fam >= 0)
      HIP_TRY(launch_elfa(d.g, ep, lay, fam, true, s));
    else
      HIP_TRY(launch_wlfa(p, lay, true, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return OPENR_SPF_OK;
}

// openr_spf_whatif_lfa: sets split in contiguous blocks across the devices, each device's CSR
// appended to the caller's at the running total, each unit's entries sorted by group id.
// fam >= 0: `hu` holds events of that ElfaFamily, which the caller has checked as the family's
// sweep checks them (check_whatif_host below checks their ids again).
int whatif_lfa_host(openr_spf_ctx* ctx, const WhatifUnits& hu, const uint32_t* sources, uint32_t n_sources,
                    uint32_t flags, const openr_spf_groups_t* g, uint32_t* changed, uint32_t* unprotected,
                    uint32_t* lost_backup, openr_spf_whatif_lfa_t* delta, uint64_t* out_solved, int fam = -1) {
  clear_launch_trace();
  const uint32_t n_sets = hu.n;
  if (out_solved) *out_solved = 0;
  if (!ctx) return fail(OPENR_SPF_EINVAL, "null context");
  if (!ctx->has_graph) return fail(OPENR_SPF_EINVAL, "no graph set (openr_spf_set_graph)");
  int rc = check_whatif_host(ctx, hu, sources, n_sources, changed);
  if (rc) return rc;
  if ((rc = check_groups_host(ctx, g)) != OPENR_SPF_OK) return rc;
  if (delta && !delta->ptr) return fail(OPENR_SPF_EINVAL, "null delta->ptr");
  if (delta && delta->cap && (!delta->group || !delta->metric || !delta->nh || !delta->alt))
    return fail(OPENR_SPF_EINVAL, "null delta->group, metric, nh or alt");
  const uint32_t need = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  if (delta && delta->nh_bytes < need) return fail(OPENR_SPF_EINVAL, "nh_bytes %u < required %u", delta->nh_bytes, need);
  if ((rc = check_routes_metric(ctx, flags)) != OPENR_SPF_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t nhb = delta ? delta->nh_bytes : need;
  const uint64_t cap = delta ? delta->cap : 0u;
  std::vector<uint32_t> rebased, idx;
  std::vector<uint64_t> ptr;
  const uint32_t nd = (uint32_t)ctx->devs.size();
  const uint32_t per = (n_sets + nd - 1) / std::max<uint32_t>(nd, 1);
  uint64_t solved_total = 0, at = 0;
  bool over = false;
  if (delta) delta->ptr[0] = 0;
  for (uint32_t di = 0; di < nd; ++di) {
    Device& d = ctx->devs[di];
    const uint32_t b = std::min(n_sets, di * per), e = std::min(n_sets, b + per), m = e - b;
    if (!m || !n_sources) continue;
    const size_t mu = (size_t)m * n_sources, uo = (size_t)b * n_sources;
    HIP_TRY(hipSetDevice(d.ordinal));
    WhatifUnits un;
    if ((rc = upload_whatif_units(d, hu, b, m, &rebased, &un)) != OPENR_SPF_OK) return rc;
    DevGroups gr;
    if ((rc = upload_groups(d, g, &gr)) != OPENR_SPF_OK) return rc;
    HIP_TRY(d.win_src.reserve(n_sources));
    HIP_TRY(d.wl_ochanged.reserve(mu));
    HIP_TRY(d.wl_ounprot.reserve(mu));
    HIP_TRY(d.wl_olost.reserve(mu));
    HIP_TRY(d.wl_optr.reserve(mu + 1));
    HIP_TRY(hipMemcpyAsync(d.win_src.p, sources, n_sources * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    // the device's entries land in library buffers sized to the room left in the caller's
    const uint64_t room = cap > at ? cap - at : 0;
    if (delta) {
      HIP_TRY(d.wl_ogroup.reserve(std::max<uint64_t>(room, 1)));
      HIP_TRY(d.wl_ometric.reserve(std::max<uint64_t>(room, 1)));
      HIP_TRY(d.wl_onh.reserve(std::max<uint64_t>(room * nhb, 1)));
      HIP_TRY(d.wl_oalt.reserve(std::max<uint64_t>(room * nhb, 1)));
    }
    WlfaOut out;
    out.changed = d.wl_ochanged.p;
    out.unprot = unprotected ? d.wl_ounprot.p : nullptr;
    out.lost = lost_backup ? d.wl_olost.p : nullptr;
    out.ptr = delta ? reinterpret_cast<uint64_t*>(d.wl_optr.p) : nullptr;
    out.group = d.wl_ogroup.p;
    out.metric = reinterpret_cast<uint64_t*>(d.wl_ometric.p);
    out.nh = d.wl_onh.p;
    out.alt = d.wl_oalt.p;
    out.cap = room;
    out.nhb = nhb;
    uint64_t total = 0, solved = 0;
    rc = whatif_lfa_on_device(ctx, d, un, d.win_src.p, n_sources, flags, gr, out, d.stream, &total, &solved, fam);
    if (rc && rc != OPENR_SPF_E2BIG) return rc;
    over |= rc == OPENR_SPF_E2BIG;
    solved_total += solved;
    HIP_TRY(hipMemcpyAsync(changed + uo, d.wl_ochanged.p, mu * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
    if (unprotected)
      HIP_TRY(hipMemcpyAsync(unprotected + uo, d.wl_ounprot.p, mu * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
    if (lost_backup)
      HIP_TRY(hipMemcpyAsync(lost_backup + uo, d.wl_olost.p, mu * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
    const bool fits = delta && !over && total <= room;
    if (delta) {
      ptr.resize(mu + 1);
      HIP_TRY(hipMemcpyAsync(ptr.data(), d.wl_optr.p, (mu + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
    }
    if (fits && total) {
      HIP_TRY(hipMemcpyAsync(delta->group + at, d.wl_ogroup.p, total * 4u, hipMemcpyDeviceToHost, d.stream));
      HIP_TRY(hipMemcpyAsync(delta->metric + at, d.wl_ometric.p, total * 8u, hipMemcpyDeviceToHost, d.stream));
      HIP_TRY(hipMemcpyAsync(delta->nh + at * nhb, d.wl_onh.p, total * nhb, hipMemcpyDeviceToHost, d.stream));
      HIP_TRY(hipMemcpyAsync(delta->alt + at * nhb, d.wl_oalt.p, total * nhb, hipMemcpyDeviceToHost, d.stream));
    }
    HIP_TRY(hipStreamSynchronize(d.stream));
    for (size_t u = 0; delta && u < mu; ++u) {
      delta->ptr[uo + u + 1] = at + ptr[u + 1];
      const uint32_t c = (uint32_t)(ptr[u + 1] - ptr[u]);
      if (!fits || c < 2) continue;
      // each unit's groups ascending (the device keeps the kernel's order)
      const uint64_t o = at + ptr[u];
      idx.resize(c);
      for (uint32_t k = 0; k < c; ++k) idx[k] = k;
      std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return delta->group[o + x] < delta->group[o + y]; });
      std::vector<uint32_t> tg(c);
      std::vector<uint64_t> tm(c);
      std::vector<uint8_t> th((size_t)c * nhb), ta((size_t)c * nhb);
      for (uint32_t k = 0; k < c; ++k) {
        tg[k] = delta->group[o + idx[k]];
        tm[k] = delta->metric[o + idx[k]];
        std::memcpy(&th[(size_t)k * nhb], delta->nh + (o + idx[k]) * nhb, nhb);
        std::memcpy(&ta[(size_t)k * nhb], delta->alt + (o + idx[k]) * nhb, nhb);
      }
      std::memcpy(delta->group + o, tg.data(), c * 4u);
      std::memcpy(delta->metric + o, tm.data(), c * 8u);
      std::memcpy(delta->nh + o * nhb, th.data(), (size_t)c * nhb);
      std::memcpy(delta->alt + o * nhb, ta.data(), (size_t)c * nhb);
    }
    at += total;
  }
  ctx->stats.last_batch_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (out_solved) *out_solved = solved_total;
  if (delta && (over || at > cap))
    return fail(OPENR_SPF_E2BIG, "%llu entries changed, cap %llu (ptr and the counts are filled, entries are not)",
                (unsigned long long)at, (unsigned long long)cap);
  return OPENR_SPF_OK;
}

// ---- the call forms of the event families: one body each ------------------------------------
// A public function builds its units (device forms) or names its family and calls one of these.

// metric_hops in host memory (delta: the caller's openr_spf_whatif_delta_t or _routes_t, nullable).
template <class Delta>
int metric_hops_host(uint32_t n_events, uint32_t n_sources, uint32_t* changed, Delta* delta, uint64_t* out_solved) {
  if (delta && !delta->ptr) return fail(OPENR_SPF_EINVAL, "null delta->ptr");
  const size_t units = (size_t)n_events * n_sources;
  if (units) std::memset(changed, 0, units * sizeof(uint32_t));
  if (delta) std::memset(delta->ptr, 0, (units + 1) * sizeof(uint64_t));
  if (out_solved) *out_solved = 0;
  return OPENR_SPF_OK;
}

// metric_hops in device memory.
int metric_hops_device(openr_spf_ctx* ctx, int device_index, uint32_t n_events, uint32_t n_sources,
                       uint32_t* d_changed, uint64_t* d_ptr, void* stream, uint64_t* out_total,
                       uint64_t* out_solved) {
  Device& d = ctx->devs[device_index];
  HIP_TRY(hipSetDevice(d.ordinal));
  hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : d.stream;
  const size_t units = (size_t)n_events * n_sources;
  if (units) HIP_TRY(hipMemsetAsync(d_changed, 0, units * sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(d_ptr, 0, (units + 1) * sizeof(uint64_t), s));
  HIP_TRY(hipStreamSynchronize(s));
  if (out_total) *out_total = 0;
  if (out_solved) *out_solved = 0;
  return OPENR_SPF_OK;
}

// openr_spf_whatif_<family>
template <class Events>
int event_host(openr_spf_ctx* ctx, int fam, const Events* ev, const uint32_t* sources, uint32_t n_sources,
               uint32_t flags, uint32_t* changed, openr_spf_whatif_delta_t* delta, uint64_t* out_solved) {
  clear_launch_trace();
  WhatifUnits hu;
  const int rc = check_events_host(ctx, fam, ev, sources, n_sources, flags, changed, &hu);
  if (rc) return rc;
  if (metric_hops(fam, flags)) return metric_hops_host(hu.n, n_sources, changed, delta, out_solved);
  if (!delta) return whatif_host(ctx, hu, sources, n_sources, flags, changed, out_solved);
  return whatif_delta_host(ctx, hu, sources, n_sources, flags, changed, delta, out_solved);
}

// openr_spf_whatif_<family>_routes
template <class Events>
int event_routes_host(openr_spf_ctx* ctx, int fam, const Events* ev, const uint32_t* sources, uint32_t n_sources,
                      uint32_t flags, const openr_spf_groups_t* groups, uint32_t* changed_routes,
                      openr_spf_whatif_routes_t* delta, uint64_t* out_solved) {
  clear_launch_trace();
  WhatifUnits hu;
  int rc = check_events_host(ctx, fam, ev, sources, n_sources, flags, changed_routes, &hu);
  if (rc) return rc;
  if (metric_hops(fam, flags)) {
    if ((rc = check_groups_host(ctx, groups)) != OPENR_SPF_OK) return rc;
    return metric_hops_host(hu.n, n_sources, changed_routes, delta, out_solved);
  }
  return whatif_routes_host(ctx, hu, sources, n_sources, flags, groups, changed_routes, delta, out_solved);
}

// The family's capacity check for a call whose only E2BIG is "sum(changed) > cap": a graph
// whose repair unit does not fit LDS is not supported by these calls.
int event_lfa_check(int rc) { return rc == OPENR_SPF_E2BIG ? OPENR_SPF_ENOTSUP : rc; }

// openr_spf_whatif_<family>_lfa (whatif_lfa_host clears the launch trace)
template <class Events>
int event_lfa_host(openr_spf_ctx* ctx, int fam, const Events* ev, const uint32_t* sources, uint32_t n_sources,
                   uint32_t flags, const openr_spf_groups_t* groups, uint32_t* changed, uint32_t* unprotected,
                   uint32_t* lost_backup, openr_spf_whatif_lfa_t* delta, uint64_t* out_solved) {
  if (out_solved) *out_solved = 0;
  WhatifUnits hu;
  const int rc = event_lfa_check(check_events_host(ctx, fam, ev, sources, n_sources, flags, changed, &hu));
  if (rc) return rc;
  return whatif_lfa_host(ctx, hu, sources, n_sources, flags, groups, changed, unprotected, lost_backup, delta,
                         out_solved, fam);
}

// openr_spf_whatif_<family>_device (un: the events in device memory). The family's check comes
// before device_index is looked at.
int event_device(openr_spf_ctx* ctx, int device_index, const WhatifUnits& un, int fam, const uint32_t* d_sources,
                 uint32_t n_sources, uint32_t flags, uint32_t* d_changed, uint64_t* d_ptr, uint32_t* d_node,
                 uint64_t* d_dist, uint8_t* d_nh, uint64_t cap, uint32_t nh_bytes, void* stream, uint64_t* out_total,
                 uint64_t* out_solved) {
  clear_launch_trace();
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (event_pointer_missing(un)) return fail(OPENR_SPF_EINVAL, "an event pointer is null where its count is not");
  if ((rc = check_family(ctx, fam, flags, un.n, n_sources)) != OPENR_SPF_OK) return rc;
  if (metric_hops(fam, flags)) {
    if ((rc = check_device_index(ctx, device_index)) != OPENR_SPF_OK) return rc;
    if ((n_sources && !d_sources) || (un.n && n_sources && !d_changed) || !d_ptr)
      return fail(OPENR_SPF_EINVAL, "null sources, changed or ptr");
    return metric_hops_device(ctx, device_index, un.n, n_sources, d_changed, d_ptr, stream, out_total, out_solved);
  }
  return whatif_delta_device_form(ctx, device_index, un, d_sources, n_sources, flags, d_changed, d_ptr, d_node, d_dist,
                                  d_nh, cap, nh_bytes, stream, out_total, out_solved);
}

// openr_spf_whatif_routes_device (fam < 0: un holds link sets) and openr_spf_whatif_<family>_routes_device
// (un: the events in device memory). device_index and the null pointers come before the
// family's check here.
int whatif_routes_device_form(openr_spf_ctx* ctx, int device_index, const WhatifUnits& un, int fam,
                              const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                              const uint32_t* d_group_ptr, const uint32_t* d_group_nodes, uint32_t n_groups,
                              uint32_t n_group_nodes, uint32_t* d_changed_routes, uint64_t* d_ptr, uint32_t* d_group,
                              uint64_t* d_metric, uint8_t* d_nh, uint32_t* d_n_best, uint64_t cap, uint32_t nh_bytes,
                              void* stream, uint64_t* out_total, uint64_t* out_solved) {
  clear_launch_trace();
  int rc = check_ctx(ctx);
  if (rc || (rc = check_device_index(ctx, device_index))) return rc;
  if ((fam < 0 ? un.n && !un.set_ptr : event_pointer_missing(un)) || (n_sources && !d_sources) ||
      (un.n && n_sources && !d_changed_routes) || !d_ptr)
    return fail(OPENR_SPF_EINVAL, "null units, sources, changed_routes or ptr");
  if ((n_groups && !d_group_ptr) || (n_group_nodes && !d_group_nodes))
    return fail(OPENR_SPF_EINVAL, "null group_ptr or group_nodes");
  if (cap && (!d_group || !d_metric || !d_nh)) return fail(OPENR_SPF_EINVAL, "null route buffer");
  rc = fam < 0 ? check_routes_metric(ctx, flags) : check_family(ctx, fam, flags, un.n, n_sources);
  if (rc) return rc;
  if (metric_hops(fam, flags))
    return metric_hops_device(ctx, device_index, un.n, n_sources, d_changed_routes, d_ptr, stream, out_total,
                              out_solved);
  Device& d = ctx->devs[device_index];
  HIP_TRY(hipSetDevice(d.ordinal));
  DevGroups gr;
  gr.ptr = d_group_ptr;
  gr.nodes = d_group_nodes;
  gr.n = n_groups;
  gr.m = n_group_nodes;
  uint64_t total = 0, solved = 0;
  rc = whatif_routes_on_device(ctx, d, un, d_sources, n_sources, flags, gr, d_changed_routes, d_ptr, d_group, d_metric,
                               d_nh, d_n_best, cap, nh_bytes,
                               stream ? reinterpret_cast<hipStream_t>(stream) : d.stream, &total, &solved);
  if (out_total) *out_total = total;
  if (out_solved) *out_solved = solved;
  return rc;
}

// openr_spf_whatif_<family>_lfa_device (un: events of ElfaFamily fam in device memory). The
// family's check comes before device_index is looked at.
int event_lfa_device(openr_spf_ctx* ctx, int device_index, const WhatifUnits& un, int fam,
                     const uint32_t* d_sources, uint32_t n_sources, uint32_t flags, const uint32_t* d_group_ptr,
                     const uint32_t* d_group_nodes, uint32_t n_groups, uint32_t n_group_nodes, uint32_t* d_changed,
                     uint32_t* d_unprotected, uint32_t* d_lost_backup, uint64_t* d_ptr, uint32_t* d_group,
                     uint64_t* d_metric, uint8_t* d_nh, uint8_t* d_alt, uint64_t cap, uint32_t nh_bytes, void* stream,
                     uint64_t* out_total, uint64_t* out_solved) {
  clear_launch_trace();
  if (out_total) *out_total = 0;
  if (out_solved) *out_solved = 0;
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (event_pointer_missing(un)) return fail(OPENR_SPF_EINVAL, "an event pointer is null where its count is not");
  if ((rc = event_lfa_check(check_family(ctx, fam, flags, un.n, n_sources))) != OPENR_SPF_OK) return rc;
  if ((rc = check_device_index(ctx, device_index)) != OPENR_SPF_OK) return rc;
  if ((n_sources && !d_sources) || (un.n && n_sources && !d_changed))
    return fail(OPENR_SPF_EINVAL, "null sources or changed");
  if ((n_groups && !d_group_ptr) || (n_group_nodes && !d_group_nodes))
    return fail(OPENR_SPF_EINVAL, "null group_ptr or group_nodes");
  if (cap && (!d_ptr || !d_group || !d_metric || !d_nh || !d_alt)) return fail(OPENR_SPF_EINVAL, "null entry buffer");
  if ((rc = check_routes_metric(ctx, flags)) != OPENR_SPF_OK) return rc;
  Device& d = ctx->devs[device_index];
  HIP_TRY(hipSetDevice(d.ordinal));
  DevGroups gr;
  gr.ptr = d_group_ptr;
  gr.nodes = d_group_nodes;
  gr.n = n_groups;
  gr.m = n_group_nodes;
  WlfaOut out;
  out.changed = d_changed;
  out.unprot = d_unprotected;
  out.lost = d_lost_backup;
  out.ptr = d_ptr;
  out.group = d_group;
  out.metric = d_metric;
  out.nh = d_nh;
  out.alt = d_alt;
  out.cap = cap;
  out.nhb = nh_bytes;
  uint64_t total = 0, solved = 0;
  rc = whatif_lfa_on_device(ctx, d, un, d_sources, n_sources, flags, gr, out,
                            stream ? reinterpret_cast<hipStream_t>(stream) : d.stream, &total, &solved, fam);
  if (out_total) *out_total = total;
  if (out_solved) *out_solved = solved;
  return rc;
}


}  // namespace

extern "C" {

int openr_spf_abi_version(void) { return OPENR_SPF_ABI_VERSION; }

const char* openr_spf_last_error(void) { return g_last_error.c_str(); }

int openr_spf_host_alloc(size_t bytes, void** out) {
  if (!out) return fail(OPENR_SPF_EINVAL, "openr_spf_host_alloc: null out");
  *out = nullptr;
  const hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
  if (e != hipSuccess) {
    *out = nullptr;
    return fail(OPENR_SPF_ENOMEM, "openr_spf_host_alloc: %s", hipGetErrorString(e));
  }
  return OPENR_SPF_OK;
}

void openr_spf_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

const char* openr_spf_last_kernels(void) { return g_launch_trace.c_str(); }

void openr_spf_limits(openr_spf_limits_t* out) {
  if (!out) return;
  // Largest V whose LDS-resident BFS state (<= 8 next-hop bits, no ignore set) fits a CU.
  uint32_t lo = 1, hi = 65535;
  while (lo < hi) {
    uint32_t mid = (lo + hi + 1) / 2;
    if (bfs_lds_bytes(kFamCode, mid, 0, false, kCls8)) lo = mid;
    else hi = mid - 1;
  }
  out->max_nodes = lo;
  out->max_nh_bits = 65535;  // wider than 256: the exact-order kernel
}

int openr_spf_create(const int* device_ids, int n_devices, openr_spf_ctx** out) {
  if (!out) return fail(OPENR_SPF_EINVAL, "null out");
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(OPENR_SPF_ENODEV, "no HIP device available (%s); the engine has no CPU path",
                e == hipSuccess ? "count=0" : hipGetErrorString(e));
  std::vector<int> ids;
  if (!device_ids || n_devices <= 0) {
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    ids.push_back(cur);
  } else {
    for (int i = 0; i < n_devices; ++i) {
      if (device_ids[i] < 0 || device_ids[i] >= count)
        return fail(OPENR_SPF_EINVAL, "device id %d out of range (count=%d)", device_ids[i], count);
      ids.push_back(device_ids[i]);
    }
  }
  auto* ctx = new (std::nothrow) openr_spf_ctx();
  if (!ctx) return fail(OPENR_SPF_ENOMEM, "out of host memory");
  for (int id : ids) {
    Device d;
    d.ordinal = id;
    hipDeviceProp_t prop;
    if (hipSetDevice(id) != hipSuccess || hipGetDeviceProperties(&prop, id) != hipSuccess ||
        hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&d.ev_begin) != hipSuccess || hipEventCreate(&d.ev_end) != hipSuccess) {
      openr_spf_destroy(ctx);
      return fail(OPENR_SPF_ENODEV, "failed to initialise HIP device %d", id);
    }
    d.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    ctx->devs.push_back(d);
  }
  *out = ctx;
  return OPENR_SPF_OK;
}

void openr_spf_destroy(openr_spf_ctx* ctx) {
  if (!ctx) return;
  for (Device& d : ctx->devs) {
    (void)hipSetDevice(d.ordinal);
    if (d.stream) (void)hipStreamSynchronize(d.stream);
    free_graph(d.g);
    d.src.release();
    d.ign_ptr.release();
    d.ign_links.release();
    d.dist.release();
    d.tight.release();
    d.nh.release();
    d.ovf.release();
    d.slicetmp.release();
    d.work.release();
    d.status.release();
    d.perm.release();
    d.part.release();
    d.dv_member.release();
    d.dv_nbrs.release();
    d.dv_perm.release();
    d.dv_part.release();
    d.dv_valid.release();
    d.dv_flags.release();
    d.dv_rows.release();
    d.kkeep.release();
    d.ktloff.release();
    d.ktlent.release();
    d.kpart.release();
    d.dl_off.release();
    d.dl_node.release();
    d.dl_dist.release();
    d.dl_used.release();
    d.dl_nh.release();
    d.dl_tsum.release();
    d.dlo_ptr.release();
    d.dlo_dist.release();
    d.dlo_node.release();
    d.dlo_nh.release();
    d.wbeg.release();
    d.wend.release();
    d.win_ptr.release();
    void* routes[] = {d.rt_nptr.p,  d.rt_ndist.p, d.rt_bmetric.p,  d.rt_iptr.p,   d.rt_tsum.p,   d.rt_optr.p,
                      d.rt_ometric.p, d.rt_nchanged.p, d.rt_nnode.p, d.rt_inv.p,    d.rt_icnt.p,   d.rt_icur.p,
                      d.rt_large.p, d.rt_ovl.p,   d.rt_bm.p,       d.rt_gptr.p,   d.rt_gnodes.p, d.rt_ochanged.p,
                      d.rt_ogroup.p, d.rt_onbest.p, d.rt_nnh.p,     d.rt_bnh.p,    d.rt_onh.p};
    for (void* p : routes)
      if (p) (void)hipFree(p);
    void* lfa[] = {d.lf_need.p,  d.lf_srcbm.p, d.lf_cnt.p,  d.lf_list.p,  d.lf_rowidx.p, d.lf_trow.p,
                   d.lf_nalt.p,  d.lf_onbr.p,  d.lf_wptr.p, d.lf_tsum.p,  d.lf_ttome.p,  d.lf_tfrom.p,
                   d.lf_optr.p,  d.lf_oam.p,   d.lf_nh.p,   d.lf_alt.p};
    for (void* p : lfa)
      if (p) (void)hipFree(p);
    void* wlfa[] = {d.wl_clos.p,     d.wl_bunprot.p, d.wl_alist.p,  d.wl_acount.p, d.wl_bm.p,
                    d.wl_ochanged.p, d.wl_ounprot.p, d.wl_olost.p,  d.wl_ogroup.p, d.wl_optr.p,
                    d.wl_ometric.p,  d.wl_balt.p,    d.wl_onh.p,    d.wl_oalt.p};
    for (void* p : wlfa)
      if (p) (void)hipFree(p);
    void* sweep[] = {d.base_dist.p, d.base_tight.p, d.wdist.p, d.base_nh.p, d.wnh.p, d.wsrc.p, d.wlink.p,
                     d.wunit.p,     d.wcount.p,     d.wiota.p, d.base_tin.p, d.win_links.p, d.win_src.p, d.wchanged.p, d.wchanged_t.p,
                     d.kbase.p,     d.krows.p,      d.krows16.p, d.kign.p,  d.kend.p, d.ksrc.p,      d.kptr.p,    d.kstatus.p,
                     d.kin_src.p,   d.kin_row.p,    d.kin_dst.p, d.ktok1.p,   d.ktok2.p,   d.kq.p, d.kretry.p};
    for (void* p : sweep)
      if (p) (void)hipFree(p);
    d.win_nodes.release();
    d.win_lptr.release();
    d.exscratch.release();
    d.order.release();
    d.precs.release();
    d.delta.release();
    d.alist.release();
    d.asrc.release();
    d.alist2.release();
    d.asrc2.release();
    d.acount.release();
    if (d.ev_begin) (void)hipEventDestroy(d.ev_begin);
    if (d.ev_end) (void)hipEventDestroy(d.ev_end);
    if (d.stream) (void)hipStreamDestroy(d.stream);
  }
  delete ctx;
}

int openr_spf_set_graph(openr_spf_ctx* ctx, const openr_spf_graph* gr) {
  if (!ctx || !gr) return fail(OPENR_SPF_EINVAL, "null argument");
  const uint32_t V = gr->num_nodes, E = gr->num_dir_edges, L = gr->num_links;
  if (!gr->row_ptr || !gr->node_overloaded || !gr->name_rank || (E && (!gr->col || !gr->metric || !gr->link_id ||
                                                                      !gr->edge_up)))
    return fail(OPENR_SPF_EINVAL, "null graph array");
  if (V >= kNodeSink || E >= kNodeSink) return fail(OPENR_SPF_E2BIG, "too many nodes or edges");
  if (gr->row_ptr[0] != 0 || gr->row_ptr[V] != E) return fail(OPENR_SPF_EINVAL, "row_ptr must span [0, E]");
  for (uint32_t u = 0; u < V; ++u)
    if (gr->row_ptr[u + 1] < gr->row_ptr[u]) return fail(OPENR_SPF_EINVAL, "row_ptr not monotone at %u", u);

  std::vector<uint32_t> adj(E), w(E), win(E), rev(E), lid(E), owner(E);
  std::vector<uint16_t> nbr(E);
  std::vector<uint8_t> ovl(V);
  // link id -> its two directed edges
  std::vector<uint32_t> first(L, UINT32_MAX), second(L, UINT32_MAX);
  std::vector<uint2> ledge(L);
  uint32_t nh_bits = 0, w_min = UINT32_MAX, w_max = 0;
  bool metric_ok = true;
  std::vector<uint32_t> seen_stamp(V, UINT32_MAX), seen_idx(V, 0);
  for (uint32_t u = 0; u < V; ++u) {
    ovl[u] = gr->node_overloaded[u] ? 1 : 0;
    uint32_t nd = 0;
    for (uint32_t e = gr->row_ptr[u]; e < gr->row_ptr[u + 1]; ++e) {
      const uint32_t v = gr->col[e], l = gr->link_id[e];
      if (v >= V) return fail(OPENR_SPF_EINVAL, "col[%u]=%u out of range", e, v);
      if (l >= L) return fail(OPENR_SPF_EINVAL, "link_id[%u]=%u out of range", e, l);
      owner[e] = u;
      if (seen_stamp[v] != u) {
        seen_stamp[v] = u;
        seen_idx[v] = nd++;
      }
      nbr[e] = (uint16_t)std::min<uint32_t>(seen_idx[v], 0xFFFFu);
      if (first[l] == UINT32_MAX) first[l] = e;
      else if (second[l] == UINT32_MAX) second[l] = e;
      else return fail(OPENR_SPF_EINVAL, "link %u appears more than twice", l);
      lid[e] = l;
      const bool up = gr->edge_up[e] != 0;
      adj[e] = v | (up ? 0u : kEdgeDown);
      const uint64_t m = gr->metric[e];
      w[e] = (uint32_t)std::min<uint64_t>(m, 0xFFFFFFFFull);
      if (up) {
        if (m == 0 || m > 0x7FFFFFFFull) metric_ok = false;
        else {
          w_min = std::min<uint32_t>(w_min, (uint32_t)m);
          w_max = std::max<uint32_t>(w_max, (uint32_t)m);
        }
      }
    }
    nh_bits = std::max(nh_bits, nd);
  }
  for (uint32_t l = 0; l < L; ++l) {
    if (first[l] == UINT32_MAX) continue;  // unused id
    const uint32_t a = first[l], b = second[l];
    if (b == UINT32_MAX) return fail(OPENR_SPF_EINVAL, "link %u has a single direction", l);
    if (gr->col[a] != owner[b] || gr->col[b] != owner[a])
      return fail(OPENR_SPF_EINVAL, "link %u directions do not mirror each other", l);
    if ((gr->edge_up[a] != 0) != (gr->edge_up[b] != 0))
      return fail(OPENR_SPF_EINVAL, "link %u edge_up differs by direction (Link::isUp is per link)", l);
    rev[a] = b;
    rev[b] = a;
    ledge[l] = make_uint2(a, b);
  }
  for (uint32_t e = 0; e < E; ++e) win[e] = w[rev[e]];
  for (uint32_t l = 0; l < L; ++l)
    if (first[l] == UINT32_MAX) ledge[l] = make_uint2(UINT32_MAX, UINT32_MAX);  // unused id: never affected
  // transit views: an overloaded node is reached but never expanded unless it is the
  // source (LinkState.cpp:831-838), so its transit row is empty / all-down
  std::vector<uint2> row2(V), row2t(V);
  std::vector<uint4> ellt(V), erec(E);
  for (uint32_t e = 0; e < E; ++e)
    erec[e] = make_uint4(adj[e] | (ovl[gr->col[e]] ? kNodeSink : 0u), win[e], lid[e], rev[e]);
  // rank-sorted copy of every row's in-edge records (KSP tracer, uniform cost)
  std::vector<uint32_t> erec_pos(E);
  {
    std::vector<uint32_t> idx;
    for (uint32_t u = 0; u < V; ++u) {
      const uint32_t b = gr->row_ptr[u], e1 = gr->row_ptr[u + 1];
      idx.resize(e1 - b);
      for (uint32_t e = b; e < e1; ++e) idx[e - b] = e;
      std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
        const uint32_t rx = gr->name_rank[gr->col[x]], ry = gr->name_rank[gr->col[y]];
        return rx != ry ? rx < ry : rev[x] < rev[y];
      });
      for (uint32_t i = 0; i < idx.size(); ++i) erec_pos[idx[i]] = b + i;
    }
  }
  for (uint32_t u = 0; u < V; ++u) {
    uint32_t x[4] = {kEdgeDown, kEdgeDown, kEdgeDown, kEdgeDown};
    if (!ovl[u])
      for (uint32_t j = 0; j < 4 && gr->row_ptr[u] + j < gr->row_ptr[u + 1]; ++j) x[j] = adj[gr->row_ptr[u] + j];
    else
      x[0] |= kNodeSink;
    ellt[u] = make_uint4(x[0], x[1], x[2], x[3]);
  }
  std::vector<uint32_t> ovl_bits((V + 31) / 32 + 1, 0);
  for (uint32_t u = 0; u < V; ++u) {
    row2[u] = make_uint2(gr->row_ptr[u], gr->row_ptr[u + 1]);
    row2t[u] = ovl[u] ? make_uint2(gr->row_ptr[u] | kNodeSink, gr->row_ptr[u]) : row2[u];
    if (ovl[u]) ovl_bits[u >> 5] |= 1u << (u & 31u);
  }
  // next-hop sets wider than 256 bits: only the exact-order kernel serves them (make_plan)
  // source class of every node (distinct degree -> next-hop width)
  std::vector<uint8_t> cls[kNumFamilies];
  uint32_t cls_mask[kNumFamilies] = {0, 0}, sliced_deg[kNumFamilies] = {0, 0};
  for (int f = 0; f < kNumFamilies; ++f) cls[f].resize(V);
  for (uint32_t u = 0; u < V; ++u) {
    uint32_t nd = 0;
    for (uint32_t e = gr->row_ptr[u]; e < gr->row_ptr[u + 1]; ++e) nd = std::max<uint32_t>(nd, nbr[e] + 1u);
    for (int f = 0; f < kNumFamilies; ++f) {
      const int c = std::max(0, src_class_for_degree(f, std::min<uint32_t>(nd, 256u)));
      cls[f][u] = (uint8_t)c;
      cls_mask[f] |= 1u << c;
      if (c == sliced_class(f)) sliced_deg[f] = std::max(sliced_deg[f], nd);
    }
  }
  for (int f = 0; f < kNumFamilies; ++f)
    if (!cls_mask[f]) cls_mask[f] = 1u;  // no node: class 0
  const FrontierEstimate est = estimate_frontier(V, gr->row_ptr, adj.data(), ovl.data());
  if (w_min == UINT32_MAX) w_min = w_max = 1;  // no usable edge
  // derive colouring (spf_derive.hip): greedy in node-id order, a node is derivable iff no
  // structural neighbour (link up or down) already is and it has at most kDeriveMaxNbrs
  // distinct neighbours. Independent in the link structure, so patches (attributes only)
  // keep it valid; on a row-major grid it is the checkerboard.
  std::vector<uint8_t> derivable(V, 0);
  for (uint32_t u = 0; u < V; ++u) {
    bool ok = true;
    uint32_t nd = 0;
    for (uint32_t e = gr->row_ptr[u]; e < gr->row_ptr[u + 1] && ok; ++e) {
      nd = std::max<uint32_t>(nd, nbr[e] + 1u);
      ok = gr->col[e] == u || !derivable[gr->col[e]];
    }
    derivable[u] = ok && nd <= kDeriveMaxNbrs;
  }

  for (Device& d : ctx->devs) {
    HIP_TRY(hipSetDevice(d.ordinal));
    HIP_TRY(hipStreamSynchronize(d.stream));
    free_graph(d.g);
    d.ktag_rows = 0;  // tagged KSP2 rows of another graph (another level width): zero before reuse
    DevGraph g;
    g.V = V;
    g.E = E;
    g.L = L;
    for (uint32_t u = 0; u < V; ++u) g.max_deg = std::max(g.max_deg, gr->row_ptr[u + 1] - gr->row_ptr[u]);
    g.est_width2 = est.width2;
    g.est_width1 = est.width1;
    g.est_depth = est.depth;
    auto up = [&](auto** dst, const auto* srcp, size_t count) -> hipError_t {
      using T = std::remove_pointer_t<std::remove_pointer_t<decltype(dst)>>;
      hipError_t err = hipMalloc(reinterpret_cast<void**>(dst), std::max<size_t>(count, 1) * sizeof(T));
      if (err != hipSuccess) return err;
      if (count) err = hipMemcpy(*dst, srcp, count * sizeof(T), hipMemcpyHostToDevice);
      return err;
    };
    hipError_t err = up(&g.row, gr->row_ptr, V + 1);
    if (err == hipSuccess) err = up(&g.row2, row2.data(), V);
    if (err == hipSuccess) err = up(&g.row2t, row2t.data(), V);
    if (err == hipSuccess) err = up(&g.ovl_bits, ovl_bits.data(), ovl_bits.size());
    if (err == hipSuccess) err = up(&g.ellt, ellt.data(), V);
    if (err == hipSuccess) {
      // [V] = sentinel row (lean BFS pass)
      std::vector<uint4> ellv(ellv_rows(V), make_uint4(V, V, V, V));
      for (uint32_t u = 0; u < V; ++u) ellv[u] = ellv_of(ellt[u], V);
      err = up(&g.ellv, ellv.data(), ellv.size());
      // delta rows (wave pass): every row of <= 4 edges and every column within 127 ids of
      // its row, down edges and overloaded rows included (a patch may bring them back)
      bool delta_ok = true;
      for (uint32_t u = 0; u < V && delta_ok; ++u) {
        delta_ok = gr->row_ptr[u + 1] - gr->row_ptr[u] <= 4u;
        for (uint32_t e = gr->row_ptr[u]; e < gr->row_ptr[u + 1] && delta_ok; ++e) {
          const int32_t dlt = (int32_t)gr->col[e] - (int32_t)u;
          delta_ok = dlt >= -127 && dlt <= 127;
        }
      }
      if (err == hipSuccess && delta_ok) {
        std::vector<uint32_t> elld(V);
        for (uint32_t u = 0; u < V; ++u) elld[u] = elld_of(ellv[u], u, V);
        err = up(&g.elld, elld.data(), V);
      }
    }
    if (err == hipSuccess) err = up(&g.erec, erec.data(), E);
    if (err == hipSuccess) {
      std::vector<uint4> erecs(E);
      for (uint32_t e = 0; e < E; ++e) erecs[erec_pos[e]] = erec[e];
      err = up(&g.erecs, erecs.data(), E);
    }
    if (err == hipSuccess) err = up(&g.adj, adj.data(), E);
    if (err == hipSuccess) err = up(&g.w, w.data(), E);
    if (err == hipSuccess) err = up(&g.w64, gr->metric, E);
    if (err == hipSuccess) err = up(&g.win, win.data(), E);
    if (err == hipSuccess) err = up(&g.rev, rev.data(), E);
    if (err == hipSuccess) err = up(&g.lid, lid.data(), E);
    if (err == hipSuccess) err = up(&g.nbr, nbr.data(), E);
    if (err == hipSuccess) err = up(&g.ovl, ovl.data(), V);
    if (err == hipSuccess) err = up(&g.derivable, derivable.data(), V);
    if (err == hipSuccess) err = up(&g.cls, cls[kFamCode].data(), V);
    if (err == hipSuccess) err = up(&g.cls_lvl, cls[kFamLvl].data(), V);
    if (err == hipSuccess) err = up(&g.ledge, ledge.data(), L);
    if (err == hipSuccess) err = up(&g.rank, gr->name_rank, V);
    d.g = g;
    if (err != hipSuccess) {
      ctx->has_graph = false;
      return fail(OPENR_SPF_ENOMEM, "graph upload failed: %s", hipGetErrorString(err));
    }
  }
  ctx->V = V;
  ctx->E = E;
  ctx->L = L;
  ctx->row_ptr.assign(gr->row_ptr, gr->row_ptr + V + 1);
  ctx->col.assign(gr->col, gr->col + E);
  ctx->nh_bits = nh_bits;
  ctx->w_min = w_min;
  ctx->w_max = w_max;
  ctx->metric_ok = metric_ok;
  ctx->family = est.family();
  ctx->est_depth = est.depth;
  for (int f = 0; f < kNumFamilies; ++f) {
    ctx->cls_mask[f] = cls_mask[f];
    ctx->nsl[f] = std::max<uint32_t>(1u, (sliced_deg[f] + slice_bits(f) - 1u) / slice_bits(f));
  }
  // lanes per frontier node: enough that one pass of kBfsEdgesPerLane edges per lane
  // covers an average row (grid: 1 lane x 4 edges; fabric: 8 lanes x 4 edges)
  const uint32_t avg = V ? (E + V - 1) / V : 1;
  const uint32_t per_lane = (avg + 2 * kBfsEdgesPerLane - 1) / (2 * kBfsEdgesPerLane);  // fabric: G=4 measured best
  uint32_t gl = 1;
  while (gl < per_lane && gl < 64) gl <<= 1;
  ctx->group_lanes = gl;
  ctx->metric.assign(gr->metric, gr->metric + E);
  ctx->edge_up.assign(gr->edge_up, gr->edge_up + E);
  ctx->ovl = std::move(ovl);
  ctx->adj = std::move(adj);
  ctx->w = std::move(w);
  ctx->win = std::move(win);
  ctx->rev = std::move(rev);
  ctx->lid = std::move(lid);
  ctx->owner = std::move(owner);
  ctx->ovl_bits = std::move(ovl_bits);
  ctx->ledge = std::move(ledge);
  ctx->row2t = std::move(row2t);
  ctx->erec = std::move(erec);
  ctx->ellt = std::move(ellt);
  ctx->erec_pos = std::move(erec_pos);
  ctx->delta.clear();
  ctx->delta_index.clear();
  ctx->delta_valid = false;
  ctx->wcount.clear();
  ctx->n_bad_metric = 0;
  for (uint32_t e = 0; e < E; ++e) ctx->count_metric(e, +1);
  ctx->seen_e.assign(E, 0);
  ctx->dirty_e.assign(E, 0);
  ctx->dirty_v.assign(V, 0);
  ctx->patch_epoch = 0;
  ctx->has_graph = true;
  return OPENR_SPF_OK;
}

int openr_spf_patch_graph(openr_spf_ctx* ctx, const openr_spf_patch* p) {
  if (!ctx || !p) return fail(OPENR_SPF_EINVAL, "null argument");
  if (!ctx->has_graph) return fail(OPENR_SPF_EINVAL, "no graph set (openr_spf_set_graph)");
  if ((p->n_edges && (!p->edge_ids || !p->metric)) || (p->n_links && (!p->link_ids || !p->link_up)) ||
      (p->n_nodes && (!p->node_ids || !p->node_overloaded)))
    return fail(OPENR_SPF_EINVAL, "null patch array");
  const uint32_t V = ctx->V, E = ctx->E, L = ctx->L;
  for (uint32_t i = 0; i < p->n_edges; ++i)
    if (p->edge_ids[i] >= E) return fail(OPENR_SPF_EINVAL, "edge id %u out of range (E=%u)", p->edge_ids[i], E);
  for (uint32_t i = 0; i < p->n_links; ++i)
    if (p->link_ids[i] >= L || ctx->ledge[p->link_ids[i]].x == UINT32_MAX)
      return fail(OPENR_SPF_EINVAL, "link id %u is not a link of the graph", p->link_ids[i]);
  for (uint32_t i = 0; i < p->n_nodes; ++i)
    if (p->node_ids[i] >= V) return fail(OPENR_SPF_EINVAL, "node id %u out of range (V=%u)", p->node_ids[i], V);

  // per-patch marks: stamps of this patch (epoch wrap: clear the arrays once)
  if (++ctx->patch_epoch == 0) {
    std::fill(ctx->seen_e.begin(), ctx->seen_e.end(), 0u);
    std::fill(ctx->dirty_e.begin(), ctx->dirty_e.end(), 0u);
    std::fill(ctx->dirty_v.begin(), ctx->dirty_v.end(), 0u);
    ctx->patch_epoch = 1;
  }
  const uint32_t ep = ctx->patch_epoch;

  // 1) every directed edge whose (usable, weight, tail overload) may change, old state
  std::vector<uint32_t> cand;
  auto add = [&](uint32_t e) {
    if (ctx->seen_e[e] != ep) {
      ctx->seen_e[e] = ep;
      cand.push_back(e);
    }
  };
  for (uint32_t i = 0; i < p->n_edges; ++i) add(p->edge_ids[i]);
  for (uint32_t i = 0; i < p->n_links; ++i) {
    add(ctx->ledge[p->link_ids[i]].x);
    add(ctx->ledge[p->link_ids[i]].y);
  }
  for (uint32_t i = 0; i < p->n_nodes; ++i)
    for (uint32_t e = ctx->row_ptr[p->node_ids[i]]; e < ctx->row_ptr[p->node_ids[i] + 1]; ++e) add(e);
  auto state = [&](uint32_t e, uint32_t* wout) {
    *wout = ctx->w[e];
    return ((ctx->adj[e] & kEdgeDown) ? 0u : 1u) | (ctx->ovl[ctx->owner[e]] ? 2u : 0u);
  };
  std::vector<uint32_t> w0(cand.size()), f0(cand.size());
  for (size_t k = 0; k < cand.size(); ++k) {
    f0[k] = state(cand[k], &w0[k]);
    ctx->count_metric(cand[k], -1);  // re-counted with its new state below
  }

  // 2) apply to the host attributes; collect dirty device elements
  std::vector<uint32_t> de_list, dv_list;
  auto dirty_edge = [&](uint32_t e) {
    if (ctx->dirty_e[e] != ep) {
      ctx->dirty_e[e] = ep;
      de_list.push_back(e);
    }
  };
  auto dirty_node = [&](uint32_t u) {
    if (ctx->dirty_v[u] != ep) {
      ctx->dirty_v[u] = ep;
      dv_list.push_back(u);
    }
  };
  for (uint32_t i = 0; i < p->n_edges; ++i) {  // Link::setMetricFromNode (LinkState.cpp:195-204)
    const uint32_t e = p->edge_ids[i];
    ctx->metric[e] = p->metric[i];
    ctx->w[e] = (uint32_t)std::min<uint64_t>(p->metric[i], 0xFFFFFFFFull);
    ctx->win[ctx->rev[e]] = ctx->w[e];
    dirty_edge(e);
    dirty_edge(ctx->rev[e]);
  }
  for (uint32_t i = 0; i < p->n_links; ++i) {  // Link::isUp (LinkState.cpp:233-236), per link
    const uint2 ab = ctx->ledge[p->link_ids[i]];
    for (uint32_t e : {ab.x, ab.y}) {
      ctx->edge_up[e] = p->link_up[i] ? 1 : 0;
      ctx->adj[e] = ctx->col[e] | (p->link_up[i] ? 0u : kEdgeDown);
      dirty_edge(e);
      dirty_node(ctx->owner[e]);  // ellt
    }
  }
  for (uint32_t i = 0; i < p->n_nodes; ++i) {  // LinkState::updateNodeOverloaded / isNodeOverloaded
    const uint32_t x = p->node_ids[i];
    ctx->ovl[x] = p->node_overloaded[i] ? 1 : 0;
    dirty_node(x);
    for (uint32_t e = ctx->row_ptr[x]; e < ctx->row_ptr[x + 1]; ++e) dirty_edge(ctx->rev[e]);  // erec sink flag
  }
  for (uint32_t e : cand) ctx->count_metric(e, +1);
  // records in element order (as a full scan would emit them)
  std::sort(de_list.begin(), de_list.end());
  std::sort(dv_list.begin(), dv_list.end());

  // 3) recompute the dirty device elements exactly as set_graph derives them
  std::vector<PatchRec> recs;
  recs.reserve(6 * de_list.size() + 6 * dv_list.size());
  auto rec = [&](uint32_t arr, uint32_t idx, uint4 val) { recs.push_back(PatchRec{arr, idx, 0u, 0u, val}); };
  for (uint32_t e : de_list) {
    ctx->erec[e] = make_uint4(ctx->adj[e] | (ctx->ovl[ctx->col[e]] ? kNodeSink : 0u), ctx->win[e], ctx->lid[e],
                              ctx->rev[e]);
    rec(kPatchAdj, e, make_uint4(ctx->adj[e], 0, 0, 0));
    rec(kPatchW, e, make_uint4(ctx->w[e], 0, 0, 0));
    rec(kPatchW64, e, make_uint4((uint32_t)ctx->metric[e], (uint32_t)(ctx->metric[e] >> 32), 0, 0));
    rec(kPatchWin, e, make_uint4(ctx->win[e], 0, 0, 0));
    rec(kPatchErec, e, ctx->erec[e]);
    rec(kPatchErecS, ctx->erec_pos[e], ctx->erec[e]);
  }
  uint32_t last_word = UINT32_MAX;
  for (uint32_t u : dv_list) {
    const uint32_t rb = ctx->row_ptr[u], re = ctx->row_ptr[u + 1];
    uint32_t x4[4] = {kEdgeDown, kEdgeDown, kEdgeDown, kEdgeDown};
    if (!ctx->ovl[u])
      for (uint32_t j = 0; j < 4 && rb + j < re; ++j) x4[j] = ctx->adj[rb + j];
    else
      x4[0] |= kNodeSink;
    ctx->ellt[u] = make_uint4(x4[0], x4[1], x4[2], x4[3]);
    ctx->row2t[u] = ctx->ovl[u] ? make_uint2(rb | kNodeSink, rb) : make_uint2(rb, re);
    if (ctx->ovl[u]) ctx->ovl_bits[u >> 5] |= 1u << (u & 31u);
    else ctx->ovl_bits[u >> 5] &= ~(1u << (u & 31u));
    rec(kPatchEllt, u, ctx->ellt[u]);
    rec(kPatchEllv, u, ellv_of(ctx->ellt[u], V));
    rec(kPatchElld, u, make_uint4(elld_of(ellv_of(ctx->ellt[u], V), u, V), 0, 0, 0));
    rec(kPatchRow2t, u, make_uint4(ctx->row2t[u].x, ctx->row2t[u].y, 0, 0));
    rec(kPatchOvl, u, make_uint4(ctx->ovl[u], 0, 0, 0));
  }
  for (uint32_t u : dv_list) {  // sorted: each touched overload word once, after its bits
    if ((u >> 5) == last_word) continue;
    last_word = u >> 5;
    rec(kPatchOvlBits, last_word, make_uint4(ctx->ovl_bits[last_word], 0, 0, 0));
  }

  // 4) graph-wide metric facts (kernel choice / ENOTSUP) over the usable edges, from the
  //    metric multiset kept current above
  const bool metric_ok = ctx->n_bad_metric == 0;
  uint32_t w_min = 1, w_max = 1;  // no usable edge
  if (!ctx->wcount.empty()) {
    w_min = ctx->wcount.begin()->first;
    w_max = ctx->wcount.rbegin()->first;
  }

  // 5) the delta edges of this patch (openr_spf_refresh). Patches with no refresh in
  //    between accumulate: an edge keeps its state from before the first of them, so rows
  //    of that older graph are still filtered correctly; edges back at that state drop out.
  const bool merge = ctx->delta_valid && !ctx->refreshed;
  if (!merge) {
    ctx->delta.clear();
    ctx->delta_index.clear();
  }
  for (size_t k = 0; k < cand.size(); ++k) {
    uint32_t w1 = 0;
    const uint32_t f1 = state(cand[k], &w1);
    if (f1 == f0[k] && w1 == w0[k]) continue;
    const uint32_t e = cand[k];
    const uint32_t new_flags = ((f1 & 1u) ? kDeltaUp1 : 0u) | ((f1 & 2u) ? kDeltaOvl1 : 0u);
    auto it = ctx->delta_index.find(e);
    if (it != ctx->delta_index.end()) {  // changed by an earlier, unrefreshed patch too
      DeltaEdge& de = ctx->delta[it->second];
      de.w1 = w1;
      de.flags = (de.flags & (kDeltaUp0 | kDeltaOvl0)) | new_flags;
      continue;
    }
    DeltaEdge de{};
    de.u = ctx->owner[e];
    de.v = ctx->col[e];
    de.w0 = w0[k];
    de.w1 = w1;
    de.flags = ((f0[k] & 1u) ? kDeltaUp0 : 0u) | ((f0[k] & 2u) ? kDeltaOvl0 : 0u) | new_flags;
    de.pad0 = e;
    ctx->delta_index.emplace(e, (uint32_t)ctx->delta.size());
    ctx->delta.push_back(de);
  }
  if (merge) {  // drop edges whose accumulated change cancelled out
    size_t o = 0;
    for (size_t k = 0; k < ctx->delta.size(); ++k) {
      const DeltaEdge& de = ctx->delta[k];
      const bool same = de.w0 == de.w1 && ((de.flags & kDeltaUp0) != 0) == ((de.flags & kDeltaUp1) != 0) &&
                        ((de.flags & kDeltaOvl0) != 0) == ((de.flags & kDeltaOvl1) != 0);
      if (!same) ctx->delta[o++] = de;
    }
    ctx->delta.resize(o);
    ctx->delta_index.clear();
    for (size_t k = 0; k < o; ++k) ctx->delta_index.emplace(ctx->delta[k].pad0, (uint32_t)k);
  }

  // 6) upload: one record list + one scatter kernel per replica (measured: an event that
  //    later device-form calls wait on instead of this synchronize was no faster)
  for (Device& d : ctx->devs) {
    HIP_TRY(hipSetDevice(d.ordinal));
    if (recs.empty()) continue;
    HIP_TRY(d.precs.reserve(recs.size()));
    HIP_TRY(hipMemcpyAsync(d.precs.p, recs.data(), recs.size() * sizeof(PatchRec), hipMemcpyHostToDevice, d.stream));
    HIP_TRY(launch_patch_apply(d.g, d.precs.p, (uint32_t)recs.size(), d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));  // recs is host memory of this call
  }
  ctx->w_min = w_min;
  ctx->w_max = w_max;
  ctx->delta_all = (merge && ctx->delta_all) || !ctx->metric_ok || !metric_ok;
  ctx->metric_ok = metric_ok;
  ctx->delta_valid = true;
  ctx->refreshed = false;
  return OPENR_SPF_OK;
}

int openr_spf_refresh_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_sources, uint32_t n,
                             uint32_t flags, uint64_t* d_dist, uint8_t* d_nh, uint32_t nh_bytes, uint64_t* d_tight,
                             void* stream, uint32_t* out_resolved) {
  int rc = check_solve_args(ctx, d_sources, n, d_dist, d_nh, nh_bytes);
  if (rc) return rc;
  if (device_index < 0 || device_index >= (int)ctx->devs.size())
    return fail(OPENR_SPF_EINVAL, "device_index %d out of range", device_index);
  if (!ctx->delta_valid)
    return fail(OPENR_SPF_EINVAL, "no patch since the last openr_spf_set_graph: rows must be re-solved");
  Plan plan;
  rc = make_plan(ctx, flags, false, &plan);
  if (rc) return rc;
  Device& d = ctx->devs[device_index];
  HIP_TRY(hipSetDevice(d.ordinal));
  hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : d.stream;
  const uint32_t nd = (uint32_t)ctx->delta.size();
  uint32_t count = 0;
  if (ctx->delta_all && n) {
    HIP_TRY(d.alist.reserve(n));
    HIP_TRY(launch_iota(d.alist.p, n, d.num_cus, s));
    count = n;
  } else if (nd && n) {
    HIP_TRY(d.delta.reserve(nd));
    HIP_TRY(d.alist.reserve(n));
    HIP_TRY(d.asrc.reserve(n));
    HIP_TRY(d.acount.reserve(2));
    HIP_TRY(hipMemcpyAsync(d.delta.p, ctx->delta.data(), nd * sizeof(DeltaEdge), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d.acount.p, 0, sizeof(uint32_t), s));
    HIP_TRY(launch_refresh_filter(d.delta.p, nd, d_sources, n, ctx->V, d_dist,
                                  (flags & OPENR_SPF_USE_LINK_METRIC) == 0, d.alist.p, d.asrc.p, d.acount.p,
                                  d.num_cus, s));
    // exact second stage (spf_update.hip) when next-hop rows are kept and no tight rows are:
    // of the listed rows, only those the change really moves are re-solved
    const char* ex = std::getenv("OPENR_SPF_REFRESH_EXACT");  // 0: first stage only (A/B)
    if (d_nh && !d_tight && nh_bytes <= 32u && !(ex && std::atoi(ex) == 0)) {
      HIP_TRY(d.alist2.reserve(n));
      HIP_TRY(d.asrc2.reserve(n));
      HIP_TRY(hipMemsetAsync(d.acount.p + 1, 0, sizeof(uint32_t), s));
      HIP_TRY(launch_refresh_exact(d.g, d.delta.p, nd, ctx->V, d_dist, d_nh, nh_bytes,
                                   (flags & OPENR_SPF_USE_LINK_METRIC) == 0, d.alist.p, d.asrc.p, d.acount.p, n,
                                   d.alist2.p, d.asrc2.p, d.acount.p + 1, d.num_cus, s));
      HIP_TRY(hipMemcpyAsync(&count, d.acount.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      std::swap(d.alist, d.alist2);  // the exact list is the one re-solved
      std::swap(d.asrc, d.asrc2);
    } else {
      HIP_TRY(hipMemcpyAsync(&count, d.acount.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));  // the affected-row count sizes the re-solve
    }
  }
  if (count) {
    if (d_tight) HIP_TRY(launch_zero_rows(d_tight, (ctx->E + 63u) / 64u, d.alist.p, count, d.num_cus, s));
    SolveArgs a{};
    a.sources = ctx->delta_all ? d_sources : d.asrc.p;
    a.n = count;
    a.out_row = d.alist.p;
    a.dist = d_dist;
    a.nh = d_nh;
    a.nh_bytes = nh_bytes;
    a.tight = d_tight;
    a.nh_bits = ctx->nh_bits;
    HIP_TRY(d.ovf.reserve((size_t)count * ctx->nsl_max()));
    a.ovf_list = d.ovf.p;
    HIP_TRY(reserve_counters(d));
    a.work = d.work.p;
    HIP_TRY(launch(ctx, d, plan, a, s));
    ctx->stats.spf_runs += count;
    ctx->stats.batches += 1;
  }
  if (out_resolved) *out_resolved = count;
  ctx->refreshed = true;  // the next patch starts a new delta
  return OPENR_SPF_OK;
}

int openr_spf_refresh(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n, uint32_t flags, uint64_t* dist,
                      uint8_t* nh, uint32_t nh_bytes, uint64_t* tight, uint32_t* out_resolved) {
  int rc = check_solve_args(ctx, sources, n, dist, nh, nh_bytes);
  if (rc) return rc;
  for (uint32_t i = 0; i < n; ++i)
    if (sources[i] >= ctx->V) return fail(OPENR_SPF_EINVAL, "source %u out of range (V=%u)", sources[i], ctx->V);
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t V = ctx->V, tw = (ctx->E + 63u) / 64u;
  const uint32_t ndev = (uint32_t)ctx->devs.size();
  const uint32_t per = (n + ndev - 1) / std::max<uint32_t>(ndev, 1);
  uint32_t total = 0;
  for (uint32_t di = 0; di < ndev; ++di) {
    Device& d = ctx->devs[di];
    const uint32_t b = std::min(n, di * per), e = std::min(n, b + per), m = e - b;
    if (!m) continue;
    HIP_TRY(hipSetDevice(d.ordinal));
    HIP_TRY(d.src.reserve(m));
    HIP_TRY(d.dist.reserve((size_t)m * V));
    if (nh) HIP_TRY(d.nh.reserve((size_t)m * V * nh_bytes));
    if (tight) HIP_TRY(d.tight.reserve((size_t)m * tw));
    HIP_TRY(hipMemcpyAsync(d.src.p, sources + b, m * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d.dist.p, dist + (size_t)b * V, (size_t)m * V * 8u, hipMemcpyHostToDevice, d.stream));
    if (nh)
      HIP_TRY(hipMemcpyAsync(d.nh.p, nh + (size_t)b * V * nh_bytes, (size_t)m * V * nh_bytes, hipMemcpyHostToDevice,
                             d.stream));
    if (tight)
      HIP_TRY(hipMemcpyAsync(d.tight.p, tight + (size_t)b * tw, (size_t)m * tw * 8u, hipMemcpyHostToDevice,
                             d.stream));
    uint32_t c = 0;
    rc = openr_spf_refresh_device(ctx, (int)di, d.src.p, m, flags, d.dist.p, nh ? d.nh.p : nullptr, nh_bytes,
                                  tight ? d.tight.p : nullptr, nullptr, &c);
    if (rc) return rc;
    total += c;
    HIP_TRY(hipMemcpyAsync(dist + (size_t)b * V, d.dist.p, (size_t)m * V * 8u, hipMemcpyDeviceToHost, d.stream));
    if (nh)
      HIP_TRY(hipMemcpyAsync(nh + (size_t)b * V * nh_bytes, d.nh.p, (size_t)m * V * nh_bytes, hipMemcpyDeviceToHost,
                             d.stream));
    if (tight)
      HIP_TRY(hipMemcpyAsync(tight + (size_t)b * tw, d.tight.p, (size_t)m * tw * 8u, hipMemcpyDeviceToHost,
                             d.stream));
  }
  for (Device& d : ctx->devs) {
    HIP_TRY(hipSetDevice(d.ordinal));
    HIP_TRY(hipStreamSynchronize(d.stream));
  }
  ctx->stats.last_batch_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (out_resolved) *out_resolved = total;
  return OPENR_SPF_OK;
}

int openr_spf_nh_bytes(const openr_spf_ctx* ctx, uint32_t* out) {
  if (!ctx || !out) return fail(OPENR_SPF_EINVAL, "null argument");
  if (!ctx->has_graph) return fail(OPENR_SPF_EINVAL, "no graph set");
  *out = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  return OPENR_SPF_OK;
}

int openr_spf_neighbor_map(const openr_spf_ctx* ctx, uint32_t src, uint32_t* out_nbrs, uint32_t capacity,
                           uint32_t* out_count) {
  if (!ctx || !out_count) return fail(OPENR_SPF_EINVAL, "null argument");
  if (!ctx->has_graph) return fail(OPENR_SPF_EINVAL, "no graph set");
  if (src >= ctx->V) return fail(OPENR_SPF_EINVAL, "source out of range");
  uint32_t n = 0;
  for (uint32_t e = ctx->row_ptr[src]; e < ctx->row_ptr[src + 1]; ++e) {
    const uint32_t v = ctx->col[e];
    bool dup = false;
    for (uint32_t f = ctx->row_ptr[src]; f < e && !dup; ++f) dup = ctx->col[f] == v;
    if (dup) continue;
    if (out_nbrs && n < capacity) out_nbrs[n] = v;
    ++n;
  }
  *out_count = n;
  if (out_nbrs && n > capacity) return fail(OPENR_SPF_EINVAL, "capacity %u < %u neighbours", capacity, n);
  return OPENR_SPF_OK;
}

int openr_spf_solve(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n, uint32_t flags, uint64_t* dist,
                    uint8_t* nh, uint32_t nh_bytes, uint64_t* tight) {
  return solve_host(ctx, sources, n, flags, nullptr, nullptr, dist, nh, nh_bytes, tight);
}

int openr_spf_solve_order(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n, uint32_t flags,
                          const uint32_t* ignore_ptr, const uint32_t* ignore_links, uint64_t* dist, uint8_t* nh,
                          uint32_t nh_bytes, uint64_t* tight, uint32_t* order) {
  if (n && !order) return fail(OPENR_SPF_EINVAL, "null order");
  return solve_host(ctx, sources, n, flags, ignore_ptr, ignore_links, dist, nh, nh_bytes, tight, order);
}

int openr_spf_solve_ignore(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n, uint32_t flags,
                           const uint32_t* ignore_ptr, const uint32_t* ignore_links, uint64_t* dist,
                           uint8_t* nh, uint32_t nh_bytes, uint64_t* tight) {
  if (!ignore_ptr) return fail(OPENR_SPF_EINVAL, "null ignore_ptr");
  return solve_host(ctx, sources, n, flags, ignore_ptr, ignore_links, dist, nh, nh_bytes, tight);
}

int openr_spf_solve_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_sources, uint32_t n,
                           uint32_t flags, const uint32_t* d_ignore_ptr, const uint32_t* d_ignore_links,
                           uint64_t* d_dist, uint8_t* d_nh, uint32_t nh_bytes, uint64_t* d_tight, void* stream) {
  clear_launch_trace();
  int rc = check_solve_args(ctx, d_sources, n, d_dist, d_nh, nh_bytes);
  if (rc) return rc;
  if (device_index < 0 || device_index >= (int)ctx->devs.size())
    return fail(OPENR_SPF_EINVAL, "device_index %d out of range", device_index);
  Plan plan;
  rc = make_plan(ctx, flags, d_ignore_ptr != nullptr, &plan);
  if (rc) return rc;
  Device& d = ctx->devs[device_index];
  HIP_TRY(hipSetDevice(d.ordinal));
  SolveArgs a{};
  a.sources = d_sources;
  a.n = n;
  a.ign_ptr = d_ignore_ptr;
  a.ign_links = d_ignore_links;
  a.dist = d_dist;
  a.nh = d_nh;
  a.nh_bytes = nh_bytes;
  a.tight = d_tight;
  a.nh_bits = ctx->nh_bits;
  if (flags & (OPENR_SPF_EMIT_LEVELS8 | OPENR_SPF_EMIT_LEVELS16)) {
    // level rows (the compact strong-scaling exchange): level-family uniform-cost solves
    if ((flags & OPENR_SPF_EMIT_LEVELS8) && (flags & OPENR_SPF_EMIT_LEVELS16))
      return fail(OPENR_SPF_EINVAL, "EMIT_LEVELS8 and EMIT_LEVELS16 together");
    if (plan.exact || !plan.bfs || plan.family != kFamLvl || d_tight || d_ignore_ptr)
      return fail(OPENR_SPF_ENOTSUP, "level rows need a uniform-cost graph on the level BFS family, no ignore sets "
                                     "and no tight output");
    if (!d.status.p) {
      HIP_TRY(d.status.reserve(1));
      HIP_TRY(hipMemset(d.status.p, 0, sizeof(uint32_t)));
    }
    a.lvl_rows = reinterpret_cast<uint8_t*>(d_dist);
    a.lvl_bytes = (flags & OPENR_SPF_EMIT_LEVELS8) ? 1u : 2u;
    a.status = d.status.p;
    a.dist = nullptr;
  }
  HIP_TRY(d.ovf.reserve((size_t)n * ctx->nsl_max()));
  a.ovf_list = d.ovf.p;
  HIP_TRY(reserve_counters(d));
  a.work = d.work.p;
  hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : d.stream;
  HIP_TRY(launch(ctx, d, plan, a, s, true));
  ctx->stats.spf_runs += n;
  ctx->stats.batches += 1;
  return OPENR_SPF_OK;
}

int openr_spf_last_derived(openr_spf_ctx* ctx, int device_index, uint32_t* out_derived) {
  if (!ctx || !out_derived) return fail(OPENR_SPF_EINVAL, "null argument");
  if (device_index < 0 || device_index >= (int)ctx->devs.size())
    return fail(OPENR_SPF_EINVAL, "device_index %d out of range", device_index);
  Device& d = ctx->devs[device_index];
  *out_derived = 0;
  if (!d.dv_last) return OPENR_SPF_OK;
  HIP_TRY(hipSetDevice(d.ordinal));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out_derived, d.dv_part.p + 2u * kMaxClasses, sizeof(uint32_t), hipMemcpyDeviceToHost));
  return OPENR_SPF_OK;
}

int openr_spf_take_status(openr_spf_ctx* ctx, int device_index, uint32_t* out_status) {
  if (!ctx || !out_status) return fail(OPENR_SPF_EINVAL, "null argument");
  if (device_index < 0 || device_index >= (int)ctx->devs.size())
    return fail(OPENR_SPF_EINVAL, "device_index %d out of range", device_index);
  Device& d = ctx->devs[device_index];
  *out_status = 0;
  if (!d.status.p) return OPENR_SPF_OK;
  HIP_TRY(hipSetDevice(d.ordinal));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out_status, d.status.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(d.status.p, 0, sizeof(uint32_t)));
  return OPENR_SPF_OK;
}

int openr_spf_whatif(openr_spf_ctx* ctx, const uint32_t* links, uint32_t n_links, const uint32_t* sources,
                     uint32_t n_sources, uint32_t flags, uint32_t* changed, uint64_t* out_solved) {
  clear_launch_trace();
  WhatifUnits hu;
  hu.links = links;
  hu.n = n_links;
  return whatif_host(ctx, hu, sources, n_sources, flags, changed, out_solved);
}

int openr_spf_whatif_sets(openr_spf_ctx* ctx, const uint32_t* set_ptr, const uint32_t* set_links, uint32_t n_sets,
                          const uint32_t* sources, uint32_t n_sources, uint32_t flags, uint32_t* changed,
                          uint64_t* out_solved) {
  clear_launch_trace();
  if (n_sets && !set_ptr) return fail(OPENR_SPF_EINVAL, "null set_ptr");
  return whatif_host(ctx, host_sets(set_ptr, set_links, n_sets), sources, n_sources, flags, changed, out_solved);
}

int openr_spf_whatif_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_links, uint32_t n_links,
                            const uint32_t* d_sources, uint32_t n_sources, uint32_t flags, uint32_t* d_changed,
                            void* stream, uint64_t* out_solved) {
  clear_launch_trace();
  WhatifUnits un;
  un.links = d_links;
  un.n = n_links;
  return whatif_device_form(ctx, device_index, un, d_sources, n_sources, flags, d_changed, stream, out_solved);
}

int openr_spf_whatif_sets_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_set_ptr,
                                 const uint32_t* d_set_links, uint32_t n_sets, uint32_t n_set_links,
                                 const uint32_t* d_sources, uint32_t n_sources, uint32_t flags, uint32_t* d_changed,
                                 void* stream, uint64_t* out_solved) {
  clear_launch_trace();
  if (n_sets && (!d_set_ptr || (n_set_links && !d_set_links))) return fail(OPENR_SPF_EINVAL, "null set_ptr or set_links");
  return whatif_device_form(ctx, device_index, device_sets(d_set_ptr, d_set_links, n_sets, n_set_links), d_sources,
                            n_sources, flags, d_changed, stream, out_solved);
}

int openr_spf_whatif_delta_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_links, uint32_t n_links,
                                  const uint32_t* d_sources, uint32_t n_sources, uint32_t flags, uint32_t* d_changed,
                                  uint64_t* d_ptr, uint32_t* d_node, uint64_t* d_dist, uint8_t* d_nh, uint64_t cap,
                                  uint32_t nh_bytes, void* stream, uint64_t* out_total, uint64_t* out_solved) {
  clear_launch_trace();
  WhatifUnits un;
  un.links = d_links;
  un.n = n_links;
  return whatif_delta_device_form(ctx, device_index, un, d_sources, n_sources, flags, d_changed, d_ptr, d_node, d_dist,
                                  d_nh, cap, nh_bytes, stream, out_total, out_solved);
}

int openr_spf_whatif_sets_delta_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_set_ptr,
                                       const uint32_t* d_set_links, uint32_t n_sets, uint32_t n_set_links,
                                       const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                       uint32_t* d_changed, uint64_t* d_ptr, uint32_t* d_node, uint64_t* d_dist,
                                       uint8_t* d_nh, uint64_t cap, uint32_t nh_bytes, void* stream,
                                       uint64_t* out_total, uint64_t* out_solved) {
  clear_launch_trace();
  if (n_sets && (!d_set_ptr || (n_set_links && !d_set_links))) return fail(OPENR_SPF_EINVAL, "null set_ptr or set_links");
  return whatif_delta_device_form(ctx, device_index, device_sets(d_set_ptr, d_set_links, n_sets, n_set_links),
                                  d_sources, n_sources, flags, d_changed, d_ptr, d_node, d_dist, d_nh, cap, nh_bytes,
                                  stream, out_total, out_solved);
}

int openr_spf_whatif_delta(openr_spf_ctx* ctx, const uint32_t* links, uint32_t n_links, const uint32_t* sources,
                           uint32_t n_sources, uint32_t flags, uint32_t* changed, openr_spf_whatif_delta_t* delta,
                           uint64_t* out_solved) {
  clear_launch_trace();
  WhatifUnits hu;
  hu.links = links;
  hu.n = n_links;
  return whatif_delta_host(ctx, hu, sources, n_sources, flags, changed, delta, out_solved);
}

int openr_spf_whatif_sets_delta(openr_spf_ctx* ctx, const uint32_t* set_ptr, const uint32_t* set_links,
                                uint32_t n_sets, const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                                uint32_t* changed, openr_spf_whatif_delta_t* delta, uint64_t* out_solved) {
  clear_launch_trace();
  if (n_sets && !set_ptr) return fail(OPENR_SPF_EINVAL, "null set_ptr");
  return whatif_delta_host(ctx, host_sets(set_ptr, set_links, n_sets), sources, n_sources, flags, changed, delta,
                           out_solved);
}

// ---- event sweeps: drain, metric, restore, maintenance (the forms are above, before extern "C") --
int openr_spf_whatif_drain(openr_spf_ctx* ctx, const openr_spf_drain_events_t* events, const uint32_t* sources,
                           uint32_t n_sources, uint32_t flags, uint32_t* changed, openr_spf_whatif_delta_t* delta,
                           uint64_t* out_solved) {
  return event_host(ctx, kElfaDrain, events, sources, n_sources, flags, changed, delta, out_solved);
}

int openr_spf_whatif_drain_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                  const uint32_t* d_nodes, const uint32_t* d_link_ptr, const uint32_t* d_links,
                                  uint32_t n_events, uint32_t n_nodes, uint32_t n_links, const uint32_t* d_sources,
                                  uint32_t n_sources, uint32_t flags, uint32_t* d_changed, uint64_t* d_ptr,
                                  uint32_t* d_node, uint64_t* d_dist, uint8_t* d_nh, uint64_t cap, uint32_t nh_bytes,
                                  void* stream, uint64_t* out_total, uint64_t* out_solved) {
  return event_device(ctx, device_index, drain_units(d_node_ptr, d_nodes, d_link_ptr, d_links, n_events, n_nodes, n_links),
                      kElfaDrain, d_sources, n_sources, flags, d_changed, d_ptr, d_node, d_dist, d_nh, cap, nh_bytes,
                      stream, out_total, out_solved);
}

int openr_spf_whatif_drain_routes(openr_spf_ctx* ctx, const openr_spf_drain_events_t* events, const uint32_t* sources,
                                  uint32_t n_sources, uint32_t flags, const openr_spf_groups_t* groups,
                                  uint32_t* changed_routes, openr_spf_whatif_routes_t* delta, uint64_t* out_solved) {
  return event_routes_host(ctx, kElfaDrain, events, sources, n_sources, flags, groups, changed_routes, delta,
                           out_solved);
}

int openr_spf_whatif_drain_routes_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                         const uint32_t* d_nodes, const uint32_t* d_link_ptr, const uint32_t* d_links,
                                         uint32_t n_events, uint32_t n_nodes, uint32_t n_links,
                                         const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                         const uint32_t* d_group_ptr, const uint32_t* d_group_nodes,
                                         uint32_t n_groups, uint32_t n_group_nodes, uint32_t* d_changed_routes,
                                         uint64_t* d_ptr, uint32_t* d_group, uint64_t* d_metric, uint8_t* d_nh,
                                         uint32_t* d_n_best, uint64_t cap, uint32_t nh_bytes, void* stream,
                                         uint64_t* out_total, uint64_t* out_solved) {
  return whatif_routes_device_form(
      ctx, device_index, drain_units(d_node_ptr, d_nodes, d_link_ptr, d_links, n_events, n_nodes, n_links), kElfaDrain,
      d_sources, n_sources, flags, d_group_ptr, d_group_nodes, n_groups, n_group_nodes, d_changed_routes, d_ptr, d_group,
      d_metric, d_nh, d_n_best, cap, nh_bytes, stream, out_total, out_solved);
}

int openr_spf_whatif_metric(openr_spf_ctx* ctx, const openr_spf_metric_events_t* events, const uint32_t* sources,
                            uint32_t n_sources, uint32_t flags, uint32_t* changed, openr_spf_whatif_delta_t* delta,
                            uint64_t* out_solved) {
  return event_host(ctx, kElfaMetric, events, sources, n_sources, flags, changed, delta, out_solved);
}

int openr_spf_whatif_metric_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_edge_ptr,
                                   const uint32_t* d_edges, const uint32_t* d_metrics, uint32_t n_events,
                                   uint32_t n_edges, const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                   uint32_t* d_changed, uint64_t* d_ptr, uint32_t* d_node, uint64_t* d_dist,
                                   uint8_t* d_nh, uint64_t cap, uint32_t nh_bytes, void* stream, uint64_t* out_total,
                                   uint64_t* out_solved) {
  return event_device(ctx, device_index, metric_units(d_edge_ptr, d_edges, d_metrics, n_events, n_edges), kElfaMetric,
                      d_sources, n_sources, flags, d_changed, d_ptr, d_node, d_dist, d_nh, cap, nh_bytes, stream,
                      out_total, out_solved);
}

int openr_spf_whatif_metric_routes(openr_spf_ctx* ctx, const openr_spf_metric_events_t* events,
                                   const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                                   const openr_spf_groups_t* groups, uint32_t* changed_routes,
                                   openr_spf_whatif_routes_t* delta, uint64_t* out_solved) {
  return event_routes_host(ctx, kElfaMetric, events, sources, n_sources, flags, groups, changed_routes, delta,
                           out_solved);
}

int openr_spf_whatif_metric_routes_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_edge_ptr,
                                          const uint32_t* d_edges, const uint32_t* d_metrics, uint32_t n_events,
                                          uint32_t n_edges, const uint32_t* d_sources, uint32_t n_sources,
                                          uint32_t flags, const uint32_t* d_group_ptr, const uint32_t* d_group_nodes,
                                          uint32_t n_groups, uint32_t n_group_nodes, uint32_t* d_changed_routes,
                                          uint64_t* d_ptr, uint32_t* d_group, uint64_t* d_metric, uint8_t* d_nh,
                                          uint32_t* d_n_best, uint64_t cap, uint32_t nh_bytes, void* stream,
                                          uint64_t* out_total, uint64_t* out_solved) {
  return whatif_routes_device_form(ctx, device_index, metric_units(d_edge_ptr, d_edges, d_metrics, n_events, n_edges),
                                   kElfaMetric, d_sources, n_sources, flags, d_group_ptr, d_group_nodes, n_groups,
                                   n_group_nodes, d_changed_routes, d_ptr, d_group, d_metric, d_nh, d_n_best, cap,
                                   nh_bytes, stream, out_total, out_solved);
}

int openr_spf_whatif_restore(openr_spf_ctx* ctx, const openr_spf_restore_events_t* events, const uint32_t* sources,
                             uint32_t n_sources, uint32_t flags, uint32_t* changed, openr_spf_whatif_delta_t* delta,
                             uint64_t* out_solved) {
  return event_host(ctx, kElfaRestore, events, sources, n_sources, flags, changed, delta, out_solved);
}

int openr_spf_whatif_restore_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                    const uint32_t* d_nodes, const uint32_t* d_link_ptr, const uint32_t* d_links,
                                    const uint32_t* d_edge_ptr, const uint32_t* d_edges, const uint32_t* d_metrics,
                                    uint32_t n_events, uint32_t n_nodes, uint32_t n_links, uint32_t n_edges,
                                    const uint32_t* d_sources, uint32_t n_sources, uint32_t flags, uint32_t* d_changed,
                                    uint64_t* d_ptr, uint32_t* d_node, uint64_t* d_dist, uint8_t* d_nh, uint64_t cap,
                                    uint32_t nh_bytes, void* stream, uint64_t* out_total, uint64_t* out_solved) {
  return event_device(ctx, device_index,
                      restore_units(d_node_ptr, d_nodes, d_link_ptr, d_links, d_edge_ptr, d_edges, d_metrics, n_events,
                                    n_nodes, n_links, n_edges),
                      kElfaRestore, d_sources, n_sources, flags, d_changed, d_ptr, d_node, d_dist, d_nh, cap, nh_bytes,
                      stream, out_total, out_solved);
}

int openr_spf_whatif_restore_routes(openr_spf_ctx* ctx, const openr_spf_restore_events_t* events,
                                    const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                                    const openr_spf_groups_t* groups, uint32_t* changed_routes,
                                    openr_spf_whatif_routes_t* delta, uint64_t* out_solved) {
  return event_routes_host(ctx, kElfaRestore, events, sources, n_sources, flags, groups, changed_routes, delta,
                           out_solved);
}

int openr_spf_whatif_restore_routes_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                           const uint32_t* d_nodes, const uint32_t* d_link_ptr,
                                           const uint32_t* d_links, const uint32_t* d_edge_ptr,
                                           const uint32_t* d_edges, const uint32_t* d_metrics, uint32_t n_events,
                                           uint32_t n_nodes, uint32_t n_links, uint32_t n_edges,
                                           const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                           const uint32_t* d_group_ptr, const uint32_t* d_group_nodes,
                                           uint32_t n_groups, uint32_t n_group_nodes, uint32_t* d_changed_routes,
                                           uint64_t* d_ptr, uint32_t* d_group, uint64_t* d_metric, uint8_t* d_nh,
                                           uint32_t* d_n_best, uint64_t cap, uint32_t nh_bytes, void* stream,
                                           uint64_t* out_total, uint64_t* out_solved) {
  return whatif_routes_device_form(ctx, device_index,
                                   restore_units(d_node_ptr, d_nodes, d_link_ptr, d_links, d_edge_ptr, d_edges,
                                                 d_metrics, n_events, n_nodes, n_links, n_edges),
                                   kElfaRestore, d_sources, n_sources, flags, d_group_ptr, d_group_nodes, n_groups,
                                   n_group_nodes, d_changed_routes, d_ptr, d_group, d_metric, d_nh, d_n_best, cap,
                                   nh_bytes, stream, out_total, out_solved);
}

int openr_spf_whatif_maint(openr_spf_ctx* ctx, const openr_spf_maint_events_t* events, const uint32_t* sources,
                           uint32_t n_sources, uint32_t flags, uint32_t* changed, openr_spf_whatif_delta_t* delta,
                           uint64_t* out_solved) {
  return event_host(ctx, kElfaMaint, events, sources, n_sources, flags, changed, delta, out_solved);
}

int openr_spf_whatif_maint_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                  const uint32_t* d_nodes, const uint32_t* d_link_ptr, const uint32_t* d_links,
                                  const uint32_t* d_edge_ptr, const uint32_t* d_edges, const uint32_t* d_metrics,
                                  uint32_t n_events, uint32_t n_nodes, uint32_t n_links, uint32_t n_edges,
                                  const uint32_t* d_sources, uint32_t n_sources, uint32_t flags, uint32_t* d_changed,
                                  uint64_t* d_ptr, uint32_t* d_node, uint64_t* d_dist, uint8_t* d_nh, uint64_t cap,
                                  uint32_t nh_bytes, void* stream, uint64_t* out_total, uint64_t* out_solved) {
  return event_device(ctx, device_index,
                      maint_units(d_node_ptr, d_nodes, d_link_ptr, d_links, d_edge_ptr, d_edges, d_metrics, n_events,
                                  n_nodes, n_links, n_edges),
                      kElfaMaint, d_sources, n_sources, flags, d_changed, d_ptr, d_node, d_dist, d_nh, cap, nh_bytes,
                      stream, out_total, out_solved);
}

int openr_spf_whatif_maint_routes(openr_spf_ctx* ctx, const openr_spf_maint_events_t* events,
                                  const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                                  const openr_spf_groups_t* groups, uint32_t* changed_routes,
                                  openr_spf_whatif_routes_t* delta, uint64_t* out_solved) {
  return event_routes_host(ctx, kElfaMaint, events, sources, n_sources, flags, groups, changed_routes, delta,
                           out_solved);
}

int openr_spf_whatif_maint_routes_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                         const uint32_t* d_nodes, const uint32_t* d_link_ptr,
                                         const uint32_t* d_links, const uint32_t* d_edge_ptr,
                                         const uint32_t* d_edges, const uint32_t* d_metrics, uint32_t n_events,
                                         uint32_t n_nodes, uint32_t n_links, uint32_t n_edges,
                                         const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                         const uint32_t* d_group_ptr, const uint32_t* d_group_nodes,
                                         uint32_t n_groups, uint32_t n_group_nodes, uint32_t* d_changed_routes,
                                         uint64_t* d_ptr, uint32_t* d_group, uint64_t* d_metric, uint8_t* d_nh,
                                         uint32_t* d_n_best, uint64_t cap, uint32_t nh_bytes, void* stream,
                                         uint64_t* out_total, uint64_t* out_solved) {
  return whatif_routes_device_form(ctx, device_index,
                                   maint_units(d_node_ptr, d_nodes, d_link_ptr, d_links, d_edge_ptr, d_edges, d_metrics,
                                               n_events, n_nodes, n_links, n_edges),
                                   kElfaMaint, d_sources, n_sources, flags, d_group_ptr, d_group_nodes, n_groups,
                                   n_group_nodes, d_changed_routes, d_ptr, d_group, d_metric, d_nh, d_n_best, cap,
                                   nh_bytes, stream, out_total, out_solved);
}

int openr_spf_routes(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n, uint32_t flags,
                     const openr_spf_groups_t* groups, uint64_t* metric, uint8_t* nh, uint32_t nh_bytes,
                     uint32_t* n_best) {
  return routes_host(ctx, sources, n, flags, groups, metric, nh, nh_bytes, n_best);
}

int openr_spf_routes_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_sources, uint32_t n,
                            uint32_t flags, const uint32_t* d_group_ptr, const uint32_t* d_group_nodes,
                            uint32_t n_groups, uint32_t n_group_nodes, uint64_t* d_metric, uint8_t* d_nh,
                            uint32_t nh_bytes, uint32_t* d_n_best, void* stream) {
  clear_launch_trace();
  if (int e = check_ctx(ctx)) return e;
  if (int e = check_device_index(ctx, device_index)) return e;
  if ((n && !d_sources) || (n_groups && !d_group_ptr) || (n_group_nodes && !d_group_nodes) ||
      (n && n_groups && !d_metric))
    return fail(OPENR_SPF_EINVAL, "null sources, groups or metric");
  const uint32_t need = std::max<uint32_t>(1u, (ctx->nh_bits + 7u) / 8u);
  if (d_nh && nh_bytes < need) return fail(OPENR_SPF_EINVAL, "nh_bytes %u < required %u", nh_bytes, need);
  int rc = check_routes_metric(ctx, flags);
  if (rc) return rc;
  Device& d = ctx->devs[device_index];
  HIP_TRY(hipSetDevice(d.ordinal));
  DevGroups gr;
  gr.ptr = d_group_ptr;
  gr.nodes = d_group_nodes;
  gr.n = n_groups;
  gr.m = n_group_nodes;
  return routes_on_device(ctx, d, d_sources, n, flags, gr, d_metric, d_nh, nh_bytes, d_n_best,
                          stream ? reinterpret_cast<hipStream_t>(stream) : d.stream);
}

int openr_spf_whatif_routes(openr_spf_ctx* ctx, const uint32_t* set_ptr, const uint32_t* set_links, uint32_t n_sets,
                            const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                            const openr_spf_groups_t* groups, uint32_t* changed_routes,
                            openr_spf_whatif_routes_t* delta, uint64_t* out_solved) {
  if (n_sets && !set_ptr) return fail(OPENR_SPF_EINVAL, "null set_ptr");
  return whatif_routes_host(ctx, host_sets(set_ptr, set_links, n_sets), sources, n_sources, flags, groups,
                            changed_routes, delta, out_solved);
}

int openr_spf_whatif_routes_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_set_ptr,
                                   const uint32_t* d_set_links, uint32_t n_sets, uint32_t n_set_links,
                                   const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                   const uint32_t* d_group_ptr, const uint32_t* d_group_nodes, uint32_t n_groups,
                                   uint32_t n_group_nodes, uint32_t* d_changed_routes, uint64_t* d_ptr,
                                   uint32_t* d_group, uint64_t* d_metric, uint8_t* d_nh, uint32_t* d_n_best,
                                   uint64_t cap, uint32_t nh_bytes, void* stream, uint64_t* out_total,
                                   uint64_t* out_solved) {
  return whatif_routes_device_form(ctx, device_index, device_sets(d_set_ptr, d_set_links, n_sets, n_set_links), -1,
                                   d_sources, n_sources, flags, d_group_ptr, d_group_nodes, n_groups, n_group_nodes,
                                   d_changed_routes, d_ptr, d_group, d_metric, d_nh, d_n_best, cap, nh_bytes, stream,
                                   out_total, out_solved);
}

int openr_spf_lfa_routes(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n, uint32_t flags,
                         const openr_spf_groups_t* groups, uint64_t* metric, uint8_t* nh, uint8_t* alt,
                         uint32_t nh_bytes, uint32_t* n_alt, openr_spf_lfa_entries_t* entries,
                         uint64_t* out_solved) {
  return lfa_host(ctx, sources, n, flags, groups, metric, nh, alt, nh_bytes, n_alt, entries, out_solved);
}

int openr_spf_lfa_routes_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_sources, uint32_t n,
                                uint32_t flags, const uint32_t* d_group_ptr, const uint32_t* d_group_nodes,
                                uint32_t n_groups, uint32_t n_group_nodes, uint64_t* d_metric, uint8_t* d_nh,
                                uint8_t* d_alt, uint32_t nh_bytes, uint32_t* d_n_alt, uint64_t* d_ptr,
                                uint32_t* d_nbr, uint64_t* d_alt_metric, uint64_t cap, void* stream,
                                uint64_t* out_total, uint64_t* out_solved) {
  clear_launch_trace();
  if (out_total) *out_total = 0;
  if (out_solved) *out_solved = 0;
  if (int e = check_ctx(ctx)) return e;
  if (int e = check_device_index(ctx, device_index)) return e;
  if ((n && !d_sources) || (n_groups && !d_group_ptr) || (n_group_nodes && !d_group_nodes) ||
      (n && n_groups && !d_metric))
    return fail(OPENR_SPF_EINVAL, "null sources, groups or metric");
  if (cap && (!d_ptr || !d_nbr || !d_alt_metric)) return fail(OPENR_SPF_EINVAL, "null entry buffer");
  int rc = check_routes_metric(ctx, flags);
  if (rc) return rc;
  Device& d = ctx->devs[device_index];
  HIP_TRY(hipSetDevice(d.ordinal));
  DevGroups gr;
  gr.ptr = d_group_ptr;
  gr.nodes = d_group_nodes;
  gr.n = n_groups;
  gr.m = n_group_nodes;
  LfaOut out;
  out.metric = d_metric;
  out.nh = d_nh;
  out.alt = d_alt;
  out.nhb = nh_bytes;
  out.n_alt = d_n_alt;
  out.entries = d_ptr != nullptr;
  out.ptr = d_ptr;
  out.nbr = d_nbr;
  out.alt_metric = d_alt_metric;
  out.cap = cap;
  uint64_t total = 0, solved = 0;
  rc = lfa_on_device(ctx, d, d_sources, n, flags, gr, out, stream ? reinterpret_cast<hipStream_t>(stream) : d.stream,
                     &total, &solved);
  if (out_total) *out_total = total;
  if (out_solved) *out_solved = solved;
  return rc;
}

int openr_spf_whatif_lfa(openr_spf_ctx* ctx, const uint32_t* set_ptr, const uint32_t* set_links, uint32_t n_sets,
                         const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                         const openr_spf_groups_t* groups, uint32_t* changed, uint32_t* unprotected,
                         uint32_t* lost_backup, openr_spf_whatif_lfa_t* delta, uint64_t* out_solved) {
  if (n_sets && !set_ptr) return fail(OPENR_SPF_EINVAL, "null set_ptr");
  return whatif_lfa_host(ctx, host_sets(set_ptr, set_links, n_sets), sources, n_sources, flags, groups, changed,
                         unprotected, lost_backup, delta, out_solved);
}

int openr_spf_whatif_lfa_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_set_ptr,
                                const uint32_t* d_set_links, uint32_t n_sets, uint32_t n_set_links,
                                const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                const uint32_t* d_group_ptr, const uint32_t* d_group_nodes, uint32_t n_groups,
                                uint32_t n_group_nodes, uint32_t* d_changed, uint32_t* d_unprotected,
                                uint32_t* d_lost_backup, uint64_t* d_ptr, uint32_t* d_group, uint64_t* d_metric,
                                uint8_t* d_nh, uint8_t* d_alt, uint64_t cap, uint32_t nh_bytes, void* stream,
                                uint64_t* out_total, uint64_t* out_solved) {
  clear_launch_trace();
  if (out_total) *out_total = 0;
  if (out_solved) *out_solved = 0;
  if (int e = check_ctx(ctx)) return e;
  if (int e = check_device_index(ctx, device_index)) return e;
  if ((n_sets && !d_set_ptr) || (n_sources && !d_sources) || (n_sets && n_sources && !d_changed))
    return fail(OPENR_SPF_EINVAL, "null sets, sources or changed");
  if ((n_groups && !d_group_ptr) || (n_group_nodes && !d_group_nodes))
    return fail(OPENR_SPF_EINVAL, "null group_ptr or group_nodes");
  if (cap && (!d_ptr || !d_group || !d_metric || !d_nh || !d_alt)) return fail(OPENR_SPF_EINVAL, "null entry buffer");
  int rc = check_routes_metric(ctx, flags);
  if (rc) return rc;
  Device& d = ctx->devs[device_index];
  HIP_TRY(hipSetDevice(d.ordinal));
  DevGroups gr;
  gr.ptr = d_group_ptr;
  gr.nodes = d_group_nodes;
  gr.n = n_groups;
  gr.m = n_group_nodes;
  WlfaOut out;
  out.changed = d_changed;
  out.unprot = d_unprotected;
  out.lost = d_lost_backup;
  out.ptr = d_ptr;
  out.group = d_group;
  out.metric = d_metric;
  out.nh = d_nh;
  out.alt = d_alt;
  out.cap = cap;
  out.nhb = nh_bytes;
  uint64_t total = 0, solved = 0;
  rc = whatif_lfa_on_device(ctx, d, device_sets(d_set_ptr, d_set_links, n_sets, n_set_links), d_sources, n_sources,
                            flags, gr, out, stream ? reinterpret_cast<hipStream_t>(stream) : d.stream, &total,
                            &solved);
  if (out_total) *out_total = total;
  if (out_solved) *out_solved = solved;
  return rc;
}

// ---- loop-free alternates under drain, metric, restore and maintenance events (spf_elfa.hip) --
int openr_spf_whatif_drain_lfa(openr_spf_ctx* ctx, const openr_spf_drain_events_t* events, const uint32_t* sources,
                               uint32_t n_sources, uint32_t flags, const openr_spf_groups_t* groups,
                               uint32_t* changed, uint32_t* unprotected, uint32_t* lost_backup,
                               openr_spf_whatif_lfa_t* delta, uint64_t* out_solved) {
  return event_lfa_host(ctx, kElfaDrain, events, sources, n_sources, flags, groups, changed, unprotected, lost_backup,
                        delta, out_solved);
}

int openr_spf_whatif_drain_lfa_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                      const uint32_t* d_nodes, const uint32_t* d_link_ptr, const uint32_t* d_links,
                                      uint32_t n_events, uint32_t n_nodes, uint32_t n_links,
                                      const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                      const uint32_t* d_group_ptr, const uint32_t* d_group_nodes, uint32_t n_groups,
                                      uint32_t n_group_nodes, uint32_t* d_changed, uint32_t* d_unprotected,
                                      uint32_t* d_lost_backup, uint64_t* d_ptr, uint32_t* d_group,
                                      uint64_t* d_metric, uint8_t* d_nh, uint8_t* d_alt, uint64_t cap,
                                      uint32_t nh_bytes, void* stream, uint64_t* out_total, uint64_t* out_solved) {
  return event_lfa_device(ctx, device_index,
                          drain_units(d_node_ptr, d_nodes, d_link_ptr, d_links, n_events, n_nodes, n_links),
                          kElfaDrain, d_sources, n_sources, flags, d_group_ptr, d_group_nodes, n_groups,
                          n_group_nodes, d_changed, d_unprotected, d_lost_backup, d_ptr, d_group, d_metric, d_nh,
                          d_alt, cap, nh_bytes, stream, out_total, out_solved);
}

int openr_spf_whatif_metric_lfa(openr_spf_ctx* ctx, const openr_spf_metric_events_t* events, const uint32_t* sources,
                                uint32_t n_sources, uint32_t flags, const openr_spf_groups_t* groups,
                                uint32_t* changed, uint32_t* unprotected, uint32_t* lost_backup,
                                openr_spf_whatif_lfa_t* delta, uint64_t* out_solved) {
  return event_lfa_host(ctx, kElfaMetric, events, sources, n_sources, flags, groups, changed, unprotected, lost_backup,
                        delta, out_solved);
}

int openr_spf_whatif_metric_lfa_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_edge_ptr,
                                       const uint32_t* d_edges, const uint32_t* d_metrics, uint32_t n_events,
                                       uint32_t n_edges, const uint32_t* d_sources, uint32_t n_sources,
                                       uint32_t flags, const uint32_t* d_group_ptr, const uint32_t* d_group_nodes,
                                       uint32_t n_groups, uint32_t n_group_nodes, uint32_t* d_changed,
                                       uint32_t* d_unprotected, uint32_t* d_lost_backup, uint64_t* d_ptr,
                                       uint32_t* d_group, uint64_t* d_metric, uint8_t* d_nh, uint8_t* d_alt,
                                       uint64_t cap, uint32_t nh_bytes, void* stream, uint64_t* out_total,
                                       uint64_t* out_solved) {
  return event_lfa_device(ctx, device_index, metric_units(d_edge_ptr, d_edges, d_metrics, n_events, n_edges),
                          kElfaMetric, d_sources, n_sources, flags, d_group_ptr, d_group_nodes, n_groups,
                          n_group_nodes, d_changed, d_unprotected, d_lost_backup, d_ptr, d_group, d_metric, d_nh,
                          d_alt, cap, nh_bytes, stream, out_total, out_solved);
}

int openr_spf_whatif_restore_lfa(openr_spf_ctx* ctx, const openr_spf_restore_events_t* events,
                                 const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                                 const openr_spf_groups_t* groups, uint32_t* changed, uint32_t* unprotected,
                                 uint32_t* lost_backup, openr_spf_whatif_lfa_t* delta, uint64_t* out_solved) {
  return event_lfa_host(ctx, kElfaRestore, events, sources, n_sources, flags, groups, changed, unprotected,
                        lost_backup, delta, out_solved);
}

int openr_spf_whatif_restore_lfa_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                        const uint32_t* d_nodes, const uint32_t* d_link_ptr, const uint32_t* d_links,
                                        const uint32_t* d_edge_ptr, const uint32_t* d_edges,
                                        const uint32_t* d_metrics, uint32_t n_events, uint32_t n_nodes,
                                        uint32_t n_links, uint32_t n_edges, const uint32_t* d_sources,
                                        uint32_t n_sources, uint32_t flags, const uint32_t* d_group_ptr,
                                        const uint32_t* d_group_nodes, uint32_t n_groups, uint32_t n_group_nodes,
                                        uint32_t* d_changed, uint32_t* d_unprotected, uint32_t* d_lost_backup,
                                        uint64_t* d_ptr, uint32_t* d_group, uint64_t* d_metric, uint8_t* d_nh,
                                        uint8_t* d_alt, uint64_t cap, uint32_t nh_bytes, void* stream,
                                        uint64_t* out_total, uint64_t* out_solved) {
  return event_lfa_device(ctx, device_index,
                          restore_units(d_node_ptr, d_nodes, d_link_ptr, d_links, d_edge_ptr, d_edges, d_metrics,
                                        n_events, n_nodes, n_links, n_edges),
                          kElfaRestore, d_sources, n_sources, flags, d_group_ptr, d_group_nodes, n_groups,
                          n_group_nodes, d_changed, d_unprotected, d_lost_backup, d_ptr, d_group, d_metric, d_nh,
                          d_alt, cap, nh_bytes, stream, out_total, out_solved);
}

// Loop-free alternates under a maintenance event: the maintenance sweep's rows under the drain's
// pass (kElfaMaint; the argument is at openr_spf_whatif_maint_lfa and in spf_elfa.hip's header).
int openr_spf_whatif_maint_lfa(openr_spf_ctx* ctx, const openr_spf_maint_events_t* events, const uint32_t* sources,
                               uint32_t n_sources, uint32_t flags, const openr_spf_groups_t* groups,
                               uint32_t* changed, uint32_t* unprotected, uint32_t* lost_backup,
                               openr_spf_whatif_lfa_t* delta, uint64_t* out_solved) {
  return event_lfa_host(ctx, kElfaMaint, events, sources, n_sources, flags, groups, changed, unprotected, lost_backup,
                        delta, out_solved);
}

int openr_spf_whatif_maint_lfa_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                      const uint32_t* d_nodes, const uint32_t* d_link_ptr, const uint32_t* d_links,
                                      const uint32_t* d_edge_ptr, const uint32_t* d_edges, const uint32_t* d_metrics,
                                      uint32_t n_events, uint32_t n_nodes, uint32_t n_links, uint32_t n_edges,
                                      const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                      const uint32_t* d_group_ptr, const uint32_t* d_group_nodes, uint32_t n_groups,
                                      uint32_t n_group_nodes, uint32_t* d_changed, uint32_t* d_unprotected,
                                      uint32_t* d_lost_backup, uint64_t* d_ptr, uint32_t* d_group,
                                      uint64_t* d_metric, uint8_t* d_nh, uint8_t* d_alt, uint64_t cap,
                                      uint32_t nh_bytes, void* stream, uint64_t* out_total, uint64_t* out_solved) {
  return event_lfa_device(ctx, device_index,
                          maint_units(d_node_ptr, d_nodes, d_link_ptr, d_links, d_edge_ptr, d_edges, d_metrics,
                                      n_events, n_nodes, n_links, n_edges),
                          kElfaMaint, d_sources, n_sources, flags, d_group_ptr, d_group_nodes, n_groups,
                          n_group_nodes, d_changed, d_unprotected, d_lost_backup, d_ptr, d_group, d_metric, d_nh,
                          d_alt, cap, nh_bytes, stream, out_total, out_solved);
}

int openr_spf_ksp2(openr_spf_ctx* ctx, const uint32_t* src, const uint32_t* dst, uint32_t n_pairs,
                   uint32_t tok_cap, uint32_t* tok1, uint32_t* tok2) {
  clear_launch_trace();
  if (!ctx) return fail(OPENR_SPF_EINVAL, "null context");
  if (!ctx->has_graph) return fail(OPENR_SPF_EINVAL, "no graph set (openr_spf_set_graph)");
  if (n_pairs && (!src || !dst || !tok1 || !tok2)) return fail(OPENR_SPF_EINVAL, "null argument");
  if (tok_cap < 1) return fail(OPENR_SPF_EINVAL, "tok_cap must be >= 1");
  if (!ksp_lds_bytes(ctx->V, ctx->L, ctx->devs[0].g.max_deg))
    return fail(OPENR_SPF_E2BIG, "too many links (%u) for the KSP tracer", ctx->L);
  if (!ctx->metric_ok)  // the tracer walks dist[u] + w == dist[v]: ambiguous under zero metrics
    return fail(OPENR_SPF_ENOTSUP, "KSP2 needs usable metrics in [1, 2^31-1]");
  // distinct sources (the memoized SPF of each), pair -> base row
  std::vector<uint32_t> srcs, prow(n_pairs), row_of(ctx->V, UINT32_MAX);
  for (uint32_t i = 0; i < n_pairs; ++i) {
    if (src[i] >= ctx->V || dst[i] >= ctx->V) return fail(OPENR_SPF_EINVAL, "pair %u out of range", i);
    if (row_of[src[i]] == UINT32_MAX) {
      row_of[src[i]] = (uint32_t)srcs.size();
      srcs.push_back(src[i]);
    }
    prow[i] = row_of[src[i]];
  }
  Plan bp, ip;
  int rc = whatif_plans(ctx, OPENR_SPF_USE_LINK_METRIC, &bp, &ip);  // getKthPaths uses link metrics
  if (rc) return rc;
  if (!n_pairs) return OPENR_SPF_OK;
  const auto t0 = std::chrono::steady_clock::now();
  Device& d = ctx->devs[0];
  HIP_TRY(hipSetDevice(d.ordinal));
  HIP_TRY(d.kin_src.reserve(srcs.size()));
  HIP_TRY(d.kin_row.reserve(n_pairs));
  HIP_TRY(d.kin_dst.reserve(n_pairs));
  HIP_TRY(d.ktok1.reserve((size_t)n_pairs * tok_cap));
  HIP_TRY(d.ktok2.reserve((size_t)n_pairs * tok_cap));
  HIP_TRY(hipMemcpyAsync(d.kin_src.p, srcs.data(), srcs.size() * 4u, hipMemcpyHostToDevice, d.stream));
  HIP_TRY(hipMemcpyAsync(d.kin_row.p, prow.data(), (size_t)n_pairs * 4u, hipMemcpyHostToDevice, d.stream));
  HIP_TRY(hipMemcpyAsync(d.kin_dst.p, dst, (size_t)n_pairs * 4u, hipMemcpyHostToDevice, d.stream));
  bool overflow = false;
  HIP_TRY(ksp2_on_device(ctx, d, bp, ip, d.kin_src.p, (uint32_t)srcs.size(), d.kin_row.p, d.kin_dst.p, n_pairs,
                         tok_cap, d.ktok1.p, d.ktok2.p, d.stream, &overflow));
  HIP_TRY(hipMemcpyAsync(tok1, d.ktok1.p, (size_t)n_pairs * tok_cap * 4u, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(hipMemcpyAsync(tok2, d.ktok2.p, (size_t)n_pairs * tok_cap * 4u, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(hipStreamSynchronize(d.stream));
  ctx->stats.spf_runs += srcs.size() + n_pairs;
  ctx->stats.batches += 1;
  ctx->stats.last_batch_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (overflow)
    return fail(OPENR_SPF_E2BIG,
                "a pair's paths exceed tok_cap=%u tokens or %u hops, or its trace more than %u pathLinks on the DFS "
                "stack (marked 0xFFFFFFFF)",
                tok_cap, kKspMaxDepth - 1u, kKspArena);
  return OPENR_SPF_OK;
}

int openr_spf_ksp2_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_sources, uint32_t n_sources,
                          const uint32_t* d_pair_row, const uint32_t* d_pair_dst, uint32_t n_pairs, uint32_t tok_cap,
                          uint32_t* d_tok1, uint32_t* d_tok2, void* stream) {
  clear_launch_trace();
  if (!ctx) return fail(OPENR_SPF_EINVAL, "null context");
  if (!ctx->has_graph) return fail(OPENR_SPF_EINVAL, "no graph set (openr_spf_set_graph)");
  if (device_index < 0 || device_index >= (int)ctx->devs.size())
    return fail(OPENR_SPF_EINVAL, "device_index %d out of range", device_index);
  if (n_pairs && (!d_sources || !d_pair_row || !d_pair_dst || !d_tok1 || !d_tok2))
    return fail(OPENR_SPF_EINVAL, "null argument");
  if (tok_cap < 1) return fail(OPENR_SPF_EINVAL, "tok_cap must be >= 1");
  if (!ksp_lds_bytes(ctx->V, ctx->L, ctx->devs[0].g.max_deg))
    return fail(OPENR_SPF_E2BIG, "too many links (%u) for the KSP tracer", ctx->L);
  if (!ctx->metric_ok)  // the tracer walks dist[u] + w == dist[v]: ambiguous under zero metrics
    return fail(OPENR_SPF_ENOTSUP, "KSP2 needs usable metrics in [1, 2^31-1]");
  Plan bp, ip;
  int rc = whatif_plans(ctx, OPENR_SPF_USE_LINK_METRIC, &bp, &ip);
  if (rc) return rc;
  Device& d = ctx->devs[device_index];
  HIP_TRY(hipSetDevice(d.ordinal));
  hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : d.stream;
  bool overflow = false;
  HIP_TRY(ksp2_on_device(ctx, d, bp, ip, d_sources, n_sources, d_pair_row, d_pair_dst, n_pairs, tok_cap, d_tok1,
                         d_tok2, s, &overflow));
  ctx->stats.spf_runs += (uint64_t)n_sources + n_pairs;
  ctx->stats.batches += 1;
  if (overflow)
    return fail(OPENR_SPF_E2BIG,
                "a pair's paths exceed tok_cap=%u tokens or %u hops, or its trace more than %u pathLinks on the DFS "
                "stack (marked 0xFFFFFFFF)",
                tok_cap, kKspMaxDepth - 1u, kKspArena);
  return OPENR_SPF_OK;
}

int openr_spf_get_stats(const openr_spf_ctx* ctx, openr_spf_stats_t* out) {
  if (!ctx || !out) return fail(OPENR_SPF_EINVAL, "null argument");
  *out = ctx->stats;
  return OPENR_SPF_OK;
}

}  // extern "C"
