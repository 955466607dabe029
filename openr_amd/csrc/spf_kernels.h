// spf_kernels.h — device-side graph layout and kernel launchers of the SPF engine.
//
// One workgroup owns one solve at a time (persistent loop over the batch): the
// per-solve state (levels / distances, next-hop bitsets, frontier) lives in LDS,
// the CSR mirror is streamed from L2/HBM and shared by every workgroup.
// See DESIGN.md "Kernels" for the roofline accounting.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

namespace openr_spf {

// Device copy of the CSR mirror (include/openr_spf.h openr_spf_graph), packed for
// the kernels. Built once per openr_spf_set_graph on every device of the context.
struct DevGraph {
  uint32_t V = 0, E = 0, L = 0;
  uint32_t max_deg = 0;        // largest row (source expansion must fit the frontier queue)
  uint32_t est_width2 = 0;     // sampled max |level L| + |level L+1| of a BFS (ring sizing)
  uint32_t est_width1 = 0;     // sampled max |level L| (lean BFS pass: queue halves)
  uint32_t est_depth = 0;      // sampled max BFS depth (family choice, u8 level limit)
  uint32_t* row = nullptr;     // [V+1]
  uint2* row2 = nullptr;       // [V] (row[u], row[u+1]) in one 8-byte load
  uint2* row2t = nullptr;      // [V] transit row: row2[u], or an empty range when u is overloaded
                               //     (an overloaded node other than the source is never expanded)
  uint32_t* ovl_bits = nullptr;  // [ceil(V/32)] overloaded bitmap (staged into LDS)
  uint4* ellt = nullptr;       // [V] first 4 edges of each transit row (adj encoding, kEdgeDown-padded)
  uint4* ellv = nullptr;       // [ellv_rows(V)] ellt with every down / padding slot replaced by the node id V (a
                               //     level sentinel the lvl kernel keeps at 0: never tight, no flag tests);
                               //     ellv[V] = (V, V, V, V), the row of a lane past the frontier;
  uint32_t* elld = nullptr;    // [V] ellv as four signed byte deltas (v - u; 0 = no edge), or null
  // [E] erec with every row's entries sorted by (name rank of the neighbour, reverse edge):
  // for uniform cost that is the reference's pathLinks order (DijkstraQ pops equal
  // distances by name; LinkState.cpp:820-829), so the KSP tracer ranks a frame's
  // candidates by their position alone
  uint4* erecs = nullptr;
                               //     when a row has > 4 edges or a column > 127 ids away (wave pass)
  uint32_t* adj = nullptr;     // [E] col | kEdgeDown when !edge_up
  uint32_t* w = nullptr;       // [E] metric u->v (u32; usable edges are in [1, 2^31-1])
  uint64_t* w64 = nullptr;     // [E] metric u->v as the caller gave it (exact-order kernel: 0 / wrapped values)
  uint32_t* win = nullptr;     // [E] metric of the reverse edge (col -> row owner)
  uint32_t* rev = nullptr;     // [E] index of the reverse edge
  uint32_t* lid = nullptr;     // [E] undirected link id
  uint16_t* nbr = nullptr;     // [E] distinct-neighbour index of col within its row
  uint8_t* ovl = nullptr;      // [V] overloaded
  uint8_t* derivable = nullptr;  // [V] derive colouring: an independent set of the link structure (spf_derive.hip)
  uint8_t* cls = nullptr;      // [V] source class of each node, code family (SrcClass)
  uint8_t* cls_lvl = nullptr;  // [V] source class of each node, lvl family (LvlClass)
  uint2* ledge = nullptr;      // [L] the two directed edges of each link (UINT32_MAX if unused)
  uint32_t* rank = nullptr;    // [V] name rank (pathLinks / pop-order tie-break)
  uint4* erec = nullptr;       // [E] packed edge e = u->col: {col | kEdgeDown | kNodeSink if col is
                               //     overloaded, win[e], lid[e], rev[e]} (one 16-byte load per edge)
};

constexpr uint32_t kEdgeDown = 0x80000000u;
// Sink flag of a transit row: ellt[u].x and row2t[u].x carry it when u is overloaded.
// (row2t of a sink is an empty range whose begin carries the flag, so it never loops.)
constexpr uint32_t kNodeSink = 0x40000000u;
constexpr uint32_t kBlock = 256;
// ellv slot of an ellt slot: the column, or V for a down / padding / sink-row slot
__host__ __device__ inline uint4 ellv_of(uint4 t, uint32_t V) {
  auto f = [V](uint32_t x) { return (x & kEdgeDown) ? V : x; };
  return make_uint4(f(t.x), f(t.y), f(t.z), f(t.w));
}
// elld row of an ellv row: the four slots as signed byte deltas v - u (0: V, no edge)
__host__ __device__ inline uint32_t elld_of(uint4 r, uint32_t u, uint32_t V) {
  auto d = [u, V](uint32_t x) -> uint32_t { return x >= V ? 0u : (uint32_t)(uint8_t)(int8_t)((int32_t)x - (int32_t)u); };
  return d(r.x) | (d(r.y) << 8) | (d(r.z) << 16) | (d(r.w) << 24);
}
constexpr uint32_t kBfsEdgesPerLane = 4;  // edges a lane loads ahead per pass (register prefetch)
constexpr uint32_t kBfsTargetWgs = 12;    // lvl BFS sizes its ring for this many workgroups per CU (G100: 8 -> 1.06 ms, 9..16 -> 1.02 ms)

// Next-hop bitset storage classes in LDS (chosen from the max distinct degree).
enum NhMode : int { kNhByte = 0, kNhHalf = 1, kNhW1 = 2, kNhW2 = 3, kNhW4 = 4, kNhW8 = 5, kNhNibble = 6 };
int nh_mode_for_bits(uint32_t bits);            // -1 if > 256 bits
uint32_t nh_mode_lds_bytes(int mode, uint32_t V);
uint32_t nh_words_for(int mode, uint32_t V);     // LDS dwords of V next-hop sets
bool nh_mode_single(int mode);                  // one node's set lives inside one dword
// persistent grid: workgroups that fit a CU by LDS (<= 2048 threads) x CUs, <= n
uint32_t blocks_for(uint32_t n, uint32_t lds, int num_cus, uint32_t block = 256);
// grid-stride grid: one workgroup per per_block items, at most 8 per CU, at least one
uint32_t grid_for(uint64_t items, uint32_t per_block, int num_cus);

struct LaunchInfo {
  uint32_t lds_bytes = 0;
  uint32_t grid = 0;
  const char* kernel = "";
};
// Launch trace (openr_spf_last_kernels): every solve launcher records the kernel it
// enqueued; the C-ABI clears the calling thread's trace at the start of each solve call.
void note_launch(const char* kernel);
void clear_launch_trace();

// Optional per-unit delta of a what-if sweep (openr_spf_whatif_delta): the nodes whose
// distance or next-hop set a unit's failure changes, with their new values. Unit u's
// entries are pool slots [off[u], off[u] + changed[u]) in no particular order; a unit
// reserves its slots with one atomic on `used`, and slots past `cap` are not written
// (used then exceeds cap: the caller reports OPENR_SPF_E2BIG).
struct WhatifDelta {
  uint32_t* off = nullptr;             // [units] (unit = link index * n_src + source index)
  uint32_t* node = nullptr;            // [cap] node id; null: no delta output
  unsigned long long* dist = nullptr;  // [cap] new distance (UINT64_MAX: not reached)
  uint8_t* nh = nullptr;               // [cap][nhb] new next-hop bits, zero padded past the graph's width
  uint32_t cap = 0, nhb = 0;
  unsigned long long* used = nullptr;  // pool cursor (device counter, zeroed by the launcher)
  __device__ uint32_t base_of(unsigned long long b) const { return b < 0xFFFFFFFFull ? (uint32_t)b : 0xFFFFFFFFu; }
};

// Derived rows (spf_derive.hip): rows == null means the batch is not split. Solved units
// leave their u8 level row at rows[sid * stride] and stamp valid[sid] = epoch; derived unit
// j < *count is class-local index n + j of the launch's perm.
// Distinct neighbours of a derivable node. Only the lean and the wave pass leave level rows,
// and both need every row within the 4 ELL slots, so no split batch ever meets a wider node.
constexpr uint32_t kDeriveMaxNbrs = 4;
struct DeriveArgs {
  uint8_t* rows;           // [n][stride] level rows of the solved units (0xFF: not reached)
  uint32_t stride;         // bytes per row, a multiple of 16, >= V rounded up to 16
  uint32_t epoch;          // this call's stamp (never 0)
  uint32_t* valid;         // [n] epoch of the row each sid holds
  // [n][2 * kDeriveMaxNbrs] per derived sid: its neighbour i when usable (else all ones), then the
  // sid whose level row that neighbour contributes (all ones: none, it is overloaded)
  const uint32_t* nbrs;
  const uint32_t* count;   // device: derived units of the batch
};

struct SolveArgs {
  const uint32_t* sources;
  uint32_t n;
  const uint32_t* ign_ptr;    // nullable: solve i ignores ign_links[ign_ptr[i], end_i)
  const uint32_t* ign_links;
  const uint32_t* ign_end;    // nullable: end_i = ign_end[i], else ign_ptr[i + 1]
  uint64_t* dist;             // [n][V]
  uint8_t* nh;                // nullable [n][V][nh_bytes]
  uint32_t nh_bytes;
  uint64_t* tight;            // nullable [n][ceil(E/64)] (zeroed by the launcher)
  uint32_t nh_bits;           // bits that are meaningful (max distinct degree)
  uint32_t* ovf_list;         // [n * nsl] scratch: units the ring variant could not finish (re-run list)
  uint32_t* work;             // [kWorkSlots] per-class launch counters (zero at rest: kernels reset them)
  // Source classes (next-hop width): when perm != nullptr this launch solves only the
  // sources of class `cls`: solve k < part[cls] is sid = perm[part[kMaxClasses + cls] + k]
  // (part / perm in device memory, built by partition_sources or the host).
  const uint32_t* perm;
  const uint32_t* part;       // [2 * kMaxClasses]: counts, then offsets
  uint32_t cls;
  uint32_t nsl;               // next-hop slices per solve (sliced class), else 1
  uint32_t dist_only;         // code family: no next-hop output, so no next-hop bits (one class);
                              // bit 1: the KSP2 target's pull test (2) in its per-wave form (A/B)
  // nullable, honoured by dist_only code-family solves: solve sid may stop once the level
  // of target[sid] is known; nodes at the target's distance or farther, other than the
  // target, then read UINT64_MAX (a KSP trace to the target only reads nodes nearer)
  const uint32_t* target;
  // nullable, dist_only code-family solves (GENERIC kernels) only: write u16 level rows
  // [n][V] here instead of u64 distance rows (0xFFFF = unreached; dist = level * cost;
  // levels stay below V <= 65535). KSP2 second SPFs: 4x fewer bytes per pair row.
  uint16_t* lvl16;
  // lvl16 rows in tagged form when lvl_tag != 0 (KSP2 second SPFs, round 3): a node's entry
  // is (lvl_tag << lvl_shift) | level, written only when the node is settled; the unreached
  // fill is skipped, so a row costs the bytes of the nodes the (target-bounded) solve
  // reached, and an entry with another tag reads as unreached. Levels < V < 2^lvl_shift.
  uint32_t lvl_tag, lvl_shift;
  // nullable: solve sid writes its dist / nh / tight rows at row out_row[sid] instead of
  // sid (openr_spf_refresh re-solves a scattered subset of resident rows in place; the
  // launcher then leaves zeroing those tight rows to the caller)
  const uint32_t* out_row;
  unsigned long long* prof;   // profiling builds only: per-phase cycle sums (nullable)
  uint32_t* order;            // nullable [n][V]: pop index per node (exact-order kernel only)
  // nullable, level family (OPENR_SPF_EMIT_LEVELS8 / 16): level rows [n][V] of lvl_bytes
  // (1 or 2) per node here instead of the u64 distance rows (dist = level x cost; all
  // ones = unreached); a finite level a u8 row cannot hold is written 0xFE and sets
  // kStatusLevelOverflow in *status
  uint8_t* lvl_rows;
  uint32_t lvl_bytes;
  // nullable, rounds kernel with an ignore set (what-if re-solves of large units, round 4):
  // solve sid starts from base row j = seed_unit[sid] % seed_nsrc of seed_dist / seed_tight
  // (the source's SPF without the ignore set, and its tight-edge mask) instead of from
  // scratch: only the nodes whose distance the ignored links raise are re-solved
  const uint64_t* seed_dist;
  const uint64_t* seed_tight;
  const uint32_t* seed_unit;
  uint32_t seed_nsrc;
  // nullable with seed_dist: instead of writing rows, compare the solve with the base rows
  // (seed_dist, seed_nh: nh_bytes per node) and store the count of nodes whose distance or
  // next-hop bytes differ at seed_changed[seed_unit[sid]] (the what-if unit's answer)
  const uint8_t* seed_nh;
  uint32_t* seed_changed;
  WhatifDelta delta;  // with seed_changed: the unit's changed nodes and their new rows (node == null: off)
  // rounds kernel: tin_out (nullable, solves without a seed) receives each solve's tight
  // in-degree row [out_row][V] (u16); seed_tin (nullable, with seed_dist) is such a row set
  // for the base SPF, so a seeded start reads the counts instead of scanning every in-edge
  uint16_t* tin_out;
  const uint16_t* seed_tin;
  // nullable (rounds kernel, generic): the solve count is min(n, *n_dev), read on the device
  // (n sizes the grid; n_block = threads per solve, 64 / 128 / 256) -- no host round trip
  // for a count the previous kernel produced
  const uint32_t* n_dev;
  uint32_t n_block;
  unsigned long long* prof_solve;  // nullable (OPENR_SPF_PROF): rounds kernel per-solve wall-clock start / end
  uint32_t* status;
  // code-family sliced class with next-hop output: [krows][nsl][V] 29-bit chunks of the
  // sets (slice s = bits [29s, 29s + 29)); launch_bfs_code merges them into nh rows
  uint32_t* slice_tmp;
  // sliced class with next-hop output, chunked: this launch solves the class-local solves
  // [k0, k0 + krows) and slice_tmp holds krows of them (row k - k0); krows 0 = the whole class
  uint32_t k0, krows;
  DeriveArgs dv;  // lean / wave pass of a split batch (launch_derive_split), else zero
};
__host__ __device__ constexpr uint32_t ellv_rows(uint32_t V) { return V + 1u; }
// output row of solve sid (SolveArgs::out_row)
__host__ __device__ inline size_t out_row_of(const SolveArgs& a, uint32_t sid) {
  return a.out_row ? (size_t)a.out_row[sid] : (size_t)sid;
}
constexpr uint32_t kMaxClasses = 8;
constexpr uint32_t kCtrPerClass = 8;  // [0,1] fast launch, [2,3] re-run launch, [4] flagged solves
constexpr uint32_t kWorkSlots = kCtrPerClass * kMaxClasses;
constexpr uint32_t kStatusLevelOverflow = 1u;  // = OPENR_SPF_STATUS_LEVEL_OVERFLOW
constexpr uint32_t kFringeCtr = kCtrPerClass * (kMaxClasses - 1);  // BFS classes use < 7 blocks
constexpr uint32_t kIncrCtr = kFringeCtr + 2;                        // incremental what-if
constexpr uint32_t kExactCtr = kIncrCtr + 2;                         // exact-order kernel

// Uniform-cost BFS kernel families (spf_capi.hip picks one per graph):
//  * code (spf_bfs.hip): one packed LDS field per node = [next-hop bits | 3-bit level
//    code]; distances stored when a node is expanded. Smallest LDS footprint, best on
//    shallow graphs with wide frontiers (fabrics).
//  * lvl (spf_bfs_lvl.hip): exact u8/u16 level per node + packed next-hop sets; the
//    distance row is written coalesced at the end. Best on deep graphs (grids).
enum BfsFamily : int { kFamCode = 0, kFamLvl = 1, kNumFamilies = 2 };

// Source classes by distinct degree (next-hop bitset width).
// code family: the per-node field holds the set plus a 3-bit level code in 8 bits
// (d <= 5), 16 bits (d <= 13) or 32 bits (d <= 29); d > 29 solves in ceil(d / 29)
// slices of 29 next-hop bits, one workgroup pass per slice, merged into bytes afterwards.
enum SrcClass : int { kCls8 = 0, kCls16 = 1, kCls32 = 2, kClsSliced = 3, kNumClasses = 4 };
// lvl family: next-hop sets of 4 / 8 / 16 / 32 bits; d > 32 in 32-bit slices.
enum LvlClass : int { kLvl4 = 0, kLvl8 = 1, kLvl16 = 2, kLvl32 = 3, kLvlSliced = 4, kNumLvlClasses = 5 };
int src_class_for_degree(int family, uint32_t distinct_degree);  // -1 if > 256
int num_classes(int family);
int sliced_class(int family);
uint32_t slice_bits(int family);
// Stable within a class is not required: perm maps class-local index -> sid.
hipError_t launch_partition(const uint32_t* d_sources, uint32_t n, const uint8_t* d_node_cls, uint32_t V,
                            uint32_t* d_part, uint32_t* d_perm, hipStream_t s);

// Uniform edge cost c (all usable edges cost c, or useLinkMetric=false): BFS levels,
// sources of class a.cls of `family` (a.nsl slices for the sliced class).
hipError_t launch_bfs(int family, const DevGraph& g, const SolveArgs& a, uint64_t cost, int group_lanes,
                      int num_cus, hipStream_t s, LaunchInfo* info);
hipError_t launch_bfs_code(const DevGraph& g, const SolveArgs& a, uint64_t cost, int group_lanes, int num_cus,
                           hipStream_t s, LaunchInfo* info);
hipError_t launch_bfs_lvl(const DevGraph& g, const SolveArgs& a, uint64_t cost, int group_lanes, int num_cus,
                          hipStream_t s, LaunchInfo* info);
// true when launch_bfs_lvl runs the batch on the lean or the wave pass, the two passes that
// can leave level rows for a split batch (SolveArgs::dv)
bool bfs_lvl_fast_pass(const DevGraph& g, const SolveArgs& a, int group_lanes, int num_cus);

// Derived rows (spf_derive.hip). For uniform cost the row of a source follows from the rows
// of its neighbours, so of an all-sources batch only a set that covers every link needs a
// BFS; the rule is in that file's header.
// launch_derive_split: member[source] = sid, then entry i is derived iff its node is
// derivable (DevGraph::derivable) and every neighbour it needs (link up, not overloaded) is
// a source of the batch. perm[0 .. part[cls]) = the solved sids, perm[n .. n + *count) the
// derived ones, both ascending; part[kMaxClasses + cls] = 0; nbrs as DeriveArgs::nbrs.
// member: V u32 of scratch, flags: n + 16 bytes.
hipError_t launch_derive_split(const DevGraph& g, const uint32_t* sources, uint32_t n, uint32_t cls, uint32_t* member,
                               uint8_t* flags, uint32_t* nbrs, uint32_t* perm, uint32_t* part, uint32_t* count,
                               int num_cus, hipStream_t s);
// The derived rows of a.dv from the level rows the BFS launch left. A unit one of whose
// neighbour rows is missing (its solve overflowed) is appended to a.ovf_list / *ovf_count
// for the u16 re-run, as class-local index n + j.
hipError_t launch_nh_derive(const DevGraph& g, const SolveArgs& a, uint64_t cost, uint32_t* ovf_count, int num_cus,
                            hipStream_t s);

// General positive metrics (spf_fringe.hip): one wavefront per solve, settle-safe
// buckets of width delta = min usable metric over a fringe list, next hops pulled over
// tight in-edges. Uses a.work[kFringeCtr, +2) for dynamic scheduling.
hipError_t launch_fringe(const DevGraph& g, const SolveArgs& a, uint32_t delta, bool dist64,
                         int nh_mode, int num_cus, hipStream_t s, LaunchInfo* info);
// General positive metrics on shallow graphs (spf_rounds.hip): Bellman-Ford distance
// rounds, then next hops in Kahn order of the tight DAG. Same counters as the fringe.
hipError_t launch_rounds(const DevGraph& g, const SolveArgs& a, bool dist64, int nh_mode, int num_cus,
                         hipStream_t s, LaunchInfo* info);
uint32_t rounds_lds_bytes(uint32_t V, uint32_t L, bool has_ignore, int nh_mode, bool dist64);

// What-if sweep (spf_sweep.hip): unit u = i * n_src + j (links[i] failed, sources[j]).
// Filter: changed[u] = 0 for every unit; units whose link has a tight edge in
// base_tight[j] are appended to (wsrc, wlink, wunit), *wcount of them.
hipError_t launch_whatif_filter(const DevGraph& g, const uint32_t* links, uint32_t n_links, const uint32_t* sources,
                                uint32_t n_src, const uint64_t* base_tight, uint32_t* changed, uint32_t* wsrc,
                                uint32_t* wlink, uint32_t* wunit, uint32_t* wcount, int num_cus, hipStream_t s);
// Link-set form (node failures, shared-risk groups): unit u = i * n_src + j fails every link
// of set i = set_links[set_ptr[i], set_ptr[i + 1]) for sources[j]. changed[u] = 0 for every
// unit; a unit is affected iff some link of its set has a tight edge in base_tight[j] (null
// base_tight: iff some link of its set is a link of the graph). Affected units are appended
// source-major to (wsrc, wunit, wbeg = set_ptr[i], wend = set_ptr[i + 1]), *wcount of them:
// the re-solves run with ign_ptr = wbeg, ign_end = wend, ign_links = set_links. Slices are
// clamped to set_links' n_set_links entries (a malformed device CSR reads nothing past it).
hipError_t launch_whatif_set_filter(const DevGraph& g, const uint32_t* set_ptr, const uint32_t* set_links,
                                    uint32_t n_sets, uint32_t n_set_links, const uint32_t* sources,
                                    uint32_t n_src, const uint64_t* base_tight, uint32_t* changed, uint32_t* wsrc, uint32_t* wunit,
                                    uint32_t* wbeg, uint32_t* wend, uint32_t* wcount, int num_cus, hipStream_t s);
// changed[wunit[k]] = nodes whose dist / next-hop bytes differ from base row wunit[k] % n_src.
// With dl.node: also the unit's changed nodes and their new rows (WhatifDelta).
hipError_t launch_rows_compare(uint32_t n, uint32_t V, uint32_t nb, const uint64_t* dist, const uint8_t* nh,
                               const uint64_t* base_dist, const uint8_t* base_nh, const uint32_t* wunit,
                               uint32_t n_src, uint32_t* changed, const WhatifDelta& dl, int num_cus, hipStream_t s);
// What-if delta compaction: ptr[0, n] = exclusive scan of changed (tsum: one u64 per
// 4096 units of scratch), then every unit's entries from its pool slots (off) to its CSR
// slots (ptr) in node / dist / nh.
hipError_t launch_delta_scan(const uint32_t* changed, size_t n, unsigned long long* tsum, unsigned long long* ptr,
                             hipStream_t s);
hipError_t launch_delta_gather(const uint32_t* changed, size_t n, const uint32_t* off, const unsigned long long* ptr,
                               const WhatifDelta& pool, uint32_t* node, unsigned long long* dist, uint8_t* nh,
                               int num_cus, hipStream_t s);
hipError_t launch_iota(uint32_t* p, uint32_t n, int num_cus, hipStream_t s);
// Incremental what-if (spf_sweep.hip): changed[wunit[k]] for every listed unit from the
// base rows alone (no full re-solve). Uses a.work-style counters `ctr` (2 slots).
hipError_t launch_whatif_incr(const DevGraph& g, const uint32_t* wsrc, const uint32_t* wlink, const uint32_t* wunit,
                              uint32_t count, uint32_t n_src, const uint64_t* base_dist, const uint8_t* base_nh,
                              uint32_t nb, bool unit_cost, bool dist64, uint32_t* changed, uint32_t* ctr,
                              int num_cus, hipStream_t s);
uint32_t whatif_incr_lds_bytes(uint32_t V, uint32_t nb, bool dist64);
// Grouped what-if (spf_sweep.hip, the default): one workgroup per (source, chunk of links)
// stages the source's base rows (dist, next hops, tight mask) in LDS once; its wavefronts
// filter the links (no tight edge -> 0) and repair the affected ones on private overlays.
// Writes every changed[i * n_src + j]; affected[0] = affected units, affected[1] = units
// that outgrew the dirty slots (listed in ovf_*[0, affected[1]) for a re-solve). With
// dl.node, every repaired unit also writes its delta (WhatifDelta).
hipError_t launch_whatif_group(const DevGraph& g, const uint32_t* links, uint32_t n_links, const uint32_t* sources,
                               uint32_t n_src, const uint64_t* base_dist, const uint8_t* base_nh,
                               const uint64_t* base_tight, const uint16_t* base_tin, uint32_t nb, bool unit_cost, bool dist64, uint32_t w_max,
                               uint32_t nh_bits, uint32_t* changed, uint32_t* changed_t, uint32_t* affected,
                               uint32_t* ovf_src, uint32_t* ovf_link, uint32_t* ovf_unit, uint32_t* ctr,
                               const WhatifDelta& dl, int num_cus, hipStream_t s);
// 0 when the grouped repair cannot run on the graph (ids, next-hop width, degree, LDS)
uint32_t whatif_group_lds_bytes(uint32_t V, uint32_t E, uint32_t nb, bool dist64, uint32_t max_deg);

// Route-level results (spf_routes.hip). A group table is a CSR over G prefix groups: group
// k = gnodes[gptr[k], gptr[k + 1]) (M entries, node ids ascending inside a group); its
// route in an SPF row is metric = min dist over the members, nh = OR of the next-hop bytes
// of the members at that minimum, n_best = their number (Decision.cpp:1094-1167).
// routes_reduce: metric [n][G], onh [n][G][onb] (nullable; zero past nb) and nbest [n][G]
// (nullable) from row-major dist [n][V] / nh [n][V][nb]. A lane owns a small group, a wave
// a large one; scratch holds routes_reduce_scratch_words(G) u32.
uint32_t routes_reduce_scratch_words(uint32_t G);
hipError_t launch_routes_reduce(uint32_t n, uint32_t V, uint32_t G, uint32_t M, const uint32_t* gptr,
                                const uint32_t* gnodes, const uint64_t* dist, const uint8_t* nh, uint32_t nb,
                                uint64_t* metric, uint8_t* onh, uint32_t onb, uint32_t* nbest, uint32_t* scratch,
                                int num_cus, hipStream_t s);
// Inverse map node -> groups: iptr [V + 1] (u64, scanned through tsum: one u64 per 4096
// nodes) and inv [M] group ids; cnt / cur are [V] scratch.
hipError_t launch_routes_inverse(uint32_t V, uint32_t G, uint32_t M, const uint32_t* gptr, const uint32_t* gnodes,
                                 uint32_t* cnt, uint32_t* cur, unsigned long long* tsum, unsigned long long* iptr,
                                 uint32_t* inv, int num_cus, hipStream_t s);
// Route-level what-if pass over the units of a link-set sweep (unit u = i * n_src + j): the
// unit's node delta (CSR nptr / nnode / ndist / nnh, nb bytes per next-hop entry) overlaid
// on base row j, the groups with a changed member recomputed and compared with base route
// (j, k). The count pass writes changed[u] for the units with a non-empty node delta (the
// caller zeroes changed[] first); the emit pass writes every changed route at optr[u] + its
// rank in the pass (any order inside a unit).
struct RoutesSweep {
  uint32_t V, G, M, n_src, nb, onb;
  size_t units;
  const uint32_t* gptr;
  const uint32_t* gnodes;
  const unsigned long long* iptr;
  const uint32_t* inv;
  const unsigned long long* nptr;
  const uint32_t* nnode;
  const unsigned long long* ndist;
  const uint8_t* nnh;
  const unsigned long long* bdist;    // base rows [n_src][V]
  const uint8_t* bnh;                 // [n_src][V][nb]
  const unsigned long long* bmetric;  // base routes [n_src][G]
  const uint8_t* bmnh;                // [n_src][G][nb]
  uint32_t* changed;                  // [units]
  const unsigned long long* optr;     // emit pass: [units + 1]
  uint32_t* ogroup;
  unsigned long long* ometric;
  uint8_t* onh;                       // [.][onb], zero past nb
  uint32_t* onbest;                   // nullable
  uint32_t ovl_lds, bm_lds, cand_cap; // RoutesSweepLayout
  uint32_t* g_ovl;                    // [grid][V] when the overlay is not in LDS
  uint32_t* g_bm;                     // [grid][ceil(G / 32)] when the bitmap is not
};
// Where the per-workgroup structures live for a (V, G) and the grid that follows: the
// node -> entry overlay and the candidate bitmap in LDS when they fit their limits, else
// in global scratch of ovl_words / bm_words u32; a candidate list of cand_cap groups whose
// overflow falls back to a scan of the bitmap. No limit changes a result.
struct RoutesSweepLayout {
  uint32_t ovl_lds = 1, bm_lds = 1, cand_cap = 0, lds_bytes = 0, grid = 1;
  size_t ovl_words = 0, bm_words = 0;
};
RoutesSweepLayout whatif_routes_layout(uint32_t V, uint32_t G, size_t units, int num_cus);
hipError_t launch_whatif_routes(const RoutesSweep& p, const RoutesSweepLayout& l, bool emit, hipStream_t s);

// Boundary between routes_reduce's lane-per-group and wave-per-group kernels (16;
// OPENR_SPF_ROUTES_SMALL_MAX moves it for the tests). The LFA pass splits at the same size.
uint32_t routes_small_max();

// Loop-free alternates over prefix groups (spf_lfa.hip): the LFA half of
// getNextHopsWithMetric (Decision.cpp:1169-1204) on solved rows; the rule is in that file's
// header and at openr_spf_lfa_routes.
// launch_lfa_rows: the rows a batch of n sources needs besides the sources' own are the up
// neighbours that are no source: list[0 .. wptr[ceil(V / 32)]) (device count, nodes
// ascending) and rowidx[v] = the distance row of every needed node v (a source: its
// position in the batch; else n + its rank in list). need / srcbm / cnt hold ceil(V / 32)
// u32, wptr one more u64, tsum one u64 per 4096 words, list and rowidx V u32.
hipError_t launch_lfa_rows(const DevGraph& g, const uint32_t* sources, uint32_t n, uint32_t* need, uint32_t* srcbm,
                           uint32_t* cnt, unsigned long long* tsum, unsigned long long* wptr, uint32_t* list,
                           uint32_t* rowidx, int num_cus, hipStream_t s);
// The neighbour table ([E] each, a source's row at the CSR offset of its edges): entry b of
// source s = (distance row of its b-th distinct neighbour n or 0xFFFFFFFF when no link s-n
// is up, toMe = dist_n(s), dist_s(n)). dist holds the rows rowidx addresses, row i = source i.
hipError_t launch_lfa_table(const DevGraph& g, const uint32_t* sources, uint32_t n, const uint32_t* rowidx,
                            const uint64_t* dist, uint32_t* trow, unsigned long long* ttome,
                            unsigned long long* tfrom, int num_cus, hipStream_t s);
// The pass over units u = i * G + k (source i, group k). Count pass: alt [n][G][onb]
// (nullable) and nalt [n][G] = popcount(alt) (nullable). Emit pass: (onbr, ometric) of every
// set bit from optr[u] on, bits ascending, nothing at or past optr[u + 1]. metric / nh are
// the routes routes_reduce wrote for the same rows (nh with onb bytes per route; read by the
// emit pass only), large / n_large the scratch it left (routes_reduce_scratch_words).
struct LfaPass {
  uint32_t n, V, G, M, onb;
  uint32_t small_max, slice;  // set by the launcher (routes_small_max, lfa_slice)
  const uint32_t* sources;
  const uint2* row2;
  const uint32_t* gptr;
  const uint32_t* gnodes;
  const unsigned long long* dist;
  const uint32_t* trow;
  const unsigned long long* ttome;
  const unsigned long long* tfrom;
  const unsigned long long* metric;
  const uint8_t* nh;
  uint8_t* alt;
  uint32_t* nalt;
  const unsigned long long* optr;
  uint32_t* onbr;
  unsigned long long* ometric;
  const uint32_t* large;
  const uint32_t* n_large;
};
uint32_t lfa_slice();  // neighbours staged in LDS at a time (256; OPENR_SPF_LFA_SLICE)
hipError_t launch_lfa_reduce(const LfaPass& p, bool emit, int num_cus, hipStream_t s);
// ptr[0 .. n) += carry (a chunk's scanned counts moved behind the chunks before it)
hipError_t launch_lfa_ptr_shift(unsigned long long* ptr, size_t n, unsigned long long carry, int num_cus,
                                hipStream_t s);

// Post-failure loop-free alternates (spf_wlfa.hip): the LFA entry (metric, nh, alt) of every
// (failure set i, source j, group k) where it differs from the no-failure entry, from the
// node deltas of a link-set sweep over sets x rows (rows = the sources, then their up
// neighbours that are no source: launch_lfa_rows; unit i * n_rows + row). The rule is in that
// file's header and at openr_spf_whatif_lfa.
struct WlfaPass {
  uint32_t V, G, M, n_src, n_rows, n_sets, n_set_links, nb, onb;
  const uint32_t* set_ptr;
  const uint32_t* set_links;
  const uint32_t* sources;
  const uint2* row2;
  const uint32_t* adj;
  const uint32_t* lid;
  const uint16_t* nbr;
  const uint32_t* rowidx;
  const uint32_t* gptr;
  const uint32_t* gnodes;
  const unsigned long long* iptr;
  const uint32_t* inv;
  const uint32_t* nchanged;           // [n_sets * n_rows] the sweep's changed-node counts
  const unsigned long long* nptr;     // node delta CSR over the sweep's units
  const uint32_t* nnode;
  const unsigned long long* ndist;
  const uint8_t* nnh;                 // [.][nb]
  const unsigned long long* bdist;    // base rows [n_rows][V]
  const uint8_t* bnh;                 // [n_rows][V][nb] (read for the sources only)
  const uint32_t* trow;               // base neighbour table (launch_lfa_table)
  const unsigned long long* ttome;
  const unsigned long long* bmetric;  // base entries [n_src][G]
  const uint8_t* bmnh;                // [n_src][G][nb]
  const uint8_t* balt;                // [n_src][G][nb]
  uint32_t* bunprot;                  // [n_src] base unprotected count (written by the mark launch)
  uint32_t* alist;                    // [units] affected units, *acount of them
  uint32_t* acount;
  uint32_t* changed;                  // [units]
  uint32_t* unprot;                   // [units], nullable
  uint32_t* lost;                     // [units], nullable
  const unsigned long long* optr;     // emit pass: [units + 1]
  uint32_t* ogroup;
  unsigned long long* ometric;
  uint8_t* onh;                       // [.][onb], zero past nb
  uint8_t* oalt;                      // [.][onb], zero past nb
  uint32_t hash_slots, hash_shift, cand_cap, bm_lds, slots;  // WlfaLayout (set by the launcher)
  uint32_t* g_bm;                     // [grid][ceil(G / 32)] when the bitmap is not in LDS
};
// Per-workgroup structures and the grid: hash slots (0: lookups scan the delta slices), the
// candidate list, whether the candidate bitmap is in LDS (else bm_words u32 of global
// scratch), the neighbour slots staged at a time. No limit changes a result.
struct WlfaLayout {
  uint32_t hash_slots = 0, hash_shift = 0, cand_cap = 0, bm_lds = 1, slots = 8, lds_bytes = 0, grid = 1;
  size_t bm_words = 0;
};
WlfaLayout whatif_lfa_layout(uint32_t G, size_t units, int num_cus);
// bunprot, then per unit changed = 0, lost = 0, unprot = bunprot[j], and the affected list
hipError_t launch_wlfa_mark(const WlfaPass& p, int num_cus, hipStream_t s);
// Count pass: changed / unprot / lost of every listed unit. Emit pass: its entries at
// optr[u] + rank in the pass (any order inside a unit), nothing at or past optr[u + 1].
hipError_t launch_wlfa(const WlfaPass& p, const WlfaLayout& l, bool emit, hipStream_t s);

// Event what-if sweeps (spf_repair.h): what the drain, the metric and the restore pass share. Unit
// u = i * n_src + j applies event i for sources[j].
struct RepairPass {
  uint32_t n_events, n_src, nb;
  const uint32_t* sources;
  const uint64_t* base_dist;   // base rows [n_src][V] (whatif_base_solve)
  const uint8_t* base_nh;      // [n_src][V][nb]
  const uint64_t* base_tight;  // [n_src][ceil(E / 64)]
  const uint16_t* base_tin;    // nullable [n_src][V] tight in-degrees (rounds plan)
  uint32_t* changed;           // [units]
  uint32_t* wunit;             // [units] affected units
  uint32_t* ovf_unit;          // [units] units that outgrew the narrow launch's slots
  uint32_t* wcount;            // [2] affected units, overflowed units
  uint32_t* ctr;               // 2 work counters (zero at rest)
  WhatifDelta delta;           // node == null: counts only
};

// Drain what-if sweep (spf_drain.hip): unit u = i * n_src + j overloads the nodes of event i
// (nodes[node_ptr[i], node_ptr[i + 1])) and takes its links (links[link_ptr[i], ..), null
// link_ptr: none) out of service for sources[j]; the rule is in that file's header and at
// openr_spf_whatif_drain. Slices are clamped to n_nodes / n_links entries and ids out of
// range are skipped (a malformed device CSR reads nothing past the arrays).
struct DrainPass : RepairPass {
  uint32_t n_nodes, n_links, unit_cost;
  const uint32_t* node_ptr;
  const uint32_t* nodes;
  const uint32_t* link_ptr;
  const uint32_t* links;
};
constexpr uint32_t kDrainCtr = kExactCtr + 2;
constexpr uint32_t kDrainSlots = 128;      // dirty-node slots of the narrow launch (OPENR_SPF_DRAIN_SLOTS)
constexpr uint32_t kDrainBlock = 64;       // threads per unit, narrow launch
constexpr uint32_t kDrainBlockWide = 256;  // ... and the re-run with a slot per node
uint32_t drain_slots();
// LDS of a unit with S slots; 0 when it does not fit kMaxLds (or S outgrows the u16 index)
uint32_t drain_lds_bytes(uint32_t V, uint32_t L, uint32_t S, uint32_t nb);
// changed[u] = 0 for every unit; the units with a removed base-tight edge are appended
// source-major to wunit, wcount[0] of them; wcount[1] = 0.
hipError_t launch_drain_filter(const DevGraph& g, const DrainPass& p, int num_cus, hipStream_t s);
// Repairs wunit[0, count): changed[] and the delta of every listed unit; units past the
// slots are appended to ovf_unit (wcount[1]). rerun: repairs ovf_unit[0, count) with a slot
// per node instead (nothing overflows).
hipError_t launch_drain_repair(const DevGraph& g, const DrainPass& p, uint32_t count, bool rerun, int num_cus,
                               hipStream_t s);

// Metric what-if sweep (spf_metric.hip): unit u = i * n_src + j raises the metrics of event
// i's directed edges (edges[edge_ptr[i], edge_ptr[i + 1]), ids ascending, metrics[k] the new
// metric of edges[k]) for sources[j]; the rule is in that file's header and at
// openr_spf_whatif_metric. Slices are clamped to n_edges entries; an entry whose id is out
// of range, whose edge is down or whose metric is not in (current, 2^31 - 1] is skipped.
struct MetricPass : RepairPass {
  uint32_t n_edges;
  const uint32_t* edge_ptr;
  const uint32_t* edges;
  const uint32_t* metrics;
};
constexpr uint32_t kMetricCtr = kDrainCtr + 2;
constexpr uint32_t kRestoreCtr = kMetricCtr + 2;
constexpr uint32_t kMaintCtr = kRestoreCtr + 2;
constexpr uint32_t kWorkWords = kMaintCtr + 2;  // the counter buffer: the class blocks, then one pair per sweep kernel
static_assert(kDrainCtr + 2 == kWorkSlots, "the metric sweep's counters follow the last class block");
constexpr uint32_t kMetricSlots = 256;      // dirty-node slots of the narrow launch (OPENR_SPF_METRIC_SLOTS)
constexpr uint32_t kMetricBlock = 64;       // threads per unit, narrow launch
constexpr uint32_t kMetricBlockWide = 256;  // ... and the re-run with a slot per node
uint32_t metric_slots();
// As drain_lds_bytes, with E bits for the raised edges in place of the node and link bitmaps.
uint32_t metric_lds_bytes(uint32_t V, uint32_t E, uint32_t S, uint32_t nb);
// The launchers as the drain's; the filter lists the units with a raised base-tight edge.
hipError_t launch_metric_filter(const DevGraph& g, const MetricPass& p, int num_cus, hipStream_t s);
hipError_t launch_metric_repair(const DevGraph& g, const MetricPass& p, uint32_t count, bool rerun, int num_cus,
                                hipStream_t s);

// Restore what-if sweep (spf_restore.hip): unit u = i * n_src + j clears the overload bit of
// event i's nodes, puts its links back in service and lowers the metrics of its directed edges
// (three CSRs as the drain's and the metric pass's; null link_ptr / edge_ptr: none) for
// sources[j]; the rule is in that file's header and at openr_spf_whatif_restore. Slices are
// clamped to n_nodes / n_links / n_edges entries; an id out of range, a node that is not
// overloaded, a link that is up or whose restored edges would carry a metric outside
// [1, 2^31 - 1], and an entry whose metric is not in [1, current) are skipped.
struct RestorePass : RepairPass {
  uint32_t n_nodes, n_links, n_edges, unit_cost;
  const uint32_t* node_ptr;
  const uint32_t* nodes;
  const uint32_t* link_ptr;
  const uint32_t* links;
  const uint32_t* edge_ptr;
  const uint32_t* edges;
  const uint32_t* metrics;
};
constexpr uint32_t kRestoreSlots = 256;      // dirty-node slots of the narrow launch (OPENR_SPF_RESTORE_SLOTS)
constexpr uint32_t kRestoreBlock = 64;       // threads per unit, narrow launch
constexpr uint32_t kRestoreBlockWide = 256;  // ... and the re-run with a slot per node
uint32_t restore_slots();
// As drain_lds_bytes, with V bits for the undrained nodes, L for the links and E for the lowered edges.
uint32_t restore_lds_bytes(uint32_t V, uint32_t L, uint32_t E, uint32_t S, uint32_t nb);
// The launchers as the drain's; the filter lists the units with an improved edge that reaches
// its head at or below the head's base distance.
hipError_t launch_restore_filter(const DevGraph& g, const RestorePass& p, int num_cus, hipStream_t s);
hipError_t launch_restore_repair(const DevGraph& g, const RestorePass& p, uint32_t count, bool rerun, int num_cus,
                                 hipStream_t s);

// Maintenance what-if sweep (spf_maint.hip): unit u = i * n_src + j overloads event i's nodes,
// takes its links out of service and raises the metrics of its directed edges (three CSRs as
// the drain's and the metric pass's; null link_ptr / edge_ptr: none) for sources[j]; the rule
// is in that file's header and at openr_spf_whatif_maint. Slices are clamped to n_nodes /
// n_links / n_edges entries; an id out of range, an unused link, an entry whose edge is down
// or whose metric is not in (current, 2^31 - 1] are skipped. unit_cost: the entries are ignored.
struct MaintPass : RepairPass {
  uint32_t n_nodes, n_links, n_edges, unit_cost;
  const uint32_t* node_ptr;
  const uint32_t* nodes;
  const uint32_t* link_ptr;
  const uint32_t* links;
  const uint32_t* edge_ptr;
  const uint32_t* edges;
  const uint32_t* metrics;
};
constexpr uint32_t kMaintSlots = 256;      // dirty-node slots of the narrow launch (OPENR_SPF_MAINT_SLOTS)
constexpr uint32_t kMaintBlock = 64;       // threads per unit, narrow launch
constexpr uint32_t kMaintBlockWide = 256;  // ... and the re-run with a slot per node
uint32_t maint_slots();
// As drain_lds_bytes, with V bits for the drained nodes, L for the links and E for the raised edges.
uint32_t maint_lds_bytes(uint32_t V, uint32_t L, uint32_t E, uint32_t S, uint32_t nb);
// The launchers as the drain's; the filter lists the units with a removed or raised base-tight edge.
hipError_t launch_maint_filter(const DevGraph& g, const MaintPass& p, int num_cus, hipStream_t s);
hipError_t launch_maint_repair(const DevGraph& g, const MaintPass& p, uint32_t count, bool rerun, int num_cus,
                               hipStream_t s);

// Loop-free alternates under drain, metric, restore and maintenance events (spf_elfa.hip): the pass of
// spf_wlfa.hip over the node deltas of an event sweep (events x closure rows). The rule is in
// that file's header and at openr_spf_whatif_drain_lfa.
//   w    the pass as spf_wlfa.hip reads it; n_sets = events, set_ptr / set_links = the links
//        K_i of a drain or restore event (set_ptr null: none), trow / ttome the table of the
//        neighbours *with a closure row* (restore: every neighbour, launch_elfa_table; else
//        the base table)
//   ev   restore only: the event CSRs as the restore sweep takes them (and unit_cost)
//   idle the hop-count form of a metric sweep: nothing moves, the mark pass lists no unit
// kElfaMaint (openr_spf_whatif_maint_lfa): the node sweep is the maintenance sweep, the pass is
// the drain's. The LFA loop never reads the metric of a link s-n, so a raise changes no tested
// status and acts through the rows of the sweep alone; N_i and K_i act as in a drain event.
enum ElfaFamily : int { kElfaDrain = 0, kElfaMetric = 1, kElfaRestore = 2, kElfaMaint = 3 };
struct ElfaPass {
  WlfaPass w;
  RestorePass ev;
  uint32_t idle;
};
// The closure of a restore pass: the sources, then every distinct neighbour of a source that
// is no source, whatever the state of the links between them (a neighbour behind a down link
// can become tested). Outputs and scratch as launch_lfa_rows.
hipError_t launch_elfa_rows(const DevGraph& g, const uint32_t* sources, uint32_t n, uint32_t* need, uint32_t* srcbm,
                            uint32_t* cnt, unsigned long long* tsum, unsigned long long* wptr, uint32_t* list,
                            uint32_t* rowidx, int num_cus, hipStream_t s);
// launch_lfa_table over every edge, down ones included: entry b of source s = (distance row
// of its b-th distinct neighbour n, base toMe = dist_n(s), UINT64_MAX where n does not reach s).
hipError_t launch_elfa_table(const DevGraph& g, const uint32_t* sources, uint32_t n, const uint32_t* rowidx,
                             const uint64_t* dist, uint32_t* trow, unsigned long long* ttome, int num_cus,
                             hipStream_t s);
// As launch_wlfa_mark / launch_wlfa for events of family `fam`.
hipError_t launch_elfa_mark(const DevGraph& g, const ElfaPass& p, int fam, int num_cus, hipStream_t s);
hipError_t launch_elfa(const DevGraph& g, const ElfaPass& p, const WlfaLayout& l, int fam, bool emit, hipStream_t s);

// Incremental mirror updates (spf_update.hip).
// In-place attribute patch of the device mirror: each record overwrites one element of
// one DevGraph array (structure — rows, columns, link ids — never changes).
enum PatchArray : uint32_t {
  kPatchAdj = 0, kPatchW, kPatchWin, kPatchErec, kPatchEllt, kPatchRow2t, kPatchOvl, kPatchOvlBits, kPatchEllv,
  kPatchW64,  // val.x = low, val.y = high word
  kPatchElld,
  kPatchErecS,  // DevGraph::erecs (idx = sorted position)
  kNumPatchArrays
};
struct PatchRec {
  uint32_t arr, idx, pad0, pad1;
  uint4 val;  // x (u32 / u8 arrays), xy (uint2), xyzw (uint4)
};
hipError_t launch_patch_apply(const DevGraph& g, const PatchRec* recs, uint32_t n, hipStream_t s);
// One directed edge u->v whose usability / weight / tail overload changed in a patch.
struct DeltaEdge {
  uint32_t u, v, w0, w1;  // weight before / after (u32; usable metrics are i32-positive)
  uint32_t flags, pad0, pad1, pad2;
};
constexpr uint32_t kDeltaUp0 = 1u, kDeltaUp1 = 2u, kDeltaOvl0 = 4u, kDeltaOvl1 = 8u;
// Refresh filter: row i (source sources[i], distances dist[i][V] of the graph before the
// patch) is affected iff some delta edge was tight for it or may now be tight / shorter;
// affected rows are appended to alist (row index) / asrc (source), *count of them.
hipError_t launch_refresh_filter(const DeltaEdge* delta, uint32_t n_delta, const uint32_t* sources, uint32_t n,
                                 uint32_t V, const uint64_t* dist, bool unit_cost, uint32_t* alist, uint32_t* asrc,
                                 uint32_t* count, int num_cus, hipStream_t s);
// Exact second stage: of the *count_in rows the filter listed, those whose dist or next-hop
// rows the change really moves (needs the next-hop rows; nb <= 32); n_max bounds *count_in.
hipError_t launch_refresh_exact(const DevGraph& g, const DeltaEdge* delta, uint32_t n_delta, uint32_t V,
                                const uint64_t* dist, const uint8_t* nh, uint32_t nb, bool unit_cost,
                                const uint32_t* alist_in, const uint32_t* asrc_in, const uint32_t* count_in,
                                uint32_t n_max, uint32_t* alist, uint32_t* asrc, uint32_t* count, int num_cus,
                                hipStream_t s);
// rows[alist[k]][0 .. words) = 0 for k < n
hipError_t launch_zero_rows(uint64_t* rows, uint32_t words, const uint32_t* alist, uint32_t n, int num_cus,
                            hipStream_t s);

// KSP2 tracing (spf_ksp.hip), one wavefront per (src, dest) pair of a chunk.
constexpr uint32_t kKspMaxDepth = 256;  // DFS frames (hops of a traced shortest path)
constexpr uint32_t kKspArena = 1024;    // sorted pathLinks of the frames on the DFS stack
struct KspCaps {
  uint32_t frames, arena;
};
KspCaps ksp_caps(const DevGraph& g, bool full);  // small tier (occupancy) or full tier
// kind 1 writes the k = 1 links to ign_io[k * ign_cap, ign_end[k]); kind 2 ignores them.
// Small tier: retry_list != null; pairs that outgrow it are appended there (count in
// *retry_count). Full tier: retry_list == null; with `list` it traces only the chunk-local
// pairs list[0 .. *list_count).
hipError_t launch_ksp_trace(int kind, const DevGraph& g, const uint32_t* sources, const uint32_t* prow,
                            const uint32_t* pdst, uint32_t first, uint32_t n, const uint64_t* rows, uint32_t* ign_io,
                            uint32_t* ign_end, uint32_t ign_cap, uint32_t* tok, uint32_t tok_cap, uint32_t* status,
                            uint32_t* qbuf, int num_cus, hipStream_t s, unsigned long long* stats = nullptr,
                            const uint32_t* list = nullptr, const uint32_t* list_count = nullptr,
                            uint32_t* retry_list = nullptr, uint32_t* retry_count = nullptr,
                            uint32_t* work_ctr = nullptr,  // zeroed dynamic-scheduling counter (required)
                            const uint16_t* rows16 = nullptr,  // kind 2: u16 level rows (SolveArgs::lvl16)
                            uint64_t lcost = 0,   // instead of `rows`: dist = level * lcost; non-zero lcost
                                                  // also marks a uniform-cost graph (rank by name / edge)
                            uint32_t ltag = 0,    // rows16 tagged (SolveArgs::lvl_tag): tag << 8 | lvl_shift
                            // uniform cost: the sources' pathLinks lists (launch_ksp_path_lists), row
                            // prow[pair] of each. Kind 1 reads them instead of gathering from the records
                            // and rows; kind 2 reads them for the nodes its pair's row leaves at their
                            // base distance (tl_rows: the base rows the lists were built from)
                            const uint32_t* tl_off = nullptr, const uint2* tl_ent = nullptr,
                            const uint64_t* tl_rows = nullptr,
                            // kind 2: rows16 from launch_ksp_repair where rmode[k] == 0 (base fallback)
                            const uint32_t* rmode = nullptr);
// KSP2 second SPF as a repair of the base SPF (uniform cost `cost`): for chunk-local pair k
// (list[0 .. *list_count) when list is set), source srcs[k] of base row prow[k] (base_rows,
// pathLinks list offsets tl_off: launch_ksp_path_lists), dest tgts[k], ignoring
// ign_links[ign_ptr[k], ign_end[k]): rows16[k][v] = ltag | level for the nodes whose
// distance the ignored links change (lmask: unreached or at / beyond dest's level); every
// other node keeps its base distance (the k = 2 trace's `repaired` mode reads it there).
// Requires levels < lmask. A pair whose affected set outgrows a cap gets mode[k] = 1 and
// is appended to retry_list (*retry_count) for the forward solve; else mode[k] = 0.
// work_ctr: zeroed dynamic-scheduling counter.
uint32_t ksp_repair_lds_bytes(uint32_t V, uint32_t L);  // 0: the graph does not fit
hipError_t launch_ksp_repair(const DevGraph& g, const uint32_t* srcs, const uint32_t* prow, const uint32_t* tgts,
                             const uint32_t* list, const uint32_t* list_count, uint32_t n, const uint32_t* ign_ptr,
                             const uint32_t* ign_end, const uint32_t* ign_links, const uint64_t* base_rows,
                             const uint32_t* tl_off, uint64_t cost, uint16_t* rows16, uint32_t ltag, uint32_t lmask,
                             uint32_t* mode, uint32_t* retry_list, uint32_t* retry_count, uint32_t* work_ctr,
                             int num_cus, hipStream_t s);
// OPENR_SPF_PROF only: after launch_ksp_repair, out[0] += the listed pairs it kept (mode 0),
// out[1] += those it handed to the forward solve (mode 1)
hipError_t launch_ksp_repair_count(const uint32_t* mode, const uint32_t* list, const uint32_t* list_count, uint32_t n,
                                   unsigned long long* out, int num_cus, hipStream_t s);
// The k = 1 trace's pathLinks lists: for base row j (source sources[j], distances rows[j]),
// off[j][0 .. V] (V + 1 u32) and ent[j][off[v] .. off[v + 1]) = node v's tight in-edges in
// rank order as {u->v edge, link | u << 16} (ent holds E entries per source). Needs
// DevGraph::erecs and ids below 2^16 (ksp_path_lists_ok; OPENR_SPF_KSP_TL=0 turns it off).
bool ksp_path_lists_ok(const DevGraph& g);
hipError_t launch_ksp_path_lists(const DevGraph& g, const uint32_t* sources, uint32_t n_src, const uint64_t* rows,
                                 uint32_t* off, uint2* ent, int num_cus, hipStream_t s);
uint32_t ksp_stats_count();  // counters a stats buffer holds (OPENR_SPF_PROF tuning only)
uint32_t ksp_max_grid(const DevGraph& g, int num_cus);  // qbuf must hold ksp_max_grid * (V + ceil(V / 32)) u32
hipError_t launch_strided_iota(uint32_t* p, uint32_t n, uint32_t stride, int num_cus, hipStream_t s);
hipError_t launch_gather_sources(const uint32_t* sources, const uint32_t* prow, uint32_t first, uint32_t n,
                                 uint32_t* out, int num_cus, hipStream_t s);
// After the k = 1 trace of a chunk: pairs whose k = 2 answer is empty by construction get
// n_paths = 0 in tok2; the others are listed (chunk-local k, list[0 .. *count), count
// zeroed by the caller) for the second SPF and the k = 2 trace. Also writes out_src[k] =
// the pair's source for every k (launch_gather_sources).
hipError_t launch_ksp_select_pairs(const DevGraph& g, const uint32_t* sources, const uint32_t* prow,
                                   const uint32_t* pdst, uint32_t first, uint32_t n, const uint32_t* tok1,
                                   uint32_t* tok2, uint32_t tok_cap, uint32_t* out_src, uint32_t* list,
                                   uint32_t* count, int num_cus, hipStream_t s);
uint32_t ksp_lds_bytes(uint32_t V, uint32_t L, uint32_t max_deg);

// Exact-order kernel (spf_exact.hip): LinkState::runSpf's heap process replayed per solve
// (one wavefront per solve) for graphs outside the fast kernels' domain — zero or
// wrapped-negative metrics, graphs too large for their LDS layouts, next-hop sets wider
// than 256. State in LDS when a slot fits (<= kMaxLds), else in `scratch` (slot bytes each).
// tight = the edges left in pathLinks; a.order (nullable) = pop index per node.
uint64_t exact_slot_bytes(uint32_t V, uint32_t E, uint32_t L, uint32_t nh_bits);
hipError_t launch_exact(const DevGraph& g, const SolveArgs& a, const uint64_t* w64, bool use_metric, uint32_t nh_bits,
                        uint8_t* scratch, uint64_t scratch_bytes, uint32_t* order_out, uint32_t* ctr, int num_cus,
                        hipStream_t s);

// LDS footprint of each kernel for a graph (0 if it cannot fit one workgroup per CU).
uint32_t bfs_lds_bytes(int family, uint32_t V, uint32_t L, bool has_ignore, int cls);
uint32_t bfs_code_lds_bytes(uint32_t V, uint32_t L, bool has_ignore, int cls);
uint32_t bfs_lvl_lds_bytes(uint32_t V, uint32_t L, bool has_ignore, int cls);

uint32_t fringe_lds_bytes(uint32_t V, uint32_t L, bool has_ignore, int nh_mode, bool dist64);
constexpr uint32_t kMaxLds = 160 * 1024;

// OPENR_SPF_PROF=1 (tuning only): the kernels' profiling counters (BFS level loops, the
// what-if repair phases, the KSP2 trace kinds) printed to stderr after each launch
inline bool prof_enabled() {
  const char* e = std::getenv("OPENR_SPF_PROF");
  return e && e[0] == '1';
}

}  // namespace openr_spf
