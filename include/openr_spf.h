/*
 * openr_spf.h — C-ABI of the MI355X-native SPF engine for OpenR's Decision module.
 *
 * This is the drop-in boundary under openr::LinkState. Each entry point names
 * the reference interface it replaces:
 *
 *   openr_spf_set_graph        LinkState topology mirror; call wherever the reference
 *                              clears its SPF memo: updateAdjacencyDatabase
 *                              (LinkState.cpp:714-717), deleteAdjacencyDatabase
 *                              (:730-731), decrementHolds (:509-512)
 *   openr_spf_solve            LinkState::runSpf(src, useLinkMetric)  (LinkState.cpp:808-882,
 *                              LinkState.h:436-443), batched over sources; the memoized
 *                              LinkState::getSpfResult (LinkState.cpp:793-803) and the
 *                              per-neighbour LFA solves of SpfSolver::getNextHopsWithMetric
 *                              (Decision.cpp:1170-1204) are batches of this call
 *   openr_spf_solve_ignore     LinkState::runSpf(src, true, linksToIgnore) as used by
 *                              getKthPaths k>=2 (LinkState.cpp:769-779) and per-link-failure
 *                              what-if sweeps; one (source, ignore-set) pair per solve
 *   openr_spf_solve_device     the same on device-resident buffers and a caller stream
 *                              (batched prefetch / benchmarks / multi-GPU shards)
 *   openr_spf_whatif           per-link-failure what-if sweep: runSpf(src, useLinkMetric, {link})
 *                              for every (link, source), reduced to changed-node counts
 *   openr_spf_whatif_delta     the same sweep plus each unit's changed nodes with their
 *                              new distance and next-hop bits
 *   openr_spf_whatif_sets      the sweep with a set of links per unit (node failures,
 *                              shared-risk link groups); _sets_delta adds the delta
 *   openr_spf_routes           SpfSolver::getMinCostNodes + the shortest-path half of
 *                              getNextHopsWithMetric (Decision.cpp:1094-1167) over prefix
 *                              groups, for a batch of sources
 *   openr_spf_lfa_routes       the other half of getNextHopsWithMetric: loop-free alternates
 *                              (RFC 5286, Decision.cpp:1169-1204) of every (source, prefix
 *                              group), from the rows of the sources and their neighbours
 *   openr_spf_whatif_routes    the link-set sweep resolved to routes: per (failure set,
 *                              source) the groups whose route changed, with the new route
 *   openr_spf_whatif_lfa       the same sweep resolved to LFA RIB entries: per (failure set,
 *                              source) the groups whose route or alternates changed, and
 *                              how many are left with a single next hop
 *   openr_spf_ksp2             LinkState::getKthPaths(src, dst, 1 and 2) (LinkState.cpp:762-791)
 *                              for a batch of pairs, paths traced on the device
 *   openr_spf_patch_graph      attribute-only mirror updates (metric, Link::isUp, node
 *                              overload) at the same memo-clearing points, without a rebuild
 *   openr_spf_refresh          incremental re-SPF of resident rows after a patch: only the
 *                              rows the change can touch are re-solved
 *   openr_spf_last_error       glog CHECK / exception text of the reference
 *
 * Conventions
 *   - All functions return 0 (OPENR_SPF_OK) or a negative errno-style code; no C++
 *     exception crosses the ABI. openr_spf_last_error() returns a thread-local message.
 *   - Host output buffers are caller-owned. Device memory is library-owned except in
 *     openr_spf_solve_device, where every pointer is device memory owned by the caller.
 *   - A context is single-threaded (one per LinkState, matching the reference's
 *     threading: everything in Decision runs on one event-base thread). Host-buffer calls
 *     are synchronous on return.
 *   - There is no CPU fallback: if the HIP runtime or a device is unavailable,
 *     openr_spf_create fails with OPENR_SPF_ENODEV.
 *
 * Semantics (bit-exact with LinkState::runSpf, any metric values)
 *   dist[s][v]   u64 shortest distance (NodeSpfResult::metric), UINT64_MAX if v is not
 *                in the SpfResult (unreachable). dist[s][src] = 0. (With wrapped metrics a
 *                reached node's sum can itself be UINT64_MAX: openr_spf_solve_order's
 *                order[] tells the two apart.)
 *   nh[s][v][b]  next-hop set of v as a bitset over the source's DISTINCT neighbours in
 *                CSR row order: bit i (byte i/8, bit i%8) <-> the i-th distinct `col`
 *                value of row src (openr_spf_neighbor_map). nh bits of src itself are 0.
 *   tight[s][w]  (OPENR_SPF_EMIT_TIGHT) bit e of the E-bit mask is set iff directed edge e
 *                u->v is in NodeSpfResult::pathLinks(v). For metrics in [1, 2^31-1] these
 *                are the tight in-edges: usable, dist[u]+w(e)==dist[v], u may expand
 *                (u==src or !node_overloaded[u]); pathLinks(v) orders them by
 *                (dist[u], name_rank[u]) then by position of e in row u. In general
 *                pathLinks(v) orders them by the pop index of u (openr_spf_solve_order)
 *                then by row position.
 *   A directed edge is usable iff edge_up[e] and link_id[e] is not in the solve's
 *   ignore set. Overloaded nodes other than the source are reached but never expanded.
 *   Usable metrics in [1, 2^31-1] (the positive i32 Adjacency.metric range) run on the
 *   fast kernels. Zero or wrapped-negative metrics (an i32 < 0 stored as u64, sums wrap
 *   mod 2^64 as in the reference) make the pop order history-dependent; those graphs,
 *   next-hop sets wider than 256 and graphs beyond the LDS-resident layouts run on the
 *   exact-order kernel, which replays the reference's heap process (slower, same
 *   results). openr_spf_ksp2 needs metrics in [1, 2^31-1] (OPENR_SPF_ENOTSUP otherwise).
 */
#ifndef OPENR_SPF_H
#define OPENR_SPF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OPENR_SPF_ABI_VERSION 1

enum {
  OPENR_SPF_OK = 0,
  OPENR_SPF_EIO = -5,       /* HIP runtime error */
  OPENR_SPF_ENOMEM = -12,   /* host or device allocation failed */
  OPENR_SPF_ENODEV = -19,   /* no usable GPU / HIP runtime */
  OPENR_SPF_EINVAL = -22,   /* bad argument (null, out of range, no graph set) */
  OPENR_SPF_E2BIG = -7,     /* graph too large for the engine (see openr_spf_limits) */
  OPENR_SPF_ENOTSUP = -95,  /* KSP2 on a graph with a metric outside [1, 2^31-1] */
};

enum {
  OPENR_SPF_USE_LINK_METRIC = 1u << 0, /* runSpf useLinkMetric; else every hop costs 1 */
  OPENR_SPF_EMIT_TIGHT = 1u << 1,      /* fill tight[] (pathLinks reconstruction)      */
  OPENR_SPF_EMIT_ORDER = 1u << 2,      /* exact-order kernel (openr_spf_solve_order)  */
  OPENR_SPF_EMIT_LEVELS8 = 1u << 3,    /* solve_device: u8 level rows in d_dist (below) */
  OPENR_SPF_EMIT_LEVELS16 = 1u << 4,   /* solve_device: u16 level rows in d_dist        */
};

/* Sticky device-side conditions (openr_spf_take_status) */
enum {
  OPENR_SPF_STATUS_LEVEL_OVERFLOW = 1u, /* an EMIT_LEVELS8 row held a finite level > 254 (written 0xFE) */
};

typedef struct openr_spf_ctx openr_spf_ctx;

/* CSR mirror of LinkState::linkMap_ (LinkState.h:456-467). Row u lists u's
   directed edges in LinkState::linksFromNode(u) iteration order. Every link id
   appears exactly twice (u->v and v->u). Arrays are copied by set_graph. */
typedef struct {
  uint32_t num_nodes;               /* V */
  uint32_t num_dir_edges;           /* E */
  uint32_t num_links;               /* L: link ids are in [0, L) */
  const uint32_t* row_ptr;          /* [V+1] */
  const uint32_t* col;              /* [E] neighbour node id */
  const uint64_t* metric;           /* [E] Link::getMetricFromNode(u) (hold-aware value()) */
  const uint32_t* link_id;          /* [E] undirected link id */
  const uint8_t* edge_up;           /* [E] Link::isUp() */
  const uint8_t* node_overloaded;   /* [V] LinkState::isNodeOverloaded() */
  const uint32_t* name_rank;        /* [V] rank of the node name under std::string < */
} openr_spf_graph;

typedef struct {
  uint32_t max_nodes;       /* largest V the engine accepts */
  uint32_t max_nh_bits;     /* largest distinct degree (next-hop bitset width) */
} openr_spf_limits_t;

typedef struct {
  uint64_t spf_runs;        /* logical SPFs solved (fb303 decision.spf_runs) */
  uint64_t batches;         /* solve calls */
  double last_batch_ms;     /* wall time of the last host-buffer solve (decision.spf_ms) */
  double last_kernel_ms;    /* device time of the last solve's kernels (what-if sweep: its
                               repair kernel alone, HIP events around that launch) */
} openr_spf_stats_t;

int openr_spf_abi_version(void);
/* "<sha256/16 of the engine sources> <source files>" (Makefile build_id): lets the host
   verify the library was built from the sources it ships with. */
const char* openr_spf_build_id(void);
const char* openr_spf_last_error(void);
/* Diagnostics: "name;name;..." of the kernels the calling thread's last solve call
   (openr_spf_solve*, _solve_device) enqueued, re-run launches included (tests assert
   which kernel a configuration runs); every what-if, routes, LFA and KSP2 call starts a new
   trace too. The general-metric kernels and the link what-if repairs also note their
   distance type: "fringe_kernel<u64>" / "rounds_kernel<u32>" after the plain name,
   "whatif_group<u16|u32|u64[,lds]>" (",lds": graph staged in LDS), "whatif_incr<u32|u64>". */
const char* openr_spf_last_kernels(void);
void openr_spf_limits(openr_spf_limits_t* out);

/* device_ids: n_devices HIP ordinals (NULL -> the current device). Sources of one
   solve call are split in contiguous blocks across the devices. */
int openr_spf_create(const int* device_ids, int n_devices, openr_spf_ctx** out);
void openr_spf_destroy(openr_spf_ctx* ctx);

int openr_spf_set_graph(openr_spf_ctx* ctx, const openr_spf_graph* graph);

/* Minimum nh_bytes for the current graph: ceil(max distinct degree / 8), >= 1. */
int openr_spf_nh_bytes(const openr_spf_ctx* ctx, uint32_t* out_nh_bytes);

/* Distinct neighbours of src in row order (next-hop bit i -> out_nbrs[i]). */
int openr_spf_neighbor_map(const openr_spf_ctx* ctx, uint32_t src, uint32_t* out_nbrs,
                           uint32_t capacity, uint32_t* out_count);

/* Batched SPF from sources[0..n): dist [n][V]; nh [n][V][nh_bytes] (nh_bytes >=
   openr_spf_nh_bytes, or nh == NULL); tight [n][ceil(E/64)] or NULL. */
int openr_spf_solve(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n,
                    uint32_t flags, uint64_t* dist, uint8_t* nh, uint32_t nh_bytes,
                    uint64_t* tight);

/* As openr_spf_solve_ignore (ignore_ptr may be NULL: no ignore sets), plus order [n][V]:
   the index at which runSpf popped v from its queue (0 = the source), UINT32_MAX if v is
   not in the SpfResult. Always runs the exact-order kernel; pathLinks(v) = the tight[]
   in-edges of v sorted by order[u], then by row position (what LinkState needs when
   metrics can be zero). */
int openr_spf_solve_order(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n,
                          uint32_t flags, const uint32_t* ignore_ptr,
                          const uint32_t* ignore_links, uint64_t* dist, uint8_t* nh,
                          uint32_t nh_bytes, uint64_t* tight, uint32_t* order);

/* As openr_spf_solve with a per-solve ignore set: solve i ignores the links
   ignore_links[ignore_ptr[i] .. ignore_ptr[i+1]) (ignore_ptr has n+1 entries). */
int openr_spf_solve_ignore(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n,
                           uint32_t flags, const uint32_t* ignore_ptr,
                           const uint32_t* ignore_links, uint64_t* dist, uint8_t* nh,
                           uint32_t nh_bytes, uint64_t* tight);

/* Device-buffer form on device `device_index` of the context (an index into the
   device_ids given to create). All pointers are device memory; d_ignore_ptr may be
   NULL (no ignore sets); d_nh / d_tight may be NULL. `stream` is a hipStream_t
   (NULL = the context's own stream). Asynchronous: returns after enqueueing. */
/* With OPENR_SPF_EMIT_LEVELS8 / 16 the distance rows are written in level form instead:
   d_dist points to [n][V] u8 / u16 levels (level = dist / cost; all ones = not in the
   SpfResult) — the compact rows a strong-scaling rank all-gathers, 1 or 2 bytes per node
   instead of 8, emitted by the solve itself. Only for graphs on which every usable edge
   costs the same (or useLinkMetric off) and that run on the level BFS family (uniform-cost
   rows of <= 4 ELL slots, grids), with no ignore sets and no tight output: otherwise
   OPENR_SPF_ENOTSUP. A finite level above 254 in a u8 row is written as 0xFE and sets
   OPENR_SPF_STATUS_LEVEL_OVERFLOW (openr_spf_take_status): use u16 rows for such graphs. */
int openr_spf_solve_device(openr_spf_ctx* ctx, int device_index,
                           const uint32_t* d_sources, uint32_t n, uint32_t flags,
                           const uint32_t* d_ignore_ptr, const uint32_t* d_ignore_links,
                           uint64_t* d_dist, uint8_t* d_nh, uint32_t nh_bytes,
                           uint64_t* d_tight, void* stream);

/* Waits for device `device_index` to go idle, then returns the OPENR_SPF_STATUS_* bits
   its device-form calls raised since the last call (and clears them). */
int openr_spf_take_status(openr_spf_ctx* ctx, int device_index, uint32_t* out_status);

/* Diagnostics: waits for device `device_index` to go idle, then returns how many rows of
   its last solve call (openr_spf_solve*, _solve_device) were derived from their neighbours'
   rows instead of solved (uniform-cost batches that hold those neighbours; OPENR_SPF_DERIVE
   = 0 / 1 turns the split off / on wherever it is legal). 0 when the call was not split;
   rows handed to the re-run are counted. */
int openr_spf_last_derived(openr_spf_ctx* ctx, int device_index, uint32_t* out_derived);

/* Per-link-failure what-if sweep (no reference API: the north-star what-if workload over
   LinkState::runSpf(src, useLinkMetric, {link}), LinkState.cpp:808-882 with the
   linksToIgnore argument getKthPaths uses at :769-779). Unit (i, j) fails links[i] for
   sources[j]; changed[i * n_sources + j] = number of nodes whose distance or next-hop
   set differs from the no-failure SPF of sources[j] (a node that becomes unreachable
   counts). A link with no tight edge in the base SPF cannot change the result: such
   units are 0 without a solve. *out_solved (nullable) = SPFs actually run (base solves
   + affected units), also added to stats.spf_runs. Links are split across devices. */
int openr_spf_whatif(openr_spf_ctx* ctx, const uint32_t* links, uint32_t n_links,
                     const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                     uint32_t* changed, uint64_t* out_solved);

/* Device-buffer form (pointers are device memory; d_changed [n_links][n_sources]).
   Synchronizes `stream` once (the affected-unit count sizes the chunked solves).
   Link ids >= L are never affected (0). */
int openr_spf_whatif_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_links,
                            uint32_t n_links, const uint32_t* d_sources, uint32_t n_sources,
                            uint32_t flags, uint32_t* d_changed, void* stream,
                            uint64_t* out_solved);

/* What-if sweep with the per-unit delta (round 6): besides changed[], the nodes each
   failure changes, with their new distance and next-hop bits, i.e. the part of
   runSpf(sources[j], useLinkMetric, {links[i]}) (LinkState.cpp:808-882, SpfResult
   LinkState.h:436-443) that differs from the no-failure SPF. A consumer builds
   post-failure routes from it without solving again.
   Host form: a CSR over units u = i * n_sources + j. Unit u's entries are
   [ptr[u], ptr[u + 1]), with node ids ascending and ptr[n_units] = sum(changed).
   dist[k] is UINT64_MAX for a node the failure makes unreachable. nh[k] holds nh_bytes
   bytes in openr_spf_solve's row layout (bit b = the b-th distinct neighbour of the
   source), zero past the graph's width. nh_bytes must be >= that width.
   When sum(changed) > cap, ptr and changed are filled, the entries are not, and the call
   returns OPENR_SPF_E2BIG. The entries come from the repair's own overlays (and from the
   seeded re-solve of the few units too large for them): no second solve is run for them. */
typedef struct {
  uint64_t* ptr;     /* [n_links * n_sources + 1] */
  uint32_t* node;    /* [cap] */
  uint64_t* dist;    /* [cap] */
  uint8_t* nh;       /* [cap][nh_bytes] */
  uint64_t cap;      /* entries the caller allocated */
  uint32_t nh_bytes; /* bytes per next-hop entry */
} openr_spf_whatif_delta_t;
int openr_spf_whatif_delta(openr_spf_ctx* ctx, const uint32_t* links, uint32_t n_links,
                           const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                           uint32_t* changed, openr_spf_whatif_delta_t* delta,
                           uint64_t* out_solved);

/* Device-buffer form (every buffer device memory): the same CSR, d_ptr [n_units + 1],
   with each unit's entries in the order the repair found them (not sorted). The repair
   writes into library scratch, a few slots per unit from per-wave blocks; a scan of
   changed and a gather then pack the caller's arrays. *out_total (host, nullable) =
   sum(changed). d_ptr and d_changed are always filled; when the total exceeds cap the
   entries are not, and the call returns OPENR_SPF_E2BIG (cap 0: counts and ptr only).
   Synchronizes `stream`. */
int openr_spf_whatif_delta_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_links,
                                  uint32_t n_links, const uint32_t* d_sources, uint32_t n_sources,
                                  uint32_t flags, uint32_t* d_changed, uint64_t* d_ptr,
                                  uint32_t* d_node, uint64_t* d_dist, uint8_t* d_nh, uint64_t cap,
                                  uint32_t nh_bytes, void* stream, uint64_t* out_total,
                                  uint64_t* out_solved);

/* What-if sweep over link sets: node failures (all of a router's links at once) and
   shared-risk link groups (the links that share a fibre, a line card, a conduit). The
   failure unit is a set of links instead of one link; everything else is the single-link
   sweep. Sets are a CSR: set i = set_links[set_ptr[i] .. set_ptr[i + 1]). Unit (i, j) is
   LinkState::runSpf(sources[j], useLinkMetric, set i) (LinkState.cpp:808-882, the set
   passed as the linksToIgnore argument) compared with the no-failure SPF of sources[j].
   changed [n_sets][n_sources] and *out_solved mean what they mean for openr_spf_whatif.
   An empty set changes nothing; a link listed twice in a set counts once. A unit is
   affected iff some link of its set carries a tight edge of the base SPF in either
   direction (nh and dist depend on tight edges only, so any other set changes nothing:
   0 without a solve); on exact-order plans with zero or wrapped metrics, iff some link of
   its set is a link of the graph. *out_solved = base solves + affected units, also added
   to stats.spf_runs. Every affected unit is re-solved with its set ignored (seeded from
   the base rows where the rounds kernel runs). A call whose sets are all singletons
   returns what openr_spf_whatif returns for those links.
   A link id >= num_links, or a set_ptr that does not ascend, is OPENR_SPF_EINVAL. Sets
   are split in contiguous blocks across the context's devices. */
int openr_spf_whatif_sets(openr_spf_ctx* ctx, const uint32_t* set_ptr, const uint32_t* set_links,
                          uint32_t n_sets, const uint32_t* sources, uint32_t n_sources,
                          uint32_t flags, uint32_t* changed, uint64_t* out_solved);

/* Device-buffer form (d_set_ptr [n_sets + 1], d_set_links [n_set_links], d_changed
   [n_sets][n_sources]; all device memory). Link ids >= L are ignored, as the ignore sets
   of openr_spf_solve_device are; no slice is read past n_set_links. Synchronizes `stream`
   once (the affected-unit count sizes the chunked solves). */
int openr_spf_whatif_sets_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_set_ptr,
                                 const uint32_t* d_set_links, uint32_t n_sets,
                                 uint32_t n_set_links, const uint32_t* d_sources,
                                 uint32_t n_sources, uint32_t flags, uint32_t* d_changed,
                                 void* stream, uint64_t* out_solved);

/* Link-set sweep with the per-unit delta: openr_spf_whatif_delta with unit i a set. ptr,
   node, dist, nh, cap, OPENR_SPF_E2BIG and *out_solved mean exactly what they mean there;
   delta->ptr has n_sets * n_sources + 1 entries and each unit's nodes are ascending. */
int openr_spf_whatif_sets_delta(openr_spf_ctx* ctx, const uint32_t* set_ptr,
                                const uint32_t* set_links, uint32_t n_sets,
                                const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                                uint32_t* changed, openr_spf_whatif_delta_t* delta,
                                uint64_t* out_solved);

/* Device-buffer form: openr_spf_whatif_delta_device with unit i a set. Each unit's entries
   are in the order the re-solve found them (not sorted). Synchronizes `stream`. */
int openr_spf_whatif_sets_delta_device(openr_spf_ctx* ctx, int device_index,
                                       const uint32_t* d_set_ptr, const uint32_t* d_set_links,
                                       uint32_t n_sets, uint32_t n_set_links,
                                       const uint32_t* d_sources, uint32_t n_sources,
                                       uint32_t flags, uint32_t* d_changed, uint64_t* d_ptr,
                                       uint32_t* d_node, uint64_t* d_dist, uint8_t* d_nh,
                                       uint64_t cap, uint32_t nh_bytes, void* stream,
                                       uint64_t* out_total, uint64_t* out_solved);

/* A table of prefix groups (CSR). A prefix is advertised by a set of nodes (anycast); after
   SpfSolver::selectBestRoutes its best advertisers are the group. Group k is
   group_nodes[group_ptr[k] .. group_ptr[k + 1]), node ids < V strictly ascending inside a
   group (no duplicates). Empty groups are allowed; a node may sit in any number of groups. */
typedef struct {
  uint32_t n_groups;
  const uint32_t* group_ptr;    /* [n_groups + 1] */
  const uint32_t* group_nodes;  /* [group_ptr[n_groups]] */
} openr_spf_groups_t;

/* Best-path selection over prefix groups for a batch of sources: SpfSolver::getMinCostNodes
   plus the shortest-path half of getNextHopsWithMetric (Decision.cpp:1094-1167) on the rows
   of openr_spf_solve. For source i and group k (G = n_groups):
     metric[i][k]  the minimum of dist[v] over the members with dist[v] != UINT64_MAX;
                   UINT64_MAX if there is none (an empty group is unreachable)
     nh[i][k][b]   the OR of nh[v] over the members at that minimum, nh_bytes bytes in
                   openr_spf_solve's layout, zero past the graph's width, all zero when
                   metric is UINT64_MAX (nullable; nh_bytes >= openr_spf_nh_bytes)
     n_best[i][k]  the number of members at the minimum, 0 when unreachable (nullable)
   A group that contains the source has metric 0 and an empty nh, as getMinCostNodes gives.
   With OPENR_SPF_USE_LINK_METRIC a graph with a usable metric outside [1, 2^31-1] returns
   OPENR_SPF_ENOTSUP, as openr_spf_ksp2 does (a reached node can carry UINT64_MAX there, and
   the rule would misread it); the hop-count form is always allowed. A member >= V, a
   group_ptr that does not ascend or a group that is not strictly ascending is
   OPENR_SPF_EINVAL. The sources are solved into library scratch (in chunks when n x V rows
   exceed the what-if chunk budget) and reduced on the device; they are split in contiguous
   blocks across the context's devices. The LFA half of getNextHopsWithMetric
   (Decision.cpp:1169-1204) is openr_spf_lfa_routes, which returns these routes too. */
int openr_spf_routes(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n, uint32_t flags,
                     const openr_spf_groups_t* groups, uint64_t* metric, uint8_t* nh, uint32_t nh_bytes,
                     uint32_t* n_best);

/* Device-buffer form (every pointer device memory; d_group_nodes has n_group_nodes entries;
   d_nh / d_n_best may be NULL). The group table is not validated: a slice is clamped to
   n_group_nodes and a member >= V counts as unreachable. Asynchronous on `stream`. */
int openr_spf_routes_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_sources, uint32_t n,
                            uint32_t flags, const uint32_t* d_group_ptr, const uint32_t* d_group_nodes,
                            uint32_t n_groups, uint32_t n_group_nodes, uint64_t* d_metric, uint8_t* d_nh,
                            uint32_t nh_bytes, uint32_t* d_n_best, void* stream);

/* Loop-free alternates (LFA, RFC 5286) over prefix groups for a batch of sources: the LFA
   half of SpfSolver::getNextHopsWithMetric (Decision.cpp:1169-1204), i.e.
   getNextHopsWithMetric(me, group, perDestination = false, one area) with computeLfaPaths_
   on, applied literally to the rows openr_spf_solve gives under `flags`. For source i
   (node s) and group k:
     metric, nh    exactly what openr_spf_routes returns: the minimum over the members in the
                   SpfResult and the OR of the members' sets at that minimum
     alt[i][k][b]  empty when metric is UINT64_MAX (no member reached, an empty group): the
                   reference continues before its LFA loop (:1156-1158), and metric + toMe is
                   never formed there (it would wrap). Otherwise every distinct neighbour n of
                   s with at least one up link s-n is tested; b is n's next-hop bit
                   (openr_spf_neighbor_map) and toMe = dist_n(s). Every member d of the group
                   is tested, not only those at the minimum: d qualifies when dist_n(d) !=
                   UINT64_MAX and dist_n(d) < metric + toMe. Bit b is set iff some member
                   qualifies. Same layout as nh: nh_bytes bytes, zero past the graph's width.
     n_alt[i][k]   popcount(alt) (nullable)
     alt_metric    per set bit b, the value the reference keeps under key (n, ""): the
                   minimum of dist_n(d) over the qualifying members, and of metric - dist_s(n)
                   too when b is in nh (:1163-1166, :1196-1200)
   The RIB's next-hop set is nh | alt; the LFA-only next hops are alt & ~nh. A neighbour
   reached only over down links is never tested. An overloaded neighbour is tested (its own
   SPF expands it as the source). A group that contains s has metric 0 and an empty nh, and
   its other members can still qualify a neighbour. The hop-count form applies the same rule
   to hop rows. perDestination = true (the KSP2 / BGP form) and multi-area ECMP are not
   covered; the rule over what-if rows is openr_spf_whatif_lfa.
   entries (nullable: no entry output, one pass) is a CSR over units u = i * n_groups + k:
   unit u's alternates are [ptr[u], ptr[u + 1]), next-hop bits ascending. OPENR_SPF_E2BIG
   means sum(n_alt) > cap and nothing else: ptr, n_alt, metric, nh and alt are filled, the
   entries are not. cap = 0 gives counts and ptr only. metric must be non-NULL; nh, alt and
   n_alt may be NULL; nh_bytes >= openr_spf_nh_bytes. Group validation and errors (EINVAL,
   ENOTSUP on a usable metric outside [1, 2^31-1] under link metric) are those of
   openr_spf_routes. The rows needed are the distinct nodes among the sources and their up
   neighbours; each is solved once into library scratch (next hops for the sources only).
   When they exceed the what-if chunk budget the sources are processed in chunks, each with
   its own neighbour closure: a row two chunks need is solved in both, and so is a source
   listed twice. *out_solved (nullable) = rows solved, also added to stats.spf_runs. Sources
   are split in contiguous blocks across the context's devices. */
typedef struct {
  uint64_t* ptr;      /* [n * n_groups + 1], unit u = i * n_groups + k */
  uint32_t* nbr;      /* [cap] next-hop bit index, ascending inside a unit */
  uint64_t* metric;   /* [cap] alt_metric */
  uint64_t cap;       /* entries the caller allocated */
} openr_spf_lfa_entries_t;
int openr_spf_lfa_routes(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n, uint32_t flags,
                         const openr_spf_groups_t* groups, uint64_t* metric, uint8_t* nh, uint8_t* alt,
                         uint32_t nh_bytes, uint32_t* n_alt, openr_spf_lfa_entries_t* entries,
                         uint64_t* out_solved);

/* Device-buffer form (every buffer device memory; groups as in openr_spf_routes_device: not
   validated, a slice is clamped to n_group_nodes and a member >= V counts as unreached).
   d_nh, d_alt and d_n_alt may be NULL. d_ptr NULL: no entry output (d_nbr, d_alt_metric and
   cap are ignored). Else d_ptr [n * n_groups + 1] is always filled and *out_total (host,
   nullable) = sum(n_alt); when it exceeds cap the entries are not written and the call
   returns OPENR_SPF_E2BIG (cap 0: counts and ptr only). Synchronizes `stream` once per chunk
   of sources for the number of needed rows (it sizes the solve of the neighbours' rows), and
   once more per chunk for the total when entries are requested; everything else is
   enqueued. */
int openr_spf_lfa_routes_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_sources, uint32_t n,
                                uint32_t flags, const uint32_t* d_group_ptr, const uint32_t* d_group_nodes,
                                uint32_t n_groups, uint32_t n_group_nodes, uint64_t* d_metric, uint8_t* d_nh,
                                uint8_t* d_alt, uint32_t nh_bytes, uint32_t* d_n_alt, uint64_t* d_ptr,
                                uint32_t* d_nbr, uint64_t* d_alt_metric, uint64_t cap, void* stream,
                                uint64_t* out_total, uint64_t* out_solved);

/* Route-level what-if sweep: which routes move when a router or a shared-risk group fails,
   i.e. what Decision's route rebuild (getMinCostNodes / getNextHopsWithMetric,
   Decision.cpp:1094-1167) yields on LinkState::runSpf(sources[j], useLinkMetric, set i)
   (LinkState.cpp:808-882) where it differs from the no-failure routes of sources[j].
   Failure units are link sets exactly as in openr_spf_whatif_sets (single links are
   singleton sets); its validation and the meaning of *out_solved hold here. The route of a
   group changed iff its metric or nh differs from the no-failure route of the same source; a
   move of n_best alone is not a change (the RIB entry is identical), n_best is still
   reported with each changed route. changed_routes [n_sets][n_sources] counts them.
   delta (nullable: counts only) is a CSR over units u = i * n_sources + j like the node
   delta: unit u's entries are [ptr[u], ptr[u + 1]), group ids ascending, metric UINT64_MAX
   for a route the failure removes, nh in openr_spf_routes' layout (nh_bytes >= the graph's
   width, zero past it). OPENR_SPF_E2BIG means sum(changed_routes) > cap and nothing else:
   ptr and changed_routes are filled, the entries are not. The node delta the pass reads is
   held in library scratch that grows as needed. Errors for groups and metrics as in
   openr_spf_routes. Sets are split in contiguous blocks across the context's devices. */
typedef struct {
  uint64_t* ptr;     /* [n_sets * n_sources + 1] */
  uint32_t* group;   /* [cap] group ids, ascending inside a unit */
  uint64_t* metric;  /* [cap] new metric, UINT64_MAX = route lost */
  uint8_t* nh;       /* [cap][nh_bytes] */
  uint32_t* n_best;  /* [cap], nullable */
  uint64_t cap;      /* entries the caller allocated */
  uint32_t nh_bytes; /* bytes per next-hop entry */
} openr_spf_whatif_routes_t;
int openr_spf_whatif_routes(openr_spf_ctx* ctx, const uint32_t* set_ptr, const uint32_t* set_links, uint32_t n_sets,
                            const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                            const openr_spf_groups_t* groups, uint32_t* changed_routes,
                            openr_spf_whatif_routes_t* delta, uint64_t* out_solved);

/* Device-buffer form (every buffer device memory; sets as in openr_spf_whatif_sets_device,
   groups as in openr_spf_routes_device, not validated): d_changed_routes [n_sets][n_sources],
   d_ptr [n_units + 1], each unit's entries in the order the kernel found them (not sorted);
   d_n_best may be NULL. *out_total (host, nullable) = sum(changed_routes). d_ptr and
   d_changed_routes are always filled; when the total exceeds cap the entries are not, and
   the call returns OPENR_SPF_E2BIG (cap 0: counts and ptr only). Synchronizes `stream`. */
int openr_spf_whatif_routes_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_set_ptr,
                                   const uint32_t* d_set_links, uint32_t n_sets, uint32_t n_set_links,
                                   const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                   const uint32_t* d_group_ptr, const uint32_t* d_group_nodes, uint32_t n_groups,
                                   uint32_t n_group_nodes, uint32_t* d_changed_routes, uint64_t* d_ptr,
                                   uint32_t* d_group, uint64_t* d_metric, uint8_t* d_nh, uint32_t* d_n_best,
                                   uint64_t cap, uint32_t nh_bytes, void* stream, uint64_t* out_total,
                                   uint64_t* out_solved);

/* Post-failure loop-free alternates: which (source, prefix group) pairs keep a backup next
   hop after a router or a shared-risk group fails, and which lose it. For failure set i (a
   link set as in openr_spf_whatif_sets), source j (node s) and group k the LFA RIB entry
   (metric', nh', alt') is exactly what openr_spf_lfa_routes returns for (s, k) on the graph
   in which every link of set i has edge_up = 0, under the same flags:
     - metric' and nh' are the route of openr_spf_whatif_routes for that unit. Next-hop bit
       positions are those of the unfailed graph (openr_spf_neighbor_map): a failure never
       renumbers bits.
     - a neighbour n of s is tested iff at least one link s-n is up and not in set i (the
       reference skips links that are not up in its LFA loop, Decision.cpp:1169-1204).
     - toMe = dist'_n(s); a member d qualifies when dist'_n(d) != UINT64_MAX and dist'_n(d) <
       metric' + toMe, primes denoting rows of runSpf(x, useLinkMetric, set i).
     - alt' is empty when metric' == UINT64_MAX.
     - every other rule of openr_spf_lfa_routes holds unchanged: every member is tested, an
       overloaded neighbour is tested, a group holding s has metric 0 and an empty nh, alt and
       nh are zero past the graph's width.
   An entry of unit u = i * n_sources + j changed iff metric', nh' or alt' differs from the
   no-failure entry of (s, k). An empty set changes nothing.
     changed[i][j]      changed entries of the unit
     unprotected[i][j]  (nullable) groups that are live after the failure (metric' !=
                        UINT64_MAX and nh' non-empty) with popcount(nh' | alt') == 1
     lost_backup[i][j]  (nullable) groups that were live with popcount(nh | alt) >= 2 before
                        the failure and are live with popcount(nh' | alt') == 1 after it
   delta (nullable: counts only) is a CSR over units exactly like openr_spf_whatif_routes_t:
   unit u's entries are [ptr[u], ptr[u + 1]), group ids ascending, each with the new metric,
   nh and alt (nh_bytes >= the graph's width, zero past it). OPENR_SPF_E2BIG means
   sum(changed) > cap and nothing else: ptr and all counts are filled, the entries are not;
   cap = 0 gives counts and ptr only. *out_solved (nullable) is what openr_spf_whatif_sets
   reports for the same sets over the list "the sources as given, then their up neighbours
   that are no source, ascending" (the sweep this call runs); it is added to stats.spf_runs.
   Sets are validated as in openr_spf_whatif_sets, groups and metrics as in openr_spf_routes
   (EINVAL; ENOTSUP for a usable metric outside [1, 2^31-1] under link metric, the hop-count
   form is always allowed); nh_bytes below the graph's width is EINVAL. Sets are split in
   contiguous blocks across the context's devices. Not covered: per-alternate alt_metric
   entries under failure, perDestination = true, multi-area, and chunking of the sources (the
   base rows of the sources and their neighbours must fit what the sweep accepts; larger
   inputs get the sweep's own error). */
typedef struct {
  uint64_t* ptr;     /* [n_sets * n_sources + 1] */
  uint32_t* group;   /* [cap] group ids, ascending inside a unit */
  uint64_t* metric;  /* [cap] new metric, UINT64_MAX = route lost */
  uint8_t* nh;       /* [cap][nh_bytes] */
  uint8_t* alt;      /* [cap][nh_bytes] */
  uint64_t cap;      /* entries the caller allocated */
  uint32_t nh_bytes; /* bytes per next-hop entry */
} openr_spf_whatif_lfa_t;
int openr_spf_whatif_lfa(openr_spf_ctx* ctx, const uint32_t* set_ptr, const uint32_t* set_links, uint32_t n_sets,
                         const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                         const openr_spf_groups_t* groups, uint32_t* changed, uint32_t* unprotected,
                         uint32_t* lost_backup, openr_spf_whatif_lfa_t* delta, uint64_t* out_solved);

/* Device-buffer form (every buffer device memory). Sets and groups are not validated: they
   are clamped exactly as in openr_spf_whatif_routes_device and openr_spf_lfa_routes_device (a
   slice is clamped to its array, a link id >= L matches no link, a member >= V counts as
   unreached). d_changed [n_sets][n_sources]; d_unprotected and d_lost_backup may be NULL.
   d_ptr NULL: counts only (the entry buffers and cap are ignored). Else d_ptr [n_units + 1] is
   always filled, each unit's entries in the order the kernel found them (not sorted); when
   the total exceeds cap the entries are not written and the call returns OPENR_SPF_E2BIG.
   *out_total (host, nullable) = sum(changed). Synchronizes `stream`. */
int openr_spf_whatif_lfa_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_set_ptr,
                                const uint32_t* d_set_links, uint32_t n_sets, uint32_t n_set_links,
                                const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                const uint32_t* d_group_ptr, const uint32_t* d_group_nodes, uint32_t n_groups,
                                uint32_t n_group_nodes, uint32_t* d_changed, uint32_t* d_unprotected,
                                uint32_t* d_lost_backup, uint64_t* d_ptr, uint32_t* d_group, uint64_t* d_metric,
                                uint8_t* d_nh, uint8_t* d_alt, uint64_t cap, uint32_t nh_bytes, void* stream,
                                uint64_t* out_total, uint64_t* out_solved);

/* Drain what-if sweep: what moves when an operator drains routers or links before
   maintenance. A drain event i is a set of nodes N_i, which get the overload bit, and
   optionally a set of links K_i, which are overloaded links (Link::isUp() is false: unusable
   in both directions). Unit (i, j) is runSpf(sources[j], useLinkMetric, K_i) on the graph in
   which every node of N_i has node_overloaded = 1, compared with the no-event SPF of
   sources[j]. A drained node is not a failed node: it stays reachable and keeps its own
   prefixes, but carries no transit traffic ("reached, never expanded", LinkState.cpp:831-838).
     - a drained node that is the unit's source still expands;
     - a node that is overloaded already changes nothing;
     - a node or link listed twice counts once; an empty event changes nothing;
     - next-hop bit positions are those of the unmodified graph (openr_spf_neighbor_map).
   changed [n_events][n_sources] = nodes whose distance or next-hop bytes differ (a node that
   becomes unreachable counts). delta (nullable: counts only) is the CSR of
   openr_spf_whatif_sets_delta over units u = i * n_sources + j: node ids ascending, dist
   UINT64_MAX = unreachable; OPENR_SPF_E2BIG means sum(changed) > cap and nothing else.
   *out_solved (nullable) = base solves + affected units (units with a removed edge on a
   shortest path of the source); it is added to stats.spf_runs. Events are split in
   contiguous blocks across the context's devices.
   Errors: OPENR_SPF_EINVAL for a null or non-ascending node_ptr / link_ptr, a node >= V, a
   link >= L, or n_events * n_sources > 2^32 - 1; OPENR_SPF_ENOTSUP when the base SPF needs
   the exact-order kernel (zero or wrapped metrics under link metric, next-hop sets wider
   than 256 bits, OPENR_SPF_FORCE_EXACT; the hop-count form of such a graph is served);
   OPENR_SPF_E2BIG when a unit's state does not fit LDS. Loop-free alternates under a drain
   are openr_spf_whatif_drain_lfa below. Metric raises (soft drains) are
   openr_spf_whatif_metric. */
typedef struct {
  uint32_t n_events;
  const uint32_t* node_ptr;  /* [n_events + 1] */
  const uint32_t* nodes;     /* drained node ids */
  const uint32_t* link_ptr;  /* nullable: no links in any event; else [n_events + 1] */
  const uint32_t* links;     /* drained (unusable) link ids */
} openr_spf_drain_events_t;
int openr_spf_whatif_drain(openr_spf_ctx* ctx, const openr_spf_drain_events_t* events, const uint32_t* sources,
                           uint32_t n_sources, uint32_t flags, uint32_t* changed, openr_spf_whatif_delta_t* delta,
                           uint64_t* out_solved);

/* Device-buffer form (every buffer device memory), conventions of
   openr_spf_whatif_sets_delta_device: d_nodes holds n_nodes entries and d_links n_links
   (d_link_ptr NULL: no links); every slice is clamped to them and ids out of range are
   skipped, nothing is read out of bounds. d_changed [n_events][n_sources], d_ptr
   [n_units + 1], entries of a unit in the order the kernel found them (not sorted). cap 0:
   counts and ptr only; when the total exceeds cap the entries are not written and the call
   returns OPENR_SPF_E2BIG. *out_total (host, nullable) = sum(changed). Synchronizes `stream`. */
int openr_spf_whatif_drain_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                  const uint32_t* d_nodes, const uint32_t* d_link_ptr, const uint32_t* d_links,
                                  uint32_t n_events, uint32_t n_nodes, uint32_t n_links, const uint32_t* d_sources,
                                  uint32_t n_sources, uint32_t flags, uint32_t* d_changed, uint64_t* d_ptr,
                                  uint32_t* d_node, uint64_t* d_dist, uint8_t* d_nh, uint64_t cap, uint32_t nh_bytes,
                                  void* stream, uint64_t* out_total, uint64_t* out_solved);

/* The same sweep resolved to routes over a group table: outputs, route rule and errors of
   openr_spf_whatif_routes[_device], units and errors of openr_spf_whatif_drain[_device]. The
   loopback route of a drained node keeps a finite metric wherever the base SPF reached it. */
int openr_spf_whatif_drain_routes(openr_spf_ctx* ctx, const openr_spf_drain_events_t* events, const uint32_t* sources,
                                  uint32_t n_sources, uint32_t flags, const openr_spf_groups_t* groups,
                                  uint32_t* changed_routes, openr_spf_whatif_routes_t* delta, uint64_t* out_solved);
int openr_spf_whatif_drain_routes_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                         const uint32_t* d_nodes, const uint32_t* d_link_ptr, const uint32_t* d_links,
                                         uint32_t n_events, uint32_t n_nodes, uint32_t n_links,
                                         const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                         const uint32_t* d_group_ptr, const uint32_t* d_group_nodes,
                                         uint32_t n_groups, uint32_t n_group_nodes, uint32_t* d_changed_routes,
                                         uint64_t* d_ptr, uint32_t* d_group, uint64_t* d_metric, uint8_t* d_nh,
                                         uint32_t* d_n_best, uint64_t cap, uint32_t nh_bytes, void* stream,
                                         uint64_t* out_total, uint64_t* out_solved);

/* Loop-free alternates under a drain: which (source, prefix group) pairs move and which stop
   being protected while routers or links are out for maintenance. Events are those of
   openr_spf_whatif_drain, groups and outputs those of openr_spf_whatif_lfa (changed,
   unprotected and lost_backup, each nullable, and the CSR delta), units u = i * n_sources + j.
   For event i, source j (node s) and group k the entry (metric', nh', alt') is exactly what
   openr_spf_lfa_routes returns for (s, k) on the graph patched by event i (the graph
   openr_spf_whatif_drain defines), under the same flags; next-hop bit positions are those of
   the unmodified graph. An entry changed iff metric', nh' or alt' differs from the no-event
   entry; unprotected and lost_backup mean what they mean in openr_spf_whatif_lfa.
     - the reference's LFA loop walks linksFromNode(me) and skips a link only when it is not
       up (Decision.cpp:1171-1174); it never looks at a neighbour's overload bit, and takes
       the neighbour's rows from the SPF *from* the neighbour, in which the neighbour expands
       because it is the source. So a neighbour n of s is tested iff some link s-n has edge_up
       and is not in K_i; the nodes of N_i change no tested status, and a drained neighbour
       is tested.
     - toMe = dist'_n(s); a member d qualifies when dist'_n(d) != UINT64_MAX and dist'_n(d) <
       metric' + toMe, primes denoting the rows of openr_spf_whatif_drain's unit (i, n), in
       which n expands as the unit's source. alt' is empty when metric' == UINT64_MAX. Every
       other rule of openr_spf_lfa_routes holds unchanged.
   The host form sorts a unit's entries by group id. OPENR_SPF_E2BIG means sum(changed) > cap
   and nothing else; cap = 0 gives counts and ptr only. *out_solved (nullable) is what
   openr_spf_whatif_drain reports for the same events over the list "the sources as given,
   then their up neighbours that are no source, ascending" (the sweep this call runs); it is
   added to stats.spf_runs. Events are split in contiguous blocks across the context's
   devices. Errors: events as in openr_spf_whatif_drain (a graph whose repair unit does not
   fit LDS is OPENR_SPF_ENOTSUP here), groups and metrics as in openr_spf_routes, nh_bytes
   below the graph's width EINVAL, an exact-order base plan ENOTSUP. Not covered:
   per-alternate alt_metric entries, perDestination = true, multi-area, and chunking of the
   sources (as openr_spf_whatif_lfa). */
int openr_spf_whatif_drain_lfa(openr_spf_ctx* ctx, const openr_spf_drain_events_t* events, const uint32_t* sources,
                               uint32_t n_sources, uint32_t flags, const openr_spf_groups_t* groups,
                               uint32_t* changed, uint32_t* unprotected, uint32_t* lost_backup,
                               openr_spf_whatif_lfa_t* delta, uint64_t* out_solved);

/* Device-buffer form: events as openr_spf_whatif_drain_routes_device, groups and outputs as
   openr_spf_whatif_lfa_device (d_ptr NULL: counts only; entries in the kernel's order).
   Nothing is validated: events are clamped and skipped exactly as in
   openr_spf_whatif_drain_device, groups as in openr_spf_whatif_lfa_device. Synchronizes
   `stream`. */
int openr_spf_whatif_drain_lfa_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                      const uint32_t* d_nodes, const uint32_t* d_link_ptr, const uint32_t* d_links,
                                      uint32_t n_events, uint32_t n_nodes, uint32_t n_links,
                                      const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                      const uint32_t* d_group_ptr, const uint32_t* d_group_nodes, uint32_t n_groups,
                                      uint32_t n_group_nodes, uint32_t* d_changed, uint32_t* d_unprotected,
                                      uint32_t* d_lost_backup, uint64_t* d_ptr, uint32_t* d_group,
                                      uint64_t* d_metric, uint8_t* d_nh, uint8_t* d_alt, uint64_t cap,
                                      uint32_t nh_bytes, void* stream, uint64_t* out_total, uint64_t* out_solved);

/* Metric what-if sweep: what moves when an operator soft-drains a router or a few links by
   raising metrics before maintenance. Traffic is pushed away, but the node stays a transit
   of last resort. A metric event i is a list of directed CSR edges (the edge ids of
   openr_spf_patch_graph) with a new metric each. Unit (i, j) is runSpf(sources[j], true) on
   the graph in which those edges carry the new metrics, compared with the no-event SPF of
   sources[j]. Only raises are served: a new metric below the current one is refused.
     - an entry whose new metric equals the current one changes nothing;
     - an entry on a down edge changes nothing;
     - an entry on a row of an overloaded node changes nothing, unless that node is the
       unit's source (it alone expands such a row);
     - inside an event the edge ids are strictly ascending; an empty event changes nothing;
     - next-hop bit positions are those of the unmodified graph (openr_spf_neighbor_map).
   changed [n_events][n_sources] = nodes whose distance or next-hop bytes differ. A raise
   disconnects nothing: no node becomes unreachable and no distance shrinks. delta (nullable:
   counts only) is the CSR of openr_spf_whatif_sets_delta over units u = i * n_sources + j:
   node ids ascending; OPENR_SPF_E2BIG means sum(changed) > cap and nothing else.
   *out_solved (nullable) = base solves + affected units (units with a really raised edge on
   a shortest path of the source); it is added to stats.spf_runs. Events are split in
   contiguous blocks across the context's devices.
   Without OPENR_SPF_USE_LINK_METRIC the call is served and launches no kernel: metrics do
   not enter runSpf(src, false), so every count is 0, ptr is all zero and *out_solved = 0.
   Errors: OPENR_SPF_EINVAL for a null or non-ascending edge_ptr, an edge >= E, an event
   slice that is not strictly ascending, a metric below the current one or above 2^31 - 1,
   or n_events * n_sources > 2^32 - 1; OPENR_SPF_ENOTSUP when the base SPF needs the
   exact-order kernel (as openr_spf_whatif_drain); OPENR_SPF_E2BIG when a unit's state does
   not fit LDS. Events that mix raises with overload bits or link-down sets are
   openr_spf_whatif_maint. Loop-free alternates under a metric event are openr_spf_whatif_metric_lfa below. Metric
   decreases are openr_spf_whatif_restore. */
typedef struct {
  uint32_t n_events;
  const uint32_t* edge_ptr;  /* [n_events + 1] */
  const uint32_t* edges;     /* directed CSR edge ids, strictly ascending inside an event */
  const uint32_t* metrics;   /* the new metric of edges[k] */
} openr_spf_metric_events_t;
int openr_spf_whatif_metric(openr_spf_ctx* ctx, const openr_spf_metric_events_t* events, const uint32_t* sources,
                            uint32_t n_sources, uint32_t flags, uint32_t* changed, openr_spf_whatif_delta_t* delta,
                            uint64_t* out_solved);

/* Device-buffer form (every buffer device memory), conventions of openr_spf_whatif_drain_device:
   d_edges and d_metrics hold n_edges entries. Nothing is validated: every slice is clamped
   to n_edges; an entry with an id >= E, or with a metric <= the current one or > 2^31 - 1,
   is skipped. For a slice that does not ascend, which of its entries take effect is
   unspecified; nothing is read out of bounds and every loop terminates. Cap, OPENR_SPF_E2BIG,
   *out_total and the order of a unit's entries are those of openr_spf_whatif_drain_device.
   Synchronizes `stream`. */
int openr_spf_whatif_metric_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_edge_ptr,
                                   const uint32_t* d_edges, const uint32_t* d_metrics, uint32_t n_events,
                                   uint32_t n_edges, const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                   uint32_t* d_changed, uint64_t* d_ptr, uint32_t* d_node, uint64_t* d_dist,
                                   uint8_t* d_nh, uint64_t cap, uint32_t nh_bytes, void* stream, uint64_t* out_total,
                                   uint64_t* out_solved);

/* The same sweep resolved to routes over a group table: outputs, route rule and errors of
   openr_spf_whatif_routes[_device], units and errors of openr_spf_whatif_metric[_device]. No
   route turns unreachable under a metric event. */
int openr_spf_whatif_metric_routes(openr_spf_ctx* ctx, const openr_spf_metric_events_t* events,
                                   const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                                   const openr_spf_groups_t* groups, uint32_t* changed_routes,
                                   openr_spf_whatif_routes_t* delta, uint64_t* out_solved);
int openr_spf_whatif_metric_routes_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_edge_ptr,
                                          const uint32_t* d_edges, const uint32_t* d_metrics, uint32_t n_events,
                                          uint32_t n_edges, const uint32_t* d_sources, uint32_t n_sources,
                                          uint32_t flags, const uint32_t* d_group_ptr, const uint32_t* d_group_nodes,
                                          uint32_t n_groups, uint32_t n_group_nodes, uint32_t* d_changed_routes,
                                          uint64_t* d_ptr, uint32_t* d_group, uint64_t* d_metric, uint8_t* d_nh,
                                          uint32_t* d_n_best, uint64_t cap, uint32_t nh_bytes, void* stream,
                                          uint64_t* out_total, uint64_t* out_solved);

/* Loop-free alternates under a metric event: openr_spf_whatif_drain_lfa with the events and
   the patched graph of openr_spf_whatif_metric. Tested status never changes under a metric
   event; the rows are those of openr_spf_whatif_metric's unit (i, n); closure, outputs,
   *out_solved and errors as there, with openr_spf_whatif_metric in place of the drain sweep.
   Without OPENR_SPF_USE_LINK_METRIC nothing moves: changed and lost_backup are 0, ptr is all
   zero and unprotected is each source's base count; the base rows of the closure are still
   solved for that count, no sweep kernel runs, and *out_solved is the number of closure
   rows. */
int openr_spf_whatif_metric_lfa(openr_spf_ctx* ctx, const openr_spf_metric_events_t* events, const uint32_t* sources,
                                uint32_t n_sources, uint32_t flags, const openr_spf_groups_t* groups,
                                uint32_t* changed, uint32_t* unprotected, uint32_t* lost_backup,
                                openr_spf_whatif_lfa_t* delta, uint64_t* out_solved);
int openr_spf_whatif_metric_lfa_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_edge_ptr,
                                       const uint32_t* d_edges, const uint32_t* d_metrics, uint32_t n_events,
                                       uint32_t n_edges, const uint32_t* d_sources, uint32_t n_sources,
                                       uint32_t flags, const uint32_t* d_group_ptr, const uint32_t* d_group_nodes,
                                       uint32_t n_groups, uint32_t n_group_nodes, uint32_t* d_changed,
                                       uint32_t* d_unprotected, uint32_t* d_lost_backup, uint64_t* d_ptr,
                                       uint32_t* d_group, uint64_t* d_metric, uint8_t* d_nh, uint8_t* d_alt,
                                       uint64_t cap, uint32_t nh_bytes, void* stream, uint64_t* out_total,
                                       uint64_t* out_solved);

/* Restore what-if sweep: what moves when an operator brings routers or links back after
   maintenance. A restore event i is three lists, each possibly empty: nodes N_i whose overload
   bit is cleared, links K_i that are put back in service (Link::isUp() becomes true, both
   directions), and directed CSR edges (the edge ids of openr_spf_patch_graph) with a new,
   lower metric each. Unit (i, j) is runSpf(sources[j], useLinkMetric) on the graph patched
   that way, compared with the no-event SPF of sources[j]. Each of these changes nothing:
     - a node that is not overloaded, a link that is up already, a new metric equal to the
       current one;
     - a lowered entry on an edge that is still down after the event;
     - an entry on a row of a node that still does not expand after the event (overloaded, not
       in N_i and not the unit's source);
     - an undrained node that is the unit's own source (the source always expands);
     - a node or link listed twice counts once; an empty event changes nothing;
     - next-hop bit positions are those of the unmodified graph (openr_spf_neighbor_map): bits
       are over distinct columns whatever the link state, so a link coming up renumbers none.
   changed [n_events][n_sources] = nodes whose distance or next-hop bytes differ (a node that
   becomes reachable counts). A restore lengthens nothing: no distance grows and no reachable
   node becomes unreachable. delta (nullable: counts only) is the CSR of
   openr_spf_whatif_sets_delta over units u = i * n_sources + j: node ids ascending;
   OPENR_SPF_E2BIG means sum(changed) > cap and nothing else. *out_solved (nullable) = base
   solves + affected units (units in which a new or cheaper edge reaches its head at or below
   the head's base distance); it is added to stats.spf_runs. Events are split in contiguous
   blocks across the context's devices.
   Without OPENR_SPF_USE_LINK_METRIC the node and link entries act (they add edges) and the
   metric entries are ignored; unlike openr_spf_whatif_metric the kernels run.
   Errors: OPENR_SPF_EINVAL for a null or non-ascending node_ptr / link_ptr / edge_ptr (the
   last two may be NULL), a node >= V, a link >= L, an edge >= E, an event's edge slice that
   is not strictly ascending, a new metric above the current one (a raise belongs to
   openr_spf_whatif_metric) or below 1, or n_events * n_sources > 2^32 - 1;
   OPENR_SPF_ENOTSUP when the base SPF needs the exact-order kernel (as
   openr_spf_whatif_drain; the hop-count form of such a graph is served), or when under link
   metric a link of some K_i has a directed edge whose metric after the event lies outside
   [1, 2^31 - 1] (a down edge may carry any value on a fast plan; restoring it would leave
   them); OPENR_SPF_E2BIG when a unit's state does not fit LDS. Not covered: events that mix
   restores with drains or raises, exact-order base plans. Loop-free alternates under a
   restore event are openr_spf_whatif_restore_lfa below. */
typedef struct {
  uint32_t n_events;
  const uint32_t* node_ptr;  /* [n_events + 1] */
  const uint32_t* nodes;     /* nodes whose overload bit is cleared */
  const uint32_t* link_ptr;  /* nullable: no links in any event; else [n_events + 1] */
  const uint32_t* links;     /* links put back in service */
  const uint32_t* edge_ptr;  /* nullable: no metric entries in any event; else [n_events + 1] */
  const uint32_t* edges;     /* directed CSR edge ids, strictly ascending inside an event */
  const uint32_t* metrics;   /* the new metric of edges[k], <= the current one */
} openr_spf_restore_events_t;
int openr_spf_whatif_restore(openr_spf_ctx* ctx, const openr_spf_restore_events_t* events, const uint32_t* sources,
                             uint32_t n_sources, uint32_t flags, uint32_t* changed, openr_spf_whatif_delta_t* delta,
                             uint64_t* out_solved);

/* Device-buffer form (every buffer device memory), conventions of openr_spf_whatif_drain_device:
   d_nodes holds n_nodes entries, d_links n_links (d_link_ptr NULL: no links), d_edges and
   d_metrics n_edges (d_edge_ptr NULL: no metric entries). Nothing is validated: every slice is
   clamped to its array; an id out of range, an entry whose metric is 0 or not below the
   current one, and a link whose restored edges would carry a metric outside [1, 2^31 - 1] are
   skipped. For an edge slice that does not ascend, which of its entries take effect is
   unspecified; nothing is read out of bounds and every loop terminates. Cap, OPENR_SPF_E2BIG,
   *out_total and the order of a unit's entries are those of openr_spf_whatif_drain_device.
   Synchronizes `stream`. */
int openr_spf_whatif_restore_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                    const uint32_t* d_nodes, const uint32_t* d_link_ptr, const uint32_t* d_links,
                                    const uint32_t* d_edge_ptr, const uint32_t* d_edges, const uint32_t* d_metrics,
                                    uint32_t n_events, uint32_t n_nodes, uint32_t n_links, uint32_t n_edges,
                                    const uint32_t* d_sources, uint32_t n_sources, uint32_t flags, uint32_t* d_changed,
                                    uint64_t* d_ptr, uint32_t* d_node, uint64_t* d_dist, uint8_t* d_nh, uint64_t cap,
                                    uint32_t nh_bytes, void* stream, uint64_t* out_total, uint64_t* out_solved);

/* The same sweep resolved to routes over a group table: outputs, route rule and errors of
   openr_spf_whatif_routes[_device], units and errors of openr_spf_whatif_restore[_device]. A
   route can turn reachable under a restore event, none turns unreachable. */
int openr_spf_whatif_restore_routes(openr_spf_ctx* ctx, const openr_spf_restore_events_t* events,
                                    const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                                    const openr_spf_groups_t* groups, uint32_t* changed_routes,
                                    openr_spf_whatif_routes_t* delta, uint64_t* out_solved);
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
                                           uint64_t* out_total, uint64_t* out_solved);

/* Loop-free alternates under a restore event: openr_spf_whatif_drain_lfa with the events and
   the patched graph of openr_spf_whatif_restore. A restore can make a neighbour tested that
   was not, and it can also take a backup away.
     - a neighbour n of s is tested iff some link s-n has edge_up or is an *effective* link of
       K_i: down today, and accepted by the restore sweep's own filter. The host form has
       already refused a link whose restored edges would carry a metric outside [1, 2^31 - 1]
       under link metric (OPENR_SPF_ENOTSUP); the device form skips such a link, with the
       same test as openr_spf_whatif_restore_device.
     - the rows are those of openr_spf_whatif_restore's unit (i, n).
     - the closure is the sources as given, then *every* distinct neighbour of a source that
       is no source, whatever the link state, ascending (a neighbour behind a down link can
       become tested and its base row must be resident); *out_solved is what
       openr_spf_whatif_restore reports over that list.
   Outputs, errors and limits as openr_spf_whatif_drain_lfa, with openr_spf_whatif_restore in
   place of the drain sweep. */
int openr_spf_whatif_restore_lfa(openr_spf_ctx* ctx, const openr_spf_restore_events_t* events,
                                 const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                                 const openr_spf_groups_t* groups, uint32_t* changed, uint32_t* unprotected,
                                 uint32_t* lost_backup, openr_spf_whatif_lfa_t* delta, uint64_t* out_solved);
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
                                        uint64_t* out_total, uint64_t* out_solved);

/* Maintenance what-if sweep: what moves under a maintenance plan that mixes the worsening
   kinds, e.g. router A hard-drained, its links to B out of service and neighbour C soft-drained
   by +1000 in one window. A maintenance event i is three lists, each possibly empty: nodes N_i
   that get the overload bit, links K_i taken out of service (Link::isUp() is false, both
   directions), and directed CSR edges (the edge ids of openr_spf_patch_graph) with a new, higher
   metric each. Unit (i, j) is runSpf(sources[j], useLinkMetric) on the graph patched with all
   three, compared with the no-event SPF of sources[j]. With X = N_i minus the unit's source
   minus the nodes that are overloaded already:
     - removed edges: e = u -> v is removed iff link(e) is in K_i or u is in X;
     - expansion: u may expand iff u is the source, or u is not overloaded and not in X;
     - raised edges: R = the entries whose edge is up and whose new metric lies in
       (w(e), 2^31 - 1]; w'(e) is the new metric if e is in R, else w(e);
     - a base-tight edge is lost iff it is removed or raised. The repair (A, the seeds,
       dist(A), D, the Kahn pass) is that of openr_spf_whatif_drain and openr_spf_whatif_metric,
       with weights read through w' and usability through the removed set.
   Each of these changes nothing:
     - a raise on a removed edge, on a down edge, or on a row of an overloaded node other than
       the unit's source;
     - a new metric equal to the current one;
     - a node that is overloaded already or is the unit's source (the source's row stays, and
       raises on it act);
     - an unused link id;
     - a node, link or edge listed twice counts once; an empty event changes nothing;
     - next-hop bit positions are those of the unmodified graph (openr_spf_neighbor_map).
   Running the drain and the metric sweep apart and overlaying their deltas does not give this
   answer. changed [n_events][n_sources] = nodes whose distance or next-hop bytes differ (a node
   that becomes unreachable counts). No distance shrinks. delta (nullable: counts only) is the
   CSR of openr_spf_whatif_sets_delta over units u = i * n_sources + j: node ids ascending;
   OPENR_SPF_E2BIG means sum(changed) > cap and nothing else. *out_solved (nullable) = base
   solves + affected units (units with a removed or really raised edge on a shortest path of
   the source); it is added to stats.spf_runs. Events are split in contiguous blocks across the
   context's devices.
   Without OPENR_SPF_USE_LINK_METRIC every weight is 1 and the metric entries are ignored; the
   kernels still run for N_i and K_i.
   Errors: OPENR_SPF_EINVAL for a null or non-ascending node_ptr / link_ptr / edge_ptr (the
   last two may be NULL), a node >= V, a link >= L, an edge >= E, an event's edge slice that
   is not strictly ascending, a new metric below the current one (a decrease is a restore
   event) or above 2^31 - 1, or n_events * n_sources > 2^32 - 1; OPENR_SPF_ENOTSUP when the
   base SPF needs the exact-order kernel (as openr_spf_whatif_drain; the hop-count form of such
   a graph is served); OPENR_SPF_E2BIG when a unit's state does not fit LDS. Not covered: events
   that mix worsening with restoring changes, exact-order base plans and the C++ LinkState
   mirror. Loop-free alternates under a maintenance event are openr_spf_whatif_maint_lfa below. */
typedef struct {
  uint32_t n_events;
  const uint32_t* node_ptr;  /* [n_events + 1] */
  const uint32_t* nodes;     /* nodes that get the overload bit */
  const uint32_t* link_ptr;  /* nullable: no links in any event; else [n_events + 1] */
  const uint32_t* links;     /* links taken out of service */
  const uint32_t* edge_ptr;  /* nullable: no metric entries in any event; else [n_events + 1] */
  const uint32_t* edges;     /* directed CSR edge ids, strictly ascending inside an event */
  const uint32_t* metrics;   /* the new metric of edges[k], >= the current one */
} openr_spf_maint_events_t;
int openr_spf_whatif_maint(openr_spf_ctx* ctx, const openr_spf_maint_events_t* events, const uint32_t* sources,
                           uint32_t n_sources, uint32_t flags, uint32_t* changed, openr_spf_whatif_delta_t* delta,
                           uint64_t* out_solved);

/* Device-buffer form (every buffer device memory), conventions of openr_spf_whatif_restore_device:
   d_nodes holds n_nodes entries, d_links n_links (d_link_ptr NULL: no links), d_edges and
   d_metrics n_edges (d_edge_ptr NULL: no metric entries). Nothing is validated: every slice is
   clamped to its array; an id out of range, an unused link and an entry whose metric is not in
   (current, 2^31 - 1] are skipped. For an edge slice that does not ascend, which of its entries
   take effect is unspecified; nothing is read out of bounds and every loop terminates. Cap,
   OPENR_SPF_E2BIG, *out_total and the order of a unit's entries are those of
   openr_spf_whatif_drain_device. Synchronizes `stream`. */
int openr_spf_whatif_maint_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                  const uint32_t* d_nodes, const uint32_t* d_link_ptr, const uint32_t* d_links,
                                  const uint32_t* d_edge_ptr, const uint32_t* d_edges, const uint32_t* d_metrics,
                                  uint32_t n_events, uint32_t n_nodes, uint32_t n_links, uint32_t n_edges,
                                  const uint32_t* d_sources, uint32_t n_sources, uint32_t flags, uint32_t* d_changed,
                                  uint64_t* d_ptr, uint32_t* d_node, uint64_t* d_dist, uint8_t* d_nh, uint64_t cap,
                                  uint32_t nh_bytes, void* stream, uint64_t* out_total, uint64_t* out_solved);

/* The same sweep resolved to routes over a group table: outputs, route rule and errors of
   openr_spf_whatif_routes[_device], units and errors of openr_spf_whatif_maint[_device]. A
   route can turn unreachable under a maintenance event (through K_i); a drained node's own
   prefixes stay reachable wherever the node is. */
int openr_spf_whatif_maint_routes(openr_spf_ctx* ctx, const openr_spf_maint_events_t* events,
                                  const uint32_t* sources, uint32_t n_sources, uint32_t flags,
                                  const openr_spf_groups_t* groups, uint32_t* changed_routes,
                                  openr_spf_whatif_routes_t* delta, uint64_t* out_solved);
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
                                         uint64_t* out_total, uint64_t* out_solved);

/* Loop-free alternates under a maintenance event: which prefixes stop being protected while
   the window is open. Events are those of openr_spf_whatif_maint, groups and outputs those of
   openr_spf_whatif_lfa. For event i = (N_i, K_i, raises), source j (node s) and group k the
   entry (metric', nh', alt') is what openr_spf_lfa_routes returns for (s, k) on the graph
   patched by the whole event; it is listed iff it differs from the no-event entry.
   Overlaying the answers of openr_spf_whatif_drain_lfa for (N_i, K_i) and of
   openr_spf_whatif_metric_lfa for the raises does not give this answer.
     - the reference's LFA loop (Decision.cpp:1169-1204) skips a link iff it is not up, reads
       the neighbour's own SPF row for toMe and for the members, and reads shortestMetric. It
       never reads the metric of the link s-n. So neither a raise nor an overload bit changes
       a tested status: a neighbour n of s is tested iff some link s-n is up and not in K_i,
       as under a drain event.
     - a raise acts through rows only: one on s -> n shows in the source's rows, one on n -> s
       in the rows of n (toMe = dist_n(s) moves). The rows are those of
       openr_spf_whatif_maint's unit (i, n), in which n expands because it is the source.
     - the closure is the drain's: the sources as given, then their up neighbours that are no
       source, ascending; *out_solved is what openr_spf_whatif_maint reports for the same
       events over that list (added to stats.spf_runs; a rerun of the sweep on scratch
       overflow counts once).
   Without OPENR_SPF_USE_LINK_METRIC the raises are ignored and the answer is that of
   openr_spf_whatif_drain_lfa for (N_i, K_i), bit for bit; the sweep still runs.
   Errors: events as openr_spf_whatif_maint checks them (OPENR_SPF_EINVAL for a decrease,
   OPENR_SPF_ENOTSUP for an exact-order base plan under link metric), groups and nh_bytes as
   openr_spf_whatif_lfa; a graph whose repair unit does not fit LDS is OPENR_SPF_ENOTSUP here.
   OPENR_SPF_E2BIG means sum(changed) > cap and nothing else. Events are split in contiguous
   blocks across the context's devices; each unit's entries are sorted by group. Not covered:
   per-alternate metrics, perDestination = true, multi-area, chunking of the sources. */
int openr_spf_whatif_maint_lfa(openr_spf_ctx* ctx, const openr_spf_maint_events_t* events, const uint32_t* sources,
                               uint32_t n_sources, uint32_t flags, const openr_spf_groups_t* groups,
                               uint32_t* changed, uint32_t* unprotected, uint32_t* lost_backup,
                               openr_spf_whatif_lfa_t* delta, uint64_t* out_solved);

/* Device-buffer form: events as openr_spf_whatif_maint_device (nothing is validated, every
   slice is clamped, bad ids and entries whose metric is not in (current, 2^31 - 1] are
   skipped), groups and outputs as openr_spf_whatif_lfa_device (d_ptr NULL: counts only;
   entries in the kernel's order). Synchronizes `stream`. */
int openr_spf_whatif_maint_lfa_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_node_ptr,
                                      const uint32_t* d_nodes, const uint32_t* d_link_ptr, const uint32_t* d_links,
                                      const uint32_t* d_edge_ptr, const uint32_t* d_edges, const uint32_t* d_metrics,
                                      uint32_t n_events, uint32_t n_nodes, uint32_t n_links, uint32_t n_edges,
                                      const uint32_t* d_sources, uint32_t n_sources, uint32_t flags,
                                      const uint32_t* d_group_ptr, const uint32_t* d_group_nodes, uint32_t n_groups,
                                      uint32_t n_group_nodes, uint32_t* d_changed, uint32_t* d_unprotected,
                                      uint32_t* d_lost_backup, uint64_t* d_ptr, uint32_t* d_group,
                                      uint64_t* d_metric, uint8_t* d_nh, uint8_t* d_alt, uint64_t cap,
                                      uint32_t nh_bytes, void* stream, uint64_t* out_total, uint64_t* out_solved);

/* LinkState::getKthPaths(src[i], dst[i], 1) and (.., 2) (LinkState.cpp:762-791, with
   traceOnePath :398-419) for a batch of pairs, traced on the device. Per pair, tok1 /
   tok2 [n_pairs][tok_cap] hold [n_paths, len_0, e.., len_1, e.., ...]: every path as
   its directed edge ids in src -> dest order (link = link_id[e]), paths in the
   reference's order; tokens past a row's used prefix are left unspecified. k = 2 ignores the links of the k = 1 paths. Link metrics are
   used (getKthPaths calls getSpfResult(src, true) / runSpf(src, true, ignore)). A pair
   whose paths exceed tok_cap tokens (or 255 hops) gets n_paths = 0xFFFFFFFF and the
   call returns OPENR_SPF_E2BIG after filling the others. So does a pair whose trace outgrows
   the tracer's arena: the depth-first search keeps the still untried pathLinks of every node
   on its stack, 1024 entries at most (a 33-hop path through layers of 32 nodes, each linked
   to the whole next layer, needs 1025). A row is marked on its own: tok2 may be marked where
   tok1 is not (the k = 2 paths are longer). Where tok1 is marked the k = 1 links are unknown,
   and the pair's tok2 row is marked as well. */
int openr_spf_ksp2(openr_spf_ctx* ctx, const uint32_t* src, const uint32_t* dst, uint32_t n_pairs,
                   uint32_t tok_cap, uint32_t* tok1, uint32_t* tok2);

/* Device-buffer form: pair i = (d_sources[d_pair_row[i]], d_pair_dst[i]); the base SPF
   is solved once per listed source. Synchronizes `stream` once at the end. */
int openr_spf_ksp2_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_sources,
                          uint32_t n_sources, const uint32_t* d_pair_row,
                          const uint32_t* d_pair_dst, uint32_t n_pairs, uint32_t tok_cap,
                          uint32_t* d_tok1, uint32_t* d_tok2, void* stream);

/* Page-locked host memory for the caller-owned host buffers of the batch calls (the
   openr_spf_ksp2 token rows, solve rows): their device-to-host copies then run at link rate
   instead of through a pageable staging copy (the DecisionBenchmark G100 KSP2 update copied
   2 x 20 MB of token rows at ~2.3 GB/s). openr_spf_host_free(NULL) is a no-op. */
int openr_spf_host_alloc(size_t bytes, void** out);
void openr_spf_host_free(void* p);

/* In-place attribute patch of the mirror: the link structure —
   rows, columns, link ids — is unchanged; only attributes the reference changes on an
   existing Link / node move. Replaces a full openr_spf_set_graph at the reference's
   memo-clearing points when updateAdjacencyDatabase (LinkState.cpp:564-719) or
   decrementHolds (:500-514) changed nothing but:
     metric of directed edge e         Link::setMetricFromNode   (LinkState.cpp:195-204 getter)
     usability of link l (both edges)  Link::isUp: holds / adjacency overload (:233-236)
     overload of node x                LinkState::updateNodeOverloaded / isNodeOverloaded
   The patch is also recorded as a delta for openr_spf_refresh: the first patch after a
   refresh (or set_graph) starts a new delta, later patches with no refresh in between
   merge into it (each edge keeps its state from before the first of them). No solve may
   be in flight on the context's devices. */
typedef struct {
  uint32_t n_edges;
  const uint32_t* edge_ids;         /* [n_edges] directed edge ids */
  const uint64_t* metric;           /* [n_edges] new Link::getMetricFromNode(owner) */
  uint32_t n_links;
  const uint32_t* link_ids;         /* [n_links] */
  const uint8_t* link_up;           /* [n_links] new Link::isUp() */
  uint32_t n_nodes;
  const uint32_t* node_ids;         /* [n_nodes] */
  const uint8_t* node_overloaded;   /* [n_nodes] new isNodeOverloaded() */
} openr_spf_patch;

int openr_spf_patch_graph(openr_spf_ctx* ctx, const openr_spf_patch* patch);

/* Incremental re-SPF after openr_spf_patch_graph: rows [n] (dist, and nh / tight when
   non-NULL, laid out as openr_spf_solve writes them) hold the results of sources[0..n)
   on the graph before the delta (before the first patch since the last refresh); on
   return they hold the results on the patched graph, bit-exact with a fresh solve. Every
   refresh call of the same delta (e.g. one per batch of rows) sees the same delta. Only rows the patch can change are
   re-solved: row s is affected iff some changed directed edge u->v was tight for s
   before, or is usable with d_s(u) + w_new <= d_s(v) after (u expanding for s);
   *out_resolved (nullable) = rows re-solved (added to stats.spf_runs). Fails with
   OPENR_SPF_EINVAL when no patch followed the last set_graph. The host form splits the
   rows across devices like openr_spf_solve; the device form synchronizes `stream` once.
   Multi-device callers of the device form: the delta is per context, and any refresh
   ends its merging, so refresh the rows held on EVERY device before the next patch (a
   device whose rows skipped a delta would be refreshed against the later delta only and
   stay stale; the host LinkState mirror does this). */
int openr_spf_refresh(openr_spf_ctx* ctx, const uint32_t* sources, uint32_t n, uint32_t flags, uint64_t* dist,
                      uint8_t* nh, uint32_t nh_bytes, uint64_t* tight, uint32_t* out_resolved);
int openr_spf_refresh_device(openr_spf_ctx* ctx, int device_index, const uint32_t* d_sources, uint32_t n,
                             uint32_t flags, uint64_t* d_dist, uint8_t* d_nh, uint32_t nh_bytes,
                             uint64_t* d_tight, void* stream, uint32_t* out_resolved);

int openr_spf_get_stats(const openr_spf_ctx* ctx, openr_spf_stats_t* out);

#ifdef __cplusplus
}
#endif
#endif /* OPENR_SPF_H */
