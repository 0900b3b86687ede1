/* pgq_hip.h — C ABI of libpgq_hip.so: DuckPGQ's path-finding hot path on MI355X (gfx950).
 *
 * This is the drop-in boundary for the bodies of the reference's search UDFs.  Each entry point replaces
 * one reference function (file:line relative to the cwida/duckpgq-extension tree):
 *
 *   pgq_csr_upload            device mirror of `class CSR`                 src/include/duckpgq/core/utils/compressed_sparse_row.hpp:25-47
 *                             (called lazily, under csr_lock, by the first search UDF that sees the CSR;
 *                              built by create_csr_vertex/create_csr_edge  src/core/functions/scalar/csr_creation.cpp:86-198)
 *   pgq_csr_free              ~CSR() / DuckPGQState::QueryEnd / delete_csr   src/duckpgq_state.cpp:162-170, src/core/functions/scalar/csr_deletion.cpp:10-20
 *   pgq_iterativelength       IterativeLengthFunction                      src/core/functions/scalar/iterativelength.cpp:34-143
 *                             (also serves iterativelength2                src/core/functions/scalar/iterativelength2.cpp:33-130 — same results)
 *   pgq_shortestpath          ShortestPathFunction                         src/core/functions/scalar/shortest_path.cpp:43-207
 *   pgq_cheapest_path_length  CheapestPathLengthFunction                   src/core/functions/scalar/cheapest_path_length.cpp:138-163
 *   pgq_*_bulk_device         no reference counterpart: same semantics without the 2048-row chunk ceiling,
 *                             inputs/outputs resident in HBM (used by bench.py)
 *
 * Conventions
 *   - plain C, no exceptions, no C++ or torch types.  Every function returns PGQ_OK (0) or a negative
 *     pgq_status; pgq_last_error() gives the thread-local message of the last failure on this thread.
 *   - all entry points are thread-safe and re-entrant (DuckDB calls UDFs from many worker threads); a
 *     pgq_csr_t is immutable after upload and shared read-only.
 *   - pgq_vec_t is DuckDB's UnifiedVectorFormat as the UDFs consume it (iterativelength.cpp:57-64):
 *     row r reads data[sel ? sel[r] : r]; validity (uint64 words, bit set = valid, NULL = all valid) is
 *     indexed by that same selected position.
 *   - result validity masks are written for rows [0,n): bit set = valid.  The caller provides
 *     ceil(n/64) words.
 *   - ids are DuckDB rowids: dense 0..V-1.  Out-of-range src/dst (undefined behaviour in the reference,
 *     iterativelength.cpp:105,123) return PGQ_ERR_INVALID_ARG instead of corrupting memory.
 *   - the HIP extension is mandatory: without a usable gfx950 device every call fails with
 *     PGQ_ERR_NO_DEVICE.  There is no CPU fallback in this library.
 */
#ifndef PGQ_HIP_H
#define PGQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pgq_status {
	PGQ_OK = 0,
	PGQ_ERR_NO_DEVICE = -1,    /* no HIP device / runtime failure at init */
	PGQ_ERR_HIP = -2,          /* a HIP call failed; message has the hipError string */
	PGQ_ERR_OOM = -3,          /* device or host allocation failed */
	PGQ_ERR_INVALID_ARG = -4,  /* NULL handle, id out of range, bad weight type, ... */
	PGQ_ERR_NOT_WEIGHTED = -5, /* cheapest path on a CSR without weights ("Need to initialize CSR before doing cheapest path") */
	PGQ_ERR_UNSUPPORTED = -6   /* e.g. negative weights */
} pgq_status;

typedef struct pgq_csr pgq_csr_t; /* opaque: CSR resident in HBM */

typedef struct pgq_vec {
	const void *data;
	const uint32_t *sel;      /* nullable */
	const uint64_t *validity; /* nullable */
} pgq_vec_t;

/* weight types, same numbering as csr_get_w_type (src/core/functions/scalar/csr_get_w_type.cpp:16-36) */
#define PGQ_W_NONE 0
#define PGQ_W_INT64 1
#define PGQ_W_DOUBLE 2

/* ---- process ------------------------------------------------------------------------------------- */

/* Idempotent. device < 0: use env PGQ_DEVICE, else LOCAL_RANK, else 0. */
int pgq_init(int device);
int pgq_device_count(void);
/* Multi-GPU inside one process (SURVEY.md §8b `pgq_init(device_mask)`): enables several devices of this node for the
 * *_multi entry points; the first one is the device pgq_init binds (single-device calls keep using it).  Peer access
 * (xGMI) is enabled between them where the hardware allows.  pgq_init_devices accepts a repeated index (tests on a
 * one-GPU box). */
int pgq_init_devices(const int *devices, int n);
int pgq_init_mask(uint64_t device_mask);
int pgq_num_enabled_devices(void);
const char *pgq_last_error(void);
const char *pgq_version(void);

/* ---- CSR ------------------------------------------------------------------------------------------ */

/* Host arrays in the reference's layout: offsets = CSR::v (at least V+1 int64; the reference allocates
 * V+2), adj = CSR::e, edge_ids = CSR::edge_ids (nullable: slot index is used), w = CSR::w (int64) or
 * CSR::w_double (double) selected by w_type.  Only the first offsets[V] entries of adj/edge_ids/w are read
 * (the undirected CTE over-allocates).  The device copy stores int32 adjacency.
 * SCALE LIMITS of the device mirror (the reference's CSR holds int64 everywhere, compressed_sparse_row.hpp:34-35): a CSR
 * with V >= 2^31 - 1 vertices or E = offsets[V] >= 2^31 entries is REFUSED with PGQ_ERR_UNSUPPORTED by all three
 * upload / build entry points — vertex ids are int32 on the device, the padded lists of the pair-centric kernels are
 * addressed by 32-bit group indices, their queue entries hold 32-bit list positions.  Every BASELINE configuration is
 * inside (the largest, the SF100 reply forest at V = 2^28: E = 2.2 x 10^8).  One call takes at most 2^31 - 1 rows.
 * When the ~40 bytes per edge of the pair-centric layout do not fit in device memory the upload still succeeds and the
 * searches run without the pre-pass (same answers, slower on scattered pairs): pgq_csr_has_prepass_layout() tells. */
int pgq_csr_upload(int64_t V, const int64_t *offsets, const int64_t *adj, const int64_t *edge_ids, const void *w,
                   int w_type, pgq_csr_t **out);
/* pgq_csr_upload with flags.  PGQ_UPLOAD_LAZY_EDGE_IDS: the caller keeps `edge_ids` valid and unchanged until pgq_csr_free
 * (the reference's host CSR owns the vector for as long as the CSR exists: compressed_sparse_row.hpp:34-35, and the device
 * handle dies with it); the library then does NOT copy the E x 8 bytes at upload — iterativelength, cheapest_path_length and
 * the analytics never read edge ids — but on the first call that needs them (shortestpath, pgq_csr_download,
 * pgq_csr_replicate).  Half of a query's upload bytes, off the critical path of the binder's iterativelength filter
 * (match.cpp:658-671 runs it before any shortestpath call). */
#define PGQ_UPLOAD_LAZY_EDGE_IDS 1u
int pgq_csr_upload_ex(int64_t V, const int64_t *offsets, const int64_t *adj, const int64_t *edge_ids, const void *w,
                      int w_type, unsigned flags, pgq_csr_t **out);
/* Same, but the four arrays already live in device memory of the current device (they are copied). */
int pgq_csr_upload_device(int64_t V, const int64_t *d_offsets, const int64_t *d_adj, const int64_t *d_edge_ids,
                          const void *d_w, int w_type, pgq_csr_t **out);
/* CSR construction on the GPU from edge-table rows resident in HBM: what
 * create_csr_vertex + create_csr_edge (src/core/functions/scalar/csr_creation.cpp:86-198) compute, with the slot
 * order of the reference's single-threaded schedule (rows of one source keep their table order).  d_edge_id may be
 * NULL (row index is the edge id); d_w: int64 or double column per w_type. */
int pgq_csr_build_device(int64_t V, int64_t n_rows, const int64_t *d_src, const int64_t *d_dst,
                         const int64_t *d_edge_id, const void *d_w, int w_type, pgq_csr_t **out);
/* Copies the device CSR back in the reference's layout (int64); any pointer may be NULL.  get_csr_v/e/w analogue
 * (src/core/functions/table/pgq_scan.cpp:15-153) for the device-built CSR. */
int pgq_csr_download(const pgq_csr_t *csr, int64_t *offsets, int64_t *adj, int64_t *edge_ids, void *w);
/* Copies the device CSR (base arrays and everything derived at upload) to every other enabled device with peer copies
 * over xGMI: the CSR is replicated, the pairs are sharded (north_star).  Idempotent; replicas die with the handle. */
int pgq_csr_replicate(pgq_csr_t *csr);
int pgq_csr_free(pgq_csr_t *csr);
int64_t pgq_csr_num_vertices(const pgq_csr_t *csr);
int64_t pgq_csr_num_edges(const pgq_csr_t *csr);
int pgq_csr_w_type(const pgq_csr_t *csr);
int64_t pgq_csr_device_bytes(const pgq_csr_t *csr);
/* 1: the padded adjacency + slot descriptors of the pair-centric pre-pass were built at upload; 0: they were not (option
 * meet_layout = 0, or no memory for them): searches go through the lane batches only. */
int pgq_csr_has_prepass_layout(const pgq_csr_t *csr);
/* ids per 16-byte group of the lists the pre-pass's hop-count walks read: 6 (the bit-packed copy, 21-bit ids, V <= 2^21),
 * 5 (25-bit ids, V <= 2^25 with option meet_pack = 2) or 4 (the 32-bit padded lists: meet_pack = 0, larger graphs, no
 * layout); -1 for a NULL handle. */
int pgq_csr_pack_k(const pgq_csr_t *csr);
/* 1: the bit-packed lists were built in degree order (option meet_pack_order = 1 at upload, the default): every packed
 * list holds its entries by non-increasing floor(log2(length of the entry's own list in the OTHER direction)), equal buckets
 * in the CSR's order, and the hop-count walks read the first quarter of every list's groups before the rest.  0: the CSR's
 * order (meet_pack_order = 0, or no packed copy); -1 for a NULL handle.  Hop counts are the same either way. */
int pgq_csr_pack_order(const pgq_csr_t *csr);
/* Debugging / tests: the bit-packed list of vertex v, decoded, in the order the walks read it.  dir 0: the forward list
 * (out-neighbours), 1: the reverse list (in-neighbours).  Writes min(length, cap) ids to out (host memory) and returns the
 * length; PGQ_ERR_UNSUPPORTED for a CSR without a packed copy (pgq_csr_pack_k() == 4).  Not a fast path: it copies the
 * offsets up to v to the host. */
int64_t pgq_csr_packed_list(pgq_csr_t *csr, int dir, int64_t v, int32_t *out, int64_t cap);
/* Debugging / tests: the work partition the upload built for the bottom-up kernels of the lane batches, copied to host
 * memory.  pgq_csr_pull_layout_sizes writes sizes[0 .. 4] = {parts, hub slices, hub vertices, in-slots (= edges), 1 if the
 * packed in-slot words exist else 0}.  pgq_csr_pull_layout fills whichever buffers are not NULL: parts = (begin, end)
 * vertex pairs; hub_items = (vertex, begin, end) triples, the slices of the hubs' in-lists in vertex order; hub_vertices;
 * rown = one byte per in-slot, its owner vertex as an index inside its part (0 for a hub's slots); rpk = one word per
 * in-slot of a part, in-neighbour | owner index << 28, and 0 for a hub's slots, which are never read through it
 * (PGQ_ERR_UNSUPPORTED where V >= 2^28 and the words were not built).  Read-only: no
 * search path and no layout depends on these calls. */
int pgq_csr_pull_layout_sizes(const pgq_csr_t *csr, int64_t *sizes);
int pgq_csr_pull_layout(const pgq_csr_t *csr, int32_t *parts, int64_t *hub_items, int32_t *hub_vertices, uint8_t *rown,
                        uint32_t *rpk);
/* Debugging / tests: the layout the upload derives for the pair-centric and source-centric kernels, copied to host memory.
 * pgq_csr_meet_layout_sizes writes sizes[0 .. 10] = {16-byte groups of the forward padded adjacency, of the reverse one, of
 * the forward packed copy, of the reverse one (all four 0 when the handle has no layout, the packed two 0 without a packed
 * copy), ids per packed group (pgq_csr_pack_k), groups the packed lists are aligned to, pgq_csr_pack_order, 1 if the
 * fixed-stride in-list heads exist else 0, the largest out-degree, the largest in-degree, the bit pattern of the double
 * `mean over the vertices of in-degree x out-degree`}.  pgq_csr_meet_layout fills whichever buffers are not NULL for
 * direction 0 (forward: out-lists) or 1 (reverse: in-lists): offsets (V + 1); adj (E entries); seg = per vertex (first
 * group of its padded list, entries), 2 V words; padded = 4 words per group, a list's entries and then its last entry again
 * up to the end of its last alignment group; desc = per slot (neighbour, the neighbour's first group, its entries, its first
 * packed group or 0 without a packed copy), 4 E words; work = per vertex the entries of its two-hop walk, saturating at
 * 2^32 - 1; packed = 4 words per packed group (pgq_csr_packed_list decodes one list of it); rhead (dir 1 only) = 64 words per
 * vertex: word 31 the in-degree, words 0 .. 30 in-list entries 0 .. 30, words 32 .. 63 entries 31 .. 62, the last entry
 * repeated past the list's end, all ones for an empty list.  Only these defined parts are copied, not the spare entries the
 * device arrays carry behind them.  PGQ_ERR_UNSUPPORTED for a buffer whose array this handle does not have (no layout, no
 * packed copy, no heads, heads of direction 0).  Read-only: no search path and no layout depends on these calls. */
int pgq_csr_meet_layout_sizes(const pgq_csr_t *csr, int64_t *sizes);
int pgq_csr_meet_layout(const pgq_csr_t *csr, int dir, int64_t *offsets, int32_t *adj, uint32_t *seg, int32_t *padded,
                        uint32_t *desc, uint32_t *work, uint32_t *packed, uint32_t *rhead);
/* Debugging / tests: the hub tables the upload built for k_meet3 (options meet_hubs, meet_hub_min_degree, meet_hub_min_count,
 * meet_hub_mb), copied to host memory.  The hubs are the vertices with the most edges (out-degree + in-degree, at
 * least meet_hub_min_degree; ties to the smaller id), at most H of them; hub h is bit h & 63 of 64-bit word h >> 6 of a table
 * row, bits of unused slots are zero.  pgq_csr_hub_sizes writes sizes[0 .. 2] = {H, hubs in use, 64-bit words per row = H / 64}.
 * pgq_csr_hub_tables fills whichever buffers are not NULL: hub_ids (H entries, the hubs in bit order, -1 in unused slots) and
 * the four tables of V rows: hub1_out[v] bit h = an edge v -> h exists; hub1_in[v] bit h = an edge h -> v exists; hub2_out[v]
 * = OR of hub1_out over the out-neighbours of v; hub2_in[v] = OR of hub1_in over the in-neighbours of v.  replica < 0: the
 * handle's own tables; replica = k: those of the copy pgq_csr_replicate made for the k-th enabled device.
 * PGQ_ERR_UNSUPPORTED for a handle without tables.  Read-only: no search path depends on these calls. */
int pgq_csr_hub_sizes(const pgq_csr_t *csr, int64_t *sizes);
int pgq_csr_hub_tables(pgq_csr_t *csr, int replica, int32_t *hub_ids, uint64_t *hub1_out, uint64_t *hub1_in, uint64_t *hub2_out,
                       uint64_t *hub2_in);
/* Debugging / tests: device blocks the library's block cache has handed out and not got back yet (CSR arrays and build
 * temporaries of every live handle; cached free blocks, workspaces and pinned memory are not counted).  The same figure
 * before a handle is created and after it is freed = the handle left nothing behind. */
int64_t pgq_debug_live_device_blocks(void);

/* ---- searches, chunk form (host memory, UnifiedVectorFormat in, FLAT vector out) --------------------- */

/* iterativelength(csr_id, V, src, dst) -> BIGINT.  NULL src -> NULL (payload -1); src == dst -> 0; reachable
 * -> hop count; unreachable -> NULL (payload -1).  dst validity is ignored exactly like the reference.
 * Cost of one call (round 4): the columns are resolved into a pinned staging block of a pooled workspace that the
 * kernels read and write directly — two or three kernel launches and one wait, no copy commands (0.03 ms for one row,
 * 0.07 ms for 2048 rows on the SF100-shaped graph); re-entrant, every calling thread gets its own workspace and stream. */
int pgq_iterativelength(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t *out_len,
                        uint64_t *out_valid);

/* iterativelength(csr_id, V, src, dst, upper) -> BIGINT: pgq_iterativelength, except that a row whose hop count exceeds
 * max_hops is NULL (payload -1).  This is the call the binder's path-quantifier condition needs: AddPathQuantifierCondition
 * (src/core/functions/table/match.cpp:658-671) emits `iterativelength(...) BETWEEN lower AND upper` for every quantified edge
 * pattern, so whatever lies beyond `upper` is discarded by the filter — here the search stops there instead of running the
 * far and unreachable rows to exhaustion (the lower bound needs nothing from the search and stays with the filter).
 * src == dst -> 0 for every max_hops >= 0; max_hops >= V - 1 (INT64_MAX: the binder's "no upper bound") is the unbounded
 * search, same values as pgq_iterativelength; max_hops < 0 -> PGQ_ERR_INVALID_ARG.  Same staging path and cost per call. */
int pgq_iterativelength_within(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops,
                               int64_t *out_len, uint64_t *out_valid);

/* iterativelengthbidirectional(csr_id, V, src, dst) -> BIGINT (src/core/functions/scalar/iterativelength_bidirectional.cpp:43-153,
 * intended semantics: the reference's version is unreachable from the binder and indexes its backward CSR wrongly).
 * The same hop counts as pgq_iterativelength, found by one bidirectional BFS per row: forward over the CSR from src,
 * backward over the transposed CSR (built at upload) from dst, always expanding the cheaper side. */
int pgq_iterativelength_bidirectional(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst,
                                      int64_t *out_len, uint64_t *out_valid);

/* shortestpath(csr_id, V, src, dst) -> LIST(BIGINT) [src, e1, v1, ..., ek, dst].  list entries go to
 * out_offset/out_length (list_entry_t fields), the child payload to *out_child (owned by the library, valid
 * until the next pgq_shortestpath call on the same thread or pgq_thread_release).  NULL rows keep entry {0,0}. */
int pgq_shortestpath(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, uint64_t *out_offset,
                     uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child, uint64_t *out_child_len);

/* shortestpath(csr_id, V, src, dst, upper) -> LIST(BIGINT): pgq_shortestpath, except that a row whose path has more than
 * max_hops hops is NULL — validity bit clear, entry {0,0}, and NO elements in the child payload: *out_child_len counts the
 * lists of the rows within the bound only.  The binder computes shortestpath over the very pairs it filters with
 * `iterativelength(...) BETWEEN lower AND upper` (match.cpp:467-495, 658-671), so a row beyond `upper` is NULL to the query
 * anyway; here its search stops at the bound and no level frontier is kept for a list nobody reads.  src == dst -> [src]
 * for every max_hops >= 0; max_hops >= V - 1 (INT64_MAX: the binder's "no upper bound") is the unbounded search, same lists,
 * lengths and payload as pgq_shortestpath; max_hops < 0 -> PGQ_ERR_INVALID_ARG. */
int pgq_shortestpath_within(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops,
                            uint64_t *out_offset, uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child,
                            uint64_t *out_child_len);

/* cheapest_path_length(csr_id, V, src, dst) -> BIGINT | DOUBLE (by the CSR's weight type; out is int64_t* or
 * double*).  NULL src, NULL dst or unreachable -> NULL. */
int pgq_cheapest_path_length(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, void *out,
                             uint64_t *out_valid);

/* cheapest_path_length(csr_id, V, src, dst, upper) -> BIGINT | DOUBLE: the cost of the cheapest walk src -> dst of AT MOST
 * max_hops edges, for a quantified edge pattern with an upper bound (match.cpp:658-671).  With INF = numeric_limits<T>::max() / 2
 * (cheapest_path_length.cpp:15) the result is D_K[dst], K = max_hops, of
 *     D_0[src] = 0, D_0[v] = INF otherwise;   D_k[n] = min(D_{k-1}[n], min over edges (u, n) of D_{k-1}[u] + w(u, n))
 * — the sum is the reference's `dist[v] + w` (cheapest_path_length.cpp:29-36) and counts only where it is < D_{k-1}[n] — and NULL
 * when D_K[dst] == INF.  For non-negative weights that is the minimum, over the walks of at most K edges, of the left-to-right
 * fold of their weights, bit for bit, for int64 and for double.  NaN and +inf weights never relax an edge, -0.0 is accepted.
 * WARNING: this is NOT pgq_cheapest_path_length with far rows set to NULL.  The cheapest walk of at most K edges is in general a
 * different walk from the unbounded cheapest one and costs more; no filter around the unbounded call can produce it.  The
 * reference has no counterpart either: its Bellman-Ford sweeps in place, so its rounds are not hops.
 * NULL src or NULL dst -> NULL; src == dst -> 0 (+0.0) for every max_hops >= 0; max_hops >= V - 1 (INT64_MAX: the binder's "no
 * upper bound") is the unbounded search, the same bits as pgq_cheapest_path_length; max_hops < 0 -> PGQ_ERR_INVALID_ARG.  An
 * unweighted CSR, negative weights and ids out of range fail as in pgq_cheapest_path_length. */
int pgq_cheapest_path_length_within(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops, void *out,
                                    uint64_t *out_valid);

/* cheapest_path(csr_id, V, src, dst) -> LIST(BIGINT) [src, e1, v1, ..., ek, dst]: the cheapest path itself, next to the cost
 * pgq_cheapest_path_length returns (the reference has no counterpart: its Bellman-Ford keeps no parents).  With D[v] the labels
 * pgq_cheapest_path_length defines (the least fixpoint of dist[n] = min(dist[n], dist[v] + w) from dist[src] = 0, INF = max(T) / 2,
 * the reference's arithmetic for int64 and for double):
 *   - a slot s of u's out-list with adj[s] = x is TIGHT when D[u] < INF and D[u] + w[s] == D[x], computed as the relaxation
 *     computes it; NaN and +inf weights are never tight;
 *   - H[src] = 0 and H[x] = 1 + min H[u] over the tight slots (u, x): the BFS levels of the tight subgraph;
 *   - for a row with D[dst] < INF and k = H[dst]: x_k = dst, and for i = k .. 1, x_{i-1} = the smallest u with H[u] = i - 1 that
 *     has a tight slot into x_i (shortestpath's min-parent rule), e_i = edge_ids[the first tight slot of that u into x_i]
 *     (shortestpath's first-slot rule among the tight slots); the list is [x_0, e_1, x_1, ..., e_k, x_k].
 * The path is hop-minimal among the cheapest ones, so zero-weight cycles and absorbed double edges (2^53 + 1.0 == 2^53) cannot
 * make it loop.  The left-to-right fold of the weights of e_1 .. e_k is pgq_cheapest_path_length's result, bit for bit; when every
 * weight is the same positive int64 the list is pgq_shortestpath's.  src == dst -> [src]; NULL src, NULL dst or unreachable ->
 * NULL (validity clear, entry {0,0}, no payload).  Signature and thread-local child arena as pgq_shortestpath (the arena is the
 * same one: valid until the next list-returning call on the thread).  An unweighted CSR, negative weights and ids out of range fail
 * as in pgq_cheapest_path_length.  The hop-bounded form is pgq_cheapest_path_within; there is no _multi form, and the two-ended
 * search is not used. */
int pgq_cheapest_path(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, uint64_t *out_offset,
                      uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child, uint64_t *out_child_len);

/* cheapest_path(csr_id, V, src, dst, upper) -> LIST(BIGINT) [src, e1, v1, ..., eh, dst]: the cheapest walk of AT MOST max_hops
 * edges itself, next to the cost pgq_cheapest_path_length_within returns (the reference has no counterpart).  With D_0 .. D_K the
 * labels that call defines for the row's source and K = max_hops, every sum computed as the relaxation computes it:
 *   - NULL when D_K[dst] == INF, or src or dst is NULL; src == dst -> [src] for every K >= 0;
 *   - h = the smallest k with D_k[dst] == D_K[dst] as bit patterns: the fewest edges among the cheapest walks of at most K edges;
 *   - x_h = dst, and for i = h .. 1, x_{i-1} = the smallest u with D_{i-1}[u] < INF and a slot (u, x_i) whose
 *     D_{i-1}[u] + w[s] == D_i[x_i], e_i = edge_ids[the first such slot of u's out-list into x_i] (shortestpath's min-parent and
 *     first-slot rules); NaN and +inf weights are never tight; the list is [x_0, e_1, x_1, ..., e_h, x_h] with x_0 = src.
 * WARNING: this is NOT pgq_cheapest_path's list with rows of more than max_hops edges set to NULL: the cheapest walk of at most K
 * edges is in general another walk than the cheapest one.  The left-to-right fold of the weights of e_1 .. e_h is
 * pgq_cheapest_path_length_within's result, bit for bit, and h <= max_hops; when every weight is the same positive int64 the list
 * is pgq_shortestpath_within's.  max_hops >= V - 1 changes nothing any more (D_k stands still from V - 1 on): for int64 weights
 * the list is then pgq_cheapest_path's; for DOUBLE weights the two CAN DIFFER, where a label absorbs a difference — with edges
 * 0->2 (1.0), 0->1 (0.25), 1->2 (0.25), 2->3 (2^53) this call answers the two-hop walk 0, 2, 3 for every max_hops >= 2
 * (1.0 + 2^53 == 0.5 + 2^53: the third round improves nothing), pgq_cheapest_path the three-hop path through vertex 1; both fold
 * to 2^53.  max_hops < 0 -> PGQ_ERR_INVALID_ARG.  Signature, arena and NULL conventions as pgq_cheapest_path; an unweighted CSR,
 * negative weights and ids out of range fail as in pgq_cheapest_path_length.  The search keeps a log of every round's changed
 * label rows (rounds x changed vertices x 528 bytes per 64 sources): PGQ_ERR_OOM when it cannot be allocated, PGQ_ERR_UNSUPPORTED
 * beyond 2^31 entries, no list written in either case.  No _multi form. */
int pgq_cheapest_path_within(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops,
                             uint64_t *out_offset, uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child,
                             uint64_t *out_child_len);

/* cheapest_walk_length(csr_id, V, src, dst, lower, upper) -> BIGINT / DOUBLE and cheapest_walk(csr_id, V, src, dst, lower, upper)
 * -> LIST(BIGINT): the cost and the list of the cheapest WALK of lower..upper edges — what a weighted -[e]->{lower,upper} needs in
 * WALK mode (the reference has no counterpart).  A filter around the _within calls is wrong twice: a row whose cheapest walk of at
 * most `upper` edges has fewer than `lower` edges may well have a costlier walk of lower..upper edges, and that walk is the answer;
 * and src == dst is answered 0 / [src] where the pattern asks for a closed walk.  With lo = min_hops, K = max_hops, INF = max(T) / 2,
 * every sum computed as the relaxation computes it (`dist[v] + w`, cheapest_path_length.cpp:29-36; it counts only below INF; NaN and
 * +inf weights never relax an edge and are never tight, -0.0 is accepted):
 *     E_0[src] = 0, E_0[v] = INF otherwise
 *     E_t[x]   = min over the in-slots (u, x) with E_{t-1}[u] < INF of E_{t-1}[u] + w     t = 1 .. lo  (INF if none: NO carry-over of E_{t-1}[x])
 *     L_lo     = E_lo
 *     L_t[x]   = min(L_{t-1}[x], min over the in-slots (u, x) of L_{t-1}[u] + w)          t = lo + 1 .. K  (the _within recurrence)
 * E_t[x] is the minimum over the walks of exactly t edges of the left-to-right fold of their weights, L_t[x] that minimum over
 * the walks of lo..t edges, bit for bit, for int64 and for double (x -> x + w is monotone for a fixed non-negative w).
 *   pgq_cheapest_walk_length  L_K[dst]; NULL when that is INF or when src or dst is NULL.
 *   pgq_cheapest_walk         [x_0, e_1, x_1, ..., e_h, x_h] in shortestpath's layout, the empty walk [src]: h = the smallest t in
 *                             [lo, K] with L_t[dst] == L_K[dst] as bit patterns (the fewest edges among the cheapest walks of lo..K
 *                             edges).  With Λ_i = E_i for i <= lo and L_i for i > lo: x_h = dst, and for i = h .. 1, x_{i-1} = the
 *                             smallest u with Λ_{i-1}[u] < INF and a slot (u, x_i) with Λ_{i-1}[u] + w[s] == Λ_i[x_i], e_i =
 *                             edge_ids[the first such slot of u's out-list into x_i] (shortestpath's min-parent and first-slot rules).
 * src == dst is NOT special, as in pgq_walk_length: with lo == 0 the row is 0 (+0.0) / [src], otherwise the cheapest closed walk of
 * lo..K edges; a vertex without an out-edge or without an in-edge gives NULL for lo >= 1.
 * Identities: (1) lo == 0 is exactly pgq_cheapest_path_length_within(K) / pgq_cheapest_path_within(K) — values, validity, lists and
 * payload; the calls forward.  (2) The left-to-right fold of the list's edge weights is pgq_cheapest_walk_length's value bit for bit,
 * and lo <= h <= K.  (3) Where pgq_cheapest_path_within(K)'s h is at least lo, the value is the _within value; with int64 weights
 * the list is that call's list too, with DOUBLE weights an absorbed sum can make the lists differ (README).  (4) With one positive
 * int64 weight c on every edge and K <= 64 the value is c x pgq_walk_length(lo, K) with the same NULLs, and the list is walk 0 of
 * pgq_k_shortest_walks(lo, K, k = 1).
 * min_hops < 0 or max_hops < min_hops -> PGQ_ERR_INVALID_ARG.  min_hops > PGQ_WALK_MAX_HOPS -> PGQ_ERR_UNSUPPORTED (in a cyclic graph
 * the exact rounds never run dry, so `lo` rounds over everything reached need a limit).  max_hops may be anything from min_hops
 * up, INT64_MAX = no upper bound: the rounds behind lo are Bellman-Ford from E_lo, stand still after at most V - 1 of them and end
 * with the queue; a large max_hops is NOT forwarded to the unbounded search when lo >= 1.  An unweighted CSR, negative weights,
 * ids out of range and a V mismatch fail as in pgq_cheapest_path_length_within; a NULL handle -> PGQ_ERR_INVALID_ARG ("NULL csr")
 * before any device is asked for; a failed call has written nothing.  The list call keeps pgq_cheapest_path_within's log errors
 * (PGQ_ERR_OOM, PGQ_ERR_UNSUPPORTED beyond 2^31 entries), and its log is larger: the exact rounds log everything they reach in every
 * round (lo x reached vertices x 528 bytes per 64 sources on top).  pgq_stats_t: `levels` counts the rounds of both phases.
 * Outputs as pgq_cheapest_path_length_within / pgq_cheapest_path_within.  Not built: _multi forms, a heavy-list split, a
 * destination bound, the path modes, a two-ended search, forwarding upper - lower >= V - 1 to the unbounded rounds. */
int pgq_cheapest_walk_length(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops,
                             void *out, uint64_t *out_valid);
int pgq_cheapest_walk(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops,
                      uint64_t *out_offset, uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child,
                      uint64_t *out_child_len);

/* shortestpath_count(csr_id, V, src, dst, upper) -> BIGINT and all_shortestpaths(csr_id, V, src, dst, upper, max_paths) ->
 * LIST(LIST(BIGINT)): what SQL/PGQ's ALL SHORTEST needs (the reference's binder rejects the form: "ALL SHORTEST has not been
 * implemented yet", match.cpp:82).  Both are hop-bounded: max_hops = INT64_MAX or >= V - 1 means no bound, max_hops < 0 ->
 * PGQ_ERR_INVALID_ARG.  Both work on any CSR and ignore weights.  For a row (src, dst), with L[v] the BFS level of v from src and
 * d = L[dst]:
 *     sigma[src] = 1;   sigma[x] = min(INT64_MAX, sum of sigma[u] over the in-slots (u, x) with L[u] = L[x] - 1)
 * Parallel edges are separate slots and count separately (a path is a sequence of edges, as in shortestpath's list); the sum
 * saturates at 2^63 - 1 and never wraps.
 *   - pgq_shortestpath_count: sigma[dst]; 1 for src == dst; 0 when dst is unreachable or d > max_hops; NULL (payload -1) for a
 *     NULL src or a NULL dst.
 *   - pgq_all_shortestpaths: a row's list holds its first min(sigma[dst], max_paths) shortest paths, each in shortestpath's
 *     layout [src, e1, v1, ..., ed, dst].  Order: compare two paths from the destination end, first by (x_{d-1}, forward slot of
 *     e_d), then by (x_{d-2}, slot of e_{d-1}), and so on — the lexicographic order of in-list positions (an in-list is ordered by
 *     parent id, then forward slot).  Path number r is found by unranking: start at x_d = dst with rank r; scan the in-list of x_t in
 *     its stored order, and for every in-slot (u, x_t) with L[u] = t - 1: if r < sigma[u] take that slot, otherwise r -= sigma[u].
 *     The taken in-slot is the m-th in-slot from u into x_t; its edge is the m-th slot of u's out-list whose target is x_t.
 *     Path 0 is therefore pgq_shortestpath's list; with max_paths = 1 the call returns pgq_shortestpath_within's lists, validity
 *     and payload, wrapped one level deeper.  src == dst -> [[src]].  NULL src, NULL dst, unreachable dst or d > max_hops -> NULL:
 *     no inner list, no payload.  max_paths < 1 -> PGQ_ERR_INVALID_ARG.  A call that would emit more than 2^31 - 1 paths returns
 *     PGQ_ERR_UNSUPPORTED and writes nothing.  A saturated sigma stays valid for unranking: every emitted rank is below 2^31.
 * Outer entry i = {out_first[i], out_npaths[i]} into the inner entries {(*out_path_offset)[k], (*out_path_length)[k]},
 * k < *out_path_total, which index *out_child.  The inner entries and the child live in the thread's result arena: valid until
 * the next list-returning call on that thread.  NULL rows keep the outer entry {0, 0}.
 * Workspace: about 768 bytes per vertex (hop counts and sigma of one batch of 64 sources); PGQ_ERR_OOM with nothing written when
 * it cannot be had.  A NULL handle is answered with PGQ_ERR_INVALID_ARG ("NULL csr") before any device is asked for.
 * NOT BUILT: _multi forms; splitting long in-lists over several wavefronts (a list is walked by one wavefront); sharing prefixes
 * between the paths of one row; any change to how shortestpath or iterativelength are routed. */
int pgq_shortestpath_count(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops, int64_t *out_count,
                           uint64_t *out_valid);
int pgq_all_shortestpaths(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops, int64_t max_paths,
                          uint64_t *out_first, uint64_t *out_npaths, uint64_t *out_valid, const uint64_t **out_path_offset,
                          const uint64_t **out_path_length, uint64_t *out_path_total, const int64_t **out_child,
                          uint64_t *out_child_len);

/* walk_count(csr_id, V, src, dst, lower, upper) -> BIGINT and k_shortest_walks(csr_id, V, src, dst, lower, upper, k) ->
 * LIST(LIST(BIGINT)): the walks a quantified pattern -[e]->{lower,upper} matches in WALK mode, and SQL/PGQ's SHORTEST k over them
 * (the reference's binder rejects TopK, match.cpp:82-98, and filters {lower,upper} with iterativelength BETWEEN lower AND upper,
 * match.cpp:658-671, which drops a pair at distance 1 that also has a walk of 2 edges from {2,3} and never finds a cycle).  Both
 * work on any CSR and ignore weights.  For a row (src, dst), lo = min_hops, K = max_hops, over the forward CSR's slots (parallel
 * edges are separate slots):
 *     W_0[v] = 1 if v == src else 0
 *     W_t[x] = min(INT64_MAX, sum of W_{t-1}[u] over ALL in-slots (u, x))      t = 1 .. K
 *     count  = min(INT64_MAX, sum of W_t[dst] for t = lo .. K)
 * The sums saturate at 2^63 - 1 and never wrap.
 *   - pgq_walk_count: count, 0 when there is no such walk.  src == dst is not special: it counts the empty walk when lo == 0 and
 *     every closed walk of lo..K edges.  NULL (payload -1) for a NULL src or a NULL dst.
 *   - pgq_k_shortest_walks: a row's list holds its first min(count, k) walks, each in shortestpath's layout
 *     [x_0, e_1, x_1, ..., e_t, x_t]; the empty walk is [src].  Shorter walks come first; walks of equal length t are ordered by
 *     in-list positions read from the destination end: pgq_all_shortestpaths' order with "W_{i-1}[u] > 0" in place of
 *     "L[u] = i - 1" and W_{i-1}[u] in place of sigma[u].  Walk number r of a row:
 *       1. take the smallest t >= lo with r < W_t[dst], after subtracting W_t[dst] of the shorter lengths from r;
 *       2. start at x_t = dst; for i = t .. 1 scan x_i's in-list in stored order; for each in-slot (u, x_i): if r < W_{i-1}[u] take
 *          it, otherwise r -= W_{i-1}[u];
 *       3. the taken in-slot is the m-th from u into x_i; its edge is the m-th slot of u's out-list whose target is x_i.
 *     A saturated W stays valid for unranking: every emitted rank is below 2^31.  Consequence: for src != dst, d = dist(src, dst)
 *     and lo <= d <= K the walks of length d come first and are exactly pgq_all_shortestpaths' lists in its order, so walk 0 is
 *     pgq_shortestpath's list.  A row with count 0, or with a NULL endpoint, is NULL: outer entry {0, 0}, no inner list, no payload.
 * min_hops < 0, max_hops < min_hops or k < 1 -> PGQ_ERR_INVALID_ARG.  max_hops > PGQ_WALK_MAX_HOPS -> PGQ_ERR_UNSUPPORTED (this
 * includes INT64_MAX, the binder's "no upper bound"): walks need an upper bound, in a cyclic graph their number is unbounded (what
 * match.cpp:100-104 says about ALL with WALK).  More than 2^31 - 1 emitted walks in one call -> PGQ_ERR_UNSUPPORTED, nothing
 * written.  A NULL handle is answered with PGQ_ERR_INVALID_ARG ("NULL csr") before any device is asked for.
 * Outputs as pgq_all_shortestpaths (the walks of one row differ in length: (*out_path_length)[k] says how many elements walk k
 * has); the inner entries and the child live in the thread's result arena.  A failed call has written nothing to the caller.
 * The rounds of the list form stop once no row of a batch of 64 sources is short of k walks (k = 1 on a pair d apart costs d
 * rounds, not K); pgq_walk_count runs every round up to K or to the round that activates no vertex.
 * Workspace per batch of 64 sources: pgq_walk_count two rounds (1040 bytes per vertex); pgq_k_shortest_walks every round it runs,
 * 0..K at most, for the unranking: 520 bytes per vertex and round; PGQ_ERR_OOM with nothing written when it cannot be had.
 * NOT BUILT: _multi forms; splitting long in-lists over several wavefronts (a list is walked by one wavefront); any change to how
 * the binder's iterativelength filter is emitted.  The path modes are the _mode calls below, SHORTEST k GROUP is
 * pgq_k_shortest_groups. */
#define PGQ_WALK_MAX_HOPS 64
int pgq_walk_count(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops,
                   int64_t *out_count, uint64_t *out_valid);
int pgq_k_shortest_walks(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops,
                         int64_t k, uint64_t *out_first, uint64_t *out_npaths, uint64_t *out_valid, const uint64_t **out_path_offset,
                         const uint64_t **out_path_length, uint64_t *out_path_total, const int64_t **out_child,
                         uint64_t *out_child_len);

/* walk_length(csr_id, V, src, dst, lower, upper) -> BIGINT: the length of the shortest walk of lower..upper edges — with W_t as
 * above, the smallest t in [min_hops, max_hops] with W_t[dst] > 0.  `walk_length(...) IS NOT NULL` is the filter a quantified pattern
 * -[e]->{lower,upper} needs in WALK mode (the reference's iterativelength BETWEEN lower AND upper is wrong for walks, see above).
 *   - NULL (payload -1) when there is no such t, or when src or dst is NULL.
 *   - src == dst is not special: 0 when min_hops == 0, otherwise the length of the shortest closed walk of at least min_hops edges.
 *   - Any CSR; weights are ignored; parallel edges change nothing.
 * Three identities hold: the result equals pgq_k_shortest_walks_bulk_device(k = 1)'s d_out_len; it is non-NULL exactly where
 * pgq_walk_count > 0; for min_hops <= dist <= max_hops it equals pgq_iterativelength_within(max_hops), and for min_hops == 0 it
 * equals that call on every row.
 * min_hops < 0 or max_hops < min_hops -> PGQ_ERR_INVALID_ARG.  max_hops > PGQ_WALK_MAX_HOPS (INT64_MAX included) ->
 * PGQ_ERR_UNSUPPORTED with pgq_walk_count's text: a larger or unbounded upper is NOT BUILT.  A NULL handle is answered with
 * PGQ_ERR_INVALID_ARG ("NULL csr") before any device is asked for; ids out of range fail as in the other walk calls.  A failed
 * call has written nothing.
 * How: the distance d first, by pgq_iterativelength_within's routes under max_hops (off the route memo's record): min_hops <= d <=
 * max_hops answers d, d > max_hops or unreachable answers NULL.  Only the rows with d < min_hops (every src == dst row when
 * min_hops >= 1) go through rounds, in batches of 64 sources: one 8-byte mask word per vertex and round, two mask arrays and two
 * queues per batch (24 bytes per vertex; PGQ_ERR_OOM with nothing written when they cannot be had), no visited set.  The rounds
 * stop behind round max_hops, when no row of the batch is open, or when nothing is active.  Option "walk_length_pull": 0 = every
 * round top-down (pgq_walk_count's activation kernel), 1 = every round bottom-up over the upload's work partition (hubs slice by
 * slice), 2 (shipped) = bottom-up once the queue's out-edges exceed E / "walk_length_pull_div", and from then on.  pgq_stats_t:
 * batches / levels / push_levels / pull_levels / edges_scanned count these rounds alone (not the distance stage's own search).
 * NOT BUILT: _multi forms, a boolean-only form, the path modes, rounds enqueued ahead of the host. */
int pgq_walk_length(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops,
                    int64_t *out_len, uint64_t *out_valid);

/* k_shortest_walks_mode / walk_count_mode: SHORTEST k and a limited count under SQL/PGQ's path modes (the reference's binder rejects
 * every mode but WALK, match.cpp:80-108, and tells its users to pick one when ALL explodes on a cyclic graph, match.cpp:100-104).
 * The modes are numbered as the reference's PGQPathMode (subpath_element.hpp:9); any other value is PGQ_ERR_INVALID_ARG.
 * For a row (src, dst), lo = min_hops, K = max_hops, let S be the whole sequence pgq_k_shortest_walks would list with unlimited k:
 * every walk of lo..K edges, shortest first, equal lengths ordered by in-list positions from the destination end.  A walk
 * [x_0, e_1, x_1, ..., e_t, x_t] is ADMITTED by a mode when, judged on the list itself:
 *   PGQ_MODE_ACYCLIC  no two of x_0 .. x_t are equal.  For src == dst only the empty walk is admitted.
 *   PGQ_MODE_SIMPLE   no two of x_0 .. x_t are equal, except that x_0 == x_t is allowed: a self-loop [a, e, a] and a ring back to its
 *                     start are simple.
 *   PGQ_MODE_TRAIL    no two of e_1 .. e_t are equal, compared as the list's elements (edge_ids[slot], or the slot when the CSR has
 *                     no edge ids).  Parallel slots with different ids are different edges; the two slots the binder's undirected CTE
 *                     gives one edge share an id, so a trail cannot go back over it (GQL's meaning).  Ids are taken to be shared by
 *                     an edge's two directions at most: then every walk of dist(src, dst) edges is a trail.
 *   PGQ_MODE_NONE / PGQ_MODE_WALK  every walk.
 *   - pgq_k_shortest_walks_mode: a row's list is the first min(a, k) admitted walks of S, in S's order, a being the number of
 *     admitted walks — NOT the admitted ones among the first k of S.  Outputs, arena and NULL conventions as pgq_k_shortest_walks.
 *     A row with no admitted walk, or with a NULL endpoint, is NULL: outer entry {0, 0}, no inner list, no payload.
 *   - pgq_walk_count_mode: min(a, limit); NULL (payload -1) for a NULL endpoint.  The same search with nothing emitted.  There is
 *     no unlimited count: counting simple paths is #P-hard, so the count is only ever taken up to a limit.
 * With path_mode NONE or WALK both calls go to the existing code and return exactly what pgq_k_shortest_walks and
 * min(pgq_walk_count, limit) return.
 * min_hops < 0, max_hops < min_hops, k < 1 or limit < 1 -> PGQ_ERR_INVALID_ARG.  max_hops > PGQ_WALK_MAX_HOPS (INT64_MAX included) ->
 * PGQ_ERR_UNSUPPORTED: an unbounded upper under a mode, finite though the answer would be, is NOT BUILT.  A NULL handle ->
 * PGQ_ERR_INVALID_ARG before any device is asked for.  More than 2^31 - 1 emitted walks -> PGQ_ERR_UNSUPPORTED.  A failed call has
 * written nothing to the caller.
 * How: the rounds of pgq_k_shortest_walks with every round's table kept, then a depth-first search per row from the destination over
 * the stored in-list order, pruned by the tables (a parent must still reach the source in exactly the edges left) and by the mode's
 * test on the partial walk; a counting pass, then an emitting pass.  The walks of d = dist(src, dst) edges are admitted by every mode,
 * so a row with lo <= d is settled once W_d[dst] >= k and the rounds of a batch stop when all its rows are (k = 1 on a pair d >= lo
 * apart costs d rounds); every other row keeps them going to round K.
 * WORK LIMIT: finding a simple path of an exact length is NP-hard, a row's search can take exponentially long.  Option
 * "mode_step_cap" (pgq_set_option / pgq_csr_set_option; shipped 2^24, a safety limit, not a tuned number) bounds the steps of one row
 * in one pass, a step being one 64-entry in-list chunk examined or one descent; a row beyond it ends the call with
 * PGQ_ERR_UNSUPPORTED, pgq_last_error() names the cap, nothing is written.  pgq_debug_mode_steps gives the steps the calling thread's
 * last mode call took: their sum over rows and passes, and the most one row took in one pass (both 0 under NONE / WALK).
 * NOT BUILT: _multi forms; an unbounded upper; an unlimited count; a smarter prune than the walk tables (they admit a parent that
 * reaches the source only through the stack); several wavefronts per row. */
#define PGQ_MODE_NONE 0
#define PGQ_MODE_WALK 1
#define PGQ_MODE_SIMPLE 2
#define PGQ_MODE_TRAIL 3
#define PGQ_MODE_ACYCLIC 4
int pgq_walk_count_mode(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops,
                        int64_t limit, int path_mode, int64_t *out_count, uint64_t *out_valid);
int pgq_k_shortest_walks_mode(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops,
                              int64_t k, int path_mode, uint64_t *out_first, uint64_t *out_npaths, uint64_t *out_valid,
                              const uint64_t **out_path_offset, const uint64_t **out_path_length, uint64_t *out_path_total,
                              const int64_t **out_child, uint64_t *out_child_len);
int pgq_debug_mode_steps(int64_t *total, int64_t *row_max);

/* k_shortest_groups(csr_id, V, src, dst, lower, upper, groups, max_paths, path_mode) -> LIST(LIST(BIGINT)): SQL/PGQ's SHORTEST k
 * GROUP — every path of the k smallest distinct lengths a row has (the reference's parser carries the selector next to topk,
 * PathPattern::group, path_pattern.hpp:22; its binder rejects it with TopK, match.cpp:80-108).  pgq_k_shortest_walks(k) cuts in the
 * middle of a length and pgq_all_shortestpaths knows one length only.  For a row (src, dst), lo = min_hops, K = max_hops,
 * g = groups, P = max_paths and a path_mode numbered as PGQ_MODE_*:
 *   S            the sequence pgq_k_shortest_walks_mode defines for that mode with unlimited k: every admitted walk of lo..K edges,
 *                shortest first, equal lengths ordered by in-list positions read from the destination end.  NONE and WALK admit
 *                every walk.
 *   the lengths  t_1 < t_2 < ...: the lengths in [lo, K] that have at least one admitted walk.  A length whose W_t[dst] is 0 is no
 *                group; under a mode a length all of whose walks the mode refuses is no group; lengths below lo are no groups.
 *   A            the admitted walks of lengths t_1 .. t_min(g, number of lengths): a prefix of S that ends on a group boundary.
 *   the list     the first min(|A|, P) walks of A, each in shortestpath's layout.  P is a cap, as max_paths is in
 *                pgq_all_shortestpaths; when it cuts it may cut inside a group, which is emitted as far as P goes.
 * Per row: npaths = min(|A|, P); ngroups = the distinct lengths among the emitted walks (a cut-off group counts);
 * count = min(|A|, P + 1), computed without overflow, so count > npaths exactly when the cap cut the row's answer; len = the hops
 * of the first walk, -1 when there is none.  A row with no admitted walk, or with a NULL endpoint, is NULL: outer entry {0, 0}, no
 * inner list, no payload, ngroups 0, count 0 (no walk) or -1 (NULL endpoint).  src == dst is not special, as in
 * pgq_k_shortest_walks: with lo == 0 the empty walk [src] is group 1, and under ACYCLIC the only group.
 * Consequences: g = 1 under NONE / WALK with src != dst and lo <= dist <= K gives pgq_all_shortestpaths(max_hops = K, max_paths = P)'s
 * lists in its order; g >= K - lo + 1 gives pgq_k_shortest_walks_mode(k = P)'s lists under every mode; P = 1 with lo <= dist gives
 * pgq_shortestpath's list as walk 0.
 * Errors as pgq_k_shortest_walks_mode for the arguments it shares; groups < 1 or max_paths < 1 -> PGQ_ERR_INVALID_ARG; max_hops >
 * PGQ_WALK_MAX_HOPS -> PGQ_ERR_UNSUPPORTED; more than 2^31 - 1 emitted walks -> PGQ_ERR_UNSUPPORTED; "mode_step_cap" bounds a row's
 * steps per pass as there (the counting pass looks for P + 1 walks) and pgq_debug_mode_steps reports this call's steps too.  A NULL
 * handle fails before any device is asked for.  A failed call has written nothing.
 * How: NONE / WALK — pgq_k_shortest_walks' rounds; a row is open while it has seen fewer than g non-empty lengths and their walks'
 * saturating sum is <= P (not < P: on a boundary a later non-empty length still makes count P + 1), a batch's rounds stop when no
 * row is open; A is a prefix of S, so a rank means the same walk and the unranking serves as it is.  Under a mode — the search of
 * pgq_k_shortest_walks_mode; a length is a group once it yields an admitted walk and a row's search ends behind the length that
 * completed group g, or at P + 1 walks; a row is settled at its distance d when lo <= d and g == 1 or W_d[dst] > P, every other
 * row keeps its batch going to round K.  Outputs as pgq_k_shortest_walks_mode plus out_ngroups (n entries).
 * NOT BUILT: _multi forms; a count-only form; an unbounded upper; several wavefronts per row; a split of long in-lists. */
int pgq_k_shortest_groups(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops,
                          int64_t groups, int64_t max_paths, int path_mode, uint64_t *out_first, uint64_t *out_npaths,
                          uint64_t *out_ngroups, uint64_t *out_valid, const uint64_t **out_path_offset,
                          const uint64_t **out_path_length, uint64_t *out_path_total, const int64_t **out_child,
                          uint64_t *out_child_len);

void pgq_thread_release(void); /* drop this thread's result arena */
/* Frees the pooled per-call workspaces (search state sized by V x lanes is kept between calls for reuse) and the
 * freed CSR / upload blocks kept for the next upload (PGQ_ALLOC_CACHE_MB). */
int pgq_release_cached_memory(void);

/* ---- searches, bulk form (device memory, no chunk ceiling) ---------------------------------------------- */

/* d_src/d_dst/d_out_len: n int64 each in HBM.  d_out_len[i] = hop count, 0 for src==dst, -1 for NULL. */
int pgq_iterativelength_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst,
                                    int64_t *d_out_len);
/* pgq_iterativelength_within without the chunk ceiling (match.cpp:658-671: the pattern's upper bound): d_out_len[i] = hop
 * count when it is at most max_hops, 0 for src == dst, -1 for NULL rows, unreachable rows and rows farther apart. */
int pgq_iterativelength_within_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst,
                                           int64_t max_hops, int64_t *d_out_len);
/* the same rows through one bidirectional search each (pgq_iterativelength_bidirectional without the chunk ceiling) */
int pgq_iterativelength_bidirectional_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst,
                                                  int64_t *d_out_len);
/* Rows in host memory, answered by all enabled devices: contiguous shards, one host thread and one CSR replica per
 * device, results gathered into out_len (same values as pgq_iterativelength_bulk_device: hop count, 0, or -1). */
int pgq_iterativelength_multi(pgq_csr_t *csr, int64_t n, const int64_t *src, const int64_t *dst, int64_t *out_len);
/* shortestpath (ShortestPathFunction, src/core/functions/scalar/shortest_path.cpp:43-207) by all enabled devices:
 * out_len / out_offset as in the bulk form; the lists of all shards are gathered
 * into child (host memory, capacity child_cap int64) in row order of the shards.  *child_used = elements needed;
 * PGQ_ERR_INVALID_ARG when child_cap is too small (out_len is complete, the payload is not usable). */
int pgq_shortestpath_multi(pgq_csr_t *csr, int64_t n, const int64_t *src, const int64_t *dst, int64_t *out_len,
                           int64_t *out_offset, int64_t *child, int64_t child_cap, int64_t *child_used);
/* pgq_shortestpath_multi under the pattern's upper bound (pgq_shortestpath_within_bulk_device per shard): rows farther apart
 * than max_hops have out_len -1 and no list; *child_used and the gathered payload count the rows within the bound only. */
int pgq_shortestpath_within_multi(pgq_csr_t *csr, int64_t n, const int64_t *src, const int64_t *dst, int64_t max_hops,
                                  int64_t *out_len, int64_t *out_offset, int64_t *child, int64_t child_cap, int64_t *child_used);
/* cheapest_path_length (CheapestPathLengthFunction, cheapest_path_length.cpp:138-163) by all enabled devices:
 * out = n int64 or double (by weight type), out_valid = n bytes. */
int pgq_cheapest_path_length_multi(pgq_csr_t *csr, int64_t n, const int64_t *src, const int64_t *dst, void *out,
                                   uint8_t *out_valid);
/* pgq_cheapest_path_length_multi under the pattern's upper bound (pgq_cheapest_path_length_within_bulk_device per shard): the
 * cheapest walk of at most max_hops edges per row — another number than the unbounded one, see pgq_cheapest_path_length_within. */
int pgq_cheapest_path_length_within_multi(pgq_csr_t *csr, int64_t n, const int64_t *src, const int64_t *dst, int64_t max_hops, void *out,
                                          uint8_t *out_valid);
/* Measurement helper: same search, additionally d_out_te[i] = edges traversed by pair i's own level-synchronous BFS
 * up to the level that reaches dst (all levels if unreachable) — the numerator of bench.py's MTEPS. */
int pgq_traversed_edges_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst,
                                    int64_t *d_out_len, int64_t *d_out_te);
/* d_out_len as above; paths are written packed into d_child (capacity child_cap int64), entry i at
 * d_out_offset[i] with 2*len+1 elements (no entry for NULL rows).  *child_used returns the elements needed;
 * PGQ_ERR_INVALID_ARG if child_cap was too small: d_out_len is still complete and *child_used says what to provide,
 * the child payload is not usable. */
int pgq_shortestpath_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst,
                                 int64_t *d_out_len, int64_t *d_out_offset, int64_t *d_child, int64_t child_cap,
                                 int64_t *child_used);
/* pgq_shortestpath_within without the chunk ceiling: as pgq_shortestpath_bulk_device, except that a row farther apart than
 * max_hops has d_out_len[i] = -1, no offset and no elements in d_child — *child_used (and what child_cap must hold) counts the
 * lists of the rows within the bound only. */
int pgq_shortestpath_within_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t max_hops,
                                        int64_t *d_out_len, int64_t *d_out_offset, int64_t *d_child, int64_t child_cap,
                                        int64_t *child_used);
/* out: int64 or double per weight type; NULL -> validity payload -1 (int64) / NaN is never used: d_out_valid
 * (n bytes, 1 = valid) carries validity. */
int pgq_cheapest_path_length_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst,
                                         void *d_out, uint8_t *d_out_valid);
/* pgq_cheapest_path_length_within without the chunk ceiling: as pgq_cheapest_path_length_bulk_device, each row the cost of its
 * cheapest walk of at most max_hops edges (NOT the unbounded cost with far rows NULL: see pgq_cheapest_path_length_within). */
int pgq_cheapest_path_length_within_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t max_hops,
                                                void *d_out, uint8_t *d_out_valid);
/* pgq_cheapest_path without the chunk ceiling: d_out_len[i] = hops of the cheapest path (its tight hop count H[dst]), 0 for
 * src == dst, -1 for NULL rows (d_src[i] < 0) and unreachable rows; lists and child-capacity protocol as
 * pgq_shortestpath_bulk_device: entry i at d_out_offset[i] with 2 * len + 1 elements, *child_used = the elements needed,
 * PGQ_ERR_INVALID_ARG when child_cap is too small (d_out_len is complete, the payload is not usable). */
int pgq_cheapest_path_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t *d_out_len,
                                  int64_t *d_out_offset, int64_t *d_child, int64_t child_cap, int64_t *child_used);
/* pgq_cheapest_path_within without the chunk ceiling: d_out_len[i] = h, the edges of the cheapest walk of at most max_hops edges
 * (NOT pgq_cheapest_path_bulk_device's lengths with long rows at -1: see pgq_cheapest_path_within), 0 for src == dst, -1 for
 * NULL rows and rows without such a walk; lists and child-capacity protocol as pgq_cheapest_path_bulk_device. */
int pgq_cheapest_path_within_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t max_hops,
                                         int64_t *d_out_len, int64_t *d_out_offset, int64_t *d_child, int64_t child_cap,
                                         int64_t *child_used);
/* pgq_cheapest_walk_length without the chunk ceiling: outputs as pgq_cheapest_path_length_within_bulk_device, each row the cost of
 * its cheapest walk of min_hops..max_hops edges (src == dst rows included: see pgq_cheapest_walk_length). */
int pgq_cheapest_walk_length_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops,
                                         int64_t max_hops, void *d_out, uint8_t *d_out_valid);
/* pgq_cheapest_walk without the chunk ceiling: d_out_len[i] = h, the edges of the cheapest walk of min_hops..max_hops edges
 * (0 only for a src == dst row at min_hops == 0), -1 for NULL rows and rows without such a walk; lists and child-capacity
 * protocol as pgq_cheapest_path_within_bulk_device. */
int pgq_cheapest_walk_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops,
                                  int64_t max_hops, int64_t *d_out_len, int64_t *d_out_offset, int64_t *d_child, int64_t child_cap,
                                  int64_t *child_used);
/* pgq_shortestpath_count without the chunk ceiling: d_out_count[i] = sigma[dst] (saturated), 1 for src == dst, 0 for an
 * unreachable row or one farther apart than max_hops, -1 for a NULL row (d_src[i] < 0). */
int pgq_shortestpath_count_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t max_hops,
                                       int64_t *d_out_count);
/* pgq_all_shortestpaths without the chunk ceiling.  Per row: d_out_len[i] = hops (0 for src == dst, -1 for NULL rows, unreachable
 * rows and rows beyond max_hops), d_out_count[i] = sigma as pgq_shortestpath_count_bulk_device reports it (whatever max_paths),
 * d_out_npaths[i] = the paths emitted, min(sigma, max_paths), d_out_first[i] = the index of its first path.  Path k starts at
 * d_path_offset[k] in d_child and has 2 * len + 1 elements; paths and payload are packed in row order.  *paths_used / *child_used =
 * the paths and elements needed; PGQ_ERR_INVALID_ARG when path_cap or child_cap is too small: d_out_len, d_out_count and
 * d_out_npaths are complete then and both *_used values say what to provide, the payload is not usable.  A NULL handle:
 * PGQ_ERR_INVALID_ARG, both *_used values 0. */
int pgq_all_shortestpaths_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t max_hops,
                                      int64_t max_paths, int64_t *d_out_len, int64_t *d_out_count, int64_t *d_out_first,
                                      int64_t *d_out_npaths, int64_t *d_path_offset, int64_t path_cap, int64_t *d_child,
                                      int64_t child_cap, int64_t *paths_used, int64_t *child_used);
/* pgq_walk_count without the chunk ceiling: d_out_count[i] = count (saturated), 0 when there is no such walk, -1 for a NULL row
 * (d_src[i] < 0). */
int pgq_walk_count_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops,
                               int64_t max_hops, int64_t *d_out_count);
/* pgq_walk_length without the chunk ceiling: d_out_len[i] = the length, -1 when there is no such walk and for a NULL row
 * (d_src[i] < 0). */
int pgq_walk_length_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops,
                                int64_t max_hops, int64_t *d_out_len);
/* pgq_k_shortest_walks without the chunk ceiling; outputs as pgq_all_shortestpaths_bulk_device with these differences.  The walks
 * of one row differ in length: walk j starts at d_path_offset[j] in d_child and has 2 * d_path_hops[j] + 1 elements (both arrays
 * path_cap entries).  d_out_len[i] = the hops of the row's first walk, -1 if it has none.  d_out_npaths[i] = min(count, k).
 * d_out_count[i] = the walks of lo..T edges, T the length of the row's last emitted walk (the rounds stop there, and a row that
 * has its k walks adds no more): this is count whenever count <= k, otherwise at least k and at most count —
 * pgq_walk_count_bulk_device gives count itself; -1 for a NULL row.  Capacity protocol: *paths_used / *child_used = the walks and
 * elements needed; PGQ_ERR_INVALID_ARG when path_cap or child_cap is too small: d_out_len, d_out_count and d_out_npaths are
 * complete then, the payload is not usable.  A NULL handle: PGQ_ERR_INVALID_ARG, both *_used values 0. */
int pgq_k_shortest_walks_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops,
                                     int64_t max_hops, int64_t k, int64_t *d_out_len, int64_t *d_out_count, int64_t *d_out_first,
                                     int64_t *d_out_npaths, int64_t *d_path_offset, int64_t *d_path_hops, int64_t path_cap,
                                     int64_t *d_child, int64_t child_cap, int64_t *paths_used, int64_t *child_used);
/* pgq_walk_count_mode without the chunk ceiling: d_out_count[i] = min(a, limit), -1 for a NULL row (d_src[i] < 0). */
int pgq_walk_count_mode_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops,
                                    int64_t max_hops, int64_t limit, int path_mode, int64_t *d_out_count);
/* pgq_k_shortest_walks_mode without the chunk ceiling: pgq_k_shortest_walks_bulk_device with path_mode behind k, the same outputs and
 * the same two-buffer capacity protocol.  Under a mode d_out_len[i] = the hops of the row's first admitted walk (-1: none) and
 * d_out_npaths[i] = d_out_count[i] = min(a, k) (-1 / 0 for a NULL row as there); under NONE / WALK all of them are that call's. */
int pgq_k_shortest_walks_mode_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops,
                                          int64_t max_hops, int64_t k, int path_mode, int64_t *d_out_len, int64_t *d_out_count,
                                          int64_t *d_out_first, int64_t *d_out_npaths, int64_t *d_path_offset, int64_t *d_path_hops,
                                          int64_t path_cap, int64_t *d_child, int64_t child_cap, int64_t *paths_used,
                                          int64_t *child_used);
/* pgq_k_shortest_groups without the chunk ceiling: pgq_k_shortest_walks_mode_bulk_device with groups and max_paths in k's place and
 * d_out_ngroups (n entries) behind d_out_npaths; the same two-buffer capacity protocol and arena rules.  d_out_len[i] = the hops of
 * the row's first walk (-1: none), d_out_npaths[i] = min(|A|, P), d_out_ngroups[i] = the distinct lengths among the emitted walks,
 * d_out_count[i] = min(|A|, P + 1), -1 for a NULL row.  When path_cap or child_cap is too small (PGQ_ERR_INVALID_ARG) d_out_len,
 * d_out_count, d_out_npaths and d_out_ngroups are complete, the payload is not usable. */
int pgq_k_shortest_groups_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops,
                                      int64_t max_hops, int64_t groups, int64_t max_paths, int path_mode, int64_t *d_out_len,
                                      int64_t *d_out_count, int64_t *d_out_first, int64_t *d_out_npaths, int64_t *d_out_ngroups,
                                      int64_t *d_path_offset, int64_t *d_path_hops, int64_t path_cap, int64_t *d_child,
                                      int64_t child_cap, int64_t *paths_used, int64_t *child_used);

/* ---- the other CSR consumers ------------------------------------------------------------- */

/* local_clustering_coefficient(csr_id, id) -> FLOAT   src/core/functions/scalar/local_clustering_coefficient.cpp:11-72
 * (bit-identical: integer counting + the reference's three float operations).  NULL rows -> NULL; ids outside [0,V)
 * (undefined behaviour in the reference) -> PGQ_ERR_INVALID_ARG.  Bulk form: d_src[i] < 0 = NULL row (value 0). */
int pgq_local_clustering_coefficient(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, float *out, uint64_t *out_valid);
int pgq_local_clustering_coefficient_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, float *d_out);
/* pagerank(csr_id, id) -> DOUBLE   src/core/functions/scalar/pagerank.cpp:11-111: power iteration over V + 2 entries,
 * damping 0.85, threshold 1e-6, computed once per handle; rows outside [0, V + 2) or NULL -> NULL.  Partial sums follow
 * the reference's accumulation order; the dangling total is a two-level sum (tests: 1e-12 relative).
 * pgq_pagerank_device copies all V + 2 ranks into d_rank (may be NULL) and reports the iteration count. */
int pgq_pagerank(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, double *out, uint64_t *out_valid);
int pgq_pagerank_device(pgq_csr_t *csr, double *d_rank, int *iterations);

/* weakly_connected_component(csr_id, id) -> BIGINT   src/core/functions/scalar/weakly_connected_component.cpp:36-104: the
 * component id is the root the reference's sequential union-find (Link(i, neighbour): i's root under the neighbour's,
 * vertices and slots in CSR order) ends in.  The edges that change that forest are the minimum spanning forest under
 * the weights "slot index": found on the device (Boruvka rounds), replayed in slot order by the reference's own Link
 * (V - 1 edges at most).  Computed once per handle.  NULL id -> NULL; ids outside [0, V + 2) -> NULL; the two trailing
 * forest entries behave like the reference's (V: its own root; V + 1: the root of vertex 0).
 * pgq_weakly_connected_component_device copies all V + 2 ids into d_ids (may be NULL: just compute). */
int pgq_weakly_connected_component(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, int64_t *out, uint64_t *out_valid);
int pgq_weakly_connected_component_device(pgq_csr_t *csr, int64_t *d_ids);

/* ---- tuning & measurement --------------------------------------------------------------------------------- */

/* Knobs (also readable from the environment at pgq_init: PGQ_WORDS, PGQ_PUSH_DIV, PGQ_PROFILE ...).
 * key/value strings; returns PGQ_ERR_INVALID_ARG for unknown keys. */
int pgq_set_option(const char *key, const char *value);
/* Current value of a knob (integers are returned as doubles). */
int pgq_get_option(const char *key, double *value);
/* the value the library ships with for this key, whatever the process or the environment has set since */
int pgq_get_default_option(const char *key, double *value);
/* Options of ONE handle: the first pgq_csr_set_option copies the process-wide set into the handle; searches on this
 * handle then run under the copy (on every host thread that works for the call), so that two connections, or a test,
 * can tune their own CSR without touching each other's.  Options consumed at upload (meet_align, hub_chunk, ...) are
 * not affected. */
int pgq_csr_set_option(pgq_csr_t *csr, const char *key, const char *value);
int pgq_csr_get_option(pgq_csr_t *csr, const char *key, double *value);

/* Per-thread counters of the searches run since the last reset, and per-kernel-class HIP-event time
 * (only accumulated while option "profile" = "1"). */
#define PGQ_KCLASS_MAX 16
typedef struct pgq_stats {
	int64_t batches;          /* lane batches started */
	int64_t levels;           /* BFS levels executed (all batches) */
	int64_t push_levels;      /* of which top-down */
	int64_t pull_levels;      /* of which bottom-up */
	int64_t edges_scanned;    /* physical adjacency entries read by push+pull kernels */
	int64_t word_gathers;     /* lane-words (8 B) gathered / RMW'd along those entries */
	int64_t frontier_vertices;/* sum over levels of vertices with a non-empty frontier word */
	int64_t unique_sources;   /* lanes used */
	int64_t pairs;            /* rows handled */
	int64_t deferred_pairs;   /* rows re-run in a narrow straggler batch */
	int64_t meet_pairs;       /* rows answered by the pair-centric pre-pass (distance <= 3, NULL, trivial) */
	double algo_bytes[PGQ_KCLASS_MAX]; /* algorithmic bytes per kernel class (DESIGN.md formulas) */
	double kernel_ms[PGQ_KCLASS_MAX];  /* HIP-event time per kernel class (profile=1) */
	int64_t launches[PGQ_KCLASS_MAX];
	int64_t spec_batches;     /* lane batches whose levels were enqueued ahead of the host (one wait per batch) */
	int64_t spec_levels;      /* levels that ran that way */
	int64_t spec_aborts;      /* batches whose enqueued levels were called off on the device (plan mismatch / too short) */
	int64_t host_waits;       /* stream synchronisations of the lane-batched search (lane assignment, levels, results) */
	int64_t ball_segments;    /* round 6: source runs (cut at 1024-row windows) the source-centric kernel answered, one ball each */
	int64_t ball_calls;       /* calls (or straggler passes) the source-centric kernel took */
	/* of launches[], those whose per-vertex (or frontier) bit map sat in LDS rather than in global memory: k_src_ball (ball),
	 * k_meet4 / k_meet4d (meet4), k_bibfs (bibfs), k_pull_lanes / k_pull_sparse (pull_sparse) */
	int64_t lds_map_launches[PGQ_KCLASS_MAX];
} pgq_stats_t;
const char *pgq_kclass_name(int kclass); /* NULL past the last class */
/* pgq_stats_t grows at its END from release to release (pgq_version() names the release).  pgq_get_stats_sized writes at most
 * struct_size bytes — what a caller compiled against an older header passes as sizeof(pgq_stats_t) — so an old binary keeps
 * working against a newer library; pgq_get_stats(out) = pgq_get_stats_sized(out, sizeof(pgq_stats_t) of THIS header) and is
 * only safe for callers compiled against it. */
int pgq_get_stats_sized(pgq_stats_t *out, size_t struct_size);
int pgq_get_stats(pgq_stats_t *out);
int pgq_reset_stats(void);

/* Raw copy-bandwidth probe (bytes moved / second, read+write) used by bench.py for the measured HBM ceiling. */
int pgq_measure_copy_bandwidth(int64_t bytes, int iters, double *out_gbps);

#ifdef __cplusplus
}
#endif
#endif /* PGQ_HIP_H */
