/* pgq_udf.h — C ABI of libpgq_udf.so: DuckDB-free host mirror of DuckPGQ's scalar-function layer (L5/L6).
 *
 * The reference's UDF bodies take `(DataChunk &args, ExpressionState &state, Vector &result)` and reach their
 * CSR through `DuckPGQState` (per connection).  DuckDB is not available in this build environment, so the same
 * logic is exposed here with the chunk's columns passed as pgq_vec_t (UnifiedVectorFormat) and the result as a
 * FLAT vector + validity mask.  A DuckDB glue file only has to forward `ToUnifiedFormat` output to these
 * calls and rethrow pgq_udf_last_error() (INTEGRATION.md shows it).  One function per reference UDF:
 *
 *   pgq_udf_create_csr_vertex       CreateCsrVertexFunction      src/core/functions/scalar/csr_creation.cpp:86-110
 *   pgq_udf_create_csr_edge         CreateCsrEdgeFunction        src/core/functions/scalar/csr_creation.cpp:112-198
 *   pgq_udf_bind_search             IterativeLengthBind          src/core/functions/function_data/iterative_length_function_data.cpp:18-30
 *   pgq_udf_iterativelength         IterativeLengthFunction      src/core/functions/scalar/iterativelength.cpp:34-143
 *   pgq_udf_iterativelength_within  IterativeLengthFunction with the pattern's upper bound as fifth argument (match.cpp:658-671)
 *   pgq_udf_iterativelength2        IterativeLength2Function     src/core/functions/scalar/iterativelength2.cpp:33-130 (same results)
 *   pgq_udf_iterativelengthbidirectional  IterativeLengthBidirectionalFunction  src/core/functions/scalar/iterativelength_bidirectional.cpp:43-153 (intended semantics)
 *   pgq_udf_shortestpath            ShortestPathFunction         src/core/functions/scalar/shortest_path.cpp:43-207
 *   pgq_udf_shortestpath_within     ShortestPathFunction with the pattern's upper bound as fifth argument (match.cpp:467-495, 658-671)
 *   pgq_udf_shortestpath_count      (no counterpart: ALL SHORTEST, match.cpp:82) the number of shortest paths within the upper bound
 *   pgq_udf_all_shortestpaths       (no counterpart) ... and the first max_paths of them as a list of lists; both bound like shortestpath
 *   pgq_udf_walk_count              (no counterpart: {lower,upper} in WALK mode) the number of walks of lower..upper edges
 *   pgq_udf_walk_length             (no counterpart: the filter {lower,upper} needs in WALK mode, where match.cpp:658-671 emits iterativelength BETWEEN) the shortest such walk's length
 *   pgq_udf_k_shortest_walks        (no counterpart: TopK, match.cpp:82-98) ... and the first k of them, shortest first; both bound like shortestpath
 *   pgq_udf_walk_count_mode         (no counterpart: path modes, match.cpp:80-108) the admitted walks under TRAIL / ACYCLIC / SIMPLE, up to a limit
 *   pgq_udf_k_shortest_walks_mode   (no counterpart) ... and the first k of them, shortest first; both bound like shortestpath
 *   pgq_udf_k_shortest_groups       (no counterpart: SHORTEST k GROUP, path_pattern.hpp:22) every walk of the k smallest lengths; bound like shortestpath
 *   pgq_udf_bind_cheapest           CheapestPathLengthBind      src/core/functions/function_data/cheapest_path_length_function_data.cpp:7-32
 *   pgq_udf_cheapest_path_length    CheapestPathLengthFunction   src/core/functions/scalar/cheapest_path_length.cpp:138-163
 *   pgq_udf_cheapest_path_length_within  CheapestPathLengthFunction with the pattern's upper bound as fifth argument (match.cpp:658-671)
 *   pgq_udf_cheapest_path           (no counterpart) the cheapest path as a list; bound like cheapest_path_length
 *   pgq_udf_cheapest_path_within    (no counterpart) ... of at most the pattern's upper bound of edges, fifth argument
 *   pgq_udf_cheapest_walk_length    (no counterpart: a weighted {lower,upper} in WALK mode) the cost of the cheapest walk of lower..upper edges
 *   pgq_udf_cheapest_walk           (no counterpart) ... and that walk as a list; both bound like cheapest_path_length
 *   pgq_udf_delete_csr              DeleteCsrFunction            src/core/functions/scalar/csr_deletion.cpp:10-20
 *   pgq_udf_csr_get_w_type          GetCsrWTypeFunction          src/core/functions/scalar/csr_get_w_type.cpp:16-36
 *   pgq_udf_reachability            ReachabilityFunction         src/core/functions/scalar/reachability.cpp:165-254 (intended semantics)
 *   pgq_state_query_end             DuckPGQState::QueryEnd       src/duckpgq_state.cpp:162-170
 *   pgq_udf_scan_csr_v / _e / _w    get_csr_v / get_csr_e / get_csr_w   src/core/functions/table/pgq_scan.cpp:84-153
 *
 * Error convention: 0 on success; -1 with pgq_udf_last_error() holding the reference's exception text
 * ("Constraint Error: ...", "Invalid Input Error: ...") or the device library's message.
 */
#ifndef PGQ_UDF_H
#define PGQ_UDF_H

#include "pgq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgq_state pgq_state_t; /* DuckPGQState: csr_list + csr_lock + csr_to_delete (duckpgq_state.hpp:36-38) */

pgq_state_t *pgq_state_new(void);
void pgq_state_free(pgq_state_t *);
int pgq_state_query_end(pgq_state_t *);
const char *pgq_udf_last_error(void);

int pgq_udf_create_csr_vertex(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t dense_id, pgq_vec_t cnt,
                              int64_t *out, uint64_t *out_valid);
/* w may be NULL (7-argument form); w_type PGQ_W_INT64 / PGQ_W_DOUBLE for the 8-argument form */
int pgq_udf_create_csr_edge(pgq_state_t *, int32_t id, int64_t V, int64_t e_sum, int64_t e_count, int64_t n,
                            pgq_vec_t src, pgq_vec_t dst, pgq_vec_t edge_id, const pgq_vec_t *w, int w_type,
                            int32_t *out, uint64_t *out_valid);

int pgq_udf_bind_search(pgq_state_t *, int32_t id);
int pgq_udf_iterativelength(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst,
                            int64_t *out, uint64_t *out_valid);
/* iterativelength(id, V, src, dst, upper): rows more than max_hops hops apart are NULL (pgq_iterativelength_within);
 * errors as for pgq_udf_iterativelength, max_hops < 0 is the device library's PGQ_ERR_INVALID_ARG */
int pgq_udf_iterativelength_within(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst,
                                   int64_t max_hops, int64_t *out, uint64_t *out_valid);
int pgq_udf_iterativelength2(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst,
                             int64_t *out, uint64_t *out_valid);
/* iterativelengthbidirectional(id, V, src, dst) -> BIGINT (src/core/functions/scalar/iterativelength_bidirectional.cpp:43-153).
 * The reference alternates a source-side and a destination-side BFS but indexes its inputs through a uint8_t* and
 * walks the forward CSR on the destination side: untested, parity unpinned.  What it intends to
 * return is the hop count, which is what this entry point returns (same values as pgq_udf_iterativelength). */
int pgq_udf_iterativelengthbidirectional(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst,
                                         int64_t *out, uint64_t *out_valid);
int pgq_udf_shortestpath(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst,
                         uint64_t *out_offset, uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child,
                         uint64_t *out_child_len);
/* shortestpath(id, V, src, dst, upper): rows whose path has more than max_hops hops are NULL and take no room in the child
 * payload (pgq_shortestpath_within); errors as for pgq_udf_shortestpath, max_hops < 0 is the device library's PGQ_ERR_INVALID_ARG */
int pgq_udf_shortestpath_within(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops,
                                uint64_t *out_offset, uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child,
                                uint64_t *out_child_len);
/* shortestpath_count(id, V, src, dst, upper) -> BIGINT: the number of shortest paths of at most max_hops hops, saturated at
 * 2^63 - 1 (pgq_shortestpath_count: 1 for src == dst, 0 for unreachable or farther rows, NULL for a NULL endpoint); bound through
 * pgq_udf_bind_search, errors as for pgq_udf_shortestpath, max_hops < 0 is the device library's PGQ_ERR_INVALID_ARG */
int pgq_udf_shortestpath_count(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops,
                               int64_t *out, uint64_t *out_valid);
/* all_shortestpaths(id, V, src, dst, upper, max_paths) -> LIST(LIST(BIGINT)): the first max_paths shortest paths of every row in
 * the contract's order (pgq_all_shortestpaths; path 0 is shortestpath's list); outputs as that call's: outer entries per row,
 * inner entries and child payload in the thread's result arena.  Bound through pgq_udf_bind_search, errors as for
 * pgq_udf_shortestpath; max_hops < 0 and max_paths < 1 are the device library's PGQ_ERR_INVALID_ARG */
int pgq_udf_all_shortestpaths(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops,
                              int64_t max_paths, uint64_t *out_first, uint64_t *out_npaths, uint64_t *out_valid,
                              const uint64_t **out_path_offset, const uint64_t **out_path_length, uint64_t *out_path_total,
                              const int64_t **out_child, uint64_t *out_child_len);
/* walk_count(id, V, src, dst, lower, upper) -> BIGINT: the number of walks of lower..upper edges, saturated at 2^63 - 1
 * (pgq_walk_count: src == dst counts the empty walk when lower == 0 and every closed walk; 0 when there is none, NULL for a NULL
 * endpoint); bound through pgq_udf_bind_search, errors as for pgq_udf_shortestpath; bounds out of range are the device library's
 * PGQ_ERR_INVALID_ARG / PGQ_ERR_UNSUPPORTED (upper > PGQ_WALK_MAX_HOPS: walks need an upper bound) */
int pgq_udf_walk_count(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops,
                       int64_t *out, uint64_t *out_valid);
/* walk_length(id, V, src, dst, lower, upper) -> BIGINT: the length of the shortest walk of lower..upper edges (pgq_walk_length:
 * src == dst is not special; NULL when there is no such walk and for a NULL endpoint) — `walk_length(...) IS NOT NULL` is the
 * filter of a quantified pattern in WALK mode.  Bound through pgq_udf_bind_search, errors as for pgq_udf_walk_count */
int pgq_udf_walk_length(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops,
                        int64_t *out, uint64_t *out_valid);
/* k_shortest_walks(id, V, src, dst, lower, upper, k) -> LIST(LIST(BIGINT)): the first k walks of lower..upper edges of every row,
 * shorter walks first, in the contract's order (pgq_k_shortest_walks; for src != dst and lower <= dist <= upper walk 0 is
 * shortestpath's list); outputs as pgq_udf_all_shortestpaths.  Bound through pgq_udf_bind_search, errors as for
 * pgq_udf_walk_count; k < 1 is the device library's PGQ_ERR_INVALID_ARG */
int pgq_udf_k_shortest_walks(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops,
                             int64_t max_hops, int64_t k, uint64_t *out_first, uint64_t *out_npaths, uint64_t *out_valid,
                             const uint64_t **out_path_offset, const uint64_t **out_path_length, uint64_t *out_path_total,
                             const int64_t **out_child, uint64_t *out_child_len);
/* walk_count(id, V, src, dst, lower, upper, limit, path_mode) -> BIGINT: min(admitted walks, limit) under path_mode (PGQ_MODE_*,
 * pgq_walk_count_mode; NONE / WALK: min(walk_count, limit)); NULL for a NULL endpoint.  Bound through pgq_udf_bind_search, errors as
 * for pgq_udf_walk_count; limit < 1 and an unknown mode are the device library's PGQ_ERR_INVALID_ARG, a row's search beyond option
 * mode_step_cap its PGQ_ERR_UNSUPPORTED */
int pgq_udf_walk_count_mode(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops,
                            int64_t max_hops, int64_t limit, int path_mode, int64_t *out, uint64_t *out_valid);
/* k_shortest_walks(id, V, src, dst, lower, upper, k, path_mode) -> LIST(LIST(BIGINT)): the first k walks of lower..upper edges that
 * path_mode admits, in k_shortest_walks' order (pgq_k_shortest_walks_mode; NONE / WALK: that call's lists); outputs and errors as
 * pgq_udf_k_shortest_walks, plus those of pgq_udf_walk_count_mode */
int pgq_udf_k_shortest_walks_mode(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops,
                                  int64_t max_hops, int64_t k, int path_mode, uint64_t *out_first, uint64_t *out_npaths,
                                  uint64_t *out_valid, const uint64_t **out_path_offset, const uint64_t **out_path_length,
                                  uint64_t *out_path_total, const int64_t **out_child, uint64_t *out_child_len);
/* k_shortest_groups(id, V, src, dst, lower, upper, groups, max_paths, path_mode) -> LIST(LIST(BIGINT)): SHORTEST k GROUP — every walk
 * of the `groups` smallest distinct lengths in lower..upper that have a walk path_mode admits, in k_shortest_walks' order, cut at
 * max_paths walks per row (pgq_k_shortest_groups); out_ngroups[i] = the distinct lengths among row i's walks.  Outputs and errors as
 * pgq_udf_k_shortest_walks_mode; groups < 1 and max_paths < 1 are the device library's PGQ_ERR_INVALID_ARG */
int pgq_udf_k_shortest_groups(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops,
                              int64_t max_hops, int64_t groups, int64_t max_paths, int path_mode, uint64_t *out_first,
                              uint64_t *out_npaths, uint64_t *out_ngroups, uint64_t *out_valid, const uint64_t **out_path_offset,
                              const uint64_t **out_path_length, uint64_t *out_path_total, const int64_t **out_child,
                              uint64_t *out_child_len);
/* *ret_type: PGQ_W_INT64 -> BIGINT result, PGQ_W_DOUBLE -> DOUBLE result */
int pgq_udf_bind_cheapest(pgq_state_t *, int32_t id, int *ret_type);
int pgq_udf_cheapest_path_length(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst,
                                 void *out, uint64_t *out_valid);
/* cheapest_path_length(id, V, src, dst, upper): the cheapest walk of at most max_hops edges (pgq_cheapest_path_length_within: not
 * the unbounded cost with far rows NULL); errors as for pgq_udf_cheapest_path_length, max_hops < 0 is the device library's
 * PGQ_ERR_INVALID_ARG */
int pgq_udf_cheapest_path_length_within(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops,
                                        void *out, uint64_t *out_valid);
/* cheapest_path(id, V, src, dst) -> LIST(BIGINT): the cheapest path itself, [src, e1, v1, ..., ek, dst] (pgq_cheapest_path: the
 * hop-minimal cheapest path under shortestpath's tie-breaks); bound through pgq_udf_bind_cheapest, outputs as
 * pgq_udf_shortestpath, errors as for pgq_udf_cheapest_path_length.  The reference has no such function. */
int pgq_udf_cheapest_path(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, uint64_t *out_offset,
                          uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child, uint64_t *out_child_len);
/* cheapest_path(id, V, src, dst, upper) -> LIST(BIGINT): the cheapest walk of at most max_hops edges itself
 * (pgq_cheapest_path_within: the list whose cost pgq_udf_cheapest_path_length_within returns, not pgq_udf_cheapest_path's list
 * with long rows NULL); errors as for pgq_udf_cheapest_path, max_hops < 0 is the device library's PGQ_ERR_INVALID_ARG */
int pgq_udf_cheapest_path_within(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops,
                                 uint64_t *out_offset, uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child,
                                 uint64_t *out_child_len);
/* cheapest_walk_length(id, V, src, dst, lower, upper) -> BIGINT / DOUBLE and cheapest_walk(id, V, src, dst, lower, upper) ->
 * LIST(BIGINT): the cost and the list of the cheapest walk of lower..upper edges (pgq_cheapest_walk_length / pgq_cheapest_walk:
 * src == dst is not special, NULL when there is no such walk and for a NULL endpoint; NOT a filter around the _within calls).
 * Bound through pgq_udf_bind_cheapest, outputs as the _within forms, errors as for pgq_udf_cheapest_path_length; bad bounds are the
 * device library's PGQ_ERR_INVALID_ARG / PGQ_ERR_UNSUPPORTED (lower > PGQ_WALK_MAX_HOPS).  The reference has no such function. */
int pgq_udf_cheapest_walk_length(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops,
                                 int64_t max_hops, void *out, uint64_t *out_valid);
int pgq_udf_cheapest_walk(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops,
                          uint64_t *out_offset, uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child,
                          uint64_t *out_child_len);
/* reachability(id, is_variant, V, src, dst) -> BOOL; the reference's BOOL argument only selects one of its three
 * internal BFS modes (reachability.cpp:154-163) and does not change the result, so it is not part of this call.
 * Boolean reachability with the semantics the reference intends (reachability.cpp:165-254 indexes its inputs
 * through a uint8_t* and has no test: parity unpinned): out[i] = 1 iff a path exists
 * (src == dst counts as reachable). */
int pgq_udf_reachability(pgq_state_t *, int32_t id, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst,
                         uint8_t *out, uint64_t *out_valid);

/* The other CSR consumers.  Errors as in the reference: "Constraint Error: CSR not found. Is the
 * graph populated?" / "Need to initialize CSR before ..." (local_clustering_coefficient.cpp:16-23, pagerank.cpp:17-24,
 * weakly_connected_component.cpp:41-48).  All three run on the device (pgq_local_clustering_coefficient / pgq_pagerank /
 * pgq_weakly_connected_component).  The component id of weakly_connected_component is the root the reference's
 * sequential union-find schedule ends in (weakly_connected_component.cpp:14-34,83-90 — the goldens pin it): the device
 * finds the spanning forest under that schedule's edge order, the reference's Link replays its edges. */
int pgq_udf_local_clustering_coefficient(pgq_state_t *, int32_t id, int64_t n, pgq_vec_t src, float *out, uint64_t *out_valid);
int pgq_udf_pagerank(pgq_state_t *, int32_t id, int64_t n, pgq_vec_t src, double *out, uint64_t *out_valid);
int pgq_udf_weakly_connected_component(pgq_state_t *, int32_t id, int64_t n, pgq_vec_t src, int64_t *out, uint64_t *out_valid);

int pgq_udf_delete_csr(pgq_state_t *, int32_t id, int *out_flag);
int pgq_udf_csr_get_w_type(pgq_state_t *, int32_t id, int32_t *out);

/* table-function scans used by the reference's tests to observe the CSR: copy up to cap entries, return count */
int64_t pgq_udf_scan_csr_v(pgq_state_t *, int32_t id, int64_t *out, int64_t cap);
int64_t pgq_udf_scan_csr_e(pgq_state_t *, int32_t id, int64_t *out, int64_t cap);
int64_t pgq_udf_scan_csr_w(pgq_state_t *, int32_t id, void *out, int64_t cap);
/* device handle of a CSR (uploads it if needed); NULL on error */
pgq_csr_t *pgq_udf_device_csr(pgq_state_t *, int32_t id);

#ifdef __cplusplus
}
#endif
#endif
