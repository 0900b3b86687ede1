// pgq_relax.h — what other translation units may use from pgq_cheapest.hip, the batched relaxation, and nothing else: the lane
// count and the label sentinels, the round counters' layout, the two hooks a driver hangs into the lane batches, the CSR's
// once-per-handle weight tables, and the two entry functions that run the batches with a hook.  The kernels, RelaxWorker, the
// *Batches drivers and their launch helpers stay private to pgq_cheapest.hip: k_relax and k_relax_hops are instantiated there,
// once.  Users: pgq_cheapest_path.hip (everything), pgq_path_lists.h (LC), pgq_all_shortest.hip (LC, fill32).
#pragma once

#include <limits>

#include "pgq_search.h"

namespace pgq {

static constexpr int LC = 64; // lanes of a batch: searches per label row, one per lane of a wavefront

template <typename T> struct Inf;
template <> struct Inf<int64_t> {
	static constexpr int64_t bits = std::numeric_limits<int64_t>::max() / 2; // cheapest_path_length.cpp:15
};
template <> struct Inf<double> {
	// bit pattern of DBL_MAX / 2 = 0x7FDFFFFFFFFFFFFF
	static constexpr int64_t bits = 0x7FDFFFFFFFFFFFFFll;
};

// The counter block of a worker's rounds, at the head of its ws->counters.  Outside pgq_cheapest.hip only `tcount` is read (by
// address, on the device): the fill of the batch's touched list, over which a driver resets what it set per labelled vertex.
struct RelaxCounters {
	u32 nq[2];
	u32 tcount;
	u32 rounds; // rounds executed by the last k_relax_small launch
	u64 relaxed_edges;
	long long min_deferred; // smallest label (bit pattern) a round left for later (k_relax's threshold)
	u32 relaxed_vertices;   // vertices a round expanded
	u32 snap_rows;          // label rows k_hop_snapshot copied (hop-bounded rounds; runs on over a batch, like `rounds` there)
	u64 heavy;              // (entries << 32) | chunks of the round's heavy list (k_relax)
	long long bound[64];    // per lane: the largest tentative label among its destinations (nothing beyond it matters)
	u32 take_rows;          // of snap_rows, the rows an exact round took (cheapest_walk: 512 more bytes written each)
	u32 pad_;
};

// What cheapest_path asks of the lane batches (pgq_cheapest_path.hip) instead of the rows' costs: the labels of EVERY vertex a
// lane reaches settled (no lane stops at its destinations' bound: see k_lane_unbound), and a call per settled batch — rows
// [lo, hi) of the sorted arrays, lane 0 = distinct source `base` — while the batch's labels are still in place.
struct SettledBatch {
	std::function<int(int64_t lo, int64_t hi, int64_t base)> then;
};

// What cheapest_path_within asks of the hop-bounded rounds (pgq_cheapest_path_within.hip) instead of the rows' costs: the snapshot
// rows of every round KEPT, in a log that grows round by round, and a call per finished batch while the log is in place.
struct HopLog {
	// In k_hop_snapshot's place: logs the `nq` vertices of the queue of parity `par` with their label rows as they stand after
	// `round` rounds, takes their dirty words, and says where these entries' rows and masks lie — what the next k_relax_hops
	// reads.  The host knows nq: a logged batch waits after every round, so the log has its room before a launch appends to it.
	// take: an exact round of cheapest_walk (round < lower) — the logged rows go back to INF in the label array, as k_hop_snapshot's take does.
	std::function<int(int par, u32 nq, int64_t round, bool take, const int64_t **snap, const u64 **snapmask)> append;
	// behind the batch's last round and the log pass of the vertices it changed: rows [lo, hi) of the sorted arrays, lane 0 =
	// distinct source `base`
	std::function<int(int64_t lo, int64_t hi, int64_t base)> then;
};

// in-edge weights in reverse-CSR order + the mean weight, built on first use.  with_mean = false: the weights alone
int ensure_reverse_weights(pgq_csr *c, Workspace *ws, bool with_mean = true);
// mean edge weight (int64 or double), computed once per CSR: the band width of the ordered relaxation rounds
int ensure_weight_mean(pgq_csr *c, Workspace *ws);
// the weighted entry points' first check: a handle, with weights, none of them negative
int check_weighted(pgq_csr_t *csr);

// cheapest_walk's bounds: min_hops < 0 or max_hops < min_hops -> PGQ_ERR_INVALID_ARG, min_hops > PGQ_WALK_MAX_HOPS -> PGQ_ERR_UNSUPPORTED
int check_walk_bounds(int64_t min_hops, int64_t max_hops);

// p[0 .. n) = value, enqueued on `st` (k_fill32)
void fill32(int32_t *p, int64_t n, int32_t value, hipStream_t st);

// The lane batches 0 .. nb - 1 of a call on one worker (`ws` holds the sorted rows and the distinct sources, and everything a
// batch writes), U distinct sources, T = the CSR's weight type.
// settle_every_label: plain rounds over the unsorted lists with 8-byte labels and without the lanes' bounds; settled.then() per batch.
// hop_rounds_logged:  at most K rounds of one edge each per batch, the first `lower` of them exact (0: cheapest_path_within),
//                     log.append() in k_hop_snapshot's place, log.then() per batch.
template <typename T> int settle_every_label(pgq_csr *c, Workspace *ws, int nb, u32 U, const SettledBatch &settled);
template <typename T> int hop_rounds_logged(pgq_csr *c, Workspace *ws, int nb, u32 U, int64_t lower, int64_t K, const HopLog &log);
extern template int settle_every_label<int64_t>(pgq_csr *, Workspace *, int, u32, const SettledBatch &);
extern template int settle_every_label<double>(pgq_csr *, Workspace *, int, u32, const SettledBatch &);
extern template int hop_rounds_logged<int64_t>(pgq_csr *, Workspace *, int, u32, int64_t, int64_t, const HopLog &);
extern template int hop_rounds_logged<double>(pgq_csr *, Workspace *, int, u32, int64_t, int64_t, const HopLog &);

} // namespace pgq
