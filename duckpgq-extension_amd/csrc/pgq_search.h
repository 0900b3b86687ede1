// pgq_search.h — per-call workspace and lane assignment shared by the BFS and cheapest-path drivers
#pragma once
#include <cmath>
#include <memory>
#include <optional>
#include <type_traits>

#include "pgq_internal.h"

namespace pgq {

static constexpr u32 kNoLane = 0xFFFFFFFFu;   // NULL rows
static constexpr u32 kTrivial = 0xFFFFFFFEu;  // src == dst rows (no search needed)
static constexpr int kSpecLevels = 61;        // levels of a batch enqueued ahead of the host at most (the pinned log holds 64 entries)

struct Counters {
	u32 q_count[2];      // work items in the frontier queues (by level parity)
	u32 front_vertices;  // vertices that received fresh bits this level
	u32 unresolved;      // pairs of the batch still without an answer
	u64 front_edges;     // sum of their out-degrees
	u64 edges_scanned;   // adjacency entries read this level
	u64 word_gathers;    // 8-byte lane-words gathered or RMW'd this level
	u32 front_words;     // non-empty lane-words of the frontier just produced
	u32 pad;             // packed frontier: records written ...
	u32 pad2;            // ... and overflow words written (k_compact_frontier totals)
	u32 done;            // levels enqueued ahead (spec_levels): set by k_level_reset when the batch is over (1), when the level's
	                     // plan is not what the counters call for (2) or when the plan has run out (3); every level kernel returns at once
	u32 r1[4];
	u64 act[2][32];      // active-lane masks (lanes that still have open pairs), double buffered
};

#ifdef __HIPCC__
// A level kernel has nothing to do when the batch is over on the device's own account (`done`) or when the probe before
// it left at most `stop_limit` rows open (the host defers them).
__device__ __forceinline__ bool level_is_off(const Counters *__restrict__ cnt, int stop_limit) {
	return cnt->done != 0 || (stop_limit >= 0 && cnt->unresolved <= (u32)stop_limit);
}
#endif

// bytes (at streaming rate) the lane-batched search is priced at for `distinct` sources: full 2048-lane batches of 32
// lane-words plus one narrower batch for the rest, E x (12 + 3 wd) each; `edge_bytes` = meet_bias x E.  Shared by the
// host-side decision (few rows) and k_meet_decide (sampled distinct sources).
// Round 5: `rows` / `V` add the DENSE bottom-up level, E x (8 + 6 wd), to every batch that holds more than V / 8 rows — with
// that many open rows the probes do not replace it (2048 sources x 128 .. 1024 destinations on the SF100-shaped graph: 2.1 -
// 2.3 ms per batch against 0.73 ms at x 32, where the probes do; priced without it a 2048 x 256 product went through the
// lanes at 2.05 ms where the pre-pass takes 1.16).
__host__ __device__ static inline double lanes_cost_bytes(double edge_bytes, double distinct, double rows, double V) {
	const double full = floor(distinct / 2048.0), rest = distinct - full * 2048.0;
	double wd = 0.0;
	if (rest > 0.0) {
		wd = 1.0;
		while (wd * 64.0 < rest) wd *= 2.0;
	}
	const double batches = full + (rest > 0.0 ? 1.0 : 0.0);
	const bool dense = batches > 0.0 && rows / batches > V / 8.0;
	return edge_bytes * (full * (12.0 + 3.0 * 32.0 + (dense ? 8.0 + 6.0 * 32.0 : 0.0)) +
	                     (rest > 0.0 ? 12.0 + 3.0 * wd + (dense ? 8.0 + 6.0 * wd : 0.0) : 0.0));
}

// ---- how many distinct sources? (the pre-pass's sampled decision; pgq_meet.hip and the lane assignment both run it) ----
struct MeetDecision {
	u32 go;           // 1: the pre-pass runs
	u32 sample_rows;  // non-NULL rows sampled
	u32 sample_fresh; // distinct sources among them
	u32 pad;
	double estimate;  // distinct sources of the whole input
};
#ifdef __HIPCC__
constexpr u32 kSampleEmpty = 0xFFFFFFFFu;
constexpr int kSampleRows = 2048, kSampleSlots = 4096;
// Every thread of ONE workgroup (any multiple of 64 threads).  s_set: kSampleSlots words of LDS the caller lends (its own
// array, or a map it is not using yet).  h_go (nullable): pinned host word that gets the verdict + 1.
__device__ __forceinline__ void sample_distinct_sources(int64_t n, const int64_t *__restrict__ src, int64_t V, double meet_bytes,
                                                        double edge_bytes, MeetDecision *__restrict__ out, u32 *__restrict__ h_go,
                                                        u32 *s_set) {
	const int nt = (int)blockDim.x;
	__shared__ u32 s_count[4];
	for (int k = threadIdx.x; k < kSampleSlots; k += nt) s_set[k] = kSampleEmpty;
	if (threadIdx.x < 4) s_count[threadIdx.x] = 0;
	__syncthreads();
	const int64_t sample = n < kSampleRows ? n : kSampleRows;
	// the sample = runs of 64 consecutive rows at evenly spaced offsets.  A join emits a cross product grouped by source:
	// single rows at a fixed stride can land on a different source every time (stride = group size) and make it look
	// like distinct pairs; inside a run a grouped input shows its repeats, and a shuffled one is sampled as well as by
	// single rows
	const double stride = (double)n / (double)((sample + 63) >> 6);
	// (round 5: every run is shifted by a pseudo-random part of its stride — offsets at exact multiples of n / 32 start every
	// run on a group boundary of a product whose groups divide that stride, and the boundary count below was off by 2x)
	auto run_start = [&](int64_t r) {
		const int64_t room = (int64_t)stride - 64;
		const int64_t jitter = room > 0 ? (int64_t)((((u64)r + 1) * 0x9E3779B97F4A7C15ull) >> 33) % room : 0;
		return (int64_t)((double)r * stride) + jitter;
	};
	// Round 5: the runs also show how the input is GROUPED.  `changes` counts the adjacent rows of a run whose sources
	// differ: a join's output (every source's rows in one stretch) changes source once per group, so n x changes / pairs
	// is its number of groups = distinct sources — which the hash-set estimate below cannot see (32 runs of a 2048 x 32
	// product hold 64 sources: "64 distinct", and the product went to the lane batches at three times the pre-pass's time).
	u32 fresh = 0, rows = 0, changes = 0, pairs = 0;
	const int64_t sample_up = (sample + 63) & ~(int64_t)63; // whole wavefronts stay in the loop for the shuffle
	for (int64_t k = threadIdx.x; k < sample_up; k += nt) {
		const bool in = k < sample;
		const int64_t at = min(n - 1, run_start(k >> 6) + (k & 63));
		const int64_t v = in ? src[at] : (int64_t)-1;
		int64_t pv = __shfl_up(v, 1);
		// a run's first row is compared with the row in front of the run: runs that start on a group boundary (evenly spaced
		// offsets and equal groups: a 2048 x 32 product sampled at stride 2048) would otherwise never see that boundary
		if ((k & 63) == 0) pv = in && at > 0 ? src[at - 1] : (int64_t)-1;
		if (in && v >= 0 && pv >= 0) {
			pairs++;
			changes += v != pv ? 1u : 0u;
		}
		if (v < 0) continue; // NULL row (or past the sample)
		rows++;
		const u32 x = (u32)v;
		u32 h = (x * 0x9E3779B1u) >> 20; // 12 bits
		for (;;) {
			const u32 old = atomicCAS(&s_set[h], kSampleEmpty, x);
			if (old == kSampleEmpty) fresh++;
			if (old == kSampleEmpty || old == x) break;
			h = (h + 1) & (kSampleSlots - 1);
		}
	}
	if (fresh) atomicAdd(&s_count[0], fresh);
	if (rows) atomicAdd(&s_count[1], rows);
	if (changes) atomicAdd(&s_count[2], changes);
	if (pairs) atomicAdd(&s_count[3], pairs);
	__syncthreads();
	// E[distinct](U) = U (1 - (1 - 1/U)^s) is increasing in U: every thread evaluates one point of a geometric grid between
	// the distinct sources seen and n ((1 - 1/U)^s as exp(s log1p(-1/U)), single precision) and the first point that
	// reaches the sampled count is the estimate — round 3 bisected on one thread (18 dependent steps: 4 of the 16 us this
	// kernel sits in front of every large call with)
	__shared__ u32 s_first;
	if (threadIdx.x == 0) s_first = (u32)nt - 1u;
	__syncthreads();
	const double d = s_count[0], sr = s_count[1];
	double est;
	if (sr < 1 || d < 1) {
		est = 1;
	} else if (d >= sr - 0.5) { // every sampled row had its own source
		est = (double)n;
	} else { // block-uniform branch
		const float fd = (float)d, fs = (float)sr, fn = (float)n;
		const float u = fd * __expf(__logf(fn / fd) * ((float)threadIdx.x / (float)(nt - 1)));
		const float e = u * (1.0f - __expf(fs * log1pf(-1.0f / u)));
		if (e >= fd) atomicMin(&s_first, threadIdx.x);
		__syncthreads();
		const float uf = fd * __expf(__logf(fn / fd) * ((float)s_first / (float)(nt - 1)));
		est = fmin((double)n, ceil((double)uf));
	}
	// grouped input (fewer than half of the adjacent sampled rows change their source): the groups counted through the
	// density of the changes.  A handful of changes in the whole sample (groups of hundreds of rows and more) is too few to
	// count by: then the first row of every run measures its own group — gallop + bisection to both ends, ~2 log2(g) loads —
	// and, a uniformly drawn row falling into a group in proportion to its length, n x mean(1 / g) is the number of groups.
	const double ch = s_count[2], pr = s_count[3];
	const bool grouped = pr >= 32.0 && ch * 2.0 < pr; // block-uniform
	__shared__ float s_inv[32];
	const int runs = (int)((sample + 63) >> 6);
	if (grouped && ch < 16.0) {
		if ((int)threadIdx.x < runs && threadIdx.x < 32) {
			const int64_t p = min(n - 1, run_start((int64_t)threadIdx.x));
			const int64_t v = src[p];
			auto extent = [&](int64_t dir) { // rows of v's stretch strictly beyond p in direction dir
				const int64_t room = dir > 0 ? n - 1 - p : p;
				int64_t step = 1;
				while (step <= room && src[p + dir * step] == v) step <<= 1;
				int64_t lo = step >> 1, hi = min(step, room + 1); // src[p + dir*lo] == v (or lo == 0); first mismatch in (lo, hi]
				while (hi - lo > 1) {
					const int64_t mid = (lo + hi) >> 1;
					if (src[p + dir * mid] == v) lo = mid;
					else hi = mid;
				}
				return lo;
			};
			s_inv[threadIdx.x] = 1.0f / (float)(1 + extent(1) + extent(-1));
		}
		__syncthreads();
	}
	if (threadIdx.x != 0) return;
	if (grouped) {
		double groups = (double)n * fmax(ch, 0.5) / pr;
		if (ch < 16.0) {
			double inv = 0;
			const int m = runs < 32 ? runs : 32;
			for (int r = 0; r < m; r++) inv += (double)s_inv[r];
			groups = (double)n * inv / (double)m;
		}
		est = fmin((double)n, fmax(d, groups));
	}
	const double distinct = fmin(est, (double)V);
	out->go = meet_bytes <= lanes_cost_bytes(edge_bytes, distinct, (double)n, (double)V) ? 1u : 0u;
	if (h_go) *h_go = out->go + 1u;
	out->sample_rows = s_count[1];
	out->sample_fresh = s_count[0];
	out->estimate = est;
}

#endif
// a sample riding in another kernel's launch (k_mark_sources: the lane assignment; k_meet4d: the pre-pass chain)
struct SampleArgs {
	double meet_bytes, edge_bytes;
	MeetDecision *out;
	u32 *h_go; // null: no sample
	int64_t n;
	const int64_t *src;
	int64_t V;
};

// What a level's kernels leave in the counter block, as the host needs it after the level (read back per level, or logged
// by the next level's k_level_reset into pinned memory when levels are enqueued ahead).
struct LevelLog {
	u64 front_edges, edges_scanned, word_gathers;
	u32 front_vertices, unresolved, front_words, pad2;
	u32 nzw; // non-empty words of the active-lane mask
	u32 r0;
};

// The per-level choices (top-down / bottom-up sparse / bottom-up dense, probe first or detect after) as one function of
// the counters, shared by the host loop and by k_level_reset, which checks an enqueued-ahead level against it.
struct LevelRule {
	double E, V, push_div, sparse_below;
	int wd, force_mode, force_pull, probe_always, use_probe;
};
enum : u32 { kLvPush = 1, kLvSparse = 2, kLvProbe = 4, kLvNone = 0x80 };
__host__ __device__ static inline u32 decide_level(const LevelRule &r, u64 front_edges, u32 front_words, u32 front_vertices,
                                                   u32 unresolved, int nzw) {
	bool push = r.force_mode == 1 || (r.force_mode == 0 && (double)front_edges * r.push_div < r.E);
	if (r.force_mode == 2) push = false;
	// expected wanted non-empty words per scanned in-edge: share of edges leaving frontier vertices x non-empty words per
	// frontier vertex x share of lane-words that still hold an active lane
	const double active_frac = (double)nzw / (double)r.wd;
	const double wpn = (double)front_edges / (r.E > 1.0 ? r.E : 1.0) *
	                   ((double)front_words / (double)(front_vertices > 1u ? front_vertices : 1u)) * active_frac;
	const bool sparse = !push && (r.force_pull == 1 || (r.force_pull == 0 && wpn < r.sparse_below));
	// The probe answers the pairs at distance t from frontier t-1 (one in-list scan per open pair) BEFORE level t is
	// expanded.  That only pays when it can spare an expensive expansion: before a top-down level (tiny) or a sparse
	// bottom-up level it costs more than it saves (cross product of 2048 sources x 32 destinations on the SF100-shaped
	// graph: the probes of levels 1 and 2 took 0.6 ms and spared nothing), before a DENSE bottom-up level (1.5 ms at WD = 32)
	// it answers what that level would have been run for.  Few open pairs: always.  In bytes at the rate the expansion
	// kernels stream: a probe is one latency-bound wavefront per open pair (measured 4.7 ns per pair at mean in-degree 89:
	// ~256 B per in-edge); a dense level moves ~E (8 + 6 WD), a sparse one ~4 E + 16 per frontier out-edge + V (4 + 24 WD), a
	// top-down one ~20 per frontier out-edge.
	bool probe = false;
	if (r.use_probe) {
		const double probe_bytes = (double)unresolved * (r.E / (r.V > 1.0 ? r.V : 1.0)) * 256.0;
		const double level_bytes = push ? (double)front_edges * 20.0
		                                : (!sparse ? r.E * (8.0 + 6.0 * r.wd)
		                                           : r.E * 4.0 + (double)front_edges * 16.0 + r.V * (4.0 + 24.0 * r.wd));
		probe = r.probe_always || probe_bytes <= level_bytes;
	}
	return (push ? kLvPush : 0u) | (sparse ? kLvSparse : 0u) | (probe ? kLvProbe : 0u);
}


struct LevelBuf {
	DevBuf buf;        // frontier lane-words [V][WD]
	DevBuf nz;         // per vertex: which of its WD words are non-empty (u32 bit mask)
	bool dirty = true; // may hold non-zero words
	// sparse pool (pgq_msbfs.hip): the allocation and the (V, WD) layout this buffer was zeroed whole for
	const void *init_buf = nullptr, *init_nz = nullptr;
	int64_t lay_V = -1;
	int lay_WD = 0;
};

// The pinned block of a workspace's pre-pass chain: the chain's last workgroup writes its report (a MeetHostBlock,
// pgq_meet.hip) at the front; two words behind it come back the same way, so that a call still waits once.
struct MeetPinned {
	alignas(16) unsigned char report[4096];
	int64_t paths_total; // shortestpath: elements of the lists the chain wrote (copied behind its scan)
	u32 sample_go;       // the sampled decision's verdict + 1 (k_meet_decide alone, riding in k_meet4d, lane_ranks); 0: none taken
	                     // (behind a finished bounded shortestpath search: the flag of the entry point's check for rows beyond the bound)
};

// One direction's search state of the batched relaxation (pgq_cheapest.hip): labels dist[V][64], the lanes of a vertex that
// improved and the queues of such vertices by round parity, and every vertex a batch labelled (once, by flag).  Between calls
// the labels are all "unlabelled" — a batch resets what it touched — for ONE (V, label type), or the array is filled whole.
struct RelaxSide {
	DevBuf dist, dirty[2], q[2], touched, tflag;
	int64_t dist_V = -1; // -1: not to be trusted (new, or a call bailed out half-way)
	int dist_tag = 0;    // relax_label_tag: 1 = int64 labels, 2 = double, 3 = 4-byte labels
	// before a worker's first batch (pgq_cheapest.hip, by its fill kernels); dist_V stays invalid until settle()
	template <typename DT> int prepare(int64_t V, int type_tag, DT inf_label, hipStream_t st);
	void settle(int64_t V, int type_tag) { dist_V = V, dist_tag = type_tag; } // behind the last batch's k_reset_touched, waited for
	void release() { for (DevBuf *b : { &dist, &dirty[0], &dirty[1], &q[0], &q[1], &touched, &tflag }) b->release(); }
};

struct Workspace {
	hipStream_t stream = nullptr;
	hipEvent_t ev_block = nullptr; // blocking event of wait_stream (created when the process first has many calls in flight)
	int device = 0; // where its buffers live (workspaces are pooled per device)
	DevBuf seen, qbuf[2], qflag, counters, flag, rank, usrc, key, idx, skey, sidx, ssrc, sdst, sres, soff,
	    sort_tmp, scan_tmp, bstart, levels_tab, child, in_src, in_dst, out_len, out_off, out_val, out_ok, lane_sums, ste, def_src, def_dst, def_len, def_idx, def_off, def_ent, cbits, cbbase, cmeta, cwords, lblk, lrec, meet_cnt, meet_rec, meet_poff, meet_maps, meet_trace, wb_scratch, hv, hmask, hstart, hmap,
	    route_dec, ball_segs, ball_trace, sort_src, sort_dst, sort_out, bi_block, dpart; // [kOpenGrid][WD + 1]: every workgroup's open-lane words + open-row count of the level's detection / probe
	std::vector<std::unique_ptr<LevelBuf>> levels; // shortestpath: one per level
	std::vector<std::unique_ptr<LevelBuf>> pool;   // otherwise: [0], [1] sparse pool, [2], [3] dense pool
	bool pool_trusted = false;                     // the last batch ended normally: the sparse pool's dirty flags are true
	int64_t prereset_V = -1;                       // batch_state_reset has run ahead for this (V, WD): the next batch's start is done
	int prereset_WD = 0;
	Counters *h_cnt = nullptr; // pinned
	LevelLog *h_log = nullptr; // pinned: [kSpecLevels + 2] counters per enqueued-ahead level, then two status words
	int64_t wb_V = -1;  // what wb_scratch's label arrays are initialised for
	int wb_grid = 0;
	MeetPinned *h_meet = nullptr; // pinned: the last workgroup of the pre-pass chain writes its statistics here
	bool meet_cnt_clean = false; // the device statistics block is all zero (the chain's last kernel leaves it so)
	// where the pre-pass left the rows it could not answer (one of the two queue regions inside def_src / def_dst / def_idx)
	int64_t *open_src = nullptr, *open_dst = nullptr;
	u32 *open_idx = nullptr;
	// chunk entry points: pinned staging block the kernels read the rows from / write the results to (device-addressable)
	void *h_io = nullptr;
	size_t h_io_cap = 0;
	int64_t *h_bstart = nullptr;
	size_t h_bstart_cap = 0;
	RelaxSide relax[2];    // cheapest path: the forward (0) and the backward (1, BidirBatches) search state; the hop-bounded rounds
	                       // (HopBatches) keep their snapshot rows and masks in [1]'s label and first dirty array and leave its dist_V at -1
	void *h_bi = nullptr;  // pinned: the bidirectional relaxation's counter block, copied back once per round
	// cheapest_path (pgq_cheapest_path.hip): tight hop counts H[V][64] (-1 = none; a batch resets what it set, tight_V says for
	// which V that holds), the frontier of a tight-level round (lane masks and vertex queues by round parity), its counters, the
	// lists of the finished batches in batch order.  tight_cnt is ONE small block that the list-producing drivers overlay their own
	// counter struct on, one call at a time (TightCounters, AspCounters, WalkCounters): each reserves kTightCntBytes and asserts
	// that its struct fits
	static constexpr size_t kTightCntBytes = 64;
	DevBuf tight_h, tight_mask[2], tight_q[2], tight_cnt, tight_stage;
	int64_t tight_V = -1;
	// cheapest_path_within (pgq_cheapest_path_within.hip): the round log of one lane batch — per entry the 512-byte label row,
	// the lanes that changed and {round, the vertex's previous entry} — and per vertex its latest entry (-1 = none; a batch
	// resets what it set, hop_last_V says for which V that holds)
	DevBuf hop_row, hop_mask, hop_ent, hop_last;
	int64_t hop_last_V = -1;
	// The nested-list calls (ListCall, pgq_path_lists.h): the rows' results in row order until the call has succeeded, and the chunk
	// form's inner list entries; the staged lists lie in tight_stage.  shortestpath_count / all_shortestpaths (pgq_all_shortest.hip)
	// keep their levels in tight_h and the tight_* frontier buffers (same invariants), sigma is block-cache memory of the call;
	// walk_count / k_shortest_walks (pgq_k_walks.hip) use tight_cnt and nothing else of the tight_* state
	DevBuf asp_rows, asp_paths;
	~Workspace();
};

struct WorkspaceLease {
	Workspace *ws = nullptr;
	int acquire();
	~WorkspaceLease();
};

// The opening of a C entry point: the handle's options for the whole call, ensure_init before any argument check (without
// a device every call answers PGQ_ERR_NO_DEVICE first), the entry's own checks, then the body.  check() returns PGQ_OK, an
// error, or kNoRows when the call is answered without a search.  body(ws) runs on a workspace leased for the call, body()
// without one (the *_multi entry points lease one per shard).  Search: the call counts towards `block_above` (wait_stream).
constexpr int kNoRows = 1;
struct NoCallScope {};
template <bool Search, typename Check, typename Body>
int c_entry(const pgq_csr *csr, Check &&check, Body &&body) {
	[[maybe_unused]] std::conditional_t<Search, CallScope, NoCallScope> in_flight;
	OptionScope opt_scope(csr);
	PGQ_TRY(ensure_init());
	const int rc = check();
	if (rc != PGQ_OK) return rc == kNoRows ? PGQ_OK : rc;
	if constexpr (std::is_invocable_v<Body &, Workspace *>) {
		WorkspaceLease lease;
		PGQ_TRY(lease.acquire());
		return body(lease.ws);
	} else {
		return body();
	}
}

// The usual checks: a handle, and the caller's arrays when there are rows (`arrays`: none of them NULL; `missing`: the
// message otherwise).
inline int check_arrays(const pgq_csr *csr, int64_t n, bool arrays, const char *missing) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	if (n < 0 || (n > 0 && !arrays)) return fail(PGQ_ERR_INVALID_ARG, missing);
	return PGQ_OK;
}

// Host staging of the entry points (pgq_runtime.hip).  n host rows into ws->in_src / ws->in_dst, queued on ws->stream.
int stage_pairs(Workspace *ws, int64_t n, const int64_t *src, const int64_t *dst);
// n 8-byte values at ws->out_val and their ok bytes at ws->out_ok into the caller's array and validity mask (a row whose ok
// byte is 0 is NULL; its payload is whatever the kernel left there); waits for ws->stream.
int download_valid(Workspace *ws, int64_t n, void *out, uint64_t *out_valid);

static inline unsigned blocks_for(int64_t n, int block = 256) {
	return (unsigned)std::max<int64_t>(1, (n + block - 1) / block);
}

// One sparse bottom-up level in lane-list form (pgq_lanes.hip): packs the frontier (front/nz) and expands it into
// next/nz_next/seen on ws->stream; per-level statistics go to d_cnt like the other level kernels.
int pull_lanes_level(pgq_csr *c, Workspace *ws, int wd, const u64 *front, const u32 *nz, u64 *seen, u64 *next,
                     u32 *nz_next, const u64 *active, int stop, Counters *d_cnt);

// Pair-centric pre-pass (pgq_meet.hip): answers rows at distance <= 3 (and NULL / trivial / dead-end rows) into d_out,
// compacts the others into ws->def_src/def_dst/def_idx; meet_apply scatters their lengths back.  decide: whether the
// pre-pass pays (distinct sources, sampled) is settled on the device in the same launch chain (DecideMode::Gate).
// shortestpath through the pre-pass: where the lists of the rows it answers go ([src, e, v, ..., dst], first-slot edges;
// entry i at the scanned offset, also stored in d_out_off[i]; a list that does not fit child_cap is not written) and how
// many elements they take
struct MeetPathsOut {
	int64_t *d_child = nullptr;
	int64_t child_cap = 0;
	int64_t *d_out_off = nullptr;
	int64_t total = 0;
};
// the lists of the rows the last meet_prepass(po) on this workspace answered, written again into po's (now larger) buffer
int meet_reemit_paths(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst, const int64_t *d_out, MeetPathsOut *po);
// Decision in front of the chain: None = the pre-pass runs; Gate = the sampled decision (k_meet_decide) gates it on the
// device; Ride = it runs ungated and the sample rides in k_meet4d's launch, for the route memo (Gate when it cannot ride).
enum class DecideMode { None, Gate, Ride };
// The source-centric kernels (pgq_ball.h) at the head of the chain: Off; Decide = the device decides whether they take the
// call; Always = they do (tests); Only = the chain is those kernels alone, the stage kernels are not launched behind them.
enum class BallMode { Off, Decide, Always, Only };
struct PrepassArgs {
	int64_t n = 0;
	const int64_t *d_src = nullptr, *d_dst = nullptr;
	int64_t *d_out = nullptr;
	MeetPathsOut *po = nullptr; // shortestpath: where the lists go
	double meet_bytes = 0, edge_bytes = 0; // the byte rule's two sides (decision kernel, source-centric kernel)
	DecideMode decide = DecideMode::None;
	BallMode ball = BallMode::Off;
	int64_t max_hops = -1; // *_within: >= 0 = rows farther apart are NULL (the kernels' bounded instantiations)
	bool no_hubs = false;  // k_meet3 does not consult the hub tables: every row is walked (the routing calibration measures the walks)
};
struct PrepassResult {
	u32 n_open = 0;              // rows left in ws->open_src / open_dst / open_idx
	bool answered = true;        // false: called off (decision, or BallMode::Only declined); nothing was written
	bool ball_attempted = false; // the source-centric kernels were launched
	bool ball_took = false;      // ... and took the call: the open rows are what they left
	double est_sources = -1.0;   // distinct sources: the decision kernel's estimate, or the source runs the ball counted
	int observed_go = -1;        // DecideMode::Ride: the sample's verdict (1 = the pre-pass pays), -1 when none was taken
	int64_t hub_settled = 0;     // rows k_meet3 answered from the hub tables instead of walking them
};
int meet_prepass(pgq_csr *c, Workspace *ws, const PrepassArgs &a, PrepassResult *r);
// the pre-pass's sampled decision alone, waited for (*go: the pre-pass pays)
int meet_decide_alone(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, double meet_bytes, double edge_bytes, bool *go);
// iterativelengthbidirectional: every row through k_bibfs (forward CSR from src, transposed CSR from dst); rows over its
// caps are compacted like the pre-pass's open rows
int meet_bidirectional(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t *d_out,
                       u32 *n_open);
// lengths + shifted offsets of the rows answered elsewhere, scattered back to row order
int meet_apply_paths(Workspace *ws, int64_t nd, const int64_t *d_len, const int64_t *d_off, int64_t base,
                     int64_t *d_out_len, int64_t *d_out_off);
int meet_apply(Workspace *ws, int64_t nd, const int64_t *d_len, int64_t *d_out);
// Assigns one lane per distinct source: fills ws->usrc (lane -> vertex), the row arrays sorted by lane
// (skey/sidx/ssrc/sdst/sres) and returns the number of distinct sources in *U.  src == dst rows are "trivial" and take no
// lane; closed_rows (walk_count / k_shortest_walks): they take one like any other row, and only those without an out-edge
// or an in-edge stay trivial.
int prepare_lanes(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst, u32 *U,
                  bool dst_rule = true, bool closed_rows = false);
// bstart (pinned host) <- sorted-row boundaries of nb batches of L lanes (+ trivial / NULL tails)
int batch_bounds(Workspace *ws, int64_t n, int64_t L, int nb);

// ---- the BFS driver (pgq_route.hip picks the route, pgq_msbfs.hip runs the lane batches) ------------------------------
// What a search is asked for beside the lengths.  The caller owns it: no callee writes into it.
struct SearchAsk {
	bool want_te = false; // fill ws->ste with per-row traversed-edge counts
	int depth = 0;        // nesting level of the straggler pass
	bool bidir = false;    // iterativelengthbidirectional: every row through the per-row bidirectional search first
	bool from_meet = false; // these rows are what the pair-centric pre-pass left open: do not run it on them again
	bool no_ball = false;   // these rows are what the source-centric kernel left open: the pre-pass may take them, that kernel not again
	int ball_hint = -1;     // the caller has looked at the rows (chunk entry points: they sit in host memory): 0 = not grouped by source
	// chunk entry points: the rows sit in a staging buffer whose address is the same for every chunk, so what the route memo
	// remembers about "these buffers" says nothing about THESE rows (round-5 advisor finding: unrelated chunks hit the memo,
	// and every change of shape was routed one call late) — such calls neither read nor write it
	bool no_memo = false;
	// iterativelength_within / shortestpath_within: >= 0 = a row whose distance exceeds it is NULL; negative = unbounded.  Every
	// stage stops where the bound lets it and the open rows' searches inherit it, but no stage is relied on to: the entry point
	// clamps what comes back (a lane batch's probes answer rows a level or two ahead, k_meet4d reports 4 for a cut row under a
	// bound of 3).  With paths a row beyond the bound must be NULL before its list is laid out (k_path_counts, batch_paths), so
	// that offsets and child_used count the rows within the bound only; the entry points check that once more.  A bounded
	// call is off the record of what unbounded calls are routed by (route memo, route timing, ball_open_frac, the refinement of
	// meet_bpr, meet_far_rows; its lane batches store no level plan): a bounded row costs something else.
	int64_t max_hops = -1;
};
// What a search reports back beside the lengths; written by the route that answered and by search_open_rows.
struct SearchReport {
	int64_t child_used = 0;  // elements of the path lists (all of them, also when they did not fit)
	bool overflow = false;   // the caller's child buffer was too small (lengths are still complete)
	int route = 0;           // 1: the source-centric kernel took the call (as it lay, or sorted by source)
	double source_runs = -1; // ... and counted this many source runs
};
// shortestpath: [src,e,v,...,dst] lists go into the caller's child buffer (d_child_ext) or ws->child, with per-row offsets
struct SearchPaths { int64_t *d_out_off = nullptr, *d_child_ext = nullptr, child_cap_ext = 0; };
// The rows of one search (-1 src = NULL row), resident in device memory, and where the answers go
struct SearchCall {
	int64_t n = 0;
	const int64_t *d_src = nullptr, *d_dst = nullptr;
	int64_t *d_out_len = nullptr;
	std::optional<SearchPaths> paths; // present: shortestpath
	SearchAsk ask;
};
// every wait of the lane-batched search on its stream is counted (pgq_stats_t::host_waits)
#define PGQ_WAIT(stream) do { PGQ_TRY(wait_stream(stream, thread_wait_event())); tstats().s.host_waits++; } while (0)
// This host thread's arena for the list payloads the chunk entry points hand out (pgq_route.hip; pgq_thread_release drops it).
std::vector<int64_t> &thread_child_arena();
// A bigger buffer with the first `keep` bytes of the old one (waited for).
int grow_keeping(DevBuf &buf, size_t bytes, size_t keep, hipStream_t st);
// Answers the call's rows by whichever route pays: the per-row bidirectional search, the source-centric kernel, the
// pair-centric pre-pass, the lane batches (pgq_route.hip).
int search_device(pgq_csr *c, Workspace *ws, const SearchCall &call, SearchReport &rep);
// SearchAsk::max_hops for a pattern's upper bound: V - 1 hops and more reach whatever is reachable, the unbounded search (-1)
int64_t search_bound(const pgq_csr *c, int64_t max_hops);
// The lane-batched MS-BFS (pgq_msbfs.hip): lane assignment, the batches, the straggler pass, results back to row order.
// sampled: the route memo sent the rows here without the pre-pass (the sample rides in the lane assignment's first launch);
// ahead_wd: the memo's width for stage 2 ahead of the wait (MemoVerdict; -1: not looked up yet).
struct LanesPlan {
	bool sampled;
	int ahead_wd;
	double meet_bytes, edge_bytes; // the byte rule's two sides, for the sample
};
int search_lanes(pgq_csr *c, Workspace *ws, const SearchCall &call, SearchReport &rep, const LanesPlan &lp);
// The route memo (pgq_csr::RouteMemo): what it says about n rows on these buffers, and what a call records there
// (fields left at -1 / false are not written; an empty outcome takes no lock).
struct MemoVerdict {
	int ball = -1, go = -1; // the source-centric kernels took (1) / declined (0) these buffers; the pre-pass (1) / lanes (0) took them
	bool sorted = false;    // ... the source-centric kernels took them after a sort by source
	int ahead_wd = -1;      // width of the last one-batch call of n rows whose rows stayed in place (0: none)
};
MemoVerdict memo_lookup(pgq_csr *c, int64_t n, const void *src, const void *dst);
struct MemoOutcome {
	int ball = -1, go = -1, sorted = -1; // ball_yes; go (the entry becomes these buffers, sorted_yes cleared); sorted_yes
	bool go_again = false;               // go = 1: the sample of a call the memo sent to the lanes says the pre-pass pays again
	int id_wd = -1;                      // the lanes' width and whether the rows stayed in place (id_n / id_wd)
	bool in_place = false;
};
void memo_record(pgq_csr *c, int64_t n, const void *src, const void *dst, const MemoOutcome &o);

// The rows a route left open (nd at src / dst), searched again one level deeper on a workspace of their own as `ask` says;
// S.pairs counts them once.  Lengths land in ws->def_len; a parent with paths: offsets in ws->def_off, lists appended behind
// `base` elements of the parent's child buffer (d_child_ext, else ws->child grown to fit; rep.overflow / rep.child_used as
// for the parent's own lists).  apply(lists appended) puts the results in place; the stream is waited for before the inner
// workspace goes back when `wait` says so or lists were appended.
struct OpenRows {
	u32 nd;
	const int64_t *src, *dst;
	SearchAsk ask; // depth, max_hops (and with it no_memo) are the parent's say: set below
	int64_t base = 0;
	bool wait = true;
};
template <typename Apply>
int search_open_rows(pgq_csr *c, Workspace *ws, const SearchCall &parent, SearchReport &rep, const OpenRows &open, Apply &&apply) {
	hipStream_t st = ws->stream;
	const u32 nd = open.nd;
	WorkspaceLease inner;
	SearchReport child_rep;
	if (nd > 0) {
		PGQ_TRY(ws->def_len.reserve((size_t)nd * 8));
		SearchCall child { nd, open.src, open.dst, ws->def_len.as<int64_t>(), std::nullopt, open.ask };
		if (parent.paths) {
			PGQ_TRY(ws->def_off.reserve((size_t)nd * 8));
			child.paths = SearchPaths { ws->def_off.as<int64_t>(), nullptr, 0 };
		}
		PGQ_TRY(inner.acquire());
		child.ask.depth = parent.ask.depth + 1;
		child.ask.max_hops = parent.ask.max_hops;
		if (child.ask.max_hops >= 0) child.ask.no_memo = true;
		tstats().s.pairs -= nd; // counted once
		PGQ_TRY(search_device(c, inner.ws, child, child_rep));
	}
	bool lists = false;
	if (parent.paths) { // the open rows' lists land in the inner workspace's child buffer: appended behind the parent's
		const int64_t need = open.base + child_rep.child_used;
		int64_t *d_child = parent.paths->d_child_ext;
		if (d_child) {
			if (need > parent.paths->child_cap_ext) rep.overflow = true;
		} else {
			if ((size_t)need * 8 > ws->child.cap) PGQ_TRY(grow_keeping(ws->child, (size_t)need * 8, (size_t)open.base * 8, st));
			d_child = ws->child.as<int64_t>();
		}
		lists = !rep.overflow; // (lengths are still reported when the lists did not fit)
		if (lists && child_rep.child_used > 0)
			PGQ_HIP_TRY(hipMemcpyAsync(d_child + open.base, inner.ws->child.p, (size_t)child_rep.child_used * 8, hipMemcpyDeviceToDevice, st));
		rep.child_used = need;
	}
	if (nd == 0) return PGQ_OK;
	PGQ_TRY(apply(lists));
	if (open.wait || lists) {
		PGQ_WAIT(st); // the inner workspace goes back to the pool after this
		KernelTimer::flush();
	}
	return PGQ_OK;
}

} // namespace pgq
