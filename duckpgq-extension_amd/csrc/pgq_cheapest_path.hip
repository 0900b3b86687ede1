// pgq_cheapest_path.hip — cheapest_path on MI355X: the cheapest path itself as a list [src, e1, v1, ..., ek, dst], next to
// the cost pgq_cheapest_path_length returns.  The reference has no counterpart (its Bellman-Ford keeps no parents,
// cheapest_path_length.cpp:52-136); the list follows shortestpath's layout (shortest_path.cpp:43-207).
//
// The root file of pgq_cheapest_path.o, with pgq_cheapest_path_within.hip included further down (PathBatches and path_call are
// theirs and nobody else's).  The labels are settled in pgq_cheapest.o — its relaxation state (RelaxSide), its lane batches and
// its k_relax launches — through pgq_relax.h: settle_every_label with a SettledBatch hook, LC, Inf, RelaxCounters::tcount,
// ensure_reverse_weights, ensure_weight_mean, check_weighted, fill32.  From pgq_path_lists.h: ListStage and
// stage_rows_null_as_minus_one.
//
// The contract.  D[v] = the labels pgq_cheapest_path_length defines: the least fixpoint of dist[n] = min(dist[n], dist[v] + w)
// from dist[src] = 0 under INF = max(T) / 2, in the reference's arithmetic (cheapest_path_length.cpp:29-36), int64 and double.
//   tight slot   a slot s of u's out-list with adj[s] = x is tight when D[u] < INF and D[u] + w[s] == D[x], the sum computed
//                exactly as the relaxation computes it (relax_sum); NaN and +inf weights are never tight
//   hop count    H[src] = 0, H[x] = 1 + min H[u] over the tight slots (u, x): the BFS levels of the tight subgraph
//   the path     for a row with D[dst] < INF and k = H[dst]: x_k = dst; for i = k .. 1, x_{i-1} = the SMALLEST u with
//                H[u] = i - 1 that has a tight slot into x_i (shortestpath's min-parent rule) and e_i = edge_ids[the FIRST tight
//                slot of that u into x_i] (its first-slot rule, among tight slots); the list is [x_0, e_1, x_1, ..., e_k, x_k]
//   special      src == dst: [src]; NULL src, NULL dst, unreachable: NULL
// Hop-minimal and not "any tight predecessor", because tight edges form cycles — zero weights, and double edges whose weight
// the label absorbs (2^53 + 1.0 == 2^53) — around which a greedy walk back never ends; down the levels of H a walk ends after
// exactly H[dst] steps.  H[dst] is finite whenever D[dst] is: the edge that last wrote a label is tight against the final
// labels, and following those edges back cannot cycle (around a cycle of them all labels are equal, so every write came after
// its predecessor's final write).  Two consequences the tests use: the left-to-right fold of the weights of e_1 .. e_k is
// pgq_cheapest_path_length's result, bit for bit; with one positive int64 weight on every edge the list is shortestpath's.
//
// Per lane batch (at most 64 distinct sources, lane l = search l, LC is pgq_relax.h's):
//   1. D settles through RelaxBatches over the plain, unsorted lists with 8-byte labels and WITHOUT the lanes' destination
//      bounds (SettledBatch / k_lane_unbound: a pruned lane leaves the labels at its bound unsettled, and a zero-weight tight edge
//      into a destination comes from exactly there).  The 4-byte labels, the light-edges-first lists, the chain pre-pass and the
//      two-ended search answer rows without leaving labels, or leave only some: this driver takes none of them.
//   2. k_tight_levels, a launch per round: the vertices whose H some lane set in the round before (queue + lane mask per
//      vertex, like k_relax's dirty words) walk their out-lists, H[n][l] is set ONCE, to the round's number, where the slot is
//      tight.  All freshness comes from kernel boundaries, as in k_relax_hops: a round reads the labels (final) and the H the
//      earlier rounds wrote, and writes one value, the round's number — two wavefronts that set the same H[n][l] in a round store
//      the same thing.  Rounds end with the frontier, or when every destination of the batch has its H (k_tight_pending).
//   3. k_cheapest_walkback, a wavefront per row: step i scans x_i's in-list (reverse CSR + the in-edge weights of
//      ensure_reverse_weights), lanes striding, for the smallest u with H[u] = i - 1 and a tight in-slot, then u's out-list for
//      the first tight slot into x_i.  Every loop is bounded by H[dst] and the lists' lengths; a step that finds nothing raises
//      the batch's error flag and the call fails with PGQ_ERR_HIP.
//   4. The batch's lists go to a staging buffer in batch order; behind the last batch the lengths are scanned in ROW order and
//      the lists gathered into the caller's child buffer (shortestpath's layout: lengths 2 H + 1, exclusive scan, fill).
// Kernel-class time: the settling is K_RELAX as ever, the level rounds are booked as K_PUSH (they are top-down frontier
// expansions), lengths / walk-back / gather as K_RECON, the staging as K_PREP.
// The hop-bounded form, pgq_cheapest_path_within, needs per-round parents — HopBatches' D_k, not D — and lives in
// pgq_cheapest_path_within.hip, on this file's staging, layout and entry points (PathBatches, path_call).
// Not built: _multi, the two-ended search, and any speed-up of the level rounds (a long list is walked by the one wavefront
// that finds it).
// H, the frontier masks and the queues (ws->tight_*) also serve pgq_all_shortest.o, which keeps its BFS levels there: the
// workspace's fields and their invariants (pgq_search.h) are all the two objects share.
#include <hipcub/hipcub.hpp>

#include <type_traits>
#include <vector>

#include "pgq_relax.h"
#include "pgq_path_lists.h"

namespace pgq {

// dist[v] + w as k_relax computes it: labels are bit patterns, a NaN weight counts as +inf (neither ever relaxes an edge)
template <typename T> __device__ __forceinline__ int64_t relax_sum(int64_t dvb, T wt) {
	if constexpr (std::is_same<T, double>::value) {
		const double ww = wt == wt ? wt : __longlong_as_double(0x7FF0000000000000ll);
		return __double_as_longlong(__longlong_as_double(dvb) + ww);
	} else {
		return (int64_t)((u64)dvb + (u64)wt);
	}
}

struct TightCounters {
	u32 nq[2];   // frontier vertices by round parity
	u32 pending; // destinations of the batch with a label and no H yet
	u32 error;   // a labelled destination without H behind the last round (1), a walk-back step without a parent (2) or slot (4)
};

// the batch's sources: H[src][lane] = 0, in the first frontier (distinct sources: distinct vertices, plain stores)
__global__ void k_tight_init(const int32_t *__restrict__ usrc, int64_t U, int64_t base, int32_t *__restrict__ H,
                             u64 *__restrict__ mask, int32_t *__restrict__ q, TightCounters *__restrict__ tc) {
	const int l = threadIdx.x;
	const int64_t g = base + l;
	if (l == 0) {
		tc->nq[0] = (u32)min((int64_t)LC, U - base);
		tc->nq[1] = 0;
		tc->pending = 0;
		tc->error = 0;
	}
	if (l >= LC || g >= U) return;
	const int v = usrc[g];
	H[(size_t)v * LC + l] = 0;
	mask[v] = 1ull << l;
	q[l] = v;
}

__global__ void k_tight_round_reset(TightCounters *__restrict__ tc, int next_par) {
	tc->nq[next_par] = 0;
	tc->pending = 0;
}

// One round: a wavefront per frontier vertex v, lane l = search l.  The lanes whose H[v] the round before set walk v's
// out-list: a tight slot into a vertex n without H gives H[n][l] = round and puts n, with the lane's bit, into the next frontier
// (the returning atomicOr says who is first to: it appends n, so a vertex is queued once per round and a queue holds <= V).
// A label below INF is a touched vertex's (k_relax's touched list), so H is only ever set where the batch's reset reaches.
template <typename T>
__global__ __launch_bounds__(256) void k_tight_levels(const int64_t *__restrict__ off, const int32_t *__restrict__ adj, const T *__restrict__ w,
                                                      const int64_t *__restrict__ dist, int32_t *__restrict__ H,
                                                      u64 *__restrict__ mask_cur, u64 *__restrict__ mask_nxt,
                                                      const int32_t *__restrict__ qcur, int32_t *__restrict__ qnxt,
                                                      TightCounters *__restrict__ tc, int par, int round) {
	const int lane = threadIdx.x & 63;
	const u32 wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
	const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
	const u32 nq = tc->nq[par];
	for (u32 i = wave; i < nq; i += nwaves) {
		const int v = qcur[i];
		const u64 m = mask_cur[v];
		const int64_t dvb = dist[(size_t)v * LC + lane];
		const int64_t b = off[v], e = off[v + 1];
		__builtin_amdgcn_wave_barrier();
		if (lane == 0) mask_cur[v] = 0; // consumed; v is in this round's queue once, nobody else touches its word
		const bool mine = ((m >> lane) & 1ull) && dvb < Inf<T>::bits;
		for (int64_t k = b; k < e; k++) {
			const int n = adj[k];
			const int64_t cand = relax_sum<T>(dvb, w[k]);
			bool fresh = false;
			if (mine && cand >= 0 && cand < Inf<T>::bits && dist[(size_t)n * LC + lane] == cand && H[(size_t)n * LC + lane] < 0) {
				H[(size_t)n * LC + lane] = round;
				fresh = true;
			}
			const u64 fm = __ballot(fresh);
			if (fm && lane == 0 && atomicOr(&mask_nxt[n], fm) == 0ull) qnxt[atomicAdd(&tc->nq[par ^ 1], 1u)] = n;
		}
	}
}

// destinations of the batch that have a label and no H yet (rows [lo, hi) are sorted by lane)
__global__ void k_tight_pending(int64_t lo, int64_t hi, const u32 *__restrict__ skey, const int32_t *__restrict__ sdst, u32 base_lane,
                                const int64_t *__restrict__ dist, const int32_t *__restrict__ H, int64_t inf_bits,
                                TightCounters *__restrict__ tc) {
	const int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool open = false;
	if (i < hi) {
		const size_t cell = (size_t)sdst[i] * LC + (skey[i] - base_lane);
		open = dist[cell] < inf_bits && H[cell] < 0;
	}
	const u64 om = __ballot(open);
	if (om && (threadIdx.x & 63) == 0) atomicAdd(&tc->pending, (u32)__popcll(om));
}

// out_len[row] = H[dst] (-1: no path), cnt[i - lo] = elements of the row's list
__global__ void k_tight_lengths(int64_t lo, int64_t hi, const u32 *__restrict__ skey, const u32 *__restrict__ sidx,
                                const int32_t *__restrict__ sdst, u32 base_lane, const int64_t *__restrict__ dist,
                                const int32_t *__restrict__ H, int64_t inf_bits, int64_t *__restrict__ out_len,
                                int64_t *__restrict__ cnt, TightCounters *__restrict__ tc) {
	const int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= hi) return;
	const size_t cell = (size_t)sdst[i] * LC + (skey[i] - base_lane);
	int64_t k = -1;
	if (dist[cell] < inf_bits) {
		k = H[cell];
		if (k < 0) tc->error = 1; // (the header's argument says this cannot happen; the call fails rather than return a wrong NULL)
	}
	out_len[sidx[i]] = k < 0 ? -1 : k;
	cnt[i - lo] = k < 0 ? 0 : 2 * k + 1;
}

// One wavefront per row: the list, written back to front into stage[loc[i - lo] ..]; soff[i] = where it starts.
template <typename T>
__global__ __launch_bounds__(64) void k_cheapest_walkback(int64_t lo, int64_t hi, const u32 *__restrict__ skey, const int32_t *__restrict__ sdst,
                                                         u32 base_lane, const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                         const T *__restrict__ w, const int64_t *__restrict__ edge_ids,
                                                         const int64_t *__restrict__ roff, const int32_t *__restrict__ radj,
                                                         const T *__restrict__ rw, const int64_t *__restrict__ dist,
                                                         const int32_t *__restrict__ H, const int64_t *__restrict__ loc, int64_t stage_base,
                                                         int64_t *__restrict__ stage, int64_t *__restrict__ soff,
                                                         TightCounters *__restrict__ tc) {
	const int lane = threadIdx.x;
	for (int64_t i = lo + blockIdx.x; i < hi; i += gridDim.x) {
		const u32 l = skey[i] - base_lane;
		int x = sdst[i];
		int64_t dx = dist[(size_t)x * LC + l];
		const int k = dx < Inf<T>::bits ? H[(size_t)x * LC + l] : -1;
		if (lane == 0) soff[i] = stage_base + loc[i - lo];
		if (k < 0) continue; // no path: no list
		int64_t *out = stage + stage_base + loc[i - lo]; // 2 k + 1 elements (k_tight_lengths)
		if (lane == 0) out[2 * k] = x;
		for (int t = k; t >= 1; t--) {
			// the smallest u with H[u] = t - 1 and a tight in-slot into x
			int best = 0x7FFFFFFF;
			const int64_t rb = roff[x], re = roff[x + 1];
			for (int64_t j = rb + lane; j < re; j += 64) {
				const int u = radj[j];
				const int64_t du = dist[(size_t)u * LC + l];
				if (u < best && du < Inf<T>::bits && H[(size_t)u * LC + l] == t - 1 && relax_sum<T>(du, rw[j]) == dx) best = u;
			}
			for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
			if (best == 0x7FFFFFFF) {
				if (lane == 0) atomicOr(&tc->error, 2u);
				break;
			}
			// its first tight slot into x
			const int64_t du = dist[(size_t)best * LC + l];
			int64_t slot = -1;
			const int64_t fb = off[best], fe = off[best + 1];
			for (int64_t e0 = fb; e0 < fe && slot < 0; e0 += 64) {
				const int64_t e = e0 + lane;
				const u64 hit = __ballot(e < fe && adj[e] == x && relax_sum<T>(du, w[e]) == dx);
				if (hit) slot = e0 + __ffsll((long long)hit) - 1;
			}
			if (slot < 0) {
				if (lane == 0) atomicOr(&tc->error, 4u);
				break;
			}
			if (lane == 0) {
				out[2 * t - 1] = edge_ids ? edge_ids[slot] : slot;
				out[2 * t - 2] = best;
			}
			x = best;
			dx = du;
		}
	}
}

// the batch is over: H back to "none" wherever it may have been set (every labelled vertex is on the touched list)
__global__ void k_tight_reset_touched(const int32_t *__restrict__ touched, const u32 *__restrict__ tcount, int32_t *__restrict__ H) {
	const u32 nt = *tcount;
	int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (; t < (int64_t)nt * LC; t += stride) H[(size_t)touched[t / LC] * LC + (t % LC)] = -1;
}

// src == dst rows: length 0; rows without a lane (NULL, or no edge to leave src / reach dst by): -1
__global__ void k_path_tails(int64_t lo_trivial, int64_t lo_null, int64_t n, const u32 *__restrict__ sidx, int64_t *__restrict__ out_len) {
	const int64_t i = lo_trivial + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) out_len[sidx[i]] = i < lo_null ? 0 : -1;
}
__global__ void k_list_counts(int64_t n, const int64_t *__restrict__ len, int64_t *__restrict__ cnt) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) cnt[i] = len[i] < 0 ? 0 : 2 * len[i] + 1;
	if (i == n) cnt[i] = 0;
}
// the staged lists (sorted positions [0, lo_trivial)) and the one-element lists of the src == dst rows into row order
__global__ void k_list_gather(int64_t lo_trivial, int64_t lo_null, const u32 *__restrict__ sidx, const int32_t *__restrict__ sdst,
                              const int64_t *__restrict__ len, const int64_t *__restrict__ soff, const int64_t *__restrict__ stage,
                              const int64_t *__restrict__ noff, int64_t *__restrict__ child) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= lo_null) return;
	const u32 row = sidx[i];
	const int64_t k = len[row];
	if (k < 0) return;
	int64_t *out = child + noff[row];
	if (i >= lo_trivial) {
		out[0] = sdst[i];
		return;
	}
	const int64_t *in = stage + soff[i];
	for (int64_t j = 0; j < 2 * k + 1; j++) out[j] = in[j];
}

// The tight levels, the walk-back and the staging of one settled batch; the layout of the whole call behind the last one.
// levels = false: the staging and the layout alone, for a driver with a walk-back of its own (cheapest_path_within).
template <typename T> class PathBatches {
public:
	PathBatches(pgq_csr *c, Workspace *ws, u32 U, int64_t *d_out_len, bool levels = true, bool closed_rows = false)
	    : stage(ws), c(c), ws(ws), U(U), d_out_len(d_out_len), levels(levels), closed_rows(closed_rows) {}

	ListStage stage; // the places of a batch's lists and the room for them: also for a driver with a walk-back of its own

	int prepare() {
		static_assert(sizeof(TightCounters) <= Workspace::kTightCntBytes, "counter block too small");
		PGQ_TRY(ws->tight_cnt.reserve(Workspace::kTightCntBytes));
		tc = ws->tight_cnt.as<TightCounters>();
		PGQ_TRY(ensure_reverse_weights(c, ws, false));
		PGQ_TRY(ensure_edge_ids(c));
		if (!levels) return PGQ_OK;
		for (DevBuf &b : ws->tight_mask) PGQ_TRY(b.reserve(Vn * 8));
		for (DevBuf &b : ws->tight_q) PGQ_TRY(b.reserve(Vn * 4));
		const size_t cells = Vn * LC;
		const bool fresh = ws->tight_h.cap < cells * 4 || ws->tight_V != c->V;
		ws->tight_V = -1; // stays invalid if the call bails out half-way
		PGQ_TRY(ws->tight_h.reserve(cells * 4));
		if (fresh) fill32(ws->tight_h.as<int32_t>(), (int64_t)cells, -1, st);
		for (DevBuf &b : ws->tight_mask) PGQ_HIP_TRY(hipMemsetAsync(b.p, 0, Vn * 8, st));
		return PGQ_OK;
	}
	void settle() { // behind the last batch's reset, waited for
		if (levels) ws->tight_V = c->V;
	}
	TightCounters *counters() const { return tc; }

	// rows [lo, hi) of the sorted arrays, lane 0 = distinct source `base`; the batch's labels are final and in place
	int batch(int64_t lo, int64_t hi, int64_t base) {
		const int64_t *dist = ws->relax[0].dist.as<int64_t>();
		int32_t *H = ws->tight_h.as<int32_t>();
		const unsigned row_blocks = blocks_for(hi - lo);
		TightCounters h {};
		{
			KernelTimer kt(st, K_PUSH);
			hipLaunchKernelGGL(k_tight_init, dim3(1), dim3(64), 0, st, ws->usrc.as<int32_t>(), (int64_t)U, base, H, ws->tight_mask[0].as<u64>(),
			                   ws->tight_q[0].as<int32_t>(), tc);
			kt.stop();
		}
		int par = 0;
		u32 nq = (u32)std::min<int64_t>(LC, (int64_t)U - base);
		bool early = false;
		for (int round = 1; nq > 0; round++) { // (at most V rounds: a vertex enters a lane's frontier once, and every round has one)
			KernelTimer kt(st, K_PUSH);
			hipLaunchKernelGGL(k_tight_round_reset, dim3(1), dim3(1), 0, st, tc, par ^ 1);
			hipLaunchKernelGGL(k_tight_levels<T>, dim3(std::min((unsigned)device_cus() * 8, std::max(1u, (nq + 3) / 4))), dim3(256), 0, st, c->off, c->adj,
			                   (const T *)c->w, dist, H, ws->tight_mask[par].as<u64>(), ws->tight_mask[par ^ 1].as<u64>(), ws->tight_q[par].as<int32_t>(),
			                   ws->tight_q[par ^ 1].as<int32_t>(), tc, par, round);
			hipLaunchKernelGGL(k_tight_pending, dim3(row_blocks), dim3(256), 0, st, lo, hi, ws->skey.as<u32>(), ws->sdst.as<int32_t>(), (u32)base, dist, H,
			                   Inf<T>::bits, tc);
			kt.stop();
			PGQ_TRY(stage.read_back(&h, tc, sizeof(h)));
			S.levels++;
			par ^= 1;
			nq = h.nq[par];
			if (h.pending == 0) { // every destination has its H: the rest of the tight subgraph is nobody's business
				early = nq > 0;
				break;
			}
		}
		// lengths, their scan, the batch's total
		const int64_t m = hi - lo;
		int64_t *loc = nullptr, total = 0, at = 0;
		PGQ_TRY(stage.place(m, [&](int64_t *const *cnt) {
			hipLaunchKernelGGL(k_tight_lengths, dim3(row_blocks), dim3(256), 0, st, lo, hi, ws->skey.as<u32>(), ws->sidx.as<u32>(), ws->sdst.as<int32_t>(),
			                   (u32)base, dist, H, Inf<T>::bits, d_out_len, cnt[0], tc);
		}, 1, &loc, &total));
		PGQ_TRY(stage.read_back(&h, tc, sizeof(h)));
		if (h.error) return fail(PGQ_ERR_HIP, "cheapest_path: internal error: a destination with a label has no tight hop count");
		PGQ_TRY(stage.stage_reserve(total, &at));
		{
			KernelTimer kt(st, K_RECON);
			hipLaunchKernelGGL(k_cheapest_walkback<T>, dim3((unsigned)std::min<int64_t>(m, 1 << 20)), dim3(64), 0, st, lo, hi, ws->skey.as<u32>(),
			                   ws->sdst.as<int32_t>(), (u32)base, c->off, c->adj, (const T *)c->w, c->edge_ids, c->roff, c->radj, (const T *)c->rw, dist, H, loc,
			                   at, ws->tight_stage.as<int64_t>(), ws->soff.as<int64_t>(), tc);
			kt.stop();
		}
		// H back to "none"; a frontier the early end left behind is dropped
		hipLaunchKernelGGL(k_tight_reset_touched, dim3((unsigned)device_cus() * 4), dim3(256), 0, st, ws->relax[0].touched.as<int32_t>(),
		                   &reinterpret_cast<RelaxCounters *>(ws->counters.p)->tcount, H);
		if (early) PGQ_HIP_TRY(hipMemsetAsync(ws->tight_mask[par].p, 0, Vn * 8, st));
		PGQ_TRY(stage.read_back(&h, tc, sizeof(h)));
		if (h.error) return fail(PGQ_ERR_HIP, "cheapest_path: internal error: the walk back found no tight parent at some step");
		return PGQ_OK;
	}

	// behind the last batch: the trivial and NULL rows' lengths, the offsets in row order, the lists where they belong.
	// d_child == nullptr: into ws->child, grown to fit (chunk form).  A child_cap that is too small: every length and offset is
	// written, no list, *overflow set.
	int layout(int64_t n, int64_t *d_out_off, int64_t *d_child, int64_t child_cap, int64_t *child_used, bool *overflow) {
		const int64_t *bs = ws->h_bstart;
		const int64_t lo_t = bs[nb_of(U) + 1], lo_n = bs[nb_of(U) + 2];
		PGQ_TRY(ws->meet_poff.reserve((size_t)(n + 1) * 8 * 2));
		int64_t *noff = ws->meet_poff.as<int64_t>(), *cnt = noff + (n + 1), total = 0;
		KernelTimer kt(st, K_RECON);
		// (closed_rows: the src == dst rows left trivial have no closed walk — NULL like the rows behind them, no [src])
		if (n > lo_t) hipLaunchKernelGGL(k_path_tails, dim3(blocks_for(n - lo_t)), dim3(256), 0, st, lo_t, closed_rows ? lo_t : lo_n, n, ws->sidx.as<u32>(), d_out_len);
		hipLaunchKernelGGL(k_list_counts, dim3(blocks_for(n + 1)), dim3(256), 0, st, n, d_out_len, cnt);
		PGQ_TRY(cub_run(ws->scan_tmp, [&](void *tmp, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(tmp, tb, cnt, noff, (int)(n + 1), st); }));
		PGQ_HIP_TRY(hipMemcpyAsync(d_out_off, noff, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
		PGQ_HIP_TRY(hipMemcpyAsync(&total, noff + n, 8, hipMemcpyDeviceToHost, st));
		PGQ_HIP_TRY(hipStreamSynchronize(st));
		*child_used = total;
		*overflow = false;
		if (!d_child) {
			PGQ_TRY(ws->child.reserve((size_t)std::max<int64_t>(total, 1) * 8));
			d_child = ws->child.as<int64_t>();
		} else if (total > child_cap) {
			*overflow = true;
		}
		if (!*overflow && lo_n > 0)
			hipLaunchKernelGGL(k_list_gather, dim3(blocks_for(lo_n)), dim3(256), 0, st, lo_t, lo_n, ws->sidx.as<u32>(), ws->sdst.as<int32_t>(), d_out_len,
			                   ws->soff.as<int64_t>(), ws->tight_stage.as<int64_t>(), noff, d_child);
		kt.stop();
		PGQ_HIP_TRY(hipStreamSynchronize(st));
		KernelTimer::flush();
		S.algo_bytes[K_RECON] += (double)total * 16.0 + (double)n * 32.0;
		return PGQ_OK;
	}
	static int nb_of(u32 U) { return (int)(((int64_t)U + LC - 1) / LC); }

private:
	pgq_csr *const c;
	Workspace *const ws;
	const u32 U;
	int64_t *const d_out_len;
	const bool levels, closed_rows;
	const hipStream_t st = ws->stream;
	const size_t Vn = (size_t)std::max<int64_t>(c->V, 1);
	pgq_stats_t &S = tstats().s;
	TightCounters *tc = nullptr;
};

// The rows of one call (device memory, src < 0 = NULL row): lengths, offsets and lists.  One worker: the batches share the
// staging buffer and the hop counts.  run(paths, nb, U) settles the nb lane batches and stages their lists through `paths`;
// levels: PathBatches' own tight levels and walk-back are part of it.  closed_rows (cheapest_walk with a lower bound): src == dst
// rows take a lane like any other, and those that cannot (no out-edge or no in-edge) are NULL.
struct PathOut {
	int64_t *d_len, *d_off, *d_child, child_cap, *child_used;
	bool *overflow;
};
template <typename T, typename Run>
static int path_call(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst, const PathOut &out, bool levels, bool closed_rows, Run &&run) {
	pgq_stats_t &S = tstats().s;
	S.pairs += n;
	*out.child_used = 0;
	*out.overflow = false;
	if (n == 0) return PGQ_OK;
	if (n >= (1LL << 31)) return fail(PGQ_ERR_INVALID_ARG, "more than 2^31-1 rows in one call");
	u32 U = 0;
	PGQ_TRY(prepare_lanes(c, ws, n, d_src, d_dst, &U, true, closed_rows));
	S.unique_sources += U;
	const int nb = PathBatches<T>::nb_of(U);
	PGQ_TRY(batch_bounds(ws, n, LC, nb));
	if (options().relax_delta_div > 0) PGQ_TRY(ensure_weight_mean(c, ws));
	PathBatches<T> paths(c, ws, U, out.d_len, levels, closed_rows);
	if (nb > 0) {
		PGQ_TRY(paths.prepare());
		PGQ_TRY(run(paths, nb, U));
		paths.settle();
	}
	return paths.layout(n, out.d_off, out.d_child, out.child_cap, out.child_used, out.overflow);
}

template <typename T> static int cheapest_path_device(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst, const PathOut &out) {
	return path_call<T>(c, ws, n, d_src, d_dst, out, true, false, [&](PathBatches<T> &paths, int nb, u32 U) {
		const SettledBatch settled { [&](int64_t lo, int64_t hi, int64_t base) { return paths.batch(lo, hi, base); } };
		return settle_every_label<T>(c, ws, nb, U, settled);
	});
}

} // namespace pgq

#include "pgq_cheapest_path_within.hip" // the hop-bounded form: HopBatches' rounds with a round log, on PathBatches' staging and layout

using namespace pgq;

extern "C" {

// max_hops: null = unbounded (cheapest_bulk's convention).  The bounded forms answer a NULL handle before anything else.
// min_hops > 0: cheapest_walk (its bounds are checked by the caller; 0 is forwarded to the _within form).
static int cheapest_path_bulk(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, const int64_t *max_hops, int64_t *d_out_len,
                              int64_t *d_out_offset, int64_t *d_child, int64_t child_cap, int64_t *child_used, int64_t min_hops = 0) {
	if (child_used) *child_used = 0;
	if (max_hops && !csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	const bool arrays = d_src && d_dst && d_out_len && d_out_offset && d_child;
	auto check = [&]() -> int {
		PGQ_TRY(check_weighted(csr));
		PGQ_TRY(check_arrays(csr, n, arrays, "NULL device array"));
		if (child_cap < 0) return fail(PGQ_ERR_INVALID_ARG, "negative child_cap");
		if (max_hops && *max_hops < 0) return fail(PGQ_ERR_INVALID_ARG, "max_hops must not be negative");
		return PGQ_OK;
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		int64_t used = 0;
		bool overflow = false;
		const PathOut out { d_out_len, d_out_offset, d_child, child_cap, &used, &overflow };
		const int rc = csr->w_type == PGQ_W_INT64 ? cheapest_path_rows<int64_t>(csr, ws, n, d_src, d_dst, out, max_hops, min_hops)
		                                          : cheapest_path_rows<double>(csr, ws, n, d_src, d_dst, out, max_hops, min_hops);
		if (child_used) *child_used = used;
		if (rc == PGQ_OK && overflow) return fail(PGQ_ERR_INVALID_ARG, "child buffer too small for the path lists (see *child_used)");
		return rc;
	});
}

static int cheapest_path_chunk(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, const int64_t *max_hops, uint64_t *out_offset,
                               uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child, uint64_t *out_child_len, int64_t min_hops = 0) {
	if (max_hops && !csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	auto check = [&]() -> int {
		PGQ_TRY(check_weighted(csr));
		if (V != csr->V) return fail(PGQ_ERR_INVALID_ARG, "V does not match the uploaded CSR");
		if (n < 0 || (n > 0 && (!out_offset || !out_length || !out_valid)) || !out_child || !out_child_len)
			return fail(PGQ_ERR_INVALID_ARG, "NULL output");
		if (max_hops && *max_hops < 0) return fail(PGQ_ERR_INVALID_ARG, "max_hops must not be negative");
		*out_child = nullptr;
		*out_child_len = 0;
		return n == 0 ? kNoRows : PGQ_OK;
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		PGQ_TRY(stage_rows_null_as_minus_one(ws, V, n, src, dst)); // NULL dst -> NULL, as in pgq_cheapest_path_length
		for (DevBuf *b : { &ws->out_len, &ws->out_off }) PGQ_TRY(b->reserve((size_t)n * 8));
		const int64_t *d_src = ws->in_src.as<int64_t>(), *d_dst = ws->in_dst.as<int64_t>();
		int64_t used = 0;
		bool overflow = false;
		const PathOut out { ws->out_len.as<int64_t>(), ws->out_off.as<int64_t>(), nullptr, 0, &used, &overflow };
		PGQ_TRY(csr->w_type == PGQ_W_INT64 ? cheapest_path_rows<int64_t>(csr, ws, n, d_src, d_dst, out, max_hops, min_hops)
		                                   : cheapest_path_rows<double>(csr, ws, n, d_src, d_dst, out, max_hops, min_hops));
		std::vector<int64_t> len(n), off(n);
		PGQ_TRY(staged_download(len.data(), ws->out_len.p, (size_t)n * 8, ws->stream));
		PGQ_TRY(staged_download(off.data(), ws->out_off.p, (size_t)n * 8, ws->stream));
		std::vector<int64_t> &arena = thread_child_arena();
		arena.resize((size_t)used);
		if (used > 0) PGQ_TRY(staged_download(arena.data(), ws->child.p, (size_t)used * 8, ws->stream));
		mask_fill_valid(out_valid, n);
		for (int64_t i = 0; i < n; i++) {
			if (len[i] < 0) {
				mask_set_invalid(out_valid, i);
				out_offset[i] = 0;
				out_length[i] = 0;
			} else {
				out_offset[i] = (uint64_t)off[i];
				out_length[i] = (uint64_t)(2 * len[i] + 1);
			}
		}
		*out_child = arena.data();
		*out_child_len = (uint64_t)used;
		return PGQ_OK;
	});
}

int pgq_cheapest_path_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t *d_out_len,
                                  int64_t *d_out_offset, int64_t *d_child, int64_t child_cap, int64_t *child_used) {
	return cheapest_path_bulk(csr, n, d_src, d_dst, nullptr, d_out_len, d_out_offset, d_child, child_cap, child_used);
}
int pgq_cheapest_path_within_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t max_hops,
                                         int64_t *d_out_len, int64_t *d_out_offset, int64_t *d_child, int64_t child_cap, int64_t *child_used) {
	return cheapest_path_bulk(csr, n, d_src, d_dst, &max_hops, d_out_len, d_out_offset, d_child, child_cap, child_used);
}
int pgq_cheapest_path(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, uint64_t *out_offset, uint64_t *out_length,
                      uint64_t *out_valid, const int64_t **out_child, uint64_t *out_child_len) {
	return cheapest_path_chunk(csr, V, n, src, dst, nullptr, out_offset, out_length, out_valid, out_child, out_child_len);
}
int pgq_cheapest_path_within(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops, uint64_t *out_offset,
                             uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child, uint64_t *out_child_len) {
	return cheapest_path_chunk(csr, V, n, src, dst, &max_hops, out_offset, out_length, out_valid, out_child, out_child_len);
}

// The cheapest walk of min_hops .. max_hops edges as a list (include/pgq_hip.h).  min_hops == 0 IS the _within call.
int pgq_cheapest_walk_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops, int64_t max_hops,
                                  int64_t *d_out_len, int64_t *d_out_offset, int64_t *d_child, int64_t child_cap, int64_t *child_used) {
	if (child_used) *child_used = 0;
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	PGQ_TRY(check_walk_bounds(min_hops, max_hops));
	return cheapest_path_bulk(csr, n, d_src, d_dst, &max_hops, d_out_len, d_out_offset, d_child, child_cap, child_used, min_hops);
}
int pgq_cheapest_walk(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops, uint64_t *out_offset,
                      uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child, uint64_t *out_child_len) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	PGQ_TRY(check_walk_bounds(min_hops, max_hops));
	return cheapest_path_chunk(csr, V, n, src, dst, &max_hops, out_offset, out_length, out_valid, out_child, out_child_len, min_hops);
}

} // extern "C"
