// pgq_path_lists.h — what the list-producing calls share: cheapest_path and cheapest_path_within (one list per row) use the
// staging helper, all_shortestpaths and k_shortest_walks (a list of lists per row) everything.  A header like any other, included
// at the head of three translation units (pgq_cheapest_path.hip, pgq_all_shortest.hip, pgq_k_walks.hip); it takes LC from
// pgq_relax.h and the workspace from pgq_search.h.  Linkage, so that the three objects link: the device functions are
// __forceinline__ and the host functions are class members or templates, all inline as they stand; the one kernel, k_asp_tails, is
// `static` (a kernel cannot be `inline`) — internal linkage: each of the three objects holds and registers a copy of its own (a few hundred bytes;
// pgq_cheapest_path.o never launches its one), and no kernel is launched from an object that does not define it; the one plain host function, stage_rows_null_as_minus_one, is `inline`, one copy in the library.
//
// Device side, for pgq_all_shortest.hip and pgq_k_walks.hip (their headers give the contracts):
//   asp_sat_add, wave_sat_scan   the saturating add and its inclusive scan over a wavefront
//   pull_masked_sum              a vertex's in-list, 64 entries and 64 mask words per trip: the saturating sum, per lane, of the
//                                table rows of the in-neighbours whose mask word has the lane's bit
//   rank_row                     the row of a batch that a global path number belongs to
//   unrank_slot                  the forward slot of an in-slot (the m-th-slot rule below), callable alone
//   unrank_step                  one step of the unranking: the in-slot of x that rank r falls into, by a caller-given weight per
//                                candidate, and the forward slot it stands for — the m-th in-slot from u into x is the m-th slot of
//                                u's out-list into x, because the reverse CSR is the forward slot list stably sorted by target
//   k_asp_tails                  the rows without a lane
// Host side:
//   ListStage   the batches' lists in ws->tight_stage, one batch behind the other: count arrays and their scans (place), room
//               (stage_reserve), the waited-for copy of a counter block (read_back)
//   ListOut     where a nested-list call's results go
//   ListCall    the skeleton of such a call: lanes and row arrays (run), a batch's plan / scans / staging / unranking launch (emit),
//               and behind the last batch the tails, the scans in row order, capacities, the gather and the caller's arrays (layout).
//               Nothing reaches the caller's arrays before layout.
//   the C entry points' shared checks, prologues and epilogues.
#pragma once

#include <hipcub/hipcub.hpp>

#include <string>
#include <vector>

#include "pgq_relax.h"
#include "pgq_search.h"

namespace pgq {

constexpr int64_t kAspMax = 0x7FFFFFFFFFFFFFFFll;
__device__ __forceinline__ int64_t asp_sat_add(int64_t a, int64_t b) { // a, b >= 0
	const u64 s = (u64)a + (u64)b;
	return s > (u64)kAspMax ? kAspMax : (int64_t)s;
}
// saturating inclusive prefix sum over the wavefront (v >= 0): the result never falls along the lanes
__device__ __forceinline__ int64_t wave_sat_scan(int64_t inc, int lane) {
	for (int o = 1; o < 64; o <<= 1) {
		const int64_t y = __shfl_up(inc, o);
		if (lane >= o) inc = asp_sat_add(inc, y);
	}
	return inc;
}

// Vertex n's in-list for a wavefront whose lane l = search l: the saturating sum of w_prev[u][lane] over the in-slots (u, n) whose
// m_prev[u] has the lane's bit, for the lanes that `want` it (0 for the others).  64 in-neighbours and their mask words per trip, a
// ballot names those with any bit and only they are visited (in in-list order; a saturating sum of non-negative terms does not
// depend on it anyway).
__device__ __forceinline__ int64_t pull_masked_sum(int n, int lane, bool want, const int64_t *__restrict__ roff, const int32_t *__restrict__ radj,
                                                   const u64 *__restrict__ m_prev, const int64_t *__restrict__ w_prev) {
	int64_t acc = 0;
	const int64_t rb = roff[n], re = roff[n + 1];
	for (int64_t j0 = rb; j0 < re; j0 += 64) {
		const int cand = j0 + lane < re ? radj[j0 + lane] : -1;
		const u64 cm = cand >= 0 ? m_prev[cand] : 0ull;
		u64 live = __ballot(cm != 0ull);
		while (live) {
			const int bpos = __ffsll((long long)live) - 1;
			live &= live - 1;
			const int u = __shfl(cand, bpos);
			const u64 mu = __shfl(cm, bpos);
			if (want && ((mu >> lane) & 1ull)) acc = asp_sat_add(acc, w_prev[(size_t)u * LC + lane]);
		}
	}
	return acc;
}

// the row of global path number p: the last j in [0, m) with ploc[j] <= p (rows without paths share their successor's start and
// are passed over)
__device__ __forceinline__ int64_t rank_row(const int64_t *__restrict__ ploc, int64_t m, int64_t p) {
	int64_t a = 0, b = m;
	while (b - a > 1) {
		const int64_t mid = (a + b) >> 1;
		if (ploc[mid] <= p) a = mid;
		else b = mid;
	}
	return a;
}

struct UnrankStep {
	int u;        // the parent the step goes to
	int64_t slot; // the forward slot of the edge (u, x)
	u32 error;    // 0; 2: rank r lies behind x's in-list; 4: u's out-list has no such slot
};
// The forward slot that the in-slot at position jsel of x's in-list (radj[jsel] = u, the list starts at rb) stands for, for a whole
// wavefront; -1 when u's out-list has no such slot.  On its own for the path modes' search (pgq_path_modes.h), which needs a
// candidate's edge before it takes it.
__device__ __forceinline__ int64_t unrank_slot(int x, int u, int64_t jsel, int lane, int64_t rb, const int32_t *__restrict__ radj,
                                               const int64_t *__restrict__ off, const int32_t *__restrict__ adj) {
	// the taken in-slot is the mth from u into x (they are consecutive: the in-list is ordered by parent, then forward slot)
	int mth = 0;
	for (int64_t j = rb + lane; j < jsel; j += 64) mth += radj[j] == u ? 1 : 0;
	for (int o = 32; o > 0; o >>= 1) mth += __shfl_xor(mth, o);
	// ... its edge the mth slot of u's out-list into x
	int64_t slot = -1;
	const int64_t fb = off[u], fe = off[u + 1];
	for (int64_t e0 = fb; e0 < fe && slot < 0; e0 += 64) {
		const int64_t e = e0 + lane;
		u64 hm = __ballot(e < fe && adj[e] == x);
		const int c = __popcll(hm);
		if (mth < c) {
			for (int k = 0; k < mth; k++) hm &= hm - 1;
			slot = e0 + __ffsll((long long)hm) - 1;
		} else {
			mth -= c;
		}
	}
	return slot;
}

// One step of the unranking, a wavefront at x with rank r (uniform over the lanes): x's in-list in its stored order, 64 positions
// at a time; weight(cand) = the paths that reach x through candidate cand (0: not a parent).  The first position whose inclusive
// prefix sum passes r is taken and r loses the exclusive prefix.
template <typename Weight>
__device__ __forceinline__ UnrankStep unrank_step(int x, int64_t &r, int lane, const int64_t *__restrict__ roff, const int32_t *__restrict__ radj,
                                                  const int64_t *__restrict__ off, const int32_t *__restrict__ adj, Weight &&weight) {
	const int64_t rb = roff[x], re = roff[x + 1];
	int64_t jsel = -1;
	int u = -1;
	for (int64_t j0 = rb; j0 < re; j0 += 64) {
		const int64_t j = j0 + lane;
		const int cand = j < re ? radj[j] : -1;
		const int64_t upto = wave_sat_scan(cand >= 0 ? weight(cand) : 0, lane);
		int64_t before = __shfl_up(upto, 1);
		if (lane == 0) before = 0;
		const u64 hit = __ballot(r < upto); // upto never falls along the lanes: the first lane past r holds the slot
		if (hit) {
			const int pos = __ffsll((long long)hit) - 1;
			r -= __shfl(before, pos);
			u = __shfl(cand, pos);
			jsel = j0 + pos;
			break;
		}
		r -= __shfl(upto, 63); // (<= r, so it is a true sum)
	}
	if (jsel < 0) return UnrankStep { -1, -1, 2u };
	const int64_t slot = unrank_slot(x, u, jsel, lane, rb, radj, off, adj);
	return UnrankStep { u, slot, slot < 0 ? 4u : 0u };
}

// Rows without a lane.  Trivial ([lo_trivial, lo_null)): src == dst — one list, [src], of no hops when min_hops == 0, nothing
// otherwise; the others: a NULL endpoint (count -1) or a row that cannot have a path (0).  r_np == null: the counts alone.
// r_ng != null (k_shortest_groups): the row's groups, 1 with the list and 0 without.
[[maybe_unused]] static __global__ void k_asp_tails(int64_t lo_trivial, int64_t lo_null, int64_t n, int64_t min_hops, const u32 *__restrict__ sidx, const int64_t *__restrict__ src,
                            const int64_t *__restrict__ dst, int64_t *__restrict__ r_len, int64_t *__restrict__ r_count, int64_t *__restrict__ r_np,
                            int64_t *__restrict__ r_el, int64_t *__restrict__ r_ng) {
	const int64_t i = lo_trivial + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const u32 row = sidx[i];
	const bool one = i < lo_null && min_hops == 0;
	r_len[row] = one ? 0 : -1;
	r_count[row] = one ? 1 : (i >= lo_null && (src[row] < 0 || dst[row] < 0) ? -1 : 0);
	if (r_np) r_np[row] = r_el[row] = one ? 1 : 0;
	if (r_ng) r_ng[row] = one ? 1 : 0;
}

// The lists of a call's finished batches lie behind each other in ws->tight_stage; a batch's rows get their places there from
// count arrays (ws->def_len) and their exclusive scans (ws->def_ent).
class ListStage {
public:
	explicit ListStage(Workspace *ws) : ws(ws) {}

	int wait() {
		PGQ_HIP_TRY(hipStreamSynchronize(st));
		KernelTimer::flush();
		return PGQ_OK;
	}
	int read_back(void *host, const void *dev, size_t bytes) {
		PGQ_HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
		return wait();
	}
	// The places of a batch's m rows.  fill(cnt) enqueues the kernel that writes every row's count into each of the ncounts (1 or
	// 2) arrays cnt[0 .. ncounts), m + 1 entries each; loc[c] = the exclusive scan of cnt[c]; totals[c] (its sum) is on its way to
	// the host: there once the stream has been waited for.
	template <typename Fill> int place(int64_t m, Fill &&fill, int ncounts, int64_t **loc, int64_t *totals) {
		PGQ_TRY(ws->def_len.reserve((size_t)(m + 1) * 8 * ncounts));
		PGQ_TRY(ws->def_ent.reserve((size_t)(m + 1) * 8 * ncounts));
		int64_t *cnt[2] = { ws->def_len.as<int64_t>(), ws->def_len.as<int64_t>() + (m + 1) };
		for (int k = 0; k < ncounts; k++) loc[k] = ws->def_ent.as<int64_t>() + k * (m + 1);
		KernelTimer kt(st, K_RECON);
		// the entry behind the last row counts nothing (two arrays: one memset over both)
		if (ncounts == 1) PGQ_HIP_TRY(hipMemsetAsync(cnt[0] + m, 0, 8, st));
		else PGQ_HIP_TRY(hipMemsetAsync(cnt[0], 0, (size_t)(m + 1) * 8 * 2, st));
		fill(cnt);
		for (int k = 0; k < ncounts; k++)
			PGQ_TRY(cub_run(ws->scan_tmp, [&](void *tmp, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(tmp, tb, cnt[k], loc[k], (int)(m + 1), st); }));
		kt.stop();
		for (int k = 0; k < ncounts; k++) PGQ_HIP_TRY(hipMemcpyAsync(&totals[k], loc[k] + m, 8, hipMemcpyDeviceToHost, st));
		return PGQ_OK;
	}
	// room for `total` more elements in the staging buffer, behind the finished batches' lists: *at = where they start
	int stage_reserve(int64_t total, int64_t *at) {
		const size_t need = (size_t)(staged + total) * 8;
		if (need > ws->tight_stage.cap) PGQ_TRY(grow_keeping(ws->tight_stage, std::max(need, 2 * ws->tight_stage.cap), (size_t)staged * 8, st));
		*at = staged;
		staged += total;
		tstats().s.algo_bytes[K_RECON] += (double)total * 8.0;
		return PGQ_OK;
	}

private:
	Workspace *const ws;
	const hipStream_t st = ws->stream;
	int64_t staged = 0; // elements of the finished batches' lists
};

// Where a nested-list call's results go.  lists = false: the counts alone (d_count).  External buffers (bulk form) with their
// capacities, or none (chunk form): then the inner entries and the payload land in ws->asp_paths / ws->child, grown to fit.
struct ListOut {
	bool lists = false;
	int64_t limit = 1; // AspCall's max_paths (WalkCall reads its WalkQuery's limit)
	int64_t *d_len = nullptr, *d_count = nullptr, *d_first = nullptr, *d_np = nullptr;
	int64_t *d_ng = nullptr; // k_shortest_groups only: the groups among a row's lists
	int64_t *d_path_off = nullptr, *d_path_hops = nullptr, path_cap = 0, *d_child = nullptr, child_cap = 0; // d_path_hops: k_shortest_walks only
	bool external = false;
	int64_t paths_used = 0, child_used = 0;
	bool overflow = false;
};

// The skeleton of shortestpath_count / all_shortestpaths (AspCall) and walk_count / k_shortest_walks (WalkCall).  `name` and `noun`
// ("paths" / "walks") go into the error texts.
class ListCall {
protected:
	ListCall(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst, ListOut &out, const char *name, const char *noun)
	    : c(c), ws(ws), n(n), d_src(d_src), d_dst(d_dst), out(out), name(name), noun(noun), stage(ws) {}

	pgq_csr *const c;
	Workspace *const ws;
	const int64_t n;
	const int64_t *const d_src, *const d_dst;
	ListOut &out;
	const std::string name, noun;
	ListStage stage;
	const hipStream_t st = ws->stream;
	const size_t Vn = (size_t)std::max<int64_t>(c->V, 1);
	pgq_stats_t &S = tstats().s;
	// the rows' results, in row order: hops (of the first list), count, lists, elements, first list, first element (n + 1 entries each)
	int64_t *r_len = nullptr, *r_count = nullptr, *r_np = nullptr, *r_el = nullptr, *r_first = nullptr, *r_eoff = nullptr;
	int64_t *r_ng = nullptr; // a seventh, for the call that has out.d_ng: the groups (k_shortest_groups; during its rounds the groups seen)

	int too_many() const { return fail(PGQ_ERR_UNSUPPORTED, name + ": the call would emit more than 2^31-1 " + noun); }
	// what the unranking kernel left in its batch's error flag
	int unrank_status(u32 error) const {
		return error ? fail(PGQ_ERR_HIP, name + ": internal error: the unranking lost its way (no parent, no slot, or not at the source)") : PGQ_OK;
	}

	// Lanes, batch bounds and row arrays; prepare() once when there is a batch, batch(lo, hi, base, U) for the rows [lo, hi) of the
	// sorted arrays whose lane 0 is distinct source `base`; finish(nb) behind the last batch, waited for: it ends in layout.
	template <typename Prepare, typename Batch, typename Finish> int run(bool closed_rows, Prepare &&prepare, Batch &&batch, Finish &&finish) {
		S.pairs += n;
		if (n == 0) return PGQ_OK;
		if (n >= (1LL << 31)) return fail(PGQ_ERR_INVALID_ARG, "more than 2^31-1 rows in one call");
		u32 U = 0;
		PGQ_TRY(prepare_lanes(c, ws, n, d_src, d_dst, &U, true, closed_rows));
		S.unique_sources += U;
		const int nb = (int)(((int64_t)U + LC - 1) / LC);
		PGQ_TRY(batch_bounds(ws, n, LC, nb));
		PGQ_TRY(ws->asp_rows.reserve((size_t)(n + 1) * 8 * (out.d_ng ? 7 : 6)));
		int64_t *rows = ws->asp_rows.as<int64_t>();
		r_len = rows, r_count = rows + (n + 1), r_np = rows + 2 * (n + 1), r_el = rows + 3 * (n + 1), r_first = rows + 4 * (n + 1), r_eoff = rows + 5 * (n + 1);
		if (out.d_ng) r_ng = rows + 6 * (n + 1);
		if (nb > 0) {
			PGQ_TRY(prepare());
			const int64_t *bs = ws->h_bstart;
			for (int b = 0; b < nb; b++) PGQ_TRY(batch(bs[b], bs[b + 1], (int64_t)b * LC, U));
			PGQ_TRY(stage.wait());
		}
		return finish(nb);
	}

	// A batch's lists, from the end of its rounds to the unranking launch.  plan(cntp, cnte) enqueues the kernel that writes the
	// lists and the staged elements of each of the batch's m rows; unrank(lists, ploc, eloc, at) the one that writes them, `at`
	// being where the batch's block of tight_stage starts.  The caller reads the error flag back.  planned(), if given, runs once
	// the plan kernel has been waited for: what it returns other than PGQ_OK ends the batch before anything is staged.
	template <typename Plan, typename Unrank> int emit(int64_t m, Plan &&plan, Unrank &&unrank) {
		return emit(m, plan, unrank, [] { return PGQ_OK; });
	}
	template <typename Plan, typename Unrank, typename Planned> int emit(int64_t m, Plan &&plan, Unrank &&unrank, Planned &&planned) {
		int64_t *loc[2], totals[2] = { 0, 0 }, at = 0;
		PGQ_TRY(stage.place(m, [&](int64_t *const *cnt) { if (m > 0) plan(cnt[0], cnt[1]); }, 2, loc, totals));
		PGQ_TRY(stage.wait());
		PGQ_TRY(planned());
		emitted += totals[0];
		if (emitted > 0x7FFFFFFFll) return too_many();
		PGQ_TRY(stage.stage_reserve(totals[1], &at));
		if (totals[0] > 0) {
			KernelTimer kt(st, K_RECON);
			unrank(totals[0], loc[0], loc[1], at);
			kt.stop();
		}
		return PGQ_OK;
	}

	// Behind the last batch: the trivial and NULL rows, the scans in row order, capacities, the gather, the caller's arrays.
	// gather(lo_trivial, lo_null, path_off, path_len, child) enqueues the kernel that moves the staged lists to row order.  On
	// overflow d_len, d_count and d_np are complete, d_first and the payload are not written.
	template <typename Gather> int layout(int nb, int64_t min_hops, Gather &&gather, double bytes_per_path) {
		const int64_t *bs = ws->h_bstart;
		const int64_t lo_t = bs[nb + 1], lo_n = bs[nb + 2];
		int64_t totals[2] = { 0, 0 };
		KernelTimer kt(st, K_RECON);
		if (n > lo_t)
			hipLaunchKernelGGL(k_asp_tails, dim3(blocks_for(n - lo_t)), dim3(256), 0, st, lo_t, lo_n, n, min_hops, ws->sidx.as<u32>(), d_src, d_dst, r_len, r_count,
			                   out.lists ? r_np : nullptr, r_el, out.lists ? r_ng : nullptr);
		if (!out.lists) {
			PGQ_HIP_TRY(hipMemcpyAsync(out.d_count, r_count, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
			kt.stop();
			return stage.wait();
		}
		PGQ_HIP_TRY(hipMemsetAsync(r_np + n, 0, 8, st));
		PGQ_HIP_TRY(hipMemsetAsync(r_el + n, 0, 8, st));
		PGQ_TRY(cub_run(ws->scan_tmp, [&](void *tmp, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(tmp, tb, r_np, r_first, (int)(n + 1), st); }));
		PGQ_TRY(cub_run(ws->scan_tmp, [&](void *tmp, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(tmp, tb, r_el, r_eoff, (int)(n + 1), st); }));
		PGQ_HIP_TRY(hipMemcpyAsync(&totals[0], r_first + n, 8, hipMemcpyDeviceToHost, st));
		PGQ_HIP_TRY(hipMemcpyAsync(&totals[1], r_eoff + n, 8, hipMemcpyDeviceToHost, st));
		PGQ_HIP_TRY(hipStreamSynchronize(st));
		if (totals[0] > 0x7FFFFFFFll) return too_many();
		out.paths_used = totals[0];
		out.child_used = totals[1];
		int64_t *path_off = out.d_path_off, *path_len = nullptr, *child = out.d_child;
		if (!out.external) {
			PGQ_TRY(ws->asp_paths.reserve((size_t)std::max<int64_t>(totals[0], 1) * 8 * 2));
			PGQ_TRY(ws->child.reserve((size_t)std::max<int64_t>(totals[1], 1) * 8));
			path_off = ws->asp_paths.as<int64_t>();
			path_len = path_off + std::max<int64_t>(totals[0], 1);
			child = ws->child.as<int64_t>();
		} else if (totals[0] > out.path_cap || totals[1] > out.child_cap) {
			out.overflow = true;
		}
		if (!out.overflow && lo_n > 0) gather(lo_t, lo_n, path_off, path_len, child);
		PGQ_HIP_TRY(hipMemcpyAsync(out.d_len, r_len, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
		PGQ_HIP_TRY(hipMemcpyAsync(out.d_count, r_count, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
		PGQ_HIP_TRY(hipMemcpyAsync(out.d_np, r_np, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
		if (out.d_ng) PGQ_HIP_TRY(hipMemcpyAsync(out.d_ng, r_ng, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
		if (!out.overflow) PGQ_HIP_TRY(hipMemcpyAsync(out.d_first, r_first, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
		kt.stop();
		PGQ_TRY(stage.wait());
		S.algo_bytes[K_RECON] += (double)totals[1] * 16.0 + (double)totals[0] * bytes_per_path + (double)n * 64.0;
		return PGQ_OK;
	}

private:
	int64_t emitted = 0; // lists of the finished batches
};

// ---- the C entry points' shared pieces --------------------------------------------------------------------------------------

// the chunk forms' rows on the device: NULL src or NULL dst -> -1
inline int stage_rows_null_as_minus_one(Workspace *ws, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst) {
	FlatPairs fp;
	PGQ_TRY(flatten_pairs(V, n, src, dst, fp, true));
	for (int64_t i = 0; i < n; i++)
		if (!fp.dst_valid[i]) fp.src[i] = -1;
	return stage_pairs(ws, n, fp.src.data(), fp.dst.data());
}

// The count forms (shortestpath_count, walk_count).  bounds(): the call's own argument checks.
template <typename Bounds> static int count_chunk_check(const pgq_csr *csr, int64_t V, int64_t n, const int64_t *out_count, const uint64_t *out_valid, Bounds &&bounds) {
	if (V != csr->V) return fail(PGQ_ERR_INVALID_ARG, "V does not match the uploaded CSR");
	if (n < 0 || (n > 0 && (!out_count || !out_valid))) return fail(PGQ_ERR_INVALID_ARG, "NULL output");
	PGQ_TRY(bounds());
	return n == 0 ? kNoRows : PGQ_OK;
}
// run(out, d_src, d_dst) answers the staged rows into out.d_count
template <typename Run> static int count_chunk_body(Workspace *ws, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, Run &&run, int64_t *out_count, uint64_t *out_valid) {
	PGQ_TRY(stage_rows_null_as_minus_one(ws, V, n, src, dst));
	PGQ_TRY(ws->out_len.reserve((size_t)n * 8));
	ListOut out;
	out.d_count = ws->out_len.as<int64_t>();
	PGQ_TRY(run(out, ws->in_src.as<int64_t>(), ws->in_dst.as<int64_t>()));
	PGQ_TRY(staged_download(out_count, ws->out_len.p, (size_t)n * 8, ws->stream));
	mask_fill_valid(out_valid, n);
	for (int64_t i = 0; i < n; i++)
		if (out_count[i] < 0) mask_set_invalid(out_valid, i);
	return PGQ_OK;
}

// The list forms (all_shortestpaths, k_shortest_walks): the chunk form's outputs
struct ListChunkOut {
	uint64_t *first, *npaths, *valid;
	const uint64_t **path_offset, **path_length;
	uint64_t *path_total;
	const int64_t **child;
	uint64_t *child_len;
	uint64_t *ngroups = nullptr; // k_shortest_groups only
};
template <typename Bounds> static int list_chunk_check(const pgq_csr *csr, int64_t V, int64_t n, const ListChunkOut &o, Bounds &&bounds) {
	if (V != csr->V) return fail(PGQ_ERR_INVALID_ARG, "V does not match the uploaded CSR");
	if (n < 0 || (n > 0 && (!o.first || !o.npaths || !o.valid)) || !o.path_offset || !o.path_length || !o.path_total || !o.child || !o.child_len)
		return fail(PGQ_ERR_INVALID_ARG, "NULL output");
	PGQ_TRY(bounds());
	*o.path_offset = *o.path_length = nullptr;
	*o.child = nullptr;
	*o.path_total = *o.child_len = 0;
	return n == 0 ? kNoRows : PGQ_OK;
}
// run(out, d_src, d_dst) answers the staged rows into the workspace; then one arena block, filled whole before the caller's arrays
// are touched: the child payload, then the inner entries' offsets and lengths
template <typename Run> static int list_chunk_body(Workspace *ws, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t limit, Run &&run, const ListChunkOut &o) {
	PGQ_TRY(stage_rows_null_as_minus_one(ws, V, n, src, dst));
	PGQ_TRY(ws->out_len.reserve((size_t)n * 8 * (o.ngroups ? 3 : 2)));
	PGQ_TRY(ws->out_off.reserve((size_t)n * 8 * 2));
	ListOut out;
	out.lists = true;
	out.limit = std::min<int64_t>(limit, 1LL << 31);
	out.d_len = ws->out_len.as<int64_t>(), out.d_count = out.d_len + n, out.d_first = ws->out_off.as<int64_t>(), out.d_np = out.d_first + n;
	if (o.ngroups) out.d_ng = out.d_len + 2 * n;
	PGQ_TRY(run(out, ws->in_src.as<int64_t>(), ws->in_dst.as<int64_t>()));
	std::vector<int64_t> len(n), first_np((size_t)2 * n), ng(o.ngroups ? (size_t)n : 0);
	PGQ_TRY(staged_download(len.data(), ws->out_len.p, (size_t)n * 8, ws->stream));
	if (o.ngroups) PGQ_TRY(staged_download(ng.data(), out.d_ng, (size_t)n * 8, ws->stream));
	PGQ_TRY(staged_download(first_np.data(), ws->out_off.p, (size_t)n * 8 * 2, ws->stream));
	const size_t P = (size_t)out.paths_used, C = (size_t)out.child_used;
	std::vector<int64_t> &arena = thread_child_arena();
	arena.resize(C + 2 * P);
	if (C > 0) PGQ_TRY(staged_download(arena.data(), ws->child.p, C * 8, ws->stream));
	if (P > 0) {
		PGQ_TRY(staged_download(arena.data() + C, ws->asp_paths.p, P * 8, ws->stream));
		PGQ_TRY(staged_download(arena.data() + C + P, ws->asp_paths.as<int64_t>() + P, P * 8, ws->stream));
	}
	mask_fill_valid(o.valid, n);
	for (int64_t i = 0; i < n; i++) {
		if (len[i] < 0) {
			mask_set_invalid(o.valid, i);
			o.first[i] = 0;
			o.npaths[i] = 0;
		} else {
			o.first[i] = (uint64_t)first_np[i];
			o.npaths[i] = (uint64_t)first_np[(size_t)n + i];
		}
		if (o.ngroups) o.ngroups[i] = (uint64_t)ng[i];
	}
	*o.child = arena.data();
	*o.child_len = (uint64_t)C;
	*o.path_offset = reinterpret_cast<const uint64_t *>(arena.data() + C);
	*o.path_length = reinterpret_cast<const uint64_t *>(arena.data() + C + P);
	*o.path_total = (uint64_t)P;
	return PGQ_OK;
}
// The bulk list forms: run(out) answers the rows into the caller's buffers.  *paths_used / *child_used are what `out` says after
// the run, whatever it returned: 0 unless the layout got as far as the totals.
template <typename Run> static int list_bulk_body(ListOut &out, int64_t limit, Run &&run, int64_t *paths_used, int64_t *child_used) {
	out.lists = true, out.external = true;
	out.limit = std::min<int64_t>(limit, 1LL << 31);
	const int rc = run(out);
	if (paths_used) *paths_used = out.paths_used;
	if (child_used) *child_used = out.child_used;
	if (rc == PGQ_OK && out.overflow) return fail(PGQ_ERR_INVALID_ARG, "path or child buffer too small for the lists (see *paths_used, *child_used)");
	return rc;
}

} // namespace pgq
