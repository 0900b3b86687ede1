// pgq_walk_length.hip — walk_length on MI355X: the length of the shortest walk of lower..upper edges per row, NULL where there is
// none.  `walk_length(...) IS NOT NULL` is the filter a quantified pattern -[e]->{lower,upper} needs in WALK mode; the reference's
// binder emits iterativelength BETWEEN lower AND upper instead (match.cpp:658-671), which drops a pair at distance 1 that also has a
// walk of 2 edges from {2,3} and never finds a cycle.  walk_count (> 0) and k_shortest_walks(k = 1) answer the same question with a
// V x 64 table of 8-byte counts per round, every row through whole-graph rounds; this call needs neither.
//
// Part of pgq_k_walks.o: included at the end of pgq_k_walks.hip, not compiled on its own.  k_walk_activate, WalkCounters,
// walk_query / walk_check and kWalkLimit are that file's; the chunk forms' shared pieces and LC come through pgq_path_lists.h.
//
// The contract, with W_t as pgq_k_walks.hip defines it: the smallest t in [lo, K] with W_t[dst] > 0; -1 (NULL) when there is none or
// an endpoint is NULL.  src == dst is not special.  Weights are never read; parallel edges change nothing.
//
// Stage 1, the distance (existing kernels): search_device under the bound K, off the route memo's record.  k_wl_classify then
// writes the answer of every row but those with 0 <= d < lo: NULL rows and d < 0 or d > K give -1 (no walk of at most K edges), d >= lo
// gives d (the shortest walk of at least lo edges is a shortest path).  The others — every src == dst row when lo >= 1 — are
// compacted; with lo == 0 there are none.  What stage 1's own search ran is not booked in pgq_stats_t's batches / levels / push_levels /
// pull_levels / edges_scanned: those five say what stage 2 ran (stage 1 shows in pairs, meet_pairs, ball_calls, bytes and times).
// Stage 2, bit rounds over the rows left: lane-assigned by source (prepare_lanes on the compacted rows: ws->skey / sidx / sdst /
// usrc are stage 1's no longer), batches of at most 64 sources.  Per batch two mask arrays (ping-pong) and two queues, 24 B per
// vertex.  Round t: M_t[x] = OR over in-slots (u, x) of M_{t-1}[u] — NO visited set, which is all that separates it from a BFS level.
//   push   M_t zeroed, then k_walk_activate as it is (it touches masks only); k_wl_after adds up the new queue's out-edges
//   pull   k_wl_pull: a wavefront per work item of the partition the upload built for the bottom-up kernels, a lane per in-slot,
//          64 ids and 64 words per trip (two trips in flight), OR-reduced across the wavefront; a list ends early once the word
//          holds every lane of the batch, (1 << U) - 1.  Ordinary vertices go by parts; a hub's in-list goes slice by slice over
//          several wavefronts, merged by one vector atomicOr per slice into the hub's word (zeroed by k_wl_round_reset).  Every
//          vertex's word is written: no reset.  Non-zero words are counted for the stop test.  No wavefront walks more than
//          hub_threshold entries of one list; on a graph without hubs (in-degrees at or below option hub_chunk at upload) an
//          in-list is still one wavefront's.
//   k_wl_after, a thread per row: an open row takes t if t >= lo and M_t[dst] has its lane's bit; open rows counted by ballot.
// The rounds stop behind round K, when no row is open, or when nothing is active; rows still open stay NULL.  One host wait per
// round.  Direction (option walk_length_pull: 0 push, 1 pull, 2 automatic): automatic goes dense once the queue's out-edges exceed
// E / walk_length_pull_div and stays dense, because a pull leaves no queue.
// Statistics: push rounds in push_levels, pull rounds in pull_levels, every round in levels, every batch in batches, time K_PUSH.
// Results reach the caller behind the last batch: a failed call has written nothing.
// Not built: _multi forms, K above PGQ_WALK_MAX_HOPS, a boolean-only form, the path modes, rounds enqueued ahead of the host.

namespace pgq {

__device__ __forceinline__ u64 wl_wave_or(u64 x) {
	for (int o = 32; o > 0; o >>= 1) x |= __shfl_xor(x, o);
	return x;
}

// Stage 1's distances in r become the rows' answers; the rows with 0 <= d < lo are listed (in no particular order) at crow, their
// endpoints at csrc / cdst, their number in *cnt (zeroed before).
__global__ void k_wl_classify(int64_t n, int64_t lo, int64_t hi, const int64_t *__restrict__ src, const int64_t *__restrict__ dst, int64_t *__restrict__ r,
                              int64_t *__restrict__ csrc, int64_t *__restrict__ cdst, u32 *__restrict__ crow, u32 *__restrict__ cnt) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int lane = threadIdx.x & 63;
	bool rest = false;
	if (i < n) {
		const int64_t d = r[i];
		if (src[i] < 0 || d < 0 || d > hi) r[i] = -1;
		else if (d < lo) rest = true, r[i] = -1; // (open; what it stays when no round answers it)
	}
	const u64 rm = __ballot(rest);
	if (!rm) return;
	u32 at = 0;
	if (lane == 0) at = atomicAdd(cnt, (u32)__popcll(rm));
	at = __shfl(at, 0);
	if (rest) {
		const u32 p = at + (u32)__popcll(rm & ((1ull << lane) - 1ull));
		csrc[p] = src[i];
		cdst[p] = dst[i];
		crow[p] = (u32)i;
	}
}

// The batch's lanes: M_0 and the first queue, the counters (steps = the queue's out-edges, pending = the batch's rows: all open).
__global__ void k_wl_init(const int32_t *__restrict__ usrc, int64_t U, int64_t base, const int64_t *__restrict__ off, u32 rows, u64 *__restrict__ M0,
                          int32_t *__restrict__ q, WalkCounters *__restrict__ tc) {
	const int l = threadIdx.x;
	const int64_t g = base + l;
	u64 deg = 0;
	if (g < U) {
		const int v = usrc[g];
		M0[v] = 1ull << l; // (distinct sources: distinct vertices)
		q[l] = v;
		deg = (u64)(off[v + 1] - off[v]);
	}
	for (int o = 32; o > 0; o >>= 1) deg += __shfl_xor(deg, o);
	if (l == 0) {
		tc->nq[0] = (u32)min((int64_t)LC, U - base);
		tc->nq[1] = 0;
		tc->pending = rows;
		tc->error = 0;
		tc->edges = 0;
		tc->steps = deg;
		tc->row_max = 0;
	}
}

// In front of a round: the counters it fills; pull rounds: the hubs' words, which their slices OR into.
__global__ void k_wl_round_reset(WalkCounters *__restrict__ tc, int next_par, const int32_t *__restrict__ hubs, int64_t nh, u64 *__restrict__ m_cur) {
	const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (h == 0) {
		tc->nq[next_par] = 0;
		tc->pending = 0;
		tc->steps = 0;
	}
	if (h < nh) m_cur[hubs[h]] = 0;
}

// The OR of m_prev over the in-slots [b, e) (b < e), for a whole wavefront; ends early once the word, with `seed`, holds `full`.
// Two trips of 64 slots in flight; a lane past the end re-reads slot b (same lines, masked): no load under a per-lane condition.
__device__ __forceinline__ u64 wl_or_list(int64_t b, int64_t e, int lane, const int32_t *__restrict__ radj, const u64 *__restrict__ m_prev, u64 full, u64 seed,
                                          u64 &scanned) {
	u64 acc = 0;
	for (int64_t j0 = b; j0 < e; j0 += 128) {
		const int64_t i0 = j0 + lane, i1 = i0 + 64;
		const int c0 = radj[i0 < e ? i0 : b];
		if (j0 + 64 < e) { // (wave-uniform)
			const int c1 = radj[i1 < e ? i1 : b];
			const u64 w0 = m_prev[c0], w1 = m_prev[c1];
			acc |= (i0 < e ? w0 : 0ull) | (i1 < e ? w1 : 0ull);
		} else {
			const u64 w0 = m_prev[c0];
			acc |= i0 < e ? w0 : 0ull;
		}
		scanned += (u64)min((int64_t)128, e - j0);
		if (j0 + 128 < e) {
			const u64 t = wl_wave_or(acc);
			if (((t | seed) & full) == full) return t;
		}
	}
	return wl_wave_or(acc);
}

// Round t, dense: work items 0 .. n_parts are the parts (contiguous vertex ranges without a hub), the rest the hubs' slices.
__global__ __launch_bounds__(256) void k_wl_pull(const int64_t *__restrict__ roff, const int32_t *__restrict__ radj, const int32_t *__restrict__ parts, int n_parts,
                                                 const HubItem *__restrict__ items, int64_t n_items, const u64 *__restrict__ m_prev, u64 *__restrict__ m_cur,
                                                 u64 full, WalkCounters *__restrict__ tc, int par_cur) {
	const int lane = threadIdx.x & 63;
	const int64_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
	const int64_t nwaves = (gridDim.x * blockDim.x) >> 6;
	u32 nz = 0;
	u64 scanned = 0;
	for (int64_t w = wave; w < (int64_t)n_parts + n_items; w += nwaves) {
		if (w < n_parts) {
			const int v0 = parts[2 * w], v1 = parts[2 * w + 1];
			for (int n = v0; n < v1; n++) {
				const int64_t b = roff[n], e = roff[n + 1];
				const u64 acc = b < e ? wl_or_list(b, e, lane, radj, m_prev, full, 0ull, scanned) : 0ull;
				if (lane == 0) m_cur[n] = acc;
				nz += acc != 0ull;
			}
		} else {
			const HubItem it = items[w - n_parts];
			const u64 have = __hip_atomic_load(&m_cur[it.vertex], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // what other slices have found
			if ((have & full) == full || it.begin >= it.end) continue;
			const u64 acc = wl_or_list(it.begin, it.end, lane, radj, m_prev, full, have, scanned);
			if (acc & ~have) { // (wave-uniform) the slice that finds the word at 0 counts the hub
				u64 old = 1;
				if (lane == 0) old = atomicOr(&m_cur[it.vertex], acc);
				nz += __shfl(old, 0) == 0ull;
			}
		}
	}
	if (lane == 0) {
		if (nz) atomicAdd(&tc->nq[par_cur], nz);
		if (scanned) atomicAdd(&tc->edges, scanned);
	}
}

// Round t is over.  A thread per row of the batch: an open row (res < 0) takes t when t >= lo and M_t[dst] has its lane's bit; the
// rows still open are counted.  q_cur != null (a push round): the new queue's out-edges are added up, for the direction rule.
__global__ void k_wl_after(int t, int64_t min_hops, int64_t lo, int64_t hi, const u32 *__restrict__ skey, const u32 *__restrict__ sidx,
                           const int32_t *__restrict__ sdst, u32 base_lane, const u64 *__restrict__ m_cur, const u32 *__restrict__ crow, int64_t *__restrict__ res,
                           const int64_t *__restrict__ off, const int32_t *__restrict__ q_cur, int par_cur, WalkCounters *__restrict__ tc) {
	const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (q_cur) {
		const int64_t stride = (int64_t)gridDim.x * blockDim.x;
		const int64_t nq = tc->nq[par_cur];
		u64 deg = 0;
		for (int64_t k = tid; k < nq; k += stride) {
			const int v = q_cur[k];
			deg += (u64)(off[v + 1] - off[v]);
		}
		for (int o = 32; o > 0; o >>= 1) deg += __shfl_xor(deg, o);
		if (deg && (threadIdx.x & 63) == 0) atomicAdd(&tc->steps, deg);
	}
	const int64_t i = lo + tid;
	bool open = false;
	if (i < hi) {
		const u32 row = crow[sidx[i]];
		open = res[row] < 0;
		if (open && t >= min_hops && ((m_cur[sdst[i]] >> (skey[i] - base_lane)) & 1ull)) {
			res[row] = t;
			open = false;
		}
	}
	const u64 om = __ballot(open);
	if (om && (threadIdx.x & 63) == 0) atomicAdd(&tc->pending, (u32)__popcll(om));
}

class WalkLengthCall {
public:
	WalkLengthCall(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops, int64_t max_hops, int64_t *d_out)
	    : c(c), ws(ws), n(n), d_src(d_src), d_dst(d_dst), lo_hops(min_hops), hi_hops(max_hops), d_out(d_out), stage(ws), temps(ws->stream) {}

	int run() {
		if (n == 0) return PGQ_OK;
		PGQ_TRY(temps.alloc(&res, (size_t)n));
		PGQ_TRY(distances());
		u32 rest = 0;
		if (lo_hops > 0) PGQ_TRY(classify(&rest));
		else hipLaunchKernelGGL(k_wl_classify, dim3(blocks_for(n)), dim3(256), 0, st, n, lo_hops, hi_hops, d_src, d_dst, res, (int64_t *)nullptr,
		                        (int64_t *)nullptr, (u32 *)nullptr, (u32 *)nullptr); // (no row has d < 0 <= lo: nothing is listed)
		if (rest > 0) PGQ_TRY(rounds(rest));
		PGQ_HIP_TRY(hipMemcpyAsync(d_out, res, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
		return stage.wait();
	}

private:
	pgq_csr *const c;
	Workspace *const ws;
	const int64_t n;
	const int64_t *const d_src, *const d_dst;
	const int64_t lo_hops, hi_hops;
	int64_t *const d_out;
	ListStage stage;
	DevTemps temps; // the rows' answers until the call has succeeded, the rows left, a batch's masks and queues: block-cache memory of the call
	const hipStream_t st = ws->stream;
	const size_t Vn = (size_t)std::max<int64_t>(c->V, 1);
	pgq_stats_t &S = tstats().s;
	int64_t *res = nullptr, *csrc = nullptr, *cdst = nullptr;
	u32 *crow = nullptr;
	WalkCounters *tc = nullptr;
	u64 *M[2] = { nullptr, nullptr };
	int32_t *q[2] = { nullptr, nullptr };

	// Stage 1.  What its own lane batches ran is kept out of the five counters that stage 2 reports in.
	int distances() {
		SearchCall call { n, d_src, d_dst, res };
		call.ask.max_hops = search_bound(c, hi_hops);
		call.ask.no_memo = true;
		SearchReport rep;
		const int64_t batches = S.batches, levels = S.levels, push = S.push_levels, pull = S.pull_levels, edges = S.edges_scanned;
		const int rc = search_device(c, ws, call, rep);
		S.batches = batches, S.levels = levels, S.push_levels = push, S.pull_levels = pull, S.edges_scanned = edges;
		return rc;
	}
	int classify(u32 *rest) {
		u32 *cnt = nullptr;
		PGQ_TRY(temps.alloc(&csrc, (size_t)n));
		PGQ_TRY(temps.alloc(&cdst, (size_t)n));
		PGQ_TRY(temps.alloc(&crow, (size_t)n));
		PGQ_TRY(temps.alloc(&cnt, 1));
		PGQ_HIP_TRY(hipMemsetAsync(cnt, 0, 4, st));
		hipLaunchKernelGGL(k_wl_classify, dim3(blocks_for(n)), dim3(256), 0, st, n, lo_hops, hi_hops, d_src, d_dst, res, csrc, cdst, crow, cnt);
		return stage.read_back(rest, cnt, 4);
	}

	// Stage 2 over the `m` rows left.
	int rounds(int64_t m) {
		u32 U = 0;
		PGQ_TRY(prepare_lanes(c, ws, m, csrc, cdst, &U, true, true));
		S.unique_sources += U;
		const int nb = (int)(((int64_t)U + LC - 1) / LC);
		PGQ_TRY(batch_bounds(ws, m, LC, nb));
		if (nb == 0) return PGQ_OK; // (closed rows without an out-edge or an in-edge: no walk)
		static_assert(sizeof(WalkCounters) <= Workspace::kTightCntBytes, "counter block too small");
		PGQ_TRY(ws->tight_cnt.reserve(Workspace::kTightCntBytes));
		tc = ws->tight_cnt.as<WalkCounters>();
		for (u64 *&mk : M) PGQ_TRY(temps.alloc(&mk, Vn));
		for (int32_t *&b : q) PGQ_TRY(temps.alloc(&b, Vn));
		const int64_t *bs = ws->h_bstart;
		for (int b = 0; b < nb; b++) PGQ_TRY(batch(bs[b], bs[b + 1], (int64_t)b * LC, U));
		return PGQ_OK;
	}

	// rows [lo, hi) of the sorted arrays, lane 0 = distinct source `base`
	int batch(int64_t lo, int64_t hi, int64_t base, u32 U) {
		const int64_t m = hi - lo;
		const Options &o = options();
		const unsigned cus = (unsigned)device_cus();
		const int lanes = (int)std::min<int64_t>(LC, (int64_t)U - base);
		const u64 full = lanes >= 64 ? ~0ull : (1ull << lanes) - 1ull;
		const int64_t items = (int64_t)c->n_pull_parts + c->n_pull_hub_items;
		const double dense_above = (double)c->E / (double)std::max(1, o.walk_length_pull_div);
		WalkCounters h {};
		S.batches++;
		for (u64 *mk : M) PGQ_HIP_TRY(hipMemsetAsync(mk, 0, Vn * 8, st)); // what the batch before left
		{
			KernelTimer kt(st, K_PUSH);
			hipLaunchKernelGGL(k_wl_init, dim3(1), dim3(64), 0, st, ws->usrc.as<int32_t>(), (int64_t)U, base, c->off, (u32)m, M[0], q[0], tc);
			kt.stop();
		}
		PGQ_TRY(stage.read_back(&h, tc, sizeof(h)));
		int par = 0;
		u32 active = h.nq[0];
		bool dense = o.walk_length_pull == 1;
		for (int64_t t = 1; t <= hi_hops && active > 0 && h.pending > 0; t++) {
			if (o.walk_length_pull == 2 && (double)h.steps > dense_above) dense = true; // ... and from then on
			const u64 *prev = M[(t - 1) & 1];
			u64 *cur = M[t & 1];
			KernelTimer kt(st, K_PUSH);
			hipLaunchKernelGGL(k_wl_round_reset, dim3(blocks_for(dense ? c->n_pull_hub_vertices : 1)), dim3(256), 0, st, tc, par ^ 1, c->pull_hub_vertices,
			                   dense ? c->n_pull_hub_vertices : 0, cur);
			if (dense) {
				hipLaunchKernelGGL(k_wl_pull, dim3((unsigned)std::min<int64_t>(cus * 8, std::max<int64_t>(1, (items + 3) / 4))), dim3(256), 0, st, c->roff, c->radj,
				                   c->pull_parts, c->n_pull_parts, c->pull_hubs, c->n_pull_hub_items, prev, cur, full, tc, par ^ 1);
				S.pull_levels++;
			} else {
				PGQ_HIP_TRY(hipMemsetAsync(cur, 0, Vn * 8, st));
				hipLaunchKernelGGL(k_walk_activate, dim3(std::min(cus * 8, std::max(1u, (active + 3) / 4))), dim3(256), 0, st, c->off, c->adj, prev, cur, q[par],
				                   q[par ^ 1], tc, par);
				S.push_levels++;
			}
			// (a push round's new queue is not known here: the grid takes it in strides)
			hipLaunchKernelGGL(k_wl_after, dim3(blocks_for(std::max<int64_t>(m, dense ? 1 : std::min<int64_t>((int64_t)Vn, 1 << 16)))), dim3(256), 0, st, (int)t,
			                   lo_hops, lo, hi, ws->skey.as<u32>(), ws->sidx.as<u32>(), ws->sdst.as<int32_t>(), (u32)base, cur, crow, res, c->off,
			                   dense ? (const int32_t *)nullptr : q[par ^ 1], par ^ 1, tc);
			kt.stop();
			PGQ_TRY(stage.read_back(&h, tc, sizeof(h)));
			S.levels++;
			par ^= 1;
			active = h.nq[par]; // push: queued vertices; pull: vertices with a non-zero word
		}
		S.edges_scanned += (int64_t)h.edges;
		S.algo_bytes[K_PUSH] += (double)h.edges * (4.0 + 8.0);
		return PGQ_OK;
	}
};

} // namespace pgq

using namespace pgq;

static int walk_length_check(int64_t min_hops, int64_t max_hops) { return walk_check(walk_query(min_hops, max_hops, nullptr, 0, kWalkMax), kWalkLimit); }

extern "C" {

int pgq_walk_length_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops, int64_t max_hops, int64_t *d_out_len) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	auto check = [&]() -> int {
		PGQ_TRY(check_arrays(csr, n, d_src && d_dst && d_out_len, "NULL device array"));
		return walk_length_check(min_hops, max_hops);
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int { return WalkLengthCall(csr, ws, n, d_src, d_dst, min_hops, max_hops, d_out_len).run(); });
}

int pgq_walk_length(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops, int64_t *out_len, uint64_t *out_valid) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	auto check = [&] { return count_chunk_check(csr, V, n, out_len, out_valid, [&] { return walk_length_check(min_hops, max_hops); }); };
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		auto run = [&](ListOut &o, const int64_t *d_src, const int64_t *d_dst) { return WalkLengthCall(csr, ws, n, d_src, d_dst, min_hops, max_hops, o.d_count).run(); };
		return count_chunk_body(ws, V, n, src, dst, run, out_len, out_valid);
	});
}

} // extern "C"
