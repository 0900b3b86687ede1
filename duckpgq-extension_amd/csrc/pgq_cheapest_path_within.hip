// pgq_cheapest_path_within.hip — cheapest_path_within on MI355X: the cheapest walk of at most `max_hops` edges itself, as a
// list [src, e1, v1, ..., eh, dst], next to the cost pgq_cheapest_path_length_within returns.  The reference has no
// counterpart; the list follows shortestpath's layout, the tie-breaks are shortestpath's and pgq_cheapest_path's.
//
// Part of pgq_cheapest_path.o: included by pgq_cheapest_path.hip behind PathBatches and path_call, whose staging, layout and
// child-capacity protocol it uses; not compiled on its own.  The rounds are HopBatches' in pgq_cheapest.o (k_relax_hops, one edge
// per round), reached through pgq_relax.h: hop_rounds_logged with a HopLog hook, LC, Inf, RelaxCounters::tcount, fill32.
//
// The contract.  D_0 .. D_K = the labels of pgq_cheapest_path_length_within for the row's source and K = max_hops (HopBatches'
// header), INF = max(T) / 2, every sum computed as the relaxation computes it (relax_sum); NaN and +inf weights never relax an
// edge and are never tight.
//   NULL         D_K[dst] == INF, or a NULL src or dst.  src == dst: [src], for every K >= 0.
//   h            the smallest k with D_k[dst] == D_K[dst] as bit patterns: the fewest edges among the cheapest walks of at most
//                K edges.  d_out_len = h.
//   the path     x_h = dst; for i = h .. 1, x_{i-1} = the SMALLEST u with D_{i-1}[u] < INF and a slot (u, x_i) with
//                relax_sum(D_{i-1}[u], w[s]) == D_i[x_i], and e_i = edge_ids[the FIRST such slot of u's out-list into x_i].
//                The list is [x_0, e_1, x_1, ..., e_h, x_h], and x_0 = src.
// Facts the walk-back and the tests rest on.
//   1. Level by level.  D_k[v] never rises with k, and D_h[dst] < D_{h-1}[dst] by the choice of h: dst improved strictly in
//      round h.  Let x_i have improved strictly in round i, D_i[x_i] < D_{i-1}[x_i], and let u be tight for it:
//      D_{i-1}[u] + w == D_i[x_i].  Had u reached D_{i-1}[u] already in a round j < i - 1 (D_j[u] == D_{i-1}[u]), round j + 1
//      would have offered D_j[u] + w to x_i: D_{j+1}[x_i] <= D_i[x_i] with j + 1 <= i - 1, so D_{i-1}[x_i] <= D_i[x_i], against
//      the strict improvement.  So every tight parent improved strictly in round i - 1, exactly; a tight parent exists, since
//      the round's minimum was offered by some edge.  By induction the walk-back takes exactly h steps; at step 0 it stands on
//      a vertex that "improved in round 0", and only src did.  It cannot loop on zero-weight cycles or on cycles a double label
//      absorbs: every step goes down one round.  Nothing here depends on the weight type.
//   2. Fold.  D_i[x_i] = D_{i-1}[x_{i-1}] + w(e_i) at every step and D_0[src] = 0, so the left-to-right fold of the weights of
//      e_1 .. e_h is D_h[dst] = D_K[dst], pgq_cheapest_path_length_within's value bit for bit; h <= K.
//   3. Unit weights.  With one positive int64 weight c on every edge D_k[v] = c x (hops to v) once v is within k hops, every
//      edge from level i - 1 to level i is tight, and the rules above are shortestpath_within's.
//   4. K >= V - 1.  D_k stands still from k = V - 1 on, so such a K is K = V - 1.  For int64 weights the list is then
//      pgq_cheapest_path's: sums are exact, a tight walk is a cheapest walk and vice versa, and that call's H[u] is the first
//      round that shows D[u].  For double weights the two lists CAN DIFFER: edges 0->2 (1.0), 0->1 (0.25), 1->2 (0.25),
//      2->3 (2^53).  Round 2 labels vertex 3 with 1.0 + 2^53 == 2^53; round 3 offers 0.5 + 2^53, the same bits, no improvement.
//      This call answers [0, ., 2, ., 3] (h = 2) for every K >= 2; pgq_cheapest_path follows the final label 0.5 of vertex 2 and
//      answers [0, ., 1, ., 2, ., 3].  Both fold to 2^53.  So a large K is NOT forwarded to pgq_cheapest_path: the hop rounds
//      run until the queue is empty.
//
// Per lane batch (one worker; lane l = search l, LC is pgq_relax.h's):
//   1. The rounds are HopBatches' with a HopLog: in k_hop_snapshot's place k_hop_log APPENDS the queue's label rows to a log
//      instead of overwriting last round's.  Entry g: the 512-byte row of its vertex v as it stood after round r (every lane,
//      changed or not), the mask of the lanes that changed in round r, r, and prev[g], v's entry before this one;
//      hop_last[v] = v's latest entry.  k_relax_hops reads the round's slice of the log (pointer + base): the rounds move the
//      bytes the length call's move.  A vertex is in a round's queue once, so the wavefront that logs it is the only writer of
//      hop_last[v] and the only reader of its old value in that launch: no atomics; freshness comes from kernel boundaries.
//      Behind the batch's last round — at the bound, or on an empty queue — one more pass logs the vertices that round changed
//      and takes their dirty words (the length call's memset of the "stopped at the bound" case is not needed here).
//      D_j[v] is then the row of v's latest entry with round <= j, INF in every lane if there is none.
//   2. The log's room is known before a launch that appends to it: a logged batch waits for the host after every round, the
//      host knows the next queue's fill, grows the log and hands the kernel the count by value.  528 bytes per entry (row, mask,
//      round, prev); entries are 32-bit indices, a batch that would pass 2^31 of them fails with PGQ_ERR_UNSUPPORTED, a log that
//      cannot be allocated with PGQ_ERR_OOM — before any list is written (the lists are gathered behind the last batch).
//   3. k_hop_lengths, a thread per row: dst's latest entry with the row's lane bit gives h (its round) — the last round in
//      which the lane's label changed there is the first that shows the final one; no such entry: NULL.
//   4. k_hop_walkback, a wavefront per row, shaped like k_cheapest_walkback: step i strides x_i's in-list (reverse CSR + the
//      in-edge weights), follows hop_last[u] and prev to u's entry of round <= i - 1 (indices fall along the chain: at most
//      K - i + 2 dependent loads), tests relax_sum(value, w) == target; a wave min-reduce picks the smallest u, a ballot over u's
//      out-list its first tight slot.  Every loop is bounded by h, a chain's or a list's length.  A step without a parent or a
//      slot, or a walk that does not end on src, raises the batch's error flag and the call fails with PGQ_ERR_HIP.
//   5. hop_last goes back to "none" through the batch's touched list; the lists are staged and laid out by PathBatches.
// Kernel-class time: the rounds and the log passes are K_RELAX, lengths / walk-back / gather K_RECON.
// Not built: _multi, a heavy-list split of the rounds (HopBatches' known limit), more than one worker.
//
// cheapest_walk (pgq_cheapest_walk, lo = min_hops >= 1; lo == 0 IS the call above): the cheapest walk of lo .. K edges as a list,
// on the same log.  E_t and L_t are HopBatches' labels with a lower bound (pgq_cheapest.hip); Λ_i = E_i for i <= lo, L_i for i > lo.
//   NULL         L_K[dst] == INF, or a NULL src or dst.  src == dst is NOT special: its cheapest closed walk of lo .. K edges.
//   h            the smallest t in [lo, K] with L_t[dst] == L_K[dst] as bit patterns;  d_out_len = h.
//   the walk     x_h = dst; for i = h .. 1, x_{i-1} = the SMALLEST u with Λ_{i-1}[u] < INF and a slot (u, x_i) with
//                relax_sum(Λ_{i-1}[u], w[s]) == Λ_i[x_i], e_i = edge_ids[the FIRST such slot of u's out-list into x_i].
// The log: k_hop_log TAKES in the rounds below lo (the logged row goes back to INF in the label array, like k_hop_snapshot's take),
// so for every round r <= lo the log holds one entry per vertex with a finite lane of E_r, and its row is E_r[v] exactly — the
// lanes not reached are INF, nothing is carried over.  Behind lo the entries are the call's above.  The look-up (hop_entry_at):
// Λ_j[v] is the row of v's entry of round EXACTLY j when j <= lo; of v's latest entry of round <= j when j > lo, and only if
// that round is >= lo; INF otherwise.  An entry of an earlier exact round is stale: that label was taken.  k_hop_lengths: dst's
// latest entry with the row's lane bit gives h; no such entry, or one of a round below lo: NULL.
// A tight parent exists at every step, and step 0 stands on src:
//   i - 1 >= lo  fact 1 above, read with L for D and started at L_lo = E_lo.  x_h = dst has an entry of round h with its lane's bit:
//                h > lo is a strict improvement in round h, h == lo is a finite lane of E_lo (every finite lane of an exact round is
//                dirty, HopBatches' invariant).  A tight parent u of a vertex that improved strictly in round i > lo has not shown
//                L_{i-1}[u] in a round j with lo <= j < i - 1 (round j + 1 would have offered it), so u improved in round i - 1
//                exactly when i - 1 > lo, and has a finite lane of E_lo — hence an entry of round lo — when i - 1 == lo.  One exists:
//                the round's minimum was offered by some slot.
//   i <= lo      Λ_i[x_i] = E_i[x_i] < INF is a minimum over the in-slots (u, x_i) with E_{i-1}[u] < INF, and a minimum over a finite,
//                non-empty set is attained: that u is tight and has an entry of round exactly i - 1.
//   step 0       Λ_0 = E_0 is finite at src alone, so x_0 = src.  Every step goes down one round: h steps, no loop on zero-weight
//                cycles.  The fold of the list's weights is L_K[dst] as in fact 2 (Λ_i[x_i] = Λ_{i-1}[x_{i-1}] + w(e_i), Λ_0[src] = 0).
// Rows the bound does not bind (the _within call's h >= lo) have the _within VALUE; with int64 weights the same list, with doubles
// an absorbed sum can make the lists differ (README).  A large K is not forwarded to anything: fact 4.
// Memory: the exact phase logs everything it reaches in EVERY round — lo x reached vertices x 528 bytes per lane batch on top of
// what the call above logs (which logs a vertex only in the rounds that improve it).
// Not built for cheapest_walk: _multi forms, a heavy-list split, a destination bound, the path modes, a two-ended search,
// forwarding upper - lower >= V - 1 to k_relax.

namespace pgq {

struct HopEntry {
	int32_t round; // the labels of the entry's row are D_round of its vertex
	int32_t prev;  // the vertex's entry before this one, -1: none
};

// In k_hop_snapshot's place (HopLog::append): entries [log_base, log_base + nq) of the log, one wavefront per queue entry.
// nq comes from the host, which has made room for exactly that many.
// take (an exact round of cheapest_walk, round < lo): the logged row goes back to INF in `dist`, as in k_hop_snapshot.
__global__ __launch_bounds__(256) void k_hop_log(const int32_t *__restrict__ qcur, u32 nq, u64 *__restrict__ dirty_cur,
                                                 int64_t *__restrict__ dist, int32_t round, u32 log_base,
                                                 int64_t *__restrict__ row, u64 *__restrict__ mask, HopEntry *__restrict__ ent,
                                                 int32_t *__restrict__ hop_last, int take, int64_t inf_bits) {
	const int lane = threadIdx.x & 63;
	const u32 wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
	const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
	for (u32 i = wave; i < nq; i += nwaves) {
		const int v = qcur[i];
		const u32 g = log_base + i;
		row[(size_t)g * LC + lane] = dist[(size_t)v * LC + lane];
		if (take) dist[(size_t)v * LC + lane] = inf_bits;
		if (lane == 0) {
			mask[g] = atomicExch(&dirty_cur[v], 0ull); // consumed: the word is clean for the round after next, and for the next batch
			ent[g] = HopEntry { round, hop_last[v] };
			hop_last[v] = (int32_t)g;
		}
	}
}

// the latest entry of vertex x in which lane l changed (-1: none): its round is the row's h, its row holds the row's cost
__device__ __forceinline__ int32_t hop_final_entry(int x, u32 l, const int32_t *__restrict__ hop_last, const u64 *__restrict__ mask,
                                                   const HopEntry *__restrict__ ent) {
	int32_t g = hop_last[x];
	while (g >= 0 && !((mask[g] >> l) & 1ull)) g = ent[g].prev; // (indices fall along the chain)
	return g;
}
// the entry of vertex u that holds D_j[u] (-1: none, every lane at INF).  With a lower bound lo (cheapest_walk; 0 otherwise) the
// labels are Λ_j: for j <= lo the entry of round EXACTLY j (an exact round carries nothing over: an earlier entry is stale), for
// j > lo the latest entry of round <= j, and only if that round is >= lo (what an exact round logged was taken afterwards).
__device__ __forceinline__ int32_t hop_entry_at(int u, int32_t j, int32_t lo, const int32_t *__restrict__ hop_last, const HopEntry *__restrict__ ent) {
	int32_t g = hop_last[u];
	while (g >= 0 && ent[g].round > j) g = ent[g].prev;
	if (g >= 0 && (j <= lo ? ent[g].round != j : ent[g].round < lo)) g = -1;
	return g;
}

// out_len[row] = h (-1: no walk of min_hops .. K edges), cnt[i - lo] = elements of the row's list.  A final entry of a round
// below min_hops is an exact round's: that label was taken, the row is NULL.
__global__ void k_hop_lengths(int64_t lo, int64_t hi, const u32 *__restrict__ skey, const u32 *__restrict__ sidx,
                              const int32_t *__restrict__ sdst, u32 base_lane, const int32_t *__restrict__ hop_last,
                              const u64 *__restrict__ mask, const HopEntry *__restrict__ ent, int32_t min_hops, int64_t *__restrict__ out_len,
                              int64_t *__restrict__ cnt) {
	const int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= hi) return;
	const int32_t g = hop_final_entry(sdst[i], skey[i] - base_lane, hop_last, mask, ent);
	const int64_t h = g < 0 || ent[g].round < min_hops ? -1 : ent[g].round;
	out_len[sidx[i]] = h;
	cnt[i - lo] = h < 0 ? 0 : 2 * h + 1;
}

// One wavefront per row: the list, written back to front into stage[stage_base + loc[i - lo] ..]; soff[i] = where it starts.
template <typename T>
__global__ __launch_bounds__(64) void k_hop_walkback(int64_t lo, int64_t hi, const u32 *__restrict__ skey, const int32_t *__restrict__ sdst,
                                                    u32 base_lane, const int32_t *__restrict__ usrc, const int64_t *__restrict__ off,
                                                    const int32_t *__restrict__ adj, const T *__restrict__ w, const int64_t *__restrict__ edge_ids,
                                                    const int64_t *__restrict__ roff, const int32_t *__restrict__ radj, const T *__restrict__ rw,
                                                    const int32_t *__restrict__ hop_last, const u64 *__restrict__ mask,
                                                    const HopEntry *__restrict__ ent, const int64_t *__restrict__ row, int32_t min_hops,
                                                    const int64_t *__restrict__ loc, int64_t stage_base, int64_t *__restrict__ stage,
                                                    int64_t *__restrict__ soff, TightCounters *__restrict__ tc) {
	const int lane = threadIdx.x;
	for (int64_t i = lo + blockIdx.x; i < hi; i += gridDim.x) {
		const u32 l = skey[i] - base_lane;
		int x = sdst[i];
		if (lane == 0) soff[i] = stage_base + loc[i - lo];
		const int32_t g = hop_final_entry(x, l, hop_last, mask, ent);
		if (g < 0 || ent[g].round < min_hops) continue; // no walk: no list (k_hop_lengths)
		const int h = ent[g].round;
		int64_t dx = row[(size_t)g * LC + l];
		int64_t *out = stage + stage_base + loc[i - lo]; // 2 h + 1 elements (k_hop_lengths)
		if (lane == 0) out[2 * h] = x;
		bool lost = false;
		for (int t = h; t >= 1; t--) {
			// the smallest u with a tight in-slot into x against D_{t-1}[u]
			int best = 0x7FFFFFFF;
			const int64_t rb = roff[x], re = roff[x + 1];
			for (int64_t j = rb + lane; j < re; j += 64) {
				const int u = radj[j];
				const int32_t eu = hop_entry_at(u, t - 1, min_hops, hop_last, ent);
				if (eu < 0 || u >= best) continue;
				const int64_t du = row[(size_t)eu * LC + l];
				if (du < Inf<T>::bits && relax_sum<T>(du, rw[j]) == dx) best = u;
			}
			for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
			if (best == 0x7FFFFFFF) {
				if (lane == 0) atomicOr(&tc->error, 2u);
				lost = true;
				break;
			}
			// its first tight slot into x
			const int64_t du = row[(size_t)hop_entry_at(best, t - 1, min_hops, hop_last, ent) * LC + l];
			int64_t slot = -1;
			const int64_t fb = off[best], fe = off[best + 1];
			for (int64_t e0 = fb; e0 < fe && slot < 0; e0 += 64) {
				const int64_t e = e0 + lane;
				const u64 hit = __ballot(e < fe && adj[e] == x && relax_sum<T>(du, w[e]) == dx);
				if (hit) slot = e0 + __ffsll((long long)hit) - 1;
			}
			if (slot < 0) {
				if (lane == 0) atomicOr(&tc->error, 4u);
				lost = true;
				break;
			}
			if (lane == 0) {
				out[2 * t - 1] = edge_ids ? edge_ids[slot] : slot;
				out[2 * t - 2] = best;
			}
			x = best;
			dx = du;
		}
		if (!lost && lane == 0 && x != usrc[base_lane + l]) atomicOr(&tc->error, 8u); // (fact 1 says it cannot)
	}
}

// the batch is over: hop_last back to "none" wherever it was set (every logged vertex is on the touched list)
__global__ void k_hop_reset_last(const int32_t *__restrict__ touched, const u32 *__restrict__ tcount, int32_t *__restrict__ hop_last) {
	const u32 nt = *tcount;
	u32 t = blockIdx.x * blockDim.x + threadIdx.x;
	for (; t < nt; t += gridDim.x * blockDim.x) hop_last[touched[t]] = -1;
}

// The round log of one worker's lane batches, and what a finished batch does with it: lengths, walk-back, staging.
template <typename T> class HopPathLog {
public:
	HopPathLog(pgq_csr *c, Workspace *ws, PathBatches<T> &paths, int64_t *d_out_len, int64_t min_hops = 0)
	    : c(c), ws(ws), paths(paths), d_out_len(d_out_len), min_hops((int32_t)min_hops) {}

	int prepare() {
		const bool fresh = ws->hop_last.cap < Vn * 4 || ws->hop_last_V != c->V;
		ws->hop_last_V = -1; // stays invalid if the call bails out half-way
		PGQ_TRY(ws->hop_last.reserve(Vn * 4));
		if (fresh) fill32(ws->hop_last.as<int32_t>(), (int64_t)Vn, -1, st);
		return PGQ_OK;
	}
	void settle() { ws->hop_last_V = c->V; } // behind the last batch's reset, waited for
	size_t peak_bytes() const { return peak * kEntryBytes; }

	HopLog hook() {
		return HopLog { [this](int par, u32 nq, int64_t round, bool take, const int64_t **snap, const u64 **snapmask) { return append(par, nq, round, take, snap, snapmask); },
		                [this](int64_t lo, int64_t hi, int64_t base) { return batch(lo, hi, base); } };
	}

private:
	static constexpr size_t kEntryBytes = LC * 8 + 8 + sizeof(HopEntry);
	pgq_csr *const c;
	Workspace *const ws;
	PathBatches<T> &paths;
	int64_t *const d_out_len;
	const int32_t min_hops; // cheapest_walk's lower bound (<= PGQ_WALK_MAX_HOPS), 0: cheapest_path_within
	const hipStream_t st = ws->stream;
	const size_t Vn = (size_t)std::max<int64_t>(c->V, 1);
	pgq_stats_t &S = tstats().s;
	size_t count = 0, peak = 0; // entries of the batch's log so far; the most a batch of this call had
	std::string name() const { return min_hops > 0 ? "cheapest_walk" : "cheapest_path_within"; } // the call an error message names

	// room for `need` entries, the first `count` kept
	int reserve(size_t need) {
		if (need >= ((size_t)1 << 31)) return fail(PGQ_ERR_UNSUPPORTED, name() + ": the round log of one lane batch would pass 2^31 entries");
		const size_t cap = ws->hop_mask.cap / 8;
		if (need <= cap && need * LC * 8 <= ws->hop_row.cap && need * sizeof(HopEntry) <= ws->hop_ent.cap) return PGQ_OK;
		const size_t grown = std::max<size_t>(std::max(need, 2 * cap), 1024);
		PGQ_TRY(grow_keeping(ws->hop_row, grown * LC * 8, count * LC * 8, st));
		PGQ_TRY(grow_keeping(ws->hop_mask, grown * 8, count * 8, st));
		PGQ_TRY(grow_keeping(ws->hop_ent, grown * sizeof(HopEntry), count * sizeof(HopEntry), st));
		return PGQ_OK;
	}

	int append(int par, u32 nq, int64_t round, bool take, const int64_t **snap, const u64 **snapmask) {
		if (round >= (int64_t)0x7FFFFFFF) return fail(PGQ_ERR_UNSUPPORTED, name() + ": more than 2^31-1 rounds");
		PGQ_TRY(reserve(count + nq));
		RelaxSide &sd = ws->relax[0];
		KernelTimer kt(st, K_RELAX);
		hipLaunchKernelGGL(k_hop_log, dim3(std::min((unsigned)device_cus() * 8, std::max(1u, (nq + 3) / 4))), dim3(256), 0, st, sd.q[par].as<int32_t>(), nq,
		                   sd.dirty[par].as<u64>(), sd.dist.as<int64_t>(), (int32_t)round, (u32)count, ws->hop_row.as<int64_t>(), ws->hop_mask.as<u64>(),
		                   ws->hop_ent.as<HopEntry>(), ws->hop_last.as<int32_t>(), take ? 1 : 0, Inf<T>::bits);
		kt.stop();
		*snap = ws->hop_row.as<int64_t>() + count * LC;
		*snapmask = ws->hop_mask.as<u64>() + count;
		count += nq;
		peak = std::max(peak, count);
		// a row read and written, the dirty word exchanged, mask, entry and hop_last; a take writes the row once more
		S.algo_bytes[K_RELAX] += (double)nq * (2.0 * 8 * LC + 16.0 + 2.0 * sizeof(HopEntry) + (take ? 8.0 * LC : 0.0));
		return PGQ_OK;
	}

	// rows [lo, hi) of the sorted arrays, lane 0 = distinct source `base`; the batch's log is complete
	int batch(int64_t lo, int64_t hi, int64_t base) {
		const int64_t m = hi - lo;
		TightCounters *tc = paths.counters();
		const int32_t *last = ws->hop_last.as<int32_t>();
		const u64 *mask = ws->hop_mask.as<u64>();
		const HopEntry *ent = ws->hop_ent.as<HopEntry>();
		int64_t *loc = nullptr, total = 0, at = 0;
		PGQ_HIP_TRY(hipMemsetAsync(tc, 0, sizeof(TightCounters), st));
		PGQ_TRY(paths.stage.place(m, [&](int64_t *const *cnt) {
			hipLaunchKernelGGL(k_hop_lengths, dim3(blocks_for(m)), dim3(256), 0, st, lo, hi, ws->skey.as<u32>(), ws->sidx.as<u32>(), ws->sdst.as<int32_t>(),
			                   (u32)base, last, mask, ent, min_hops, d_out_len, cnt[0]);
		}, 1, &loc, &total));
		PGQ_TRY(paths.stage.wait());
		PGQ_TRY(paths.stage.stage_reserve(total, &at));
		{
			KernelTimer kt(st, K_RECON);
			hipLaunchKernelGGL(k_hop_walkback<T>, dim3((unsigned)std::min<int64_t>(m, 1 << 20)), dim3(64), 0, st, lo, hi, ws->skey.as<u32>(),
			                   ws->sdst.as<int32_t>(), (u32)base, ws->usrc.as<int32_t>(), c->off, c->adj, (const T *)c->w, c->edge_ids, c->roff, c->radj,
			                   (const T *)c->rw, last, mask, ent, ws->hop_row.as<int64_t>(), min_hops, loc, at, ws->tight_stage.as<int64_t>(), ws->soff.as<int64_t>(), tc);
			kt.stop();
		}
		hipLaunchKernelGGL(k_hop_reset_last, dim3((unsigned)device_cus() * 4), dim3(256), 0, st, ws->relax[0].touched.as<int32_t>(),
		                   &reinterpret_cast<RelaxCounters *>(ws->counters.p)->tcount, ws->hop_last.as<int32_t>());
		count = 0;
		TightCounters h {};
		PGQ_TRY(paths.stage.read_back(&h, tc, sizeof(h)));
		if (h.error) return fail(PGQ_ERR_HIP, name() + ": internal error: the walk back lost its way (no tight parent, no tight slot, or not at the source)");
		return PGQ_OK;
	}
};

// cheapest_path_device's bounded sibling.  Every K takes the hop rounds, K >= V - 1 included (fact 4): they end with the queue.
// min_hops >= 1: cheapest_walk — the first min_hops rounds exact, src == dst rows on a lane (path_call's closed_rows).
template <typename T>
static int cheapest_path_within_device(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t max_hops, const PathOut &out,
                                       int64_t min_hops = 0) {
	return path_call<T>(c, ws, n, d_src, d_dst, out, false, min_hops > 0, [&](PathBatches<T> &paths, int nb, u32 U) -> int {
		HopPathLog<T> log(c, ws, paths, out.d_len, min_hops);
		PGQ_TRY(log.prepare());
		PGQ_TRY(hop_rounds_logged<T>(c, ws, nb, U, min_hops, max_hops, log.hook()));
		log.settle();
		if (getenv("PGQ_RELAX_TRACE")) fprintf(stderr, "hop log: peak %zu bytes in a batch\n", log.peak_bytes());
		return PGQ_OK;
	});
}

// max_hops: null = unbounded
template <typename T>
static int cheapest_path_rows(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst, const PathOut &out, const int64_t *max_hops,
                             int64_t min_hops = 0) {
	return max_hops ? cheapest_path_within_device<T>(c, ws, n, d_src, d_dst, *max_hops, out, min_hops) : cheapest_path_device<T>(c, ws, n, d_src, d_dst, out);
}

} // namespace pgq
