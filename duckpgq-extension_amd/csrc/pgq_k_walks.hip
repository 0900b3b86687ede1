// pgq_k_walks.hip — walk_count and k_shortest_walks on MI355X: how many walks of lower..upper edges a row has, and the first k of
// them as lists, shortest first, for SQL/PGQ's quantified pattern -[e]->{lower,upper} in WALK mode and its SHORTEST k.  The reference
// has no counterpart: its binder rejects TopK (match.cpp:82-98) and filters a quantified pattern with iterativelength BETWEEN lower
// AND upper (match.cpp:658-671), which drops a pair at distance 1 that also has a walk of 2 edges from {2,3} and never finds a cycle
// (src == dst is 0 hops there).  Every list follows shortestpath's layout (shortest_path.cpp:43-207).
//
// The root file of pgq_k_walks.o, compiled on its own, with pgq_walk_rule.h, pgq_path_modes.h and, at its end, pgq_walk_length.hip.
// The saturating add, the pull's inner loop, one step of the unranking, the tails kernel, the list staging and the call skeleton
// ListCall with its layout are all_shortestpaths' too: pgq_path_lists.h, described there once.  Of pgq_relax.h it takes LC (through
// pgq_path_lists.h) and nothing else.  Weights are never read: the calls work on any CSR.
//
// The contract, for a row (src, dst), lo = min_hops, K = max_hops, over the forward CSR's slots (parallel edges are separate slots):
//   W_0[v] = 1 if v == src else 0
//   W_t[x] = min(INT64_MAX, sum of W_{t-1}[u] over ALL in-slots (u, x))      t = 1 .. K
//   count  = min(INT64_MAX, sum of W_t[dst] for t = lo .. K)
// The sums saturate at 2^63 - 1 and never wrap.  src == dst is not special: it counts the empty walk when lo == 0 and every closed
// walk of lo..K edges.  NULL src or dst: NULL (bulk form: -1).
//   the walks    the first min(count, k) walks, each [x_0, e_1, x_1, ..., e_t, x_t] (the empty walk is [src]).  Shorter walks come
//                first; walks of equal length t are ordered by in-list positions read from the destination end — all_shortestpaths'
//                order with "W_{i-1}[u] > 0" in place of "L[u] = i - 1" and W_{i-1}[u] in place of sigma[u].  Walk number r:
//                1. the smallest t >= lo with r < W_t[dst], after subtracting W_t[dst] of the shorter lengths from r;
//                2. x_t = dst; for i = t .. 1 scan x_i's in-list in stored order; for each in-slot (u, x_i): r < W_{i-1}[u] takes it,
//                   otherwise r -= W_{i-1}[u];
//                3. the taken in-slot is the m-th from u into x_i, its edge the m-th slot of u's out-list whose target is x_i.
//                A saturated W stays valid for unranking: every emitted rank is below 2^31.
//                For src != dst, d = dist(src, dst) and lo <= d <= K the walks of length d come first and are all_shortestpaths'
//                lists in its order: walk 0 is shortestpath's list.
//   no walk      count 0 (or a NULL endpoint): the row's list is NULL, no inner list, no payload.
//   the list form's count   the rounds of a lane batch stop once none of its rows is short of k walks, and a row stops adding once it
//                has k: d_out_count is the number of walks of lo..T edges, T the length of the row's last emitted walk.  That is
//                `count` whenever count <= k; otherwise it is at least k and at most count (walk_count gives count itself).
//
// Per lane batch (at most 64 distinct sources, lane l = source l); per round t one table W_t of V x 64 int64 and one mask word per
// vertex, M_t[v] = the lanes with W_t[v] > 0.  W_t[v][l] is only read where M_t[v] has bit l: the tables need no reset, the masks do.
// walk_count keeps two rounds (ping-pong, 1040 B x V); k_shortest_walks keeps rounds 0..R (R <= K the last round run) for the
// unranking: 520 B x V per round and batch, block-cache memory of the call, PGQ_ERR_OOM with nothing written if it cannot be had.
//   0. k_walk_init: W_0[src][l] = 1, M_0, the first queue.
//   1. k_walk_activate, round t: a wavefront per vertex v of round t-1's queue walks v's out-list 64 targets per load, ONE lane per
//      edge does atomicOr(&M_t[n], M_{t-1}[v]) (skipped where a plain read shows nothing to add); who sees the old value 0 queues n.
//   2. k_walk_pull, behind it: a wavefront per queued n reads n's in-list 64 entries and 64 mask words at a time, ballots the
//      neighbours with a non-empty M_{t-1}; lane l in M_t[n] saturating-adds W_{t-1}[u][l] where M_{t-1}[u] has bit l.  One plain
//      store per (vertex, lane), no atomics on W: the same on every run.
//   3. k_walk_after: for t >= lo a thread per row feeds the row W_t[dst][lane] (0 where the mask bit is clear) by the rule below,
//      notes the first length, counts the rows still open; walk_count: M_{t-1} back to zero over round t-1's queue.
//   Rounds stop after round K, with an empty queue, and (lists) when no row of the batch is open: k = 1 on a pair d apart
//   costs d rounds.  walk_count has no such stop.  The host waits once per round for the counters.
//   4. k_walk_plan, a thread per row: walks and elements per row from W_t[dst], t = lo..R, by the same rule; two exclusive scans
//      place them.
//   5. k_walk_unrank, a wavefront per emitted walk: its t by the same small loop, then unrank_step (pgq_path_lists.h) per step, with
//      the weight W_{i-1}[u][l].  A step that finds no parent or no slot, or a walk that does not end on the lane's source, raises
//      the error flag: PGQ_ERR_HIP.
//   6. Behind the last batch: trivial rows (src == dst without a lane: [[src]] when lo == 0, nothing otherwise), NULL rows, scans in
//      ROW order, k_walk_gather (ListCall::layout).  Results go to the caller only then: a call that fails has written nothing.
// The call owns its tables, masks and queues (block cache); it does not touch ws->tight_h / tight_mask / tight_q / tight_V, so
// PathBatches and AspCall find them as they left them.  Lists are staged in ws->tight_stage, rows in ws->asp_rows.
// Kernel-class time: the rounds are K_PUSH, plan / unranking / gather K_RECON.
// THE RULE.  Every entry point turns its arguments into one WalkQuery (walk_query, at the entry points), and when a row has enough
// is decided in one place, pgq_walk_rule.h: a row is open while it has been fed fewer than G non-empty lengths and their saturating
// sum is <= B.  SHORTEST k is G unbounded, B = k - 1; walk_count B = INT64_MAX - 1; SHORTEST k GROUP (pgq_k_shortest_groups: every
// walk of a row's g smallest non-empty lengths, capped at P = max_paths) G = g, B = P.  k_walk_after feeds a row one round at a
// time, k_walk_plan all rounds at once and takes min(W_t[dst], what is left of the limit) from each fed length; the groups' count
// is min(sum, P + 1), their ngroups the lengths emitted from, in a seventh row array (ListCall::r_ng) reserved for that call.  A
// group list is a prefix of S, so a rank means the same walk: k_walk_unrank, the staging and k_walk_gather serve every form.
// The path modes TRAIL / ACYCLIC / SIMPLE (pgq_k_shortest_walks_mode, pgq_walk_count_mode, the groups under a mode) run the rounds
// with every table kept and the rows closed by distance, then search each row over the tables, feeding it by the same rule one
// admitted walk at a time: pgq_path_modes.h, included below, has the contract.
// Not built: _multi forms, splitting long in-lists over several wavefronts (a list is walked by the one wavefront that meets it), any
// change to how the binder's iterativelength filter is emitted; under a mode: an unbounded upper, an unlimited count, a smarter
// prune than W, several wavefronts per row; for the groups: a count-only form.

#include "pgq_path_lists.h"
#include "pgq_walk_rule.h"

namespace pgq {

struct WalkCounters {
	u32 nq[2];   // queued vertices by round parity
	u32 pending; // rows of the batch still open (pgq_walk_rule.h)
	u32 error;   // unranking: no length / parent (2), no slot (4), not at the source (8)
	u64 edges;   // adjacency entries the rounds walked
	u64 steps;   // path modes: the steps of the batch's searches, both passes ...
	u64 row_max; // ... and the most a row took in one pass
};
struct WalkRound {
	const int64_t *W;
	const u64 *M;
};

__device__ __forceinline__ int64_t walk_w(const WalkRound &rd, int x, u32 l) { return (rd.M[x] >> l) & 1ull ? rd.W[(size_t)x * LC + l] : 0; }

__global__ void k_walk_init(const int32_t *__restrict__ usrc, int64_t U, int64_t base, int64_t *__restrict__ W0, u64 *__restrict__ M0,
                            int32_t *__restrict__ q, WalkCounters *__restrict__ tc) {
	const int l = threadIdx.x;
	const int64_t g = base + l;
	if (l == 0) {
		tc->nq[0] = (u32)min((int64_t)LC, U - base);
		tc->nq[1] = 0;
		tc->pending = 0;
		tc->error = 0;
		tc->edges = 0;
		tc->steps = 0;
		tc->row_max = 0;
	}
	if (l >= LC || g >= U) return;
	const int v = usrc[g];
	W0[(size_t)v * LC + l] = 1;
	M0[v] = 1ull << l; // (distinct sources: distinct vertices)
	q[l] = v;
}
__global__ void k_walk_rows(int64_t lo, int64_t hi, const u32 *__restrict__ sidx, int64_t *__restrict__ r_len, int64_t *__restrict__ r_count,
                            int64_t *__restrict__ r_ng) {
	const int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= hi) return;
	r_len[sidx[i]] = -1;
	r_count[sidx[i]] = 0;
	if (r_ng) r_ng[sidx[i]] = 0;
}
__global__ void k_walk_round_reset(WalkCounters *__restrict__ tc, int next_par) {
	tc->nq[next_par] = 0;
	tc->pending = 0;
}

// Round t, activation: a wavefront per vertex v of the last round's queue, a LANE per out-slot.
__global__ __launch_bounds__(256) void k_walk_activate(const int64_t *__restrict__ off, const int32_t *__restrict__ adj, const u64 *__restrict__ m_prev,
                                                       u64 *__restrict__ m_cur, const int32_t *__restrict__ qprev, int32_t *__restrict__ qcur,
                                                       WalkCounters *__restrict__ tc, int par) {
	const int lane = threadIdx.x & 63;
	const u32 wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
	const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
	const u32 nq = tc->nq[par];
	for (u32 i = wave; i < nq; i += nwaves) {
		const int v = qprev[i];
		const u64 mv = m_prev[v];
		const int64_t b = off[v], e = off[v + 1];
		for (int64_t k0 = b; k0 < e; k0 += 64) {
			int n = -1;
			bool fresh = false;
			if (k0 + lane < e) {
				n = adj[k0 + lane];
				// (a stale read only costs the atomic it would have spared: bits are never taken away during the launch)
				if ((__atomic_load_n(&m_cur[n], __ATOMIC_RELAXED) & mv) != mv) fresh = atomicOr(&m_cur[n], mv) == 0ull;
			}
			const u64 fm = __ballot(fresh); // each vertex sees the old value 0 once per round: <= V queue entries
			if (fm) {
				u32 at = 0;
				if (lane == 0) at = atomicAdd(&tc->nq[par ^ 1], (u32)__popcll(fm));
				at = __shfl(at, 0);
				if (fresh) qcur[at + (u32)__popcll(fm & ((1ull << lane) - 1ull))] = n;
			}
		}
		if (lane == 0 && e > b) atomicAdd(&tc->edges, (u64)(e - b));
	}
}

// Round t, the sums: a wavefront per vertex n the round queued (once), lane l = source l.
__global__ __launch_bounds__(256) void k_walk_pull(const int64_t *__restrict__ roff, const int32_t *__restrict__ radj, const int64_t *__restrict__ w_prev,
                                                   const u64 *__restrict__ m_prev, int64_t *__restrict__ w_cur, const u64 *__restrict__ m_cur,
                                                   const int32_t *__restrict__ qcur, WalkCounters *__restrict__ tc, int par_cur) {
	const int lane = threadIdx.x & 63;
	const u32 wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
	const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
	const u32 nq = tc->nq[par_cur];
	for (u32 i = wave; i < nq; i += nwaves) {
		const int n = qcur[i];
		const bool want = (m_cur[n] >> lane) & 1ull;
		const int64_t acc = pull_masked_sum(n, lane, want, roff, radj, m_prev, w_prev); // (only the active in-neighbours are visited)
		const int64_t rb = roff[n], re = roff[n + 1];
		if (want) w_cur[(size_t)n * LC + lane] = acc; // (> 0: some in-neighbour gave the lane its mask bit)
		if (lane == 0 && re > rb) atomicAdd(&tc->edges, (u64)(re - rb));
	}
}

// Round t is over.  A thread per row of the batch feeds the row W_t[dst] by the rule of pgq_walk_rule.h — state in r_count and,
// for the groups, r_ng; r_len notes the first length fed — and counts the rows still open.  m_zero != null (walk_count's
// ping-pong): round t-1's mask words back to zero over its queue.
// by_distance (the path modes): r_len notes the distance d, the first t >= 0 with W_t[dst] > 0, whether or not d >= min_hops;
// the row closes there or never (WalkRow::close_at_distance).  k_walk_plan / the search overwrite the arrays they own.
__global__ void k_walk_after(int t, WalkQuery q, int64_t lo, int64_t hi, const u32 *__restrict__ skey, const u32 *__restrict__ sidx,
                             const int32_t *__restrict__ sdst, u32 base_lane, WalkRound cur, int64_t *__restrict__ r_len, int64_t *__restrict__ r_count,
                             int64_t *__restrict__ r_ng, const int32_t *__restrict__ qprev, u64 *__restrict__ m_zero, int par_prev,
                             WalkCounters *__restrict__ tc) {
	const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (m_zero && tid < (int64_t)tc->nq[par_prev]) m_zero[qprev[tid]] = 0;
	const int64_t i = lo + tid;
	bool open = false;
	if (i < hi) {
		const WalkRule rule = q.rule();
		const u32 row = sidx[i];
		WalkRow s { r_count[row], !q.by_distance() && r_ng ? r_ng[row] : 0 };
		// not read: by distance once the distance is known; otherwise below min_hops and for a closed row
		const bool skip = q.by_distance() ? r_len[row] >= 0 : t < q.min_hops || !s.open(rule);
		const int64_t w = skip ? 0 : walk_w(cur, sdst[i], skey[i] - base_lane);
		if (w > 0) {
			if (r_len[row] < 0) r_len[row] = t;
			if (!q.by_distance()) s.add(w);
			else if (t >= q.min_hops) s.close_at_distance(w, rule);
			r_count[row] = s.count; // (by distance: B + 1 <= 2^31 + 1 or the count's limit)
			if (!q.by_distance() && r_ng) r_ng[row] = s.groups;
		}
		open = s.open(rule);
	}
	const u64 om = __ballot(open);
	if (om && (threadIdx.x & 63) == 0) atomicAdd(&tc->pending, (u32)__popcll(om));
}

// per row of the batch: the walks it emits and their elements; staged per row as [hops of each walk][the walks' elements].  The
// row is fed the lengths lo .. rounds by the rule and takes from each by WalkPlan.  The groups' count and groups are the plan's:
// min(sum, P + 1) and the lengths emitted from.  SHORTEST k's r_count stays what the rounds left, the walks of lo..T edges.
__global__ void k_walk_plan(int64_t lo, int64_t hi, const u32 *__restrict__ skey, const u32 *__restrict__ sidx, const int32_t *__restrict__ sdst,
                            u32 base_lane, const WalkRound *__restrict__ tabs, WalkQuery q, int rounds, int64_t *__restrict__ r_np,
                            int64_t *__restrict__ r_el, int64_t *__restrict__ r_count, int64_t *__restrict__ r_ng, int64_t *__restrict__ cntp,
                            int64_t *__restrict__ cnte) {
	const int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= hi) return;
	const int x = sdst[i];
	const u32 l = skey[i] - base_lane;
	const u32 row = sidx[i];
	const WalkRule rule = q.rule();
	WalkRow s;
	WalkPlan plan;
	for (int64_t t = q.min_hops; t <= rounds && s.open(rule); t++) { // (SHORTEST k: open is "fewer than k taken")
		const int64_t w = walk_w(tabs[t], x, l);
		if (w <= 0) continue;
		plan.take(s, q.limit, t, w);
		s.add(w);
	}
	if (q.groups > 0) {
		r_count[row] = min(s.count, rule.bound + 1); // (P <= 2^31)
		r_ng[row] = plan.ngroups;
	}
	const int64_t np = WalkPlan::np(s, q.limit);
	r_np[row] = np;
	r_el[row] = plan.el;
	cntp[i - lo] = np;
	cnte[i - lo] = np > 0 ? np + plan.el : 0;
}

// One wavefront per emitted walk (row, rank): its length, then the list, written back to front into the row's staged block.
__global__ __launch_bounds__(64) void k_walk_unrank(int64_t lo, int64_t m, int64_t nwalks, const u32 *__restrict__ skey, const int32_t *__restrict__ sdst,
                                                   u32 base_lane, const int32_t *__restrict__ usrc, const int64_t *__restrict__ off,
                                                   const int32_t *__restrict__ adj, const int64_t *__restrict__ edge_ids,
                                                   const int64_t *__restrict__ roff, const int32_t *__restrict__ radj,
                                                   const WalkRound *__restrict__ tabs, WalkQuery q, int rounds,
                                                   const int64_t *__restrict__ ploc, const int64_t *__restrict__ eloc, int64_t stage_base,
                                                   int64_t *__restrict__ stage, int64_t *__restrict__ soff, WalkCounters *__restrict__ tc) {
	const int lane = threadIdx.x;
	for (int64_t p = blockIdx.x; p < nwalks; p += gridDim.x) {
		const int64_t a = rank_row(ploc, m, p);
		const int64_t i = lo + a;
		const int64_t rank = p - ploc[a], np = ploc[a + 1] - ploc[a];
		int64_t r = rank;
		const u32 l = skey[i] - base_lane;
		int x = sdst[i];
		// the walk's length: the shorter lengths' walks come first
		int64_t eoff = 0;
		int t = -1;
		for (int64_t tt = q.min_hops; tt <= rounds; tt++) {
			const int64_t w = walk_w(tabs[tt], x, l);
			if (r < w) {
				t = (int)tt;
				break;
			}
			r -= w; // (w <= r < 2^31)
			eoff += w * (2 * tt + 1);
		}
		if (t < 0) { // (k_walk_plan gave the row no such walk)
			if (lane == 0) atomicOr(&tc->error, 2u);
			continue;
		}
		const int64_t rowbase = stage_base + eloc[a];
		int64_t *out = stage + rowbase + np + eoff + r * (2 * (int64_t)t + 1);
		if (lane == 0) {
			if (rank == 0) soff[i] = rowbase;
			stage[rowbase + rank] = t;
			out[2 * t] = x;
		}
		bool lost = false;
		for (int s = t; s >= 1 && !lost; s--) {
			const WalkRound pr = tabs[s - 1];
			const UnrankStep step = unrank_step(x, r, lane, roff, radj, off, adj, [&](int cand) -> int64_t { return walk_w(pr, cand, l); });
			if (step.error) {
				if (lane == 0) atomicOr(&tc->error, step.error);
				lost = true;
				break;
			}
			if (lane == 0) {
				out[2 * s - 1] = edge_ids ? edge_ids[step.slot] : step.slot;
				out[2 * s - 2] = step.u;
			}
			x = step.u;
		}
		if (!lost && lane == 0 && x != usrc[base_lane + l]) atomicOr(&tc->error, 8u);
	}
}

// Row order: a wavefront per sorted position below lo_null copies the row's staged walks to its place in the child payload and
// writes its inner entries (offsets from a running prefix sum over the walks' lengths); trivial rows write their [src].
__global__ __launch_bounds__(64) void k_walk_gather(int64_t lo_trivial, int64_t lo_null, const u32 *__restrict__ sidx, const int32_t *__restrict__ sdst,
                                                   const int64_t *__restrict__ r_np, const int64_t *__restrict__ r_el, const int64_t *__restrict__ r_first,
                                                   const int64_t *__restrict__ r_eoff, const int64_t *__restrict__ soff, const int64_t *__restrict__ stage,
                                                   int64_t *__restrict__ path_off, int64_t *__restrict__ path_hops, int64_t *__restrict__ path_len,
                                                   int64_t *__restrict__ child) {
	const int lane = threadIdx.x;
	for (int64_t i = blockIdx.x; i < lo_null; i += gridDim.x) {
		const u32 row = sidx[i];
		const int64_t np = r_np[row];
		if (np <= 0) continue;
		const int64_t f = r_first[row], eo = r_eoff[row];
		if (i >= lo_trivial) {
			if (lane == 0) {
				child[eo] = sdst[i];
				path_off[f] = eo;
				if (path_hops) path_hops[f] = 0;
				if (path_len) path_len[f] = 1;
			}
			continue;
		}
		const int64_t *hp = stage + soff[i], *in = hp + np;
		const int64_t el = r_el[row];
		for (int64_t k = lane; k < el; k += 64) child[eo + k] = in[k];
		int64_t run = 0;
		for (int64_t k0 = 0; k0 < np; k0 += 64) {
			const int64_t k = k0 + lane;
			const int64_t h = k < np ? hp[k] : 0, w = k < np ? 2 * h + 1 : 0;
			int64_t inc = w;
			for (int o = 1; o < 64; o <<= 1) {
				const int64_t y = __shfl_up(inc, o);
				if (lane >= o) inc += y;
			}
			if (k < np) {
				path_off[f + k] = eo + run + inc - w;
				if (path_hops) path_hops[f + k] = h;
				if (path_len) path_len[f + k] = w;
			}
			run += __shfl(inc, 63);
		}
	}
}

} // namespace pgq

#include "pgq_path_modes.h" // k_mode_search: the depth-first search of TRAIL / ACYCLIC / SIMPLE over the rounds' tables

namespace pgq {

// the steps of this thread's last path-mode call (pgq_debug_mode_steps)
struct ModeSteps {
	int64_t total = 0, row_max = 0;
};
static ModeSteps &mode_steps() {
	static thread_local ModeSteps s;
	return s;
}

// The walk rounds of the lane batches on ListCall's skeleton (pgq_path_lists.h): its run, emit and layout.
class WalkCall : ListCall {
public:
	// q.mode != 0: every round's table is kept, the rounds stop by distance and the rows are searched (pgq_path_modes.h).
	// q.groups > 0: k_shortest_groups — out.d_ng is set.  The call's limit is q.limit, not out.limit.
	WalkCall(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst, const WalkQuery &q, ListOut &out)
	    : ListCall(c, ws, n, d_src, d_dst, out, q.groups ? "k_shortest_groups" : q.mode ? "k_shortest_walks_mode" : "k_shortest_walks", "walks"), query(q),
	      keep_rounds(out.lists || q.mode != 0), step_cap(std::max(options().mode_step_cap, 0)), temps(ws->stream) {}

	int run() {
		return ListCall::run(
		    true, [&] { return prepare(); }, [&](int64_t lo, int64_t hi, int64_t base, u32 U) { return batch(lo, hi, base, U); },
		    [&](int nb) {
			    return layout(nb, query.min_hops, [&](int64_t lo_t, int64_t lo_n, int64_t *path_off, int64_t *path_len, int64_t *child) {
				    hipLaunchKernelGGL(k_walk_gather, dim3((unsigned)std::min<int64_t>(lo_n, 1 << 20)), dim3(64), 0, st, lo_t, lo_n, ws->sidx.as<u32>(),
				                       ws->sdst.as<int32_t>(), r_np, r_el, r_first, r_eoff, ws->soff.as<int64_t>(), ws->tight_stage.as<int64_t>(), path_off,
				                       out.d_path_hops, path_len, child);
			    }, 24.0);
		    });
	}

private:
	const WalkQuery query;
	const bool keep_rounds; // a table per round (the unranking, the search) instead of walk_count's two
	const int64_t step_cap; // path modes: steps a row's search may take per pass
	uint64_t steps_seen = 0; // ... the batch's steps already booked
	DevTemps temps; // the rounds' tables, masks and queues: block-cache memory for the call
	WalkCounters *tc = nullptr;
	std::vector<int64_t *> W; // lists: one per round; counts: two
	std::vector<u64 *> M;
	std::vector<WalkRound> h_tabs;
	WalkRound *d_tabs = nullptr;
	int32_t *q[2] = { nullptr, nullptr };

	size_t slot_of(int64_t t) const { return keep_rounds ? (size_t)t : (size_t)(t & 1); }
	// round t's table and (zeroed) mask
	int ensure_round(int64_t t) {
		while (W.size() <= slot_of(t)) {
			int64_t *w = nullptr;
			u64 *m = nullptr;
			PGQ_TRY(temps.alloc(&w, Vn * LC));
			PGQ_TRY(temps.alloc(&m, Vn));
			PGQ_HIP_TRY(hipMemsetAsync(m, 0, Vn * 8, st));
			W.push_back(w), M.push_back(m);
		}
		return PGQ_OK;
	}
	WalkRound round_of(int64_t t) const { return WalkRound { W[slot_of(t)], M[slot_of(t)] }; }

	int prepare() {
		static_assert(sizeof(WalkCounters) <= Workspace::kTightCntBytes, "counter block too small");
		PGQ_TRY(ws->tight_cnt.reserve(Workspace::kTightCntBytes));
		tc = ws->tight_cnt.as<WalkCounters>();
		if (out.lists || query.mode == PGQ_MODE_TRAIL) PGQ_TRY(ensure_edge_ids(c));
		if (keep_rounds) PGQ_TRY(temps.alloc(&d_tabs, (size_t)PGQ_WALK_MAX_HOPS + 1));
		for (int32_t *&b : q) PGQ_TRY(temps.alloc(&b, Vn));
		return PGQ_OK;
	}

	// rows [lo, hi) of the sorted arrays, lane 0 = distinct source `base`
	int batch(int64_t lo, int64_t hi, int64_t base, u32 U) {
		const int64_t m = hi - lo;
		const unsigned cus = (unsigned)device_cus();
		const u32 *skey = ws->skey.as<u32>(), *sidx = ws->sidx.as<u32>();
		const int32_t *sdst = ws->sdst.as<int32_t>();
		WalkCounters h {};
		S.batches++;
		for (u64 *mk : M) PGQ_HIP_TRY(hipMemsetAsync(mk, 0, Vn * 8, st)); // what the batch before left
		PGQ_TRY(ensure_round(0));
		u32 nq = (u32)std::min<int64_t>(LC, (int64_t)U - base);
		{
			KernelTimer kt(st, K_PUSH);
			hipLaunchKernelGGL(k_walk_init, dim3(1), dim3(64), 0, st, ws->usrc.as<int32_t>(), (int64_t)U, base, W[0], M[0], q[0], tc);
			if (m > 0) hipLaunchKernelGGL(k_walk_rows, dim3(blocks_for(m)), dim3(256), 0, st, lo, hi, sidx, r_len, r_count, r_ng);
			hipLaunchKernelGGL(k_walk_after, dim3(blocks_for(std::max<int64_t>(m, 1))), dim3(256), 0, st, 0, query, lo, hi, skey, sidx, sdst, (u32)base,
			                   round_of(0), r_len, r_count, r_ng, (const int32_t *)nullptr, (u64 *)nullptr, 0, tc);
			kt.stop();
		}
		PGQ_TRY(stage.read_back(&h, tc, sizeof(h)));
		int par = 0;
		int rounds = 0;
		for (int64_t t = 1; t <= query.max_hops && nq > 0 && m > 0 && !(keep_rounds && h.pending == 0); t++) {
			PGQ_TRY(ensure_round(t));
			KernelTimer kt(st, K_PUSH);
			const WalkRound prev = round_of(t - 1), cur = round_of(t);
			hipLaunchKernelGGL(k_walk_round_reset, dim3(1), dim3(1), 0, st, tc, par ^ 1);
			hipLaunchKernelGGL(k_walk_activate, dim3(std::min(cus * 8, std::max(1u, (nq + 3) / 4))), dim3(256), 0, st, c->off, c->adj, prev.M, M[slot_of(t)], q[par],
			                   q[par ^ 1], tc, par);
			// (the new queue's fill is not known here: the grid is sized for a queue of any size, its wavefronts stride)
			hipLaunchKernelGGL(k_walk_pull, dim3(cus * 8), dim3(256), 0, st, c->roff, c->radj, prev.W, prev.M, W[slot_of(t)], cur.M, q[par ^ 1], tc, par ^ 1);
			hipLaunchKernelGGL(k_walk_after, dim3(blocks_for(std::max<int64_t>(m, nq))), dim3(256), 0, st, (int)t, query, lo, hi, skey, sidx, sdst, (u32)base,
			                   cur, r_len, r_count, r_ng, (const int32_t *)q[par], keep_rounds ? (u64 *)nullptr : M[slot_of(t - 1)], par, tc);
			kt.stop();
			PGQ_TRY(stage.read_back(&h, tc, sizeof(h)));
			S.levels++;
			rounds = (int)t;
			par ^= 1;
			nq = h.nq[par];
		}
		S.edges_scanned += (int64_t)h.edges;
		S.algo_bytes[K_PUSH] += (double)h.edges * (4.0 + 8.0 + 512.0);
		if (!keep_rounds) return PGQ_OK; // (before any staging)
		// walks and elements per row; where the batch's walks and staged blocks go
		h_tabs.assign((size_t)PGQ_WALK_MAX_HOPS + 1, WalkRound { nullptr, nullptr });
		for (int t = 0; t <= rounds; t++) h_tabs[t] = round_of(t);
		PGQ_HIP_TRY(hipMemcpyAsync(d_tabs, h_tabs.data(), h_tabs.size() * sizeof(WalkRound), hipMemcpyHostToDevice, st));
		if (query.mode) return search(lo, m, (u32)base, rounds);
		PGQ_TRY(emit(
		    m,
		    [&](int64_t *cntp, int64_t *cnte) {
			    hipLaunchKernelGGL(k_walk_plan, dim3(blocks_for(m)), dim3(256), 0, st, lo, hi, skey, sidx, sdst, (u32)base, d_tabs, query, rounds, r_np,
			                       r_el, r_count, r_ng, cntp, cnte);
		    },
		    [&](int64_t nwalks, const int64_t *ploc, const int64_t *eloc, int64_t at) {
			    hipLaunchKernelGGL(k_walk_unrank, dim3((unsigned)std::min<int64_t>(nwalks, 1 << 20)), dim3(64), 0, st, lo, m, nwalks, skey, sdst, (u32)base,
			                       ws->usrc.as<int32_t>(), c->off, c->adj, c->edge_ids, c->roff, c->radj, d_tabs, query, rounds, ploc, eloc, at,
			                       ws->tight_stage.as<int64_t>(), ws->soff.as<int64_t>(), tc);
		    }));
		PGQ_TRY(stage.read_back(&h, tc, sizeof(h))); // (also: the next batch's memsets and table upload come behind this batch's kernels)
		return unrank_status(h.error);
	}

	// Path modes: the batch's rows searched over the tables of rounds 0..rounds, a wavefront per row.  The counting pass is emit's
	// plan step; the count form ends behind it.
	template <bool EMIT> void launch_search(int64_t lo, int64_t m, u32 base, int rounds, int64_t *cntp, int64_t *cnte, const int64_t *ploc, const int64_t *eloc, int64_t at) {
		hipLaunchKernelGGL(k_mode_search<EMIT>, dim3((unsigned)std::min<int64_t>(m, 1 << 20)), dim3(64), 0, st, lo, m, ws->skey.as<u32>(), ws->sidx.as<u32>(),
		                   ws->sdst.as<int32_t>(), base, ws->usrc.as<int32_t>(), c->off, c->adj, c->edge_ids, c->roff, c->radj, d_tabs, query, rounds, step_cap,
		                   r_len, r_count, r_np, r_el, r_ng, cntp, cnte, ploc, eloc, at, ws->tight_stage.as<int64_t>(), ws->soff.as<int64_t>(), tc);
	}
	// what a pass left in the batch's counters: its steps booked, the step cap and the search's own errors reported
	int search_status() {
		WalkCounters h {};
		PGQ_TRY(stage.read_back(&h, tc, sizeof(h)));
		ModeSteps &ms = mode_steps();
		ms.total += (int64_t)(h.steps - steps_seen);
		ms.row_max = std::max(ms.row_max, (int64_t)h.row_max);
		steps_seen = h.steps;
		if (h.error & kModeOverCap)
			return fail(PGQ_ERR_UNSUPPORTED, name + ": a row's search took more than mode_step_cap = " + std::to_string(step_cap) +
			                                     " steps in one pass (finding a simple path of an exact length is NP-hard; raise the option or lower the bounds)");
		return unrank_status(h.error);
	}
	int search(int64_t lo, int64_t m, u32 base, int rounds) {
		steps_seen = 0; // (k_walk_init zeroed the batch's counters)
		if (m == 0) return PGQ_OK;
		if (!out.lists) {
			KernelTimer kt(st, K_RECON);
			launch_search<false>(lo, m, base, rounds, nullptr, nullptr, nullptr, nullptr, 0);
			kt.stop();
			return search_status();
		}
		PGQ_TRY(emit(
		    m, [&](int64_t *cntp, int64_t *cnte) { launch_search<false>(lo, m, base, rounds, cntp, cnte, nullptr, nullptr, 0); },
		    [&](int64_t, const int64_t *ploc, const int64_t *eloc, int64_t at) { launch_search<true>(lo, m, base, rounds, nullptr, nullptr, ploc, eloc, at); },
		    [&] { return search_status(); }));
		return search_status();
	}
};

// min(count, limit) over n counts, -1 (NULL) kept: pgq_walk_count_mode under NONE / WALK
__global__ void k_walk_clamp(int64_t n, int64_t limit, int64_t *__restrict__ count) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n && count[i] > limit) count[i] = limit;
}

} // namespace pgq

using namespace pgq;

// ---- the C entry points: each is its argument list, a query and one of the helpers below -----------------------------------------

// what a form's q.limit is, for the error text: k (the list forms), the count's limit, max_paths beside the groups
enum WalkForm { kWalkK, kWalkLimit, kWalkGroups };

// The call's arguments as the query.  path_mode: null for the entry points that have none.  NONE / WALK become mode 0 here and
// nowhere else; any other number is kept, for walk_check to refuse.  A call that has a path_mode starts the thread's step counts
// (pgq_debug_mode_steps) afresh, whatever becomes of it.
static WalkQuery walk_query(int64_t min_hops, int64_t max_hops, const int *path_mode, int64_t groups, int64_t limit) {
	if (path_mode) mode_steps() = ModeSteps {};
	const bool walks = !path_mode || *path_mode == PGQ_MODE_NONE || *path_mode == PGQ_MODE_WALK;
	return WalkQuery { min_hops, max_hops, groups, limit, walks ? 0 : *path_mode };
}

// the mode's number, the bounds, the limit, the groups; an unbounded upper is not built under a mode either
static int walk_check(const WalkQuery &q, WalkForm form) {
	static const char *const limit_name[] = { "k", "limit", "max_paths" };
	if (q.mode < 0 || q.mode > PGQ_MODE_ACYCLIC) return fail(PGQ_ERR_INVALID_ARG, "path_mode must be PGQ_MODE_NONE, _WALK, _SIMPLE, _TRAIL or _ACYCLIC (0 .. 4)");
	if (q.min_hops < 0) return fail(PGQ_ERR_INVALID_ARG, "min_hops must not be negative");
	if (q.max_hops < q.min_hops) return fail(PGQ_ERR_INVALID_ARG, "max_hops must not be below min_hops");
	if (q.limit < 1) return fail(PGQ_ERR_INVALID_ARG, std::string(limit_name[form]) + " must be at least 1");
	if (q.max_hops > PGQ_WALK_MAX_HOPS)
		return fail(PGQ_ERR_UNSUPPORTED, "walks need an upper bound of at most " + std::to_string(PGQ_WALK_MAX_HOPS) +
		                                     " edges: in a cyclic graph the number of walks is unbounded");
	if (form == kWalkGroups && q.groups < 1) return fail(PGQ_ERR_INVALID_ARG, "groups must be at least 1");
	return PGQ_OK;
}

// The count forms' run.  Under a mode: the search's counting pass.  The walks themselves: their rounds have no limit, the count
// is cut at q.limit behind them (pgq_walk_count asks with INT64_MAX: nothing to cut).
static int walk_count_run(pgq_csr *csr, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst, WalkQuery q, ListOut &o) {
	const int64_t limit = q.limit;
	if (!q.mode) q.limit = kWalkMax;
	PGQ_TRY(WalkCall(csr, ws, n, d_src, d_dst, q, o).run());
	if (q.mode || limit == kWalkMax) return PGQ_OK;
	if (n > 0) hipLaunchKernelGGL(k_walk_clamp, dim3(blocks_for(n)), dim3(256), 0, ws->stream, n, limit, o.d_count);
	PGQ_HIP_TRY(hipStreamSynchronize(ws->stream));
	return PGQ_OK;
}
static int walk_count_bulk(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, const WalkQuery &q, int64_t *d_out_count) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	auto check = [&]() -> int {
		PGQ_TRY(check_arrays(csr, n, d_src && d_dst && d_out_count, "NULL device array"));
		return walk_check(q, kWalkLimit);
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		ListOut out;
		out.d_count = d_out_count;
		return walk_count_run(csr, ws, n, d_src, d_dst, q, out);
	});
}
static int walk_count_chunk(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, const WalkQuery &q, int64_t *out_count, uint64_t *out_valid) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	auto check = [&] { return count_chunk_check(csr, V, n, out_count, out_valid, [&] { return walk_check(q, kWalkLimit); }); };
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		auto run = [&](ListOut &o, const int64_t *d_src, const int64_t *d_dst) { return walk_count_run(csr, ws, n, d_src, d_dst, q, o); };
		return count_chunk_body(ws, V, n, src, dst, run, out_count, out_valid);
	});
}

// The bulk list forms: `out` arrives with the caller's arrays and capacities (d_ng: the groups' form alone).
static int walk_lists_bulk(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, WalkQuery q, WalkForm form, ListOut out, int64_t *paths_used,
                           int64_t *child_used) {
	if (paths_used) *paths_used = 0;
	if (child_used) *child_used = 0;
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	auto check = [&]() -> int {
		const bool arrays = d_src && d_dst && out.d_len && out.d_count && out.d_first && out.d_np && (out.d_ng || form != kWalkGroups) && out.d_path_off &&
		                    out.d_path_hops && out.d_child;
		PGQ_TRY(check_arrays(csr, n, arrays, "NULL device array"));
		if (out.path_cap < 0 || out.child_cap < 0) return fail(PGQ_ERR_INVALID_ARG, "negative capacity");
		return walk_check(q, form);
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		q.limit = std::min<int64_t>(q.limit, 1LL << 31);
		return list_bulk_body(out, q.limit, [&](ListOut &o) { return WalkCall(csr, ws, n, d_src, d_dst, q, o).run(); }, paths_used, child_used);
	});
}
// the ListOut of a bulk list form's arguments
static ListOut walk_bulk_out(int64_t *d_len, int64_t *d_count, int64_t *d_first, int64_t *d_np, int64_t *d_ng, int64_t *d_path_off, int64_t *d_path_hops,
                             int64_t path_cap, int64_t *d_child, int64_t child_cap) {
	ListOut out;
	out.d_len = d_len, out.d_count = d_count, out.d_first = d_first, out.d_np = d_np, out.d_ng = d_ng;
	out.d_path_off = d_path_off, out.d_path_hops = d_path_hops, out.path_cap = path_cap, out.d_child = d_child, out.child_cap = child_cap;
	return out;
}

// The chunk list forms (o.ngroups: the groups' form alone).
static int walk_lists_chunk(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, WalkQuery q, WalkForm form, ListChunkOut o) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	uint64_t no_rows = 0; // (the groups' form with n == 0: nothing is written through it)
	const bool no_groups_out = form == kWalkGroups && !o.ngroups;
	if (no_groups_out) o.ngroups = &no_rows;
	auto check = [&] {
		return list_chunk_check(csr, V, n, o, [&]() -> int {
			if (n > 0 && no_groups_out) return fail(PGQ_ERR_INVALID_ARG, "NULL output");
			return walk_check(q, form);
		});
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		q.limit = std::min<int64_t>(q.limit, 1LL << 31);
		auto run = [&](ListOut &lo, const int64_t *d_src, const int64_t *d_dst) { return WalkCall(csr, ws, n, d_src, d_dst, q, lo).run(); };
		return list_chunk_body(ws, V, n, src, dst, q.limit, run, o);
	});
}

extern "C" {

int pgq_walk_count_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops, int64_t max_hops,
                               int64_t *d_out_count) {
	return walk_count_bulk(csr, n, d_src, d_dst, walk_query(min_hops, max_hops, nullptr, 0, kWalkMax), d_out_count);
}

int pgq_k_shortest_walks_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops, int64_t max_hops, int64_t k,
                                     int64_t *d_out_len, int64_t *d_out_count, int64_t *d_out_first, int64_t *d_out_npaths, int64_t *d_path_offset,
                                     int64_t *d_path_hops, int64_t path_cap, int64_t *d_child, int64_t child_cap, int64_t *paths_used, int64_t *child_used) {
	return walk_lists_bulk(csr, n, d_src, d_dst, walk_query(min_hops, max_hops, nullptr, 0, k), kWalkK,
	                       walk_bulk_out(d_out_len, d_out_count, d_out_first, d_out_npaths, nullptr, d_path_offset, d_path_hops, path_cap, d_child, child_cap),
	                       paths_used, child_used);
}

int pgq_walk_count(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops, int64_t *out_count,
                   uint64_t *out_valid) {
	return walk_count_chunk(csr, V, n, src, dst, walk_query(min_hops, max_hops, nullptr, 0, kWalkMax), out_count, out_valid);
}

int pgq_k_shortest_walks(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops, int64_t k,
                         uint64_t *out_first, uint64_t *out_npaths, uint64_t *out_valid, const uint64_t **out_path_offset, const uint64_t **out_path_length,
                         uint64_t *out_path_total, const int64_t **out_child, uint64_t *out_child_len) {
	return walk_lists_chunk(csr, V, n, src, dst, walk_query(min_hops, max_hops, nullptr, 0, k), kWalkK,
	                        ListChunkOut { out_first, out_npaths, out_valid, out_path_offset, out_path_length, out_path_total, out_child, out_child_len });
}

// ---- the path modes ------------------------------------------------------------------------------------------------------------

int pgq_walk_count_mode_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops, int64_t max_hops, int64_t limit,
                                    int path_mode, int64_t *d_out_count) {
	return walk_count_bulk(csr, n, d_src, d_dst, walk_query(min_hops, max_hops, &path_mode, 0, limit), d_out_count);
}

int pgq_k_shortest_walks_mode_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops, int64_t max_hops, int64_t k,
                                          int path_mode, int64_t *d_out_len, int64_t *d_out_count, int64_t *d_out_first, int64_t *d_out_npaths,
                                          int64_t *d_path_offset, int64_t *d_path_hops, int64_t path_cap, int64_t *d_child, int64_t child_cap, int64_t *paths_used,
                                          int64_t *child_used) {
	return walk_lists_bulk(csr, n, d_src, d_dst, walk_query(min_hops, max_hops, &path_mode, 0, k), kWalkK,
	                       walk_bulk_out(d_out_len, d_out_count, d_out_first, d_out_npaths, nullptr, d_path_offset, d_path_hops, path_cap, d_child, child_cap),
	                       paths_used, child_used);
}

int pgq_walk_count_mode(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops, int64_t limit, int path_mode,
                        int64_t *out_count, uint64_t *out_valid) {
	return walk_count_chunk(csr, V, n, src, dst, walk_query(min_hops, max_hops, &path_mode, 0, limit), out_count, out_valid);
}

int pgq_k_shortest_walks_mode(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops, int64_t k, int path_mode,
                              uint64_t *out_first, uint64_t *out_npaths, uint64_t *out_valid, const uint64_t **out_path_offset, const uint64_t **out_path_length,
                              uint64_t *out_path_total, const int64_t **out_child, uint64_t *out_child_len) {
	return walk_lists_chunk(csr, V, n, src, dst, walk_query(min_hops, max_hops, &path_mode, 0, k), kWalkK,
	                        ListChunkOut { out_first, out_npaths, out_valid, out_path_offset, out_path_length, out_path_total, out_child, out_child_len });
}

// ---- SHORTEST k GROUP ----------------------------------------------------------------------------------------------------------

int pgq_k_shortest_groups_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops, int64_t max_hops, int64_t groups,
                                      int64_t max_paths, int path_mode, int64_t *d_out_len, int64_t *d_out_count, int64_t *d_out_first, int64_t *d_out_npaths,
                                      int64_t *d_out_ngroups, int64_t *d_path_offset, int64_t *d_path_hops, int64_t path_cap, int64_t *d_child, int64_t child_cap,
                                      int64_t *paths_used, int64_t *child_used) {
	return walk_lists_bulk(csr, n, d_src, d_dst, walk_query(min_hops, max_hops, &path_mode, groups, max_paths), kWalkGroups,
	                       walk_bulk_out(d_out_len, d_out_count, d_out_first, d_out_npaths, d_out_ngroups, d_path_offset, d_path_hops, path_cap, d_child, child_cap),
	                       paths_used, child_used);
}

int pgq_k_shortest_groups(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops, int64_t groups, int64_t max_paths,
                          int path_mode, uint64_t *out_first, uint64_t *out_npaths, uint64_t *out_ngroups, uint64_t *out_valid, const uint64_t **out_path_offset,
                          const uint64_t **out_path_length, uint64_t *out_path_total, const int64_t **out_child, uint64_t *out_child_len) {
	return walk_lists_chunk(csr, V, n, src, dst, walk_query(min_hops, max_hops, &path_mode, groups, max_paths), kWalkGroups,
	                        ListChunkOut { out_first, out_npaths, out_valid, out_path_offset, out_path_length, out_path_total, out_child, out_child_len, out_ngroups });
}

int pgq_debug_mode_steps(int64_t *total, int64_t *row_max) {
	if (!total || !row_max) return fail(PGQ_ERR_INVALID_ARG, "pgq_debug_mode_steps: NULL output");
	*total = mode_steps().total;
	*row_max = mode_steps().row_max;
	return PGQ_OK;
}

} // extern "C"

#include "pgq_walk_length.hip" // walk_length: stage 1 by distance, bit rounds over the rows left, on this file's k_walk_activate and counters
