// pgq_all_shortest.hip — shortestpath_count and all_shortestpaths on MI355X: how many shortest paths a row has, and the first
// max_paths of them as lists, for SQL/PGQ's ALL SHORTEST.  The reference has no counterpart: its binder rejects the form
// ("ALL SHORTEST has not been implemented yet", match.cpp:82).  Every list follows shortestpath's layout (shortest_path.cpp:43-207).
//
// The root file of pgq_all_shortest.o, compiled on its own.  The hop counts live in cheapest_path's H table (ws->tight_h, 64 lanes
// per vertex, "-1 everywhere between calls"), the frontier masks and queues are k_tight_levels': workspace fields with their
// invariants (pgq_search.h), no code of pgq_cheapest_path.o.  From pgq_relax.h: LC and fill32, nothing else.  What this call
// shares with k_shortest_walks (pgq_k_walks.o) — the saturating add and scan, the pull's inner loop, one step of the unranking,
// the tails kernel, the list staging, the call skeleton ListCall with its layout, the C entry points' prologues and epilogues —
// is in pgq_path_lists.h, described there once.  Weights are never read: the calls work on any CSR.
//
// The contract, for a row (src, dst).  L[v] = the BFS level of v from src, d = L[dst];
//   sigma[src] = 1,  sigma[x] = min(INT64_MAX, sum of sigma[u] over the in-slots (u, x) with L[u] = L[x] - 1)
// Parallel edges are separate slots and count separately (a path is a sequence of edges); the sum saturates, it never wraps.
//   count        sigma[dst]; 1 for src == dst; 0 when dst is unreachable or d > max_hops; NULL (-1) for a NULL src or dst
//   the paths    the first min(sigma[dst], max_paths) shortest paths, each [x_0, e_1, x_1, ..., e_d, x_d], in the lexicographic
//                order of in-list positions read from the destination end: first by (x_{d-1}, forward slot of e_d), then by
//                (x_{d-2}, slot of e_{d-1}), ...  Path number r is found by UNRANKING: x_d = dst; at step t scan x_t's in-list in
//                its stored order — the reverse CSR is the forward slot list stably sorted by destination, so an in-list is
//                ordered by (parent id, forward slot) — and for every in-slot (u, x_t) with L[u] = t - 1: r < sigma[u] takes the
//                slot, otherwise r -= sigma[u].  The taken slot is the m-th in-slot from u into x_t, its edge the m-th slot of
//                u's out-list whose target is x_t.  Path 0 is shortestpath's list (smallest parent of the level, its first slot);
//                with max_paths = 1 the call is shortestpath_within, one level deeper.
//   special      src == dst: [[src]].  NULL src, NULL dst, unreachable, d > max_hops: NULL, no inner list, no payload.
// A saturated sigma stays valid for unranking: every emitted rank is below 2^31, and a prefix sum that saturates has passed it.
//
// Per lane batch (at most 64 distinct sources, lane l = search l):
//   1. k_asp_levels, a launch per round, in k_tight_levels' shape with every slot tight: a wavefront per frontier vertex v walks
//      v's out-list, H[n][l] is set ONCE, to the round's number; the returning atomicOr on n's mask word queues n once per round.
//      Freshness comes from kernel boundaries: two wavefronts that set the same H[n][l] in a round store the same value.
//   2. k_asp_sigma, behind it in the same round: a wavefront per newly queued vertex n walks n's in-list; lane l with
//      H[n][l] == round adds sigma[u][l] where u's mask word of the round before has bit l (that word IS "H[u][l] == round - 1").
//      The in-list is read 64 entries and 64 mask words at a time, a ballot names the neighbours of the last frontier and only
//      those are visited: a 512-byte sigma row each.  The add saturates in registers, one plain store per
//      (vertex, lane) writes sigma: written once, no atomics, the same on every run.  The wavefront also puts n on the batch's
//      touched list when this round is the first to give it any H.
//   3. k_asp_after clears the consumed mask words and counts the destinations still without H.  The rounds end with the
//      frontier, when every destination has its H (its sigma was completed in the same round), or after max_hops rounds.
//   4. k_asp_plan, a thread per row: hops, sigma, the paths the row emits and their elements; two exclusive scans place them.
//   5. k_asp_unrank, a wavefront per emitted path: step t is unrank_step (pgq_path_lists.h) with the weight sigma[u][l] where
//      H[u][l] == t - 1.  Loops are bounded by d and the lists' lengths; a step that finds nothing, or a walk that does not end
//      on the lane's source, raises the batch's error flag and the call fails with PGQ_ERR_HIP.
//   6. H and the masks go back to "none" over the touched list.  sigma needs no reset: it is only read where H says it was
//      written in this batch.  On an error return ws->tight_V stays invalid and the next call fills H whole (PathBatches' rule).
//   7. Behind the last batch (ListCall::layout): the src == dst and NULL rows, scans in ROW order, and the gather of outer
//      entries {first path, paths}, inner entries {offset, 2 d + 1} and the child payload.  Results go to the caller only then: a
//      call that fails has written nothing.
// Kernel-class time: the rounds are K_PUSH, plan / unranking / gather K_RECON.  768 bytes per vertex per batch: H (shared with
// cheapest_path) and sigma (from the block cache for the call).
// Not built: _multi forms, splitting long in-lists over several wavefronts (a list is walked by the one wavefront that meets
// it), sharing prefixes between the paths of one row, any change to how shortestpath or iterativelength are routed.

#include "pgq_path_lists.h"

namespace pgq {

struct AspCounters {
	u32 nq[2];   // frontier vertices by round parity
	u32 pending; // destinations of the batch without H
	u32 error;   // unranking: no parent (2), no slot (4), not at the source (8)
	u32 nt;      // touched vertices
	u32 pad;
	u64 edges;   // adjacency entries the rounds walked
};

// the batch's sources: H = 0, sigma = 1, in the first frontier and on the touched list (distinct sources: distinct vertices)
__global__ void k_asp_init(const int32_t *__restrict__ usrc, int64_t U, int64_t base, int32_t *__restrict__ H, int64_t *__restrict__ sigma,
                           u64 *__restrict__ mask, int32_t *__restrict__ q, int32_t *__restrict__ touched, AspCounters *__restrict__ tc) {
	const int l = threadIdx.x;
	const int64_t g = base + l;
	if (l == 0) {
		const u32 cnt = (u32)min((int64_t)LC, U - base);
		tc->nq[0] = cnt;
		tc->nq[1] = 0;
		tc->pending = 0;
		tc->error = 0;
		tc->nt = cnt;
		tc->edges = 0;
	}
	if (l >= LC || g >= U) return;
	const int v = usrc[g];
	H[(size_t)v * LC + l] = 0;
	sigma[(size_t)v * LC + l] = 1;
	mask[v] = 1ull << l;
	q[l] = v;
	touched[l] = v;
}

__global__ void k_asp_round_reset(AspCounters *__restrict__ tc, int next_par) {
	tc->nq[next_par] = 0;
	tc->pending = 0;
}

// One round's levels: a wavefront per frontier vertex v, lane l = search l.  mask_cur[v] = the lanes whose H[v] the round before
// set; it stays in place for k_asp_sigma.
__global__ __launch_bounds__(256) void k_asp_levels(const int64_t *__restrict__ off, const int32_t *__restrict__ adj, int32_t *__restrict__ H,
                                                    const u64 *__restrict__ mask_cur, u64 *__restrict__ mask_nxt,
                                                    const int32_t *__restrict__ qcur, int32_t *__restrict__ qnxt,
                                                    AspCounters *__restrict__ tc, int par, int round) {
	const int lane = threadIdx.x & 63;
	const u32 wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
	const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
	const u32 nq = tc->nq[par];
	for (u32 i = wave; i < nq; i += nwaves) {
		const int v = qcur[i];
		const bool mine = (mask_cur[v] >> lane) & 1ull;
		const int64_t b = off[v], e = off[v + 1];
		for (int64_t k0 = b; k0 < e; k0 += 64) { // 64 targets per coalesced load, handed round by lane index
			const int mine_n = k0 + lane < e ? adj[k0 + lane] : -1;
			const int cnt = (int)min((int64_t)64, e - k0);
			for (int t = 0; t < cnt; t++) {
				const int n = __shfl(mine_n, t);
				bool fresh = false;
				if (mine && H[(size_t)n * LC + lane] < 0) {
					H[(size_t)n * LC + lane] = round;
					fresh = true;
				}
				const u64 fm = __ballot(fresh);
				if (fm && lane == 0 && atomicOr(&mask_nxt[n], fm) == 0ull) qnxt[atomicAdd(&tc->nq[par ^ 1], 1u)] = n;
			}
		}
		if (lane == 0 && e > b) atomicAdd(&tc->edges, (u64)(e - b));
	}
}

// The round's sigma: a wavefront per vertex n the round queued (once), lane l = search l.
__global__ __launch_bounds__(256) void k_asp_sigma(const int64_t *__restrict__ roff, const int32_t *__restrict__ radj, const int32_t *__restrict__ H,
                                                   int64_t *__restrict__ sigma, const u64 *__restrict__ mask_prev,
                                                   const int32_t *__restrict__ qnew, int32_t *__restrict__ touched,
                                                   AspCounters *__restrict__ tc, int par_new, int round) {
	const int lane = threadIdx.x & 63;
	const u32 wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
	const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
	const u32 nq = tc->nq[par_new];
	for (u32 i = wave; i < nq; i += nwaves) {
		const int n = qnew[i];
		const int h = H[(size_t)n * LC + lane];
		const bool want = h == round;
		const bool first = !__any(h >= 0 && h < round); // no lane had reached n before this round
		// (mask_prev[u] IS "H[u][l] == round - 1": only the neighbours of the last frontier are visited)
		const int64_t acc = pull_masked_sum(n, lane, want, roff, radj, mask_prev, sigma);
		const int64_t rb = roff[n], re = roff[n + 1];
		if (want) sigma[(size_t)n * LC + lane] = acc;
		if (lane == 0) {
			if (first) touched[atomicAdd(&tc->nt, 1u)] = n; // a vertex is queued once per round and is `first` in one round only: <= V entries
			if (re > rb) atomicAdd(&tc->edges, (u64)(re - rb));
		}
	}
}

// the round is over: the consumed frontier's mask words back to zero, the destinations still without H counted
__global__ void k_asp_after(const int32_t *__restrict__ qcur, u64 *__restrict__ mask_cur, int par, int64_t lo, int64_t hi,
                            const u32 *__restrict__ skey, const int32_t *__restrict__ sdst, u32 base_lane, const int32_t *__restrict__ H,
                            AspCounters *__restrict__ tc) {
	const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t < (int64_t)tc->nq[par]) mask_cur[qcur[t]] = 0;
	const int64_t i = lo + t;
	const bool open = i < hi && H[(size_t)sdst[i] * LC + (skey[i] - base_lane)] < 0;
	const u64 om = __ballot(open);
	if (om && (threadIdx.x & 63) == 0) atomicAdd(&tc->pending, (u32)__popcll(om));
}

// per row of the batch: hops (-1: none within the bound), sigma, the paths it emits, their elements
__global__ void k_asp_plan(int64_t lo, int64_t hi, const u32 *__restrict__ skey, const u32 *__restrict__ sidx, const int32_t *__restrict__ sdst,
                           u32 base_lane, const int32_t *__restrict__ H, const int64_t *__restrict__ sigma, int64_t max_paths,
                           int64_t *__restrict__ r_len, int64_t *__restrict__ r_count, int64_t *__restrict__ r_np, int64_t *__restrict__ r_el,
                           int64_t *__restrict__ cntp, int64_t *__restrict__ cnte) {
	const int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= hi) return;
	const size_t cell = (size_t)sdst[i] * LC + (skey[i] - base_lane);
	const int64_t d = H[cell];
	const int64_t count = d < 0 ? 0 : sigma[cell];
	const u32 row = sidx[i];
	r_len[row] = d < 0 ? -1 : d;
	r_count[row] = count;
	if (!r_np) return; // the count alone
	const int64_t np = min(count, max_paths);
	r_np[row] = np;
	cntp[i - lo] = np;
	r_el[row] = cnte[i - lo] = np * (2 * d + 1); // np <= 2^31, 2 d + 1 < 2^32 (np = 0 where d < 0)
}

// One wavefront per emitted path (row, rank): the list, written back to front into the row's slice of the staging buffer.
__global__ __launch_bounds__(64) void k_asp_unrank(int64_t lo, int64_t m, int64_t npaths, const u32 *__restrict__ skey, const int32_t *__restrict__ sdst,
                                                  u32 base_lane, const int32_t *__restrict__ usrc, const int64_t *__restrict__ off,
                                                  const int32_t *__restrict__ adj, const int64_t *__restrict__ edge_ids,
                                                  const int64_t *__restrict__ roff, const int32_t *__restrict__ radj,
                                                  const int32_t *__restrict__ H, const int64_t *__restrict__ sigma,
                                                  const int64_t *__restrict__ ploc, const int64_t *__restrict__ eloc, int64_t stage_base,
                                                  int64_t *__restrict__ stage, int64_t *__restrict__ soff, AspCounters *__restrict__ tc) {
	const int lane = threadIdx.x;
	for (int64_t p = blockIdx.x; p < npaths; p += gridDim.x) {
		const int64_t a = rank_row(ploc, m, p);
		const int64_t i = lo + a;
		int64_t r = p - ploc[a];
		const u32 l = skey[i] - base_lane;
		int x = sdst[i];
		const int d = H[(size_t)x * LC + l];
		if (d < 1) { // (k_asp_plan gave such a row no path)
			if (lane == 0) atomicOr(&tc->error, 2u);
			continue;
		}
		int64_t *out = stage + stage_base + eloc[a] + r * (2 * (int64_t)d + 1);
		if (lane == 0) {
			if (r == 0) soff[i] = stage_base + eloc[a];
			out[2 * d] = x;
		}
		bool lost = false;
		for (int t = d; t >= 1 && !lost; t--) {
			const UnrankStep step = unrank_step(x, r, lane, roff, radj, off, adj, [&](int cand) -> int64_t {
				return H[(size_t)cand * LC + l] == t - 1 ? sigma[(size_t)cand * LC + l] : 0;
			});
			if (step.error) {
				if (lane == 0) atomicOr(&tc->error, step.error);
				lost = true;
				break;
			}
			if (lane == 0) {
				out[2 * t - 1] = edge_ids ? edge_ids[step.slot] : step.slot;
				out[2 * t - 2] = step.u;
			}
			x = step.u;
		}
		if (!lost && lane == 0 && x != usrc[base_lane + l]) atomicOr(&tc->error, 8u);
	}
}

// the batch is over: H and both mask words back to "none" wherever the batch set them (every such vertex is on the touched list)
__global__ void k_asp_reset(const int32_t *__restrict__ touched, const AspCounters *__restrict__ tc, int32_t *__restrict__ H,
                            u64 *__restrict__ mask0, u64 *__restrict__ mask1) {
	const u32 nt = tc->nt;
	int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (; t < (int64_t)nt * LC; t += stride) {
		const int v = touched[t / LC];
		H[(size_t)v * LC + (t % LC)] = -1;
		if (t % LC == 0) mask0[v] = mask1[v] = 0;
	}
}

// Row order: a wavefront per sorted position below lo_null copies the row's staged lists (they lie behind each other by rank)
// to its place in the child payload and writes its inner entries; src == dst rows write their one-element list.
__global__ __launch_bounds__(64) void k_asp_gather(int64_t lo_trivial, int64_t lo_null, const u32 *__restrict__ sidx, const int32_t *__restrict__ sdst,
                                                  const int64_t *__restrict__ r_len, const int64_t *__restrict__ r_np,
                                                  const int64_t *__restrict__ r_first, const int64_t *__restrict__ r_eoff,
                                                  const int64_t *__restrict__ soff, const int64_t *__restrict__ stage,
                                                  int64_t *__restrict__ path_off, int64_t *__restrict__ path_len, int64_t *__restrict__ child) {
	const int lane = threadIdx.x;
	for (int64_t i = blockIdx.x; i < lo_null; i += gridDim.x) {
		const u32 row = sidx[i];
		const int64_t np = r_np[row];
		if (np <= 0) continue;
		const int64_t w = 2 * r_len[row] + 1, f = r_first[row], eo = r_eoff[row];
		if (i >= lo_trivial) {
			if (lane == 0) {
				child[eo] = sdst[i];
				path_off[f] = eo;
				if (path_len) path_len[f] = 1;
			}
			continue;
		}
		const int64_t *in = stage + soff[i];
		for (int64_t k = lane; k < np * w; k += 64) child[eo + k] = in[k];
		for (int64_t k = lane; k < np; k += 64) {
			path_off[f + k] = eo + k * w;
			if (path_len) path_len[f + k] = w;
		}
	}
}

// The level and sigma rounds of the lane batches on ListCall's skeleton (pgq_path_lists.h): its run, emit and layout.
class AspCall : ListCall {
public:
	AspCall(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t max_hops, ListOut &out)
	    : ListCall(c, ws, n, d_src, d_dst, out, "all_shortestpaths", "paths"), max_hops(max_hops), temps(ws->stream) {}

	int run() {
		return ListCall::run(
		    false, [&] { return prepare(); }, [&](int64_t lo, int64_t hi, int64_t base, u32 U) { return batch(lo, hi, base, U); },
		    [&](int nb) {
			    if (nb > 0) ws->tight_V = c->V; // behind the last batch's reset, waited for
			    return layout(nb, 0, [&](int64_t lo_t, int64_t lo_n, int64_t *path_off, int64_t *path_len, int64_t *child) {
				    hipLaunchKernelGGL(k_asp_gather, dim3((unsigned)std::min<int64_t>(lo_n, 1 << 20)), dim3(64), 0, st, lo_t, lo_n, ws->sidx.as<u32>(),
				                       ws->sdst.as<int32_t>(), r_len, r_np, r_first, r_eoff, ws->soff.as<int64_t>(), ws->tight_stage.as<int64_t>(), path_off, path_len, child);
			    }, 16.0);
		    });
	}

private:
	const int64_t max_hops;
	DevTemps temps; // sigma and the touched list: block-cache memory for the call
	AspCounters *tc = nullptr;
	int64_t *sigma = nullptr;
	int32_t *touched = nullptr;

	// H as PathBatches::prepare keeps it (shared with cheapest_path: tight_V says for which V "-1 everywhere" holds)
	int prepare() {
		static_assert(sizeof(AspCounters) <= Workspace::kTightCntBytes, "counter block too small");
		PGQ_TRY(ws->tight_cnt.reserve(Workspace::kTightCntBytes));
		tc = ws->tight_cnt.as<AspCounters>();
		if (out.lists) PGQ_TRY(ensure_edge_ids(c));
		for (DevBuf &b : ws->tight_mask) PGQ_TRY(b.reserve(Vn * 8));
		for (DevBuf &b : ws->tight_q) PGQ_TRY(b.reserve(Vn * 4));
		const size_t cells = Vn * LC;
		PGQ_TRY(temps.alloc(&sigma, cells));
		PGQ_TRY(temps.alloc(&touched, Vn));
		const bool fresh = ws->tight_h.cap < cells * 4 || ws->tight_V != c->V;
		ws->tight_V = -1; // stays invalid if the call bails out half-way
		PGQ_TRY(ws->tight_h.reserve(cells * 4));
		if (fresh) fill32(ws->tight_h.as<int32_t>(), (int64_t)cells, -1, st);
		for (DevBuf &b : ws->tight_mask) PGQ_HIP_TRY(hipMemsetAsync(b.p, 0, Vn * 8, st));
		return PGQ_OK;
	}

	// rows [lo, hi) of the sorted arrays, lane 0 = distinct source `base`
	int batch(int64_t lo, int64_t hi, int64_t base, u32 U) {
		int32_t *H = ws->tight_h.as<int32_t>();
		const int64_t m = hi - lo;
		const unsigned cus = (unsigned)device_cus();
		const u32 *skey = ws->skey.as<u32>(), *sidx = ws->sidx.as<u32>();
		const int32_t *sdst = ws->sdst.as<int32_t>();
		AspCounters h {};
		S.batches++;
		{
			KernelTimer kt(st, K_PUSH);
			hipLaunchKernelGGL(k_asp_init, dim3(1), dim3(64), 0, st, ws->usrc.as<int32_t>(), (int64_t)U, base, H, sigma, ws->tight_mask[0].as<u64>(),
			                   ws->tight_q[0].as<int32_t>(), touched, tc);
			kt.stop();
		}
		int par = 0;
		u32 nq = (u32)std::min<int64_t>(LC, (int64_t)U - base);
		for (int64_t round = 1; nq > 0 && m > 0 && round <= max_hops; round++) { // (at most V - 1 rounds find anything; none is launched past the bound)
			KernelTimer kt(st, K_PUSH);
			u64 *mcur = ws->tight_mask[par].as<u64>(), *mnxt = ws->tight_mask[par ^ 1].as<u64>();
			int32_t *qcur = ws->tight_q[par].as<int32_t>(), *qnxt = ws->tight_q[par ^ 1].as<int32_t>();
			hipLaunchKernelGGL(k_asp_round_reset, dim3(1), dim3(1), 0, st, tc, par ^ 1);
			hipLaunchKernelGGL(k_asp_levels, dim3(std::min(cus * 8, std::max(1u, (nq + 3) / 4))), dim3(256), 0, st, c->off, c->adj, H, mcur, mnxt, qcur, qnxt, tc,
			                   par, (int)round);
			// (the new queue's fill is not known here: the grid is sized for a frontier of any size, its wavefronts stride)
			hipLaunchKernelGGL(k_asp_sigma, dim3(cus * 8), dim3(256), 0, st, c->roff, c->radj, H, sigma, mcur, qnxt, touched, tc, par ^ 1, (int)round);
			hipLaunchKernelGGL(k_asp_after, dim3(blocks_for(std::max<int64_t>(m, nq))), dim3(256), 0, st, qcur, mcur, par, lo, hi, skey, sdst, (u32)base, H, tc);
			kt.stop();
			PGQ_TRY(stage.read_back(&h, tc, sizeof(h)));
			S.levels++;
			par ^= 1;
			nq = h.nq[par];
			if (h.pending == 0) break; // every destination has its H and its sigma: the rest of the graph is nobody's business
		}
		S.edges_scanned += (int64_t)h.edges;
		S.algo_bytes[K_PUSH] += (double)h.edges * (4.0 + 256.0 + 512.0);
		// hops, sigma, paths and elements per row (the count alone: no places, nothing staged)
		auto plan = [&](int64_t *cntp, int64_t *cnte) {
			hipLaunchKernelGGL(k_asp_plan, dim3(blocks_for(m)), dim3(256), 0, st, lo, hi, skey, sidx, sdst, (u32)base, H, sigma, out.limit, r_len, r_count,
			                   out.lists ? r_np : nullptr, r_el, cntp, cnte);
		};
		if (out.lists) {
			PGQ_TRY(emit(m, plan, [&](int64_t npaths, const int64_t *ploc, const int64_t *eloc, int64_t at) {
				hipLaunchKernelGGL(k_asp_unrank, dim3((unsigned)std::min<int64_t>(npaths, 1 << 20)), dim3(64), 0, st, lo, m, npaths, skey, sdst, (u32)base,
				                   ws->usrc.as<int32_t>(), c->off, c->adj, c->edge_ids, c->roff, c->radj, H, sigma, ploc, eloc, at, ws->tight_stage.as<int64_t>(),
				                   ws->soff.as<int64_t>(), tc);
			}));
		} else {
			KernelTimer kt(st, K_RECON);
			if (m > 0) plan(nullptr, nullptr);
			kt.stop();
		}
		// (between the unranking launch and the wait for its error flag)
		hipLaunchKernelGGL(k_asp_reset, dim3(cus * 4), dim3(256), 0, st, touched, tc, H, ws->tight_mask[0].as<u64>(), ws->tight_mask[1].as<u64>());
		if (!out.lists) return PGQ_OK;
		PGQ_TRY(stage.read_back(&h, tc, sizeof(h)));
		return unrank_status(h.error);
	}
};

} // namespace pgq

using namespace pgq;

extern "C" {

static int asp_check_bounds(int64_t max_hops, const int64_t *max_paths) {
	if (max_hops < 0) return fail(PGQ_ERR_INVALID_ARG, "max_hops must not be negative");
	if (max_paths && *max_paths < 1) return fail(PGQ_ERR_INVALID_ARG, "max_paths must be at least 1");
	return PGQ_OK;
}

int pgq_shortestpath_count_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t max_hops, int64_t *d_out_count) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	auto check = [&]() -> int {
		PGQ_TRY(check_arrays(csr, n, d_src && d_dst && d_out_count, "NULL device array"));
		return asp_check_bounds(max_hops, nullptr);
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		ListOut out;
		out.d_count = d_out_count;
		return AspCall(csr, ws, n, d_src, d_dst, max_hops, out).run();
	});
}

int pgq_all_shortestpaths_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t max_hops, int64_t max_paths,
                                      int64_t *d_out_len, int64_t *d_out_count, int64_t *d_out_first, int64_t *d_out_npaths, int64_t *d_path_offset,
                                      int64_t path_cap, int64_t *d_child, int64_t child_cap, int64_t *paths_used, int64_t *child_used) {
	if (paths_used) *paths_used = 0;
	if (child_used) *child_used = 0;
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	auto check = [&]() -> int {
		PGQ_TRY(check_arrays(csr, n, d_src && d_dst && d_out_len && d_out_count && d_out_first && d_out_npaths && d_path_offset && d_child, "NULL device array"));
		if (path_cap < 0 || child_cap < 0) return fail(PGQ_ERR_INVALID_ARG, "negative capacity");
		return asp_check_bounds(max_hops, &max_paths);
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		ListOut out;
		out.d_len = d_out_len, out.d_count = d_out_count, out.d_first = d_out_first, out.d_np = d_out_npaths;
		out.d_path_off = d_path_offset, out.path_cap = path_cap, out.d_child = d_child, out.child_cap = child_cap;
		return list_bulk_body(out, max_paths, [&](ListOut &o) { return AspCall(csr, ws, n, d_src, d_dst, max_hops, o).run(); }, paths_used, child_used);
	});
}

int pgq_shortestpath_count(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops, int64_t *out_count, uint64_t *out_valid) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	auto check = [&] { return count_chunk_check(csr, V, n, out_count, out_valid, [&] { return asp_check_bounds(max_hops, nullptr); }); };
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		auto run = [&](ListOut &o, const int64_t *d_src, const int64_t *d_dst) { return AspCall(csr, ws, n, d_src, d_dst, max_hops, o).run(); };
		return count_chunk_body(ws, V, n, src, dst, run, out_count, out_valid);
	});
}

int pgq_all_shortestpaths(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops, int64_t max_paths, uint64_t *out_first,
                          uint64_t *out_npaths, uint64_t *out_valid, const uint64_t **out_path_offset, const uint64_t **out_path_length,
                          uint64_t *out_path_total, const int64_t **out_child, uint64_t *out_child_len) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	const ListChunkOut o { out_first, out_npaths, out_valid, out_path_offset, out_path_length, out_path_total, out_child, out_child_len };
	auto check = [&] { return list_chunk_check(csr, V, n, o, [&] { return asp_check_bounds(max_hops, &max_paths); }); };
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		auto run = [&](ListOut &lo, const int64_t *d_src, const int64_t *d_dst) { return AspCall(csr, ws, n, d_src, d_dst, max_hops, lo).run(); };
		return list_chunk_body(ws, V, n, src, dst, max_paths, run, o);
	});
}

} // extern "C"
