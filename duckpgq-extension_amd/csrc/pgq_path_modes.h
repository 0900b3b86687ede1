// pgq_path_modes.h — SHORTEST k under the path modes TRAIL, ACYCLIC and SIMPLE: the search kernel of pgq_k_shortest_walks_mode and
// pgq_walk_count_mode.  Part of pgq_k_walks.o: included into pgq_k_walks.hip behind the walk rounds (WalkRound, walk_w, WalkCounters;
// unrank_slot is pgq_path_lists.h's), not compiled on its own.  The reference's binder rejects every mode but WALK ("Path modes other than WALK have not been implemented yet",
// match.cpp:80-108) and at the same place tells its users to pick one when ALL over a cyclic graph explodes (match.cpp:100-104).
//
// The contract, for a row (src, dst), lo = min_hops, K = max_hops.  S = every walk of lo..K edges in k_shortest_walks' order (by
// length, then by in-list positions read from the destination end).  A walk [x_0, e_1, x_1, ..., e_t, x_t] is admitted when
//   ACYCLIC   no two of x_0 .. x_t are equal (src == dst: the empty walk alone)
//   SIMPLE    no two of x_0 .. x_t are equal, except that x_0 == x_t is allowed (a self-loop, a ring back to its start)
//   TRAIL     no two of e_1 .. e_t are equal, compared as the list's elements: edge_ids[slot], or the slot without edge ids
// and the row's list is the first min(a, k) ADMITTED walks of S (a = their number), not the admitted ones among S's first k.
//
// A rank cannot be unranked under a mode — counting simple paths has no table recurrence — so the rows are searched: one wavefront
// per row of the lane batch, depth-first from x_t = dst for t = lo .. R (R the last round run) with W_t[dst] > 0.  At depth i the
// wavefront reads x_i's in-list from the depth's cursor, 64 positions per trip; a position is live when W_{i-1}[u] > 0 for its
// parent u (the walk tables prune: u can still reach the source in exactly i - 1 edges) and the mode admits it:
//   vertex modes   u is not on the stack x_i .. x_t — a loop over the depth, all 64 candidates tested at once — and is not the
//                  source unless i - 1 == 0 (W_0 makes it the source there); SIMPLE leaves x_t out of the test when i - 1 == 0.
//   TRAIL          the edge of the first live position is looked up before it is taken (unrank_slot: the m-th in-slot from u into
//                  x_i is the m-th slot of u's out-list into x_i); if its id is among e_{i+1} .. e_t the cursor moves on by one.
// A ballot and find-first-set take the first live position; the cursor stays behind it, so that backtracking resumes there.
// Reaching depth 0 is an admitted walk.  The stack (x_0 .. x_64, 64 cursors, 64 edge ids) is in LDS; every lane stores the same
// value, so each lane reads back what it wrote itself.  Every loop is bounded by the depth, a list's length or the step cap: a
// STEP is one 64-position trip or one descent, and a row that takes more than `step_cap` of them in a pass raises error bit 16 (the
// call fails with PGQ_ERR_UNSUPPORTED, nothing written) — finding a simple path of an exact length is NP-hard.
//
// Two passes over one device function: EMIT = false counts (r_np / r_el / r_len / r_count and the count arrays of ListCall::emit's
// plan step, stopping a row at k), EMIT = true repeats the search and writes each admitted walk into the row's staged block in
// k_walk_unrank's layout, [hops of each walk][elements], for k_walk_gather.  pgq_walk_count_mode runs the first pass only.
// When a row has enough is pgq_walk_rule.h's rule, fed one admitted walk at a time: a length is a group once it yields an admitted
// walk, and a length that completes the last group is searched to its end or to B + 1 walks.  For pgq_k_shortest_groups B = P, so
// that r_count = min(|A|, P + 1); WalkPlan keeps the first P (r_np, r_el, the count arrays; r_ng = the lengths among them) for
// the emitting pass, which looks for exactly those.
// Not built: a smarter prune than W (a vertex that W admits may only be reachable through the stack), several wavefronts per row.

namespace pgq {

constexpr u32 kModeOverCap = 16u; // WalkCounters::error: a row's search went over the step cap

__device__ __forceinline__ bool mode_is_vertex(int mode) { return mode == PGQ_MODE_SIMPLE || mode == PGQ_MODE_ACYCLIC; }

template <bool EMIT>
__global__ __launch_bounds__(64) void k_mode_search(int64_t lo, int64_t m, const u32 *__restrict__ skey, const u32 *__restrict__ sidx,
                                                   const int32_t *__restrict__ sdst, u32 base_lane, const int32_t *__restrict__ usrc,
                                                   const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                   const int64_t *__restrict__ edge_ids, const int64_t *__restrict__ roff,
                                                   const int32_t *__restrict__ radj, const WalkRound *__restrict__ tabs, WalkQuery q, int rounds,
                                                   int64_t step_cap, int64_t *__restrict__ r_len,
                                                   int64_t *__restrict__ r_count, int64_t *__restrict__ r_np, int64_t *__restrict__ r_el,
                                                   int64_t *__restrict__ r_ng, int64_t *__restrict__ cntp,
                                                   int64_t *__restrict__ cnte, const int64_t *__restrict__ ploc, const int64_t *__restrict__ eloc,
                                                   int64_t stage_base, int64_t *__restrict__ stage, int64_t *__restrict__ soff,
                                                   WalkCounters *__restrict__ tc) {
	__shared__ int sx[PGQ_WALK_MAX_HOPS + 1];     // x_0 .. x_t
	__shared__ u32 scur[PGQ_WALK_MAX_HOPS + 1];   // depth i: the next position of x_i's in-list
	__shared__ int64_t se[PGQ_WALK_MAX_HOPS + 1]; // e_1 .. e_t
	const int lane = threadIdx.x;
	const int mode = q.mode;
	const bool vertex_mode = mode_is_vertex(mode), trail = mode == PGQ_MODE_TRAIL;
	for (int64_t a = blockIdx.x; a < m; a += gridDim.x) {
		const int64_t row_i = lo + a;
		const u32 l = skey[row_i] - base_lane;
		const int dst = sdst[row_i], src = usrc[base_lane + l];
		// The row is fed its admitted walks one by one (pgq_walk_rule.h): found.count walks, found.groups lengths with one.  The
		// counting pass looks for B + 1 of them — k, or one past max_paths — and plans the first q.limit; the emitting pass for the
		// `want` walks that were planned.
		const int64_t want = EMIT ? ploc[a + 1] - ploc[a] : q.rule().bound + 1;
		const WalkRule rule { q.rule().groups, want - 1 };
		const int64_t rowbase = EMIT ? stage_base + eloc[a] : 0;      // the row's staged block ...
		const int64_t room = EMIT ? eloc[a + 1] - eloc[a] - want : 0; // ... and the elements it holds behind the hops
		const int64_t keep = EMIT ? want : q.limit;
		WalkRow found;
		WalkPlan plan;
		int64_t steps = 0, first = -1;
		u32 error = 0;
		for (int64_t t64 = q.min_hops; t64 <= rounds && found.open(rule) && !error; t64++) {
			const int t = (int)t64;
			if (walk_w(tabs[t], dst, l) <= 0) continue;
			bool fresh = true; // the length has yielded no admitted walk yet
			int i = t;
			sx[t] = dst;
			scur[t] = 0;
			// depth i > 0: look for the next parent of x_i; depth 0: an admitted walk, then on at depth 1
			while (i <= t && found.count < want && !error) { // (a length that counts as the last group is searched to its end)
				if (i == 0) {
					if (t > 0 && sx[0] != src) { // (W_0 admits the source alone)
						error = 8u;
						break;
					}
					if (EMIT) {
						if (plan.el + 2 * t + 1 > room) { // (the counting pass found less)
							error = 2u;
							break;
						}
						int64_t *out = stage + rowbase + want + plan.el;
						if (lane == 0) stage[rowbase + found.count] = t;
						for (int j = lane; j <= t; j += 64) {
							out[2 * j] = j == 0 ? src : sx[j];
							if (j > 0) out[2 * j - 1] = se[j];
						}
					}
					if (first < 0) first = t;
					plan.take(found, keep, t, 1, fresh);
					found.add(1, fresh);
					fresh = false;
					i = 1; // (t == 0: past the loop)
					continue;
				}
				const int x = sx[i];
				const int64_t rb = roff[x], len = roff[x + 1] - rb;
				const WalkRound pr = tabs[i - 1];
				const int top = mode == PGQ_MODE_SIMPLE && i == 1 ? t - 1 : t; // the stack entries a candidate is tested against
				int64_t cur = scur[i], pos = -1;
				int u = -1;
				while (cur < len) {
					if (++steps > step_cap) {
						error = kModeOverCap;
						break;
					}
					const int64_t j = cur + lane;
					const int cand = j < len ? radj[rb + j] : -1;
					bool live = cand >= 0 && walk_w(pr, cand, l) > 0;
					if (vertex_mode && live) {
						if (i > 1 && cand == src) live = false;
						for (int d = i; d <= top; d++) live = live && sx[d] != cand;
					}
					const u64 bm = __ballot(live);
					if (bm) {
						const int p = __ffsll((long long)bm) - 1;
						pos = cur + p;
						u = __shfl(cand, p);
						break;
					}
					cur += 64;
				}
				if (error) break;
				if (pos < 0) { // the list is used up: back to the depth above, behind its cursor
					i++;
					continue;
				}
				scur[i] = (u32)(pos + 1);
				int64_t eid = 0;
				if (EMIT || trail) {
					const int64_t slot = unrank_slot(x, u, rb + pos, lane, rb, radj, off, adj);
					if (slot < 0) {
						error = 4u;
						break;
					}
					eid = edge_ids ? edge_ids[slot] : slot;
					if (trail) {
						bool used = false;
						for (int d = i + 1; d <= t; d++) used = used || se[d] == eid;
						if (used) continue; // (the cursor stands one behind it)
					}
				}
				if (++steps > step_cap) {
					error = kModeOverCap;
					break;
				}
				se[i] = eid;
				sx[i - 1] = u;
				i--;
				if (i > 0) scur[i] = 0;
			}
		}
		if (lane == 0) {
			if (!EMIT) {
				const u32 row = sidx[row_i];
				r_len[row] = first;
				const int64_t np = WalkPlan::np(found, keep);
				r_count[row] = found.count;
				r_np[row] = np;
				r_el[row] = plan.el;
				if (r_ng) r_ng[row] = plan.ngroups;
				if (cntp) {
					cntp[a] = np;
					cnte[a] = np > 0 ? np + plan.el : 0;
				}
			} else if (found.count > 0) {
				soff[row_i] = rowbase;
			}
			if (error) atomicOr(&tc->error, error);
			atomicAdd((unsigned long long *)&tc->steps, (unsigned long long)steps);
			atomicMax((unsigned long long *)&tc->row_max, (unsigned long long)steps);
		}
	}
}

} // namespace pgq
