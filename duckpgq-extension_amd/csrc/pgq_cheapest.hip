// pgq_cheapest.hip — cheapest_path_length on MI355X: batched, frontier-driven label-correcting SSSP.
//
// Replaces TemplatedBatchBellmanFord / TemplatedBellmanFord / CheapestPathLengthFunction
// (src/core/functions/scalar/cheapest_path_length.cpp:52-89, :91-136, :138-163).
//
// The reference sweeps every vertex x every out-edge x every lane until nothing changes, relaxing with
//     new = dist[v] + w;  if (new < dist[n]) dist[n] = new            (cheapest_path_length.cpp:29-36)
// For non-negative weights that relaxation is monotone (IEEE + is monotone in its left operand for a fixed
// non-negative right operand), so the fixpoint does not depend on the order of relaxations: the result is the
// minimum over paths of the left-to-right fold of the weights, bit for bit, for int64 and for double.  We
// therefore only relax out of vertices whose distance improved in the previous round (delta = "changed since
// last round" frontier), with atomicMin on the 64-bit pattern (non-negative doubles order like their bits).
// Negative weights are rejected (PGQ_ERR_UNSUPPORTED): the reference does not terminate on negative cycles
// and its max/2 sentinel leaks for unreachable lanes.
//
// Layout: dist[V][LC] (vertex-major, LC = 64 lanes -> one 512-byte row per vertex, fully coalesced per wave),
// dirty[parity][V] = 64-bit mask of lanes of v that improved in the previous round.  A lane is one distinct
// source.  Rounds are kernel launches: improvements made in round r are consumed in round r+1, so no
// intra-kernel visibility between XCDs is needed.
//
// pgq_cheapest_path_length_within (the cheapest walk of at most K edges: another number, not this one clamped) cannot use these
// rounds, in which a label travels several edges per launch; its round of exactly one edge is k_hop_snapshot + k_relax_hops
// under HopBatches, further down.
//
// This file is pgq_cheapest.o, alone.  What cheapest_path and cheapest_path_within (pgq_cheapest_path.o) take from it is declared in
// pgq_relax.h and defined here: LC, Inf, RelaxCounters, the hooks SettledBatch and HopLog, the handle's weight tables
// (ensure_reverse_weights, ensure_weight_mean), check_weighted, fill32, and the two functions that run the lane batches with a hook
// (settle_every_label, hop_rounds_logged, at the end of namespace pgq).  Everything else here is this file's own.
#include <hipcub/hipcub.hpp>

#include <cstddef>
#include <mutex>
#include <limits>
#include <type_traits>

#include "pgq_relax.h"
#include <chrono>
#include <thread>
#include <vector>
#include <string>

namespace pgq {

// Label STORAGE of the batched relaxation (round 5): int64 weights whose largest possible path sum fits 31 bits
// (w_max x V < 2^31 - 1: weights 1..999 on the 448 K-vertex knows graph are at 4.5 x 10^8) keep their labels as int32 —
// a label row is 256 bytes instead of 512, and the rows are what the relaxation moves (2 rows per relaxed edge).  All
// arithmetic and every comparison stay in the 64-bit domain of the reference (cheapest_path_length.cpp:29-36): a stored
// label is widened on load, "unlabelled" (0x7FFFFFFF) to the reference's max / 2 sentinel, and a candidate is only
// narrowed when it is stored, where the precondition makes it exact.  Doubles and wider int64 ranges keep 8-byte labels.
template <typename DT> struct Lab;
template <> struct Lab<int64_t> {
	static constexpr int64_t unlabelled(int64_t inf_bits) { return inf_bits; }
	static __device__ __forceinline__ int64_t widen(int64_t v, int64_t) { return v; }
	static __device__ __forceinline__ int64_t min_into(int64_t *p, int64_t cand, int64_t) {
		return (int64_t)atomicMin((long long *)p, (long long)cand);
	}
};
template <> struct Lab<int32_t> {
	static constexpr int32_t kUnlabelled = 0x7FFFFFFF;
	static constexpr int32_t unlabelled(int64_t) { return kUnlabelled; }
	static __device__ __forceinline__ int64_t widen(int32_t v, int64_t inf_bits) { return v == kUnlabelled ? inf_bits : (int64_t)v; }
	static __device__ __forceinline__ int64_t min_into(int32_t *p, int64_t cand, int64_t inf_bits) {
		return widen(atomicMin(p, (int32_t)cand), inf_bits);
	}
};
__global__ void k_fill32(int32_t *__restrict__ p, int64_t n, int32_t value) {
	int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (; i < n; i += stride) p[i] = value;
}
void fill32(int32_t *p, int64_t n, int32_t value, hipStream_t st) {
	hipLaunchKernelGGL(k_fill32, dim3((unsigned)device_cus() * 8), dim3(256), 0, st, p, n, value);
}
__global__ void k_fill64(int64_t *__restrict__ p, int64_t n, int64_t value) {
	int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (; i < n; i += stride) p[i] = value;
}

// sources of the batch: dist[src][lane] = 0, dirty, queued
template <typename DT>
__global__ void k_cheapest_init(const int32_t *__restrict__ usrc, int64_t U, int64_t base, DT *__restrict__ dist,
                                u64 *__restrict__ dirty, u32 *__restrict__ tflag, u32 tepoch,
                                int32_t *__restrict__ touched, u32 *__restrict__ qcount, u32 *__restrict__ tcount,
                                int32_t *__restrict__ q) {
	int64_t g = base + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= U || g >= base + LC) return;
	const int v = usrc[g];
	const int l = (int)(g - base);
	dist[(size_t)v * LC + l] = 0;
	atomicOr(&dirty[v], 1ull << l);
	q[atomicAdd(qcount, 1u)] = v; // distinct sources -> distinct vertices
	tflag[v] = tepoch;
	touched[atomicAdd(tcount, 1u)] = v;
}

// ---------------------------------------------------------------------------------------------------------------
// One round of the batched relaxation: one wavefront per changed vertex v, lane l = search l.  Every lane relaxes its
// own label over v's out-edges: coalesced 512-byte rows of dist[n][*].  Two things keep it from being a plain Jacobi
// sweep:
//  * ORDER (optional, relax_delta_div): only labels below `thr` are expanded this round, the others stay dirty.
//  * BOUND: a lane never expands a vertex whose label already reaches the largest tentative label among the lane's own
//    destinations (`bound`, refreshed every round): with non-negative weights nothing beyond can improve an answer.
// Neither changes the fixpoint at the destinations (every vertex on a cheaper path has a smaller label than the bound
// and is expanded after its last improvement), nor the left-to-right fold of the reference (cheapest_path_length.cpp:29-36),
// so int64 and double results stay bit-identical.  Labels are compared as their (non-negative) bit patterns.
//
// What a round costs is the number of DEPENDENT memory round trips a wavefront makes per vertex (the per-round trace of
// the weighted knows graph: ~420 K changed vertices with 4-6 useful edges each, for a dozen rounds), so the kernel is
// written to keep that chain short:
//  * the edges are handled eight at a time: adjacency+weights, then the eight label rows, then the eight atomicMin,
//    then — lanes 0..7, one improved neighbour each — the returning atomicOr on the neighbour's dirty word, whose old
//    value 0 says "first to dirty it this round: append it" (no separate queue flag), and the first-touch flag;
//  * appends to the next queue / the touched list are collected per wavefront in LDS and written 64 at a time (one
//    atomicAdd per VERTEX on the list counters serialised at ~12 ns each: 5 ms per round);
//  * the header of the wavefront's next vertex (dirty word, label row, list bounds) is requested before the current
//    vertex's edges are walked, the vertex after that is read from the queue.
// ---------------------------------------------------------------------------------------------------------------
// Compile-time variants of k_relax for tuning sweeps (tools/build_variants.sh, selected with PGQ_HIP_LIB); the defaults
// are what ships.
//   PGQ_RELAX_UNROLL   edges per dependent trip
//   PGQ_RELAX_WAVES    wavefronts per SIMD asked of the register allocator
//   PGQ_RELAX_NVFIRST  1: decide which of the trip's edges count before their label rows are requested (fewer rows, one
//                      more dependent step) — measured together with SEGCOND once: 117 -> 130 ms per 512 pairs
//   PGQ_RELAX_SEGCOND  1: a lane that cannot improve an edge's label reads v's first word instead of its own word of the
//                      row (tools/relax_model.py: 4.3 of a row's 8 segments hold a lane that still can)
#ifndef PGQ_RELAX_UNROLL
#define PGQ_RELAX_UNROLL 8
#endif
#ifndef PGQ_RELAX_WAVES
#define PGQ_RELAX_WAVES 6
#endif
#ifndef PGQ_RELAX_NVFIRST
#define PGQ_RELAX_NVFIRST 0
#endif
#ifndef PGQ_RELAX_SEGCOND
#define PGQ_RELAX_SEGCOND 0
#endif
static constexpr int kRelaxUnroll = PGQ_RELAX_UNROLL;
static constexpr int kPendCap = 64 + kRelaxUnroll;

// wave-level buffered append: lanes with `fresh` add n to the wavefront's pending list (LDS), 64 entries go out at once
__device__ __forceinline__ void relax_append(int *s_buf, int &pend, bool fresh, int n, int32_t *__restrict__ list,
                                             u32 *__restrict__ counter, int lane) {
	const u64 fm = __ballot(fresh);
	if (!fm) return;
	if (fresh) s_buf[pend + __popcll(fm & ((1ull << lane) - 1ull))] = n;
	pend += __popcll(fm);
	__builtin_amdgcn_wave_barrier();
	if (pend >= 64) {
		u32 base = 0;
		if (lane == 0) base = atomicAdd(counter, 64u);
		base = (u32)__builtin_amdgcn_readfirstlane((int)base);
		list[base + lane] = s_buf[lane];
		const int rest = pend - 64; // < kRelaxUnroll
		const int r = lane < rest ? s_buf[64 + lane] : 0;
		__builtin_amdgcn_wave_barrier();
		if (lane < rest) s_buf[lane] = r;
		pend = rest;
		__builtin_amdgcn_wave_barrier();
	}
}

template <typename T, typename DT>
__global__ __launch_bounds__(256, PGQ_RELAX_WAVES) void k_relax(const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                               const T *__restrict__ w, DT *__restrict__ dist,
                                               u64 *__restrict__ dirty_cur, u64 *__restrict__ dirty_nxt,
                                               const int32_t *__restrict__ qcur, const u32 *__restrict__ nq_ptr,
                                               int32_t *__restrict__ qnxt, u32 *__restrict__ nq_nxt,
                                               u32 *__restrict__ tflag, u32 tepoch, int32_t *__restrict__ touched,
                                               u32 *__restrict__ tcount, u64 *__restrict__ relaxed_edges, long long thr,
                                               const long long *__restrict__ bound, long long *__restrict__ min_deferred,
                                               u32 *__restrict__ relaxed_vertices, int sorted, T wcap,
                                               int heavy_pass, u64 *__restrict__ heavy_ctr, int32_t *__restrict__ hv,
                                               u64 *__restrict__ hmask, u32 *__restrict__ hstart, u32 *__restrict__ hmap,
                                               const DT *__restrict__ other, long long *__restrict__ mu,
                                               u32 *__restrict__ alive, const long long *__restrict__ thr_ptr) {
	// `other` != nullptr: one side of the bidirectional search (BidirBatches).  Lane l is one (src, dst) PAIR, `dist` this
	// side's labels and `other` the other side's; `bound` is the pair's best known src -> dst length mu[l] (both sides prune
	// with it), `*thr_ptr` the distance cap both sides expand under.  A vertex expanded here that carries a label of the other
	// side closes a path: mu[l] = min(mu[l], label + other label).  alive[l] = 1: the lane left a labelled vertex unexpanded
	// (over the cap) this round — a side without one has exhausted its closure.
	// Long lists are not walked by the wavefront that finds them (a round would take as long as its longest list: one
	// hub of 1 800 edges = 230 dependent trips).  Pass 0 (heavy_pass = 0) appends such a vertex to the heavy list — one
	// packed 64-bit atomicAdd hands out its entry index and the first of its chunk numbers together — and writes
	// hmap[chunk] = entry; pass 1 (a second launch, items = chunks) walks kHeavyChunk edges per wavefront.  Over
	// weight-sorted lists only the prefix under the cap counts: a list is heavy if its 129th edge is still under it.
	constexpr int64_t kHeavyMin = 128;
	constexpr int64_t kHeavyChunk = 64;
	constexpr int UNR = kRelaxUnroll;
	__shared__ int s_pq[4][kPendCap];
	__shared__ int s_pt[4][kPendCap];
	// what the workgroup hands to the round's counters goes through LDS first: ~5 atomics per WAVEFRONT on one cache
	// line (two list tails, three statistics) were 25 K serialised L2 operations per launch — ~150 us, the whole
	// time of a round with few changed vertices
	__shared__ u64 s_edges;
	__shared__ u32 s_expanded;
	__shared__ long long s_min_def;
	__shared__ int s_pend[2][4];
	__shared__ u32 s_base[2];
	if (threadIdx.x == 0) {
		s_edges = 0;
		s_expanded = 0;
		s_min_def = 0x7FFFFFFFFFFFFFFFll;
	}
	__syncthreads();
	const int lane = threadIdx.x & 63;
	const int wib = threadIdx.x >> 6;
	const u32 wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
	const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
	const u32 nq = heavy_pass ? (u32)(*heavy_ctr & 0xFFFFFFFFull) : *nq_ptr;
	long long my_bound = bound[lane];
	const long long mu_b = my_bound; // (bidirectional) the pair's bound proper
	if (thr_ptr) {
		thr = *thr_ptr;
		// nothing is labelled at or above twice the cap: a pair that needs such a label is not finished in this phase anyway
		// (exactness: BidirBatches), and an expansion walks the few edges under 2 C - label instead of its whole list
		if (other) my_bound = min(my_bound, 2 * thr);
	}
	long long my_mu = 0x7FFFFFFFFFFFFFFFll; // (bidirectional) smallest label + other side's label this wavefront's lane has seen
	bool my_alive = false;
	u64 edges = 0;
	u32 expanded = 0;
	long long min_def = 0x7FFFFFFFFFFFFFFFll;
	int pend_q = 0, pend_t = 0; // wave-uniform
	int *const pq = s_pq[wib];
	int *const pt = s_pt[wib];

	// relax the edges [b, e) of v (label row dvb, lanes `mine`)
	auto walk = [&](int v, int64_t dvb, bool mine, int64_t b, int64_t e) {
		if (!sorted) edges += (u64)(e - b);
		bool stop = false;
		for (int64_t k0 = b; k0 < e && !stop; k0 += UNR) {
			int nn[UNR];
			T ww[UNR];
			int64_t cand[UNR], curv[UNR];
#pragma unroll
			for (int u = 0; u < UNR; u++) {
				const bool in = k0 + u < e;
				nn[u] = in ? adj[k0 + u] : v;
				ww[u] = in ? w[k0 + u] : T(0);
				// labels are compared as bit patterns: a NaN sum with the sign bit set would look like an improvement.  A NaN
				// weight never relaxes an edge in the reference (`dist + w < dist[n]` is false): +inf behaves the same here
				if constexpr (std::is_same<T, double>::value) ww[u] = ww[u] == ww[u] ? ww[u] : __longlong_as_double(0x7FF0000000000000ll);
			}
#pragma unroll
			for (int u = 0; u < UNR; u++) {
				if constexpr (std::is_same<T, double>::value) cand[u] = __double_as_longlong(__longlong_as_double(dvb) + ww[u]);
				else cand[u] = dvb + (int64_t)ww[u];
#if !PGQ_RELAX_NVFIRST
#if PGQ_RELAX_SEGCOND
				curv[u] = Lab<DT>::widen(dist[mine && (!sorted || cand[u] < my_bound) ? (size_t)nn[u] * LC + lane : (size_t)v * LC], Inf<T>::bits);
#else
				curv[u] = Lab<DT>::widen(dist[(size_t)nn[u] * LC + lane], Inf<T>::bits); // unconditional: all eight rows are in flight together
#endif
#endif
			}
			// how many of the eight count: up to the end of the list, the cap of the phase, or the first edge no lane's
			// candidate gets under its bound with (the list ascends by weight: no later one can either)
			int nv = 0;
#pragma unroll
			for (int u = 0; u < UNR; u++) {
				if (stop || k0 + u >= e) break;
				if (sorted && (ww[u] > wcap || !__any(mine && cand[u] < my_bound))) {
					stop = true;
					break;
				}
				nv++;
			}
#if PGQ_RELAX_NVFIRST
			if (nv == 0) break;
#pragma unroll
			for (int u = 0; u < UNR; u++) { // past nv (and, with SEGCOND, in lanes that cannot improve): v's first word, a cached segment
#if PGQ_RELAX_SEGCOND
				const bool need = u < nv && mine && (!sorted || cand[u] < my_bound);
#else
				const bool need = u < nv;
#endif
				curv[u] = Lab<DT>::widen(dist[need ? (size_t)nn[u] * LC + lane : (size_t)v * LC], Inf<T>::bits);
			}
#endif
			if (sorted) edges += (u64)nv;
			if (other) { // an edge the cap cut (not the pair's bound): the lane's side is not exhausted, and the next cap must reach it
#pragma unroll
				for (int u = 0; u < UNR; u++) {
					if (k0 + u < e && mine && cand[u] >= my_bound && cand[u] < mu_b) {
						my_alive = true;
						min_def = min(min_def, (long long)(cand[u] >> 1));
					}
				}
			}
#pragma unroll
			for (int u = 0; u < UNR; u++) {
				const bool go = u < nv && mine && (!sorted || cand[u] < my_bound) && cand[u] < curv[u];
				curv[u] = cand[u]; // "not improved" unless the atomic says otherwise
				if (go) curv[u] = Lab<DT>::min_into(&dist[(size_t)nn[u] * LC + lane], cand[u], Inf<T>::bits);
			}
			u64 my_im = 0;
			int my_n = 0;
#pragma unroll
			for (int u = 0; u < UNR; u++) {
				const u64 im = __ballot(cand[u] < curv[u]);
				if (lane == u) {
					my_im = im;
					my_n = nn[u];
				}
			}
			if (!__any(my_im != 0)) continue;
			bool fresh_q = false, fresh_t = false;
			if (my_im) { // lanes 0..7, one improved neighbour each
				fresh_q = atomicOr(&dirty_nxt[my_n], my_im) == 0ull;
				fresh_t = tflag[my_n] != tepoch && atomicExch(&tflag[my_n], tepoch) != tepoch;
			}
			relax_append(pq, pend_q, fresh_q, my_n, qnxt, nq_nxt, lane);
			relax_append(pt, pend_t, fresh_t, my_n, touched, tcount, lane);
		}
	};

	if (heavy_pass) {
		for (u32 i = wave; i < nq; i += nwaves) {
			const u32 ent = hmap[i];
			const int v = hv[ent];
			const int64_t b = off[v] + (int64_t)(i - hstart[ent]) * kHeavyChunk;
			const int64_t e = min(b + kHeavyChunk, off[v + 1]);
			if (sorted && w[b] > wcap) continue; // the whole chunk lies above this phase's cap
			// the label may have improved since pass 0 queued v: any label is the length of a real path, the smaller the better
			const int64_t dvb = Lab<DT>::widen(dist[(size_t)v * LC + lane], Inf<T>::bits);
			walk(v, dvb, (hmask[ent] >> lane) & 1ull, b, e);
		}
	} else {
		// software pipeline over the wavefront's vertices: queue entry two ahead, header one ahead
		u32 i = wave, i1 = wave + nwaves, i2 = wave + 2 * nwaves;
		int v = i < nq ? qcur[i] : 0;
		int v1 = i1 < nq ? qcur[i1] : 0;
		u64 mask = 0;
		int64_t dvb = 0, b = 0, e = 0, ob = Inf<T>::bits;
		if (i < nq) {
			mask = dirty_cur[v];
			dvb = Lab<DT>::widen(dist[(size_t)v * LC + lane], Inf<T>::bits);
			if (other) ob = Lab<DT>::widen(other[(size_t)v * LC + lane], Inf<T>::bits);
			b = off[v];
			e = off[v + 1];
		}
		while (i < nq) {
			u64 mask1 = 0;
			int64_t dvb1 = 0, b1 = 0, e1 = 0, ob1 = Inf<T>::bits;
			if (i1 < nq) {
				mask1 = dirty_cur[v1];
				dvb1 = Lab<DT>::widen(dist[(size_t)v1 * LC + lane], Inf<T>::bits);
				if (other) ob1 = Lab<DT>::widen(other[(size_t)v1 * LC + lane], Inf<T>::bits);
				b1 = off[v1];
				e1 = off[v1 + 1];
			}
			const int v2 = i2 < nq ? qcur[i2] : 0;
			if (lane == 0) dirty_cur[v] = 0; // consumed; nobody else touches dirty_cur this round
			const bool live = ((mask >> lane) & 1ull) && dvb < my_bound;
			const bool mine = live && dvb < thr;
			if (other && mine && ob != Inf<T>::bits) my_mu = min(my_mu, (long long)(dvb + ob)); // (int64 weights only: exact in any order)
			const u64 deferred = __ballot(live && !mine);
			if (deferred) { // stays dirty for a later round
				my_alive |= live && !mine;
				if (live && !mine) min_def = min(min_def, (long long)dvb);
				bool fresh = false;
				if (lane == 0) fresh = atomicOr(&dirty_nxt[v], deferred) == 0ull;
				relax_append(pq, pend_q, fresh, v, qnxt, nq_nxt, lane);
			}
			const u64 mine_mask = __ballot(mine);
			if (mine_mask) {
				expanded++;
				bool is_heavy = false;
				if (heavy_ctr && e - b > kHeavyMin) is_heavy = !sorted || !(w[b + kHeavyMin] > wcap);
				if (is_heavy && other && sorted) { // no cap on the edge weight here: heavy only if the 129th edge can still get a lane under its bound
					if constexpr (!std::is_same<T, double>::value) is_heavy = __any(mine && dvb + (int64_t)w[b + kHeavyMin] < my_bound);
				}
				if (is_heavy) {
					const u32 nch = (u32)((e - b + kHeavyChunk - 1) / kHeavyChunk);
					u64 t = 0;
					if (lane == 0) t = atomicAdd(heavy_ctr, (1ull << 32) | (u64)nch);
					const u32 cs = (u32)__builtin_amdgcn_readfirstlane((int)(u32)t);
					const u32 ent = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(t >> 32));
					if (lane == 0) {
						hv[ent] = v;
						hmask[ent] = mine_mask;
						hstart[ent] = cs;
					}
					for (u32 c = lane; c < nch; c += 64) hmap[cs + c] = ent;
				} else {
					walk(v, dvb, mine, b, e);
				}
			}
			i = i1;
			i1 = i2;
			i2 += nwaves;
			v = v1;
			v1 = v2;
			mask = mask1;
			dvb = dvb1;
			ob = ob1;
			b = b1;
			e = e1;
		}
	}
	if (other) { // (wave-uniform)
		if (my_alive) alive[lane] = 1u; // plain stores of one value: no ordering needed
		if (my_mu < mu_b) atomicMin(&mu[lane], my_mu); // rare: a lane's bound improves a handful of times per search
	}
	for (int o = 32; o > 0; o >>= 1) min_def = min(min_def, (long long)__shfl_xor(min_def, o));
	if (lane == 0) {
		if (edges) atomicAdd(&s_edges, edges);
		if (expanded) atomicAdd(&s_expanded, expanded);
		if (min_def != 0x7FFFFFFFFFFFFFFFll) atomicMin(&s_min_def, min_def);
		s_pend[0][wib] = pend_q;
		s_pend[1][wib] = pend_t;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		const u32 tq = (u32)(s_pend[0][0] + s_pend[0][1] + s_pend[0][2] + s_pend[0][3]);
		const u32 tt = (u32)(s_pend[1][0] + s_pend[1][1] + s_pend[1][2] + s_pend[1][3]);
		s_base[0] = tq ? atomicAdd(nq_nxt, tq) : 0u;
		s_base[1] = tt ? atomicAdd(tcount, tt) : 0u;
		if (s_edges) atomicAdd(relaxed_edges, s_edges);
		if (s_expanded) atomicAdd(relaxed_vertices, s_expanded);
		if (s_min_def != 0x7FFFFFFFFFFFFFFFll) atomicMin(min_deferred, s_min_def);
	}
	__syncthreads();
	u32 oq = s_base[0], ot = s_base[1];
	for (int k = 0; k < wib; k++) {
		oq += (u32)s_pend[0][k];
		ot += (u32)s_pend[1][k];
	}
	if (lane < pend_q) qnxt[oq + lane] = pq[lane];
	if (lane < pend_t) touched[ot + lane] = pt[lane];
}

// bound[lane] = the largest tentative label among the lane's destinations (rows [lo, hi) are sorted by lane); INF while
// one of them is unlabelled.  Workgroup-local maxima in LDS, one atomicMax per lane and workgroup.
template <typename DT>
__global__ __launch_bounds__(256) void k_lane_bounds(int64_t lo, int64_t hi, const u32 *__restrict__ skey,
                                                     const int32_t *__restrict__ sdst, u32 base_lane,
                                                     const DT *__restrict__ dist, int64_t inf_bits, long long *__restrict__ bound) {
	__shared__ long long s_b[64];
	if (threadIdx.x < 64) s_b[threadIdx.x] = 0;
	__syncthreads();
	for (int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (int64_t)gridDim.x * blockDim.x) {
		const u32 l = skey[i] - base_lane;
		const long long d = (long long)Lab<DT>::widen(dist[(size_t)sdst[i] * LC + l], inf_bits);
		if (d > s_b[l]) atomicMax(&s_b[l], d);
	}
	__syncthreads();
	if (threadIdx.x < 64 && s_b[threadIdx.x] > 0) atomicMax(&bound[threadIdx.x], s_b[threadIdx.x]);
}

// the start of a round (RelaxCounters: pgq_relax.h): the next queue's count, the round's statistics, the lanes' bounds
__global__ void k_round_reset(RelaxCounters *__restrict__ rc, int next_par) {
	const int t = threadIdx.x;
	if (t < 64) rc->bound[t] = 0;
	if (t == 0) {
		rc->nq[next_par] = 0;
		rc->relaxed_vertices = 0;
		rc->min_deferred = 0x7F7F7F7F7F7F7F7Fll; // > every label
		rc->heavy = 0;
	}
}

#define PGQ_LD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define PGQ_ST(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// Small-frontier rounds without the host: ONE 1024-thread workgroup keeps relaxing round after round while the
// queue of changed vertices stays <= `limit` (a forest / long chain advances one hop per round: 18 host round
// trips per batch otherwise).  Everything another wavefront may have changed is read with agent-scope atomic
// loads (distances are updated by L2 atomics, a plain load could hit a stale L1 line); rounds are separated by
// __syncthreads().  Same relaxation and bookkeeping as k_relax.
template <typename T>
__global__ __launch_bounds__(1024) void k_relax_small(const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                      const T *__restrict__ w, int64_t *__restrict__ dist,
                                                      u64 *__restrict__ dirty0, u64 *__restrict__ dirty1,
                                                      int32_t *__restrict__ q0, int32_t *__restrict__ q1,
                                                      RelaxCounters *__restrict__ rc, int par, u32 limit,
                                                      u32 *__restrict__ qflag, u32 epoch0, u32 *__restrict__ tflag,
                                                      u32 tepoch, int32_t *__restrict__ touched, int max_rounds) {
	__shared__ u32 s_nq;
	const int lane = threadIdx.x & 63;
	const u32 wib = threadIdx.x >> 6;
	const u32 nw = blockDim.x >> 6;
	u64 edges = 0;
	int round = 0;
	for (; round < max_rounds; round++) {
		if (threadIdx.x == 0) s_nq = PGQ_LD(&rc->nq[par]);
		__syncthreads();
		const u32 nq = s_nq;
		if (nq == 0 || nq > limit) break;
		if (threadIdx.x == 0) PGQ_ST(&rc->nq[par ^ 1], 0u);
		__syncthreads();
		u64 *dirty_cur = par ? dirty1 : dirty0, *dirty_nxt = par ? dirty0 : dirty1;
		const int32_t *qcur = par ? q1 : q0;
		int32_t *qnxt = par ? q0 : q1;
		const u32 epoch = epoch0 + (u32)round;
		for (u32 i = wib; i < nq; i += nw) {
			const int v = PGQ_LD(&qcur[i]);
			u64 mask = 0;
			if (lane == 0) mask = atomicExch(&dirty_cur[v], 0ull);
			mask = __shfl(mask, 0);
			const bool mine = (mask >> lane) & 1ull;
			const int64_t dvb = PGQ_LD(&dist[(size_t)v * LC + lane]);
			const int64_t b = off[v], e = off[v + 1];
			edges += (u64)(e - b);
			for (int64_t k = b; k < e; k++) {
				const int n = adj[k];
				T wt = w[k];
				if constexpr (std::is_same<T, double>::value) wt = wt == wt ? wt : __longlong_as_double(0x7FF0000000000000ll); // NaN: like k_relax
				bool improved = false;
				if (mine) {
					int64_t cand;
					if constexpr (std::is_same<T, double>::value) cand = __double_as_longlong(__longlong_as_double(dvb) + wt);
					else cand = dvb + (int64_t)wt;
					int64_t *dp = &dist[(size_t)n * LC + lane];
					if (cand < PGQ_LD(dp)) {
						const int64_t old = atomicMin((long long *)dp, (long long)cand);
						improved = cand < old;
					}
				}
				const u64 imask = __ballot(improved);
				if (imask && lane == 0) {
					atomicOr(&dirty_nxt[n], imask);
					if (atomicExch(&qflag[n], epoch) != epoch) PGQ_ST(&qnxt[atomicAdd(&rc->nq[par ^ 1], 1u)], n);
					if (atomicExch(&tflag[n], tepoch) != tepoch) touched[atomicAdd(&rc->tcount, 1u)] = n;
				}
			}
		}
		__syncthreads();
		par ^= 1;
	}
	if (lane == 0 && edges) atomicAdd(&rc->relaxed_edges, edges);
	if (threadIdx.x == 0) rc->rounds = (u32)round;
}

// results: out[row] = dist[dst][lane]; INF -> invalid.  Also trivial rows.
template <typename DT>
__global__ void k_cheapest_results(int64_t lo, int64_t hi, const u32 *__restrict__ skey, const u32 *__restrict__ sidx,
                                   const int32_t *__restrict__ sdst, u32 base_lane, const DT *__restrict__ dist,
                                   int64_t inf_bits, int64_t *__restrict__ out, uint8_t *__restrict__ ok) {
	int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= hi) return;
	const u32 l = skey[i] - base_lane;
	const int64_t d = Lab<DT>::widen(dist[(size_t)sdst[i] * LC + l], inf_bits);
	const u32 row = sidx[i];
	if (d == inf_bits) {
		ok[row] = 0;
		out[row] = 0;
	} else {
		ok[row] = 1;
		out[row] = d;
	}
}

__global__ void k_cheapest_tails(int64_t lo_trivial, int64_t lo_null, int64_t n, const u32 *__restrict__ sidx,
                                 int64_t *__restrict__ out, uint8_t *__restrict__ ok) {
	int64_t i = lo_trivial + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const u32 row = sidx[i];
	out[row] = 0; // int64 0 and +0.0 share the bit pattern
	ok[row] = i < lo_null ? 1 : 0;
}

template <typename DT>
__global__ void k_reset_touched(const int32_t *__restrict__ touched, const u32 *__restrict__ tcount,
                                DT *__restrict__ dist, DT inf_bits) {
	const u32 nt = *tcount;
	int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (; t < (int64_t)nt * LC; t += stride) dist[(size_t)touched[t / LC] * LC + (t % LC)] = inf_bits;
}


// ---- chain pre-pass ----------------------------------------------------------------------------------------------------
// While every vertex on the way has exactly one out-edge, the set of vertices reachable from src IS that chain: if dst
// is on it the only path's cost is the answer (folded left to right like `dist[v] + w`, cheapest_path_length.cpp:29-36,
// so int64 and double results are bit-identical), if the chain ends in a vertex without out-edges first, dst is
// unreachable (NULL, :74-85).  Message-reply forests (BASELINE configs[4]) are answered entirely here; a row whose
// chain reaches a vertex with several out-edges (or runs for `cap` steps: a cycle) is left to the batched relaxation.
// One thread per row; ok = 2 marks "open".
template <typename T>
__global__ void k_chain_walk(int64_t n, const int64_t *__restrict__ src, const int64_t *__restrict__ dst, int64_t V,
                             const int64_t *__restrict__ off, const int32_t *__restrict__ adj, const T *__restrict__ w,
                             T *__restrict__ out, uint8_t *__restrict__ ok, int cap, u32 *__restrict__ counters) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const T sentinel = std::numeric_limits<T>::max() / 2;
	int step = 0;
	if (i < n) {
		const int64_t s = src[i], d = dst[i];
		T acc = (T)0;
		uint8_t state = 0; // 0 NULL, 1 found, 2 open
		if (s >= V || (s >= 0 && (d < 0 || d >= V))) {
			counters[1] = 1; // id out of range
		} else if (s >= 0) {
			int64_t x = s;
			for (;; step++) {
				if (x == d) {
					state = 1;
					break;
				}
				const int64_t b = off[x], deg = off[x + 1] - b;
				if (deg == 0) break;
				if (deg > 1 || step >= cap) {
					state = 2;
					break;
				}
				// the reference relaxes `dist[v] + w < dist[n]` against the max/2 sentinel (cheapest_path_length.cpp:15,29-36):
				// a sum that does not get under it (inf or NaN weights, sums past max/2) never labels the next vertex, and
				// nothing else leads on from a vertex with one out-edge
				const T nacc = acc + w[b];
				if (!(nacc < sentinel)) break; // state stays 0: NULL
				acc = nacc;
				x = adj[b];
			}
		}
		out[i] = state == 1 ? acc : (T)0;
		ok[i] = state;
	}
	// statistics: open rows and chain steps, one atomic each per wave
	const u64 open = __ballot(i < n && ok[i] == 2);
	int steps = step;
	for (int sh = 32; sh; sh >>= 1) steps += __shfl_xor(steps, sh);
	if ((threadIdx.x & 63) == 0) {
		if (open) atomicAdd(&counters[0], (u32)__popcll(open));
		if (steps) atomicAdd(&counters[3], (u32)steps);
	}
}
__global__ void k_collect_open_rows(int64_t n, const uint8_t *__restrict__ ok, const int64_t *__restrict__ src,
                                    const int64_t *__restrict__ dst, int64_t *__restrict__ dsrc, int64_t *__restrict__ ddst,
                                    u32 *__restrict__ didx, u32 *__restrict__ count) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool open = i < n && ok[i] == 2;
	const u64 m = __ballot(open);
	if (!m) return;
	const int lane = threadIdx.x & 63;
	u32 base = 0;
	if (lane == 0) base = atomicAdd(count, (u32)__popcll(m));
	base = __shfl(base, 0);
	if (open) {
		const u32 p = base + (u32)__popcll(m & ((1ull << lane) - 1ull));
		dsrc[p] = src[i];
		ddst[p] = dst[i];
		didx[p] = (u32)i;
	}
}
__global__ void k_apply_open_rows(int64_t nd, const u32 *__restrict__ didx, const int64_t *__restrict__ dval,
                                  const uint8_t *__restrict__ dok, int64_t *__restrict__ out, uint8_t *__restrict__ ok) {
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= nd) return;
	out[didx[j]] = dval[j];
	ok[didx[j]] = dok[j];
}

// ---- weighted pairs on general graphs: bidirectional band-wise label correcting per row (k_wbibfs, int64 weights) ------
// The batched relaxation below computes, per lane, the distances from the source to EVERY vertex it can reach: on the
// weighted knows graph that is the whole graph per distinct source (8.6 visits per edge, 725 pairs/s in round 1).  A
// single pair needs far less: the forward ball of src and the backward ball of dst, each of about half the distance.
// One 1024-thread workgroup per row runs delta-stepping from both ends (a row-private distance array per side in global
// memory, reset through the list of touched vertices; near / far vertex queues per side):
//     expand the side with the smaller radius by one band [r, r + delta): relax the near queue to its fixpoint (a vertex
//     improved to below r + delta goes back into the near queue, others into the far queue); every improvement of a vertex
//     the other side has labelled offers  best = min(best, new label + other side's label)
//     the band is complete: r += delta; stop when r_fwd + r_bwd >= best; refill the near queue from the far queue
//     (skipping bands without vertices); an empty far queue means that side's closure is exhausted
// Exactness (int64 sums, any order): when r_fwd + r_bwd >= best > D were to hold, take the last vertex x of an optimal path
// with d_fwd(x) < r_fwd and its successor y: d_bwd(y) = D - d_fwd(y) <= D - r_fwd < r_bwd, so both are final, and the later
// of "x relaxed forward" / "y relaxed backward" has offered d_fwd(x) + w + d_bwd(y) = D.  Checked against Dijkstra in a
// Python model of exactly this schedule (zero weights, band skipping, duplicates in the queues) before it was written here.
// A row whose queues or work exceed their caps stays open (ok = 2) and goes to the batched relaxation.
constexpr long long kWbInf = 1LL << 62;
struct WbCounters {
	u32 open;
	u32 pad;
	unsigned long long relaxed;
};

__global__ void k_iota32(int64_t n, u32 *__restrict__ out) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) out[i] = (u32)i;
}
__global__ void k_gather_weights(int64_t n, const u32 *__restrict__ slot, const int64_t *__restrict__ w, int64_t *__restrict__ rw) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) rw[i] = w[slot[i]];
}

// adjacency walk of a vertex list with each vertex's 64-bit payload (its own label) and the slot position of a lane's four
// entries (for the weights): g(v, valid, payload, t)
template <typename G>
__device__ __forceinline__ unsigned long long wb_walk(const u32 *__restrict__ list, int list_n, int w, int stride,
                                                      const int64_t *__restrict__ xoff, const int32_t *__restrict__ xadj,
                                                      const long long *__restrict__ pay, G g) {
	const int lane = threadIdx.x & 63;
	unsigned long long entries = 0;
	for (int pb = w; pb < list_n; pb += 64 * stride) {
		int vb = 0, ve = 0;
		long long pv = 0;
		const int p = pb + lane * stride;
		if (p < list_n) {
			const u32 vid = list[p];
			vb = (int)xoff[vid];
			ve = (int)xoff[vid + 1];
			pv = __hip_atomic_load(&pay[vid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		const int cnt = min(64, (list_n - pb + stride - 1) / stride);
		int j = -1, q = 0, e = 0, b = 0;
		long long cp = 0;
		auto seek = [&]() {
			for (j++; j < cnt; j++) {
				b = __builtin_amdgcn_readlane(vb, j);
				e = __builtin_amdgcn_readlane(ve, j);
				if (e > b) {
					q = b & ~3;
					const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)pv, j);
					const u32 hi = (u32)__builtin_amdgcn_readlane((int)(u32)((unsigned long long)pv >> 32), j);
					cp = (long long)(((unsigned long long)hi << 32) | lo);
					return;
				}
			}
		};
		seek();
		while (j < cnt) { // one chunk at a time: the callback's own memory operations are the long part
			const int t = q + 4 * lane;
			typedef int v4i __attribute__((ext_vector_type(4)));
			const v4i r = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(xadj + (t < e ? t : q)));
			const u32 valid = (u32)(t >= b && t < e) | ((u32)(t + 1 >= b && t + 1 < e) << 1) |
			                  ((u32)(t + 2 >= b && t + 2 < e) << 2) | ((u32)(t + 3 >= b && t + 3 < e) << 3);
			entries += (unsigned long long)(min(e, q + 256) - max(b, q));
			const long long cur = cp;
			q += 256;
			if (q >= e) seek();
			g(make_int4(r.x, r.y, r.z, r.w), valid, cur, t);
		}
	}
	return entries;
}

__global__ __launch_bounds__(1024) void k_wbibfs(int64_t n, const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                                                 const u32 *__restrict__ didx, const int64_t *__restrict__ off,
                                                 const int32_t *__restrict__ adj, const int64_t *__restrict__ w,
                                                 const int64_t *__restrict__ roff, const int32_t *__restrict__ radj,
                                                 const int64_t *__restrict__ rw, int64_t V, long long delta,
                                                 long long work_cap, int qcap, int fcap, int prune, long long *__restrict__ dist_all,
                                                 u32 *__restrict__ queues_all, int64_t *__restrict__ out,
                                                 uint8_t *__restrict__ ok, WbCounters *__restrict__ wc) {
	// per workgroup: dist[side][V + 1] (entry V takes the masked lanes), near[side][parity][qcap] (vertices inside the
	// current band, duplicates possible), far[side][parity][fcap] and touched[side][fcap] (every labelled vertex once)
	long long *const dist0 = dist_all + (size_t)blockIdx.x * 2 * (size_t)(V + 1);
	u32 *const qb = queues_all + (size_t)blockIdx.x * (4 * (size_t)qcap + 6 * (size_t)fcap);
	u32 *const fb = qb + 4 * (size_t)qcap;  // far[side][parity]
	u32 *const tb = fb + 4 * (size_t)fcap;  // touched[side]
	__shared__ u32 s_nn, s_nfar[2], s_nt[2], s_cnt2[2];
	__shared__ unsigned long long s_best, s_min, s_work;
	const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
	unsigned long long relaxed = 0;
	u32 open_rows = 0;
	for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
		__syncthreads();
		const int64_t s = src[i], d = dst[i]; // open rows of the chain pre-pass: ids in range, src != dst
		const u32 row = didx[i];
		if (tid == 0) {
			s_nfar[0] = s_nfar[1] = 0;
			s_nt[0] = s_nt[1] = 1;
			s_best = (unsigned long long)kWbInf;
			s_work = 0;
			__hip_atomic_store(&dist0[s], 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			__hip_atomic_store(&dist0[(V + 1) + d], 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			tb[0] = (u32)s;
			tb[(size_t)fcap] = (u32)d;
			qb[0] = (u32)s;
			qb[2 * (size_t)qcap] = (u32)d;
		}
		u32 nn0 = 1, nn1 = 1;      // near-queue fill per side
		int par0 = 0, par1 = 0;    // which of a side's two near buffers is current
		int fpar0 = 0, fpar1 = 0;  // ... and of its two far buffers
		long long r0 = 0, r1 = 0;  // completed radius per side
		int state = 2;             // 0 NULL, 1 found, 2 open
		__threadfence_block();
		__syncthreads();
		if (s == d) state = 1, s_best = 0; // not expected here; kept for safety (every thread writes the same value)
		while (state == 2 && s != d) {
			const int side = r0 <= r1 ? 0 : 1;
			const int64_t *xoff = side ? roff : off;
			const int32_t *xadj = side ? radj : adj;
			const int64_t *xw = side ? rw : w;
			long long *mine = dist0 + (size_t)side * (size_t)(V + 1);
			const long long *theirs = dist0 + (size_t)(side ^ 1) * (size_t)(V + 1);
			const int fpar = side ? fpar1 : fpar0;
			u32 *far = fb + (size_t)(side * 2 + fpar) * fcap;
			u32 *touched = tb + (size_t)side * fcap;
			const long long rn = (side ? r1 : r0) + delta;
			u32 nn = side ? nn1 : nn0;
			int par = side ? par1 : par0;
			bool over = false;
			// -- the band [r, rn): relax the near queue to its fixpoint
			while (nn > 0) {
				const u32 *cur = qb + (size_t)(side * 2 + par) * qcap;
				u32 *nxt = qb + (size_t)(side * 2 + (par ^ 1)) * qcap;
				if (tid == 0) s_nn = 0;
				__syncthreads();
				unsigned long long lbest = (unsigned long long)kWbInf;
				const long long r_other = side ? r0 : r1;
				const unsigned long long e2 = wb_walk(cur, (int)nn, wib, 16, xoff, xadj, mine, [&](const int4 &v, u32 valid, long long dv, int t) {
					// optional pruning (wbibfs_prune): a vertex whose label plus the other side's completed radius already
					// reaches `best` cannot start a better path — an out-neighbour u the other side has settled with
					// w + d_other(u) < r_other makes this vertex settled there too, and its own labelling offered that sum
					if (prune && (unsigned long long)(dv + r_other) >= *(volatile unsigned long long *)&s_best) valid = 0;
					const u32 xs[4] = { (u32)v.x, (u32)v.y, (u32)v.z, (u32)v.w };
					u32 x[4];
					long long nd[4], old[4], oth[4];
					// no per-lane branches around memory operations: masked lanes use the spare entry V with an infinite label
#pragma unroll
					for (int k = 0; k < 4; k++) {
						const bool in = (valid >> k) & 1u;
						x[k] = in ? xs[k] : (u32)V;
						const long long wt = xw[in ? (size_t)(t + k) : (size_t)0]; // masked lanes read slot 0
						nd[k] = in ? dv + wt : kWbInf;
					}
#pragma unroll
					for (int k = 0; k < 4; k++) old[k] = atomicMin(&mine[x[k]], nd[k]);
#pragma unroll
					for (int k = 0; k < 4; k++) oth[k] = __hip_atomic_load(&theirs[x[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
					for (int k = 0; k < 4; k++) {
						const bool in = (valid >> k) & 1u;
						const bool better = in && nd[k] < old[k];
						const bool first = better && old[k] >= kWbInf;
						if (better && oth[k] < kWbInf) lbest = min(lbest, (unsigned long long)(nd[k] + oth[k]));
						// a vertex enters the far queue once, when it is first labelled beyond the band: a later improvement either
						// stays beyond the band (its entry is still there) or moves it into the near queue
						const bool to_near = better && nd[k] < rn, to_far = first && !(nd[k] < rn);
						const u64 mn = __ballot(to_near), mf = __ballot(to_far), mt = __ballot(first);
						if (mn) {
							u32 base = 0;
							if (lane == 0) base = atomicAdd(&s_nn, (u32)__popcll(mn));
							base = (u32)__shfl((int)base, 0);
							const u32 slot = base + __builtin_amdgcn_mbcnt_hi((u32)(mn >> 32), __builtin_amdgcn_mbcnt_lo((u32)mn, 0u));
							if (to_near && slot < (u32)qcap) nxt[slot] = x[k];
						}
						if (mf) {
							u32 base = 0;
							if (lane == 0) base = atomicAdd(&s_nfar[side], (u32)__popcll(mf));
							base = (u32)__shfl((int)base, 0);
							const u32 slot = base + __builtin_amdgcn_mbcnt_hi((u32)(mf >> 32), __builtin_amdgcn_mbcnt_lo((u32)mf, 0u));
							if (to_far && slot < (u32)fcap) far[slot] = x[k];
						}
						if (mt) {
							u32 base = 0;
							if (lane == 0) base = atomicAdd(&s_nt[side], (u32)__popcll(mt));
							base = (u32)__shfl((int)base, 0);
							const u32 slot = base + __builtin_amdgcn_mbcnt_hi((u32)(mt >> 32), __builtin_amdgcn_mbcnt_lo((u32)mt, 0u));
							if (first && slot < (u32)fcap) touched[slot] = x[k];
						}
					}
				});
				for (int o = 32; o > 0; o >>= 1) {
					const unsigned long long y = __shfl_xor(lbest, o);
					lbest = y < lbest ? y : lbest;
				}
				if (lane == 0) {
					if (lbest < (unsigned long long)kWbInf) atomicMin(&s_best, lbest);
					if (e2) atomicAdd(&s_work, e2);
				}
				__syncthreads();
				nn = s_nn;
				par ^= 1;
				if (nn > (u32)qcap || s_nfar[side] > (u32)fcap || s_nt[side] > (u32)fcap || (long long)s_work > work_cap) {
					over = true;
					break;
				}
				__syncthreads(); // s_nn is reset by the next round
			}
			if (over) break; // state stays 2: the row is left to the batched relaxation
			if (side) r1 = rn, nn1 = 0, par1 = par;
			else r0 = rn, nn0 = 0, par0 = par;
			if ((unsigned long long)(r0 + r1) >= s_best) {
				state = 1;
				break;
			}
			// -- refill the near queue from the far queue; bands without vertices are skipped
			const u32 nf = s_nfar[side];
			const long long rr = side ? r1 : r0;
			if (tid == 0) s_min = (unsigned long long)kWbInf;
			__syncthreads();
			unsigned long long lm = (unsigned long long)kWbInf;
			for (u32 p = tid; p < nf; p += 1024) {
				const long long dv = __hip_atomic_load(&mine[far[p]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if (dv >= rr) lm = min(lm, (unsigned long long)dv); // below rr: settled in an earlier band (a stale copy)
			}
			for (int o = 32; o > 0; o >>= 1) {
				const unsigned long long y = __shfl_xor(lm, o);
				lm = y < lm ? y : lm;
			}
			if (lane == 0 && lm < (unsigned long long)kWbInf) atomicMin(&s_min, lm);
			__syncthreads();
			const unsigned long long m = s_min;
			if (m >= (unsigned long long)kWbInf) { // nothing left on this side: its closure is complete
				state = s_best < (unsigned long long)kWbInf ? 1 : 0;
				break;
			}
			long long base_r = rr;
			if ((long long)m >= rr + delta) base_r = ((long long)m / delta) * delta;
			if (side) r1 = base_r;
			else r0 = base_r;
			if ((unsigned long long)(r0 + r1) >= s_best) {
				state = 1;
				break;
			}
			// the side's near buffers are free now: [par] becomes the new near queue; what stays far goes to the other far buffer
			u32 *newnear = qb + (size_t)(side * 2 + par) * qcap;
			u32 *keep = fb + (size_t)(side * 2 + (fpar ^ 1)) * fcap;
			if (tid == 0) s_cnt2[0] = s_cnt2[1] = 0;
			__syncthreads();
			for (u32 p0 = 0; p0 < nf; p0 += 1024) {
				const u32 p = p0 + tid;
				u32 u = 0;
				long long dv = -1;
				if (p < nf) {
					u = far[p];
					dv = __hip_atomic_load(&mine[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				}
				const bool live = p < nf && dv >= base_r;
				const bool tn = live && dv < base_r + delta, tk = live && !tn;
				const u64 mn = __ballot(tn), mk = __ballot(tk);
				if (mn) {
					u32 b2 = 0;
					if (lane == 0) b2 = atomicAdd(&s_cnt2[0], (u32)__popcll(mn));
					b2 = (u32)__shfl((int)b2, 0);
					const u32 slot = b2 + __builtin_amdgcn_mbcnt_hi((u32)(mn >> 32), __builtin_amdgcn_mbcnt_lo((u32)mn, 0u));
					if (tn && slot < (u32)qcap) newnear[slot] = u;
				}
				if (mk) {
					u32 b2 = 0;
					if (lane == 0) b2 = atomicAdd(&s_cnt2[1], (u32)__popcll(mk));
					b2 = (u32)__shfl((int)b2, 0);
					if (tk) keep[b2 + __builtin_amdgcn_mbcnt_hi((u32)(mk >> 32), __builtin_amdgcn_mbcnt_lo((u32)mk, 0u))] = u;
				}
			}
			__syncthreads();
			const u32 nnew = s_cnt2[0], nkeep = s_cnt2[1];
			if (nnew > (u32)qcap) break; // more vertices in one band than the near queue holds: the row stays open
			if (tid == 0) s_nfar[side] = nkeep;
			if (side) nn1 = nnew, fpar1 = fpar ^ 1;
			else nn0 = nnew, fpar0 = fpar ^ 1;
			__threadfence_block();
			__syncthreads();
		}
		__syncthreads();
		if (tid == 0) {
			if (state == 2) open_rows++;
			else {
				out[row] = state == 1 ? (int64_t)s_best : 0;
				ok[row] = (uint8_t)state;
			}
		}
		// the labels go back to "infinite" through the touched lists (a list that overflowed: everything)
		for (int sd = 0; sd < 2; sd++) {
			long long *dd = dist0 + (size_t)sd * (size_t)(V + 1);
			const u32 nt = s_nt[sd];
			if (nt <= (u32)fcap) {
				const u32 *tl = tb + (size_t)sd * fcap;
				for (u32 p = tid; p < nt; p += 1024) dd[tl[p]] = kWbInf;
			} else {
				for (int64_t v = tid; v < V; v += 1024) dd[v] = kWbInf;
			}
			if (tid == 0) dd[V] = kWbInf;
		}
		relaxed += tid == 0 ? s_work : 0ull;
	}
	if (tid == 0) {
		if (open_rows) atomicAdd(&wc->open, open_rows);
		if (relaxed) atomicAdd(&wc->relaxed, relaxed);
	}
}


static std::mutex g_rw_lock;
// in-edge weights in reverse-CSR order + the mean weight, built on first use (a stable sort of the forward slots by
// destination: the permutation the upload used for radj).  with_mean = false: the weights alone, w_mean stays what it is (the
// sum below adds the weights as int64: cheapest_path reads the in-edge weights of double CSRs too)
int ensure_reverse_weights(pgq_csr *c, Workspace *ws, bool with_mean) {
	std::lock_guard<std::mutex> g(g_rw_lock);
	if (c->E == 0) return PGQ_OK;
	// (a copy that cheapest_path built came without the mean: a caller that wants one gets it here, unless the handle has it)
	const bool build = !c->rw, mean = with_mean && (build || !(c->w_mean > 0));
	if (!build && !mean) return PGQ_OK;
	hipStream_t st = ws->stream;
	const int64_t E = c->E;
	DevTemps temps(st);
	u32 *iota = nullptr, *sslot = nullptr, *skey = nullptr;
	int64_t *sum = nullptr;
	void *rw = nullptr;
	if (build) {
		for (u32 **b : { &iota, &sslot, &skey }) PGQ_TRY(temps.alloc(b, (size_t)E));
		hipLaunchKernelGGL(k_iota32, dim3(blocks_for(E)), dim3(256), 0, st, E, iota);
		int end_bit = 1;
		while ((1LL << end_bit) < c->V) end_bit++;
		const u32 *keys = reinterpret_cast<const u32 *>(c->adj);
		PGQ_TRY(cub_run(temps, [&](void *tmp, size_t &tb) { return hipcub::DeviceRadixSort::SortPairs(tmp, tb, keys, skey, iota, sslot, (int)E, 0, end_bit, st); }));
		PGQ_TRY(temps.alloc_bytes(&rw, csr_bytes(c, c->rw)));
		hipLaunchKernelGGL(k_gather_weights, dim3(blocks_for(E)), dim3(256), 0, st, E, sslot, (const int64_t *)c->w, (int64_t *)rw);
	}
	int64_t total = 0;
	if (mean) {
		PGQ_TRY(temps.alloc(&sum, 8));
		PGQ_TRY(cub_run(temps, [&](void *tmp, size_t &tb) { return hipcub::DeviceReduce::Sum(tmp, tb, (const int64_t *)c->w, sum, (int)E, st); }));
		PGQ_HIP_TRY(hipMemcpyAsync(&total, sum, 8, hipMemcpyDeviceToHost, st));
	}
	PGQ_HIP_TRY(hipStreamSynchronize(st));
	if (mean) c->w_mean = (double)total / (double)E;
	if (build) {
		temps.keep(rw);
		c->rw = rw;
	}
	return PGQ_OK;
}

// a new phase (higher cap on the edge weight): every labelled vertex is expanded again over the longer prefix of its list
__global__ void k_redirty(const int32_t *__restrict__ touched, const u32 *__restrict__ tcount, u64 *__restrict__ dirty,
                          int32_t *__restrict__ q, u32 *__restrict__ nq) {
	const u32 n = *tcount;
	for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const int v = touched[i];
		dirty[v] = ~0ull; // lanes without a label are skipped by their bound test
		q[i] = v;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) *nq = n;
}

// the forward adjacency with every vertex's list sorted by weight (non-negative weights: their bit patterns sort like the
// values, int64 and double alike) — segmented radix sort, once per CSR — and the largest weight
// sort keys of double weights: the bit pattern orders non-negative doubles like their values, once -0.0 (accepted: it
// is not < 0, and adds like +0.0) has lost its sign and a NaN (never relaxes an edge: `dist + w < dist[n]` is false,
// here as in the reference) counts as +inf
__global__ void k_weight_keys(const unsigned long long *__restrict__ w, int64_t E, unsigned long long *__restrict__ key) {
	int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= E) return;
	key[i] = min(w[i] & 0x7FFFFFFFFFFFFFFFull, 0x7FF0000000000000ull);
}

static int ensure_weight_sorted(pgq_csr *c, Workspace *ws) {
	std::lock_guard<std::mutex> g(g_rw_lock);
	if (c->wadj || c->E == 0 || !c->w) return PGQ_OK;
	hipStream_t st = ws->stream;
	const int64_t E = c->E;
	DevTemps temps(st);
	int32_t *wadj = nullptr;
	void *wsorted = nullptr;
	unsigned long long *mx = nullptr;
	PGQ_TRY(temps.alloc_bytes((void **)&wadj, csr_bytes(c, c->wadj)));
	PGQ_TRY(temps.alloc_bytes(&wsorted, csr_bytes(c, c->wsorted)));
	PGQ_TRY(temps.alloc(&mx, 8));
	const unsigned long long *keys = (const unsigned long long *)c->w;
	if (c->w_type == PGQ_W_DOUBLE) {
		unsigned long long *canon = nullptr;
		PGQ_TRY(temps.alloc(&canon, (size_t)E));
		hipLaunchKernelGGL(k_weight_keys, dim3(blocks_for(E)), dim3(256), 0, st, keys, E, canon);
		keys = canon;
	}
	unsigned long long *keys_out = (unsigned long long *)wsorted;
	PGQ_TRY(cub_run(temps, [&](void *tmp, size_t &tb) {
		return hipcub::DeviceSegmentedRadixSort::SortPairs(tmp, tb, keys, keys_out, c->adj, wadj, (int)E, (int)c->V, c->off, c->off + 1, 0, 64, st);
	}));
	PGQ_TRY(cub_run(temps, [&](void *tmp, size_t &tb) { return hipcub::DeviceReduce::Max(tmp, tb, keys, mx, (int)E, st); }));
	unsigned long long m = 0;
	PGQ_HIP_TRY(hipMemcpyAsync(&m, mx, 8, hipMemcpyDeviceToHost, st));
	PGQ_HIP_TRY(hipStreamSynchronize(st));
	c->w_max_bits = m; // the largest weight, as its bit pattern (int64: the value)
	temps.keep(wadj);
	temps.keep(wsorted);
	c->wsorted = wsorted;
	c->wadj = wadj;
	return PGQ_OK;
}

// mean edge weight (int64 or double), computed once per CSR: the band width of the ordered relaxation rounds
int ensure_weight_mean(pgq_csr *c, Workspace *ws) {
	std::lock_guard<std::mutex> g(g_rw_lock);
	if (c->w_mean > 0 || c->E == 0 || !c->w) return PGQ_OK;
	hipStream_t st = ws->stream;
	DevTemps temps(st);
	void *sum = nullptr;
	PGQ_TRY(temps.alloc_bytes(&sum, 64));
	double total = 0;
	if (c->w_type == PGQ_W_DOUBLE) {
		PGQ_TRY(cub_run(temps, [&](void *tmp, size_t &tb) { return hipcub::DeviceReduce::Sum(tmp, tb, (const double *)c->w, (double *)sum, (int)c->E, st); }));
		PGQ_HIP_TRY(hipMemcpyAsync(&total, sum, 8, hipMemcpyDeviceToHost, st));
		PGQ_HIP_TRY(hipStreamSynchronize(st));
	} else {
		int64_t t = 0;
		PGQ_TRY(cub_run(temps, [&](void *tmp, size_t &tb) { return hipcub::DeviceReduce::Sum(tmp, tb, (const int64_t *)c->w, (int64_t *)sum, (int)c->E, st); }));
		PGQ_HIP_TRY(hipMemcpyAsync(&t, sum, 8, hipMemcpyDeviceToHost, st));
		PGQ_HIP_TRY(hipStreamSynchronize(st));
		total = (double)t;
	}
	c->w_mean = std::max(total / (double)c->E, 1e-300);
	return PGQ_OK;
}

// rows [0, nd) in ws->def_src / def_dst / def_idx (the chain pre-pass's open rows): answered rows get their value and
// flag written into d_out / d_ok, the others keep ok = 2.  *left = rows still open.
static int weighted_pairs_prepass(pgq_csr *c, Workspace *ws, u32 nd, int64_t *d_out, uint8_t *d_ok, u32 *left) {
	*left = nd;
	const Options &opt = options();
	if (!opt.wbibfs || c->w_type != PGQ_W_INT64 || (int64_t)nd > (int64_t)opt.wbibfs_rows) return PGQ_OK;
	const int qcap = std::max(1024, opt.wbibfs_queue);
	// far / touched hold every labelled vertex once: the boundary of a ball in a graph of degree ~90 is ~90 x the ball
	const int fcap = (int)std::min<int64_t>(std::max<int64_t>(c->V, 1024), (int64_t)std::max(1024, opt.wbibfs_far));
	const size_t q_words = (size_t)4 * qcap + (size_t)6 * fcap;
	const size_t per_wg = (size_t)2 * (size_t)(c->V + 1) * 8 + q_words * 4;
	const size_t budget = (size_t)std::max(0, opt.wbibfs_mem_mb) << 20;
	const u32 grid = (u32)std::min<size_t>(std::min<u32>(nd, 256), budget / per_wg);
	if (grid == 0) return PGQ_OK;
	PGQ_TRY(ensure_reverse_weights(c, ws));
	hipStream_t st = ws->stream;
	const size_t dist_words = (size_t)grid * 2 * (size_t)(c->V + 1);
	const bool fresh = ws->wb_scratch.cap < dist_words * 8 + (size_t)grid * q_words * 4 + 64 || ws->wb_V != c->V || ws->wb_grid != (int)grid;
	PGQ_TRY(ws->wb_scratch.reserve(dist_words * 8 + (size_t)grid * q_words * 4 + 64));
	long long *dist = ws->wb_scratch.as<long long>();
	u32 *queues = reinterpret_cast<u32 *>(dist + dist_words);
	if (fresh) { // every label infinite; the kernel restores what it touched
		hipLaunchKernelGGL(k_fill64, dim3((unsigned)device_cus() * 8), dim3(256), 0, st, (int64_t *)dist, (int64_t)dist_words, (int64_t)kWbInf);
		ws->wb_V = c->V;
		ws->wb_grid = (int)grid;
	}
	PGQ_TRY(ws->counters.reserve(sizeof(Counters)));
	WbCounters *wc = reinterpret_cast<WbCounters *>(reinterpret_cast<char *>(ws->counters.p) + 32);
	PGQ_HIP_TRY(hipMemsetAsync(wc, 0, sizeof(WbCounters), st));
	const long long delta = std::max<long long>(1, (long long)(c->w_mean / std::max(1, opt.wbibfs_delta_div)));
	{
		KernelTimer kt(st, K_RELAX);
		hipLaunchKernelGGL(k_wbibfs, dim3(grid), dim3(1024), 0, st, (int64_t)nd, ws->def_src.as<int64_t>(), ws->def_dst.as<int64_t>(),
		                   ws->def_idx.as<u32>(), c->off, c->adj, (const int64_t *)c->w, c->roff, c->radj, (const int64_t *)c->rw,
		                   c->V, delta, (long long)std::max(1, opt.wbibfs_cap), qcap, fcap, opt.wbibfs_prune, dist, queues, d_out, d_ok, wc);
		kt.stop();
	}
	WbCounters h;
	PGQ_HIP_TRY(hipMemcpyAsync(&h, wc, sizeof(h), hipMemcpyDeviceToHost, st));
	PGQ_HIP_TRY(hipStreamSynchronize(st));
	KernelTimer::flush();
	pgq_stats_t &S = tstats().s;
	S.edges_scanned += (int64_t)h.relaxed;
	S.algo_bytes[K_RELAX] += 28.0 * (double)h.relaxed; // adjacency entry, weight, label RMW, other side's label
	S.meet_pairs += (int64_t)nd - (int64_t)h.open;
	*left = h.open;
	return PGQ_OK;
}

template <typename T>
static int cheapest_device(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst,
                           int64_t *d_out, uint8_t *d_ok, bool chain, int64_t max_hops = -1, int64_t min_hops = 0);

template <typename T>
static int cheapest_with_chains(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst,
                                int64_t *d_out, uint8_t *d_ok) {
	hipStream_t st = ws->stream;
	PGQ_TRY(ws->counters.reserve(sizeof(Counters)));
	u32 *d_cnt = reinterpret_cast<u32 *>(ws->counters.p); // [0] open rows, [1] bad id, [2] compaction cursor
	PGQ_HIP_TRY(hipMemsetAsync(d_cnt, 0, 16, st));
	{
		KernelTimer kt(st, K_RELAX);
		hipLaunchKernelGGL(k_chain_walk<T>, dim3(blocks_for(n)), dim3(256), 0, st, n, d_src, d_dst, c->V, c->off, c->adj,
		                   (const T *)c->w, (T *)d_out, d_ok, std::max(1, options().chain_cap), d_cnt);
		kt.stop();
	}
	u32 h[4] = { 0, 0, 0, 0 };
	PGQ_HIP_TRY(hipMemcpyAsync(h, d_cnt, sizeof(h), hipMemcpyDeviceToHost, st));
	PGQ_HIP_TRY(hipStreamSynchronize(st));
	KernelTimer::flush();
	{ // a chain step reads off[x], off[x+1], w[b], adj[b]; a row reads its pair and writes value + flag
		pgq_stats_t &S = tstats().s;
		S.edges_scanned += h[3];
		S.algo_bytes[K_RELAX] += 28.0 * h[3] + 25.0 * (double)n;
	}
	if (h[1]) return fail(PGQ_ERR_INVALID_ARG, "src/dst rowid out of range [0,V)");
	const u32 nd_chain = h[0];
	tstats().s.meet_pairs += n - (int64_t)nd_chain;
	if (nd_chain == 0) {
		tstats().s.pairs += n;
		return PGQ_OK;
	}
	PGQ_TRY(ws->def_src.reserve((size_t)nd_chain * 8));
	PGQ_TRY(ws->def_dst.reserve((size_t)nd_chain * 8));
	PGQ_TRY(ws->def_idx.reserve((size_t)nd_chain * 4));
	PGQ_TRY(ws->def_len.reserve((size_t)nd_chain * 8));
	PGQ_TRY(ws->def_off.reserve((size_t)nd_chain));
	auto collect_open = [&]() -> int { // the open rows (ok = 2) compacted into ws->def_src / def_dst / def_idx, waited for
		PGQ_HIP_TRY(hipMemsetAsync(d_cnt + 2, 0, 4, st));
		hipLaunchKernelGGL(k_collect_open_rows, dim3(blocks_for(n)), dim3(256), 0, st, n, d_ok, d_src, d_dst,
		                   ws->def_src.as<int64_t>(), ws->def_dst.as<int64_t>(), ws->def_idx.as<u32>(), d_cnt + 2);
		PGQ_HIP_TRY(hipStreamSynchronize(st));
		return PGQ_OK;
	};
	PGQ_TRY(collect_open());
	u32 nd = nd_chain;
	{ // general graphs: a bidirectional search per row; what it leaves open (caps) is collected again
		u32 left = nd;
		PGQ_TRY(weighted_pairs_prepass(c, ws, nd, d_out, d_ok, &left));
		if (left != nd) {
			nd = left;
			if (nd == 0) {
				tstats().s.pairs += n;
				return PGQ_OK;
			}
			PGQ_TRY(collect_open());
		}
	}
	{
		WorkspaceLease inner;
		PGQ_TRY(inner.acquire());
		PGQ_TRY(cheapest_device<T>(c, inner.ws, nd, ws->def_src.as<int64_t>(), ws->def_dst.as<int64_t>(),
		                           ws->def_len.as<int64_t>(), ws->def_off.as<uint8_t>(), false));
		hipLaunchKernelGGL(k_apply_open_rows, dim3(blocks_for(nd)), dim3(256), 0, st, (int64_t)nd, ws->def_idx.as<u32>(),
		                   ws->def_len.as<int64_t>(), ws->def_off.as<uint8_t>(), d_out, d_ok);
		PGQ_HIP_TRY(hipStreamSynchronize(st));
	}
	tstats().s.pairs += n - (int64_t)nd; // the rows of the inner call were counted there
	return PGQ_OK;
}

// Whether the relaxation of this CSR runs "light edges first" (weight-sorted lists under a doubling cap, one host round
// trip per round) or plain rounds (every edge of a changed vertex; few changed vertices loop on the device, k_relax_small).
// The cap pays by the edges it does not scan: on the weighted knows graph (89 edges per vertex, cheapest paths use the
// lightest few per cent) it took 9.3 s to 0.6 s per 4096 pairs.  A vertex with three or four edges has nothing to skip:
// a weighted ring with chords ran 1830 rounds (0.28 s) under the cap against 365 rounds (0.05 s) plain — round 4 shipped
// that regression.  relax_light = 1 (shipped): by the mean out-degree; 2: always (tests); 0: never.
static bool light_edges_first(const pgq_csr *c) {
	const Options &o = options();
	if (o.relax_light == 0 || c->E <= 0) return false;
	if (o.relax_light >= 2) return true;
	return (double)c->E >= (double)std::max(1, o.relax_light_min_degree) * (double)std::max<int64_t>(c->V, 1);
}

// Whether this CSR's labels are stored as int32 (Lab<int32_t> above): int64 weights, the light-edges-first path (the
// device-side small rounds of the plain path keep 8-byte labels), and no path sum that could reach 2^31 - 1.
template <typename T> static bool labels_fit_32(const pgq_csr *c) {
	if (!std::is_same<T, int64_t>::value || !options().relax_labels32 || !light_edges_first(c) || !c->wadj) return false;
	if (!(c->w_mean > 0 && c->w_mean < 1e300)) return false; // (plain rounds then: cheapest_device's own test)
	const unsigned long long w_max = c->w_max_bits; // int64 weights are non-negative here: the bit pattern is the value
	return w_max < (1ull << 31) && (double)w_max * (double)std::max<int64_t>(c->V, 1) < 2147483000.0;
}

// ---- what the two relaxation drivers share ------------------------------------------------------------------------------
// what a label array holds (RelaxSide::dist_tag): INF differs between int64 and double, the cell size between 8 and 4 bytes
template <typename T, typename DT> constexpr int relax_label_tag() { return sizeof(DT) == 4 ? 3 : (std::is_same<T, double>::value ? 2 : 1); }

// distances start at INF; a full fill only when the array is new, afterwards only touched rows are reset
template <typename DT> int RelaxSide::prepare(int64_t V, int type_tag, DT inf_label, hipStream_t st) {
	const size_t Vn = (size_t)std::max<int64_t>(V, 1), cells = Vn * LC;
	const bool fresh = dist.cap < cells * sizeof(DT) || dist_V != V || dist_tag != type_tag;
	dist_V = -1; // stays invalid if we bail out half-way; restored by settle()
	PGQ_TRY(dist.reserve(cells * sizeof(DT)));
	for (DevBuf &b : dirty) PGQ_TRY(b.reserve(Vn * 8));
	for (DevBuf *b : { &q[0], &q[1], &touched, &tflag }) PGQ_TRY(b->reserve(Vn * 4));
	if (fresh && sizeof(DT) == 4) fill32(dist.as<int32_t>(), (int64_t)cells, (int32_t)inf_label, st);
	if (fresh && sizeof(DT) == 8) hipLaunchKernelGGL(k_fill64, dim3((unsigned)device_cus() * 8), dim3(256), 0, st, dist.as<int64_t>(), (int64_t)cells, (int64_t)inf_label);
	for (DevBuf &b : dirty) PGQ_HIP_TRY(hipMemsetAsync(b.p, 0, Vn * 8, st));
	PGQ_HIP_TRY(hipMemsetAsync(tflag.p, 0, Vn * 4, st));
	return PGQ_OK;
}

// the persistent grid of a round: exactly what is resident at once (each wavefront takes every nwaves-th vertex; a
// grid larger than the chip makes the last workgroups start when the first finish: 8192 waves on 7168 slots was 2x)
static std::mutex g_relax_grid_lock;
template <typename Kernel> static int resident_grid(Kernel kernel, unsigned (&cached)[64], unsigned *grid) {
	std::lock_guard<std::mutex> g(g_relax_grid_lock);
	int dev = 0, per_cu = 0, cus = 0;
	PGQ_HIP_TRY(hipGetDevice(&dev));
	if (!cached[dev & 63]) {
		PGQ_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0));
		PGQ_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
		cached[dev & 63] = (unsigned)std::max(1, per_cu) * (unsigned)std::max(1, cus);
	}
	*grid = cached[dev & 63];
	return PGQ_OK;
}
template <typename T, typename DT> static int relax_grid(unsigned *grid) {
	static unsigned cached[64] = {}; // per instantiation and device: a node's devices need not be alike
	return resident_grid(k_relax<T, DT>, cached, grid);
}

// a fraction of the mean weight as a weight: a band width, a first cap (integers: at least 1)
template <typename T> static T weight_fraction(double mean, int div) {
	return std::is_same<T, double>::value ? (T)(mean / div) : (T)std::max<int64_t>(1, (int64_t)(mean / div));
}

struct BiBlock { // the two-ended search's device block (BidirBatches)
	RelaxCounters rc[2]; // forward / backward: k_relax's round counters
	long long mu[64];    // per lane: best src -> dst length so far = both sides' bound; 0 once the lane is finished
	long long res[64];   // per lane: the answer (INF: no path)
	u32 alive[2][64];    // per side and lane: a labelled vertex was left unexpanded (over the cap) this round
	u32 done[64];
	long long cap, step;
	u32 active, phases;
};

// What one k_relax launch works on: everything but the pass, the grid and the queue's fill.
template <typename T> struct RelaxRound {
	Workspace *h;       // the worker's: stream, sides and heavy lists (hv, hmask, hstart, hmap)
	int s, par;         // the side that expands; which of its dirty words / queues are the input, the other parity the output
	const int64_t *off; // the lists the side walks
	const int32_t *adj;
	const T *w;
	u32 tepoch;
	RelaxCounters *rc; // the side's counter block
	long long thr;     // one-sided: only labels below it are expanded this round, no lane beyond rc->bound
	int sorted;        // the lists ascend by weight, and only the prefix under wcap counts
	T wcap;
	bool heavy;            // long lists are set aside for a heavy pass
	BiBlock *bb = nullptr; // two-ended: the pairs' bounds mu, the side's alive flags, the common cap; the other side's labels close paths
};

// The one launch of k_relax: pass 0 over the nq changed vertices (a workgroup per four), the heavy pass over the long lists' chunks.
template <typename T, typename DT> static void launch_relax(const RelaxRound<T> &r, int heavy_pass, unsigned grid, u32 nq) {
	Workspace *const h = r.h;
	RelaxSide &s = h->relax[r.s], &o = h->relax[r.s ^ 1];
	BiBlock *const bb = r.bb;
	const int p = r.par;
	if (!heavy_pass) grid = std::min(grid, std::max(1u, (nq + 3) / 4));
	hipLaunchKernelGGL((k_relax<T, DT>), dim3(grid), dim3(256), 0, h->stream, r.off, r.adj, r.w, s.dist.as<DT>(), s.dirty[p].as<u64>(),
	                   s.dirty[p ^ 1].as<u64>(), s.q[p].as<int32_t>(), &r.rc->nq[p], s.q[p ^ 1].as<int32_t>(), &r.rc->nq[p ^ 1],
	                   s.tflag.as<u32>(), r.tepoch, s.touched.as<int32_t>(), &r.rc->tcount, &r.rc->relaxed_edges, r.thr,
	                   (const long long *)(bb ? bb->mu : r.rc->bound), &r.rc->min_deferred, &r.rc->relaxed_vertices, r.sorted, r.wcap,
	                   heavy_pass, r.heavy ? &r.rc->heavy : (u64 *)nullptr, h->hv.as<int32_t>(), h->hmask.as<u64>(), h->hstart.as<u32>(),
	                   h->hmap.as<u32>(), bb ? (const DT *)o.dist.as<DT>() : (const DT *)nullptr, bb ? bb->mu : (long long *)nullptr,
	                   bb ? bb->alive[r.s] : (u32 *)nullptr, bb ? (const long long *)&bb->cap : (const long long *)nullptr);
}

// One worker of a call: `ws` holds the sorted rows and the distinct sources (read-only here), `priv` everything a batch
// writes (labels, dirty words, queues, heavy lists, counters) and the stream.  Batches are independent, so several host
// threads run side by side on their own workspaces (cheapest_device).
struct RelaxWorker {
	pgq_csr *const c;
	Workspace *const ws, *const priv;
	const int nb; // the call's batches; this worker runs b0, b0 + bstride, ... < nb
	int64_t *const d_out;
	uint8_t *const d_ok;
	const hipStream_t st = priv->stream;
	const int64_t V = c->V;
	const size_t Vn = (size_t)std::max<int64_t>(V, 1);
	pgq_stats_t &S = tstats().s;
	unsigned grid = 0; // relax_grid
	u32 tepoch = 0;    // the batch's first-touch stamp
	int b = 0;         // the batch
	const bool trace = getenv("PGQ_RELAX_TRACE") != nullptr; // a line per round on stderr (measurement only)
	// `sides` sides ready for a batch, a round's heavy lists (entries, and the map of <= E/64 + V chunks to them), the grid
	template <typename T, typename DT> int prepare(int sides) {
		for (int s = 0; s < sides; s++) PGQ_TRY(priv->relax[s].prepare<DT>(V, relax_label_tag<T, DT>(), (DT)Lab<DT>::unlabelled(Inf<T>::bits), st));
		for (DevBuf *b : { &priv->hv, &priv->hstart }) PGQ_TRY(b->reserve(Vn * 4));
		PGQ_TRY(priv->hmask.reserve(Vn * 8));
		PGQ_TRY(priv->hmap.reserve(((size_t)(c->E / 64) + Vn) * 4));
		return relax_grid<T, DT>(&grid);
	}
	int read_back(void *host, const void *dev, size_t bytes) { // a round's counters on the host, its timers (if any) resolved
		PGQ_HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
		PGQ_HIP_TRY(hipStreamSynchronize(st));
		KernelTimer::flush();
		return PGQ_OK;
	}
	// a finished batch: its statistics (adjacency entry, weight, two label rows per relaxed edge), its touched labels back to INF
	template <typename T, typename DT> void end_batch(u64 edges, int sides, RelaxCounters *rc) {
		S.edges_scanned += (int64_t)edges;
		S.algo_bytes[K_RELAX] += (double)edges * (4.0 + 8.0 + 2.0 * (double)sizeof(DT) * LC);
		for (int s = 0; s < sides; s++)
			hipLaunchKernelGGL(k_reset_touched<DT>, dim3((unsigned)device_cus() * 4), dim3(256), 0, st, priv->relax[s].touched.as<int32_t>(), &rc[s].tcount,
			                   priv->relax[s].dist.as<DT>(), (DT)Lab<DT>::unlabelled(Inf<T>::bits));
	}
	template <typename T, typename DT> int settle(int sides) { // behind the worker's last batch: every touched row is back at INF
		PGQ_HIP_TRY(hipStreamSynchronize(st));
		KernelTimer::flush();
		for (int s = 0; s < sides; s++) priv->relax[s].settle(V, relax_label_tag<T, DT>());
		return PGQ_OK;
	}
};

// The lanes' bounds of a round for a driver that needs every label final (SettledBatch, pgq_relax.h), not only the destinations': k_lane_bounds prunes a
// lane at the largest tentative label B among its destinations, which leaves the vertices with a final label of exactly B
// unexpanded — and what lies behind them over zero-weight edges (final label B as well) unlabelled or too high.  A tight edge
// into a destination may come from just there.  Without a bound the rounds run to the fixpoint of everything reachable.
__global__ void k_lane_unbound(long long *__restrict__ bound) { bound[threadIdx.x] = 0x7FFFFFFFFFFFFFFFll; }

// The lane batches b0, b0 + bstride, ... < nb of a call, one lane per distinct source: plain rounds (every edge of a changed
// vertex; few changed vertices loop on the device) or light edges first (light_edges_first).
template <typename T, typename DT> class RelaxBatches : RelaxWorker {
public:
	RelaxBatches(const RelaxWorker &w, u32 U, bool light, const SettledBatch *settled = nullptr) : RelaxWorker(w), U(U), light(light), settled(settled) {}

	int run(int b0, int bstride) {
		if (!light && sizeof(DT) == 4) return fail(PGQ_ERR_HIP, "internal error: 4-byte labels outside the light-edges-first path");
		PGQ_TRY((prepare<T, DT>(1)));
		PGQ_TRY(priv->qflag.reserve(Vn * 4));
		PGQ_TRY(priv->counters.reserve(sizeof(Counters)));
		static_assert(sizeof(RelaxCounters) <= sizeof(Counters), "counter block too small");
		d_rc = reinterpret_cast<RelaxCounters *>(priv->counters.p);
		PGQ_HIP_TRY(hipMemsetAsync(priv->qflag.p, 0, Vn * 4, st));
		for (b = b0; b < nb; b += bstride) {
			lo = ws->h_bstart[b], hi = ws->h_bstart[b + 1];
			if (lo == hi) continue;
			PGQ_TRY(start_batch());
			for (;;) {
				if (!light && nq_now <= small_limit) {
					PGQ_TRY(small_rounds());
					if (nq_now == 0) break;
					if (nq_now <= small_limit && h_rc->rounds > 0) continue; // hit max_rounds: go again
				}
				PGQ_TRY(round());
				if (nq_now != 0) next_band();
				else if (light) PGQ_TRY(next_phase()); // (leaves nq_now at 0 when no heavier edge can matter)
				if (nq_now == 0) break;
			}
			PGQ_TRY(finish_batch());
		}
		return settle<T, DT>(1);
	}
private:
	const u32 U;
	const bool light;
	const SettledBatch *const settled; // null: the rows' costs (k_cheapest_results)
	RelaxSide &sd = priv->relax[0];
	RelaxCounters *d_rc = nullptr, *const h_rc = reinterpret_cast<RelaxCounters *>(priv->h_cnt); // priv's counter block, its pinned copy
	u32 epoch = 0; // queue-flag stamp of the device-side small rounds
	int par = 0;   // from here on: the batch's (start_batch)
	int64_t lo = 0, hi = 0, base = 0;
	u32 nq_now = 0, small_limit = 0;
	bool heavy = false;
	T band = T(0), thr_val = T(0), wcap = T(0);
	std::chrono::steady_clock::time_point t_round;

	int start_batch() {
		const Options &opt = options();
		S.batches++;
		base = (int64_t)b * LC;
		tepoch++;
		PGQ_HIP_TRY(hipMemsetAsync(d_rc, 0, sizeof(RelaxCounters), st));
		KernelTimer kt(st, K_PREP);
		hipLaunchKernelGGL(k_cheapest_init<DT>, dim3(1), dim3(64), 0, st, ws->usrc.as<int32_t>(), (int64_t)U, base, sd.dist.as<DT>(), sd.dirty[0].as<u64>(),
		                   sd.tflag.as<u32>(), tepoch, sd.touched.as<int32_t>(), &d_rc->nq[0], &d_rc->tcount, sd.q[0].as<int32_t>());
		kt.stop();
		par = 0;
		nq_now = (u32)std::min<int64_t>(LC, (int64_t)U - base);
		small_limit = (u32)std::max(0, opt.relax_small_limit);
		// band width of the ordered rounds: a fraction of the mean weight (0: plain Jacobi rounds, everything at once)
		band = T(0);
		if (opt.relax_delta_div > 0) {
			PGQ_TRY(ensure_weight_mean(c, ws));
			band = weight_fraction<T>(c->w_mean, opt.relax_delta_div);
		}
		thr_val = band;
		// "light edges first" (relax_light): the rounds run over weight-sorted lists under a cap on the edge weight that doubles
		// phase by phase — early phases touch a few per cent of the edges and give every lane a tight bound on its destinations,
		// later phases hardly relax anything (a vertex stops at the first edge whose weight cannot beat its lanes' bounds) — until
		// it reaches the largest bound.  `light`: cheapest_device has left the sorted lists and a positive finite mean on the handle.
		heavy = opt.relax_split != 0;
		t_round = std::chrono::steady_clock::now();
		wcap = light ? weight_fraction<T>(c->w_mean, std::max(1, opt.relax_light_div)) : T(0);
		return PGQ_OK;
	}
	// few changed vertices: rounds loop on the device inside one workgroup (8-byte labels only: labels_fit_32)
	int small_rounds() {
		KernelTimer kt(st, K_RELAX);
		hipLaunchKernelGGL(k_relax_small<T>, dim3(1), dim3(1024), 0, st, c->off, c->adj, (const T *)c->w, sd.dist.as<int64_t>(), sd.dirty[0].as<u64>(),
		                   sd.dirty[1].as<u64>(), sd.q[0].as<int32_t>(), sd.q[1].as<int32_t>(), d_rc, par, small_limit, priv->qflag.as<u32>(), epoch + 1,
		                   sd.tflag.as<u32>(), tepoch, sd.touched.as<int32_t>(), 4096); // (at most that many rounds per launch)
		kt.stop();
		PGQ_TRY(read_back(h_rc, d_rc, sizeof(RelaxCounters)));
		epoch += h_rc->rounds + 1;
		S.levels += h_rc->rounds;
		par ^= (int)(h_rc->rounds & 1u);
		nq_now = h_rc->nq[par];
		return PGQ_OK;
	}
	int round() {
		epoch++;
		// one launch instead of five fills per round (2459 rounds per 4096-pair step on the weighted knows graph)
		hipLaunchKernelGGL(k_round_reset, dim3(1), dim3(64), 0, st, d_rc, par ^ 1);
		const long long thr_bits = band > T(0) ? __builtin_bit_cast(long long, thr_val) : (long long)0x7FFFFFFFFFFFFFFFll;
		const RelaxRound<T> rr { priv, 0, par, c->off, light ? c->wadj : c->adj, light ? (const T *)c->wsorted : (const T *)c->w, tepoch, d_rc,
		                         thr_bits, light ? 1 : 0, wcap, heavy };
		KernelTimer kt(st, K_RELAX);
		if (settled) hipLaunchKernelGGL(k_lane_unbound, dim3(1), dim3(64), 0, st, d_rc->bound);
		else hipLaunchKernelGGL(k_lane_bounds<DT>, dim3((unsigned)std::min<int64_t>(blocks_for(hi - lo), 256)), dim3(256), 0, st, lo, hi,
		                        ws->skey.as<u32>(), ws->sdst.as<int32_t>(), (u32)base, sd.dist.as<DT>(), Inf<T>::bits, d_rc->bound);
		launch_relax<T, DT>(rr, 0, grid, nq_now);
		if (heavy) launch_relax<T, DT>(rr, 1, grid, nq_now); // the long lists of the round, a chunk per wavefront
		kt.stop();
		PGQ_TRY(read_back(h_rc, d_rc, sizeof(RelaxCounters)));
		if (trace) {
			const auto t1 = std::chrono::steady_clock::now();
			fprintf(stderr, "relax b=%d round=%lld cap=%g nq=%u expanded=%u heavy=%u/%u edges=%llu next=%u us=%.1f\n", b, (long long)S.levels,
			        (double)wcap, nq_now, h_rc->relaxed_vertices, (u32)(h_rc->heavy >> 32), (u32)h_rc->heavy,
			        (unsigned long long)h_rc->relaxed_edges, h_rc->nq[par ^ 1], std::chrono::duration<double, std::micro>(t1 - t_round).count());
			t_round = t1;
		}
		S.levels++;
		par ^= 1;
		nq_now = h_rc->nq[par];
		return PGQ_OK;
	}
	// The phase has reached its fixpoint.  Done when no heavier edge can matter: the cap has reached the largest bound of a
	// lane (the bounds of the last round: labels only got smaller since) or the largest weight.  Otherwise the cap doubles.
	int next_phase() {
		T max_bound = T(0);
		bool unbounded = false;
		for (const long long bits : h_rc->bound) {
			if (bits >= (long long)Inf<T>::bits) unbounded = true;
			if (__builtin_bit_cast(T, bits) > max_bound) max_bound = __builtin_bit_cast(T, bits);
		}
		// (negated comparisons: a cap that is NaN or inf ends the search like one that has reached the largest weight)
		if (!(wcap < __builtin_bit_cast(T, c->w_max_bits)) || (!unbounded && !(wcap < max_bound))) return PGQ_OK;
		if constexpr (std::is_same<T, double>::value) wcap = wcap + wcap;
		else wcap = wcap > std::numeric_limits<int64_t>::max() / 2 ? std::numeric_limits<int64_t>::max() : wcap + wcap;
		PGQ_HIP_TRY(hipMemsetAsync(&d_rc->nq[par], 0, 4, st));
		hipLaunchKernelGGL(k_redirty, dim3((unsigned)device_cus() * 4), dim3(256), 0, st, sd.touched.as<int32_t>(), &d_rc->tcount,
		                   sd.dirty[par].as<u64>(), sd.q[par].as<int32_t>(), &d_rc->nq[par]);
		PGQ_TRY(read_back(h_rc, d_rc, sizeof(RelaxCounters)));
		nq_now = h_rc->nq[par];
		return PGQ_OK;
	}
	void next_band() { // an empty band is skipped: straight to the smallest label left
		if (!(band > T(0))) return;
		thr_val = thr_val + band;
		if (h_rc->relaxed_vertices == 0 && h_rc->min_deferred != 0x7F7F7F7F7F7F7F7Fll)
			thr_val = std::max(thr_val, __builtin_bit_cast(T, h_rc->min_deferred) + band);
	}
	int finish_batch() {
		if (settled) PGQ_TRY(settled->then(lo, hi, base));
		else hipLaunchKernelGGL(k_cheapest_results<DT>, dim3(blocks_for(hi - lo)), dim3(256), 0, st, lo, hi, ws->skey.as<u32>(),
		                        ws->sidx.as<u32>(), ws->sdst.as<int32_t>(), (u32)base, sd.dist.as<DT>(), Inf<T>::bits, d_out, d_ok);
		end_batch<T, DT>(h_rc->relaxed_edges, 1, d_rc);
		return PGQ_OK;
	}
};

// ---- hop-bounded rounds: the cheapest walk of at most K edges (HopBatches) -----------------------------------------------
// pgq_cheapest_path_length_within answers, per row (src, dst), D_K[dst] of
//     D_0[src] = 0, D_0[v] = INF otherwise;   D_k[n] = min(D_{k-1}[n], min over edges (u, n) of D_{k-1}[u] + w(u, n))
// where the sum is the reference's `dist[v] + w` (cheapest_path_length.cpp:29-36) and counts only where it is < D_{k-1}[n]
// (so a sum that does not get under INF = max / 2 never labels a vertex); NULL when D_K[dst] == INF.  The reference has NO
// counterpart: its Bellman-Ford sweeps in place, so its rounds are not hops, and neither are k_relax's or k_relax_small's —
// a vertex expanded late in a launch may carry a label an earlier wavefront of the same launch improved, labels travel
// several edges per round (the order-independence the file's header relies on).  The result is NOT "the unbounded answer with
// far rows set to NULL" either: the cheapest walk of at most K edges is in general another walk than the cheapest one, and
// costs more.  A bound needs a round that moves every label by exactly ONE edge: two launches.
//   k_hop_snapshot  one wavefront per queue entry i: takes the dirty word of the queue's vertex v with an exchange and copies
//                   v's 512-byte label row into snap[i][0..63], the word into snapmask[i].  Behind this launch `snap` holds
//                   D_{k-1} of every vertex that changed in round k-1, frozen.
//   k_relax_hops    a persistent grid; wavefronts stride over the queue, lane l = search l.  A wavefront reads v, snapmask[i]
//                   and its lane's snap[i][l] — never dist[v] — and walks v's whole out-list eight edges per dependent trip
//                   (k_relax's plain, unsorted path): lanes whose mask bit is set atomicMin snap + w into dist[n][l].
// Exact per round: the sources of a relaxation come only from `snap` (D_{k-1}), the targets are only `dist`, so no label
// written in round k is read in round k; a lane whose label at v did not change in round k-1 made its offers the round after
// it last changed and has nothing new, so only dirty lanes relax.  The plain pre-check load of dist[n][l] may be stale-high
// within a launch (another wavefront's atomic): that costs an atomic and never an answer, the atomicMin decides.  All
// freshness comes from kernel boundaries: no fence, no agent-scope load, no round loop inside a kernel.
// Exact per walk (what makes the result the reference's arithmetic, bit for bit, for int64 and for double):
//   claim      D_k[n] = the minimum, over the walks src -> n of at most k edges, of the left-to-right fold of their weights.
//   k = 0      the empty walk at src folds to 0; no other vertex has a walk.
//   k-1 -> k   a walk of <= k edges into n is a walk P of <= k-1 edges into some u plus an edge (u, n), fold(P) + w.  For a
//              fixed non-negative w, x -> x + w is monotone (IEEE round-to-nearest as well as int64), so the minimum over P of
//              fold(P) + w is (min over P of fold(P)) + w = D_{k-1}[u] + w: the recurrence above.
// NaN and +inf weights never relax an edge, -0.0 is accepted: as in k_relax.  K >= V - 1 is the unbounded search (a cheapest
// walk needs no repeated vertex under non-negative weights) and takes the unbounded drivers.
// Known limits: lists over 128 edges are walked by the wavefront that finds them (correct, only slow: no heavy-list split
// here yet), and there is no destination-bound pruning — a lane relaxes everything within K edges of its source.
//
// With a lower bound (pgq_cheapest_walk_length, lo = min_hops >= 1): the cheapest walk of lo .. K edges.  Rounds 1 .. lo are EXACT,
//     E_0 = D_0;   E_t[x] = min over the in-slots (u, x) with E_{t-1}[u] < INF of E_{t-1}[u] + w   (INF if none: E_{t-1}[x] is NOT carried)
//     L_lo = E_lo; L_t[x] = min(L_{t-1}[x], min over the in-slots (u, x) of L_{t-1}[u] + w),  t = lo + 1 .. K  (the recurrence above)
// and the row's answer is L_K[dst].  An exact round is the round above with ONE difference: k_hop_snapshot TAKES the row — behind
// the copy to `snap` and the exchange of the dirty word it writes INF into all 64 lanes of dist[v] (`take`, by value: the host
// knows hop < lo when it enqueues the launch, so groups of rounds are enqueued ahead as ever and may span the phase boundary).
//   invariant   before exact round t, every label below INF was written by an improving atomicMin of round t-1 (or is the
//               source's 0 of k_cheapest_init): its vertex is queued and its lane's bit is in the dirty word.  True at t = 1; the
//               take launch of round t then leaves dist at INF EVERYWHERE (it takes every queued row, whole), the round's atomicMins
//               build E_t from snap = E_{t-1} into it, and each label they leave was an improvement over INF or over a larger offer
//               of the same round — queued, bit set: the invariant at t + 1.  The dirty bits of the next parity are exactly the
//               finite lanes of E_t, so k_relax_hops's "only dirty lanes relax" loses nothing, and the kernel is unchanged.
//   claim       E_t[x] = the minimum, over the walks src -> x of EXACTLY t edges, of the left-to-right fold of their weights:
//               t = 0 as above; a walk of t edges into x is a walk P of t-1 edges into some u plus a slot (u, x), and by the
//               monotonicity of x -> x + w the minimum over P of fold(P) + w is E_{t-1}[u] + w.  (A sum that does not get under
//               INF labels nothing, as above.)  Then L_t[x] = the minimum over the walks of lo .. t edges, by the k-1 -> k step
//               above started from L_lo = E_lo instead of D_0 — bit for bit, for int64 and for double.
// Take and relax stay two launches: with a self-loop or a ring a vertex is source and target of one round, and only the kernel
// boundary puts every take before every atomicMin.  Taken vertices stay on the touched list (k_reset_touched and the "stopped
// at the bound" memset cover them like any other).  src == dst is no special row here: it takes a lane (prepare_lanes'
// closed_rows) and is answered by its cheapest closed walk; the rows that stay trivial there — no out-edge or no in-edge — are NULL.
// A lower bound takes these rounds for EVERY K, K >= V - 1 included: phase 2 is Bellman-Ford from E_lo, stands still after at
// most V - 1 rounds and ends with the queue.  lo is capped (PGQ_WALK_MAX_HOPS): in a cyclic graph the exact phase never runs dry.
template <typename DT>
__global__ __launch_bounds__(256) void k_hop_snapshot(const int32_t *__restrict__ qcur, const u32 *__restrict__ nq_ptr,
                                                      u64 *__restrict__ dirty_cur, DT *__restrict__ dist,
                                                      DT *__restrict__ snap, u64 *__restrict__ snapmask, u32 *__restrict__ snap_rows,
                                                      int take, DT inf_bits, u32 *__restrict__ take_rows) {
	const int lane = threadIdx.x & 63;
	const u32 wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
	const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
	const u32 nq = *nq_ptr;
	for (u32 i = wave; i < nq; i += nwaves) {
		const int v = qcur[i];
		snap[(size_t)i * LC + lane] = dist[(size_t)v * LC + lane];
		if (lane == 0) snapmask[i] = atomicExch(&dirty_cur[v], 0ull); // consumed: the word is clean for the round after next
		if (take) dist[(size_t)v * LC + lane] = inf_bits; // an exact round: the row is TAKEN, nothing of E_{t-1} is carried into E_t
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		*snap_rows += nq; // (statistics; the batch's launches never overlap)
		if (take) *take_rows += nq;
	}
}

template <typename T>
__global__ __launch_bounds__(256, PGQ_RELAX_WAVES) void k_relax_hops(const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                    const T *__restrict__ w, int64_t *__restrict__ dist,
                                                    const int64_t *__restrict__ snap, const u64 *__restrict__ snapmask,
                                                    u64 *__restrict__ dirty_nxt, const int32_t *__restrict__ qcur,
                                                    const u32 *__restrict__ nq_ptr, int32_t *__restrict__ qnxt, u32 *__restrict__ nq_nxt,
                                                    u32 *__restrict__ tflag, u32 tepoch, int32_t *__restrict__ touched,
                                                    u32 *__restrict__ tcount, u64 *__restrict__ relaxed_edges, u32 *__restrict__ rounds) {
	constexpr int UNR = kRelaxUnroll;
	__shared__ int s_pq[4][kPendCap];
	__shared__ int s_pt[4][kPendCap];
	__shared__ u64 s_edges; // the workgroup's counters go through LDS first, like k_relax's
	__shared__ int s_pend[2][4];
	__shared__ u32 s_base[2];
	if (threadIdx.x == 0) s_edges = 0;
	__syncthreads();
	const int lane = threadIdx.x & 63;
	const int wib = threadIdx.x >> 6;
	const u32 wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
	const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
	const u32 nq = *nq_ptr;
	u64 edges = 0;
	int pend_q = 0, pend_t = 0; // wave-uniform
	int *const pq = s_pq[wib];
	int *const pt = s_pt[wib];
	for (u32 i = wave; i < nq; i += nwaves) {
		const int v = qcur[i];
		const bool mine = (snapmask[i] >> lane) & 1ull; // the lane's label at v changed in the previous round (so it is below INF)
		const u64 dvb = (u64)snap[(size_t)i * LC + lane];
		const int64_t b = off[v], e = off[v + 1];
		edges += (u64)(e - b);
		for (int64_t k0 = b; k0 < e; k0 += UNR) {
			int nn[UNR];
			T ww[UNR];
			u64 cand[UNR], curv[UNR];
#pragma unroll
			for (int u = 0; u < UNR; u++) {
				const bool in = k0 + u < e;
				nn[u] = in ? adj[k0 + u] : v;
				ww[u] = in ? w[k0 + u] : T(0);
				// labels are compared as bit patterns; a NaN weight never relaxes an edge in the reference, +inf behaves the same here
				if constexpr (std::is_same<T, double>::value) ww[u] = ww[u] == ww[u] ? ww[u] : __longlong_as_double(0x7FF0000000000000ll);
			}
#pragma unroll
			for (int u = 0; u < UNR; u++) {
				// labels and weights are non-negative: the int64 sum cannot wrap as an unsigned one, a double's bits order like its value
				if constexpr (std::is_same<T, double>::value) cand[u] = (u64)__double_as_longlong(__longlong_as_double((long long)dvb) + ww[u]);
				else cand[u] = dvb + (u64)ww[u];
				curv[u] = (u64)dist[(size_t)nn[u] * LC + lane]; // all eight rows in flight together; <= INF, possibly stale-high
			}
#pragma unroll
			for (int u = 0; u < UNR; u++) {
				const bool go = k0 + u < e && mine && cand[u] < curv[u]; // (then cand < INF: it fits the signed atomic)
				curv[u] = cand[u]; // "not improved" unless the atomic says otherwise
				if (go) curv[u] = (u64)atomicMin((long long *)&dist[(size_t)nn[u] * LC + lane], (long long)cand[u]);
			}
			u64 my_im = 0;
			int my_n = 0;
#pragma unroll
			for (int u = 0; u < UNR; u++) {
				const u64 im = __ballot(cand[u] < curv[u]);
				if (lane == u) {
					my_im = im;
					my_n = nn[u];
				}
			}
			if (!__any(my_im != 0)) continue;
			bool fresh_q = false, fresh_t = false;
			if (my_im) { // lanes 0..7, one improved neighbour each: dirty in the NEXT parity's word, queued on its 0 -> non-zero transition
				fresh_q = atomicOr(&dirty_nxt[my_n], my_im) == 0ull;
				fresh_t = tflag[my_n] != tepoch && atomicExch(&tflag[my_n], tepoch) != tepoch;
			}
			relax_append(pq, pend_q, fresh_q, my_n, qnxt, nq_nxt, lane);
			relax_append(pt, pend_t, fresh_t, my_n, touched, tcount, lane);
		}
	}
	if (lane == 0) {
		if (edges) atomicAdd(&s_edges, edges);
		s_pend[0][wib] = pend_q;
		s_pend[1][wib] = pend_t;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		const u32 tq = (u32)(s_pend[0][0] + s_pend[0][1] + s_pend[0][2] + s_pend[0][3]);
		const u32 tt = (u32)(s_pend[1][0] + s_pend[1][1] + s_pend[1][2] + s_pend[1][3]);
		s_base[0] = tq ? atomicAdd(nq_nxt, tq) : 0u;
		s_base[1] = tt ? atomicAdd(tcount, tt) : 0u;
		if (s_edges) atomicAdd(relaxed_edges, s_edges);
		if (blockIdx.x == 0 && nq) *rounds += 1; // a round enqueued behind an empty queue is none
	}
	__syncthreads();
	u32 oq = s_base[0], ot = s_base[1];
	for (int k = 0; k < wib; k++) {
		oq += (u32)s_pend[0][k];
		ot += (u32)s_pend[1][k];
	}
	if (lane < pend_q) qnxt[oq + lane] = pq[lane];
	if (lane < pend_t) touched[ot + lane] = pt[lane];
}

template <typename T> static int hop_grid(unsigned *grid) { // relax_grid for k_relax_hops
	static unsigned cached[64] = {};
	return resident_grid(k_relax_hops<T>, cached, grid);
}

// The lane batches b0, b0 + bstride, ... < nb of a bounded call, one lane per distinct source like RelaxBatches: each batch
// runs min(K, rounds until its queue is empty) rounds of the two launches above.  Rounds are enqueued in groups of up to
// kHopGroup without a host wait — the kernels read the queue's fill on the device, k_round_reset clears the next one, a
// round behind an empty queue does nothing — and the counter block comes back once per group.  `snap` and `snapmask`
// live in the worker's second RelaxSide (labels, first dirty array), whose labels a later two-ended call must not trust.
// With a HopLog (pgq_relax.h) the snapshot rows of every round are kept instead, by the hook, and a batch ends in its `then`.
template <typename T> class HopBatches : RelaxWorker {
	using DT = int64_t; // 8-byte labels only
	static constexpr int kHopGroup = 8;
public:
	HopBatches(const RelaxWorker &w, u32 U, int64_t lower, int64_t K, const HopLog *log = nullptr) : RelaxWorker(w), U(U), lower(lower), K(K), log(log) {}

	int run(int b0, int bstride) {
		PGQ_TRY(sd.prepare<DT>(V, relax_label_tag<T, DT>(), (DT)Inf<T>::bits, st));
		sn.dist_V = -1; // (stays so: what is left here is no label array)
		if (!log) {
			PGQ_TRY(sn.dist.reserve(Vn * LC * sizeof(DT)));
			PGQ_TRY(sn.dirty[0].reserve(Vn * 8));
		}
		PGQ_TRY(hop_grid<T>(&grid));
		PGQ_TRY(priv->counters.reserve(sizeof(Counters)));
		d_rc = reinterpret_cast<RelaxCounters *>(priv->counters.p);
		for (b = b0; b < nb; b += bstride) {
			lo = ws->h_bstart[b], hi = ws->h_bstart[b + 1];
			if (lo == hi) continue;
			PGQ_TRY(start_batch());
			const int group = log ? 1 : kHopGroup;
			for (int64_t done = 0; done < K && nq_now != 0; done += group) PGQ_TRY(round_group((int)std::min<int64_t>(group, K - done)));
			PGQ_TRY(finish_batch());
		}
		return settle<T, DT>(1);
	}
private:
	const u32 U;
	const int64_t lower, K; // rounds 1 .. lower are exact (they take), the rounds behind them carry over
	const HopLog *const log; // null: the rows' costs (k_cheapest_results)
	RelaxSide &sd = priv->relax[0], &sn = priv->relax[1];
	RelaxCounters *d_rc = nullptr, *const h_rc = reinterpret_cast<RelaxCounters *>(priv->h_cnt);
	int par = 0; // from here on: the batch's (start_batch)
	int64_t lo = 0, hi = 0, base = 0, hop = 0; // hop: the rounds enqueued so far
	u32 nq_now = 0, rounds_seen = 0, snap_seen = 0, take_seen = 0;
	u64 edges = 0;

	int start_batch() {
		S.batches++;
		base = (int64_t)b * LC;
		tepoch++;
		PGQ_HIP_TRY(hipMemsetAsync(d_rc, 0, sizeof(RelaxCounters), st));
		KernelTimer kt(st, K_PREP);
		hipLaunchKernelGGL(k_cheapest_init<DT>, dim3(1), dim3(64), 0, st, ws->usrc.as<int32_t>(), (int64_t)U, base, sd.dist.as<DT>(), sd.dirty[0].as<u64>(),
		                   sd.tflag.as<u32>(), tepoch, sd.touched.as<int32_t>(), &d_rc->nq[0], &d_rc->tcount, sd.q[0].as<int32_t>());
		kt.stop();
		par = 0;
		nq_now = (u32)std::min<int64_t>(LC, (int64_t)U - base);
		rounds_seen = snap_seen = take_seen = 0;
		edges = 0;
		hop = 0;
		return PGQ_OK;
	}
	int round_group(int rounds) {
		for (int r = 0; r < rounds; r++, par ^= 1, hop++) {
			hipLaunchKernelGGL(k_round_reset, dim3(1), dim3(64), 0, st, d_rc, par ^ 1);
			// the group's first round knows its queue's fill; the others size their grids for a full one
			const unsigned g = r == 0 ? std::min(grid, std::max(1u, (nq_now + 3) / 4)) : grid;
			const int64_t *snap = sn.dist.as<DT>();
			const u64 *snapmask = sn.dirty[0].as<u64>();
			const bool take = hop < lower; // known here, handed over by value: a group may span the phase boundary
			if (log) PGQ_TRY(log->append(par, nq_now, hop, take, &snap, &snapmask)); // (a group of one round: nq_now is this round's)
			KernelTimer kt(st, K_RELAX);
			if (!log)
				hipLaunchKernelGGL(k_hop_snapshot<DT>, dim3(g), dim3(256), 0, st, sd.q[par].as<int32_t>(), &d_rc->nq[par], sd.dirty[par].as<u64>(), sd.dist.as<DT>(),
				                   sn.dist.as<DT>(), sn.dirty[0].as<u64>(), &d_rc->snap_rows, take ? 1 : 0, (DT)Inf<T>::bits, &d_rc->take_rows);
			hipLaunchKernelGGL(k_relax_hops<T>, dim3(g), dim3(256), 0, st, c->off, c->adj, (const T *)c->w, sd.dist.as<DT>(), snap,
			                   snapmask, sd.dirty[par ^ 1].as<u64>(), sd.q[par].as<int32_t>(), &d_rc->nq[par], sd.q[par ^ 1].as<int32_t>(),
			                   &d_rc->nq[par ^ 1], sd.tflag.as<u32>(), tepoch, sd.touched.as<int32_t>(), &d_rc->tcount, &d_rc->relaxed_edges, &d_rc->rounds);
			kt.stop();
		}
		PGQ_TRY(read_back(h_rc, d_rc, sizeof(RelaxCounters)));
		if (trace)
			fprintf(stderr, "hops b=%d rounds=%u edges=%llu next=%u\n", b, h_rc->rounds, (unsigned long long)h_rc->relaxed_edges, h_rc->nq[par]);
		// the block's counters run on over the batch: what this group added
		S.levels += h_rc->rounds - rounds_seen;
		S.algo_bytes[K_RELAX] += (double)(h_rc->snap_rows - snap_seen) * (2.0 * sizeof(DT) * LC + 16.0); // a row read and written, the dirty word exchanged, the mask written
		S.algo_bytes[K_RELAX] += (double)(h_rc->take_rows - take_seen) * (double)(sizeof(DT) * LC); // the row a take writes back as INF
		rounds_seen = h_rc->rounds;
		snap_seen = h_rc->snap_rows;
		take_seen = h_rc->take_rows;
		edges = h_rc->relaxed_edges;
		nq_now = h_rc->nq[par];
		return PGQ_OK;
	}
	int finish_batch() {
		if (log) { // the vertices the last round changed are logged too, which takes their dirty words: nothing is left queued
			const int64_t *snap = nullptr;
			const u64 *snapmask = nullptr;
			if (nq_now != 0) PGQ_TRY(log->append(par, nq_now, hop, false, &snap, &snapmask)); // (hop >= lower here, or the queue is empty)
			PGQ_TRY(log->then(lo, hi, base));
			end_batch<T, DT>(edges, 1, d_rc);
			return PGQ_OK;
		}
		hipLaunchKernelGGL(k_cheapest_results<DT>, dim3(blocks_for(hi - lo)), dim3(256), 0, st, lo, hi, ws->skey.as<u32>(),
		                   ws->sidx.as<u32>(), ws->sdst.as<int32_t>(), (u32)base, sd.dist.as<DT>(), Inf<T>::bits, d_out, d_ok);
		end_batch<T, DT>(edges, 1, d_rc);
		// stopped at the bound with vertices still queued: their dirty words go back to zero for the next batch
		if (nq_now != 0) PGQ_HIP_TRY(hipMemsetAsync(sd.dirty[par].p, 0, Vn * 8, st));
		return PGQ_OK;
	}
};

// ---- general graphs, about one destination per source: both ends at once (BidirBatches, round 6) ------------------
// The batched relaxation above gives a lane the distances from its source to EVERY vertex under the lane's bound: on the
// weighted knows graph (weights 1..999, mean degree 89) that is most of the graph per source, ~14 expansions per vertex and
// batch — 0.64 s per 4096 pairs, `k_relax` 94 % of it.  A single pair needs the ball of half the distance around each end:
// balls grow by e^(0.089 r) there, so two of radius D / 2 hold a few hundred settled vertices where one of radius D holds
// most of V.  Here a lane is one (src, dst) PAIR and a batch runs the same kernel from both ends — forward over the
// weight-sorted out-lists into `dist`, backward over the weight-sorted in-lists into the backward side's labels (Workspace::relax[1]):
//     mu[l]  = the best src -> dst length seen (the bound BOTH sides prune with; INF at first)
//     a round = k_relax forward, then k_relax backward, each expanding what is dirty with a label below the common cap C
//               (the kernel's threshold, read from the device) and below mu[l], labelling what gets under min(mu[l], 2 C) —
//               an expansion walks the few edges under 2 C - label, not its list; a vertex expanded on one side that carries
//               a label of the other side offers mu[l] = label + other label
//     a phase ends with a round in which neither side expanded anything (both at their fixpoint under C): a lane is finished
//               when mu[l] < 2 C, or when one of its sides has neither a labelled vertex left over the cap nor an edge the
//               cap cut (closure exhausted); then C rises — by a step, by a quarter, and past empty bands to the smallest
//               label left — and every labelled vertex is expanded again (k_redirty: the longer prefix of its list)
// Exactness (int64 sums, any order).  At a phase end every vertex with d(src, x) < min(C, mu) carries its exact forward
// label and has been expanded with it, likewise backward.  Let D < 2 C be the distance and x the last vertex of an optimal
// path with d(src, x) < C, y its successor: d(src, y) >= C, so d(y, dst) = D - d(src, y) < C, and both labels the two
// offer each other — d(src, x) + w forward on y, w + d(y, dst) backward on x — are at most D < 2 C: not cut.  The later of "x expanded
// forward for the last time" / "y expanded backward for the last time" reads the other's final label — x finds db[x] <=
// w + d(y, dst), or y finds df[y] <= d(src, x) + w — and offers D (launches of one batch never overlap, so one of the two
// IS later).  Hence mu < 2 C implies D <= mu < 2 C implies mu = D.  A side that has nothing labelled left below mu has
// expanded its whole closure below mu: were D < mu, dst (src) itself would have been expanded there and offered D.
// int64 weights only: a double's sum depends on the order of its additions (cheapest_path_length.cpp:29-36 folds from the
// source), so doubles keep the one-sided relaxation above.
// MEASURED (round 6, weighted knows graph, 512 pairs): 232 ms against 89 ms one-sided, so `relax_bidir` ships OFF.  That
// graph has no small balls: its hubs (1800 edges) sit within half a typical distance (D ~ 60..230, median 95) of nearly
// every vertex, a batch of 64 pairs relaxes 30 M edges from both ends against 40 M one-sided — and pays 83 rounds
// (9 phases of caps 15, 22, 29, 36, 45, 56, 70, 87, 108, each re-expanding what is labelled) instead of 35, every one of
// them a rescan of ~400 K labelled vertices per side.  Both variants move a 64-lane label row per relaxed edge for the
// one or two lanes that need it; that row traffic, not the number of edges, is what a round costs.  On
// graphs whose balls stay small (bounded degree, road-like) the two-ended search is the cheaper one; kept, tested, optional.

template <typename DT>
__global__ __launch_bounds__(64) void k_bidir_init(int64_t lo, int nl, const int32_t *__restrict__ ssrc, const int32_t *__restrict__ sdst,
                                                   DT *__restrict__ dist_f, DT *__restrict__ dist_b, u64 *__restrict__ dirty_f,
                                                   u64 *__restrict__ dirty_b, u32 *__restrict__ tflag_f, u32 *__restrict__ tflag_b, u32 tepoch,
                                                   int32_t *__restrict__ touched_f, int32_t *__restrict__ touched_b,
                                                   int32_t *__restrict__ q_f, int32_t *__restrict__ q_b, BiBlock *__restrict__ bb,
                                                   long long cap0, long long step, long long inf) {
	const int t = threadIdx.x; // the block arrives zeroed
	bb->res[t] = inf;
	if (t < nl) {
		const int s = ssrc[lo + t], d = sdst[lo + t]; // s != d (trivial rows sort behind the lanes); several lanes may share an endpoint
		bb->mu[t] = inf;
		dist_f[(size_t)s * LC + t] = 0;
		if (atomicOr(&dirty_f[s], 1ull << t) == 0ull) q_f[atomicAdd(&bb->rc[0].nq[0], 1u)] = s;
		if (atomicExch(&tflag_f[s], tepoch) != tepoch) touched_f[atomicAdd(&bb->rc[0].tcount, 1u)] = s;
		dist_b[(size_t)d * LC + t] = 0;
		if (atomicOr(&dirty_b[d], 1ull << t) == 0ull) q_b[atomicAdd(&bb->rc[1].nq[0], 1u)] = d;
		if (atomicExch(&tflag_b[d], tepoch) != tepoch) touched_b[atomicAdd(&bb->rc[1].tcount, 1u)] = d;
	} else {
		bb->done[t] = 1; // no pair on this lane: bound 0, nothing is ever expanded for it
	}
	if (t == 0) {
		bb->cap = cap0;
		bb->step = step;
		bb->active = (u32)nl;
	}
}

__global__ __launch_bounds__(64) void k_bidir_round_reset(BiBlock *__restrict__ bb, int next_f, int next_b) {
	const int t = threadIdx.x;
	if (t < 2) {
		RelaxCounters *rc = &bb->rc[t];
		rc->nq[t == 0 ? next_f : next_b] = 0;
		rc->relaxed_vertices = 0;
		rc->min_deferred = 0x7F7F7F7F7F7F7F7Fll;
		rc->heavy = 0;
	}
}

// after the two sides' launches of a round (see the header above)
__global__ __launch_bounds__(64) void k_bidir_phase_end(BiBlock *__restrict__ bb) {
	const int t = threadIdx.x;
	const bool fix = bb->rc[0].relaxed_vertices == 0 && bb->rc[1].relaxed_vertices == 0;
	const long long C = bb->cap;
	if (fix && !bb->done[t]) {
		const long long m = bb->mu[t];
		if (m < 2 * C || !bb->alive[0][t] || !bb->alive[1][t]) {
			bb->res[t] = m;
			bb->mu[t] = 0; // the lane's bound: nothing of it is expanded or labelled any more
			bb->done[t] = 1;
		}
	}
	if (fix) { // the flags gather over a phase's rounds (an edge is cut in the round its vertex is expanded)
		bb->alive[0][t] = 0;
		bb->alive[1][t] = 0;
	}
	const u64 open = __ballot(!bb->done[t]);
	if (t == 0) {
		bb->active = (u32)__popcll(open);
		if (fix) {
			const long long md = min(bb->rc[0].min_deferred, bb->rc[1].min_deferred);
			long long nc = max(C + bb->step, C + C / 4);
			if (md != 0x7F7F7F7F7F7F7F7Fll && md + 1 > nc) nc = md + 1; // an empty band: straight to the smallest label left
			bb->cap = nc;
			bb->phases++;
		}
	}
}

__global__ __launch_bounds__(64) void k_bidir_results(int64_t lo, int nl, const u32 *__restrict__ sidx, const BiBlock *__restrict__ bb,
                                                      long long inf, int64_t *__restrict__ out, uint8_t *__restrict__ ok) {
	const int t = threadIdx.x;
	if (t >= nl) return;
	const u32 row = sidx[lo + t];
	const long long d = bb->res[t];
	ok[row] = d == inf ? 0 : 1;
	out[row] = d == inf ? 0 : d;
}

static std::mutex g_rws_lock;
// the in-lists sorted by weight (radj / rw -> rwadj / rwsorted), once per CSR: ensure_weight_sorted for the other direction
static int ensure_reverse_sorted(pgq_csr *c, Workspace *ws) {
	PGQ_TRY(ensure_reverse_weights(c, ws));
	std::lock_guard<std::mutex> g(g_rws_lock);
	if (c->rwadj || c->E == 0 || !c->rw) return PGQ_OK;
	hipStream_t st = ws->stream;
	const int64_t E = c->E;
	DevTemps temps(st);
	int32_t *rwadj = nullptr;
	void *rwsorted = nullptr;
	PGQ_TRY(temps.alloc_bytes((void **)&rwadj, csr_bytes(c, c->rwadj)));
	PGQ_TRY(temps.alloc_bytes(&rwsorted, csr_bytes(c, c->rwsorted)));
	const unsigned long long *keys = (const unsigned long long *)c->rw; // int64 weights >= 0: the bit pattern is the value
	PGQ_TRY(cub_run(temps, [&](void *tmp, size_t &tb) {
		return hipcub::DeviceSegmentedRadixSort::SortPairs(tmp, tb, keys, (unsigned long long *)rwsorted, c->radj, rwadj, (int)E, (int)c->V, c->roff,
		                                                   c->roff + 1, 0, 64, st);
	}));
	PGQ_HIP_TRY(hipStreamSynchronize(st));
	temps.keep(rwadj);
	temps.keep(rwsorted);
	c->rwsorted = rwsorted;
	c->rwadj = rwadj;
	return PGQ_OK;
}

// The pair batches b0, b0 + bstride, ... < nb of a call: batch b = the sorted rows [64 b, 64 b + 64) of the R rows that need a
// search (`ws`: sorted rows, read-only; `priv`: everything a batch writes, and the stream — like RelaxBatches).
template <typename DT> class BidirBatches : RelaxWorker {
	using T = int64_t;
public:
	BidirBatches(const RelaxWorker &w, int64_t R) : RelaxWorker(w), R(R) {}

	int run(int b0, int bstride) {
		PGQ_TRY((prepare<T, DT>(2)));
		PGQ_TRY(priv->bi_block.reserve(sizeof(BiBlock)));
		if (!priv->h_bi) PGQ_HIP_TRY(hipHostMalloc(&priv->h_bi, sizeof(BiBlock)));
		bb = priv->bi_block.as<BiBlock>();
		hb = static_cast<const BiBlock *>(priv->h_bi);
		for (b = b0; b < nb; b += bstride) {
			lo = (int64_t)b * LC;
			nl = (int)std::min<int64_t>(LC, R - lo);
			if (nl <= 0) continue;
			PGQ_TRY(start_batch());
			for (int64_t r = 0;; r++) {
				if (r > (int64_t)1 << 22) return fail(PGQ_ERR_HIP, "internal error: the bidirectional relaxation does not terminate");
				PGQ_TRY(round(r));
				if (hb->active == 0) break;
				if (hb->phases != phases_seen) redirty_sides();
			}
			PGQ_TRY(finish_batch());
		}
		return settle<T, DT>(2);
	}
private:
	const int64_t R;
	// (the mean of a shortest path's edges is far below the mean weight: the caps are fractions of twice the mean)
	const long long cap0 = weight_fraction<T>(2.0 * c->w_mean, std::max(1, options().relax_bidir_c0_div));
	const long long step = weight_fraction<T>(2.0 * c->w_mean, std::max(1, options().relax_bidir_step_div));
	RelaxSide *const side = priv->relax;
	BiBlock *bb = nullptr;       // both sides' counters, the pairs' bounds and answers, the cap
	const BiBlock *hb = nullptr; // ... and its pinned copy of the last round
	int nl = 0, par[2] = { 0, 0 }; // from here on: the batch's (start_batch)
	int64_t lo = 0;
	u32 nq[2] = { 0, 0 }, phases_seen = 0;

	int start_batch() {
		S.batches++;
		tepoch++;
		PGQ_HIP_TRY(hipMemsetAsync(bb, 0, sizeof(BiBlock), st));
		KernelTimer kt(st, K_PREP);
		hipLaunchKernelGGL(k_bidir_init<DT>, dim3(1), dim3(64), 0, st, lo, nl, ws->ssrc.as<int32_t>(), ws->sdst.as<int32_t>(), side[0].dist.as<DT>(),
		                   side[1].dist.as<DT>(), side[0].dirty[0].as<u64>(), side[1].dirty[0].as<u64>(), side[0].tflag.as<u32>(), side[1].tflag.as<u32>(), tepoch,
		                   side[0].touched.as<int32_t>(), side[1].touched.as<int32_t>(), side[0].q[0].as<int32_t>(), side[1].q[0].as<int32_t>(), bb, cap0, step, (long long)Inf<T>::bits);
		kt.stop();
		par[0] = par[1] = 0;
		nq[0] = nq[1] = (u32)nl;
		phases_seen = 0;
		return PGQ_OK;
	}
	// k_relax forward, then backward, each with its heavy pass; then the phase's book-keeping on the device
	int round(int64_t r) {
		hipLaunchKernelGGL(k_bidir_round_reset, dim3(1), dim3(64), 0, st, bb, par[0] ^ 1, par[1] ^ 1);
		KernelTimer kt(st, K_RELAX);
		for (int s = 0; s < 2; s++) {
			if (nq[s] == 0) continue;
			// forward over the weight-sorted out-lists, backward over the weight-sorted in-lists
			const RelaxRound<T> rr { priv, s, par[s], s ? c->roff : c->off, s ? c->rwadj : c->wadj, (const T *)(s ? c->rwsorted : c->wsorted),
			                         tepoch, &bb->rc[s], 0, 1, std::numeric_limits<T>::max(), true, bb };
			for (int hp = 0; hp < 2; hp++) launch_relax<T, DT>(rr, hp, grid, nq[s]);
		}
		hipLaunchKernelGGL(k_bidir_phase_end, dim3(1), dim3(64), 0, st, bb);
		kt.stop();
		PGQ_TRY(read_back(priv->h_bi, bb, sizeof(BiBlock)));
		S.levels++;
		if (trace)
			fprintf(stderr, "bidir b=%d round=%lld cap=%lld phases=%u nq=%u/%u expanded=%u/%u next=%u/%u active=%u edges=%llu/%llu\n", b, (long long)r,
			        hb->cap, hb->phases, nq[0], nq[1], hb->rc[0].relaxed_vertices, hb->rc[1].relaxed_vertices, hb->rc[0].nq[par[0] ^ 1],
			        hb->rc[1].nq[par[1] ^ 1], hb->active, (unsigned long long)hb->rc[0].relaxed_edges, (unsigned long long)hb->rc[1].relaxed_edges);
		for (int s = 0; s < 2; s++) {
			if (nq[s] == 0) continue; // (nothing was launched: the side's queues and parity stay as they are)
			par[s] ^= 1;
			nq[s] = hb->rc[s].nq[par[s]];
		}
		return PGQ_OK;
	}
	void redirty_sides() { // a higher cap: every labelled vertex again, over the longer prefix of its list
		phases_seen = hb->phases;
		for (int s = 0; s < 2; s++) {
			hipLaunchKernelGGL(k_redirty, dim3((unsigned)device_cus() * 4), dim3(256), 0, st, side[s].touched.as<int32_t>(), &bb->rc[s].tcount,
			                   side[s].dirty[par[s]].as<u64>(), side[s].q[par[s]].as<int32_t>(), &bb->rc[s].nq[par[s]]);
			nq[s] = hb->rc[s].tcount;
		}
	}
	int finish_batch() {
		hipLaunchKernelGGL(k_bidir_results, dim3(1), dim3(64), 0, st, lo, nl, ws->sidx.as<u32>(), bb, (long long)Inf<T>::bits, d_out, d_ok);
		end_batch<T, DT>(hb->rc[0].relaxed_edges + hb->rc[1].relaxed_edges, 2, bb->rc);
		for (int s = 0; s < 2; s++) // what the finished lanes left dirty: the next batch starts from clean words
			for (DevBuf &d : side[s].dirty) PGQ_HIP_TRY(hipMemsetAsync(d.p, 0, Vn * 8, st));
		return PGQ_OK;
	}
};

// max_hops: negative = unbounded.  A bound of V - 1 or more IS the unbounded search (a cheapest walk repeats no vertex under
// non-negative weights) and takes its drivers; a smaller one takes HopBatches alone — no chain pre-pass, no k_wbibfs, no
// light-edges-first lists, no two-ended batches, no 4-byte labels: none of them knows hops.
template <typename T>
static int cheapest_device(pgq_csr *c, Workspace *ws, int64_t n, const int64_t *d_src, const int64_t *d_dst,
                           int64_t *d_out, uint8_t *d_ok, bool chain, int64_t max_hops, int64_t min_hops) {
	// a lower bound never takes the unbounded drivers: their labels are not rounds (and see fact 4 of pgq_cheapest_path_within.hip)
	const bool bounded = max_hops >= 0 && (min_hops > 0 || max_hops < c->V - 1);
	if (!bounded && chain && options().chain && n > 0 && n < (1LL << 31)) return cheapest_with_chains<T>(c, ws, n, d_src, d_dst, d_out, d_ok);
	hipStream_t st = ws->stream;
	pgq_stats_t &S = tstats().s;
	S.pairs += n;
	if (n == 0) return PGQ_OK;
	if (n >= (1LL << 31)) return fail(PGQ_ERR_INVALID_ARG, "more than 2^31-1 rows in one call");
	u32 U = 0;
	PGQ_TRY(prepare_lanes(c, ws, n, d_src, d_dst, &U, true, min_hops > 0)); // a closed walk of min_hops >= 1 edges needs a lane
	S.unique_sources += U;
	const int nb = (int)(((int64_t)U + LC - 1) / LC);
	PGQ_TRY(batch_bounds(ws, n, LC, nb));
	const int64_t *bs = ws->h_bstart;
	if (!bounded && light_edges_first(c)) { // once per CSR, before the workers need them (hop-bounded rounds: plain lists, no mean)
		PGQ_TRY(ensure_weight_sorted(c, ws));
		PGQ_TRY(ensure_weight_mean(c, ws));
	} else if (!bounded && options().relax_delta_div > 0) {
		PGQ_TRY(ensure_weight_mean(c, ws));
	}
	// Independent batches overlap on several streams (one host thread each, like the lane batches of the unweighted
	// search): the rounds with few changed vertices — a third of a batch's rounds — leave most of the chip idle.
	int workers = std::max(1, std::min(options().relax_streams > 0 ? options().relax_streams : options().streams, nb));
	if (workers > 1) { // every extra worker holds its own label array (V x 64 x 8 bytes): only while half the free memory covers them
		size_t free_b = 0, total_b = 0;
		PGQ_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
		// (a bounded worker: the snapshot rows and their masks besides)
		const size_t per_worker = (size_t)std::max<int64_t>(c->V, 1) * (LC * 8 + 64 + (bounded ? LC * 8 + 8 : 0)) + (size_t)(c->E / 64) * 4;
		workers = (int)std::min<size_t>((size_t)workers, 1 + free_b / 2 / per_worker);
	}
	// `light` (and with it the label width DT) is decided ONCE, here, and handed to every worker: a concurrent pgq_set_option
	// between two evaluations used to leave a worker with 4-byte labels outside the light-edges-first path (an "internal error"
	// return).  The weight-sorted copy above has left the mean on the handle; one that is not positive and finite: plain rounds.
	const bool light = !bounded && light_edges_first(c) && c->wadj && c->w_mean > 0 && c->w_mean < 1e300;
	const bool narrow = light && labels_fit_32<T>(c);
	// about one destination per source (a list of pairs, not a cross product): every row is a lane of its own, searched from
	// both ends (BidirBatches); many destinations per source share their source's lane as before
	const int64_t R = bs[nb]; // the rows that need a search (sorted by source; trivial and NULL rows behind them)
	bool bidir = false;
	if constexpr (std::is_same<T, int64_t>::value)
		bidir = options().relax_bidir && light && R > 0 && R <= (int64_t)std::max(1, options().relax_bidir_rows) * (int64_t)U;
	int nb_run = nb;
	if (bidir) {
		PGQ_TRY(ensure_reverse_sorted(c, ws));
		bidir = c->rwadj != nullptr;
		if (bidir) {
			nb_run = (int)((R + LC - 1) / LC);
			workers = std::max(1, std::min(workers, nb_run));
		}
	}
	auto run_relax = [&](Workspace *priv, int b0, int bstride) -> int {
		const RelaxWorker w { c, ws, priv, nb_run, d_out, d_ok };
		if (bounded) return HopBatches<T>(w, U, min_hops, max_hops).run(b0, bstride);
		if constexpr (std::is_same<T, int64_t>::value) {
			if (bidir) return narrow ? BidirBatches<int32_t>(w, R).run(b0, bstride) : BidirBatches<int64_t>(w, R).run(b0, bstride);
			if (narrow) return RelaxBatches<T, int32_t>(w, U, light).run(b0, bstride);
		}
		return RelaxBatches<T, int64_t>(w, U, light).run(b0, bstride);
	};
	int rc = PGQ_OK;
	if (workers == 1) {
		rc = run_relax(ws, 0, 1);
	} else {
		std::vector<WorkspaceLease> leases((size_t)workers - 1);
		for (auto &l : leases) PGQ_TRY(l.acquire());
		rc = fan_out(std::vector<int>((size_t)workers, current_device()),
		             [&](int t) { return run_relax(t == 0 ? ws : leases[(size_t)t - 1].ws, t, workers); });
	}
	if (rc != PGQ_OK) return rc;
	const int64_t lo_t = bs[nb + 1], lo_n = bs[nb + 2];
	if (n > lo_t)
		// (min_hops >= 1: the src == dst rows left trivial have no closed walk at all — NULL, not the empty walk's 0)
		hipLaunchKernelGGL(k_cheapest_tails, dim3(blocks_for(n - lo_t)), dim3(256), 0, st, lo_t, min_hops > 0 ? lo_t : lo_n, n,
		                   ws->sidx.as<u32>(), d_out, d_ok);
	PGQ_HIP_TRY(hipStreamSynchronize(st));
	KernelTimer::flush();
	return PGQ_OK;
}

int check_weighted(pgq_csr_t *csr) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	if (csr->w_type == PGQ_W_NONE || !csr->w)
		return fail(PGQ_ERR_NOT_WEIGHTED, "Constraint Error: Need to initialize CSR before doing cheapest path");
	if (csr->has_negative_weight)
		return fail(PGQ_ERR_UNSUPPORTED, "cheapest_path_length: negative edge weights are not supported");
	return PGQ_OK;
}

// cheapest_walk's bounds, for the length call here and the list call in pgq_cheapest_path.o
int check_walk_bounds(int64_t min_hops, int64_t max_hops) {
	if (min_hops < 0) return fail(PGQ_ERR_INVALID_ARG, "min_hops must not be negative");
	if (max_hops < min_hops) return fail(PGQ_ERR_INVALID_ARG, "max_hops must not be below min_hops");
	if (min_hops > PGQ_WALK_MAX_HOPS)
		return fail(PGQ_ERR_UNSUPPORTED, "cheapest_walk: a lower bound above " + std::to_string(PGQ_WALK_MAX_HOPS) +
		                                     " is not supported (every exact round runs over all it reaches)");
	return PGQ_OK;
}

// pgq_relax.h's two entries to the lane batches: one worker on the call's own workspace, every batch, no cost outputs.
template <typename T> int settle_every_label(pgq_csr *c, Workspace *ws, int nb, u32 U, const SettledBatch &settled) {
	return RelaxBatches<T, int64_t>(RelaxWorker { c, ws, ws, nb, nullptr, nullptr }, U, false, &settled).run(0, 1);
}
template <typename T> int hop_rounds_logged(pgq_csr *c, Workspace *ws, int nb, u32 U, int64_t lower, int64_t K, const HopLog &log) {
	return HopBatches<T>(RelaxWorker { c, ws, ws, nb, nullptr, nullptr }, U, lower, K, &log).run(0, 1);
}
template int settle_every_label<int64_t>(pgq_csr *, Workspace *, int, u32, const SettledBatch &);
template int settle_every_label<double>(pgq_csr *, Workspace *, int, u32, const SettledBatch &);
template int hop_rounds_logged<int64_t>(pgq_csr *, Workspace *, int, u32, int64_t, int64_t, const HopLog &);
template int hop_rounds_logged<double>(pgq_csr *, Workspace *, int, u32, int64_t, int64_t, const HopLog &);

} // namespace pgq

using namespace pgq;

extern "C" {

// max_hops: null = unbounded (iterativelength_bulk's convention).  The bounded forms answer a NULL handle before anything else.
// min_hops > 0: cheapest_walk_length (its bounds are checked by the caller; 0 is forwarded to the _within form).
static int cheapest_bulk(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, void *d_out, uint8_t *d_out_valid,
                         const int64_t *max_hops, int64_t min_hops = 0) {
	if (max_hops && !csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	const bool arrays = d_src && d_dst && d_out && d_out_valid;
	auto check = [&]() -> int {
		PGQ_TRY(check_weighted(csr));
		PGQ_TRY(check_arrays(csr, n, arrays, "NULL device array"));
		if (max_hops && *max_hops < 0) return fail(PGQ_ERR_INVALID_ARG, "max_hops must not be negative");
		return PGQ_OK;
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) {
		const int64_t bound = max_hops ? *max_hops : -1;
		if (csr->w_type == PGQ_W_INT64)
			return cheapest_device<int64_t>(csr, ws, n, d_src, d_dst, (int64_t *)d_out, d_out_valid, true, bound, min_hops);
		return cheapest_device<double>(csr, ws, n, d_src, d_dst, (int64_t *)d_out, d_out_valid, true, bound, min_hops);
	});
}

static int cheapest_chunk(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, void *out, uint64_t *out_valid,
                          const int64_t *max_hops, int64_t min_hops = 0) {
	if (max_hops && !csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	auto check = [&]() -> int {
		PGQ_TRY(check_weighted(csr));
		if (V != csr->V) return fail(PGQ_ERR_INVALID_ARG, "V does not match the uploaded CSR");
		if (n < 0 || (n > 0 && (!out || !out_valid))) return fail(PGQ_ERR_INVALID_ARG, "NULL output");
		if (max_hops && *max_hops < 0) return fail(PGQ_ERR_INVALID_ARG, "max_hops must not be negative");
		return n == 0 ? kNoRows : PGQ_OK;
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		FlatPairs fp;
		PGQ_TRY(flatten_pairs(V, n, src, dst, fp, true));
		for (int64_t i = 0; i < n; i++)
			if (!fp.dst_valid[i]) fp.src[i] = -1; // NULL dst -> NULL (cheapest_path_length.cpp:74-76)
		PGQ_TRY(ws->out_val.reserve((size_t)n * 8));
		PGQ_TRY(ws->out_ok.reserve((size_t)n));
		PGQ_TRY(stage_pairs(ws, n, fp.src.data(), fp.dst.data()));
		const int64_t *d_src = ws->in_src.as<int64_t>(), *d_dst = ws->in_dst.as<int64_t>();
		const int64_t bound = max_hops ? *max_hops : -1;
		PGQ_TRY(csr->w_type == PGQ_W_INT64
		            ? cheapest_device<int64_t>(csr, ws, n, d_src, d_dst, ws->out_val.as<int64_t>(), ws->out_ok.as<uint8_t>(), true, bound, min_hops)
		            : cheapest_device<double>(csr, ws, n, d_src, d_dst, ws->out_val.as<int64_t>(), ws->out_ok.as<uint8_t>(), true, bound, min_hops));
		return download_valid(ws, n, out, out_valid);
	});
}

int pgq_cheapest_path_length_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst,
                                         void *d_out, uint8_t *d_out_valid) {
	return cheapest_bulk(csr, n, d_src, d_dst, d_out, d_out_valid, nullptr);
}
int pgq_cheapest_path_length_within_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t max_hops,
                                                void *d_out, uint8_t *d_out_valid) {
	return cheapest_bulk(csr, n, d_src, d_dst, d_out, d_out_valid, &max_hops);
}

int pgq_cheapest_path_length(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, void *out,
                             uint64_t *out_valid) {
	return cheapest_chunk(csr, V, n, src, dst, out, out_valid, nullptr);
}
int pgq_cheapest_path_length_within(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops, void *out,
                                    uint64_t *out_valid) {
	return cheapest_chunk(csr, V, n, src, dst, out, out_valid, &max_hops);
}

// The cheapest walk of min_hops .. max_hops edges (include/pgq_hip.h).  min_hops == 0 IS the _within call; otherwise HopBatches
// with a lower bound, for every max_hops (INT64_MAX: the rounds end with the queue).
int pgq_cheapest_walk_length_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t min_hops, int64_t max_hops,
                                         void *d_out, uint8_t *d_out_valid) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	PGQ_TRY(check_walk_bounds(min_hops, max_hops));
	return cheapest_bulk(csr, n, d_src, d_dst, d_out, d_out_valid, &max_hops, min_hops);
}
int pgq_cheapest_walk_length(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t min_hops, int64_t max_hops, void *out,
                             uint64_t *out_valid) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	PGQ_TRY(check_walk_bounds(min_hops, max_hops));
	return cheapest_chunk(csr, V, n, src, dst, out, out_valid, &max_hops, min_hops);
}

} // extern "C"
