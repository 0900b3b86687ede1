// pgq_walk_rule.h — the query of the walk calls and the ONE rule that says when a row has enough: walk_count, k_shortest_walks,
// their path-mode forms and k_shortest_groups (pgq_k_walks.hip, pgq_path_modes.h).  Plain C++: the kernels take these structs by
// value, the host builds them, and a host compiler alone compiles this file (tests/test_walk_rule_cpu.py holds it against the
// Python models).
//
// A row (src, dst) meets its candidate lengths t = min_hops, min_hops + 1, ... in order; a length with w > 0 walks is a GROUP.
// The row's state is (count, groups): the saturating sum of the w it was fed and how many lengths fed it.  It is OPEN while
//     groups < G  and  count <= B
// and a closed row is fed nothing more.  The forms differ in G and B alone:
//     SHORTEST k GROUP   G = groups, B = max_paths P.  Not count < P: with count == P on a group boundary a later non-empty length
//                        still makes the row's count P + 1, which is what tells "exactly P" from "more than P".
//     SHORTEST k         G unbounded, B = k - 1: "short of k walks" is count <= k - 1.
//     walk_count         G unbounded, B = INT64_MAX - 1: a saturated count neither adds nor changes.
// What a form emits from a fed length is WalkPlan's: min(w, what is left of `limit`) walks of 2 t + 1 elements each.
#pragma once
#include <cstdint>

#ifndef PGQ_HD // (pgq_pack.h's, for a program that includes this file alone)
#if defined(__HIPCC__) || defined(__HIP__)
#define PGQ_HD __host__ __device__ __forceinline__
#else
#define PGQ_HD inline
#endif
#endif

namespace pgq {

constexpr int64_t kWalkMax = 0x7FFFFFFFFFFFFFFFll;

struct WalkRule {
	int64_t groups; // G
	int64_t bound;  // B
};

// What a walk call asks, the same for every row; built once per call (walk_query, pgq_k_walks.hip).
struct WalkQuery {
	int64_t min_hops, max_hops;
	int64_t groups; // 0, or SHORTEST k GROUP's k
	int64_t limit;  // k, the count's limit or max_paths; lists: at most 2^31
	int mode;       // 0: the walks themselves (NONE / WALK), or PGQ_MODE_SIMPLE / _TRAIL / _ACYCLIC

	// the rounds stop by distance and the rows are searched (pgq_path_modes.h)
	PGQ_HD bool by_distance() const { return mode != 0; }
	PGQ_HD WalkRule rule() const { return groups > 0 ? WalkRule { groups, limit } : WalkRule { kWalkMax, limit - 1 }; }
};

struct WalkRow {
	int64_t count = 0, groups = 0;

	PGQ_HD bool open(const WalkRule &r) const { return groups < r.groups && count <= r.bound; }
	// w > 0 walks of one length.  fresh = false: more walks of the length fed last (the search finds a length's walks one by one).
	PGQ_HD void add(int64_t w, bool fresh = true) {
		const uint64_t s = (uint64_t)count + (uint64_t)w;
		count = s > (uint64_t)kWalkMax ? kWalkMax : (int64_t)s;
		groups += fresh ? 1 : 0;
	}
	// By distance, at the row's distance d >= min_hops with w = W_d[dst] > 0: a mode may refuse any longer walk and refuses none of
	// length d, so the row is closed there exactly when feeding it w closes it (G == 1 or w > B) — its count is then B + 1, whatever
	// w was — and stays open to the last round otherwise.  The search overwrites the count.
	PGQ_HD void close_at_distance(int64_t w, const WalkRule &r) {
		WalkRow at_d;
		at_d.add(w);
		if (!at_d.open(r)) count = r.bound + 1;
	}
};

// What a row emits of what it is fed: the first `limit` walks.  Their number is np(); the plan adds up their elements and the
// lengths they come from.
struct WalkPlan {
	int64_t el = 0, ngroups = 0;

	// `row` is about to be fed w walks of t edges (fresh as above): those that the limit still has room for are emitted
	PGQ_HD void take(const WalkRow &row, int64_t limit, int64_t t, int64_t w, bool fresh = true) {
		const int64_t left = row.count < limit ? limit - row.count : 0;
		const int64_t n = w < left ? w : left;
		if (n > 0 && fresh) ngroups++;
		el += n * (2 * t + 1); // n <= 2^31, 2 t + 1 <= 129
	}
	PGQ_HD static int64_t np(const WalkRow &row, int64_t limit) { return row.count < limit ? row.count : limit; }
};

} // namespace pgq
