// The stop rule of the walk calls (csrc/pgq_walk_rule.h) driven from a host program, for test_walk_rule_cpu.py.
// stdin, one case per line:   lo g limit by_distance n W_0 .. W_{n-1}      (g = 0: SHORTEST k / a count with limit k)
// stdout, one line per case:  for t = lo .. n-1: count groups open  — the row behind round t, fed as k_walk_after feeds it;
//                             np el count ngroups                   — the plan over all rounds, as k_walk_plan makes it;
//                             np el count ngroups                   — the same fed one walk at a time, as k_mode_search does.
#include <cstdio>
#include <vector>

#include "pgq_walk_rule.h"

using namespace pgq;

int main() {
	long long lo, g, limit, by_distance, n;
	while (scanf("%lld %lld %lld %lld %lld", &lo, &g, &limit, &by_distance, &n) == 5) {
		std::vector<long long> W((size_t)n);
		for (long long &w : W)
			if (scanf("%lld", &w) != 1) return 1;
		const WalkQuery q { lo, n - 1, g, limit, by_distance ? 2 : 0 };
		const WalkRule rule = q.rule();
		WalkRow s;
		long long first = -1;
		for (long long t = 0; t < n; t++) {
			const long long w = W[(size_t)t];
			if (q.by_distance()) {
				if (first < 0 && w > 0) {
					first = t;
					if (t >= q.min_hops) s.close_at_distance(w, rule);
				}
			} else if (t >= q.min_hops && s.open(rule) && w > 0) {
				s.add(w);
			}
			if (t >= q.min_hops) printf("%lld %lld %d ", (long long)s.count, (long long)s.groups, s.open(rule) ? 1 : 0);
		}
		WalkRow all, one;
		WalkPlan plan, plan1;
		for (long long t = q.min_hops; t < n && all.open(rule); t++) {
			if (W[(size_t)t] <= 0) continue;
			plan.take(all, q.limit, t, W[(size_t)t]);
			all.add(W[(size_t)t]);
		}
		const long long rule_count = all.count < rule.bound + 1 ? all.count : rule.bound + 1;
		printf("%lld %lld %lld %lld ", (long long)WalkPlan::np(all, q.limit), (long long)plan.el, q.groups > 0 ? rule_count : (long long)s.count,
		       (long long)plan.ngroups);
		for (long long t = q.min_hops; t < n && one.open(rule); t++) {
			bool fresh = true;
			for (long long i = 0; i < W[(size_t)t] && one.count <= rule.bound; i++, fresh = false) {
				plan1.take(one, q.limit, t, 1, fresh);
				one.add(1, fresh);
			}
		}
		printf("%lld %lld %lld %lld\n", (long long)WalkPlan::np(one, q.limit), (long long)plan1.el, (long long)one.count, (long long)plan1.ngroups);
	}
	return 0;
}
