// pgq_route.hip — which route answers the rows of an iterativelength / shortestpath call, and the C entry points.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>

#include "pgq_search.h"

namespace pgq {

// ---- rows sorted by source for the source-centric kernel (Route::run_sorted_ball) -------------------------------
// NULL and out-of-range sources sort behind every vertex (key V); the gathered rows carry the ORIGINAL ids, so that the
// kernel answers NULL rows with NULL and reports ids outside [0, V) like every other route.
__global__ void k_sort_keys(int64_t n, const int64_t *__restrict__ src, int64_t V, u32 *__restrict__ key, u32 *__restrict__ idx) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const int64_t s = src[i];
	key[i] = (s < 0 || s >= V) ? (u32)V : (u32)s;
	idx[i] = (u32)i;
}
__global__ void k_sort_gather(int64_t n, const u32 *__restrict__ sidx, const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                              int64_t *__restrict__ ssrc, int64_t *__restrict__ sdst) {
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= n) return;
	const u32 i = sidx[j];
	ssrc[j] = src[i];
	sdst[j] = dst[i];
}
__global__ void k_sort_scatter(int64_t n, const u32 *__restrict__ sidx, const int64_t *__restrict__ sout, int64_t *__restrict__ out) {
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j < n) out[sidx[j]] = sout[j];
}
__global__ void k_scatter_te(int64_t n, const u32 *__restrict__ sidx, const int64_t *__restrict__ ste,
                             int64_t *__restrict__ out) {
	int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) out[sidx[i]] = ste[i];
}

// iterativelength_within: whatever a stage reported beyond the bound becomes NULL (SearchAsk::max_hops)
__global__ void k_clamp_hops(int64_t n, int64_t max_hops, int64_t *__restrict__ len) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n && len[i] > max_hops) len[i] = -1;
}
// shortestpath_within: the entry points' own check behind the search (SearchAsk::max_hops: no stage is relied on).  *beyond (a
// pinned host word) becomes 1 when a stage reported a row beyond the bound: a plain store, and none in a call that needs none.
__global__ void k_bound_check(int64_t n, int64_t max_hops, const int64_t *__restrict__ len, u32 *__restrict__ beyond) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n && len[i] > max_hops) *beyond = 1u;
}
// When there were such rows: cnt[i] = the elements of row i's list when the row lies within the bound, else 0 ...
__global__ void k_bound_counts(int64_t n, int64_t max_hops, const int64_t *__restrict__ len, int64_t *__restrict__ cnt) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const int64_t k = len[i];
	cnt[i] = (k >= 0 && k <= max_hops) ? 2 * k + 1 : 0;
}
// ... and, behind their scan: the lists of the others packed in row order (from child to packed, or none when the lists
// were not written), the rows beyond the bound NULL
__global__ void k_bound_pack(int64_t n, int64_t max_hops, int64_t *__restrict__ len, int64_t *__restrict__ off, const int64_t *__restrict__ noff,
                             const int64_t *__restrict__ child, int64_t *__restrict__ packed) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const int64_t k = len[i];
	if (k > max_hops) {
		len[i] = -1;
		off[i] = 0;
	} else if (k >= 0) {
		if (packed)
			for (int64_t j = 0; j < 2 * k + 1; j++) packed[noff[i] + j] = child[off[i] + j];
		off[i] = noff[i];
	}
}
// The bound a search runs under: V - 1 hops and more reach whatever is reachable — the unbounded search (INT64_MAX is what
// the binder holds for "no upper bound")
int64_t search_bound(const pgq_csr *c, int64_t max_hops) { return max_hops >= c->V - 1 ? -1 : max_hops; }

// Whether the pair-centric pre-pass may run for this call at all, and whether the host-side cost model sends n rows
// (each taken as a distinct source) to it.  Shared by search_device and the chunk entry point (zero-copy staging).
constexpr int64_t kMeetDecideRows = 16384; // above: the distinct sources are sampled and the decision is taken on the device
static bool prepass_may(const pgq_csr *c, const SearchAsk &ask) {
	// depth 1 = the stragglers a lane batch deferred (a few far pairs of a cross product): the pre-pass answers them from
	// two-hop scans instead of another round of whole-graph levels
	return options().meet && !ask.want_te && ask.depth <= 1 && !ask.from_meet && c->E > 0 && c->fdesc != nullptr;
}
// Bytes the pre-pass moves per row.  Known once a pre-pass has run on this CSR (measured: its kernels count the entries
// they walk; calibrate_prepass runs 1024 pseudo-random pairs through it before the first large call is routed).  Before
// that: the cheaper endpoint's WHOLE two-hop neighbourhood, ~0.6 x E[in-degree x out-degree] entries — what a far pair
// costs.  Close pairs stop after a fraction of it: on the SF100-shaped graph the bound is 6x what 65,536 random pairs
// move (12 KB per row), and a 2048 x 32 cross product priced with it went through the lane batches at 0.73 ms where the
// pre-pass takes 0.22.
static double prepass_row_bytes(const pgq_csr *c) {
	const double measured = c->cal.meet_bpr.load(std::memory_order_relaxed);
	return measured > 0 ? measured : c->two_hop_mean * 4.0 * 0.6;
}
__global__ void k_calibration_pairs(int64_t n, int64_t V, int64_t *__restrict__ src, int64_t *__restrict__ dst) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	auto mix = [](u64 x) { // splitmix64
		x += 0x9E3779B97F4A7C15ull;
		x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
		x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
		return x ^ (x >> 31);
	};
	src[i] = (int64_t)(mix(2 * (u64)i) % (u64)V);
	dst[i] = (int64_t)(mix(2 * (u64)i + 1) % (u64)V);
}
static int calibrate_prepass(pgq_csr *c) {
	std::lock_guard<std::mutex> g(c->lazy_lock);
	if (c->cal.meet_bpr.load() > 0) return PGQ_OK;
	const int64_t n0 = 1024;
	WorkspaceLease lease;
	PGQ_TRY(lease.acquire());
	Workspace *w = lease.ws;
	for (DevBuf *b : { &w->in_src, &w->in_dst, &w->out_len }) PGQ_TRY(b->reserve((size_t)n0 * 8));
	hipLaunchKernelGGL(k_calibration_pairs, dim3(blocks_for(n0)), dim3(256), 0, w->stream, n0, c->V, w->in_src.as<int64_t>(), w->in_dst.as<int64_t>());
	pgq_stats_t &S = tstats().s;
	const pgq_stats_t saved = S; // the caller's statistics are about its own rows
	const double rb0 = tstats().route_bytes;
	PrepassResult r;
	// (without the hub tables: the figure is what a row's WALK moves, on a handle with tables as on one without, so that the
	// tables move no route — they make the pre-pass faster where it runs, the lane batches' model was fitted against the walks)
	PrepassArgs pa { n0, w->in_src.as<int64_t>(), w->in_dst.as<int64_t>(), w->out_len.as<int64_t>() };
	pa.no_hubs = true;
	const int rc = meet_prepass(c, w, pa, &r);
	const double bytes = tstats().route_bytes - rb0; // at 4 B per list entry (ThreadStats::route_bytes)
	S = saved;
	PGQ_TRY(rc);
	c->cal.meet_bpr.store(std::max(64.0, bytes / (double)n0));
	calibration_store(c); // the next handle over a graph of this shape starts with it
	return PGQ_OK;
}
static bool prepass_takes(const pgq_csr *c, int64_t n, const SearchAsk &ask) {
	if (!prepass_may(c, ask)) return false;
	const double meet_bytes = (double)n * prepass_row_bytes(c);
	const double edge_bytes = options().meet_bias * (double)c->E;
	return meet_bytes <= lanes_cost_bytes(edge_bytes, (double)std::min<int64_t>(n, c->V), (double)n, (double)c->V);
}

// ---- the route memo (pgq_csr::RouteMemo): one look-up and one record per step, each under plan_lock once -------------
MemoVerdict memo_lookup(pgq_csr *c, int64_t n, const void *src, const void *dst) {
	std::lock_guard<std::mutex> g(c->plan_lock);
	const pgq_csr::RouteMemo &m = c->route_memo;
	MemoVerdict v;
	if (m.ball_n == n && m.ball_src == src && m.ball_dst == dst) v.ball = m.ball_yes ? 1 : 0;
	if (m.n == n && m.src == src && m.dst == dst) {
		v.go = m.go;
		v.sorted = m.sorted_yes;
	}
	v.ahead_wd = m.id_n == n ? m.id_wd : 0;
	return v;
}
void memo_record(pgq_csr *c, int64_t n, const void *src, const void *dst, const MemoOutcome &o) {
	if (o.ball < 0 && o.go < 0 && o.sorted < 0 && !o.go_again && o.id_wd < 0) return; // nothing to write: no lock
	std::lock_guard<std::mutex> g(c->plan_lock);
	pgq_csr::RouteMemo &m = c->route_memo;
	if (o.ball >= 0) {
		m.ball_n = n;
		m.ball_src = src;
		m.ball_dst = dst;
		m.ball_yes = o.ball != 0;
	}
	if (o.go >= 0) {
		m.n = n;
		m.src = src;
		m.dst = dst;
		m.go = o.go;
		m.sorted_yes = false;
	}
	if (o.sorted >= 0) m.sorted_yes = o.sorted != 0;
	if (o.go_again) m.go = 1;
	if (o.id_wd >= 0) {
		m.id_n = o.in_place ? n : -1;
		m.id_wd = o.id_wd;
	}
}

// One search_device call.  The route, in order (run): the per-row bidirectional search (iterativelengthbidirectional); a plan on
// the host (no launches); the source-centric kernel on the rows sorted by source when the memo says that took these buffers; the
// pair-centric pre-pass, its chain opened by the source-centric kernels when the rows may be grouped by source; the sort by source
// when neither took rows of few sources; the lane batches for the rest.  Every route is exact: the choice moves time.  The
// caller's SearchCall is only read; what the call decides for itself (prefer_lanes, no_memo) lives here.
class Route {
public:
	Route(pgq_csr *c, Workspace *ws, const SearchCall &call, SearchReport &rep) : c(c), ws(ws), call(call), rep(rep) {}
	// The byte models that pick a route price kernels at streaming rate; on a graph past the caches the source-centric route is
	// nothing like that (R-MAT-22, 2048 x 1024 rows: global bit maps marked through DRAM atomics, 35,000 far rows searched one
	// by one — 16.7 ms where the model says 0.1) and the lane batches are 4.6 x their model (12 ms).  So large grouped calls are
	// TIMED, per graph shape: the best wall time per row of the source-centric route is kept (the best of at least two calls: a
	// process's first call of a kind pays for allocations, kernel attributes and the calibration); when it is over
	// `route_try_factor` x the lane batches' modelled time the next two such calls go through the lanes, and from then on through
	// whichever measured faster.  Every route is exact, so this only moves time.  (The figures travel with the calibration cache.)
	int search() {
		if (!timed) return run();
		const int64_t levels0 = S.levels;
		const auto t0 = std::chrono::steady_clock::now();
		PGQ_TRY(run());
		const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / (double)n;
		if (rep.route == 1) {
			const double best = nb_s > 0 ? std::min(tb, ns) : ns;
			c->cal.route_ball_ns.store(best, std::memory_order_relaxed);
			c->cal.route_ball_samples.store(nb_s + 1, std::memory_order_relaxed);
			if (nb_s == 0 || n > c->cal.route_rows.load(std::memory_order_relaxed)) c->cal.route_rows.store(n, std::memory_order_relaxed);
			if (nb_s + 1 >= 2 && rep.source_runs > 0) { // the lane batches' modelled time per row, at 8 TB/s
				const double lanes_ns = lanes_cost_bytes(mopt.meet_bias * (double)c->E, std::min(rep.source_runs, (double)c->V), (double)n, (double)c->V) / 8000.0 / (double)n;
				if (best > mopt.route_try_factor * lanes_ns) c->cal.route_try_lanes.store(1, std::memory_order_relaxed);
			}
		} else if (prefer_lanes && S.levels > levels0) { // (the lane batches did run)
			c->cal.route_lanes_ns.store(nl_s > 0 ? std::min(tl, ns) : ns, std::memory_order_relaxed);
			c->cal.route_lanes_samples.store(nl_s + 1, std::memory_order_relaxed);
		}
		return PGQ_OK;
	}
private:
	// ---- per call ----
	pgq_csr *const c;
	Workspace *const ws;
	const SearchCall &call;
	SearchReport &rep;
	const SearchAsk &ask = call.ask;
	const int64_t n = call.n, *const d_src = call.d_src, *const d_dst = call.d_dst;
	int64_t *const d_out_len = call.d_out_len;
	const bool with_paths = call.paths.has_value();
	const hipStream_t st = ws->stream;
	pgq_stats_t &S = tstats().s;
	const Options &mopt = options();
	// a bounded call is off the record (SearchAsk::max_hops): it neither reads nor feeds the calibration (before it exists: the
	// pre-pass priced by the graph's two-hop mean), the route memo or the route timing
	const bool bounded = ask.max_hops >= 0;
	const bool timed = !bounded && mopt.route_timing && mopt.ball == 1 && ask.depth == 0 && !with_paths && !ask.want_te && !ask.bidir && !ask.no_ball &&
	                   ask.ball_hint != 0 && n >= (int64_t)std::max(1, mopt.route_timing_rows);
	const double tb = c->cal.route_ball_ns.load(std::memory_order_relaxed), tl = c->cal.route_lanes_ns.load(std::memory_order_relaxed);
	const int nb_s = c->cal.route_ball_samples.load(std::memory_order_relaxed), nl_s = c->cal.route_lanes_samples.load(std::memory_order_relaxed);
	// both figures are the best of at least two calls before they decide anything (a first call pays one-time costs)
	// ... and they speak for calls of their own size: a lane batch costs the same for 32 rows per source as for 1024, the
	// source-centric route does not — a call with under half the measured rows is left to the byte models
	const bool same_size = n * 2 >= c->cal.route_rows.load(std::memory_order_relaxed);
	const bool trial = same_size && nb_s >= 2 && nl_s < 2 && c->cal.route_try_lanes.load(std::memory_order_relaxed) != 0;
	// large grouped call on a graph where the lane batches measured faster than the source-centric route, or their trial
	const bool prefer_lanes = timed && (trial || (same_size && nb_s >= 2 && nl_s >= 2 && tl < tb));
	// (such a call neither follows nor feeds the route memo: what it would leave there — "these buffers go to the lanes" — must
	// not outlive the preference, and the decision kernel in front of the lanes is 40 us of a call that takes milliseconds)
	const bool no_memo = ask.no_memo || bounded || prefer_lanes;
	const bool read_memo = mopt.route_memo && !no_memo, write_memo = !no_memo;
	// few rows: every row is taken as a distinct source (the pessimistic case for the pre-pass); many rows: a sampled
	// estimate of the distinct sources decides ON THE DEVICE, in the same launch chain (cross products share their lanes)
	const bool decide = n > kMeetDecideRows;
	// ---- the plan (plan) ----
	double meet_bytes = 0, edge_bytes = 0; // the byte rule's two sides
	BallMode ball = BallMode::Off;
	bool sort_allowed = false;
	MemoVerdict memo;
	DecideMode decide_mode = DecideMode::None;

	int run() {
		S.pairs += n;
		if (n == 0) return PGQ_OK;
		if (n >= (1LL << 31)) return fail(PGQ_ERR_INVALID_ARG, "more than 2^31-1 rows in one call");
		if (with_paths) PGQ_TRY(ensure_edge_ids(c)); // PGQ_UPLOAD_LAZY_EDGE_IDS: the first shortestpath call brings them over
		// a large call is about to be routed on the pre-pass's bytes per row: measured first if this CSR has none yet
		if (prepass_may(c, ask) && decide && mopt.meet_calibrate && !bounded && c->cal.meet_bpr.load(std::memory_order_relaxed) <= 0) PGQ_TRY(calibrate_prepass(c));
		if (ask.bidir && !with_paths && !ask.want_te && ask.depth == 0 && c->E > 0) return run_bidirectional();
		plan();
		bool sampled = false; // the sampled decision was asked for without the chain: read it after the next wait
		if (prepass_takes(c, n, ask)) {
			bool took = false;
			if (sort_allowed && read_memo && memo.sorted) { // these buffers went through the sort last time: straight there
				PGQ_TRY(run_sorted_ball(&took));
				if (took) return PGQ_OK;
				record_sorted(false);
			}
			if (decide && read_memo && memo.go == 0) {
				sampled = true; // taken inside the lane assignment's first launch (k_mark_sources)
			} else {
				PrepassResult r;
				PGQ_TRY(with_paths ? run_prepass_paths(r) : run_prepass(r));
				record_prepass(r);
				if (r.answered) return PGQ_OK;
				// neither the source-centric kernel (the rows are not grouped) nor the pre-pass (few distinct sources) took the call:
				// with at least 64 rows per source on average a sort by source makes it the former's
				if (sort_allowed && r.est_sources > 0 && r.est_sources * 64.0 <= (double)n) {
					PGQ_TRY(run_sorted_ball(&took));
					record_sorted(took);
					if (took) return PGQ_OK;
				}
			}
		}
		return search_lanes(c, ws, call, rep, LanesPlan { sampled, memo.ahead_wd, meet_bytes, edge_bytes });
	}
	int run_bidirectional() {
		u32 nd = 0;
		PGQ_TRY(meet_bidirectional(c, ws, n, d_src, d_dst, d_out_len, &nd));
		OpenRows open { nd, ws->open_src, ws->open_dst }; // over k_bibfs's caps: the lane-batched search
		open.ask.from_meet = true;
		return search_open_rows(c, ws, call, rep, open, [&](bool) { return meet_apply(ws, nd, ws->def_len.as<int64_t>(), d_out_len); });
	}
	// Pair-centric pre-pass: rows at distance <= 3 are answered from two-hop neighbourhood scans (pgq_meet.hip); only what it
	// leaves open goes through the lane-batched search.  Cost model (bytes at streaming rate, prepass_takes): the pre-pass
	// walks, per row, the cheaper endpoint's two-hop neighbourhood (~0.6 of E[in-degree x out-degree] entries when it has to
	// walk all of it; it usually stops far earlier: the estimate is on the safe side).  A lane batch of `wd` lane-words costs
	// about one sparse and one dense bottom-up level (or the probes that replace it): E x (12 + 3 wd) bytes — calibrated on
	// the 2048-lane batch of the SF100-shaped graph (0.94 ms ~ 4.3 GB at streaming rate; round 2 priced a batch at 16 B per
	// edge and sent a 2048 x 32 cross product through the lanes at three times the cost of the pre-pass).  `meet_bias`
	// scales the lanes' side.
	void plan() {
		meet_bytes = (double)n * prepass_row_bytes(c);
		edge_bytes = mopt.meet_bias * (double)c->E; // x (12 + 3 wd) per batch
		// round 6: the source-centric kernels open the pre-pass's chain and decide on the device (pgq_ball.h); not for paths,
		// not for the rows that kernel itself left open
		if (!(with_paths || ask.no_ball || ask.bidir || prefer_lanes || n < 2) && mopt.ball > 0)
			ball = mopt.ball == 1 ? BallMode::Decide : BallMode::Always;
		const bool ball_possible = ball != BallMode::Off && (bounded || c->cal.ball_open_frac.load(std::memory_order_relaxed) <= 0.02); // before the memo's say on THESE rows as they lie
		if (ball == BallMode::Decide && (ask.ball_hint == 0 || !ball_possible)) ball = BallMode::Off;
		// the caller has counted the source runs on the host and found the rows grouped: the chain is the two kernels alone (if
		// the device's byte rule declines after all, run_prepass falls back to the stage kernels)
		if (ball == BallMode::Decide && ask.ball_hint == 1) ball = BallMode::Only;
		// the memo is read only when a step below uses it (chunk calls and small nested searches take no lock for it)
		const bool memo_ball = ball == BallMode::Decide && ask.ball_hint < 0; // (a caller that has looked at the rows knows better than the memo)
		if (read_memo && (decide || memo_ball)) memo = memo_lookup(c, n, d_src, d_dst);
		if (memo_ball && memo.ball >= 0) ball = memo.ball ? BallMode::Only : BallMode::Off;
		// the memo vouches for the pre-pass on these buffers: the sample only observes (it rides in the chain)
		decide_mode = !decide ? DecideMode::None : (read_memo && memo.go > 0 ? DecideMode::Ride : DecideMode::Gate);
		sort_allowed = mopt.ball_sort && ball_possible && !ask.want_te && decide;
	}
	// the pre-pass chain over the rows as they lie (lengths)
	int run_prepass(PrepassResult &r) {
		const double b0 = tstats().route_bytes;
		PrepassArgs a { n, d_src, d_dst, d_out_len, nullptr, meet_bytes, edge_bytes, decide_mode, ball, ask.max_hops };
		PGQ_TRY(meet_prepass(c, ws, a, &r));
		if (ball == BallMode::Only && r.ball_attempted && !r.ball_took) { // the kernels-alone chain declined these rows: the stage kernels after all
			a.ball = BallMode::Off;
			PGQ_TRY(meet_prepass(c, ws, a, &r));
			r.est_sources = -1.0; // (the source-centric kernel has just declined these rows: no sort by source for them)
		}
		if (r.ball_took) {
			if (n >= 1024 && !bounded) {
				const double now = (double)r.n_open / (double)n, old = c->cal.ball_open_frac.load(std::memory_order_relaxed);
				c->cal.ball_open_frac.store(0.5 * old + 0.5 * now, std::memory_order_relaxed);
			}
			rep.route = 1;
			rep.source_runs = r.est_sources;
		}
		if (!r.answered) return PGQ_OK;
		if (n >= 1024 && !r.ball_took && !bounded) { // what these rows really moved refines the CSR's bytes per row (half the weight to the newest call)
			// (a row answered from the hub tables moved next to nothing: it counts with the estimate it was routed under, see calibrate_prepass)
			const double now = std::max(64.0, (tstats().route_bytes - b0 + (double)r.hub_settled * prepass_row_bytes(c)) / (double)n);
			const double old = c->cal.meet_bpr.load(std::memory_order_relaxed);
			c->cal.meet_bpr.store(old > 0 ? 0.5 * old + 0.5 * now : now, std::memory_order_relaxed);
		}
		// what the source-centric kernel left open (distance >= 5, unreachable, segments over its cap) is the pre-pass's kind
		// of row (k_meet4d / k_bibfs) before it is the lane batches'
		OpenRows open { r.n_open, ws->open_src, ws->open_dst };
		open.ask.from_meet = !r.ball_took;
		open.ask.no_ball = true;
		return search_open_rows(c, ws, call, rep, open, [&](bool) { return meet_apply(ws, r.n_open, ws->def_len.as<int64_t>(), d_out_len); });
	}
	// shortestpath: the pre-pass also records each answered row's inner vertices (reference tie-break); their lists are
	// packed first, the lists of the rows left to the lane-batched search are appended behind them
	int run_prepass_paths(PrepassResult &r) {
		// the lists of the rows the pre-pass answers have at most 9 elements (distance <= 4): the buffer for them is sized
		// up front, so that they are written in the same launch chain as the search
		DecideMode dm = decide_mode;
		if (dm == DecideMode::Gate) { // asked first, on its own: the buffers below are only worth reserving when the pre-pass runs
			bool go = true;
			PGQ_TRY(meet_decide_alone(c, ws, n, d_src, meet_bytes, edge_bytes, &go));
			S.host_waits++;
			r.answered = go;
			if (!go) return PGQ_OK;
			dm = DecideMode::None;
		}
		const SearchPaths &p = *call.paths;
		MeetPathsOut po { p.d_child_ext, p.child_cap_ext, p.d_out_off };
		if (!p.d_child_ext) {
			// at most 9 elements per row (distance 4) — up to paths_reserve_mb; a call whose lists need more (over ~15 M rows at
			// the shipped 1 GB) has them written again into a buffer of the exact size (round-5 advisor finding: 72 bytes per row
			// reserved up front whatever the call)
			const size_t want = (size_t)std::max<int64_t>(n * 9, 1) * 8, lim = (size_t)std::max(0, mopt.paths_reserve_mb) << 20; // (0: 4 KB — the tests' way to the second emission)
			PGQ_TRY(ws->child.reserve(std::min(want, std::max<size_t>(lim, 4096))));
			po.d_child = ws->child.as<int64_t>();
			po.child_cap = (int64_t)(ws->child.cap / 8);
		}
		PGQ_HIP_TRY(hipMemsetAsync(p.d_out_off, 0, (size_t)n * 8, st));
		PGQ_TRY(meet_prepass(c, ws, PrepassArgs { n, d_src, d_dst, d_out_len, &po, meet_bytes, edge_bytes, dm, BallMode::Off, ask.max_hops }, &r));
		if (!r.answered) return PGQ_OK;
		if (!p.d_child_ext && po.total > po.child_cap) { // (the kernel skipped the lists that did not fit)
			PGQ_TRY(ws->child.reserve((size_t)po.total * 8));
			po.d_child = ws->child.as<int64_t>();
			po.child_cap = (int64_t)(ws->child.cap / 8);
			PGQ_TRY(meet_reemit_paths(c, ws, n, d_src, d_dst, d_out_len, &po));
		}
		OpenRows open { r.n_open, ws->open_src, ws->open_dst, SearchAsk(), po.total }; // (search_open_rows hands the bound on)
		open.ask.from_meet = true;
		PGQ_TRY(search_open_rows(c, ws, call, rep, open, [&](bool) {
			return meet_apply_paths(ws, r.n_open, ws->def_len.as<int64_t>(), ws->def_off.as<int64_t>(), po.total, d_out_len, p.d_out_off);
		}));
		if (rep.overflow) return fail(PGQ_ERR_INVALID_ARG, "child buffer too small: need " + std::to_string(rep.child_used) + " elements");
		return PGQ_OK;
	}
	// Rows of few sources that are NOT grouped (a hash join's output order, a shuffled cross product): sorted by source — one
	// radix sort of (source, row) over log2 V bits, one gather — they are the source-centric kernel's input after all; its
	// answers (and those of the rows it leaves open) are scattered back by the sorted row index.  2.1 M rows: ~0.2 ms of
	// sorting + 0.3 ms of kernel against 2.2 ms through the lane batches.  *took = false: the device's byte rule declined.
	int run_sorted_ball(bool *took) {
		*took = false;
		const int64_t V = c->V;
		for (DevBuf *b : { &ws->key, &ws->idx, &ws->skey, &ws->sidx }) PGQ_TRY(b->reserve((size_t)n * 4));
		for (DevBuf *b : { &ws->sort_src, &ws->sort_dst, &ws->sort_out }) PGQ_TRY(b->reserve((size_t)n * 8));
		int bits = 1;
		while (bits < 32 && (1ll << bits) <= V) bits++;
		{
			KernelTimer kt(st, K_PREP);
			hipLaunchKernelGGL(k_sort_keys, dim3(blocks_for(n)), dim3(256), 0, st, n, d_src, V, ws->key.as<u32>(), ws->idx.as<u32>());
			PGQ_TRY(cub_run(ws->sort_tmp, [&](void *tmp, size_t &tb) {
				return hipcub::DeviceRadixSort::SortPairs(tmp, tb, ws->key.as<u32>(), ws->skey.as<u32>(), ws->idx.as<u32>(), ws->sidx.as<u32>(), (int)n, 0, bits, st);
			}));
			hipLaunchKernelGGL(k_sort_gather, dim3(blocks_for(n)), dim3(256), 0, st, n, ws->sidx.as<u32>(), d_src, d_dst, ws->sort_src.as<int64_t>(),
			                   ws->sort_dst.as<int64_t>());
			kt.stop();
			// keys (8 B read, 8 written), the sort (a read and a write of 8-byte pairs per 8 key bits), the gather (4 + 16 read, 16 written)
			S.algo_bytes[K_PREP] += (double)n * (16.0 + 16.0 * ((bits + 7) / 8) + 36.0);
		}
		PrepassResult r;
		PGQ_TRY(meet_prepass(c, ws, PrepassArgs { n, ws->sort_src.as<int64_t>(), ws->sort_dst.as<int64_t>(), ws->sort_out.as<int64_t>(), nullptr,
		                                          meet_bytes, edge_bytes, DecideMode::None, BallMode::Only, ask.max_hops }, &r));
		if (!r.ball_took) return PGQ_OK;
		rep.route = 1;
		rep.source_runs = r.est_sources;
		// what the kernel left open, in sorted positions: answered like run_prepass's open rows, applied to the sorted output
		OpenRows open { r.n_open, ws->open_src, ws->open_dst, SearchAsk(), 0, false };
		open.ask.no_ball = true;
		open.ask.no_memo = true;
		PGQ_TRY(search_open_rows(c, ws, call, rep, open, [&](bool) { return meet_apply(ws, r.n_open, ws->def_len.as<int64_t>(), ws->sort_out.as<int64_t>()); }));
		{
			KernelTimer kt(st, K_PREP);
			hipLaunchKernelGGL(k_sort_scatter, dim3(blocks_for(n)), dim3(256), 0, st, n, ws->sidx.as<u32>(), ws->sort_out.as<int64_t>(), d_out_len);
			kt.stop();
			S.algo_bytes[K_PREP] += (double)n * 20.0;
		}
		PGQ_WAIT(st);
		KernelTimer::flush();
		*took = true;
		return PGQ_OK;
	}
	// ---- the memo record: what the chain said about these buffers; whether the sort by source took them ----
	void record(const MemoOutcome &o) { if (write_memo) memo_record(c, n, d_src, d_dst, o); }
	void record_prepass(const PrepassResult &r) {
		MemoOutcome o;
		if ((ball == BallMode::Decide || ball == BallMode::Only) && ask.ball_hint < 0) o.ball = r.ball_took; // what the kernels said about these buffers
		// these rows look like a cross product now: gated again next time
		if (decide) o.go = r.answered && !(decide_mode == DecideMode::Ride && r.observed_go == 0 && !r.ball_took);
		record(o);
	}
	void record_sorted(bool took) { MemoOutcome o; o.sorted = took; record(o); }
};
int search_device(pgq_csr *c, Workspace *ws, const SearchCall &call, SearchReport &rep) { return Route(c, ws, call, rep).search(); }

static int check_csr(pgq_csr_t *csr, int64_t V) {
	if (!csr) return fail(PGQ_ERR_INVALID_ARG, "Constraint Error: Need to initialize CSR before doing shortest path");
	if (V != csr->V) return fail(PGQ_ERR_INVALID_ARG, "V does not match the uploaded CSR");
	return PGQ_OK;
}

} // namespace pgq

using namespace pgq;

// per-thread arena for list payloads returned by the chunk API
static thread_local std::vector<int64_t> t_child;
namespace pgq {
std::vector<int64_t> &thread_child_arena() { return t_child; }
} // namespace pgq

// body(k, lo, hi, replica, ws): shard k = rows [lo, hi) on device k's replica, called on a thread bound to that device
template <typename Body>
static int run_shards(pgq_csr_t *csr, int64_t n, Body body) {
	PGQ_TRY(pgq_csr_replicate(csr));
	std::vector<int> devs;
	std::vector<pgq_csr *> replicas;
	{ // a snapshot: another caller may rebuild the list for a new device set meanwhile (old replicas stay alive)
		std::lock_guard<std::mutex> g(csr->replica_lock);
		devs = csr->replica_devices;
		replicas = csr->replicas;
	}
	const int W = (int)devs.size();
	if (W == 0 || replicas.size() != (size_t)W) return fail(PGQ_ERR_INVALID_ARG, "CSR replicas do not match the enabled devices");
	for (int k = 0; k < W; k++)
		if (!replicas[(size_t)k] || replicas[(size_t)k]->device != devs[(size_t)k])
			return fail(PGQ_ERR_INVALID_ARG, "CSR replica on the wrong device");
	const int64_t per = (n + W - 1) / W;
	return fan_out(devs, [&](int k) -> int {
		const int64_t lo = std::min<int64_t>((int64_t)k * per, n), hi = std::min<int64_t>(lo + per, n);
		if (hi == lo) return PGQ_OK;
		WorkspaceLease lease;
		PGQ_TRY(lease.acquire());
		return body(k, lo, hi, replicas[(size_t)k], lease.ws);
	});
}

extern "C" {

void pgq_thread_release(void) {
	t_child.clear();
	t_child.shrink_to_fit();
}

int pgq_release_cached_memory(void) {
	PGQ_TRY(ensure_init());
	drop_idle_workspaces();
	dev_cache_trim(); // and the freed CSR / upload blocks kept for the next upload
	return PGQ_OK;
}

// max_hops: null = unbounded
static int iterativelength_bulk(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t *d_out_len, bool bidir, const int64_t *max_hops = nullptr) {
	const bool arrays = d_src && d_dst && d_out_len;
	auto check = [&]() -> int {
		PGQ_TRY(check_arrays(csr, n, arrays, "NULL device array"));
		if (max_hops && *max_hops < 0) return fail(PGQ_ERR_INVALID_ARG, "max_hops must not be negative");
		return PGQ_OK;
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		SearchCall call { n, d_src, d_dst, d_out_len };
		call.ask.bidir = bidir;
		call.ask.max_hops = max_hops ? search_bound(csr, *max_hops) : -1;
		SearchReport rep;
		PGQ_TRY(search_device(csr, ws, call, rep));
		if (call.ask.max_hops >= 0 && n > 0) {
			hipLaunchKernelGGL(k_clamp_hops, dim3(blocks_for(n)), dim3(256), 0, ws->stream, n, call.ask.max_hops, d_out_len);
			PGQ_HIP_TRY(hipStreamSynchronize(ws->stream));
		}
		return PGQ_OK;
	});
}
int pgq_iterativelength_within_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t max_hops,
                                           int64_t *d_out_len) {
	return iterativelength_bulk(csr, n, d_src, d_dst, d_out_len, false, &max_hops);
}
int pgq_iterativelength_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst,
                                    int64_t *d_out_len) {
	return iterativelength_bulk(csr, n, d_src, d_dst, d_out_len, false);
}
int pgq_iterativelength_bidirectional_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst,
                                                  int64_t *d_out_len) {
	return iterativelength_bulk(csr, n, d_src, d_dst, d_out_len, true);
}
int pgq_traversed_edges_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst,
                                    int64_t *d_out_len, int64_t *d_out_te) {
	const bool arrays = d_src && d_dst && d_out_len && d_out_te;
	return c_entry<true>(csr, [&] { return check_arrays(csr, n, arrays, "NULL device array"); }, [&](Workspace *ws) -> int {
		SearchCall call { n, d_src, d_dst, d_out_len };
		call.ask.want_te = true;
		SearchReport rep;
		PGQ_TRY(search_device(csr, ws, call, rep));
		if (n > 0) {
			hipLaunchKernelGGL(k_scatter_te, dim3(blocks_for(n)), dim3(256), 0, ws->stream, n, ws->sidx.as<u32>(), ws->ste.as<int64_t>(), d_out_te);
			PGQ_HIP_TRY(hipStreamSynchronize(ws->stream));
		}
		return PGQ_OK;
	});
}

// shortestpath_within, behind search_device: the stages lay out no list of a row beyond the bound (k_path_counts, batch_paths),
// and this is where the entry points hold them to it.  path_bound_broken: one launch over the lengths and one wait (the chunk
// form looks at the lengths it has downloaded anyway).  pack_within_bound, when a stage did report such a row: those rows become
// NULL, the other rows' lists are packed in row order and rep.child_used counts those alone.  `lists`: the lists were written
// (at d_child); without them (the caller's buffer was too small) only the lengths, offsets and the count are put right.
static int path_bound_broken(Workspace *ws, const SearchCall &call, bool *broken) {
	*broken = false;
	if (call.ask.max_hops < 0 || call.n == 0) return PGQ_OK;
	u32 *flag = &ws->h_meet->sample_go; // pinned, device-addressable; no chain is in flight behind a finished search
	*flag = 0;
	hipLaunchKernelGGL(k_bound_check, dim3(blocks_for(call.n)), dim3(256), 0, ws->stream, call.n, call.ask.max_hops, call.d_out_len, flag);
	PGQ_HIP_TRY(hipStreamSynchronize(ws->stream));
	*broken = *flag != 0;
	*flag = 0;
	return PGQ_OK;
}
static int pack_within_bound(Workspace *ws, const SearchCall &call, SearchReport &rep, int64_t *d_child, bool lists) {
	const int64_t n = call.n, bound = call.ask.max_hops;
	hipStream_t st = ws->stream;
	PGQ_TRY(ws->meet_poff.reserve((size_t)(n + 1) * 8 * 2));
	int64_t *noff = ws->meet_poff.as<int64_t>(), *cnt = noff + (n + 1), total = 0;
	PGQ_HIP_TRY(hipMemsetAsync(cnt + n, 0, 8, st));
	hipLaunchKernelGGL(k_bound_counts, dim3(blocks_for(n)), dim3(256), 0, st, n, bound, call.d_out_len, cnt);
	PGQ_TRY(cub_run(ws->scan_tmp, [&](void *tmp, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(tmp, tb, cnt, noff, (int)(n + 1), st); }));
	PGQ_HIP_TRY(hipMemcpyAsync(&total, noff + n, 8, hipMemcpyDeviceToHost, st));
	PGQ_HIP_TRY(hipStreamSynchronize(st));
	const bool copy = lists && total > 0;
	DevBuf packed;
	int rc = copy ? packed.reserve((size_t)total * 8) : PGQ_OK;
	if (rc == PGQ_OK) {
		hipLaunchKernelGGL(k_bound_pack, dim3(blocks_for(n)), dim3(256), 0, st, n, bound, call.d_out_len, call.paths->d_out_off, noff, d_child,
		                   copy ? packed.as<int64_t>() : nullptr);
		if (copy && hipMemcpyAsync(d_child, packed.p, (size_t)total * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = fail(PGQ_ERR_HIP, "packing the path lists failed");
		if (hipStreamSynchronize(st) != hipSuccess && rc == PGQ_OK) rc = fail(PGQ_ERR_HIP, "packing the path lists failed");
	}
	packed.release();
	rep.child_used = total;
	return rc;
}
static int enforce_path_bound(Workspace *ws, const SearchCall &call, SearchReport &rep, int64_t *d_child, bool lists) {
	bool broken = false;
	PGQ_TRY(path_bound_broken(ws, call, &broken));
	return broken ? pack_within_bound(ws, call, rep, d_child, lists) : PGQ_OK;
}

// max_hops: null = unbounded
static int shortestpath_bulk(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t *d_out_len, int64_t *d_out_offset,
                             int64_t *d_child, int64_t child_cap, int64_t *child_used, const int64_t *max_hops = nullptr) {
	const bool arrays = d_src && d_dst && d_out_len && d_out_offset && d_child;
	auto check = [&]() -> int {
		PGQ_TRY(check_arrays(csr, n, arrays, "NULL device array"));
		if (max_hops && *max_hops < 0) return fail(PGQ_ERR_INVALID_ARG, "max_hops must not be negative");
		return PGQ_OK;
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) {
		SearchCall call { n, d_src, d_dst, d_out_len, SearchPaths { d_out_offset, d_child, child_cap } };
		call.ask.max_hops = max_hops ? search_bound(csr, *max_hops) : -1;
		SearchReport rep;
		int rc = search_device(csr, ws, call, rep);
		// (a search that failed for want of room in `d_child` has still written every length: the count is put right for them too)
		if (rc == PGQ_OK || rep.overflow) {
			const int rc2 = enforce_path_bound(ws, call, rep, d_child, rc == PGQ_OK);
			if (rc == PGQ_OK) rc = rc2;
		}
		if (child_used) *child_used = rep.child_used;
		return rc;
	});
}
int pgq_shortestpath_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t *d_out_len,
                                 int64_t *d_out_offset, int64_t *d_child, int64_t child_cap, int64_t *child_used) {
	return shortestpath_bulk(csr, n, d_src, d_dst, d_out_len, d_out_offset, d_child, child_cap, child_used);
}
int pgq_shortestpath_within_bulk_device(pgq_csr_t *csr, int64_t n, const int64_t *d_src, const int64_t *d_dst, int64_t max_hops,
                                        int64_t *d_out_len, int64_t *d_out_offset, int64_t *d_child, int64_t child_cap, int64_t *child_used) {
	return shortestpath_bulk(csr, n, d_src, d_dst, d_out_len, d_out_offset, d_child, child_cap, child_used, &max_hops);
}

// Multi-GPU inside one process (the single DuckDB process the boundary targets): rows are cut into contiguous shards,
// one host thread per enabled device runs the identical single-GPU path on its shard against that device's replica of
// the CSR, and the results land in the caller's host array (the gather).  No collective inside the search
// (results are a pure function of (CSR, src, dst)).
int pgq_iterativelength_multi(pgq_csr_t *csr, int64_t n, const int64_t *src, const int64_t *dst, int64_t *out_len) {
	auto check = [&] {
		PGQ_TRY(check_arrays(csr, n, src && dst && out_len, "NULL array"));
		return n == 0 ? kNoRows : PGQ_OK;
	};
	auto shard = [&](int, int64_t lo, int64_t hi, pgq_csr_t *replica, Workspace *ws) -> int {
		const size_t bytes = (size_t)(hi - lo) * 8;
		PGQ_TRY(ws->out_len.reserve(bytes));
		PGQ_TRY(stage_pairs(ws, hi - lo, src + lo, dst + lo));
		SearchReport rep;
		PGQ_TRY(search_device(replica, ws, SearchCall { hi - lo, ws->in_src.as<int64_t>(), ws->in_dst.as<int64_t>(), ws->out_len.as<int64_t>() }, rep));
		return staged_download(out_len + lo, ws->out_len.p, bytes, ws->stream);
	};
	return c_entry<false>(csr, check, [&] { return run_shards(csr, n, shard); });
}

// shortestpath on all enabled devices: every shard writes its lists into its own device buffer (grown once if the first
// guess was too small), the payloads are then concatenated in shard order into `child` and the list offsets shifted by
// the preceding shards' sizes — the gather of the ragged [v,e,v,...] lists.
// max_hops: null = unbounded
static int shortestpath_multi(pgq_csr_t *csr, int64_t n, const int64_t *src, const int64_t *dst, int64_t *out_len,
                              int64_t *out_offset, int64_t *child, int64_t child_cap, int64_t *child_used, const int64_t *max_hops = nullptr) {
	auto check = [&] {
		PGQ_TRY(check_arrays(csr, n, src && dst && out_len && out_offset, "NULL array"));
		if (max_hops && *max_hops < 0) return fail(PGQ_ERR_INVALID_ARG, "max_hops must not be negative");
		if (child_cap < 0 || (child_cap > 0 && !child)) return fail(PGQ_ERR_INVALID_ARG, "NULL array");
		if (child_used) *child_used = 0;
		return n == 0 ? kNoRows : PGQ_OK;
	};
	std::vector<std::vector<int64_t>> payload;
	std::vector<int64_t> shard_lo, shard_hi;
	auto shard = [&](int k, int64_t lo, int64_t hi, pgq_csr_t *replica, Workspace *ws) -> int {
		const int64_t m = hi - lo;
		const size_t bytes = (size_t)m * 8;
		for (DevBuf *b : { &ws->out_len, &ws->out_off }) PGQ_TRY(b->reserve(bytes));
		PGQ_TRY(stage_pairs(ws, m, src + lo, dst + lo));
		DevBuf dchild; // not a workspace buffer: search_device uses ws->child for its own staging
		int64_t cap = std::max<int64_t>(16 * m, 1024), used = 0;
		int rc = PGQ_OK;
		for (int attempt = 0; attempt < 2; attempt++) {
			rc = dchild.reserve((size_t)cap * 8);
			if (rc != PGQ_OK) break;
			SearchCall call { m, ws->in_src.as<int64_t>(), ws->in_dst.as<int64_t>(), ws->out_len.as<int64_t>(), SearchPaths { ws->out_off.as<int64_t>(), dchild.as<int64_t>(), cap } };
			call.ask.max_hops = max_hops ? search_bound(replica, *max_hops) : -1;
			SearchReport rep;
			rc = search_device(replica, ws, call, rep);
			if (rc == PGQ_OK || rep.overflow) {
				const int rc2 = enforce_path_bound(ws, call, rep, dchild.as<int64_t>(), rc == PGQ_OK);
				if (rc == PGQ_OK) rc = rc2;
			}
			used = rep.child_used;
			if (rc == PGQ_OK || used <= cap) break;
			cap = used; // too small: the search reported what it needs
		}
		if (rc == PGQ_OK) rc = staged_download(out_len + lo, ws->out_len.p, bytes, ws->stream);
		if (rc == PGQ_OK) rc = staged_download(out_offset + lo, ws->out_off.p, bytes, ws->stream);
		if (rc == PGQ_OK) {
			payload[(size_t)k].resize((size_t)used);
			if (used > 0) rc = staged_download(payload[(size_t)k].data(), dchild.p, (size_t)used * 8, ws->stream);
		}
		shard_lo[(size_t)k] = lo;
		shard_hi[(size_t)k] = hi;
		dchild.release();
		return rc;
	};
	return c_entry<false>(csr, check, [&]() -> int {
		const size_t W = enabled_devices().size();
		payload.resize(W);
		shard_lo.assign(W, 0);
		shard_hi.assign(W, 0);
		PGQ_TRY(run_shards(csr, n, shard));
		int64_t total = 0;
		for (size_t k = 0; k < W; k++) total += (int64_t)payload[k].size();
		if (child_used) *child_used = total;
		if (total > child_cap) return fail(PGQ_ERR_INVALID_ARG, "child buffer too small for the path lists (see *child_used)");
		int64_t base = 0;
		for (size_t k = 0; k < W; k++) {
			if (!payload[k].empty()) memcpy(child + base, payload[k].data(), payload[k].size() * 8);
			if (base)
				for (int64_t i = shard_lo[k]; i < shard_hi[k]; i++)
					if (out_len[i] >= 0) out_offset[i] += base;
			base += (int64_t)payload[k].size();
		}
		return PGQ_OK;
	});
}

int pgq_shortestpath_multi(pgq_csr_t *csr, int64_t n, const int64_t *src, const int64_t *dst, int64_t *out_len,
                           int64_t *out_offset, int64_t *child, int64_t child_cap, int64_t *child_used) {
	return shortestpath_multi(csr, n, src, dst, out_len, out_offset, child, child_cap, child_used);
}
int pgq_shortestpath_within_multi(pgq_csr_t *csr, int64_t n, const int64_t *src, const int64_t *dst, int64_t max_hops, int64_t *out_len,
                                  int64_t *out_offset, int64_t *child, int64_t child_cap, int64_t *child_used) {
	return shortestpath_multi(csr, n, src, dst, out_len, out_offset, child, child_cap, child_used, &max_hops);
}

// cheapest_path_length on all enabled devices: out = n values (int64 or double by the CSR's weight type), out_valid = n
// bytes (1 = a path exists)
// (max_hops: null = unbounded; the bounded form answers a NULL handle before anything else, like its single-device forms)
static int cheapest_multi(pgq_csr_t *csr, int64_t n, const int64_t *src, const int64_t *dst, void *out, uint8_t *out_valid,
                          const int64_t *max_hops = nullptr) {
	if (max_hops && !csr) return fail(PGQ_ERR_INVALID_ARG, "NULL csr");
	auto check = [&]() -> int {
		PGQ_TRY(check_arrays(csr, n, src && dst && out && out_valid, "NULL array"));
		if (max_hops && *max_hops < 0) return fail(PGQ_ERR_INVALID_ARG, "max_hops must not be negative");
		return n == 0 ? kNoRows : PGQ_OK;
	};
	auto shard = [&](int, int64_t lo, int64_t hi, pgq_csr_t *replica, Workspace *ws) -> int {
		const int64_t m = hi - lo;
		const size_t bytes = (size_t)m * 8;
		DevBuf d_src, d_dst, d_val, d_ok; // the bulk entry point leases its own workspace
		int rc = d_src.reserve(bytes);
		if (rc == PGQ_OK) rc = d_dst.reserve(bytes);
		if (rc == PGQ_OK) rc = d_val.reserve(bytes);
		if (rc == PGQ_OK) rc = d_ok.reserve((size_t)m);
		if (rc == PGQ_OK && (hipMemcpyAsync(d_src.p, src + lo, bytes, hipMemcpyHostToDevice, ws->stream) != hipSuccess ||
		                     hipMemcpyAsync(d_dst.p, dst + lo, bytes, hipMemcpyHostToDevice, ws->stream) != hipSuccess ||
		                     hipStreamSynchronize(ws->stream) != hipSuccess))
			rc = fail(PGQ_ERR_HIP, "copying a shard's rows to its device failed");
		if (rc == PGQ_OK)
			rc = max_hops ? pgq_cheapest_path_length_within_bulk_device(replica, m, d_src.as<int64_t>(), d_dst.as<int64_t>(), *max_hops, d_val.p,
			                                                            d_ok.as<uint8_t>())
			              : pgq_cheapest_path_length_bulk_device(replica, m, d_src.as<int64_t>(), d_dst.as<int64_t>(), d_val.p, d_ok.as<uint8_t>());
		if (rc == PGQ_OK) rc = staged_download(static_cast<char *>(out) + (size_t)lo * 8, d_val.p, bytes, ws->stream);
		if (rc == PGQ_OK) rc = staged_download(out_valid + lo, d_ok.p, (size_t)m, ws->stream);
		for (DevBuf *b : { &d_src, &d_dst, &d_val, &d_ok }) b->release();
		return rc;
	};
	return c_entry<false>(csr, check, [&] { return run_shards(csr, n, shard); });
}
int pgq_cheapest_path_length_multi(pgq_csr_t *csr, int64_t n, const int64_t *src, const int64_t *dst, void *out,
                                   uint8_t *out_valid) {
	return cheapest_multi(csr, n, src, dst, out, out_valid);
}
int pgq_cheapest_path_length_within_multi(pgq_csr_t *csr, int64_t n, const int64_t *src, const int64_t *dst, int64_t max_hops, void *out,
                                          uint8_t *out_valid) {
	return cheapest_multi(csr, n, src, dst, out, out_valid, &max_hops);
}

// pinned, device-addressable staging block of a workspace (grown on demand)
static int io_block(Workspace *ws, size_t bytes, void **host, void **dev) {
	if (ws->h_io_cap < bytes) {
		if (ws->h_io) (void)hipHostFree(ws->h_io);
		ws->h_io = nullptr;
		ws->h_io_cap = 0;
		const size_t want = std::max<size_t>(bytes * 2, 64 << 10);
		PGQ_HIP_TRY(hipHostMalloc(&ws->h_io, want));
		ws->h_io_cap = want;
	}
	*host = ws->h_io;
	PGQ_HIP_TRY(hipHostGetDevicePointer(dev, ws->h_io, 0));
	return PGQ_OK;
}

// max_hops: null = unbounded; else the rows farther apart are NULL (clamped here, on the host's pass over the results)
static int iterativelength_chunk(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t *out_len,
                                 uint64_t *out_valid, bool bidir, const int64_t *max_hops = nullptr) {
	auto check = [&] {
		PGQ_TRY(check_csr(csr, V));
		if (max_hops && *max_hops < 0) return fail(PGQ_ERR_INVALID_ARG, "max_hops must not be negative");
		if (n < 0 || (n > 0 && (!out_len || !out_valid))) return fail(PGQ_ERR_INVALID_ARG, "NULL output");
		return n == 0 ? kNoRows : PGQ_OK;
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		const int64_t bound = max_hops ? search_bound(csr, *max_hops) : -1;
		const int64_t top = bound < 0 ? INT64_MAX : bound; // lengths above it are NULL
		SearchAsk ask; // of either branch: a chunk's staging buffers say nothing to the route memo (SearchAsk::no_memo)
		ask.no_memo = true;
		ask.max_hops = bound;
		if (!bidir && options().chunk_zero_copy && prepass_takes(csr, n, SearchAsk()) && n <= kMeetDecideRows) {
			// One DuckDB chunk through the pair-centric kernels: they read the rows straight out of a pinned staging block and
			// write the hop counts straight back into it (2048 rows = 32 KB in, 16 KB out over PCIe, one access per row), so the
			// call is two or three kernel launches and ONE wait — no copy commands (each is a stream operation of its own:
			// two in, two out cost more than the search of a chunk).
			void *hp = nullptr, *dp = nullptr;
			PGQ_TRY(io_block(ws, (size_t)n * 24, &hp, &dp));
			int64_t *h = static_cast<int64_t *>(hp), *d = static_cast<int64_t *>(dp);
			PGQ_TRY(flatten_pairs_into(V, n, src, dst, h, h + n));
			SearchCall call { n, d, d + n, d + 2 * n, std::nullopt, ask };
			{ // the rows are in host memory: whether they are grouped by source costs a pass over 2048 words here, two launches there
				int64_t runs = 1;
				for (int64_t i = 1; i < n; i++) runs += h[i] != h[i - 1];
				call.ask.ball_hint = runs * 8 <= n ? 1 : 0;
			}
			SearchReport rep;
			PGQ_TRY(search_device(csr, ws, call, rep));
			const int64_t *res = h + 2 * n;
			for (int64_t w = 0; w < (n + 63) / 64; w++) { // payload of a NULL row stays -1 like iterativelength.cpp:100,137
				uint64_t m = 0;
				const int64_t lo = w * 64, cnt = std::min<int64_t>(64, n - lo);
				for (int64_t k = 0; k < cnt; k++) {
					const int64_t v = res[lo + k] > top ? -1 : res[lo + k];
					out_len[lo + k] = v;
					m |= (uint64_t)(v >= 0) << k;
				}
				out_valid[w] = cnt == 64 ? m : (m | (~0ULL << cnt)); // bits past n stay set, as mask_fill_valid leaves them
			}
			return PGQ_OK;
		}
		FlatPairs fp;
		PGQ_TRY(flatten_pairs(V, n, src, dst, fp, false));
		PGQ_TRY(ws->out_len.reserve((size_t)n * 8));
		PGQ_TRY(stage_pairs(ws, n, fp.src.data(), fp.dst.data()));
		SearchCall call { n, ws->in_src.as<int64_t>(), ws->in_dst.as<int64_t>(), ws->out_len.as<int64_t>(), std::nullopt, ask };
		call.ask.bidir = bidir;
		SearchReport rep;
		PGQ_TRY(search_device(csr, ws, call, rep));
		PGQ_TRY(staged_download(out_len, ws->out_len.p, (size_t)n * 8, ws->stream));
		mask_fill_valid(out_valid, n);
		for (int64_t i = 0; i < n; i++) {
			if (out_len[i] > top) out_len[i] = -1;
			if (out_len[i] < 0) mask_set_invalid(out_valid, i); // payload stays -1 like iterativelength.cpp:100,137
		}
		return PGQ_OK;
	});
}
int pgq_iterativelength(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t *out_len,
                        uint64_t *out_valid) {
	return iterativelength_chunk(csr, V, n, src, dst, out_len, out_valid, false);
}
int pgq_iterativelength_within(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops, int64_t *out_len,
                               uint64_t *out_valid) {
	return iterativelength_chunk(csr, V, n, src, dst, out_len, out_valid, false, &max_hops);
}
int pgq_iterativelength_bidirectional(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t *out_len,
                                      uint64_t *out_valid) {
	return iterativelength_chunk(csr, V, n, src, dst, out_len, out_valid, true);
}

// max_hops: null = unbounded
static int shortestpath_chunk(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, uint64_t *out_offset, uint64_t *out_length,
                              uint64_t *out_valid, const int64_t **out_child, uint64_t *out_child_len, const int64_t *max_hops = nullptr) {
	auto check = [&] {
		PGQ_TRY(check_csr(csr, V));
		if (max_hops && *max_hops < 0) return fail(PGQ_ERR_INVALID_ARG, "max_hops must not be negative");
		if (n < 0 || (n > 0 && (!out_offset || !out_length || !out_valid)) || !out_child || !out_child_len)
			return fail(PGQ_ERR_INVALID_ARG, "NULL output");
		*out_child = nullptr;
		*out_child_len = 0;
		return n == 0 ? kNoRows : PGQ_OK;
	};
	return c_entry<true>(csr, check, [&](Workspace *ws) -> int {
		FlatPairs fp;
		PGQ_TRY(flatten_pairs(V, n, src, dst, fp, false));
		for (DevBuf *b : { &ws->out_len, &ws->out_off }) PGQ_TRY(b->reserve((size_t)n * 8));
		PGQ_TRY(stage_pairs(ws, n, fp.src.data(), fp.dst.data()));
		SearchCall call { n, ws->in_src.as<int64_t>(), ws->in_dst.as<int64_t>(), ws->out_len.as<int64_t>(), SearchPaths { ws->out_off.as<int64_t>() } };
		call.ask.no_memo = true;
		call.ask.max_hops = max_hops ? search_bound(csr, *max_hops) : -1;
		SearchReport rep;
		PGQ_TRY(search_device(csr, ws, call, rep));
		std::vector<int64_t> len(n), off(n);
		PGQ_TRY(staged_download(len.data(), ws->out_len.p, (size_t)n * 8, ws->stream));
		if (call.ask.max_hops >= 0 && std::any_of(len.begin(), len.end(), [&](int64_t k) { return k > call.ask.max_hops; })) {
			// (SearchAsk::max_hops: no stage is relied on — a row beyond the bound takes no room in the payload)
			PGQ_TRY(pack_within_bound(ws, call, rep, ws->child.as<int64_t>(), true));
			PGQ_TRY(staged_download(len.data(), ws->out_len.p, (size_t)n * 8, ws->stream));
		}
		PGQ_TRY(staged_download(off.data(), ws->out_off.p, (size_t)n * 8, ws->stream));
		t_child.resize((size_t)rep.child_used);
		if (rep.child_used > 0) PGQ_TRY(staged_download(t_child.data(), ws->child.p, (size_t)rep.child_used * 8, ws->stream));
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
		*out_child = t_child.data();
		*out_child_len = (uint64_t)rep.child_used;
		return PGQ_OK;
	});
}
int pgq_shortestpath(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, uint64_t *out_offset,
                     uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child, uint64_t *out_child_len) {
	return shortestpath_chunk(csr, V, n, src, dst, out_offset, out_length, out_valid, out_child, out_child_len);
}
int pgq_shortestpath_within(pgq_csr_t *csr, int64_t V, int64_t n, pgq_vec_t src, pgq_vec_t dst, int64_t max_hops, uint64_t *out_offset,
                            uint64_t *out_length, uint64_t *out_valid, const int64_t **out_child, uint64_t *out_child_len) {
	return shortestpath_chunk(csr, V, n, src, dst, out_offset, out_length, out_valid, out_child, out_child_len, &max_hops);
}

} // extern "C"
