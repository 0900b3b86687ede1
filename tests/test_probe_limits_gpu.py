"""The lane batches' deciding kernels — k_probe, k_probe2, k_detect, the deferral behind them — ON their queue and list limits.

helpers.probe_gadgets puts the one in-neighbour that answers a row at a chosen position of an in-list of 1 .. 8193 entries
(k_probe: 64 entries per trip of a wavefront; hub destinations, more than probe_max_in entries, 4 x 1024 per step of the
workgroup) and of k_probe2's two nested lists, with the two-hop walk one under, on and one over probe2_cap
(test_probe_gadgets_cpu.py proves all that on the CPU, and that a scan which loses such an entry answers a gadget wrongly).
A layered graph keeps a million rows open through two probes: 2048 per workgroup, twice k_probe's LDS queue, and with
probe_max_in 64 far more hub rows than the hub queue holds.  Row counts sit on the edges of the shared-chunk split (8192
rows: the grid stops growing; 262,144: two wavefronts per chunk become one), and the deferral on its threshold.

Every test forces the lane batches (meet 0, ball 0), every expected value is the CPU oracle's, every comparison is exact, and
every call is made twice on the same handle: the first makes a round trip per level, the second replays the stored plan
ahead of the host."""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from helpers import PROBE2_CAP, PROBE_LIMITS, probe_gadgets
from oracle.pgq_oracle import OracleCSR
from test_within_gpu import Rows, clamp

pytestmark = pytest.mark.gpu

# every option these tests depend on: the library's defaults first (another file may have left its own values)
KEYS = ("meet", "meet_bias", "meet_cap", "meet_cap_small", "meet_cap_paths", "meet4", "meet4_cap", "meet4_test_cap",
        "meet4_lds_kb", "meet4_global_mb", "meet_layout", "meet_align", "meet_pack", "meet_pack_align", "meet_small_rows",
        "meet_wide_rows", "meet_wide_rows_always", "meet_spin_wait", "paths_reserve_mb", "bibfs_rows", "bibfs_rows_max", "bibfs_cap",
        "bibfs_queue", "bibfs_grid", "wbibfs", "ball", "ball_head_mb", "ball_cap", "ball_test_cap", "ball_grid", "ball_bias",
        "ball_sort", "ball_seg_kb", "ball_seg_rows_small", "words", "max_words", "lanes", "lanes_unroll", "force_mode",
        "force_pull", "sparse_lds", "blocks_per_cu", "hub_chunk", "push_chunk", "push_div", "probe", "probe2", "defer", "streams",
        "route_timing", "route_timing_rows", "route_try_factor", "route_memo", "calibration_cache", "meet_calibrate",
        "spec_levels", "chunk_zero_copy", "probe_max_in", "probe2_cap", "probe2_div", "probe2_abs", "probe_always",
        "detect_unroll", "detect_grid_mult")


def defaults():
    for k in KEYS:
        pgq.set_option(k, pgq.get_default_option(k))


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    defaults()
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


def lanes(**options):
    """Every row through the lane batches, under `options`."""
    for k, v in dict(meet=0, ball=0, **options).items():
        pgq.set_option(k, v)


class Graph:
    """An uploaded graph and its oracle (uploaded under the library's defaults, whatever the file before left)."""

    def __init__(self, V, src, dst):
        self.V = V
        self.ora = OracleCSR.from_edges(V, src, dst)
        self.upload(src, dst)

    def upload(self, src, dst):
        saved = {k: pgq.get_option(k) for k in KEYS}
        defaults()
        self.st = pgq.PgqState()
        self.st.build_csr(0, self.V, src, dst)
        for k, v in saved.items():
            pgq.set_option(k, v)
        self.dev = self.st.device_csr(0)

    def distances(self, ps, pd):
        ln, ok = self.ora.lean_iterativelength(self.V, ps, pd, nthreads=8)
        return np.where(ok, ln, -1)

    def chunk(self, ps, pd):
        out, ok = self.dev.iterativelength(ps, pd)
        assert (out[~ok] == -1).all(), "a NULL row's payload is -1"
        return np.where(ok, out, -1)

    def close(self):
        self.st.delete_csr(0)


class Bulk:
    """The bulk form on rows that stay on the device; a prefix of them with n."""

    def __init__(self, graph, ps, pd):
        import torch
        self.dev = graph.dev
        self.t_s, self.t_d = torch.from_numpy(np.ascontiguousarray(ps)).cuda(), torch.from_numpy(np.ascontiguousarray(pd)).cuda()
        self.t_o = torch.empty(len(ps), dtype=torch.int64, device="cuda")

    def __call__(self, n=None):
        n = len(self.t_s) if n is None else n
        self.t_o.fill_(-7)
        self.dev.iterativelength_bulk_ptr(n, self.t_s.data_ptr(), self.t_d.data_ptr(), self.t_o.data_ptr())
        return self.t_o[:n].cpu().numpy()


def twice(call, want, what, tags=None):
    """`call` two times (a round trip per level, then the stored plan ahead of the host): both answer `want`, both through the
    lane batches alone.  Returns the statistics of the two calls."""
    seen = []
    for turn in ("first call", "second call"):
        pgq.reset_stats()
        got = call()
        stats = pgq.get_stats()
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, "%s, %s: %d of %d rows differ, first: row %d%s got %d, expected %d" % (
            what, turn, len(bad), len(want), bad[0], "" if tags is None else " (gadget %s)" % tags[bad[0]], got[bad[0]], want[bad[0]])
        assert stats["meet_pairs"] == 0 and stats["ball_calls"] == 0 and stats["launches"]["detect"] > 0, (
            what, turn, stats["meet_pairs"], stats["ball_calls"], stats["launches"])
        seen.append(stats)
    return seen


# ---- the gadgets -----------------------------------------------------------------------------------------------------------
class GadgetCase(Graph):
    def __init__(self):
        g = self.g = probe_gadgets()
        super().__init__(g.V, g.src, g.dst)
        self.dist = self.distances(g.rs, g.rd)
        assert (self.dist == g.dist).all()  # the builder's own distances (test_probe_gadgets_cpu.py): the expected values are the oracle's


@pytest.fixture(scope="module")
def gadgets():
    case = GadgetCase()
    yield case
    case.close()


def run_both_forms(case, rows, what):
    g = case.g
    ps, pd, want, tags = g.rs[rows], g.rd[rows], case.dist[rows], g.tag[rows]
    bulk = Bulk(case, ps, pd)
    return [twice(lambda: case.chunk(ps, pd), want, what + ", chunk form", tags), twice(bulk, want, what + ", bulk form", tags)]


# a. k_probe alone decides: no two-hop probe in front of the list the gadget is about
@pytest.mark.parametrize("words", [1, 8])
@pytest.mark.parametrize("max_in", [PROBE_LIMITS["probe_max_in"], 64])
def test_one_hop_gadgets_probe(gadgets, max_in, words):
    lanes(probe=1, probe_always=1, probe2=0, probe_max_in=max_in, words=words)
    every = np.arange(len(gadgets.g.rs))
    run_both_forms(gadgets, every, "probe_max_in %d, words %d" % (max_in, words))


@pytest.mark.parametrize("unroll", [1, 2, 4])
def test_one_hop_gadgets_detect(gadgets, unroll):
    every = np.arange(len(gadgets.g.rs))
    for words in (1, 8):
        lanes(probe=0, detect_unroll=unroll, words=words)
        run_both_forms(gadgets, every, "probe 0, detect_unroll %d, words %d" % (unroll, words))


# b. k_probe2 answers level + 1
def two_hop_rows(g):
    near = g.rows_where(lambda x: x["kind"] == "two" and x["k"] == 2 and x["walk"] <= PROBE2_CAP)
    over = g.rows_where(lambda x: x["kind"] == "two" and x["k"] == 2 and x["walk"] > PROBE2_CAP)
    far = g.rows_where(lambda x: x["kind"] == "two" and x["k"] == 3)
    direct = g.rows_where(lambda x: x["kind"] == "one" and x["k"] == 1)
    return near, over, far, direct


def test_two_hop_gadgets_levels(gadgets):
    """Path evidence: with every row two hops away and within the cap, the probe pair of level 1 answers the whole call and no
    expansion counts (levels == 0); one row over the cap stays open behind k_probe2, and a level runs for it."""
    g = gadgets.g
    near, over, _, _ = two_hop_rows(g)
    assert len(near) >= 128 and len(over) >= 8
    lanes(probe=1, probe_always=1, probe2=1, probe2_cap=PROBE2_CAP, words=1)
    for part in (near[:64], near[64:128], near[-64:]):
        assert len(set(g.rs[part].tolist())) == 64  # one lane each: the open count stays under run_below, whose floor is 64
        for stats in run_both_forms(gadgets, part, "64 two-hop rows within the cap"):
            print("within the cap: levels", [s["levels"] for s in stats], "detect launches", [s["launches"]["detect"] for s in stats])
            assert [s["levels"] for s in stats] == [0, 0]
    for k in range(0, len(over), max(1, len(over) // 6)):
        mixed = np.concatenate([near[:31], over[k:k + 1], near[31:63]])
        for stats in run_both_forms(gadgets, mixed, "63 two-hop rows within the cap, one over it"):
            print("one over the cap: levels", [s["levels"] for s in stats])
            assert all(s["levels"] >= 1 for s in stats)


@pytest.mark.parametrize("upper", [1, 2, 3])
def test_two_hop_gadgets_within_a_bound(gadgets, upper):
    # k_probe2 answers level + 1: at the last level a bound admits that is one past the bound
    g = gadgets.g
    near, over, far, _ = two_hop_rows(g)
    pick = np.concatenate([near[::4][:32], over[:8], far[:24]])
    assert len(pick) == 64 and set(gadgets.dist[pick].tolist()) == {2, 3}
    lanes(probe=1, probe_always=1, probe2=1, probe2_cap=PROBE2_CAP, words=1)
    rows = Rows(gadgets.st, g.V, g.rs[pick], g.rd[pick])
    want = clamp(gadgets.dist[pick], rows.valid, upper)
    for form in ("chunk", "bulk"):
        twice(lambda: getattr(rows, form)(upper), want, "max_hops %d, %s form" % (upper, form), g.tag[pick])


@pytest.mark.parametrize("n", [65, 129])
def test_two_hop_gadgets_chunk_shared_by_workgroups(gadgets, n):
    # other values of B, the workgroups that share a 64-row chunk: 64 rows give 64, 65 give 32, 129 give 43.  One batch of 512
    # lanes; the rows one hop away are k_probe's at level 1, what it leaves open is within k_probe2's run_below
    g = gadgets.g
    near, over, far, direct = two_hop_rows(g)
    two = np.concatenate([near[:n // 2 - 8], over[:4], far[:4]])
    pick = np.concatenate([two, direct[:n - len(two)]])
    pick = pick[np.random.default_rng(n).permutation(n)]
    assert len(pick) == n and len(set(g.rs[pick].tolist())) == n
    lanes(probe=1, probe_always=1, probe2=1, probe2_cap=PROBE2_CAP, words=8)
    run_both_forms(gadgets, pick, "%d rows" % n)


# f. k_probe in front of shortestpath's levels (k_open_merge behind it, no k_probe2)
def test_one_hop_gadgets_paths(gadgets):
    g = gadgets.g
    rows = g.rows_where(lambda x: x["kind"] == "one" and x["b"] >= 1023)
    assert len(rows) >= 3 * 40 and set(gadgets.dist[rows].tolist()) == {1, 2, 3}
    ps, pd = g.rs[rows], g.rd[rows]
    want = gadgets.ora.lean_shortestpath(g.V, ps, pd)
    assert all(len(p) == 2 * k + 1 for p, k in zip(want, gadgets.dist[rows]))
    for max_in in (PROBE_LIMITS["probe_max_in"], 64):
        for words in (1, 8):
            lanes(probe=1, probe_always=1, probe_max_in=max_in, words=words)
            for turn in ("first call", "second call"):
                pgq.reset_stats()
                got = gadgets.dev.shortestpath(ps, pd)
                stats = pgq.get_stats()
                bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
                assert not bad, "probe_max_in %d, words %d, %s: %d of %d lists differ, first: gadget %s got %s, expected %s" % (
                    max_in, words, turn, len(bad), len(want), g.tag[rows[bad[0]]], got[bad[0]], want[bad[0]])
                assert stats["meet_pairs"] == 0 and stats["ball_calls"] == 0 and stats["launches"]["detect"] > 0


# ---- c. the pooled queue and the hub queue over their capacity -------------------------------------------------------------
N_SOURCES, N_DESTS = 64, 16384


class LayeredCase(Graph):
    """64 sources -> layer A -> layer B -> half of the destinations, and B -> layer C -> the other half.  A source reaches a few
    vertices of B and C, every destination has 65 .. 80 in-neighbours, so a row is at distance 3 or 4 or unreachable: open at the
    probes of levels 1 and 2 wherever it lies in the batch."""

    def __init__(self, seed=7):
        rng = np.random.default_rng(seed)
        nA, nB, nC = 600, 3000, 3000
        ids = np.cumsum([0, N_SOURCES, nA, nB, nC, N_DESTS])
        S, A, B, C, D = (np.arange(lo, hi, dtype=np.int64) for lo, hi in zip(ids[:-1], ids[1:]))
        es, ed = [], []

        def fan_in(frm, to, lo, hi):  # every vertex of `to` gets lo .. hi - 1 in-neighbours out of `frm`
            n = rng.integers(lo, hi, len(to))
            es.append(rng.choice(frm, n.sum()))
            ed.append(np.repeat(to, n))

        def fan_out(frm, to, k):
            es.append(np.repeat(frm, k))
            ed.append(rng.choice(to, k * len(frm)))

        fan_out(S, A, 6)
        fan_out(A, B, 3)
        fan_in(B, C, 1, 2)
        fan_in(B, D[:N_DESTS // 2], 65, 81)
        fan_in(C, D[N_DESTS // 2:], 65, 81)
        src, dst = np.concatenate(es), np.concatenate(ed)
        super().__init__(int(ids[-1]), src, dst)
        assert np.bincount(dst, minlength=self.V)[D].min() >= 65
        dests = D[rng.permutation(N_DESTS)]
        self.ps, self.pd = np.tile(S, N_DESTS), np.repeat(dests, N_SOURCES)  # 64 rows per destination, one per source
        self.dist = self.distances(self.ps, self.pd)
        self.rows = Bulk(self, self.ps, self.pd)


@pytest.fixture(scope="module")
def layered():
    case = LayeredCase()
    d = case.dist
    assert len(d) == 1 << 20 and set(d.tolist()) <= {-1, 3, 4}, "no row closer than 3: every row is open at two probes"
    assert (d == 3).mean() >= 0.10 and (d == 4).mean() >= 0.10 and (d == -1).mean() >= 0.10
    yield case
    case.close()


@pytest.mark.parametrize("max_in", [PROBE_LIMITS["probe_max_in"], 64])
def test_queue_overflow(layered, max_in):
    # 16384 chunks over 8192 wavefronts: every workgroup finds 2048 open rows, twice kQueue; at probe_max_in 64 each of them is a
    # hub row, eight times kHubQueue
    assert len(layered.dist) // 64 == 2 * PROBE_LIMITS["kOpenGrid"] * 16
    assert len(layered.dist) // PROBE_LIMITS["kOpenGrid"] == 2 * PROBE_LIMITS["kQueue"] == 8 * PROBE_LIMITS["kHubQueue"]
    lanes(probe=1, probe_always=1, probe_max_in=max_in, words=1)
    twice(layered.rows, layered.dist, "2048 open rows per workgroup, probe_max_in %d" % max_in)


@pytest.mark.parametrize("extra", [0, 64])
def test_queue_exactly_full(layered, extra):
    # 8192 chunks: 1024 open rows per workgroup, the queue exactly full; one chunk more: the first workgroup's does not fit
    n = PROBE_LIMITS["kOpenGrid"] * PROBE_LIMITS["kQueue"] + extra
    lanes(probe=1, probe_always=1, words=1)
    twice(lambda: layered.rows(n), layered.dist[:n], "%d rows" % n)


# ---- d. row counts on the edges of the shared-chunk split ---------------------------------------------------------------------
ROW_COUNTS = (1, 63, 64, 65, 1023, 1025, 8191, 8192, 8193, 8256, 262_080, 262_144, 262_145, 262_208)


class RandomCase(Graph):
    def __init__(self, seed=11):
        rng = np.random.default_rng(seed)
        V, n = 4096, max(ROW_COUNTS)
        src, dst = rng.integers(0, V, 4 * V), rng.integers(0, V, 4 * V)
        super().__init__(V, src.astype(np.int64), dst.astype(np.int64))
        sources = rng.choice(V, 32, replace=False)
        self.ps, self.pd = sources[rng.integers(0, 32, n)].astype(np.int64), rng.integers(0, V, n).astype(np.int64)
        self.dist = self.distances(self.ps, self.pd)
        self.rows = Bulk(self, self.ps, self.pd)


@pytest.fixture(scope="module")
def random_case():
    case = RandomCase()
    d = case.dist
    assert (d < 0).mean() > 0.01 and all((d == k).any() for k in (0, 1, 2)) and all((d == k).mean() > 0.01 for k in range(3, 9)), np.bincount(d[d >= 0])
    assert (d[:63] > 1).any()  # the smallest calls have something to search for too (the first row alone may be anything)
    yield case
    case.close()


@pytest.mark.parametrize("setting", ["probe", "detect"])
def test_row_count_edges(random_case, setting):
    # 8192 rows: one wavefront per row, the grid stops growing (kOpenGrid); 262,144: G = 2 wavefronts per chunk, one row more: 1,
    # the pooled queue; k_detect: 4 rows per thread, the tail padded
    assert {PROBE_LIMITS["kOpenGrid"] * 16 + k for k in (-1, 0, 1)} <= set(ROW_COUNTS)
    assert {PROBE_LIMITS["kOpenGrid"] * 16 * 32 + k for k in (0, 1)} <= set(ROW_COUNTS)
    if setting == "probe":
        lanes(probe=1, probe_always=1)
    else:
        lanes(probe=0, detect_unroll=4)
    for n in ROW_COUNTS:
        twice(lambda: random_case.rows(n), random_case.dist[:n], "%s, %d rows" % (setting, n))


# ---- e. deferral on its threshold -------------------------------------------------------------------------------------------
def deferral_graph(n_far):
    """512 sources x 8 destinations, an edge from every source to every destination but for n_far pairs, which a chain of six
    edges joins instead."""
    S, D = np.arange(512, dtype=np.int64), 512 + np.arange(8, dtype=np.int64)
    ps, pd = np.repeat(S, 8), np.tile(D, 512)
    far = (ps < n_far) & (pd - 512 == ps % 8)
    assert far.sum() == n_far
    inner = 520 + np.arange(5 * n_far, dtype=np.int64).reshape(n_far, 5)
    chains = np.concatenate([ps[far][:, None], inner, pd[far][:, None]], axis=1)
    src = np.concatenate([ps[~far], chains[:, :-1].ravel()])
    dst = np.concatenate([pd[~far], chains[:, 1:].ravel()])
    return 520 + 5 * n_far, src, dst, ps, pd, far


def test_deferral_threshold():
    """A batch of 512 lanes and 4096 rows ends when a probe leaves at most stop = min(512 / 8, 4096 / 8) = 64 rows open: 64 rows
    six hops away are deferred after the probe of level 1 (deferred_pairs == 64), 65 are not (0: the batch runs on, and the probe
    of level 6 answers all of them at once)."""
    seen = {}
    for n_far in (64, 65):
        V, src, dst, ps, pd, far = deferral_graph(n_far)
        case = Graph(V, src, dst)
        want = case.distances(ps, pd)
        assert (want[far] == 6).all() and (want[~far] == 1).all()
        lanes(probe=1, probe_always=1, words=8, defer=8)
        stats = twice(lambda: case.chunk(ps, pd), want, "%d far rows" % n_far)
        case.close()
        seen[n_far] = [s["deferred_pairs"] for s in stats]
        print("%d far rows: deferred_pairs %s, levels %s, batches %s" % (
            n_far, seen[n_far], [s["levels"] for s in stats], [s["batches"] for s in stats]))
    assert seen[64] == [64, 64] and seen[65] == [0, 0], seen
