"""The bit-map kernels on both sides of their LDS limits (helpers.LDS_LIMITS): V = limit and V = limit + 1.

k_src_ball, k_meet4d / k_meet4, k_bibfs, k_pull_lanes and k_pull_sparse keep a per-vertex (or frontier) bit map in LDS when
it fits and switch to a global-memory map (or, for k_src_ball, to one workgroup per CU) above that; the host decides from V
alone.  Each case runs a graph of ~12 k active vertices spread over [0, V) — ids in the map's last word and last 128-vertex
block, chains for distances 5 to 10, unreachable pairs, a hub, multi-edges — and checks
  - every iterativelength row (NULL rows and src == dst rows among them) and a slice of shortestpath lists against the
    CPU oracle;
  - which variant ran: lds_map_launches equals launches for the kernel's class at the limit and is 0 one vertex above it
    (the pre-pass chain passes what a stage left open on to the next one, so right answers alone would not show it).
    Above its two-per-CU edge k_src_ball keeps its map in LDS on one workgroup per CU: there both sides are LDS;
  - that the kernel under test answered rows itself."""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from helpers import LDS_LIMITS, sparse_ids_graph
from oracle.pgq_oracle import OracleCSR

pytestmark = pytest.mark.gpu

WDS = (1, 2, 4, 8, 16, 32)
CASES = [("ball_2_per_cu", 0), ("ball_1_per_cu", 0), ("meet4", 0), ("bibfs", 0)] + \
        [("pull_lanes", wd) for wd in WDS] + [("pull_sparse", wd) for wd in WDS]

# every option these cases depend on: the library's defaults first (another test file may have left its own values), then
# each case's own
KEYS = ("meet", "meet_bias", "meet_cap", "meet_cap_small", "meet_cap_paths", "meet4", "meet4_cap", "meet4_test_cap",
        "meet4_lds_kb", "meet4_global_mb", "meet_layout", "meet_small_rows", "bibfs_rows", "bibfs_cap", "bibfs_queue",
        "bibfs_grid", "ball", "ball_head_mb", "ball_cap", "ball_test_cap", "ball_grid", "ball_bias", "words", "lanes",
        "force_mode", "force_pull", "sparse_lds", "wbibfs", "blocks_per_cu")


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k in KEYS:
        pgq.set_option(k, pgq.get_default_option(k))
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


def where(row, wd):
    return "helpers.LDS_LIMITS[%r]%s" % (row, "[%d]" % wd if wd else "")


def lens(out, ok):
    return [int(v) if k else None for v, k in zip(out, ok)]


class Case:
    """One graph at one V, its oracle, and candidate rows with their oracle distances."""

    def __init__(self, V, seed):
        rng = self.rng = np.random.default_rng(seed)
        self.V = V
        act, s, d, hubs, chains = sparse_ids_graph(rng, V, 12000, 30000, hubs=1, chains=8, chain_len=10)
        self.act, self.s, self.d, self.hubs, self.chains = act, s, d, hubs, chains
        self.ora = OracleCSR.from_edges(V, s, d)
        top = V - 1
        ends = np.array([0, V - 1, V - 2, V // 2, top // 32 * 32, top // 128 * 128, hubs[0]], dtype=np.int64)
        ps = [act[rng.integers(0, len(act), 1500)], np.repeat(ends, 8), rng.choice(ends, 60)]
        pd = [act[rng.integers(0, len(act), 1500)], rng.choice(act, 8 * len(ends)), np.repeat(ends, 60 // len(ends) + 1)[:60]]
        for c in chains:  # every pair along a chain (distance j - i) and against it (unreachable)
            i, j = np.triu_indices(len(c), 1)
            ps += [c[i], c[j]]
            pd += [c[j], c[i]]
        ps, pd = np.concatenate(ps).astype(np.int64), np.concatenate(pd).astype(np.int64)
        same = rng.random(len(ps)) < 0.01  # src == dst rows
        pd[same] = ps[same]
        perm = rng.permutation(len(ps))
        self.ps, self.pd = ps[perm], pd[perm]
        self.valid = rng.random(len(ps)) > 0.03  # NULL rows
        oln, ook = self.ora.lean_iterativelength(V, self.ps, self.pd, nthreads=8)
        self.dist = np.where(ook, oln, -1)
        assert (self.dist == 4).any() and (self.dist >= 5).sum() >= 100 and (self.dist < 0).any()

    def want(self, sel=slice(None), valid=None):
        valid = self.valid[sel] if valid is None else valid
        return [int(v) if (v >= 0 and ok) else None for v, ok in zip(self.dist[sel], valid)]

    def upload(self):
        st = pgq.PgqState()
        st.build_csr(0, self.V, self.s, self.d)
        return st


def check_placement(stats, kclass, lds, row, wd, V, what):
    n, in_lds = stats["launches"][kclass], stats["lds_map_launches"][kclass]
    assert n >= 1, "%s: no %s launch at V = %d (%s)" % (what, kclass, V, where(row, wd))
    want = n if lds else 0
    assert in_lds == want, (
        "%s at V = %d: %d of %d %s launches had their map in LDS, expected %d.  The host's LDS edge for this kernel moved: "
        "update %s (test_lds_budget_cpu.py recomputes it from the built kernels)" % (what, V, in_lds, n, kclass, want, where(row, wd)))


def run_ball(case, row, lds):
    # k_src_ball takes rows grouped by source (ball = 2: always); what it leaves open goes on through the older routes
    V, rng = case.V, case.rng
    pgq.set_option("meet", 1)
    pgq.set_option("meet_bias", 1e9)
    pgq.set_option("ball", 2)
    runs = [1, 3, 64, 700, 1024, 300, 1, 90, 500, 5]
    srcs = np.concatenate([[0, V - 1, V - 2, case.hubs[0], case.chains[0][0]], case.act[rng.integers(0, len(case.act), 5)]])
    ps = np.concatenate([np.full(r, s, dtype=np.int64) for s, r in zip(srcs, runs)])
    pool = np.concatenate([case.act] + case.chains)
    pd = pool[rng.integers(0, len(pool), len(ps))].astype(np.int64)
    pd[::97] = ps[::97]
    valid = np.ones(len(ps), dtype=bool)
    valid[len(ps) // 2:len(ps) // 2 + 37] = False
    oln, ook = case.ora.lean_iterativelength(V, ps, pd, nthreads=8)
    want = [int(v) if (k and vv) else None for v, k, vv in zip(oln, ook, valid)]
    for head_mb in (512, 0):  # in-list heads at a fixed stride (read at upload and launch) / list positions gathered per row
        pgq.set_option("ball_head_mb", head_mb)
        st = case.upload()
        pgq.reset_stats()
        ln, ok = st.iterativelength(0, V, ps, pd, src_valid=valid)
        assert lens(ln, ok) == want, (V, head_mb)
        stats = pgq.get_stats()
        check_placement(stats, "ball", lds, row, 0, V, "k_src_ball (ball_head_mb %d)" % head_mb)
        assert stats["ball_calls"] >= 1 and stats["meet_pairs"] > 0, (V, head_mb, stats["ball_calls"], stats["meet_pairs"])
        st.delete_csr(0)


def run_meet4(case, row, lds):
    V = case.V
    pgq.set_option("meet", 1)
    pgq.set_option("meet_bias", 1e9)
    pgq.set_option("ball", 0)
    st = case.upload()
    pgq.reset_stats()
    ln, ok = st.iterativelength(0, V, case.ps, case.pd, src_valid=case.valid)
    assert lens(ln, ok) == case.want(), V
    check_placement(pgq.get_stats(), "meet4", lds, row, 0, V, "k_meet4d")
    # rows at distance 4 alone, no k_bibfs behind it: k_meet3 answers up to 3 hops, so every row the pre-pass answers is
    # k_meet4d's
    pgq.set_option("bibfs_rows", 0)
    four = np.flatnonzero(case.dist == 4)
    pgq.reset_stats()
    ln, ok = st.iterativelength(0, V, case.ps[four], case.pd[four])
    assert lens(ln, ok) == [4] * len(four), V
    stats = pgq.get_stats()
    check_placement(stats, "meet4", lds, row, 0, V, "k_meet4d (distance-4 rows)")
    assert stats["meet_pairs"] > 0, (V, len(four), stats["levels"])
    # shortestpath through the pre-pass: k_meet4<paths>
    sl = slice(0, 600)
    pgq.reset_stats()
    got = st.shortestpath(0, V, case.ps[sl], case.pd[sl], src_valid=case.valid[sl])
    opaths = case.ora.lean_shortestpath(V, case.ps[sl], case.pd[sl])
    assert got == [p if vv else None for p, vv in zip(opaths, case.valid[sl])], V
    stats = pgq.get_stats()
    check_placement(stats, "meet4", lds, row, 0, V, "k_meet4<paths>")
    assert stats["meet_pairs"] > 0
    st.delete_csr(0)


def run_bibfs(case, row, lds):
    V = case.V
    pgq.set_option("meet", 1)
    pgq.set_option("meet_bias", 1e9)
    pgq.set_option("ball", 0)
    pgq.set_option("bibfs_rows", 4096)  # every open row of these calls, not the shipped handful
    st = case.upload()
    pgq.reset_stats()
    ln, ok = st.iterativelength(0, V, case.ps, case.pd, src_valid=case.valid)
    assert lens(ln, ok) == case.want(), V
    check_placement(pgq.get_stats(), "bibfs", lds, row, 0, V, "k_bibfs")
    # rows at distance 5 and more alone: neither two-hop kernel answers them, so the pre-pass answered them through k_bibfs
    far = np.flatnonzero(case.dist >= 5)
    pgq.reset_stats()
    ln, ok = st.iterativelength(0, V, case.ps[far], case.pd[far])
    assert lens(ln, ok) == case.dist[far].tolist(), V
    stats = pgq.get_stats()
    check_placement(stats, "bibfs", lds, row, 0, V, "k_bibfs (rows at distance >= 5)")
    assert stats["meet_pairs"] > 0, (V, len(far), stats["levels"])
    st.delete_csr(0)


def run_lanes(case, row, wd, lds):
    # the lane batches alone, every level bottom-up through the sparse kernel: k_pull_lanes (lanes = 1) / k_pull_sparse (0)
    V = case.V
    for k, v in (("meet", 0), ("force_mode", 2), ("force_pull", 1), ("sparse_lds", 1), ("words", wd),
                 ("lanes", 1 if row == "pull_lanes" else 0)):
        pgq.set_option(k, v)
    st = case.upload()
    pgq.reset_stats()
    ln, ok = st.iterativelength(0, V, case.ps, case.pd, src_valid=case.valid)
    assert lens(ln, ok) == case.want(), (V, wd)
    stats = pgq.get_stats()
    name = "k_pull_lanes<%d>" % wd if row == "pull_lanes" else "k_pull_sparse<%d>" % wd
    check_placement(stats, "pull_sparse", lds, row, wd, V, name)
    assert stats["levels"] > 0 and stats["meet_pairs"] == 0
    sl = slice(0, 400)
    pgq.reset_stats()
    got = st.shortestpath(0, V, case.ps[sl], case.pd[sl], src_valid=case.valid[sl])
    opaths = case.ora.lean_shortestpath(V, case.ps[sl], case.pd[sl])
    assert got == [p if vv else None for p, vv in zip(opaths, case.valid[sl])], (V, wd)
    check_placement(pgq.get_stats(), "pull_sparse", lds, row, wd, V, name + " (shortestpath)")
    st.delete_csr(0)


@pytest.mark.parametrize("above", [0, 1], ids=["at_limit", "limit_plus_1"])
@pytest.mark.parametrize("row,wd", CASES, ids=["%s%s" % (r, "_wd%d" % w if w else "") for r, w in CASES])
def test_bit_map_kernel_at_its_lds_limit(row, wd, above):
    limit = LDS_LIMITS[row][wd] if wd else LDS_LIMITS[row]
    V = limit + above
    # one vertex over two workgroups' maps k_src_ball still keeps its map in LDS, on one workgroup per CU
    lds = not above or row == "ball_2_per_cu"
    case = Case(V, seed=V % 100_003)
    if row.startswith("ball"):
        run_ball(case, row, lds)
    elif row == "meet4":
        run_meet4(case, row, lds)
    elif row == "bibfs":
        run_bibfs(case, row, lds)
    else:
        run_lanes(case, row, wd, lds)
