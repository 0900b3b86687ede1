"""k_meet3's tapered schedule (options meet_rows_per_wave = R and meet_tail_rows = T): the first max(0, n - T) rows, rounded
down to a multiple of R, go R consecutive rows to a wavefront, which fetches their headers together and settles the trivial
rows (NULL, src == dst, an endpoint without edges, an id out of range) in the header's lane; the rows behind them go one per
wavefront.

One small random graph with isolated vertices and a second component.  A block of rows holds every kind (NULL sources,
src == dst, endpoints with an empty list, distances 1 .. 6, unreachable pairs); a call of n rows is the block repeated from a
rotation that depends on the call, so that every kind stands in head and in tail positions over the sweep and within every
call of 257 rows.  The result buffer is pre-filled with a sentinel; no row may keep it, every row equals the CPU oracle and,
byte for byte, the meet_rows_per_wave = 1 call.  Every call is made twice."""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from oracle.pgq_oracle import OracleCSR
from test_within_gpu import clamp, payload

pytestmark = pytest.mark.gpu

KEYS = ("meet", "meet_bias", "meet_cap", "meet_cap_small", "meet_cap_paths", "meet4", "meet4_batch", "meet_pack", "meet_small_rows",
        "meet_wide_rows", "meet_wide_rows_always", "meet_grid_mult", "meet_rows_per_wave", "meet_tail_rows", "ball", "route_memo",
        "route_timing", "calibration_cache", "meet_calibrate", "chunk_zero_copy", "streams", "lanes")
SENTINEL = -7
V, VA, VB = 400, 300, 60  # component A on [0, 300), component B on [300, 360), 40 isolated vertices behind them


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k in KEYS:
        pgq.set_option(k, pgq.get_default_option(k))
    # k_meet3 sees every row of every call, and no call is a small one (those keep one row per wavefront)
    for k, v in (("meet", 1), ("meet_bias", 1e9), ("ball", 0), ("route_memo", 0), ("meet_small_rows", 0)):
        pgq.set_option(k, v)
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


class Case:
    def __init__(self):
        import torch
        rng = np.random.default_rng(14)
        # A: 1250 edges among 300 vertices (distances up to 4 and beyond), B: 250 among 60; nothing between them
        s = np.concatenate([rng.integers(0, VA, 1250), VA + rng.integers(0, VB, 250)]).astype(np.int64)
        d = np.concatenate([rng.integers(0, VA, 1250), VA + rng.integers(0, VB, 250)]).astype(np.int64)
        self.ora = OracleCSR.from_edges(V, s, d)
        self.st = pgq.PgqState()
        self.st.build_csr(0, V, s, d)
        self.dev = self.st.device_csr(0)
        outdeg, indeg = np.bincount(s, minlength=V), np.bincount(d, minlength=V)
        # all pairs of A (and a few of B) with the oracle's distance, to pick each kind from
        a, b = np.meshgrid(np.arange(VA), np.arange(VA), indexing="ij")
        a, b = a.ravel().astype(np.int64), b.ravel().astype(np.int64)
        ln, ok = self.ora.lean_iterativelength(V, a, b, nthreads=8)
        dist = np.where(ok, ln, -1)
        ps, pd, valid = [], [], []

        def add(x, y, v=True):
            ps.append(int(x)), pd.append(int(y)), valid.append(v)

        for k in (1, 2, 3, 4, 5, 6):  # three pairs at each distance (5 and 6: what k_meet3 hands on with distances 1 .. 3 excluded)
            at = np.flatnonzero(dist == k)
            assert len(at) >= 3, "the graph has pairs at distance %d" % k
            for j in at[rng.integers(0, len(at), 3)]:
                add(a[j], b[j])
        far = np.flatnonzero((dist == -1) & (outdeg[a] > 0) & (indeg[b] > 0))
        assert len(far) >= 2, "component A has unreachable pairs whose endpoints have edges"
        for j in far[:2]:
            add(a[j], b[j])
        add(5, VA + 5), add(VA + 7, 9)  # the other component
        add(3, 4, False), add(3, 3, False), add(V - 1, 0, False)  # NULL sources
        add(17, 17), add(V - 2, V - 2)  # src == dst: with edges, isolated
        add(V - 3, 11), add(11, V - 3), add(V - 4, V - 5)  # isolated endpoints: empty lists
        no_out, no_in = np.flatnonzero(outdeg[:VA] == 0), np.flatnonzero(indeg[:VA] == 0)
        if len(no_out):
            add(no_out[0], 21)  # in-edges only: an empty out-list
        if len(no_in):
            add(21, no_in[0])
        self.ps, self.pd, self.valid = np.array(ps, dtype=np.int64), np.array(pd, dtype=np.int64), np.array(valid)
        ln, ok = self.ora.lean_iterativelength(V, self.ps, self.pd, nthreads=8)
        self.dist = np.where(ok, ln, -1)
        assert set(self.dist[self.valid]) >= {-1, 0, 1, 2, 3, 4, 5, 6}
        self.block = len(self.ps)
        self.paths = self.ora.lean_shortestpath(V, self.ps, self.pd)
        self.torch = torch

    def pick(self, n, rot):
        return (rot + np.arange(n)) % self.block

    def want(self, idx, bound=None):
        if bound is None:
            return np.where(self.valid[idx], self.dist[idx], -1).astype(np.int64)
        return clamp(self.dist[idx], self.valid[idx], bound)

    def bulk(self, idx, bound=None):
        """One call through the device-pointer form over a pre-filled result buffer; NULL sources are src < 0."""
        torch = self.torch
        t_s = torch.from_numpy(np.where(self.valid[idx], self.ps[idx], -1)).cuda()
        t_d = torch.from_numpy(self.pd[idx]).cuda()
        t_o = torch.full((len(idx),), SENTINEL, dtype=torch.int64, device="cuda")
        if bound is None:
            self.dev.iterativelength_bulk_ptr(len(idx), t_s.data_ptr(), t_d.data_ptr(), t_o.data_ptr())
        else:
            self.dev.iterativelength_within_bulk_ptr(len(idx), t_s.data_ptr(), t_d.data_ptr(), bound, t_o.data_ptr())
        return t_o.cpu().numpy()

    def check(self, idx, R, T, bound=None, what=""):
        """The call under R = 1 and, twice, under R: no sentinel left, the oracle's answers, the same bytes."""
        pgq.set_option("meet_tail_rows", T)
        pgq.set_option("meet_rows_per_wave", 1)
        one = self.bulk(idx, bound)
        pgq.set_option("meet_rows_per_wave", R)
        want = self.want(idx, bound)
        for turn in (0, 1):
            got = self.bulk(idx, bound)
            where = "%s R %d, T %d, n %d, call %d" % (what, R, T, len(idx), turn)
            assert (got != SENTINEL).all(), "%s: row %d was not written" % (where, np.flatnonzero(got == SENTINEL)[0])
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, "%s: %d rows differ, first: row %d (src %d, dst %d) got %d, expected %d" % (
                where, len(bad), bad[0], self.ps[idx][bad[0]], self.pd[idx][bad[0]], got[bad[0]], want[bad[0]])
            assert got.tobytes() == one.tobytes(), where + ": differs from meet_rows_per_wave = 1"


@pytest.fixture(scope="module")
def case():
    return Case()


def default_tail():
    """meet_tail_rows = 0: twice the wavefronts k_meet3 over the packed lists has resident (7 per SIMD, 4 SIMDs per CU)."""
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count * 4 * 7


def sizes(R, T):
    return sorted({n for n in (1, R - 1, R, R + 1, T, T + 1, T + R - 1, T + R, T + R + 1, 257) if n >= 1})


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_every_kind_in_head_and_tail_positions(case, R):
    pgq.reset_stats()
    calls = 0
    for T in (1, 3, 64, 0):
        for n in sizes(R, T if T else default_tail()):
            case.check(case.pick(n, rot=calls * 5), R, T)
            calls += 1
    assert pgq.get_stats()["launches"]["meet"] >= 3 * calls, "every call went through k_meet3"


@pytest.mark.parametrize("bound", [1, 2, 3])
def test_bounded_calls(case, bound):
    for R in (2, 4, 8):
        for T in (1, 64):
            for n in (R + 1, T + R + 1, 257):
                case.check(case.pick(n, rot=n + bound), R, T, bound=bound, what="bound %d," % bound)


def test_paths(case):
    for R in (2, 4, 8):
        pgq.set_option("meet_rows_per_wave", R)
        for T in (1, 64):
            pgq.set_option("meet_tail_rows", T)
            for n in (R + 1, T + R + 1, 257):
                idx = case.pick(n, rot=n)
                want = [case.paths[j] if case.valid[j] else None for j in idx]
                for turn in (0, 1):
                    got = case.st.shortestpath(0, V, case.ps[idx], case.pd[idx], src_valid=case.valid[idx])
                    assert got == want, "shortestpath, R %d, T %d, n %d, call %d" % (R, T, n, turn)


def test_an_id_out_of_range_fails(case):
    torch = case.torch
    idx = case.pick(257, rot=0)
    for R, T, at in ((4, 64, 2), (4, 64, 250), (8, 1, 7)):  # in a head group's lane, in the tail, in a group's last lane
        pgq.set_option("meet_rows_per_wave", R)
        pgq.set_option("meet_tail_rows", T)
        for which in (0, 1):
            ps, pd = np.where(case.valid[idx], case.ps[idx], -1), case.pd[idx].copy()
            (ps, pd)[which][at] = V
            t_s, t_d = torch.from_numpy(ps).cuda(), torch.from_numpy(pd).cuda()
            t_o = torch.full((len(idx),), SENTINEL, dtype=torch.int64, device="cuda")
            with pytest.raises(pgq.PgqError, match="error -4.*out of range"):
                case.dev.iterativelength_bulk_ptr(len(idx), t_s.data_ptr(), t_d.data_ptr(), t_o.data_ptr())
    case.check(idx, 4, 64, what="after the failed calls,")


def test_more_groups_than_the_grid_holds(case):
    # meet_grid_mult = 1: the grid is the 8192 workgroups of one round; 70,001 rows under R = 4 are over 17,000 groups, so every
    # workgroup takes further groups at the grid's stride, head groups and single rows
    pgq.set_option("meet_grid_mult", 1)
    idx = case.pick(70_001, rot=3)
    case.check(idx, 4, 3000)
    case.check(idx, 8, 0)


def test_the_options_take_their_values_only():
    for bad in (0, 3, 5, 16, -1):
        with pytest.raises(pgq.PgqError):
            pgq.set_option("meet_rows_per_wave", bad)
    with pytest.raises(pgq.PgqError):
        pgq.set_option("meet_tail_rows", -1)
    assert pgq.get_default_option("meet_tail_rows") == 0
