"""walk_length on the GPU, in every entry form (bulk, chunk, UDF) and under every direction (walk_length_pull = 0 push, 1 pull,
2 automatic, set per handle), against the Python model of its contract and of its two stages (walk_length_model.py — checked on the
CPU against a brute-force enumeration of walks and walk_count's tables; the fixtures used here catch its mutants there).  Every
comparison is exact: the answers, and the statistics that say which rounds ran (batches, levels, push_levels, pull_levels, and the
adjacency entries walked wherever the model knows them exactly)."""
import numpy as np
import pytest

import all_shortest_model as A
import duckpgq_extension_amd as pgq
import k_walks_model as KW
import walk_length_model as W
from duckpgq_extension_amd.binding import PgqError

pytestmark = pytest.mark.gpu

FIXTURES = W.gpu_fixtures()
MODES = {"push": 0, "pull": 1, "auto": 2}
UPLOAD_KEYS = ("part_weight", "hub_chunk")
_cases, _want = {}, {}


class Case:
    """A fixture's graph uploaded under a layout: one CSR behind the UDF state, its device handle for the bulk and chunk forms."""

    def __init__(self, name, layout):
        self.fx = FIXTURES[name][0]
        V, off, adj, eid = self.fx[:4]
        self.layout, self.graph = layout, W.Graph(V, off, adj)
        saved = {k: pgq.get_option(k) for k in UPLOAD_KEYS}
        for k, v in zip(UPLOAD_KEYS, layout):  # read at upload, from the process-wide options
            pgq.set_option(k, v)
        self.st = pgq.PgqState()
        self.st.build_csr(0, V, A.slot_sources(V, off), adj, eid)
        self.dev = self.st.device_csr(0)  # the upload itself
        for k, v in saved.items():
            pgq.set_option(k, v)
        self.hubless = not self.graph.parts(layout)[1]


def case_of(name, layout=W.DEFAULT_LAYOUT):
    if (name, layout) not in _cases:
        _cases[name, layout] = Case(name, layout)
    return _cases[name, layout]


def want_of(name, layout, lo, hi, direction):
    """(answers, stats) of the model for the fixture's own rows, computed once and left unchanged."""
    key = (name, layout, lo, hi, direction)
    if key not in _want:
        c = case_of(name, layout)
        _want[key] = W.solve(*c.fx[:3], c.fx[4], c.fx[5], lo, hi, direction, layout, graph=c.graph)
    return _want[key]


def bulk(dev, rs, rd, lo, hi):
    import torch
    n = len(rs)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(rs)).cuda(), torch.from_numpy(np.ascontiguousarray(rd)).cuda()
    t_o = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    dev.walk_length_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, hi, t_o.data_ptr())
    return t_o.cpu().numpy()[:n].tolist()


def payload(out, ok):
    assert (out[~ok] == -1).all(), "a NULL row's payload is -1"
    return np.where(ok, out, -1).tolist()


def same(got, want, rs, rd, what):
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, "%s: %d of %d rows differ, first: %d -> %d got %r, expected %r" % (
        what, len(bad), len(want), rs[bad[0]], rd[bad[0]], got[bad[0]], want[bad[0]])


def check(name, layout=W.DEFAULT_LAYOUT, bounds=None):
    """The fixture's rows under every bound and direction: the bulk form with its statistics, the chunk and the UDF form."""
    c = case_of(name, layout)
    V, off, adj, eid, rs, rd = c.fx
    for lo, hi in bounds or FIXTURES[name][1]:
        answers = set()
        for direction, mode in MODES.items():
            want, stats = want_of(name, layout, lo, hi, direction)
            what = "%s, layout %r, {%d,%d}, %s" % (name, layout, lo, hi, direction)
            c.dev.set_option("walk_length_pull", mode)
            pgq.binding.reset_stats()
            same(bulk(c.dev, rs, rd, lo, hi), want, rs, rd, what + ", bulk form")
            got = pgq.get_stats()
            seen = {k: got[k] for k in ("batches", "levels", "push_levels", "pull_levels")}
            assert seen == {k: stats[k] for k in seen}, (what, seen, stats)
            if direction == "push" or c.hubless:
                assert got["edges_scanned"] == stats["edges"], (what, got["edges_scanned"], stats["edges"])
            if direction != "auto":  # the direction that was forced is the one that ran
                assert got["pull_levels" if direction == "push" else "push_levels"] == 0
            same(payload(*c.dev.walk_length(rs, rd, lo, hi)), want, rs, rd, what + ", chunk form")
            same(payload(*c.st.walk_length(0, V, rs, rd, lo, hi)), want, rs, rd, what + ", udf form")
            answers.add(tuple(want))
        assert len(answers) == 1  # the directions agree
    c.dev.set_option("walk_length_pull", 2)


# ---- 1. small graphs and bounds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring5", "self_loop", "pair", "chain3", "two_loops", "loops_and_fan", "wide_exit"])
def test_small_graphs(name):
    check(name)


def test_small_graphs_say_what_the_contract_says():
    ring = lambda lo, hi: want_of("ring5", W.DEFAULT_LAYOUT, lo, hi, "push")[0][0]  # noqa: E731  (the row (0, 0))
    assert [ring(1, 4), ring(1, 5), ring(6, 10), ring(0, 3)] == [-1, 5, 10, 0]
    assert want_of("self_loop", W.DEFAULT_LAYOUT, 1, 1, "push")[0][0] == 1
    assert want_of("pair", W.DEFAULT_LAYOUT, 2, 2, "push")[0][0] == -1 and want_of("pair", W.DEFAULT_LAYOUT, 2, 3, "push")[0][0] == 3
    for direction in MODES:  # a directed chain at distance 2 under {3,5}: the rounds end when nothing is active
        want, stats = want_of("chain3", W.DEFAULT_LAYOUT, 3, 5, direction)
        assert want == [-1] and stats["levels"] == 3


# ---- 2. list lengths and hubs: the only live parent in the last slot, on a row whose distance is below lower ------------------------
@pytest.mark.parametrize("layout", [W.DEFAULT_LAYOUT, W.SMALL_LAYOUT], ids=["default", "small"])
@pytest.mark.parametrize("deg", W.LIST_DEGREES)
def test_list_lengths_and_hubs(deg, layout):
    name = "last_slot_%d" % deg
    check(name, layout)
    c = case_of(name, layout)
    assert want_of(name, layout, 2, 3, "pull")[0][0] == 3 and want_of(name, layout, 2, 2, "pull")[0][0] == -1
    got = c.dev.pull_layout()  # the partition the model walks is the one the upload built
    parts, hubs, slices = c.graph.parts(layout)
    assert got["parts"].tolist() == [list(p) for p in parts] and got["hub_vertices"].tolist() == hubs
    assert got["hub_items"].tolist() == [list(s) for s in slices]
    x = int(c.fx[5][0])
    assert (x in hubs) == (layout == W.SMALL_LAYOUT and deg > 64)  # 63, 64: at and below the threshold; 65: above; 129: past a slice boundary


# ---- 3. batches: 1 .. 129 distinct sources among the rows left ------------------------------------------------------------------------
@pytest.mark.parametrize("n", W.SOURCE_COUNTS)
def test_batch_boundaries(n):
    check("sources_%d" % n)
    assert want_of("sources_%d" % n, W.DEFAULT_LAYOUT, 1, 3, "pull")[1]["batches"] == -(-n // 64)
    check("pair")  # a smaller graph on the same thread afterwards


# ---- 4. random rows: NULL rows, selection vectors, closed rows; the device's own k_shortest_walks(k = 1) and walk_count ----------------
def k1_hops(dev, rs, rd, lo, hi):
    import torch
    n = len(rs)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(rs)).cuda(), torch.from_numpy(np.ascontiguousarray(rd)).cuda()
    row = [torch.full((n,), -7, dtype=torch.int64, device="cuda") for _ in range(4)]
    cap = n * (2 * hi + 1)
    t_po, t_ph = (torch.zeros((n,), dtype=torch.int64, device="cuda") for _ in range(2))
    t_ch = torch.zeros((cap,), dtype=torch.int64, device="cuda")
    rc, _, _ = dev.k_shortest_walks_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, hi, 1, row[0].data_ptr(), row[1].data_ptr(), row[2].data_ptr(),
                                             row[3].data_ptr(), t_po.data_ptr(), t_ph.data_ptr(), n, t_ch.data_ptr(), cap)
    assert rc == 0
    t_c = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    dev.walk_count_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, hi, t_c.data_ptr())
    return row[0].cpu().numpy().tolist(), t_c.cpu().numpy().tolist()


@pytest.mark.parametrize("layout", [W.DEFAULT_LAYOUT, W.SMALL_LAYOUT], ids=["default", "small"])
@pytest.mark.parametrize("lo,hi", W.RANDOM_BOUNDS)
def test_random_rows(lo, hi, layout):
    c = case_of("random", layout)
    V, off, adj, eid, rs, rd = c.fx
    check("random", layout, ((lo, hi),))
    want = want_of("random", layout, lo, hi, "push")[0]
    if layout == W.DEFAULT_LAYOUT:  # the three identities, on the device itself
        hops, counts = k1_hops(c.dev, rs, rd, lo, hi)
        assert want == hops and [w >= 0 for w in want] == [x > 0 for x in counts]
        within = payload(*c.dev.iterativelength_within(rs, rd, hi))
        assert all(w == d for w, d in zip(want, within) if lo <= d) and (lo > 0 or want == within)
        assert sum(1 for w, d in zip(want, within) if w != d) >= (50 if lo else 0)  # where the reference's filter is wrong
    # NULL rows and selection vectors
    brs = rs.copy()
    brs[4::9] = -1
    nulls = W.solve(V, off, adj, brs, rd, lo, hi, graph=c.graph)[0]
    assert -1 in nulls[4::9] and set(nulls[4::9]) == {-1}
    sv, dv = np.ones(len(rs), dtype=bool), np.ones(len(rs), dtype=bool)
    sv[3::7] = False
    dv[5::7] = False
    masked = [-1 if not (a and b) else w for a, b, w in zip(sv, dv, want)]
    sel = np.array([7, 7, 0, len(rs) - 1, 12, 3, 12, 10, 20], dtype=np.uint32)
    for mode in MODES.values():
        c.dev.set_option("walk_length_pull", mode)
        assert bulk(c.dev, brs, rd, lo, hi) == nulls
        for obj, args in ((c.dev, ()), (c.st, (0, V))):
            out, ok = obj.walk_length(*args, rs, rd, lo, hi, src_valid=sv, dst_valid=dv)
            assert (ok == ((sv & dv) & (np.array(want) >= 0))).all() and payload(out, ok) == masked
            assert payload(*obj.walk_length(*args, rs, rd, lo, hi, src_sel=sel, dst_sel=sel)) == [want[i] for i in sel]
    c.dev.set_option("walk_length_pull", 2)


# ---- 5. stage 1 is really used ---------------------------------------------------------------------------------------------------------
def test_rows_that_stage_1_settles_start_no_batch():
    c = case_of("random")
    V, off, adj, eid, rs, rd = c.fx
    dist = np.array([c.graph.dist(s).get(d, -1) for s, d in zip(rs.tolist(), rd.tolist())])
    settled = (dist < 0) | (dist >= 2)  # under {2,3}: lower <= d, d > upper or unreachable
    assert settled.sum() > 1000 and (~settled).sum() > 100 and (dist[settled] > 3).sum() > 100
    for mode in MODES.values():
        c.dev.set_option("walk_length_pull", mode)
        pgq.binding.reset_stats()
        want = [int(d) if 2 <= d <= 3 else -1 for d in dist[settled]]
        assert bulk(c.dev, rs[settled], rd[settled], 2, 3) == want
        st = pgq.get_stats()
        assert st["batches"] == 0 and st["levels"] == 0 and st["edges_scanned"] == 0
        pgq.binding.reset_stats()  # lower == 0: the call ends behind stage 1 whatever the rows
        assert bulk(c.dev, rs, rd, 0, 3) == want_of("random", W.DEFAULT_LAYOUT, 0, 3, "push")[0]
        st = pgq.get_stats()
        assert st["batches"] == 0 and st["levels"] == 0
        pgq.binding.reset_stats()  # a mixed call starts batches for the sources of the rows left alone
        want, stats = want_of("random", W.DEFAULT_LAYOUT, 2, 4, "push")
        assert bulk(c.dev, rs, rd, 2, 4) == want
        st = pgq.get_stats()
        rest = (dist >= 0) & (dist < 2)
        left = {int(s) for s, d in zip(rs[rest], rd[rest]) if c.graph.out[s] and c.graph.roff[d + 1] > c.graph.roff[d]}
        assert st["batches"] == stats["batches"] == -(-len(left) // 64) < -(-len(set(rs.tolist())) // 64)
    c.dev.set_option("walk_length_pull", 2)


def test_forced_directions_show_in_the_statistics():
    c = case_of("random")
    V, off, adj, eid, rs, rd = c.fx
    for direction, mine, other in (("push", "push_levels", "pull_levels"), ("pull", "pull_levels", "push_levels")):
        c.dev.set_option("walk_length_pull", MODES[direction])
        pgq.binding.reset_stats()
        c.dev.walk_length(rs, rd, 2, 4)
        st = pgq.get_stats()
        assert st[mine] == st["levels"] == want_of("random", W.DEFAULT_LAYOUT, 2, 4, direction)[1]["levels"] > 0 and st[other] == 0
    c.dev.set_option("walk_length_pull", 2)
    assert pgq.get_default_option("walk_length_pull") == 2 and pgq.get_option("walk_length_pull") == 2  # the handle's option, not the process's


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------
def test_error_codes_and_no_rows():
    import torch
    c = case_of("ring5")
    V, off, adj, eid, rs, rd = c.fx
    L = pgq.load_hip()
    err = lambda: L.pgq_last_error().decode()  # noqa: E731
    t_s, t_d = torch.from_numpy(rs).cuda(), torch.from_numpy(rd).cuda()
    t_o = torch.full((len(rs),), -7, dtype=torch.int64, device="cuda")

    def raw(lo, hi, src=t_s):
        return L.pgq_walk_length_bulk_device(c.dev.h, len(rs), src.data_ptr(), t_d.data_ptr(), lo, hi, t_o.data_ptr())

    for lo, hi in ((-1, 3), (3, 2)):  # PGQ_ERR_INVALID_ARG
        assert raw(lo, hi) == -4
        with pytest.raises(PgqError):
            c.dev.walk_length(rs, rd, lo, hi)
        with pytest.raises(PgqError):
            c.st.walk_length(0, V, rs, rd, lo, hi)
    for hi in (W.MAX_HOPS + 1, KW.INT64_MAX):  # PGQ_ERR_UNSUPPORTED, with walk_check's text
        assert raw(0, hi) == -6 and "upper bound" in err()
        with pytest.raises(PgqError, match="upper bound"):
            c.dev.walk_length(rs, rd, 0, hi)
        with pytest.raises(PgqError, match="upper bound"):
            c.st.walk_length(0, V, rs, rd, 1, hi)
    bad = torch.from_numpy(np.array([0, V, 0, 0, 0], dtype=np.int64)).cuda()
    assert raw(1, 3, bad) == -4 and "out of range" in err()
    for bad_call in (lambda: c.dev.walk_length([0, V], [1, 1], 1, 3), lambda: c.dev.walk_length([0], [V], 1, 3), lambda: c.dev.walk_length([0], [-2], 0, 3)):
        with pytest.raises(PgqError):
            bad_call()
    assert L.pgq_walk_length_bulk_device(c.dev.h, 1, None, t_d.data_ptr(), 1, 3, t_o.data_ptr()) == -4 and "NULL device array" in err()
    assert (t_o.cpu().numpy() == -7).all()  # a failed call has written nothing
    assert L.pgq_walk_length_bulk_device(c.dev.h, 0, None, None, 1, 3, None) == 0  # n == 0
    for obj, args in ((c.dev, ()), (c.st, (0, V))):
        out, ok = obj.walk_length(*args, [], [], 1, 3)
        assert len(out) == 0 and len(ok) == 0
    assert raw(W.MAX_HOPS, W.MAX_HOPS) == 0 and t_o.cpu().numpy().tolist() == W.solve(V, off, adj, rs, rd, W.MAX_HOPS, W.MAX_HOPS)[0]


# ---- 7. the neighbours on the shared workspace -------------------------------------------------------------------------------------------
def test_neighbours_unchanged_and_nothing_left_behind():
    V, off, adj, eid, rs, rd = FIXTURES["random"][0]
    rs, rd = rs[:400], rd[:400]
    before_handle = pgq.live_device_blocks()
    dev = pgq.DeviceCSR(V, off, adj, eid)

    def neighbours():
        count, cok = dev.walk_count(rs, rd, 1, 3)
        within, wok = dev.iterativelength_within(rs, rd, 3)
        return (count.tolist(), cok.tolist(), dev.k_shortest_walks(rs, rd, 1, 3, 2), within.tolist(), wok.tolist(), dev.shortestpath(rs, rd))

    first = neighbours()
    want = W.solve(V, off, adj, rs, rd, 2, 4)[0]
    for mode in (2, 0, 1):
        dev.set_option("walk_length_pull", mode)
        assert payload(*dev.walk_length(rs, rd, 2, 4)) == want
        assert neighbours() == first
        with pytest.raises(PgqError):  # a call that failed
            dev.walk_length(rs, rd, 2, W.MAX_HOPS + 1)
        with pytest.raises(PgqError):
            dev.walk_length(np.append(rs, V), np.append(rd, 0), 2, 4)
        assert neighbours() == first
        assert bulk(dev, rs, rd, 2, 4) == want
    dev.close()
    assert pgq.live_device_blocks() == before_handle
