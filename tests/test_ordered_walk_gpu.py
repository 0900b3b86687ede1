"""The degree-ordered packed lists (option meet_pack_order) and the two-part walk of k_meet3 / k_meet3w over them.

Directed gadget graphs of at most 4096 vertices, every expected value the CPU oracle's, every comparison exact, and the same
answers with meet_pack_order 1 and 0.  A gadget is  s -> mids -> entries,  witness -> d : the forward two-hop walk of s meets the
only witness (the one entry that is an in-neighbour of d) at a chosen place of a chosen mid's list.  Every d also has two
in-neighbours of in-degree 3000 that nothing reachable from a source points at: its backward walk is the longer one, so k_meet3
— and k_meet4d after it, which chooses again — walk forward from s.  The transposed graph walks the reverse lists the same way.

  tail1 / tail2   one witness of in-degree 1 among 49 decoys of high in-degree in a 50-entry list: in the list's tail under the
                  degree order (and, having the smallest id, in its head under the id order); 5 mids (one round) / 70 mids (two
                  rounds, the witness's mid once in each)
  head            the witness has the highest in-degree and the largest id of a 50-entry list: in the head under the degree
                  order only
  short           70 lists of 1 .. K entries: no list of either round has a tail
  g4 / g5         lists of exactly 4 and 5 groups, the witness the last entry of each kind
  cut0 / cut1     192 mids (three rounds) of 30 entries: 2 groups of head, 3 of tail.  cut0: the witness in the FIRST mid's tail,
                  meet_cap 1000 cuts the walk among the heads of round 1.  cut1: the witness in the LAST mid's tail, meet_cap
                  2904 lets every head through (2304 entries) and cuts the tails in their first pass.  Both rows are k_meet4d's
  far4            tail1 with one more hop: distance 4 (NULL under a bound of 3, which k_meet3 may only say after both parts)

Every call must be answered by the pre-pass alone (meet_pairs == rows): a row that fell through to the lane batches would hide
a wrong walk behind a right answer."""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from helpers import csr_arrays_from_rows
from oracle.pgq_oracle import OracleCSR

pytestmark = pytest.mark.gpu

K = 6  # ids per packed group for V <= 2^21
KEYS = ("meet", "meet_bias", "meet_cap", "meet_cap_small", "meet4", "meet4_cap", "meet_layout", "meet_align", "meet_pack",
        "meet_pack_align", "meet_pack_order", "meet_small_rows", "meet_wide_rows", "meet_wide_rows_always", "bibfs_rows", "ball",
        "route_timing", "route_memo", "calibration_cache", "meet_calibrate")


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k in KEYS:
        pgq.set_option(k, pgq.get_default_option(k))
    for k, v in (("meet", 1), ("meet_bias", 1e9), ("ball", 0)):  # the pre-pass, whatever the call's size
        pgq.set_option(k, v)
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


class Builder:
    def __init__(self):
        self.n = 0
        self.src, self.dst = [], []
        self.rows = {}

    def new(self, k=1):
        self.n += k
        return list(range(self.n - k, self.n))

    def edge(self, a, b):
        self.src.append(a)
        self.dst.append(b)


def build_gadgets():
    b = Builder()
    feeders = b.new(3000)
    heavy = b.new(2)  # in-neighbours of every destination with long in-lists: the backward walk is the longer one
    for x in heavy:
        for f in feeders:
            b.edge(f, x)
    def gadget(name, lists, witness_at, hops=3):
        """lists: per mid the list of entries, None = a new vertex of in-degree 1; witness_at = (mid, position)."""
        s = b.new()[0]
        mids = b.new(len(lists))
        wit = None
        for j, (m, lst) in enumerate(zip(mids, lists)):
            b.edge(s, m)
            for p, x in enumerate(lst):
                if x is None:
                    x = b.new()[0]
                b.edge(m, x)
                if (j, p) == witness_at:
                    wit = x
        last = wit
        for _ in range(hops - 3):
            nxt = b.new()[0]
            b.edge(last, nxt)
            last = nxt
        d = b.new()[0]
        b.edge(last, d)
        for x in heavy:
            b.edge(x, d)
        b.rows[name] = (s, d)
        return wit

    # the witnesses first: the smallest ids of their lists (the head of the id order)
    low = {name: None for name in ("tail1", "tail2a", "tail2b", "far4")}
    for name in low:
        low[name] = b.new()[0]
    pool = b.new(49)  # decoys: in-degree in the hundreds
    for x in pool:
        for f in feeders[:100]:
            b.edge(f, x)
    fill = lambda n: pool[:n]
    gadget("tail1", [[low["tail1"]] + fill(49)] + [fill(7)] * 4, (0, 0))
    gadget("tail2a", [[low["tail2a"]] + fill(49)] + [fill(7)] * 69, (0, 0))   # the witness's list in round 0
    gadget("tail2b", [fill(7)] * 69 + [[low["tail2b"]] + fill(49)], (69, 0))  # ... in round 1
    gadget("far4", [[low["far4"]] + fill(49)] + [fill(7)] * 4, (0, 0), hops=4)
    # head: 49 entries of in-degree 1 and, with the largest id, the witness of in-degree 41
    hw = gadget("head", [[None] * 50] + [fill(7)] * 4, (0, 49))
    for f in feeders[:40]:
        b.edge(f, hw)
    gadget("short", [fill(1 + j % K) for j in range(69)] + [fill(K - 1) + [None]], (69, K - 1))
    gadget("g4", [fill(4 * K - 1) + [None]] + [fill(4 * K)] * 3, (0, 4 * K - 1))
    gadget("g5", [fill(5 * K)] * 3 + [fill(5 * K - 1) + [None]], (3, 5 * K - 1))
    gadget("cut0", [fill(29) + [None]] + [fill(30)] * 191, (0, 29))
    gadget("cut1", [fill(30)] * 191 + [fill(29) + [None]], (191, 29))
    return b


class Graph:
    def __init__(self, V, src, dst, rows):
        order = np.lexsort((dst, src))  # lists in id order
        self.V, self.src, self.dst, self.rows = V, src[order], dst[order], rows
        self.ora = OracleCSR.from_edges(V, self.src, self.dst)

    def pairs(self, names):
        rs = np.array([self.rows[n][0] for n in names], dtype=np.int64)
        rd = np.array([self.rows[n][1] for n in names], dtype=np.int64)
        ln, ok = self.ora.lean_iterativelength(self.V, rs, rd, nthreads=4)
        return rs, rd, np.where(ok, ln, -1)


@pytest.fixture(scope="module")
def graphs():
    b = build_gadgets()
    assert b.n <= 4096, b.n
    src, dst = np.array(b.src, dtype=np.int64), np.array(b.dst, dtype=np.int64)
    g = Graph(b.n, src, dst, b.rows)
    t = Graph(b.n, dst, src, {n: (d, s) for n, (s, d) in b.rows.items()})
    # the gadgets are what they are meant to be
    names = sorted(b.rows)
    for gr in (g, t):
        _, _, dist = gr.pairs(names)
        assert {n: int(x) for n, x in zip(names, dist)} == {n: (4 if n == "far4" else 3) for n in names}
    off, adj, _ = csr_arrays_from_rows(g.V, g.src, g.dst)
    roff, radj, _ = csr_arrays_from_rows(g.V, g.dst, g.src)
    ind, outd = np.diff(roff), np.diff(off)
    for n, (s, d) in b.rows.items():  # the forward walk from s is the shorter one, and the other list fits the register set
        assert outd[adj[off[s]:off[s + 1]]].sum() <= ind[radj[roff[d]:roff[d + 1]]].sum() and ind[d] == 3, n
    s = b.rows["tail1"][0]
    lst = adj[off[adj[off[s]]]:off[adj[off[s]] + 1]]
    assert len(lst) == 50 and ind[lst[0]] == 1 and ind[lst[1:]].min() >= 64  # the witness: lowest id, lowest in-degree
    return g, t


def upload(gr):
    st = pgq.PgqState()
    st.build_csr(0, gr.V, gr.src, gr.dst)
    return st


def check(gr, st, names, what, bound=None):
    rs, rd, dist = gr.pairs(names)
    pgq.reset_stats()
    if bound is None:
        ln, ok = st.iterativelength(0, gr.V, rs, rd)
        want = dist
    else:
        ln, ok = st.iterativelength_within(0, gr.V, rs, rd, bound)
        want = np.where((dist >= 0) & (dist <= bound), dist, -1)
    got = np.where(ok, ln, -1)
    print("%s: got %s, expected %s" % (what, got.tolist(), want.tolist()))
    assert got.tolist() == want.tolist(), what
    assert pgq.get_stats()["meet_pairs"] == len(names), what
    return got


# the three first-stage kernels: k_meet3 with 4 requests in flight (a call this small), with 2 (every call "large"), k_meet3w
MODES = {"small": {}, "large": {"meet_small_rows": 0}, "wide": {"meet_wide_rows_always": 1}}
PLAIN = ["tail1", "tail2a", "tail2b", "head", "short", "g4", "g5", "far4"]


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("side", [0, 1], ids=["graph", "transpose"])
def test_witness_in_head_or_tail(graphs, side, order):
    gr = graphs[side]
    pgq.set_option("meet_pack_order", order)  # read at upload
    st = upload(gr)
    assert st.device_csr(0).pack_k == K and st.device_csr(0).pack_order == order
    for mode, opts in MODES.items():
        for k, v in opts.items():
            pgq.set_option(k, v)
        what = "%s, order %d, %s" % (("graph", "transpose")[side], order, mode)
        check(gr, st, PLAIN, what)
        got = check(gr, st, PLAIN, what + ", within 3", bound=3)
        assert got[PLAIN.index("tail1")] == 3 and got[PLAIN.index("far4")] == -1
        for name in PLAIN:  # one row per call: the row's own walk, nothing beside it
            check(gr, st, [name], what + ", " + name)
        for k in opts:
            pgq.set_option(k, pgq.get_default_option(k))
    st.delete_csr(0)


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("side", [0, 1], ids=["graph", "transpose"])
def test_small_cap_hands_the_row_to_meet4d(graphs, side, order):
    gr = graphs[side]
    pgq.set_option("meet_pack_order", order)
    st = upload(gr)
    # cut0: 1000 < the 1536 entries requested once round 1's heads are in flight; cut1: the heads are 192 x 12 = 2304 entries,
    # 600 more end the tails' first pass (two requests of 64 groups = 768 entries)
    for name, cap in (("cut0", 1000), ("cut1", 2304 + 600)):
        for mode, opts in MODES.items():
            for k, v in dict(opts, meet_cap=cap, meet_cap_small=cap).items():
                pgq.set_option(k, v)
            what = "%s, order %d, %s, %s under meet_cap %d" % (("graph", "transpose")[side], order, mode, name, cap)
            check(gr, st, [name], what)
            check(gr, st, [name], what + ", within 3", bound=3)
            # k_meet3 WAS cut: without the bit-map kernels the pre-pass leaves the row open.  (Not asked of the id order, which
            # meets cut0's witness in its first request, nor of k_meet3w: its wavefronts stop one by one, and the one that has no
            # head request starts on the tails with its whole share of the cap and may find what the others were cut short of)
            if order and mode != "wide":
                pgq.set_option("meet4", 0)
                rs, rd, dist = gr.pairs([name])
                pgq.reset_stats()
                ln, ok = st.iterativelength(0, gr.V, rs, rd)
                assert np.where(ok, ln, -1).tolist() == dist.tolist() and pgq.get_stats()["meet_pairs"] == 0, what
            for k in list(opts) + ["meet_cap", "meet_cap_small", "meet4"]:
                pgq.set_option(k, pgq.get_default_option(k))
        # under the shipped cap k_meet3 keeps the row
        pgq.set_option("meet4", 0)
        check(gr, st, [name], "%s, shipped cap, no meet4" % name)
        pgq.set_option("meet4", pgq.get_default_option("meet4"))
    st.delete_csr(0)


def test_five_ids_per_group(graphs):
    g = graphs[0]
    V = (1 << 21) + 64
    shift = V - g.V  # the gadgets at the top of the id range; nothing else has an edge
    pgq.set_option("meet_pack", 2)
    st = pgq.PgqState()
    st.build_csr(0, V, g.src + shift, g.dst + shift)
    assert st.device_csr(0).pack_k == 5 and st.device_csr(0).pack_order == 1
    names = ["tail1", "tail2a", "tail2b", "head", "far4"]
    rs, rd, dist = g.pairs(names)
    for mode, opts in MODES.items():
        for k, v in opts.items():
            pgq.set_option(k, v)
        pgq.reset_stats()
        ln, ok = st.iterativelength(0, V, rs + shift, rd + shift)
        assert np.where(ok, ln, -1).tolist() == dist.tolist(), mode  # distances do not move with the ids
        assert pgq.get_stats()["meet_pairs"] == len(names), mode
        for k in opts:
            pgq.set_option(k, pgq.get_default_option(k))
    st.delete_csr(0)


def test_packed_lists_read_back_in_degree_order():
    rng = np.random.default_rng(11)
    V, E = 2000, 30000
    w = 1.0 / np.arange(1, V + 1) ** 0.8  # skewed degrees in both directions: many buckets per list
    src = rng.choice(V, E, p=w / w.sum())
    dst = rng.permutation(V)[rng.choice(V, E, p=w / w.sum())]
    order = np.lexsort((dst, src))
    src, dst = src[order].astype(np.int64), dst[order].astype(np.int64)
    off, adj, _ = csr_arrays_from_rows(V, src, dst)
    rorder = np.lexsort((src, dst))
    roff, radj, _ = csr_arrays_from_rows(V, dst[rorder], src[rorder])
    bucket = lambda deg: np.floor(np.log2(np.maximum(deg, 1))).astype(np.int64)
    for order_opt in (1, 0):
        pgq.set_option("meet_pack_order", order_opt)
        st = pgq.PgqState()
        st.build_csr(0, V, src, dst)
        csr = st.device_csr(0)
        assert csr.pack_k == K and csr.pack_order == order_opt
        seen = 0
        for direction, o, a, other in ((0, off, adj, np.diff(roff)), (1, roff, radj, np.diff(off))):
            for v in range(V):
                want = a[o[v]:o[v + 1]]
                got = csr.packed_list(direction, v).astype(np.int64)
                if order_opt:
                    # non-increasing bucket of the OTHER direction's degree, ties in the CSR's (id) order: the stable sort itself
                    want = want[np.argsort(-bucket(other[want]), kind="stable")]
                    seen = max(seen, len(set(bucket(other[want]).tolist())))
                assert got.tolist() == want.tolist(), (order_opt, direction, v)
        assert not order_opt or seen >= 4  # lists with several buckets were among them
        st.delete_csr(0)
