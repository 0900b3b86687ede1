"""tests/layout_model.py held to a plain per-vertex restatement of the same contract, its mutants told apart, and the graphs of
helpers.layout_* shown to be what test_upload_layout_gpu.py takes them for.  No GPU: the device's arrays are compared with this
model in test_upload_layout_gpu.py.

Which family tells which mutant from the contract (TELLS, asserted below, under the shipped options: meet_align 32,
meet_pack 1, meet_pack_align 8, meet_pack_order 1, ball_head_mb 512):

    a  blocks (V = 1 .. 769, as given and transposed)      every mutant but work_wraps and k6_lt
    b  saturation                                          work_wraps (h's sum is 2^32: it wraps to 0), and what any graph
                                                           shows; its lists of one repeated id hide pad_first, align_unfilled,
                                                           rhead_unshifted and rhead_clamp_cnt
    c  second trips, scaled down (vb = 512, eb = 1024)     as a
    d  id width, V = 2^21 (without rhead)                  k6_lt, the only family at the size where `<` and `<=` part
    e  degenerate (V = 0, E = 0, meet_layout = 0)          nothing: there is no layout to get wrong

No mutant is left that cannot differ: k6_lt differs at V = 2^21 alone, so the model is run there once without rhead
(ball_head_mb = 0: the V x 64 words are not needed to see pack_k change)."""
import ctypes as C

import numpy as np
import pytest

import layout_model as lm
from helpers import (LAYOUT_BLOCK_V, LAYOUT_LENGTHS, LAYOUT_LONG, LayoutGraph, layout_blocks, layout_end_bit, layout_id_width,
                     layout_saturation, layout_second_trips)
from test_packed_layout_cpu import shim  # noqa: F401 (the g++ shim of pgq_pack.h, a module fixture)


def both(g):
    return [g, g.transposed()]


@pytest.fixture(scope="module")
def families():
    fam = {
        "a": [x for V in LAYOUT_BLOCK_V for x in both(layout_blocks(V))],
        "b": both(layout_saturation()),
        "c": both(layout_second_trips(vb=512, eb=1024)),
        "d": [layout_id_width(1 << 21)],
        "e": [LayoutGraph("no_vertices", 0, [], []), LayoutGraph("no_edges", 300, [], [])],
    }
    return fam


def options_of(name):
    return dict(ball_head_mb=0) if name == "d" else {}


@pytest.fixture(scope="module")
def models(families):
    return {name: [lm.layout(g.V, *g.csr(), **options_of(name)) for g in gs] for name, gs in families.items()}


# ---- the graphs are what they are taken for ------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [v for v in LAYOUT_BLOCK_V if v >= 255])
def test_blocks_have_their_edges(V):
    for g in both(layout_blocks(V)):
        off, adj = g.csr()
        roff, radj = lm.reverse_csr(V, off, adj)
        own = lm.slot_owners(off)
        assert (own == adj).any(), "a self loop"
        pairs = own * V + adj
        assert len(np.unique(pairs)) < len(pairs), "parallel edges"
        for o in (off, roff):
            ln = np.diff(o)
            v = np.arange(V)
            assert set(LAYOUT_LENGTHS) <= set(ln.tolist()) and (ln == LAYOUT_LONG).sum() == 1
            assert len(set(ln.tolist()) - set(LAYOUT_LENGTHS) - {LAYOUT_LONG}) <= 1  # the slack vertex
            assert (ln[(v % 256 == 0) | (v % 256 == 255) | (v == V - 1)] == 0).all()  # block edges; no in-edges at 0 and V - 1
            if V == 769:
                assert (ln[256:512] == 0).all() and ln[:256].sum() > 5000 and ln[512:].sum() > 5000
            # k_two_hop_work's trips of 64 lanes count from the block's first slot (block 0: slot 0)
            assert (o[1] % 64, o[2] % 64) == (0, 0), "vertex 1: lane 0 to lane 63"
            assert o[2] % 64 == 0 and o[3] % 64 == 63, "vertex 2 starts on lane 0; vertex 3 starts on lane 63 ..."
            assert o[4] % 64 == 0 and o[4] // 64 - o[3] // 64 == 3, "... and ends on lane 63 two trips on: three trips"
            assert (ln > 512).any()  # longer than two trips of 256 threads


def test_saturation_sums():
    g = layout_saturation()
    assert len(g.src) == 4 * 65536 - 1
    off, adj = g.csr()
    m = lm.layout(g.V, off, adj)
    assert int(m["dirs"][0]["work"][g.h]) == (1 << 32) - 1 and int(m["dirs"][0]["work"][g.h2]) == (1 << 32) - 65536
    ln = np.diff(off)
    assert int(ln[adj[off[g.h]:off[g.h + 1]]].sum()) == 1 << 32  # the sum itself is one past the word


def test_second_trips_tail():
    from helpers import LAYOUT_TRIPS as T
    for vb, eb in ((512, 1024), (T["slot_sources_v"], T["slots_e"])):
        g = layout_second_trips(vb=vb, eb=eb)
        assert g.V == vb + 257 and len(g.src) == eb + 300
        assert (g.src[eb:] >= vb).all() and (g.src[:eb] < vb).all() and (g.dst[eb:] >= vb).all()  # the tail: last vertices, last slots
        assert g.dst[-1] == g.V - 1 and g.src[-1] == g.V - 1
        off, adj = g.csr()
        roff, _ = lm.reverse_csr(g.V, off, adj)
        assert np.argmax(np.diff(off)) >= vb and np.argmax(np.diff(roff)) >= vb  # the maxima come from the second trip
        assert T["degree_stats_v"] < T["slot_sources_v"]


def test_id_width_positions():
    for V, K in (((1 << 21), 6), ((1 << 21) + 1, 5)):
        g = layout_id_width(V)
        off, adj = g.csr()
        m = lm.layout(V, off, adj, meet_pack=2, meet_pack_order=0, meet_pack_align=1, ball_head_mb=0)
        assert m["pack_k"] == K
        W = 128 // K
        f = m["dirs"][0]
        words = f["packed"].astype(object)
        big = (words[:, 0] | words[:, 1] << 32 | words[:, 2] << 64 | words[:, 3] << 96)
        seen = {k for x in big for k in range(K) if (int(x) >> (k * W)) & ((1 << W) - 1) == V - 1}
        assert seen == set(range(K))
        assert lm.layout(V, off, adj, meet_pack=1, ball_head_mb=0)["pack_k"] == (6 if K == 6 else 4)


# ---- the model against a loop over the vertices -----------------------------------------------------------------------------------
def naive(V, off, adj, ooff, align, K, palign, order):
    """One direction, vertex by vertex and entry by entry."""
    seg, padded, pk, pfirst, g = [], [], [], [], 0
    for v in range(V):
        lst = adj[off[v]:off[v + 1]].tolist()
        n = len(lst)
        ng = -(-n // align) * align // 4
        seg.append((g, n))
        g += ng
        padded += [lst[min(i, n - 1)] for i in range(4 * ng)]
        pfirst.append(len(pk) // K if K > 4 else 0)
        if K > 4 and n:
            if order:
                lst = [x for _, _, x in sorted((-(max(int(ooff[x + 1] - ooff[x]), 1).bit_length() - 1), i, x) for i, x in enumerate(lst))]
            png = -(-n // (K * palign)) * palign
            pk += [lst[min(i, n - 1)] for i in range(K * png)]
    ln = np.diff(off)
    desc = [(u, seg[u][0], seg[u][1], pfirst[u]) for u in adj.tolist()]
    work = [min(int(ln[adj[off[v]:off[v + 1]]].sum()), (1 << 32) - 1) for v in range(V)]
    return seg, padded, desc, work, pk


def naive_rhead(V, roff, radj):
    out = []
    for v in range(V):
        lst = radj[roff[v]:roff[v + 1]].tolist()
        n = len(lst)
        row = [lst[min(e, n - 1)] if n else 0xFFFFFFFF for e in range(63)]
        out.append(row[:31] + [n] + row[31:])
    return out


@pytest.mark.parametrize("V", [1, 2, 257, 769])
@pytest.mark.parametrize("opts", [dict(), dict(meet_align=4, meet_pack_align=1, meet_pack_order=0), dict(meet_align=9, meet_pack=0)])
def test_model_equals_the_loop(V, opts, shim):  # noqa: F811
    for g in both(layout_blocks(V)):
        off, adj = g.csr()
        m = lm.layout(V, off, adj, **opts)
        o = dict(lm.DEFAULTS, **opts)
        K = m["pack_k"]
        assert K == (6 if o["meet_pack"] else 4) and m["has_layout"] == 1 and m["has_rhead"] == 1
        f, r = m["dirs"]
        # the reverse CSR from the definition: in-lists by (source, slot)
        own = lm.slot_owners(off)
        want = sorted(zip(adj.tolist(), own.tolist(), range(len(adj))))
        assert r["adj"].tolist() == [s for _, s, _ in want]
        assert r["off"].tolist() == [0] + np.cumsum(np.bincount(adj, minlength=V)).tolist()
        align = max(4, o["meet_align"]) & ~3
        for d, other in ((f, r), (r, f)):
            seg, padded, desc, work, pk = naive(V, d["off"], d["adj"].astype(np.int64), other["off"], align, K, o["meet_pack_align"],
                                                o["meet_pack_order"])
            assert d["seg"].tolist() == [list(x) for x in seg]
            assert d["padded"].ravel().tolist() == padded
            assert d["desc"].tolist() == [list(x) for x in desc]
            assert d["work"].tolist() == work
            if K > 4:
                ids = np.zeros(K, dtype=np.uint32)
                got = []
                for w in d["packed"]:
                    shim.shim_unpack(K, np.ascontiguousarray(w), ids)
                    got += ids.tolist()
                assert got == pk
            else:
                assert d["packed"] is None
        assert r["rhead"].tolist() == naive_rhead(V, r["off"], r["adj"].astype(np.int64))
        assert m["two_hop_mean"] == float(int((np.diff(off) * np.diff(r["off"])).sum())) / V
        assert (m["max_out_degree"], m["max_in_degree"]) == (int(np.diff(off).max()), int(np.diff(r["off"]).max()))
        assert (m["groups"], m["rgroups"]) == (len(f["padded"]), len(r["padded"]))


def test_degenerate(models):
    for m in models["e"]:
        assert m["has_layout"] == 0 and m["pack_k"] == 4 and m["has_rhead"] == 0
        assert (m["groups"], m["rgroups"], m["pgroups"], m["prgroups"]) == (0, 0, 0, 0)
        assert all(d[k] is None for d in m["dirs"] for k in ("seg", "padded", "desc", "work", "packed", "rhead"))
    g = layout_blocks(257)
    m = lm.layout(g.V, *g.csr(), meet_layout=0)
    assert m["has_layout"] == 0 and m["dirs"][1]["off"][-1] == len(g.src) and m["max_in_degree"] == LAYOUT_LONG
    m = lm.layout(g.V, *g.csr(), ball=0)
    assert m["has_rhead"] == 0 and m["dirs"][1]["rhead"] is None and m["has_layout"] == 1


def test_rhead_exists_while_it_fits():
    g = layout_blocks(256)
    assert lm.layout(256, *g.csr(), ball_head_mb=1)["has_rhead"] == 1  # 256 x 256 B = 64 KB
    g = layout_end_bit(4097)
    assert lm.layout(4097, *g.csr(), ball_head_mb=1)["has_rhead"] == 0  # one vertex past 1 MB
    assert lm.layout(4096, *layout_end_bit(4096).csr(), ball_head_mb=1)["has_rhead"] == 1


# ---- pack_put against the header's ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 6])
def test_pack_put_bits_agree_with_the_header(K, shim):  # noqa: F811
    rng = np.random.default_rng(K)
    W = 128 // K
    ids = rng.integers(0, 1 << W, (400, K)).astype(np.uint32)
    ids[0], ids[1] = (1 << W) - 1, 0
    ids[2:2 + K] = np.eye(K, dtype=np.uint32) * ((1 << W) - 1)  # the top id alone in every position
    words = lm.pack_put(ids, K)
    back = np.zeros(K, dtype=np.uint32)
    gbeg = np.zeros(2, dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    for row, w in zip(ids, words):
        shim.shim_unpack(K, np.ascontiguousarray(w), back)
        assert back.tolist() == row.tolist()
        shim.shim_build(1, np.array([0, K], dtype=np.int64), row.astype(np.int32), K, 1, gbeg, out)  # pack_list_group -> pack_put
        assert out.tolist() == w.tolist()
    for n in (0, 1, 5, 6, 7, 47, 48, 49, 700):
        for a in (1, 8):
            assert int(lm.pack_list_groups(np.int64(n), K, a)) == shim.shim_groups(n, K, a)
    for V in ((1 << 21) - 1, 1 << 21, (1 << 21) + 1, 1 << 25, (1 << 25) + 1):
        for with5 in (0, 1):
            assert lm.pack_k_for(V, with5) == shim.shim_k_for(V, with5)
    lens = np.array([0, 1, 2, 3, 4, 7, 8, 255, 256, (1 << 31) - 1, 1 << 31, (1 << 32) - 1])
    assert lm.pack_order_bucket(lens).tolist() == [max(int(x), 1).bit_length() - 1 for x in lens]


# ---- the mutants -----------------------------------------------------------------------------------------------------------------
TELLS = {
    "pad_first": "acd",       # b: every list is one id over and over, its first entry is its last
    "pad_zero": "abcd",
    "align_unfilled": "acd",  # b: every list is a multiple of 32 entries but one of 65,535, whose last group is no alignment group
    "no_ceil": "abcd",
    "desc_own_seg": "abcd",
    "desc_other_scan": "abcd",
    "work_wraps": "b",        # nowhere else does a sum reach 2^32
    "work_counts_own": "abcd",
    "sort_unstable": "abcd",
    "roff_gap_late": "abcd",
    "rhead_count_32": "abc",  # d: (rhead is not modelled there)
    "rhead_unshifted": "ac",  # b: entries 31 and 32 of every in-list are the same id
    "rhead_clamp_cnt": "ac",  # b: no in-list is shorter than 63 but those of one parallel run
    "k6_lt": "d",             # V = 2^21 alone
    "pack_ties_id_desc": "abcd",
}


def test_every_mutant_is_told_apart(families, models):
    assert set(TELLS) == set(lm.MUTANTS)
    seen = {}
    for mutant in lm.MUTANTS:
        fams, arrays = "", set()
        for name, gs in families.items():
            diff = set()
            for g, m in zip(gs, models[name]):
                diff |= set(lm.differences(m, lm.layout(g.V, *g.csr(), mutant=mutant, **options_of(name))))
            if diff:
                fams += name
                arrays |= diff
        seen[mutant] = fams
        print("%-18s families %-5s arrays %s" % (mutant, fams, sorted(arrays)))
        assert fams, "%s: differs nowhere" % mutant
    assert seen == TELLS


def test_a_mutant_changes_the_array_it_names(families, models):
    g, m = families["a"][-2], models["a"][-2]  # V = 769, as given
    where = {"pad_first": {"f.padded", "r.padded"}, "work_counts_own": {"f.work", "r.work"}, "desc_own_seg": {"f.desc", "r.desc"},
             "sort_unstable": None, "roff_gap_late": {"r.off"}, "rhead_count_32": {"r.rhead"}, "rhead_unshifted": {"r.rhead"},
             "rhead_clamp_cnt": {"r.rhead"}, "pack_ties_id_desc": {"f.packed", "r.packed"}, "desc_other_scan": {"f.desc", "r.desc"}}
    for mutant, want in where.items():
        got = set(lm.differences(m, lm.layout(g.V, *g.csr(), mutant=mutant)))
        if want is None:  # an unstable sort moves in-list entries: the reverse adjacency and what is copied from it
            assert "r.adj" in got and "f.adj" not in got and "r.off" not in got
        else:
            assert got == want, (mutant, got)
