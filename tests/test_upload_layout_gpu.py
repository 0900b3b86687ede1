"""Everything the upload derives for the pair-centric and source-centric kernels (csrc/pgq_runtime.hip: finish_upload,
build_meet_layout), read back through pgq_csr_meet_layout and compared entry for entry with tests/layout_model.py: the reverse
CSR, padj / rpadj, fseg / rseg, fdesc / rdesc, fwork / rwork, ppadj / prpadj, rhead and the scalars.  Every comparison is exact
and of whole arrays.  The graphs are helpers.layout_*: blocks of 256 vertices on the edges of the upload kernels' LDS
searches (a), a two-hop sum of 2^32 (b), one vertex block and one slot trip more than the grid-stride loops' grids (c), the top
of the 21- and 25-bit id ranges and V = 2^k, 2^k + 1 (d), no vertices, no edges, no layout (e); each as given and transposed.
test_layout_model_cpu.py holds the model to a loop over the vertices and shows which family tells which wrong decision apart."""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
import layout_model as lm
from helpers import (LAYOUT_BLOCK_V, LayoutGraph, layout_blocks, layout_end_bit, layout_id_width, layout_saturation,
                     layout_second_trips)
from oracle.pgq_oracle import OracleCSR

pytestmark = pytest.mark.gpu

# every option this file touches (all but meet / meet_bias are read at upload)
KEYS = ("meet_layout", "meet_align", "meet_pack", "meet_pack_align", "meet_pack_order", "ball", "ball_head_mb", "upload_narrow_host",
        "hub_chunk", "part_weight", "meet", "meet_bias")
MODEL_KEYS = ("meet_layout", "meet_align", "meet_pack", "meet_pack_align", "meet_pack_order", "ball", "ball_head_mb")
PATHS = ("narrow_host", "wide_host", "device_ptrs", "device_rows")


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k in KEYS:
        pgq.set_option(k, pgq.get_default_option(k))
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


def set_options(**kw):
    for k, v in kw.items():
        pgq.set_option(k, v)


def model_of(g):
    """The model under the options in force."""
    return lm.layout(g.V, *g.csr(), **{k: int(pgq.get_option(k)) for k in MODEL_KEYS})


def shuffled_rows(rng, off, adj):
    """The CSR's slots as edge-table rows in a shuffled arrival order that keeps the rows of one source in slot order (the
    order create_csr_edge's single-threaded schedule turns into slots), with arbitrary edge ids and weights."""
    src = lm.slot_owners(off)
    place = np.argsort(src[rng.permutation(len(src))], kind="stable")  # where the rows of each source arrive
    s, d = np.empty_like(src), np.empty_like(src)
    s[place], d[place] = src, adj
    eid = rng.permutation(len(src)).astype(np.int64) + 1000
    w = rng.integers(0, 1000, len(src)).astype(np.int64)
    return s, d, eid, w


def upload(g, path, rows=None, w=None, adj=None):
    """A handle for graph g by one of the four upload paths.  `rows` (shuffled_rows) feeds device_rows; `adj` replaces the
    adjacency (the refused uploads), `w` the weights."""
    import torch
    off, a = g.csr()
    a = a if adj is None else adj
    if path in ("narrow_host", "wide_host"):
        pgq.set_option("upload_narrow_host", 1 if path == "narrow_host" else 0)
        return pgq.DeviceCSR(g.V, off, a, None, w)
    if path == "device_ptrs":
        t = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).cuda() for x in (off, a if len(a) else np.zeros(1))]
        tw = None if w is None else torch.from_numpy(np.ascontiguousarray(w)).cuda()
        torch.cuda.synchronize()
        return pgq.DeviceCSR.from_device_ptrs(g.V, t[0].data_ptr(), t[1].data_ptr(), 0, 0 if w is None else tw.data_ptr(), 0 if w is None else 1)
    s, d, eid, rw = rows
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (s, d, eid, rw)]
    torch.cuda.synchronize()
    return pgq.DeviceCSR.build_from_device_rows(g.V, len(s), *(x.data_ptr() for x in t), w_type=1)


def read_back(dev):
    """The handle's arrays in the shape of layout_model.layout's result."""
    dirs = [dev.meet_layout(0), dev.meet_layout(1)]
    res = {k: dirs[0][k] for k in lm.SCALARS}
    assert all(dirs[1][k] == res[k] for k in lm.SCALARS)
    res["has_layout"] = dev.has_prepass_layout
    res["dirs"] = dirs
    return res


def check(dev, want, what):
    got = read_back(dev)
    diff = lm.differences(got, want)
    assert got["has_layout"] == want["has_layout"] and diff == [], "%s: differs from the model in %s" % (what, diff)
    return got


def both(g):
    return [g, g.transposed()]


# ---- a: blocks, the whole option grid ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blocks():
    return [x for V in LAYOUT_BLOCK_V for x in both(layout_blocks(V))]


@pytest.mark.parametrize("meet_align", [4, 8, 32, 64])
def test_blocks_under_every_option(blocks, meet_align):
    n = 0
    for pack_align in (1, 8):
        for order in (0, 1):
            for pack in (0, 1):
                for head_mb in (512, 0):
                    set_options(meet_align=meet_align, meet_pack_align=pack_align, meet_pack_order=order, meet_pack=pack, ball_head_mb=head_mb)
                    for g in blocks:
                        want = model_of(g)
                        assert want["pack_k"] == (6 if pack else 4) and want["has_rhead"] == (1 if head_mb else 0)
                        dev = upload(g, "narrow_host")
                        check(dev, want, "%s, meet_align %d, meet_pack_align %d, meet_pack_order %d, meet_pack %d, ball_head_mb %d" % (
                            g.name, meet_align, pack_align, order, pack, head_mb))
                        dev.close()
                        n += 1
    assert n == 16 * 2 * len(LAYOUT_BLOCK_V)


def test_ball_off_builds_no_heads(blocks):
    set_options(ball=0)
    g = blocks[-2]
    dev = upload(g, "narrow_host")
    got = check(dev, model_of(g), g.name + ", ball 0")
    assert got["has_rhead"] == 0 and got["dirs"][1]["rhead"] is None
    dev.close()


# ---- the four upload paths -------------------------------------------------------------------------------------------------------
def paths_agree(g, rng, what):
    want = model_of(g)
    off, adj = g.csr()
    rows = shuffled_rows(rng, off, adj)
    first = None
    for path in PATHS:
        dev = upload(g, path, rows=rows)
        got = check(dev, want, "%s, %s" % (what, path))
        if first is None:
            first = got
        assert lm.differences(got, first) == []
        if path == "device_rows":
            s, d, eid, w = rows
            ora = OracleCSR.from_edges(g.V, s, d, eid, w)
            o, a, e, ww = dev.download()
            assert (o == ora.v[:g.V + 1]).all() and (a == ora.e).all() and (e == ora.edge_ids).all() and (ww == ora.w).all()
            assert (o == off).all() and (a == adj).all()
        dev.close()


@pytest.mark.parametrize("V", LAYOUT_BLOCK_V)
def test_upload_paths_agree_on_blocks(V):
    rng = np.random.default_rng(V)
    for g in both(layout_blocks(V)):
        paths_agree(g, rng, g.name)


@pytest.fixture(scope="module")
def second_trips():
    return layout_second_trips()


@pytest.mark.parametrize("side", [0, 1], ids=["graph", "transpose"])
def test_upload_paths_agree_past_the_grids(second_trips, side):
    # one list per group and per packed group keeps the read-back small; the shapes are the issue, not the padding
    set_options(meet_align=4, meet_pack_align=1)
    paths_agree(both(second_trips)[side], np.random.default_rng(side), "second trips")


def test_second_trips_under_the_shipped_options(second_trips):
    check_one(second_trips, "second trips, shipped options")


def check_one(g, what, path="narrow_host"):
    dev = upload(g, path)
    got = check(dev, model_of(g), what)
    dev.close()
    return got


# ---- the last slot, the last row ----------------------------------------------------------------------------------------------------
def refusal(call):
    with pytest.raises(pgq.PgqError) as e:
        call()
    return str(e.value)


def test_negative_weight_in_the_last_slot(second_trips):
    g = second_trips
    E = len(g.src)
    off, adj = g.csr()
    rows = (g.src, g.dst, np.arange(E, dtype=np.int64), None)
    said = {}
    for path in PATHS:
        for slot in (0, E - 1):
            w = np.ones(E, dtype=np.int64)
            w[slot] = -1
            dev = upload(g, path, rows=rows[:3] + (w,), w=w)
            said[path, slot] = refusal(lambda: dev.cheapest_path_length(np.array([0]), np.array([1])))
            dev.close()
        assert "negative edge weights" in said[path, 0] and said[path, E - 1] == said[path, 0]
    dev = upload(g, "narrow_host", w=np.ones(E, dtype=np.int64))  # and no flag without one
    out, ok = dev.cheapest_path_length(np.array([0]), np.array([1]))  # the edge 0 -> 1
    assert ok.tolist() == [True] and out.tolist() == [1]
    dev.close()


def test_id_out_of_range_in_the_last_slot(second_trips):
    g = second_trips
    E = len(g.src)
    off, adj = g.csr()
    before = pgq.live_device_blocks()
    for path in PATHS:
        said = []
        for slot in (0, E - 1):
            bad = adj.copy()
            bad[slot] = g.V
            if path == "device_rows":
                said.append(refusal(lambda: upload(g, path, rows=(g.src, bad, np.arange(E, dtype=np.int64), np.ones(E, dtype=np.int64)))))
            else:
                said.append(refusal(lambda: upload(g, path, adj=bad)))
        assert said[0] == said[1] and ("out of" in said[0]), (path, said)
    assert pgq.live_device_blocks() == before  # a refused upload leaves nothing behind


# ---- b: saturation ----------------------------------------------------------------------------------------------------------------
def test_two_hop_work_saturates():
    g = layout_saturation()
    got = check_one(g, "saturation")
    work = got["dirs"][0]["work"]
    assert int(work[g.h]) == (1 << 32) - 1 and int(work[g.h2]) == (1 << 32) - 65536
    got = check_one(g.transposed(), "saturation, transposed")
    assert int(got["dirs"][1]["work"][g.h]) == (1 << 32) - 1 and int(got["dirs"][1]["work"][g.h2]) == (1 << 32) - 65536


# ---- d: the width of an id ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,pack,pack_k,head_mb", [(1 << 21, 1, 6, 512), (1 << 21, 1, 6, 0), ((1 << 21) + 1, 2, 5, 512), ((1 << 21) + 1, 1, 4, 512)],
                         ids=["2^21_heads", "2^21", "2^21+1_pack_2", "2^21+1_pack_1"])
def test_top_of_the_id_range(V, pack, pack_k, head_mb):
    g = layout_id_width(V)
    heads = 1 if V * 256 <= head_mb << 20 else 0
    for order in (0, 1):
        for k, side in enumerate(both(g)):
            if heads and (order, k) != (1, 0):
                continue  # 512 MB of heads are read back and modelled once; the case without them runs every combination
            set_options(meet_pack=pack, meet_pack_order=order, ball_head_mb=head_mb)
            got = check_one(side, "%s, meet_pack %d, meet_pack_order %d" % (side.name, pack, order))
            assert got["pack_k"] == pack_k and (got["dirs"][0]["packed"] is None) == (pack_k == 4)
            assert got["has_rhead"] == heads


@pytest.mark.parametrize("V", [1024, 1025])
def test_sort_keys_at_a_power_of_two(V):
    for side in both(layout_end_bit(V)):
        for order in (0, 1):
            set_options(meet_pack_order=order)
            check_one(side, "%s, meet_pack_order %d" % (side.name, order))


# ---- e: degenerate -----------------------------------------------------------------------------------------------------------------
def test_no_layout():
    L = pgq.load_hip()
    word = np.zeros(16, dtype=np.uint32)
    cases = [(LayoutGraph("no_vertices", 0, [], []), {}), (LayoutGraph("no_edges", 300, [], []), {}),
             (layout_blocks(257), dict(meet_layout=0))]
    for g, opts in cases:
        set_options(**opts)
        for path in ("narrow_host", "device_ptrs"):
            dev = upload(g, path)
            got = check(dev, model_of(g), g.name + ", " + path)
            assert got["has_layout"] == 0 and dev.has_prepass_layout == 0
            assert [got[k] for k in ("groups", "rgroups", "pgroups", "prgroups", "has_rhead", "pack_k")] == [0, 0, 0, 0, 0, 4]
            for d in got["dirs"]:
                assert all(d[k] is None for k in ("seg", "padded", "desc", "work", "packed", "rhead"))
            for slot in range(2, 8):  # seg, padded, desc, work, packed, rhead: none of them exists
                args = [None] * 8
                args[slot] = word.ctypes.data
                assert L.pgq_csr_meet_layout(dev.h, 1, *args) == -6, slot  # PGQ_ERR_UNSUPPORTED
            dev.close()
    set_options(meet_layout=1, meet_pack=0)
    dev = upload(layout_blocks(257), "narrow_host")
    none = [None] * 8
    assert L.pgq_csr_meet_layout(dev.h, 2, *none) == -4 and L.pgq_csr_meet_layout(None, 0, *none) == -4  # PGQ_ERR_INVALID_ARG
    assert L.pgq_csr_meet_layout_sizes(None, word.ctypes.data) == -4 and L.pgq_csr_meet_layout_sizes(dev.h, None) == -4
    assert L.pgq_csr_meet_layout(dev.h, 0, *none[:6], word.ctypes.data, None) == -6  # no packed copy under meet_pack 0
    assert L.pgq_csr_meet_layout(dev.h, 0, *none[:7], word.ctypes.data) == -6  # heads are the reverse direction's
    assert L.pgq_csr_meet_layout(dev.h, 0, *none) == 0
    dev.close()


# ---- the comparison bites --------------------------------------------------------------------------------------------------------------
def test_the_device_differs_from_every_mutant():
    """What the device built equals the model and differs from each of the model's one-decision mutants on at least one of
    three graphs: the comparison above would not pass a kernel that took any of those decisions."""
    set_options(ball_head_mb=0)
    wide = layout_id_width(1 << 21)
    cases = [(wide, check_one(wide, wide.name), dict(ball_head_mb=0))]
    set_options(ball_head_mb=512)
    for g in both(layout_blocks(769)) + [layout_saturation()]:
        cases.append((g, check_one(g, g.name), {}))
    for mutant in lm.MUTANTS:
        told = [g.name for g, got, opts in cases if lm.differences(got, lm.layout(g.V, *g.csr(), mutant=mutant, **opts))]
        assert told, "%s: the device's arrays equal this mutant's on every graph" % mutant


# ---- recycled blocks ----------------------------------------------------------------------------------------------------------------
def test_a_recycled_block_shows_nowhere():
    before = pgq.live_device_blocks()
    a = layout_blocks(513)
    b = a.transposed()  # the same V and E, other lists
    assert len(a.src) == len(b.src) and lm.differences(model_of(a), model_of(b)) != []
    for order in (0, 1):
        set_options(meet_pack_order=order)
        dev = upload(a, "narrow_host")
        check(dev, model_of(a), "A")
        dev.close()
        dev = upload(b, "narrow_host")  # takes A's blocks from the cache: same sizes
        check(dev, model_of(b), "B after A, meet_pack_order %d" % order)
        dev.close()
    assert pgq.live_device_blocks() == before


# ---- a handle that was read back still searches --------------------------------------------------------------------------------------
def test_searching_after_read_back():
    g = layout_end_bit(1025)
    rng = np.random.default_rng(11)
    ps, pd = rng.integers(0, g.V, 500), rng.integers(0, g.V, 500)
    ora = OracleCSR.from_edges(g.V, g.src, g.dst)
    want = ora.lean_shortestpath(g.V, ps, pd)
    assert sum(p is not None for p in want) > 250
    set_options(meet=1, meet_bias=1e9)
    dev = upload(g, "narrow_host")
    m = model_of(g)
    check(dev, m, g.name)
    assert dev.shortestpath(ps, pd) == want
    check(dev, m, g.name + ", after the search")  # and the search left the layout alone
    dev.close()
