"""Who owns a CSR handle's device memory (csr_arrays in pgq_internal.h): nothing a handle allocated outlives it, a replica
carries every array the upload built, and a first-use build that fails leaves nothing behind.  The count is
pgq_debug_live_device_blocks(): blocks the library's block cache has handed out and not got back, whatever it keeps cached.

One graph for all of it: 3,000 vertices, about 40,000 edges with positive int64 weights, and one planted vertex with 200
in-edges, uploaded under hub_chunk = 64 so that the hub slices (pull_hubs, pull_hub_vertices) exist; V <= 2^21, so the
bit-packed lists (pack_k = 6) and the fixed-stride in-list heads are built as well."""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from duckpgq_extension_amd import graphgen
from oracle.pgq_oracle import OracleCSR

pytestmark = pytest.mark.gpu

V, E_RANDOM, HUB, HUB_IN = 3000, 39800, 1234, 200
GLOBAL_KEYS = ("hub_chunk", "upload_narrow_host")  # read by the upload, before a handle (and its own options) exists
HANDLE_KEYS = ("hub_chunk", "meet", "meet_bias", "ball", "ball_sort", "force_mode", "relax_light", "wbibfs", "relax_bidir")


class Graph:
    def __init__(self):
        rng = np.random.default_rng(2029)
        s = np.concatenate([rng.integers(0, V, E_RANDOM), rng.choice(V, HUB_IN, replace=False)])
        d = np.concatenate([rng.integers(0, V, E_RANDOM), np.full(HUB_IN, HUB)])
        self.rows = (s.astype(np.int64), d.astype(np.int64))
        self.off, self.adj, self.eid = graphgen.csr_from_rows(V, *self.rows)
        self.w = rng.integers(1, 50, len(self.adj)).astype(np.int64)
        self.row_w = np.empty_like(self.w)
        self.row_w[self.eid] = self.w  # the weights in edge-table order: csr_from_rows puts row eid[k] into slot k
        self.ora = OracleCSR.adopt(V, self.off, self.adj, self.eid, self.w)
        assert int(np.bincount(self.adj, minlength=V)[HUB]) > 64
        self.ps, self.pd = rng.integers(0, V, 300), rng.integers(0, V, 300)
        self.pd[:8] = HUB
        # the binder's shape: 8 sources x 512 destinations, grouped by source, and the same rows in a hash join's order
        src = rng.choice(V, 8, replace=False)
        self.cs, self.cd = np.repeat(src, 512).astype(np.int64), rng.integers(0, V, 8 * 512)
        self.cd[::64] = HUB
        self.shuffle = rng.permutation(len(self.cs))
        ln, ok = self.ora.lean_iterativelength(V, self.cs, self.cd, nthreads=8)
        self.cross_want = np.where(ok, ln, -1)
        self.paths_want = self.ora.lean_shortestpath(V, self.ps, self.pd)
        self.cheap_want, self.cheap_ok = self.ora.lean_cheapest_path_length(V, self.ps, self.pd)
        # about one destination per source: the shape the bidirectional relaxation takes
        self.us = rng.permutation(V)[:64].astype(np.int64)
        self.ud = rng.integers(0, V, 64)
        self.ucheap_want, self.ucheap_ok = self.ora.lean_cheapest_path_length(V, self.us, self.ud)


@pytest.fixture(scope="module")
def graph():
    return Graph()


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in GLOBAL_KEYS}
    pgq.set_option("hub_chunk", 64)
    yield
    for k, v in saved.items():
        pgq.set_option(k, int(v))
    pgq.init_devices([0])


def set_on(dev, **kw):
    assert set(kw) <= set(HANDLE_KEYS)
    for k, v in kw.items():
        dev.set_option(k, v)


def upload_lazy(g):
    return pgq.DeviceCSR(V, g.off, g.adj, g.eid, g.w, lazy_edge_ids=True)


def upload_wide(g):  # the adjacency crosses PCIe as int64 and is narrowed on the device: upload_impl's second temporary
    pgq.set_option("upload_narrow_host", 0)
    try:
        return pgq.DeviceCSR(V, g.off, g.adj, g.eid, g.w, lazy_edge_ids=True)
    finally:
        pgq.set_option("upload_narrow_host", 1)


def build_on_device(g):
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (*g.rows, np.arange(len(g.adj), dtype=np.int64), g.row_w)]
    torch.cuda.synchronize()
    dev = pgq.DeviceCSR.build_from_device_rows(V, len(g.adj), *(x.data_ptr() for x in t), w_type=1)
    del t
    return dev


def whole_life(g, make):
    """Everything that allocates for a handle, once: upload, replicas, the lazily copied edge ids, every array built on
    first use (wadj / wsorted, rw, rwadj / rwsorted, pagerank, wcc), on the primary and through the *_multi entry point
    on the replicas; then the handle is closed."""
    dev = make(g)
    try:
        assert dev.pack_k == 6
        set_on(dev, hub_chunk=64)
        assert pgq.init_devices([0, 0, 0]) == 3
        dev.replicate()
        assert dev.shortestpath(g.ps[:64], g.pd[:64]) == g.paths_want[:64]
        set_on(dev, relax_light=2, wbibfs=1)
        out, ok = dev.cheapest_path_length(g.ps[:64], g.pd[:64])
        assert (ok == g.cheap_ok[:64]).all() and (out[ok] == g.cheap_want[:64][ok]).all()
        set_on(dev, relax_bidir=1)
        out, ok = dev.cheapest_path_length(g.us, g.ud)
        assert (ok == g.ucheap_ok).all() and (out[ok] == g.ucheap_want[ok]).all()
        out, ok = dev.cheapest_path_length_multi(g.ps, g.pd)  # the replicas build their own first-use arrays
        assert (ok == g.cheap_ok).all() and (out[ok] == g.cheap_want[ok]).all()
        rank, ok, _ = dev.pagerank(np.arange(8))
        assert ok.all() and (rank > 0).all()
        assert dev.L.pgq_weakly_connected_component_device(dev.h, None) == 0
    finally:
        dev.close()
        pgq.init_devices([0])


@pytest.mark.parametrize("make", [upload_lazy, build_on_device, upload_wide], ids=lambda f: f.__name__)
def test_nothing_outlives_a_handle(graph, make):
    whole_life(graph, make)  # a throw-away handle first: workspaces, pooled streams and pinned blocks exist from here on
    before = pgq.live_device_blocks()
    whole_life(graph, make)
    assert pgq.live_device_blocks() == before


def test_a_replica_carries_every_upload_time_array(graph):
    """Device list [0, 0]: the second shard of every *_multi call runs on the clone.  Each route is first run on shard
    0's rows alone (device list [0]: the primary), so that its counter over both shards shows the clone took the route
    too and did not fall back to another one; every row is compared with the oracle."""
    g = graph
    dev = pgq.DeviceCSR(V, g.off, g.adj, g.eid, g.w)
    routes = {  # name: (handle options, rows, the counter that shows the route ran)
        # source-centric kernel: rseg, rhead, rpadj
        "ball": (dict(meet=1, meet_bias=1e9, ball=2, force_mode=0), (g.cs, g.cd, g.cross_want), lambda st: st["ball_calls"]),
        # pair-centric pre-pass: the packed lists and the slot descriptors
        "prepass": (dict(meet=1, meet_bias=1e9, ball=0, force_mode=0),
                    (g.cs[g.shuffle], g.cd[g.shuffle], g.cross_want[g.shuffle]), lambda st: st["meet_pairs"]),
        # bottom-up lane batches: pull_parts, rown, rpk and the hub slices
        "pull": (dict(meet=0, ball=0, force_mode=2), (g.cs[g.shuffle], g.cd[g.shuffle], g.cross_want[g.shuffle]),
                 lambda st: st["levels"]),
    }
    try:
        assert dev.pack_k == 6
        set_on(dev, hub_chunk=64)
        shard0 = {}
        for name, (opts, (ps, pd, want), counter) in routes.items():
            set_on(dev, **opts)
            h = (len(ps) + 1) // 2
            pgq.reset_stats()
            assert (dev.iterativelength_multi(ps[:h], pd[:h]) == want[:h]).all(), name
            shard0[name] = counter(pgq.get_stats())
            assert shard0[name] > 0, name
        assert pgq.get_stats()["launches"]["pull_hub"] > 0  # (the pull route ran last: the planted vertex is a hub)
        assert pgq.init_devices([0, 0]) == 2
        for name, (opts, (ps, pd, want), counter) in routes.items():
            set_on(dev, **opts)
            pgq.reset_stats()
            assert (dev.iterativelength_multi(ps, pd) == want).all(), name
            st = pgq.get_stats()
            print(name, "shard 0 alone:", shard0[name], "both shards:", counter(st))
            assert st["pairs"] == len(ps) and counter(st) > shard0[name], name
        set_on(dev, meet=1, meet_bias=1.0, ball=1, force_mode=0)
        ln, off, child = dev.shortestpath_multi(g.ps, g.pd)
        got = [None if ln[i] < 0 else child[off[i]:off[i] + 2 * ln[i] + 1].tolist() for i in range(len(g.ps))]
        assert got == g.paths_want
        out, ok = dev.cheapest_path_length_multi(g.ps, g.pd)
        assert (ok == g.cheap_ok).all() and (out[ok] == g.cheap_want[ok]).all()
    finally:
        dev.close()
        pgq.init_devices([0])


def test_a_refused_first_use_build_leaves_nothing_behind(graph):
    g = graph
    dev = pgq.DeviceCSR(V, g.off, g.adj, g.eid)  # no weights
    try:
        ln, ok = dev.iterativelength(g.ps, g.pd)  # (its workspace exists before the count is taken)
        before = pgq.live_device_blocks()
        with pytest.raises(pgq.PgqError, match="Need to initialize CSR before doing cheapest path"):
            dev.cheapest_path_length(g.ps, g.pd)
        assert pgq.live_device_blocks() == before
        ln2, ok2 = dev.iterativelength(g.ps, g.pd)
        want, want_ok = g.ora.lean_iterativelength(V, g.ps, g.pd)
        assert (ok2 == want_ok).all() and (ln2[ok2] == want[want_ok]).all()
        assert (ok == ok2).all() and (ln == ln2).all()
    finally:
        dev.close()
