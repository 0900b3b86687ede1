"""The hub tables an upload builds for k_meet3 (options meet_hubs, meet_hub_min_degree, meet_hub_min_count, meet_hub_mb), read
back with pgq_csr_hub_sizes / pgq_csr_hub_tables and compared bit for bit with the numpy model (tests/hub_model.py).

The graph: 5,000 vertices, directed; 130 planted vertices whose out-degree + in-degree is exactly 100 + 3 j (j = 0 .. 129), all
other vertices far below 100, so that meet_hub_min_degree = 100 + 3 (130 - n) selects exactly the n largest; vertices with an
empty out-list, with an empty in-list and with no edges at all.  Hub counts 1, 63, 64, 65, 127, 128 put a hub on each side of
every 64-bit word boundary; min_degree = 1 fills all H slots and cuts the ranking inside a run of equal degrees."""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from duckpgq_extension_amd import graphgen

import hub_model

pytestmark = pytest.mark.gpu

KEYS = ("meet_hubs", "meet_hub_min_degree", "meet_hub_min_count", "meet_hub_mb", "meet_layout")
V, PLANTED = 5000, 130
TABLES = ("hub1_out", "hub1_in", "hub2_out", "hub2_in")


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k in KEYS:
        pgq.set_option(k, int(pgq.get_default_option(k)))
    yield
    for k, v in saved.items():
        pgq.set_option(k, int(v))
    pgq.init_devices([0])


class Graph:
    def __init__(self):
        rng = np.random.default_rng(24)
        live = V - 100  # the last 100 ids have no edges
        s, d = rng.integers(0, live, 14000), rng.integers(0, live, 14000)
        planted = rng.choice(live, PLANTED, replace=False)
        pool = np.setdiff1d(np.arange(live), planted)[:2000]  # where the planted vertices' extra edges go, evenly
        deg = np.bincount(s, minlength=V) + np.bincount(d, minlength=V)
        at = 0
        for j, v in enumerate(planted):
            extra = 100 + 3 * j - int(deg[v])
            assert extra > 0
            other = pool[(at + np.arange(extra)) % len(pool)]
            at += extra
            out = j % 2 == 0  # every other planted vertex collects in-edges instead
            s = np.concatenate([s, np.full(extra, v) if out else other])
            d = np.concatenate([d, other if out else np.full(extra, v)])
        self.s, self.d = s.astype(np.int64), d.astype(np.int64)
        deg = np.bincount(self.s, minlength=V) + np.bincount(self.d, minlength=V)
        assert sorted(deg[planted]) == [100 + 3 * j for j in range(PLANTED)]
        assert np.delete(deg, planted).max() < 100
        outdeg, indeg = np.bincount(self.s, minlength=V), np.bincount(self.d, minlength=V)
        assert ((outdeg == 0) & (indeg > 0)).any() and ((indeg == 0) & (outdeg > 0)).any() and ((outdeg + indeg) == 0).any()
        self.off, self.adj, self.eid = graphgen.csr_from_rows(V, self.s, self.d)

    def upload(self, **opts):
        for k, v in opts.items():
            pgq.set_option(k, v)
        return pgq.DeviceCSR(V, self.off, self.adj, self.eid)


@pytest.fixture(scope="module")
def graph():
    return Graph()


def same_as_model(g, got, H, min_degree, hubs):
    ids = hub_model.select_hubs(V, g.s, g.d, H, min_degree=min_degree, min_count=1)
    assert got["H"] == H and got["words"] == H // 64 and got["hubs"] == hubs == int((ids >= 0).sum())
    assert (got["ids"] == ids).all(), "hub ids in bit order"
    want = hub_model.build_tables(V, g.s, g.d, ids)
    for name in TABLES:
        bad = np.argwhere(got[name] != want[name])
        assert len(bad) == 0, "%s: %d words differ, first: vertex %d word %d, %016x for %016x" % (
            name, len(bad), bad[0][0], bad[0][1], got[name][tuple(bad[0])], want[name][tuple(bad[0])])
    assert want["hub2_out"].any() and want["hub2_in"].any()


@pytest.mark.parametrize("H", [256, 1024])
@pytest.mark.parametrize("hubs", [1, 63, 64, 65, 127, 128, "H"])
def test_tables_are_the_models(graph, H, hubs):
    min_degree = 1 if hubs == "H" else 100 + 3 * (PLANTED - hubs)
    dev = graph.upload(meet_hubs=H, meet_hub_min_degree=min_degree, meet_hub_min_count=1)
    try:
        same_as_model(graph, dev.hub_tables(), H, min_degree, H if hubs == "H" else hubs)
    finally:
        dev.close()


def test_h_512_and_the_budget(graph):
    """meet_hubs = 512 as it is; 1024 under a budget of 2 MB (four tables of 5,000 x 128 bytes are 2.4 MB) is halved to 512."""
    for opts in (dict(meet_hubs=512), dict(meet_hubs=1024, meet_hub_mb=2)):
        dev = graph.upload(meet_hub_min_degree=100, meet_hub_min_count=1, **opts)
        try:
            same_as_model(graph, dev.hub_tables(), 512, 100, PLANTED)
        finally:
            dev.close()
        pgq.set_option("meet_hub_mb", int(pgq.get_default_option("meet_hub_mb")))


@pytest.mark.parametrize("opts", [dict(meet_hubs=0), dict(meet_hub_mb=0), dict(meet_hub_min_count=PLANTED + 1),
                                  dict(meet_hub_min_degree=100 + 3 * PLANTED), dict(meet_layout=0)],
                         ids=["meet_hubs_0", "over_the_budget", "too_few_hubs", "no_hub", "no_layout"])
def test_no_tables_is_unsupported(graph, opts):
    base = dict(meet_hubs=256, meet_hub_min_degree=100, meet_hub_min_count=1)
    base.update(opts)
    dev = graph.upload(**base)
    try:
        for call in (dev.hub_sizes, dev.hub_tables):
            with pytest.raises(pgq.PgqError, match="error -6"):
                call()
        out, ok = dev.iterativelength(graph.s[:64], graph.d[:64])  # the handle works without them
        assert ok.all() and (out == 1).all()
    finally:
        dev.close()


def test_defaults_leave_a_small_graph_alone(graph):
    """As shipped a hub has 128 edges and 64 of them make a table: this graph has 130 planted vertices, 120 of them with 128 or more."""
    dev = graph.upload()
    try:
        got = dev.hub_tables()
        same_as_model(graph, got, 1024, 128, int((np.bincount(graph.s, minlength=V) + np.bincount(graph.d, minlength=V) >= 128).sum()))
    finally:
        dev.close()


def test_a_replica_holds_the_same_tables(graph):
    dev = graph.upload(meet_hubs=256, meet_hub_min_degree=100, meet_hub_min_count=1)
    try:
        bytes_with = dev.device_bytes
        own = dev.hub_tables()
        assert pgq.init_devices([0, 0]) == 2
        dev.replicate()
        copy = dev.hub_tables(replica=1)
        for name in TABLES + ("ids", "H", "hubs", "words"):
            assert np.array_equal(own[name], copy[name]), name
        with pytest.raises(pgq.PgqError):
            dev.hub_tables(replica=2)
    finally:
        dev.close()
        pgq.init_devices([0])
    plain = graph.upload(meet_hubs=0)
    try:  # the tables are counted in the handle's bytes: four of V x H / 8 and the ids
        assert bytes_with - plain.device_bytes == 4 * V * (256 // 8) + 4 * 256
    finally:
        plain.close()


def test_the_tables_move_no_route():
    """The routing calibration (bytes a pre-pass row moves) is about the walks, with tables as without: after a call of random
    pairs has refined it, a cross product of 256 sources x 2048 destinations takes the lane batches on both handles or on neither,
    and so does every other shape here; all answers equal."""
    import torch
    saved = {k: pgq.get_option(k) for k in ("calibration_cache", "route_memo", "route_timing")}
    for k in saved:
        pgq.set_option(k, 0)  # every handle measures for itself, every call is routed afresh
    Vk, s, d = graphgen.snb_knows_like(20000, 600_000, seed=3)
    off, adj, eid = graphgen.csr_from_rows(Vk, s, d)
    rng = np.random.default_rng(5)
    shapes = {"random": (rng.integers(0, Vk, 32768), rng.integers(0, Vk, 32768))}
    for sources, dests in ((256, 2048), (2048, 32), (16, 4096)):
        shapes["%d x %d" % (sources, dests)] = (np.repeat(rng.choice(Vk, sources, replace=False), dests), rng.integers(0, Vk, sources * dests))
    seen = {}
    try:
        for hubs in (1024, 0):
            pgq.set_option("meet_hubs", hubs)
            dev = pgq.DeviceCSR(Vk, off, adj, eid)
            try:
                assert (hubs > 0) == (dev.hub_sizes()["hubs"] > 64) if hubs else True
                for turn in (0, 1):  # the second turn is routed under what the first one measured
                    for name, (ps, pd) in shapes.items():
                        t_s, t_d = torch.from_numpy(ps).cuda(), torch.from_numpy(pd).cuda()
                        t_o = torch.full((len(ps),), -7, dtype=torch.int64, device="cuda")
                        pgq.reset_stats()
                        dev.iterativelength_bulk_ptr(len(ps), t_s.data_ptr(), t_d.data_ptr(), t_o.data_ptr())
                        st = pgq.get_stats()
                        seen[hubs, turn, name] = (st["levels"] > 0, st["ball_calls"] > 0, t_o.cpu().numpy())
                        print("meet_hubs %d, turn %d, %s: levels %d, ball_calls %d, meet_pairs %d" % (
                            hubs, turn, name, st["levels"], st["ball_calls"], st["meet_pairs"]))
            finally:
                dev.close()
        for (hubs, turn, name), (lanes, ball, out) in seen.items():
            want = seen[0, turn, name]
            assert (lanes, ball) == want[:2], "%s, turn %d: another route with the tables" % (name, turn)
            assert (out == want[2]).all(), name
    finally:
        for k, v in saved.items():
            pgq.set_option(k, int(v))
