"""The lane batches' expansion kernels — k_push with k_queue_from_dense, k_pull, k_pull_sparse, k_pull_lanes, k_pull_hub with
its zero and fold — and the work partition finish_upload builds for them, ON their partition limits.

helpers.pull_gadgets puts the one in-edge that answers a row at a chosen in-slot: the first and last slot of a part of 16
vertices, either side of the weight rule, of a run of 256 and of a hub; the ends of the trips of 64 x UN in-slots; roff[v0] mod
4 = 0 .. 3; the first and last slot of a hub's first, middle and last slice; the last slot of a push item.  Its decoys are
frontier vertices with other lanes' bits (test_pull_gadgets_cpu.py proves all that on the CPU, and that a scan which loses or
misplaces such an entry answers a gadget row wrongly).  Two graphs: one uploaded under part_weight 64 and hub_chunk 64, one
under the defaults.

Every run forces the lane batches (meet 0, ball 0) and turns the probes off (probe 0, probe2 0): the expansion decides a row,
k_detect only reads what it left.  Every expected value is the CPU oracle's, every comparison is exact, and every call is made
twice on the same handle: the first makes a round trip per level, the second replays the stored plan.  After a configuration
the launch counters say that the kernel class it aims at ran (k_pull_lanes counts as pull_sparse: pull_level times it under
K_PULL_SPARSE)."""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from duckpgq_extension_amd import graphgen
from helpers import PULL_LIMITS, hub_slices_model, pull_gadgets, pull_parts_model
from oracle.pgq_oracle import OracleCSR
from test_probe_limits_gpu import KEYS as PROBE_KEYS

pytestmark = pytest.mark.gpu

KEYS = PROBE_KEYS + ("part_weight", "sparse_unroll", "sparse_pw", "sparse_spill", "sparse_below")
CONFIGS = {"smallest": (64, 64), "defaults": (PULL_LIMITS["part_weight"], PULL_LIMITS["hub_chunk"])}
BOUNDS = (0, 1, 2, 3, 4, 5)  # the rows are 1, 2, 3 and 5 hops long: every row sees max_hops = its distance and one less


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


def expansion(**options):
    """Every row through the lane batches, the probes off, under `options`."""
    for k, v in dict(meet=0, ball=0, probe=0, probe2=0, **options).items():
        pgq.set_option(k, v)


def upload(V, src, dst, part_weight, hub_chunk):
    """hub_chunk and part_weight are read at upload, from the process-wide options; everything else is the library's default."""
    saved = {k: pgq.get_option(k) for k in KEYS}
    defaults()
    pgq.set_option("part_weight", part_weight)
    pgq.set_option("hub_chunk", hub_chunk)
    st = pgq.PgqState()
    st.build_csr(0, V, src, dst)
    dev = st.device_csr(0)  # the upload itself: the first request for the device handle
    for k, v in saved.items():
        pgq.set_option(k, v)
    return st, dev


class Case:
    """The gadget graph of a configuration, uploaded under it; the oracle's distances and path lists, computed once."""

    def __init__(self, config):
        g = self.g = pull_gadgets(*CONFIGS[config])
        self.config = config
        self.ora = OracleCSR.from_edges(g.V, g.src, g.dst)
        ln, ok = self.ora.lean_iterativelength(g.V, g.rs, g.rd, nthreads=8)
        self.dist = np.where(ok, ln, -1)
        assert (self.dist == g.dist).all()  # the builder's own distances (test_pull_gadgets_cpu.py): the expected values are the oracle's
        self.path_rows = np.flatnonzero(self.dist > 0)
        paths = self.ora.lean_shortestpath(g.V, g.rs[self.path_rows], g.rd[self.path_rows])
        assert all(len(p) == 2 * k + 1 for p, k in zip(paths, self.dist[self.path_rows]))
        self.paths = dict(zip(self.path_rows.tolist(), paths))
        self.st, self.dev = upload(g.V, g.src, g.dst, g.part_weight, g.hub_chunk)

    def close(self):
        self.st.delete_csr(0)


@pytest.fixture(scope="module", params=list(CONFIGS))
def case(request):
    c = Case(request.param)
    yield c
    c.close()


def payload(out, ok):
    assert (out[~ok] == -1).all(), "a NULL row's payload is -1"
    return np.where(ok, out, -1)


class Launches:
    """The launch counters of every call of a configuration, summed; every call went through the lane batches alone."""

    def __init__(self):
        self.n = {}

    def add(self, stats, what, levels=True):
        assert stats["meet_pairs"] == 0 and stats["ball_calls"] == 0 and (stats["launches"]["detect"] > 0 or not levels), (
            what, stats["meet_pairs"], stats["ball_calls"], stats["launches"])
        for k, v in stats["launches"].items():
            self.n[k] = self.n.get(k, 0) + v


def twice(call, want, what, tags, seen, levels=True):
    """`call` two times (a round trip per level, then the stored plan ahead of the host): both answer `want`."""
    for turn in ("first call", "second call"):
        pgq.reset_stats()
        got = call()
        seen.add(pgq.get_stats(), what, levels)
        bad = [i for i in range(len(want)) if not np.array_equal(got[i], want[i])]
        assert not bad, "%s, %s: %d of %d rows differ, first: gadget %s got %s, expected %s" % (
            what, turn, len(bad), len(want), tags[bad[0]], got[bad[0]], want[bad[0]])


def check_rows(case, rows, what, seen, lengths_only=False):
    """The four forms on one set of rows: iterativelength by chunk and in bulk, iterativelength_within at every bound,
    shortestpath on the rows that have a path, as whole lists (k_reconstruct reads the same `seen` levels)."""
    import torch
    g, dev = case.g, case.dev
    ps, pd, want, tags = g.rs[rows], g.rd[rows], case.dist[rows], g.tag[rows]
    twice(lambda: payload(*dev.iterativelength(ps, pd)), want, what + ", chunk form", tags, seen)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(ps)).cuda(), torch.from_numpy(np.ascontiguousarray(pd)).cuda()
    t_o = torch.empty(len(ps), dtype=torch.int64, device="cuda")

    def bulk():
        t_o.fill_(-7)
        dev.iterativelength_bulk_ptr(len(ps), t_s.data_ptr(), t_d.data_ptr(), t_o.data_ptr())
        return t_o.cpu().numpy()

    twice(bulk, want, what + ", bulk form", tags, seen)
    if lengths_only:
        return
    for U in BOUNDS:
        clamped = np.where((want >= 0) & (want <= U), want, -1)
        twice(lambda: payload(*dev.iterativelength_within(ps, pd, U)), clamped, "%s, max_hops %d" % (what, U), tags, seen,
              levels=U > 0)  # max_hops 0 runs no level
    with_path = np.array([r for r in rows if int(r) in case.paths], dtype=np.int64)
    if len(with_path):
        lists = [case.paths[int(r)] for r in with_path]
        twice(lambda: dev.shortestpath(g.rs[with_path], g.rd[with_path]), lists, what + ", shortestpath", g.tag[with_path], seen)


def run_configuration(case, words, what):
    """Every gadget row, in calls of one batch each (64 x words lanes) that all hold the decoy sources; the two-lane pairs also
    on their own (nothing else wanted: the early exits fire); a hub reached in one call and unreachable in the next; from 4 words on the call whose sources spread over four words."""
    g = case.g
    seen = Launches()
    for i, rows in enumerate(g.calls(words)):
        check_rows(case, rows, "%s, %s graph, call %d" % (what, case.config, i), seen)
    for rows in g.pairs:
        check_rows(case, np.array(rows, dtype=np.int64), "%s, %s graph, pair alone" % (what, case.config), seen, lengths_only=True)
    for rows in (g.stale["first"], g.stale["second"]):  # in this order: the second call asks for the hub the first one reached
        check_rows(case, np.array(rows, dtype=np.int64), "%s, %s graph, stale hub" % (what, case.config), seen, lengths_only=True)
    if words >= 4:
        check_rows(case, g.spread, "%s, %s graph, spread call" % (what, case.config), seen)
    print(what, case.config, {k: v for k, v in seen.n.items() if v})
    return seen.n


# (The other classes' counters need not be 0: a handle keeps the level plan of the last batch of a width, a configuration's first
# call enqueues the plan the configuration before left, and the device calls those levels off against the rule of the day.)
# One kernel per configuration; every configuration runs every family of both graphs.  The options of one kernel are paired, not
# crossed: each value of each option appears, the widths 1 .. 32 with every unroll, and the LDS map on and off at small and
# large widths.
# a. k_pull_lanes (lanes 1): lanes_unroll 1, 2, 4 (a trip = 64 x UN in-slots), the block map in LDS or not, all six widths
LANES = [(1, 1, 1), (2, 2, 0), (4, 4, 1), (8, 1, 0), (16, 2, 1), (32, 4, 0), (1, 4, 0), (8, 4, 1), (4, 2, 0)]


@pytest.mark.parametrize("words,unroll,lds", LANES)
def test_pull_lanes(case, words, unroll, lds):
    expansion(force_mode=2, force_pull=1, lanes=1, lanes_unroll=unroll, sparse_lds=lds, words=words)
    n = run_configuration(case, words, "k_pull_lanes, words %d, unroll %d, LDS map %d" % (words, unroll, lds))
    assert n["pull_sparse"] > 0 and n["pull_hub"] > 0, n


# b. k_pull_sparse (lanes 0): its six (unroll, words per trip) instantiations, the bit map in LDS or not, the spill queue off (0),
#    on, and on with a threshold no trip reaches (99: the same path, the option is only tested against 0)
SPARSE = [(1, 4, 1, 1, 3), (2, 2, 1, 0, 3), (4, 4, 2, 1, 0), (4, 1, 2, 0, 1), (8, 4, 3, 0, 99), (8, 2, 2, 1, 0), (16, 1, 2, 1, 1),
          (32, 4, 1, 0, 99), (4, 2, 1, 1, 99), (16, 4, 3, 1, 0)]


@pytest.mark.parametrize("words,unroll,pw,lds,spill", SPARSE)
def test_pull_sparse(case, words, unroll, pw, lds, spill):
    expansion(force_mode=2, force_pull=1, lanes=0, sparse_unroll=unroll, sparse_pw=pw, sparse_lds=lds, sparse_spill=spill, words=words)
    n = run_configuration(case, words, "k_pull_sparse, words %d, unroll %d, pw %d, LDS map %d, spill %d" % (words, unroll, pw, lds, spill))
    assert n["pull_sparse"] > 0 and n["pull_hub"] > 0, n


# c. k_pull: NS = 64 / words in-neighbours per gather, the GRP loop breaks at r0 x NS entries of the last chunk (words 16, 32)
@pytest.mark.parametrize("words", [1, 2, 4, 8, 16, 32])
def test_pull_dense(case, words):
    expansion(force_mode=2, force_pull=2, words=words)
    n = run_configuration(case, words, "k_pull, words %d" % words)
    assert n["pull"] > 0 and n["pull_hub"] > 0, n


# d. k_push: items of push_chunk out-edges (64, the smallest; the default once), the queue rebuilt from nz before every level
@pytest.mark.parametrize("words,chunk", [(1, 64), (4, 64), (32, 64), (8, PULL_LIMITS["push_chunk"])])
def test_push(case, words, chunk):
    expansion(force_mode=1, push_chunk=chunk, words=words)
    n = run_configuration(case, words, "k_push, words %d, push_chunk %d" % (words, chunk))
    assert n["push"] > 0 and n["queue"] > 0, n


# e. the host's own choice: the first levels' frontiers (the decoy sources' out-edges) are bottom-up, the fifth level's handful
#    of vertices top-down: k_queue_from_dense rebuilds the queue from a bottom-up level's nz.  push_div 4 flips between them.
@pytest.mark.parametrize("words", [1, 8])
def test_pull_then_push(case, words):
    expansion(force_mode=0, push_div=4.0, push_chunk=64, words=words)
    n = run_configuration(case, words, "adaptive, words %d" % words)
    assert n["push"] > 0 and n["pull"] + n["pull_sparse"] > 0 and n["pull_hub"] > 0, n


# ---- the partition itself -------------------------------------------------------------------------------------------------
def check_layout(dev, V, part_weight, hub_chunk, what):
    """pull_layout() against the contract, entry for entry: roff and radj from a stable sort of the downloaded CSR."""
    off, adj, _, _ = dev.download()
    src = np.repeat(np.arange(V, dtype=np.int64), np.diff(off))
    order = np.argsort(adj, kind="stable")  # by destination; the forward CSR is in (source id, slot) order already
    radj = src[order]
    roff = np.concatenate([[0], np.cumsum(np.bincount(adj, minlength=V))]).astype(np.int64)
    lay = dev.pull_layout()
    parts, hubs = pull_parts_model(roff, part_weight, hub_chunk)
    assert lay["parts"].shape == parts.shape and (lay["parts"] == parts).all(), what
    assert (lay["hub_vertices"] == hubs).all() and len(lay["hub_vertices"]) == len(hubs), what
    slices = hub_slices_model(roff, hubs, hub_chunk)
    assert lay["hub_items"].shape == slices.shape and (lay["hub_items"] == slices).all(), what
    S = max(64, max(64, hub_chunk) // PULL_LIMITS["hub_slice_div"])
    assert len(slices) == 0 or (slices[:, 2] - slices[:, 1]).max() <= S
    for v in hubs:  # the slices of a hub tile its in-list in order
        mine = lay["hub_items"][lay["hub_items"][:, 0] == v]
        assert mine[0, 1] == roff[v] and mine[-1, 2] == roff[v + 1] and (mine[1:, 1] == mine[:-1, 2]).all(), (what, v)
    # every vertex that is no hub lies in exactly one part, a hub in none
    cover = np.zeros(V + 1, dtype=np.int64)
    np.add.at(cover, lay["parts"][:, 0], 1)
    np.add.at(cover, lay["parts"][:, 1], -1)
    cover = np.cumsum(cover)[:V]
    is_hub = np.zeros(V, dtype=bool)
    is_hub[hubs] = True
    assert (cover[~is_hub] == 1).all() and (cover[is_hub] == 0).all(), what
    assert (np.diff(lay["parts"], axis=1) <= PULL_LIMITS["part_vertices"]).all() and (np.diff(lay["parts"], axis=1) >= 1).all()
    # rown[e] = owner - v0 for every in-slot of a part, 0 for a hub's slots; rpk = radj | rown << 28 for every in-slot of a part
    v0_of = np.zeros(V, dtype=np.int64)
    for a, b in lay["parts"]:
        v0_of[a:b] = a
    owner = np.repeat(np.arange(V, dtype=np.int64), np.diff(roff))
    rown = np.where(is_hub[owner], 0, owner - v0_of[owner])
    assert rown.max() <= 15
    assert (lay["rown"] == rown).all(), what
    # (a hub's slots are never read through rpk: the upload leaves them 0)
    rpk = np.where(is_hub[owner], 0, radj.astype(np.uint32) | (rown.astype(np.uint32) << np.uint32(28))).astype(np.uint32)
    assert lay["rpk"] is not None and (lay["rpk"] == rpk).all(), what
    return lay


def test_partition_of_the_gadget_graph(case):
    g = case.g
    lay = check_layout(case.dev, g.V, g.part_weight, g.hub_chunk, case.config)
    assert len(lay["hub_vertices"]) >= 10 and lay["parts"][-1, 1] == g.V
    if case.config == "defaults":
        assert lay["rown"].max() == 15


@pytest.mark.parametrize("part_weight,hub_chunk", [(64, 64), (200, 300), (1024, 4096), (1, 1)])
def test_partition_of_a_skewed_graph(part_weight, hub_chunk):
    V, s, d = graphgen.rmat(13, seed=5)
    st, dev = upload(V, s, d, part_weight, hub_chunk)
    try:
        lay = check_layout(dev, V, part_weight, hub_chunk, (part_weight, hub_chunk))
        assert len(lay["parts"]) > V // 16 and (hub_chunk > 300 or len(lay["hub_vertices"]) > 0)
    finally:
        st.delete_csr(0)
