"""helpers.degree_gadgets(**WEIGHTED_GADGETS) with helpers.weighted_gadgets' weights is what test_weighted_gadgets_gpu.py
assumes: checked here with numpy and the CPU oracle alone.

The list lengths sit on the constants of the cheapest-path relaxation (pgq_cheapest.hip): eight edges per trip of k_relax, a
heavy pass in chunks of 64 edges for lists of more than 128, a chunk map filled 64 chunks per trip of a loop (4097 edges are
the first list of 65 chunks), caps that double per phase over weight-sorted lists.  For the graph and its transpose and for
every weight scheme: the endpoint degrees and the slot of the path vertex are read back from the CSR arrays, its rank from a
model of the weight sort; the oracle's answer is the left fold of the path's weights; every (degree, position, k) cell that
fits exists; int64 witness weights of 2^j and 2^j + 1 exist for j = 3, 6, 7, 12; 4-byte labels and the shipped light rule
are taken.

A single-lane model of k_relax's list walk (trips of eight with their padding, the stop rule under a cap, the heavy split with
its chunk skip and 129th-edge rule, the doubling cap, the re-queueing of touched vertices) equals the oracle on every gadget
row; five mutants of it — the mistakes a kernel of this shape makes — each change a gadget row's answer.  That is the evidence
that the GPU file would catch such a kernel, obtained without running a wrong kernel."""
import numpy as np
import pytest

from helpers import (WEIGHT_DTYPES, WEIGHT_SCHEMES, WEIGHTED_GADGETS, csr_arrays_from_rows, degree_gadgets, gadget_index,
                     weight_sort_keys, weighted_gadgets)
from oracle.pgq_oracle import OracleCSR

ORIENT = ("graph", "transpose")


class Built:
    def __init__(self, g):
        self.g = g
        self.off, self.adj, self.order = csr_arrays_from_rows(g.V, g.src, g.dst)
        self.deg = np.diff(self.off)
        self.owner = np.repeat(np.arange(g.V, dtype=np.int64), self.deg)  # the source of every slot
        # rows by source, one lane each (like a batch of the relaxation: a lane is a distinct source with all its destinations)
        by = np.argsort(g.rs, kind="stable")
        cut = np.flatnonzero(np.diff(g.rs[by])) + 1
        self.lanes = [(int(g.rs[r[0]]), r) for r in np.split(by, cut)]
        self._w, self._want = {}, {}

    def out_list(self, v):
        return self.adj[self.off[v]:self.off[v + 1]]

    def weights(self, scheme, dtype="int64"):
        """In slot order (the CSR's w array)."""
        if (scheme, dtype) not in self._w:
            self._w[scheme, dtype] = weighted_gadgets(self.g, scheme, dtype)[self.order]
        return self._w[scheme, dtype]

    def oracle(self, scheme, dtype="int64"):
        if (scheme, dtype) not in self._want:
            ora = OracleCSR.adopt(self.g.V, self.off, self.adj, np.arange(len(self.adj), dtype=np.int64), self.weights(scheme, dtype))
            self._want[scheme, dtype] = ora.lean_cheapest_path_length(self.g.V, self.g.rs, self.g.rd)
        return self._want[scheme, dtype]

    def sorted_lists(self, w):
        """ensure_weight_sorted: every list stably sorted by its weights' keys.  Returns the permutation of the slots."""
        return np.lexsort((weight_sort_keys(w), self.owner))

    def edge_weight(self, w, u, v):
        k = self.off[u] + int(np.flatnonzero(self.out_list(u) == v)[0])
        return w[k]


@pytest.fixture(scope="module")
def both():
    g = degree_gadgets(**WEIGHTED_GADGETS)
    return [Built(g), Built(g.transposed())]


def test_sizes_label_width_and_light_rule(both):
    g = both[0].g
    assert (g.V, len(g.src), len(g.gadgets), len(g.rs), len(both[0].lanes)) == (13_638, 1_310_422, 776, 2_904, 1_553)
    assert (g.dist >= 0).sum() == 2_128
    assert g.src.min() >= 0 and g.dst.min() >= 0 and g.src.max() < g.V and g.dst.max() < g.V
    assert len(set(g.tag.tolist())) == len(g.tag), "tags name one row each"
    assert (g.rs != g.rd).all(), "every row needs a search"
    for b in both:
        assert len(b.lanes) == 1_553
        for scheme in WEIGHT_SCHEMES:
            w = b.weights(scheme)
            assert w.min() >= 0 and int(w.max()) * g.V < 2147483000, "4-byte labels are taken (labels_fit_32)"
    assert len(g.src) >= 16 * g.V, "relax_light = 1 picks the light-edges-first path (light_edges_first)"


def test_degrees_and_slots(both):
    for b in both:
        roff, radj, _ = csr_arrays_from_rows(b.g.V, b.g.dst, b.g.src)
        for x in b.g.gadgets:
            out = b.out_list(x["src"])
            assert len(out) == x["a"] and roff[x["dst"] + 1] - roff[x["dst"]] == x["b"], x["tag"]
            if x["tie"]:
                slots = [int(np.flatnonzero(out == p[1])[0]) for p in x["paths"]]
                want = [0, x["a"] - 1] if len(slots) == 2 else [0, x["a"] // 2, x["a"] - 1]
                assert sorted(slots) == want, x["tag"]
                continue
            (path,) = x["paths"]
            assert len(path) == x["k"] + 1
            assert out[gadget_index(x["pos"], x["a"])] == path[1] and (out == path[1]).sum() == 1, x["tag"]
            for u, v in zip(path[:-1], path[1:]):
                assert (b.out_list(u) == v).sum() == 1, x["tag"]


@pytest.mark.parametrize("dtype", WEIGHT_DTYPES)
@pytest.mark.parametrize("scheme", WEIGHT_SCHEMES)
def test_rank_in_weight_sorted_order(both, scheme, dtype):
    for b in both:
        w = b.weights(scheme, dtype)
        perm = b.sorted_lists(w)
        rank = np.empty(len(perm), dtype=np.int64)
        rank[perm] = np.arange(len(perm)) - b.off[b.owner[perm]]
        slot = np.arange(len(perm)) - b.off[b.owner]
        assert (np.diff(weight_sort_keys(w[perm]).view(np.int64))[np.diff(b.owner[perm]) == 0] >= 0).all()
        if scheme in ("ascending", "zeros"):
            assert (rank == slot).all()
        elif scheme == "descending":
            assert (rank == b.deg[b.owner] - 1 - slot).all()
        for x in b.g.gadgets:
            s, n = x["src"], x["a"]
            ranks = sorted(int(rank[b.off[s] + int(np.flatnonzero(b.out_list(s) == p[1])[0])]) for p in x["paths"])
            if x["tie"]:
                if scheme == "witness_heaviest":  # the path edges behind every decoy edge
                    assert ranks == list(range(n - len(ranks), n)), x["tag"]
                else:
                    assert ranks == ([0, n - 1] if len(ranks) == 2 else [0, n // 2 if scheme != "descending" else n - 1 - n // 2, n - 1]), x["tag"]
                continue
            i = gadget_index(x["pos"], n)
            assert ranks == [{"ascending": i, "zeros": i, "descending": n - 1 - i, "witness_heaviest": n - 1}[scheme]], x["tag"]


def fold(b, w, path):
    acc = w.dtype.type(0)
    for u, v in zip(path[:-1], path[1:]):
        acc = acc + b.edge_weight(w, u, v)  # left to right, like dist[v] + w
    return acc


@pytest.mark.parametrize("dtype", WEIGHT_DTYPES)
@pytest.mark.parametrize("scheme", WEIGHT_SCHEMES)
def test_oracle_answer_is_the_left_fold_of_the_path(both, scheme, dtype):
    for b in both:
        g = b.g
        w = b.weights(scheme, dtype)
        out, ok = b.oracle(scheme, dtype)
        assert (ok == (g.dist >= 0)).all(), "exactly the builder's reachable rows"
        for x in g.gadgets:
            costs = [fold(b, w, p) for p in x["paths"]]
            got = out[x["row"]]
            assert ok[x["row"]], x["tag"]
            if x["tie"] and scheme in ("ascending", "descending"):
                win = 0 if scheme == "ascending" else len(costs) - 1  # the paths are listed in slot order
                assert all(costs[win] < c for i, c in enumerate(costs) if i != win), (x["tag"], costs)
                want = costs[win]
            else:
                want = min(costs)
            assert np.asarray(got).tobytes() == np.asarray(want).tobytes(), (x["tag"], got, want)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_every_degree_position_cell_exists(both, k):
    for b in both:
        plain = [x for x in b.g.gadgets if x["k"] == k and not x["tie"]]
        have_a = {(x["a"], gadget_index(x["pos"], x["a"])) for x in plain}
        have_b = {(x["b"], gadget_index(x["pos"], x["b"])) for x in plain}
        for n in WEIGHTED_GADGETS["degrees"]:
            for pos in WEIGHTED_GADGETS["positions"]:
                i = gadget_index(pos, n)
                if i is not None:
                    assert (n, i) in have_a and (n, i) in have_b, (k, n, pos)
        pairs = {(x["a"], x["b"]) for x in b.g.gadgets if x["k"] == k}
        for n in WEIGHTED_GADGETS["degrees"]:
            assert {(n, n), (n, 1), (1, n)} <= pairs, (k, n)
        assert (129, 4097) in pairs or (4097, 129) in pairs
    ties = {(x["k"], len(x["paths"]), x["a"]) for x in both[0].g.gadgets if x["tie"]}
    assert ties == {(kk, n, d) for kk in (2, 3, 4) for n in (2, 3) for d in WEIGHTED_GADGETS["tie_degrees"]}


def test_witness_weights_on_both_sides_of_every_power_of_two_boundary(both):
    # trip (8), chunk (64), heavy list (128) and chunk-map trip (4096): a witness edge of weight 2^j and one of 2^j + 1
    for b in both:
        w = b.weights("ascending")
        first = {int(b.edge_weight(w, p[0], p[1])) for x in b.g.gadgets for p in x["paths"]}
        for j in (3, 6, 7, 12):
            assert {1 << j, (1 << j) + 1} <= first, (j, sorted(first))


# ---- a single-lane model of k_relax's list walk -----------------------------------------------------------------------------

MUTANTS = ("drop_eighth_edge", "drop_single_edge_last_chunk", "drop_chunk_64", "stop_at_the_cap", "unsorted_weights")


class RelaxModel:
    """One lane (a source and its destinations) under RelaxBatches' schedule, on one label array that is reset through the list
    of touched vertices.  A round expands every queued vertex whose label is under the lane's bound (the largest tentative label
    among its destinations, INF while one is unlabelled): a list of more than 128 edges — over sorted lists: whose 129th
    edge is not above the cap — is set aside and walked in chunks of 64 behind the others, from the label it has by then; a
    chunk whose first edge is above the cap is skipped.  A walk takes trips of eight entries, the last one padded with
    (v, weight 0); over sorted lists it ends at the first edge above the cap or whose candidate does not get under the
    bound.  Improved vertices form the next queue.  At a phase's fixpoint the search is over when the cap has reached the
    largest weight or the bound; else the cap doubles and every touched vertex is queued again.  The vertices of a round
    read the labels the round started with, one of the orders the kernel's concurrent wavefronts may take.

    Mutants: drop_eighth_edge (a trip's last entry never counts), drop_single_edge_last_chunk (the chunk count rounds a
    remainder of one edge down), drop_chunk_64 (the chunk map's loop makes one trip), unsorted_weights (the sorted
    neighbours paired with the weights in table order), stop_at_the_cap (an edge AT the cap is taken for one above it; alone
    that only delays the edge by a phase, so with it the phases end as soon as the cap reaches the largest label among the
    destinations labelled so far, the bound as measured before the doubling, without waiting for the unlabelled ones)."""

    def __init__(self, b, w, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.off, self.mutant = b.off, mutant
        perm = b.sorted_lists(w)
        self.plain = (b.adj, w)
        self.light = (b.adj[perm], w if mutant == "unsorted_weights" else w[perm])
        self.w_max = w[np.argmax(weight_sort_keys(w))]
        self.inf = np.iinfo(np.int64).max // 2 if w.dtype.kind == "i" else np.finfo(np.float64).max / 2
        self.dist = np.full(len(b.off) - 1, self.inf, dtype=w.dtype)
        self.seen = np.zeros(len(b.off) - 1, dtype=bool)
        self.phases = 0

    def over(self, ww, cap):
        return ww >= cap if self.mutant == "stop_at_the_cap" else ww > cap

    def walk(self, vs, dvs, bs, es, lists, is_sorted, cap, bound):
        adj, w = lists
        npad = (es - bs + 7) // 8 * 8
        tot = int(npad.sum())
        if tot == 0:
            return np.zeros(0, dtype=np.int64)
        seg = np.repeat(np.arange(len(vs)), npad)
        pos = np.arange(tot) - np.repeat(np.cumsum(npad) - npad, npad)
        idx = bs[seg] + pos
        inside = idx < es[seg]
        at = np.where(inside, idx, 0)
        nn = np.where(inside, adj[at], vs[seg])           # the padding: the vertex itself ...
        ww = np.where(inside, w[at], w.dtype.type(0))     # ... at weight 0, which never improves it
        cand = dvs[seg] + ww
        counted = inside.copy()
        if is_sorted:
            stop = inside & (self.over(ww, cap) | ~(cand < bound))
            first = np.full(len(vs), tot, dtype=np.int64)
            np.minimum.at(first, seg[stop], pos[stop])
            counted &= pos < first[seg]
        if self.mutant == "drop_eighth_edge":
            counted &= pos % 8 != 7
        go = counted & (cand < self.dist[nn])
        np.minimum.at(self.dist, nn[go], cand[go])
        return nn[go]

    def round(self, q, is_sorted, split, cap, bound):
        lists = self.light if is_sorted else self.plain
        dv = self.dist[q]
        live = dv < bound
        q, dv = q[live], dv[live]
        b, e = self.off[q], self.off[q + 1]
        heavy = np.zeros(len(q), dtype=bool)
        if split:
            heavy = e - b > 128
            if is_sorted:
                heavy &= ~self.over(lists[1][np.where(heavy, b + 128, 0)], cap)
        improved = [self.walk(q[~heavy], dv[~heavy], b[~heavy], e[~heavy], lists, is_sorted, cap, bound)]
        if heavy.any():
            hq, hb, he = q[heavy], b[heavy], e[heavy]
            nch = (he - hb + (62 if self.mutant == "drop_single_edge_last_chunk" else 63)) // 64
            seg = np.repeat(np.arange(len(hq)), nch)
            c = np.arange(int(nch.sum())) - np.repeat(np.cumsum(nch) - nch, nch)
            cb = hb[seg] + 64 * c
            ce = np.minimum(cb + 64, he[seg])
            keep = np.ones(len(c), dtype=bool)
            if self.mutant == "drop_chunk_64":
                keep &= c < 64
            if is_sorted:
                keep &= ~self.over(lists[1][cb], cap)
            vs = hq[seg][keep]
            improved.append(self.walk(vs, self.dist[vs], cb[keep], ce[keep], lists, is_sorted, cap, bound))
        return np.unique(np.concatenate(improved))

    def bound(self, dests):
        return self.dist[dests].max()  # INF while one of them is unlabelled

    def run(self, src, dests, light, split=True, cap0=1):
        dist, seen = self.dist, self.seen
        dist[src] = 0
        seen[src] = True
        touched = [np.array([src], dtype=np.int64)]
        q = touched[0]
        cap = dist.dtype.type(cap0)
        while True:
            self.phases += 1
            while len(q):
                q = self.round(q, light, split, cap, self.bound(dests))
                new = q[~seen[q]]
                seen[new] = True
                touched.append(new)
            if not light:
                break
            bound = self.bound(dests)
            if self.mutant == "stop_at_the_cap":
                lab = dist[dests][dist[dests] < self.inf]
                bound = lab.max() if len(lab) else bound
            if not cap < self.w_max or not cap < bound:
                break
            cap = cap + cap
            q = np.concatenate(touched)
        out = dist[dests].copy()
        t = np.concatenate(touched)
        dist[t] = self.inf
        seen[t] = False
        return out


def model_answers(b, w, light, mutant=None, lanes=None, split=True):
    """(row indices, labels) of the lanes' rows under the model."""
    m = RelaxModel(b, w, mutant)
    rows, labels = [], []
    for src, r in (b.lanes if lanes is None else lanes):
        rows.append(r)
        labels.append(m.run(src, b.g.rd[r], light, split))
    return np.concatenate(rows), np.concatenate(labels), m


def differing(b, scheme, dtype, rows, labels, inf):
    out, ok = b.oracle(scheme, dtype)
    want = np.where(ok[rows], out[rows], inf)
    return rows[labels.view(np.int64) != want.astype(labels.dtype).view(np.int64)]


# (scheme, dtype, light, orientations): plain and light on both orientations with the ascending int64 weights, whose ranks are
# the slots; the transpose once more where the sort reverses every list; the other schemes and the doubles on the graph
EQUAL = [("ascending", "int64", False, (0, 1)), ("ascending", "int64", True, (0, 1)), ("descending", "int64", True, (1,)),
         ("witness_heaviest", "int64", True, (0,)), ("zeros", "int64", True, (0,)), ("ascending", "double_inexact", False, (0,)),
         ("descending", "double_inexact", True, (0,)), ("zeros", "double", True, (1,))]


@pytest.mark.parametrize("scheme,dtype,light,orientations", EQUAL, ids=["%s-%s-%s" % (s, d, "light" if l else "plain") for s, d, l, _ in EQUAL])
def test_model_equals_the_oracle_on_every_row(both, scheme, dtype, light, orientations):
    for k in orientations:
        b = both[k]
        rows, labels, m = model_answers(b, b.weights(scheme, dtype), light)
        assert sorted(rows.tolist()) == list(range(len(b.g.rs))), "no row is left out"
        bad = differing(b, scheme, dtype, rows, labels, m.inf)
        assert len(bad) == 0, (ORIENT[k], len(bad), b.g.tag[bad[0]])
        if light and scheme == "ascending":  # caps 1, 2, 4, ... up to the lane's bound: more phases than lanes
            assert m.phases > 4 * len(b.lanes)


def lanes_of(b, pick):
    srcs = {x["src"] for x in b.g.gadgets if pick(x)}
    return [(s, r) for s, r in b.lanes if s in srcs]


# (mutant, scheme, light, the gadgets whose lanes are run: the ones the mutant should get wrong and their neighbours in degree)
KILLS = [("drop_eighth_edge", "ascending", False, lambda x: x["a"] in (7, 8, 9, 15, 16, 17)),
         ("drop_eighth_edge", "ascending", True, lambda x: x["a"] in (7, 8, 9, 15, 16, 17)),
         ("drop_single_edge_last_chunk", "ascending", False, lambda x: x["a"] in (128, 129, 130, 192, 193)),
         ("drop_single_edge_last_chunk", "descending", True, lambda x: x["a"] in (128, 129, 130, 192, 193)),
         ("drop_chunk_64", "ascending", False, lambda x: x["a"] in (4096, 4097) and x["pos"] == "last"),
         ("drop_chunk_64", "witness_heaviest", True, lambda x: x["a"] in (4096, 4097) and x["pos"] == "last"),
         ("stop_at_the_cap", "ascending", True, lambda x: x["a"] in (63, 64, 65, 127, 128, 129)),
         ("unsorted_weights", "descending", True, lambda x: x["a"] in (2, 7, 8, 9))]


@pytest.mark.parametrize("mutant,scheme,light,pick", KILLS, ids=["%s-%s-%s" % (m, s, "light" if l else "plain") for m, s, l, _ in KILLS])
def test_every_mutant_changes_a_gadget_row(both, mutant, scheme, light, pick):
    for k, b in enumerate(both):
        lanes = lanes_of(b, pick)
        assert lanes
        w = b.weights(scheme)
        rows, labels, m = model_answers(b, w, light, None, lanes)
        assert len(differing(b, scheme, "int64", rows, labels, m.inf)) == 0
        rows, labels, m = model_answers(b, w, light, mutant, lanes)
        bad = differing(b, scheme, "int64", rows, labels, m.inf)
        print("%s, %s, %s, %s: %d of %d rows differ, first %s" % (mutant, scheme, "light" if light else "plain", ORIENT[k],
                                                                   len(bad), len(rows), b.g.tag[bad[0]] if len(bad) else None))
        assert len(bad) > 0, (mutant, ORIENT[k])


def test_the_heavy_split_changes_no_answer(both):
    b = both[0]
    lanes = lanes_of(b, lambda x: x["a"] in (128, 129, 192, 193, 4096, 4097) and x["pos"] == "last" and x["k"] == 2)
    w = b.weights("ascending")
    r1, l1, _ = model_answers(b, w, False, None, lanes, split=True)
    r0, l0, _ = model_answers(b, w, False, None, lanes, split=False)
    assert (r1 == r0).all() and (l1 == l0).all()
