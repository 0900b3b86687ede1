"""k_bibfs (pgq_meet.hip) and its list walk (pgq_walk.h: meet_walk_chunks) restated in plain Python, decision by decision.

solve() answers rows the way the kernel does: k_bidir_classify's shortcuts, then per open row the bound test, the side rule, the
cap test, one expansion, and found before empty before queue overflow.  An expansion walks the frontier queue in the kernel's
structure: 16 wavefronts, wavefront w takes the queue positions w + 16 * lane, 1024 positions per pass, cnt = min(64, ceil((n -
pb) / 16)) lists per wavefront and pass, every list in chunks of 256 entries from b & ~3 with head and tail masked, empty lists
skipped.  With `grid` and `gm` it carries the two visited maps and the touched-word list from row i to row i + grid as the
global-map variant does: a row clears the words the row before listed, or the whole map when the list overflowed or the
workgroup has not run a row yet.

The queue's fill order is decided by atomics on the device; here it is the order of discovery.  Nothing a test takes from
this model may depend on that order (helpers.bibfs_gadgets gives every position and slot a row of its own instead).

MUTANTS names one wrong decision each; solve(..., mutant=name) takes it.  test_bibfs_gadgets_cpu.py holds the model to the
oracle's BFS and shows which gadget family tells each mutant from the kernel's rule."""
from collections import namedtuple

import numpy as np

NULL, OPEN = -1, -2
WAVES, LANES, CHUNK, DEPTH = 16, 64, 256, 2  # PGQ_BIBFS_DEPTH chunks are requested before the first one is used
PASS = WAVES * LANES                         # queue positions per pass of the workgroup

MUTANTS = {
    "cap_ge": "a side whose work EQUALS bibfs_cap leaves the row open",
    "queue_ge": "a level of exactly qcap new vertices leaves the row open",
    "queue_drop_last": "slot qcap - 1 of the next frontier is not stored",
    "second_pass_lost": "queue positions from 1024 on are not walked",
    "cnt_floor": "cnt rounded down: the last positions of a pass are lost",
    "head_unmasked": "entries in [b & ~3, b) count",
    "tail_unmasked": "entries in [e, chunk end) count",
    "second_chunk_lost": "the second chunk a wavefront requests in a pass is dropped",
    "third_chunk_lost": "the refill after DEPTH chunks is dropped",
    "empty_list_stops": "an empty list ends the wavefront's pass instead of being skipped",
    "bound_after_cap": "the cap test stands in front of the bound test",
    "bound_ge_plus_1": "the bound closes a row at a + b >= bound + 1",
    "tie_backward": "equal work expands the backward side",
    "stale_own": "the listed words of the forward map are not cleared",
    "stale_other": "the listed words of the backward map are not cleared",
    "overflow_list_clear": "an overflowed list clears its qcap stored words only",
    "first_row_trusts_map": "a workgroup's first row clears nothing",
}

# answer: hops, NULL or OPEN; sides: the sides expanded, in order (0 forward, 1 backward); entries: adjacency entries the
# expansions covered; levels: per expansion (side, frontier vertices, work, new vertices, adjacency indices that met the other
# side); listed: words on the touched list when the row ended (gm only, else 0)
Row = namedtuple("Row", "answer sides entries levels listed")


class Graph:
    """Forward lists in table order, backward lists by (source, slot): the upload's layouts."""

    def __init__(self, V, src, dst):
        src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
        self.V, self.E = int(V), len(src)
        order = np.argsort(src, kind="stable")
        adj = dst[order]
        back = np.argsort(adj, kind="stable")
        self.xadj = (adj, src[order][back])
        self.xoff = tuple(np.concatenate([[0], np.cumsum(np.bincount(k, minlength=V))]).astype(np.int64) for k in (src, dst))
        self.bm_words = (self.V + 127) // 128 * 4  # MapPlan: words of one map; four spare words behind it
        self.mw = self.bm_words + 4


def walk(g, side, cur, mutant=None):
    """meet_walk_chunks over the queue `cur`: (adjacency indices covered, any lane masked)."""
    xoff, E = g.xoff[side], g.E
    nf = len(cur)
    p = np.arange(nf, dtype=np.int64)
    w, lane, k = p % WAVES, p // WAVES % LANES, p // PASS
    pb = w + PASS * k
    cnt = np.minimum(LANES, (nf - pb) // WAVES if mutant == "cnt_floor" else (nf - pb + WAVES - 1) // WAVES)
    walked = lane < cnt
    if mutant == "second_pass_lost":
        walked &= k == 0
    b, e = xoff[cur], xoff[cur + 1]
    stream = k * WAVES + w  # one wavefront's pass: its lists are sought in lane order, their chunks requested back to back
    if mutant == "empty_list_stops":
        first = np.full(int(stream.max()) + 1 if nf else 1, LANES, dtype=np.int64)
        empty = walked & (e == b)
        np.minimum.at(first, stream[empty], lane[empty])
        walked &= lane < first[stream]
    sel = np.flatnonzero(walked & (e > b))
    if mutant in ("second_chunk_lost", "third_chunk_lost"):
        sel = sel[np.lexsort((lane[sel], stream[sel]))]
    vb, ve = b[sel], e[sel]
    q0 = vb & ~3
    nch = (ve - q0 + CHUNK - 1) // CHUNK
    first_chunk = np.cumsum(nch) - nch
    rep = np.repeat(np.arange(len(sel)), nch)
    ci = np.arange(int(nch.sum())) - first_chunk[rep]
    q = q0[rep] + CHUNK * ci
    lo, hi = np.maximum(vb[rep], q), np.minimum(ve[rep], q + CHUNK)
    masked = bool(((lo > q) | (hi < q + CHUNK)).any())
    if mutant == "head_unmasked":
        lo = q
    if mutant == "tail_unmasked":
        hi = np.minimum(q + CHUNK, E)  # past the adjacency: padding, no vertex
    if mutant in ("second_chunk_lost", "third_chunk_lost"):
        st = stream[sel][rep]
        pos = np.arange(len(st))
        start = np.full(int(st.max()) + 1 if len(st) else 1, len(st), dtype=np.int64)
        np.minimum.at(start, st, pos)  # the stream's first chunk: its chunks stand side by side, in request order
        keep = pos - start[st] != (1 if mutant == "second_chunk_lost" else DEPTH)
        lo, hi = lo[keep], hi[keep]
    n = hi - lo
    idx = np.repeat(lo - (np.cumsum(n) - n), n) + np.arange(int(n.sum()))
    return idx, masked


class Maps:
    """One workgroup's two maps and its touched-word list."""

    def __init__(self, g, gm):
        self.g, self.gm = g, gm
        self.m = np.full((2, g.mw), 0xFFFFFFFF if gm else 0, dtype=np.uint32)  # global maps arrive with whatever was there
        self.tn, self.tl = None, []  # tn None: no row yet (s_tn = ~0u)

    def clear(self, qcap, mutant):
        g = self.g
        if not self.gm:
            self.m[:] = 0
            return
        if self.tn is None:
            if mutant != "first_row_trusts_map":
                self.m[:] = 0
        elif self.tn > qcap and mutant != "overflow_list_clear":
            self.m[:] = 0
        else:
            t = np.asarray(self.tl[:qcap], dtype=np.int64)
            if mutant == "stale_own":
                t = t[t >= g.mw]
            if mutant == "stale_other":
                t = t[t < g.mw]
            self.m.reshape(-1)[t] = 0
        self.tn, self.tl = 0, []

    def touch(self, side, words):
        if self.gm:
            self.tn += len(words)
            self.tl.extend((side * self.g.mw + words).tolist())


def search(g, s, d, cap, qcap, bound, maps, mutant=None):
    """One open row: src != dst, src has out-edges, dst has in-edges."""
    maps.clear(qcap, mutant)
    m = maps.m
    for side, v in ((0, s), (1, d)):
        m[side, v >> 5] |= np.uint32(1 << (v & 31))
    if maps.gm:  # listed whatever they held
        maps.tn, maps.tl = 2, [s >> 5, g.mw + (d >> 5)]
    front = [np.array([s], dtype=np.int64), np.array([d], dtype=np.int64)]
    lvl = [0, 0]
    work = [int(g.xoff[0][s + 1] - g.xoff[0][s]), int(g.xoff[1][d + 1] - g.xoff[1][d])]
    answer, sides, entries, levels = OPEN, [], 0, []
    over = (lambda x: x >= cap) if mutant == "cap_ge" else (lambda x: x > cap)
    while True:
        if mutant == "bound_after_cap" and over(min(work)):
            break
        if bound is not None and lvl[0] + lvl[1] >= bound + (mutant == "bound_ge_plus_1"):
            answer = NULL
            break
        side = 0 if (work[0] < work[1] if mutant == "tie_backward" else work[0] <= work[1]) else 1
        if over(work[side]):
            break
        idx, masked = walk(g, side, front[side], mutant)
        xs = g.xadj[side][idx]
        wd, bit = xs >> 5, np.uint32(1) << (xs & 31).astype(np.uint32)
        own, oth = m[side], m[side ^ 1]
        hits = idx[(oth[wd] & bit) != 0]
        cand = xs[(own[wd] & bit) == 0]
        _, at = np.unique(cand, return_index=True)
        new = cand[np.sort(at)]
        zero = np.unique(wd[own[wd] == 0])
        if masked and own[g.bm_words] == 0:  # the masked lanes' bit: bit 0 of the first spare word (every chunk has such lanes: early)
            zero = np.append(g.bm_words, zero)
        maps.touch(side, zero)
        np.bitwise_or.at(own, wd, bit)
        if masked:
            own[g.bm_words] |= np.uint32(1)
        sides.append(side)
        entries += len(idx)
        levels.append((side, len(front[side]), work[side], len(new), hits))
        if len(hits):
            answer = lvl[0] + lvl[1] + 1
            break
        if len(new) == 0:
            answer = NULL
            break
        if len(new) >= qcap if mutant == "queue_ge" else len(new) > qcap:
            break
        if mutant == "queue_drop_last" and len(new) >= qcap:
            new = np.delete(new, qcap - 1)
        front[side] = new
        work[side] = int((g.xoff[side][new + 1] - g.xoff[side][new]).sum())
        lvl[side] += 1
    return Row(answer, tuple(sides), entries, levels, maps.tn if maps.gm else 0)


def solve(g, rows, cap, qcap, bound=None, grid=None, gm=False, mutant=None):
    """rows: (src, dst) arrays.  One Row per row.  grid: open row i runs on workgroup i mod grid, behind row i - grid."""
    rs, rd = (np.asarray(a, dtype=np.int64) for a in rows)
    fresh = grid is None
    wgs = {}
    out, i = [], 0
    for s, d in zip(rs.tolist(), rd.tolist()):
        if s < 0:  # a NULL row
            out.append(Row(NULL, (), 0, [], 0))
        elif s == d:
            out.append(Row(0, (), 0, [], 0))
        elif g.xoff[0][s + 1] == g.xoff[0][s] or g.xoff[1][d + 1] == g.xoff[1][d]:  # k_bidir_classify: no path can exist
            out.append(Row(NULL, (), 0, [], 0))
        else:
            k = 0 if fresh else i % grid
            if k not in wgs:
                wgs[k] = Maps(g, gm)
            out.append(search(g, s, d, cap, qcap, bound, wgs[k], mutant))
            i += 1
    return out


def bibfs_model(off, adj, roff, radj, s, d):
    """The side rule and the termination tests alone, on CSR arrays: a distance or None (test_schedule_models_cpu.py)."""
    g = Graph.__new__(Graph)
    g.V, g.E = len(off) - 1, len(adj)
    g.xoff, g.xadj = (np.asarray(off, dtype=np.int64), np.asarray(roff, dtype=np.int64)), (np.asarray(adj), np.asarray(radj))
    g.bm_words = (g.V + 127) // 128 * 4
    g.mw = g.bm_words + 4
    if s == d:
        return 0
    if off[s + 1] == off[s] or roff[d + 1] == roff[d]:
        return None
    r = search(g, int(s), int(d), 1 << 60, 1 << 60, None, Maps(g, False))
    return None if r.answer == NULL else r.answer
