"""What finish_upload and build_meet_layout (csrc/pgq_runtime.hip) derive from a CSR for the pair-centric and source-centric
kernels, restated in vectorised numpy: the contract of pgq_csr_meet_layout (include/pgq_hip.h), array by array.

    reverse CSR   roff / radj = the forward slots sorted stably by destination: in-lists ordered by (source, forward slot)
    seg[v]        (first group, len): first group = exclusive scan of ceil(len / align) x align / 4, align = max(4, meet_align) & ~3
    padded        every group of a list, its alignment groups included: position i holds adj[b + min(i, len - 1)]
    desc[e]       (u, seg[u].x, seg[u].y, first packed group of u in the same direction or 0 when K = 4), u = adj[e]
    work[v]       min(sum of len(adj[e]) over v's slots, 2^32 - 1)
    packed        pgq_pack.h: K = pack_k_for(V) ids of 128 / K bits per group, little-endian across the four words, lists of
                  pack_list_groups groups, positions past the end repeat the last entry; with meet_pack_order the entries of a
                  list in non-increasing pack_order_bucket of the OTHER direction's degree, stable
    rhead[v]      64 words: word 31 the count, words 0 .. 30 entries 0 .. 30, words 32 .. 63 entries 31 .. 62, positions past the
                  end repeat the last entry, all ones for an empty list; exists when ball is on and V x 256 <= ball_head_mb << 20
    scalars       max_in, max_out, two_hop_mean = float(sum of indeg x outdeg) / float(max(V, 1))

There is no Python loop over vertices or slots: the model runs at V = 2^21 (rhead is filled in blocks of vertices).

MUTANTS names one wrong decision each; layout(..., mutant=name) takes it.  A mutant changes the array its decision writes
and nothing derived from it, so that the array which tells it apart is the one a reader would look at.
test_layout_model_cpu.py shows which graph family tells each mutant from the contract."""
import numpy as np

U32_MAX = (1 << 32) - 1

MUTANTS = {
    "pad_first": "padding repeats the list's FIRST entry",
    "pad_zero": "padding is 0",
    "align_unfilled": "the groups that only align a list are left unfilled (all ones here)",
    "no_ceil": "the group count rounds len / align DOWN",
    "desc_own_seg": "a descriptor carries the seg of the slot's owner, not of the neighbour",
    "desc_other_scan": "a descriptor's fourth word comes from the other direction's packed scan",
    "work_wraps": "work wraps mod 2^32 instead of saturating",
    "work_counts_own": "work counts the vertex's own list too",
    "sort_unstable": "the reverse sort puts equal destinations in DEscending slot order",
    "roff_gap_late": "k_row_bounds leaves the rows of a gap of in-edge-less vertices at the START of the list before the gap",
    "rhead_count_32": "the count sits in word 32 (entries 0 .. 31 before it, 32 .. 62 behind it)",
    "rhead_unshifted": "words 32 .. 63 hold entries 32 .. 63: entry 31 is lost",
    "rhead_clamp_cnt": "rhead clamps an entry's index at cnt instead of cnt - 1",
    "k6_lt": "K = 6 is chosen for V < 2^21 instead of V <= 2^21",
    "pack_ties_id_desc": "equal buckets of a packed list are ordered by id, descending, not by slot",
}


def pack_k_for(V, with5, mutant=None):
    if (V < 1 << 21) if mutant == "k6_lt" else (V <= 1 << 21):
        return 6
    return 5 if with5 and V <= 1 << 25 else 4


def pack_list_groups(ln, K, align):
    per = K * align
    return (ln + per - 1) // per * align


def pack_order_bucket(ln):
    """floor(log2(max(len, 1))), exactly: frexp's exponent."""
    return np.frexp(np.maximum(np.asarray(ln, dtype=np.int64), 1).astype(np.float64))[1].astype(np.int64) - 1


def pack_put(ids, K):
    """ids [n, K] -> words [n, 4]: id k at bits k W .. k W + W - 1 of the 128-bit group, W = 128 / K."""
    W = 128 // K
    ids = np.asarray(ids, dtype=np.uint64)
    w = np.zeros((len(ids), 4), dtype=np.uint64)
    for k in range(K):
        b = k * W
        i, o = b >> 5, b & 31
        w[:, i] |= (ids[:, k] << np.uint64(o)) & np.uint64(U32_MAX)
        if o + W > 32:
            w[:, i + 1] |= ids[:, k] >> np.uint64(32 - o)
    return w.astype(np.uint32)


def _exclusive(n):
    out = np.zeros(len(n) + 1, dtype=np.int64)
    np.cumsum(n, out=out[1:])
    return out


def slot_owners(off):
    return np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))


def reverse_csr(V, off, adj, mutant=None):
    """(roff, radj): the forward slots sorted stably by destination."""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    owner = slot_owners(off)
    if mutant == "sort_unstable":
        order = np.lexsort((-np.arange(len(adj)), adj))
    else:
        order = np.argsort(adj, kind="stable")
    indeg = np.bincount(adj, minlength=V)[:V] if V else np.zeros(0, dtype=np.int64)
    roff = _exclusive(indeg)
    if mutant == "roff_gap_late" and V:
        v = np.arange(V)
        last = np.maximum.accumulate(np.where(indeg > 0, v, -1))  # the last vertex with in-edges at or before v
        gap = (indeg == 0) & (last >= 0)
        roff = roff.copy()
        roff[:V][gap] = roff[last[gap]]
    return roff, owner[order]


def _lists(off, ln, ng, per_group, src):
    """[groups, per_group] entries: group g of vertex v holds src[b + min(i, len - 1)] for i = g per_group .. + per_group - 1.
    Returns (entries, positions i, owner's len, owner's first slot): the last three for the padding mutants."""
    V = len(ln)
    gbeg = _exclusive(ng)
    owner = np.repeat(np.arange(V, dtype=np.int64), ng)
    local = np.arange(int(gbeg[-1]), dtype=np.int64) - gbeg[owner]
    i = local[:, None] * per_group + np.arange(per_group, dtype=np.int64)[None, :]
    n = ln[owner][:, None]
    idx = off[owner][:, None] + np.minimum(i, n - 1)
    return src[idx] if len(src) else np.zeros(idx.shape, dtype=np.int64), i, n, off[owner][:, None]


def direction(V, off, adj, ooff, pfirst_other, opt, K, mutant=None):
    """One direction's arrays from its own CSR (off, adj) and the other direction's offsets."""
    ln = np.diff(off)
    align = max(4, int(opt["meet_align"])) & ~3
    ng = (ln // align if mutant == "no_ceil" else (ln + align - 1) // align) * (align // 4)
    gbeg = _exclusive(ng)
    seg = np.stack([gbeg[:V], ln], axis=1).astype(np.uint32)
    padded, i, n, b = _lists(off, ln, ng, 4, adj)
    if mutant == "pad_first":
        padded = np.where(i >= n, adj[np.minimum(b, len(adj) - 1)], padded)
    elif mutant == "pad_zero":
        padded = np.where(i >= n, 0, padded)
    elif mutant == "align_unfilled":
        padded = np.where((i >> 2) >= ((n + 3) >> 2), -1, padded)
    owner = slot_owners(off)
    # the packed copy
    packed, pfirst = None, np.zeros(V + 1, dtype=np.int64)
    if K > 4:
        palign = max(1, int(opt["meet_pack_align"]))
        png = pack_list_groups(ln, K, palign)
        pfirst = _exclusive(png)
        src = adj
        if opt["meet_pack_order"]:
            bucket = pack_order_bucket(np.diff(ooff)[adj])
            keys = (-bucket, owner) if mutant != "pack_ties_id_desc" else (-adj, -bucket, owner)
            src = adj[np.lexsort(keys)]  # stable: equal buckets of a vertex keep the CSR's order
        packed = pack_put(_lists(off, ln, png, K, src)[0], K)
    u = adj
    word4 = (pfirst_other if mutant == "desc_other_scan" else pfirst)[u] if K > 4 else np.zeros(len(u), dtype=np.int64)
    who = owner if mutant == "desc_own_seg" else u
    desc = np.stack([u, gbeg[who], ln[who], word4], axis=1).astype(np.uint32)
    c = _exclusive(ln[adj])
    work = c[off[1:]] - c[off[:-1]]
    if mutant == "work_counts_own":
        work = work + ln
    work = (work & U32_MAX if mutant == "work_wraps" else np.minimum(work, U32_MAX)).astype(np.uint32)
    return dict(off=off, adj=adj.astype(np.int32), seg=seg, padded=padded.astype(np.int32), desc=desc, work=work, packed=packed,
                rhead=None, pfirst=pfirst)


def rhead_model(V, roff, radj, mutant=None, block=1 << 16):
    out = np.empty((V, 64), dtype=np.uint32)
    w = np.arange(64, dtype=np.int64)
    cw = 32 if mutant == "rhead_count_32" else 31
    if mutant == "rhead_count_32":
        e_of = np.where(w < 32, w, w - 1)
    elif mutant == "rhead_unshifted":
        e_of = w.copy()
    else:
        e_of = np.where(w < 31, w, w - 1)
    ext = np.concatenate([radj, radj[-1:]]) if len(radj) else np.zeros(1, dtype=np.int64)  # (rhead_clamp_cnt reads one past a list)
    for v0 in range(0, V, block):  # blocks of vertices: the index array of all V x 64 words at once is a gigabyte at 2^21
        v1 = min(V, v0 + block)
        b, cnt = roff[v0:v1, None], np.diff(roff[v0:v1 + 1])[:, None]
        e = np.minimum(e_of[None, :], cnt if mutant == "rhead_clamp_cnt" else cnt - 1)
        blk = ext[np.minimum(b + np.maximum(e, 0), len(ext) - 1)]
        blk = np.where(cnt == 0, U32_MAX, blk)
        blk[:, cw] = cnt[:, 0]
        out[v0:v1] = blk.astype(np.uint32)
    return out


DEFAULTS = dict(meet_layout=1, meet_align=32, meet_pack=1, meet_pack_align=8, meet_pack_order=1, ball=1, ball_head_mb=512)


def layout(V, off, adj, mutant=None, **options):
    """The whole contract for the CSR (off, adj) of V vertices under the upload's options (DEFAULTS: the shipped values).
    Returns a dict: has_layout, pack_k, pack_align, pack_order, has_rhead, max_out_degree, max_in_degree, two_hop_mean, groups,
    rgroups, pgroups, prgroups and dirs = [forward, reverse], each a dict off, adj, seg, padded, desc, work, packed, rhead (None
    for an array that does not exist; without a layout only off and adj do)."""
    assert mutant is None or mutant in MUTANTS, mutant
    opt = dict(DEFAULTS)
    assert set(options) <= set(opt), options
    opt.update(options)
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    E = len(adj)
    assert len(off) == V + 1 and off[V] == E
    roff_true, radj = reverse_csr(V, off, adj, mutant if mutant == "sort_unstable" else None)
    outdeg, indeg = np.diff(off), np.diff(roff_true)
    res = dict(has_layout=0, pack_k=4, pack_align=1, pack_order=0, has_rhead=0, groups=0, rgroups=0, pgroups=0, prgroups=0,
               max_out_degree=int(outdeg.max()) if V else 0, max_in_degree=int(indeg.max()) if V else 0,
               two_hop_mean=float(int((indeg * outdeg).sum())) / float(max(V, 1)))
    none = dict(seg=None, padded=None, desc=None, work=None, packed=None, rhead=None)
    dirs = [dict(none, off=off, adj=adj.astype(np.int32)), dict(none, off=roff_true, adj=radj.astype(np.int32))]
    if opt["meet_layout"] and V > 0 and E > 0:
        K = pack_k_for(V, opt["meet_pack"] >= 2, mutant) if opt["meet_pack"] else 4
        f = direction(V, off, adj, roff_true, None, opt, K, None if mutant == "desc_other_scan" else mutant)
        r = direction(V, roff_true, radj, off, f["pfirst"], opt, K, mutant)
        if mutant == "desc_other_scan":
            f = direction(V, off, adj, roff_true, r["pfirst"], opt, K, mutant)
        if opt["ball"] and V * 256 <= max(0, int(opt["ball_head_mb"])) << 20:
            r["rhead"] = rhead_model(V, roff_true, radj, mutant)
            res["has_rhead"] = 1
        dirs = [f, r]
        res.update(has_layout=1, pack_k=K, groups=len(f["padded"]), rgroups=len(r["padded"]))
        if K > 4:
            res.update(pack_align=max(1, int(opt["meet_pack_align"])), pack_order=1 if opt["meet_pack_order"] else 0,
                       pgroups=len(f["packed"]), prgroups=len(r["packed"]))
    if mutant == "roff_gap_late":
        dirs[1]["off"] = reverse_csr(V, off, adj, mutant)[0]
    res["dirs"] = dirs
    return res


ARRAYS = ("off", "adj", "seg", "padded", "desc", "work", "packed", "rhead")
SCALARS = ("pack_k", "pack_align", "pack_order", "has_rhead", "groups", "rgroups", "pgroups", "prgroups", "max_out_degree",
           "max_in_degree", "two_hop_mean")


def differences(a, b):
    """Names of everything in which two results differ: scalars by name, arrays as 'f.seg' / 'r.rhead'.  Exact comparison, of
    whole arrays; an array that exists on one side only counts."""
    out = [k for k in SCALARS if a[k] != b[k]]
    for d, (x, y) in zip("fr", zip(a["dirs"], b["dirs"])):
        for k in ARRAYS:
            p, q = x[k], y[k]
            if (p is None) != (q is None) or (p is not None and (p.shape != q.shape or not np.array_equal(p, q))):
                out.append("%s.%s" % (d, k))
    return out
