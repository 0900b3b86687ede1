"""A numpy model of the hub tables a CSR upload builds for k_meet3 (pgq_csr_hub_tables): the selection of the hubs
and the four tables, bit for bit, and the two proofs read from them.  Not a test module: the tests import it.

Hubs are the top H vertices by out-degree + in-degree (parallel edges count), ties broken by the smaller id, among the vertices
whose sum is at least min_degree; fewer than min_count such vertices: no tables.  Hub h is bit h & 63 of 64-bit word h >> 6."""
import numpy as np


def fit_hubs(V, H, budget_mb):
    """The H an upload uses: the option rounded down to 1024 / 512 / 256 (below 256: none), halved down to 256 while the four
    tables of V x H / 8 bytes and the H hub ids are over the budget; 0: no tables."""
    H = 1024 if H >= 1024 else 512 if H >= 512 else 256 if H >= 256 else 0
    budget = max(0, int(budget_mb)) << 20
    size = lambda h: 4 * V * (h // 8) + 4 * h  # the four tables and the hub ids
    while H > 256 and size(H) > budget:
        H //= 2
    return 0 if H == 0 or size(H) > budget else H


def select_hubs(V, src, dst, H, min_degree=128, min_count=64):
    """The hub ids in bit order as an int32 array of H entries (-1 in unused slots), or None: no tables."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    deg = np.bincount(src, minlength=V) + np.bincount(dst, minlength=V)
    ok = np.flatnonzero(deg >= max(0, int(min_degree)))
    if len(ok) < max(1, int(min_count)):
        return None
    order = ok[np.lexsort((ok, -deg[ok]))]  # most edges first, then the smaller id
    ids = np.full(H, -1, dtype=np.int32)
    n = min(H, len(order))
    ids[:n] = order[:n]
    return ids


def _pack(bits):
    """bool [V, H] -> uint64 [V, H / 64], bit h of a row = bit h & 63 of word h >> 6."""
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8").astype(np.uint64)


def build_tables(V, src, dst, ids):
    """dict of hub1_out, hub1_in, hub2_out, hub2_in: uint64 [V, H / 64]."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    H = len(ids)
    slot = np.full(V, -1, dtype=np.int64)
    used = np.flatnonzero(ids >= 0)
    slot[ids[used]] = used
    one_out, one_in = np.zeros((V, H), dtype=bool), np.zeros((V, H), dtype=bool)
    e = slot[dst] >= 0
    one_out[src[e], slot[dst[e]]] = True  # v -> h
    e = slot[src] >= 0
    one_in[dst[e], slot[src[e]]] = True  # h -> v
    h1o, h1i = _pack(one_out), _pack(one_in)
    h2o, h2i = np.zeros_like(h1o), np.zeros_like(h1i)
    np.bitwise_or.at(h2o, src, h1o[dst])  # OR of hub1_out over the out-neighbours
    np.bitwise_or.at(h2i, dst, h1i[src])  # OR of hub1_in over the in-neighbours
    return dict(hub1_out=h1o, hub1_in=h1i, hub2_out=h2o, hub2_in=h2i)


def proofs(t, s, d):
    """(P3, P4) for the rows (s[k], d[k]): a 3-edge walk s -> d exists / a 4-edge walk exists."""
    s, d = np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)
    p3 = ((t["hub2_out"][s] & t["hub1_in"][d]) | (t["hub1_out"][s] & t["hub2_in"][d])).any(axis=1)
    p4 = (t["hub2_out"][s] & t["hub2_in"][d]).any(axis=1)
    return p3, p4
