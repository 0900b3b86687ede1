"""CPU checks of the bit-packed list layout (duckpgq-extension_amd/csrc/pgq_pack.h): the header the upload kernel and the
device walk share is compiled with g++ into a small shim, the packed copy of random CSRs is built group by group with it
exactly as k_fill_packed does, and unpacked again.  A lane-by-lane model of seg_walk's requests (pgq_walk.h: seg_round<K>,
the descriptor word that holds the first group, seg_owner, the clamp past a round's end) checks that a walk over the packed
groups hands every lane entries of its own list and yields the same entries, round by round, as the walk over the 32-bit
padded lists."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "duckpgq-extension_amd", "csrc")

SHIM = r"""
#include "pgq_pack.h"
using namespace pgq;
extern "C" {
int shim_k_for(long long V, int with5) { return pack_k_for(V, with5 != 0); }
unsigned shim_groups(unsigned len, int K, unsigned align) { return pack_list_groups(len, K, align); }
// the packed copy of a CSR: gbeg[V + 1] (exclusive scan of the group counts), out[4 x total groups]
void shim_build(long long V, const long long *off, const int *adj, int K, unsigned align, unsigned *gbeg, unsigned *out) {
	unsigned g = 0;
	for (long long v = 0; v < V; v++) {
		gbeg[v] = g;
		const long long len = off[v + 1] - off[v];
		const unsigned ng = pack_list_groups((unsigned)len, K, align);
		for (unsigned j = 0; j < ng; j++, g++) {
			if (K == 6) pack_list_group<6>(adj + off[v], len, j, out + 4ull * g);
			else if (K == 5) pack_list_group<5>(adj + off[v], len, j, out + 4ull * g);
			else pack_list_group<4>(adj + off[v], len, j, out + 4ull * g);
		}
	}
	gbeg[V] = g;
}
void shim_unpack(int K, const unsigned *w, unsigned *ids) {
	for (int k = 0; k < K; k++) ids[k] = K == 6 ? pack_get<6>(w, k) : (K == 5 ? pack_get<5>(w, k) : pack_get<4>(w, k));
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the layout shim")
    d = tmp_path_factory.mktemp("pack")
    src, so = d / "shim.cpp", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)],
                   check=True)
    lib = C.CDLL(str(so))
    lib.shim_k_for.restype = C.c_int
    lib.shim_k_for.argtypes = [C.c_longlong, C.c_int]
    lib.shim_groups.restype = C.c_uint
    lib.shim_groups.argtypes = [C.c_uint, C.c_int, C.c_uint]
    P = np.ctypeslib.ndpointer
    lib.shim_build.argtypes = [C.c_longlong, P(np.int64), P(np.int32), C.c_int, C.c_uint, P(np.uint32), P(np.uint32)]
    lib.shim_unpack.argtypes = [C.c_int, P(np.uint32), P(np.uint32)]
    return lib


def pack_csr(shim, V, off, adj, K, align):
    total = sum(shim.shim_groups(int(off[v + 1] - off[v]), K, align) for v in range(V))
    gbeg = np.zeros(V + 1, dtype=np.uint32)
    out = np.zeros(4 * max(total, 1), dtype=np.uint32)
    shim.shim_build(V, np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(adj, dtype=np.int32), K, align, gbeg, out)
    return gbeg, out


def unpack_groups(shim, K, words, first, n):
    ids = np.zeros(K, dtype=np.uint32)
    res = []
    for g in range(first, first + n):
        shim.shim_unpack(K, np.ascontiguousarray(words[4 * g:4 * g + 4]), ids)
        res.extend(ids.tolist())
    return res


def random_csr(rng, V, E, id_hi):
    """A CSR over V vertices whose listed ids reach id_hi - 1: empty lists, lists of every short length around the group
    sizes, multi-edges and a hub."""
    lens = list(range(0, 14)) + [0, 0, 1, 1] + [int(x) for x in rng.integers(0, 40, max(0, V - 19))]
    lens = lens[:V - 1] + [E]  # the last vertex is a hub
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    adj = rng.integers(0, id_hi, int(off[-1])).astype(np.int32)
    adj[:5] = id_hi - 1
    if len(adj) > 40:
        adj[30:40] = adj[20:30]  # multi-edges
    return off, adj


@pytest.mark.parametrize("V,K", [((1 << 16) - 1, 6), (1 << 16, 6), ((1 << 16) + 1, 6), ((1 << 21) - 1, 6), (1 << 21, 6),
                                 ((1 << 21) + 1, 5), ((1 << 25) - 1, 5), (1 << 25, 5), ((1 << 25) + 1, 4)])
def test_k_choice(shim, V, K):
    assert shim.shim_k_for(V, 1) == K  # meet_pack = 2
    assert shim.shim_k_for(V, 0) == (K if K == 6 else 4)  # meet_pack = 1: K = 5 is not taken


@pytest.mark.parametrize("id_hi", [1 << 16, (1 << 21), (1 << 25)])
@pytest.mark.parametrize("align", [1, 8])
def test_unpack_returns_every_list(shim, id_hi, align):
    rng = np.random.default_rng(id_hi % 97 + align)
    K = shim.shim_k_for(id_hi, 1)
    V = 300
    off, adj = random_csr(rng, V, 5000, id_hi)
    gbeg, words = pack_csr(shim, V, off, adj, K, align)
    for v in range(V):
        lst = adj[off[v]:off[v + 1]].tolist()
        n = len(lst)
        ng = int(gbeg[v + 1] - gbeg[v])
        assert ng == -(-n // (K * align)) * align  # ceil(n / (K align)) x align groups: the walk reads ceil(n / K) of them
        assert gbeg[v] % align == 0
        if n == 0:
            continue
        got = unpack_groups(shim, K, words, int(gbeg[v]), -(-n // K))
        assert got[:n] == lst
        assert got[n:] == [lst[-1]] * (len(got) - n)  # padding repeats the last entry
        if ng * K > len(got):  # whole groups of alignment past the walked ones: the last entry too
            rest = unpack_groups(shim, K, words, int(gbeg[v]) + -(-n // K), ng - -(-n // K))
            assert set(rest) == {lst[-1]}


def test_bits_past_the_ids_are_zero(shim):
    for K, W in ((6, 21), (5, 25)):
        off = np.array([0, K], dtype=np.int64)
        adj = np.full(K, (1 << W) - 1, dtype=np.int32)
        _, words = pack_csr(shim, 1, off, adj, K, 1)
        bits = sum(bin(int(w)).count("1") for w in words[:4])
        assert bits == K * W
        assert int(words[3]) >> (K * W - 96) == 0


def seg_walk_model(shim, descs, words, K):
    """The requests of seg_walk (pgq_walk.h) over slot descriptors {neighbour, first group, entries, first packed group},
    lane by lane as the device makes them: seg_round<K> (groups ceil(len / K), inclusive prefix P, D = first group - (P -
    groups), the first group taken from the 2nd descriptor word for K = 4 and from the 4th for K > 4), seg_owner (lane + 1
    dropped at the window position where a list begins, an inclusive max-scan over the window), the clamp of lanes past the
    round's end, and the group at D[owner] + x decoded with pgq_pack.h.  Yields per round (round's descriptors, [(owner,
    ok, group index inside the owner's list, ids)])."""
    for r0 in range(0, len(descs), 64):
        rnd = descs[r0:r0 + 64]
        rnd = rnd + [(0, 0, 0, 0)] * (64 - len(rnd))
        ng = [(d[2] + K - 1) // K for d in rnd]
        P = np.cumsum(ng).tolist()
        D = [(d[1] if K == 4 else d[3]) - (P[l] - ng[l]) for l, d in enumerate(rnd)]
        total = P[63]
        reqs = []
        for c in range(-(-total // 64)):
            x0 = 64 * c
            win = [0] * 64
            for l in range(64):
                start = P[l] - ng[l]
                if ng[l] and start < x0 + 64 and P[l] > x0:
                    win[start - x0 if start > x0 else 0] = l + 1
            own, m = [], 0
            for l in range(64):
                m = max(m, win[l])
                own.append(m - 1)
            for l in range(64):
                xx = x0 + l
                ok = xx < total
                xs = xx if ok else total - 1
                j = own[l]
                reqs.append((j, ok, xs - (P[j] - ng[j]), unpack_groups(shim, K, words, D[j] + xs, 1)))
        yield rnd, reqs


@pytest.mark.parametrize("id_hi", [1 << 16, 1 << 21, 1 << 25])
def test_packed_walk_model_matches_32bit_walk(shim, id_hi):
    rng = np.random.default_rng(5 + id_hi % 13)
    K = shim.shim_k_for(id_hi, 1)
    V = 200
    off, adj = random_csr(rng, V, 3000, id_hi)
    gbeg4, w4 = pack_csr(shim, V, off, adj, 4, 8)  # the 32-bit padded layout (meet_align = 32 entries = 8 groups)
    gbegK, wK = pack_csr(shim, V, off, adj, K, 8)
    # one two-hop walk's descriptors (k_fill_desc): 130 neighbours = three rounds, empty lists and the hub among them
    order = rng.permutation(V)[:129].tolist() + [V - 1]
    descs = [(u, int(gbeg4[u]), int(off[u + 1] - off[u]), int(gbegK[u])) for u in order]
    per_k = {}
    for k, words in ((4, w4), (K, wK)):
        rounds = []
        for rnd, reqs in seg_walk_model(shim, descs, words, k):
            got = {}
            for j, ok, g, ids in reqs:
                u, n = rnd[j][0], rnd[j][2]
                lst = adj[off[u]:off[u + 1]].tolist()
                assert n > 0 and set(ids) <= set(lst)  # every lane holds real entries of its owner's list (padding too)
                if ok:
                    assert 0 <= g < (n + k - 1) // k and g not in got.get(j, {})
                    got.setdefault(j, {})[g] = ids
            walked = []
            for j, d in enumerate(rnd):
                if d[2] == 0:
                    assert j not in got
                    continue
                ids = [x for g in sorted(got[j]) for x in got[j][g]]
                lst = adj[off[d[0]]:off[d[0] + 1]].tolist()
                assert sorted(got[j]) == list(range((d[2] + k - 1) // k))  # every group of the list, once
                assert ids[:d[2]] == lst and set(ids[d[2]:]) <= {lst[-1]}
                walked.append((d[0], ids[:d[2]]))
            rounds.append(walked)
        per_k[k] = rounds
    assert per_k[4] == per_k[K]  # the same entries of the same lists, round by round
