"""GPU parity of the pair-centric pre-pass over the bit-packed lists (pgq_pack.h: six 21-bit / five 25-bit ids per
16-byte group) against the 32-bit lists (meet_pack = 0) and the CPU oracle, on graphs whose vertex counts sit just below
and above the limits of each packing (2^16, 2^21, 2^25) and whose ids reach the top of the id range.  Every handle's
pack_k is checked, so that a build which quietly skipped the packed copy (or packed past its limit) fails.  Hub endpoints
and a small walk cap send rows through k_meet3w (chunk-sized calls) and k_meet4d (cut walks taken up, distance 4)."""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from helpers import sparse_ids_graph
from oracle.pgq_oracle import OracleCSR

pytestmark = pytest.mark.gpu

KEYS = {"meet": 1, "meet_bias": 1e9, "meet_cap": 512, "meet_cap_small": 512, "meet_wide_rows_always": 0, "ball": 0,
        "wbibfs": 0, "meet_pack": 1}


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k, v in KEYS.items():
        pgq.set_option(k, v)
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


def run(V, act, s, d, hubs, rng, n_pairs, packs):
    """packs: {meet_pack option: the pack_k the upload must choose}"""
    ora = OracleCSR.from_edges(V, s, d)
    ps = act[rng.integers(0, len(act), n_pairs)].astype(np.int64)
    pd = act[rng.integers(0, len(act), n_pairs)].astype(np.int64)
    ps[:8] = hubs[:2].repeat(4)
    pd[4:12] = hubs[-1]
    ps[12] = pd[12]
    oln, ook = ora.lean_iterativelength(V, ps, pd)
    want = [int(v) if k else None for v, k in zip(oln, ook)]
    got = {}
    for pack, want_k in packs.items():
        pgq.set_option("meet_pack", pack)  # read at upload
        st = pgq.PgqState()
        st.build_csr(0, V, s, d)
        assert st.device_csr(0).pack_k == want_k, (V, pack)
        for wide in (0, 1):  # k_meet3 / k_meet3w (several wavefronts per row)
            pgq.set_option("meet_wide_rows_always", wide)
            ln, ok = st.iterativelength(0, V, ps, pd)
            got[(pack, wide)] = [int(v) if k else None for v, k in zip(ln, ok)]
            assert got[(pack, wide)] == want, (V, pack, wide)
        assert pgq.get_stats()["meet_pairs"] > 0
        st.delete_csr(0)
    return want


@pytest.mark.parametrize("V", [(1 << 16) - 1, 1 << 16, (1 << 16) + 1, (1 << 21) - 1, 1 << 21, (1 << 21) + 1])
def test_packed_walk_matches_oracle(V):
    rng = np.random.default_rng(V % 1000)
    act, s, d, hubs, _ = sparse_ids_graph(rng, V, 6000, 60000)
    packed = 6 if V <= 1 << 21 else 4  # meet_pack = 1 packs up to 2^21 vertices
    want = run(V, act, s, d, hubs, rng, 2000, {1: packed, 0: 4, 2: 6 if V <= 1 << 21 else 5})
    assert any(w is not None and w >= 3 for w in want)


@pytest.mark.parametrize("V", [(1 << 25) - 1, 1 << 25, (1 << 25) + 1])
def test_packed_walk_matches_oracle_bigv(V):
    # 25-bit ids (K = 5, meet_pack = 2) up to 2^25 vertices; one more and the upload keeps the 32-bit lists only
    rng = np.random.default_rng(V % 1000)
    act, s, d, hubs, _ = sparse_ids_graph(rng, V, 3000, 24000)
    run(V, act, s, d, hubs, rng, 256, {2: 5 if V <= 1 << 25 else 4, 1: 4, 0: 4})
