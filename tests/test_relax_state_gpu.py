"""The label arrays a pooled workspace carries from one cheapest-path call to the next (RelaxSide::prepare / settle).

Between calls a workspace's labels are all "unlabelled" for ONE (V, label type, side): int64 labels, doubles and 4-byte labels
have different patterns and cell sizes, and the two-ended search keeps a second array for its backward side.  A call that
trusts an array left by another kind of call starts from wrong labels.  Here two handles on the same V and edges (int64 weights
whose sums fit 31 bits, double weights) are searched in a fixed order of label widths, weight types, one- and two-ended
searches, forwards and backwards, then through the chain pre-pass's inner workspace — every call checked exactly against the
CPU oracle, on the smallest graph that has heavy lists on both sides and three batches per call.

Every call searches 130 pairs with distinct sources (three batches of 64 lanes, one lane per source or per pair) and 10
trivial rows beside them, which take no lane."""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from oracle.pgq_oracle import OracleCSR

pytestmark = pytest.mark.gpu

# every option these calls depend on, at the value the sequence starts from (another file may have left its own)
KEYS = {"streams": 1, "relax_streams": 0, "chain": 0, "chain_cap": 4096, "wbibfs": 0, "relax_light": 2, "relax_light_div": 4,
        "relax_light_min_degree": 16, "relax_labels32": 1, "relax_split": 1, "relax_delta_div": 0, "relax_small_limit": 2048,
        "relax_bidir": 0, "relax_bidir_rows": 2, "relax_bidir_c0_div": 64, "relax_bidir_step_div": 128}

V, HUB_OUT, HUB_IN = 300, 7, 11
INT64, DOUBLE = 0, 1  # csr ids

# (handle, options on top of KEYS)
STEPS = [(INT64, {"relax_light": 2, "relax_labels32": 1}),
         (INT64, {"relax_light": 2, "relax_labels32": 0}),
         (DOUBLE, {"relax_light": 2}),
         (INT64, {"relax_light": 2, "relax_bidir": 1, "relax_labels32": 1}),
         (INT64, {"relax_light": 2, "relax_bidir": 1, "relax_labels32": 0}),
         (INT64, {"relax_light": 0, "relax_small_limit": 0}),
         (INT64, {"relax_light": 0, "relax_small_limit": 2048}),
         (DOUBLE, {"relax_light": 0})]


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k, v in KEYS.items():
        pgq.set_option(k, v)
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


def graph(rng):
    others_out = np.setdiff1d(np.arange(V), [HUB_OUT])
    others_in = np.setdiff1d(np.arange(V), [HUB_IN])
    s = np.concatenate([rng.integers(0, V, 2000), np.full(200, HUB_OUT), rng.permutation(others_in)[:200]])
    d = np.concatenate([rng.integers(0, V, 2000), rng.permutation(others_out)[:200], np.full(200, HUB_IN)])
    return s.astype(np.int64), d.astype(np.int64), np.arange(len(s), dtype=np.int64)


def test_label_arrays_across_widths_types_and_sides():
    rng = np.random.default_rng(4242)
    s, d, e = graph(rng)
    assert (np.bincount(s, minlength=V)[HUB_OUT] >= 200) and (np.bincount(d, minlength=V)[HUB_IN] >= 200)  # over kHeavyMin = 128
    w = {INT64: rng.integers(1, 1000, len(s)).astype(np.int64), DOUBLE: rng.random(len(s)) + 0.01}
    assert 999 * V < 2 ** 31 - 1  # 4-byte labels are taken
    st = pgq.PgqState()
    ora = {}
    for cid in (INT64, DOUBLE):
        st.build_csr(cid, V, s, d, e, w[cid])
        ora[cid] = OracleCSR.from_edges(V, s, d, e, w[cid])
    # 130 distinct sources with several out-edges (the chain pre-pass leaves such rows open), both hubs among the pairs
    outdeg = np.bincount(s, minlength=V)
    src = rng.permutation(np.flatnonzero(outdeg >= 2))[:130]
    if HUB_OUT not in src:
        src[0] = HUB_OUT
    dst = (src + 1 + rng.integers(0, V - 1, 130)) % V  # never the source
    dst[:5] = HUB_IN
    dst[src == dst] = HUB_OUT
    assert len(np.unique(src)) == 130 and (src != dst).all()
    triv = rng.integers(0, V, 10)
    ps, pd = np.concatenate([src[:70], triv, src[70:]]), np.concatenate([dst[:70], triv, dst[70:]])
    want = {cid: ora[cid].lean_cheapest_path_length(V, ps, pd) for cid in (INT64, DOUBLE)}
    assert want[INT64][1].sum() > 100  # most pairs are connected

    def call(step, chain):
        cid, opts = STEPS[step]
        for k, v in {**KEYS, **opts, "chain": chain}.items():
            pgq.set_option(k, v)
        pgq.reset_stats()
        out, ok = st.cheapest_path_length(cid, V, ps, pd)
        lout, lok = want[cid]
        assert (ok == lok).all(), (step + 1, chain)
        if cid == INT64:
            assert (out[ok] == lout[ok]).all(), (step + 1, chain)
            assert pgq.get_stats()["batches"] == 3, (step + 1, chain)
        else:  # bit for bit
            assert (np.asarray(out)[ok].view(np.int64) == np.asarray(lout)[lok].view(np.int64)).all(), (step + 1, chain)

    order = list(range(len(STEPS)))
    for step in order + order[::-1]:
        call(step, 0)
    for step in (0, 2, 3):  # the inner workspace lease of the chain pre-pass
        call(step, 1)
