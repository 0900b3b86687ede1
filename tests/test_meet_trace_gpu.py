"""The TRACE instantiations of the pre-pass (option meet_trace): k_meet4d<*, true> and k_src_ball<*, true>.

No other test sets meet_trace, and the launch dispatch alone picks these instantiations from the runtime flags.  A traced
kernel times its rows and phases and writes the times into a buffer of its own (summarised on stderr); its answers are the
untraced kernel's.  One graph — a hub, random edges, 8 chains of 10 edges over ids of their own: distances 1 to 9 and
unreachable pairs, so rows reach k_meet4d and k_bibfs — and about 2000 rows (random pairs, the chain pairs both ways,
src == dst rows, NULL sources) run with meet_trace = 1 for the LDS and the global-map placement (meet4_lds_kb 150 / 0), with
and without the source-centric kernel in front (ball 2 / 0), always with meet4_batch = 2:
  - every row equals the CPU oracle's;
  - the pre-pass answered rows itself (meet_pairs), and under ball = 2 k_src_ball took the call (ball_calls);
  - the same call with meet_trace = 0 gives byte-identical output;
  - the traced instantiation really ran: the summary on stderr is made of what the kernel wrote into the (zeroed) trace buffer, so
    an untraced kernel behind meet_trace = 1 would report no rows (k_meet4d) or a longest segment of 0 us (k_src_ball).
About 4096 vertex ids make a 512-byte map, below the 4 KB of one wavefront's filter: the batch pass is off there whatever
meet4_batch says.  The same graph over 65,536 ids (an 8-KB map: two rows per batch) runs it inside the traced kernel."""
import re

import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from helpers import sparse_ids_graph
from oracle.pgq_oracle import OracleCSR

pytestmark = pytest.mark.gpu

KEYS = ("meet", "meet_bias", "meet_cap", "meet_cap_small", "meet4", "meet4_cap", "meet4_test_cap", "meet4_lds_kb",
        "meet4_global_mb", "meet4_batch", "meet_layout", "meet_small_rows", "bibfs_rows", "bibfs_cap", "bibfs_queue",
        "bibfs_grid", "ball", "ball_head_mb", "ball_cap", "ball_test_cap", "ball_grid", "ball_bias", "meet_trace")


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k in KEYS:
        pgq.set_option(k, pgq.get_default_option(k))
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


class Case:
    """The graph over V vertex ids, its rows and their oracle distances (computed once per V)."""

    def __init__(self, V):
        rng = np.random.default_rng(V)
        self.V = V
        act, s, d, _, chains = sparse_ids_graph(rng, V, 3000, 8000, hubs=1, chains=8, chain_len=10)
        self.s, self.d = s, d
        ps = [act[rng.integers(0, len(act), 1100)]]
        pd = [act[rng.integers(0, len(act), 1100)]]
        for c in chains:  # every pair along a chain (distance j - i) and against it (unreachable)
            i, j = np.triu_indices(len(c), 1)
            ps += [c[i], c[j]]
            pd += [c[j], c[i]]
        ps, pd = np.concatenate(ps).astype(np.int64), np.concatenate(pd).astype(np.int64)
        same = rng.random(len(ps)) < 0.01  # src == dst rows
        pd[same] = ps[same]
        perm = rng.permutation(len(ps))
        self.ps, self.pd = ps[perm], pd[perm]
        self.valid = rng.random(len(ps)) > 0.03  # NULL sources
        oln, ook = OracleCSR.from_edges(V, s, d).lean_iterativelength(V, self.ps, self.pd, nthreads=8)
        self.want = [int(v) if (k and ok) else None for v, k, ok in zip(oln, ook, self.valid)]
        dist = np.where(ook, oln, -1)
        assert all((dist == k).any() for k in range(1, 10)) and (dist < 0).any(), "the rows miss a distance"


_cases = {}


def case_for(V):
    if V not in _cases:
        _cases[V] = Case(V)
    return _cases[V]


@pytest.mark.parametrize("ball", [0, 2])
@pytest.mark.parametrize("lds_kb", [150, 0], ids=["lds_map", "global_map"])
@pytest.mark.parametrize("V", [4096, 65536])
def test_traced_kernels_answer_like_untraced(V, lds_kb, ball, capfd):
    case = case_for(V)
    for k, v in (("meet", 1), ("meet_bias", 1e9), ("meet4_lds_kb", lds_kb), ("ball", ball), ("meet4_batch", 2)):
        pgq.set_option(k, v)
    out = {}
    for trace in (1, 0):
        pgq.set_option("meet_trace", trace)
        st = pgq.PgqState()  # a fresh handle: both calls are its first (k_bibfs in the chain, no route memo)
        st.build_csr(0, V, case.s, case.d)
        pgq.reset_stats()
        settled = pgq.get_option("meet4_batch_settled")
        ln, ok = st.iterativelength(0, V, case.ps, case.pd, src_valid=case.valid)
        settled = int(pgq.get_option("meet4_batch_settled") - settled)
        stats = pgq.get_stats()
        st.delete_csr(0)
        err = capfd.readouterr().err
        out[trace] = (np.asarray(ln).tobytes(), np.asarray(ok).tobytes())
        if not trace:
            assert "trace:" not in err, err
            continue
        assert [int(v) if k else None for v, k in zip(ln, ok)] == case.want, (V, lds_kb, ball)
        assert stats["meet_pairs"] > 0, (V, lds_kb, ball, stats["meet_pairs"])
        if ball == 2:
            assert stats["ball_calls"] >= 1, (V, lds_kb, stats["ball_calls"])
            m = re.search(r"k_src_ball trace: (\d+) segments, .* longest segment ([0-9.]+) us", err)
            assert m and int(m.group(1)) >= 1 and float(m.group(2)) > 0, err
        else:
            m = re.search(r"k_meet4d trace: \d+ workgroups, queue (\d+) front \+ (\d+) back, (\d+) whole-workgroup rows.*batch pass: (\d+) rows", err)
            assert m, err
            front, back, whole, batched = (int(x) for x in m.groups())
            # every queued row was taken by a whole workgroup or by the batch pass (a batch's miss by both)
            assert front + back > 0 and front + back <= whole + batched <= 2 * (front + back), err
        if ball == 0 and lds_kb and V == 65536:
            # the chains' distance-4 pairs: k_meet3 proves them far, and the two endpoints' two-hop walks are one vertex each,
            # the same one: a batch row finds it
            assert settled >= 1, "the batch pass settled no row inside the traced kernel"
    assert out[1] == out[0], "meet_trace changed the output (V %d, meet4_lds_kb %d, ball %d)" % (V, lds_kb, ball)
