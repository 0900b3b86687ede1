"""csrc/pgq_analytics.hip bit for bit: PageRank (k_pr_*) against tests/analytics_model.py in device mode at the sizes around
k_pr_dangling's slicing, the Boruvka rounds of weakly_connected_component (k_wcc_*) on graphs that need many rounds, deep hook
chains or none, and k_lcc / k_lcc_big with counts that a float32 cannot hold.  test_analytics_cpu.py holds the model against
the oracle, the reference's goldens and extended precision, and shows what each fixture is for.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import analytics_model as am
import duckpgq_extension_amd as pgq
from oracle.pgq_oracle import OracleCSR

pytestmark = pytest.mark.gpu

PR_NAMES = [f[0] for f in am.pagerank_fixtures()]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def edge_table(V, off, adj):
    """An edge table that builds (off, adj) again: one row per slot, in slot order."""
    return np.repeat(np.arange(V, dtype=np.int64), np.diff(off)), np.asarray(adj, dtype=np.int64)


def explain(name, got, want):
    bad = np.flatnonzero(bits(got) != bits(want))
    return "%s: %d of %d entries differ, first: entry %d got %r, model %r" % (
        name, len(bad), len(want), bad[0] if len(bad) else -1, got[bad[0]] if len(bad) else None, want[bad[0]] if len(bad) else None)


# ---- PageRank ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PR_NAMES)
def test_pagerank_is_the_model_bit_for_bit(name):
    V, off, adj = next(f for f in am.pagerank_fixtures() if f[0] == name)[1:]
    want, wit, _ = am.pagerank_of(name, "device")
    dev = pgq.DeviceCSR(V, off, adj)
    ids = np.arange(V + 2, dtype=np.int64)
    out, ok, it = dev.pagerank(ids)
    assert ok.all() and it == wit, (name, it, wit)
    assert (bits(out) == bits(want)).all(), explain(name, out, want)
    again, ok, it = dev.pagerank(ids)  # the handle's table, not a second computation that could sum differently
    assert ok.all() and it == wit and (bits(again) == bits(want)).all(), name
    dev.close()


def test_pagerank_through_the_udf_state():
    name = "edges_V1023"  # 1025 entries: device mode and reference mode differ here
    V, off, adj = next(f for f in am.pagerank_fixtures() if f[0] == name)[1:]
    want, _, _ = am.pagerank_of(name, "device")
    assert (bits(want) != bits(am.pagerank_of(name, "reference")[0])).any()
    st = pgq.PgqState()
    st.build_csr(0, V, *edge_table(V, off, adj))
    out, ok = st.pagerank(0, np.concatenate([np.arange(V + 2), [-1, V + 2]]))
    assert ok[:V + 2].all() and not ok[V + 2:].any()
    assert (bits(out[:V + 2]) == bits(want)).all(), explain(name, out[:V + 2], want)
    st.delete_csr(0)


# ---- weakly connected components ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f[0] for f in am.wcc_fixtures()])
def test_wcc_ids_are_the_oracles_and_a_partition(name):
    V, s, d = next(f for f in am.wcc_fixtures() if f[0] == name)[1:]
    off, adj = am.csr(V, s, d)
    st = pgq.PgqState()
    st.build_csr(0, V, s, d)
    if len(s) == 0:  # no edge chunk ever arrives, and a CSR whose edge step never ran is refused: a chunk of zero rows runs it
        st.create_csr_edge(0, V, 0, 0, s, d, s)
    ids = np.arange(V + 2, dtype=np.int64)
    out, ok = st.weakly_connected_component(0, ids)
    st.delete_csr(0)
    want, wok = OracleCSR.adopt(V, off, adj if len(adj) else np.zeros(1, dtype=np.int64)).weakly_connected_component(ids)
    assert ok.all() and wok.all()
    assert (out == want).all(), "%s: %d ids differ from the oracle's" % (name, int((out != want).sum()))
    # without the oracle: the ids induce scipy's partition, and every id is a vertex of the component it names
    ncomp, label = connected_components(coo_matrix((np.ones(len(s)), (s, d)), shape=(V, V)), directed=False)
    comp = out[:V]
    assert ((comp >= 0) & (comp < V)).all() and (label[comp] == label).all(), name
    assert len(np.unique(comp)) == ncomp and (comp[comp] == comp).all(), name
    assert out[V] == V and out[V + 1] == comp[0], name  # the two trailing forest entries (weakly_connected_component.cpp:77-96)


# ---- local clustering coefficient ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(am.LCC_GADGETS))
def test_lcc_count_above_2_to_24(kernel):
    import torch
    p, q = am.LCC_GADGETS[kernel]
    V, off, adj = am.lcc_gadget(p, q)
    rows, valid = am.LCC_ROWS, am.LCC_ROWS >= 0
    want = am.lcc(V, off, adj, rows)
    ora = OracleCSR.adopt(V, off, adj).local_clustering_coefficient(rows[valid])
    assert (want[valid].view(np.uint32) == ora.view(np.uint32)).all()
    assert want[0] > 1 and am.lcc_count(V, off, adj, 0) > 1 << 24 and off[3] - off[2] == 2
    dev = pgq.DeviceCSR(V, off, adj)
    out, ok = dev.local_clustering_coefficient(np.where(valid, rows, 0), src_valid=valid)  # chunk form
    assert (ok == valid).all() and (out[valid].view(np.uint32) == want[valid].view(np.uint32)).all(), (kernel, out, want)
    t_rows = torch.from_numpy(rows).cuda()  # bulk form: device arrays, -1 marks a NULL row
    t_out = torch.full((len(rows),), -1.0, dtype=torch.float32, device="cuda")
    rc = dev.L.pgq_local_clustering_coefficient_bulk_device(dev.h, len(rows), C.c_void_p(t_rows.data_ptr()), C.c_void_p(t_out.data_ptr()))
    torch.cuda.synchronize()
    assert rc == 0 and (t_out.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all(), (kernel, t_out.cpu().numpy(), want)
    dev.close()
    st = pgq.PgqState()
    st.build_csr(0, V, *edge_table(V, off, adj))
    out, ok = st.local_clustering_coefficient(0, rows[valid])
    st.delete_csr(0)
    assert ok.all() and (out.view(np.uint32) == want[valid].view(np.uint32)).all(), (kernel, out, want)
