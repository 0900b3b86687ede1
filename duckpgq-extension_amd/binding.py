"""ctypes binding of libpgq_hip.so / libpgq_udf.so (no compute here — see include/pgq_hip.h, include/pgq_udf.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
KCLASS_MAX = 16


class PgqError(RuntimeError):
    pass


class Vec(C.Structure):
    """pgq_vec_t: DuckDB UnifiedVectorFormat (data, optional selection, optional validity words)."""
    _fields_ = [("data", C.c_void_p), ("sel", C.c_void_p), ("validity", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("batches", C.c_int64), ("levels", C.c_int64), ("push_levels", C.c_int64),
                ("pull_levels", C.c_int64), ("edges_scanned", C.c_int64), ("word_gathers", C.c_int64),
                ("frontier_vertices", C.c_int64), ("unique_sources", C.c_int64), ("pairs", C.c_int64),
                ("deferred_pairs", C.c_int64), ("meet_pairs", C.c_int64),
                ("algo_bytes", C.c_double * KCLASS_MAX), ("kernel_ms", C.c_double * KCLASS_MAX),
                ("launches", C.c_int64 * KCLASS_MAX), ("spec_batches", C.c_int64), ("spec_levels", C.c_int64),
                ("spec_aborts", C.c_int64), ("host_waits", C.c_int64), ("ball_segments", C.c_int64),
                ("ball_calls", C.c_int64), ("lds_map_launches", C.c_int64 * KCLASS_MAX)]


def lib_paths():
    # PGQ_HIP_LIB: another build of the device library (tuning sweeps compare compile-time variants); the product path is csrc/
    return os.environ.get("PGQ_HIP_LIB") or os.path.join(_CSRC, "libpgq_hip.so"), os.path.join(_CSRC, "libpgq_udf.so")


def build_native(force=False):
    """Compile csrc/ for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", _CSRC, "all"]
    if force:
        args.append("-B")
    subprocess.check_call(args)


# The C signatures of the walk family (include/pgq_hip.h, include/pgq_udf.h), in pieces: the rows, the form's scalars, its per-row
# outputs, and for a list form the nested lists.
_P, _I = C.c_void_p, C.c_int64
_CHUNK_ROWS = (_P, _I, _I, Vec, Vec)  # csr, V, n, src, dst (the UDFs: state and id in the handle's place)
_BULK_ROWS = (_P, _I, _P, _P)  # csr, n, d_src, d_dst
# out_path_offset, out_path_length, out_path_total, out_child, out_child_len
_CHUNK_LISTS = (C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_uint64), C.POINTER(_P), C.POINTER(C.c_uint64))
# d_path_offset, d_path_hops, path_cap, d_child, child_cap, paths_used, child_used
_BULK_LISTS = (_P, _P, _I, _P, _I, C.POINTER(_I), C.POINTER(_I))
# name -> (scalars, per-row outputs of the chunk form, of the bulk form, a list form?)
_WALK_FORMS = {"walk_count": ((_I, _I), 2, 1, False),
               "walk_length": ((_I, _I), 2, 1, False),
               "k_shortest_walks": ((_I, _I, _I), 3, 4, True),
               "walk_count_mode": ((_I, _I, _I, C.c_int), 2, 1, False),
               "k_shortest_walks_mode": ((_I, _I, _I, C.c_int), 3, 4, True),
               "k_shortest_groups": ((_I, _I, _I, _I, C.c_int), 4, 5, True)}


def _walk_argtypes(L, prefix, rows, bulk):
    for name, (scalars, chunk_outs, bulk_outs, lists) in _WALK_FORMS.items():
        getattr(L, prefix + name).argtypes = list(rows + scalars + (_P,) * chunk_outs + (_CHUNK_LISTS if lists else ()))
        if bulk:
            getattr(L, prefix + name + "_bulk_device").argtypes = list(_BULK_ROWS + scalars + (_P,) * bulk_outs + (_BULK_LISTS if lists else ()))


_hip = None
_udf = None


def load_hip():
    global _hip
    if _hip is not None:
        return _hip
    path = lib_paths()[0]
    if not os.path.exists(path):
        raise PgqError("libpgq_hip.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'`"
                       % path)
    L = C.CDLL(path, mode=C.RTLD_GLOBAL)
    L.pgq_last_error.restype = C.c_char_p
    L.pgq_version.restype = C.c_char_p
    L.pgq_kclass_name.restype = C.c_char_p
    L.pgq_kclass_name.argtypes = [C.c_int]
    L.pgq_init.argtypes = [C.c_int]
    L.pgq_csr_upload.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                 C.POINTER(C.c_void_p)]
    L.pgq_csr_upload_device.argtypes = L.pgq_csr_upload.argtypes
    L.pgq_csr_upload_ex.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint,
                                    C.POINTER(C.c_void_p)]
    L.pgq_csr_build_device.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.POINTER(C.c_void_p)]
    L.pgq_csr_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pgq_csr_free.argtypes = [C.c_void_p]
    for f in ("pgq_csr_num_vertices", "pgq_csr_num_edges", "pgq_csr_device_bytes"):
        getattr(L, f).restype = C.c_int64
        getattr(L, f).argtypes = [C.c_void_p]
    L.pgq_csr_w_type.argtypes = [C.c_void_p]
    L.pgq_csr_pack_k.argtypes = [C.c_void_p]
    L.pgq_csr_pack_order.argtypes = [C.c_void_p]
    L.pgq_csr_packed_list.restype = C.c_int64
    L.pgq_csr_packed_list.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64]
    L.pgq_csr_pull_layout_sizes.restype = C.c_int
    L.pgq_csr_pull_layout_sizes.argtypes = [C.c_void_p, C.c_void_p]
    L.pgq_csr_pull_layout.restype = C.c_int
    L.pgq_csr_pull_layout.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    L.pgq_csr_meet_layout_sizes.restype = C.c_int
    L.pgq_csr_meet_layout_sizes.argtypes = [C.c_void_p, C.c_void_p]
    L.pgq_csr_meet_layout.restype = C.c_int
    L.pgq_csr_meet_layout.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
    L.pgq_csr_hub_sizes.restype = C.c_int
    L.pgq_csr_hub_sizes.argtypes = [C.c_void_p, C.c_void_p]
    L.pgq_csr_hub_tables.restype = C.c_int
    L.pgq_csr_hub_tables.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
    L.pgq_csr_has_prepass_layout.argtypes = [C.c_void_p]
    L.pgq_debug_live_device_blocks.restype = C.c_int64
    L.pgq_debug_live_device_blocks.argtypes = []
    L.pgq_iterativelength.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, Vec, C.c_void_p, C.c_void_p]
    L.pgq_iterativelength_within.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_void_p, C.c_void_p]
    L.pgq_iterativelength_within_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                                         C.c_void_p]
    L.pgq_shortestpath.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, Vec, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pgq_shortestpath_within.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pgq_shortestpath_within_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.pgq_shortestpath_within_multi.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.pgq_cheapest_path_length.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, Vec, C.c_void_p, C.c_void_p]
    L.pgq_cheapest_path_length_within.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_void_p, C.c_void_p]
    L.pgq_cheapest_path_length_within_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                                              C.c_void_p, C.c_void_p]
    L.pgq_cheapest_path_length_within_multi.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                        C.c_void_p]
    L.pgq_iterativelength_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pgq_iterativelength_bidirectional_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pgq_traversed_edges_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pgq_shortestpath_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.pgq_cheapest_path_length_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]
    L.pgq_cheapest_path.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, Vec, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pgq_cheapest_path_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.pgq_cheapest_path_within.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pgq_cheapest_path_within_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.pgq_cheapest_walk_length.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    L.pgq_cheapest_walk_length_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                       C.c_void_p, C.c_void_p]
    L.pgq_cheapest_walk.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pgq_cheapest_walk_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.pgq_shortestpath_count.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_void_p, C.c_void_p]
    L.pgq_shortestpath_count_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.pgq_all_shortestpaths.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pgq_all_shortestpaths_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                    C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    _walk_argtypes(L, "pgq_", _CHUNK_ROWS, True)
    L.pgq_debug_mode_steps.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.pgq_local_clustering_coefficient.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, C.c_void_p, C.c_void_p]
    L.pgq_local_clustering_coefficient_bulk_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.pgq_pagerank.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, C.c_void_p, C.c_void_p]
    L.pgq_pagerank_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    L.pgq_iterativelength_multi.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pgq_shortestpath_multi.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.POINTER(C.c_int64)]
    L.pgq_cheapest_path_length_multi.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pgq_init_devices.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.pgq_init_mask.argtypes = [C.c_uint64]
    L.pgq_csr_replicate.argtypes = [C.c_void_p]
    L.pgq_set_option.argtypes = [C.c_char_p, C.c_char_p]
    L.pgq_get_option.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
    L.pgq_get_default_option.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
    L.pgq_csr_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    L.pgq_csr_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
    L.pgq_iterativelength_bidirectional.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, Vec, C.c_void_p, C.c_void_p]
    L.pgq_weakly_connected_component.argtypes = [C.c_void_p, C.c_int64, C.c_int64, Vec, C.c_void_p, C.c_void_p]
    L.pgq_weakly_connected_component_device.argtypes = [C.c_void_p, C.c_void_p]
    L.pgq_get_stats.argtypes = [C.POINTER(Stats)]
    L.pgq_get_stats_sized.argtypes = [C.POINTER(Stats), C.c_size_t]
    L.pgq_measure_copy_bandwidth.argtypes = [C.c_int64, C.c_int, C.POINTER(C.c_double)]
    _hip = L
    return L


def load_udf():
    global _udf
    if _udf is not None:
        return _udf
    load_hip()
    path = lib_paths()[1]
    if not os.path.exists(path):
        raise PgqError("libpgq_udf.so is not built (%s)" % path)
    L = C.CDLL(path)
    L.pgq_udf_last_error.restype = C.c_char_p
    L.pgq_state_new.restype = C.c_void_p
    L.pgq_state_free.argtypes = [C.c_void_p]
    L.pgq_state_query_end.argtypes = [C.c_void_p]
    L.pgq_udf_create_csr_vertex.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, Vec, Vec, C.c_void_p,
                                            C.c_void_p]
    L.pgq_udf_create_csr_edge.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, Vec, Vec,
                                          Vec, C.POINTER(Vec), C.c_int, C.c_void_p, C.c_void_p]
    L.pgq_udf_bind_search.argtypes = [C.c_void_p, C.c_int32]
    for f in ("pgq_udf_iterativelength", "pgq_udf_iterativelength2", "pgq_udf_iterativelengthbidirectional",
              "pgq_udf_cheapest_path_length",
              "pgq_udf_reachability"):
        getattr(L, f).argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, Vec, Vec, C.c_void_p, C.c_void_p]
    L.pgq_udf_iterativelength_within.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, Vec, Vec, C.c_int64,
                                                 C.c_void_p, C.c_void_p]
    L.pgq_udf_shortestpath.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, Vec, Vec, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pgq_udf_shortestpath_within.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pgq_udf_shortestpath_count.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_void_p,
                                             C.c_void_p]
    L.pgq_udf_all_shortestpaths.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    _walk_argtypes(L, "pgq_udf_", (C.c_void_p, C.c_int32) + _CHUNK_ROWS[1:], False)
    L.pgq_udf_bind_cheapest.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int)]
    L.pgq_udf_cheapest_path.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, Vec, Vec, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pgq_udf_cheapest_path_within.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pgq_udf_cheapest_path_length_within.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, Vec, Vec, C.c_int64,
                                                      C.c_void_p, C.c_void_p]
    L.pgq_udf_cheapest_walk_length.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_int64,
                                               C.c_void_p, C.c_void_p]
    L.pgq_udf_cheapest_walk.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, Vec, Vec, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for f in ("pgq_udf_local_clustering_coefficient", "pgq_udf_pagerank", "pgq_udf_weakly_connected_component"):
        getattr(L, f).argtypes = [C.c_void_p, C.c_int32, C.c_int64, Vec, C.c_void_p, C.c_void_p]
    L.pgq_udf_delete_csr.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int)]
    L.pgq_udf_csr_get_w_type.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    for f in ("pgq_udf_scan_csr_v", "pgq_udf_scan_csr_e", "pgq_udf_scan_csr_w"):
        getattr(L, f).restype = C.c_int64
        getattr(L, f).argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    L.pgq_udf_device_csr.restype = C.c_void_p
    L.pgq_udf_device_csr.argtypes = [C.c_void_p, C.c_int32]
    _udf = L
    return L


def _check(rc):
    if rc != 0:
        raise PgqError("pgq_hip error %d: %s" % (rc, load_hip().pgq_last_error().decode()))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def pack_validity(valid):
    valid = np.asarray(valid, dtype=bool)
    words = np.zeros((len(valid) + 63) // 64, dtype=np.uint64)
    idx = np.nonzero(valid)[0]
    np.bitwise_or.at(words, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return words


def unpack_validity(words, n):
    i = np.arange(n)
    return ((words[i // 64] >> (i % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)


def make_vec(data, sel=None, valid=None, keep=None):
    d = np.ascontiguousarray(data)
    s = None if sel is None else np.ascontiguousarray(sel, dtype=np.uint32)
    m = None if valid is None else pack_validity(valid)
    if keep is not None:
        keep.extend([d, s, m])
    return Vec(_p(d), _p(s), _p(m))


def set_option(key, value):
    _check(load_hip().pgq_set_option(str(key).encode(), str(value).encode()))


def get_default_option(key):
    """The value the library ships with (a process that sets nothing runs under it)."""
    v = C.c_double(0)
    _check(load_hip().pgq_get_default_option(str(key).encode(), C.byref(v)))
    return v.value


def get_option(key):
    v = C.c_double(0.0)
    _check(load_hip().pgq_get_option(str(key).encode(), C.byref(v)))
    return v.value


def kclass_names():
    L = load_hip()
    out = []
    for k in range(KCLASS_MAX):
        nm = L.pgq_kclass_name(k)
        if nm is None:
            break
        out.append(nm.decode())
    return out


def get_stats():
    st = Stats()
    _check(load_hip().pgq_get_stats_sized(C.byref(st), C.sizeof(st)))  # the library writes at most this mirror's size
    names = kclass_names()
    d = {f: getattr(st, f) for f, t in Stats._fields_ if t is C.c_int64}
    d["algo_bytes"] = {n: st.algo_bytes[i] for i, n in enumerate(names)}
    d["kernel_ms"] = {n: st.kernel_ms[i] for i, n in enumerate(names)}
    d["launches"] = {n: st.launches[i] for i, n in enumerate(names)}
    d["lds_map_launches"] = {n: st.lds_map_launches[i] for i, n in enumerate(names)}
    return d


def init_devices(devices):
    arr = (C.c_int * len(devices))(*devices)
    _check(load_hip().pgq_init_devices(arr, len(devices)))
    return load_hip().pgq_num_enabled_devices()


def reset_stats():
    _check(load_hip().pgq_reset_stats())


def live_device_blocks():
    """Device blocks handed out by the library's block cache and not freed yet (pgq_debug_live_device_blocks)."""
    return load_hip().pgq_debug_live_device_blocks()


# the path modes of k_shortest_walks / walk_count, numbered as the reference's PGQPathMode (include/pgq_hip.h: PGQ_MODE_*)
MODE_NONE, MODE_WALK, MODE_SIMPLE, MODE_TRAIL, MODE_ACYCLIC = range(5)


def mode_steps():
    """(total, row_max): the steps this thread's last path-mode call took over all rows and both passes, and the most one row took
    in one pass (pgq_debug_mode_steps); a step is one 64-entry in-list chunk examined or one descent."""
    total, row_max = C.c_int64(0), C.c_int64(0)
    _check(load_hip().pgq_debug_mode_steps(C.byref(total), C.byref(row_max)))
    return total.value, row_max.value


def copy_bandwidth_gbps(nbytes=1 << 30, iters=10):
    out = C.c_double(0)
    _check(load_hip().pgq_measure_copy_bandwidth(nbytes, iters, C.byref(out)))
    return out.value


def _lists(off, ln, valid, child):
    return [child[int(o):int(o) + int(l)].tolist() if ok else None for o, l, ok in zip(off, ln, valid)]


def _u64_copy(ptr, count):
    if not count:
        return np.zeros(0, dtype=np.uint64)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(count,)).copy()


def _all_shortestpaths(call, n, raw):
    """Runs call(first, npaths, validity words, &path_offset, &path_length, &path_total, &child, &child_len) and unpacks the
    LIST(LIST(BIGINT)) it fills: per row a list of paths (None for NULL rows).  raw=True: the vectors as DuckDB sees them —
    outer entries (first, npaths), validity words, inner entries (offset, length), child payload."""
    first = np.zeros(n, dtype=np.uint64)
    npaths = np.zeros(n, dtype=np.uint64)
    ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
    poff, plen, child = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ptotal, clen = C.c_uint64(), C.c_uint64()
    call(_p(first), _p(npaths), _p(ov), C.byref(poff), C.byref(plen), C.byref(ptotal), C.byref(child), C.byref(clen))
    po, pl = _u64_copy(poff, ptotal.value), _u64_copy(plen, ptotal.value)
    ch = _u64_copy(child, clen.value).view(np.int64)
    if raw:
        return first, npaths, ov, po, pl, ch
    valid = unpack_validity(ov, n)
    return [[ch[int(po[k]):int(po[k]) + int(pl[k])].tolist() for k in range(int(f), int(f) + int(c))] if ok else None
            for f, c, ok in zip(first, npaths, valid)]


def _grouped_shortestpaths(call, n, raw):
    """_all_shortestpaths for k_shortest_groups, whose call takes the groups per row behind npaths: (its result, ngroups)."""
    ngroups = np.zeros(n, dtype=np.uint64)
    return _all_shortestpaths(lambda first, npaths, *rest: call(first, npaths, _p(ngroups), *rest), n, raw), ngroups


class DeviceCSR:
    """pgq_csr_t: a CSR resident in HBM (include/pgq_hip.h)."""

    def __init__(self, V, offsets, adj, edge_ids=None, w=None, handle=None, lazy_edge_ids=False):
        self.L = load_hip()
        self.V = int(V)
        self.h = C.c_void_p(handle) if handle else None
        self._owned = handle is None
        if handle is None:
            _check(self.L.pgq_init(-1))
            offsets, adj = _i64(offsets), _i64(adj)
            eids = None if edge_ids is None else _i64(edge_ids)
            wtype = 0
            if w is not None:
                w = np.asarray(w)
                wtype = 2 if w.dtype.kind == "f" else 1
                w = np.ascontiguousarray(w, dtype=np.float64 if wtype == 2 else np.int64)
            if len(adj) == 0:
                adj = np.zeros(1, dtype=np.int64)
            h = C.c_void_p()
            if lazy_edge_ids:  # PGQ_UPLOAD_LAZY_EDGE_IDS: the array must outlive the handle — this object keeps it
                self._keep_eids = eids
                _check(self.L.pgq_csr_upload_ex(self.V, _p(offsets), _p(adj), _p(eids), _p(w), wtype, 1, C.byref(h)))
            else:
                _check(self.L.pgq_csr_upload(self.V, _p(offsets), _p(adj), _p(eids), _p(w), wtype, C.byref(h)))
            self.h = h

    @classmethod
    def from_device_ptrs(cls, V, d_offsets, d_adj, d_edge_ids=0, d_w=0, w_type=0):
        """Arrays already in HBM (e.g. torch tensors' data_ptr())."""
        self = cls.__new__(cls)
        self.L = load_hip()
        self.V = int(V)
        self._owned = True
        _check(self.L.pgq_init(-1))
        h = C.c_void_p()
        _check(self.L.pgq_csr_upload_device(self.V, C.c_void_p(d_offsets), C.c_void_p(d_adj),
                                            C.c_void_p(d_edge_ids or None), C.c_void_p(d_w or None), w_type,
                                            C.byref(h)))
        self.h = h
        return self

    @classmethod
    def build_from_device_rows(cls, V, n_rows, d_src, d_dst, d_edge_id=0, d_w=0, w_type=0):
        """create_csr_vertex/create_csr_edge on the GPU: edge-table rows (device pointers) -> device CSR."""
        self = cls.__new__(cls)
        self.L = load_hip()
        self.V = int(V)
        self._owned = True
        _check(self.L.pgq_init(-1))
        h = C.c_void_p()
        _check(self.L.pgq_csr_build_device(self.V, n_rows, C.c_void_p(d_src), C.c_void_p(d_dst),
                                           C.c_void_p(d_edge_id or None), C.c_void_p(d_w or None), w_type, C.byref(h)))
        self.h = h
        return self

    def download(self):
        """(offsets[V+1], adj[E], edge_ids[E], w or None) as numpy, reference layout."""
        E = self.num_edges
        off = np.zeros(self.V + 1, dtype=np.int64)
        adj = np.zeros(max(E, 1), dtype=np.int64)
        eid = np.zeros(max(E, 1), dtype=np.int64)
        wt = self.w_type
        w = None if wt == 0 else np.zeros(max(E, 1), dtype=np.int64 if wt == 1 else np.float64)
        _check(self.L.pgq_csr_download(self.h, _p(off), _p(adj), _p(eid), _p(w)))
        return off, adj[:E], eid[:E], (None if w is None else w[:E])

    def close(self):
        if getattr(self, "h", None) and self._owned:
            self.L.pgq_csr_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_edges(self):
        return self.L.pgq_csr_num_edges(self.h)

    @property
    def w_type(self):
        return self.L.pgq_csr_w_type(self.h)

    @property
    def device_bytes(self):
        return self.L.pgq_csr_device_bytes(self.h)

    @property
    def pack_k(self):
        """Ids per 16-byte group of the lists the pre-pass walks (6 / 5: bit-packed, 4: 32-bit)."""
        return self.L.pgq_csr_pack_k(self.h)

    @property
    def pack_order(self):
        """1: the packed lists are in degree order and walked heads first (option meet_pack_order at upload), else 0."""
        return self.L.pgq_csr_pack_order(self.h)

    def packed_list(self, direction, v):
        """Vertex v's bit-packed list, decoded, in the order the walks read it (0: forward, 1: reverse)."""
        n = self.L.pgq_csr_packed_list(self.h, direction, v, None, 0)
        _check(min(n, 0))
        out = np.zeros(max(int(n), 1), dtype=np.int32)
        _check(min(self.L.pgq_csr_packed_list(self.h, direction, v, out.ctypes.data, n), 0))
        return out[:n]

    def pull_layout(self):
        """The bottom-up work partition built at upload, as a dict of numpy arrays: parts [n, 2] (begin, end), hub_items
        [n, 3] (vertex, begin, end), hub_vertices, rown (one byte per in-slot) and rpk (one word per in-slot, or None where
        the upload did not build them)."""
        sizes = np.zeros(5, dtype=np.int64)
        _check(self.L.pgq_csr_pull_layout_sizes(self.h, _p(sizes)))
        n_parts, n_items, n_hubs, E, has_rpk = (int(x) for x in sizes)
        parts = np.zeros((max(n_parts, 1), 2), dtype=np.int32)
        items = np.zeros((max(n_items, 1), 3), dtype=np.int64)
        hubs = np.zeros(max(n_hubs, 1), dtype=np.int32)
        rown = np.zeros(max(E, 1), dtype=np.uint8)
        rpk = np.zeros(max(E, 1), dtype=np.uint32) if has_rpk else None
        _check(self.L.pgq_csr_pull_layout(self.h, _p(parts), _p(items), _p(hubs), _p(rown), _p(rpk)))
        return dict(parts=parts[:n_parts], hub_items=items[:n_items], hub_vertices=hubs[:n_hubs], rown=rown[:E],
                    rpk=None if rpk is None else rpk[:E])

    @property
    def has_prepass_layout(self):
        """1: the upload built the pair-centric layout (pgq_csr_has_prepass_layout), else 0."""
        return self.L.pgq_csr_has_prepass_layout(self.h)

    def meet_layout_sizes(self):
        """pgq_csr_meet_layout_sizes as a dict: groups, rgroups, pgroups, prgroups, pack_k, pack_align, pack_order, has_rhead,
        max_out_degree, max_in_degree, two_hop_mean."""
        sizes = np.zeros(11, dtype=np.int64)
        _check(self.L.pgq_csr_meet_layout_sizes(self.h, _p(sizes)))
        names = ("groups", "rgroups", "pgroups", "prgroups", "pack_k", "pack_align", "pack_order", "has_rhead",
                 "max_out_degree", "max_in_degree")
        d = {k: int(v) for k, v in zip(names, sizes)}
        d["two_hop_mean"] = float(sizes[10:11].view(np.float64)[0])
        return d

    def meet_layout(self, direction):
        """What the upload derived for the pair-centric and source-centric kernels in one direction (0: forward, 1: reverse), as
        a dict of numpy arrays: off [V + 1], adj [E], seg [V, 2] (first group, entries), padded [groups, 4], desc [E, 4], work
        [V], packed [packed groups, 4], rhead [V, 64] (direction 1), and the scalars of meet_layout_sizes().  None for an array
        the handle does not have."""
        s = self.meet_layout_sizes()
        V, E = self.V, self.num_edges
        layout = bool(self.has_prepass_layout)
        groups = s["rgroups" if direction else "groups"]
        pgroups = s["prgroups" if direction else "pgroups"]
        off = np.zeros(V + 1, dtype=np.int64)
        adj = np.zeros(max(E, 1), dtype=np.int32)
        seg = np.zeros((max(V, 1), 2), dtype=np.uint32) if layout else None
        padded = np.zeros((max(groups, 1), 4), dtype=np.int32) if layout else None
        desc = np.zeros((max(E, 1), 4), dtype=np.uint32) if layout else None
        work = np.zeros(max(V, 1), dtype=np.uint32) if layout else None
        packed = np.zeros((max(pgroups, 1), 4), dtype=np.uint32) if layout and s["pack_k"] > 4 else None
        rhead = np.zeros((max(V, 1), 64), dtype=np.uint32) if direction == 1 and s["has_rhead"] else None
        _check(self.L.pgq_csr_meet_layout(self.h, direction, _p(off), _p(adj), _p(seg), _p(padded), _p(desc), _p(work),
                                          _p(packed), _p(rhead)))
        cut = lambda a, n: None if a is None else a[:n]
        out = dict(off=off, adj=adj[:E], seg=cut(seg, V), padded=cut(padded, groups), desc=cut(desc, E), work=cut(work, V),
                   packed=cut(packed, pgroups), rhead=cut(rhead, V))
        out.update(s)
        return out

    def hub_sizes(self):
        """pgq_csr_hub_sizes as a dict: H (hub bits per table row), hubs (how many of them are in use), words (64-bit words
        per row).  A handle without hub tables raises PgqError (PGQ_ERR_UNSUPPORTED, -6)."""
        sizes = np.zeros(3, dtype=np.int64)
        _check(self.L.pgq_csr_hub_sizes(self.h, _p(sizes)))
        return dict(H=int(sizes[0]), hubs=int(sizes[1]), words=int(sizes[2]))

    def hub_tables(self, replica=-1):
        """The hub tables k_meet3 settles distance-3 and distance-4 rows from (pgq_csr_hub_tables), as a dict: ids [H] (the
        hubs in bit order, -1 in unused slots), hub1_out, hub1_in, hub2_out, hub2_in [V, words] of uint64, and the scalars of
        hub_sizes().  replica >= 0: the copy that replicate() made for that entry of the enabled device list.  A handle
        without tables raises PgqError (PGQ_ERR_UNSUPPORTED, -6)."""
        s = self.hub_sizes()
        ids = np.zeros(s["H"], dtype=np.int32)
        t = [np.zeros((max(self.V, 1), s["words"]), dtype=np.uint64) for _ in range(4)]
        _check(self.L.pgq_csr_hub_tables(self.h, int(replica), _p(ids), *(_p(x) for x in t)))
        out = dict(ids=ids, hub1_out=t[0][:self.V], hub1_in=t[1][:self.V], hub2_out=t[2][:self.V], hub2_in=t[3][:self.V])
        out.update(s)
        return out

    # -- chunk form (host arrays) ----------------------------------------------
    def _vecs(self, src, dst, src_valid, src_sel, dst_sel, dst_valid, keep):
        sv = make_vec(_i64(src), sel=src_sel, valid=src_valid, keep=keep)
        dv = make_vec(_i64(dst), sel=dst_sel, valid=dst_valid, keep=keep)
        n = len(src_sel) if src_sel is not None else len(src)
        return sv, dv, n

    def iterativelength(self, src, dst, src_valid=None, src_sel=None, dst_sel=None):
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, None, keep)
        out = np.zeros(n, dtype=np.int64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        _check(self.L.pgq_iterativelength(self.h, self.V, n, sv, dv, _p(out), _p(ov)))
        return out, unpack_validity(ov, n)

    def iterativelength_within(self, src, dst, max_hops, src_valid=None, src_sel=None, dst_sel=None):
        """iterativelength with the pattern's upper bound: rows more than max_hops hops apart are NULL."""
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, None, keep)
        out = np.zeros(n, dtype=np.int64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        _check(self.L.pgq_iterativelength_within(self.h, self.V, n, sv, dv, int(max_hops), _p(out), _p(ov)))
        return out, unpack_validity(ov, n)

    def iterativelength_bidirectional(self, src, dst, src_valid=None, src_sel=None, dst_sel=None):
        """iterativelength's hop counts by one bidirectional search per row (k_bibfs); rows over its caps go on to the lane batches."""
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, None, keep)
        out = np.zeros(n, dtype=np.int64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        _check(self.L.pgq_iterativelength_bidirectional(self.h, self.V, n, sv, dv, _p(out), _p(ov)))
        return out, unpack_validity(ov, n)

    def shortestpath(self, src, dst, src_valid=None, src_sel=None, dst_sel=None, raw=False, max_hops=None):
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, None, keep)
        off = np.zeros(n, dtype=np.uint64)
        ln = np.zeros(n, dtype=np.uint64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        child = C.c_void_p()
        clen = C.c_uint64()
        if max_hops is None:
            _check(self.L.pgq_shortestpath(self.h, self.V, n, sv, dv, _p(off), _p(ln), _p(ov), C.byref(child),
                                           C.byref(clen)))
        else:
            _check(self.L.pgq_shortestpath_within(self.h, self.V, n, sv, dv, int(max_hops), _p(off), _p(ln), _p(ov),
                                                  C.byref(child), C.byref(clen)))
        ch = np.zeros(0, dtype=np.int64)
        if clen.value:
            ch = np.ctypeslib.as_array(C.cast(child, C.POINTER(C.c_int64)), shape=(clen.value,)).copy()
        if raw:  # the LIST vector as DuckDB sees it: list_entry_t{offset,length} per row, validity words, child payload
            return off, ln, ov, ch
        return _lists(off, ln, unpack_validity(ov, n), ch)

    def shortestpath_within(self, src, dst, max_hops, src_valid=None, src_sel=None, dst_sel=None, raw=False):
        """shortestpath with the pattern's upper bound: rows whose path has more than max_hops hops are NULL and take no room
        in the child payload."""
        return self.shortestpath(src, dst, src_valid, src_sel, dst_sel, raw, max_hops=int(max_hops))

    def shortestpath_count(self, src, dst, max_hops, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None):
        """The number of shortest paths of at most max_hops hops per row (saturated at 2^63 - 1): 1 for src == dst, 0 for
        unreachable or farther rows, NULL for a NULL endpoint (include/pgq_hip.h)."""
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, dst_valid, keep)
        out = np.zeros(n, dtype=np.int64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        _check(self.L.pgq_shortestpath_count(self.h, self.V, n, sv, dv, int(max_hops), _p(out), _p(ov)))
        return out, unpack_validity(ov, n)

    def all_shortestpaths(self, src, dst, max_hops, max_paths, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None,
                          raw=False):
        """Per row the list of its first max_paths shortest paths of at most max_hops hops, each [src, e1, v1, ..., dst], in the
        contract's order (path 0 is shortestpath's); None for NULL rows.  raw=True: see _all_shortestpaths."""
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, dst_valid, keep)

        def call(*outs):
            _check(self.L.pgq_all_shortestpaths(self.h, self.V, n, sv, dv, int(max_hops), int(max_paths), *outs))

        return _all_shortestpaths(call, n, raw)

    def walk_count(self, src, dst, min_hops, max_hops, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None, limit=None,
                   path_mode=None):
        """The number of walks of min_hops..max_hops edges per row (saturated at 2^63 - 1): src == dst counts the empty walk when
        min_hops == 0 and every closed walk; 0 when there is none, NULL for a NULL endpoint (include/pgq_hip.h).
        With limit and path_mode (MODE_*): min(the walks the mode admits, limit) — pgq_walk_count_mode; both or neither."""
        if (limit is None) != (path_mode is None):
            raise PgqError("walk_count: limit and path_mode go together")
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, dst_valid, keep)
        out = np.zeros(n, dtype=np.int64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        if path_mode is None:
            _check(self.L.pgq_walk_count(self.h, self.V, n, sv, dv, int(min_hops), int(max_hops), _p(out), _p(ov)))
        else:
            _check(self.L.pgq_walk_count_mode(self.h, self.V, n, sv, dv, int(min_hops), int(max_hops), int(limit), int(path_mode), _p(out),
                                              _p(ov)))
        return out, unpack_validity(ov, n)

    def walk_length(self, src, dst, min_hops, max_hops, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None):
        """The length of the shortest walk of min_hops..max_hops edges per row; NULL when there is none and for a NULL endpoint.
        src == dst is not special (include/pgq_hip.h: pgq_walk_length).  `valid` is the filter of {lower,upper} in WALK mode."""
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, dst_valid, keep)
        out = np.zeros(n, dtype=np.int64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        _check(self.L.pgq_walk_length(self.h, self.V, n, sv, dv, int(min_hops), int(max_hops), _p(out), _p(ov)))
        return out, unpack_validity(ov, n)

    def k_shortest_walks(self, src, dst, min_hops, max_hops, k, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None,
                         raw=False, path_mode=None):
        """Per row the list of its first k walks of min_hops..max_hops edges, shorter walks first, each [x_0, e_1, x_1, ..., x_t],
        in the contract's order; None for rows without a walk and NULL rows.  raw=True: see _all_shortestpaths.
        path_mode (MODE_*): the first k walks the mode admits — pgq_k_shortest_walks_mode."""
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, dst_valid, keep)

        def call(*outs):
            if path_mode is not None:
                return _check(self.L.pgq_k_shortest_walks_mode(self.h, self.V, n, sv, dv, int(min_hops), int(max_hops), int(k), int(path_mode),
                                                               *outs))
            _check(self.L.pgq_k_shortest_walks(self.h, self.V, n, sv, dv, int(min_hops), int(max_hops), int(k), *outs))

        return _all_shortestpaths(call, n, raw)

    def k_shortest_groups(self, src, dst, min_hops, max_hops, groups, max_paths, path_mode=0, src_valid=None, dst_valid=None,
                          src_sel=None, dst_sel=None, raw=False):
        """SHORTEST k GROUP: per row every walk of its `groups` smallest distinct lengths in min_hops..max_hops that have a walk
        path_mode (MODE_*) admits, in k_shortest_walks' order, cut at max_paths walks; None for rows without one and NULL rows.
        Returns (lists, groups per row) — pgq_k_shortest_groups.  raw=True: see _all_shortestpaths."""
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, dst_valid, keep)

        def call(*outs):
            _check(self.L.pgq_k_shortest_groups(self.h, self.V, n, sv, dv, int(min_hops), int(max_hops), int(groups), int(max_paths),
                                                int(path_mode), *outs))

        return _grouped_shortestpaths(call, n, raw)

    def cheapest_path_length(self, src, dst, src_valid=None, dst_valid=None):
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, None, None, dst_valid, keep)
        out = np.zeros(n, dtype=np.int64 if self.w_type == 1 else np.float64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        _check(self.L.pgq_cheapest_path_length(self.h, self.V, n, sv, dv, _p(out), _p(ov)))
        return out, unpack_validity(ov, n)

    def cheapest_path_length_within(self, src, dst, max_hops, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None):
        """The cost of the cheapest walk of at most max_hops edges per row: another number than cheapest_path_length's, not
        that one with far rows NULL (include/pgq_hip.h)."""
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, dst_valid, keep)
        out = np.zeros(n, dtype=np.int64 if self.w_type == 1 else np.float64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        _check(self.L.pgq_cheapest_path_length_within(self.h, self.V, n, sv, dv, int(max_hops), _p(out), _p(ov)))
        return out, unpack_validity(ov, n)

    def cheapest_path(self, src, dst, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None, raw=False, max_hops=None):
        """The cheapest path itself as a list [src, e1, v1, ..., ek, dst] per row (None for NULL rows): hop-minimal among the
        cheapest paths, shortestpath's tie-breaks (include/pgq_hip.h).  raw=True: offsets, lengths, validity words, child.
        max_hops: the cheapest walk of at most that many edges instead (cheapest_path_within)."""
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, dst_valid, keep)
        off = np.zeros(n, dtype=np.uint64)
        ln = np.zeros(n, dtype=np.uint64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        child = C.c_void_p()
        clen = C.c_uint64()
        if max_hops is None:
            _check(self.L.pgq_cheapest_path(self.h, self.V, n, sv, dv, _p(off), _p(ln), _p(ov), C.byref(child), C.byref(clen)))
        else:
            _check(self.L.pgq_cheapest_path_within(self.h, self.V, n, sv, dv, int(max_hops), _p(off), _p(ln), _p(ov),
                                                   C.byref(child), C.byref(clen)))
        ch = np.zeros(0, dtype=np.int64)
        if clen.value:
            ch = np.ctypeslib.as_array(C.cast(child, C.POINTER(C.c_int64)), shape=(clen.value,)).copy()
        if raw:
            return off, ln, ov, ch
        return _lists(off, ln, unpack_validity(ov, n), ch)

    def cheapest_path_within(self, src, dst, max_hops, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None, raw=False):
        """The cheapest walk of at most max_hops edges per row, as cheapest_path's list: the walk whose cost
        cheapest_path_length_within returns, not cheapest_path's list with long rows None (include/pgq_hip.h)."""
        return self.cheapest_path(src, dst, src_valid, dst_valid, src_sel, dst_sel, raw, max_hops=int(max_hops))

    def cheapest_walk_length(self, src, dst, min_hops, max_hops, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None):
        """The cost of the cheapest walk of min_hops..max_hops edges per row; src == dst is not special: its cheapest closed
        walk when min_hops >= 1 (include/pgq_hip.h: pgq_cheapest_walk_length).  Not a filter around cheapest_path_length_within."""
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, dst_valid, keep)
        out = np.zeros(n, dtype=np.int64 if self.w_type == 1 else np.float64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        _check(self.L.pgq_cheapest_walk_length(self.h, self.V, n, sv, dv, int(min_hops), int(max_hops), _p(out), _p(ov)))
        return out, unpack_validity(ov, n)

    def cheapest_walk(self, src, dst, min_hops, max_hops, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None, raw=False):
        """The cheapest walk of min_hops..max_hops edges per row as cheapest_path's list: the walk whose cost
        cheapest_walk_length returns (include/pgq_hip.h: pgq_cheapest_walk).  raw=True: offsets, lengths, validity words, child."""
        keep = []
        sv, dv, n = self._vecs(src, dst, src_valid, src_sel, dst_sel, dst_valid, keep)
        off = np.zeros(n, dtype=np.uint64)
        ln = np.zeros(n, dtype=np.uint64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        child = C.c_void_p()
        clen = C.c_uint64()
        _check(self.L.pgq_cheapest_walk(self.h, self.V, n, sv, dv, int(min_hops), int(max_hops), _p(off), _p(ln), _p(ov),
                                        C.byref(child), C.byref(clen)))
        ch = np.zeros(0, dtype=np.int64)
        if clen.value:
            ch = np.ctypeslib.as_array(C.cast(child, C.POINTER(C.c_int64)), shape=(clen.value,)).copy()
        if raw:
            return off, ln, ov, ch
        return _lists(off, ln, unpack_validity(ov, n), ch)

    # -- bulk form (device pointers; torch tensors supply them) ------------------
    def iterativelength_bulk_ptr(self, n, d_src, d_dst, d_out):
        _check(self.L.pgq_iterativelength_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst),
                                                      C.c_void_p(d_out)))

    def iterativelength_bidirectional_bulk_ptr(self, n, d_src, d_dst, d_out):
        _check(self.L.pgq_iterativelength_bidirectional_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst),
                                                                    C.c_void_p(d_out)))

    def iterativelength_within_bulk_ptr(self, n, d_src, d_dst, max_hops, d_out):
        _check(self.L.pgq_iterativelength_within_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst),
                                                             int(max_hops), C.c_void_p(d_out)))

    def local_clustering_coefficient(self, src, src_valid=None):
        keep = []
        sv = make_vec(_i64(src), valid=src_valid, keep=keep)
        n = len(src)
        out = np.zeros(n, dtype=np.float32)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        _check(self.L.pgq_local_clustering_coefficient(self.h, self.V, n, sv, _p(out), _p(ov)))
        return out, unpack_validity(ov, n)

    def pagerank(self, src):
        keep = []
        sv = make_vec(_i64(src), keep=keep)
        n = len(src)
        out = np.zeros(n, dtype=np.float64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        _check(self.L.pgq_pagerank(self.h, self.V, n, sv, _p(out), _p(ov)))
        it = C.c_int(0)
        _check(self.L.pgq_pagerank_device(self.h, None, C.byref(it)))
        return out, unpack_validity(ov, n), it.value

    def iterativelength_multi(self, src, dst):
        """Host arrays answered by every enabled device (pgq_init_devices): shards + in-library gather."""
        src, dst = _i64(src), _i64(dst)
        out = np.zeros(len(src), dtype=np.int64)
        _check(self.L.pgq_iterativelength_multi(self.h, len(src), _p(src), _p(dst), _p(out)))
        return out

    def shortestpath_multi(self, src, dst, max_hops=None):
        """Paths of host rows by every enabled device; returns (lengths, offsets, child) like the bulk form."""
        src, dst = _i64(src), _i64(dst)
        n = len(src)
        ln, off = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        used = C.c_int64(0)
        cap = max(1024, 16 * n)
        for _ in range(2):
            child = np.zeros(cap, dtype=np.int64)
            if max_hops is None:
                rc = self.L.pgq_shortestpath_multi(self.h, n, _p(src), _p(dst), _p(ln), _p(off), _p(child), cap, C.byref(used))
            else:
                rc = self.L.pgq_shortestpath_within_multi(self.h, n, _p(src), _p(dst), int(max_hops), _p(ln), _p(off),
                                                          _p(child), cap, C.byref(used))
            if rc == 0 or used.value <= cap:
                break
            cap = used.value  # too small: the call reported what it needs
        _check(rc)
        return ln, off, child[:used.value]

    def shortestpath_within_multi(self, src, dst, max_hops):
        """shortestpath_multi under the pattern's upper bound: only the rows within it have lists."""
        return self.shortestpath_multi(src, dst, max_hops=int(max_hops))

    def cheapest_path_length_multi(self, src, dst):
        src, dst = _i64(src), _i64(dst)
        n = len(src)
        out = np.zeros(n, dtype=np.int64 if self.w_type == 1 else np.float64)
        ok = np.zeros(n, dtype=np.uint8)
        _check(self.L.pgq_cheapest_path_length_multi(self.h, n, _p(src), _p(dst), _p(out), _p(ok)))
        return out, ok.astype(bool)

    def cheapest_path_length_within_multi(self, src, dst, max_hops):
        """cheapest_path_length_within of host rows by every enabled device."""
        src, dst = _i64(src), _i64(dst)
        n = len(src)
        out = np.zeros(n, dtype=np.int64 if self.w_type == 1 else np.float64)
        ok = np.zeros(n, dtype=np.uint8)
        _check(self.L.pgq_cheapest_path_length_within_multi(self.h, n, _p(src), _p(dst), int(max_hops), _p(out), _p(ok)))
        return out, ok.astype(bool)

    def replicate(self):
        _check(self.L.pgq_csr_replicate(self.h))

    def set_option(self, key, value):
        """An option of THIS handle only (pgq_csr_set_option); the process-wide set stays as it is."""
        _check(self.L.pgq_csr_set_option(self.h, str(key).encode(), str(value).encode()))

    def get_option(self, key):
        v = C.c_double(0.0)
        _check(self.L.pgq_csr_get_option(self.h, str(key).encode(), C.byref(v)))
        return v.value

    def traversed_edges_bulk_ptr(self, n, d_src, d_dst, d_out_len, d_out_te):
        _check(self.L.pgq_traversed_edges_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst),
                                                      C.c_void_p(d_out_len), C.c_void_p(d_out_te)))

    def shortestpath_bulk_ptr(self, n, d_src, d_dst, d_out_len, d_out_off, d_child, child_cap):
        used = C.c_int64(0)
        rc = self.L.pgq_shortestpath_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst), C.c_void_p(d_out_len),
                                                 C.c_void_p(d_out_off), C.c_void_p(d_child), child_cap, C.byref(used))
        return rc, used.value

    def shortestpath_within_bulk_ptr(self, n, d_src, d_dst, max_hops, d_out_len, d_out_off, d_child, child_cap):
        used = C.c_int64(0)
        rc = self.L.pgq_shortestpath_within_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst), int(max_hops),
                                                        C.c_void_p(d_out_len), C.c_void_p(d_out_off), C.c_void_p(d_child),
                                                        child_cap, C.byref(used))
        return rc, used.value

    def cheapest_bulk_ptr(self, n, d_src, d_dst, d_out, d_ok):
        _check(self.L.pgq_cheapest_path_length_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst),
                                                           C.c_void_p(d_out), C.c_void_p(d_ok)))

    def cheapest_path_bulk_ptr(self, n, d_src, d_dst, d_out_len, d_out_off, d_child, child_cap):
        """(status, elements needed): as shortestpath_bulk_ptr, the lists of the cheapest paths."""
        used = C.c_int64(0)
        rc = self.L.pgq_cheapest_path_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst), C.c_void_p(d_out_len),
                                                  C.c_void_p(d_out_off), C.c_void_p(d_child), child_cap, C.byref(used))
        return rc, used.value

    def cheapest_path_within_bulk_ptr(self, n, d_src, d_dst, max_hops, d_out_len, d_out_off, d_child, child_cap):
        """(status, elements needed): as cheapest_path_bulk_ptr, the cheapest walks of at most max_hops edges."""
        used = C.c_int64(0)
        rc = self.L.pgq_cheapest_path_within_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst), int(max_hops),
                                                         C.c_void_p(d_out_len), C.c_void_p(d_out_off), C.c_void_p(d_child),
                                                         child_cap, C.byref(used))
        return rc, used.value

    def shortestpath_count_bulk_ptr(self, n, d_src, d_dst, max_hops, d_out_count):
        _check(self.L.pgq_shortestpath_count_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst), int(max_hops),
                                                         C.c_void_p(d_out_count)))

    def all_shortestpaths_bulk_ptr(self, n, d_src, d_dst, max_hops, max_paths, d_out_len, d_out_count, d_out_first, d_out_npaths,
                                   d_path_offset, path_cap, d_child, child_cap):
        """(status, paths needed, elements needed): the capacity protocol of shortestpath_bulk_ptr for both buffers."""
        return self._lists_bulk(self.L.pgq_all_shortestpaths_bulk_device, n, d_src, d_dst, (max_hops, max_paths),
                                (d_out_len, d_out_count, d_out_first, d_out_npaths, d_path_offset), path_cap, d_child, child_cap)

    def _lists_bulk(self, fn, n, d_src, d_dst, scalars, arrays, path_cap, d_child, child_cap):
        """A bulk list form: fn(handle, n, d_src, d_dst, the scalars, the device arrays, path_cap, d_child, child_cap, &lists,
        &elements) -> (status, lists needed, elements needed)."""
        paths, used = C.c_int64(0), C.c_int64(0)
        rc = fn(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst), *[int(x) for x in scalars], *[C.c_void_p(a) for a in arrays], path_cap,
                C.c_void_p(d_child), child_cap, C.byref(paths), C.byref(used))
        return rc, paths.value, used.value

    def walk_count_bulk_ptr(self, n, d_src, d_dst, min_hops, max_hops, d_out_count):
        _check(self.L.pgq_walk_count_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst), int(min_hops), int(max_hops),
                                                 C.c_void_p(d_out_count)))

    def walk_length_bulk_ptr(self, n, d_src, d_dst, min_hops, max_hops, d_out_len):
        _check(self.L.pgq_walk_length_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst), int(min_hops), int(max_hops),
                                                  C.c_void_p(d_out_len)))

    def k_shortest_walks_bulk_ptr(self, n, d_src, d_dst, min_hops, max_hops, k, d_out_len, d_out_count, d_out_first, d_out_npaths,
                                  d_path_offset, d_path_hops, path_cap, d_child, child_cap):
        """(status, walks needed, elements needed): the capacity protocol of all_shortestpaths_bulk_ptr."""
        return self._lists_bulk(self.L.pgq_k_shortest_walks_bulk_device, n, d_src, d_dst, (min_hops, max_hops, k),
                                (d_out_len, d_out_count, d_out_first, d_out_npaths, d_path_offset, d_path_hops), path_cap, d_child, child_cap)

    def walk_count_mode_bulk_ptr(self, n, d_src, d_dst, min_hops, max_hops, limit, path_mode, d_out_count):
        _check(self.L.pgq_walk_count_mode_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst), int(min_hops), int(max_hops),
                                                      int(limit), int(path_mode), C.c_void_p(d_out_count)))

    def k_shortest_walks_mode_bulk_ptr(self, n, d_src, d_dst, min_hops, max_hops, k, path_mode, d_out_len, d_out_count, d_out_first,
                                       d_out_npaths, d_path_offset, d_path_hops, path_cap, d_child, child_cap):
        """(status, walks needed, elements needed): k_shortest_walks_bulk_ptr under a path mode."""
        return self._lists_bulk(self.L.pgq_k_shortest_walks_mode_bulk_device, n, d_src, d_dst, (min_hops, max_hops, k, path_mode),
                                (d_out_len, d_out_count, d_out_first, d_out_npaths, d_path_offset, d_path_hops), path_cap, d_child, child_cap)

    def k_shortest_groups_bulk_ptr(self, n, d_src, d_dst, min_hops, max_hops, groups, max_paths, path_mode, d_out_len, d_out_count,
                                   d_out_first, d_out_npaths, d_out_ngroups, d_path_offset, d_path_hops, path_cap, d_child, child_cap):
        """(status, walks needed, elements needed): k_shortest_walks_mode_bulk_ptr with groups and max_paths in k's place and the
        groups per row behind d_out_npaths."""
        return self._lists_bulk(self.L.pgq_k_shortest_groups_bulk_device, n, d_src, d_dst, (min_hops, max_hops, groups, max_paths, path_mode),
                                (d_out_len, d_out_count, d_out_first, d_out_npaths, d_out_ngroups, d_path_offset, d_path_hops), path_cap, d_child,
                                child_cap)

    def cheapest_walk_length_bulk_ptr(self, n, d_src, d_dst, min_hops, max_hops, d_out, d_ok):
        _check(self.L.pgq_cheapest_walk_length_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst), int(min_hops),
                                                           int(max_hops), C.c_void_p(d_out), C.c_void_p(d_ok)))

    def cheapest_walk_bulk_ptr(self, n, d_src, d_dst, min_hops, max_hops, d_out_len, d_out_off, d_child, child_cap):
        """(status, elements needed): as cheapest_path_within_bulk_ptr, the cheapest walks of min_hops..max_hops edges."""
        used = C.c_int64(0)
        rc = self.L.pgq_cheapest_walk_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst), int(min_hops), int(max_hops),
                                                  C.c_void_p(d_out_len), C.c_void_p(d_out_off), C.c_void_p(d_child), child_cap,
                                                  C.byref(used))
        return rc, used.value

    def cheapest_within_bulk_ptr(self, n, d_src, d_dst, max_hops, d_out, d_ok):
        _check(self.L.pgq_cheapest_path_length_within_bulk_device(self.h, n, C.c_void_p(d_src), C.c_void_p(d_dst),
                                                                  int(max_hops), C.c_void_p(d_out), C.c_void_p(d_ok)))


class PgqState:
    """Host mirror of DuckPGQState + the scalar UDFs (include/pgq_udf.h); one call == one DataChunk."""

    def __init__(self):
        self.U = load_udf()
        self.s = C.c_void_p(self.U.pgq_state_new())

    def __del__(self):
        if getattr(self, "s", None):
            self.U.pgq_state_free(self.s)
            self.s = None

    def _ck(self, rc):
        if rc != 0:
            raise PgqError(self.U.pgq_udf_last_error().decode())

    def query_end(self):
        self._ck(self.U.pgq_state_query_end(self.s))

    def create_csr_vertex(self, csr_id, V, dense_id, cnt):
        keep = []
        n = len(dense_id)
        out = np.zeros(n, dtype=np.int64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        self._ck(self.U.pgq_udf_create_csr_vertex(self.s, csr_id, V, n, make_vec(_i64(dense_id), keep=keep),
                                                  make_vec(_i64(cnt), keep=keep), _p(out), _p(ov)))
        return out

    def create_csr_edge(self, csr_id, V, e_sum, e_count, src, dst, eid, w=None, valid=None):
        keep = []
        n = len(src)
        out = np.zeros(n, dtype=np.int32)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        wv, wtype = None, 0
        if w is not None:
            w = np.asarray(w)
            wtype = 2 if w.dtype.kind == "f" else 1
            wvec = make_vec(np.ascontiguousarray(w, dtype=np.float64 if wtype == 2 else np.int64), keep=keep)
            wv = C.pointer(wvec)
            keep.append(wvec)
        self._ck(self.U.pgq_udf_create_csr_edge(self.s, csr_id, V, e_sum, e_count, n,
                                                make_vec(_i64(src), valid=valid, keep=keep),
                                                make_vec(_i64(dst), keep=keep), make_vec(_i64(eid), keep=keep), wv,
                                                wtype, _p(out), _p(ov)))
        return out, unpack_validity(ov, n)

    def build_csr(self, csr_id, V, src, dst, eid=None, w=None, chunk=2048):
        """The cte1 SQL of compressed_sparse_row.cpp:234-251, single-threaded: vertex degrees, then edge chunks."""
        src, dst = _i64(src), _i64(dst)
        eid = np.arange(len(src), dtype=np.int64) if eid is None else _i64(eid)
        cnt = np.bincount(src, minlength=V).astype(np.int64) if len(src) else np.zeros(V, dtype=np.int64)
        e_sum = 0
        for lo in range(0, V, chunk):
            e_sum += int(self.create_csr_vertex(csr_id, V, np.arange(lo, min(V, lo + chunk)), cnt[lo:lo + chunk]).sum())
        for lo in range(0, len(src), chunk):
            sl = slice(lo, lo + chunk)
            self.create_csr_edge(csr_id, V, e_sum, len(src), src[sl], dst[sl], eid[sl],
                                 None if w is None else np.asarray(w)[sl])
        return e_sum

    def bind_search(self, csr_id):
        self._ck(self.U.pgq_udf_bind_search(self.s, csr_id))

    @staticmethod
    def _rows(src, dst, src_valid, dst_valid, src_sel, dst_sel):
        """(n, the src vector, the dst vector, what keeps their memory alive) of a search call's rows"""
        keep = []
        sv = make_vec(_i64(src), sel=src_sel, valid=src_valid, keep=keep)
        dv = make_vec(_i64(dst), sel=dst_sel, valid=dst_valid, keep=keep)
        return (len(src_sel) if src_sel is not None else len(src)), sv, dv, keep

    def _search(self, fn, csr_id, V, src, dst, src_valid, src_sel, dst_sel, dst_valid, out):
        n, sv, dv, _keep = self._rows(src, dst, src_valid, dst_valid, src_sel, dst_sel)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        self._ck(fn(self.s, csr_id, V, n, sv, dv, _p(out), _p(ov)))
        return unpack_validity(ov, n)

    def iterativelength(self, csr_id, V, src, dst, src_valid=None, src_sel=None, dst_sel=None, variant=1):
        n = len(src_sel) if src_sel is not None else len(src)
        out = np.zeros(n, dtype=np.int64)
        fn = {1: self.U.pgq_udf_iterativelength, 2: self.U.pgq_udf_iterativelength2,
              3: self.U.pgq_udf_iterativelengthbidirectional}[variant]
        ok = self._search(fn, csr_id, V, src, dst, src_valid, src_sel, dst_sel, None, out)
        return out, ok

    def iterativelength_within(self, csr_id, V, src, dst, max_hops, src_valid=None, src_sel=None, dst_sel=None):
        n = len(src_sel) if src_sel is not None else len(src)
        out = np.zeros(n, dtype=np.int64)
        hops = int(max_hops)

        def fn(s, csr_id, V, n, sv, dv, out_p, ov_p):
            return self.U.pgq_udf_iterativelength_within(s, csr_id, V, n, sv, dv, hops, out_p, ov_p)

        ok = self._search(fn, csr_id, V, src, dst, src_valid, src_sel, dst_sel, None, out)
        return out, ok

    def reachability(self, csr_id, V, src, dst, src_valid=None):
        out = np.zeros(len(src), dtype=np.uint8)
        ok = self._search(self.U.pgq_udf_reachability, csr_id, V, src, dst, src_valid, None, None, None, out)
        return out.astype(bool), ok

    def shortestpath(self, csr_id, V, src, dst, src_valid=None, src_sel=None, dst_sel=None, max_hops=None):
        keep = []
        sv = make_vec(_i64(src), sel=src_sel, valid=src_valid, keep=keep)
        dv = make_vec(_i64(dst), sel=dst_sel, keep=keep)
        n = len(src_sel) if src_sel is not None else len(src)
        off = np.zeros(n, dtype=np.uint64)
        ln = np.zeros(n, dtype=np.uint64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        child = C.c_void_p()
        clen = C.c_uint64()
        if max_hops is None:
            self._ck(self.U.pgq_udf_shortestpath(self.s, csr_id, V, n, sv, dv, _p(off), _p(ln), _p(ov), C.byref(child),
                                                 C.byref(clen)))
        else:
            self._ck(self.U.pgq_udf_shortestpath_within(self.s, csr_id, V, n, sv, dv, int(max_hops), _p(off), _p(ln), _p(ov),
                                                        C.byref(child), C.byref(clen)))
        ch = np.zeros(0, dtype=np.int64)
        if clen.value:
            ch = np.ctypeslib.as_array(C.cast(child, C.POINTER(C.c_int64)), shape=(clen.value,)).copy()
        return _lists(off, ln, unpack_validity(ov, n), ch)

    def shortestpath_within(self, csr_id, V, src, dst, max_hops, src_valid=None, src_sel=None, dst_sel=None):
        return self.shortestpath(csr_id, V, src, dst, src_valid, src_sel, dst_sel, max_hops=int(max_hops))

    def shortestpath_count(self, csr_id, V, src, dst, max_hops, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None):
        n = len(src_sel) if src_sel is not None else len(src)
        out = np.zeros(n, dtype=np.int64)
        hops = int(max_hops)

        def fn(s, csr_id, V, n, sv, dv, out_p, ov_p):
            return self.U.pgq_udf_shortestpath_count(s, csr_id, V, n, sv, dv, hops, out_p, ov_p)

        ok = self._search(fn, csr_id, V, src, dst, src_valid, src_sel, dst_sel, dst_valid, out)
        return out, ok

    def all_shortestpaths(self, csr_id, V, src, dst, max_hops, max_paths, src_valid=None, dst_valid=None, src_sel=None,
                          dst_sel=None, raw=False):
        n, sv, dv, _keep = self._rows(src, dst, src_valid, dst_valid, src_sel, dst_sel)

        def call(*outs):
            self._ck(self.U.pgq_udf_all_shortestpaths(self.s, csr_id, V, n, sv, dv, int(max_hops), int(max_paths), *outs))

        return _all_shortestpaths(call, n, raw)

    def walk_count(self, csr_id, V, src, dst, min_hops, max_hops, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None,
                   limit=None, path_mode=None):
        if (limit is None) != (path_mode is None):
            raise PgqError("walk_count: limit and path_mode go together")
        n = len(src_sel) if src_sel is not None else len(src)
        out = np.zeros(n, dtype=np.int64)
        lo, hi = int(min_hops), int(max_hops)

        def fn(s, csr_id, V, n, sv, dv, out_p, ov_p):
            if path_mode is not None:
                return self.U.pgq_udf_walk_count_mode(s, csr_id, V, n, sv, dv, lo, hi, int(limit), int(path_mode), out_p, ov_p)
            return self.U.pgq_udf_walk_count(s, csr_id, V, n, sv, dv, lo, hi, out_p, ov_p)

        ok = self._search(fn, csr_id, V, src, dst, src_valid, src_sel, dst_sel, dst_valid, out)
        return out, ok

    def walk_length(self, csr_id, V, src, dst, min_hops, max_hops, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None):
        n = len(src_sel) if src_sel is not None else len(src)
        out = np.zeros(n, dtype=np.int64)
        lo, hi = int(min_hops), int(max_hops)

        def fn(s, csr_id, V, n, sv, dv, out_p, ov_p):
            return self.U.pgq_udf_walk_length(s, csr_id, V, n, sv, dv, lo, hi, out_p, ov_p)

        ok = self._search(fn, csr_id, V, src, dst, src_valid, src_sel, dst_sel, dst_valid, out)
        return out, ok

    def k_shortest_walks(self, csr_id, V, src, dst, min_hops, max_hops, k, src_valid=None, dst_valid=None, src_sel=None,
                         dst_sel=None, raw=False, path_mode=None):
        n, sv, dv, _keep = self._rows(src, dst, src_valid, dst_valid, src_sel, dst_sel)

        def call(*outs):
            if path_mode is not None:
                return self._ck(self.U.pgq_udf_k_shortest_walks_mode(self.s, csr_id, V, n, sv, dv, int(min_hops), int(max_hops), int(k),
                                                                     int(path_mode), *outs))
            self._ck(self.U.pgq_udf_k_shortest_walks(self.s, csr_id, V, n, sv, dv, int(min_hops), int(max_hops), int(k), *outs))

        return _all_shortestpaths(call, n, raw)

    def k_shortest_groups(self, csr_id, V, src, dst, min_hops, max_hops, groups, max_paths, path_mode=0, src_valid=None,
                          dst_valid=None, src_sel=None, dst_sel=None, raw=False):
        n, sv, dv, _keep = self._rows(src, dst, src_valid, dst_valid, src_sel, dst_sel)

        def call(*outs):
            self._ck(self.U.pgq_udf_k_shortest_groups(self.s, csr_id, V, n, sv, dv, int(min_hops), int(max_hops), int(groups),
                                                      int(max_paths), int(path_mode), *outs))

        return _grouped_shortestpaths(call, n, raw)

    def bind_cheapest(self, csr_id):
        t = C.c_int(0)
        self._ck(self.U.pgq_udf_bind_cheapest(self.s, csr_id, C.byref(t)))
        return t.value

    def cheapest_path_length(self, csr_id, V, src, dst, src_valid=None, dst_valid=None):
        rt = self.bind_cheapest(csr_id)
        out = np.zeros(len(src), dtype=np.int64 if rt == 1 else np.float64)
        ok = self._search(self.U.pgq_udf_cheapest_path_length, csr_id, V, src, dst, src_valid, None, None, dst_valid,
                          out)
        return out, ok

    def cheapest_path_length_within(self, csr_id, V, src, dst, max_hops, src_valid=None, dst_valid=None, src_sel=None,
                                    dst_sel=None):
        rt = self.bind_cheapest(csr_id)
        n = len(src_sel) if src_sel is not None else len(src)
        out = np.zeros(n, dtype=np.int64 if rt == 1 else np.float64)
        hops = int(max_hops)

        def fn(s, csr_id, V, n, sv, dv, out_p, ov_p):
            return self.U.pgq_udf_cheapest_path_length_within(s, csr_id, V, n, sv, dv, hops, out_p, ov_p)

        ok = self._search(fn, csr_id, V, src, dst, src_valid, src_sel, dst_sel, dst_valid, out)
        return out, ok

    def cheapest_path(self, csr_id, V, src, dst, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None, max_hops=None):
        self.bind_cheapest(csr_id)
        keep = []
        sv = make_vec(_i64(src), sel=src_sel, valid=src_valid, keep=keep)
        dv = make_vec(_i64(dst), sel=dst_sel, valid=dst_valid, keep=keep)
        n = len(src_sel) if src_sel is not None else len(src)
        off = np.zeros(n, dtype=np.uint64)
        ln = np.zeros(n, dtype=np.uint64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        child = C.c_void_p()
        clen = C.c_uint64()
        if max_hops is None:
            self._ck(self.U.pgq_udf_cheapest_path(self.s, csr_id, V, n, sv, dv, _p(off), _p(ln), _p(ov), C.byref(child),
                                                  C.byref(clen)))
        else:
            self._ck(self.U.pgq_udf_cheapest_path_within(self.s, csr_id, V, n, sv, dv, int(max_hops), _p(off), _p(ln), _p(ov),
                                                         C.byref(child), C.byref(clen)))
        ch = np.zeros(0, dtype=np.int64)
        if clen.value:
            ch = np.ctypeslib.as_array(C.cast(child, C.POINTER(C.c_int64)), shape=(clen.value,)).copy()
        return _lists(off, ln, unpack_validity(ov, n), ch)

    def cheapest_path_within(self, csr_id, V, src, dst, max_hops, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None):
        return self.cheapest_path(csr_id, V, src, dst, src_valid, dst_valid, src_sel, dst_sel, max_hops=int(max_hops))

    def cheapest_walk_length(self, csr_id, V, src, dst, min_hops, max_hops, src_valid=None, dst_valid=None, src_sel=None,
                             dst_sel=None):
        rt = self.bind_cheapest(csr_id)
        n = len(src_sel) if src_sel is not None else len(src)
        out = np.zeros(n, dtype=np.int64 if rt == 1 else np.float64)
        lo, hi = int(min_hops), int(max_hops)

        def fn(s, csr_id, V, n, sv, dv, out_p, ov_p):
            return self.U.pgq_udf_cheapest_walk_length(s, csr_id, V, n, sv, dv, lo, hi, out_p, ov_p)

        ok = self._search(fn, csr_id, V, src, dst, src_valid, src_sel, dst_sel, dst_valid, out)
        return out, ok

    def cheapest_walk(self, csr_id, V, src, dst, min_hops, max_hops, src_valid=None, dst_valid=None, src_sel=None, dst_sel=None):
        self.bind_cheapest(csr_id)
        keep = []
        sv = make_vec(_i64(src), sel=src_sel, valid=src_valid, keep=keep)
        dv = make_vec(_i64(dst), sel=dst_sel, valid=dst_valid, keep=keep)
        n = len(src_sel) if src_sel is not None else len(src)
        off = np.zeros(n, dtype=np.uint64)
        ln = np.zeros(n, dtype=np.uint64)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        child = C.c_void_p()
        clen = C.c_uint64()
        self._ck(self.U.pgq_udf_cheapest_walk(self.s, csr_id, V, n, sv, dv, int(min_hops), int(max_hops), _p(off), _p(ln), _p(ov),
                                              C.byref(child), C.byref(clen)))
        ch = np.zeros(0, dtype=np.int64)
        if clen.value:
            ch = np.ctypeslib.as_array(C.cast(child, C.POINTER(C.c_int64)), shape=(clen.value,)).copy()
        return _lists(off, ln, unpack_validity(ov, n), ch)

    def _analytics(self, fn, csr_id, src, dtype):
        keep = []
        sv = make_vec(_i64(src), keep=keep)
        n = len(src)
        out = np.zeros(n, dtype=dtype)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        self._ck(fn(self.s, csr_id, n, sv, _p(out), _p(ov)))
        return out, unpack_validity(ov, n)

    def local_clustering_coefficient(self, csr_id, src):
        return self._analytics(self.U.pgq_udf_local_clustering_coefficient, csr_id, src, np.float32)

    def pagerank(self, csr_id, src):
        return self._analytics(self.U.pgq_udf_pagerank, csr_id, src, np.float64)

    def weakly_connected_component(self, csr_id, src):
        return self._analytics(self.U.pgq_udf_weakly_connected_component, csr_id, src, np.int64)

    def delete_csr(self, csr_id):
        f = C.c_int(0)
        self._ck(self.U.pgq_udf_delete_csr(self.s, csr_id, C.byref(f)))
        return bool(f.value)

    def csr_get_w_type(self, csr_id):
        t = C.c_int32(0)
        self._ck(self.U.pgq_udf_csr_get_w_type(self.s, csr_id, C.byref(t)))
        return t.value

    def get_csr_v(self, csr_id):
        n = self.U.pgq_udf_scan_csr_v(self.s, csr_id, None, 0)
        if n < 0:
            raise PgqError(self.U.pgq_udf_last_error().decode())
        out = np.zeros(n, dtype=np.int64)
        self.U.pgq_udf_scan_csr_v(self.s, csr_id, _p(out), n)
        return out

    def get_csr_e(self, csr_id):
        n = self.U.pgq_udf_scan_csr_e(self.s, csr_id, None, 0)
        if n < 0:
            raise PgqError(self.U.pgq_udf_last_error().decode())
        out = np.zeros(max(n, 1), dtype=np.int64)
        self.U.pgq_udf_scan_csr_e(self.s, csr_id, _p(out), n)
        return out[:n]

    def get_csr_w(self, csr_id):
        """get_csr_w (pgq_scan.cpp:113-153): int64 or float64 by the CSR's weight type."""
        n = self.U.pgq_udf_scan_csr_w(self.s, csr_id, None, 0)
        if n < 0:
            raise PgqError(self.U.pgq_udf_last_error().decode())
        out = np.zeros(max(n, 1), dtype=np.float64 if self.csr_get_w_type(csr_id) == 2 else np.int64)
        self.U.pgq_udf_scan_csr_w(self.s, csr_id, _p(out), n)
        return out[:n]

    def device_csr(self, csr_id):
        h = self.U.pgq_udf_device_csr(self.s, csr_id)
        if not h:
            raise PgqError(self.U.pgq_udf_last_error().decode())
        V = load_hip().pgq_csr_num_vertices(C.c_void_p(h))
        return DeviceCSR(V, None, None, handle=h)
