"""ctypes bindings of the two in-tree shared libraries.

libsatabsearch.so is the product: HIP kernels behind the C ABI of
include/satabsearch.h.  There is no Python or CPU stand-in for it: if the library
is missing, or no HIP device is usable, the calls raise.
"""
import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
# SAT_DEVICE_LIB lets kernel experiments (scripts/exp/) load an alternative build of the same ABI
DEVICE_LIB = os.environ.get("SAT_DEVICE_LIB") or os.path.join(PKG, "libsatabsearch.so")
HOST_LIB = os.path.join(PKG, "libsathost.so")

MAXDIM = 111
LABELSIZE = 8

# every symbol include/satabsearch.h declares
ABI_SYMBOLS = (
    "sat_last_error", "sat_abi_version", "sat_device_count", "sat_ctx_create", "sat_ctx_destroy",
    "sat_db_upload_packed", "sat_db_upload_search", "sat_db_upload_dense", "sat_db_size", "sat_query_set", "sat_search",
    "sat_search_async", "sat_device_scores", "sat_device_ssemaps", "sat_query_order", "sat_sync",
    "sat_search_timed", "sat_use_stream", "sat_use_own_stream", "sat_results", "sat_queries_set", "sat_query_count", "sat_topk",
    "sat_topk_hits", "sat_stat_d2h_bytes", "sat_debug_lds_layout", "sat_last_launch_info",
    "sat_multi_create", "sat_multi_destroy", "sat_multi_device_count", "sat_multi_gather_kind", "sat_multi_db_upload_packed",
    "sat_multi_shards", "sat_multi_queries_set", "sat_multi_search", "sat_multi_search_topk", "sat_multi_stat_d2h_bytes",
    "sat_search_matches", "sat_multi_search_matches",
    "sat_search_pairs", "sat_search_refine", "sat_multi_search_refine",
    "sat_hits_cutoff", "sat_multi_search_cutoff", "sat_multi_hits_cutoff",
    "sat_search_pairs_matches", "sat_multi_search_pairs_matches",
    "sat_score_histogram", "sat_stats_fit", "sat_stats_set",
    "sat_multi_score_histogram", "sat_multi_stats_set", "sat_multi_search_fit",
    "sat_search_pairs_polish", "sat_search_refine_polish", "sat_multi_search_pairs_polish", "sat_multi_search_refine_polish",
    "sat_polish_all_set", "sat_polish_all_get", "sat_results_base", "sat_multi_polish_all_set",
    "sat_queries_from_db", "sat_multi_queries_from_db", "sat_stat_query_h2d_bytes",
    "sat_queries_from_db_sses", "sat_multi_queries_from_db_sses",
    "sat_cluster_begin", "sat_cluster_add", "sat_cluster_labels", "sat_cluster_end",
    "sat_multi_search_only", "sat_multi_cluster_begin", "sat_multi_cluster_add", "sat_multi_cluster_labels",
    "sat_cluster_begin_levels", "sat_cluster_add_levels", "sat_cluster_labels_levels",
    "sat_multi_cluster_begin_levels", "sat_multi_cluster_add_levels", "sat_multi_cluster_labels_levels",
    "sat_eval_classes", "sat_eval_rows", "sat_eval_tables", "sat_multi_eval_classes", "sat_multi_eval_rows",
    "sat_cover_begin", "sat_cover_add", "sat_cover_solve", "sat_cover_end",
    "sat_multi_cover_begin", "sat_multi_cover_add", "sat_multi_cover_solve",
    "sat_profile_rows", "sat_multi_profile_rows",
    "sat_baseline_keep", "sat_baseline_drop", "sat_baseline_results", "sat_reorder_hits", "sat_search_reordered",
    "sat_multi_baseline_keep", "sat_multi_baseline_drop", "sat_multi_baseline_results", "sat_multi_reorder_hits",
    "sat_multi_search_reordered",
    "sat_search_exact", "sat_exact_results", "sat_exact_stats",
    "sat_multi_search_exact", "sat_multi_exact_results", "sat_multi_exact_stats",
    "sat_reach_begin", "sat_reach_add", "sat_reach_frontier", "sat_reach_rows", "sat_reach_end", "sat_search_reach",
    "sat_multi_reach_begin", "sat_multi_reach_add", "sat_multi_reach_frontier", "sat_multi_reach_rows",
    "sat_multi_reach_end", "sat_multi_search_reach",
)

MAX_CLUSTER_LEVELS = 8
# rounds of the cover's solve queued between two looks at its `done` flag (SAT_COVER_ROUND_BATCH of include/satabsearch.h)
COVER_ROUND_BATCH = 64
# rows of one query a block of eval_histogram (csrc/sat_eval.hip: kEvalRows) counts, and the bins a side its LDS holds
EVAL_BLOCK_ROWS = 4096
EVAL_WINDOW_BINS = 2048
STAT_BINS = 4096
# SAT_EXACT_MAX_QUERY and SAT_EXACT_DEFAULT_NODES of include/satabsearch.h
EXACT_MAX_QUERY = 16
EXACT_DEFAULT_NODES = 1 << 18
STAT_BINS_PER_UNIT = 256
# the key of the transitive search (csrc/host/sat_reach.h) and the stop reasons of sat_search_reach
REACH_UNREACHED = 0xFFFFFFFFFFFFFFFF
REACH_NO_PARENT = 0x7FFFFFF
REACH_MAX_DEPTH = 62
REACH_EXHAUSTED, REACH_DEPTH, REACH_BUDGET = 0, 1, 2


class SatError(RuntimeError):
    pass


class Hit(C.Structure):
    """struct sat_hit of include/satabsearch.h"""
    _fields_ = [("entry", C.c_int32), ("score", C.c_int32), ("norm2", C.c_double), ("zscore", C.c_double),
                ("pvalue", C.c_double)]


class ReorderHit(C.Structure):
    """struct sat_reorder_hit of include/satabsearch.h, 64 bytes"""
    _fields_ = [("hit", Hit), ("base_pvalue", C.c_double), ("base_score", C.c_int32), ("kind", C.c_int32),
                ("matched", C.c_int32), ("descents", C.c_int32), ("cut", C.c_int32), ("pad", C.c_int32)]


class Fit(C.Structure):
    """struct sat_fit of include/satabsearch.h"""
    _fields_ = [("a", C.c_double), ("b", C.c_double), ("rows", C.c_int32), ("censored", C.c_int32),
                ("below", C.c_int32), ("fitted", C.c_int32)]


class Eval(C.Structure):
    """struct sat_eval of include/satabsearch.h (sat_eval_row of csrc/host/sat_eval.h)"""
    _fields_ = [("u2", C.c_uint64), ("t2", C.c_uint64), ("positives", C.c_int32), ("negatives", C.c_int32),
                ("n_used", C.c_int32), ("query_class", C.c_int32)]


class ExactStat(C.Structure):
    """struct sat_exact_stat of include/satabsearch.h, 40 bytes"""
    _fields_ = [("rows", C.c_int64), ("proven", C.c_int64), ("improved", C.c_int64), ("gain", C.c_int64),
                ("nodes", C.c_uint64)]


class ReachRow(C.Structure):
    """struct sat_reach_row of include/satabsearch.h (sat_reach_rec of csrc/host/sat_reach.h), 20 bytes"""
    _fields_ = [("node", C.c_int32), ("depth", C.c_int32), ("parent", C.c_int32), ("support", C.c_int32),
                ("pvalue", C.c_float)]


class ReachInfo(C.Structure):
    """struct sat_reach_info of include/satabsearch.h, 32 bytes"""
    _fields_ = [("levels", C.c_int32), ("queries", C.c_int32), ("reached", C.c_int32), ("stop", C.c_int32),
                ("search_ms", C.c_double), ("pass_ms", C.c_double)]


class StructSetC(C.Structure):
    """struct sat_struct_set of csrc/host/sat_parse.h"""
    _fields_ = [
        ("count", C.c_int), ("capacity", C.c_int),
        ("cells", C.c_int64), ("cells_cap", C.c_int64),
        ("order", C.POINTER(C.c_int)), ("name", C.POINTER(C.c_char)),
        ("cell_off", C.POINTER(C.c_int64)), ("tab", C.POINTER(C.c_uint8)),
        ("dist", C.POINTER(C.c_float)), ("skipped", C.c_int),
    ]


_device = None
_host = None


def device_lib():
    """Load libsatabsearch.so (raises SatError when it has not been built)."""
    global _device
    if _device is None:
        if not os.path.exists(DEVICE_LIB):
            raise SatError(f"{DEVICE_LIB} is missing: run `python -m cuda_satabsearch_amd.build` "
                           "(the GPU search has no fallback implementation)")
        lib = C.CDLL(DEVICE_LIB)
        lib.sat_last_error.restype = C.c_char_p
        lib.sat_abi_version.restype = C.c_int
        lib.sat_device_count.restype = C.c_int
        lib.sat_ctx_create.restype = C.c_void_p
        lib.sat_ctx_create.argtypes = [C.c_int, C.c_uint64]
        lib.sat_ctx_destroy.argtypes = [C.c_void_p]
        lib.sat_ctx_destroy.restype = None
        lib.sat_db_upload_packed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
        lib.sat_db_upload_search.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        lib.sat_db_upload_dense.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_void_p]
        lib.sat_db_size.argtypes = [C.c_void_p]
        lib.sat_query_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_uint32]
        lib.sat_search.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_double)]
        lib.sat_search_async.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        lib.sat_use_stream.argtypes = [C.c_void_p, C.c_void_p]
        lib.sat_use_own_stream.argtypes = [C.c_void_p]
        lib.sat_results.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.sat_queries_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_uint32]
        lib.sat_query_count.argtypes = [C.c_void_p]
        lib.sat_topk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.sat_topk_hits.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.sat_stat_d2h_bytes.argtypes = [C.c_void_p]
        lib.sat_stat_d2h_bytes.restype = C.c_uint64
        lib.sat_last_launch_info.argtypes = [C.c_void_p]
        lib.sat_last_launch_info.restype = C.c_char_p
        lib.sat_debug_lds_layout.argtypes = [C.c_int] * 8 + [C.c_void_p]
        lib.sat_debug_lds_layout.restype = None
        lib.sat_multi_create.restype = C.c_void_p
        lib.sat_multi_create.argtypes = [C.c_int, C.c_void_p, C.c_uint64]
        lib.sat_multi_destroy.argtypes = [C.c_void_p]
        lib.sat_multi_destroy.restype = None
        lib.sat_multi_device_count.argtypes = [C.c_void_p]
        lib.sat_multi_gather_kind.argtypes = [C.c_void_p]
        lib.sat_multi_gather_kind.restype = C.c_char_p
        lib.sat_multi_db_upload_packed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sat_multi_shards.argtypes = [C.c_void_p, C.c_void_p]
        lib.sat_multi_queries_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
        lib.sat_multi_search.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        lib.sat_multi_search_topk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_double)]
        lib.sat_search_matches.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.POINTER(C.c_double)]
        lib.sat_multi_search_matches.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        lib.sat_search_pairs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        lib.sat_search_pairs_matches.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        lib.sat_multi_search_pairs_matches.argtypes = lib.sat_search_pairs_matches.argtypes
        lib.sat_search_refine.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sat_multi_search_refine.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                                C.POINTER(C.c_double)]
        lib.sat_search_pairs_polish.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        lib.sat_multi_search_pairs_polish.argtypes = lib.sat_search_pairs_polish.argtypes
        lib.sat_search_refine_polish.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sat_multi_search_refine_polish.argtypes = lib.sat_search_refine_polish.argtypes + [C.POINTER(C.c_double)]
        # (a build of the parent commit loaded through SAT_DEVICE_LIB for an A/B run predates the whole-database polish)
        if hasattr(lib, "sat_polish_all_set"):
            lib.sat_polish_all_set.argtypes = [C.c_void_p, C.c_int]
            lib.sat_polish_all_get.argtypes = [C.c_void_p]
            lib.sat_results_base.argtypes = [C.c_void_p, C.c_void_p]
            lib.sat_multi_polish_all_set.argtypes = [C.c_void_p, C.c_int]
        # (as above: a build of the parent commit predates queries taken from the resident database)
        if hasattr(lib, "sat_queries_from_db"):
            lib.sat_queries_from_db.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
            lib.sat_multi_queries_from_db.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
            lib.sat_stat_query_h2d_bytes.argtypes = [C.c_void_p]
            lib.sat_stat_query_h2d_bytes.restype = C.c_uint64
            lib.sat_debug_query_blob.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]      # include/satabsearch_debug.h
            lib.sat_debug_query_blob.restype = C.c_longlong
        # (as above: a build of the parent commit predates the motif queries)
        if hasattr(lib, "sat_queries_from_db_sses"):
            lib.sat_queries_from_db_sses.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
            lib.sat_multi_queries_from_db_sses.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
            lib.sat_debug_multi_ctx.argtypes = [C.c_void_p, C.c_int]                          # include/satabsearch_debug.h
            lib.sat_debug_multi_ctx.restype = C.c_void_p
        # (as above: a build of the parent commit predates the clustering)
        if hasattr(lib, "sat_cluster_begin"):
            lib.sat_cluster_begin.argtypes = [C.c_void_p, C.c_int]
            lib.sat_cluster_add.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
            lib.sat_cluster_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.sat_cluster_end.argtypes = [C.c_void_p]
            lib.sat_multi_search_only.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
            lib.sat_multi_cluster_begin.argtypes = [C.c_void_p]
            lib.sat_multi_cluster_add.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
            lib.sat_multi_cluster_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # (as above: a build of the parent commit predates the leveled clustering)
        if hasattr(lib, "sat_cluster_begin_levels"):
            lib.sat_cluster_begin_levels.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
            lib.sat_cluster_add_levels.argtypes = [C.c_void_p, C.c_void_p]
            lib.sat_cluster_labels_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.sat_multi_cluster_begin_levels.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            lib.sat_multi_cluster_add_levels.argtypes = [C.c_void_p, C.c_void_p]
            lib.sat_multi_cluster_labels_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # (as above: a build of the parent commit predates the evaluation against a classification)
        if hasattr(lib, "sat_eval_rows"):
            lib.sat_eval_classes.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            lib.sat_eval_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
            lib.sat_eval_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.sat_multi_eval_classes.argtypes = [C.c_void_p, C.c_void_p]
            lib.sat_multi_eval_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        # (as above: a build of the parent commit predates the cover)
        if hasattr(lib, "sat_cover_begin"):
            lib.sat_cover_begin.argtypes = [C.c_void_p, C.c_int]
            lib.sat_cover_add.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
            lib.sat_cover_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.sat_cover_end.argtypes = [C.c_void_p]
            lib.sat_multi_cover_begin.argtypes = [C.c_void_p]
            lib.sat_multi_cover_add.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
            lib.sat_multi_cover_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # (as above: a build of the parent commit predates the profile)
        if hasattr(lib, "sat_profile_rows"):
            lib.sat_profile_rows.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.sat_multi_profile_rows.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # (as above: a build of the parent commit predates the reordered hits)
        if hasattr(lib, "sat_reorder_hits"):
            for name in ("sat_baseline_keep", "sat_baseline_drop", "sat_multi_baseline_keep", "sat_multi_baseline_drop"):
                getattr(lib, name).argtypes = [C.c_void_p]
            lib.sat_baseline_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            lib.sat_multi_baseline_results.argtypes = lib.sat_baseline_results.argtypes
            lib.sat_reorder_hits.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p]
            lib.sat_multi_reorder_hits.argtypes = lib.sat_reorder_hits.argtypes
            lib.sat_search_reordered.argtypes = [C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_double)]
            lib.sat_multi_search_reordered.argtypes = lib.sat_search_reordered.argtypes
            lib.sat_debug_baseline_shape.argtypes = [C.c_void_p, C.c_int, C.c_int]        # include/satabsearch_debug.h
        # (as above: a build of the parent commit predates the exact search)
        if hasattr(lib, "sat_search_exact"):
            lib.sat_search_exact.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_ulonglong, C.POINTER(C.c_double)]
            lib.sat_exact_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.sat_exact_stats.argtypes = [C.c_void_p, C.c_void_p]
            lib.sat_multi_search_exact.argtypes = lib.sat_search_exact.argtypes
            lib.sat_multi_exact_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.sat_multi_exact_stats.argtypes = [C.c_void_p, C.c_void_p]
        # (as above: a build of the parent commit predates the transitive search)
        if hasattr(lib, "sat_reach_begin"):
            lib.sat_reach_begin.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
            lib.sat_reach_add.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p]
            lib.sat_reach_frontier.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32)]
            lib.sat_reach_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int32)]
            lib.sat_reach_end.argtypes = [C.c_void_p]
            lib.sat_search_reach.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                             C.c_double, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(ReachInfo)]
            lib.sat_multi_reach_begin.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            lib.sat_multi_reach_add.argtypes = lib.sat_reach_add.argtypes
            lib.sat_multi_reach_frontier.argtypes = lib.sat_reach_frontier.argtypes
            lib.sat_multi_reach_rows.argtypes = lib.sat_reach_rows.argtypes
            lib.sat_multi_reach_end.argtypes = [C.c_void_p]
            lib.sat_multi_search_reach.argtypes = lib.sat_search_reach.argtypes
        lib.sat_hits_cutoff.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.sat_multi_search_cutoff.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                                C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        lib.sat_multi_hits_cutoff.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.sat_multi_stat_d2h_bytes.argtypes = [C.c_void_p]
        lib.sat_multi_stat_d2h_bytes.restype = C.c_uint64
        lib.sat_score_histogram.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sat_stats_fit.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        lib.sat_stats_set.argtypes = [C.c_void_p, C.c_void_p]
        lib.sat_multi_score_histogram.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sat_multi_stats_set.argtypes = [C.c_void_p, C.c_void_p]
        lib.sat_multi_search_fit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p,
                                             C.POINTER(C.c_double)]
        lib.sat_debug_set_scores.argtypes = [C.c_void_p, C.c_void_p]          # include/satabsearch_debug.h
        # a test hook outside the ABI (include/satabsearch_debug.h): a build loaded through SAT_DEVICE_LIB may predate it
        if hasattr(lib, "sat_debug_sa_instances"):
            lib.sat_debug_sa_instances.argtypes = []
            lib.sat_debug_sa_instances.restype = C.c_char_p
        lib.sat_device_scores.argtypes = [C.c_void_p]
        lib.sat_device_scores.restype = C.c_void_p
        lib.sat_device_ssemaps.argtypes = [C.c_void_p]
        lib.sat_device_ssemaps.restype = C.c_void_p
        lib.sat_query_order.argtypes = [C.c_void_p]
        lib.sat_sync.argtypes = [C.c_void_p]
        lib.sat_search_timed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _device = lib
    return _device


def host_lib():
    """Load libsathost.so (ASCII reader + Gumbel statistics, plain C)."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise SatError(f"{HOST_LIB} is missing: run `python -m cuda_satabsearch_amd.build`")
        lib = C.CDLL(HOST_LIB)
        lib.sat_set_init.argtypes = [C.POINTER(StructSetC)]
        lib.sat_set_init.restype = None
        lib.sat_set_free.argtypes = [C.POINTER(StructSetC)]
        lib.sat_set_free.restype = None
        lib.sat_read_structures.argtypes = [C.c_void_p, C.POINTER(StructSetC), C.c_char_p]
        lib.sat_read_structures.restype = C.c_int
        lib.sat_read_structures_file.argtypes = [C.c_char_p, C.POINTER(StructSetC), C.c_char_p]
        lib.sat_read_structures_file.restype = C.c_int
        lib.sat_set_save_binary.argtypes = [C.POINTER(StructSetC), C.c_char_p]
        lib.sat_set_load_binary.argtypes = [C.c_char_p, C.POINTER(StructSetC)]
        lib.sat_set_write_ascii.argtypes = [C.POINTER(StructSetC), C.c_char_p]
        lib.sat_distance_cell.argtypes = [C.c_char_p]
        lib.sat_distance_cell.restype = C.c_float
        lib.sat_norm2.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.sat_norm2.restype = C.c_double
        lib.sat_z_gumbel_trunc.argtypes = [C.c_double]
        lib.sat_z_gumbel_trunc.restype = C.c_double
        lib.sat_pv_gumbel.argtypes = [C.c_double]
        lib.sat_pv_gumbel.restype = C.c_double
        lib.sat_stat_bin.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.sat_stat_bin.restype = C.c_int
        lib.sat_stat_histogram.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sat_stat_histogram.restype = None
        lib.sat_gumbel_fit_binned.argtypes = [C.c_void_p, C.c_double, C.POINTER(Fit)]
        lib.sat_gumbel_fit_binned.restype = C.c_int
        lib.sat_gumbel_fit_table.argtypes = [C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        lib.sat_gumbel_fit_table.restype = None
        lib.sat_entry_cost.argtypes = [C.c_int]
        lib.sat_entry_cost.restype = C.c_double
        lib.sat_shard_cuts.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        lib.sat_cluster_join.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.sat_cluster_reps.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sat_cluster_nested.argtypes = [C.c_int, C.c_int, C.c_void_p]
        lib.sat_eval_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Eval)]
        lib.sat_cover_sizes.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        lib.sat_cover_greedy.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sat_profile_core.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        lib.sat_map_kind.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sat_map_kind.restype = C.c_int32
        lib.sat_exact_host.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_int32, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sat_reach_pack_key.argtypes = [C.c_int32, C.c_double, C.c_int32]
        lib.sat_reach_pack_key.restype = C.c_uint64
        lib.sat_reach_unpack_key.argtypes = [C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        lib.sat_reach_unpack_key.restype = None
        lib.sat_reach_join.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sat_reach_decode.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _host = lib
    return _host


_libc = C.CDLL(None)
_libc.fopen.restype = C.c_void_p
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fclose.argtypes = [C.c_void_p]
_libc.fgets.restype = C.c_void_p
_libc.fgets.argtypes = [C.c_char_p, C.c_int, C.c_void_p]


def libc():
    return _libc
