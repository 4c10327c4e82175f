"""ctypes mirror of include/smx.h (structs and prototypes).

Shared by the product loader (``_lib.py``) and, in tests, by the CPU oracle
loader (``oracle/oracle.py``): both libraries use the same structs.
"""
from __future__ import annotations

import ctypes as C

c_i64p = C.POINTER(C.c_int64)


class SmxOps(C.Structure):
    _fields_ = [
        ("n_a", C.c_int64),
        ("n_b", C.c_int64),
        ("n_sym", C.c_int64),
        ("kind", C.c_void_p),
        ("ts", C.c_void_p),
        ("oid_hi", C.c_void_p),
        ("oid_lo", C.c_void_p),
        ("sym", C.c_void_p),
        ("v0", C.c_void_p),
        ("v1", C.c_void_p),
        ("b_gap", C.c_int64),
    ]


class SmxComposeOut(C.Structure):
    _fields_ = [
        ("order", C.c_void_p),
        ("addr", C.c_void_p),
        ("file", C.c_void_p),
        ("ctx", C.c_void_p),
        ("conflicts", C.c_void_p),
        ("conflict_cap", C.c_int64),
        ("counts", C.c_void_p),
    ]


class SmxBatch(C.Structure):
    _fields_ = [
        ("n_merges", C.c_int64),
        ("n_total", C.c_int64),
        ("n_sym", C.c_int64),
        ("off", C.c_void_p),
        ("n_a", C.c_void_p),
        ("kind", C.c_void_p),
        ("ts", C.c_void_p),
        ("oid_hi", C.c_void_p),
        ("oid_lo", C.c_void_p),
        ("sym", C.c_void_p),
        ("v0", C.c_void_p),
        ("v1", C.c_void_p),
        ("order", C.c_void_p),
        ("addr", C.c_void_p),
        ("file", C.c_void_p),
        ("ctx", C.c_void_p),
        ("conflicts", C.c_void_p),
        ("conf_off", C.c_void_p),
        ("counts", C.c_void_p),
        ("grid_cap", C.c_int32),
    ]


class SmxBatchShared(C.Structure):
    _fields_ = [
        ("n_merges", C.c_int64),
        ("n_total", C.c_int64),
        ("n_sym", C.c_int64),
        ("n_shared", C.c_int64),
        ("off", C.c_void_p),
        ("kind", C.c_void_p),
        ("ts", C.c_void_p),
        ("oid_hi", C.c_void_p),
        ("oid_lo", C.c_void_p),
        ("sym", C.c_void_p),
        ("v0", C.c_void_p),
        ("v1", C.c_void_p),
        ("order", C.c_void_p),
        ("addr", C.c_void_p),
        ("file", C.c_void_p),
        ("ctx", C.c_void_p),
        ("conflicts", C.c_void_p),
        ("conf_off", C.c_void_p),
        ("counts", C.c_void_p),
        ("grid_cap", C.c_int32),
        ("shared_is_b", C.c_int32),
    ]


class SmxScreen(C.Structure):
    _fields_ = [
        ("n_logs", C.c_int64),
        ("n_total", C.c_int64),
        ("n_pairs", C.c_int64),
        ("log_off", C.c_void_p),
        ("kind", C.c_void_p),
        ("ts", C.c_void_p),
        ("oid_hi", C.c_void_p),
        ("oid_lo", C.c_void_p),
        ("sym", C.c_void_p),
        ("v0", C.c_void_p),
        ("pair_a", C.c_void_p),
        ("pair_b", C.c_void_p),
        ("conflicts", C.c_void_p),
        ("conf_off", C.c_void_p),
        ("counts", C.c_void_p),
        ("grid_cap", C.c_int32),
    ]


class SmxCandidates(C.Structure):
    _fields_ = [
        ("n_logs", C.c_int64),
        ("n_total", C.c_int64),
        ("log_off", C.c_void_p),
        ("kind", C.c_void_p),
        ("sym", C.c_void_p),
        ("v0", C.c_void_p),
        ("pair_a", C.c_void_p),
        ("pair_b", C.c_void_p),
        ("pair_cap", C.c_int64),
        ("counts", C.c_void_p),
        ("log_info", C.c_void_p),
        ("grid_cap", C.c_int32),
    ]


class SmxPairs(C.Structure):
    _fields_ = [
        ("n_logs", C.c_int64),
        ("n_total", C.c_int64),
        ("n_pairs", C.c_int64),
        ("n_sym", C.c_int64),
        ("n_out", C.c_int64),
        ("log_off", C.c_void_p),
        ("kind", C.c_void_p),
        ("ts", C.c_void_p),
        ("oid_hi", C.c_void_p),
        ("oid_lo", C.c_void_p),
        ("sym", C.c_void_p),
        ("v0", C.c_void_p),
        ("v1", C.c_void_p),
        ("pair_a", C.c_void_p),
        ("pair_b", C.c_void_p),
        ("res_off", C.c_void_p),
        ("order", C.c_void_p),
        ("addr", C.c_void_p),
        ("file", C.c_void_p),
        ("ctx", C.c_void_p),
        ("conflicts", C.c_void_p),
        ("conf_off", C.c_void_p),
        ("counts", C.c_void_p),
        ("grid_cap", C.c_int32),
    ]


class SmxTrain(C.Structure):
    _fields_ = [
        ("n_logs", C.c_int64),
        ("n_total", C.c_int64),
        ("n_trains", C.c_int64),
        ("n_steps", C.c_int64),
        ("n_sym", C.c_int64),
        ("n_out", C.c_int64),
        ("log_off", C.c_void_p),
        ("kind", C.c_void_p),
        ("ts", C.c_void_p),
        ("oid_hi", C.c_void_p),
        ("oid_lo", C.c_void_p),
        ("sym", C.c_void_p),
        ("v0", C.c_void_p),
        ("v1", C.c_void_p),
        ("v1_alt", C.c_void_p),
        ("train_off", C.c_void_p),
        ("train_log", C.c_void_p),
        ("res_off", C.c_void_p),
        ("src", C.c_void_p),
        ("addr", C.c_void_p),
        ("file", C.c_void_p),
        ("ctx", C.c_void_p),
        ("conflicts", C.c_void_p),
        ("conf_off", C.c_void_p),
        ("counts", C.c_void_p),
        ("step_counts", C.c_void_p),
        ("grid_cap", C.c_int32),
        ("empty_str", C.c_int32),
    ]


TREE_MAX_LEVELS = 4096  # SMX_TREE_MAX_LEVELS


class SmxTree(C.Structure):
    _fields_ = [
        ("n_logs", C.c_int64),
        ("n_total", C.c_int64),
        ("n_nodes", C.c_int64),
        ("n_levels", C.c_int64),
        ("n_sym", C.c_int64),
        ("n_out", C.c_int64),
        ("log_off", C.c_void_p),
        ("kind", C.c_void_p),
        ("ts", C.c_void_p),
        ("oid_hi", C.c_void_p),
        ("oid_lo", C.c_void_p),
        ("sym", C.c_void_p),
        ("v0", C.c_void_p),
        ("v1", C.c_void_p),
        ("v1_alt", C.c_void_p),
        ("level_off", C.c_void_p),
        ("node_parent", C.c_void_p),
        ("node_log", C.c_void_p),
        ("res_off", C.c_void_p),
        ("src", C.c_void_p),
        ("addr", C.c_void_p),
        ("file", C.c_void_p),
        ("ctx", C.c_void_p),
        ("conflicts", C.c_void_p),
        ("conf_off", C.c_void_p),
        ("node_counts", C.c_void_p),
        ("node_acc", C.c_void_p),
        ("grid_cap", C.c_int32),
        ("empty_str", C.c_int32),
    ]


class SmxTrainStep(C.Structure):
    _fields_ = [
        ("n_total", C.c_int64),
        ("n_sym", C.c_int64),
        ("kind", C.c_void_p),
        ("ts", C.c_void_p),
        ("oid_hi", C.c_void_p),
        ("oid_lo", C.c_void_p),
        ("sym", C.c_void_p),
        ("v0", C.c_void_p),
        ("v1", C.c_void_p),
        ("v1_alt", C.c_void_p),
        ("n_acc", C.c_int64),
        ("acc_src", C.c_void_p),
        ("acc_addr", C.c_void_p),
        ("acc_file", C.c_void_p),
        ("acc_ctx", C.c_void_p),
        ("log_lo", C.c_int64),
        ("log_n", C.c_int64),
        ("st_kind", C.c_void_p),
        ("st_ts", C.c_void_p),
        ("st_oid_hi", C.c_void_p),
        ("st_oid_lo", C.c_void_p),
        ("st_sym", C.c_void_p),
        ("st_v0", C.c_void_p),
        ("st_v1", C.c_void_p),
        ("order", C.c_void_p),
        ("addr", C.c_void_p),
        ("file", C.c_void_p),
        ("ctx", C.c_void_p),
        ("conflicts", C.c_void_p),
        ("conflict_cap", C.c_int64),
        ("counts", C.c_void_p),
        ("out_src", C.c_void_p),
        ("out_addr", C.c_void_p),
        ("out_file", C.c_void_p),
        ("out_ctx", C.c_void_p),
        ("records", C.c_void_p),
        ("record_cap", C.c_int64),
        ("status", C.c_void_p),
        ("empty_str", C.c_int32),
    ]


class SmxScreenTrain(C.Structure):
    _fields_ = [
        ("n_logs", C.c_int64),
        ("n_total", C.c_int64),
        ("n_trains", C.c_int64),
        ("n_steps", C.c_int64),
        ("n_acc", C.c_int64),
        ("log_off", C.c_void_p),
        ("kind", C.c_void_p),
        ("ts", C.c_void_p),
        ("oid_hi", C.c_void_p),
        ("oid_lo", C.c_void_p),
        ("sym", C.c_void_p),
        ("v0", C.c_void_p),
        ("train_off", C.c_void_p),
        ("train_log", C.c_void_p),
        ("acc_off", C.c_void_p),
        ("conflicts", C.c_void_p),
        ("conf_off", C.c_void_p),
        ("counts", C.c_void_p),
        ("step_counts", C.c_void_p),
        ("grid_cap", C.c_int32),
    ]


class SmxScreenTree(C.Structure):
    _fields_ = [
        ("n_logs", C.c_int64),
        ("n_total", C.c_int64),
        ("n_nodes", C.c_int64),
        ("n_levels", C.c_int64),
        ("n_acc", C.c_int64),
        ("log_off", C.c_void_p),
        ("kind", C.c_void_p),
        ("ts", C.c_void_p),
        ("oid_hi", C.c_void_p),
        ("oid_lo", C.c_void_p),
        ("sym", C.c_void_p),
        ("v0", C.c_void_p),
        ("level_off", C.c_void_p),
        ("node_parent", C.c_void_p),
        ("node_log", C.c_void_p),
        ("acc_off", C.c_void_p),
        ("conflicts", C.c_void_p),
        ("conf_off", C.c_void_p),
        ("node_counts", C.c_void_p),
        ("grid_cap", C.c_int32),
    ]


CAND_MAX_LOGS = 16384       # logs per smx_screen_candidates call (include/smx.h SMX_CAND_MAX_LOGS)
SCREEN_MAX_RENAMES = 2048     # renames per pair of smx_screen, both logs together (more: counts -2)
SCREEN_CLASSES = (128, 512, 2048)  # its size classes, in renames (csrc/smx_screen.h)
BATCH_MAX_OPS = 2048          # ops per merge of smx_compose_batch (larger: counts -2)
BATCH_CLASSES = (256, 1024, 2048)  # its size classes (csrc/smx_batch.h)


class SmxShard(C.Structure):
    _fields_ = [
        ("rank", C.c_int32),
        ("world", C.c_int32),
        ("src_a", C.c_int64),
        ("src_b", C.c_int64),
        ("halo_n", C.c_int64 * 2),
        ("halo_more", C.c_int32 * 2),
        ("halo_sym", C.c_void_p * 2),
        ("halo_cls", C.c_void_p * 2),
        ("halo_src", C.c_void_p * 2),
        ("in_ahead", C.c_int32),
        ("in_d", C.c_int64),
        ("summary", C.c_void_p),
        ("halo_cap", C.c_int64),
        ("export_sym", C.c_void_p),
        ("export_cls", C.c_void_p),
        ("export_src", C.c_void_p),
        ("part_tab", C.c_void_p),
        ("fin_tab", C.c_void_p),
        ("glob", C.c_void_p),
        ("mv_prefix", C.c_void_p),
        ("halo_dev", C.c_void_p),
        ("in_state_dev", C.c_void_p),
        ("src_map", C.c_void_p),
        ("summary_host", C.c_void_p),
        ("order_gather", C.c_void_p),
        ("tab32", C.c_int32),
    ]


SHARD_ORDER, SHARD_WALK, SHARD_TABLES, SHARD_EMIT = 0, 1, 2, 3
SHARD_ORDER_FIX = 4
SHARD_SCATTER = 5
PLAN_NAMES = ("presorted", "segmented", "radix", "radix+oid_lo", "presorted-wide", "small")  # smx_last_plan()
SHARD_SUMMARY = 32


class SmxRgaOps(C.Structure):
    _fields_ = [
        ("n_ops", C.c_int64),
        ("n_lists", C.c_int64),
        ("list", C.c_void_p),
        ("op", C.c_void_p),
        ("value", C.c_void_p),
        ("anchor", C.c_void_p),
        ("t", C.c_void_p),
        ("author", C.c_void_p),
        ("opid_hi", C.c_void_p),
        ("opid_lo", C.c_void_p),
    ]


class SmxRgaOut(C.Structure):
    _fields_ = [
        ("out_value", C.c_void_p),
        ("out_src", C.c_void_p),
        ("out_offsets", C.c_void_p),
        ("counts", C.c_void_p),
        ("out_tomb", C.c_void_p),
    ]


class SmxRgaOnto(C.Structure):
    _fields_ = [
        ("n_total", C.c_int64),
        ("n_bases", C.c_int64),
        ("n_jobs", C.c_int64),
        ("n_out", C.c_int64),
        ("base_off", C.c_void_p),
        ("own_off", C.c_void_p),
        ("job_base", C.c_void_p),
        ("op", C.c_void_p),
        ("value", C.c_void_p),
        ("anchor", C.c_void_p),
        ("t", C.c_void_p),
        ("author", C.c_void_p),
        ("opid_hi", C.c_void_p),
        ("opid_lo", C.c_void_p),
    ]


class SmxRgaChain(C.Structure):
    _fields_ = [
        ("n_total", C.c_int64),
        ("n_segs", C.c_int64),
        ("n_jobs", C.c_int64),
        ("n_links", C.c_int64),
        ("n_out", C.c_int64),
        ("seg_off", C.c_void_p),
        ("job_off", C.c_void_p),
        ("job_seg", C.c_void_p),
        ("op", C.c_void_p),
        ("value", C.c_void_p),
        ("anchor", C.c_void_p),
        ("t", C.c_void_p),
        ("author", C.c_void_p),
        ("opid_hi", C.c_void_p),
        ("opid_lo", C.c_void_p),
    ]


# Every symbol include/smx.h declares (tests check the built library exports them).
RGA_GROUPED = 1   # smx_rga_replay_ex flag (include/smx.h SMX_RGA_GROUPED)
SCREEN_LARGE = 1  # smx_screen_ex flag (include/smx.h SMX_SCREEN_LARGE): no limit on renames
BATCH_LARGE = 1   # smx_compose_batch_ex / _shared_ex flag (include/smx.h SMX_BATCH_LARGE): no limit on ops

EXPORTS = (
    "smx_compose_workspace_bytes",
    "smx_compose",
    "smx_compose_async",
    "smx_compose_finish",
    "smx_release_graphs",
    "smx_last_plan",
    "smx_set_small_limit",
    "smx_compose_batch_workspace_bytes",
    "smx_compose_batch",
    "smx_compose_batch_shared_workspace_bytes",
    "smx_compose_batch_shared",
    "smx_compose_batch_ex_workspace_bytes",
    "smx_compose_batch_ex",
    "smx_compose_batch_shared_ex_workspace_bytes",
    "smx_compose_batch_shared_ex",
    "smx_compose_pairs_workspace_bytes",
    "smx_compose_pairs",
    "smx_compose_train_workspace_bytes",
    "smx_compose_train",
    "smx_compose_tree_workspace_bytes",
    "smx_compose_tree",
    "smx_train_stage",
    "smx_train_land",
    "smx_screen_workspace_bytes",
    "smx_screen",
    "smx_screen_ex_workspace_bytes",
    "smx_screen_ex",
    "smx_screen_candidates_workspace_bytes",
    "smx_screen_candidates",
    "smx_screen_train_workspace_bytes",
    "smx_screen_train",
    "smx_screen_tree_workspace_bytes",
    "smx_screen_tree",
    "smx_shard_step",
    "smx_shard_range_info",
    "smx_set_profiling",
    "smx_set_profiling_stages",
    "smx_stage_times",
    "smx_stage_name",
    "smx_reset_stage_times",
    "smx_rga_workspace_bytes",
    "smx_rga_replay",
    "smx_rga_replay_ex",
    "smx_rga_replay_onto_workspace_bytes",
    "smx_rga_replay_onto",
    "smx_rga_replay_chain_workspace_bytes",
    "smx_rga_replay_chain",
    "smx_last_error",
    "smx_version",
)


def declare(lib: C.CDLL) -> C.CDLL:
    """Attach argtypes/restype for the product library."""
    lib.smx_compose_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64,
                                                C.POINTER(C.c_size_t)]
    lib.smx_compose_workspace_bytes.restype = C.c_int
    lib.smx_compose.argtypes = [C.POINTER(SmxOps), C.POINTER(SmxComposeOut), C.c_void_p,
                                C.c_size_t, C.c_void_p]
    lib.smx_compose.restype = C.c_int
    for f in ("smx_compose_async", "smx_compose_finish"):
        getattr(lib, f).argtypes = lib.smx_compose.argtypes
        getattr(lib, f).restype = C.c_int
    lib.smx_release_graphs.argtypes = [C.c_void_p]
    lib.smx_release_graphs.restype = C.c_int
    lib.smx_last_plan.argtypes = []
    lib.smx_last_plan.restype = C.c_int
    lib.smx_set_small_limit.argtypes = [C.c_int64]
    lib.smx_set_small_limit.restype = C.c_int64
    if hasattr(lib, "smx_compose_batch"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_compose_batch_workspace_bytes.argtypes = [C.c_int64, C.POINTER(C.c_size_t)]
        lib.smx_compose_batch_workspace_bytes.restype = C.c_int
        lib.smx_compose_batch.argtypes = [C.POINTER(SmxBatch), C.c_void_p, C.c_size_t, C.c_void_p]
        lib.smx_compose_batch.restype = C.c_int
    if hasattr(lib, "smx_compose_batch_shared"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_compose_batch_shared_workspace_bytes.argtypes = [C.c_int64, C.POINTER(C.c_size_t)]
        lib.smx_compose_batch_shared_workspace_bytes.restype = C.c_int
        lib.smx_compose_batch_shared.argtypes = [C.POINTER(SmxBatchShared), C.c_void_p, C.c_size_t, C.c_void_p]
        lib.smx_compose_batch_shared.restype = C.c_int
    if hasattr(lib, "smx_compose_batch_ex"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_compose_batch_ex_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_uint32, C.POINTER(C.c_size_t)]
        lib.smx_compose_batch_ex_workspace_bytes.restype = C.c_int
        lib.smx_compose_batch_ex.argtypes = [C.POINTER(SmxBatch), C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
        lib.smx_compose_batch_ex.restype = C.c_int
        lib.smx_compose_batch_shared_ex_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_uint32,
                                                                    C.POINTER(C.c_size_t)]
        lib.smx_compose_batch_shared_ex_workspace_bytes.restype = C.c_int
        lib.smx_compose_batch_shared_ex.argtypes = [C.POINTER(SmxBatchShared), C.c_void_p, C.c_size_t, C.c_uint32,
                                                    C.c_void_p]
        lib.smx_compose_batch_shared_ex.restype = C.c_int
    if hasattr(lib, "smx_compose_pairs"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_compose_pairs_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_uint32,
                                                          C.POINTER(C.c_size_t)]
        lib.smx_compose_pairs_workspace_bytes.restype = C.c_int
        lib.smx_compose_pairs.argtypes = [C.POINTER(SmxPairs), C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
        lib.smx_compose_pairs.restype = C.c_int
    if hasattr(lib, "smx_compose_train"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_compose_train_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_uint32,
                                                          C.POINTER(C.c_size_t)]
        lib.smx_compose_train_workspace_bytes.restype = C.c_int
        lib.smx_compose_train.argtypes = [C.POINTER(SmxTrain), C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
        lib.smx_compose_train.restype = C.c_int
    if hasattr(lib, "smx_compose_tree"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_compose_tree_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_uint32,
                                                         C.POINTER(C.c_size_t)]
        lib.smx_compose_tree_workspace_bytes.restype = C.c_int
        lib.smx_compose_tree.argtypes = [C.POINTER(SmxTree), C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
        lib.smx_compose_tree.restype = C.c_int
    if hasattr(lib, "smx_train_stage"):  # (older builds, e.g. A/B baselines, lack it)
        for f in ("smx_train_stage", "smx_train_land"):
            getattr(lib, f).argtypes = [C.POINTER(SmxTrainStep), C.c_void_p]
            getattr(lib, f).restype = C.c_int
    if hasattr(lib, "smx_screen"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_screen_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]
        lib.smx_screen_workspace_bytes.restype = C.c_int
        lib.smx_screen.argtypes = [C.POINTER(SmxScreen), C.c_void_p, C.c_size_t, C.c_void_p]
        lib.smx_screen.restype = C.c_int
    if hasattr(lib, "smx_screen_ex"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_screen_ex_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_uint32,
                                                      C.POINTER(C.c_size_t)]
        lib.smx_screen_ex_workspace_bytes.restype = C.c_int
        lib.smx_screen_ex.argtypes = [C.POINTER(SmxScreen), C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
        lib.smx_screen_ex.restype = C.c_int
    if hasattr(lib, "smx_screen_candidates"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_screen_candidates_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]
        lib.smx_screen_candidates_workspace_bytes.restype = C.c_int
        lib.smx_screen_candidates.argtypes = [C.POINTER(SmxCandidates), C.c_void_p, C.c_size_t, C.c_void_p]
        lib.smx_screen_candidates.restype = C.c_int
    if hasattr(lib, "smx_screen_train"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_screen_train_workspace_bytes.argtypes = [C.c_int64] * 5 + [C.c_uint32, C.POINTER(C.c_size_t)]
        lib.smx_screen_train_workspace_bytes.restype = C.c_int
        lib.smx_screen_train.argtypes = [C.POINTER(SmxScreenTrain), C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
        lib.smx_screen_train.restype = C.c_int
    if hasattr(lib, "smx_screen_tree"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_screen_tree_workspace_bytes.argtypes = [C.c_int64] * 5 + [C.c_uint32, C.POINTER(C.c_size_t)]
        lib.smx_screen_tree_workspace_bytes.restype = C.c_int
        lib.smx_screen_tree.argtypes = [C.POINTER(SmxScreenTree), C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
        lib.smx_screen_tree.restype = C.c_int
    lib.smx_shard_step.argtypes = [C.POINTER(SmxOps), C.POINTER(SmxShard), C.POINTER(SmxComposeOut),
                                   C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    lib.smx_shard_step.restype = C.c_int
    if hasattr(lib, "smx_shard_range_info"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_shard_range_info.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        lib.smx_shard_range_info.restype = C.c_int
    lib.smx_set_profiling.argtypes = [C.c_int]
    lib.smx_set_profiling.restype = C.c_int
    lib.smx_set_profiling_stages.argtypes = [C.c_uint32]
    lib.smx_set_profiling_stages.restype = C.c_int
    lib.smx_stage_times.argtypes = [C.POINTER(C.c_double), c_i64p, C.c_int]
    lib.smx_stage_times.restype = C.c_int
    lib.smx_stage_name.argtypes = [C.c_int]
    lib.smx_stage_name.restype = C.c_char_p
    lib.smx_reset_stage_times.argtypes = []
    lib.smx_reset_stage_times.restype = C.c_int
    lib.smx_rga_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]
    lib.smx_rga_workspace_bytes.restype = C.c_int
    lib.smx_rga_replay.argtypes = [C.POINTER(SmxRgaOps), C.POINTER(SmxRgaOut), C.c_void_p,
                                   C.c_size_t, C.c_void_p]
    lib.smx_rga_replay.restype = C.c_int
    lib.smx_rga_replay_ex.argtypes = [C.POINTER(SmxRgaOps), C.POINTER(SmxRgaOut), C.c_void_p,
                                      C.c_size_t, C.c_uint32, C.c_void_p]
    lib.smx_rga_replay_ex.restype = C.c_int
    if hasattr(lib, "smx_rga_replay_onto"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_rga_replay_onto_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]
        lib.smx_rga_replay_onto_workspace_bytes.restype = C.c_int
        lib.smx_rga_replay_onto.argtypes = [C.POINTER(SmxRgaOnto), C.POINTER(SmxRgaOut), C.c_void_p,
                                            C.c_size_t, C.c_void_p]
        lib.smx_rga_replay_onto.restype = C.c_int
    if hasattr(lib, "smx_rga_replay_chain"):  # (older builds, e.g. A/B baselines, lack it)
        lib.smx_rga_replay_chain_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]
        lib.smx_rga_replay_chain_workspace_bytes.restype = C.c_int
        lib.smx_rga_replay_chain.argtypes = [C.POINTER(SmxRgaChain), C.POINTER(SmxRgaOut), C.c_void_p,
                                             C.c_size_t, C.c_void_p]
        lib.smx_rga_replay_chain.restype = C.c_int
    lib.smx_last_error.argtypes = []
    lib.smx_last_error.restype = C.c_char_p
    lib.smx_version.argtypes = []
    lib.smx_version.restype = C.c_char_p
    return lib
