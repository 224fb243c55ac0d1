"""ctypes binding of the C ABI declared in include/keraslm_hip.h.

The product path has no CPU fallback: importing this module is harmless (so the
host-side logic can be unit-tested), but `load()` raises if the gfx950 shared
library has not been built, and every compute entry point needs a GPU.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (KL_LIB: another build of the same library, e.g. the -DKL_STAMP diagnostic build or an A/B candidate)
LIB_PATH = os.environ.get("KL_LIB") or os.path.join(os.path.dirname(_HERE), "libkeraslm_hip.so")

KL_PREC_BF16 = 1
KL_PREC_SPLIT = 3
KL_RATE_ALTS_MAX = 8     # alternatives per position kl_rate_window_alts delivers at most
KL_SPAN_LEN_MAX = 64     # ids of a span and of a candidate of kl_span_windows at most
KL_CTX_CAND_MAX = 256    # candidate contexts of kl_rate_scatter_planes / kl_context_mix at most
KL_LEXICON_V_MAX, KL_LEXICON_DIST_MAX, KL_LEXICON_K_MAX = 4096, 8, 16      # kl_lexicon_neighbours: ids, max_dist and K at most
KL_LEXICON_MIN_PART_MAX = 32      # kl_lexicon_splits: min_part at most
KL_LEXICON_PARTS_MAX, KL_LEXICON_LINKS_MAX, KL_LEXICON_LINK_LEN_MAX = 8, 8, 3      # kl_lexicon_chains: parts, links, ids of a link
KL_CHANNEL_RULES_MAX, KL_CHANNEL_COST_MAX = 1024, 4095     # kl_lexicon_channel: rules, and unit, max_cost and a rule's cost at most
KL_ALIGN_DIST_MAX, KL_ALIGN_LEN_MAX = 255, 4096      # kl_align_pairs: max_dist and symbols of a text at most
KL_CONFUSION_CHARS_MAX = 4      # kl_confusion_counts: symbols of a source and of a target at most
KL_WITNESS_MAX = 64      # kl_witness_clusters: witnesses (pairs) of a text at most
KL_RATE_SELECT_BLOCK = 1024          # positions per workgroup of kl_rate_select
KL_RATE_SELECT_SCAN_THREADS = 256    # ... and blocks per round of its one offsets workgroup
KL_SAMPLE_MAX_ROWS = 1024  # chains per kl_sample_pick call
KL_SAMPLE_MAX_TOPK = 64
# kl_window_view.wg_route
KL_WG_KMAJOR, KL_WG_SCAN_T, KL_WG_TRANSPOSE, KL_WG_SEGSUM, KL_WG_PAIR_CTX = 1, 2, 4, 8, 16
# kl_window_view.out_route
KL_OUT_LOGITS_WS, KL_OUT_LOGITS_W128, KL_OUT_DH_WS, KL_OUT_DE_KMAJOR = 1, 2, 4, 8
# kl_forward_view.family / .passed_mask; .handoff
KL_FWD_SPLIT_PAIRS, KL_FWD_SPLIT_LAYERS, KL_FWD_SPLIT_FUSED, KL_FWD_WAVEFRONT = 1, 2, 4, 8
KL_FWD_HANDOFF_NONE, KL_FWD_HANDOFF_SENTINELS, KL_FWD_HANDOFF_COUNTERS = 0, 1, 2
# kl_derived_view.current; the first three bits of the mask of kl_test_prepare_lazy
KL_DV_EAGER, KL_DV_LO, KL_DV_INTERLEAVED, KL_DV_INC, KL_DV_BIG, KL_DV_COMB = 1, 2, 4, 8, 16, 32
KL_LAZY_INC, KL_LAZY_BIG, KL_LAZY_COMB = 1, 2, 4
# kl_step_route.layers / .out / .idx
KL_STEP_TILES, KL_STEP_CELLS, KL_STEP_GEMM_FUSED, KL_STEP_GEMM_PLAIN, KL_STEP_THIN = 1, 2, 3, 4, 5
KL_STEP_OUT_FUSED, KL_STEP_OUT_THIN, KL_STEP_OUT_BIG = 1, 2, 3
KL_STEP_IDX_DEVICE, KL_STEP_IDX_KERNARG, KL_STEP_IDX_PACKED = 1, 2, 3


class KlConfig(C.Structure):
    _fields_ = [("depth", C.c_int32), ("width", C.c_int32), ("voc_size", C.c_int32),
                ("n_ctx", C.c_int32), ("ctx_vocab", C.c_int32), ("ctx_dim", C.c_int32)]


class KlWindowView(C.Structure):
    """kl_window_view of include/keraslm_hip.h (kl_test_window_view)"""
    _fields_ = [("depth", C.c_int32), ("width", C.c_int32), ("B", C.c_int32), ("T", C.c_int32),
                ("g_interleaved", C.c_int32), ("c_in_cb", C.c_int32), ("dh_bf16", C.c_int32), ("p_bf16_mask", C.c_int32),
                ("scan2_rows", C.c_int32), ("wg_route", C.c_int32), ("wg_pair_mask", C.c_int32),
                ("wg_db_scan_mask", C.c_int32), ("out_route", C.c_int32), ("reserved", C.c_int32 * 3),
                ("off_H", C.c_uint64 * 16), ("off_C", C.c_uint64 * 16), ("off_Cb", C.c_uint64 * 16),
                ("off_G", C.c_uint64 * 16), ("off_dZ", C.c_uint64 * 16), ("off_Hd", C.c_uint64 * 16),
                ("off_dlogits", C.c_uint64), ("ld_dlogits", C.c_uint64)]


class KlForwardView(C.Structure):
    """kl_forward_view of include/keraslm_hip.h (kl_test_forward_view)"""
    _fields_ = ([(n, C.c_int32) for n in ("depth", "width", "B", "T", "family", "passed_mask", "ring_mask", "thin_mask", "handoff",
                                          "c_every_step", "precision", "p1_layer")] + [("reserved", C.c_int32 * 4)] +
                [("off_" + n, C.c_uint64 * 16) for n in ("H", "C", "Xhi", "Xlo")] + [("off_P1", C.c_uint64)])


class KlDerivedView(C.Structure):
    """kl_derived_view of include/keraslm_hip.h (kl_test_derived_view)"""
    _fields_ = ([(n, C.c_int32) for n in ("depth", "width", "voc_size", "Vp", "n_ctx", "ctx_vocab", "ctx_dim", "precision",
                                          "current", "has_comb", "mask_il", "mask_KF")] + [("reserved", C.c_int32 * 4)] +
                [("off_" + n, C.c_uint64 * 16) for n in ("UT_hi", "UT_lo", "KT_hi", "KT_lo", "Un", "Kn", "KTp", "bp", "UF", "KF",
                                                         "WTcat", "WTperm")] +
                [("off_CtxK", C.c_uint64 * 8), ("off_CtxKp", C.c_uint64 * 8)] +
                [("off_" + n, C.c_uint64) for n in ("E_hi", "E_lo", "ET", "EK", "EKp", "comb", "EF", "Ecat")] +
                [("bytes", C.c_uint64)])


class KlStepRoute(C.Structure):
    """kl_step_route of include/keraslm_hip.h (kl_test_step_route)"""
    _fields_ = ([(n, C.c_int32) for n in ("layers", "out", "idx", "lo", "gathered", "depth", "tile_rows", "px", "py")] +
                [("nmt", C.c_int32 * 16), ("gen", C.c_int32 * 16), ("reserved", C.c_int32 * 7)])


class KlError(RuntimeError):
    pass


# name -> (restype, argtypes): every symbol include/keraslm_hip.h declares
SIGNATURES = {
    "kl_abi_version": (C.c_int, []),
    "kl_error_string": (C.c_char_p, [C.c_int]),
    "kl_param_count": (C.c_size_t, [C.POINTER(KlConfig)]),
    "kl_param_layout": (C.c_int, [C.POINTER(KlConfig), C.c_int, C.c_char_p, C.c_size_t,
                                  C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "kl_create": (C.c_void_p, [C.POINTER(KlConfig)]),
    "kl_destroy": (None, [C.c_void_p]),
    "kl_derived_bytes": (C.c_size_t, [C.c_void_p]),
    "kl_bind": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "kl_prepare": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "kl_window_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "kl_forward_window": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_rate_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "kl_rate_window": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_rate_alts_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "kl_rate_window_alts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    "kl_rate_bulk_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "kl_rate_window_bulk": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_rate_scatter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_rate_text_bits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "kl_rate_alts_bulk_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "kl_rate_window_alts_bulk": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.c_void_p]),
    "kl_rate_scatter_alts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_rate_select_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "kl_rate_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_int,
                                 C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p]),
    "kl_variant_windows": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "kl_edit_windows": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "kl_prefix_windows": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kl_state_fanout": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "kl_span_windows": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_int64,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "kl_span_pick": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p]),
    "kl_rate_scatter_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_size_t, C.c_size_t, C.c_void_p]),
    "kl_context_mix": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kl_word_bounds_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_int]),
    "kl_word_bounds": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_rate_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "kl_segment_select_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "kl_segment_select": (C.c_int, [C.c_void_p] * 8 + [C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_size_t] + [C.c_void_p] * 11
                          + [C.c_size_t, C.c_void_p]),
    "kl_lexicon_neighbours_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_int]),
    "kl_lexicon_neighbours": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p]),
    "kl_lexicon_channel_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_int, C.c_int]),
    "kl_lexicon_channel": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_lexicon_splits_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_int]),
    "kl_lexicon_splits": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                    C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_lexicon_chains_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_int]),
    "kl_lexicon_chains": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                    C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_align_pairs_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_int, C.c_int]),
    "kl_align_pairs": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                 C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_confusion_counts_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_int, C.c_size_t]),
    "kl_confusion_counts": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_witness_clusters_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_int, C.c_size_t]),
    "kl_witness_clusters": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_size_t, C.c_int] + [C.c_void_p] * 9 + [C.c_size_t, C.c_void_p]),
    "kl_witness_pool": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_train_window": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_assemble_windows": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "kl_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float,
                               C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "kl_adam_step_scaled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                     C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "kl_step_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "kl_step_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_host_alloc": (C.c_void_p, [C.c_size_t]),
    "kl_host_free": (None, [C.c_void_p]),
    "kl_step_host_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "kl_step_batch_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                     C.c_size_t, C.c_void_p]),
    "kl_walk_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "kl_walk_stage_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "kl_walk_batch_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_beam_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "kl_beam_expand": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_sample_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "kl_sample_pick": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_float, C.c_uint64,
                                 C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.c_void_p]),
    "kl_sample_pick_from": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_float,
                                      C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    "kl_edge_costs": (C.c_int, [C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "kl_edge_decode_out_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_long, C.c_long]),
    "kl_edge_decode": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 11 + [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                 C.c_long, C.c_long, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kl_step_wait": (C.c_int, [C.c_void_p, C.c_uint32, C.c_double]),
    "kl_state_dist2": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_void_p]),
    "kl_trace_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "kl_set_window_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "kl_set_loss_rows": (C.c_int, [C.c_void_p, C.c_int]),
    "kl_trace_kernel_name": (C.c_char_p, [C.c_void_p, C.c_int]),
    "kl_trace_read": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int),
                                C.POINTER(C.c_double)]),
    "kl_test_gemm_tn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                  C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p]),
    "kl_test_gemm_an": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long,
                                  C.c_long, C.c_int, C.c_int, C.c_void_p]),
    "kl_test_gemm_an2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long,
                                   C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p]),
    "kl_test_gemm_tn_route": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.c_size_t,
                                        C.c_int, C.POINTER(C.c_int)]),
    "kl_test_gemm_an_route": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, C.c_int,
                                        C.POINTER(C.c_int)]),
    "kl_test_segment_sums_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "kl_test_segment_sums_share": (C.c_int, [C.c_int, C.c_int]),
    "kl_test_segment_sums": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kl_test_thin_gemm": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_void_p]),
    "kl_test_thin_gemm_ex": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int,
                                       C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p]),
    "kl_test_softmax_ce": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                     C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "kl_test_logits_ce_ws": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_float, C.c_int, C.c_void_p]),
    "kl_test_logits_ce_w128": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "kl_test_dh_ws": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]),
    "kl_test_regulariser_grads": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kl_test_rate_topk": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kl_test_window_view": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(KlWindowView)]),
    "kl_test_forward_view": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(KlForwardView)]),
    "kl_test_derived_view": (C.c_int, [C.c_void_p, C.POINTER(KlDerivedView)]),
    "kl_test_prepare_lazy": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "kl_test_step_route": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(KlStepRoute)]),
}

_lib = None


def load():
    """Load libkeraslm_hip.so (built by `make -C ocrd_keraslm_amd/csrc` or
    __graft_entry__.build()).  Raises if it is missing -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KlError("HIP extension %s not built: run `make -C ocrd_keraslm_amd/csrc` "
                      "(the Rater has no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code, what=""):
    if code != 0:
        msg = load().kl_error_string(code).decode()
        raise KlError("%s failed: %s (code %d)" % (what or "keraslm_hip call", msg, code))
