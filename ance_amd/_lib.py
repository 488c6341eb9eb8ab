"""ctypes binding of libance_amd.so (the C ABI declared in include/ance_amd.h).

The product path has NO CPU fallback: if the HIP library is missing or fails to load, every
entry point raises.  ``build()`` compiles it in-tree with hipcc for gfx950.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# ANCE_AMD_LIB: another build of the same ABI (the measurement library of `make -C ance_amd/csrc measure`)
LIB_PATH = os.environ.get("ANCE_AMD_LIB") or os.path.join(_HERE, "libance_amd.so")
CSRC = os.path.join(_HERE, "csrc")

ANCE_OK = 0
ANCE_E_INVALID = -1  # include/ance_amd.h: a refused argument
ABI_VERSION = 7

c_i32p = ctypes.POINTER(ctypes.c_int32)
c_i64p = ctypes.POINTER(ctypes.c_int64)
c_f32p = ctypes.POINTER(ctypes.c_float)


class AnceEncoderDesc(ctypes.Structure):
    _fields_ = [
        ("arch", ctypes.c_int32), ("n_layers", ctypes.c_int32), ("hidden", ctypes.c_int32),
        ("n_heads", ctypes.c_int32), ("intermediate", ctypes.c_int32), ("vocab_size", ctypes.c_int32),
        ("max_position", ctypes.c_int32), ("pad_token_id", ctypes.c_int32), ("ln_eps", ctypes.c_float),
        ("has_head", ctypes.c_int32), ("max_seq_len", ctypes.c_int32), ("max_tokens", ctypes.c_int32),
        ("precision", ctypes.c_int32),
    ]


class AnceGemmDebugArgs(ctypes.Structure):
    """include/ance_amd.h: the arguments of ance_debug_gemm_hw (field names of the encoder's GemmArgs)."""
    _fields_ = [
        ("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("lda", ctypes.c_int32), ("ldb", ctypes.c_int32),
        ("M", ctypes.c_int32), ("N", ctypes.c_int32), ("K", ctypes.c_int32),
        ("bias", ctypes.c_void_p), ("csum", ctypes.c_void_p), ("part_in", ctypes.c_void_p), ("ln_eps", ctypes.c_float),
        ("tok_lo", ctypes.c_void_p), ("scale", ctypes.c_float), ("scale_cols", ctypes.c_int32), ("col_map", ctypes.c_void_p),
        ("n_valid", ctypes.c_int32), ("ldc", ctypes.c_int32), ("out", ctypes.c_void_p), ("res_hi", ctypes.c_void_p),
        ("res_lo", ctypes.c_void_p), ("res_gamma", ctypes.c_void_p), ("res_beta", ctypes.c_void_p), ("out_lo", ctypes.c_void_p),
        ("part_out", ctypes.c_void_p), ("ldr", ctypes.c_int32), ("wscale_inv", ctypes.c_void_p), ("n_split", ctypes.c_int32),
    ]


class AnceAttnDebugArgs(ctypes.Structure):
    """include/ance_amd.h: the arguments of ance_debug_attention (h_desc is HOST memory)."""
    _fields_ = [
        ("kind", ctypes.c_int32), ("n_heads", ctypes.c_int32), ("n_seq", ctypes.c_int32), ("max_seq_len", ctypes.c_int32),
        ("cls_only", ctypes.c_int32), ("q_compact", ctypes.c_int32), ("h_desc", ctypes.c_void_p), ("d_desc", ctypes.c_void_p),
        ("d_desc_bytes", ctypes.c_int64), ("qk", ctypes.c_void_p), ("ld_qk", ctypes.c_int32), ("qk_rows", ctypes.c_int32),
        ("vt", ctypes.c_void_p), ("ld_vt", ctypes.c_int32), ("ctx", ctypes.c_void_p), ("ld_ctx", ctypes.c_int32),
        ("ctx_rows", ctypes.c_int32),
    ]


class AnceLambTensor(ctypes.Structure):
    """include/ance_amd.h: one row of ance_lamb_step's host tensor table."""
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("numel", ctypes.c_int64), ("group", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AnceAdamwTensor(ctypes.Structure):
    """include/ance_amd.h: one row of ance_adamw_step's host tensor table."""
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("step", ctypes.c_void_p), ("numel", ctypes.c_int64), ("group", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AnceLambGroup(ctypes.Structure):
    """include/ance_amd.h: one row of ance_lamb_step's host group table."""
    _fields_ = [("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("weight_decay", ctypes.c_double)]


class AnceGatherSegment(ctypes.Structure):
    """include/ance_amd.h: one segment (tower) of ance_gather_batch."""
    _fields_ = [("d_records", ctypes.c_void_p), ("n_records", ctypes.c_int64), ("d_index", ctypes.c_void_p),
                ("n_index", ctypes.c_int64), ("d_ids", ctypes.c_void_p), ("d_mask", ctypes.c_void_p), ("d_types", ctypes.c_void_p),
                ("L", ctypes.c_int32), ("mask_rule", ctypes.c_int32), ("type_rule", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AnceAttnTrainArgs(ctypes.Structure):
    """include/ance_amd.h: the arguments of ance_attention_forward / ance_attention_backward."""
    _fields_ = [("q", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p), ("ctx", ctypes.c_void_p),
                ("ld_q", ctypes.c_int32), ("ld_k", ctypes.c_int32), ("ld_v", ctypes.c_int32), ("ld_ctx", ctypes.c_int32),
                ("d_seq_first", ctypes.c_void_p), ("d_seq_len", ctypes.c_void_p), ("n_seq", ctypes.c_int32),
                ("max_seq_len", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("n_heads", ctypes.c_int32),
                ("seq_rows", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("dropout_p", ctypes.c_float), ("training", ctypes.c_int32), ("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64),
                ("d_workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t)]


class AnceAttnGradArgs(ctypes.Structure):
    """include/ance_amd.h: the gradient side of ance_attention_backward."""
    _fields_ = [("dctx", ctypes.c_void_p), ("dq", ctypes.c_void_p), ("dk", ctypes.c_void_p), ("dv", ctypes.c_void_p),
                ("ld_dctx", ctypes.c_int32), ("ld_dq", ctypes.c_int32), ("ld_dk", ctypes.c_int32), ("ld_dv", ctypes.c_int32)]


ANCE_DTYPE_F32, ANCE_DTYPE_F16, ANCE_DTYPE_BF16 = 0, 1, 2


class AnceAttn16Args(ctypes.Structure):
    """include/ance_amd.h: the arguments of ance_attention16_forward / ance_attention16_backward (16-bit rows, a dtype)."""
    _fields_ = [("q", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p), ("ctx", ctypes.c_void_p),
                ("ld_q", ctypes.c_int32), ("ld_k", ctypes.c_int32), ("ld_v", ctypes.c_int32), ("ld_ctx", ctypes.c_int32),
                ("d_seq_first", ctypes.c_void_p), ("d_seq_len", ctypes.c_void_p), ("n_seq", ctypes.c_int32),
                ("max_seq_len", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("n_heads", ctypes.c_int32),
                ("seq_rows", ctypes.c_int32), ("dtype", ctypes.c_int32),
                ("dropout_p", ctypes.c_float), ("training", ctypes.c_int32), ("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64),
                ("d_workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t)]


class AnceAttn16GradArgs(ctypes.Structure):
    """include/ance_amd.h: the gradient side of ance_attention16_backward."""
    _fields_ = [("dctx", ctypes.c_void_p), ("dq", ctypes.c_void_p), ("dk", ctypes.c_void_p), ("dv", ctypes.c_void_p),
                ("ld_dctx", ctypes.c_int32), ("ld_dq", ctypes.c_int32), ("ld_dk", ctypes.c_int32), ("ld_dv", ctypes.c_int32)]


class AnceLayerTailArgs(ctypes.Structure):
    """include/ance_amd.h: the arguments of ance_layer_tail_forward / ance_layer_tail_backward."""
    _fields_ = [("x", ctypes.c_void_p), ("res", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("gamma", ctypes.c_void_p),
                ("beta", ctypes.c_void_p), ("y", ctypes.c_void_p), ("ld_x", ctypes.c_int32), ("ld_res", ctypes.c_int32),
                ("ld_y", ctypes.c_int32), ("H", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("eps", ctypes.c_float),
                ("dropout_p", ctypes.c_float), ("training", ctypes.c_int32), ("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64),
                ("d_workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t)]


class AnceLayerTailGradArgs(ctypes.Structure):
    """include/ance_amd.h: the gradient side of ance_layer_tail_backward (every output nullable)."""
    _fields_ = [("dy", ctypes.c_void_p), ("dx", ctypes.c_void_p), ("dres", ctypes.c_void_p), ("dgamma", ctypes.c_void_p),
                ("dbeta", ctypes.c_void_p), ("dbias", ctypes.c_void_p), ("ld_dy", ctypes.c_int32), ("ld_dx", ctypes.c_int32),
                ("ld_dres", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AnceBiasGeluArgs(ctypes.Structure):
    """include/ance_amd.h: the arguments of ance_bias_gelu_forward / ance_bias_gelu_backward."""
    _fields_ = [("x", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("y", ctypes.c_void_p), ("ld_x", ctypes.c_int32),
                ("ld_y", ctypes.c_int32), ("N", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("d_workspace", ctypes.c_void_p),
                ("workspace_bytes", ctypes.c_size_t)]


class AnceBiasGeluGradArgs(ctypes.Structure):
    """include/ance_amd.h: the gradient side of ance_bias_gelu_backward."""
    _fields_ = [("dy", ctypes.c_void_p), ("dx", ctypes.c_void_p), ("dbias", ctypes.c_void_p), ("ld_dy", ctypes.c_int32),
                ("ld_dx", ctypes.c_int32)]


class AnceLayerTail16Args(ctypes.Structure):
    """include/ance_amd.h: the arguments of ance_layer_tail16_forward / ance_layer_tail16_backward (x and y16 in `dtype`)."""
    _fields_ = [("x", ctypes.c_void_p), ("res", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("gamma", ctypes.c_void_p),
                ("beta", ctypes.c_void_p), ("y", ctypes.c_void_p), ("y16", ctypes.c_void_p), ("ld_x", ctypes.c_int32),
                ("ld_res", ctypes.c_int32), ("ld_y", ctypes.c_int32), ("ld_y16", ctypes.c_int32), ("H", ctypes.c_int32),
                ("n_rows", ctypes.c_int32), ("dtype", ctypes.c_int32), ("eps", ctypes.c_float), ("dropout_p", ctypes.c_float),
                ("training", ctypes.c_int32), ("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64),
                ("d_workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t)]


class AnceLayerTail16GradArgs(ctypes.Structure):
    """include/ance_amd.h: the gradient side of ance_layer_tail16_backward (dy fp32 and dy16 each nullable, one given; every output
    nullable)."""
    _fields_ = [("dy", ctypes.c_void_p), ("dy16", ctypes.c_void_p), ("dx", ctypes.c_void_p), ("dres", ctypes.c_void_p),
                ("dgamma", ctypes.c_void_p), ("dbeta", ctypes.c_void_p), ("dbias", ctypes.c_void_p), ("ld_dy", ctypes.c_int32),
                ("ld_dy16", ctypes.c_int32), ("ld_dx", ctypes.c_int32), ("ld_dres", ctypes.c_int32)]


class AnceBiasGelu16Args(ctypes.Structure):
    """include/ance_amd.h: the arguments of ance_bias_gelu16_forward / ance_bias_gelu16_backward."""
    _fields_ = [("x", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("y", ctypes.c_void_p), ("ld_x", ctypes.c_int32),
                ("ld_y", ctypes.c_int32), ("N", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("dtype", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("d_workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t)]


class AnceBiasGelu16GradArgs(ctypes.Structure):
    """include/ance_amd.h: the gradient side of ance_bias_gelu16_backward."""
    _fields_ = [("dy", ctypes.c_void_p), ("dx", ctypes.c_void_p), ("dbias", ctypes.c_void_p), ("ld_dy", ctypes.c_int32),
                ("ld_dx", ctypes.c_int32)]


class AnceEmbedArgs(ctypes.Structure):
    """include/ance_amd.h: the arguments of ance_embed_forward / ance_embed_backward."""
    _fields_ = [("ids", ctypes.c_void_p), ("type_ids", ctypes.c_void_p), ("word", ctypes.c_void_p), ("pos", ctypes.c_void_p),
                ("type", ctypes.c_void_p), ("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("positions", ctypes.c_void_p), ("n_seq", ctypes.c_int32), ("L", ctypes.c_int32), ("H", ctypes.c_int32),
                ("vocab", ctypes.c_int32), ("max_pos", ctypes.c_int32), ("n_types", ctypes.c_int32),
                ("position_mode", ctypes.c_int32), ("padding_idx", ctypes.c_int32), ("eps", ctypes.c_float),
                ("dropout_p", ctypes.c_float), ("training", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64), ("d_workspace", ctypes.c_void_p),
                ("workspace_bytes", ctypes.c_size_t)]


class AnceEmbedGradArgs(ctypes.Structure):
    """include/ance_amd.h: the gradient side of ance_embed_backward (every output nullable; the tables zero-filled by the caller)."""
    _fields_ = [("dy", ctypes.c_void_p), ("dword", ctypes.c_void_p), ("dpos", ctypes.c_void_p), ("dtype", ctypes.c_void_p),
                ("dgamma", ctypes.c_void_p), ("dbeta", ctypes.c_void_p), ("word_keys", ctypes.c_void_p), ("word_perm", ctypes.c_void_p),
                ("pos_keys", ctypes.c_void_p), ("pos_perm", ctypes.c_void_p), ("type_keys", ctypes.c_void_p),
                ("type_perm", ctypes.c_void_p)]


class AncePackArgs(ctypes.Structure):
    """include/ance_amd.h: the arguments of ance_pack_tokens."""
    _fields_ = [("ids", ctypes.c_void_p), ("type_ids", ctypes.c_void_p), ("d_seq_len", ctypes.c_void_p), ("d_seq_off", ctypes.c_void_p),
                ("d_seq_kept", ctypes.c_void_p), ("d_dropped", ctypes.c_void_p), ("packed_ids", ctypes.c_void_p),
                ("packed_type_ids", ctypes.c_void_p), ("packed_positions", ctypes.c_void_p), ("n_seq", ctypes.c_int32),
                ("L", ctypes.c_int32), ("rows", ctypes.c_int32), ("position_mode", ctypes.c_int32), ("padding_idx", ctypes.c_int32),
                ("vocab", ctypes.c_int32), ("max_pos", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AncePackByIdArgs(ctypes.Structure):
    """include/ance_amd.h: the arguments of ance_pack_tokens_by_id."""
    _fields_ = [("ids", ctypes.c_void_p), ("d_seq_len", ctypes.c_void_p), ("d_seq_off", ctypes.c_void_p),
                ("d_seq_kept", ctypes.c_void_p), ("d_dropped", ctypes.c_void_p), ("packed_ids", ctypes.c_void_p),
                ("packed_positions", ctypes.c_void_p), ("n_seq", ctypes.c_int32), ("L", ctypes.c_int32), ("rows", ctypes.c_int32),
                ("padding_idx", ctypes.c_int32), ("vocab", ctypes.c_int32), ("max_pos", ctypes.c_int32)]


class AnceFirstRowsArgs(ctypes.Structure):
    """include/ance_amd.h: the arguments of ance_first_rows_gather / ance_first_rows_scatter."""
    _fields_ = [("rows_matrix", ctypes.c_void_p), ("first", ctypes.c_void_p), ("d_seq_off", ctypes.c_void_p),
                ("d_seq_kept", ctypes.c_void_p), ("ld_rows", ctypes.c_int32), ("ld_first", ctypes.c_int32), ("n_seq", ctypes.c_int32),
                ("rows", ctypes.c_int32), ("H", ctypes.c_int32), ("dtype", ctypes.c_int32)]


class AncePackedGatherSegment(ctypes.Structure):
    """include/ance_amd.h: one segment (tower) of ance_gather_batch_packed."""
    _fields_ = [("d_records", ctypes.c_void_p), ("n_records", ctypes.c_int64), ("d_index", ctypes.c_void_p),
                ("n_index", ctypes.c_int64), ("d_cum", ctypes.c_void_p), ("packed_ids", ctypes.c_void_p),
                ("packed_positions", ctypes.c_void_p), ("d_seq_off", ctypes.c_void_p), ("d_seq_kept", ctypes.c_void_p),
                ("d_dropped", ctypes.c_void_p), ("L", ctypes.c_int32), ("chunk_len", ctypes.c_int32), ("rows", ctypes.c_int32),
                ("position_mode", ctypes.c_int32), ("padding_idx", ctypes.c_int32), ("vocab", ctypes.c_int32),
                ("max_pos", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# include/ance_amd.h: ANCE_EMBED_SEGMENT_CHUNK (the library states the same number through ance_embed_segment_chunk), ANCE_EMBED_POSITION_*
EMBED_SEGMENT_CHUNK = 64
EMBED_POSITION_MODES = {"absolute": 0, "roberta": 1}

# rows per workgroup of the layer-tail and bias-GELU kernels (include/ance_amd.h: ANCE_LAYER_TAIL_ROWS_PER_WORKGROUP; the library
# states the same number through ance_layer_tail_rows_per_workgroup)
LAYER_TAIL_ROWS_PER_WORKGROUP = 16

# ance_gather_batch codes (include/ance_amd.h: ANCE_GATHER_*)
GATHER_MASK_LENGTH, GATHER_MASK_NONZERO = 0, 1
GATHER_TYPES_ZERO, GATHER_TYPES_LENGTH = 0, 1
GATHER_REFERENCE, GATHER_WIDE = 0, 1

# AnceEncoderDesc.precision (include/ance_amd.h: ANCE_PRECISION_*)
PRECISION_CODES = {None: 0, "split": 1, "fp16": 2, "fp32": 3}
PRECISION_NAMES = {1: "split", 2: "fp16", 3: "fp32"}


# name -> (restype, argtypes): every symbol include/ance_amd.h declares
SYMBOLS = {
    "ance_abi_version": (ctypes.c_int, []),
    "ance_last_error": (ctypes.c_char_p, []),
    "ance_profile_enable": (None, [ctypes.c_int]),
    "ance_profile_read": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                         ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]),
    "ance_ip_topk_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "ance_ip_topk": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_size_t, ctypes.c_void_p]),
    "ance_ip_topk_scan_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "ance_ip_topk_scan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_size_t, ctypes.c_void_p]),
    "ance_ip_index_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "ance_ip_index_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                           ctypes.c_void_p]),
    "ance_ip_topk_indexed_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "ance_ip_topk_indexed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "ance_topk_merge_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int64, ctypes.c_int]),
    "ance_topk_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.c_void_p]),
    "ance_ip_score_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ance_encoder_weight_bytes": (ctypes.c_size_t, [ctypes.POINTER(AnceEncoderDesc)]),
    "ance_encoder_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(AnceEncoderDesc)]),
    "ance_encoder_create": (ctypes.c_int, [ctypes.POINTER(AnceEncoderDesc), ctypes.POINTER(ctypes.c_void_p),
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                           ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "ance_encoder_destroy": (None, [ctypes.c_void_p]),
    "ance_encoder_precision": (ctypes.c_int, [ctypes.c_void_p]),
    "ance_encoder_range_faults": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "ance_encode_records": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "ance_encode_ids": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "ance_encoder_flops_per_sequence": (ctypes.c_double, [ctypes.c_int]),
    "ance_host_py_shuffle": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "ance_host_select_negatives": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                                  ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    "ance_host_write_ann_training": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
    "ance_reload_env": (None, []),
    "ance_debug_search_stamps": (None, [ctypes.c_void_p]),
    "ance_debug_gemm": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "ance_search_bad_image_calls": (ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    "ance_nll_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p]),
    "ance_debug_gemm_split": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ance_debug_gemm_hw": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(AnceGemmDebugArgs), ctypes.c_void_p]),
    "ance_debug_attention": (ctypes.c_int, [ctypes.POINTER(AnceAttnDebugArgs), ctypes.c_void_p]),
    "ance_lamb_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int64]),
    "ance_lamb_step": (ctypes.c_int, [ctypes.POINTER(AnceLambTensor), ctypes.c_int, ctypes.POINTER(AnceLambGroup), ctypes.c_int,
                                      ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "ance_lamb_clipped_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int64]),
    "ance_lamb_step_clipped": (ctypes.c_int, [ctypes.POINTER(AnceLambTensor), ctypes.c_int, ctypes.POINTER(AnceLambGroup), ctypes.c_int,
                                              ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_size_t, ctypes.c_void_p]),
    "ance_lamb_amp_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int64]),
    "ance_lamb_step_amp": (ctypes.c_int, [ctypes.POINTER(AnceLambTensor), ctypes.c_int, ctypes.POINTER(AnceLambGroup), ctypes.c_int,
                                          ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.c_void_p]),
    "ance_adamw_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int]),
    "ance_adamw_step": (ctypes.c_int, [ctypes.POINTER(AnceAdamwTensor), ctypes.c_int, ctypes.POINTER(AnceLambGroup), ctypes.c_int,
                                       ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "ance_nll_backward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    "ance_inbatch_nll_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    "ance_inbatch_nll_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                                ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                ctypes.c_void_p]),
    "ance_inbatch_nll_backward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                                 ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_size_t, ctypes.c_void_p]),
    "ance_gather_batch": (ctypes.c_int, [ctypes.POINTER(AnceGatherSegment), ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                         ctypes.c_void_p]),
    "ance_record_lengths": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    "ance_gather_batch_packed": (ctypes.c_int, [ctypes.POINTER(AncePackedGatherSegment), ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                                ctypes.c_void_p, ctypes.c_void_p]),
    "ance_attention_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "ance_attention_forward": (ctypes.c_int, [ctypes.POINTER(AnceAttnTrainArgs), ctypes.c_void_p]),
    "ance_attention_backward": (ctypes.c_int, [ctypes.POINTER(AnceAttnTrainArgs), ctypes.POINTER(AnceAttnGradArgs), ctypes.c_void_p]),
    "ance_attention16_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "ance_attention16_forward": (ctypes.c_int, [ctypes.POINTER(AnceAttn16Args), ctypes.c_void_p]),
    "ance_attention16_backward": (ctypes.c_int, [ctypes.POINTER(AnceAttn16Args), ctypes.POINTER(AnceAttn16GradArgs), ctypes.c_void_p]),
    "ance_layer_tail_rows_per_workgroup": (ctypes.c_int, []),
    "ance_layer_tail_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "ance_bias_gelu_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "ance_layer_tail_forward": (ctypes.c_int, [ctypes.POINTER(AnceLayerTailArgs), ctypes.c_void_p]),
    "ance_layer_tail_backward": (ctypes.c_int, [ctypes.POINTER(AnceLayerTailArgs), ctypes.POINTER(AnceLayerTailGradArgs), ctypes.c_void_p]),
    "ance_bias_gelu_forward": (ctypes.c_int, [ctypes.POINTER(AnceBiasGeluArgs), ctypes.c_void_p]),
    "ance_bias_gelu_backward": (ctypes.c_int, [ctypes.POINTER(AnceBiasGeluArgs), ctypes.POINTER(AnceBiasGeluGradArgs), ctypes.c_void_p]),
    "ance_layer_tail16_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "ance_bias_gelu16_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "ance_layer_tail16_forward": (ctypes.c_int, [ctypes.POINTER(AnceLayerTail16Args), ctypes.c_void_p]),
    "ance_layer_tail16_backward": (ctypes.c_int, [ctypes.POINTER(AnceLayerTail16Args), ctypes.POINTER(AnceLayerTail16GradArgs), ctypes.c_void_p]),
    "ance_bias_gelu16_forward": (ctypes.c_int, [ctypes.POINTER(AnceBiasGelu16Args), ctypes.c_void_p]),
    "ance_bias_gelu16_backward": (ctypes.c_int, [ctypes.POINTER(AnceBiasGelu16Args), ctypes.POINTER(AnceBiasGelu16GradArgs), ctypes.c_void_p]),
    "ance_embed_segment_chunk": (ctypes.c_int, []),
    "ance_embed_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "ance_embed_forward": (ctypes.c_int, [ctypes.POINTER(AnceEmbedArgs), ctypes.c_void_p]),
    "ance_embed_backward": (ctypes.c_int, [ctypes.POINTER(AnceEmbedArgs), ctypes.POINTER(AnceEmbedGradArgs), ctypes.c_void_p]),
    # the dropout entry points with the device stream {seed, base} (a null stream is the plain call)
    "ance_attention_forward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceAttnTrainArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "ance_attention_backward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceAttnTrainArgs), ctypes.POINTER(AnceAttnGradArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "ance_attention16_forward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceAttn16Args), ctypes.c_void_p, ctypes.c_void_p]),
    "ance_attention16_backward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceAttn16Args), ctypes.POINTER(AnceAttn16GradArgs), ctypes.c_void_p, ctypes.c_void_p]),
    # the first-query-row core (csrc/attention_row0.hip): AnceAttn16Args with dtype ANCE_DTYPE_F32, _F16 or _BF16
    "ance_attention_row0_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "ance_attention_row0_forward": (ctypes.c_int, [ctypes.POINTER(AnceAttn16Args), ctypes.c_void_p]),
    "ance_attention_row0_backward": (ctypes.c_int, [ctypes.POINTER(AnceAttn16Args), ctypes.POINTER(AnceAttn16GradArgs), ctypes.c_void_p]),
    "ance_attention_row0_forward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceAttn16Args), ctypes.c_void_p, ctypes.c_void_p]),
    "ance_attention_row0_backward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceAttn16Args), ctypes.POINTER(AnceAttn16GradArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "ance_layer_tail_forward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceLayerTailArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "ance_layer_tail_backward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceLayerTailArgs), ctypes.POINTER(AnceLayerTailGradArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "ance_layer_tail16_forward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceLayerTail16Args), ctypes.c_void_p, ctypes.c_void_p]),
    "ance_layer_tail16_backward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceLayerTail16Args), ctypes.POINTER(AnceLayerTail16GradArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "ance_embed_forward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceEmbedArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "ance_embed_backward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceEmbedArgs), ctypes.POINTER(AnceEmbedGradArgs), ctypes.c_void_p, ctypes.c_void_p]),
    # packed token rows of a fixed capacity (csrc/pack_rows.hip) and the embeddings over rows with given positions
    "ance_pack_tokens": (ctypes.c_int, [ctypes.POINTER(AncePackArgs), ctypes.c_void_p]),
    "ance_pack_tokens_by_id": (ctypes.c_int, [ctypes.POINTER(AncePackByIdArgs), ctypes.c_void_p]),
    "ance_embed_rows_forward": (ctypes.c_int, [ctypes.POINTER(AnceEmbedArgs), ctypes.c_void_p]),
    "ance_embed_rows_backward": (ctypes.c_int, [ctypes.POINTER(AnceEmbedArgs), ctypes.POINTER(AnceEmbedGradArgs), ctypes.c_void_p]),
    "ance_embed_rows_forward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceEmbedArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "ance_embed_rows_backward_dstream": (ctypes.c_int, [ctypes.POINTER(AnceEmbedArgs), ctypes.POINTER(AnceEmbedGradArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "ance_first_rows_gather": (ctypes.c_int, [ctypes.POINTER(AnceFirstRowsArgs), ctypes.c_void_p]),
    "ance_first_rows_scatter": (ctypes.c_int, [ctypes.POINTER(AnceFirstRowsArgs), ctypes.c_void_p]),
    "ance_dropout_stream_advance": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    # the fused optimizers' resident plans (tables built once into caller-owned host memory; steps that only launch) and the schedule
    "ance_lamb_plan_table_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int64]),
    "ance_lamb_plan_build": (ctypes.c_int, [ctypes.POINTER(AnceLambTensor), ctypes.c_int, ctypes.POINTER(AnceLambGroup), ctypes.c_void_p,
                                            ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64),
                                            ctypes.POINTER(ctypes.c_size_t)]),
    "ance_lamb_step_planned": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "ance_adamw_plan_table_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int64]),
    "ance_adamw_plan_build": (ctypes.c_int, [ctypes.POINTER(AnceAdamwTensor), ctypes.c_int, ctypes.POINTER(AnceLambGroup), ctypes.c_void_p,
                                             ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64),
                                             ctypes.POINTER(ctypes.c_size_t)]),
    "ance_adamw_step_planned": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                               ctypes.c_void_p]),
    "ance_lamb_step_scaled": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "ance_adamw_step_scaled": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                              ctypes.c_void_p]),
    "ance_loss_scale_update": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double,
                                              ctypes.c_int32, ctypes.c_void_p]),
    "ance_debug_staging_sends": (ctypes.c_longlong, []),
    "ance_linear_warmup_step": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                               ctypes.c_int64, ctypes.c_void_p]),
    "ance_pair_layout": (None, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                ctypes.POINTER(ctypes.c_float)]),
}

_lib = None


class AnceLibraryError(RuntimeError):
    pass


class AnceRangeError(AnceLibraryError):
    """The split (default) arithmetic met a value outside the fp16 range -- its stated precondition -- or produced NaN rows."""


def build(verbose=False, force=False):
    """Compile every HIP source for gfx950 into ance_amd/libance_amd.so (hipcc cross-compiles
    without a GPU).  force: rebuild every object (``make -B``) -- the tree ships its .o files to the GPU box, and a
    "does it build" check must not pass on stale objects."""
    cmd = ["make", "-C", CSRC, "-j8"] + (["-B"] if force else [])
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise AnceLibraryError("hipcc build of libance_amd.so failed")
    return LIB_PATH


def lib():
    """The loaded C-ABI library.  Raises AnceLibraryError (never falls back) when unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AnceLibraryError(
            "%s not found: the HIP extension is required (run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C ance_amd/csrc`); there is no CPU fallback" % LIB_PATH)
    try:
        import torch  # noqa: F401  -- loads the HIP runtime torch ships, so both share one runtime
    except Exception:  # pragma: no cover
        pass
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise AnceLibraryError("cannot load %s: %s" % (LIB_PATH, e))
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            raise AnceLibraryError("%s does not export %s" % (LIB_PATH, name))
        fn.restype = res
        fn.argtypes = args
    if L.ance_abi_version() != ABI_VERSION:
        raise AnceLibraryError("ABI version mismatch: library %d, binding %d" % (L.ance_abi_version(), ABI_VERSION))
    _lib = L
    return L


def reload_env():
    """The library reads its ANCE_* knobs once; call this after changing one inside a running process."""
    lib().ance_reload_env()


def check(rc, what):
    if rc != ANCE_OK:
        msg = lib().ance_last_error()
        raise AnceLibraryError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))


PROFILE_CATEGORIES = ("plan", "embed_ln", "gemm_qk", "gemm_vt", "attention", "gemm_attn_out", "layernorm",
                      "gemm_ffn1", "gemm_ffn2", "head", "ip_topk_scan", "topk_finalize", "ip_topk_rescore")


def profile_enable(on=True):
    lib().ance_profile_enable(1 if on else 0)


def profile_read():
    """{category: dict(ms=, work=, count=)} accumulated since profile_enable."""
    n = len(PROFILE_CATEGORIES)
    ms = (ctypes.c_double * n)()
    work = (ctypes.c_double * n)()
    cnt = (ctypes.c_longlong * n)()
    lib().ance_profile_read(ms, work, cnt, n)
    return {c: dict(ms=ms[i], work=work[i], count=int(cnt[i])) for i, c in enumerate(PROFILE_CATEGORIES)}


def current_stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_cuda_tensor(t, dtype, what):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise AnceLibraryError("%s must be a CUDA(HIP) tensor" % what)
    if t.dtype != dtype:
        raise AnceLibraryError("%s must have dtype %s, got %s" % (what, dtype, t.dtype))
    if not t.is_contiguous():
        raise AnceLibraryError("%s must be contiguous" % what)
    return t
