"""ctypes binding of libpio_hip.so (C-ABI declared in include/pio_hip.h).

The library is built in-tree (``perceiverio_pytorch_amd/libpio_hip.so``) by ``__graft_entry__.build()``
or ``make -C perceiverio_pytorch_amd/csrc``.  There is NO fallback: if the shared object is missing or
fails to load, importing the compute modules raises -- the hot path only exists as HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PIO_LIB_PATH", os.path.join(_HERE, "libpio_hip.so"))  # override: A/B builds only
CSRC = os.path.join(_HERE, "csrc")

PIO_DT_F16 = 0
PIO_DT_BF16 = 1

PIO_OK = 0
_ERRORS = {-1: "PIO_E_SHAPE", -2: "PIO_E_ALIGN", -3: "PIO_E_ARCH", -4: "PIO_E_WORKSPACE", -5: "PIO_E_LAUNCH",
           -6: "PIO_E_ARG", -7: "PIO_E_RANGE"}


class PioError(RuntimeError):
    pass


class Linear(C.Structure):
    _fields_ = [("w_hi", C.c_void_p), ("w_lo", C.c_void_p), ("bias", C.c_void_p), ("n", C.c_int32), ("k", C.c_int32),
                ("lo_row0", C.c_int32)]


class LayerNorm(C.Structure):
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p), ("c", C.c_int32), ("eps", C.c_float)]


class Attention(C.Structure):
    _fields_ = [("q", Linear), ("k", Linear), ("v", Linear), ("o", Linear), ("heads", C.c_int32),
                ("dk", C.c_int32), ("dv", C.c_int32), ("dkp", C.c_int32), ("dvp", C.c_int32),
                ("q_in", C.c_int32), ("k_in", C.c_int32), ("v_in", C.c_int32), ("out", C.c_int32), ("dtype", C.c_int32),
                ("act_split", C.c_int32), ("qk", Linear), ("qkv", Linear), ("kq", Linear), ("vo", Linear)]


class Mlp(C.Structure):
    _fields_ = [("fc1", Linear), ("fc2", Linear), ("in_", C.c_int32), ("hidden", C.c_int32), ("out", C.c_int32),
                ("dtype", C.c_int32), ("act_split", C.c_int32)]


class LnFold(C.Structure):
    _fields_ = [("qkv", Linear), ("qkv_c", C.c_void_p), ("fc1", Linear), ("fc1_c", C.c_void_p),
                ("range_flag", C.c_void_p)]


class SelfAttention(C.Structure):
    _fields_ = [("ln1", LayerNorm), ("ln2", LayerNorm), ("attn", Attention), ("mlp", Mlp), ("fold", LnFold)]


class CrossAttention(C.Structure):
    _fields_ = [("ln_q", LayerNorm), ("ln_kv", LayerNorm), ("ln2", LayerNorm), ("attn", Attention), ("mlp", Mlp),
                ("use_query_residual", C.c_int32)]


class Tensor3(C.Structure):
    _fields_ = [("data", C.c_void_p), ("stride_b", C.c_int64), ("stride_t", C.c_int64), ("B", C.c_int32),
                ("T", C.c_int32), ("C", C.c_int32)]


class CallOpts(C.Structure):
    """pio_call_opts_t: per-call LayerNorm-fold mode and CU budget."""
    _fields_ = [("ln_fold", C.c_int32), ("cu_budget", C.c_int32)]


class EncoderCall(C.Structure):
    """pio_encoder_call_t: one pio_encoder_fwd call (a zeroed field is its default: no tail, no mask, shared images)."""
    _fields_ = [("cross", C.POINTER(CrossAttention)), ("layers", C.POINTER(SelfAttention)), ("L", C.c_int32),
                ("num_blocks", C.c_int32), ("per_block", C.c_int32), ("inputs", C.POINTER(Tensor3)),
                ("inputs_tail", C.POINTER(Tensor3)), ("latents", C.POINTER(Tensor3)), ("input_mask", C.c_void_p),
                ("out", C.c_void_p), ("opts", CallOpts)]


class DecoderCall(C.Structure):
    """pio_decoder_call_t: one pio_decoder_fwd call (a zeroed field is its default: no final layer, tail, mask, cache)."""
    _fields_ = [("cross", C.POINTER(CrossAttention)), ("final_layer", C.POINTER(Linear)), ("final_out", C.c_int32),
                ("query", C.POINTER(Tensor3)), ("query_tail", C.POINTER(Tensor3)), ("latents", C.POINTER(Tensor3)),
                ("query_mask", C.c_void_p), ("out", C.c_void_p), ("q16_hi", C.c_void_p), ("q16_lo", C.c_void_p),
                ("q16_valid", C.c_int32)]


PIO_TOKENS_ROWS = 0
PIO_TOKENS_S2D = 1
PIO_MAX_TOKEN_SEGMENTS = 8


class TokenSegment(C.Structure):
    """pio_token_segment_t: one row segment of pio_assemble_tokens (features | position table | padding, optional token)."""
    _fields_ = [("feature", C.c_void_p), ("table", C.c_void_p), ("pad", C.c_void_p), ("token", C.c_void_p),
                ("sb", C.c_int64), ("sm", C.c_int64), ("st", C.c_int64), ("sc", C.c_int64), ("sy", C.c_int64),
                ("ldt", C.c_int64), ("kind", C.c_int32), ("row0", C.c_int32), ("M", C.c_int32), ("C1", C.c_int32),
                ("C2", C.c_int32), ("T", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("s", C.c_int32)]


PIO_QUERY_FOURIER = 0
PIO_QUERY_TABLE = 1
PIO_MAX_QUERY_SEGMENTS = 4


class QuerySegment(C.Structure):
    """pio_query_segment_t: one row segment of pio_build_queries (Fourier features of index points, or a table | padding)."""
    _fields_ = [("axis", C.c_void_p * 3), ("bands", C.c_void_p), ("points", C.c_void_p), ("table", C.c_void_p),
                ("pad", C.c_void_p), ("start", C.c_int64), ("ldb", C.c_int64), ("ldt", C.c_int64), ("kind", C.c_int32),
                ("row0", C.c_int32), ("M", C.c_int32), ("d", C.c_int32), ("dims", C.c_int32 * 3), ("K", C.c_int32),
                ("concat_pos", C.c_int32), ("sine_only", C.c_int32), ("C", C.c_int32)]


PIO_MAX_HEAD_SEGMENTS = 4


class HeadSegment(C.Structure):
    """pio_head_segment_t: one row segment of pio_project_heads (rows of the decoder output through one narrow fp32 head)."""
    _fields_ = [("row0", C.c_int32), ("rows", C.c_int32), ("w", C.c_void_p), ("ldw", C.c_int64), ("bias", C.c_void_p),
                ("n_out", C.c_int32), ("y", C.c_void_p), ("y_sb", C.c_int64), ("y_rs", C.c_int64)]


PIO_MAX_BLEND_AXIS = 64
PIO_MAX_BLEND_GROUPS = 64


class FlowBlend(C.Structure):
    """pio_flow_blend_t: the tile groups, corners and sizes of pio_flow_blend_tiles (passed by value into the kernel)."""
    _fields_ = [("group", C.c_void_p * PIO_MAX_BLEND_GROUPS), ("sn", C.c_int64), ("sc", C.c_int64), ("sy", C.c_int64),
                ("sx", C.c_int64), ("ngroups", C.c_int32), ("tiles_per_group", C.c_int32), ("ny", C.c_int32),
                ("nx", C.c_int32), ("ys", C.c_int32 * PIO_MAX_BLEND_AXIS), ("xs", C.c_int32 * PIO_MAX_BLEND_AXIS),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("h", C.c_int32), ("w", C.c_int32)]


# descriptors per pio_prepare_images launch: 32 x 64 bytes of the kernel's own table + ~100 bytes of sizes, mean and std keep
# the argument block well inside HIP's 4 KB; longer lists are launched in groups (fused_io.prepare_images)
PIO_MAX_IMAGE_SOURCES = 32
PIO_IMAGE_MAX_REDUCTION = 40
PIO_IMAGE_U8 = 0
PIO_IMAGE_F32 = 1
PIO_MEDIA_U8 = 0
PIO_MEDIA_S16 = 1
# output channels of pio_conv1x1_tokens: a lane keeps 4 C weights + 4 biases per 256 of them in registers
PIO_CONV1X1_MAX_N = 1024


class ImageSource(C.Structure):
    """pio_image_src_t: n images of one size, layout and dtype of pio_prepare_images, read in place, with their crop box."""
    _fields_ = [("data", C.c_void_p), ("sb", C.c_int64), ("sc", C.c_int64), ("sy", C.c_int64), ("sx", C.c_int64),
                ("dtype", C.c_int32), ("n", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("y0", C.c_int32), ("x0", C.c_int32), ("ch", C.c_int32), ("cw", C.c_int32)]


class Gemm(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("A_lo", C.c_void_p), ("B_lo", C.c_void_p), ("C", C.c_void_p),
                ("C_lo", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("lda", C.c_int64), ("ldb", C.c_int64), ("ldc", C.c_int64),
                ("batch", C.c_int32), ("nh", C.c_int32),
                ("sAb", C.c_int64), ("sAh", C.c_int64), ("sBb", C.c_int64), ("sBh", C.c_int64),
                ("sCb", C.c_int64), ("sCh", C.c_int64),
                ("bias", C.c_void_p), ("bias_mode", C.c_int32), ("act", C.c_int32), ("alpha", C.c_float),
                ("R", C.c_void_p), ("ldr", C.c_int64), ("r_stride_b", C.c_int64),
                ("r_rows_per_batch", C.c_int32), ("out_f32", C.c_int32), ("n_store", C.c_int32),
                ("dtype", C.c_int32),
                ("X16", C.c_void_p), ("ld16", C.c_int64), ("row_part", C.c_void_p), ("ln_part", C.c_void_p),
                ("ln_c", C.c_void_p), ("ln_eps", C.c_float),
                ("X16_lo", C.c_void_p), ("R16_hi", C.c_void_p), ("R16_lo", C.c_void_p), ("b_lo_n0", C.c_int32),
                ("range_flag", C.c_void_p), ("ln_slots", C.c_int32), ("row_slot_w", C.c_int32)]


# name -> (restype, argtypes); must list EVERY function declared in include/pio_hip.h
# (tests/test_capi_symbols.py parses the header and checks this table and the .so against it).
P = C.POINTER
_vp, _i32, _i64, _sz, _f = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_float
SIGNATURES = {
    "pio_version": (C.c_int, []),
    "pio_arch_ok": (C.c_int, []),
    "pio_error_string": (C.c_char_p, [C.c_int]),
    "pio_prof_begin": (C.c_int, [_i32]),
    "pio_prof_end": (C.c_int, [P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_int64)]),
    "pio_qk_logit_absmax": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _i64, _vp, _vp,
                                      _vp, _vp, _vp]),
    "pio_logit_probe_begin": (C.c_int, [_vp, _i32]),
    "pio_logit_probe_end": (C.c_int, []),
    "pio_absmax16": (C.c_int, [_i32, _vp, _i64, _i32, _i64, _i32, _i64, _vp, _vp]),
    "pio_range_probe_begin": (C.c_int, [_vp, _i32]),
    "pio_range_probe_mark": (C.c_int, [_i32]),
    "pio_range_probe_end": (C.c_int, [P(_i32), P(_i32), _i32]),
    "pio_pad8": (_i32, [_i32]),
    "pio_padc": (_i32, [_i32]),
    "pio_gemm_kernel_override": (C.c_int, [C.c_int]),
    "pio_ln_fold_enable": (C.c_int, [C.c_int]),
    "pio_set_cu_budget": (C.c_int, [_i32]),
    "pio_packed_weight_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "pio_pack_linear": (C.c_int, [_vp, _vp, _i32, _i32, _i64, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "pio_layernorm_cast": (C.c_int, [P(Tensor3), P(LayerNorm), _vp, _vp, _i32, _i32, _vp]),
    "pio_layernorm_cast_cat": (C.c_int, [P(Tensor3), P(Tensor3), P(LayerNorm), _vp, _vp, _i32, _i32, _vp]),
    "pio_rowstats_cast": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "pio_transpose16": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _i64, _vp]),
    "pio_bn_relu_maxpool_tokens": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "pio_flow_patch_tokens": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32,
                                        _i32, _i32, _vp]),
    "pio_conv1x1_tokens": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32,
                                     _i32, _i32, _vp]),
    "pio_assemble_tokens": (C.c_int, [P(TokenSegment), _i32, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "pio_build_queries": (C.c_int, [P(QuerySegment), _i32, _vp, _i64, _i32, _i32, _vp]),
    "pio_project_heads": (C.c_int, [P(HeadSegment), _i32, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "pio_vocab_topk": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pio_embed_tokens": (C.c_int, [_vp, _i32, _i64, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i32,
                                   _i32, _i32, _vp]),
    "pio_flow_blend_tiles": (C.c_int, [P(FlowBlend), _vp, _i64, _i64, _i64, _vp]),
    "pio_flow_to_image": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _f, _i32, _i32, _vp, _vp, _vp]),
    "pio_finish_media": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "pio_prepare_images": (C.c_int, [P(ImageSource), _i32, _i32, _i32, _i32, _i32, _i32, P(_f), P(_f), _vp, _i64, _vp]),
    "pio_gemm_nt": (C.c_int, [P(Gemm), _vp]),
    "pio_softmax_rows": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _f, _vp, _vp, _vp, _vp, _i32, _vp]),
    "pio_flash_attention": (C.c_int, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i64, _i64, _i64,
                                      _i64, _i64, _i64, _i64, _i64, _i32, _vp]),
    "pio_flash_attention_pair_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "pio_flash_attention_pair": (C.c_int, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32,
                                           _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _i32, _vp, _sz,
                                           _vp]),
    "pio_attention_workspace_bytes": (_sz, [P(Attention), _i32, _i32, _i32]),
    "pio_attention_fwd": (C.c_int, [P(Attention), P(Tensor3), P(Tensor3), P(Tensor3), _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _sz, _vp]),
    "pio_mlp_workspace_bytes": (_sz, [P(Mlp), _i64]),
    "pio_mlp_fwd": (C.c_int, [P(Mlp), P(Tensor3), _vp, _vp, _sz, _vp]),
    "pio_self_attention_workspace_bytes": (_sz, [P(SelfAttention), _i32, _i32]),
    "pio_self_attention_fwd": (C.c_int, [P(SelfAttention), P(Tensor3), _vp, _vp, _vp, _vp, _vp, _vp, P(CallOpts), _vp, _sz,
                                         _vp]),
    "pio_cross_attention_workspace_bytes": (_sz, [P(CrossAttention), _i32, _i32, _i32]),
    "pio_cross_attention_fwd": (C.c_int, [P(CrossAttention), P(Tensor3), P(Tensor3), _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _sz, _vp]),
    "pio_encoder_workspace_bytes": (_sz, [P(CrossAttention), P(SelfAttention), _i32, _i32, _i32, _i32]),
    "pio_encoder_fwd": (C.c_int, [P(EncoderCall), _vp, _sz, _vp]),
    "pio_decoder_workspace_bytes": (_sz, [P(CrossAttention), P(Linear), _i32, _i32, _i32]),
    "pio_decoder_qcache_bytes": (_sz, [P(CrossAttention), _i32, _i32]),
    "pio_decoder_fwd": (C.c_int, [P(DecoderCall), _vp, _sz, _vp]),
}

_lib = None


def build(verbose: bool = False) -> str:
    """Compile libpio_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    out = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if verbose or out.returncode:
        print(out.stdout[-4000:])
        print(out.stderr[-4000:])
    if out.returncode:
        raise PioError("building libpio_hip.so failed")
    return LIB_PATH


def lib() -> C.CDLL:
    """The loaded library with argtypes set.  Raises loudly if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PioError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU / eager fallback for the PerceiverIO hot path)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)      # AttributeError => stale .so: fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(code: int, what: str = "") -> None:
    if code != PIO_OK:
        raise PioError(f"{what}: {_ERRORS.get(code, code)}")
