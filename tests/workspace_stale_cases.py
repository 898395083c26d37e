"""Cases of the stale-workspace tests: one per (block entry point, route), each at the smallest shape that reaches the
route, with ragged extents on purpose -- key counts that are multiples of neither 8 nor 32 (13, 33, 100), query counts 1,
33, 129, head widths below their padded width (dk < dkp), channel counts below padc(c), B = 2 wherever a batch stride
matters, stride-0 (broadcast) queries / latents.

Numpy only; shared by tests/test_workspace_stale_host.py (CPU: the labelled routes against csrc/pio_attn_route.h and
csrc/pio_block_route.h) and tests/test_workspace_stale_gpu.py (MI355X: every case on a zeroed, a 0xFF- and a 0x7B-filled
workspace).

Fields of a case
  id, entry   the C entry point is pio_<entry>
  policy      precision policy (perceiverio_pytorch_amd/runtime.py)
  cores       the AttnCore (csrc/pio_attn_route.h) of every attention call the entry point makes, in order: an encoder
              makes the cross-attend's, then ONE label for its self-attend blocks (they share the shape)
  fold        SelfFold family (csrc/pio_block_route.h) of the SelfAttention blocks, None where there is none
  plan        the workspace plan struct (csrc/pio_block_route.h) the entry point carves
  launches    launches per profiler class of ONE call (pio_prof_begin / pio_prof_end; csrc/pio_internal.h): 0 gemm_nt_256,
              1 batched gemm_nt_128, 2 layernorm / casts, 3 softmax_rows, 4 pack, 5 fused attention cores, 6 flat
              gemm_nt_128, 7 gemm_nt_stream, 8 gemm_nt_wide.  LITERALS: classes 2, 3 and 5 and the number of GEMMs are read
              off pio_blocks.hip launch by launch (the comment above each group); which GEMM class a projection lands in
              was recorded from one run on an MI355X -- a case that silently takes another route fails on them
  ragged      the extents of the case that are not whole tiles / pitches, or
  no_ragged   the reason why the route cannot take one
"""
import numpy as np

import primitive_cases as PC

ATTN_CORES = ("QKV_FLASH", "KVFOLD_XATTN", "KVFOLD_XTALL", "PAIR_FLASH", "PAIR_XATTN", "FLASH", "XATTN", "XTALL",
              "MATERIALISED")
FOLD_FAMILIES = ("NONE", "SMALL", "WIDE")
PLANS = ("AttentionPlan", "MlpPlan", "SelfPlan", "CrossPlan", "DecoderPlan")
FILLS = (0x00, 0xFF, 0x7B)     # zero: the baseline | NaN in every 16-bit / fp32 word, every mask byte "attend" | 61 280 / 1.3e36

CASES = []


def _add(**c):
    c.setdefault("fold", None)
    assert ("ragged" in c) != ("no_ragged" in c), c["id"]
    CASES.append(c)


# ----------------------------------------------------------------------------------------------------
# pio_mlp_fwd                                         (launches: cast of x | fc1, fc2)
# ----------------------------------------------------------------------------------------------------
_add(id="mlp_single_sweep", entry="mlp_fwd", policy="fp16", plan="MlpPlan", cores=(), B=2, T=33, C=60, widening=4,
     launches=[0, 0, 1, 0, 0, 0, 2, 0, 0], ragged="66 rows, 60 channels on a pitch of 64")
_add(id="mlp_split_activations", entry="mlp_fwd", policy="fp16x3", plan="MlpPlan", cores=(), B=2, T=33, C=60, widening=4,
     launches=[0, 0, 1, 0, 0, 0, 2, 0, 0], ragged="66 rows, 60 channels on a pitch of 64, (hi, lo) pairs")


# ----------------------------------------------------------------------------------------------------
# pio_attention_fwd
#   inputs: "three" q, k, v three arrays | "kv" k and v one array | "self" q, k, v one array (the entry point still casts
#   q and k into two carves: 2 casts, and never the q|k or q|k|v form -- those belong to the SelfAttention block)
#   masks: subset of kv, q, full, bias, probs; kv_dead: sample 1 has every key masked; q_bcast: stride-0 queries
#   launches, un-fused projections: 3 casts ("kv" / "self": 2 / 1) | q, k, out flat GEMMs + the batched V^T GEMM | the core
# ----------------------------------------------------------------------------------------------------
def _attn(id, policy, core, H, qk, v, Tq, Tk, launches, inputs="three", masks=(), cin=40, kv_in=None, B=2, **kw):
    _add(id=id, entry="attention_fwd", policy=policy, plan="AttentionPlan", cores=(core,), H=H, qk=qk, v=v, Tq=Tq, Tk=Tk,
         q_in=cin, kv_in=kv_in or cin, out=cin, B=B, inputs=inputs, masks=tuple(masks), launches=launches, **kw)


_WS_CORE = {"self_core": "FLASH", "cross_core_kv_mask_key_split": "XATTN", "tall_core": "XTALL",
            "materialised_full_mask": "MATERIALISED"}
_WS_LAUNCHES = {
    "self_core": [0, 1, 3, 0, 0, 1, 3, 0, 0],
    "cross_core_kv_mask_key_split": [0, 1, 3, 0, 0, 1, 3, 0, 0],
    "tall_core": [0, 1, 3, 0, 0, 1, 3, 0, 0],
    "materialised_full_mask": [0, 3, 3, 1, 0, 0, 3, 0, 0],     # batched: V^T, Q K^T, P V
}
for _name, _H, _qk, _vv, _Tq, _Tk, _mask, _fused, _softmax in PC.ATTN_WS_CASES:        # (reused, not copied)
    assert _WS_LAUNCHES[_name][5] == _fused and (_softmax is None or _WS_LAUNCHES[_name][3] == _softmax)
    _attn("ws_" + _name, "fp16", _WS_CORE[_name], _H, _qk, _vv, _Tq, _Tk, _WS_LAUNCHES[_name], cin=64,
          masks=(_mask,) if _mask else (),
          no_ragged="the shape is the row of primitive_cases.ATTN_WS_CASES, whose extents are whole tiles")

_attn("materialised_x3_full_mask_bias_probs", "fp16x3", "MATERIALISED", 2, 24, 24, 33, 13, [0, 3, 3, 1, 0, 0, 3, 0, 0],
      masks=("full", "bias", "probs"), ragged="Tk 13 (P pitch 16, V^T pitch 32), Tq 33, dk 12 < dkp 16, 40 channels")
_attn("pair_xattn_kv_mask_bcast_q", "fp16x3fq", "PAIR_XATTN", 2, 24, 40, 33, 100, [0, 1, 3, 0, 0, 1, 3, 0, 0],
      masks=("kv",), q_bcast=True, ragged="Tk 100 (V^T pitch 128), Tq 33, dk 12 < 16, dv 20 < 24, stride-0 queries")
_attn("pair_flash_self_input", "fp16x3fq", "PAIR_FLASH", 2, 56, 56, 129, 129, [0, 1, 2, 0, 0, 1, 3, 0, 0], inputs="self",
      ragged="Tq = Tk 129 (two query tiles, V^T pitch 160), dk 28 < 32")
_attn("x2af_output_pair", "fp16x2af", "XATTN", 2, 24, 24, 33, 100, [0, 1, 2, 0, 0, 1, 3, 0, 0], inputs="kv",
      ragged="Tk 100, Tq 33, dk 12 < 16; the core's output leaves as a pair")
_attn("bf16_flash", "bf16", "FLASH", 2, 56, 56, 129, 100, [0, 1, 2, 0, 0, 1, 3, 0, 0], inputs="kv",
      ragged="Tq 129, Tk 100 (V^T pitch 128), dk 28 < 32")
_attn("xattn_dead_sample_q_mask", "fp16", "XATTN", 2, 24, 40, 33, 33, [0, 1, 3, 0, 0, 1, 3, 0, 0], masks=("kv", "q"),
      kv_dead=True, ragged="Tq = Tk 33, dk 12 < 16, dv 20 < 24; sample 1 has no attendable key")
_attn("xtall_ragged", "fp16", "XTALL", 1, 90, 762, 33, 100, [0, 1, 3, 0, 0, 1, 3, 0, 0],
      ragged="Tk 100 of the kernel's 512, Tq 33, dk 90 < 96, dv 762 < 768")
_attn("xattn_key_split", "fp16", "XATTN", 2, 24, 40, 33, 520, [0, 1, 3, 0, 0, 1, 3, 0, 0],
      ragged="Tk 520: 17 key tiles in two splits of 9 and 8, the last tile 8 keys; Tq 33")
# K / V fold: 2 casts + the 16-bit transpose of the inputs (counted as a cast) | Q, Q Wk, out | the core
_attn("kvfold_xattn", "fp16", "KVFOLD_XATTN", 1, 44, 44, 8, 100, [0, 0, 3, 0, 0, 1, 3, 0, 0], inputs="kv", kv_in=44,
      ragged="Tk 100 (V^T pitch 128), Tq 8, 44 channels = dk < dkp 48")
_attn("kvfold_xtall", "fp16", "KVFOLD_XTALL", 1, 762, 762, 8, 100, [0, 0, 3, 0, 0, 1, 3, 0, 0], inputs="kv", kv_in=762,
      ragged="Tk 100 of the kernel's 512, Tq 8, 762 channels = dk < dkp 768")


# ----------------------------------------------------------------------------------------------------
# pio_self_attention_fwd            (ln_fold: pio_call_opts_t.ln_fold; alias: `out` is `x`)
#   launches as tests/test_block_route_gpu.py: un-folded 2 casts, 4 flat GEMMs, 1 core; folded 1 row-statistics cast
# ----------------------------------------------------------------------------------------------------
def _self(id, policy, core, fold, C, H, B, N, ln_fold, launches, **kw):
    _add(id=id, entry="self_attention_fwd", policy=policy, plan="SelfPlan", cores=(core,), fold=fold, C=C, H=H, B=B, N=N,
         ln_fold=ln_fold, launches=launches, **kw)


_self("self_unfolded_qkv_flash", "fp16", "QKV_FLASH", "NONE", 60, 2, 2, 129, 0, [0, 0, 2, 0, 0, 1, 4, 0, 0],
      ragged="N 129, 60 channels on a pitch of 64, dk 30 < 32")
_self("self_out_aliases_x", "fp16", "QKV_FLASH", "NONE", 60, 2, 2, 129, 0, [0, 0, 2, 0, 0, 1, 4, 0, 0], alias=True,
      ragged="N 129, 60 channels on a pitch of 64, dk 30 < 32")
_self("self_small_fold", "fp16", "QKV_FLASH", "SMALL", 512, 8, 2, 300, 0, [0, 0, 1, 0, 0, 1, 4, 0, 0],
      ragged="N 300: 600 rows, neither a multiple of the 128-row query tile nor of the 64-row GEMM tile")
_self("self_wide_fold_forced", "fp16", "QKV_FLASH", "WIDE", 512, 8, 2, 1024, 3, [0, 0, 1, 0, 0, 1, 0, 0, 4],
      no_ragged="the wide family starts at 2048 rows and 2048 x 512 is the largest shape of this file; the fold takes "
                "channel counts that are multiples of 256 only")
_self("self_x3_materialised", "fp16x3", "MATERIALISED", "NONE", 60, 2, 2, 33, 0, [0, 3, 2, 1, 0, 0, 5, 0, 0],
      ragged="N 33 (P pitch 40, V^T pitch 64), 60 channels on 64, dk 30 < 32")


# ----------------------------------------------------------------------------------------------------
# pio_cross_attention_fwd           (same_input: inputs_q is inputs_kv)
#   launches: LN_kv, LN_q, LN2 | q, k, out, fc1, fc2 flat + V^T batched | the core
# ----------------------------------------------------------------------------------------------------
def _cross(id, core, q_in, kv_in, H, Tq, Tk, resid, launches, masks=(), **kw):
    _add(id=id, entry="cross_attention_fwd", policy="fp16", plan="CrossPlan", cores=(core,), q_in=q_in, kv_in=kv_in, H=H,
         B=2, Tq=Tq, Tk=Tk, resid=resid, masks=tuple(masks), launches=launches, **kw)


_cross("cross_query_residual", "XATTN", 60, 44, 2, 33, 100, True, [0, 1, 3, 0, 0, 1, 5, 0, 0],
       ragged="Tk 100, Tq 33, 60 / 44 channels on 64 / 48, dk 22 < 24")
_cross("cross_no_residual_bcast_q", "XATTN", 60, 44, 2, 33, 100, False, [0, 1, 3, 0, 0, 1, 5, 0, 0], q_bcast=True,
       ragged="Tk 100, Tq 33, dk 22 < 24, stride-0 queries")
_cross("cross_kv_mask", "XATTN", 60, 44, 2, 1, 13, True, [0, 1, 3, 0, 0, 1, 5, 0, 0], masks=("kv",),
       ragged="Tq 1, Tk 13, dk 22 < 24")
# inputs_q is inputs_kv: layer_norm_q and layer_norm_kv are two LayerNorms, so the block normalises the array twice into
# two carves and attention_core never sees q and k reading one 16-bit input -- the q|k form is out of this entry point's
# reach (AttnCall.same_qk is false); the case pins that: two projection GEMMs, the self-attention kernel on V^T
_cross("cross_same_input", "FLASH", 60, 60, 2, 33, 33, True, [0, 1, 3, 0, 0, 1, 5, 0, 0], same_input=True,
       ragged="Tq = Tk 33, 60 channels on 64, dk 30 < 32")


# ----------------------------------------------------------------------------------------------------
# encoders: L = 2 layers x 2 blocks (the ping-pong / in-place streams are reused inside one call), stride-0 latents
#   one entry point, pio_encoder_fwd; a case's fields fill its record: tail (inputs_tail), per_block, ln_fold (opts), input_mask
#   launches: cross-attend as above (un-fused: 3 casts, 5 flat + 1 batched, core) + 4 self-attend blocks
# ----------------------------------------------------------------------------------------------------
def _enc(id, entry, cores, fold, launches, C_in=44, M=100, N=33, D=60, H=2, policy="fp16", **kw):
    _add(id=id, entry=entry, policy=policy, plan="CrossPlan+SelfPlan", cores=cores, fold=fold, C_in=C_in, M=M, N=N, D=D,
         H=H, B=2, L=2, blocks=2, launches=launches, **kw)


_enc("encoder_input_mask", "encoder_fwd", ("XATTN", "QKV_FLASH"), "NONE", [0, 1, 11, 0, 0, 5, 21, 0, 0], input_mask=True,
     ragged="M 100, N 33, 44 / 60 channels on 48 / 64, dk 30 < 32")
# un-masked single-head cross-attend over 200 keys for 33 stride-0 query rows: the K / V fold (Q, Q Wk, out, fc1, fc2; the
# 16-bit transpose counts as a cast)
_enc("encoder_split_tail_kvfold", "encoder_fwd", ("KVFOLD_XATTN", "QKV_FLASH"), "NONE",
     [0, 0, 12, 0, 0, 5, 21, 0, 0], tail=6, ragged="M 100, N 33, inputs as 38 + 6 channels of a [1, M, 6] table")
_enc("encoder_per_block_images", "encoder_fwd", ("KVFOLD_XATTN", "QKV_FLASH"), "NONE",
     [0, 0, 12, 0, 0, 5, 21, 0, 0], per_block=1, ragged="M 100, N 33, 44 / 60 channels on 48 / 64")
# the folded stack: ONE row-statistics cast for four blocks, the 16-bit residual stream updated in place
_enc("encoder_opts_fold_stack", "encoder_fwd", ("XATTN", "QKV_FLASH"), "SMALL", [0, 1, 4, 0, 0, 5, 21, 0, 0],
     N=300, D=512, H=8, input_mask=True, ln_fold=0, ragged="M 100, N 300 (600 rows), 44 input channels on 48")


# ----------------------------------------------------------------------------------------------------
# decoders: one single-head cross-attend (queries x latents), optional final Linear on y16 rows of pitch padc(Dq)
#   one entry point, pio_decoder_fwd; a case's fields fill its record: tail (query_tail), qcache (q16_hi / q16_lo), query_mask
#   launches: LN_kv, LN_q, LN2 | q, k, out, fc1, fc2 (+ final) flat + V^T batched | the core
# ----------------------------------------------------------------------------------------------------
def _dec(id, entry, launches, final, resid, policy="fp16", Dq=60, D=44, Q=33, N=13, out=10, **kw):
    _add(id=id, entry=entry, policy=policy, plan="DecoderPlan", cores=("XATTN",), Dq=Dq, D=D, Q=Q, N=N, B=2,
         out=out if final else Dq, final=final, resid=resid, launches=launches, **kw)


_dec("decoder_final_query_mask", "decoder_fwd", [0, 1, 3, 0, 0, 1, 6, 0, 0], True, False, query_mask=True,
     ragged="Q 33, 13 latents, 60 query channels on y16 rows of pitch 64, 44 = dk < 48")
_dec("decoder_no_final_query_mask", "decoder_fwd", [0, 1, 3, 0, 0, 1, 5, 0, 0], False, True, query_mask=True,
     ragged="Q 33, 13 latents, 60 / 44 channels on 64 / 48")
_dec("decoder_split_query", "decoder_fwd", [0, 1, 3, 0, 0, 1, 6, 0, 0], True, False, tail=6,
     ragged="Q 33, 13 latents, queries as 54 + 6 channels of a [1, Q, 6] table")
_dec("decoder_qcache", "decoder_fwd", [0, 1, 3, 0, 0, 1, 6, 0, 0], True, False, policy="fp16x2af", q_bcast=True,
     qcache=True, launches_valid=[0, 1, 2, 0, 0, 1, 5, 0, 0],      # q16_valid = 1: no LayerNorm_q, no proj_q
     ragged="Q 33, 13 latents, stride-0 queries, the projected queries as a caller-owned (hi, lo) pair")

BY_ID = {c["id"]: c for c in CASES}

# the sequence test: this masked key-split cross-attend first, then `SEQUENCE_SECOND` on the same buffer
SEQUENCE_FIRST = dict(id="seq_masked_key_split", entry="attention_fwd", policy="fp16", plan="AttentionPlan", cores=("XATTN",),
                      H=2, qk=24, v=40, Tq=129, Tk=1000, q_in=40, kv_in=40, out=40, B=2, inputs="three", masks=("kv", "q"),
                      launches=[0, 1, 3, 0, 0, 1, 3, 0, 0], fold=None, ragged="Tk 1000: 32 key tiles in 4 splits; Tq 129")
SEQUENCE_SECOND = "xattn_key_split"


def rng_for(case, salt=0):
    import zlib
    return np.random.default_rng([zlib.crc32(case["id"].encode()), salt])
