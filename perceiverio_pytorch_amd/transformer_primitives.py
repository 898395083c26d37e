"""MI355X-native counterparts of the reference's ``perceiver_io/transformer_primitives.py``.

Same class names, constructor arguments, sub-module names (=> identical ``state_dict`` keys) and
``forward`` signatures as the reference; the arithmetic runs in ``libpio_hip.so`` (hand-written gfx950
kernels behind the C-ABI of ``include/pio_hip.h``).  Forward / inference only: there is no autograd
through the HIP path and no CPU fallback -- a CPU tensor raises.

Reference lines (under /root/reference/perceiver_io/transformer_primitives.py):
  make_cross_attention_mask 10-15 | Attention 18-180 | MLP 183-216 | SelfAttention 219-297 |
  CrossAttention 300-406
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import probe as LP
from . import runtime as R


# --------------------------------------------------------------------------------------------------
# init helpers (the reference takes these from timm; only the distribution matters, and only at init)
# --------------------------------------------------------------------------------------------------
def variance_scaling_(tensor: torch.Tensor, scale: float = 1.0, mode: str = "fan_in",
                      distribution: str = "truncated_normal") -> torch.Tensor:
    fan_out, fan_in = tensor.shape[0], int(math.prod(tensor.shape[1:]))
    denom = {"fan_in": fan_in, "fan_out": fan_out, "fan_avg": (fan_in + fan_out) / 2}[mode]
    variance = scale / denom
    with torch.no_grad():
        if distribution == "truncated_normal":
            std = math.sqrt(variance) / 0.87962566103423978
            nn.init.trunc_normal_(tensor, std=std, a=-2 * std, b=2 * std)
        elif distribution == "normal":
            tensor.normal_(std=math.sqrt(variance))
        elif distribution == "uniform":
            bound = math.sqrt(3 * variance)
            tensor.uniform_(-bound, bound)
        else:
            raise ValueError(f"invalid distribution {distribution}")
    return tensor


def lecun_normal_(tensor: torch.Tensor) -> torch.Tensor:
    return variance_scaling_(tensor, mode="fan_in", distribution="truncated_normal")


def make_cross_attention_mask(query_mask: torch.Tensor, kv_mask: torch.Tensor) -> torch.Tensor:
    """mask[b,i,j] = query_mask[b,i] & kv_mask[b,j] (reference :10-15).  Pure index bookkeeping; the
    encoder/decoder never materialise it -- they hand the two vectors to the kernels instead."""
    batch_size, query_len = query_mask.shape
    _, key_len = kv_mask.shape
    mask = query_mask[:, :, None] & kv_mask[:, None, :] if query_mask.dtype == torch.bool and \
        kv_mask.dtype == torch.bool else torch.einsum("bi,bj->bij", (query_mask, kv_mask))
    assert mask.shape == (batch_size, query_len, key_len)
    return mask


# per-head (qk, v) widths, padded to 8, that the fused self-attention kernel covers with V read row-major (pio_flash.hip):
# for these q | k | v come out of ONE GEMM over a stacked weight image
FUSED_SELF_HEADS = {(128, 128), (64, 64), (32, 32), (32, 160)}


def _no_training_dropout(mod: nn.Module, *probs: float) -> None:
    if mod.training and any(p > 0.0 for p in probs):
        raise NotImplementedError("the HIP path is forward/inference only: call .eval() or use dropout_prob=0")


def _block_call(entry, ws_entry, ws_args, d, tensors, dims, out_channels, mask, bias, return_matrix, deps, **opts):
    """The common tail of the three block forwards: full mask to bytes, bias broadcast over `dims` = (B, H, Tq, Tk), the
    `out` / `probs` buffers, the workspace of `ws_entry(d, *ws_args)`, the launch of `entry` on `tensors` (its descriptor
    and input tensors lead every block prototype; the rest goes by name), and the result tied to `deps`
    (runtime.forward_only).  Returns out, or (probs, out) with `return_matrix`.  `opts`: what the entry takes beyond the
    common parameters (pio_self_attention_fwd: opts, its pio_call_opts_t pointer)."""
    B, H, Tq, Tk = dims
    dev = tensors[0].device
    fm, fm_ptr = R.mask_u8(mask, (B, Tq, Tk), dev)
    bias_t = None
    if bias is not None:
        bias_t = torch.broadcast_to(bias.to(device=dev, dtype=torch.float32), dims).contiguous()
    out = torch.empty((B, Tq, out_channels), dtype=torch.float32, device=dev)
    probs = torch.empty(dims, dtype=torch.float32, device=dev) if return_matrix else None
    ws = R.workspace(dev, getattr(L.lib(), ws_entry)(d, *ws_args))
    LP.expect("attention")
    R.call_named(dev, entry, d, *[R.tensor3(t) for t in tensors], kv_mask=None, q_mask=None, full_mask=fm_ptr,
                 attention_bias=bias_t.data_ptr() if bias_t is not None else None, out=out.data_ptr(),
                 probs_out=probs.data_ptr() if probs is not None else None, workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                 **opts)
    out = R.forward_only(out, *deps)
    return (probs, out) if return_matrix else out


class _HipModule(R.PackedOwner):
    """A block module: its descriptor (and the images behind it) under its parameters' key."""

    def _desc(self):
        return self._packed.get(R.param_key(*self._params()), self._build_desc)

    def _child_entries(self):
        """For a parent's `keep`.  INVARIANT: parent entry alive => child images alive.  The parent's descriptor holds raw
        pointers into the images of attention / mlp; it names the children's current entries -- the ones their _desc()
        calls just returned -- as dependencies, so a child that repacks cannot free what a live parent entry points to."""
        return [self.attention._packed.held(), self.mlp._packed.held()]


# ==================================================================================================
# Attention (reference :18-180)
# ==================================================================================================
class Attention(_HipModule):
    """Multi-headed {cross, self}-attention: proj_q/k/v -> softmax(q k^T / sqrt(d)) v -> final."""

    def __init__(self, q_in_channels: int, k_in_channels: int = None, v_in_channels: int = None,
                 num_heads: int = 8, init_scale: float = 1.0, with_final_bias: bool = True,
                 final_init_scale_multiplier: float = 1., dropout_prob: float = 0.0,
                 qk_out_channels: int = None, v_out_channels: int = None, output_channels: int = None):
        super().__init__()
        self._num_heads = num_heads
        final_init_scale = final_init_scale_multiplier * init_scale
        if qk_out_channels is None:
            qk_out_channels = q_in_channels
        if v_out_channels is None:
            v_out_channels = qk_out_channels
        if output_channels is None:
            output_channels = v_out_channels
        self._qk_channels_per_head = qk_out_channels // num_heads
        self._v_channels_per_head = v_out_channels // num_heads
        if qk_out_channels % num_heads != 0:
            raise ValueError(f"qk_out_channels ({qk_out_channels}) must be divisible by"
                             f" num_heads ({num_heads}).")
        if v_out_channels % num_heads != 0:
            raise ValueError(f"v_channels ({v_out_channels}) must be divisible by"
                             f" num_heads ({num_heads}).")
        self.proj_q = nn.Linear(q_in_channels, qk_out_channels, bias=True)
        self.proj_k = nn.Linear(k_in_channels, qk_out_channels, bias=True)
        self.proj_v = nn.Linear(v_in_channels, v_out_channels, bias=True)
        for lin in (self.proj_q, self.proj_k, self.proj_v):
            variance_scaling_(lin.weight, scale=init_scale, mode="fan_in", distribution="truncated_normal")
            nn.init.constant_(lin.bias, 0)
        self.dropout = nn.Dropout(dropout_prob)
        self.final = nn.Linear(v_out_channels, output_channels, bias=with_final_bias)
        variance_scaling_(self.final.weight, scale=final_init_scale, mode="fan_in",
                          distribution="truncated_normal")
        if self.final.bias is not None:
            nn.init.constant_(self.final.bias, 0)

    # ---- packed descriptor -------------------------------------------------------------------
    def _build_desc(self, ov=None):
        """`ov` (policy "fp16sd"): {linear: fp32 weight image to pack instead of its parameter} for one block."""
        dtype, split = R.policy_dtype()
        H = self._num_heads
        q_two, k_two, v_two = R.splits("proj_q"), R.splits("proj_k"), R.splits("proj_v")
        wt = (lambda lin: ov[lin]) if ov else (lambda lin: lin.weight)
        q = R.PackedLinear(wt(self.proj_q), self.proj_q.bias, H, 1, dtype, q_two)
        k = R.PackedLinear(wt(self.proj_k), self.proj_k.bias, H, 1, dtype, k_two)
        v = R.PackedLinear(wt(self.proj_v), self.proj_v.bias, H, 1, dtype, v_two)
        o = R.PackedLinear(wt(self.final), self.final.bias, 1, H, dtype, R.splits("final"), k_channels=False)
        dk, dv = self._qk_channels_per_head, self._v_channels_per_head
        d = L.Attention(q.desc, k.desc, v.desc, o.desc, H, dk, dv, R.pad8(dk), R.pad8(dv),
                        self.proj_q.in_features, self.proj_k.in_features, self.proj_v.in_features,
                        self.final.out_features, dtype, R.attention_act_split())
        keep = [q, k, v, o]
        # K / V projection fold of a single-head cross-attend (pio_attention_t.kq / vo; SURVEY.md section 7 "legal algebraic
        # restructurings", reference :93-95,138,163): q (x Wk^T + bk)^T = (q Wk) x^T + const and
        # P (x Wv^T + bv) Wo^T + bo = (P x)(Wo Wv)^T + (Wo bv + bo).  The folded weights are formed in float64 and packed
        # like any other; the library takes them when keys outnumber query rows 4 : 1 (the encoders' cross-attends).
        # Offered where the weights are single (runtime.kv_fold_offered: below "x2s"): there it replaces single-sweep K / V
        # projections with exact (float64-folded, pair-packed) weights -- on the eight classifier goldens "fp16sd" moves from
        # 8.3e-4 / 1.72e-3 (fails the trained-like one) to 7.7e-4 / 9.0e-4, the multimodal model under "fp16/fp16x3f" from
        # 9.7e-4 / 1.06e-3 to 5.4e-4 / 5.6e-4, the flow forward from 5.66 to 5.42 ms.  Under the split-weight policies the
        # un-folded projections (K rounded AFTER an exact product) stay: 5.5e-4 / 5.8e-4 against 6.0e-4 / 8.4e-4 folded --
        # Q Wk concentrates on the outlier columns of a heavy-tailed Wk and multiplies the rounding of x there.
        # The library also takes it for the ImageNet DECODER (1024-wide head over 512 latents, batch-invariant queries:
        # xattn_tall_kernel reads the LayerNorm'd latents) -- under "fp16x2af" its K / V projections (2 x 34 GFLOP x 2
        # sweeps at B = 32) are gone: 6.5e-4 / 7.0e-4 -> 6.05e-4 / 5.6e-4 on the eight goldens, 16.49 -> 16.26 ms against
        # the split-operand ("x3f") decoder.
        kin = self.proj_k.in_features
        if H == 1 and kin == self.proj_v.in_features and dk == kin and dv == kin and (
                R.kv_fold_offered() or os.environ.get("PIO_KV_FOLD_ANY") == "1"):   # (env: A/B experiments, tools/)
            with torch.no_grad():
                Wk, Wv, Wo = wt(self.proj_k).double(), wt(self.proj_v).double(), wt(self.final).double()
                bv = self.proj_v.bias.double() if self.proj_v.bias is not None else torch.zeros(kin, device=Wv.device)
                bo = self.final.bias.double() if self.final.bias is not None else 0.0
                kq = R.PackedLinear(Wk.t().float().contiguous(), None, 1, 1, dtype, True, k_channels=False)
                # (always a pair: a single image under "fp16x2af" saves 0.2 % of the step and costs 6.05e-4 -> 6.35e-4)
                vo = R.PackedLinear((Wo @ Wv).float().contiguous(), (Wo @ bv + bo).float().contiguous(), 1, 1, dtype,
                                    True, k_channels=False)
            d.kq, d.vo = kq.desc, vo.desc
            keep += [kq, vo]
        if self.proj_q.in_features == self.proj_k.in_features and not split:
            pq, pk, pv = ((wt(lin), lin.bias) for lin in (self.proj_q, self.proj_k, self.proj_v))
            qk = R.PackedStack([pq, pk], H, dtype, [q_two, k_two])
            d.qk = qk.desc
            keep.append(qk)
            # q | k | v in one image when the fused attention kernel can read V row-major (the head widths it covers).
            # Under "x2s" / "x2w" the V rows alone carry a lo image (pio_linear_t.lo_row0): the wide GEMM kernel runs
            # its second K sweep for those columns only -- the library takes such an image inside the LayerNorm fold.
            if (R.qkv_stack_allowed() and self.proj_v.in_features == self.proj_q.in_features
                    and (R.pad8(dk), R.pad8(dv)) in FUSED_SELF_HEADS
                    and (not v_two or (2 * H * R.pad8(dk)) % 256 == 0)):
                qkv = R.PackedStack([pq, pk, pv], H, dtype, [False, False, v_two])
                d.qkv = qkv.desc
                keep.append(qkv)
        return d, keep

    def _params(self):
        return (self.proj_q.weight, self.proj_q.bias, self.proj_k.weight, self.proj_k.bias, self.proj_v.weight,
                self.proj_v.bias, self.final.weight, self.final.bias)

    def forward(self, inputs_q, inputs_k, inputs_v, attention_mask=None, attention_bias=None,
                return_matrix=False):
        if R.cpu_plumbing(inputs_q, "Attention.forward"):
            from . import cpu_plumbing as CP
            return CP.attention(self, inputs_q, inputs_k, inputs_v, attention_mask, attention_bias, return_matrix)
        R.require_device(inputs_q, "Attention.forward")
        _no_training_dropout(self, self.dropout.p)
        xq, xk, xv = R.as_f32_3d(inputs_q), R.as_f32_3d(inputs_k), R.as_f32_3d(inputs_v)
        if inputs_v is inputs_k:
            xv = xk
        B, Tq, _ = xq.shape
        Tk = xk.shape[1]
        return _block_call("pio_attention_fwd", "pio_attention_workspace_bytes", (B, Tq, Tk), self._desc(), (xq, xk, xv),
                           (B, self._num_heads, Tq, Tk), self.final.out_features, attention_mask, attention_bias,
                           return_matrix, (inputs_q, inputs_k, inputs_v) + self._params())


# ==================================================================================================
# MLP (reference :183-216)
# ==================================================================================================
class MLP(_HipModule):
    """Transformer-style dense module: fc2(gelu(fc1(x))), exact (erf) GELU."""

    def __init__(self, in_channels: int, out_channels: int = None, widening_factor: int = 4,
                 dropout_prob: float = 0.0, init_scale: float = 1.):
        super().__init__()
        out_channels = out_channels or in_channels
        self.fc1 = nn.Linear(in_channels, widening_factor * in_channels)
        variance_scaling_(self.fc1.weight, scale=init_scale, mode="fan_in", distribution="truncated_normal")
        nn.init.constant_(self.fc1.bias, 0)
        self.fc2 = nn.Linear(widening_factor * in_channels, out_channels)
        variance_scaling_(self.fc2.weight, scale=init_scale, mode="fan_in", distribution="truncated_normal")
        nn.init.constant_(self.fc2.bias, 0)
        self.dropout = nn.Dropout(dropout_prob)

    def _build_desc(self, ov=None):
        dtype, split = R.policy_dtype()
        wt = (lambda lin: ov[lin]) if ov else (lambda lin: lin.weight)
        f1 = R.PackedLinear(wt(self.fc1), self.fc1.bias, 1, 1, dtype, R.splits("fc1"), n_channels=True)
        f2 = R.PackedLinear(wt(self.fc2), self.fc2.bias, 1, 1, dtype, R.splits("fc2"))
        d = L.Mlp(f1.desc, f2.desc, self.fc1.in_features, self.fc1.out_features, self.fc2.out_features, dtype,
                  int(split))
        return d, [f1, f2]

    def _params(self):
        return (self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias)

    def forward(self, x):
        if R.cpu_plumbing(x, "MLP.forward"):
            from . import cpu_plumbing as CP
            return CP.mlp(self, x)
        R.require_device(x, "MLP.forward")
        _no_training_dropout(self, self.dropout.p)
        lib = L.lib()
        shape = x.shape
        x3 = R.as_f32_3d(x.reshape(-1, shape[-2], shape[-1]) if x.dim() != 3 else x)
        d = self._desc()
        dev = x3.device
        out = torch.empty(x3.shape[:2] + (self.fc2.out_features,), dtype=torch.float32, device=dev)
        rows = x3.shape[0] * x3.shape[1]
        ws = R.workspace(dev, lib.pio_mlp_workspace_bytes(d, rows))
        R.call_named(dev, "pio_mlp_fwd", m=d, x=R.tensor3(x3), out=out.data_ptr(), workspace=ws.data_ptr(),
                     workspace_bytes=ws.numel())
        out = R.forward_only(out, x, *self._params())
        return out.reshape(shape[:-1] + (self.fc2.out_features,))


# ==================================================================================================
# SelfAttention (reference :219-297)
# ==================================================================================================
class SelfAttention(_HipModule):
    """Pre-LN block: x + Attn(LN1(x)); x + MLP(LN2(x))."""

    def __init__(self, in_channels: int, widening_factor: int = 4, dropout_prob: float = 0.0,
                 dropout_attn_prob: float = 0.0, num_heads: int = 8, att_init_scale: float = 1.0,
                 dense_init_scale: float = 1.0, qk_channels: int = None, v_channels: int = None):
        super().__init__()
        if qk_channels is None:
            qk_channels = in_channels
        if v_channels is None:
            v_channels = qk_channels
        self.mlp = MLP(in_channels=v_channels, widening_factor=widening_factor, dropout_prob=dropout_prob,
                       init_scale=dense_init_scale)
        self.attention = Attention(q_in_channels=in_channels, k_in_channels=in_channels,
                                   v_in_channels=in_channels, num_heads=num_heads, init_scale=att_init_scale,
                                   qk_out_channels=qk_channels, v_out_channels=v_channels,
                                   dropout_prob=dropout_attn_prob)
        self.layer_norm1 = nn.LayerNorm(in_channels)
        self.layer_norm2 = nn.LayerNorm(v_channels)
        self.dropout = nn.Dropout(dropout_prob)
        self._in_channels = in_channels
        self._v_channels = v_channels

    def _build_desc(self):
        keep = []
        a = self.attention._desc()
        m = self.mlp._desc()
        d = L.SelfAttention(R.layernorm_desc(self.layer_norm1, keep), R.layernorm_desc(self.layer_norm2, keep), a, m)
        self._build_ln_fold(d, a, keep)
        return d, keep + self._child_entries()

    def _desc_blocks(self, nblk: int):
        """Policy "fp16sd": one descriptor per block of a weight-shared stack, block b packed from the b-th
        error-feedback rounding of every weight (runtime.feedback_images) -- of W for the plain images, of W * gamma
        for the images of the LayerNorm fold (the feedback runs over what the GEMM actually multiplies with)."""
        return self._packed.get(R.param_key(*self._params()) + (nblk,), lambda: self._build_blocks(nblk), slot="blocks")

    def _build_blocks(self, nblk: int):
        dtype = R.policy().dtype
        att, mlp = self.attention, self.mlp
        lins = (att.proj_q, att.proj_k, att.proj_v, att.final, mlp.fc1, mlp.fc2)
        descs, keep = [], []
        with torch.no_grad():
            g1, g2 = self.layer_norm1.weight.float(), self.layer_norm2.weight.float()
            plain = {lin: R.feedback_images(lin.weight, nblk, dtype) for lin in lins}
            fold = {lin: R.feedback_images(lin.weight.float() * g[None, :], nblk, dtype)
                    for lin, g in ((att.proj_q, g1), (att.proj_k, g1), (att.proj_v, g1), (mlp.fc1, g2))}
            for b in range(nblk):
                a, ka = att._build_desc({lin: plain[lin][b] for lin in lins[:4]})
                m, km = mlp._build_desc({lin: plain[lin][b] for lin in lins[4:]})
                d = L.SelfAttention(R.layernorm_desc(self.layer_norm1, keep), R.layernorm_desc(self.layer_norm2, keep), a, m)
                self._build_ln_fold(d, a, keep, {lin: imgs[b] for lin, imgs in fold.items()})
                descs.append(d)
                keep.extend([ka, km])
        return descs, keep

    def _build_ln_fold(self, d, a, keep, fold_ov=None):
        """LayerNorm folded into the consuming GEMMs (pio_ln_fold_t): LN(x) W^T + b = rstd (x W'^T - mean c) + b' with
        W' = W * gamma, c = rowsum(W' as packed), b' = W beta + b (reference :281-292 computes LN then Linear).
        Offered for blocks of 512 / 768 / 1024 / 1280 / 1536 channels (widening factor 1) under the single-sweep policies;
        the library decides per call."""
        dtype = R.policy().dtype
        att, mlp = self.attention, self.mlp
        C_ = self._in_channels
        if (not R.ln_fold_offered() or C_ % 256 or not 512 <= C_ <= 1536 or not a.qkv.w_hi
                or mlp.fc1.in_features != C_ or mlp.fc1.out_features != C_ or att.proj_q.in_features != C_):
            return
        with torch.no_grad():
            g1, b1 = self.layer_norm1.weight.float(), self.layer_norm1.bias.float()
            g2, b2 = self.layer_norm2.weight.float(), self.layer_norm2.bias.float()

            def folded(lin, g, b):
                w = lin.weight.float()
                bias = lin.bias.float() if lin.bias is not None else torch.zeros(w.shape[0], device=w.device)
                # (fold_ov: this block's image of W * gamma; the bias is that of the parameters)
                wg = fold_ov[lin] if fold_ov else w * g[None, :]
                return wg.contiguous(), (w @ b + bias).contiguous()

            H = att._num_heads
            qkv = R.PackedStack([folded(att.proj_q, g1, b1), folded(att.proj_k, g1, b1), folded(att.proj_v, g1, b1)],
                                H, dtype, [False, False, R.splits("proj_v")])
            fc1 = R.PackedLinear(*folded(mlp.fc1, g2, b2), 1, 1, dtype, R.splits("fc1"), n_channels=True)
            # c[n] = sum_k of the packed weights the GEMM actually multiplies with: hi (+ lo where there is one)
            qkv_c = (qkv.hi.float() + (qkv.lo.float() if qkv.lo is not None else 0)).sum(1).contiguous()
            fc1_c = (fc1.hi.float() + (fc1.lo.float() if fc1.lo is not None else 0)).sum(1).contiguous()
        d.fold = L.LnFold(qkv.desc, qkv_c.data_ptr(), fc1.desc, fc1_c.data_ptr())
        keep.extend([qkv, fc1, qkv_c, fc1_c])

    def _params(self):
        return self.attention._params() + self.mlp._params() + (self.layer_norm1.weight, self.layer_norm1.bias,
                                                                 self.layer_norm2.weight, self.layer_norm2.bias)

    def forward(self, inputs, *, attention_mask=None, attention_bias=None, return_matrix: bool = False):
        if R.cpu_plumbing(inputs, "SelfAttention.forward"):
            from . import cpu_plumbing as CP
            if self._v_channels != self._in_channels:
                raise RuntimeError(f"The size of tensor a ({self._in_channels}) must match the size of tensor b "
                                   f"({self._v_channels}) at non-singleton dimension 2")
            return CP.self_attention(self, inputs, attention_mask, attention_bias, return_matrix)
        R.require_device(inputs, "SelfAttention.forward")
        _no_training_dropout(self, self.dropout.p, self.attention.dropout.p, self.mlp.dropout.p)
        if self._v_channels != self._in_channels:
            # the residual add of the reference (:290) raises for mismatched widths
            raise RuntimeError(f"The size of tensor a ({self._in_channels}) must match the size of tensor b "
                               f"({self._v_channels}) at non-singleton dimension 2")
        x = R.as_f32_3d(inputs)
        B, N, D = x.shape
        return _block_call("pio_self_attention_fwd", "pio_self_attention_workspace_bytes", (B, N), self._desc(), (x,),
                           (B, self.attention._num_heads, N, N), D, attention_mask, attention_bias, return_matrix,
                           (inputs,) + self._params(), opts=None)     # (NULL: the library's defaults)


# ==================================================================================================
# CrossAttention (reference :300-406)
# ==================================================================================================
class CrossAttention(_HipModule):
    """Pre-LN cross-attention block with optional query residual, followed by an MLP."""

    def __init__(self, q_in_channels: int, kv_in_channels: int, widening_factor: int = 1,
                 dropout_prob: float = 0.0, dropout_attn_prob: float = 0.0, num_heads: int = 8,
                 attn_init_scale: float = 1.0, mlp_init_scale: float = 1.0, shape_for_attn: str = "kv",
                 use_query_residual: bool = True, qk_channels: int = None, v_channels: int = None):
        super().__init__()
        self._use_query_residual = use_query_residual
        output_channels = q_in_channels
        if qk_channels is None:
            if shape_for_attn == "q":
                qk_channels = q_in_channels
            elif shape_for_attn == "kv":
                qk_channels = kv_in_channels
            else:
                raise ValueError(f"Unknown value {shape_for_attn} for "
                                 "shape_for_attention.")
        if v_channels is None:
            v_channels = qk_channels
        self.attention = Attention(q_in_channels=q_in_channels, k_in_channels=kv_in_channels,
                                   v_in_channels=kv_in_channels, num_heads=num_heads, init_scale=attn_init_scale,
                                   dropout_prob=dropout_attn_prob, qk_out_channels=qk_channels,
                                   v_out_channels=v_channels, output_channels=output_channels)
        self.mlp = MLP(in_channels=output_channels, widening_factor=widening_factor, dropout_prob=dropout_prob,
                       init_scale=mlp_init_scale)
        self.layer_norm_q = nn.LayerNorm(q_in_channels)
        self.layer_norm_kv = nn.LayerNorm(kv_in_channels)
        self.layer_norm2 = nn.LayerNorm(output_channels)
        self.dropout = nn.Dropout(dropout_prob)

    def _build_desc(self):
        keep = []
        d = L.CrossAttention(R.layernorm_desc(self.layer_norm_q, keep), R.layernorm_desc(self.layer_norm_kv, keep),
                             R.layernorm_desc(self.layer_norm2, keep), self.attention._desc(), self.mlp._desc(),
                             1 if self._use_query_residual else 0)
        return d, keep + self._child_entries()

    def _params(self):
        return self.attention._params() + self.mlp._params() + (
            self.layer_norm_q.weight, self.layer_norm_q.bias, self.layer_norm_kv.weight, self.layer_norm_kv.bias,
            self.layer_norm2.weight, self.layer_norm2.bias)

    def forward(self, inputs_q, inputs_kv, *, attention_mask=None, attention_bias=None,
                return_matrix: bool = False):
        if R.cpu_plumbing(inputs_q, "CrossAttention.forward"):
            from . import cpu_plumbing as CP
            return CP.cross_attention(self, inputs_q, inputs_kv, attention_mask, attention_bias, return_matrix)
        R.require_device(inputs_q, "CrossAttention.forward")
        _no_training_dropout(self, self.dropout.p, self.attention.dropout.p, self.mlp.dropout.p)
        xq, xkv = R.as_f32_3d(inputs_q), R.as_f32_3d(inputs_kv)
        B, Tq, Cq = xq.shape
        Tk = xkv.shape[1]
        return _block_call("pio_cross_attention_fwd", "pio_cross_attention_workspace_bytes", (B, Tq, Tk), self._desc(),
                           (xq, xkv), (B, self.attention._num_heads, Tq, Tk), Cq, attention_mask, attention_bias,
                           return_matrix, (inputs_q, inputs_kv) + self._params())
