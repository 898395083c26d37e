"""Host-side plumbing between torch tensors and the C-ABI: precision policy, packed-weight images,
descriptors, workspaces.  PyTorch is used for device memory and streams only."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import _lib as L

# ------------------------------------------------------------------------------------------------
# precision policy: operand dtype of the MFMA matrices x number of MFMA sweeps per product.
#   fp16x3   every operand is a (hi, lo) fp16 pair, products = hi*hi + hi*lo + lo*hi: ~fp32-exact
#            results (1e-5 of the reference) at 1/3 of the MFMA rate.  DEFAULT: a drop-in must be safe.
#   fp16x2w  weights are (hi, lo) pairs, activations single fp16: removes the systematic weight-rounding
#            error that the 8x weight sharing amplifies; 3e-4 on the ImageNet config.
#   fp16     one sweep, plain fp16 operands: 7e-4 on the ImageNet config (meets 1e-3, thin margin).
#   bf16*    the same with bf16 operands (wider range, 8x coarser mantissa; only bf16x3 meets 1e-3).
# (numbers: tools/numerics_model.py and tests/test_parity_gpu.py; discussion in DESIGN.md)
# ------------------------------------------------------------------------------------------------
# One record per policy.  `split`: the linears whose WEIGHTS are (hi, lo) pairs -- Attention: proj_q, proj_k, proj_v, final;
# MLP: fc1, fc2; decoder: final_layer; heads behind the decoder (hip_linear): post.  `act_split`: activations are pairs,
# around the attention `core` named (attention_act_split).  `feedback`: one image set per block of a weight-shared stack.
class Policy(NamedTuple):
    dtype: int
    split: frozenset
    act_split: bool = False
    core: str = "materialised"
    feedback: bool = False


# nested weight sets: "x2s" the two projections whose weight rounding matters most (4.5e-4 on the ImageNet model at 1.2x the
# fp16 cost) | "x2w" + fc1, fc2, final_layer, post (3.1e-4) | "x3" every weight.  proj_q / proj_k stay single below "x3": their
# rounding is not measurable in the output (3.13e-4 with or without it, tools/numerics_model.py attribution).
_NONE = frozenset()
_X2S = frozenset({"proj_v", "final"})
_X2W = _X2S | {"fc1", "fc2", "final_layer", "post"}
_X3 = _X2W | {"proj_q", "proj_k"}
_F16, _BF16 = L.PIO_DT_F16, L.PIO_DT_BF16
_POLICIES = {
    "fp16": Policy(_F16, _NONE), "fp16x2s": Policy(_F16, _X2S), "fp16x2w": Policy(_F16, _X2W),
    "fp16x3": Policy(_F16, _X3, True),
    "bf16": Policy(_BF16, _NONE), "bf16x2w": Policy(_BF16, _X2W), "bf16x3": Policy(_BF16, _X3, True),
    # x3f: every GEMM with split operands as x3, but the attention core (Q K^T, softmax, P V) single-sweep on the fused
    # kernels (q / k / v / p rounded once; the core's output leaves as a pair): no score matrix
    "fp16x3f": Policy(_F16, _X3, True, "fused"), "bf16x3f": Policy(_BF16, _X3, True, "fused"),
    # x3fq: "x3f" with Q and K entering the fused core as (hi, lo) pairs -- S = Q_hi K_hi + Q_lo K_hi + Q_hi K_lo
    # inside the kernel (pio_attention_t.act_split = 3): the one rounding "x3f" leaves in front of the exponent is
    # gone, still no score matrix.  For models whose logits are large (trained LayerNorm gains: |s| ~ 10-15).
    # Pair cores exist for fp16 heads of dk <= 32; any other shape runs the materialised path of "x3" (fp16 only:
    # there is no bf16 pair core, hence no "bf16x3fq")
    "fp16x3fq": Policy(_F16, _X3, True, "fused_pair"),
    # x2af: split ACTIVATIONS against single weights (A_hi B^T + A_lo B^T: two sweeps) around a single-sweep
    # fused attention core -- for decoders whose error is dominated by the rounding of wide-range inputs
    # (Fourier / position features of dense outputs), at 2/3 of the x3f cost
    "fp16x2af": Policy(_F16, _NONE, True, "fused"),
    # fp16sd: "fp16" with ERROR-FEEDBACK rounding of the weights an encoder shares over its blocks: block b
    # multiplies with fp16(W + E_{b-1}), E_b = (W + E_{b-1}) - that image (first-order sigma-delta over the
    # block index).  Every image is a rounding of W within one ulp; the error the 8 applications of a shared
    # weight accumulate stays below half an ulp instead of growing 8-fold.  Same kernels, same time, 8 x the
    # packed images (604 MB for the ImageNet stack); -18..-21 % error on the ImageNet goldens.  Everything
    # that is not a weight-shared block stack runs as under "fp16".
    "fp16sd": Policy(_F16, _NONE, feedback=True),
    # finer weight splits of a self-attend stack (round 4): only the out projection ("final"), or only proj_v, of
    # the two that "x2s" splits -- a second K sweep costs its GEMM's time again
    "fp16x2o": Policy(_F16, frozenset({"final"})), "fp16x2v": Policy(_F16, frozenset({"proj_v"})),
    # x2afo: "x2af" (split activations around the single-sweep fused core) + split WEIGHTS on the output side of a
    # decoder only -- the attention's out projection, the decoder's final_layer, the heads behind it -- where a
    # dense-output model has nothing left to average a weight's rounding away (multimodal, second seed: x2af
    # 1.01e-3 / 1.14e-3, x2afo 4.0e-4 / 5.3e-4 at +4 % time; x3f 0.6e-4 / 2.7e-4 at +17 %)
    "fp16x2afo": Policy(_F16, frozenset({"final", "final_layer", "post"}), True, "fused")}


def _known(name: str, message: str = "unknown precision policy {name!r}; choose from {names}") -> str:
    if name not in _POLICIES:
        raise ValueError(message.format(name=name, names=sorted(_POLICIES)))
    return name


_policy = _known(os.environ.get("PIO_PRECISION", "fp16x3"), "PIO_PRECISION={name!r} not in {names}")


def set_precision_policy(name: str) -> None:
    global _policy
    _policy = _known(name)


def get_precision_policy() -> str:
    return _policy


class precision:
    """Context manager: run a block under another precision policy (None = leave the current one)."""

    def __init__(self, name: Optional[str]):
        self._name = None if name is None else _known(name)
        self._saved = None

    def __enter__(self):
        global _policy
        self._saved = _policy
        if self._name is not None:
            _policy = self._name
        return self

    def __exit__(self, *exc):
        global _policy
        _policy = self._saved
        return False


def split_policy3(policy):
    """"X/A/B" -> (X, A, B): X for the encoder's cross-attend alone, A for the latent self-attend stack, B for the decoder;
    "A/B" -> (None, A, B) (the cross-attend runs under A); a plain name (or None) applies everywhere."""
    parts = policy.split("/") if policy is not None else [None]
    if len(parts) > 3:
        raise ValueError(f"precision policy {policy!r}: expected 'name', 'encoder/decoder' or 'cross/stack/decoder'")
    return tuple(parts) if len(parts) == 3 else (None, parts[0], parts[-1])


def split_policy(policy):
    """(encoder policy, decoder policy) of a task model's policy string (split_policy3 without the cross-attend's)."""
    return split_policy3(policy)[1:]


# ---- what the packing sites ask (name: a policy, None = the ambient one) ----
def policy(name: Optional[str] = None) -> Policy:
    return _POLICIES[name or _policy]


def policy_dtype(name: Optional[str] = None) -> Tuple[int, bool]:
    """(operand dtype, activations split)"""
    return policy(name).dtype, policy(name).act_split


def torch_dtype(dtype: int) -> torch.dtype:
    return torch.float16 if dtype == L.PIO_DT_F16 else torch.bfloat16


def splits(linear: str, name: Optional[str] = None) -> bool:
    """Are the weights of `linear` (a name of Policy.split) packed as (hi, lo) pairs?  PIO_EXTRA_SPLIT=a,b adds names on
    top of every policy (A/B experiments: tools/); it is read per call."""
    return linear in policy(name).split or linear in os.environ.get("PIO_EXTRA_SPLIT", "").split(",")


def attention_act_split(name: Optional[str] = None) -> int:
    """pio_attention_t.act_split of a policy: 0 single activations, 1 split everywhere (materialised core), 2 split
    projections around the single-operand fused core, 3 the same with pair-operand Q K^T in the core."""
    p = policy(name)
    return {"materialised": 1, "fused": 2, "fused_pair": 3}[p.core] if p.act_split else 0


def kv_fold_offered(name: Optional[str] = None) -> bool:
    """K / V projection fold of a single-head cross-attend (Attention._build_desc, which says why): every policy whose
    weight set lies below "x2s" -- the finer ones ("x2o", "x2v", "x2afo") keep the offer.  PIO_EXTRA_SPLIT does not count."""
    return not _X2S <= policy(name).split


def ln_fold_offered(name: Optional[str] = None) -> bool:
    """LayerNorm fold of a self-attend block (SelfAttention._build_ln_fold): single proj_q / proj_k, single activations."""
    return not ("proj_q" in policy(name).split or policy(name).act_split)


def qkv_stack_allowed(name: Optional[str] = None) -> bool:
    """q | k | v in one packed image: only a suffix of a stack may carry a lo image, so proj_q / proj_k must be single."""
    return not (splits("proj_q", name) or splits("proj_k", name))


# ------------------------------------------------------------------------------------------------
# range guard of the LayerNorm-folded stack.  Inside it the residual stream is an fp16 PAIR (hi + lo) and the GEMMs
# read the un-normalised hi half: a latent beyond +-65504 becomes inf (the un-folded path keeps the stream in fp32 and
# only ever rounds LayerNorm OUTPUTS, which are O(1)).  The guard lives ON THE DEVICE: every GEMM that produces the
# folded stream already reduces each result row's (sum, sum of squares) and ORs 1 into a device word when one of them
# is not finite (pio_ln_fold_t.range_flag) -- no extra kernel, no host synchronisation inside the forward.  With the
# guard on (default; PIO_RANGE_CHECK=0 or set_range_check(False) turns it off) the word is read
#   * by PerceiverIO.forward ONCE, after the decoder and the postprocessors have been enqueued (the point where the
#     caller is about to consume the result), or
#   * by PerceiverEncoder.forward itself when it is called on its own;
# a set word re-runs the call with the fold off and raises PIO_E_RANGE if the un-folded result is not finite either
# (then the model needs a wider operand type: precision policy "bf16x3").  During stream capture nothing is read:
# the word stays in `last_range_flag()` for the owner of the graph to look at after a replay.
# ------------------------------------------------------------------------------------------------
_range_check = os.environ.get("PIO_RANGE_CHECK", "1") != "0"
_range_flags: Dict[tuple, torch.Tensor] = {}
_range_deferred: Optional[list] = None      # not None: PerceiverIO.forward collects the encoder's pending checks


def range_check() -> bool:
    return _range_check


def set_range_check(on: bool) -> None:
    global _range_check
    _range_check = bool(on)


def range_flag(device: torch.device, owner=None) -> torch.Tensor:
    """The device word a folded stack reports into (int32[1]): ONE PER OWNER (a PerceiverEncoder instance) and device, so
    that two models running on one device never clear or read each other's word; `last_range_flag(device)` is the word of
    the forward that ran last there (what the owner of a captured graph reads after a replay)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, id(owner) if owner is not None else 0)
    t = _range_flags.get(key)
    if t is None:
        with torch.inference_mode(False):     # (a normal tensor: zeroed in place from inside and outside inference mode)
            t = torch.zeros(1, dtype=torch.int32, device=device)
        _range_flags[key] = t
        if owner is not None:
            import weakref
            weakref.finalize(owner, _range_flags.pop, key, None)
    _range_flags[(idx, "last")] = t
    return t


def last_range_flag(device: Optional[torch.device] = None) -> Optional[torch.Tensor]:
    idx = (device.index if device is not None and device.index is not None else torch.cuda.current_device())
    return _range_flags.get((idx, "last"))


class defer_range_checks:
    """PerceiverIO.forward: the encoder registers its pending check here instead of synchronising mid-forward."""

    def __enter__(self):
        global _range_deferred
        self._saved = _range_deferred
        _range_deferred = []
        self.pending = _range_deferred
        return self

    def __exit__(self, *exc):
        global _range_deferred
        _range_deferred = self._saved
        return False


def range_deferred() -> Optional[list]:
    return _range_deferred


def capturing(device: torch.device) -> bool:
    try:
        return bool(torch.cuda.is_current_stream_capturing())
    except Exception:  # noqa: BLE001
        return False


def feedback_images(w: torch.Tensor, nblk: int, dtype: int):
    """The nblk error-feedback roundings of the fp32 weight `w` to the operand dtype, as fp32 tensors that are exactly
    representable in it (packing them is exact): image_b = round(w + E_{b-1}), E_b = (w + E_{b-1}) - image_b, E_{-1} = 0.
    |w - image_b| < 1 ulp for every b and |sum_{b<=k} (w - image_b)| = |E_k| <= ulp / 2 for every k."""
    w = w.detach().float()
    out, e = [], torch.zeros_like(w)
    for _ in range(nblk):
        t = w + e
        hi = t.to(torch_dtype(dtype)).float()
        e = t - hi
        out.append(hi)
    return out


def pad8(c: int) -> int:
    return (c + 7) & ~7


def padc(c: int) -> int:
    """Pitch of a CHANNEL axis in the 16-bit operand arrays (csrc/pio_internal.h padc): a multiple of 8, from 256
    channels on a multiple of 64 (the staged GEMM kernels read whole 64-deep K slices)."""
    return int(L.lib().pio_padc(int(c)))


# ------------------------------------------------------------------------------------------------
# backend.  "hip" (default): the hot path exists only as gfx950 kernels -- CPU tensors raise.  "torch": the opt-in CPU
# PLUMBING backend (cpu_plumbing.py) for machines without a GPU (BASELINE config 1) -- CUDA tensors raise.  Nothing ever
# switches by itself; there is no fallback in either direction.
# ------------------------------------------------------------------------------------------------
_backend = os.environ.get("PIO_BACKEND", "hip")
if _backend not in ("hip", "torch"):
    raise ValueError(f"PIO_BACKEND={_backend!r}: 'hip' or 'torch'")


def set_backend(name: str) -> None:
    global _backend
    if name not in ("hip", "torch"):
        raise ValueError(f"unknown backend {name!r}: 'hip' (MI355X kernels) or 'torch' (opt-in CPU plumbing)")
    _backend = name


def get_backend() -> str:
    return _backend


def cpu_plumbing(t: torch.Tensor, what: str) -> bool:
    """True when this call runs on the opt-in CPU plumbing backend.  A CUDA tensor under that backend raises: GPU
    tensors only ever run on the HIP kernels."""
    if _backend != "torch":
        return False
    if t.is_cuda:
        raise L.PioError(f"{what}: backend 'torch' is the CPU plumbing path and got a {t.device} tensor; GPU tensors run "
                         "on the HIP kernels only -- set_backend('hip')")
    return True


def require_device(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise L.PioError(f"{what}: perceiverio_pytorch_amd computes on an MI355X (HIP) device only; got a "
                         f"{t.device} tensor. There is no CPU or eager fallback (an explicit CPU plumbing backend "
                         "exists for machines without a GPU: perceiverio_pytorch_amd.set_backend('torch')).")


def stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


# ------------------------------------------------------------------------------------------------
# tensors at the boundary
# ------------------------------------------------------------------------------------------------
def as_f32_3d(t: torch.Tensor) -> torch.Tensor:
    """float32, last dim contiguous, 3-D; broadcast (stride-0) batch views are kept as views."""
    if t.dim() != 3:
        raise ValueError(f"expected a [B, T, C] tensor, got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        t = t.float()
    if t.stride(2) != 1 and t.shape[2] != 1:
        t = t.contiguous()
    if t.stride(1) < t.shape[2] and t.shape[1] > 1:    # exotic row-overlapping views
        t = t.contiguous()
    return t


def tensor3(t: torch.Tensor) -> L.Tensor3:
    B, T, Cc = t.shape
    sb = t.stride(0) if B > 1 else T * Cc
    st = t.stride(1) if T > 1 else Cc
    return L.Tensor3(t.data_ptr(), sb, st, B, T, Cc)


def mask_u8(m: Optional[torch.Tensor], shape, device) -> Tuple[Optional[torch.Tensor], Optional[int]]:
    """bool/any mask -> contiguous uint8 tensor on `device` (kept alive by the caller) + pointer."""
    if m is None:
        return None, None
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"mask shape {tuple(m.shape)} != {tuple(shape)}")
    mm = m.to(device=device)
    mm = (mm != 0) if mm.dtype != torch.bool else mm
    mm = mm.contiguous().view(torch.uint8)
    return mm, mm.data_ptr()


# ------------------------------------------------------------------------------------------------
# workspaces: one grow-only byte buffer per (device, stream); launches on a stream are ordered, so
# consecutive blocks can share it.
# ------------------------------------------------------------------------------------------------
_workspaces: Dict[Tuple[int, int], torch.Tensor] = {}


def workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device(), stream_ptr(device))
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = None
        _workspaces.pop(key, None)
        ws = torch.empty(int(nbytes * 1.05) + 4096, dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def release_workspaces() -> None:
    _workspaces.clear()


# ------------------------------------------------------------------------------------------------
# packed weights
# ------------------------------------------------------------------------------------------------
class PackedLinear:
    """Device image of one nn.Linear in kernel layout (hi [+ lo] + padded bias) and its descriptor."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor], row_heads: int, col_heads: int,
                 dtype: int, two_pass: bool, *, k_channels: bool = True, n_channels: bool = False):
        """`k_channels`: the input axis is a channel axis (pitch padc) -- everything but Attention.final, whose input
        is heads x padded head dim; `n_channels`: so is the OUTPUT (MLP.fc1: its 16-bit output is fc2's operand)."""
        require_device(weight, "pack_linear")
        lib = L.lib()
        out, inn = weight.shape
        if out % row_heads or inn % col_heads:
            raise ValueError("channels must be divisible by the head count")
        rows_packed = row_heads * pad8(out // row_heads)
        self.n = padc(out) if (n_channels and row_heads == 1) else rows_packed
        self.k = padc(inn) if (k_channels and col_heads == 1) else col_heads * pad8(inn // col_heads)
        dev = weight.device
        w = weight.detach()
        if w.dtype != torch.float32 or not w.is_contiguous():
            w = w.float().contiguous()
        tdt = torch_dtype(dtype)
        alloc = torch.zeros if self.n > rows_packed else torch.empty     # (rows behind the packed ones stay zero)
        self.hi = alloc((self.n, self.k), dtype=tdt, device=dev)
        self.lo = alloc((self.n, self.k), dtype=tdt, device=dev) if two_pass else None
        self.bias = alloc((self.n,), dtype=torch.float32, device=dev)
        b = None
        if bias is not None:
            b = bias.detach()
            if b.dtype != torch.float32 or not b.is_contiguous():
                b = b.float().contiguous()
        L.check(lib.pio_pack_linear(*L.arguments("pio_pack_linear", (), dict(
            w=w.data_ptr(), bias=b.data_ptr() if b is not None else None, out=out, in_=inn, ldw=inn,
            row_heads=row_heads, col_heads=col_heads, dst_hi=self.hi.data_ptr(),
            dst_lo=self.lo.data_ptr() if two_pass else None, dst_bias=self.bias.data_ptr(), dst_row0=0, k_pad=self.k,
            dtype=dtype, stream=stream_ptr(dev)))), "pio_pack_linear")
        self.desc = L.Linear(self.hi.data_ptr(), self.lo.data_ptr() if two_pass else None, self.bias.data_ptr(),
                             self.n, self.k)


class PackedStack:
    """Several nn.Linear with equal in_features stacked along the output rows in ONE packed image
    (e.g. proj_q | proj_k, consumed by a single GEMM when both read the same input).  `two_pass` is a bool (every part)
    or one bool per part: only a SUFFIX of the parts may carry a lo image (q | k | v with v alone split); the
    descriptor's lo_row0 then names the first row that has one."""

    def __init__(self, pairs, row_heads: int, dtype: int, two_pass):
        lib = L.lib()
        flags = [bool(two_pass)] * len(pairs) if isinstance(two_pass, bool) else [bool(f) for f in two_pass]
        if any(a and not b for a, b in zip(flags, flags[1:])):
            raise ValueError("only a suffix of the stacked linears may be split")
        two_pass = any(flags)
        w0 = pairs[0][0]
        require_device(w0, "pack_linear")
        dev = w0.device
        inn = w0.shape[1]
        self.k = padc(inn)
        rows = [row_heads * pad8(w.shape[0] // row_heads) for w, _ in pairs]
        self.n = sum(rows)
        tdt = torch_dtype(dtype)
        self.hi = torch.empty((self.n, self.k), dtype=tdt, device=dev)
        self.lo = torch.empty((self.n, self.k), dtype=tdt, device=dev) if two_pass else None
        self.bias = torch.empty((self.n,), dtype=torch.float32, device=dev)
        if self.lo is not None and not all(flags):
            self.lo.zero_()          # rows without a lo half are never read; keep them defined
        r0 = 0
        lo_row0 = 0
        for (w, b), nr, fl in zip(pairs, rows, flags):
            if w.shape[1] != inn:
                raise ValueError("stacked linears need equal in_features")
            wf = w.detach().float().contiguous()
            bf = b.detach().float().contiguous() if b is not None else None
            L.check(lib.pio_pack_linear(*L.arguments("pio_pack_linear", (), dict(
                w=wf.data_ptr(), bias=bf.data_ptr() if bf is not None else None, out=w.shape[0], in_=inn, ldw=inn,
                row_heads=row_heads, col_heads=1, dst_hi=self.hi.data_ptr(), dst_lo=self.lo.data_ptr() if fl else None,
                dst_bias=self.bias.data_ptr(), dst_row0=r0, k_pad=self.k, dtype=dtype, stream=stream_ptr(dev)))),
                "pio_pack_linear")
            if not fl:
                lo_row0 = r0 + nr
            r0 += nr
        self.lo_row0 = lo_row0 if two_pass else 0
        self.desc = L.Linear(self.hi.data_ptr(), self.lo.data_ptr() if two_pass else None, self.bias.data_ptr(),
                             self.n, self.k, self.lo_row0)


def _version_of(p: torch.Tensor) -> int:
    # (tensors created or moved under torch.inference_mode() do not track a version counter)
    return 0 if p.is_inference() else p._version


def param_key(*params) -> tuple:
    """Cache key that changes whenever a parameter is rebound, moved or modified in place through autograd-visible
    ops.  Writes through ``p.data`` (``p.data.copy_()``, some checkpoint loaders) do NOT bump the version counter:
    ``load_state_dict`` is covered by a hook of the modules; after any other raw write call
    ``invalidate_packed_weights(module)``."""
    return tuple((p.data_ptr(), _version_of(p), str(p.device)) if p is not None else None for p in params) + (_policy,)


class PackedCache:
    """What a module derives from its parameters (packed images, descriptors, parameter-only arrays), by slot:
    slot -> (key, value, keep).  `keep` is whatever the value points into without owning it; it lives exactly as long as
    the entry.  A plain object: no parameter, no buffer, nothing in state_dict().  A deepcopy or pickle of the owner
    carries an EMPTY cache (ctypes descriptors cannot be copied, and a copy's parameters live elsewhere): it repacks on
    first use."""

    def __init__(self):
        self._entries = {}

    def get(self, key, build, slot=None):
        """The value of `slot`, from `build() -> (value, keep)` when there is none under `key` yet."""
        e = self._entries.get(slot)
        if e is None or e[0] != key:
            value, keep = build()
            self._entries[slot] = e = (key, value, keep)
        return e[1]

    def held(self, slot=None):
        """The current entry of `slot` as one object: what a parent's entry lists in its `keep` to hold a child's images."""
        return self._entries.get(slot)

    def values(self):
        return [e[1] for e in self._entries.values()]

    def clear(self) -> None:
        self._entries.clear()

    def __len__(self) -> int:
        return len(self._entries)

    def __getstate__(self):         # (copy.deepcopy and pickle both come through here)
        return {"_entries": {}}


class PackedOwner(torch.nn.Module):
    """A module that keeps something derived from parameters: ONE cache, dropped by everything that can change a
    parameter behind the key's back."""

    def __init__(self):
        super().__init__()
        self._packed = PackedCache()

    def clear_packed(self) -> None:
        self._packed.clear()

    def _apply(self, fn, *a, **k):       # .to()/.cuda()/.float() invalidate packed images
        self._packed.clear()
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):   # load_state_dict copies through .data on some paths: repack
        self._packed.clear()
        return super()._load_from_state_dict(*a, **k)


def invalidate_packed_weights(module: torch.nn.Module) -> None:
    """Drop everything cached from parameters under ``module``: packed / folded weight images, descriptors, parameter-only
    query arrays and their projections (all rebuilt on the next forward)."""
    for m in module.modules():
        if isinstance(m, PackedOwner):
            m.clear_packed()


class _ForwardOnly(torch.autograd.Function):
    """Identity whose backward raises: the HIP path has no autograd.  Outputs of the HIP modules are fresh buffers
    without a grad_fn, so without this a ``loss.backward()`` would silently skip every encoder / decoder parameter."""

    @staticmethod
    def forward(ctx, out, *deps):
        return out.view_as(out)

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError("perceiverio_pytorch_amd is a forward / inference path: there is no backward "
                                  "through the HIP kernels (run under torch.inference_mode() or torch.no_grad())")


def forward_only(out: torch.Tensor, *deps) -> torch.Tensor:
    """Tie `out` to the tensors it was computed from when autograd is recording, with a backward that raises."""
    if torch.is_grad_enabled():
        live = [t for t in deps if isinstance(t, torch.Tensor) and t.requires_grad]
        if live:
            return _ForwardOnly.apply(out, *live)
    return out


class on_device:
    """Make the tensor's GPU the current HIP device around a C call: the library launches on the given stream, but
    hipGetLastError, the architecture check and the cached CU count consult the CURRENT device."""

    def __init__(self, device: torch.device):
        self._ctx = torch.cuda.device(device)

    def __enter__(self):
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        return self._ctx.__exit__(*exc)


def call(dev, name, *args, stream=None, declines=()):
    """One launch through the C-ABI with `dev` current: entry point `name` with `args`, then the stream (the current one of
    `dev` unless given): every launching entry point ends in its stream.  An error code raises PioError labelled `name`;
    a code in `declines` (the entry refused, nothing launched) returns False."""
    with on_device(dev):
        code = getattr(L.lib(), name)(*args, stream_ptr(dev) if stream is None else stream)
    if code in declines:
        return False
    L.check(code, name)
    return True


def call_named(dev, name, *args, stream=None, declines=(), **named):
    """`call` with the arguments behind `args` given by the header's parameter names: _lib.arguments lays them out and
    refuses a wrong, missing or repeated name before anything runs.  The header's trailing `stream` is the one `call`
    fills; `call` itself sees the arguments in the header's order."""
    argv = L.arguments(name, args, {**named, "stream": stream})
    return call(dev, name, *argv[:-1], stream=argv[-1], declines=declines)


def layernorm_desc(ln: torch.nn.LayerNorm, keep: list) -> L.LayerNorm:
    w, b = ln.weight.detach(), ln.bias.detach()
    if w.dtype != torch.float32:
        w, b = w.float(), b.float()
    w, b = w.contiguous(), b.contiguous()
    keep += [w, b]
    return L.LayerNorm(w.data_ptr(), b.data_ptr(), w.numel(), float(ln.eps))


# ------------------------------------------------------------------------------------------------
# a plain nn.Linear through the C-ABI primitives (pio_layernorm_cast as the operand cast + pio_gemm_nt): used by the
# I/O plumbing right behind the decoder (tied-embedding vocabulary projection of the language model)
# ------------------------------------------------------------------------------------------------
def hip_linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], cache: PackedCache) -> torch.Tensor:
    """y[..., out] = x[..., in] W^T + b on the MI355X under the current precision policy (the weight is the policy's
    "post").  `cache` (the owner's) keeps the packed weight image between calls."""
    require_device(x, "hip_linear")
    dev = x.device
    dtype, split = policy_dtype()
    lin = cache.get(param_key(weight, bias), lambda: (PackedLinear(weight, bias, 1, 1, dtype, splits("post")), None))
    lead = x.shape[:-1]
    x3 = as_f32_3d(x.reshape(1, -1, x.shape[-1]))
    rows, n_out = x3.shape[1], weight.shape[0]
    tdt = torch_dtype(dtype)
    x16 = torch.empty((rows, lin.k), dtype=tdt, device=dev)
    x16lo = torch.empty((rows, lin.k), dtype=tdt, device=dev) if split else None
    out = torch.empty((rows, n_out), dtype=torch.float32, device=dev)
    call_named(dev, "pio_layernorm_cast", x=tensor3(x3), ln=None, y=x16.data_ptr(), y_lo=x16lo.data_ptr() if split else None,
               c_pad=lin.k, dtype=dtype)
    g = L.Gemm()
    g.A, g.B = x16.data_ptr(), lin.hi.data_ptr()
    g.A_lo = x16lo.data_ptr() if split else None
    g.B_lo = lin.lo.data_ptr() if lin.lo is not None else None
    g.C = out.data_ptr()
    g.M, g.N, g.K = rows, n_out, lin.k
    g.lda = g.ldb = lin.k
    g.ldc = n_out
    g.batch = g.nh = 1
    g.bias = lin.bias.data_ptr()
    g.bias_mode = 1
    g.alpha = 1.0
    g.out_f32 = 1
    g.n_store = n_out
    g.dtype = dtype
    call(dev, "pio_gemm_nt", C.byref(g))
    return forward_only(out.reshape(lead + (n_out,)), x, weight, bias)
