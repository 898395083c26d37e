"""The step behind the models on the tensors' own device: what example_multimodal.py does on the host with the outputs of
forward -- frames as (np.clip(image, 0, 1) * 255).astype(np.uint8), sound as (audio * 2**15).astype(np.int16), the best
labels as softmax + top-k -- for torch tensors.

CUDA fp32 tensors under the hip backend go through ONE pio_finish_media launch (csrc/pio_media.hip; plan and launch:
fused_io.finish_media), read in place through their strides, and labels through pio_vocab_topk's selection mode
(fused_io.top_labels).  CPU tensors, other dtypes (upcast to fp32), the torch backend (CPU tensors only: that backend's
rule) and fused_media = False run `restatement`, the same formulas in torch ops on the tensor's device, with the same bits.

Where numpy is undefined the two agree with each other, not with numpy: a NaN gives 0 in both sample types, and an audio
value outside [-1, 1) SATURATES to -32768 / 32767 (numpy's conversion wraps on common builds)."""
from __future__ import annotations

import sys
from typing import Optional

import torch

from . import _lib as L, fused_io as FIO, runtime as R

U8, S16 = L.PIO_MEDIA_U8, L.PIO_MEDIA_S16


def restatement(x: torch.Tensor, kind: int, reverse: bool = False) -> torch.Tensor:
    """pio_finish_media in torch ops on x's device: uint8 (kind U8; reverse flips the last axis) or int16 (S16) of x's shape.
    U8: v = x > 0 ? (x > 1 ? 1 : x) : 0 (-0 and NaN give 0), trunc(v * 255); S16: trunc(x * 32768) saturated, NaN gives 0."""
    x = x.detach().float()
    if kind == U8:
        v = torch.where(x > 0, torch.where(x > 1, torch.ones_like(x), x), torch.zeros_like(x))
        y = (v * 255.0).to(torch.int32).to(torch.uint8)
        return y.flip(-1).contiguous() if reverse else y.contiguous()
    if kind != S16 or reverse:
        raise ValueError("restatement: kind U8 (with or without reverse) or S16 (without)")
    t = x * 32768.0
    c = torch.clamp(t, -32768.0, 32767.0)
    return torch.where(t == t, c, torch.zeros_like(c)).to(torch.int32).to(torch.int16).contiguous()


def _collapse(x: torch.Tensor, keep: int) -> torch.Tensor:
    """x with everything in front of its last `keep` axes as ONE axis: a view where the strides allow it, else ONE copy."""
    lead, tail = x.shape[:x.dim() - keep], x.shape[x.dim() - keep:]
    n = 1
    for s in lead:
        n *= s
    dims = [(s, st) for s, st in zip(lead, x.stride()) if s != 1]
    if all(a[1] == b[0] * b[1] for a, b in zip(dims, dims[1:])):
        return x.as_strided((n,) + tuple(tail), ((dims[-1][1] if dims else 0),) + tuple(x.stride()[x.dim() - keep:]))
    return x.contiguous().reshape((n,) + tuple(tail))


def _finish(x4: torch.Tensor, kind: int, reverse: bool, what: str) -> torch.Tensor:
    fused = sys.modules[__package__].fused_media
    if not R.cpu_plumbing(x4, what) and x4.dtype == torch.float32:
        y = FIO.finish_media(fused, x4, kind, reverse)
        if y is not None:
            return y
    return restatement(x4, kind, reverse)


def to_frames(image: torch.Tensor, *, bgr: bool = False, channels_first: Optional[bool] = None) -> torch.Tensor:
    """uint8 [.., H, W, C] on the same device of an image tensor [.., C, H, W] or [.., H, W, C] with values in [0, 1]: clipped,
    times 255, truncated -- the bits of numpy's (np.clip(a, 0, 1) * 255).astype(np.uint8); a NaN gives 0.  bgr: channels
    reversed, the order OpenCV's writer wants.  channels_first: None infers it from the last three axes (first <= 4 < last:
    channels first; last <= 4 < first: channels last; anything else raises).  Views are read in place (MultiModalPerceiver's
    [b, t, 3, h, w] `image` output is one of [b, t*h*w, 3] storage); leading axes whose strides do not collapse cost one copy."""
    if not isinstance(image, torch.Tensor) or image.dim() < 3:
        raise ValueError("to_frames takes an image tensor [.., C, H, W] or [.., H, W, C]")
    if not image.dtype.is_floating_point:
        raise ValueError(f"to_frames: a floating-point image with values in [0, 1], got {image.dtype}")
    first, last = image.shape[-3], image.shape[-1]
    if channels_first is None:
        if first <= 4 < last:
            channels_first = True
        elif last <= 4 < first:
            channels_first = False
        else:
            raise ValueError(f"to_frames: cannot tell the channel axis of shape {tuple(image.shape[-3:])}; pass "
                             "channels_first=True or False")
    x = image.detach().movedim(-3, -1) if channels_first else image.detach()
    h, w, c = x.shape[-3:]
    if not 1 <= c <= 4:
        raise ValueError(f"to_frames: 1 to 4 channels, got {c}")
    if h * w >= 2 ** 31:
        raise ValueError(f"to_frames: a frame of {h} x {w} pixels is beyond 2^31 - 1")
    if x.numel() == 0:
        return torch.empty(tuple(x.shape), dtype=torch.uint8, device=x.device)
    return _finish(_collapse(x, 3), U8, bool(bgr), "to_frames").reshape(tuple(x.shape))


_PCM_SPAN = 1 << 30      # samples per launch of a long contiguous waveform (h * w of a call stays below 2^31)


def to_pcm16(audio: torch.Tensor) -> torch.Tensor:
    """int16 of the same shape and device of a waveform tensor with values in [-1, 1): trunc(audio * 2**15), numpy's
    (a * 2**15).astype(np.int16) there.  Outside that range the sample saturates (-32768 / 32767) and a NaN gives 0."""
    if not isinstance(audio, torch.Tensor) or not audio.dtype.is_floating_point:
        raise ValueError("to_pcm16 takes a floating-point waveform tensor")
    x = audio.detach()
    if x.numel() == 0:
        return torch.empty(tuple(x.shape), dtype=torch.int16, device=x.device)
    if x.is_contiguous():
        flat = x.reshape(-1)
        parts = [_finish(flat[i:i + _PCM_SPAN].view(1, 1, -1, 1), S16, False, "to_pcm16")
                 for i in range(0, flat.numel(), _PCM_SPAN)]
        return (parts[0] if len(parts) == 1 else torch.cat([p.reshape(-1) for p in parts])).reshape(tuple(x.shape))
    # a view: its last two axes as rows and columns of one channel, everything in front as one axis
    v = x.reshape((1,) * (2 - x.dim()) + tuple(x.shape)) if x.dim() < 2 else x
    if v.shape[-2] * v.shape[-1] >= 2 ** 31:
        v = v.contiguous()
        return to_pcm16(v).reshape(tuple(x.shape))
    return _finish(_collapse(v, 2).unsqueeze(-1), S16, False, "to_pcm16").reshape(tuple(x.shape))


def top_labels(logits: torch.Tensor, k: int = 5):
    """(ids int64 [.., k], probs fp32 [.., k]) of logits [.., V]: the k most probable classes of every row under softmax,
    most probable first, the lower id first among equal logits.  CUDA fp32 logits under the hip backend with V <= 1024 and
    k <= 8 are ONE pio_vocab_topk launch (its selection mode); larger V or k, CPU tensors, the torch backend and an active
    range probe take log_softmax and a stable descending sort on the tensor's device."""
    if not isinstance(logits, torch.Tensor) or logits.dim() < 1 or not logits.dtype.is_floating_point:
        raise ValueError("top_labels takes a floating-point tensor of logits [.., V]")
    v, k = logits.shape[-1], int(k)
    if not 1 <= k <= v:
        raise ValueError(f"top_labels: k = {k} outside [1, V = {v}]")
    if not R.cpu_plumbing(logits, "top_labels"):
        fused = FIO.top_labels(logits, k)
        if fused is not None:
            return fused
    logprob, ids = torch.sort(torch.log_softmax(logits.float(), dim=-1), dim=-1, descending=True, stable=True)
    return ids[..., :k].contiguous(), torch.exp(logprob[..., :k]).contiguous()
