"""The step in front of the models on the tensors' own device: crop, bilinear resize (antialiased or not), channel reversal
and (v - mean) / std of a batch or a list of uint8 / fp32 images -- what the examples do per image on the host
(example_img_classify.py: resized_crop + Normalize; example_multimodal.py: crop_center_square, cv2.resize, BGR -> RGB, / 255;
example_opt_flow.py: 2 (x / 255) - 1).

CUDA uint8 / fp32 images under the hip backend go through ONE pio_prepare_images launch per 32 differently shaped sources
(csrc/pio_imageprep.hip; plan and launch: fused_io.prepare_images), read in place through their strides.  CPU tensors, the
torch backend (CPU tensors only: that backend's rule), fused_image_prep = False and whatever the plan declines run `chain`,
the same step as torch ops per image on the tensors' device."""
from __future__ import annotations

import operator
import sys
from typing import Optional, Sequence, Union

import torch
import torch.nn.functional as F

from . import fused_io as FIO, runtime as R

Box = Sequence[int]


def center_box(h: int, w: int) -> tuple:
    """The centred square of an h x w image as example_img_classify.py computes it: (top, left, m, m)."""
    m = min(h, w)
    return int(h / 2 - m / 2), int(w / 2 - m / 2), m, m


def _as_nchw(x: torch.Tensor, channels_last: Optional[bool], what: str) -> torch.Tensor:
    """A 3-D image as a [1, C, H, W] view, a 4-D batch as a [N, C, H, W] view (nothing is copied)."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4):
        raise ValueError(f"{what} must be a 3-D image tensor or a 4-D batch of them")
    x = x.detach()
    if x.dim() == 3:
        x = x.unsqueeze(0)
    first, last = x.shape[1], x.shape[3]
    if channels_last is None:
        if last <= 4 < first:
            channels_last = True
        elif first <= 4 < last:
            channels_last = False
        else:
            raise ValueError(f"{what}: cannot tell the channel axis of shape {tuple(x.shape[1:])}; pass channels_last=True "
                             "or False")
    x = x.permute(0, 3, 1, 2) if channels_last else x
    if not 1 <= x.shape[1] <= 4:
        raise ValueError(f"{what}: 1 to 4 channels, got {x.shape[1]}")
    if min(x.shape) < 1:
        raise ValueError(f"{what} is empty: {tuple(x.shape)}")
    if x.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{what}: uint8 or float32 images, got {x.dtype}")
    return x


def _boxes(crop, views) -> list:
    """One (top, left, height, width) per image of every view: [[box, ..] per view]."""
    count = sum(v.shape[0] for v in views)
    if crop is None:
        return [[(0, 0, v.shape[2], v.shape[3])] * v.shape[0] for v in views]
    if isinstance(crop, str):
        if crop != "center":
            raise ValueError(f"crop={crop!r}: None, 'center', a (top, left, height, width) tuple or a list of them")
        return [[center_box(v.shape[2], v.shape[3])] * v.shape[0] for v in views]
    crop = list(crop)
    single = len(crop) == 4 and not any(isinstance(v, (tuple, list)) for v in crop)
    if not single and len(crop) != count:
        raise ValueError(f"crop lists {len(crop)} boxes for {count} images")
    try:
        flat = [tuple(operator.index(e) for e in b) for b in ([crop] * count if single else crop)]
    except TypeError:
        raise ValueError(f"a crop box is four integers (top, left, height, width), got {crop!r}") from None
    out, i = [], 0
    for v in views:
        mine = flat[i:i + v.shape[0]]
        i += v.shape[0]
        for b in mine:
            if len(b) != 4:
                raise ValueError(f"a crop box is four integers (top, left, height, width), got {b!r}")
            top, left, ch, cw = b
            if top < 0 or left < 0 or ch < 1 or cw < 1 or top + ch > v.shape[2] or left + cw > v.shape[3]:
                raise ValueError(f"crop box {b} is empty or not inside a {v.shape[2]} x {v.shape[3]} image")
        out.append(mine)
    return out


def _per_channel(v, c: int, default: float, what: str) -> list:
    if v is None:
        return [default] * c
    vals = [float(v)] * c if isinstance(v, (int, float)) else [float(e) for e in v]
    if len(vals) != c:
        raise ValueError(f"{what}: a number or {c} numbers, got {len(vals)}")
    return vals


def chain(items, c, oh, ow, antialias, reverse, mean, std, out):
    """The step in torch ops, image by image, on the tensors' device: crop view, .float(), F.interpolate (bilinear, half-pixel
    centres) unless the box already has the output size, flip, subtract, divide, and the copy into `out`."""
    dev = out.device
    m = torch.tensor(mean, dtype=torch.float32, device=dev).view(c, 1, 1)
    s = torch.tensor(std, dtype=torch.float32, device=dev).view(c, 1, 1)
    g = 0
    for x, (top, left, ch, cw) in items:
        for i in range(x.shape[0]):
            v = x[i, :, top:top + ch, left:left + cw].float()
            if (ch, cw) != (oh, ow):
                v = F.interpolate(v[None], size=(oh, ow), mode="bilinear", align_corners=False, antialias=antialias)[0]
            if reverse:
                v = v.flip(0)
            out[g].copy_((v - m) / s)
            g += 1
    return out


def prepare_images(images: Union[torch.Tensor, Sequence[torch.Tensor]], size=None, *, crop=None, antialias: bool = True,
                   mean=None, std=None, reverse_channels: bool = False, channels_last: Optional[bool] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [N, C, oh, ow]: every image cropped, resized to `size`, its channels reversed and normalised.

    images: a tensor [N, C, H, W] / [N, H, W, C], a single 3-D image, or a list / tuple of 3-D images of any sizes (uint8
    and float32 may be mixed) on one device.  channels_last: None infers it (last axis <= 4 < first image axis: channels
    last; the other way round: channels first; anything else raises).  size: None keeps the crop's size (no resampling), an
    integer or (oh, ow).  crop: None (the whole image), "center" (the centred square), one (top, left, height, width) or a
    list of them, one per image.  mean / std: None (0 / 1), a number or C numbers, indexed by OUTPUT channel.  out: an fp32
    [N, C, oh, ow] tensor on the same device, contiguous within an image, any batch stride: written in place and returned."""
    if isinstance(images, torch.Tensor):
        views = [_as_nchw(images, channels_last, "images")]
    elif isinstance(images, (list, tuple)) and len(images) > 0:
        for i, x in enumerate(images):
            if not isinstance(x, torch.Tensor) or x.dim() != 3:
                raise ValueError(f"images[{i}] must be a 3-D image tensor")
        views = [_as_nchw(x, channels_last, f"images[{i}]") for i, x in enumerate(images)]
    else:
        raise ValueError("images: a tensor or a non-empty list / tuple of 3-D tensors")
    dev, c = views[0].device, views[0].shape[1]
    if any(v.device != dev for v in views) or any(v.shape[1] != c for v in views):
        raise ValueError("every image must be on the same device and have the same number of channels")
    boxes = _boxes(crop, views)
    if size is None:
        sizes = {b[2:] for per in boxes for b in per}
        if len(sizes) != 1:
            raise ValueError(f"size=None keeps the crop's size, and the crops have different sizes: {sorted(sizes)}")
        oh, ow = sizes.pop()
    else:
        oh, ow = (size, size) if isinstance(size, int) else tuple(size)
        if not (isinstance(oh, int) and isinstance(ow, int) and oh >= 1 and ow >= 1):
            raise ValueError(f"size: None, a positive integer or two of them, got {size!r}")
    mean_c, std_c = _per_channel(mean, c, 0.0, "mean"), _per_channel(std, c, 1.0, "std")
    if any(s == 0.0 for s in std_c):
        raise ValueError("std must not be zero")
    # one item per run of images that share a view and a box: a uniform batch with one box is ONE item
    items = []
    for v, per in zip(views, boxes):
        if len(set(per)) == 1:
            items.append((v, per[0]))
        else:
            items += [(v[i:i + 1], b) for i, b in enumerate(per)]
    n = sum(v.shape[0] for v in views)
    if out is None:
        out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=dev)
    elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != (n, c, oh, ow) or out.dtype != torch.float32
            or out.device != dev or not out[0].is_contiguous() or (n > 1 and out.stride(0) < c * oh * ow)):
        raise ValueError(f"out must be a float32 [{n}, {c}, {oh}, {ow}] tensor on {dev}, contiguous within an image")
    fused = sys.modules[__package__].fused_image_prep
    if not R.cpu_plumbing(views[0], "prepare_images"):
        if FIO.prepare_images(fused, items, c, oh, ow, antialias, reverse_channels, mean_c, std_c, out) is not None:
            return out
    return chain(items, c, oh, ow, bool(antialias), bool(reverse_channels), mean_c, std_c, out)
