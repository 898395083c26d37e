"""Optical-flow visualisation on the tensor's own device: utils/flow_utils.py flow_to_image (the Middlebury colour wheel,
every image scaled by its own largest radius) for torch tensors.

CUDA fp32 flows under the hip backend go through pio_flow_to_image (csrc/pio_flowviz.hip): read in place through their
strides, two launches behind a memset of the maxima words, no synchronisation, no host read.  CPU tensors, other dtypes
(upcast to fp32), the torch backend (CPU tensors only: that backend's rule) and fused_flow_image = False run
`restatement`, the same formula in torch ops on the tensor's device."""
from __future__ import annotations

import math
import sys
from typing import Optional

import torch

from . import runtime as R

SEGMENTS = (15, 6, 4, 11, 13, 6)          # RY YG GC CB BM MR
_wheels = {}


def colorwheel() -> list:
    """The 55 x 3 wheel as integers: per segment one channel at 255, one ramping floor(255 i / n) (rising in the even
    segments, falling from 255 in the odd ones), one at 0."""
    rows = []
    for s, n in enumerate(SEGMENTS):
        full, ramping = ((s + 1) // 2) % 3, (1 + 2 * s) % 3
        for i in range(n):
            row = [0, 0, 0]
            row[full] = 255
            row[ramping] = 255 - 255 * i // n if s % 2 else 255 * i // n
            rows.append(row)
    return rows


def _wheel_on(device: torch.device) -> torch.Tensor:
    if device not in _wheels:                  # (one copy per device, ever: not per call)
        _wheels[device] = torch.tensor(colorwheel(), dtype=torch.float64).to(device)
    return _wheels[device]


def _sqrt(x: torch.Tensor) -> torch.Tensor:
    # the correctly rounded fp32 square root on every device: through float64 (53 >= 2 * 24 + 2 bits: the second rounding
    # never changes the result); torch.sqrt of an fp32 CPU tensor is not correctly rounded
    return torch.sqrt(x.double()).float()


def _div(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return (x.double() / y.double()).float()       # correctly rounded for the same reason, whatever the device's fp32 division


def normalised(flow: torch.Tensor, clip_flow: Optional[float] = None):
    """(u_n, v_n, rad_n) of an fp32 [b, h, w, 2] flow: numpy's fp32 operations one by one (clip with the lower bound 0,
    radius, the maximum of every image on its own, + 1e-5, two divisions, radius again)."""
    if clip_flow is not None:
        flow = torch.where(flow < 0, 0.0, flow)            # (as np.clip: a bound replaces what lies strictly beyond it,
        flow = torch.where(flow > clip_flow, float(clip_flow), flow)       # -0 stays -0)
    u, v = flow[..., 0], flow[..., 1]
    s = _sqrt(u * u + v * v).amax(dim=(1, 2), keepdim=True) + 1e-5
    un, vn = _div(u, s), _div(v, s)
    return un, vn, _sqrt(un * un + vn * vn)


def restatement(flow: torch.Tensor, clip_flow: Optional[float] = None, convert_to_bgr: bool = False) -> torch.Tensor:
    """flow_to_image of an fp32 [b, h, w, 2] tensor in torch ops, on its device: uint8 [b, h, w, 3].  As in numpy the wheel
    position is fp32 and everything behind `pos - k0` float64."""
    un, vn, radn = normalised(flow, clip_flow)
    wheel = _wheel_on(flow.device)
    n = wheel.shape[0]
    pos = (torch.atan2(-vn, -un) / math.pi + 1) / 2 * (n - 1)
    k0f = torch.floor(pos)
    k0 = k0f.clamp(0, n - 1).long()
    k1 = torch.where(k0 + 1 == n, 0, k0 + 1)
    frac = (pos.double() - k0f.double()).unsqueeze(-1)
    col = (1 - frac) * wheel[k0] / 255.0 + frac * wheel[k1] / 255.0
    radn = radn.unsqueeze(-1)
    col = torch.where(radn <= 1, 1 - radn * (1 - col), col * 0.75)
    img = torch.floor(255 * col).clamp(0, 255).to(torch.uint8)
    return img.flip(-1).contiguous() if convert_to_bgr else img


def flow_to_image(flow: torch.Tensor, clip_flow: Optional[float] = None, convert_to_bgr: bool = False) -> torch.Tensor:
    """The colour image of a flow field [h, w, 2] (utils/flow_utils.py's layout) or a batch [b, h, w, 2] of them, views
    welcome (the model's [b, 2, h, w] as .permute(0, 2, 3, 1)): uint8 [h, w, 3] or [b, h, w, 3] on the same device."""
    if not isinstance(flow, torch.Tensor):
        raise TypeError("flow_to_image takes a torch tensor (utils.flow_utils.flow_to_image takes numpy arrays as well)")
    if flow.dim() not in (3, 4) or flow.shape[-1] != 2:
        raise ValueError(f"input flow must have shape [H,W,2] or [B,H,W,2], got {tuple(flow.shape)}")
    f4 = flow.unsqueeze(0) if flow.dim() == 3 else flow
    b, h, w, _ = f4.shape
    if b < 1 or h < 1 or w < 1:
        raise ValueError(f"input flow is empty: {tuple(flow.shape)}")
    fused = sys.modules[__package__].fused_flow_image
    if R.cpu_plumbing(flow, "flow_to_image") or not flow.is_cuda or flow.dtype != torch.float32 or not fused:
        img = restatement(f4.detach().float(), clip_flow, convert_to_bgr)
    else:
        dev = flow.device
        img = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev)
        rad_max = torch.empty(b, dtype=torch.int32, device=dev)
        sn, sy, sx, sc = f4.stride()
        R.call_named(dev, "pio_flow_to_image", flow=f4.data_ptr(), sn=sn, sy=sy, sx=sx, sc=sc, b=b, h=h, w=w,
                     clip_flow=0.0 if clip_flow is None else float(clip_flow), has_clip=clip_flow is not None,
                     bgr=bool(convert_to_bgr), out=img.data_ptr(), rad_max=rad_max.data_ptr())
    return img[0] if flow.dim() == 3 else img
