"""Logit probe: how large are a model's attention logits, and which parts need pair-operand Q K^T?

The fused attention cores round q and k once to fp16 in front of Q K^T, which puts delta s ~ |s| 2^-11 into the exponent.
For logits of O(1) that is invisible; with trained LayerNorm gains |s| reaches 10-15 and it is not (models.py, KNOWN
LIMIT).  `logit_probe()` measures max |q . k| / sqrt(dk) of every attention call of a forward -- a separate calibration
kernel (csrc/pio_qkprobe.hip) behind the process-wide switch pio_logit_probe_begin / _end, or plain torch under the CPU
plumbing backend -- and `recommend_precision_policy()` turns the figures into a "cross/stack/decoder" policy string.

Range probe: do a model's 16-bit operands fit fp16, and if not, which part has to run in bf16?

Every matrix operand inside the library is 16-bit; with fp16 anything beyond 65 504 becomes inf and the forward returns
NaN.  `range_probe()` measures max |x| of every 16-bit activation buffer a forward produces -- LayerNorm / cast outputs,
q / k / v projections, attention-core outputs, GELU'd hidden activations, the LayerNorm fold's 16-bit residual stream and
the decoders' y16 -- with a separate calibration kernel (csrc/pio_rangeprobe.hip) behind the process-wide switch
pio_range_probe_begin / _end, or plain torch on the same tensors under the CPU plumbing backend (fp32 there: the true
magnitude), and `recommend_operand_dtype()` turns the figures into a "cross/stack/decoder" policy string.

Tooling, not product path: one probe of each kind at a time (a logit_probe and a range_probe may be active together), one
device, not thread-safe, not capturable.  With a probe off nothing is measured and nothing extra is launched.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L
from . import runtime as R

PARTS = ("cross", "stack", "decoder", "attention")

_active: Optional["logit_probe"] = None
_part: List[str] = []          # CPU plumbing: the part the enclosing encoder / decoder names for the calls inside it


def active() -> bool:
    return _active is not None


class part:
    """CPU plumbing backend: label the attention calls made inside the block (a no-op without an active probe)."""

    def __init__(self, name: str):
        assert name in PARTS
        self._name = name

    def __enter__(self):
        _part.append(self._name)
        return self

    def __exit__(self, *exc):
        _part.pop()
        return False


def expect(*labels: str) -> None:
    """HIP backend: the labels, in call order, of the attention calls the library call that follows will make."""
    if _active is not None:
        _active._labels.extend(labels)


def record_cpu(q: torch.Tensor, k: torch.Tensor, attention_mask: Optional[torch.Tensor]) -> None:
    """CPU plumbing backend: q [B,H,Tq,d], k [B,H,Tk,d] as projected, attention_mask [B,Tq,Tk] (bool) or None -- the
    quantity and the mask semantics of pio_qk_logit_absmax (no bias; a non-finite product reports inf; nothing attendable
    gives 0)."""
    if _active is None:
        return
    s = (q.detach().double() @ k.detach().double().transpose(-1, -2)).abs() * (1.0 / math.sqrt(q.shape[-1]))
    s = torch.where(torch.isfinite(s), s, torch.full_like(s, float("inf")))
    if attention_mask is not None:
        s = torch.where(attention_mask[:, None, :, :].bool(), s, torch.zeros_like(s))
    _active.records.append((_part[-1] if _part else "attention", float(s.max()) if s.numel() else 0.0))


class logit_probe:
    """Context manager: after exit, `.records` is the list of (part, absmax) of every attention call made inside it, in
    call order; part is "cross" / "stack" / "decoder" (PerceiverEncoder / PerceiverDecoder forwards) or "attention" (the
    raw Attention / SelfAttention / CrossAttention modules).  `.by_part()` gives the maximum per part.

    On the HIP backend the records live in a device buffer of `max_records` floats on the current device (calls past it
    are counted in `.calls` but not recorded); exit synchronises that device.  Entering during stream capture raises."""

    def __init__(self, max_records: int = 4096):
        if max_records <= 0:
            raise ValueError("max_records must be positive")
        self.max_records = int(max_records)
        self.records: List[Tuple[str, float]] = []
        self.calls = 0
        self._labels: List[str] = []
        self._buf = None

    def __enter__(self):
        global _active
        if _active is not None:
            raise L.PioError("logit_probe: a probe is already active (one at a time: the switch is process-wide)")
        self.records, self._labels, self.calls = [], [], 0
        if R.get_backend() == "hip":
            if not torch.cuda.is_available():
                raise L.PioError("logit_probe: the HIP backend needs an MI355X device (CPU: set_backend('torch'))")
            dev = torch.device("cuda", torch.cuda.current_device())
            if R.capturing(dev):
                raise L.PioError("logit_probe: cannot start during stream capture (the probe is host-side state, and its "
                                 "records are read back on exit)")
            with torch.inference_mode(False):
                self._buf = torch.zeros(self.max_records, dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)      # (the zeros are in place whatever stream a call inside uses)
            L.check(L.lib().pio_logit_probe_begin(self._buf.data_ptr(), self.max_records), "pio_logit_probe_begin")
        _active = self
        return self

    def __exit__(self, *exc):
        global _active
        _active = None
        if self._buf is not None:
            n = int(L.lib().pio_logit_probe_end())
            buf, self._buf = self._buf, None
            torch.cuda.synchronize(buf.device)
            self.calls = n
            if exc[0] is None:
                if n != len(self._labels):
                    raise L.PioError(f"logit_probe: the library saw {n} attention calls, the modules announced "
                                     f"{len(self._labels)}")
                vals = buf[:min(n, self.max_records)].cpu().tolist()
                self.records = list(zip(self._labels, vals))
        else:
            self.calls = len(self.records)
        return False

    def by_part(self) -> dict:
        out: dict = {}
        for name, v in self.records:
            out[name] = max(out.get(name, 0.0), v)
        return out


# Default threshold of recommend_precision_policy: measured on the MI355X over every tests/golden/model_*.npz model at
# its class default (profiles/logit_probe.json).  Between the largest per-part figure among the
# goldens that hold 1e-3 at their class default (49.6: the stack of model_classify_b4_trained2) and the largest figure of
# model_language_trained, which does not (63.2: its encoder cross-attend); initialiser-like goldens stay below 8.4.
DEFAULT_THRESHOLD: Optional[float] = 56.0


def recommend_precision_policy(model, *inputs, threshold: Optional[float] = None, **kw):
    """Run ONE forward of `model(*inputs, **kw)` under the probe and return (policy string, report).

    The string starts from the model's current policy (`model.precision_policy`, else the ambient one) split into its
    three parts cross / stack / decoder (runtime.split_policy3); every part whose largest logit exceeds `threshold`
    becomes "fp16x3fq" (Q and K as fp16 pairs inside the fused cores), the others are left alone -- when none does, the
    model's own string comes back unchanged.  Nothing is set: assign `model.precision_policy` yourself.
    report = {"absmax": {part: figure}, "threshold": t, "calls": n, "policy": the model's current string}."""
    if threshold is None:
        threshold = DEFAULT_THRESHOLD
    if threshold is None:
        raise ValueError("recommend_precision_policy: no default threshold is set; pass threshold=")
    current = getattr(model, "precision_policy", None) or R.get_precision_policy()
    cross, stack, dec = R.split_policy3(current)
    parts = {"cross": cross if cross is not None else stack, "stack": stack, "decoder": dec}
    with torch.no_grad(), logit_probe() as probe:
        model(*inputs, **kw)
    figures = probe.by_part()
    changed = False
    for name in ("cross", "stack", "decoder"):
        if figures.get(name, 0.0) > threshold and parts[name] != "fp16x3fq":
            parts[name] = "fp16x3fq"
            changed = True
    policy = "/".join(parts[n] for n in ("cross", "stack", "decoder")) if changed else current
    return policy, {"absmax": figures, "threshold": float(threshold), "calls": probe.calls, "policy": current}


# ======================================================================================================================
# range probe
# ======================================================================================================================
# part / kind names, indexed by the library's PIO_RP_* / PIO_RK_* values (include/pio_hip.h)
RANGE_PARTS = ("attention", "cross", "stack", "decoder")
RANGE_KINDS = ("cast", "q", "k", "v", "attn", "hidden", "stream")
FP16_MAX = 65504.0

_range_active: Optional["range_probe"] = None


def range_active() -> bool:
    return _range_active is not None


def mark_range(name: str) -> None:
    """HIP backend: the part of the records the library call that follows will make (pio_range_probe_mark); "attention"
    resets it.  A no-op without an active range_probe on the HIP backend."""
    if _range_active is not None and _range_active._buf is not None:
        L.check(L.lib().pio_range_probe_mark(RANGE_PARTS.index(name)), "pio_range_probe_mark")


def record_range_cpu(kind: str, x: torch.Tensor) -> None:
    """CPU plumbing backend: max |x| of the fp32 tensor whose 16-bit image the HIP backend measures as `kind`, under the
    part the enclosing encoder / decoder names (a non-finite element reports inf, an empty tensor 0)."""
    if _range_active is None:
        return
    assert kind in RANGE_KINDS
    v = float(x.detach().abs().max()) if x.numel() else 0.0
    if not math.isfinite(v):
        v = float("inf")
    _range_active.records.append((_part[-1] if _part else "attention", kind, v))


class range_probe:
    """Context manager: after exit, `.records` is the list of (part, kind, absmax) of every 16-bit activation buffer
    produced inside it, in call order, and `.calls` their count.  part: "cross" / "stack" / "decoder" (PerceiverEncoder /
    PerceiverDecoder forwards) or "attention" (the raw Attention / MLP / SelfAttention / CrossAttention modules); kind:
    one of RANGE_KINDS.  `.by_part()` gives {part: {kind: max}}, `.worst()` {part: max}.

    On the HIP backend the figures live in a device buffer of `max_records` floats on the current device (buffers past it
    are counted in `.calls` but not recorded); exit synchronises that device.  Entering during stream capture raises.
    Only one range_probe may be active at a time; a logit_probe may be active beside it."""

    def __init__(self, max_records: int = 16384):
        if max_records <= 0:
            raise ValueError("max_records must be positive")
        self.max_records = int(max_records)
        self.records: List[Tuple[str, str, float]] = []
        self.calls = 0
        self._buf = None

    def __enter__(self):
        global _range_active
        if _range_active is not None:
            raise L.PioError("range_probe: a probe is already active (one at a time: the switch is process-wide)")
        self.records, self.calls = [], 0
        if R.get_backend() == "hip":
            if not torch.cuda.is_available():
                raise L.PioError("range_probe: the HIP backend needs an MI355X device (CPU: set_backend('torch'))")
            dev = torch.device("cuda", torch.cuda.current_device())
            if R.capturing(dev):
                raise L.PioError("range_probe: cannot start during stream capture (the probe is host-side state, and its "
                                 "records are read back on exit)")
            with torch.inference_mode(False):
                self._buf = torch.zeros(self.max_records, dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)      # (the zeros are in place whatever stream a call inside uses)
            L.check(L.lib().pio_range_probe_begin(self._buf.data_ptr(), self.max_records), "pio_range_probe_begin")
        _range_active = self
        return self

    def __exit__(self, *exc):
        global _range_active
        _range_active = None
        if self._buf is not None:
            parts = (C.c_int32 * self.max_records)()
            kinds = (C.c_int32 * self.max_records)()
            n = int(L.lib().pio_range_probe_end(parts, kinds, self.max_records))
            buf, self._buf = self._buf, None
            torch.cuda.synchronize(buf.device)
            self.calls = n
            # (the labels are the library's own: what was recorded before an exception stays readable)
            vals = buf[:min(n, self.max_records)].cpu().tolist()
            self.records = [(RANGE_PARTS[parts[i]], RANGE_KINDS[kinds[i]], v) for i, v in enumerate(vals)]
        else:
            self.calls = len(self.records)
        return False

    def by_part(self) -> Dict[str, Dict[str, float]]:
        out: Dict[str, Dict[str, float]] = {}
        for name, kind, v in self.records:
            d = out.setdefault(name, {})
            d[kind] = max(d.get(kind, 0.0), v)
        return out

    def worst(self) -> Dict[str, float]:
        return {name: max(d.values()) for name, d in self.by_part().items()}


def recommend_operand_dtype(model, *inputs, limit: float = FP16_MAX, **kw):
    """Run ONE forward of `model(*inputs, **kw)` under the range probe and return (policy string, report).

    The string starts from the model's current policy (`model.precision_policy`, else the ambient one) split into its
    three parts cross / stack / decoder (runtime.split_policy3); every part whose largest 16-bit operand is inf or exceeds
    `limit` becomes "bf16x3" -- the only bf16 policy that meets 1e-3 (runtime.py) -- the others are left alone, and when
    none does the model's own string comes back unchanged.  Nothing is set: assign `model.precision_policy` yourself.
    `limit` defaults to the fp16 maximum, 65 504 (not a tuned number): pass a lower one for headroom.
    report = {"absmax": {part: {kind: figure}}, "limit": l, "calls": n, "policy": the model's current string}.

    A forward that ends in the library's own PIO_E_RANGE error (the guard of the LayerNorm-folded stack) still yields its
    figures: that is the case the recommendation exists for."""
    current = getattr(model, "precision_policy", None) or R.get_precision_policy()
    cross, stack, dec = R.split_policy3(current)
    parts = {"cross": cross if cross is not None else stack, "stack": stack, "decoder": dec}
    probe = range_probe()
    try:
        with torch.no_grad(), probe:
            model(*inputs, **kw)
    except L.PioError as e:
        if "PIO_E_RANGE" not in str(e):
            raise
    worst = probe.worst()
    changed = False
    for name in ("cross", "stack", "decoder"):
        if worst.get(name, 0.0) > limit and parts[name] != "bf16x3":      # (inf > limit as well)
            parts[name] = "bf16x3"
            changed = True
    policy = "/".join(parts[n] for n in ("cross", "stack", "decoder")) if changed else current
    return policy, {"absmax": probe.by_part(), "limit": float(limit), "calls": probe.calls, "policy": current}
