"""GPU: the media samples on the device -- pio_finish_media through raw ctypes on every case of tests/media_cases.py, bytes
equal to media.restatement (which tests/test_media_host.py holds to numpy's formulas), y at every alignment inside a
sentinel-filled guard band that must stay untouched; the refusals; to_frames / to_pcm16 against the raw entry, with the
switch off, on other inputs, on the model's own view without a copy; graph capture."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import media_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096
RUNS = [(n, off) for n in sorted(MC.CASES) for off in MC.Y_OFFSETS.get(n, (0,))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


_WANT = {}


def want_bytes(name):
    """The restatement of the case on the CPU as flat bytes, computed once and shared (read-only)."""
    if name not in _WANT:
        from perceiverio_pytorch_amd import media as M
        y = M.restatement(torch.from_numpy(np.array(MC.gen(name))), MC.kind_of(name), MC.reverse_of(name))
        assert np.array_equal(y.numpy(), MC.definition(MC.gen(name), MC.kind_of(name), MC.reverse_of(name)))
        _WANT[name] = y.reshape(-1).view(torch.uint8).clone()
    return _WANT[name]


def run_raw(dev, name, y_off=0):
    """One call of the raw entry on the case in its layout, y at byte y_off behind a 4 KiB band; returns (code, buffer,
    pattern, number of output bytes)."""
    from perceiverio_pytorch_amd import _lib as L
    storage, off, strides = MC.place(name)
    x = torch.from_numpy(storage).to(dev)
    nbytes = MC.gen(name).size * (1 if MC.kind_of(name) == MC.U8 else 2)
    pattern = ((torch.arange(GUARD + 16, dtype=torch.int64) * 37 + 11) % 251).to(torch.uint8).to(dev)
    buf = torch.full((GUARD + 16 + nbytes + GUARD + 16,), 0x5a, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
    start = GUARD + y_off
    buf[:start], buf[start + nbytes:start + nbytes + GUARD] = pattern[:start], pattern[:GUARD]
    code = MC.raw(L, x.data_ptr() + 4 * off, strides, MC.gen(name).shape, MC.kind_of(name), MC.reverse_of(name),
                  buf.data_ptr() + start, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code, buf, pattern, nbytes, start


@pytest.mark.parametrize("name,y_off", RUNS, ids=[f"{n}-y{o}" for n, o in RUNS])
def test_raw_entry_equals_the_restatement_inside_guard_bands(dev, name, y_off):
    code, buf, pattern, nbytes, start = run_raw(dev, name, y_off)
    assert code == MC.PIO_OK
    assert torch.equal(buf[:start], pattern[:start]), "bytes in FRONT of y were written"
    assert torch.equal(buf[start + nbytes:start + nbytes + GUARD], pattern[:GUARD]), "bytes BEHIND y were written"
    assert bool((buf[start + nbytes + GUARD:] == 0x5a).all())
    got, want = buf[start:start + nbytes].cpu(), want_bytes(name)
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want).reshape(-1)
        raise AssertionError(f"{name} at y + {y_off}: {bad.numel()} of {nbytes} bytes differ, first at byte {int(bad[0])}: "
                             f"{int(got[bad[0]])} for {int(want[bad[0]])}")


@pytest.mark.parametrize("what,ch,code", MC.REFUSALS, ids=[r[0] for r in MC.REFUSALS])
def test_refusals_leave_the_output_untouched(dev, what, ch, code):
    from perceiverio_pytorch_amd import _lib as L
    h, w, c = MC.R_H, MC.R_W, MC.R_C
    x = torch.rand(h * w * c + 8, device=dev)
    out = torch.full((2 * h * w * c + 8,), 0x5a, dtype=torch.uint8, device=dev)
    shape = (ch.get("n", 1), ch.get("h", h), ch.get("w", w), ch.get("C", c))
    got = MC.raw(L, None if "x" in ch else x.data_ptr() + ch.get("x_offset", 0), (h * w * c, w * c, c, 1), shape,
                 ch.get("kind", MC.U8), ch.get("reverse", 0), None if "y" in ch else out.data_ptr() + ch.get("y_offset", 0),
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert got == code, (what, got)
    assert bool((out == 0x5a).all()), f"{what}: a refused call wrote"


def test_the_valid_call_of_the_refusal_table_runs(dev):
    from perceiverio_pytorch_amd import _lib as L, media as M
    h, w, c = MC.R_H, MC.R_W, MC.R_C
    x = torch.rand((1, h, w, c), device=dev)
    out = torch.full((h * w * c + 8,), 0x5a, dtype=torch.uint8, device=dev)
    assert MC.raw(L, x.data_ptr(), (h * w * c, w * c, c, 1), (1, h, w, c), MC.U8, 0, out.data_ptr(),
                  torch.cuda.current_stream().cuda_stream) == MC.PIO_OK
    torch.cuda.synchronize()
    assert torch.equal(out[:h * w * c].cpu(), M.restatement(x.cpu(), M.U8).reshape(-1)) and bool((out[h * w * c:] == 0x5a).all())


def _spy(monkeypatch):
    """runtime.call as fused_io sees it: the pio_finish_media calls kept, everything passed on."""
    from perceiverio_pytorch_amd import runtime as R
    calls, real = [], R.call

    def call(dev, name, *args, **kw):
        if name == "pio_finish_media":
            calls.append(args)
        return real(dev, name, *args, **kw)
    monkeypatch.setattr(R, "call", call)
    return calls


def device_view(dev, name):
    storage, off, strides = MC.place(name)
    return torch.from_numpy(storage).to(dev).as_strided(MC.gen(name).shape, strides, off)


@pytest.mark.parametrize("name", ["u8_p1027", "u8_n3_flat", "u8_chw", "u8_crop", "u8_n3_gap", "u8_p5_c1", "s16_p1027_c3",
                                  "s16_chw_c2", "s16_crop"])
def test_python_functions_equal_the_raw_entry_and_the_switch(dev, monkeypatch, name):
    """to_frames (U8 cases, their [n, h, w, C] view as channels-last frames) and to_pcm16 (S16 cases, the view as a
    waveform of that shape): one launch on the view's own pointer, the raw entry's bytes; fused_media = False: no launch,
    the same bytes."""
    import perceiverio_pytorch_amd as P
    calls = _spy(monkeypatch)
    view = device_view(dev, name)
    code, buf, _, nbytes, start = run_raw(dev, name)
    assert code == MC.PIO_OK
    raw_bytes = buf[start:start + nbytes]

    def public():
        if MC.kind_of(name) == MC.U8:
            return P.to_frames(view, bgr=MC.reverse_of(name), channels_first=False)
        return P.to_pcm16(view)
    got = public()
    assert tuple(got.shape) == tuple(view.shape) and got.is_contiguous() and got.device == view.device
    assert got.dtype == (torch.uint8 if MC.kind_of(name) == MC.U8 else torch.int16)
    assert len(calls) == 1
    if MC.kind_of(name) == MC.U8 or view.is_contiguous() or view.dim() <= 3:
        assert calls[0][0] == view.data_ptr(), "the view was copied"
    assert torch.equal(got.reshape(-1).view(torch.uint8), raw_bytes)
    monkeypatch.setattr(P, "fused_media", False)
    off = public()
    assert len(calls) == 1 and torch.equal(off, got)


def test_models_image_view_is_read_in_place(dev, monkeypatch):
    """[b, t, 3, h, w] seen through moveaxis over [b, t*h*w, 3] storage, as MultiModalPerceiver hands its image out: one
    launch on the storage's own pointer with b*t images of adjacent rows (the contiguous path), no copy."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import media as M
    calls = _spy(monkeypatch)
    b, t, h, w = 2, 3, 10, 14
    store = torch.rand((b, t * h * w, 3), device=dev) * 1.5 - 0.25
    view = store.reshape(b, t, h, w, 3).moveaxis(-1, -3)
    assert not view.is_contiguous() and tuple(view.shape) == (b, t, 3, h, w)
    frames = P.to_frames(view)
    assert len(calls) == 1
    a = calls[0]
    assert a[0] == store.data_ptr() and tuple(a[1:5]) == (h * w * 3, w * 3, 3, 1) and tuple(a[5:9]) == (b * t, h, w, 3)
    assert tuple(frames.shape) == (b, t, h, w, 3)
    assert torch.equal(frames.cpu(), M.restatement(store.cpu().reshape(b, t, h, w, 3), M.U8))
    # leading axes that do not collapse: ONE copy, still one launch
    part = P.to_frames(view[:, ::2])
    assert len(calls) == 2 and calls[1][0] != store.data_ptr() and torch.equal(part, frames[:, ::2])


def test_other_inputs_take_the_restatement(dev, monkeypatch):
    import perceiverio_pytorch_amd as P
    calls = _spy(monkeypatch)
    view = device_view(dev, "u8_chw")
    want = P.to_frames(view, channels_first=False)
    assert len(calls) == 1
    assert torch.equal(P.to_frames(view.double(), channels_first=False), want)
    assert torch.equal(P.to_frames(view.half().float().half(), channels_first=False),
                       P.to_frames(view.half().float(), channels_first=False))
    cpu = P.to_frames(view.cpu(), channels_first=False)
    assert cpu.device.type == "cpu" and torch.equal(cpu, want.cpu())
    assert len(calls) == 2                                                       # (the fp32 image of the half tensor)
    audio = device_view(dev, "s16_p1027")
    assert torch.equal(P.to_pcm16(audio.double()), P.to_pcm16(audio)) and len(calls) == 3


def test_capturable(dev):
    """No synchronisation, no host read: both calls capture into a graph, and the replay follows the input."""
    import perceiverio_pytorch_amd as P
    x = device_view(dev, "u8_n3_flat").clone()
    a = device_view(dev, "s16_p1027").clone()
    eager = P.to_frames(x, channels_first=False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frames, pcm = P.to_frames(x, channels_first=False), P.to_pcm16(a)
    x.copy_(torch.nan_to_num(x, nan=0.3, posinf=2.0, neginf=-2.0).flip(2) * 0.5)
    a.copy_(torch.nan_to_num(a, nan=0.1, posinf=2.0, neginf=-2.0).flip(2) * 0.25)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(frames, P.to_frames(x, channels_first=False)) and not torch.equal(frames, eager)
    assert torch.equal(pcm, P.to_pcm16(a))
