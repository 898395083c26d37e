"""GPU: the multimodal front end -- pio_assemble_tokens through the raw C-ABI on every case of tests/mm_front_cases.py
against the definition, bit for bit; the fused branch of MultimodalPreprocessor against its own chain of copies; and
MultiModalPerceiver.fused_front_end on the small golden and on the full-size front end.

No tolerance anywhere: the call only moves values, and the masked expression token + 0 * x is exact (where x is not
finite both sides give NaN, whose sign and payload are the platform's: there the NaN POSITIONS are compared).

Memory safety by construction: the output sits between 4 KiB guard bands and is NaN before the call; ldy gaps and rows no
segment covers must still be NaN afterwards; every input is surrounded by NaN, and every unmasked output must be finite."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mm_front_cases as MC  # noqa: E402
from test_flow_front_gpu import GuardedOut  # noqa: E402
from test_mm_front_host import (MODULE_CASES, assemble, assert_same_bits, module_case, module_inputs)  # noqa: E402
from test_models import TOL, _close, _load_generated, build  # noqa: E402
from _golden import load  # noqa: E402
from cases import model_inputs, model_seed, model_stats  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


_REF = {}


def case_data(name):
    """(inputs, definition) of a case, computed once and shared (read-only) by the tests below."""
    if name not in _REF:
        data = MC.gen(name)
        _REF[name] = (data, MC.reference(name, data))
    return _REF[name]


def launch(dev, name, data):
    """One call of the raw entry on the case's NaN-surrounded inputs; returns the guarded output [B Mtot, ldy]."""
    from perceiverio_pytorch_amd import _lib as L
    c = MC.CASES[name]
    held = {}
    for i, d in enumerate(data):
        for what in ("feat", "table", "pad", "token"):
            if d[what + "_full"] is not None:
                held[(i, what)] = torch.from_numpy(d[what + "_full"]).to(dev)
    segs, args = MC.call_fields(name, data, lambda i, what: held[(i, what)].data_ptr())
    y = GuardedOut(dev, c["B"] * c["Mtot"], c["ldy"])
    L.check(assemble(L, segs, y.t.data_ptr(), args, torch.cuda.current_stream().cuda_stream), f"pio_assemble_tokens[{name}]")
    y.check(name)
    return y


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_raw_entry_against_the_definition(dev, name):
    c = MC.CASES[name]
    data, ref = case_data(name)
    y = launch(dev, name, data)
    got = y.t.cpu().numpy().reshape(ref.shape)
    cov = np.broadcast_to(MC.covered(name), ref.shape)
    masked = MC.masked_rows(name)
    assert np.isnan(got[~cov]).all(), f"{name}: an ldy gap or a row no segment covers was written"
    unmasked = cov & ~masked[None, :, None]
    assert np.isfinite(got[unmasked]).all(), f"{name}: non-finite unmasked outputs (a read outside an input?)"
    # (outside the covered elements both sides are the NaN prefill: bit-equal as well)
    assert_same_bits(got, ref, name, masked=masked)
    if name in MC.PLANTED:
        assert np.array_equal(np.isnan(got[cov]), np.isnan(ref[cov])) and np.isnan(got[cov]).sum() == len(MC.PLANTED[name][1])
    y2 = launch(dev, name, data)
    assert torch.equal(y.t.view(torch.int32), y2.t.view(torch.int32)), f"{name}: two launches differ"


def _refusal_buffers(dev):
    bufs = {"y": GuardedOut(dev, MC.VALID_ARGS["B"] * MC.VALID_ARGS["Mtot"] + 4, 16)}       # (room for moved pointers / ldy = 10)
    for i, fields in enumerate(MC.VALID_PTRS):
        for f in fields:
            bufs[(i, f)] = torch.randn(256, device=dev)
    ptrs = {k: (v.t.data_ptr() if k == "y" else v.data_ptr()) for k, v in bufs.items()}
    return bufs, ptrs


def test_the_valid_call_of_the_refusal_table_runs(dev):
    from perceiverio_pytorch_amd import _lib as L
    bufs, ptrs = _refusal_buffers(dev)
    segs, args, y = MC.refusal_fields(ptrs, {})
    assert assemble(L, segs, y, args, torch.cuda.current_stream().cuda_stream) == MC.PIO_OK
    bufs["y"].check("valid call")
    out = bufs["y"].t.reshape(-1)[:2 * 56].reshape(2, 7, 8)
    assert bool(torch.isfinite(out).all()) and bool(torch.isnan(bufs["y"].t.reshape(-1)[2 * 56:]).all())


@pytest.mark.parametrize("what,changes,code", MC.REFUSALS, ids=[r[0] for r in MC.REFUSALS])
def test_refusals_launch_nothing(dev, what, changes, code):
    from perceiverio_pytorch_amd import _lib as L
    bufs, ptrs = _refusal_buffers(dev)
    segs, args, y = MC.refusal_fields(ptrs, changes)
    assert assemble(L, segs, y, args, torch.cuda.current_stream().cuda_stream) == code
    bufs["y"].check(what)
    assert torch.isnan(bufs["y"].t).all(), f"{what}: a refused call wrote to y"


def _counting_cat(monkeypatch):
    """torch.cat as perceiver.py and fused_io.py see it, counted (the modules' `torch` name is replaced by a stand-in that
    forwards everything else)."""
    from perceiverio_pytorch_amd import fused_io as FIO
    from perceiverio_pytorch_amd import perceiver as PV
    calls = []

    class _Torch:
        def __getattr__(self, k):
            return getattr(torch, k)

        def cat(self, *a, **kw):
            calls.append(1)
            return torch.cat(*a, **kw)
    monkeypatch.setattr(PV, "torch", _Torch())
    monkeypatch.setattr(FIO, "torch", PV.torch)
    return calls


@pytest.mark.parametrize("name", ["mini_model", "s2d_small", "masked"])
def test_preprocessor_fused_on_and_off(dev, name, monkeypatch):
    """MultimodalPreprocessor on CUDA inputs (mini_model: Cc = 405, the dword path; s2d_small: Cc = 60, 16-byte rows):
    fused on and off give equal x, sizes and without_pos, both equal to the definition; on, perceiver.py calls no
    torch.cat."""
    mm, data = module_case(name)
    mm = mm.to(dev)
    ins = module_inputs(name, data, dev)
    ref = MC.reference(name, data)
    calls = _counting_cat(monkeypatch)
    assert mm.fused_assembly is True
    x_on, sizes_on, wo_on = mm(ins)
    assert calls == [], "the fused path called torch.cat"
    assert mm._assemble(ins, None) is not None
    mm.fused_assembly = False
    x_off, sizes_off, wo_off = mm(ins)
    assert len(calls) >= 1
    masked = MC.masked_rows(name)
    assert_same_bits(x_on.cpu().numpy(), ref, f"{name} fused", masked=masked)
    assert_same_bits(x_off.cpu().numpy(), ref, f"{name} chain", masked=masked)
    if name not in MC.PLANTED:
        assert torch.equal(x_on, x_off)
    assert sizes_on == sizes_off and list(sizes_on) == list(sizes_off)
    assert sorted(wo_on) == sorted(wo_off)
    for m in wo_on:
        assert wo_on[m].shape == wo_off[m].shape
        assert torch.equal(wo_on[m].contiguous().view(torch.int32), wo_off[m].contiguous().view(torch.int32)), m
    for m, g in zip(MODULE_CASES[name], MC.CASES[name]["segs"]):
        if not g["masked"]:                    # a view of x: no extra copy
            assert wo_on[m].data_ptr() == x_on[:, g["row0"]:, :].data_ptr()


def test_small_golden_fused_on_and_off(dev):
    name = "model_multimodal_small"
    g = load(name)
    model = _load_generated(build(name), g, dev, model_seed(name), model_stats(name))
    assert model.fused_front_end is True and model.perceiver._multi_preprocessor.fused_assembly is True
    ins = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]
    outs = {}
    for encode_once in (True, False):
        model.encode_once = encode_once
        for on in (True, False):
            model.fused_front_end = on
            assert model.perceiver._multi_preprocessor.fused_assembly is on
            with torch.inference_mode():
                out = model(ins[0], ins[1], n_chunks=2)
            for m in ("image", "audio", "label"):
                _close(out[m], g[f"out_{m}"], f"{name} {m}, fused={on}, encode_once={encode_once}", TOL)
            outs[(encode_once, on)] = out
        for m in ("image", "audio", "label"):
            assert torch.equal(outs[(encode_once, True)][m], outs[(encode_once, False)][m]), (m, encode_once)


def test_full_size_front_end(dev):
    """The default MultiModalPerceiver's front end at full size, B = 1: 1 920 audio + 50 176 video + 1 label rows of 704
    channels -- the real strip counts and the 50 176-row position table."""
    name = "model_multimodal_full"
    g = load(name)
    model = _load_generated(build(name), g, dev, model_seed(name), model_stats(name))
    images, audio = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]
    inputs = {"image": images, "audio": audio, "label": torch.zeros((images.shape[0], model.num_classes), device=dev)}
    mp = model.perceiver._multi_preprocessor
    assert mp.fused_assembly is True and mp._assemble(inputs, None) is not None
    x_on, sizes_on, wo_on = mp(inputs, pos=None)
    mp.fused_assembly = False
    x_off, sizes_off, wo_off = mp(inputs, pos=None)
    assert x_on.shape == (1, 52097, 704) and sizes_on == sizes_off == {"audio": 1920, "image": 50176, "label": 1}
    assert bool(torch.isfinite(x_on).all())
    assert torch.equal(x_on, x_off)
    for m in wo_on:
        assert torch.equal(wo_on[m], wo_off[m]), m
