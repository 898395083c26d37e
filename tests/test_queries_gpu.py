"""GPU: the decoder query builder -- pio_build_queries through the raw C-ABI on every case of tests/query_cases.py against
the definition (moves bit for bit, sine and cosine within QC.SINCOS_BOUND of the float64 value of the fp32 phase);
PerceiverIO.decoder_query's fused branch against the definition and against its own chain of torch ops; and
MultiModalPerceiver.fused_queries on the small golden.

Memory safety by construction: the output sits between 4 KiB guard bands and is NaN before the call; ldy gaps and rows no
segment covers must still be NaN afterwards; every float input is surrounded by NaN and the index points by indices of other
grid points, and every output must be finite and equal to the definition."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import query_cases as QC  # noqa: E402
from test_flow_front_gpu import GuardedOut  # noqa: E402
from test_queries_host import (MODULE_CASES, build_queries, module_case, module_points, stand_in)  # noqa: E402
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
        data = QC.gen(name)
        _REF[name] = (data, QC.reference(name, data))
    return _REF[name]


def launch(dev, name, data):
    """One call of the raw entry on the case's surrounded inputs; returns the guarded output [Qtot, ldy]."""
    from perceiverio_pytorch_amd import _lib as L
    c = QC.CASES[name]
    held = {}
    for i, d in enumerate(data):
        for what in QC.POINTER_FIELDS:
            if d[what + "_full"] is not None:
                held[(i, what)] = torch.from_numpy(d[what + "_full"]).to(dev)
    segs, args = QC.call_fields(name, data, lambda i, what: held[(i, what)].data_ptr())
    y = GuardedOut(dev, c["Qtot"], c["ldy"])
    L.check(build_queries(L, segs, y.t.data_ptr(), args, torch.cuda.current_stream().cuda_stream), f"pio_build_queries[{name}]")
    y.check(name)
    return y


@pytest.mark.parametrize("name", sorted(QC.CASES))
def test_raw_entry_against_the_definition(dev, name):
    data, ref = case_data(name)
    y = launch(dev, name, data)
    QC.compare(y.t.cpu().numpy(), ref, name)
    y2 = launch(dev, name, data)
    assert torch.equal(y.t.view(torch.int32), y2.t.view(torch.int32)), f"{name}: two launches differ"


def _refusal_buffers(dev):
    bufs = {"y": GuardedOut(dev, 8, 1024)}       # (room for Cq = 1024 and for moved pointers)
    for i in range(len(QC.VALID_SEGS)):
        for f in QC.POINTER_FIELDS:
            bufs[(i, f)] = torch.zeros(2048, dtype=torch.int64, device=dev) if f == "points" else \
                torch.randn(2048, device=dev)
    ptrs = {k: (v.t.data_ptr() if k == "y" else v.data_ptr()) for k, v in bufs.items()}
    return bufs, ptrs


@pytest.mark.parametrize("what,changes", QC.ACCEPTED, ids=[r[0] for r in QC.ACCEPTED])
def test_accepted_calls_of_the_refusal_table_run(dev, what, changes):
    """The valid call, and the alignments / pitches that only choose narrower stores: five rows written, nothing else."""
    from perceiverio_pytorch_amd import _lib as L
    bufs, ptrs = _refusal_buffers(dev)
    segs, args, y = QC.refusal_fields(ptrs, changes)
    assert build_queries(L, segs, y, args, torch.cuda.current_stream().cuda_stream) == QC.PIO_OK
    bufs["y"].check(what)
    flat = bufs["y"].t.reshape(-1)[(y - ptrs["y"]) // 4:]
    out = flat[:args["Qtot"] * args["ldy"]].reshape(args["Qtot"], args["ldy"])
    assert bool(torch.isfinite(out[:, :args["Cq"]]).all()) and bool(torch.isnan(out[:, args["Cq"]:]).all())
    assert bool(torch.isnan(flat[args["Qtot"] * args["ldy"]:]).all())


@pytest.mark.parametrize("what,changes,code", QC.REFUSALS, ids=[r[0] for r in QC.REFUSALS])
def test_refusals_launch_nothing(dev, what, changes, code):
    from perceiverio_pytorch_amd import _lib as L
    bufs, ptrs = _refusal_buffers(dev)
    segs, args, y = QC.refusal_fields(ptrs, changes)
    assert build_queries(L, segs, y, args, torch.cuda.current_stream().cuda_stream) == code
    bufs["y"].check(what)
    assert torch.isnan(bufs["y"].t).all(), f"{what}: a refused call wrote to y"


def _counting(monkeypatch):
    """torch.cat as perceiver.py and fused_io.py see it (the hook of tests/test_mm_front_gpu.py) and pio_build_queries as
    every module sees it, both counted."""
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd import fused_io as FIO
    from perceiverio_pytorch_amd import perceiver as PV
    calls = {"cat": 0, "kernel": 0}
    real = L.lib()

    class _Torch:
        def __getattr__(self, k):
            return getattr(torch, k)

        def cat(self, *a, **kw):
            calls["cat"] += 1
            return torch.cat(*a, **kw)

    class _Lib:
        def __getattr__(self, k):
            return getattr(real, k)

        def pio_build_queries(self, *a):
            calls["kernel"] += 1
            return real.pio_build_queries(*a)
    proxy = _Lib()
    monkeypatch.setattr(PV, "torch", _Torch())
    monkeypatch.setattr(FIO, "torch", PV.torch)
    monkeypatch.setattr(L, "lib", lambda: proxy)
    return calls


@pytest.mark.parametrize("name", sorted(MODULE_CASES))
def test_decoder_query_fused_on_and_off(dev, name, monkeypatch):
    """PerceiverIO.decoder_query on the GPU: the fused branch and the chain both equal the definition (moves bit for bit,
    the chain's own sines and cosines within the same bound); ONE kernel call and no torch.cat when eligible, no kernel call
    when not; the fused result is ONE array behind a stride-0 batch axis."""
    io, data = module_case(name)
    io = io.to(dev)
    c = QC.CASES[name]
    ref = QC.reference(name, data)
    pts = module_points(name, dev)
    x, sizes = stand_in(io, 3, dev)
    calls = _counting(monkeypatch)
    assert io.fused_queries is True
    with torch.no_grad():
        q_on, sizes_on = io.decoder_query(x, sizes, None, subsampled_points=pts)
    assert calls == {"cat": 0, "kernel": 1}, calls
    assert q_on.shape[0] == 3 and q_on.stride(0) == 0 and q_on.stride(2) == 1 and q_on.dtype == torch.float32
    io.fused_queries = False
    with torch.no_grad():
        q_off, sizes_off = io.decoder_query(x, sizes, None, subsampled_points=pts)
    assert calls["kernel"] == 1 and calls["cat"] >= 1, calls
    io.fused_queries = True
    full = {m: None for m in pts}                                            # Fourier queries over the full grid: the chain
    with torch.no_grad():
        q_full, _ = io.decoder_query(x, sizes, None, subsampled_points=full)
    assert calls["kernel"] == 1 and q_full.shape[2] == c["Cq"], calls
    assert q_on.shape == q_off.shape and sizes_on == sizes_off and list(sizes_on) == list(sizes_off)
    for q, what in ((q_on, "fused"), (q_off, "chain")):
        got = np.full(ref[0].shape, np.nan, dtype=np.float32)
        got[:, :c["Cq"]] = q[0, :c["Qtot"]].cpu().numpy()
        QC.compare(got, ref, f"{name} {what}")
    # rows behind the case's (the learned query the single-segment modules add) are moves: equal bits
    assert torch.equal(q_on[:, c["Qtot"]:].contiguous().view(torch.int32), q_off[:, c["Qtot"]:].contiguous().view(torch.int32))
    assert torch.equal(q_off[0], q_off[2])


def test_small_golden_fused_on_and_off(dev, monkeypatch):
    name = "model_multimodal_small"
    g = load(name)
    model = _load_generated(build(name), g, dev, model_seed(name), model_stats(name))
    assert model.fused_queries is True and model.perceiver.fused_queries is True
    ins = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]
    calls = _counting(monkeypatch)
    outs = {}
    for on in (True, False):
        model.fused_queries = on
        assert model.perceiver.fused_queries is on
        for cache in (True, False):
            model.cache_queries = cache
            model.clear_packed()
            before = calls["kernel"]
            with torch.inference_mode():
                out = model(ins[0], ins[1], n_chunks=2)
                again = model(ins[0], ins[1], n_chunks=2)
            # (two chunks are one group: one query array per forward, kept by the cache after the first)
            assert calls["kernel"] - before == ((1 if cache else 2) if on else 0), (on, cache, calls)
            for m in ("image", "audio", "label"):
                _close(out[m], g[f"out_{m}"], f"{name} {m}, fused_queries={on}, cache_queries={cache}", TOL)
                assert torch.equal(out[m], again[m]), (m, on, cache)
            outs[(on, cache)] = out
    for m in ("image", "audio", "label"):            # the kernel on: the cache changes nothing
        assert torch.equal(outs[(True, True)][m], outs[(True, False)][m]), m
    model.encode_once = False                    # every chunk its own forward: decoder_query inside PerceiverIO._forward
    model.fused_queries, model.cache_queries = True, True
    before = calls["kernel"]
    with torch.inference_mode():
        out = model(ins[0], ins[1], n_chunks=2)
    assert calls["kernel"] - before == 2
    for m in ("image", "audio", "label"):
        _close(out[m], g[f"out_{m}"], f"{name} {m}, fused_queries=True, encode_once=False", TOL)
