"""GPU: the output heads -- pio_project_heads through the raw C-ABI on every case of tests/heads_cases.py against the
float64 definition, row independence at the raw entry, the refusal table, MultiModalPerceiver.fused_heads on the small
golden, one full-size group, and graph capture.

Bound (derived, not measured): |y - ref| <= gamma_(K+1) (sum_k |w_k x_k| + |bias|) -- heads_cases.bound.

Memory safety by construction: every y sits between 4 KiB guard bands and is NaN before the call; y_rs gaps and the rows
around a segment's range must still be NaN afterwards; x, w and bias are surrounded by NaN, rows of x that no segment covers
are NaN, and every output must be finite (except the one row with a planted NaN)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_cases as HC  # noqa: E402
from test_flow_front_gpu import GuardedOut  # noqa: E402
from test_heads_host import project_heads  # noqa: E402
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
    """(inputs, per-segment (definition, error scale)) of a case, computed once and shared (read-only) by the tests."""
    if name not in _REF:
        data = HC.gen(name)
        _REF[name] = (data, HC.reference(name, data))
    return _REF[name]


def _bits(t):
    return t.contiguous().view(torch.int32)


def launch(dev, name, data):
    """One call of the raw entry on the case's NaN-surrounded inputs; returns the guarded outputs, one per segment, each
    [B * y_rows, y_rs]."""
    from perceiverio_pytorch_amd import _lib as L
    c = HC.CASES[name]
    held = {"x": torch.from_numpy(data["x_full"]).to(dev)}
    ys = []
    for i, (g, d) in enumerate(zip(c["segs"], data["segs"])):
        held[(i, "w")] = torch.from_numpy(d["w_full"]).to(dev)
        if d["bias"] is not None:
            held[(i, "bias")] = torch.from_numpy(d["bias_full"]).to(dev)
        ys.append(GuardedOut(dev, c["B"] * HC.y_rows(g), g["y_rs"]))
        held[(i, "y")] = ys[-1].t
    segs, args = HC.call_fields(name, data, lambda what: held[what].data_ptr())
    L.check(project_heads(L, segs, args, torch.cuda.current_stream().cuda_stream), f"pio_project_heads[{name}]")
    for y in ys:
        y.check(name)
    return ys


def written(c, g, y):
    """(the [B, rows, n_out] block a segment's call writes, the whole [B, y_rows, y_rs] buffer, bool mask of the block)."""
    full = y.t.reshape(c["B"], HC.y_rows(g), g["y_rs"])
    mask = torch.zeros(full.shape, dtype=torch.bool, device=full.device)
    mask[:, HC.Y_FRONT:HC.Y_FRONT + g["rows"], :g["n_out"]] = True
    return full[:, HC.Y_FRONT:HC.Y_FRONT + g["rows"], :g["n_out"]], full, mask


@pytest.mark.parametrize("name", sorted(HC.CASES))
def test_raw_entry_against_the_definition(dev, name):
    c = HC.CASES[name]
    data, refs = case_data(name)
    ys, ys2 = launch(dev, name, data), launch(dev, name, data)
    for i, (g, (ref, mag)) in enumerate(zip(c["segs"], refs)):
        got, full, mask = written(c, g, ys[i])
        assert torch.isnan(full[~mask]).all(), f"{name}[{i}]: a y_rs gap or a row outside the segment's range was written"
        HC.assert_within_bound(got.cpu().numpy(), ref, mag, c["K"], f"{name}[{i}]")
        assert torch.equal(_bits(ys[i].t), _bits(ys2[i].t)), f"{name}[{i}]: two launches differ"
    if name in HC.PLANTED:
        b, r, _ = HC.PLANTED[name]
        got = written(c, c["segs"][0], ys[0])[0]
        nan = torch.isnan(got).all(dim=2)
        assert int(nan.sum()) == 1 and bool(nan[b, r - c["segs"][0]["row0"]]) and int(torch.isnan(got).sum()) == got.shape[2]


def test_rows_do_not_depend_on_where_they_run(dev):
    """The same 64 rows as ONE segment at B = 1, and split over two segments at B = 2 (other row0, other strides, another
    segment of another width between them, the halves in other strips and samples): equal bits."""
    from perceiverio_pytorch_amd import _lib as L
    K, n = 512, 3
    gen = torch.Generator().manual_seed(11)
    rows = torch.randn(64, K, generator=gen).to(dev)
    w = (torch.randn(n, K, generator=gen) / K ** 0.5).to(dev)
    bias = torch.randn(n, generator=gen).to(dev)
    w2 = torch.randn(16, K, generator=gen).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    ya = GuardedOut(dev, 64, n)
    L.check(project_heads(L, [dict(row0=0, rows=64, n_out=n, w=w.data_ptr(), ldw=K, bias=bias.data_ptr(), y=ya.t.data_ptr(),
                                   y_sb=0, y_rs=n)],
                          dict(x=rows.data_ptr(), x_sb=0, ldx=K, B=1, Q=64, K=K), stream), "one segment")
    ya.check("one segment")
    # B = 2, Q = 200, ldx = K + 8: sample 0 holds rows 0 .. 31 at [101, 133), sample 1 rows 32 .. 63 at [101, 133); a second
    # copy of each half at [7, 39) in the OTHER sample's order; a 16-column segment over [40, 100) in between
    Q, ldx = 200, K + 8
    x = torch.randn(2, Q, ldx, generator=gen).to(dev)
    x[0, 101:133, :K], x[1, 101:133, :K] = rows[:32], rows[32:]
    x[0, 7:39, :K], x[1, 7:39, :K] = rows[32:], rows[:32]
    yb, yc, yd = GuardedOut(dev, 2 * 40, 5), GuardedOut(dev, 2 * 32, n), GuardedOut(dev, 2 * 60, 16)
    segs = [dict(row0=101, rows=32, n_out=n, w=w.data_ptr(), ldw=K, bias=bias.data_ptr(), y=yb.t.data_ptr() + 4 * 5 * 3,
                 y_sb=40 * 5, y_rs=5),
            dict(row0=40, rows=60, n_out=16, w=w2.data_ptr(), ldw=K, bias=None, y=yd.t.data_ptr(), y_sb=60 * 16, y_rs=16),
            dict(row0=7, rows=32, n_out=n, w=w.data_ptr(), ldw=K, bias=bias.data_ptr(), y=yc.t.data_ptr(), y_sb=32 * n, y_rs=n)]
    L.check(project_heads(L, segs, dict(x=x.data_ptr(), x_sb=Q * ldx, ldx=ldx, B=2, Q=Q, K=K), stream), "two segments")
    for y in (yb, yc, yd):
        y.check("two segments")
    one = ya.t
    split_b = yb.t.reshape(2, 40, 5)[:, 3:35, :n].reshape(64, n)                    # sample 0: rows 0 .. 31, sample 1: 32 .. 63
    split_c = yc.t.reshape(2, 32, n)
    assert bool(torch.isfinite(one).all())
    assert torch.equal(_bits(one), _bits(split_b))
    assert torch.equal(_bits(one[32:]), _bits(split_c[0])) and torch.equal(_bits(one[:32]), _bits(split_c[1]))


def _refusal_buffers(dev):
    a = HC.VALID_ARGS
    bufs = {"x": torch.randn(2 * a["x_sb"] + 64, device=dev)}
    ys = {}
    for i, g in enumerate(HC.VALID_SEGS):
        bufs[(i, "w")] = torch.randn(g["n_out"] * g["ldw"] + 64, device=dev)
        bufs[(i, "bias")] = torch.randn(32, device=dev)
        ys[i] = GuardedOut(dev, 2 * g["y_sb"] // g["y_rs"] + 2, g["y_rs"])          # (+2 rows: room for a moved pointer)
        bufs[(i, "y")] = ys[i].t
    return ys, {k: v.data_ptr() for k, v in bufs.items()}, bufs


def test_the_valid_call_of_the_refusal_table_runs(dev):
    from perceiverio_pytorch_amd import _lib as L
    ys, ptrs, keep = _refusal_buffers(dev)
    segs, args = HC.refusal_fields(ptrs, {})
    assert project_heads(L, segs, args, torch.cuda.current_stream().cuda_stream) == HC.PIO_OK
    for i, g in enumerate(HC.VALID_SEGS):
        ys[i].check("valid call")
        out = ys[i].t.reshape(-1)[:2 * g["y_sb"]].reshape(2, -1, g["y_rs"])
        assert bool(torch.isfinite(out[:, :g["rows"], :g["n_out"]]).all())
        assert int(torch.isfinite(ys[i].t).sum()) == 2 * g["rows"] * g["n_out"]


@pytest.mark.parametrize("what,changes,code", HC.REFUSALS, ids=[r[0] for r in HC.REFUSALS])
def test_refusals_launch_nothing(dev, what, changes, code):
    from perceiverio_pytorch_amd import _lib as L
    ys, ptrs, keep = _refusal_buffers(dev)
    segs, args = HC.refusal_fields(ptrs, changes)
    assert project_heads(L, segs, args, torch.cuda.current_stream().cuda_stream) == code
    for y in ys.values():
        y.check(what)
        assert torch.isnan(y.t).all(), f"{what}: a refused call wrote to y"


# ----------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------
def _counting_cat(monkeypatch):
    """torch.cat as models.py and fused_io.py see it: the shapes of every call's first piece (the stand-in of
    tests/test_mm_front_gpu.py, applied to `models` and `fused_io`)."""
    from perceiverio_pytorch_amd import fused_io as FIO
    from perceiverio_pytorch_amd import models as M
    calls = []

    class _Torch:
        def __getattr__(self, k):
            return getattr(torch, k)

        def cat(self, tensors, *a, **kw):
            calls.append(tuple(tensors[0].shape))
            return torch.cat(tensors, *a, **kw)
    monkeypatch.setattr(M, "torch", _Torch())
    monkeypatch.setattr(FIO, "torch", M.torch)
    return calls


@pytest.fixture(scope="module")
def small(dev):
    name = "model_multimodal_small"
    g = load(name)
    model = _load_generated(build(name), g, dev, model_seed(name), model_stats(name))
    ins = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]
    return name, g, model, ins


def test_small_golden_fused_heads_on_and_off(dev, small, monkeypatch):
    name, g, model, ins = small
    assert model.fused_heads is True and model.encode_once is True
    calls = _counting_cat(monkeypatch)
    outs = {}
    for on in (True, False):
        model.fused_heads = on
        del calls[:]
        with torch.inference_mode():
            out = model(ins[0], ins[1], n_chunks=2)
            again = model(ins[0], ins[1], n_chunks=2)
        ncat = len(calls) // 2
        for m in ("image", "audio", "label"):
            _close(out[m], g[f"out_{m}"], f"{name} {m}, fused_heads={on}", TOL)
            assert torch.equal(out[m], again[m]), f"{m}, fused_heads={on}: two forwards differ"
        # on: models.py concatenates the label estimates only ([B, 1, classes] pieces); off: image and audio as well
        assert (ncat == 1 and all(len(s) == 3 and s[1] == 1 for s in calls)) if on else ncat == 3, (on, calls)
        outs[on] = out
    model.fused_heads = True
    for m in ("image", "audio", "label"):
        a, b = outs[True][m], outs[False][m]
        assert a.shape == b.shape and a.dtype == b.dtype and a.stride() == b.stride(), m
        print(f"{name} {m}: max |fused - chain| = {float((a - b).abs().max()):.3e}")
    assert torch.equal(outs[True]["label"], outs[False]["label"])
    assert not outs[True]["image"].is_contiguous()                # (the moveaxis view of [B, T, H, W, C], as the chain's)


def test_small_golden_chunk_loops_agree_bit_for_bit(dev, small):
    """With one chunk per decoder call, the encode-once loop (heads written in place) and the reference's recompute loop
    (heads through PerceiverIO._forward, pieces concatenated) are the same bits -- and so is the default grouping for the
    heads' share: the same decoder rows give the same outputs wherever they sit."""
    name, g, model, ins = small
    assert model.fused_heads is True
    try:
        with torch.inference_mode():
            model.decode_chunks_per_call = 1
            out1 = model(ins[0], ins[1], n_chunks=2)
            model.encode_once = False
            out2 = model(ins[0], ins[1], n_chunks=2)
    finally:
        model.encode_once, model.decode_chunks_per_call = True, 16
    for m in ("image", "audio", "label"):
        assert torch.equal(out1[m], out2[m]), m


def test_heads_call_on_the_small_shapes(dev, small):
    """PerceiverIO._project_heads on a seeded decoder output of the small model's shape, B = 2: into= views and fresh
    arrays give the same bits, both within the bound of the definition; the call captures into a graph on one stream and
    the replay reproduces the eager bits on new data."""
    name, g, model, ins = small
    P = model.perceiver
    sizes = {"audio": 4, "image": 512, "label": 1}
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 517, 512, generator=gen).to(dev)
    x2 = torch.randn(2, 517, 512, generator=gen).to(dev)
    posts = P._output_postprocessors
    with torch.inference_mode(), model_policy(model):
        fresh = P._project_heads(x, sizes)
        assert fresh is not None and fresh["image"].shape == (2, 512, 3) and fresh["audio"].shape == (2, 64)
        big = {"image": torch.full((2, 600, 3), float("nan"), device=dev), "audio": torch.full((2, 9, 16), float("nan"), device=dev)}
        into = {"image": big["image"][:, 40:552], "audio": big["audio"][:, 5:9]}
        placed = P._project_heads(x, sizes, into=into)
        assert placed["image"].data_ptr() == into["image"].data_ptr() and placed["audio"].shape == (2, 4, 16)
        assert torch.equal(_bits(placed["image"]), _bits(fresh["image"]))
        assert torch.equal(_bits(placed["audio"].reshape(2, 64)), _bits(fresh["audio"]))
        assert torch.equal(placed["label"], fresh["label"])
        assert bool(torch.isnan(big["image"][:, :40]).all()) and bool(torch.isnan(big["image"][:, 552:]).all())
        assert bool(torch.isnan(big["audio"][:, :5]).all())
        for m, lin, sl in (("audio", posts["audio"].linear, slice(0, 4)), ("image", posts["image"].projection, slice(4, 516))):
            ref, mag = HC.definition(x[:, sl].cpu().numpy(), lin.weight.detach().cpu().numpy(), lin.bias.detach().cpu().numpy())
            HC.assert_within_bound(fresh[m].cpu().numpy(), ref, mag, 512, f"_project_heads, {m}")
        # graph capture on the current stream (the label head's packed weights exist since the eager calls above)
        xin = x.clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = P._project_heads(xin, sizes, into=into)
        xin.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        eager = P._project_heads(x2, sizes)
        assert torch.equal(_bits(captured["image"]), _bits(eager["image"]))
        assert torch.equal(_bits(captured["audio"].reshape(2, 64)), _bits(eager["audio"]))
        assert not torch.equal(_bits(eager["image"]), _bits(fresh["image"]))


def model_policy(model):
    from perceiverio_pytorch_amd.models import split_policy
    from perceiverio_pytorch_amd.runtime import precision
    return precision(split_policy(model.precision_policy)[1])


def test_one_full_size_group(dev):
    """One decoder call of the default model at B = 1: a seeded [1, 100 593, 512] array (240 audio + 100 352 image + 1 label
    rows) through _project_heads with the default model's heads.  The first and last 64 rows of each modality and 256
    seeded rows against the definition within the bound; everything else finite."""
    from perceiverio_pytorch_amd.io_processors import (AudioPostprocessor, ClassificationPostprocessor,
                                                       ProjectionPostprocessor)
    from test_heads_host import tiny
    torch.manual_seed(7)
    posts = {"audio": AudioPostprocessor(in_channels=512, samples_per_patch=16),
             "image": ProjectionPostprocessor(num_inputs=512, num_outputs=3),
             "label": ClassificationPostprocessor(num_input_channels=512, num_classes=700)}
    io = tiny(posts, k=512).to(dev)
    with torch.no_grad():
        for p in (posts["audio"].linear.bias, posts["image"].projection.bias):
            p.copy_(torch.randn_like(p))
    sizes = {"audio": 240, "image": 100352, "label": 1}
    x = torch.randn(1, 100593, 512, device=dev, generator=torch.Generator(device=dev).manual_seed(19))
    with torch.inference_mode():
        out = io._project_heads(x, sizes)
    assert out is not None and out["image"].shape == (1, 100352, 3) and out["audio"].shape == (1, 240 * 16)
    assert out["label"].shape == (1, 700)
    assert bool(torch.isfinite(out["image"]).all()) and bool(torch.isfinite(out["audio"]).all())
    rng = np.random.default_rng(23)
    for m, lin, row0, rows, got in (("audio", posts["audio"].linear, 0, 240, out["audio"].reshape(1, 240, 16)),
                                    ("image", posts["image"].projection, 240, 100352, out["image"])):
        pick = np.unique(np.concatenate([np.arange(min(64, rows)), np.arange(max(rows - 64, 0), rows),
                                         rng.integers(0, rows, size=256)]))
        idx = torch.from_numpy(pick).to(dev)
        ref, mag = HC.definition(x[0, row0 + idx].cpu().numpy(), lin.weight.detach().cpu().numpy(),
                                 lin.bias.detach().cpu().numpy())
        HC.assert_within_bound(got[0, idx].cpu().numpy(), ref, mag, 512, f"full-size group, {m}")
