"""CPU: the definition of the decoder query builder (tests/query_cases.py) against the chain of torch ops it stands for --
PerceiverIO.decoder_query under set_backend("torch"): position, table and padding channels bit for bit, sine and cosine
against the float64 value of the fp32 phase -- which pins segment order, channel order and the phase arithmetic to what the
reference goldens already pin; the refusal table of pio_build_queries (no launch: a refused call returns before it touches
a device); every reason for PerceiverIO._fused_decoder_query to decline; the fused_queries switches."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import query_cases as QC  # noqa: E402


def make_segments(L, seg_fields, count=None):
    """ctypes array of pio_query_segment_t from the plain field dicts of query_cases (count: array length, >= 1)."""
    arr = (L.QuerySegment * max(count or len(seg_fields), len(seg_fields), 1))()
    for i, f in enumerate(seg_fields):
        for k, v in f.items():
            if k in ("axis", "dims"):
                for j, e in enumerate(v):
                    getattr(arr[i], k)[j] = e
            else:
                setattr(arr[i], k, v)
    return arr


def build_queries(L, seg_fields, y, args, stream=None):
    nseg = args.get("nseg", len(seg_fields))
    segs = make_segments(L, seg_fields, count=max(nseg, 1))
    return L.lib().pio_build_queries(segs, nseg, y, args["ldy"], args["Qtot"], args["Cq"], stream)


# ----------------------------------------------------------------------------------------------------
# modules that correspond to cases: the case's pad / table values go into the module's parameters, the module's own
# torch.linspace bands into the case
# ----------------------------------------------------------------------------------------------------
MODULE_CASES = {
    # case -> (query names in the case's segment order; sorted order = row order, as decoder_query places them)
    "mini_model_c0": ("audio", "image", "label"),
    "mini_model_c1": ("audio", "image", "label"),
    "sine_only": ("a",),       # (the module adds a learned query "b" behind it: decoder_query's chain needs two to concatenate)
    "no_pos": ("a",),
}


def make_perceiver(name):
    """PerceiverIO whose output queries are the case's (plus, for the single-segment cases, a learned query "b" of one
    row behind them)."""
    from perceiverio_pytorch_amd.output_queries import FourierQuery, TrainableQuery
    from perceiverio_pytorch_amd.perceiver import PerceiverIO
    if name.startswith("mini_model"):
        from test_models import build
        return build("model_multimodal_small").perceiver.eval()
    c = QC.CASES[name]
    g = c["segs"][0]
    queries = {"a": FourierQuery(output_index_dims=g["dims"], num_bands=g["K"], max_resolution=g["res"],
                                 sine_only=g["sine_only"], concat_pos=g["concat_pos"]),
               "b": TrainableQuery(output_index_dims=(1,), num_channels=g["width"] - 1)}
    return PerceiverIO(num_blocks=1, num_self_attends_per_block=1, num_latents=4, num_latent_channels=16, input_channels=8,
                       output_queries=queries, output_query_padding_channels=c["Cq"] - g["width"]).eval()


def module_bands(io, name):
    """{segment: [d, K]} the bands generate_fourier_features uses for the case's Fourier queries."""
    out = {}
    for i, (m, g) in enumerate(zip(MODULE_CASES[name], QC.CASES[name]["segs"])):
        if g["kind"] == QC.FOURIER:
            enc = io._output_queries[m]._position_encoding
            assert tuple(enc._index_dims) == g["dims"] and enc._num_bands == g["K"] and tuple(enc._max_resolution) == g["res"]
            out[i] = torch.stack([torch.linspace(1.0, r / 2, steps=g["K"]) for r in g["res"]]).numpy()
    return out


def load_case_parameters(io, name, data):
    with torch.no_grad():
        for m, g, d in zip(MODULE_CASES[name], QC.CASES[name]["segs"], data):
            if d["pad"] is not None:
                io.padding_embeddings[m].pos_embs.copy_(torch.from_numpy(d["pad"])[None])
            if g["kind"] == QC.TABLE:
                io._output_queries[m]._position_encoding.pos_embs.copy_(torch.from_numpy(d["table"]))
        for m in io._output_queries:
            if m not in MODULE_CASES[name]:
                torch.nn.init.normal_(io.padding_embeddings[m].pos_embs, std=0.02)
    return io


def module_case(name):
    io = make_perceiver(name)
    data = QC.gen(name, module_bands(io, name))
    return load_case_parameters(io, name, data), data


def module_points(name, dev="cpu"):
    pts = {m: None if g["kind"] == QC.TABLE else torch.from_numpy(g["points"]).to(dev)
           for m, g in zip(MODULE_CASES[name], QC.CASES[name]["segs"])}
    return pts


def stand_in(io, batch, dev="cpu"):
    """(x, sizes) as MultiModalPerceiver._chunk_queries passes them: the queries read batch size and device only."""
    sizes = {m: 2 for m in io._output_queries}
    return torch.zeros((batch, 2 * len(sizes), 1), device=dev), sizes


@pytest.mark.parametrize("name", sorted(MODULE_CASES))
def test_definition_equals_the_torch_chain(name):
    import perceiverio_pytorch_amd as P
    io, data = module_case(name)
    c = QC.CASES[name]
    ref = QC.reference(name, data)
    x, sizes = stand_in(io, 2)
    prev = P.get_backend()
    P.set_backend("torch")
    try:
        with torch.no_grad():
            q, qsizes = io.decoder_query(x, sizes, None, subsampled_points=module_points(name))
    finally:
        P.set_backend(prev)
    assert c["ldy"] >= c["Cq"] and q.shape[0] == 2 and q.shape[2] == c["Cq"] and q.shape[1] >= c["Qtot"]
    assert [qsizes[m] for m in MODULE_CASES[name]] == [g["M"] for g in c["segs"]] and list(qsizes) == list(io._output_queries)
    assert torch.equal(q[0], q[1])
    got = np.full(ref[0].shape, np.nan, dtype=np.float32)
    got[:, :c["Cq"]] = q[0, :c["Qtot"]].numpy()
    QC.compare(got, ref, f"{name}: the torch chain")


def test_case_table_covers_what_it_claims():
    c = QC.CASES
    assert all(g["M"] == 1 for g in c["one_row"]["segs"]) and len(c["one_row"]["segs"]) == 3
    assert c["one_row"]["segs"][2]["width"] == c["one_row"]["Cq"]                      # a zero-width pad
    for n in ("mini_model_c0", "mini_model_c1"):
        assert [(g["kind"], g["width"]) for g in c[n]["segs"]] == [(0, 385), (0, 195), (1, 1024)] and c[n]["Cq"] == 1026
    assert c["mini_model_c0"]["segs"][1]["points"][-1] + 1 == c["mini_model_c1"]["segs"][1]["points"][0]
    g = c["seams"]["segs"][0]
    assert g["dims"] == (3, 70) and g["M"] > 2 * QC.STRIP and g["points"][0] % 70 and len(set(g["points"] // 70)) == 3
    g = c["wrap"]["segs"][0]
    assert (g["points"] >= 15).any() and (g["points"] < 0).any() and len(set(g["points"].tolist())) < g["M"]
    assert c["sine_only"]["segs"][0]["sine_only"] and c["sine_only"]["segs"][0]["d"] == 3
    assert not c["no_pos"]["segs"][0]["concat_pos"] and c["no_pos"]["segs"][0]["d"] == 3
    assert c["start_only"]["segs"][0]["points"] is None and c["start_only"]["segs"][0]["start"] > 0
    data = QC.gen("big_phase")
    assert 48000 < QC.max_phase("big_phase", data) < 48300
    assert [g["row0"] for g in c["holes"]["segs"]] == [7, 2] and not QC.covered("holes").any(axis=1)[[0, 1, 5, 6, 10, 11]].any()
    widths = {(k["Cq"] % 2 == 1, k["Cq"] % 4 == 2, k["Cq"] % 4 == 0, k["ldy"] > k["Cq"]) for k in c.values()}
    for odd, two, four in ((True, False, False), (False, True, False), (False, False, True)):
        assert (odd, two, four, False) in widths and (odd, two, four, True) in widths
    for name in c:
        data = QC.gen(name)
        y, exact, kind = QC.reference(name, data)
        cov = QC.covered(name)
        assert np.isfinite(exact[cov]).all() and np.isnan(exact[~cov]).all() and np.isnan(y[~cov]).all(), name
        assert (np.abs(exact[kind != QC.MOVE]) <= 1).all()
        for g, d in zip(c[name]["segs"], data):
            for what in ("axis0", "axis1", "axis2", "bands", "table", "pad"):
                if d[what] is not None:              # every array is NaN outside what the formulas address
                    assert np.isfinite(d[what + "_full"]).sum() == d[what].size < d[what + "_full"].size, (name, what)
            if d["points"] is not None:
                assert d["points_full"].size == g["M"] + 2 * min(3, g["M"])


def test_struct_size_matches_the_c_layout():
    import subprocess
    import tempfile
    from perceiverio_pytorch_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "pio_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d\\n", ' \
           'sizeof(pio_query_segment_t), offsetof(pio_query_segment_t, start), offsetof(pio_query_segment_t, kind), ' \
           'offsetof(pio_query_segment_t, dims), offsetof(pio_query_segment_t, C), PIO_MAX_QUERY_SEGMENTS); return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    S = L.QuerySegment
    assert got == [ctypes.sizeof(S), S.start.offset, S.kind.offset, S.dims.offset, S.C.offset, L.PIO_MAX_QUERY_SEGMENTS]
    assert (L.PIO_QUERY_FOURIER, L.PIO_QUERY_TABLE, L.PIO_MAX_QUERY_SEGMENTS) == (QC.FOURIER, QC.TABLE, 4)


def made_up_pointers():
    ptrs = {"y": 0x100000}
    for i in range(len(QC.VALID_SEGS)):
        for k, f in enumerate(QC.POINTER_FIELDS):
            ptrs[(i, f)] = 0x200000 + 0x10000 * (8 * i + k)
    return ptrs


@pytest.mark.parametrize("what,changes,code", QC.REFUSALS, ids=[r[0] for r in QC.REFUSALS])
def test_refusal_table(what, changes, code):
    """Bad arguments are refused with the documented code before anything is launched: made-up (aligned, non-NULL)
    addresses are enough, and no device is needed."""
    from perceiverio_pytorch_amd import _lib as L
    segs, args, y = QC.refusal_fields(made_up_pointers(), changes)
    assert build_queries(L, segs, y, args) == code


def test_null_segment_table_is_refused():
    from perceiverio_pytorch_amd import _lib as L
    a = QC.VALID_ARGS
    assert L.lib().pio_build_queries(None, 2, 0x100000, a["ldy"], a["Qtot"], a["Cq"], None) == QC.PIO_E_ARG


# ----------------------------------------------------------------------------------------------------
# eligibility: every reason to decline.  On a machine without a GPU the inputs are CPU tensors, which is itself a reason;
# the others are checked with a stand-in that says it is on a GPU, the entry point replaced by one that raises.
# ----------------------------------------------------------------------------------------------------
class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on a GPU: lets the configuration checks run where no device exists."""
    @property
    def is_cuda(self):
        return True


def _declines(io, points, x=None):
    """_fused_decoder_query on a stand-in "CUDA" input: must return None (a configuration it accepted would go on to launch
    on host addresses -- so that the test fails loudly instead, the entry point is replaced by one that raises)."""
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd import runtime as R

    class _Lib:
        def pio_build_queries(self, *a):
            raise AssertionError("_fused_decoder_query accepted a configuration it must decline")
    if x is None:
        x = stand_in(io, 2)[0].as_subclass(_FakeCuda)
    real = L.lib, R.on_device, R.stream_ptr
    L.lib, R.on_device, R.stream_ptr = (lambda: _Lib()), (lambda d: contextlib.nullcontext()), (lambda d: 0)
    try:
        return io._fused_decoder_query(x, points) is None
    finally:
        L.lib, R.on_device, R.stream_ptr = real


def test_switches_exist():
    from perceiverio_pytorch_amd.perceiver import PerceiverIO
    from test_models import build
    assert PerceiverIO.fused_queries is True
    model = build("model_multimodal_small")
    assert model.fused_queries is True and model.perceiver.fused_queries is True
    model.fused_queries = False
    assert model.fused_queries is False and model.perceiver.fused_queries is False and PerceiverIO.fused_queries is True
    model.fused_queries = True
    assert model.perceiver.fused_queries is True
    assert model.cache_queries is True and model.query_cache_max_bytes == 8 << 30        # (the cache's defaults stay)


def test_fused_query_eligibility():
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd.output_queries import BasicQuery, FlowQuery, FourierQuery, TrainableQuery
    from perceiverio_pytorch_amd.perceiver import PerceiverIO
    from perceiverio_pytorch_amd.position_encoding import PosEncodingType, PositionEncodingProjector

    name = "mini_model_c0"

    def fresh():
        return module_case(name)[0], module_points(name)

    def tiny(queries, pad=2):
        return PerceiverIO(num_blocks=1, num_self_attends_per_block=1, num_latents=4, num_latent_channels=16,
                           input_channels=8, output_queries=queries, output_query_padding_channels=pad).eval()

    def fq(dims=(3, 5), k=2, **kw):
        return FourierQuery(output_index_dims=dims, num_bands=k, max_resolution=dims, **kw)

    # (the stand-in itself: an eligible configuration is NOT declined -- it reaches the entry point)
    io, pts = fresh()
    with pytest.raises(AssertionError, match="accepted"):
        _declines(io, pts)
    assert io._fused_decoder_query(stand_in(io, 2)[0], pts) is None                 # CPU tensors
    prev = P.get_backend()
    P.set_backend("torch")
    try:
        assert _declines(io, pts)                                                   # the torch backend
    finally:
        P.set_backend(prev)
    io.fused_queries = False
    assert _declines(io, pts)                                                       # the switch
    io.fused_queries = True
    assert _declines(io, dict(pts, image=None))                                     # a Fourier query over the full grid
    assert _declines(io, dict(pts, image=pts["image"].to(torch.int32)))             # points not int64
    assert _declines(io, dict(pts, image=pts["image"][None]))                       # points not 1-D
    assert _declines(io, dict(pts, image=pts["image"].tolist()))                    # points not a tensor
    assert _declines(io, dict(pts, label=torch.zeros(1, dtype=torch.int64)))        # points for a learned query
    with pytest.raises(AssertionError, match="accepted"):
        _declines(io, dict(pts, image=pts["image"][::2]))                           # (strided points: taken, copied)
    io.padding_embeddings["audio"].double()
    assert _declines(io, pts)                                                       # a padding embedding that is not fp32
    io, pts = fresh()
    io._output_queries["label"]._position_encoding.double()
    assert _declines(io, pts)                                                       # a learned query that is not fp32
    io, pts = fresh()
    enc = io._output_queries["audio"]._position_encoding
    io._output_queries["audio"]._position_encoding = PositionEncodingProjector(enc.n_output_channels(),
                                                                               enc.n_output_channels(), enc)
    assert _declines(io, pts)                                                       # a projected Fourier encoding

    p15 = torch.arange(15)
    with pytest.raises(AssertionError, match="accepted"):
        _declines(tiny({"a": fq(), "b": TrainableQuery(output_index_dims=(1,), num_channels=4)}), {"a": p15})
    with pytest.raises(AssertionError, match="accepted"):
        _declines(tiny({"a": fq(), "b": fq((4,), 3, sine_only=True)}), {"a": p15, "b": torch.arange(4)})
    assert _declines(tiny({"a": fq()}), {"a": p15})                                 # a single output query
    assert _declines(tiny({"a": TrainableQuery(output_index_dims=(2,), num_channels=4),
                           "b": TrainableQuery(output_index_dims=(1,), num_channels=6)}), {})   # no Fourier query
    assert _declines(tiny({"a": fq((2, 2, 2, 2), 1), "b": fq()}), {"a": p15, "b": p15})          # d = 4
    assert _declines(tiny({"a": fq((3, 5), 124), "b": fq()}), {"a": p15, "b": p15})  # feature rows beyond the kernel's LDS
    with pytest.raises(AssertionError, match="accepted"):
        _declines(tiny({"a": fq((3, 5), 123), "b": fq()}), {"a": p15, "b": p15})
    assert _declines(tiny({"a": fq(), "b": fq(concat_preprocessed_input=True, preprocessed_input_channels=8)}),
                     {"a": p15, "b": p15})                                          # a query that reads the inputs
    assert _declines(tiny({"a": fq(), "b": FlowQuery(8, (2, 2))}), {"a": p15})      # FlowQuery
    five = {f"q{i}": fq() for i in range(5)}
    assert _declines(tiny(five), {m: p15 for m in five})                            # more queries than segments
    assert isinstance(fq(), BasicQuery) and PosEncodingType.FOURIER is not None
