"""CPU: the definition of the multimodal front end (tests/mm_front_cases.py) against the chain of copies it stands for --
MultimodalPreprocessor.forward under set_backend("torch"), bit for bit, which pins segment order, channel order and the
masked expression to what the reference goldens already pin; the refusal table of pio_assemble_tokens (no launch: a
refused call returns before it touches a device); and every reason for MultimodalPreprocessor._assemble to decline."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mm_front_cases as MC  # noqa: E402


def make_segments(L, seg_fields, count=None):
    """ctypes array of pio_token_segment_t from the plain field dicts of mm_front_cases (count: array length, >= 1)."""
    arr = (L.TokenSegment * max(count or len(seg_fields), len(seg_fields), 1))()
    for i, f in enumerate(seg_fields):
        for k, v in f.items():
            setattr(arr[i], k, v)
    return arr


def assemble(L, seg_fields, y, args, stream=None):
    nseg = args.get("nseg", len(seg_fields))
    segs = make_segments(L, seg_fields, count=max(nseg, 1))
    return L.lib().pio_assemble_tokens(segs, nseg, y, args["ldy"], args["sYb"], args["B"], args["Mtot"], args["Cc"], stream)


# ----------------------------------------------------------------------------------------------------
# module configurations that correspond to cases: the case's pad / token / (trainable) table values go into the module's
# parameters, the case's clean inputs into forward
# ----------------------------------------------------------------------------------------------------
MODULE_CASES = {
    # case -> modality names in the case's segment order (sorted order = row order, as MultimodalPreprocessor places them)
    "mini_model": ("audio", "image", "label"),
    "s2d_small": ("image",),
    "masked": ("audio", "label"),
}


def make_module(name):
    """(MultimodalPreprocessor, Fourier tables {segment: [M, C2]} to generate the case with).  Trainable position tables,
    padding embeddings and mask tokens are set by load_case_parameters."""
    from perceiverio_pytorch_amd.io_processors import AudioPreprocessor, ImagePreprocessor, OneHotPreprocessor
    from perceiverio_pytorch_amd.perceiver import MultimodalPreprocessor
    from perceiverio_pytorch_amd.position_encoding import PosEncodingType
    if name == "mini_model":
        preps = {
            "audio": AudioPreprocessor(samples_per_batch=64, samples_per_patch=16,
                                       position_encoding_type=PosEncodingType.FOURIER,
                                       fourier_position_encoding_kwargs=dict(num_bands=192, max_resolution=(64,),
                                                                             sine_only=False, concat_pos=True)),
            "image": ImagePreprocessor(img_size=(16, 16), input_channels=3, num_frames=2, prep_type="patches",
                                       spatial_downsample=4, temporal_downsample=1,
                                       position_encoding_type=PosEncodingType.FOURIER,
                                       fourier_position_encoding_kwargs=dict(num_bands=32, max_resolution=(2, 4, 4),
                                                                             sine_only=False, concat_pos=True)),
            "label": OneHotPreprocessor(input_channels=10)}
        mm = MultimodalPreprocessor(torch.nn.ModuleDict(preps), mask_probs={"audio": 0.0, "image": 0.0, "label": 1.0},
                                    min_padding_size=4)
        tables = {i: preps[m]._positional_encoding(batch_size=1)[0].numpy() for i, m in enumerate(("audio", "image"))}
        return mm, tables
    if name == "s2d_small":
        preps = {"image": ImagePreprocessor(img_size=(8, 8), input_channels=3, num_frames=2, prep_type="patches",
                                            spatial_downsample=4, temporal_downsample=1,
                                            position_encoding_type=PosEncodingType.TRAINABLE,
                                            trainable_position_encoding_kwargs=dict(num_channels=7))}
        return MultimodalPreprocessor(torch.nn.ModuleDict(preps), mask_probs=None, min_padding_size=5), None
    assert name == "masked"
    preps = {"audio": AudioPreprocessor(samples_per_batch=64, samples_per_patch=16,
                                        position_encoding_type=PosEncodingType.TRAINABLE,
                                        trainable_position_encoding_kwargs=dict(num_channels=9)),
             "label": OneHotPreprocessor(input_channels=10)}
    return MultimodalPreprocessor(torch.nn.ModuleDict(preps), mask_probs={"audio": 0.0, "label": 1.0},
                                  min_padding_size=2), None


def load_case_parameters(name, mm, data):
    """Non-zero padding embeddings, mask tokens and trainable position tables: the case's values."""
    from perceiverio_pytorch_amd.position_encoding import TrainablePositionEncoding
    with torch.no_grad():
        for m, d in zip(MODULE_CASES[name], data):
            if d["pad"] is not None:
                mm.padding_embeddings[m].pos_embs.copy_(torch.from_numpy(d["pad"])[None])
            if mm._mask_probs is not None:
                tok = d["token"] if d["token"] is not None else 0.02 * np.random.default_rng(5).standard_normal(
                    MC.CASES[name]["Cc"]).astype(np.float32)      # (a token of an unmasked modality: present, never read)
                mm.mask_tokens[m].pos_embs.copy_(torch.from_numpy(tok)[None])
            pe = getattr(mm._preprocessors[m], "_positional_encoding", None)
            if isinstance(pe, TrainablePositionEncoding):
                pe.pos_embs.copy_(torch.from_numpy(d["table"]))
    return mm.eval()


def module_inputs(name, data, dev="cpu"):
    ins = {}
    for m, g, d in zip(MODULE_CASES[name], MC.CASES[name]["segs"], data):
        x = torch.from_numpy(d["feat"])
        if m == "audio":
            x = x.reshape(x.shape[0], -1, 1)       # the waveform [B, samples, 1]
        elif m == "label":
            x = x[:, 0, :]                         # [B, classes]
        ins[m] = x.to(dev)
    return ins


def module_case(name):
    mm, tables = make_module(name)
    data = MC.gen(name, tables)
    return load_case_parameters(name, mm, data), data


def assert_same_bits(got, ref, what, masked=None):
    """got, ref float32 arrays of one shape: equal as int32 bits; in masked rows (bool over axis -2) NaN positions must
    agree and every other element must be bit-equal (the sign / payload of a produced NaN is the platform's)."""
    got, ref = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    same = got.view(np.int32) == ref.view(np.int32)
    if masked is not None:
        both_nan = np.isnan(got) & np.isnan(ref)
        both_nan[..., ~masked, :] = False
        same |= both_nan
    if not same.all():
        i = tuple(int(v[0]) for v in np.nonzero(~same))
        raise AssertionError(f"{what}: {int((~same).sum())} elements differ, first at {i}: got {got[i]!r} ref {ref[i]!r}")


@pytest.mark.parametrize("name", sorted(MODULE_CASES))
def test_definition_equals_the_torch_chain(name):
    import perceiverio_pytorch_amd as P
    mm, data = module_case(name)
    c = MC.CASES[name]
    ref = MC.reference(name, data)
    prev = P.get_backend()
    P.set_backend("torch")
    try:
        with torch.no_grad():
            x, sizes, without_pos = mm(module_inputs(name, data))
    finally:
        P.set_backend(prev)
    assert x.shape == (c["B"], c["Mtot"], c["Cc"]) and c["ldy"] == c["Cc"]
    assert sizes == {m: g["M"] for m, g in zip(MODULE_CASES[name], c["segs"])}
    assert_same_bits(x.numpy(), ref, name, masked=MC.masked_rows(name))
    if name == "masked":
        # inf and NaN in the masked modality's x come out as NaN at exactly those channels, the token everywhere else
        g, d = c["segs"][1], data[1]
        row = x.numpy()[:, g["row0"]]
        expect_nan = np.zeros_like(row, dtype=bool)
        for (b, m, j, v) in MC.PLANTED[name][1]:
            expect_nan[b, j] = True
        assert np.array_equal(np.isnan(row), expect_nan)
        assert np.array_equal(row[~expect_nan], np.broadcast_to(d["token"], row.shape)[~expect_nan])
    for m, g, d in zip(MODULE_CASES[name], c["segs"], data):
        feats = d["feat"] if g["kind"] == MC.ROWS else ref[:, g["row0"]:g["row0"] + g["M"], :g["C1"]]
        assert_same_bits(without_pos[m].numpy(), feats, f"{name} without_pos[{m}]", masked=np.ones(g["M"], dtype=bool))


def test_case_table_covers_what_it_claims():
    c = MC.CASES
    assert all(g["M"] == 1 for g in c["one_token"]["segs"]) and c["one_token"]["Cc"] % 2 == 1
    g = c["s2d_small"]["segs"][0]
    assert (g["M"], g["C1"], g["C2"], c["s2d_small"]["Cc"]) == (8, 48, 7, 60)
    g = c["s2d_seams"]["segs"][0]
    assert g["s"] == 1 and g["W"] > 2 * MC.STRIP and g["W"] % MC.STRIP and g["M"] > MC.STRIP
    assert c["s2d_c1_s2"]["segs"][0]["four_d"] and c["s2d_c1_s2"]["Cc"] % 4
    assert c["rows_strided"]["segs"][0]["sm"] == 24 and c["rows_strided"]["segs"][0]["M"] > MC.STRIP
    g = c["no_pos_no_pad"]["segs"][0]
    assert g["C2"] == 0 and g["C1"] == c["no_pos_no_pad"]["Cc"]
    assert c["dword_path"]["ldy"] == 405 and c["dword_path_ld412"]["ldy"] == 412
    assert [(g["C1"], g["C2"]) for g in c["mini_model"]["segs"]] == [(16, 385), (48, 195), (10, 0)]
    assert not MC.covered("holes").all(axis=1)[[0, 1, 5, 6, 11]].any()
    assert {k["Cc"] % 4 == 0 for k in c.values()} == {True, False}
    for name in c:
        data = MC.gen(name)
        ref = MC.reference(name, data)
        cov = np.broadcast_to(MC.covered(name), ref.shape)
        unmasked = cov & ~MC.masked_rows(name)[None, :, None]
        assert np.isfinite(ref[unmasked]).all(), name           # the definition reads no NaN surroundings
        assert np.isnan(ref[~cov]).all(), name
        for g, d in zip(c[name]["segs"], data):
            # every array is NaN outside what the formulas address
            n_addr = c[name]["B"] * g["M"] * g["C1"]
            assert 0 < (~np.isnan(d["feat_full"])).sum() <= n_addr < d["feat_full"].size, name
            if d["table_full"] is not None:
                assert np.isfinite(d["table_full"]).sum() == g["M"] * g["C2"] < d["table_full"].size


def test_struct_size_matches_the_c_layout():
    import subprocess
    import tempfile
    from perceiverio_pytorch_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "pio_hip.h"\nint main(void){printf("%zu %zu %zu %d\\n", ' \
           'sizeof(pio_token_segment_t), offsetof(pio_token_segment_t, kind), offsetof(pio_token_segment_t, s), ' \
           'PIO_MAX_TOKEN_SEGMENTS); return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(L.TokenSegment), L.TokenSegment.kind.offset, L.TokenSegment.s.offset,
                   L.PIO_MAX_TOKEN_SEGMENTS]


@pytest.mark.parametrize("what,changes,code", MC.REFUSALS, ids=[r[0] for r in MC.REFUSALS])
def test_refusal_table(what, changes, code):
    """Bad arguments are refused with the documented code before anything is launched: made-up (aligned, non-NULL)
    addresses are enough, and no device is needed."""
    from perceiverio_pytorch_amd import _lib as L
    ptrs = {"y": 0x100000}
    for i, fields in enumerate(MC.VALID_PTRS):
        for k, f in enumerate(fields):
            ptrs[(i, f)] = 0x200000 + 0x10000 * (4 * i + k)
    segs, args, y = MC.refusal_fields(ptrs, changes)
    assert assemble(L, segs, y, args) == code


def test_null_segment_table_is_refused():
    from perceiverio_pytorch_amd import _lib as L
    a = MC.VALID_ARGS
    assert L.lib().pio_assemble_tokens(None, 2, 0x100000, a["ldy"], a["sYb"], a["B"], a["Mtot"], a["Cc"], None) == MC.PIO_E_ARG


# ----------------------------------------------------------------------------------------------------
# eligibility: every reason to decline.  On a machine without a GPU the inputs are CPU tensors, which is itself a reason;
# the others are checked with `meta`-free stand-ins by patching what _assemble inspects first.
# ----------------------------------------------------------------------------------------------------
class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on a GPU: lets _assemble's configuration checks run where no device exists.  Only used
    for configurations that decline BEFORE any pointer is taken or anything is launched."""
    @property
    def is_cuda(self):
        return True


def _as_cuda(ins):
    return {m: x.as_subclass(_FakeCuda) for m, x in ins.items()}


def test_assemble_declines_cpu_tensors_and_the_torch_backend():
    import perceiverio_pytorch_amd as P
    mm, data = module_case("mini_model")
    ins = module_inputs("mini_model", data)
    assert mm.fused_assembly is True
    assert mm._assemble(ins, None) is None                          # CPU tensors
    prev = P.get_backend()
    P.set_backend("torch")
    try:
        assert mm._assemble(ins, None) is None                      # the torch backend
    finally:
        P.set_backend(prev)
    mm.fused_assembly = False
    assert mm._assemble(ins, None) is None                          # the switch
    mm.fused_assembly = True
    assert mm._assemble(ins, torch.zeros(2, 37, 3)) is None         # caller-supplied positions


def _declines(mm, ins):
    """_assemble on stand-in "CUDA" tensors: must return None (a configuration it accepted would go on to launch on host
    addresses -- so that the test fails loudly instead, the entry point is replaced by one that raises)."""
    from perceiverio_pytorch_amd import _lib as L

    class _Lib:
        def pio_assemble_tokens(self, *a):
            raise AssertionError("_assemble accepted a configuration it must decline")
    import contextlib
    from perceiverio_pytorch_amd import runtime as R
    real = L.lib, R.on_device, R.stream_ptr
    L.lib, R.on_device, R.stream_ptr = (lambda: _Lib()), (lambda d: contextlib.nullcontext()), (lambda d: 0)
    try:
        return mm._assemble(_as_cuda(ins), None) is None
    finally:
        L.lib, R.on_device, R.stream_ptr = real


def test_assemble_eligibility_reasons():
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd.io_processors import EmbeddingPreprocessor, ImagePreprocessor
    from perceiverio_pytorch_amd.perceiver import MultimodalPreprocessor
    from perceiverio_pytorch_amd.position_encoding import PosEncodingType

    def fresh():
        mm, data = module_case("mini_model")
        return mm, module_inputs("mini_model", data)

    # (the stand-in itself: an eligible configuration is NOT declined -- it reaches the entry point)
    mm, ins = fresh()
    with pytest.raises(AssertionError, match="accepted"):
        _declines(mm, ins)

    mm, ins = fresh()
    assert _declines(mm, dict(ins, audio=ins["audio"].double()))                    # not fp32
    assert _declines(mm, dict(ins, image=ins["image"].half()))
    mm._mask_probs = {"audio": 0.0, "image": 0.5, "label": 1.0}
    assert _declines(mm, ins)                                                       # random masking
    mm._mask_probs = {"audio": 0.0, "image": 1.0, "label": 1.0}
    assert _declines(mm, ins)                                                       # a masked space-to-depth segment
    mm._mask_probs = {"audio": 1.0, "image": 0.0, "label": 0.0}
    with pytest.raises(AssertionError, match="accepted"):
        _declines(mm, ins)                                                          # (masked ROWS: taken)

    fourier = dict(position_encoding_type=PosEncodingType.FOURIER,
                   fourier_position_encoding_kwargs=dict(num_bands=4, max_resolution=(16, 16), sine_only=False,
                                                         concat_pos=True))
    x4 = torch.randn(2, 3, 16, 16)

    def image_only(**kw):
        args = dict(img_size=(16, 16), input_channels=3, prep_type="patches", spatial_downsample=4, temporal_downsample=1)
        args.update(fourier)
        args.update(kw)
        return MultimodalPreprocessor(torch.nn.ModuleDict({"image": ImagePreprocessor(**args)}), min_padding_size=2).eval()
    with pytest.raises(AssertionError, match="accepted"):
        _declines(image_only(), {"image": x4})                                      # (4-D patches: taken)
    with pytest.raises(AssertionError, match="accepted"):
        _declines(image_only(prep_type="pixels", spatial_downsample=1), {"image": x4})     # (pixels, no subsampling: taken)
    assert _declines(image_only(prep_type="pixels", spatial_downsample=2), {"image": x4})  # pixels with subsampling
    assert _declines(image_only(prep_type="conv1x1", spatial_downsample=1), {"image": x4})  # another preprocessing type
    assert _declines(image_only(conv_after_patching=True, num_channels=8), {"image": x4})
    assert _declines(image_only(concat_or_add_pos="add", spatial_downsample=1, prep_type="pixels",
                                position_encoding_type=PosEncodingType.TRAINABLE,
                                trainable_position_encoding_kwargs=dict(num_channels=3)), {"image": x4})   # added positions
    assert _declines(image_only(n_extra_pos_mlp=1), {"image": x4})                  # extra position MLPs
    video = torch.randn(2, 4, 3, 16, 16)
    assert _declines(image_only(num_frames=4, temporal_downsample=2,
                                fourier_position_encoding_kwargs=dict(num_bands=4, max_resolution=(2, 4, 4), sine_only=False,
                                                                      concat_pos=True)), {"image": video})   # temporal block 2
    assert _declines(image_only(input_channels=5), {"image": torch.randn(2, 5, 16, 16)})   # C > 4
    mm = MultimodalPreprocessor(torch.nn.ModuleDict({"text": EmbeddingPreprocessor(16, 8, 12)}), min_padding_size=2).eval()
    assert _declines(mm, {"text": torch.zeros(2, 8)})                                # another preprocessor
    assert L.PIO_MAX_TOKEN_SEGMENTS == 8
