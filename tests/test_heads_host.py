"""CPU: the output heads (pio_project_heads) as far as they go without a device -- the header declares the entry and the
built library exports it; the ctypes struct against the C layout; the refusal table (a refused call returns before it
touches a device) and its self-consistency; every reason for PerceiverIO._project_heads to decline; the switches; and the
chain the torch backend and CPU tensors take, against the float64 definition within the derived bound."""
import contextlib
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_cases as HC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_segments(L, seg_fields, count=None):
    """ctypes array of pio_head_segment_t from the plain field dicts of heads_cases (count: array length, >= 1)."""
    arr = (L.HeadSegment * max(count or len(seg_fields), len(seg_fields), 1))()
    for i, f in enumerate(seg_fields):
        for k, v in f.items():
            setattr(arr[i], k, v)
    return arr


def project_heads(L, seg_fields, args, stream=None):
    nseg = args.get("nseg", len(seg_fields))
    segs = make_segments(L, seg_fields, count=max(nseg, 1))
    return L.lib().pio_project_heads(segs, nseg, args["x"], args["x_sb"], args["ldx"], args["B"], args["Q"], args["K"], stream)


def test_header_declares_and_library_exports_the_entry():
    from perceiverio_pytorch_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "pio_hip.h")).read()
    assert re.search(r"\bint\s+pio_project_heads\s*\(\s*const\s+pio_head_segment_t\s*\*", header)
    assert re.search(r"#define\s+PIO_MAX_HEAD_SEGMENTS\s+4\b", header)
    assert "pio_project_heads" in L.SIGNATURES and L.PIO_MAX_HEAD_SEGMENTS == 4
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "pio_project_heads"), "libpio_hip.so does not export pio_project_heads"
    assert L.lib().pio_project_heads.argtypes[0] == ctypes.POINTER(L.HeadSegment)


def test_struct_matches_the_c_layout():
    from perceiverio_pytorch_amd import _lib as L
    fields = [f for f, _ in L.HeadSegment._fields_]
    assert fields == ["row0", "rows", "w", "ldw", "bias", "n_out", "y", "y_sb", "y_rs"]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "pio_hip.h"\nint main(void){printf("%zu", ' \
           'sizeof(pio_head_segment_t));\n' + \
           "".join(f'printf(" %zu", offsetof(pio_head_segment_t, {f}));\n' for f in fields) + \
           'printf(" %d\\n", PIO_MAX_HEAD_SEGMENTS); return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    S = L.HeadSegment
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields] + [L.PIO_MAX_HEAD_SEGMENTS]


def made_up_pointers():
    ptrs = {"x": 0x100000}
    for i in range(len(HC.VALID_SEGS)):
        for k, f in enumerate(HC.POINTER_FIELDS):
            ptrs[(i, f)] = 0x200000 + 0x10000 * (4 * i + k)
    return ptrs


def test_refusal_table_is_self_consistent():
    """Every row changes exactly ONE field of the valid call, to a value it does not have; names are unique; the valid
    call itself satisfies every documented condition."""
    a, segs = HC.VALID_ARGS, HC.VALID_SEGS
    assert len({r[0] for r in HC.REFUSALS}) == len(HC.REFUSALS)
    assert {r[2] for r in HC.REFUSALS} == {HC.PIO_E_ARG, HC.PIO_E_SHAPE, HC.PIO_E_ALIGN}
    for what, changes, code in HC.REFUSALS:
        assert len(changes) == 1, what
        (k, v), = changes.items()
        if isinstance(k, tuple):
            assert 0 <= k[0] < len(segs) and (k[1] in HC.POINTER_FIELDS or (k[1] in segs[k[0]] and segs[k[0]][k[1]] != v)), what
        else:
            assert k == "x" or (k in a and a[k] != v), what
        if isinstance(v, str):
            assert v.startswith("ptr+") and int(v[4:]) > 0, what
    assert a["nseg"] == len(segs) and 1 <= a["nseg"] <= 4 and a["B"] >= 1 and a["Q"] >= 1
    assert 4 <= a["K"] <= 1024 and a["K"] % 4 == 0 and a["ldx"] >= a["K"] and a["ldx"] % 4 == 0 and a["x_sb"] % 4 == 0
    assert a["x_sb"] >= a["Q"] * a["ldx"]
    spans = []
    for g in segs:
        assert 1 <= g["n_out"] <= 16 and g["rows"] >= 0 and g["row0"] >= 0 and g["row0"] + g["rows"] <= a["Q"]
        assert g["ldw"] >= a["K"] and g["ldw"] % 4 == 0 and g["y_rs"] >= g["n_out"] and g["y_sb"] >= g["rows"] * g["y_rs"]
        spans.append((g["row0"], g["row0"] + g["rows"]))
    assert spans[0][1] <= spans[1][0]
    p = made_up_pointers()
    assert p["x"] % 16 == 0 and all(p[(i, "w")] % 16 == 0 for i in range(len(segs)))


@pytest.mark.parametrize("what,changes,code", HC.REFUSALS, ids=[r[0] for r in HC.REFUSALS])
def test_refusal_table(what, changes, code):
    """Bad arguments are refused with the documented code before anything is launched: made-up (aligned, non-NULL)
    addresses are enough, and no device is needed."""
    from perceiverio_pytorch_amd import _lib as L
    segs, args = HC.refusal_fields(made_up_pointers(), changes)
    assert project_heads(L, segs, args) == code


def test_null_segment_table_is_refused():
    from perceiverio_pytorch_amd import _lib as L
    a = HC.VALID_ARGS
    assert L.lib().pio_project_heads(None, 2, 0x100000, a["x_sb"], a["ldx"], a["B"], a["Q"], a["K"], None) == HC.PIO_E_ARG


def test_case_table_covers_what_it_claims():
    c = HC.CASES
    assert {k["K"] for k in c.values()} >= {4, 8, 260, 512, 1024}
    assert {g["n_out"] for k in c.values() for g in k["segs"]} >= {1, 2, 3, 5, 16}
    assert {g["rows"] for k in c.values() for g in k["segs"]} >= {0, 1, HC.STRIP - 1, HC.STRIP, HC.STRIP + 1, 257}
    assert {k["B"] for k in c.values()} == {1, 2}
    assert any(k["ldx"] > k["K"] for k in c.values()) and any(g["y_rs"] > g["n_out"] for k in c.values() for g in k["segs"])
    assert any(not g["bias"] for k in c.values() for g in k["segs"])
    three = c["k512_three"]
    assert len({g["n_out"] for g in three["segs"]}) == 3 and not HC.covered_rows(three).all()
    for name, k in c.items():
        assert k["ldx"] % 4 == 0 and k["K"] % 4 == 0
        data = HC.gen(name)
        assert data["x_sb"] > k["Q"] * k["ldx"]
        cov = HC.covered_rows(k)
        assert np.isnan(data["x"][:, ~cov]).all() and np.isnan(data["x_full"][:, :, k["K"]:]).all()
        for (ref, mag), g in zip(HC.reference(name, data), k["segs"]):
            assert ref.shape == (k["B"], g["rows"], g["n_out"])
            if name in HC.PLANTED:
                b, r, _ = HC.PLANTED[name]
                nan = np.zeros(ref.shape, dtype=bool)
                nan[b, r - g["row0"]] = True
                assert np.array_equal(np.isnan(ref), nan)
            else:
                assert np.isfinite(ref).all()


# ----------------------------------------------------------------------------------------------------
# eligibility and the chain
# ----------------------------------------------------------------------------------------------------
def tiny(posts, k=8):
    """PerceiverIO with the given output postprocessors over decoder rows of k channels (one learned query per head)."""
    from perceiverio_pytorch_amd.output_queries import TrainableQuery
    from perceiverio_pytorch_amd.perceiver import PerceiverIO
    queries = {m: TrainableQuery(output_index_dims=(2,), num_channels=4) for m in posts}
    return PerceiverIO(num_blocks=1, num_self_attends_per_block=1, num_latents=4, num_latent_channels=8, final_project_out_channels=k,
                       input_channels=8, output_queries=queries, output_postprocessors=posts).eval()


def heads(k=8, image=3, audio=16, label=True):
    from perceiverio_pytorch_amd.io_processors import (AudioPostprocessor, ClassificationPostprocessor,
                                                       ProjectionPostprocessor)
    posts = {}
    if audio:
        posts["audio"] = AudioPostprocessor(in_channels=k, samples_per_patch=audio)
    if image:
        posts["image"] = ProjectionPostprocessor(num_inputs=k, num_outputs=image)
    if label:
        posts["label"] = ClassificationPostprocessor(num_input_channels=k, num_classes=5)
    return posts


def test_switches_exist():
    from perceiverio_pytorch_amd.perceiver import PerceiverIO
    from test_models import build
    assert PerceiverIO.fused_heads is True
    model = build("model_multimodal_small")
    assert model.fused_heads is True and model.perceiver.fused_heads is True
    model.fused_heads = False
    assert model.fused_heads is False and model.perceiver.fused_heads is False and PerceiverIO.fused_heads is True
    model.fused_heads = True
    assert model.perceiver.fused_heads is True and model.perceiver._heads_eligible(512)


def test_acceptance_predicate():
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd.io_processors import FlowPostprocessor, IdentityPostprocessor
    assert tiny(heads())._heads_eligible(8)
    assert tiny(heads(label=False))._heads_eligible(8)                          # two narrow heads, no classifier
    assert tiny(heads(audio=0))._heads_eligible(8)                              # one narrow head + the classifier
    io = tiny(heads())
    io.fused_heads = False
    assert not io._heads_eligible(8)                                            # the switch
    assert not tiny(dict(heads(), label=IdentityPostprocessor()))._heads_eligible(8)        # a wrong head type
    assert not tiny(dict(heads(), image=FlowPostprocessor((1, 2))))._heads_eligible(8)
    assert tiny(heads(audio=16))._heads_eligible(8) and not tiny(heads(audio=17))._heads_eligible(8)   # n_out = 17
    io = tiny(heads())
    io._output_postprocessors["image"].double()
    assert not io._heads_eligible(8)                                            # fp64 weights
    assert not tiny(heads(audio=0, label=False))._heads_eligible(8)             # a single modality
    assert not tiny({"label": heads()["label"], "other": heads()["label"]})._heads_eligible(8)    # no narrow head at all
    io = tiny(heads())
    assert not io._heads_eligible(6) and not io._heads_eligible(16)             # K % 4; K that is not the heads' width
    assert tiny(heads(k=1024), k=1024)._heads_eligible(1024) and not tiny(heads(k=1028), k=1028)._heads_eligible(1028)
    prev = P.get_backend()
    P.set_backend("torch")
    try:
        with P.range_probe():
            assert not io._heads_eligible(8)                                    # an active range probe
    finally:
        P.set_backend(prev)
    assert io._heads_eligible(8)


def _chain(io, x, sizes):
    from perceiverio_pytorch_amd.perceiver import restructure
    per_mod = restructure(sizes, x)
    return {m: post(per_mod[m], pos=None, modality_sizes=None) for m, post in io._output_postprocessors.items()}


def test_cpu_tensors_and_the_torch_backend_take_the_chain():
    """_project_heads declines CPU tensors (under either backend) and the torch backend; the chain they take instead equals
    the float64 definition within the derived bound."""
    import perceiverio_pytorch_amd as P
    k, sizes = 260, {"audio": 3, "image": 70, "label": 1}
    torch.manual_seed(5)
    io = tiny(heads(k=k, image=3, audio=16), k=k)
    with torch.no_grad():
        for p in io._output_postprocessors.parameters():
            p.copy_(torch.randn_like(p) / (k ** 0.5 if p.dim() == 2 else 1.0))
    x = torch.randn(2, sum(sizes.values()), k)
    assert io._heads_eligible(k) and not io._heads_accept(x) and io._project_heads(x, sizes) is None

    class FakeCuda(torch.Tensor):
        @property
        def is_cuda(self):
            return True
    prev = P.get_backend()
    P.set_backend("torch")
    try:
        assert not io._heads_accept(x.as_subclass(FakeCuda)) and io._project_heads(x.as_subclass(FakeCuda), sizes) is None
        with torch.no_grad():
            out = _chain(io, x, sizes)
    finally:
        P.set_backend(prev)
    assert out["image"].shape == (2, 70, 3) and out["audio"].shape == (2, 3 * 16) and out["label"].shape == (2, 5)
    for m, lin, rows in (("audio", io._output_postprocessors["audio"].linear, x[:, 0:3]),
                         ("image", io._output_postprocessors["image"].projection, x[:, 3:73])):
        ref, mag = HC.definition(rows.numpy(), lin.weight.detach().numpy(), lin.bias.detach().numpy())
        HC.assert_within_bound(out[m].numpy(), ref, mag, k, f"the chain on CPU tensors, {m}")


def test_declined_configurations_never_reach_the_entry(monkeypatch):
    """With a stand-in "CUDA" tensor under the hip backend an eligible configuration reaches the entry point (replaced by
    one that raises); the declined ones return None before it."""
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd import runtime as R

    class FakeCuda(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    class _Lib:
        def pio_project_heads(self, *a):
            raise AssertionError("reached the entry point")
    monkeypatch.setattr(L, "lib", lambda: _Lib())
    monkeypatch.setattr(R, "on_device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(R, "stream_ptr", lambda d: 0)
    sizes = {"audio": 3, "image": 5}
    x = torch.randn(2, 8, 8).as_subclass(FakeCuda)
    io = tiny(heads(label=False))
    with pytest.raises(AssertionError, match="reached the entry point"):
        io._project_heads(x, sizes)
    assert io._project_heads(x.double().as_subclass(FakeCuda), sizes) is None       # not fp32
    assert io._project_heads(x[:, :, ::2], sizes) is None                           # channel stride 2 (and K = 4 != 8)
    assert io._project_heads(x, {"audio": 3, "other": 5}) is None                   # sizes of other modalities
    assert io._project_heads(x, {"audio": 3, "image": 6}) is None                   # more rows than the decoder made
    io.fused_heads = False
    assert io._project_heads(x, sizes) is None
