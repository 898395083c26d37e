"""CPU, no launch: the 1x1-conv and pixel front ends of the classifier -- the header and the signature table carry
pio_conv1x1_tokens; its refusal table (a refused call returns before it touches a device); every decline rule of
fused_io.conv1x1_tokens and the arguments of an accepted plan, with runtime.call stubbed; the projected position table's
cache on the preprocessor; the float64 definition against torch's convolution; and the three classifier variants on CPU
under the torch backend, where nothing fused runs."""
import copy
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv1x1_cases as CC  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pio_hip.h")


class FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on a GPU: what fused_io.gate asks of its tensors."""
    @property
    def is_cuda(self):
        return True


def fake(t):
    return t.as_subclass(FakeCuda)


def make_prep(c=3, n=8, s=1, hw=(6, 10), pos=8, trainable=True, **kw):
    from perceiverio_pytorch_amd.io_processors import ImagePreprocessor
    from perceiverio_pytorch_amd.position_encoding import PosEncodingType
    index = (hw[0] // s) * (hw[1] // s)
    if trainable:
        enc = dict(position_encoding_type=PosEncodingType.TRAINABLE,
                   trainable_position_encoding_kwargs=dict(init_scale=0.02, num_channels=pos))
    else:
        enc = dict(position_encoding_type=PosEncodingType.FOURIER,
                   fourier_position_encoding_kwargs=dict(num_bands=3, max_resolution=[d // s for d in hw], concat_pos=True,
                                                         sine_only=False))
    args = dict(img_size=hw, input_channels=c, prep_type="conv1x1", num_channels=n, spatial_downsample=s,
                project_pos_dim=pos, concat_or_add_pos="concat")
    args.update(enc)
    args.update(kw)
    prep = ImagePreprocessor(**args).eval()
    assert int(np.prod(prep.index_dims)) == index
    return prep


@pytest.fixture
def calls(monkeypatch):
    """runtime.call stubbed: the launches fused_io would have made, as (name, args)."""
    from perceiverio_pytorch_amd import runtime as R
    seen = []

    def call(dev, name, *args, **kw):
        seen.append((name, args))
        return True
    monkeypatch.setattr(R, "call", call)
    return seen


def test_header_and_signature_table_carry_the_entry_point():
    from perceiverio_pytorch_amd import _lib as L
    text = open(HEADER).read()
    decl = re.search(r"\bint\s+pio_conv1x1_tokens\s*\(([^;]*)\)\s*;", text)
    assert decl is not None
    names = [a.strip().split()[-1].lstrip("*") for a in decl.group(1).replace("\n", " ").split(",")]
    assert tuple(names) == CC.ARG_ORDER + ("stream",)
    assert "pio_conv1x1_tokens" in L.SIGNATURES and len(L.SIGNATURES["pio_conv1x1_tokens"][1]) == len(CC.ARG_ORDER) + 1
    cap = re.search(r"#define\s+PIO_CONV1X1_MAX_N\s+(\d+)", text)
    assert cap is not None and int(cap.group(1)) == L.PIO_CONV1X1_MAX_N == CC.N_CAP >= 256


@pytest.mark.parametrize("what,changes,code", CC.REFUSALS, ids=[r[0] for r in CC.REFUSALS])
def test_refusal_table(what, changes, code):
    from perceiverio_pytorch_amd import _lib as L
    assert changes and set(changes) <= set(CC.ARG_ORDER)
    assert CC.refusal_call(L.lib(), changes) == code


def test_definition_equals_torch_convolution_in_float64():
    for kind, shape in CC.ACCURACY_CASES[:3] + CC.ACCURACY_CASES[4:]:
        x, w, bias = CC.accuracy_data("image", shape, 3)
        s = shape[4]
        ref, mag = CC.reference(x, w, bias, s)
        got = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double()[:, :, None, None],
                                         torch.from_numpy(bias).double(), stride=s)
        got = got.movedim(1, -1).reshape(shape[0], -1, shape[5]).numpy()
        assert got.shape == ref.shape and float(np.abs(got - ref).max()) <= 1e-14
        assert (mag >= np.abs(ref) - 1e-14).all()
    # the exact-addressing parameters select a plane and add n
    x = CC.exact_pixels(2, 3, 4, 6)
    w, bias = CC.exact_params(3, 8)
    assert np.array_equal(CC.reference(x, w, bias, 2)[0], CC.exact_expected(x, 2, 8).astype(np.float64))
    assert len(np.unique(x)) == x.size and CC.gamma(4) > 4 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------
# fused_io.conv1x1_tokens: decline rules and accepted plans
# ---------------------------------------------------------------------------------------------------
def _image(b=2, c=3, hw=(6, 10)):
    return torch.arange(b * c * hw[0] * hw[1], dtype=torch.float32).reshape(b, c, *hw)


def _swap_conv(prep, conv):
    prep.convnet_1x1 = conv
    return prep


def _param(prep, name, value):
    setattr(prep.convnet_1x1, name, torch.nn.Parameter(value))
    return prep


DECLINES = {
    "switch off": lambda: (setattr_(make_prep(), "fused_conv1x1", False), fake(_image())),
    "cpu tensor": lambda: (make_prep(), _image()),
    "float64 tensor": lambda: (make_prep(), fake(_image().double())),
    "5-D input": lambda: (make_prep(), fake(_image()[:, None])),
    "3-D input": lambda: (make_prep(), fake(_image()[0])),
    "prep_type pixels": lambda: (make_prep(prep_type="pixels", project_pos_dim=-1), fake(_image())),
    "groups": lambda: (_swap_conv(make_prep(c=4), torch.nn.Conv2d(4, 8, 1, groups=2)), fake(_image(c=4))),
    "dilation": lambda: (_swap_conv(make_prep(), torch.nn.Conv2d(3, 8, 1, dilation=2)), fake(_image())),
    "padding": lambda: (_swap_conv(make_prep(), torch.nn.Conv2d(3, 8, 1, padding=1)), fake(_image())),
    "padding mode": lambda: (_swap_conv(make_prep(), torch.nn.Conv2d(3, 8, 1, padding_mode="reflect")), fake(_image())),
    "non-square stride": lambda: (_swap_conv(make_prep(), torch.nn.Conv2d(3, 8, 1, stride=(1, 2))), fake(_image())),
    "3x3 kernel": lambda: (_swap_conv(make_prep(), torch.nn.Conv2d(3, 8, 3)), fake(_image())),
    "float64 weight": lambda: (_param(make_prep(), "weight", torch.zeros(8, 3, 1, 1).double()), fake(_image())),
    "bias on another device": lambda: (_param(make_prep(), "bias", torch.zeros(8, device="meta")), fake(_image())),
    "float64 bias": lambda: (_param(make_prep(), "bias", torch.zeros(8).double()), fake(_image())),
    "C = 5": lambda: (make_prep(c=5), fake(_image(c=5))),
    "s = 9": lambda: (make_prep(s=9, hw=(9, 9)), fake(_image(hw=(9, 9)))),
    "H % s": lambda: (make_prep(s=4, hw=(8, 8)), fake(_image(hw=(6, 8)))),
    "W % s": lambda: (make_prep(s=4, hw=(8, 8)), fake(_image(hw=(8, 6)))),
    "N % 4": lambda: (make_prep(n=6), fake(_image())),
    "N above the cap": lambda: (make_prep(n=CC.N_CAP + 4), fake(_image())),
    "empty batch": lambda: (make_prep(), fake(_image()[:0])),
    "OH*OW != prod(index_dims)": lambda: (make_prep(), fake(_image(hw=(6, 8)))),
}


def setattr_(obj, name, value):
    setattr(obj, name, value)
    return obj


@pytest.mark.parametrize("what", sorted(DECLINES))
def test_every_decline_rule_runs_the_chain(what, calls):
    from perceiverio_pytorch_amd import fused_io as FIO
    prep, x = DECLINES[what]()
    assert FIO.conv1x1_tokens(prep, x) is None and prep._conv1x1_front(x) is None and calls == []


def test_the_torch_backend_declines(calls):
    import perceiverio_pytorch_amd as P
    prep, x = make_prep(), fake(_image())
    prev = P.get_backend()
    P.set_backend("torch")
    try:
        assert prep._conv1x1_front(x) is None and calls == []
    finally:
        P.set_backend(prev)
    assert prep._conv1x1_front(x) is not None and len(calls) == 1         # (the same pair is taken under hip)


def _plan(calls, prep, x):
    del calls[:]
    with torch.no_grad():
        y = prep._conv1x1_front(x)
    assert len(calls) == 1 and calls[0][0] == "pio_conv1x1_tokens" and len(calls[0][1]) == len(CC.ARG_ORDER)
    return y, dict(zip(CC.ARG_ORDER, calls[0][1]))


def test_accepted_plans_pass_the_source_as_it_stands(calls):
    prep = make_prep(c=3, n=8, s=2, hw=(6, 10))
    conv = prep.convnet_1x1
    sizes = dict(C=3, H=6, W=10, s=2, N=8, ldw=3, ldy=8, sYb=15 * 8)
    # contiguous
    x = fake(_image())
    y, f = _plan(calls, prep, x)
    assert tuple(y.shape) == (2, 15, 8) and y.dtype == torch.float32 and y.is_contiguous()
    assert (f["x"], f["sb"], f["sc"], f["sy"], f["sx"]) == (x.data_ptr(), 180, 60, 10, 1)
    assert (f["w"], f["bias"], f["y"], f["B"]) == (conv.weight.data_ptr(), conv.bias.data_ptr(), y.data_ptr(), 2)
    assert {k: f[k] for k in sizes} == sizes
    # a permute of a channels-last buffer: read in place
    nhwc = torch.arange(2 * 6 * 10 * 3, dtype=torch.float32).reshape(2, 6, 10, 3)
    x = fake(nhwc.permute(0, 3, 1, 2))
    y, f = _plan(calls, prep, x)
    assert (f["x"], f["sb"], f["sc"], f["sy"], f["sx"]) == (nhwc.data_ptr(), 180, 1, 30, 3)
    assert {k: f[k] for k in sizes} == sizes and f["B"] == 2
    # a batch slice of a larger tensor, starting one element in and wider than the image
    big = torch.arange(5 * 3 * 7 * 12, dtype=torch.float32).reshape(5, 3, 7, 12)
    x = fake(big[1:4:2, :, 1:, 1:11])
    y, f = _plan(calls, prep, x)
    assert f["x"] == big.data_ptr() + 4 * (252 + 12 + 1) and (f["sb"], f["sc"], f["sy"], f["sx"]) == (504, 84, 12, 1)
    assert {k: f[k] for k in sizes} == sizes and f["B"] == 2 and tuple(y.shape) == (2, 15, 8)
    # a stride-0 batch; no bias
    conv.bias = None
    x = fake(_image(b=1).expand(4, 3, 6, 10))
    y, f = _plan(calls, prep, x)
    assert (f["sb"], f["B"], f["bias"], f["sYb"]) == (0, 4, None, 120) and tuple(y.shape) == (4, 15, 8)
    # a weight whose rows are not contiguous is read through a detached copy; its pitch is the copy's
    wide = torch.nn.Parameter(torch.randn(8, 6, 1, 1))
    conv.weight = torch.nn.Parameter(wide[:, ::2])
    assert not conv.weight.is_contiguous()
    y, f = _plan(calls, prep, fake(_image()))
    assert f["w"] != conv.weight.data_ptr() and f["ldw"] == 3


def test_result_is_tied_to_its_inputs_when_autograd_records(calls):
    prep = make_prep()
    y = prep._conv1x1_front(fake(_image()))
    assert y.requires_grad and y.grad_fn is not None
    with pytest.raises(NotImplementedError, match="no backward"):
        y.sum().backward()
    with torch.no_grad():
        assert not prep._conv1x1_front(fake(_image())).requires_grad


# ---------------------------------------------------------------------------------------------------
# the projected position table: once per parameter set, in the preprocessor's PackedCache
# ---------------------------------------------------------------------------------------------------
def _feats(prep, b=2):
    return fake(torch.zeros(b, int(np.prod(prep.index_dims)), 8))


@pytest.mark.parametrize("trainable", [True, False], ids=["learned", "fourier"])
def test_projected_table_is_built_once_and_dropped_by_every_invalidation_point(trainable, monkeypatch):
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import runtime as R
    prep = make_prep(trainable=trainable)
    assert isinstance(prep, R.PackedOwner) and len(prep._packed) == 0
    enc = prep._positional_encoding
    lin = enc._projector
    built = []
    real = torch.nn.functional.linear

    def linear(*a, **k):
        built.append(a[0].shape)
        return real(*a, **k)
    monkeypatch.setattr(torch.nn.functional, "linear", linear)
    with torch.no_grad():
        a = prep._split_pos(_feats(prep))
        b = prep._split_pos(_feats(prep, b=5))
    assert a is not None and b is not None and a[1] is b[1] and len(built) == 1 and len(built[0]) == 2   # ONE [M, .] call
    table = a[1]
    base = enc._base_position_encoding(None, None, device=torch.device("cpu")) if not trainable \
        else enc._base_position_encoding.pos_embs
    assert tuple(table.shape) == (60, 8) and table.is_contiguous() and not table.requires_grad
    assert torch.equal(table, real(base.detach(), lin.weight.detach(), lin.bias.detach()))
    assert len(prep._packed) == 1 and prep._packed.held("pos_table")[1] is table
    # inside inference mode the cached table is an ordinary tensor, and the same one
    with torch.inference_mode():
        c = prep._split_pos(_feats(prep))
    assert c[1] is table and not table.is_inference() and len(built) == 1

    def rebuilt(n):
        with torch.no_grad():
            t = prep._split_pos(_feats(prep))[1]
        assert len(built) == n and torch.equal(t, real(base.detach(), lin.weight.detach(), lin.bias.detach()))
        return t
    with torch.no_grad():
        lin.bias.add_(1.0)                      # an in-place update bumps the version
    t2 = rebuilt(2)
    assert t2 is not table and not torch.equal(t2, table)
    prep.load_state_dict(prep.state_dict())
    assert len(prep._packed) == 0
    t3 = rebuilt(3)
    P.invalidate_packed_weights(prep)
    assert len(prep._packed) == 0
    t4 = rebuilt(4)
    prep.float()                                # (_apply: .to() / .cuda() / .float())
    assert len(prep._packed) == 0
    assert rebuilt(5) is not t4 and t3 is not t4
    twin = copy.deepcopy(prep)
    assert len(prep._packed) == 1 and len(twin._packed) == 0 and twin._packed is not prep._packed
    keys = list(prep.state_dict())
    assert keys == list(twin.state_dict()) and not list(prep.buffers())
    assert sorted(k for k in keys if "_positional_encoding" in k) == sorted(
        ["_positional_encoding._projector.weight", "_positional_encoding._projector.bias"]
        + (["_positional_encoding._base_position_encoding.pos_embs"] if trainable else []))
    assert not any("packed" in k or "table" in k for k in keys)


def test_projected_table_declines_what_the_chain_must_keep(calls):
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd.position_encoding import PosEncodingType

    def split(prep, feats=None):
        with torch.no_grad():
            return prep._split_pos(_feats(prep) if feats is None else feats)
    assert split(make_prep()) is not None
    assert split(setattr_(make_prep(), "fused_conv1x1", False)) is None              # the switch: the concatenated hand-off
    prep = make_prep()
    assert split(prep, torch.zeros(2, 60, 8)) is None and len(prep._packed) == 0     # CPU features
    assert split(make_prep(concat_or_add_pos="add")) is None
    assert split(make_prep(n_extra_pos_mlp=1)) is None
    assert split(make_prep(pos=7)) is None                                           # an odd width cannot be split
    prev = P.get_backend()
    P.set_backend("torch")
    try:
        assert split(make_prep()) is None
    finally:
        P.set_backend(prev)
    # an unprojected learned table is the stride-0 view it always was: no cache entry
    plain = make_prep(project_pos_dim=-1)
    got = split(plain)
    assert got is not None and got[1].data_ptr() == plain._positional_encoding.pos_embs.data_ptr() and len(plain._packed) == 0
    # forward() with caller-supplied positions and the "full" hand-off never consult the cache
    prep = make_prep(trainable=False)
    with torch.no_grad():
        prep(_image(), pos=None)
    assert len(prep._packed) == 0 and prep._position_encoding_type == PosEncodingType.FOURIER


# ---------------------------------------------------------------------------------------------------
# the pixel variant's plan and the model's switch
# ---------------------------------------------------------------------------------------------------
def test_pixel_front_declines_what_can_be_split_or_is_not_plain_pixels(calls):
    def pix(c=3, **kw):
        return make_prep(c=c, prep_type="pixels", project_pos_dim=-1, trainable=False, **kw)
    prep = pix()
    assert prep._positional_encoding.n_output_channels() == 14 and prep.fused_pixels is True
    with torch.no_grad():
        got = prep._pixel_front(fake(_image()))
    assert got is not None and [c[0] for c in calls] == ["pio_assemble_tokens"]
    x, wo = got
    assert tuple(x.shape) == (2, 60, 17) and tuple(wo.shape) == (2, 60, 3) and wo.data_ptr() == x.data_ptr()
    del calls[:]
    with torch.no_grad():
        assert setattr_(pix(), "fused_pixels", False)._pixel_front(fake(_image())) is None
        assert pix()._pixel_front(_image()) is None                                       # a CPU tensor
        assert pix(c=4)._pixel_front(fake(_image(c=4))) is None                           # 4 | 14: the split form fits
        assert pix(s=2)._pixel_front(fake(_image())) is None                              # subsampling
        assert pix()._pixel_front(fake(_image()[:, None])) is None                        # video
        assert pix(concat_or_add_pos="add")._pixel_front(fake(_image())) is None
        assert make_prep()._pixel_front(fake(_image())) is None                           # not "pixels"
    assert calls == []


def test_classifier_switch_forwards_to_both_preprocessor_switches():
    from perceiverio_pytorch_amd.io_processors import ImagePreprocessor
    from perceiverio_pytorch_amd.models import ClassificationPerceiver, PrepType
    assert isinstance(ClassificationPerceiver.fused_front_end, property)
    assert ImagePreprocessor.fused_conv1x1 is True and ImagePreprocessor.fused_pixels is True
    model = ClassificationPerceiver(num_classes=5, img_size=(8, 8), prep_type=PrepType.LEARNED_POS_1X1CONV,
                                    num_self_attends_per_block=1, num_blocks=1, num_latents=4, num_latent_channels=16)
    prep = model.perceiver._multi_preprocessor._preprocessors["__default"]
    keys = list(model.state_dict())
    assert model.fused_front_end is True
    model.fused_front_end = False
    assert model.fused_front_end is False and prep.fused_conv1x1 is False and prep.fused_pixels is False
    model.fused_front_end = 1
    assert model.fused_front_end is True and prep.fused_conv1x1 is True and prep.fused_pixels is True
    assert ImagePreprocessor.fused_conv1x1 is True and list(model.state_dict()) == keys


@pytest.mark.parametrize("prep_type", ["FOURIER_POS_CONVNET", "LEARNED_POS_1X1CONV", "FOURIER_POS_PIXEL"])
def test_classifier_on_cpu_equals_itself_with_the_switch_off(prep_type, calls):
    """Under the torch backend on CPU tensors the switch changes nothing: both settings run the chain, nothing is launched
    and nothing is cached."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd.models import ClassificationPerceiver, PrepType
    torch.manual_seed(11)
    model = ClassificationPerceiver(num_classes=5, img_size=(8, 8), prep_type=PrepType[prep_type],
                                    num_self_attends_per_block=1, num_blocks=1, num_latents=4,
                                    num_latent_channels=16).eval()
    prep = model.perceiver._multi_preprocessor._preprocessors["__default"]
    img = torch.randn(2, 3, 8, 8)
    prev = P.get_backend()
    P.set_backend("torch")
    try:
        with torch.no_grad():
            a = model(img)
            model.fused_front_end = False
            b = model(img)
    finally:
        P.set_backend(prev)
    assert a.shape == (2, 5) and torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert calls == [] and len(prep._packed) == 0
