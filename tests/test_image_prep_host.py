"""CPU: prepare_images -- the float64 definition of tests/image_prep_cases.py against F.interpolate and against the torch
chain on every case, argument handling, the plan's decline rules, the three model helpers against the examples' own lines,
and the C-ABI symbol in header, library and ctypes table."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_prep_cases as PC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(PC.CASES)


def aten_bound(in_y, in_x):
    """Four fp32 ulps of the largest source coordinate times the value range: what ATen's fp32 coordinates
    (scale * (i + 0.5) rounded to fp32) cost against the exact weights."""
    return 4 * 2.0 ** -23 * max(in_y, in_x) * 255


@pytest.mark.parametrize("antialias", [True, False])
def test_integer_weights_are_the_written_formulas(antialias):
    for n_in, n_out in [(5, 5), (37, 16), (53, 24), (7, 16), (5, 24), (257, 8), (130, 8), (375, 224), (1, 4), (1920, 224)]:
        W, _ = PC.axis_weights(n_in, n_out, antialias)
        assert np.abs(W - PC.axis_weights_literal(n_in, n_out, antialias)).max() < 1e-12
        assert np.abs(W.sum(1) - 1).max() < 1e-14 and W.min() >= 0


def test_definition_against_interpolate():
    """The restatement against F.interpolate on fp32 CPU tensors of integers 0 .. 255: equal at in == out, elsewhere
    within aten_bound; the worst ratio is printed."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for (h, w), (oh, ow) in [((5, 7), (5, 7)), ((37, 53), (16, 24)), ((7, 5), (16, 24)), ((130, 257), (8, 8)),
                             ((375, 375), (224, 224)), ((500, 375), (224, 224)), ((1080, 1920), (224, 224))]:
        x = rng.integers(0, 256, (3, h, w)).astype(np.float32)
        for aa in (True, False):
            want, _, _ = PC.restate(x, (0, 0, h, w), (oh, ow), aa, False, [0.0] * 3, [1.0] * 3)
            got = F.interpolate(torch.from_numpy(x)[None], size=(oh, ow), mode="bilinear", align_corners=False,
                                antialias=aa)[0].double().numpy()
            err = np.abs(got - want).max()
            if (h, w) == (oh, ow):
                assert err == 0.0
            else:
                ratio = err / aten_bound(h, w)
                worst = max(worst, ratio)
                print(f"{h}x{w} -> {oh}x{ow} antialias={aa}: {err:.3e} ({ratio:.3f} of the bound)")
                assert ratio <= 1.0
    print(f"worst ratio {worst:.3f}")


def check_chain(got, name):
    """A chain result [N, C, oh, ow] against the restatement: bit-equal to the fp32 (x - mean) / std at in == out, elsewhere
    within aten_bound / |std| plus the two fp32 roundings of the subtraction and the division (2 . 2^-23 |r|)."""
    spec = PC.CASES[name]
    c = spec["C"]
    std = np.abs(np.asarray(np.float32(PC.per_channel(spec["std"], c, 1.0)), np.float64)).reshape(-1, 1, 1)
    worst = 0.0
    for i, ((r64, _), box, x) in enumerate(zip(PC.expected(name), PC.boxes_of(name), PC.gen(name))):
        g = got[i].double().numpy()
        assert g.shape == r64.shape
        if r64.shape[1:] == (box[2], box[3]):
            m = np.float32(PC.per_channel(spec["mean"], c, 0.0)).reshape(-1, 1, 1)
            s = np.float32(PC.per_channel(spec["std"], c, 1.0)).reshape(-1, 1, 1)
            v = x[:, box[0]:box[0] + box[2], box[1]:box[1] + box[3]].astype(np.float32)
            exact = ((v[::-1] if spec["rev"] else v) - m) / s
            assert np.array_equal(got[i].numpy(), exact), f"{name}[{i}]: not the bits of (x - mean) / std"
        else:
            bound = aten_bound(box[2], box[3]) / std + 2 * 2.0 ** -23 * np.abs(r64)
            worst = max(worst, float((np.abs(g - r64) / bound).max()))
    assert worst <= 1.0, f"{name}: {worst:.3f} of the bound"
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_chain_on_cpu_tensors_is_the_definition(name):
    import perceiverio_pytorch_amd as P
    images, kw = PC.torch_inputs(name, "cpu")
    out = P.prepare_images(images, **kw)
    assert out.dtype == torch.float32 and out.dim() == 4 and out.shape[0] == len(PC.CASES[name]["imgs"])
    print(f"{name}: {check_chain(out, name):.3f} of the bound")


def test_switch_off_and_torch_backend_take_the_chain():
    import perceiverio_pytorch_amd as P
    images, kw = PC.torch_inputs("down_aa", "cpu")
    want = P.prepare_images(images, **kw)
    P.fused_image_prep = False
    try:
        assert torch.equal(P.prepare_images(images, **kw), want)
    finally:
        P.fused_image_prep = True
    prev = P.get_backend()
    P.set_backend("torch")
    try:
        assert torch.equal(P.prepare_images(images, **kw), want)
    finally:
        P.set_backend(prev)


def test_layout_inference():
    import perceiverio_pytorch_amd as P
    x = torch.arange(3 * 6 * 8, dtype=torch.float32).reshape(3, 6, 8)
    a = P.prepare_images(x)                                     # channels first: 3 <= 4 < 8
    b = P.prepare_images(x.permute(1, 2, 0))                    # channels last: 3 <= 4 < 6
    assert tuple(a.shape) == (1, 3, 6, 8) and torch.equal(a, b) and torch.equal(a[0], x)
    assert tuple(P.prepare_images(torch.zeros(2, 6, 8, 3, dtype=torch.uint8)).shape) == (2, 3, 6, 8)
    for shape in [(3, 4, 4), (4, 4, 3), (8, 8, 8), (2, 3, 3, 3)]:
        with pytest.raises(ValueError, match="channels_last"):
            P.prepare_images(torch.zeros(shape))
    assert tuple(P.prepare_images(torch.zeros(4, 4, 3), channels_last=True).shape) == (1, 3, 4, 4)
    assert tuple(P.prepare_images(torch.zeros(3, 4, 4), channels_last=False).shape) == (1, 3, 4, 4)


def test_bad_arguments_raise_value_errors():
    import perceiverio_pytorch_amd as P
    x = torch.zeros(3, 6, 8)
    for bad in [dict(crop=(0, 0, 7, 8)), dict(crop=(-1, 0, 2, 2)), dict(crop=(0, 0, 0, 2)), dict(crop="centre"),
                dict(crop=[(0, 0, 2, 2), (0, 0, 2, 2)]), dict(crop=(0.5, 0, 2, 2)), dict(size=0), dict(size=(4, -1)),
                dict(mean=(1.0, 2.0)), dict(std=0.0), dict(std=(1.0, 0.0, 1.0)), dict(out=torch.zeros(1, 3, 6, 7)),
                dict(out=torch.zeros(1, 3, 6, 8, dtype=torch.float64)), dict(out=torch.zeros(1, 3, 8, 6).transpose(2, 3))]:
        with pytest.raises(ValueError):
            P.prepare_images(x, **bad)
    for images in [[], [x, torch.zeros(1, 6, 8)], [x, x[None]], torch.zeros(6, 8), x.double(), torch.zeros(5, 6, 8),
                   np.zeros((3, 6, 8), np.float32)]:
        with pytest.raises(ValueError):
            P.prepare_images(images)
    with pytest.raises(ValueError, match="different sizes"):
        P.prepare_images([x, torch.zeros(3, 7, 9)])              # size=None needs one crop size


def test_center_boxes_for_odd_and_even_sizes():
    from perceiverio_pytorch_amd.image_prep import center_box
    assert center_box(500, 375) == (62, 0, 375, 375) and center_box(375, 500) == (0, 62, 375, 375)
    assert center_box(5, 4) == (0, 0, 4, 4) and center_box(4, 7) == (0, 1, 4, 4) and center_box(6, 6) == (0, 0, 6, 6)
    assert center_box(9, 4) == (2, 0, 4, 4)
    for h, w in [(500, 375), (5, 4), (4, 7), (9, 4), (240, 320)]:
        m = min(h, w)
        assert center_box(h, w) == PC.center_box(h, w) == (int(h / 2 - m / 2), int(w / 2 - m / 2), m, m)


def test_per_image_boxes_list_against_tensor_and_out():
    import perceiverio_pytorch_amd as P
    imgs = [torch.from_numpy(x) for x in PC.gen("batch3_boxes")]
    boxes = PC.CASES["batch3_boxes"]["crop"]
    batch = P.prepare_images(torch.stack(imgs), (16, 24), crop=boxes, channels_last=False)
    as_list = P.prepare_images(imgs, (16, 24), crop=boxes, channels_last=False)
    assert torch.equal(batch, as_list)
    for i, (x, b) in enumerate(zip(imgs, boxes)):
        assert torch.equal(batch[i:i + 1], P.prepare_images(x, (16, 24), crop=b, channels_last=False))
        assert torch.equal(batch[i:i + 1], P.prepare_images(x[:, b[0]:b[0] + b[2], b[1]:b[1] + b[3]], (16, 24),
                                                            channels_last=False))
    big = torch.full((3, 2, 3, 16, 24), float("nan"))
    out = big[:, 0]                                              # batch stride twice the image
    got = P.prepare_images(imgs, (16, 24), crop=boxes, channels_last=False, out=out)
    assert got is out and torch.equal(out, batch) and torch.isnan(big[:, 1]).all()


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on a GPU: lets the plan's checks run where no device exists."""
    @property
    def is_cuda(self):
        return True


def test_plan_decline_rules():
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, fused_io as FIO
    assert (L.PIO_MAX_IMAGE_SOURCES, L.PIO_IMAGE_MAX_REDUCTION) == (PC.MAX_SOURCES, PC.MAX_REDUCTION)

    def item(shape=(2, 3, 40, 50), dtype=torch.uint8, box=None, cuda=True):
        x = torch.zeros(shape, dtype=dtype)
        return (x.as_subclass(_FakeCuda) if cuda else x), box or (0, 0, shape[2], shape[3])

    assert FIO.image_prep_decline(True, [item(), item(dtype=torch.float32)], 16, 24) is None      # (taken)
    assert FIO.image_prep_decline(True, [item(box=(0, 0, 40, 50))], 1, 2) is None                 # (reduction 40, 25)
    assert "off" in FIO.image_prep_decline(False, [item()], 16, 24)
    assert "GPU" in FIO.image_prep_decline(True, [item(), item(cuda=False)], 16, 24)
    assert "dtype" in FIO.image_prep_decline(True, [item(dtype=torch.float16)], 16, 24)
    assert "dtype" in FIO.image_prep_decline(True, [item(dtype=torch.float64)], 16, 24)
    assert "output side" in FIO.image_prep_decline(True, [item()], 1025, 24)
    assert "output side" in FIO.image_prep_decline(True, [item()], 16, 1025)
    assert "source side" in FIO.image_prep_decline(True, [item((1, 1, 2, 16385))], 16, 24)
    assert "source side" in FIO.image_prep_decline(True, [item((1, 1, 16385, 2))], 16, 24)
    assert "reduction" in FIO.image_prep_decline(True, [item(box=(0, 0, 40, 50))], 1, 1)          # 50 > 40 x 1
    assert "reduction" in FIO.image_prep_decline(True, [item((1, 3, 41, 8))], 1, 8)
    prev = P.get_backend()
    P.set_backend("torch")
    try:
        assert "backend" in FIO.image_prep_decline(True, [item()], 16, 24)
    finally:
        P.set_backend(prev)
    # what the plan declines goes down the chain: a reduction above the cap on CPU tensors is the chain's anyway
    x = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (3, 90, 8)).astype(np.uint8))
    want, _, _ = PC.restate(x.numpy(), (0, 0, 90, 8), (2, 8), True, False, [0.0] * 3, [1.0] * 3)
    assert np.abs(P.prepare_images(x, (2, 8)).double().numpy()[0] - want).max() <= aten_bound(90, 8)


def test_entry_point_refuses_before_it_launches():
    """Every PIO_E_ARG / PIO_E_SHAPE / PIO_E_ALIGN rule of pio_prepare_images on host addresses: a refused call returns
    before it touches a device (tests/test_image_prep_gpu.py repeats the table with a watched output buffer)."""
    from perceiverio_pytorch_amd import _lib as L
    for what, changes, code in REFUSALS:
        assert raw_call(L, 0x1000, 0x2000, changes) == code, what


def base_fields():
    return dict(nsrc=1, C=3, oh=4, ow=6, aa=1, rev=0, out_sb=72, null_srcs=False, null_out=False, out_off=0,
                src=dict(data_off=0, sb=0, sc=1, sy=30, sx=3, dtype=0, n=1, C=3, H=8, W=10, y0=0, x0=0, ch=8, cw=10))


REFUSALS = [
    ("NULL table", dict(null_srcs=True), -6), ("NULL out", dict(null_out=True), -6), ("NULL data", dict(src=dict(data_off=None)), -6),
    ("nsrc 0", dict(nsrc=0), -6), ("nsrc 33", dict(nsrc=33), -6), ("dtype 2", dict(src=dict(dtype=2)), -6),
    ("C 0", dict(C=0, src=dict(C=0)), -1), ("C 5", dict(C=5, src=dict(C=5)), -1), ("C differs", dict(src=dict(C=4)), -1),
    ("n 0", dict(src=dict(n=0)), -1), ("H 0", dict(src=dict(H=0)), -1), ("W 16385", dict(src=dict(W=16385)), -1),
    ("H 16385", dict(src=dict(H=16385)), -1), ("oh 0", dict(oh=0), -1), ("oh 1025", dict(oh=1025), -1),
    ("ow 0", dict(ow=0), -1), ("ow 1025", dict(ow=1025), -1), ("empty box", dict(src=dict(ch=0)), -1),
    ("empty box x", dict(src=dict(cw=0)), -1), ("box above", dict(src=dict(y0=-1)), -1), ("box left", dict(src=dict(x0=-1)), -1),
    ("box below", dict(src=dict(y0=1)), -1), ("box right", dict(src=dict(x0=1)), -1), ("negative row stride", dict(src=dict(sy=-30)), -1),
    ("negative column stride", dict(src=dict(sx=-3)), -1), ("negative channel stride", dict(src=dict(sc=-1)), -1),
    ("negative batch stride", dict(src=dict(n=2, sb=-240)), -1), ("reduction y", dict(oh=1, ow=1, src=dict(H=41, ch=41)), -1),
    ("reduction x", dict(oh=8, ow=1, src=dict(W=41, cw=41, sy=123)), -1), ("out_sb", dict(out_sb=71, src=dict(n=2, sb=240)), -1),
    ("fp32 data unaligned", dict(src=dict(dtype=1, data_off=2)), -2), ("out unaligned", dict(out_off=2), -2),
]


def raw_call(L, data, out, changes, stream=None):
    """pio_prepare_images on base_fields() with `changes` applied (src: merged), every source at address `data`."""
    f = base_fields()
    src = dict(f["src"], **changes.get("src", {}))
    f.update({k: v for k, v in changes.items() if k != "src"})
    n = max(1, min(f["nsrc"], L.PIO_MAX_IMAGE_SOURCES + 1))
    arr = (L.ImageSource * n)()
    for d in arr:
        d.data = None if src["data_off"] is None else data + src["data_off"]
        for k in ("sb", "sc", "sy", "sx", "dtype", "n", "C", "H", "W", "y0", "x0", "ch", "cw"):
            setattr(d, k, src[k])
    return L.lib().pio_prepare_images(None if f["null_srcs"] else arr, f["nsrc"], f["C"], f["oh"], f["ow"], f["aa"], f["rev"],
                                      None, None, None if f["null_out"] else out + f["out_off"], f["out_sb"], stream)


def test_struct_size_and_symbol():
    from perceiverio_pytorch_amd import _lib as L
    prog = ('#include <stdio.h>\n#include "pio_hip.h"\nint main(void){printf("%zu %d %d\\n", sizeof(pio_image_src_t), '
            'PIO_MAX_IMAGE_SOURCES, PIO_IMAGE_MAX_REDUCTION); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        size, cap, red = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert (size, cap, red) == (ctypes.sizeof(L.ImageSource), L.PIO_MAX_IMAGE_SOURCES, L.PIO_IMAGE_MAX_REDUCTION)
    src = open(os.path.join(ROOT, "include", "pio_hip.h")).read()
    assert re.search(r"\bint\s+pio_prepare_images\s*\(", src)
    assert "pio_prepare_images" in L.SIGNATURES and hasattr(L.lib(), "pio_prepare_images")


# ----------------------------------------------------------------------------------------------------
# the model helpers against the examples' own lines
# ----------------------------------------------------------------------------------------------------
def test_classifier_prepare_is_the_example():
    from perceiverio_pytorch_amd.models import ClassificationPerceiver
    model = ClassificationPerceiver.__new__(ClassificationPerceiver)      # (prepare reads img_size only: no weights built)
    model.img_size = (224, 224)
    rng = np.random.default_rng(3)
    imgs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)) for h, w in [(500, 375), (300, 420)]]
    got = model.prepare(imgs)
    assert tuple(got.shape) == (2, 3, 224, 224)
    mean = torch.tensor((0.485 * 255, 0.456 * 255, 0.406 * 255)).view(3, 1, 1)
    std = torch.tensor((0.229 * 255, 0.224 * 255, 0.225 * 255)).view(3, 1, 1)
    for g, img in zip(got, imgs):
        x = img.permute(2, 0, 1).float()
        h, w = x.shape[1:]
        m = min(h, w)
        top, left = int(h / 2 - m / 2), int(w / 2 - m / 2)                 # resized_crop(img, top, left, m, m, (224, 224))
        v = F.interpolate(x[None, :, top:top + m, left:left + m], size=(224, 224), mode="bilinear", align_corners=False,
                          antialias=True)[0]
        assert torch.equal(g, (v - mean) / std)                            # Normalize(MEAN_RGB, STDDEV_RGB)
    assert "img_size" not in ClassificationPerceiver(num_blocks=1, num_self_attends_per_block=1, num_latents=8,
                                                     num_latent_channels=64).state_dict()


def test_video_prepare_is_the_example():
    from perceiverio_pytorch_amd.models import MultiModalPerceiver
    model = MultiModalPerceiver.__new__(MultiModalPerceiver)
    model.H, model.W = 24, 24
    rng = np.random.default_rng(4)
    for h, w in [(30, 40), (41, 30)]:
        frames = torch.from_numpy(rng.integers(0, 256, (4, h, w, 3)).astype(np.uint8))
        got = model.prepare_video(frames)
        assert tuple(got.shape) == (1, 4, 3, 24, 24)
        m = min(h, w)
        sy, sx = h // 2 - m // 2, w // 2 - m // 2                          # crop_center_square
        sq = frames[:, sy:sy + m, sx:sx + m].permute(0, 3, 1, 2).float()
        v = F.interpolate(sq, size=(24, 24), mode="bilinear", align_corners=False)     # cv2.resize (INTER_LINEAR), unrounded
        want = v[:, [2, 1, 0]] / 255.0                                     # frame[:, :, [2, 1, 0]];  / 255.0
        assert torch.equal(got[0], want)
        assert torch.equal(model.prepare_video(list(frames), bgr=False)[0], v / 255.0)


def test_flow_prepare_is_the_example_up_to_rounding():
    """(x - 127.5) / 127.5 against the example's 2 * (x / 255) - 1 over all 256 byte values: the largest difference is
    printed and bounded at 2 ulp of 1.0 (2 . 2^-23)."""
    from perceiverio_pytorch_amd.models import FlowPerceiver
    x = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16).expand(3, 16, 16)
    got = FlowPerceiver.prepare(x)
    assert tuple(got.shape) == (1, 3, 16, 16)
    want = 2 * (x.float() / 255.0) - 1.0
    diff = (got[0].double() - want.double()).abs().max().item()
    print(f"largest difference over the 256 byte values: {diff:.3e} ({diff / 2.0 ** -23:.2f} ulp of 1.0)")
    assert diff <= 2 * 2.0 ** -23
    assert torch.equal(FlowPerceiver.prepare(x.float()), got)
