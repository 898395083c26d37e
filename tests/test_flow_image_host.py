"""CPU: flow_to_image -- the acceptance rule of tests/flow_image_cases.py pinned to the definition (the repository's numpy
function passes it on every case, the band share stays under its cap, the planted cases give the stated bytes), the torch
restatement on CPU tensors under the same rule and equal to numpy in the fp32 part, the tensor / ndarray dispatch of
utils.flow_utils.flow_to_image, and the C-ABI symbol in header and ctypes table."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_image_cases as IC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from utils import flow_utils as FU  # noqa: E402

NAMES = sorted(IC.CASES)


def numpy_images(name):
    """The repository's numpy function, image by image."""
    f = IC.gen(name)
    return np.stack([FU.flow_to_image(f[i], IC.clip_of(name), IC.bgr_of(name)) for i in range(f.shape[0])])


def test_the_wheel_of_the_rule_is_the_wheel_of_the_definition():
    assert IC.WHEEL.shape == (55, 3) and np.array_equal(IC.WHEEL, FU.make_colorwheel())
    assert tuple(IC.WHEEL[0]) == (255, 0, 0) and tuple(IC.WHEEL[54]) == (255, 0, 43)


@pytest.mark.parametrize("name", NAMES)
def test_numpy_definition_passes_the_rule(name):
    IC.check(numpy_images(name), IC.gen(name), IC.clip_of(name), IC.bgr_of(name), f"numpy {name}")


@pytest.mark.parametrize("name", [n for n in NAMES if not IC.planted(n)])
def test_band_share_is_under_the_cap(name):
    c, white = IC.reference_c(IC.gen(name), IC.clip_of(name))
    s = IC.share(c, white)
    print(f"{name}: band share {s:.4%} of {int((~white).sum())} values; {int(white.sum())} values are 255 by construction")
    assert s < IC.BAND_CAP
    # the values left out are one channel per pixel (and the three of a pixel clipped to (0, 0)), not most of the image
    assert (~white).sum() >= 0.4 * white.size


def test_a_wrong_image_is_rejected():
    """The rule is no rubber stamp: one byte moved by one outside the band, and a channel swap, fail it."""
    f, img = IC.gen("33x130"), numpy_images("33x130")
    c, _ = IC.reference_c(f)
    lo, hi = IC.bounds(c)
    i = tuple(np.argwhere((lo == hi) & (lo < 255))[0])
    wrong = img.copy()
    wrong[i] += 1
    with pytest.raises(AssertionError):
        IC.check(wrong, f, what="one byte off")
    with pytest.raises(AssertionError):
        IC.check(img[..., ::-1], f, what="channels swapped")


def test_planted_zero_flow_is_white():
    assert (numpy_images("zero") == 255).all()
    assert (IC.bounds(IC.reference_c(IC.gen("zero"))[0])[1] == 255).all()


def test_planted_signed_zero_selects_entries_0_and_54():
    f = IC.gen("signed_zero")
    un, vn, radn, _ = IC.steps123(f)
    assert (radn < 1).all()
    r = radn.astype(np.float64)[0]
    img = numpy_images("signed_zero")[0]
    for row, entry in ((0, 0), (1, 54)):
        want = 255 * (1 - r[row][:, None] * (1 - IC.WHEEL[entry][None, :] / 255.0))
        lo, hi = IC.bounds(want)
        assert ((img[row] >= lo) & (img[row] <= hi)).all(), (row, entry)
    assert (img[0, :, 1] == img[0, :, 2]).all() and (img[1, -1, 2] > img[1, -1, 1])     # entry 0: g = b; entry 54: b above g


def test_planted_directions_are_eight_colours():
    img = numpy_images("directions")[0]
    for row in img:
        assert len({tuple(p) for p in row}) == 8
    un, vn, _, _ = IC.steps123(IC.gen("directions"))
    fk = (np.arctan2(-vn.astype(np.float64), -un.astype(np.float64)) / np.pi + 1) / 2 * 54
    assert np.allclose(fk[0, 0], [0, 6.75, 13.5, 20.25, 27, 33.75, 40.5, 47.25], atol=1e-5)


def test_planted_big_radius_sits_on_the_branch():
    f = IC.gen("big")
    un, vn, radn, s = IC.steps123(f)
    rad = np.sqrt(f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]).max(axis=(1, 2))
    assert rad.dtype == np.float32 and (np.abs(rad - 1e4) < 1).all() and (s.ravel() == rad).all()   # s rounded back to rad_max
    assert radn[0, 4, 5] > 1 and radn[1, 2, 7] == 1 and radn[2, 8, 11] < 1
    assert (np.delete(radn[0].ravel(), 4 * 12 + 5) < 1e-3).all()
    img, (c, _) = numpy_images("big"), IC.reference_c(f)
    # the 0.75 branch (no channel above floor(191.25)) and the other one, on pixels a rounding apart
    k = 255 * 0.75
    assert img[0, 4, 5].max() <= np.floor(k) and np.floor(c[0, 4, 5]).max() <= np.floor(k)
    assert img[1, 2, 7].max() == 255 and img[1, 2, 7].min() == 0                         # wheel entry 0 at rad_n = 1


def test_a_batch_wide_maximum_would_show():
    f = IC.gen("batch3")
    per_image, _ = IC.reference_c(f)
    batch_wide, _ = IC.reference_c(f, batch_wide_max=True)
    differ = [bool((np.floor(per_image[i]) != np.floor(batch_wide[i])).mean() > 0.5) for i in range(3)]
    assert differ == [True, False, True]


def _torch_images(name, fn):
    f = torch.from_numpy(np.array(IC.gen(name)))
    if IC.CASES[name].get("chw"):
        f = f[0].permute(2, 0, 1).contiguous().permute(1, 2, 0)
        assert not f.is_contiguous()
    return fn(f, IC.clip_of(name), IC.bgr_of(name))


@pytest.mark.parametrize("name", NAMES)
def test_torch_restatement_on_cpu_passes_the_rule(name):
    import perceiverio_pytorch_amd as P
    img = _torch_images(name, P.flow_to_image)
    assert isinstance(img, torch.Tensor) and img.dtype == torch.uint8 and img.device.type == "cpu"
    f = IC.gen(name)
    assert tuple(img.shape) == (f.shape[1:3] if IC.CASES[name].get("chw") else f.shape[:3]) + (3,)
    IC.check(img.numpy(), f[0] if img.dim() == 3 else f, IC.clip_of(name), IC.bgr_of(name), f"restatement {name}")


@pytest.mark.parametrize("name", NAMES)
def test_torch_restatement_equals_numpy_in_the_fp32_part(name):
    from perceiverio_pytorch_amd import flow_image as FI
    got = FI.normalised(torch.from_numpy(np.array(IC.gen(name))), IC.clip_of(name))
    want = IC.steps123(IC.gen(name), IC.clip_of(name))[:3]
    for g, w, what in zip(got, want, ("u_n", "v_n", "rad_n")):
        assert np.array_equal(g.numpy().view(np.int32), w.view(np.int32)), f"{name}: {what} differs from numpy's bits"


def test_other_dtypes_are_upcast():
    import perceiverio_pytorch_amd as P
    f = torch.from_numpy(np.array(IC.gen("5x7")))[0]
    assert torch.equal(P.flow_to_image(f.double()), P.flow_to_image(f))
    h = f.half()
    assert torch.equal(P.flow_to_image(h), P.flow_to_image(h.float()))
    with pytest.raises(ValueError):
        P.flow_to_image(torch.zeros(4, 5, 3))
    with pytest.raises(TypeError):
        P.flow_to_image(np.zeros((4, 5, 2), np.float32))


def test_the_switch_exists_and_is_on():
    import perceiverio_pytorch_amd as P
    assert P.fused_flow_image is True


def test_dispatch_tensor_in_tensor_out_ndarray_in_ndarray_out():
    f = np.array(IC.gen("bgr"))[0]
    a = FU.flow_to_image(f, convert_to_bgr=True)
    assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.shape == (8, 13, 3)
    t = FU.flow_to_image(torch.from_numpy(f), convert_to_bgr=True)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and tuple(t.shape) == (8, 13, 3)
    IC.check(t.numpy(), f, bgr=True, what="dispatch")
    tb = FU.flow_to_image(torch.from_numpy(np.array(IC.gen("batch3"))))
    assert isinstance(tb, torch.Tensor) and tuple(tb.shape) == (3, 17, 40, 3)


def test_the_symbol_is_in_header_and_ctypes_table():
    from perceiverio_pytorch_amd import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pio_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pio_flow_to_image\s*\(", src)
    res, args = L.SIGNATURES["pio_flow_to_image"]
    assert len(args) == 14 and args[8] is L.C.c_float
    assert hasattr(L.lib(), "pio_flow_to_image")


def test_refusals_of_the_raw_entry_need_no_gpu():
    """Every refusal comes before anything touches the device: the table runs on fake, never dereferenced addresses."""
    from perceiverio_pytorch_amd import _lib as L
    for what, ch, code in IC.REFUSALS:
        flow = None if "flow" in ch else 0x10000 + ch.get("flow_offset", 0)
        out = None if "out" in ch else 0x20000
        rad = None if "rad" in ch else 0x30000
        b, h, w = ch.get("b", 1), ch.get("h", IC.R_H), ch.get("w", IC.R_W)
        got = IC.raw(L, flow, (2 * h * w, 2 * w, 2, 1), b, h, w, out, rad, None)
        assert got == code, (what, got)
