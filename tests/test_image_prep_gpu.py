"""GPU: prepare_images on the device -- pio_prepare_images through the public function on every case of
tests/image_prep_cases.py against the float64 definition under its derived tolerance (bit-equal at in == out); a
one-pixel-wide antialiased output; lists against single calls and the grouping into launches, bit for bit; planted pixels;
guard bands around a strided `out`; non-finite sources; the refusal table with a watched output; the switch; graph replay.

With PIO_IMAGE_PREP_RATIOS=<file> the worst |r - r64| / tolerance of every case is written there as JSON (the figures of
profiles/image_prep.json)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_prep_cases as PC  # noqa: E402
from test_image_prep_host import REFUSALS, check_chain, raw_call  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = sorted(PC.CASES)
RATIOS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    yield torch.device("cuda:0")
    path = os.environ.get("PIO_IMAGE_PREP_RATIOS")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


def _counting(monkeypatch):
    """pio_prepare_images as every module sees it (a proxy in front of _lib.lib()), counted."""
    from perceiverio_pytorch_amd import _lib as L
    calls = {"kernel": 0}
    real = L.lib()

    class _Lib:
        def __getattr__(self, k):
            return getattr(real, k)

        def pio_prepare_images(self, *a):
            calls["kernel"] += 1
            return real.pio_prepare_images(*a)
    proxy = _Lib()
    monkeypatch.setattr(L, "lib", lambda: proxy)
    return calls


def _hold(got, want, tol, what):
    """got fp32 [C, oh, ow] (numpy) against (r64, tolerance); returns the worst ratio."""
    ratio = float((np.abs(got.astype(np.float64) - want) / tol).max())
    print(f"{what}: {ratio:.3f} of the tolerance")
    assert ratio <= 1.0, f"{what}: {ratio:.3f} of the tolerance"
    return ratio


@pytest.mark.parametrize("name", NAMES)
def test_kernel_is_the_definition(dev, monkeypatch, name):
    import perceiverio_pytorch_amd as P
    calls = _counting(monkeypatch)
    spec = PC.CASES[name]
    images, kw = PC.torch_inputs(name, dev)
    out = P.prepare_images(images, **kw)
    n = len(spec["imgs"])
    items = 1 if spec["batch"] and not isinstance(spec["crop"], list) else n      # (a uniform batch is ONE descriptor)
    assert calls["kernel"] == (items + PC.MAX_SOURCES - 1) // PC.MAX_SOURCES
    assert out.dtype == torch.float32 and out.device == dev and out.shape[0] == n and out.is_contiguous()
    got = out.cpu().numpy()
    worst = 0.0
    for i, ((r64, tol), box, x) in enumerate(zip(PC.expected(name), PC.boxes_of(name), PC.gen(name))):
        assert got[i].shape == r64.shape
        worst = max(worst, _hold(got[i], r64, tol, f"{name}[{i}]"))
        if r64.shape[1:] == (box[2], box[3]):                  # in == out: the bits of (x - mean) / std
            c = spec["C"]
            m = np.float32(PC.per_channel(spec["mean"], c, 0.0)).reshape(-1, 1, 1)
            s = np.float32(PC.per_channel(spec["std"], c, 1.0)).reshape(-1, 1, 1)
            v = x[:, box[0]:box[0] + box[2], box[1]:box[1] + box[3]].astype(np.float32)
            assert np.array_equal(got[i], ((v[::-1] if spec["rev"] else v) - m) / s), f"{name}[{i}]: not bit-equal"
    RATIOS[name] = worst


def test_one_pixel_wide_antialiased_output(dev):
    import perceiverio_pytorch_amd as P
    x = PC.gen("down_aa")[0]
    out = P.prepare_images(torch.from_numpy(x).to(dev), (16, 1), crop=(0, 5, 37, 33), channels_last=False)
    r64, ty, tx = PC.restate(x, (0, 5, 37, 33), (16, 1), True, False, [0.0] * 3, [1.0] * 3)
    assert tx == 33
    RATIOS["one_wide_aa"] = _hold(out[0].cpu().numpy(), r64, PC.tolerance(r64, ty, tx, 255.0, [1.0] * 3), "37x33 -> 16x1")


@pytest.mark.parametrize("name", ["list3", "many", "batch3", "batch3_boxes"])
def test_an_image_does_not_depend_on_its_company(dev, name):
    """Every image of a list / batch equals the image prepared alone, bit for bit (for `many`: across the two launches)."""
    import perceiverio_pytorch_amd as P
    spec = PC.CASES[name]
    images, kw = PC.torch_inputs(name, dev)
    out = P.prepare_images(images, **kw)
    boxes = PC.boxes_of(name)
    for i in range(len(spec["imgs"])):
        alone = P.prepare_images(images[i], **dict(kw, crop=boxes[i], channels_last=spec["imgs"][i][3] == "cl"))
        assert torch.equal(out[i:i + 1], alone), f"{name}: image {i} differs from its own call"


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("shape,size", [((37, 53), (16, 24)), ((7, 5), (16, 24)), ((9, 70), (9, 130))])
def test_planted_pixels(dev, shape, size, antialias):
    """An image of zeros with one 255 at each corner and at one interior position in turn: the output is the outer product
    of that row's and column's weights within the tolerance, and zero exactly where the definition gives zero."""
    import perceiverio_pytorch_amd as P
    h, w = shape
    Wy, ty = PC.axis_weights(h, size[0], antialias)
    Wx, tx = PC.axis_weights(w, size[1], antialias)
    # (the interior position: the heaviest tap of an interior output -- without antialiasing a reduction skips pixels)
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (int(np.argmax(Wy[size[0] // 2])), int(np.argmax(Wx[size[1] // 3])))]
    x = torch.zeros((len(spots), 1, h, w), dtype=torch.uint8)
    for i, (y, xx) in enumerate(spots):
        x[i, 0, y, xx] = 255
    out = P.prepare_images(x.to(dev), size, antialias=antialias, channels_last=False).cpu().numpy()
    for i, (y, xx) in enumerate(spots):
        want = 255.0 * np.outer(Wy[:, y], Wx[:, xx])[None]
        _hold(out[i], want, PC.tolerance(want, ty, tx, 255.0, [1.0]), f"{shape}->{size} aa={antialias} spot {(y, xx)}")
        assert (want != 0).any() and np.array_equal(out[i] == 0, want == 0), f"spot {(y, xx)}: zeros are not the definition's"


def test_guard_bands(dev):
    """out= as a window of a larger NaN-patterned buffer with a batch stride larger than the image: every byte outside the
    N C oh ow values is unchanged."""
    import perceiverio_pytorch_amd as P
    images, kw = PC.torch_inputs("batch3", dev)
    want = P.prepare_images(images, **kw)
    n, c, oh, ow = want.shape
    per, guard = c * oh * ow, 257
    buf = torch.full((guard + n * (per + guard),), 0x7FC00000 + 1234567, dtype=torch.int32, device=dev).view(torch.float32)
    out = torch.as_strided(buf, (n, c, oh, ow), (per + guard, oh * ow, ow, 1), guard)
    assert P.prepare_images(images, out=out, **kw) is out
    assert torch.equal(out, want)
    bits = buf.view(torch.int32).clone()
    mask = torch.ones_like(bits, dtype=torch.bool)
    for i in range(n):
        mask[guard + i * (per + guard):guard + i * (per + guard) + per] = False
    assert bool((bits[mask] == 0x7FC00000 + 1234567).all()), "a byte outside the images was written"


def test_non_finite_sources_stay_local(dev):
    """An inf and a NaN in an fp32 source: the kernel finishes, every output with a positive weight on the pixel is not
    finite, and every output whose taps do not reach it keeps its bits."""
    import perceiverio_pytorch_amd as P
    x = torch.from_numpy(PC.gen("window_f32_cf")[0]).to(dev)
    clean = P.prepare_images(x, (16, 24), channels_last=False)
    x[1, 20, 30] = float("inf")
    x[2, 0, 0] = float("nan")
    out = P.prepare_images(x, (16, 24), channels_last=False)
    torch.cuda.synchronize()
    Wy, _ = PC.axis_weights(37, 16, True)
    Wx, _ = PC.axis_weights(53, 24, True)
    (ylo, yhi), (xlo, xhi) = PC.axis_windows(37, 16, True), PC.axis_windows(53, 24, True)
    assert torch.equal(out[0, 0], clean[0, 0])
    for c, (y, xx) in ((1, (20, 30)), (2, (0, 0))):
        touched = torch.from_numpy(np.outer(Wy[:, y] > 0, Wx[:, xx] > 0)).to(dev)
        reached = torch.from_numpy(np.outer((ylo <= y) & (y < yhi), (xlo <= xx) & (xx < xhi))).to(dev)
        assert touched.any() and not torch.isfinite(out[0, c][touched]).any()
        assert (~reached).any() and torch.equal(out[0, c][~reached], clean[0, c][~reached])


@pytest.mark.parametrize("what,changes,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_output_untouched(dev, what, changes, code):
    from perceiverio_pytorch_amd import _lib as L
    src = torch.zeros(4096, dtype=torch.uint8, device=dev)
    out = torch.full((1024,), float("nan"), device=dev)
    assert raw_call(L, src.data_ptr(), out.data_ptr(), changes, torch.cuda.current_stream().cuda_stream) == code
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_switch_off_runs_the_chain_on_the_device(dev, monkeypatch):
    import perceiverio_pytorch_amd as P
    calls = _counting(monkeypatch)
    monkeypatch.setattr(P, "fused_image_prep", False)
    for name in ("down_aa", "up_noaa", "list3", "ident_u8"):
        images, kw = PC.torch_inputs(name, dev)
        out = P.prepare_images(images, **kw)
        assert out.device == dev
        check_chain(out.cpu(), name)
    assert calls["kernel"] == 0


def test_graph_replay_gives_the_eager_bits(dev):
    import perceiverio_pytorch_amd as P
    images, kw = PC.torch_inputs("batch3", dev)
    eager = P.prepare_images(images, **kw)
    out = torch.empty_like(eager)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        P.prepare_images(images, out=out, **kw)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        P.prepare_images(images, out=out, **kw)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
