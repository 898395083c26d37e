"""GPU: flow_to_image on the device -- pio_flow_to_image through the public function on every case of
tests/flow_image_cases.py under its acceptance rule; once through raw ctypes with a sentinel-filled guard band around the
output; one maximum per image; the permuted view read in place; two calls identical; the refusals; the switch; and the small
flow golden's forward followed by the visualisation, against the numpy function on the same flow copied to the host."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_image_cases as IC  # noqa: E402
from test_models import _load_generated, build  # noqa: E402
from _golden import load  # noqa: E402
from cases import model_inputs, model_seed, model_stats  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from utils import flow_utils as FU  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096
NAMES = sorted(IC.CASES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


def _counting(monkeypatch):
    """pio_flow_to_image as every module sees it (a proxy in front of _lib.lib()): counted, its arguments kept."""
    from perceiverio_pytorch_amd import _lib as L
    calls = {"kernel": 0, "args": None}
    real = L.lib()

    class _Lib:
        def __getattr__(self, k):
            return getattr(real, k)

        def pio_flow_to_image(self, *a):
            calls["kernel"] += 1
            calls["args"] = a
            return real.pio_flow_to_image(*a)
    proxy = _Lib()
    monkeypatch.setattr(L, "lib", lambda: proxy)
    return calls


def device_flow(name, dev):
    """The case's flow on the device in the layout the case asks for: [b, h, w, 2], or a [2, h, w] tensor seen through
    .permute(1, 2, 0)."""
    f = torch.from_numpy(np.array(IC.gen(name))).to(dev)
    if IC.CASES[name].get("chw"):
        f = f[0].permute(2, 0, 1).contiguous().permute(1, 2, 0)
    return f


def run_public(name, dev):
    import perceiverio_pytorch_amd as P
    f = device_flow(name, dev)
    img = P.flow_to_image(f, IC.clip_of(name), IC.bgr_of(name))
    assert img.dtype == torch.uint8 and img.device == f.device and tuple(img.shape) == tuple(f.shape[:-1]) + (3,)
    assert img.is_contiguous()
    return img


def _check(img, name, what):
    f = IC.gen(name)
    return IC.check(img.cpu().numpy(), f[0] if img.dim() == 3 else f, IC.clip_of(name), IC.bgr_of(name), what)


@pytest.mark.parametrize("name", NAMES)
def test_kernel_passes_the_rule_through_the_public_function(dev, monkeypatch, name):
    calls = _counting(monkeypatch)
    img = run_public(name, dev)
    assert calls["kernel"] == 1
    _check(img, name, f"kernel {name}")
    if name == "zero":
        assert bool((img == 255).all())


def test_raw_entry_with_guard_bands(dev):
    """33 x 130 through raw ctypes: the 3 h w bytes of the image sit between two sentinel-filled bands that must be untouched
    (the image ends in the middle of a dword: 12 870 = 4 * 3217 + 2 bytes), the maxima word holds rad_max's bits."""
    from perceiverio_pytorch_amd import _lib as L
    name = "33x130"
    f = torch.from_numpy(np.array(IC.gen(name))).to(dev)
    _, h, w, _ = f.shape
    n = 3 * h * w
    pattern = ((torch.arange(GUARD, dtype=torch.int64) * 37 + 11) % 251).to(torch.uint8).to(dev)
    buf = torch.empty(GUARD + n + GUARD, dtype=torch.uint8, device=dev)
    buf[:GUARD], buf[GUARD + n:] = pattern, pattern
    buf[GUARD:GUARD + n] = 0x5a
    rad = torch.full((3,), -1, dtype=torch.int32, device=dev)
    code = IC.raw(L, f.data_ptr(), (2 * h * w, 2 * w, 2, 1), 1, h, w, buf.data_ptr() + GUARD, rad.data_ptr() + 4,
                  torch.cuda.current_stream().cuda_stream)
    assert code == IC.PIO_OK
    torch.cuda.synchronize()
    assert torch.equal(buf[:GUARD], pattern), "bytes in FRONT of the image were written"
    assert torch.equal(buf[GUARD + n:], pattern), "bytes BEHIND the image were written"
    IC.check(buf[GUARD:GUARD + n].view(1, h, w, 3).cpu().numpy(), IC.gen(name), what="raw entry 33x130")
    got = rad.cpu().numpy()
    g = IC.gen(name)
    want = np.sqrt(g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]).max()
    assert got[0] == -1 and got[2] == -1 and got[1] == want.view(np.int32), "the maxima word is not rad_max, or a neighbour was written"


def test_raw_entry_planar_layout_and_unaligned_output(dev):
    """The model's own [b, 2, h, w] layout through its strides, into an output that starts at an odd address (byte stores)."""
    from perceiverio_pytorch_amd import _lib as L
    name = "batch3"
    f = torch.from_numpy(np.array(IC.gen(name))).to(dev)
    b, h, w, _ = f.shape
    planar = f.permute(0, 3, 1, 2).contiguous()
    n = 3 * b * h * w
    buf = torch.full((n + 16,), 0x5a, dtype=torch.uint8, device=dev)
    rad = torch.empty(b, dtype=torch.int32, device=dev)
    code = IC.raw(L, planar.data_ptr(), (2 * h * w, w, 1, h * w), b, h, w, buf.data_ptr() + 1, rad.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    assert code == IC.PIO_OK
    torch.cuda.synchronize()
    assert bool((buf[:1] == 0x5a).all()) and bool((buf[1 + n:] == 0x5a).all())
    IC.check(buf[1:1 + n].view(b, h, w, 3).cpu().numpy(), IC.gen(name), what="raw entry, planar, odd output address")


def test_one_maximum_per_image(dev):
    """Radii x1, x50 and x0.01 in one batch: every image equals its own single-image call, and a batch-wide maximum (which
    tests/test_flow_image_host.py shows would recolour two of the three) is rejected by the rule."""
    import perceiverio_pytorch_amd as P
    f = device_flow("batch3", dev)
    img = P.flow_to_image(f)
    _check(img, "batch3", "batch3")
    for i in range(3):
        assert torch.equal(img[i], P.flow_to_image(f[i])), f"image {i} of the batch differs from its own call"


def test_permuted_view_is_read_in_place(dev, monkeypatch):
    import perceiverio_pytorch_amd as P
    calls = _counting(monkeypatch)
    chw = torch.from_numpy(np.array(IC.gen("permuted"))).to(dev)[0].permute(2, 0, 1).contiguous()
    _, h, w = chw.shape
    view = chw.permute(1, 2, 0)
    assert not view.is_contiguous()
    img = P.flow_to_image(view)
    a = calls["args"]
    assert calls["kernel"] == 1 and a[0] == chw.data_ptr() and tuple(a[2:5]) == (w, 1, h * w), "the view was copied"
    _check(img, "permuted", "permuted view")
    # ... and the model's batched layout
    f = torch.from_numpy(np.array(IC.gen("batch3"))).to(dev).permute(0, 3, 1, 2).contiguous()
    img = P.flow_to_image(f.permute(0, 2, 3, 1))
    a = calls["args"]
    assert calls["kernel"] == 2 and a[0] == f.data_ptr() and tuple(a[1:5]) == (2 * 17 * 40, 40, 1, 17 * 40)
    _check(img, "batch3", "batch3 as [b, 2, h, w]")


@pytest.mark.parametrize("name", ["33x130", "batch3", "big"])
def test_two_calls_give_identical_bytes(dev, name):
    assert torch.equal(run_public(name, dev), run_public(name, dev))


@pytest.mark.parametrize("what,ch,code", IC.REFUSALS, ids=[r[0] for r in IC.REFUSALS])
def test_refusals_leave_the_output_untouched(dev, what, ch, code):
    from perceiverio_pytorch_amd import _lib as L
    h, w = IC.R_H, IC.R_W
    f = torch.randn(h * w * 2 + 8, device=dev)
    out = torch.full((3 * h * w,), 0x5a, dtype=torch.uint8, device=dev)
    rad = torch.full((1,), -7, dtype=torch.int32, device=dev)
    got = IC.raw(L, None if "flow" in ch else f.data_ptr() + ch.get("flow_offset", 0), (2 * h * w, 2 * w, 2, 1),
                 ch.get("b", 1), ch.get("h", h), ch.get("w", w), None if "out" in ch else out.data_ptr(),
                 None if "rad" in ch else rad.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert got == code, (what, got)
    assert bool((out == 0x5a).all()) and int(rad[0]) == -7, f"{what}: a refused call wrote"


def test_the_valid_call_of_the_refusal_table_runs(dev):
    from perceiverio_pytorch_amd import _lib as L
    h, w = IC.R_H, IC.R_W
    f = torch.randn(1, h, w, 2, device=dev)
    out = torch.full((3 * h * w,), 0x5a, dtype=torch.uint8, device=dev)
    rad = torch.full((1,), -7, dtype=torch.int32, device=dev)
    assert IC.raw(L, f.data_ptr(), (2 * h * w, 2 * w, 2, 1), 1, h, w, out.data_ptr(), rad.data_ptr(),
                  torch.cuda.current_stream().cuda_stream) == IC.PIO_OK
    IC.check(out.view(1, h, w, 3).cpu().numpy(), f.cpu().numpy(), what="valid call")


@pytest.mark.parametrize("name", NAMES)
def test_switch_off_takes_the_restatement(dev, monkeypatch, name):
    import perceiverio_pytorch_amd as P
    calls = _counting(monkeypatch)
    monkeypatch.setattr(P, "fused_flow_image", False)
    img = run_public(name, dev)
    assert calls["kernel"] == 0
    _check(img, name, f"restatement on the device, {name}")


def test_other_inputs_take_the_restatement(dev, monkeypatch):
    """A float64 CUDA tensor (upcast is the restatement's) and a CPU tensor: no kernel call; a tensor through
    utils.flow_utils.flow_to_image: one."""
    import perceiverio_pytorch_amd as P
    calls = _counting(monkeypatch)
    f = device_flow("5x7", dev)
    _check(P.flow_to_image(f.double()), "5x7", "float64 on the device")
    assert P.flow_to_image(f.cpu()).device.type == "cpu" and calls["kernel"] == 0
    img = FU.flow_to_image(f[0])
    assert calls["kernel"] == 1 and isinstance(img, torch.Tensor) and img.device == f.device
    IC.check(img.cpu().numpy(), IC.gen("5x7")[0], what="utils.flow_utils on a CUDA tensor")


def test_capturable(dev):
    """No synchronisation, no host read: the call captures into a graph, and the replay follows the input."""
    import perceiverio_pytorch_amd as P
    f = device_flow("33x130", dev).clone()
    eager = P.flow_to_image(f)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = P.flow_to_image(f)
    f.copy_(f.flip(1) * 2.0)
    graph.replay()
    torch.cuda.synchronize()
    again = P.flow_to_image(f)
    assert torch.equal(captured, again) and not torch.equal(again, eager)


def test_small_flow_golden_forward_then_image(dev, monkeypatch):
    """model_flow_small under the default policy, then flow_to_image on the device result (the [b, 2, h, w] field seen as
    [b, h, w, 2]), against the numpy function on the same flow copied to the host, under the rule."""
    import perceiverio_pytorch_amd as P
    name = "model_flow_small"
    model = _load_generated(build(name), load(name), dev, model_seed(name), model_stats(name))
    ins = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]
    with torch.inference_mode():
        flow = model(ins[0], ins[1], test_mode=True, min_overlap=10)
        assert flow.shape == (1, 2, 60, 80) and flow.dtype == torch.float32
        calls = _counting(monkeypatch)
        img = P.flow_to_image(flow[0].permute(1, 2, 0))
    assert calls["kernel"] == 1 and calls["args"][0] == flow.data_ptr()
    host = flow[0].permute(1, 2, 0).cpu().numpy()
    want = FU.flow_to_image(host)
    got = img.cpu().numpy()
    IC.check(got, host, what="golden forward, kernel")
    IC.check(want, host, what="golden forward, numpy")
    c, white = IC.reference_c(host[None])
    lo, hi = IC.bounds(c)
    sure = (lo == hi)[0]
    assert np.array_equal(got[sure], want[sure]), "kernel and numpy differ outside the band"
    print(f"golden forward: {int((got != want).sum())} of {got.size} bytes differ from numpy's, all inside the band")
