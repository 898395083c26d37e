"""GPU: the flow front end -- pio_flow_patch_tokens through the raw C-ABI on every case of tests/flow_front_cases.py
against the float64 definition, the fused branch of ImagePreprocessor, and FlowPerceiver.fused_front_end on the goldens.

Bound (derived, not measured): |y - ref| <= (K + 1) 2^-24 (sum_k |w_k x_k| + |b|), K = 18 C -- K fp32 FMAs in any order;
the raw form (w == NULL) only moves values and must be exact.

Memory safety by construction: the output sits between 4 KiB guard bands and is NaN before the call, its ldy gaps must
still be NaN afterwards; every frame is a region of a larger image that is NaN outside it, and every output must be
finite -- a halo that reads one cell outside the image, even to multiply it by zero, shows."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_front_cases as FC  # noqa: E402
from test_flow_front_host import make_prep  # noqa: E402
from test_models import TOL, _close, _load_generated, build  # noqa: E402
from _golden import load  # noqa: E402
from cases import model_inputs, model_seed, model_stats  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


_REF = {}


def case_data(name):
    """(inputs, definition, error scale) of a case, computed once and shared (read-only) by the tests below."""
    if name not in _REF:
        d = FC.gen(name)
        _REF[name] = (d,) + FC.reference(d)
    return _REF[name]


class GuardedOut:
    """guard | rows x ldy fp32 | guard in one device allocation; the payload is NaN, the guards a fixed byte pattern."""

    def __init__(self, dev, rows, ldy):
        self.n = rows * ldy * 4
        self.pattern = ((torch.arange(GUARD, dtype=torch.int64) * 37 + 11) % 251).to(torch.uint8).to(dev)
        self.buf = torch.empty(GUARD + self.n + GUARD, dtype=torch.uint8, device=dev)
        self.buf[:GUARD] = self.pattern
        self.buf[GUARD + self.n:] = self.pattern
        self.t = self.buf[GUARD:GUARD + self.n].view(torch.float32).view(rows, ldy)
        self.t.fill_(float("nan"))

    def check(self, what):
        torch.cuda.synchronize()
        assert torch.equal(self.buf[:GUARD], self.pattern), f"{what}: bytes in FRONT of the output were written"
        assert torch.equal(self.buf[GUARD + self.n:], self.pattern), f"{what}: bytes BEHIND the output were written"


def launch(dev, name, d, swap=False):
    """One call of the raw entry on the case's NaN-surrounded frames; returns the guarded output [N H W, ldy]."""
    from perceiverio_pytorch_amd import _lib as L
    c = FC.CASES[name]
    keep, fr = [], []
    for t in range(2):
        img = torch.from_numpy(d["full"][t]).to(dev)
        oy, ox = c["origin"][t]
        hf, wf = c["full"][t]
        keep.append(img)
        fr.append((img.data_ptr() + 4 * (oy * wf + ox), c["C"] * hf * wf, hf * wf, wf))
    if swap:
        fr = fr[::-1]
    w = None if d["w"] is None else torch.from_numpy(d["w"]).to(dev)
    b = None if d["bias"] is None else torch.from_numpy(d["bias"]).to(dev)
    y = GuardedOut(dev, c["N"] * c["H"] * c["W"], c["ldy"])
    code = L.lib().pio_flow_patch_tokens(fr[0][0], fr[1][0], *fr[0][1:], *fr[1][1:], None if w is None else w.data_ptr(),
                                         None if b is None else b.data_ptr(), y.t.data_ptr(), c["ldy"], c["N"], c["C"],
                                         c["H"], c["W"], c["out"], torch.cuda.current_stream().cuda_stream)
    L.check(code, f"pio_flow_patch_tokens[{name}]")
    y.check(name)
    return y


def assert_within_bound(got, ref, mag, C, what):
    """got [.., out] fp32 (any device) against the float64 definition: element-wise derived bound, exact where mag == 0."""
    got = got.detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite outputs (a read outside the image?)"
    err, bnd = np.abs(got - ref), FC.bound(C, mag)
    ratio = float((err / np.where(bnd > 0, bnd, 1.0))[bnd > 0].max()) if (bnd > 0).any() else 0.0
    print(f"{what}: max |y - ref| = {err.max():.3e}, worst |y - ref| / bound = {ratio:.3f}")
    bad = err > bnd
    if bad.any():
        i = np.unravel_index(np.argmax(err - bnd), err.shape)
        raise AssertionError(f"{what}: element {i}: got {got[i]!r} ref {ref[i]!r} err {err[i]:.3e} bound {bnd[i]:.3e}")


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_raw_entry_against_the_definition(dev, name):
    c = FC.CASES[name]
    d, ref, mag = case_data(name)
    y = launch(dev, name, d)
    out = c["out"]
    assert torch.isnan(y.t[:, out:]).all(), f"{name}: the ldy gap [{out}, {c['ldy']}) was written"
    assert_within_bound(y.t[:, :out], ref, mag, c["C"], name)
    if c["raw"]:
        assert np.array_equal(y.t[:, :out].cpu().numpy().astype(np.float64).reshape(ref.shape), ref)
    # run to run: equal bits
    y2 = launch(dev, name, d)
    assert torch.equal(y.t[:, :out].view(torch.int32), y2.t[:, :out].view(torch.int32)), f"{name}: two launches differ"


def test_frame_order_matters(dev):
    d, ref, mag = case_data("odd")
    y, ys = launch(dev, "odd", d), launch(dev, "odd", d, swap=True)
    assert not torch.equal(y.t, ys.t)
    swapped = dict(d, frames=d["frames"][::-1])
    ref_s, mag_s = FC.reference(swapped)
    assert_within_bound(ys.t, ref_s, mag_s, 3, "odd, frames swapped")


@pytest.mark.parametrize("what,changes,code", FC.REFUSALS, ids=[r[0] for r in FC.REFUSALS])
def test_refusals_launch_nothing(dev, what, changes, code):
    from perceiverio_pytorch_amd import _lib as L
    v = FC.VALID
    frames = torch.randn(2, v["N"], v["C"], v["H"], v["W"], device=dev)
    w = torch.randn(v["out"], 18 * v["C"], device=dev)
    b = torch.randn(v["out"], device=dev)
    y = GuardedOut(dev, v["N"] * v["H"] * v["W"] + 1, v["ldy"])       # (+1 row: room for the moved pointer)
    ptrs = dict(frame0=frames[0].data_ptr(), frame1=frames[1].data_ptr(), w=w.data_ptr(), bias=b.data_ptr(),
                y=y.t.data_ptr())
    assert FC.refusal_call(L.lib(), ptrs, changes, torch.cuda.current_stream().cuda_stream) == code
    y.check(what)
    assert torch.isnan(y.t).all(), f"{what}: a refused call wrote to y"


@pytest.mark.parametrize("conv", [True, False], ids=["conv_after_patching", "raw_patches"])
@pytest.mark.parametrize("name", ["odd", "train"])
def test_image_preprocessor_fused_branch(dev, name, conv):
    """ImagePreprocessor on a raw CUDA frame pair (the fused branch) against the float64 definition, next to its own
    torch path on the patched frames (printed: the BLAS call behind it is not the code under test); forward and
    forward_split hand over the same features."""
    from perceiverio_pytorch_amd.io_processors import patches_for_flow
    base = FC.CASES[name]
    case = base if conv else dict(base, raw=True, out=18 * base["C"])
    d, ref_y, mag_y = case_data(name)
    if conv:
        ref, mag = ref_y, mag_y
    else:
        d = dict(d, w=None, bias=None)
        ref, mag = FC.reference(d)
    prep = make_prep(case, d, torch.float32).to(dev)
    pair = torch.stack([torch.from_numpy(f) for f in d["frames"]], dim=1).to(dev)
    feats = prep._features(pair)
    assert feats.shape == ref.shape
    assert_within_bound(feats, ref, mag, case["C"], f"{name} fused, conv={conv}")
    torch_path = prep._features(patches_for_flow(pair).movedim(-1, -3))
    diff = float((feats - torch_path).abs().max())
    print(f"{name} conv={conv}: max |fused - torch path| = {diff:.3e}")
    if not conv:
        assert diff == 0.0          # both paths only move values
    with_pos, without_pos = prep(pair)
    split = prep.forward_split(pair)
    assert torch.equal(without_pos, feats)
    assert torch.equal(split[1] if split[0] == "split" else split[2], feats)
    assert torch.equal(with_pos[..., :feats.shape[-1]], feats)


def _counting_patches(monkeypatch):
    from perceiverio_pytorch_amd import io_processors as IO
    real, calls = IO.patches_for_flow, []
    monkeypatch.setattr(IO, "patches_for_flow", lambda x: (calls.append(tuple(x.shape)), real(x))[1])
    return calls


def test_flow_perceiver_small_golden_fused_on_and_off(dev, monkeypatch):
    """The committed small flow golden (48 x 64 training size; 60 x 80 frames tiled) with fused_front_end on and off:
    both within TOL of the reference; on, patches_for_flow is never called; off, it is.  The on / off difference is
    printed (fp32 summation order of the 54 -> 64 projection, seen through the network)."""
    name = "model_flow_small"
    g = load(name)
    model = _load_generated(build(name), g, dev, model_seed(name), model_stats(name))
    assert model.fused_front_end is True
    ins = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]
    calls = _counting_patches(monkeypatch)
    outs = {}
    for on in (True, False):
        model.fused_front_end = on
        del calls[:]
        with torch.inference_mode():
            y_train = model(ins[0][..., :48, :64], ins[1][..., :48, :64])
            y_test = model(ins[0], ins[1], test_mode=True, min_overlap=10)
        _close(y_train, g["out_train"], f"{name} train, fused={on}", TOL)
        _close(y_test, g["out_test"], f"{name} tiled, fused={on}", TOL)
        assert (len(calls) == 0) if on else (len(calls) >= 2), (on, calls)
        outs[on] = (y_train, y_test)
    for i, what in enumerate(("train", "tiled")):
        print(f"{name} {what}: max |fused on - off| = {float((outs[True][i] - outs[False][i]).abs().max()):.3e}")


def test_flow_perceiver_full_size_fused_front_end(dev, monkeypatch):
    """model_flow_full with fused_front_end on: the whole field finite, the 8x sub-sampled grid within TOL, and the last
    image row and column -- the last decoder row, pixel (367, 495), among them -- against the reference values of
    tests/golden/model_flow_full_edge.npz (tools/flow_last_pixel_golden.py)."""
    name = "model_flow_full"
    g, edge = load(name), load(name + "_edge")
    model = _load_generated(build(name), g, dev, model_seed(name), model_stats(name))
    assert model.fused_front_end is True
    ins = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]
    calls = _counting_patches(monkeypatch)
    with torch.inference_mode():
        y = model(ins[0], ins[1])
    assert calls == []
    assert y.shape == (1, 2, 368, 496)
    assert bool(torch.isfinite(y).all()), "non-finite flow values"
    am = g["out_absmax"]
    _close(y[:, :, ::8, ::8], g["out_sub"], name + " fused, 8x grid", TOL, absmax=am)
    # (one compared set, so that relL2 keeps the meaning it has on the grid: error over the magnitude of the FIELD, not
    #  of one image row)
    pts = torch.cat([y[:, :, ::8, ::8].reshape(1, 2, -1), y[:, :, 367, :], y[:, :, :, 495]], dim=2)
    ref = np.concatenate([g["out_sub"].reshape(1, 2, -1), edge["out_last_row"], edge["out_last_col"]], axis=2)
    _close(pts, ref, name + " fused, 8x grid + last row + last column", TOL, absmax=am)
    last = (y[0, :, 367, 495].cpu().numpy().astype(np.float64) - edge["out_last_row"][0, :, 495]) / float(am)
    print(f"{name} fused, pixel (367, 495): (y - ref) / absmax = {last}")
    assert np.abs(last).max() <= TOL
