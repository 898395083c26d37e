"""GPU: the 1x1-conv and pixel front ends of the classifier -- pio_conv1x1_tokens through the raw C-ABI: exact addressing on
every shape and source of tests/conv1x1_cases.py (bit for bit), guard bands, accuracy against the float64 definition within
gamma_{C+1} (|bias| + sum |w x|), independence of a sample's bits from the batch around it; the module (features from the
kernel, the projected table handed to the encoder next to them, the switch); the pixel variant (one pio_assemble_tokens call,
the chain's bits); the two full-size goldens with the switch on and off; one stream capture.

Memory safety by construction: every output is carved from a larger sentinel-filled allocation with rows in front of and
behind it and a pitch wider than N, and every word outside the [B, M, N] values must still be the sentinel; batch-sliced
sources are surrounded by NaN, so a pixel read from the wrong place shows."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv1x1_cases as CC  # noqa: E402
from test_conv1x1_front_host import make_prep  # noqa: E402
from test_models import TOL, _close, _load_generated, build  # noqa: E402
from _golden import load  # noqa: E402
from cases import model_inputs, model_seed, model_stats  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5       # a NaN with a payload, as int32
GUARD_ROWS = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


def source(kind, x, dev):
    """(view [B, C, H, W] on the device laid out as `kind` says, the pixels it shows as numpy, what keeps it alive)."""
    b, c, h, w = x.shape
    if kind == "contiguous":
        t = torch.from_numpy(x).to(dev)
        return t, x, t
    if kind == "channels_last":
        buf = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).to(dev)
        return buf.permute(0, 3, 1, 2), x, buf
    if kind == "batch_slice":
        big = torch.full((2 * b + 1, c + 1, h + 2, w + 3), float("nan"), device=dev)
        view = big[1::2, 1:, 1:h + 1, 2:w + 2]
        view.copy_(torch.from_numpy(x).to(dev))
        return view, x, big
    if kind == "offset_one":
        flat = torch.full((x.size + 1,), float("nan"), device=dev)
        view = flat[1:].view(b, c, h, w)
        view.copy_(torch.from_numpy(x).to(dev))
        assert view.data_ptr() % 16 == 4
        return view, x, flat
    assert kind == "stride0_batch"
    one = torch.from_numpy(x[:1]).to(dev)
    return one.expand(b, c, h, w), np.broadcast_to(x[:1], x.shape), one


def launch(dev, view, w, bias, s, pad=4):
    """One call of the raw entry into a guarded output with row pitch N + pad and GUARD_ROWS sentinel rows in front of, between
    (B > 1) and behind the samples; returns y [B, M, N] as int32 bits after checking every other word."""
    from perceiverio_pytorch_amd import _lib as L
    b, c, h, wd = view.shape
    n, m = w.shape[0], (h // s) * (wd // s)
    ldy = n + pad
    syb = (m + GUARD_ROWS) * ldy
    total = GUARD_ROWS * ldy + b * syb
    buf = torch.full((total,), SENTINEL, dtype=torch.int32, device=dev)
    y0 = buf[GUARD_ROWS * ldy:]
    assert y0.data_ptr() % 16 == 0 and ldy % 4 == 0
    wt = torch.from_numpy(w).to(dev)
    bt = None if bias is None else torch.from_numpy(bias).to(dev)
    code = L.lib().pio_conv1x1_tokens(view.data_ptr(), *view.stride(), wt.data_ptr(), wt.stride(0),
                                      None if bt is None else bt.data_ptr(), y0.data_ptr(), ldy, syb, b, c, h, wd, s, n,
                                      torch.cuda.current_stream().cuda_stream)
    L.check(code, "pio_conv1x1_tokens")
    torch.cuda.synchronize()
    body = y0.view(b, m + GUARD_ROWS, ldy)
    y = body[:, :m, :n].clone()
    written = torch.zeros_like(buf, dtype=torch.bool)
    written[GUARD_ROWS * ldy:].view(b, m + GUARD_ROWS, ldy)[:, :m, :n] = True
    assert bool((buf[~written] == SENTINEL).all()), "a word outside the [B, M, N] values was written"
    return y


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("kind", CC.SOURCES)
@pytest.mark.parametrize("shape", CC.EXACT_SHAPES, ids=["x".join(map(str, s)) for s in CC.EXACT_SHAPES])
def test_exact_addressing(dev, shape, kind):
    b, c, h, w, s, n = shape
    wt, bias = CC.exact_params(c, n)
    view, shown, keep = source(kind, CC.exact_pixels(b, c, h, w), dev)
    y = launch(dev, view, wt, bias, s)
    want = CC.exact_expected(shown, s, n)
    assert np.array_equal(y.cpu().numpy(), bits(want)), f"{shape} {kind}"


@pytest.mark.parametrize("shape", [CC.EXACT_SHAPES[0], CC.EXACT_SHAPES[4]], ids=["2x3x5x7x1x8", "2x3x3x67x1x256"])
def test_no_bias(dev, shape):
    b, c, h, w, s, n = shape
    wt, _ = CC.exact_params(c, n)
    x = CC.exact_pixels(b, c, h, w)
    y = launch(dev, source("contiguous", x, dev)[0], wt, None, s)
    want = CC.exact_expected(x, s, n) - np.arange(n, dtype=np.float32)[None, None, :]
    assert np.array_equal(y.cpu().numpy(), bits(want))


def test_guard_bands_with_wide_pitches(dev):
    """The pitch gap, the rows between the samples and the rows around the array stay as they were (launch checks every
    word), for a pitch far wider than N and for the narrowest one the entry takes."""
    b, c, h, w, s, n = 3, 3, 5, 67, 1, 12
    wt, bias = CC.exact_params(c, n)
    x = CC.exact_pixels(b, c, h, w)
    want = bits(CC.exact_expected(x, s, n))
    for pad in (0, 4, 52):
        y = launch(dev, source("batch_slice", x, dev)[0], wt, bias, s, pad=pad)
        assert np.array_equal(y.cpu().numpy(), want), pad


@pytest.mark.parametrize("kind,shape", CC.ACCURACY_CASES, ids=[f"{k}-" + "x".join(map(str, s)) for k, s in CC.ACCURACY_CASES])
def test_accuracy_against_the_float64_definition(dev, kind, shape):
    """|y - definition| <= gamma_{C+1} (|bias| + sum |w x|): the bound any order of C fused multiply-adds plus the bias term
    satisfies.  Worst ratio to that bound seen on an MI355X over these cases: 0.64 (README)."""
    c, s = shape[1], shape[4]
    worst = 0.0
    for seed, with_bias in ((1, True), (2, False)):
        x, w, bias = CC.accuracy_data(kind, shape, seed)
        bias = bias if with_bias else None
        ref, mag = CC.reference(x, w, bias, s)
        y = launch(dev, source("contiguous", x, dev)[0], w, bias, s).view(torch.float32).cpu().numpy().astype(np.float64)
        assert np.isfinite(y).all()
        bound = CC.gamma(c + 1) * mag
        err = np.abs(y - ref)
        assert (err[mag == 0.0] == 0.0).all()
        ratio = float((err[mag > 0.0] / bound[mag > 0.0]).max())
        worst = max(worst, ratio)
        print(f"{kind} {shape} bias={with_bias}: worst |err| / bound = {ratio:.3f}")
        assert ratio <= 1.0
    print(f"{kind} {shape}: worst ratio {worst:.3f}")


def test_a_samples_bits_do_not_depend_on_the_batch(dev):
    shape = (3, 3, 5, 71, 1, 256)
    x, w, bias = CC.accuracy_data("image", shape, 5)
    alone = launch(dev, source("contiguous", x[2:3], dev)[0], w, bias, 1)
    batch = launch(dev, source("contiguous", x, dev)[0], w, bias, 1)
    sliced = launch(dev, source("batch_slice", x[1:], dev)[0], w, bias, 1)
    assert torch.equal(alone[0], batch[2]) and torch.equal(alone[0], sliced[1])
    again = launch(dev, source("channels_last", x, dev)[0], w, bias, 1)
    assert torch.equal(batch, again)


# ---------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------
def small_io(prep):
    from perceiverio_pytorch_amd.output_queries import TrainableQuery
    from perceiverio_pytorch_amd.perceiver import PerceiverIO
    return PerceiverIO(num_blocks=1, num_self_attends_per_block=1, num_latents=8, num_latent_channels=64,
                       input_preprocessors=prep, final_project_out_channels=5,
                       perceiver_encoder_kwargs=dict(num_self_attend_heads=2, num_cross_attend_heads=1),
                       output_queries=TrainableQuery(output_index_dims=4, num_channels=64))


def spy_encoder(io, seen):
    real = io._encoder.forward

    def forward(inputs, *a, **k):
        seen.append(inputs)
        return real(inputs, *a, **k)
    io._encoder.forward = forward


def test_module_hands_the_encoder_features_and_the_projected_table(dev):
    torch.manual_seed(21)
    prep = make_prep(c=3, n=8, s=1, hw=(6, 10), pos=8, trainable=True)
    with torch.no_grad():
        prep.convnet_1x1.bias.normal_(0.0, 0.1)
        prep._positional_encoding._projector.bias.normal_(0.0, 0.1)
    io = small_io(prep).to(dev).eval()
    x = torch.randn(3, 3, 6, 10, device=dev)
    seen = []
    spy_encoder(io, seen)
    conv, enc = prep.convnet_1x1, prep._positional_encoding
    with torch.inference_mode():
        y_on = io(x)
        assert len(seen) == 1 and isinstance(seen[0], tuple) and len(seen[0]) == 2
        feats, table = seen[0]
        assert tuple(feats.shape) == (3, 60, 8) and tuple(table.shape) == (60, 8) and table.is_contiguous()
        # the features are the kernel's
        w = conv.weight.detach().reshape(8, 3).cpu().numpy()
        raw = launch(dev, x, w, conv.bias.detach().cpu().numpy(), 1)
        assert torch.equal(feats.view(torch.int32), raw)
        # the table is one fp32 linear of the [M, .] base table, within gamma_{K+1} (|b| + sum |w p|) of float64
        p64 = enc._base_position_encoding.pos_embs.detach().double().cpu().numpy()
        w64 = enc._projector.weight.detach().double().cpu().numpy()
        b64 = enc._projector.bias.detach().double().cpu().numpy()
        ref = p64 @ w64.T + b64
        bound = CC.gamma(8 + 1) * (np.abs(p64) @ np.abs(w64).T + np.abs(b64))
        err = np.abs(table.double().cpu().numpy() - ref)
        print(f"projected table: worst |err| / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        assert io(x) is not None and seen[1][1] is table                 # built once
        # the switch off: one concatenated tensor, the chain's bits
        prep.fused_conv1x1 = False
        y_off = io(x)
        assert isinstance(seen[2], torch.Tensor) and tuple(seen[2].shape) == (3, 60, 16)
        chain = torch.cat([conv(x).movedim(-3, -1).reshape(3, 60, 8), enc(3, None, device=dev)], dim=-1)
        assert torch.equal(seen[2], chain)
        io.split_encoder_input = False
        y_plain = io(x)
        assert torch.equal(y_off, y_plain)
    assert tuple(y_on.shape) == tuple(y_off.shape) and bool(torch.isfinite(y_on).all())
    # same network, two hand-offs: the fused features differ from MIOpen's by rounding only
    assert float((y_on - y_off).abs().max()) <= 2e-2 * float(y_off.abs().max())


def test_pixel_variant_is_one_assemble_call_and_the_chains_bits(dev, monkeypatch):
    from perceiverio_pytorch_amd import runtime as R
    prep = make_prep(c=3, prep_type="pixels", project_pos_dim=-1, trainable=False).to(dev).eval()
    x = torch.randn(2, 3, 6, 10, device=dev)
    names = []
    real = R.call

    def call(d, name, *a, **k):
        names.append(name)
        return real(d, name, *a, **k)
    monkeypatch.setattr(R, "call", call)
    with torch.inference_mode():
        kind_on, full_on, wo_on = prep.forward_split(x)
        assert names == ["pio_assemble_tokens"]
        prep.fused_pixels = False
        kind_off, full_off, wo_off = prep.forward_split(x)
        assert names == ["pio_assemble_tokens"]
        prep.fused_pixels = True            # (a channels-last image: the same rows)
        kind_cl, full_cl, wo_cl = prep.forward_split(x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    assert kind_on == kind_off == kind_cl == "full" and tuple(full_on.shape) == (2, 60, 17)
    assert torch.equal(full_on.view(torch.int32), full_off.view(torch.int32))
    assert torch.equal(wo_on.contiguous().view(torch.int32), wo_off.contiguous().view(torch.int32))
    assert torch.equal(full_cl, full_off) and torch.equal(wo_cl, wo_off)
    assert wo_on.data_ptr() == full_on.data_ptr() and tuple(wo_on.shape) == (2, 60, 3)


@pytest.mark.parametrize("name", ["model_classify_1x1", "model_classify_pixel"])
def test_full_size_goldens_with_the_switch_on_and_off(dev, name):
    g = load(name)
    model = _load_generated(build(name), g, dev, model_seed(name), model_stats(name))
    from perceiverio_pytorch_amd.models import DEFAULT_POLICY
    assert model.precision_policy == DEFAULT_POLICY["ClassificationPerceiver"] and model.fused_front_end is True
    x = torch.from_numpy(model_inputs(name)[0]).to(dev)
    seen, outs, first = [], {}, {}
    spy_encoder(model.perceiver, seen)
    for on in (True, False):
        model.fused_front_end = on
        del seen[:]
        with torch.inference_mode():
            outs[on] = model(x)
        first[on] = seen[0]
        _close(outs[on], g["out"], f"{name}, fused_front_end={on}", TOL)
    if name == "model_classify_pixel":
        assert isinstance(first[True], torch.Tensor) and torch.equal(first[True], first[False])
        assert torch.equal(outs[True], outs[False])
    else:
        prep = model.perceiver._multi_preprocessor._preprocessors["__default"]
        cached = prep._packed.held("pos_table")[1]
        assert isinstance(first[True], tuple) and first[True][1] is cached
        assert tuple(first[True][0].shape) == (x.shape[0], 50176, 256) and tuple(cached.shape) == (50176, 256)
        if x.shape[0] > 1:
            assert isinstance(first[False], torch.Tensor) and tuple(first[False].shape) == (x.shape[0], 50176, 512)
        else:       # (one sample: the chain's projected positions are one table as they stand, and were split before)
            assert isinstance(first[False], tuple) and first[False][1] is not cached


def test_forward_split_in_a_graph(dev):
    """No allocation of the library's own, no synchronisation: after one warm-up call (the table exists) the 1x1
    preprocessor's forward_split captures into a graph, and a replay on a new image equals the eager result."""
    torch.manual_seed(23)
    prep = make_prep(c=3, n=8, s=1, hw=(6, 10), pos=8, trainable=True).to(dev).eval()
    x = torch.randn(2, 3, 6, 10, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        prep.forward_split(x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad():
        with torch.cuda.graph(g):
            kind, feats_g, table_g = prep.forward_split(x)
        new = torch.randn(2, 3, 6, 10, device=dev)
        x.copy_(new)
        g.replay()
        torch.cuda.synchronize()
        kind_e, feats, table = prep.forward_split(new)
    assert kind == kind_e == "split" and table_g is table
    assert torch.equal(feats_g.view(torch.int32), feats.view(torch.int32))
