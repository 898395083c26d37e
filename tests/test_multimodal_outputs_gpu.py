"""GPU: the output side of the models -- MultiModalPerceiver.classify and .reconstruct on the committed small multimodal golden,
ClassificationPerceiver.classify on model_classify_conv, and top_labels through pio_vocab_topk's selection mode.

classify's logits are held to the project's TOL (tests/test_models.py, both measures of _close) against the REFERENCE label
of the golden and against this build's forward()["label"]: the label is one decoder row, forward averages one estimate of it
per chunk.  Everything behind the logits is equality."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_models import TOL, _close, _load_generated, build  # noqa: E402
from _golden import load  # noqa: E402
from cases import model_inputs, model_seed, model_stats  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def small(dev):
    """(name, golden, model, inputs, forward's outputs): the forward computed once and shared (read-only)."""
    name = "model_multimodal_small"
    g = load(name)
    model = _load_generated(build(name), g, dev, model_seed(name), model_stats(name))
    ins = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]
    with torch.inference_mode():
        out = model(ins[0], ins[1], n_chunks=2)
    return name, g, model, ins, out


def _launches(monkeypatch):
    """Names of the C-ABI entries called through runtime.call, in order."""
    from perceiverio_pytorch_amd import runtime as R
    names, real = [], R.call

    def call(dev, name, *args, **kw):
        names.append((name, args))
        return real(dev, name, *args, **kw)
    monkeypatch.setattr(R, "call", call)
    return names


# fp32 probabilities against a float64 softmax: logit - lse carries the rounding of lse = m + log(S) and of the subtraction,
# a few ulp of the largest |logit| (below 16 here: ulp 1.9e-6) in all; four of them, relative to a probability of at most 1
PROB_TOL = 4 * 2.0 ** -19


def test_top_labels_is_the_kernels_selection(dev, monkeypatch):
    import perceiverio_pytorch_amd as P
    names = _launches(monkeypatch)
    g = torch.Generator().manual_seed(8)
    logits = (torch.randn((3, 2, 700), generator=g) * 3).to(dev)
    logits[1, 1, 5:9] = logits[1, 1].max() + 1.0                                # four equal logits on top
    assert float(logits.abs().max()) < 16.0
    ids, probs = P.top_labels(logits)
    assert [n for n, _ in names] == ["pio_vocab_topk"]
    assert ids.dtype == torch.int64 and probs.dtype == torch.float32 and tuple(ids.shape) == tuple(probs.shape) == (3, 2, 5)
    assert ids[1, 1].tolist()[:4] == [5, 6, 7, 8], "equal logits: the lower id first"
    want = torch.log_softmax(logits.double(), dim=-1).exp()
    assert float((probs.double() - want.gather(-1, ids)).abs().max()) <= PROB_TOL
    rest = want.scatter(-1, ids, -1.0)
    assert bool((probs.double()[..., -1:] + PROB_TOL >= rest.max(dim=-1, keepdim=True).values).all())
    assert bool((probs[..., :-1] >= probs[..., 1:]).all())
    # beyond the kernel's sizes and on the host: the torch path, the same order
    del names[:]
    big_ids, big_probs = P.top_labels(logits, k=9)
    wide = P.top_labels(torch.cat([logits, logits - 50.0], dim=-1))
    cpu_ids, cpu_probs = P.top_labels(logits.cpu())
    assert not names
    assert torch.equal(big_ids[..., :5], ids) and torch.equal(wide[0], ids) and torch.equal(cpu_ids, ids.cpu())
    assert float((cpu_probs - probs.cpu()).abs().max()) <= PROB_TOL and float((big_probs[..., :5] - probs).abs().max()) <= PROB_TOL


def test_classify_on_the_small_golden(dev, small, monkeypatch):
    import perceiverio_pytorch_amd as P
    name, g, model, ins, out = small
    core = model.perceiver
    held = len(model._packed)
    names = _launches(monkeypatch)
    seen = []
    real = core._decoder.forward
    core._decoder.forward = lambda q, *a, **k: (seen.append(tuple(q.shape)), real(q, *a, **k))[1]
    try:
        with torch.inference_mode():
            lab = model.classify(ins[0], ins[1], k=5, return_logits=True)
    finally:
        del core._decoder.forward
    assert seen == [(2, 1, core.query_channels)], f"the decoder ran {len(seen)} times on {seen}"
    called = [n for n, _ in names]
    assert "pio_build_queries" not in called and "pio_project_heads" not in called and called.count("pio_decoder_fwd") == 1
    assert called[-1] == "pio_vocab_topk" and len(model._packed) == held, "classify left a query cache entry"
    assert tuple(lab.logits.shape) == (2, 10) and lab.logits.dtype == torch.float32
    _close(lab.logits, g["out_label"], f"{name} classify vs the reference label", TOL)
    _close(lab.logits, out["label"].cpu().numpy(), f"{name} classify vs forward's label", TOL)
    ids, probs = P.top_labels(lab.logits, 5)
    assert torch.equal(lab.ids, ids) and torch.equal(lab.probs, probs)
    assert tuple(lab.ids.shape) == (2, 5) and lab.ids.dtype == torch.int64
    assert torch.equal(lab.ids[:, 0], lab.logits.argmax(dim=-1))
    with torch.inference_mode():
        bare = model.classify(ins[0], ins[1], k=3)
    assert bare.logits is None and torch.equal(bare.ids, lab.ids[:, :3])


def test_forward_is_unchanged_by_classify(dev, small):
    name, g, model, ins, out = small
    with torch.inference_mode():
        model.classify(ins[0], ins[1])
        again = model(ins[0], ins[1], n_chunks=2)
    for m in ("image", "audio", "label"):
        assert torch.equal(again[m], out[m]), f"{m}: forward after classify differs from forward before it"
        _close(again[m], g[f"out_{m}"], f"{name} {m} after classify", TOL)


def test_reconstruct_is_forward_plus_two_launches(dev, small, monkeypatch):
    import perceiverio_pytorch_amd as P
    name, g, model, ins, out = small
    names = _launches(monkeypatch)
    with torch.inference_mode():
        rec = model.reconstruct(ins[0], ins[1], n_chunks=2, bgr=True)
    media = [a for n, a in names if n == "pio_finish_media"]
    assert len(media) == 2
    b, t, c, h, w = out["image"].shape
    # the image view read in place: b*t adjacent images behind the view's own pointer (a fresh forward: not `out`'s)
    assert tuple(media[0][1:5]) == (h * w * c, w * c, c, 1) and tuple(media[0][5:9]) == (b * t, h, w, c)
    assert tuple(rec.frames.shape) == (b, t, h, w, c) and rec.frames.dtype == torch.uint8
    assert rec.pcm.shape == ins[1].shape and rec.pcm.dtype == torch.int16
    assert torch.equal(rec.frames, P.to_frames(out["image"], bgr=True, channels_first=True))
    assert torch.equal(rec.frames, P.to_frames(out["image"], bgr=True))          # (inferred: 3 <= 4 < 16)
    assert torch.equal(rec.pcm, P.to_pcm16(out["audio"]))
    assert torch.equal(rec.label, out["label"])
    with torch.inference_mode():
        rgb = model.reconstruct(ins[0], ins[1], n_chunks=2)
    assert torch.equal(rgb.frames, rec.frames.flip(-1))


def test_classifier_classify_decodes_row_0_and_restores(dev, monkeypatch):
    import perceiverio_pytorch_amd as P
    name = "model_classify_conv"
    g = load(name)
    model = _load_generated(build(name), g, dev)
    x = torch.from_numpy(model_inputs(name)[0]).to(dev)
    core = model.perceiver
    seen = []
    real = core._decoder.forward
    core._decoder.forward = lambda q, *a, **k: (seen.append(tuple(q.shape)), real(q, *a, **k))[1]
    try:
        assert model.decode_row0_only is False
        with torch.inference_mode():
            lab = model.classify(x, k=5, return_logits=True)
        assert model.decode_row0_only is False and core.decoder_query_rows is None
        assert [s[:2] for s in seen] == [(2, 1)]
        _close(lab.logits, g["out"], f"{name} classify vs the reference", TOL)
        ids, probs = P.top_labels(lab.logits, 5)
        assert torch.equal(lab.ids, ids) and torch.equal(lab.probs, probs) and tuple(ids.shape) == (2, 5)
        assert torch.equal(lab.ids[:, 0], lab.logits.argmax(dim=-1))
        # restored when the forward raises, whichever way the setting stood
        for on in (False, True):
            model.decode_row0_only = on
            with pytest.raises(Exception):
                model.classify(x[:, :, 0], k=5)
            assert model.decode_row0_only is on
    finally:
        del core._decoder.forward
