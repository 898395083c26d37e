"""CPU: the media samples and the labels without a GPU -- tests/media_cases.py against itself (its definition equals the
example's numpy expressions wherever those are defined, its layouts hold the arrays they say), media.restatement against
both bit for bit, the documented NaN and saturation values, shape and layout inference of to_frames / to_pcm16, and
top_labels / classify / reconstruct under the torch backend against log_softmax + topk, equal logits included."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import media_cases as MC  # noqa: E402

NAMES = sorted(MC.CASES)


@pytest.fixture()
def torch_backend():
    import perceiverio_pytorch_amd as P
    prev = P.get_backend()
    P.set_backend("torch")
    yield P
    P.set_backend(prev)


def test_cases_cover_what_they_claim():
    pixels = {int(np.prod(c["shape"][:3])) for c in MC.CASES.values()}
    assert {1, 3, 4, 5, 1027} <= pixels
    for kind in (MC.U8, MC.S16):
        mine = [c for c in MC.CASES.values() if c["kind"] == kind]
        assert {c["shape"][3] for c in mine} >= {1, 3, 4}
        assert {c["shape"][0] for c in mine} >= {1, 3}
        assert {c.get("layout", "flat") for c in mine} >= {"flat", "batch_gap", "chw", "crop"}
        assert any(c["shape"][2] == 1 for c in mine)
    assert {o for offs in MC.Y_OFFSETS.values() for o in offs} >= {0, 1, 2}
    # every special value is in some case
    for kind, special in ((MC.U8, MC.u8_values()), (MC.S16, MC.s16_values())):
        big = max((n for n in NAMES if MC.kind_of(n) == kind), key=lambda n: MC.gen(n).size)
        assert np.array_equal(MC.gen(big).reshape(-1)[:len(special)].view(np.int32), special.view(np.int32))


def test_named_values_of_the_definition():
    one = np.float32(1)
    below = np.nextafter(one, np.float32(0))
    a = np.array([-0.0, 0.0, 1e-40, below, 1.0, one + MC.ULP1, -2.0, 1e30, np.inf, -np.inf, np.nan, 0.5], np.float32)
    assert MC.definition(a, MC.U8).tolist() == [0, 0, 0, 254, 255, 255, 0, 255, 255, 0, 0, 127]
    s = np.array([0.0, -0.0, 1.0, -1.0, -one - MC.ULP1, 32767.0 / 32768, 32767.5 / 32768, one + MC.ULP1, np.inf, -np.inf,
                  np.nan, -0.9 / 32768, 0.5], np.float32)
    assert MC.definition(s, MC.S16).tolist() == [0, 0, 32767, -32768, -32768, 32767, 32767, 32767, 32767, -32768, 0, 0, 16384]


@pytest.mark.parametrize("name", NAMES)
def test_definition_is_numpys_formula_where_numpy_has_one(name):
    a, kind = MC.gen(name), MC.kind_of(name)
    ok = MC.in_range(a, kind)
    assert ok.sum() >= min(a.size, 3) // 2
    assert np.array_equal(MC.definition(a, kind)[ok], MC.numpy_formula(a, kind)[ok])


@pytest.mark.parametrize("name", NAMES)
def test_placement_holds_the_array(name):
    storage, off, (sn, sy, sx, sc) = MC.place(name)
    a = MC.gen(name)
    n, h, w, c = a.shape
    idx = (off + np.arange(n)[:, None, None, None] * sn + np.arange(h)[None, :, None, None] * sy
           + np.arange(w)[None, None, :, None] * sx + np.arange(c)[None, None, None, :] * sc)
    assert idx.min() >= 0 and idx.max() < storage.size and len(np.unique(idx)) == a.size
    assert np.array_equal(storage[idx].view(np.int32), a.view(np.int32))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_definition_bit_for_bit(name):
    """... and with it numpy's formulas on every in-range value, the NaN and the saturation values on the others."""
    from perceiverio_pytorch_amd import media as M
    assert (M.U8, M.S16) == (MC.U8, MC.S16)
    a, kind, rev = MC.gen(name), MC.kind_of(name), MC.reverse_of(name)
    got = M.restatement(torch.from_numpy(np.array(a)), kind, rev)
    assert got.dtype == (torch.uint8 if kind == MC.U8 else torch.int16) and got.is_contiguous()
    assert np.array_equal(got.numpy(), MC.definition(a, kind, rev))
    if not rev:
        ok = MC.in_range(a, kind)
        assert np.array_equal(got.numpy()[ok], MC.numpy_formula(a, kind)[ok])
    # read through the case's strides, as the functions hand views over
    storage, off, strides = MC.place(name)
    view = torch.from_numpy(storage).as_strided(a.shape, strides, off)
    assert torch.equal(M.restatement(view, kind, rev), got)


def test_restatement_refuses_reverse_with_int16():
    from perceiverio_pytorch_amd import media as M
    with pytest.raises(ValueError):
        M.restatement(torch.zeros(1, 1, 2, 1), M.S16, True)
    with pytest.raises(ValueError):
        M.restatement(torch.zeros(1, 1, 2, 1), 7)


def test_to_frames_layouts_and_refusals():
    import perceiverio_pytorch_amd as P
    g = torch.Generator().manual_seed(3)
    img = torch.rand((2, 3, 3, 6, 8), generator=g) * 1.5 - 0.25               # [b, t, C, H, W]
    want = torch.from_numpy(MC.definition(img.movedim(-3, -1).numpy(), MC.U8))
    got = P.to_frames(img)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 3, 6, 8, 3) and got.is_contiguous()
    assert torch.equal(got, want)
    assert torch.equal(P.to_frames(img, bgr=True), want.flip(-1))
    assert torch.equal(P.to_frames(img.movedim(-3, -1)), want)                  # channels last, inferred
    assert torch.equal(P.to_frames(img.movedim(-3, -1), channels_first=False), want)
    assert torch.equal(P.to_frames(img[0, 1]), want[0, 1])                      # a single [C, H, W] image
    assert torch.equal(P.to_frames(img[:, ::2]), want[:, ::2])                  # leading axes that do not collapse
    assert torch.equal(P.to_frames(img.double()), torch.from_numpy(MC.definition(img.double().float().movedim(-3, -1).numpy(),
                                                                                 MC.U8)))
    # the model's own view: [b, t, 3, h, w] of [b, t*h*w, 3] storage
    store = torch.rand((2, 3 * 6 * 8, 3), generator=g)
    view = store.reshape(2, 3, 6, 8, 3).moveaxis(-1, -3)
    assert torch.equal(P.to_frames(view, channels_first=True), torch.from_numpy(MC.definition(store.numpy(), MC.U8))
                       .reshape(2, 3, 6, 8, 3))
    assert tuple(P.to_frames(torch.zeros(0, 3, 6, 8)).shape) == (0, 6, 8, 3)
    for bad in (torch.zeros(3, 3, 3), torch.zeros(2, 8, 8, 8), torch.zeros(6, 8)):
        with pytest.raises(ValueError):
            P.to_frames(bad)
    with pytest.raises(ValueError):
        P.to_frames(torch.zeros(5, 8, 8), channels_first=True)                  # five channels
    with pytest.raises(ValueError):
        P.to_frames(torch.zeros(3, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError):
        P.to_frames(np.zeros((3, 8, 8), np.float32))
    assert tuple(P.to_frames(torch.zeros(3, 3, 3), channels_first=False).shape) == (3, 3, 3)    # ambiguous, but told


def test_to_pcm16_shapes():
    import perceiverio_pytorch_amd as P
    g = torch.Generator().manual_seed(4)
    a = torch.rand((2, 96, 1), generator=g) * 2 - 1
    want = torch.from_numpy(MC.definition(a.numpy(), MC.S16))
    got = P.to_pcm16(a)
    assert got.dtype == torch.int16 and got.shape == a.shape and torch.equal(got, want)
    assert torch.equal(P.to_pcm16(a[:, ::3]), want[:, ::3])
    assert torch.equal(P.to_pcm16(a[1, :, 0][::2]), want[1, :, 0][::2])
    assert torch.equal(P.to_pcm16(a.reshape(2, 2, 2, 24, 1)[:, :, 0]), want.reshape(2, 2, 2, 24, 1)[:, :, 0])
    assert torch.equal(P.to_pcm16(a[0, 5, 0]), want[0, 5, 0]) and P.to_pcm16(a[0, 5, 0]).dim() == 0
    assert tuple(P.to_pcm16(torch.zeros(0, 4)).shape) == (0, 4)
    with pytest.raises(ValueError):
        P.to_pcm16(torch.zeros(4, dtype=torch.int32))


def test_switch_and_backend_take_the_restatement_on_cpu(torch_backend, monkeypatch):
    P = torch_backend
    a = torch.from_numpy(np.array(MC.gen("u8_p1027")))
    on = P.to_frames(a, channels_first=False)
    monkeypatch.setattr(P, "fused_media", False)
    assert torch.equal(P.to_frames(a, channels_first=False), on)
    assert np.array_equal(on.numpy(), MC.definition(MC.gen("u8_p1027"), MC.U8))


def _reference_topk(logits, k):
    logprob, ids = torch.log_softmax(logits.float(), dim=-1).topk(k, dim=-1)
    return ids, logprob.exp()


@pytest.mark.parametrize("backend", ["hip", "torch"])
def test_top_labels_on_cpu_tensors(backend):
    import perceiverio_pytorch_amd as P
    prev = P.get_backend()
    P.set_backend(backend)
    try:
        g = torch.Generator().manual_seed(5)
        logits = torch.randn((3, 4, 700), generator=g) * 3
        ids, probs = P.top_labels(logits)
        rid, rp = _reference_topk(logits, 5)
        assert ids.dtype == torch.int64 and probs.dtype == torch.float32 and tuple(ids.shape) == (3, 4, 5)
        assert torch.equal(ids, rid) and torch.equal(probs, rp)
        # equal logits: the lower id first, whatever topk does with them
        tied = torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0, -0.0, 0.0], [2.0] * 7])
        ids, probs = P.top_labels(tied, k=6)
        assert ids.tolist() == [[1, 2, 4, 0, 3, 5], [0, 1, 2, 3, 4, 5]]
        assert torch.equal(probs, _reference_topk(tied, 6)[1])
        ids, probs = P.top_labels(torch.randn(2000, generator=g), k=12)         # one row, V and k beyond the kernel's
        assert tuple(ids.shape) == (12,) and bool((probs[:-1] >= probs[1:]).all())
        for bad_k in (0, 8):
            with pytest.raises(ValueError):
                P.top_labels(tied, k=bad_k)
        with pytest.raises(ValueError):
            P.top_labels(torch.zeros(3, dtype=torch.int64))
    finally:
        P.set_backend(prev)


def _small_multimodal():
    from perceiverio_pytorch_amd import models as M
    torch.manual_seed(11)
    model = M.MultiModalPerceiver(img_size=(16, 16), num_frames=2, num_classes=10, audio_samples_per_frame=32,
                                  audio_samples_per_patch=16, num_self_attends_per_block=1, num_latents=32,
                                  num_latent_channels=512).eval()
    g = torch.Generator().manual_seed(12)
    return model, torch.rand((2, 2, 3, 16, 16), generator=g), torch.rand((2, 64, 1), generator=g) * 2 - 1


def test_multimodal_classify_and_reconstruct_under_the_torch_backend(torch_backend):
    P = torch_backend
    model, images, audio = _small_multimodal()
    core = model.perceiver
    calls = []
    real = core._decoder.forward
    core._decoder.forward = lambda q, *a, **k: (calls.append(tuple(q.shape)), real(q, *a, **k))[1]
    try:
        with torch.inference_mode():
            lab = model.classify(images, audio, k=3, return_logits=True)
    finally:
        del core._decoder.forward
    assert calls == [(2, 1, core.query_channels)], calls
    with torch.inference_mode():
        out = model(images, audio, n_chunks=2)
        assert model.classify(images, audio).logits is None
        rec = model.reconstruct(images, audio, n_chunks=2, bgr=True)
    assert tuple(lab.logits.shape) == (2, 10) and tuple(lab.ids.shape) == (2, 3) and lab.ids.dtype == torch.int64
    assert float((lab.logits - out["label"]).abs().max()) <= 1e-5 * float(out["label"].abs().max())
    rid, rp = _reference_topk(lab.logits, 3)
    assert torch.equal(lab.ids, rid) and torch.equal(lab.probs, rp)
    assert torch.equal(rec.frames, P.to_frames(out["image"], bgr=True, channels_first=True))
    assert tuple(rec.frames.shape) == (2, 2, 16, 16, 3) and rec.frames.dtype == torch.uint8
    assert torch.equal(rec.pcm, P.to_pcm16(out["audio"])) and rec.pcm.shape == audio.shape
    assert torch.equal(rec.label, out["label"])


def test_decoder_query_subset_has_the_rows_of_the_whole(torch_backend):
    model, images, audio = _small_multimodal()
    core = model.perceiver
    inputs = {"image": images, "audio": audio, "label": torch.zeros((2, 10))}
    with torch.inference_mode():
        x, sizes, without_pos = core._multi_preprocessor(inputs, pos=None)
        points = {"image": torch.arange(0, 64), "audio": torch.arange(0, 2), "label": None}
        whole, wsizes = core.decoder_query(x, sizes, without_pos, subsampled_points=points)
        same, ssizes = core.decoder_query(x, sizes, without_pos, subsampled_points=points, modalities=None)
        label, lsizes = core.decoder_query(x, sizes, without_pos, modalities=("label",))
        two, tsizes = core.decoder_query(x, sizes, without_pos, subsampled_points=points, modalities=("label", "audio"))
    assert torch.equal(whole, same) and wsizes == ssizes
    assert lsizes == {"label": 1} and tuple(label.shape) == (2, 1, core.query_channels)
    row = wsizes["audio"] + wsizes["image"]                                     # (sorted order: audio | image | label)
    assert torch.equal(label, whole[:, row:row + 1])
    assert tsizes == {"audio": 2, "label": 1} and torch.equal(two, torch.cat([whole[:, :2], whole[:, row:]], dim=1))
    with pytest.raises(ValueError):
        core.decoder_query(x, sizes, without_pos, modalities=("labels",))


def test_classification_classify_restores_the_row_setting(torch_backend, monkeypatch):
    from perceiverio_pytorch_amd import models as M
    model = M.ClassificationPerceiver(num_classes=12, img_size=(8, 8), prep_type=M.PrepType.FOURIER_POS_PIXEL,
                                      num_self_attends_per_block=1, num_blocks=1, num_latents=8,
                                      num_latent_channels=64).eval()
    x = torch.rand((2, 3, 8, 8), generator=torch.Generator().manual_seed(2))
    seen = []
    real = model.perceiver._decoder.forward
    model.perceiver._decoder.forward = lambda q, *a, **k: (seen.append(tuple(q.shape)), real(q, *a, **k))[1]
    try:
        with torch.inference_mode():
            full = model(x)
            lab = model.classify(x, k=4, return_logits=True)
    finally:
        del model.perceiver._decoder.forward
    assert [s[1] for s in seen] == [12, 1] and model.decode_row0_only is False
    assert float((lab.logits - full).abs().max()) <= 1e-5 * float(full.abs().max())
    rid, rp = _reference_topk(lab.logits, 4)
    assert torch.equal(lab.ids, rid) and torch.equal(lab.probs, rp)
    # ... also when the forward raises, and a setting that was on stays on
    model.decode_row0_only = True
    with pytest.raises(Exception):
        model.classify(torch.rand(2, 3, 8), k=4)
    assert model.perceiver.decoder_query_rows == slice(0, 1)
    model.decode_row0_only = False
    with pytest.raises(Exception):
        model.classify(torch.rand(2, 3, 8), k=4)
    assert model.perceiver.decoder_query_rows is None
