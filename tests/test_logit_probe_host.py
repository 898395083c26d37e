"""CPU (opt-in `torch` plumbing backend): the logit probe's API -- records, mask semantics, part labels,
recommend_precision_policy -- against float64 numpy recomputed from the modules' own weights."""
import numpy as np
import pytest
import torch

import perceiverio_pytorch_amd as P


@pytest.fixture(autouse=True)
def _torch_backend():
    P.set_backend("torch")
    try:
        with torch.no_grad():
            yield
    finally:
        P.set_backend("hip")


def _np(t):
    return t.detach().double().numpy()


def _ln(x, ln):
    x = _np(x)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + ln.eps) * _np(ln.weight) + _np(ln.bias)


def _absmax(att, xq, xk, mask=None):
    """max |q k^T| / sqrt(dk) over the attendable positions; xq / xk: float64 numpy, already normalised."""
    H = att._num_heads
    q = xq @ _np(att.proj_q.weight).T + _np(att.proj_q.bias)
    k = xk @ _np(att.proj_k.weight).T + _np(att.proj_k.bias)
    B, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    q = q.reshape(B, Tq, H, -1).transpose(0, 2, 1, 3)
    k = k.reshape(B, Tk, H, -1).transpose(0, 2, 1, 3)
    s = np.abs(q @ k.transpose(0, 1, 3, 2)) / np.sqrt(q.shape[-1])
    if mask is not None:
        s = np.where(_np(mask)[:, None] != 0, s, 0.0)
    return float(s.max())


def test_cross_and_self_attention_records_match_float64():
    from perceiverio_pytorch_amd.transformer_primitives import CrossAttention, SelfAttention
    torch.manual_seed(0)
    ca = CrossAttention(q_in_channels=24, kv_in_channels=20, num_heads=2, qk_channels=16, v_channels=24).eval()
    sa = SelfAttention(in_channels=24, num_heads=4).eval()
    xq, xkv = torch.randn(2, 7, 24), torch.randn(2, 11, 20) * 3
    with P.logit_probe() as probe:
        y = ca(xq, xkv)
        sa(y)
    assert [p for p, _ in probe.records] == ["attention", "attention"] and probe.calls == 2
    ref_c = _absmax(ca.attention, _ln(xq, ca.layer_norm_q), _ln(xkv, ca.layer_norm_kv))
    ref_s = _absmax(sa.attention, _ln(y, sa.layer_norm1), _ln(y, sa.layer_norm1))
    assert ref_c > 0 and ref_s > 0
    assert probe.records[0][1] == pytest.approx(ref_c, rel=1e-5)
    assert probe.records[1][1] == pytest.approx(ref_s, rel=1e-5)
    assert probe.by_part() == {"attention": max(probe.records[0][1], probe.records[1][1])}


def test_masked_key_is_ignored_and_all_masked_gives_zero():
    """One key row times 50, then masked.  (The raw Attention module: in front of a CrossAttention's LayerNorm a row scale
    would be normalised away.)"""
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    torch.manual_seed(1)
    att = Attention(q_in_channels=16, k_in_channels=16, v_in_channels=16, num_heads=2).eval()
    xq, xk = torch.randn(1, 5, 16), torch.randn(1, 9, 16)
    xk50 = xk.clone()
    xk50[:, 3] *= 50
    mask = torch.ones(1, 5, 9, dtype=torch.bool)
    mask[:, :, 3] = False
    with P.logit_probe() as big:
        att(xq, xk50, xk50)
    with P.logit_probe() as masked:
        att(xq, xk50, xk50, attention_mask=mask)
    with P.logit_probe() as nothing:
        att(xq, xk50, xk50, attention_mask=torch.zeros(1, 5, 9, dtype=torch.bool))
    f = lambda pr: pr.records[0][1]                      # noqa: E731
    assert f(big) == pytest.approx(_absmax(att, _np(xq), _np(xk50)), rel=1e-5)
    assert f(masked) == pytest.approx(_absmax(att, _np(xq), _np(xk50), mask), rel=1e-5)
    assert f(masked) < f(big) / 5                        # the planted row dominates only while it is attendable
    assert f(nothing) == 0.0


def _tiny_io(L=2, blocks=2):
    from perceiverio_pytorch_amd.output_queries import TrainableQuery
    from perceiverio_pytorch_amd.perceiver import PerceiverIO
    torch.manual_seed(2)
    return PerceiverIO(num_blocks=blocks, num_self_attends_per_block=L, num_latents=6, num_latent_channels=16,
                       input_channels=12, final_project_out_channels=5,
                       perceiver_encoder_kwargs=dict(num_self_attend_heads=2, num_cross_attend_heads=1),
                       output_queries=TrainableQuery(output_index_dims=4, num_channels=16)).eval()


def test_part_labels_of_a_tiny_perceiver_io_and_outputs_unchanged():
    model = _tiny_io()
    x = torch.randn(2, 9, 12)
    y0 = model(x)
    with P.logit_probe() as probe:
        y1 = model(x)
    y2 = model(x)
    assert [p for p, _ in probe.records] == ["cross"] + 4 * ["stack"] + ["decoder"]
    assert set(probe.by_part()) == {"cross", "stack", "decoder"}
    assert all(v > 0 and np.isfinite(v) for _, v in probe.records)
    assert torch.equal(y0, y1) and torch.equal(y0, y2)


def test_probe_is_exclusive_and_off_outside_the_context():
    from perceiverio_pytorch_amd import probe as LP
    assert not LP.active()
    with P.logit_probe():
        assert LP.active()
        with pytest.raises(P.PioError, match="already active"):
            with P.logit_probe():
                pass
    assert not LP.active()


def _tiny_language():
    from perceiverio_pytorch_amd import models as M
    torch.manual_seed(3)
    m = M.LanguagePerceiver(vocab_size=32, max_seq_len=12, embed_dim=16, num_self_attends_per_block=2, num_latents=8,
                            num_latent_channels=32).eval()
    ids = torch.randint(0, 32, (2, 12))
    mask = torch.ones(2, 12)
    mask[1, 9:] = 0
    return m, ids, mask


def _cross_figure(model, ids, mask):
    core = model.perceiver
    x, _, _ = core._multi_preprocessor({"__default": ids}, pos=None)
    enc = core._encoder
    ca = enc.cross_attend
    full = (torch.ones(x.shape[0], enc.latents(x).shape[1], 1) * mask[:, None, :]) != 0
    return _absmax(ca.attention, _ln(enc.latents(x), ca.layer_norm_q), _ln(x, ca.layer_norm_kv), full)


def test_recommendation_flips_only_the_part_over_the_threshold():
    model, ids, mask = _tiny_language()
    assert model.precision_policy == "fp16x2w/fp16x2o/fp16x3f"
    small = _cross_figure(model, ids, mask)
    lnq = model.perceiver._encoder.cross_attend.layer_norm_q
    lnq.weight.mul_(8.0)
    large = _cross_figure(model, ids, mask)
    assert large > 4 * small > 0
    threshold = 0.5 * (small + large)
    policy, report = P.recommend_precision_policy(model, ids, mask, threshold=threshold)
    assert report["absmax"]["cross"] == pytest.approx(large, rel=1e-5) and report["threshold"] == threshold
    assert report["absmax"]["stack"] < threshold and report["absmax"]["decoder"] < threshold, report
    assert policy == "fp16x3fq/fp16x2o/fp16x3f"
    assert model.precision_policy == "fp16x2w/fp16x2o/fp16x3f"       # (nothing is set)
    lnq.weight.div_(8.0)
    policy, report = P.recommend_precision_policy(model, ids, mask, threshold=threshold)
    assert report["absmax"]["cross"] == pytest.approx(small, rel=1e-5)
    assert policy == "fp16x2w/fp16x2o/fp16x3f"
    assert report["calls"] == 1 + 2 + 1


def test_two_part_and_plain_policies_split_like_the_models_do():
    model, ids, mask = _tiny_language()
    model.precision_policy = "fp16/fp16x3f"
    policy, _ = P.recommend_precision_policy(model, ids, mask, threshold=1e-9)
    assert policy == "fp16x3fq/fp16x3fq/fp16x3fq"
    policy, _ = P.recommend_precision_policy(model, ids, mask, threshold=1e9)
    assert policy == "fp16/fp16x3f"
