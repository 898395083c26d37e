"""GPU: the invalidation contract of runtime.param_key holds for every cache -- after a raw write through ``p.data`` and
``invalidate_packed_weights(top)`` the next forward equals, bit for bit, that of a freshly constructed module loaded with
the new weights.  One case per kind of cache: a linear head (runtime.hip_linear), the decoder's final layer, a block
descriptor reached through its parent, and the multimodal model's cached decoder queries."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_models import _load_generated, build  # noqa: E402
from _golden import load  # noqa: E402
from cases import model_inputs, model_seed, model_stats  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


def _randn(dev, *shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def _bits(y):
    ys = list(y.values()) if isinstance(y, dict) else [y]
    return [t.contiguous().view(torch.int32).cpu() for t in ys]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _raw_write_then_invalidate(dev, top, weight, run, fresh):
    """forward, `weight`.data.copy_(new values), invalidate_packed_weights(top), forward: the second result against that of
    `fresh()` -- a newly constructed module -- loaded with top's state.  The new values are far from the old ones, so a
    stale image shows: the premise that the fresh module's result differs from the first forward's is asserted."""
    from perceiverio_pytorch_amd import invalidate_packed_weights
    before = run(top)
    new = _randn(dev, *weight.shape, seed=99) * weight.detach().abs().mean() * 2 + weight.detach().flip(0)
    weight.data.copy_(new)
    invalidate_packed_weights(top)
    after = run(top)
    twin = fresh()
    twin.load_state_dict({k: v.detach().cpu() for k, v in top.state_dict().items()}, strict=True)
    want = run(twin.to(dev).eval())
    assert not _same(before, want), "premise: the write changes the result"
    assert _same(after, want), "a stale image survived invalidate_packed_weights"


@pytest.mark.parametrize("kind", ["classification", "projection"])
def test_head_weight(dev, kind):
    from perceiverio_pytorch_amd import io_processors as IO

    def make():
        torch.manual_seed(11)
        if kind == "classification":
            return IO.ClassificationPostprocessor(num_input_channels=16, num_classes=8)
        return IO.ProjectionPostprocessor(num_inputs=16, num_outputs=3)

    x = _randn(dev, 2, 5, 16, seed=1)
    top = make().to(dev).eval()
    weight = top.linear.weight if kind == "classification" else top.projection.weight
    _raw_write_then_invalidate(dev, top, weight, lambda m: m(x, pos=None, modality_sizes=None), make)


def test_decoder_final_layer_weight(dev):
    from perceiverio_pytorch_amd.perceiver import PerceiverDecoder

    def make():
        torch.manual_seed(12)
        return PerceiverDecoder(32, 10, num_latent_channels=32, num_heads=1)

    q, z = _randn(dev, 2, 6, 32, seed=2), _randn(dev, 2, 12, 32, seed=3)
    top = make().to(dev).eval()
    _raw_write_then_invalidate(dev, top, top.final_layer.weight, lambda m: m(q, z), make)


def test_self_attention_mlp_weight(dev):
    from perceiverio_pytorch_amd.transformer_primitives import SelfAttention

    def make():
        torch.manual_seed(13)
        return SelfAttention(32, widening_factor=1, num_heads=2)

    x = _randn(dev, 2, 8, 32, seed=4)
    top = make().to(dev).eval()
    _raw_write_then_invalidate(dev, top, top.mlp.fc1.weight, lambda m: m(x), make)


def test_multimodal_query_padding_embedding(dev):
    name = "model_multimodal_small"
    model = _load_generated(build(name), load(name), dev, model_seed(name), model_stats(name))
    assert model.cache_queries is True and model.cache_projected_queries is True
    ins = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]

    def run(m):
        with torch.inference_mode():
            return m(ins[0], ins[1], n_chunks=2)

    weight = model.perceiver.padding_embeddings["image"].pos_embs
    assert weight.numel() > 0
    _raw_write_then_invalidate(dev, model, weight, run, lambda: build(name))
    assert len(model._packed) == 1          # (two chunks are one group: one cached query array, rebuilt once)
