"""CPU, no library call: runtime.PackedCache and the owner protocol (runtime.PackedOwner) -- every cache of what a module
derives from its parameters is one object on its owner, and invalidate_packed_weights, _apply and load_state_dict reach
all of them on every model kind.  Builders are stubs."""
import copy
import gc
import os
import sys
import threading
import weakref

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_models import build  # noqa: E402

MODELS = ("model_flow_small", "model_multimodal_small", "model_language", "model_classify_1x1")
OLD_NAMES = ("_pio_cache", "_pio_block_cache", "_final_cache", "_pio_linear", "_layers_cache", "_query_cache")


class _Keep:
    pass


def test_get_builds_once_per_key_and_keep_lives_with_the_entry():
    from perceiverio_pytorch_amd.runtime import PackedCache
    c, calls, refs = PackedCache(), [], []

    def builder(tag):
        def build():
            calls.append(tag)
            keep = _Keep()
            refs.append(weakref.ref(keep))
            return tag, keep
        return build

    assert len(c) == 0 and c.held() is None
    assert c.get("k1", builder("a")) == "a" and c.get("k1", builder("b")) == "a" and calls == ["a"]
    assert c.held()[:2] == ("k1", "a") and c.held()[2] is refs[0]()
    assert c.get("k2", builder("c")) == "c" and calls == ["a", "c"]         # a new key rebuilds ...
    gc.collect()
    assert refs[0]() is None and refs[1]() is not None                       # ... and the old entry's keep is gone
    assert c.get("k2", builder("d")) == "c" and calls == ["a", "c"]
    c.clear()
    gc.collect()
    assert len(c) == 0 and refs[1]() is None
    assert c.get("k2", builder("e")) == "e" and calls == ["a", "c", "e"]     # clear forces a rebuild under the same key
    # several slots side by side: each with its own key, all dropped by one clear
    assert c.get("k", builder("f"), slot="blocks") == "f" and c.get("k2", builder("g")) == "e"
    assert len(c) == 2 and sorted(c.values()) == ["e", "f"] and c.held("blocks")[1] == "f"
    c.clear()
    assert len(c) == 0 and c.held("blocks") is None


@pytest.fixture(scope="module")
def models():
    return {name: build(name) for name in MODELS}


def _owners(model):
    from perceiverio_pytorch_amd.runtime import PackedOwner
    return [m for m in model.modules() if isinstance(m, PackedOwner)]


def _plant(model):
    owners = _owners(model)
    for m in owners:
        m._packed.get("planted", lambda: (threading.Lock(), None))
        assert len(m._packed) >= 1
    return owners


@pytest.mark.parametrize("name", MODELS)
def test_every_owner_is_emptied_by_the_three_invalidation_points(models, name):
    from perceiverio_pytorch_amd import invalidate_packed_weights
    model = models[name]
    drops = (lambda: invalidate_packed_weights(model), lambda: model.float(),
             lambda: model.load_state_dict(model.state_dict()))
    for drop in drops:
        owners = _plant(model)
        assert len(owners) > 0
        drop()
        left = [type(m).__name__ for m in owners if len(m._packed) or m._packed.held() is not None]
        assert left == [], left


def test_owner_classes_cover_every_module_that_caches(models):
    from perceiverio_pytorch_amd import io_processors as IO, models as M, perceiver as PV, transformer_primitives as TP
    found = {type(m) for model in models.values() for m in _owners(model)}
    want = {IO.EmbeddingPostprocessor, IO.AudioPostprocessor, IO.ClassificationPostprocessor, IO.ProjectionPostprocessor,
            PV.PerceiverEncoder, PV.PerceiverDecoder, TP.Attention, TP.MLP, TP.SelfAttention, TP.CrossAttention,
            M.MultiModalPerceiver}
    assert want <= found, want - found
    assert models["model_multimodal_small"] in _owners(models["model_multimodal_small"])
    for model in models.values():
        for m in model.modules():
            assert not set(OLD_NAMES) & set(m.__dict__), (type(m).__name__, set(OLD_NAMES) & set(m.__dict__))


@pytest.mark.parametrize("name", MODELS)
def test_deepcopy_carries_empty_caches(models, name):
    model = models[name]
    owners = _plant(model)             # (a lock cannot be pickled or copied: the copy must not touch the entries)
    twin = copy.deepcopy(model)
    assert all(len(m._packed) >= 1 for m in owners)                          # the original keeps its own
    copies = _owners(twin)
    assert len(copies) == len(owners) and all(len(m._packed) == 0 for m in copies)
    assert all(a._packed is not b._packed for a, b in zip(owners, copies))
    assert list(twin.state_dict()) == list(model.state_dict())
