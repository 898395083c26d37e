"""CPU: masked-token prediction (LanguagePerceiver.predict) as far as it goes without a device -- the chain under the torch
backend on a small model against the full forward, every form of `positions`, the host-side validation, unchanged
parameters / buffers / state_dict keys, the switches, the plan function of fused_io.vocab_topk on everything it declines, and
the refusal table of pio_vocab_topk (no launch: a refused call returns before it touches a device)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vocab_cases as VC  # noqa: E402


def small_language_model():
    from perceiverio_pytorch_amd.models import LanguagePerceiver
    return LanguagePerceiver(vocab_size=11, max_seq_len=6, embed_dim=8, num_self_attends_per_block=1, num_latents=4,
                             num_latent_channels=16)


@pytest.fixture()
def torch_backend():
    import perceiverio_pytorch_amd as P
    prev = P.get_backend()
    P.set_backend("torch")
    yield
    P.set_backend(prev)


@pytest.fixture(scope="module")
def small():
    torch.manual_seed(3)
    model = small_language_model().eval()      # (as initialised: logits of order 1, where 1e-6 is a couple of fp32 ulps)
    ids = torch.randint(0, 11, (2, 6))
    mask = torch.ones(2, 6)
    mask[1, 4:] = 0
    return model, ids, mask


POSITIONS = {
    "list": [1, 3, 5],
    "[P]": torch.tensor([4, 0, 2, 2]),
    "[P] int32": torch.tensor([5, 1], dtype=torch.int32),
    "[B, P]": torch.tensor([[0, 2, 2], [5, 1, 0]]),
    "None": None,
}


@pytest.mark.parametrize("form", sorted(POSITIONS))
def test_predict_equals_the_rows_of_the_full_forward(torch_backend, small, form):
    model, ids, mask = small
    pos = POSITIONS[form]
    with torch.no_grad():
        full = model(ids, mask)
        got = model.predict(ids, mask, pos, k=3, return_logits=True)
        lean = model.predict(ids, mask, pos, k=3)
    idx = torch.arange(6) if pos is None else torch.as_tensor(pos).long()
    idx = idx.expand(2, -1) if idx.dim() == 1 else idx
    want = torch.gather(full, 1, idx[:, :, None].expand(-1, -1, 11))
    p = idx.shape[1]
    assert type(got).__name__ == "Prediction" and got._fields == ("ids", "logprobs", "logits")
    assert got.ids.shape == (2, p, 3) and got.ids.dtype == torch.int64
    assert got.logprobs.shape == (2, p, 3) and got.logprobs.dtype == torch.float32
    assert got.logits.shape == (2, p, 11) and got.logits.dtype == torch.float32 and lean.logits is None
    err = float((got.logits - want).abs().max())
    print(f"{form}: max |predict logits - forward rows| = {err:.3e}, max |logit| = {float(want.abs().max()):.3f}")
    assert err <= 1e-6
    lp, top = torch.log_softmax(got.logits, dim=-1).topk(3, dim=-1)
    assert torch.equal(got.ids, top) and torch.equal(got.logprobs, lp)
    assert torch.equal(lean.ids, got.ids) and torch.equal(lean.logprobs, got.logprobs)


def test_shared_positions_keep_the_batch_invariant_query(torch_backend, small):
    """[P] positions: the decoder receives ONE [1, P, C] query array behind a stride-0 batch axis (what it projects once);
    [B, P] positions: a per-sample array.  The mask is gathered with the rows."""
    model, ids, mask = small
    seen = []
    hook = model.perceiver._decoder.register_forward_pre_hook(
        lambda mod, args, kwargs: seen.append((args[0], kwargs.get("query_mask"))), with_kwargs=True)
    try:
        with torch.no_grad():
            model.predict(ids, mask, [5, 1, 4], k=1)
            model.predict(ids, mask, torch.tensor([[5, 1, 4], [0, 4, 5]]), k=1)
            model(ids, mask)
    finally:
        hook.remove()
    (q1, m1), (q2, m2), (q0, m0) = seen
    table = model.perceiver._output_queries["__default"]._position_encoding.pos_embs.detach()
    assert q1.shape == (2, 3, 8) and q1.stride(0) == 0 and torch.equal(q1[0], table[[5, 1, 4]])
    assert torch.equal(m1, mask[:, [5, 1, 4]])
    assert q2.shape == (2, 3, 8) and q2.stride(0) != 0
    assert torch.equal(q2[0], table[[5, 1, 4]]) and torch.equal(q2[1], table[[0, 4, 5]])
    assert torch.equal(m2, torch.stack([mask[0, [5, 1, 4]], mask[1, [0, 4, 5]]]))
    assert q0.shape == (2, 6, 8) and q0.stride(0) == 0 and torch.equal(m0, mask)          # (forward: as before)


@pytest.mark.parametrize("pos", [[-1], [6], [0, 6], [], torch.tensor([[0, 1], [2, -1]]), torch.zeros((2, 0), dtype=torch.int64),
                                 torch.tensor([7]), torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]]),
                                 torch.zeros((1, 1, 1), dtype=torch.int64)],
                         ids=["-1", "max_seq_len", "one bad of two", "empty list", "[B, P] with -1", "[B, 0]", "tensor 7",
                              "float positions", "[1, P] at B = 2", "3-D"])
def test_bad_positions_raise_on_the_host(torch_backend, small, monkeypatch, pos):
    model, ids, mask = small

    def never(*a, **k):
        raise AssertionError("the model ran")
    monkeypatch.setattr(model.perceiver, "forward", never)
    with pytest.raises(ValueError):
        model.predict(ids, mask, pos, k=1)


@pytest.mark.parametrize("k", [0, 12, -1])
def test_bad_k_raises(torch_backend, small, k):
    model, ids, mask = small
    with pytest.raises(ValueError):
        model.predict(ids, mask, [0], k=k)
    post = model.perceiver._output_postprocessors["__default"]
    with pytest.raises(ValueError):
        post.predict(torch.zeros(1, 1, 8), k=k)


def test_k_equal_to_the_vocabulary_is_the_whole_distribution(torch_backend, small):
    model, ids, mask = small
    with torch.no_grad():
        got = model.predict(ids, mask, [2], k=11)
    assert got.ids.shape == (2, 1, 11) and sorted(got.ids[0, 0].tolist()) == list(range(11))
    assert abs(float(got.logprobs[0, 0].exp().sum()) - 1.0) < 1e-5


def test_parameters_buffers_and_state_dict_are_unchanged():
    from _golden import load
    from test_models import build, spec_of
    ref = dict(spec_of(load("model_language")))
    model = build("model_language")
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == ref
    assert sorted(n for n, _ in model.named_parameters(remove_duplicate=False)) == sorted(ref)
    assert not list(model.buffers())


def test_the_switches_are_plain_attributes():
    from perceiverio_pytorch_amd.io_processors import EmbeddingPostprocessor
    from perceiverio_pytorch_amd.models import LanguagePerceiver
    model = small_language_model()
    post = model.perceiver._output_postprocessors["__default"]
    keys = list(model.state_dict())
    assert EmbeddingPostprocessor.fused_predict is True and "fused_predict" not in post.__dict__
    assert isinstance(LanguagePerceiver.fused_predict, property) and model.fused_predict is True
    model.fused_predict = False
    assert model.fused_predict is False and post.fused_predict is False and EmbeddingPostprocessor.fused_predict is True
    model.fused_predict = 1
    assert model.fused_predict is True and post.__dict__["fused_predict"] is True
    assert list(model.state_dict()) == keys and not list(model.buffers())
    assert model.perceiver.decoder_query_rows is None


class FakeCuda(torch.Tensor):
    """A CPU tensor that says it lives on a GPU: the plan is taken from shapes, dtypes and strides alone."""
    is_cuda = True


def test_plan_declines_and_routes(monkeypatch):
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import fused_io as FIO, probe as LP
    from perceiverio_pytorch_amd.io_processors import EmbeddingPostprocessor

    def post_of(v, k, dtype=torch.float32):
        return EmbeddingPostprocessor(torch.nn.Embedding(v, k)).to(dtype)
    post = post_of(11, 8)
    x = torch.zeros(2, 3, 8).as_subclass(FakeCuda)
    assert P.get_backend() == "hip"
    # as shipped the selection mode alone is routed (the measurement: the kernel's own multiply won nowhere)
    assert FIO.VOCAB_FUSED_MAX_ROWS == 0 and FIO.vocab_plan(post, x, 3) == "select"
    monkeypatch.setattr(FIO, "VOCAB_FUSED_MAX_ROWS", 4096)
    assert FIO.vocab_plan(post, x, 3) == "fused"
    assert FIO.vocab_plan(post, torch.zeros(2, 3, 8), 3) is None                        # CPU rows
    assert FIO.vocab_plan(post, x.double().as_subclass(FakeCuda), 3) is None            # not fp32
    assert FIO.vocab_plan(post_of(11, 8, torch.float64), x, 3) is None                  # embedding not fp32
    assert FIO.vocab_plan(post, x[:, :, ::2], 3) is None                                # channel stride 2 (and K differs)
    assert FIO.vocab_plan(post, x[0], 3) is None                                        # 2-D
    assert FIO.vocab_plan(post, x[:, :0], 3) is None                                    # no rows
    assert FIO.vocab_plan(post, x, 0) is None and FIO.vocab_plan(post, x, 9) is None    # k outside [1, 8]
    assert FIO.vocab_plan(post_of(5, 8), x, 6) is None                                  # k > V
    assert FIO.vocab_plan(post_of(1025, 8), x, 3) is None                               # V > 1024
    assert FIO.vocab_plan(post_of(1024, 8), x, 8) == "fused"
    # the multiply is the kernel's up to VOCAB_FUSED_MAX_ROWS rows and for K a multiple of 4 in [4, 1024]; hip_linear's beyond
    n = FIO.VOCAB_FUSED_MAX_ROWS
    wide = torch.zeros(1, 1, 8).as_subclass(FakeCuda)
    assert FIO.vocab_plan(post, wide.expand(1, n, 8), 3) == "fused"
    assert FIO.vocab_plan(post, wide.expand(1, n + 1, 8), 3) == "select"
    assert FIO.vocab_plan(post_of(11, 6), torch.zeros(2, 3, 6).as_subclass(FakeCuda), 3) == "select"
    assert FIO.vocab_plan(post_of(11, 1028), torch.zeros(1, 1, 1028).as_subclass(FakeCuda), 3) == "select"
    post.fused_predict = False
    assert FIO.vocab_plan(post, x, 3) is None                                           # the switch
    post.fused_predict = True
    P.set_backend("torch")
    try:
        assert FIO.vocab_plan(post, x, 3) is None                                       # the torch backend
    finally:
        P.set_backend("hip")
    LP._range_active = object()                                                          # an active range probe
    try:
        assert FIO.vocab_plan(post, x, 3) is None and FIO.vocab_topk(post, x, 3) is None
    finally:
        LP._range_active = None
    assert FIO.vocab_plan(post, x, 3) == "fused"


def test_header_struct_and_symbol():
    import ctypes
    import re
    from perceiverio_pytorch_amd import _lib as L
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pio_hip.h")).read()
    assert re.search(r"\bint\s+pio_vocab_topk\s*\(\s*const\s+float\s*\*x", header)
    assert "pio_vocab_topk" in L.SIGNATURES and len(L.SIGNATURES["pio_vocab_topk"][1]) == len(VC.ARG_ORDER) + 1
    if not os.path.exists(L.LIB_PATH):
        L.build()
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "pio_vocab_topk"), "libpio_hip.so does not export pio_vocab_topk"


def _host_pointers():
    """Real, 64-byte aligned host arrays that a refused call never touches."""
    keep = {k: np.zeros(256, dtype=np.int64) for k in VC.POINTERS}
    return keep, {k: (v.ctypes.data + 63) // 64 * 64 for k, v in keep.items()}


@pytest.mark.parametrize("what,changes,code", VC.REFUSALS, ids=[r[0] for r in VC.REFUSALS])
def test_refusal_table(what, changes, code):
    """Bad arguments are refused with the documented code before anything is launched: no device is needed."""
    from perceiverio_pytorch_amd import _lib as L
    keep, ptrs = _host_pointers()
    assert VC.call(L, VC.refusal_fields(ptrs, changes)) == code
    assert all(int(np.abs(v).max()) == 0 for v in keep.values())


def test_refusal_table_is_well_formed():
    keep, ptrs = _host_pointers()
    names = [r[0] for r in VC.REFUSALS]
    assert len(set(names)) == len(names)
    assert set(VC.refusal_fields(ptrs, {})) == set(VC.ARG_ORDER)
    for _, changes, code in VC.REFUSALS:
        assert changes and set(changes) <= set(VC.ARG_ORDER) and code in (VC.PIO_E_ARG, VC.PIO_E_SHAPE, VC.PIO_E_ALIGN)


def test_definitions_agree_with_torch():
    """The numpy restatements the GPU tests compare against: stable_topk against a brute-force order with planted ties and
    signed zeros, lse_reference against torch.logsumexp in float64."""
    rng = np.random.default_rng(5)
    lg = rng.standard_normal((7, 70)).astype(np.float32)
    lg[0, [3, 64, 65]] = lg[0].max() + 1          # three equal maxima
    lg[1, :] = 0.25                               # all equal
    lg[2] = np.where(rng.random(70) < 0.5, np.float32(0.0), np.float32(-0.0))
    lg[2, 10] = -1.0
    top = VC.stable_topk(lg, 8)
    for r in range(7):
        order = sorted(range(70), key=lambda j: (-(float(lg[r, j]) + 0.0), j))
        assert top[r].tolist() == order[:8], r
    assert top[0, :3].tolist() == [3, 64, 65] and top[1].tolist() == list(range(8)) and 10 not in top[2]
    ref, bnd = VC.lse_reference(lg)
    want = torch.logsumexp(torch.from_numpy(lg).double(), dim=-1).numpy()
    assert np.abs(ref - want).max() < 1e-12 and (bnd > 0).all() and bnd.max() < 1e-4
