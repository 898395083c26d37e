"""CPU: the range probe's C-ABI surface (header, .so symbol table, ctypes), the case tables, and the opt-in `torch`
plumbing backend -- records, parts and kinds, recommend_operand_dtype, life-cycle -- against abs-max figures recomputed
here from the modules' own weights."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import perceiverio_pytorch_amd as P
import range_probe_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["pio_absmax16", "pio_range_probe_begin", "pio_range_probe_mark", "pio_range_probe_end"]


@pytest.fixture(autouse=True)
def _torch_backend():
    P.set_backend("torch")
    try:
        with torch.no_grad():
            yield
    finally:
        P.set_backend("hip")


# ---- C-ABI surface ---------------------------------------------------------------------------------------------------
def test_header_library_and_ctypes_agree_on_the_four_symbols():
    from perceiverio_pytorch_amd import _lib as L, probe as LP
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pio_hip.h")).read(), flags=re.S)
    if not os.path.exists(L.LIB_PATH):
        L.build()
    so = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in pio_hip.h"
        assert hasattr(so, name), f"{name} is not exported by the library"
        assert name in L.SIGNATURES and L.SIGNATURES[name][0] is ctypes.c_int
    # argument counts of the prototypes against the ctypes tables
    for name in SYMBOLS:
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(proto.split(",")) == len(L.SIGNATURES[name][1]), name
    # the enums the Python names are indexed by
    for i, kind in enumerate(LP.RANGE_KINDS):
        assert re.search(r"\bPIO_RK_%s\s*=\s*%d\b" % (kind.upper(), i), src), kind
    for i, part in enumerate(LP.RANGE_PARTS):
        assert re.search(r"\bPIO_RP_%s\s*=\s*%d\b" % (part.upper(), i), src), part


def test_host_side_switch_needs_no_gpu():
    """begin / mark / end validate their arguments and keep the labels on the host (nothing is launched)."""
    lib = P.lib()
    assert lib.pio_range_probe_begin(None, 4) == -6 and lib.pio_range_probe_end(None, None, 0) == 0
    assert lib.pio_range_probe_mark(4) == -6 and lib.pio_range_probe_mark(-1) == -6 and lib.pio_range_probe_mark(2) == 0
    assert lib.pio_absmax16(0, None, 1, 1, 1, 1, 0, None, None) == -6
    assert lib.pio_absmax16(7, 16, 1, 1, 1, 1, 0, 16, None) == -6


# ---- case tables -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.LAYOUTS))
@pytest.mark.parametrize("shape", RC.SHAPES)
def test_primitive_layouts_fence_everything_outside_the_extent(shape, name):
    lay = RC.layout(shape, name)
    buf = RC.fill(lay, seed=1)
    live = np.zeros(lay["total"], bool)
    for b in range(lay["nb"]):
        for r in range(lay["rows"]):
            i = RC.index(lay, b, r, 0)
            live[i:i + lay["cols"]] = True
    assert np.isfinite(buf[live]).all() and np.isinf(buf[~live]).all()
    assert live.sum() == lay["nb"] * lay["rows"] * lay["cols"]
    assert not live[:lay["base"]].any() and not live[-RC.FENCE:].any() and lay["base"] >= RC.FENCE
    assert (lay["base"] * 2) % 16 == (2 if name == "offset2" else 0)
    if lay["batch"] > 1 and lay["stride_b"]:
        assert lay["stride_b"] > lay["rows"] * lay["ld"]
    assert np.abs(buf[live]).max() < abs(RC.PLANT)
    for t in (torch.float16, torch.bfloat16):
        assert float(torch.tensor(RC.PLANT).to(t)) == RC.PLANT
    pos = RC.plant_positions(lay)
    assert len(pos) == 4 and all(live[RC.index(lay, *p)] for p in pos)


def test_align_pairs_stacked_records_with_the_max_of_their_parts():
    cpu = [("stack", "cast", 1.0), ("stack", "q", 2.0), ("stack", "k", 5.0), ("stack", "v", 3.0), ("stack", "attn", 4.0)]
    assert RC.align(cpu, cpu) == [(p, k, v, v) for p, k, v in cpu]
    qk = [("stack", "cast", 1.0), ("stack", "q", 5.0), ("stack", "v", 3.0), ("stack", "attn", 4.0)]
    assert [r[3] for r in RC.align(qk, cpu)] == [1.0, 5.0, 3.0, 4.0]
    qkv = [("stack", "cast", 1.0), ("stack", "q", 5.0), ("stack", "attn", 4.0)]
    assert [r[3] for r in RC.align(qkv, cpu)] == [1.0, 5.0, 4.0]
    with pytest.raises(AssertionError):
        RC.align(qkv[:2], cpu)


# ---- CPU backend -----------------------------------------------------------------------------------------------------
def _tiny_io(L=2, blocks=1):
    from perceiverio_pytorch_amd.output_queries import TrainableQuery
    from perceiverio_pytorch_amd.perceiver import PerceiverIO
    torch.manual_seed(2)
    return PerceiverIO(num_blocks=blocks, num_self_attends_per_block=L, num_latents=6, num_latent_channels=16,
                       input_channels=12, final_project_out_channels=5,
                       perceiver_encoder_kwargs=dict(num_self_attend_heads=2, num_cross_attend_heads=1),
                       output_queries=TrainableQuery(output_index_dims=4, num_channels=16)).eval()


def _am(t):
    return float(t.abs().max())


def _attention_figures(att, nq, nk):
    """[(kind, abs-max)] of q, k, v and the core output of one Attention on normalised inputs (no mask), and its output."""
    H = att._num_heads
    B, Tq, Tk = nq.shape[0], nq.shape[1], nk.shape[1]
    q, k, v = att.proj_q(nq), att.proj_k(nk), att.proj_v(nk)
    qh, kh, vh = (t.reshape(B, t.shape[1], H, -1).permute(0, 2, 1, 3) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) / np.sqrt(qh.shape[-1]), dim=-1)
    o = (p @ vh).permute(0, 2, 1, 3).reshape(B, Tq, -1)
    return [("q", _am(q)), ("k", _am(k)), ("v", _am(v)), ("attn", _am(o))], att.final(o)


def _mlp_figures(mlp, n):
    h = F.gelu(mlp.fc1(n))
    return [("hidden", _am(h))], mlp.fc2(h)


def _cross_figures(ca, xq, xkv):
    kv, nq = ca.layer_norm_kv(xkv), ca.layer_norm_q(xq)
    recs, a = _attention_figures(ca.attention, nq, kv)
    x = xq + a if ca._use_query_residual else a
    n2 = ca.layer_norm2(x)
    mrecs, y = _mlp_figures(ca.mlp, n2)
    return [("cast", _am(kv)), ("cast", _am(nq))] + recs + [("cast", _am(n2))] + mrecs, x + y


def _self_figures(sa, x):
    n1 = sa.layer_norm1(x)
    recs, a = _attention_figures(sa.attention, n1, n1)
    x = x + a
    n2 = sa.layer_norm2(x)
    mrecs, y = _mlp_figures(sa.mlp, n2)
    return [("cast", _am(n1))] + recs + [("cast", _am(n2))] + mrecs, x + y


def _io_figures(model, x):
    """The records a forward of the tiny PerceiverIO must produce, recomputed from its modules: [(part, kind, abs-max)]."""
    enc, dec = model._encoder, model._decoder
    out = []
    recs, z = _cross_figures(enc.cross_attend, enc.latents(x), x)
    out += [("cross", k, v) for k, v in recs]
    for _ in range(enc._num_blocks):
        for sa in enc.self_attends:
            recs, z = _self_figures(sa, z)
            out += [("stack", k, v) for k, v in recs]
    x2, sizes, without_pos = model._multi_preprocessor({"__default": x}, pos=None)
    query, _ = model.decoder_query(x2, sizes, without_pos, subsampled_points=None)
    recs, y = _cross_figures(dec.decoding_cross_attn, query, z)
    out += [("decoder", k, v) for k, v in recs] + [("decoder", "stream", _am(y))]
    return out


def test_records_of_a_tiny_perceiver_io_match_the_recomputed_intermediates():
    model = _tiny_io()
    x = torch.randn(2, 9, 12)
    y0 = model(x)
    with P.range_probe() as probe:
        y1 = model(x)
    want = _io_figures(model, x)
    assert [(p, k) for p, k, _ in probe.records] == [(p, k) for p, k, _ in want]
    assert probe.calls == len(want) == 8 + 2 * 7 + 9
    for (p, k, got), (_, _, ref) in zip(probe.records, want):
        assert ref > 0 and got == pytest.approx(ref, rel=1e-5), (p, k, got, ref)
    assert torch.equal(y0, y1) and torch.equal(y0, model(x))
    by = probe.by_part()
    assert set(by) == {"cross", "stack", "decoder"} and set(by["stack"]) == {"cast", "q", "k", "v", "attn", "hidden"}
    assert by["stack"]["hidden"] == max(v for p, k, v in probe.records if (p, k) == ("stack", "hidden"))
    assert probe.worst() == {p: max(d.values()) for p, d in by.items()}


def test_raw_modules_are_part_attention_and_a_non_finite_value_reports_inf():
    from perceiverio_pytorch_amd.transformer_primitives import MLP, Attention, SelfAttention
    torch.manual_seed(4)
    att = Attention(q_in_channels=16, k_in_channels=16, v_in_channels=16, num_heads=2).eval()
    mlp = MLP(16, widening_factor=2).eval()
    sa = SelfAttention(16, widening_factor=1, num_heads=2).eval()
    xq, xk, xv = torch.randn(1, 5, 16), torch.randn(1, 9, 16) * 2, torch.randn(1, 9, 16) * 3
    with P.range_probe() as probe:
        att(xq, xk, xk)
        att(xq, xk, xv)
        mlp(xq)
        sa(xq)
    kinds = [k for _, k, _ in probe.records]
    assert kinds == (["cast", "cast", "q", "k", "v", "attn"] + ["cast", "cast", "cast", "q", "k", "v", "attn"]
                     + ["cast", "hidden"] + ["cast", "q", "k", "v", "attn", "cast", "hidden"])
    assert {p for p, _, _ in probe.records} == {"attention"}
    assert [v for _, _, v in probe.records[:2]] == [_am(xq), _am(xk)] and probe.records[8][2] == _am(xv)
    bad = xq.clone()
    bad[0, 2, 3] = float("nan")
    with P.range_probe() as probe:
        mlp(bad)
    assert probe.records[0] == ("attention", "cast", float("inf"))


def _raise_stack_hidden(model, limit):
    """Raise the last self-attend's LayerNorm-2 gain until its hidden activations exceed `limit` on the CPU backend."""
    sa = model.perceiver._encoder.self_attends[-1]
    sa.layer_norm2.weight.mul_(4.0 * limit)
    return sa


def _tiny_language():
    from perceiverio_pytorch_amd import models as M
    torch.manual_seed(3)
    m = M.LanguagePerceiver(vocab_size=32, max_seq_len=12, embed_dim=16, num_self_attends_per_block=2, num_latents=8,
                            num_latent_channels=32).eval()
    ids = torch.randint(0, 32, (2, 12))
    mask = torch.ones(2, 12)
    mask[1, 9:] = 0
    return m, ids, mask


def test_recommendation_turns_only_the_part_over_the_limit_into_bf16x3():
    model, ids, mask = _tiny_language()
    default = "fp16x2w/fp16x2o/fp16x3f"
    assert model.precision_policy == default
    policy, report = P.recommend_operand_dtype(model, ids, mask)
    assert policy == default and report["policy"] == default and report["limit"] == 65504.0
    assert report["calls"] == 8 + 2 * 7 + 8          # (this decoder has no final Linear: no y16)
    assert set(report["absmax"]) == {"cross", "stack", "decoder"}
    base = {p: max(d.values()) for p, d in report["absmax"].items()}
    # a LayerNorm gain raised until the stack's hidden activations exceed the limit; the limit is chosen between the
    # model's own largest figure and the planted one, so that nothing else is over it
    limit = 8.0 * max(base.values())
    _raise_stack_hidden(model, limit)
    policy, report = P.recommend_operand_dtype(model, ids, mask, limit=limit)
    worst = {p: max(d.values()) for p, d in report["absmax"].items()}
    assert report["absmax"]["stack"]["hidden"] > limit and worst["cross"] < limit, report
    # (the decoder normalises the latents before it reads them: the planted activations do not travel on)
    assert worst["decoder"] < limit and policy == "fp16x2w/bf16x3/fp16x3f", (policy, report)
    assert model.precision_policy == default          # (nothing is set)


def test_recommendation_on_a_stack_only_overflow_leaves_cross_and_decoder_alone():
    """The planted gain with the block's fc2 zeroed: the hidden activations overflow and nothing travels on."""
    model, ids, mask = _tiny_language()
    _, report = P.recommend_operand_dtype(model, ids, mask)
    limit = 8.0 * max(max(d.values()) for d in report["absmax"].values())
    sa = _raise_stack_hidden(model, limit)
    sa.mlp.fc2.weight.zero_()
    policy, report = P.recommend_operand_dtype(model, ids, mask, limit=limit)
    assert report["absmax"]["stack"]["hidden"] > limit
    assert policy == "fp16x2w/bf16x3/fp16x3f", (policy, report)
    model.precision_policy = "fp16/fp16x3f"          # two-part string: the cross-attend runs under the encoder's
    policy, _ = P.recommend_operand_dtype(model, ids, mask, limit=limit)
    assert policy == "fp16/bf16x3/fp16x3f"
    policy, _ = P.recommend_operand_dtype(model, ids, mask, limit=float("inf"))
    assert policy == "fp16/fp16x3f"


def test_life_cycle_one_probe_at_a_time_and_none_left_behind_by_an_exception():
    from perceiverio_pytorch_amd import probe as LP
    assert not LP.range_active()
    with P.range_probe():
        assert LP.range_active()
        with pytest.raises(P.PioError, match="already active"):
            with P.range_probe():
                pass
        assert LP.range_active()
        with P.logit_probe():                        # the two kinds of probe may be active together
            assert LP.active()
    assert not LP.range_active() and not LP.active()
    with pytest.raises(ZeroDivisionError):
        with P.range_probe():
            1 / 0
    assert not LP.range_active()
    with P.range_probe() as probe:
        pass
    assert probe.records == [] and probe.calls == 0
    with pytest.raises(ValueError):
        P.range_probe(max_records=0)
