"""GPU: the language front end -- pio_embed_tokens through the raw C-ABI on every case of tests/embed_cases.py against the
definition, as int32 bit patterns, twice; its refusal and accepted tables on device memory; EmbeddingPreprocessor and
MultimodalPreprocessor with the fused path on and off (equal bits, ONE kernel call and no nn.Embedding forward when
eligible, none when not); the language goldens with LanguagePerceiver.fused_front_end on and off (torch.equal, both within
TOL of the golden); one stream capture of the fused forward, replayed.

Memory safety by construction: outputs sit between 4 KiB guard bands and are NaN before the call; pitch gaps, sample gaps
and everything outside [B, T] must still be NaN afterwards; table and pos are surrounded by NaN, the ids by ids of other
rows; every bad id is one a wrong kernel would still resolve inside the allocation (embed_cases.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_cases as EC  # noqa: E402
from test_flow_front_gpu import GuardedOut  # noqa: E402
from test_embed_front_host import embed_tokens  # noqa: E402
from test_models import TOL, _cached_model, _close  # noqa: E402
from _golden import load  # noqa: E402
from cases import model_inputs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


_REF = {}


def case_data(name):
    """(inputs, definition) of a case, computed once and shared (read-only) by the tests below."""
    if name not in _REF:
        data = EC.gen(name)
        _REF[name] = (data, EC.reference(name, data))
    return _REF[name]


def launch(dev, name, data, flag_before=0):
    """One call of the raw entry on the case's surrounded inputs: (guarded y, guarded tokens or None, flag word)."""
    from perceiverio_pytorch_amd import _lib as L
    c = EC.CASES[name]
    held = {k: torch.from_numpy(data[k + "_full"]).to(dev) for k in ("ids", "table", "pos")}
    y = GuardedOut(dev, 1, EC.out_elems(c, "y"))
    tok = GuardedOut(dev, 1, EC.out_elems(c, "tokens")) if c["tokens"] else None
    flag = torch.full((1,), flag_before, dtype=torch.int32, device=dev)
    addr = {"y": y.t.data_ptr(), "tokens": tok.t.data_ptr() if tok else 0, "bad_ids": flag.data_ptr()}
    addr.update({k: v.data_ptr() for k, v in held.items()})
    f = EC.call_fields(name, data, addr.__getitem__)
    L.check(embed_tokens(L, f, torch.cuda.current_stream().cuda_stream), f"pio_embed_tokens[{name}]")
    y.check(name + " y")
    if tok:
        tok.check(name + " tokens")
    return y, tok, int(flag.item())


@pytest.mark.parametrize("name", sorted(EC.CASES))
def test_raw_entry_against_the_definition(dev, name):
    c = EC.CASES[name]
    data, (ry, rtok, rflag) = case_data(name)
    y, tok, flag = launch(dev, name, data)
    EC.compare(y.t.cpu().numpy(), ry, name + " y")
    if rtok is not None:
        EC.compare(tok.t.cpu().numpy(), rtok, name + " tokens")
    assert flag == (rflag if c["flag"] else 0), f"{name}: flag word {flag}"
    y2, tok2, flag2 = launch(dev, name, data, flag_before=7)        # (the call never clears the word)
    assert torch.equal(y.t.view(torch.int32), y2.t.view(torch.int32)), f"{name}: two launches differ"
    assert tok is None or torch.equal(tok.t.view(torch.int32), tok2.t.view(torch.int32))
    assert flag2 == (1 if rflag and c["flag"] else 7), f"{name}: flag word {flag2} after a call that found it at 7"


def _refusal_buffers(dev):
    bufs = {"y": GuardedOut(dev, 1, 256), "tokens": GuardedOut(dev, 1, 256),
            "ids": torch.zeros(64, dtype=torch.int64, device=dev), "table": torch.randn(64, device=dev),
            "pos": torch.randn(64, device=dev), "bad_ids": torch.zeros(4, dtype=torch.int32, device=dev)}
    ptrs = {k: (v.t.data_ptr() if isinstance(v, GuardedOut) else v.data_ptr()) for k, v in bufs.items()}
    return bufs, ptrs


@pytest.mark.parametrize("what,changes", EC.ACCEPTED, ids=[r[0] for r in EC.ACCEPTED])
def test_accepted_calls_of_the_refusal_table_run(dev, what, changes):
    """The valid call, the optional arguments left out and the alignments / pitches that only choose dword stores: B * T rows
    of C channels written (ids all 0: table row 0 + pos row t), nothing else."""
    from perceiverio_pytorch_amd import _lib as L
    bufs, ptrs = _refusal_buffers(dev)
    f = EC.refusal_fields(ptrs, changes)
    assert embed_tokens(L, f, torch.cuda.current_stream().cuda_stream) == EC.PIO_OK
    for which in ("y", "tokens"):
        bufs[which].check(f"{what} {which}")
        flat = bufs[which].t.reshape(-1).cpu().numpy()
        if f[which] is None:
            assert np.isnan(flat).all()
            continue
        first = (f[which] - ptrs[which]) // 4
        m = np.zeros(flat.shape, dtype=bool)
        w = EC.written(f, which)
        m[first:first + w.size] = w
        assert np.isfinite(flat[m]).all() and np.isnan(flat[~m]).all(), f"{what}: {which}"
    row0, pos = bufs["table"][:f["C"]], bufs["pos"]
    first = (f["y"] - ptrs["y"]) // 4
    got = bufs["y"].t.reshape(-1)[first + (f["B"] - 1) * f["y_sb"] + (f["T"] - 1) * f["ldy"]:][:f["C"]]
    assert torch.equal(got, row0 + pos[(f["T"] - 1) * f["ldp"]:][:f["C"]])
    assert int(bufs["bad_ids"][0].item()) == 0


@pytest.mark.parametrize("what,changes,code", EC.REFUSALS, ids=[r[0] for r in EC.REFUSALS])
def test_refusals_launch_nothing(dev, what, changes, code):
    from perceiverio_pytorch_amd import _lib as L
    bufs, ptrs = _refusal_buffers(dev)
    assert embed_tokens(L, EC.refusal_fields(ptrs, changes), torch.cuda.current_stream().cuda_stream) == code
    for which in ("y", "tokens"):
        bufs[which].check(f"{what} {which}")
        assert torch.isnan(bufs[which].t).all(), f"{what}: a refused call wrote to {which}"
    assert int(bufs["bad_ids"][0].item()) == 0


def _counting(monkeypatch, prep):
    """pio_embed_tokens as every module sees it (the proxy-lib() hook of tests/test_queries_gpu.py) and the forward of the
    preprocessor's nn.Embedding, both counted."""
    from perceiverio_pytorch_amd import _lib as L
    calls = {"kernel": 0, "embed": 0}
    real = L.lib()

    class _Lib:
        def __getattr__(self, k):
            return getattr(real, k)

        def pio_embed_tokens(self, *a):
            calls["kernel"] += 1
            return real.pio_embed_tokens(*a)
    proxy = _Lib()
    monkeypatch.setattr(L, "lib", lambda: proxy)
    real_forward = prep.embed.forward

    def forward(x):
        calls["embed"] += 1
        return real_forward(x)
    monkeypatch.setattr(prep.embed, "forward", forward)
    return calls


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32], ids=["int64", "int32"])
def test_preprocessor_fused_on_and_off(dev, dtype, monkeypatch):
    """EmbeddingPreprocessor on the GPU: equal bits with the kernel and with the chain, for both outputs; ONE kernel call and
    no nn.Embedding forward when eligible, and MultimodalPreprocessor hands the array on without a copy; no kernel call for
    every input or configuration the fused path declines."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd.io_processors import EmbeddingPreprocessor
    from perceiverio_pytorch_amd.perceiver import MultimodalPreprocessor
    torch.manual_seed(11)
    T, C, V = EC.STRIP + 5, 12, 9
    prep = EmbeddingPreprocessor(vocab_size=V, max_seq_len=T, embedding_dims=C).to(dev).eval()
    mp = MultimodalPreprocessor(input_preprocessors=torch.nn.ModuleDict({"__default": prep}), min_padding_size=0)
    ids = torch.randint(0, V, (3, T), device=dev).to(dtype)
    calls = _counting(monkeypatch, prep)
    y_on, tok_on = prep(ids)
    assert calls == {"kernel": 1, "embed": 0}, calls
    assert y_on.shape == (3, T, C) and y_on.is_contiguous() and y_on.dtype == torch.float32 and tok_on.shape == (3, T, C)
    assert int(prep.bad_ids_flag(dev).item()) == 0 and prep.bad_ids_flag(dev) is prep.bad_ids_flag(dev)
    prep.need_tokens = False
    y_only, none = prep(ids)
    assert none is None and calls == {"kernel": 2, "embed": 0}
    x, sizes, wo = mp({"__default": ids}, pos=None)
    assert calls == {"kernel": 3, "embed": 0} and sizes == {"__default": T} and wo == {"__default": None}
    prep.need_tokens = True
    sliced = torch.randint(0, V, (3, T + 3), device=dev).to(dtype)[:, :T]          # a row stride larger than T
    y_sl, _ = prep(sliced)
    assert calls == {"kernel": 4, "embed": 0}
    prep.fused_embedding = False
    y_off, tok_off = prep(ids)
    x_off, sizes_off, wo_off = mp({"__default": ids}, pos=None)
    y_sl_off, _ = prep(sliced)
    assert calls == {"kernel": 4, "embed": 3}, calls
    prep.fused_embedding = True
    for a, b in ((y_on, y_off), (tok_on, tok_off), (y_only, y_off), (x, x_off), (x_off, y_off), (wo_off["__default"], tok_off),
                 (y_sl, y_sl_off)):
        assert torch.equal(_bits(a), _bits(b))
    assert sizes == sizes_off
    # declined: a sequence shorter than the table, a transposed id matrix, other dtypes, CPU tensors, the torch backend,
    # padding_idx / max_norm, a half-precision table
    before = dict(calls)
    transposed = torch.randint(0, V, (T, 3), device=dev).to(dtype).t()                 # stride(1) != 1
    for bad in (ids[:, :T - 1], transposed, ids.to(torch.int16), ids.float(), ids[0], torch.broadcast_to(ids[:1], (3, T)),
                ids.cpu()):
        assert prep._fused(bad) is None
    prev = P.get_backend()
    P.set_backend("torch")
    try:
        assert prep._fused(ids) is None
    finally:
        P.set_backend(prev)
    prep.embed.padding_idx = 0
    assert prep._fused(ids) is None
    prep.embed.padding_idx, prep.embed.max_norm = None, 1.0
    assert prep._fused(ids) is None
    prep.embed.max_norm = None
    half = EmbeddingPreprocessor(vocab_size=V, max_seq_len=T, embedding_dims=C).to(dev).half()
    assert half._fused(ids) is None
    short =EmbeddingPreprocessor(vocab_size=V, max_seq_len=T + 2, embedding_dims=C).to(dev)
    assert short._fused(ids) is None
    assert calls == before
    assert prep._fused(ids) is not None and calls["kernel"] == before["kernel"] + 1


def test_bad_ids_through_the_module(dev):
    """NaN rows and a set word instead of ATen's device-side assert; the next forward clears the word on the stream."""
    from perceiverio_pytorch_amd.io_processors import EmbeddingPreprocessor
    torch.manual_seed(12)
    T, C, V = 5, 4, 9
    prep = EmbeddingPreprocessor(vocab_size=V, max_seq_len=T, embedding_dims=C).to(dev).eval()
    ids = torch.randint(0, V, (2, T), device=dev)
    good, _ = prep(ids)
    assert int(prep.bad_ids_flag(dev).item()) == 0
    bad = ids.clone()
    bad[0, 1], bad[1, 4] = V, -1
    y, tok = prep(bad)
    assert int(prep.bad_ids_flag(dev).item()) == 1
    rows = torch.zeros(2, T, dtype=torch.bool, device=dev)
    rows[0, 1] = rows[1, 4] = True
    assert bool(torch.isnan(y[rows]).all()) and bool(torch.isnan(tok[rows]).all())
    assert torch.equal(_bits(y[~rows]), _bits(good[~rows]))
    again, _ = prep(ids)
    assert int(prep.bad_ids_flag(dev).item()) == 0 and torch.equal(_bits(again), _bits(good))


@pytest.mark.parametrize("name", ["model_language", "model_language_s33"])
def test_language_goldens_fused_on_and_off(dev, name):
    """The whole model (s33: ragged lengths 1 and 1290) with the front end as one kernel and as the chain: the same logits
    bit for bit, both within TOL of the golden."""
    g = load(name)
    model = _cached_model(name, g, dev)
    prep = model.perceiver._multi_preprocessor._preprocessors["__default"]
    ins = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]
    assert model.fused_front_end is True and prep.need_tokens is False
    assert prep._fused(ins[0]) is not None, "the fused path declined the golden's ids"
    outs = {}
    try:
        for on in (True, False):
            model.fused_front_end = on
            with torch.inference_mode():
                out = model(ins[0], ins[1])
            _close(out[:, :96], g["out"], f"{name} head, fused_front_end={on}", TOL, absmax=g["out_absmax"])
            _close(out[:, 640:704], g["out_tail"], f"{name} tail, fused_front_end={on}", TOL, absmax=g["out_absmax"])
            outs[on] = out
    finally:
        model.fused_front_end = True
    assert torch.equal(outs[True], outs[False])
    assert int(prep.bad_ids_flag(dev).item()) == 0


def test_fused_forward_in_a_graph(dev):
    """No allocation of the library's own, no synchronisation: the fused forward (the memset of the flag word + ONE launch)
    captures into a graph, and a replay on new ids equals the eager result."""
    from perceiverio_pytorch_amd.io_processors import EmbeddingPreprocessor
    torch.manual_seed(13)
    T, C, V = EC.STRIP + 1, 8, 9
    prep = EmbeddingPreprocessor(vocab_size=V, max_seq_len=T, embedding_dims=C).to(dev).eval()
    ids = torch.randint(0, V, (2, T), device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        prep(ids)                                          # (warm-up: the flag word exists before the capture)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yg, tg = prep(ids)
    new = torch.randint(0, V, (2, T), device=dev)
    new[1, 3] = V + 1
    ids.copy_(new)
    g.replay()
    torch.cuda.synchronize()
    assert int(prep.bad_ids_flag(dev).item()) == 1        # (the owner of the graph reads the word after the replay)
    y, t = prep(new)
    assert torch.equal(_bits(yg), _bits(y)) and torch.equal(_bits(tg), _bits(t))
