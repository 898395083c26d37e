"""CPU: the definition of the language front end (tests/embed_cases.py) against the two torch lines it stands for --
`embed(ids) + pos` in fp32, bit for bit on every case's valid rows; the refusal table of pio_embed_tokens (no launch: a
refused call returns before it touches a device); what the case table claims to cover; the routing of
EmbeddingPreprocessor / MultimodalPreprocessor on CPU tensors and under the torch backend (the chain runs, both outputs come
back); LanguagePerceiver's switches; unchanged state_dict keys."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_cases as EC  # noqa: E402


def embed_tokens(L, f, stream=None):
    """pio_embed_tokens on the plain keyword values of embed_cases.call_fields / refusal_fields."""
    return L.lib().pio_embed_tokens(*[f[k] for k in EC.ARG_ORDER], stream)


def small_language_model():
    from perceiverio_pytorch_amd.models import LanguagePerceiver
    return LanguagePerceiver(vocab_size=11, max_seq_len=6, embed_dim=8, num_self_attends_per_block=1, num_latents=4,
                             num_latent_channels=16)


@pytest.mark.parametrize("name", sorted(EC.CASES))
def test_definition_equals_embedding_plus_position_in_torch(name):
    c = EC.CASES[name]
    data = EC.gen(name)
    y, tok, flag = EC.reference(name, data)
    B, T, C, V = c["B"], c["T"], c["C"], c["V"]
    table = torch.from_numpy(data["table_full"].reshape(-1)[data["table_off"]:][:(V - 1) * c["ldt"] + C].copy())
    table = torch.as_strided(table, (V, C), (c["ldt"], 1)).contiguous()
    pos = torch.from_numpy(data["pos_full"].reshape(-1)[data["pos_off"]:][:(T - 1) * c["ldp"] + C].copy())
    pos = torch.as_strided(pos, (T, C), (c["ldp"], 1)).contiguous()
    assert bool(torch.isfinite(table).all()) and bool(torch.isfinite(pos).all())
    ids = torch.from_numpy(data["ids"])
    valid = (ids >= 0) & (ids < V)
    assert flag == int(not bool(valid.all())) == int(bool(c["bad"]))
    emb = torch.nn.functional.embedding(ids.clamp(0, V - 1), table)
    want = (emb + pos[None]).numpy()
    for b in range(B):
        for t in range(T):
            o = c["y_off"] + b * c["y_sb"] + t * c["ldy"]
            if bool(valid[b, t]):
                assert np.array_equal(y[o:o + C].view(np.int32), want[b, t].view(np.int32)), (name, b, t)
                if tok is not None:
                    k = b * c["tok_sb"] + t * c["ldtok"]
                    assert np.array_equal(tok[k:k + C].view(np.int32), emb[b, t].numpy().view(np.int32)), (name, b, t)
            else:
                assert np.isnan(y[o:o + C]).all()
    # nothing but the C channels of the B * T rows is finite
    assert int(np.isfinite(y).sum()) == int(valid.sum()) * C
    assert tok is None or int(np.isfinite(tok).sum()) == int(valid.sum()) * C


def test_case_table_covers_what_it_claims():
    c = EC.CASES

    def vec(k):
        ok = all(k[f] % 4 == 0 for f in ("C", "ldt", "ldp", "ldy")) and k["y_off"] % 4 == 0 and k["col_off"] % 4 == 0
        ok = ok and (k["B"] == 1 or k["y_sb"] % 4 == 0)
        if k["tokens"]:
            ok = ok and k["ldtok"] % 4 == 0 and (k["B"] == 1 or k["tok_sb"] % 4 == 0)
        return ok
    assert {k["C"] for k in c.values()} >= {1, 3, 4, 6, 8, 260, 768}
    assert {k["T"] for k in c.values()} >= {1, 5, EC.STRIP + 1} and {k["B"] for k in c.values()} >= {1, 3}
    assert {k["V"] for k in c.values()} >= {1, 2, 262} and {k["id_bytes"] for k in c.values()} == {4, 8}
    assert not vec(c["c1"]) and not vec(c["c3_pitches"]) and vec(c["c4_vec"])
    assert c["c6_pitch8"]["C"] % 4 and all(c["c6_pitch8"][f] % 4 == 0 for f in ("ldt", "ldp", "ldy", "ldtok"))
    assert c["c8_y_off4"]["y_off"] == 1 and c["c8_y_off4"]["C"] % 4 == 0 and not vec(c["c8_y_off4"])
    assert vec(c["c260_trip2"]) and c["c260_trip2"]["C"] // 4 > 64
    assert all(c["c260_trip2"][f] > 260 for f in ("ldt", "ldp", "ldy", "ldtok"))
    assert vec(c["c768"]) and c["c768"]["T"] == 5 and c["c768"]["V"] == 262
    s = c["strips"]
    assert vec(s) and s["T"] > 2 * EC.STRIP and s["B"] == 3 and s["ids_sb"] > s["T"] and s["y_sb"] > s["T"] * s["ldy"]
    t = c["t33_tokens"]
    assert vec(t) and t["tokens"] and t["ldtok"] > t["C"] and t["tok_sb"] > t["T"] * t["ldtok"] and t["ldtok"] != t["ldy"]
    assert any(k["tokens"] for k in c.values()) and any(not k["tokens"] for k in c.values())
    for name in ("bad_i32", "bad_i64", "bad_dwords"):
        k = c[name]
        assert {-1, k["V"]} <= set(k["bad"].values()) or name == "bad_dwords"
        assert all(not 0 <= v < k["V"] for v in k["bad"].values()) and k["flag"]
    assert vec(c["bad_i32"]) and vec(c["bad_i64"]) and not vec(c["bad_dwords"])
    assert {-1, 262, 263} <= set(c["bad_i32"]["bad"].values()) and {-1, 262, 263} <= set(c["bad_i64"]["bad"].values())
    wide = [v for v in c["bad_i64"]["bad"].values() if not -2 ** 31 <= v < 2 ** 32]
    assert len(wide) >= 3 and all(0 <= v % EC.P32 < 262 for v in wide)         # (they narrow to VALID rows)
    assert any(v > 0 for v in wide) and any(v < 0 for v in wide)
    assert c["bad_no_flag"]["bad"] and not c["bad_no_flag"]["flag"]
    assert EC.GUARD_ROWS >= 2
    for name, k in c.items():
        data = EC.gen(name)
        ids = data["ids"][(data["ids"] >= 0) & (data["ids"] < k["V"])]
        if ids.size >= 4:                                   # row 0, row V - 1, a repeat
            assert 0 in ids and k["V"] - 1 in ids and len(set(ids.tolist())) < ids.size, name
        full = data["table_full"]
        assert np.isnan(full[:EC.GUARD_ROWS]).all() and np.isnan(full[-EC.GUARD_ROWS:]).all()
        assert np.isnan(data["pos_full"][0]).all() and np.isnan(data["pos_full"][-1]).all()
        if k["ids_sb"] > k["T"]:                            # the skipped ids name valid rows
            flat = data["ids_full"].reshape(-1)[data["ids_off"]:][:k["B"] * k["ids_sb"]].reshape(k["B"], k["ids_sb"])
            assert ((flat[:, k["T"]:] >= 0) & (flat[:, k["T"]:] < k["V"])).all()


def _host_pointers():
    """Made-up addresses are not enough here (tokens == y, moved pointers): real, 64-byte aligned host arrays that a refused
    call never touches."""
    keep = {k: np.zeros(256, dtype=np.int64) for k in EC.POINTERS}
    ptrs = {k: (v.ctypes.data + 63) // 64 * 64 for k, v in keep.items()}
    return keep, ptrs


@pytest.mark.parametrize("what,changes,code", EC.REFUSALS, ids=[r[0] for r in EC.REFUSALS])
def test_refusal_table(what, changes, code):
    """Bad arguments are refused with the documented code before anything is launched: no device is needed."""
    from perceiverio_pytorch_amd import _lib as L
    keep, ptrs = _host_pointers()
    assert embed_tokens(L, EC.refusal_fields(ptrs, changes)) == code
    assert all(int(np.abs(v).max()) == 0 for v in keep.values())


def test_refusals_and_accepted_rows_are_disjoint_and_complete():
    keep, ptrs = _host_pointers()
    names = [r[0] for r in EC.REFUSALS] + [r[0] for r in EC.ACCEPTED]
    assert len(set(names)) == len(names)
    for _, changes, _ in EC.REFUSALS:
        assert changes and set(changes) <= set(EC.ARG_ORDER)
    for _, changes in EC.ACCEPTED:
        assert set(changes) <= set(EC.ARG_ORDER)
    assert set(EC.refusal_fields(ptrs, {})) == set(EC.ARG_ORDER)


def _counting_chain(monkeypatch, prep):
    calls = {"embed": 0}
    real = prep.embed.forward

    def forward(x):
        calls["embed"] += 1
        return real(x)
    monkeypatch.setattr(prep.embed, "forward", forward)
    return calls


def test_cpu_tensors_and_the_torch_backend_run_the_chain(monkeypatch):
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd.io_processors import EmbeddingPreprocessor
    from perceiverio_pytorch_amd.perceiver import MultimodalPreprocessor
    torch.manual_seed(5)
    prep = EmbeddingPreprocessor(vocab_size=7, max_seq_len=5, embedding_dims=4).eval()
    assert EmbeddingPreprocessor.fused_embedding is True and EmbeddingPreprocessor.need_tokens is True
    calls = _counting_chain(monkeypatch, prep)
    ids = torch.tensor([[0, 6, 3, 3, 1], [2, 2, 5, 0, 6]])
    want_tok = prep.embed.weight.detach()[ids]
    want = want_tok + prep.input_pos_encoding.pos_embs.detach()[None]
    prev = P.get_backend()
    for backend in ("hip", "torch"):
        P.set_backend(backend)
        try:
            for need in (True, False):                   # (need_tokens is the fused path's business: the chain returns both)
                prep.need_tokens = need
                assert prep._fused(ids) is None
                with torch.no_grad():
                    y, tok = prep(ids)
                assert torch.equal(y, want) and torch.equal(tok, want_tok)
                mp = MultimodalPreprocessor(input_preprocessors=torch.nn.ModuleDict({"__default": prep}), min_padding_size=0)
                assert mp._single_embedding({"__default": ids}) is None
                with torch.no_grad():
                    x, sizes, wo = mp({"__default": ids}, pos=None)
                assert torch.equal(x, want) and sizes == {"__default": 5} and torch.equal(wo["__default"], want_tok)
        finally:
            P.set_backend(prev)
    assert calls["embed"] == 8
    prep.need_tokens = True
    prep.fused_embedding = False
    assert prep._fused(ids) is None


def test_language_model_switches_and_state_dict():
    from perceiverio_pytorch_amd.io_processors import EmbeddingPreprocessor
    from perceiverio_pytorch_amd.models import LanguagePerceiver
    model = small_language_model()
    prep = model.perceiver._multi_preprocessor._preprocessors["__default"]
    assert isinstance(prep, EmbeddingPreprocessor) and prep.need_tokens is False and prep.fused_embedding is True
    assert isinstance(LanguagePerceiver.fused_front_end, property)
    assert model.fused_front_end is True
    model.fused_front_end = False
    assert model.fused_front_end is False and prep.fused_embedding is False
    assert EmbeddingPreprocessor.fused_embedding is True          # (the instance's switch, not the class's)
    model.fused_front_end = 1
    assert model.fused_front_end is True and prep.fused_embedding is True
    # the switches and the flag word are plain attributes: parameters, buffers and state_dict keys are what they were
    keys = list(model.state_dict())
    assert "perceiver._multi_preprocessor._preprocessors.__default.embed.weight" in keys
    assert "perceiver._multi_preprocessor._preprocessors.__default.input_pos_encoding.pos_embs" in keys
    assert sorted(k.rsplit(".", 1)[-1] for k in keys if "_preprocessors" in k) == ["pos_embs", "weight"]
    assert not list(prep.buffers())


def test_full_size_state_dict_keys_equal_the_golden():
    from _golden import load
    from test_models import build, spec_of
    ref = dict(spec_of(load("model_language")))
    model = build("model_language")
    assert model.perceiver._multi_preprocessor._preprocessors["__default"].need_tokens is False
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == ref


def test_language_model_on_cpu_equals_itself_with_the_switch_off():
    """Under the torch backend on CPU tensors the switch changes nothing: both settings run the chain."""
    import perceiverio_pytorch_amd as P
    torch.manual_seed(3)
    model = small_language_model().eval()
    ids = torch.randint(0, 11, (2, 6))
    mask = torch.ones(2, 6)
    prev = P.get_backend()
    P.set_backend("torch")
    try:
        with torch.no_grad():
            a = model(ids, mask)
            model.fused_front_end = False
            b = model(ids, mask)
    finally:
        P.set_backend(prev)
    assert a.shape == (2, 6, 11) and torch.equal(a, b)
