"""CPU: what every precision policy decides, as a literal.  The table was printed from the five parallel structures the
policies were made of before they became one record each (commit bd59e02: a tuple with a numeric weight level, three name
sets and a dict beside it, and the comparisons against the level at the packing sites); the questions of runtime.py must
answer it row by row."""
import pytest

from perceiverio_pytorch_amd import _lib as L, runtime as R

NAMES = ("proj_q", "proj_k", "proj_v", "final", "fc1", "fc2", "final_layer", "post")
# policy: (weights split, in the order of NAMES; act_split; block feedback; K/V fold offered; LayerNorm fold offered)
TABLE = {
    "fp16":      ("00000000", 0, 0, 1, 1), "bf16":      ("00000000", 0, 0, 1, 1),
    "fp16sd":    ("00000000", 0, 1, 1, 1),
    "fp16x2o":   ("00010000", 0, 0, 1, 1),
    "fp16x2v":   ("00100000", 0, 0, 1, 1),
    "fp16x2s":   ("00110000", 0, 0, 0, 1),
    "fp16x2w":   ("00111111", 0, 0, 0, 1), "bf16x2w":   ("00111111", 0, 0, 0, 1),
    "fp16x2af":  ("00000000", 2, 0, 1, 0),
    "fp16x2afo": ("00010011", 2, 0, 1, 0),
    "fp16x3":    ("11111111", 1, 0, 0, 0), "bf16x3":    ("11111111", 1, 0, 0, 0),
    "fp16x3f":   ("11111111", 2, 0, 0, 0), "bf16x3f":   ("11111111", 2, 0, 0, 0),
    "fp16x3fq":  ("11111111", 3, 0, 0, 0),
}


def _weights(name):
    return "".join(str(int(R.splits(lin, name))) for lin in NAMES)


def test_the_table_names_every_policy():
    assert sorted(TABLE) == sorted(R._POLICIES) and len(TABLE) == 15


@pytest.mark.parametrize("name", sorted(TABLE))
def test_policy_row(name, monkeypatch):
    monkeypatch.delenv("PIO_EXTRA_SPLIT", raising=False)
    weights, act_split, feedback, kv_fold, ln_fold = TABLE[name]
    p = R.policy(name)
    assert _weights(name) == weights
    assert p.split == frozenset(lin for lin, c in zip(NAMES, weights) if c == "1")
    assert R.attention_act_split(name) == act_split
    assert R.policy_dtype(name) == (L.PIO_DT_BF16 if name.startswith("bf16") else L.PIO_DT_F16, act_split != 0)
    assert p.core == ("materialised", "materialised", "fused", "fused_pair")[act_split]
    assert p.feedback == bool(feedback)
    assert R.kv_fold_offered(name) == bool(kv_fold)
    assert R.ln_fold_offered(name) == bool(ln_fold)
    # q | k | v may share one image exactly where proj_q / proj_k are single
    assert R.qkv_stack_allowed(name) == (weights[:2] == "00")
    # the ambient policy answers the same as the named one
    with R.precision(name):
        assert _weights(None) == weights and R.attention_act_split() == act_split and R.policy() is p


def test_extra_split_adds_exactly_its_names(monkeypatch):
    monkeypatch.setenv("PIO_EXTRA_SPLIT", "fc1,post")        # (read per call)
    assert _weights("fp16") == "00001001"
    assert _weights("fp16x2o") == "00011001" and _weights("fp16x3") == "11111111"
    assert R.kv_fold_offered("fp16") and R.ln_fold_offered("fp16") and R.qkv_stack_allowed("fp16")
    monkeypatch.setenv("PIO_EXTRA_SPLIT", "")
    assert _weights("fp16") == "00000000"


def test_unknown_name_raises_the_same_messages():
    names = sorted(R._POLICIES)
    with pytest.raises(ValueError) as e:
        R.set_precision_policy("fp8")
    assert str(e.value) == f"unknown precision policy 'fp8'; choose from {names}"
    with pytest.raises(ValueError) as e:
        R.precision("fp8")
    assert str(e.value) == f"unknown precision policy 'fp8'; choose from {names}"
    assert R.precision(None)._name is None
    with pytest.raises(ValueError) as e:
        R._known("fp8", "PIO_PRECISION={name!r} not in {names}")       # (the read of the variable at import)
    assert str(e.value) == f"PIO_PRECISION='fp8' not in {names}"


def test_torch_dtype_and_the_string_grammar_live_beside_the_table():
    import torch
    from perceiverio_pytorch_amd import models as M
    assert R.torch_dtype(L.PIO_DT_F16) is torch.float16 and R.torch_dtype(L.PIO_DT_BF16) is torch.bfloat16
    assert M.split_policy3 is R.split_policy3 and M.split_policy is R.split_policy
    assert R.split_policy3("a/b/c") == ("a", "b", "c") and R.split_policy3("a/b") == (None, "a", "b")
    assert R.split_policy3("a") == (None, "a", "a") and R.split_policy(None) == (None, None)
    with pytest.raises(ValueError):
        R.split_policy3("a/b/c/d")
