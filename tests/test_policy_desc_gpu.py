"""GPU: the descriptors the three block modules hand to the library under each of the 15 precision policies, and one
forward of a 512-channel self-attend block under four of them.

EXPECTED and tests/golden/policy_block_<policy>.npz were recorded ONCE from commit bd59e02 (the last one whose policies were
five parallel structures compared against a weight level at the packing sites): that tree's Python printed `record()` and
saved `block_forward()`, with this file's functions.  They are not regenerated from the code under test.

The shapes: SelfAttention(512 channels, 8 heads, widening factor 1) is the smallest block in which the LayerNorm fold, the
q|k stack and the q|k|v stack can all appear (64-wide heads, C % 256 == 0); CrossAttention(64, 64, one head) the smallest
that offers the K / V projection fold; PerceiverDecoder(64, 10, 64) adds final_layer."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FORWARD_POLICIES = ("fp16", "fp16x2s", "fp16x2afo", "fp16x3fq")


def modules():
    from perceiverio_pytorch_amd.perceiver import PerceiverDecoder
    from perceiverio_pytorch_amd.transformer_primitives import CrossAttention, SelfAttention
    dev = torch.device("cuda:0")
    sa = SelfAttention(in_channels=512, num_heads=8, widening_factor=1)
    fill(sa, 11)
    ca = CrossAttention(q_in_channels=64, kv_in_channels=64, num_heads=1)
    dec = PerceiverDecoder(query_channels=64, final_project_out_channels=10, num_latent_channels=64)
    return sa.to(dev).eval(), ca.to(dev).eval(), dec.to(dev).eval()


def fill(module, seed):
    """Parameters from numpy's legacy generator (the same bits everywhere): weights ~ N(0, 1 / fan_in), LayerNorm gains
    around 1, small biases."""
    rng = np.random.RandomState(seed)
    with torch.no_grad():
        for name, p in sorted(module.named_parameters()):
            a = rng.standard_normal(tuple(p.shape)).astype(np.float32)
            if p.dim() == 2:
                a /= np.sqrt(p.shape[1]).astype(np.float32)
            elif "layer_norm" in name and name.endswith("weight"):
                a = 1 + 0.1 * a
            else:
                a *= 0.1
            p.copy_(torch.from_numpy(a))


def lin(d):
    """n x k, "+lo" when the image has a lo half, "@" the first row that has one; "-" for a descriptor that is not there."""
    return f"{d.n}x{d.k}{'+lo' if d.w_lo else ''}@{d.lo_row0}" if d.w_hi else "-"


def attn(a):
    names = ("q", "k", "v", "o", "qk", "qkv", "kq", "vo")
    return f"act{a.act_split} dt{a.dtype} " + " ".join(f"{n}={lin(getattr(a, n))}" for n in names)


def mlp(m):
    return f"act{m.act_split} dt{m.dtype} fc1={lin(m.fc1)} fc2={lin(m.fc2)}"


def self_sig(d):
    return f"{attn(d.attn)} | {mlp(d.mlp)} | fold.qkv={lin(d.fold.qkv)} fold.fc1={lin(d.fold.fc1)}"


def record(sa, ca, dec):
    """{policy: {module: signature}} over every policy of the table."""
    from perceiverio_pytorch_amd import runtime as R
    out = {}
    for name in sorted(R._POLICIES):
        with R.precision(name):
            c, dc = ca._desc(), dec.decoding_cross_attn._desc()
            out[name] = {"self": self_sig(sa._desc()), "cross": f"{attn(c.attn)} | {mlp(c.mlp)}",
                         "decoder": f"{attn(dc.attn)} | {mlp(dc.mlp)} | final_layer={lin(dec._final_desc().desc)}"}
            if name == "fp16sd":
                out[name]["blocks"] = [self_sig(d) for d in sa._desc_blocks(2)]
    return out


def block_forward(sa, policy):
    from perceiverio_pytorch_amd import runtime as R
    x = torch.from_numpy(np.random.RandomState(5).standard_normal((1, 128, 512)).astype(np.float32)).to("cuda:0")
    with torch.inference_mode(), R.precision(policy):
        y = sa(x)
    torch.cuda.synchronize()
    return y.cpu().numpy()


# ---- recorded from commit bd59e02 ------------------------------------------------------------------------------------
EXPECTED = {'bf16': {'cross': 'act0 dt1 q=64x64@0 k=64x64@0 v=64x64@0 o=64x64@0 qk=128x64@0 qkv=192x64@0 kq=64x64+lo@0 '
                   'vo=64x64+lo@0 | act0 dt1 fc1=64x64@0 fc2=64x64@0',
          'decoder': 'act0 dt1 q=64x64@0 k=64x64@0 v=64x64@0 o=64x64@0 qk=128x64@0 qkv=192x64@0 kq=64x64+lo@0 '
                     'vo=64x64+lo@0 | act0 dt1 fc1=64x64@0 fc2=64x64@0 | final_layer=16x64@0',
          'self': 'act0 dt1 q=512x512@0 k=512x512@0 v=512x512@0 o=512x512@0 qk=1024x512@0 qkv=1536x512@0 kq=- vo=- | '
                  'act0 dt1 fc1=512x512@0 fc2=512x512@0 | fold.qkv=1536x512@0 fold.fc1=512x512@0'},
 'bf16x2w': {'cross': 'act0 dt1 q=64x64@0 k=64x64@0 v=64x64+lo@0 o=64x64+lo@0 qk=128x64@0 qkv=- kq=- vo=- | act0 dt1 '
                      'fc1=64x64+lo@0 fc2=64x64+lo@0',
             'decoder': 'act0 dt1 q=64x64@0 k=64x64@0 v=64x64+lo@0 o=64x64+lo@0 qk=128x64@0 qkv=- kq=- vo=- | act0 '
                        'dt1 fc1=64x64+lo@0 fc2=64x64+lo@0 | final_layer=16x64+lo@0',
             'self': 'act0 dt1 q=512x512@0 k=512x512@0 v=512x512+lo@0 o=512x512+lo@0 qk=1024x512@0 '
                     'qkv=1536x512+lo@1024 kq=- vo=- | act0 dt1 fc1=512x512+lo@0 fc2=512x512+lo@0 | '
                     'fold.qkv=1536x512+lo@1024 fold.fc1=512x512+lo@0'},
 'bf16x3': {'cross': 'act1 dt1 q=64x64+lo@0 k=64x64+lo@0 v=64x64+lo@0 o=64x64+lo@0 qk=- qkv=- kq=- vo=- | act1 dt1 '
                     'fc1=64x64+lo@0 fc2=64x64+lo@0',
            'decoder': 'act1 dt1 q=64x64+lo@0 k=64x64+lo@0 v=64x64+lo@0 o=64x64+lo@0 qk=- qkv=- kq=- vo=- | act1 dt1 '
                       'fc1=64x64+lo@0 fc2=64x64+lo@0 | final_layer=16x64+lo@0',
            'self': 'act1 dt1 q=512x512+lo@0 k=512x512+lo@0 v=512x512+lo@0 o=512x512+lo@0 qk=- qkv=- kq=- vo=- | '
                    'act1 dt1 fc1=512x512+lo@0 fc2=512x512+lo@0 | fold.qkv=- fold.fc1=-'},
 'bf16x3f': {'cross': 'act2 dt1 q=64x64+lo@0 k=64x64+lo@0 v=64x64+lo@0 o=64x64+lo@0 qk=- qkv=- kq=- vo=- | act1 dt1 '
                      'fc1=64x64+lo@0 fc2=64x64+lo@0',
             'decoder': 'act2 dt1 q=64x64+lo@0 k=64x64+lo@0 v=64x64+lo@0 o=64x64+lo@0 qk=- qkv=- kq=- vo=- | act1 '
                        'dt1 fc1=64x64+lo@0 fc2=64x64+lo@0 | final_layer=16x64+lo@0',
             'self': 'act2 dt1 q=512x512+lo@0 k=512x512+lo@0 v=512x512+lo@0 o=512x512+lo@0 qk=- qkv=- kq=- vo=- | '
                     'act1 dt1 fc1=512x512+lo@0 fc2=512x512+lo@0 | fold.qkv=- fold.fc1=-'},
 'fp16': {'cross': 'act0 dt0 q=64x64@0 k=64x64@0 v=64x64@0 o=64x64@0 qk=128x64@0 qkv=192x64@0 kq=64x64+lo@0 '
                   'vo=64x64+lo@0 | act0 dt0 fc1=64x64@0 fc2=64x64@0',
          'decoder': 'act0 dt0 q=64x64@0 k=64x64@0 v=64x64@0 o=64x64@0 qk=128x64@0 qkv=192x64@0 kq=64x64+lo@0 '
                     'vo=64x64+lo@0 | act0 dt0 fc1=64x64@0 fc2=64x64@0 | final_layer=16x64@0',
          'self': 'act0 dt0 q=512x512@0 k=512x512@0 v=512x512@0 o=512x512@0 qk=1024x512@0 qkv=1536x512@0 kq=- vo=- | '
                  'act0 dt0 fc1=512x512@0 fc2=512x512@0 | fold.qkv=1536x512@0 fold.fc1=512x512@0'},
 'fp16sd': {'blocks': ['act0 dt0 q=512x512@0 k=512x512@0 v=512x512@0 o=512x512@0 qk=1024x512@0 qkv=1536x512@0 kq=- '
                       'vo=- | act0 dt0 fc1=512x512@0 fc2=512x512@0 | fold.qkv=1536x512@0 fold.fc1=512x512@0',
                       'act0 dt0 q=512x512@0 k=512x512@0 v=512x512@0 o=512x512@0 qk=1024x512@0 qkv=1536x512@0 kq=- '
                       'vo=- | act0 dt0 fc1=512x512@0 fc2=512x512@0 | fold.qkv=1536x512@0 fold.fc1=512x512@0'],
            'cross': 'act0 dt0 q=64x64@0 k=64x64@0 v=64x64@0 o=64x64@0 qk=128x64@0 qkv=192x64@0 kq=64x64+lo@0 '
                     'vo=64x64+lo@0 | act0 dt0 fc1=64x64@0 fc2=64x64@0',
            'decoder': 'act0 dt0 q=64x64@0 k=64x64@0 v=64x64@0 o=64x64@0 qk=128x64@0 qkv=192x64@0 kq=64x64+lo@0 '
                       'vo=64x64+lo@0 | act0 dt0 fc1=64x64@0 fc2=64x64@0 | final_layer=16x64@0',
            'self': 'act0 dt0 q=512x512@0 k=512x512@0 v=512x512@0 o=512x512@0 qk=1024x512@0 qkv=1536x512@0 kq=- vo=- '
                    '| act0 dt0 fc1=512x512@0 fc2=512x512@0 | fold.qkv=1536x512@0 fold.fc1=512x512@0'},
 'fp16x2af': {'cross': 'act2 dt0 q=64x64@0 k=64x64@0 v=64x64@0 o=64x64@0 qk=- qkv=- kq=64x64+lo@0 vo=64x64+lo@0 | '
                       'act1 dt0 fc1=64x64@0 fc2=64x64@0',
              'decoder': 'act2 dt0 q=64x64@0 k=64x64@0 v=64x64@0 o=64x64@0 qk=- qkv=- kq=64x64+lo@0 vo=64x64+lo@0 | '
                         'act1 dt0 fc1=64x64@0 fc2=64x64@0 | final_layer=16x64@0',
              'self': 'act2 dt0 q=512x512@0 k=512x512@0 v=512x512@0 o=512x512@0 qk=- qkv=- kq=- vo=- | act1 dt0 '
                      'fc1=512x512@0 fc2=512x512@0 | fold.qkv=- fold.fc1=-'},
 'fp16x2afo': {'cross': 'act2 dt0 q=64x64@0 k=64x64@0 v=64x64@0 o=64x64+lo@0 qk=- qkv=- kq=64x64+lo@0 vo=64x64+lo@0 '
                        '| act1 dt0 fc1=64x64@0 fc2=64x64@0',
               'decoder': 'act2 dt0 q=64x64@0 k=64x64@0 v=64x64@0 o=64x64+lo@0 qk=- qkv=- kq=64x64+lo@0 '
                          'vo=64x64+lo@0 | act1 dt0 fc1=64x64@0 fc2=64x64@0 | final_layer=16x64+lo@0',
               'self': 'act2 dt0 q=512x512@0 k=512x512@0 v=512x512@0 o=512x512+lo@0 qk=- qkv=- kq=- vo=- | act1 dt0 '
                       'fc1=512x512@0 fc2=512x512@0 | fold.qkv=- fold.fc1=-'},
 'fp16x2o': {'cross': 'act0 dt0 q=64x64@0 k=64x64@0 v=64x64@0 o=64x64+lo@0 qk=128x64@0 qkv=192x64@0 kq=64x64+lo@0 '
                      'vo=64x64+lo@0 | act0 dt0 fc1=64x64@0 fc2=64x64@0',
             'decoder': 'act0 dt0 q=64x64@0 k=64x64@0 v=64x64@0 o=64x64+lo@0 qk=128x64@0 qkv=192x64@0 kq=64x64+lo@0 '
                        'vo=64x64+lo@0 | act0 dt0 fc1=64x64@0 fc2=64x64@0 | final_layer=16x64@0',
             'self': 'act0 dt0 q=512x512@0 k=512x512@0 v=512x512@0 o=512x512+lo@0 qk=1024x512@0 qkv=1536x512@0 kq=- '
                     'vo=- | act0 dt0 fc1=512x512@0 fc2=512x512@0 | fold.qkv=1536x512@0 fold.fc1=512x512@0'},
 'fp16x2s': {'cross': 'act0 dt0 q=64x64@0 k=64x64@0 v=64x64+lo@0 o=64x64+lo@0 qk=128x64@0 qkv=- kq=- vo=- | act0 dt0 '
                      'fc1=64x64@0 fc2=64x64@0',
             'decoder': 'act0 dt0 q=64x64@0 k=64x64@0 v=64x64+lo@0 o=64x64+lo@0 qk=128x64@0 qkv=- kq=- vo=- | act0 '
                        'dt0 fc1=64x64@0 fc2=64x64@0 | final_layer=16x64@0',
             'self': 'act0 dt0 q=512x512@0 k=512x512@0 v=512x512+lo@0 o=512x512+lo@0 qk=1024x512@0 '
                     'qkv=1536x512+lo@1024 kq=- vo=- | act0 dt0 fc1=512x512@0 fc2=512x512@0 | '
                     'fold.qkv=1536x512+lo@1024 fold.fc1=512x512@0'},
 'fp16x2v': {'cross': 'act0 dt0 q=64x64@0 k=64x64@0 v=64x64+lo@0 o=64x64@0 qk=128x64@0 qkv=- kq=64x64+lo@0 '
                      'vo=64x64+lo@0 | act0 dt0 fc1=64x64@0 fc2=64x64@0',
             'decoder': 'act0 dt0 q=64x64@0 k=64x64@0 v=64x64+lo@0 o=64x64@0 qk=128x64@0 qkv=- kq=64x64+lo@0 '
                        'vo=64x64+lo@0 | act0 dt0 fc1=64x64@0 fc2=64x64@0 | final_layer=16x64@0',
             'self': 'act0 dt0 q=512x512@0 k=512x512@0 v=512x512+lo@0 o=512x512@0 qk=1024x512@0 qkv=1536x512+lo@1024 '
                     'kq=- vo=- | act0 dt0 fc1=512x512@0 fc2=512x512@0 | fold.qkv=1536x512+lo@1024 '
                     'fold.fc1=512x512@0'},
 'fp16x2w': {'cross': 'act0 dt0 q=64x64@0 k=64x64@0 v=64x64+lo@0 o=64x64+lo@0 qk=128x64@0 qkv=- kq=- vo=- | act0 dt0 '
                      'fc1=64x64+lo@0 fc2=64x64+lo@0',
             'decoder': 'act0 dt0 q=64x64@0 k=64x64@0 v=64x64+lo@0 o=64x64+lo@0 qk=128x64@0 qkv=- kq=- vo=- | act0 '
                        'dt0 fc1=64x64+lo@0 fc2=64x64+lo@0 | final_layer=16x64+lo@0',
             'self': 'act0 dt0 q=512x512@0 k=512x512@0 v=512x512+lo@0 o=512x512+lo@0 qk=1024x512@0 '
                     'qkv=1536x512+lo@1024 kq=- vo=- | act0 dt0 fc1=512x512+lo@0 fc2=512x512+lo@0 | '
                     'fold.qkv=1536x512+lo@1024 fold.fc1=512x512+lo@0'},
 'fp16x3': {'cross': 'act1 dt0 q=64x64+lo@0 k=64x64+lo@0 v=64x64+lo@0 o=64x64+lo@0 qk=- qkv=- kq=- vo=- | act1 dt0 '
                     'fc1=64x64+lo@0 fc2=64x64+lo@0',
            'decoder': 'act1 dt0 q=64x64+lo@0 k=64x64+lo@0 v=64x64+lo@0 o=64x64+lo@0 qk=- qkv=- kq=- vo=- | act1 dt0 '
                       'fc1=64x64+lo@0 fc2=64x64+lo@0 | final_layer=16x64+lo@0',
            'self': 'act1 dt0 q=512x512+lo@0 k=512x512+lo@0 v=512x512+lo@0 o=512x512+lo@0 qk=- qkv=- kq=- vo=- | '
                    'act1 dt0 fc1=512x512+lo@0 fc2=512x512+lo@0 | fold.qkv=- fold.fc1=-'},
 'fp16x3f': {'cross': 'act2 dt0 q=64x64+lo@0 k=64x64+lo@0 v=64x64+lo@0 o=64x64+lo@0 qk=- qkv=- kq=- vo=- | act1 dt0 '
                      'fc1=64x64+lo@0 fc2=64x64+lo@0',
             'decoder': 'act2 dt0 q=64x64+lo@0 k=64x64+lo@0 v=64x64+lo@0 o=64x64+lo@0 qk=- qkv=- kq=- vo=- | act1 '
                        'dt0 fc1=64x64+lo@0 fc2=64x64+lo@0 | final_layer=16x64+lo@0',
             'self': 'act2 dt0 q=512x512+lo@0 k=512x512+lo@0 v=512x512+lo@0 o=512x512+lo@0 qk=- qkv=- kq=- vo=- | '
                     'act1 dt0 fc1=512x512+lo@0 fc2=512x512+lo@0 | fold.qkv=- fold.fc1=-'},
 'fp16x3fq': {'cross': 'act3 dt0 q=64x64+lo@0 k=64x64+lo@0 v=64x64+lo@0 o=64x64+lo@0 qk=- qkv=- kq=- vo=- | act1 dt0 '
                       'fc1=64x64+lo@0 fc2=64x64+lo@0',
              'decoder': 'act3 dt0 q=64x64+lo@0 k=64x64+lo@0 v=64x64+lo@0 o=64x64+lo@0 qk=- qkv=- kq=- vo=- | act1 '
                         'dt0 fc1=64x64+lo@0 fc2=64x64+lo@0 | final_layer=16x64+lo@0',
              'self': 'act3 dt0 q=512x512+lo@0 k=512x512+lo@0 v=512x512+lo@0 o=512x512+lo@0 qk=- qkv=- kq=- vo=- | '
                      'act1 dt0 fc1=512x512+lo@0 fc2=512x512+lo@0 | fold.qkv=- fold.fc1=-'}}  # noqa: E501


@pytest.fixture(scope="module")
def built():
    mods = modules()
    return mods, record(*mods)


@pytest.mark.gpu
def test_every_policy_has_a_record(built):
    assert sorted(built[1]) == sorted(EXPECTED) and len(EXPECTED) == 15


@pytest.mark.gpu
@pytest.mark.parametrize("policy", sorted(EXPECTED))
def test_descriptors_are_the_parents(built, policy):
    got = built[1][policy]
    for part, sig in EXPECTED[policy].items():
        print(policy, part, got[part])
        assert got[part] == sig, (policy, part)
    assert sorted(got) == sorted(EXPECTED[policy])


@pytest.mark.gpu
@pytest.mark.parametrize("policy", FORWARD_POLICIES)
def test_block_forward_is_bit_identical_to_the_parents(built, policy):
    want = np.load(os.path.join(GOLDEN, f"policy_block_{policy}.npz"))["out"]
    got = block_forward(built[0][0], policy)
    assert got.shape == want.shape == (1, 128, 512) and np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
