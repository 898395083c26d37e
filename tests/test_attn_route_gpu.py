"""GPU: ties perceiverio_pytorch_amd/csrc/pio_attn_route.h to what pio_attention_fwd actually launches, through the
library's pio_prof_begin / pio_prof_end accounting (class 5 = fused attention cores, class 3 = softmax_rows of the
materialised path).  The expected counts are literals: they are not computed by calling the route.  Numerical parity of
these paths is held by tests/test_parity_gpu.py and tests/test_qk_pair_gpu.py; here the output only has to be finite.
(A 256-wide single head is inside the cross-attention kernel's <352, 352> instantiation, whatever the key count; the
tall-head kernel takes heads beyond its tables, hence the 1024-wide case.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import perceiver_oracle as O

pytestmark = pytest.mark.gpu

B = 2
CASES = [
    # id, heads, qk channels, v channels, Tq, Tk, mask, policy, fused-core launches, softmax_rows launches (None: >= 1)
    ("heads_32_32_plain", 2, 64, 64, 128, 128, None, "fp16", 1, 0),          # self-attention kernel (V^T form)
    ("heads_32_32_kv_mask", 2, 64, 64, 128, 128, "kv", "fp16", 1, 0),        # mask vector: cross-attention kernel
    ("heads_32_32_full_mask", 2, 64, 64, 128, 128, "full", "fp16", 0, None),  # needs the score matrix
    ("wide_256_over_96", 1, 256, 256, 128, 96, None, "fp16", 1, 0),          # one wide head over few keys
    ("tall_1024_over_96", 1, 1024, 1024, 128, 96, None, "fp16", 1, 0),       # wider than the tiled kernel: xattn_tall_kernel
    ("wide_328_over_160", 1, 328, 328, 128, 160, None, "fp16", 1, 0),        # cross-attention kernel <352, 352>
    ("heads_32_32_act_split_1", 2, 64, 64, 128, 128, None, "fp16x3", 0, None),  # split operands everywhere: materialised
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_attention_fwd_launches_the_routed_core(dev, case):
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    name, H, qk, vv, Tq, Tk, mask, policy, want_fused, want_softmax = case
    cin = 64
    p = O.gen_attention("", cin, cin, qk, vv, cin, seed=len(name) + Tk)
    m = Attention(cin, cin, cin, num_heads=H, qk_out_channels=qk, v_out_channels=vv, output_channels=cin)
    m.load_state_dict({k: torch.from_numpy(a) for k, a in p.items()})
    m = m.to(dev).eval()
    rng = np.random.default_rng(Tq + Tk + H)
    same = Tq == Tk                                         # q, k and v read the same input where the shapes allow it
    xkv = torch.from_numpy(rng.standard_normal((B, Tk, cin)).astype(np.float32)).to(dev)
    xq = xkv if same else torch.from_numpy(rng.standard_normal((B, Tq, cin)).astype(np.float32)).to(dev)
    km = fm = None
    if mask == "kv":
        k = rng.random((B, Tk)) > 0.3
        k[:, 0] = True
        km = torch.from_numpy(k).to(dev).view(torch.uint8)
    elif mask == "full":
        f = rng.random((B, Tq, Tk)) > 0.3
        f[:, :, 0] = True
        fm = torch.from_numpy(f).to(dev).view(torch.uint8)
    lib = P.lib()
    prev = R.get_precision_policy()
    P.set_precision_policy(policy)
    try:
        d = m._desc()
        assert d.act_split == (1 if policy == "fp16x3" else 0) and d.dtype == L.PIO_DT_F16
        out = torch.full((B, Tq, cin), float("nan"), dtype=torch.float32, device=dev)
        ws = R.workspace(dev, lib.pio_attention_workspace_bytes(d, B, Tq, Tk))
        L.check(lib.pio_prof_begin(64), "pio_prof_begin")
        try:
            L.check(lib.pio_attention_fwd(d, R.tensor3(xq), R.tensor3(xkv), R.tensor3(xkv),
                                          km.data_ptr() if km is not None else None, None,
                                          fm.data_ptr() if fm is not None else None, None, out.data_ptr(), None,
                                          ws.data_ptr(), ws.numel(), R.stream_ptr(dev)), "pio_attention_fwd")
        finally:
            launches = (C.c_int64 * 9)()
            assert lib.pio_prof_end(None, None, None, launches) >= 0
        torch.cuda.synchronize()
    finally:
        P.set_precision_policy(prev)
    print(f"{name}: fused-core launches={launches[5]} softmax_rows={launches[3]} batched GEMMs={launches[1]}")
    assert launches[5] == want_fused, (name, list(launches))
    if want_softmax is None:
        assert launches[3] >= 1, (name, list(launches))
    else:
        assert launches[3] == want_softmax, (name, list(launches))
    assert torch.isfinite(out).all()
