"""GPU: ties perceiverio_pytorch_amd/csrc/pio_block_route.h to what pio_self_attention_fwd actually launches, through
the library's pio_prof_begin / pio_prof_end accounting: an un-folded SelfAttention block runs two LayerNorm-cast passes
and four flat tile GEMMs, a folded one a single row-statistics cast and its four GEMMs on the tile kernels (small family)
or on the 256 x 256-tile kernel (wide family); split activations ("fp16x3") take the materialised attention path.  The expected per-class launch counts are literals: they are not computed by calling
the route.  Numerical parity of these paths is held by test_self_attention_layernorm_fold and its neighbours in
tests/test_parity_gpu.py; here the output only has to be finite."""
import ctypes as C

import numpy as np
import pytest
import torch

import perceiver_oracle as O

pytestmark = pytest.mark.gpu

D, HEADS = 512, 8
# launch classes (pio_internal.h): 0 gemm_nt_256, 1 batched gemm_nt_128, 2 layernorm / casts, 3 softmax_rows, 4 pack,
# 5 fused attention cores, 6 flat gemm_nt_128, 7 gemm_nt_stream, 8 gemm_nt_wide
# Counts: one run of this test body against the library of commit 20d166f (the parent of the move) on an MI355X.
CASES = [
    # id, B, N, per-call ln_fold (0: the process-wide default), policy, launches per class
    ("rows_256_default_unfolded", 1, 256, 0, "fp16", [0, 0, 2, 0, 0, 1, 4, 0, 0]),
    ("rows_512_default_small_family", 1, 512, 0, "fp16", [0, 0, 1, 0, 0, 1, 4, 0, 0]),
    ("rows_2048_forced_wide_family", 1, 2048, 3, "fp16", [0, 0, 1, 0, 0, 1, 0, 0, 4]),
    ("rows_2048_fold_off_unfolded", 1, 2048, 1, "fp16", [0, 0, 2, 0, 0, 1, 4, 0, 0]),
    ("rows_512_fp16x3_unfolded", 1, 512, 0, "fp16x3", [0, 2, 2, 1, 0, 0, 6, 0, 0]),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_self_attention_fwd_launches_the_routed_family(dev, case):
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import SelfAttention
    name, B, N, ln_fold, policy, want = case
    p = O.gen_self_attention("", D, seed=7)
    m = SelfAttention(D, widening_factor=1, num_heads=HEADS)
    m.load_state_dict({k: torch.from_numpy(a) for k, a in p.items()})
    m = m.to(dev).eval()
    x = torch.from_numpy(np.random.default_rng(N).standard_normal((B, N, D)).astype(np.float32)).to(dev)
    lib = P.lib()
    prev = R.get_precision_policy()
    P.set_precision_policy(policy)
    try:
        d = m._desc()
        assert d.attn.act_split == (1 if policy == "fp16x3" else 0) and d.attn.dtype == L.PIO_DT_F16
        assert (d.attn.heads, d.attn.dkp, d.attn.dvp) == (HEADS, 64, 64)
        out = torch.full((B, N, D), float("nan"), dtype=torch.float32, device=dev)
        ws = R.workspace(dev, lib.pio_self_attention_workspace_bytes(d, B, N))
        opts = L.CallOpts(ln_fold, 0)
        L.check(lib.pio_prof_begin(64), "pio_prof_begin")
        try:
            L.check(lib.pio_self_attention_fwd(d, R.tensor3(x), None, None, None, None, out.data_ptr(), None,
                                               C.byref(opts), ws.data_ptr(), ws.numel(), R.stream_ptr(dev)),
                    "pio_self_attention_fwd")
        finally:
            launches = (C.c_int64 * 9)()
            assert lib.pio_prof_end(None, None, None, launches) >= 0
        torch.cuda.synchronize()
    finally:
        P.set_precision_policy(prev)
    print(f"{name}: launches per class = {list(launches)}")
    assert list(launches) == want, (name, list(launches))
    assert torch.isfinite(out).all()
