"""GPU parity tests proper: every call goes through the C-ABI of libpio_hip.so (via the nn.Module mirror or
raw ctypes) and is compared with the committed reference goldens and with the oracle on the same seeded
inputs.  Tolerance: 1e-3 on BOTH relL2 and max-abs/abs-max (BASELINE.json north_star), written here."""
import ctypes as C

import numpy as np
import pytest
import torch

import perceiver_oracle as O
from cases import ENCDEC_CASES, gen_encdec_inputs, encdec_kwargs
from _golden import load, params, ATTN, MLP, SA, CA, ENCDEC_FULL, ENCDEC_SUB

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the parity bar of north_star (relL2 AND max-abs/abs-max), every golden, default policy
TIGHT = 5e-5        # what the default policy (fp16x3: split operands, ~fp32 products) actually delivers
# Fast policies round operands to 11 bits; on the toy-sized goldens (D=32..64, no averaging over tokens or
# channels) that alone is ~1e-3 per few layers, so for THEM the bound asserted is the error budget below; on
# every realistically sized golden (and on the headline ImageNet config) they are held to TOL as well.
FAST_TOY_BUDGET = 3e-3
BF16_FUSED_TOL = 1e-2    # "bf16" through a fused attention core against the oracle (toy widths)
PROBS_ABS_TOL = 1e-5     # returned probability matrix under "fp16x3": largest absolute difference
POLICIES = ["fp16x3", "fp16x2w", "fp16x2s", "fp16"]
# goldens whose widths are those of real configurations (>= 256 channels, or the 322-wide single head, >= 45 keys)
REALISTIC = {"sa_mid_512x256_h8", "attn_h1_dim322", "ca_keymask", "encdec_mid", "encdec_lang_like",
             "encdec_imagenet_b2"}


def tol_for(policy, name=""):
    if policy == "fp16x3":
        return TIGHT
    return TOL if name in REALISTIC else FAST_TOY_BUDGET


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1, "libpio_hip.so targets gfx950 only"
    return torch.device("cuda:0")


def _policy(name):
    import perceiverio_pytorch_amd as P
    P.set_precision_policy(name)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sd(p, dev):
    return {k: _t(v, dev) for k, v in p.items()}


def _errs(y, ref):
    return O.rel_errors(y.detach().float().cpu().numpy(), ref)


def _assert_close(y, ref, tol=TOL, what=""):
    rl2, rmax = _errs(y, ref)
    assert rl2 <= tol and rmax <= tol, f"{what}: relL2={rl2:.3e} max/absmax={rmax:.3e} > {tol}"
    return rl2, rmax


# ----------------------------------------------------------------------------------------------------
# primitive kernels through raw ctypes
# (GEMM: arithmetic on dense layouts here; every stride / pitch / offset of pio_gemm_t, exactly: test_gemm_addr_gpu.py)
# ----------------------------------------------------------------------------------------------------
GEMM_SHAPES = [
    # M, N, K, batch, nh, bias_mode, act, residual, out_f32, lo
    (128, 128, 64, 1, 1, 0, 0, False, True, False),
    (200, 136, 72, 1, 1, 1, 0, False, True, False),       # tails in M, N and K (K % 64 != 0)
    (333, 1000, 1024, 1, 1, 1, 1, True, True, False),     # gelu + residual, fp32 out, ldc=1000
    (77, 48, 328, 6, 3, 2, 0, False, False, False),       # batched (b,h), per-row bias, 16-bit out
    (512, 512, 128, 4, 2, 0, 0, False, True, False),
    (300, 264, 1024, 1, 1, 1, 0, True, True, True),       # two-pass weights
    (1, 8, 8, 1, 1, 1, 0, False, True, False),            # degenerate
    # shapes routed to the 256x256-tile / 4-slot-ring kernel (M >= 1024, N >= 256)
    (2048, 1024, 1024, 1, 1, 1, 0, True, True, False),    # the self-attend projection shape (+ residual)
    (1100, 520, 328, 1, 1, 1, 1, False, False, False),    # ragged M / N / K tails, GELU, 16-bit out
    (1030, 1000, 72, 1, 1, 1, 0, True, True, True),       # fp32 ldc=1000, residual, two-pass weights, K=72
    (1024, 256, 40, 2, 1, 2, 0, False, True, False),      # batched, per-row bias, K < one ring (2 K tiles)
    (4096, 512, 1024, 1, 1, 1, 0, False, False, False),
    # tiles that own their CU alone run as two K teams of four waves (KG = 2: DESIGN_LOG R4.11)
    (1024, 1024, 1024, 1, 1, 1, 1, False, False, False),  # 256 tiles of 64 x 64, GELU, 16-bit out
    (1000, 1000, 1096, 1, 1, 1, 0, True, True, True),     # ... ragged M / N / K, residual, two-pass weights
    (1024, 3072, 1024, 1, 1, 1, 0, False, False, False),  # 192 tiles of 128 x 128 (the B = 2 q|k|v projection)
    (512, 1024, 2048, 1, 1, 1, 0, True, True, False),     # 256 tiles of 32 x 64, K = 2048
]


SKINNY_SHAPES = [
    # M, N, n_store, ldc, K, out_f32, a_lo, b_lo     (M >= 2048, n_store <= 4: gemm_nt_skinny)
    (182528 // 8, 2, 2, 2, 328, True, True, False),      # the flow decoder's final Linear (rows / 8), split activations
    (5000, 2, 2, 2, 328, True, True, True),              # + split weights (three K sweeps)
    (4099, 3, 4, 8, 1032, False, False, False),          # 16-bit out, pad column 3 written as zero, ldc > n_store, ragged M
    (2048, 4, 4, 4, 72, True, False, True),              # short K
    (3000, 1, 1, 1, 2048, True, True, False),            # one column; K = 2048: four chunks per lane
]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", SKINNY_SHAPES)
def test_gemm_nt_few_output_columns(dev, shape, dt):
    """Many rows x a handful of output columns (decoder final Linears with 2-8 outputs): pio_gemm_nt routes them to the
    row-per-wave kernel instead of a 128 x 128 tile; every K sweep (A_lo, B_lo), the bias, alpha, pad columns and the
    output forms against float64."""
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    M, N, n_store, ldc, K, out_f32, a_lo, b_lo = shape
    tdt = torch.float16 if dt == "f16" else torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(M + 13 * N + K)
    Af = torch.randn(M, K, generator=g) * 3.0
    Ahi = Af.to(tdt)
    Alo = (Af - Ahi.float()).to(tdt)
    Bf = torch.randn(N, K, generator=g) / K ** 0.5
    Bhi = Bf.to(tdt)
    Blo = (Bf - Bhi.float()).to(tdt)
    bias = torch.randn(N, generator=g)
    Cout = torch.full((M, ldc), float("nan"), dtype=torch.float32 if out_f32 else tdt)
    Ad, Ald, Bd, Bld, bd, Cd = (x.to(dev) for x in (Ahi, Alo, Bhi, Blo, bias, Cout))
    gm = L.Gemm()
    gm.A, gm.B, gm.C = Ad.data_ptr(), Bd.data_ptr(), Cd.data_ptr()
    gm.A_lo = Ald.data_ptr() if a_lo else None
    gm.B_lo = Bld.data_ptr() if b_lo else None
    gm.M, gm.N, gm.K = M, N, K
    gm.lda, gm.ldb, gm.ldc = K, K, ldc
    gm.batch, gm.nh = 1, 1
    gm.bias, gm.bias_mode, gm.act, gm.alpha = bd.data_ptr(), 1, 0, 0.75
    gm.out_f32, gm.n_store = int(out_f32), n_store
    gm.dtype = L.PIO_DT_F16 if dt == "f16" else L.PIO_DT_BF16
    L.check(lib.pio_gemm_nt(C.byref(gm), torch.cuda.current_stream().cuda_stream), "pio_gemm_nt")
    torch.cuda.synchronize()
    Aop = Ahi.double() + (Alo.double() if a_lo else 0)
    Bop = Bhi.double() + (Blo.double() if b_lo else 0)
    ref = 0.75 * (Aop @ Bop.T) + bias.double()[None, :]
    if a_lo and b_lo:
        ref = ref - 0.75 * (Alo.double() @ Blo.double().T)     # (the dropped lo x lo term)
    got = Cd.float().cpu().double()
    assert torch.isfinite(got[:, :n_store]).all()
    assert (got[:, N:n_store] == 0).all(), "pad columns must be written as zeros"
    assert torch.isnan(got[:, n_store:]).all(), "columns past n_store must not be touched"
    tol = 2e-5 if out_f32 else (1e-3 if dt == "f16" else 8e-3)
    err = (got[:, :N] - ref).abs().max() / ref.abs().max()
    assert err <= tol, f"skinny gemm {shape} {dt}: {err:.3e}"


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_gemm_nt(dev, shape, dt):
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    M, N, K, batch, nh, bias_mode, act, resid, out_f32, lo = shape
    tdt = torch.float16 if dt == "f16" else torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(M * 7 + N)
    A = torch.randn(batch, M, K, generator=g).to(tdt)
    Bm = (torch.randn(batch, N, K, generator=g) / K ** 0.5)
    Bhi = Bm.to(tdt)
    Blo = (Bm - Bhi.float()).to(tdt)
    bias = torch.randn(N if bias_mode == 1 else M, generator=g)
    Rm = torch.randn(batch, M, N, generator=g)
    ldc = N if out_f32 else (N + 7) // 8 * 8
    Cout = torch.full((batch, M, ldc), float("nan"), dtype=torch.float32 if out_f32 else tdt)
    Ad, Bd, Bld, bd, Rd, Cd = (x.to(dev) for x in (A, Bhi, Blo, bias, Rm, Cout))
    gm = L.Gemm()
    gm.A, gm.B, gm.C = Ad.data_ptr(), Bd.data_ptr(), Cd.data_ptr()
    gm.B_lo = Bld.data_ptr() if lo else None
    gm.M, gm.N, gm.K = M, N, K
    gm.lda, gm.ldb, gm.ldc = K, K, ldc
    gm.batch, gm.nh = batch, nh
    # z = zb*nh + zh over a [batch] array: stride_b = nh matrices, stride_h = 1 matrix
    gm.sAb, gm.sAh = nh * M * K, M * K
    gm.sBb, gm.sBh = nh * N * K, N * K
    gm.sCb, gm.sCh = nh * M * ldc, M * ldc
    gm.bias = bd.data_ptr() if bias_mode else None
    gm.bias_mode, gm.act, gm.alpha = bias_mode, act, 0.5
    if resid:
        assert batch == 1
        gm.R, gm.ldr = Rd.data_ptr(), N
    gm.out_f32, gm.n_store = int(out_f32), ldc
    gm.dtype = L.PIO_DT_F16 if dt == "f16" else L.PIO_DT_BF16
    L.check(lib.pio_gemm_nt(C.byref(gm), torch.cuda.current_stream().cuda_stream), "pio_gemm_nt")
    torch.cuda.synchronize()
    W = Bhi.double() + (Blo.double() if lo else 0)
    ref = 0.5 * torch.einsum("bmk,bnk->bmn", A.double(), W)
    if bias_mode == 1:
        ref = ref + bias.double()[None, None, :]
    elif bias_mode == 2:
        ref = ref + bias.double()[None, :, None]
    if act:
        ref = torch.nn.functional.gelu(ref)
    if resid:
        ref = ref + Rm.double()
    got = Cd.float().cpu().double()
    assert torch.isfinite(got[:, :, :N]).all()
    if not out_f32:
        assert (got[:, :, N:] == 0).all(), "pad columns must be written as zeros"
    tol = 2e-5 if out_f32 else (1e-3 if dt == "f16" else 8e-3)
    err = (got[:, :, :N] - ref).abs().max() / ref.abs().max()
    assert err <= tol, f"gemm {shape} {dt}: {err:.3e}"


STREAM_SHAPES = [
    # M, N, K, batch, bias, act, residual, out_f32, lo_weights, lo_out, force   (alpha = 1 with a residual)
    (16384, 1024, 1024, 1, 1, 0, False, False, False, False, False),  # 512 tiles: 2 per workgroup, 16-bit out
    (16384, 1024, 1024, 1, 1, 0, True, True, False, False, False),    # residual preloaded into the accumulators
    (4100, 3000, 1088, 1, 1, 1, False, False, False, False, True),    # ragged M / N, 17 K steps, GELU, uneven lists
    (3000, 520, 1024, 1, 1, 0, True, True, True, False, True),        # two K sweeps (32 steps), 60 tiles on 56 WGs
    (1024, 256, 1024, 1, 0, 0, False, False, False, True, True),      # hi + lo outputs, no bias, 8 tiles
    (2048, 256, 1024, 3, 1, 0, False, True, False, False, True),      # batched slices in the tile list
    (8192, 1024, 4096, 1, 1, 0, False, False, False, False, True),    # long K: 64 steps per tile, 1 tile per WG
    (2048, 1024, 1024, 1, 1, 1, False, False, False, True, True),     # GELU with hi + lo outputs
    (16384, 1024, 1024, 1, 0, 0, False, True, False, False, False),   # fp32 out, no bias, no residual
]


WIDE_SHAPES = [
    # (same fields; force = 2 selects the 256x256 four-wave kernel wherever it is legal)
    (16384, 3072, 1024, 1, 1, 0, False, False, False, False, 0),   # the fused q|k|v projection: 768 tiles, blocked walk
    (2048, 512, 128, 1, 1, 0, False, False, False, False, 2),      # shortest K (4 slices), 16 tiles on 16 workgroups
    (3000, 776, 192, 1, 1, 0, False, False, False, False, 2),      # ragged M and N, 6 slices, 48 tiles
    (5000, 2048, 320, 1, 0, 0, False, False, False, False, 2),     # no bias, 160 tiles on 160 WGs (linear walk)
    (9000, 2304, 256, 1, 1, 0, False, False, False, False, 2),     # 324 tiles on 256 WGs: uneven lists, linear walk
    (16384, 1024, 1024, 1, 1, 1, False, False, False, False, 2),   # fc1: GELU in the exposed epilogue, 1 tile per WG
    (2100, 520, 128, 1, 1, 1, False, False, False, False, 2),      # GELU on ragged edge tiles
    (16384, 1024, 1024, 1, 1, 0, True, True, False, False, 2),     # out / fc2: fp32 out + residual, 1 tile per WG
    (3000, 776, 192, 1, 1, 0, True, True, False, False, 2),        # fp32 + residual on ragged edge tiles
    (2048, 512, 128, 1, 0, 0, False, True, False, False, 2),       # fp32 out, no residual, no bias
    (8192, 1024, 512, 1, 1, 0, True, True, False, False, 2),       # fp32 + residual, 128 tiles on 128 workgroups
]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", WIDE_SHAPES)
def test_gemm_nt_wide(dev, shape, dt):
    """The persistent 256x256 four-wave kernel (pio_gemm_wide.hip) against torch fp64 on the same operands."""
    _gemm_case(dev, shape, dt, shape[-1], "wide")


WIDE_PAIR_SHAPES = [
    # M, N, K, act, out_f32, b_lo, c_lo, resid      (A always hi + lo: the dense decoders' split-activation GEMMs)
    (4096, 1024, 1024, 1, False, False, True, False),     # decoder fc1: GELU, hi + lo result
    (3000, 1026, 1088, 1, False, False, True, False),     # ... at the multimodal decoder's widths: ragged M, N = 4 x 256 + 2
    (2048, 1024, 512, 0, True, True, False, False),       # out projection / final Linear under "x2afo": three sweeps, fp32 out
    (2304, 520, 256, 0, False, True, True, False),        # three sweeps, hi + lo result, edge tiles
    (2048, 512, 128, 0, False, False, False, False),      # two sweeps, one 16-bit result
    (4096, 1024, 1024, 0, False, False, True, True),      # decoder fc2: fp32 residual in, hi + lo result
    (3000, 1032, 1088, 0, False, False, True, True),      # ... ragged, at the multimodal decoder's widths
]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", WIDE_PAIR_SHAPES)
def test_gemm_nt_wide_split_activations(dev, shape, dt):
    """gemm_nt_wide with an A_lo sweep (split activations), all three sweeps (+ split weights) and the hi + lo result of its
    plain 16-bit epilogue -- the forms the dense decoders' projections use -- against float64."""
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    M, N, K, act, out_f32, b_lo, c_lo, resid = shape
    tdt = torch.float16 if dt == "f16" else torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(M + 3 * N + K)
    Af = torch.randn(M, K, generator=g) * 2.0
    Ahi = Af.to(tdt)
    Alo = (Af - Ahi.float()).to(tdt)
    Bf = torch.randn(N, K, generator=g) / K ** 0.5
    Bhi = Bf.to(tdt)
    Blo = (Bf - Bhi.float()).to(tdt)
    bias = torch.randn(N, generator=g)
    ldc = N if out_f32 else (N + 7) // 8 * 8
    Cd = torch.full((M, ldc), float("nan"), dtype=torch.float32 if out_f32 else tdt, device=dev)
    Cl = torch.full_like(Cd, float("nan"))
    Ad, Ald, Bd, Bld, bd = (x.to(dev) for x in (Ahi, Alo, Bhi, Blo, bias))
    gm = L.Gemm()
    gm.A, gm.A_lo, gm.B, gm.C = Ad.data_ptr(), Ald.data_ptr(), Bd.data_ptr(), Cd.data_ptr()
    gm.B_lo = Bld.data_ptr() if b_lo else None
    gm.C_lo = Cl.data_ptr() if c_lo else None
    gm.M, gm.N, gm.K = M, N, K
    gm.lda, gm.ldb, gm.ldc = K, K, ldc
    gm.batch, gm.nh = 1, 1
    gm.bias, gm.bias_mode, gm.act, gm.alpha = bd.data_ptr(), 1, act, 1.0
    Rm = torch.randn(M, (N + 3) // 4 * 4, generator=g)
    Rd = Rm.to(dev)
    if resid:
        gm.R, gm.ldr = Rd.data_ptr(), Rm.shape[1]
    gm.out_f32, gm.n_store = int(out_f32), ldc
    gm.dtype = L.PIO_DT_F16 if dt == "f16" else L.PIO_DT_BF16
    prev = lib.pio_gemm_kernel_override(2)
    try:
        L.check(lib.pio_gemm_nt(C.byref(gm), torch.cuda.current_stream().cuda_stream), "pio_gemm_nt")
        torch.cuda.synchronize()
    finally:
        lib.pio_gemm_kernel_override(prev)
    Aop = Ahi.double() + Alo.double()
    Bop = Bhi.double() + (Blo.double() if b_lo else 0)
    ref = Aop @ Bop.T
    if b_lo:
        ref = ref - Alo.double() @ Blo.double().T       # (the dropped lo x lo term)
    ref = ref + bias.double()[None, :]
    if act:
        ref = torch.nn.functional.gelu(ref)
    if resid:
        ref = ref + Rm[:, :N].double()
    got = Cd.double().cpu()
    if c_lo:
        got = got + Cl.double().cpu()
    assert torch.isfinite(got[:, :N]).all()
    if not out_f32:
        assert (Cd[:, N:] == 0).all(), "pad columns must be written as zeros"
        if c_lo:
            assert (Cl[:, N:] == 0).all(), "pad columns of the lo image must be written as zeros"
    tol = 2e-5 if (out_f32 or c_lo) else (1e-3 if dt == "f16" else 8e-3)
    if dt == "bf16" and (out_f32 or c_lo):
        tol = 2e-4      # (bf16 pair: 16 mantissa bits)
    err = (got[:, :N] - ref).abs().max() / ref.abs().max()
    assert err <= tol, f"wide, split activations {shape} {dt}: {err:.3e}"


TILE_SHAPES = [
    # (same fields) small / ragged problems on BOTH instantiations of the 128-tile kernel: 128x128 tiles (override 128)
    # and the 64x64 tiles small batches get automatically (override 64)
    (300, 264, 1024, 1, 1, 0, True, True, True, False, 0),        # fp32 + residual, two-pass weights, ragged
    (2048, 512, 512, 1, 1, 1, False, False, False, False, 0),     # a flow-model latent projection at B = 1, GELU
    (100, 72, 40, 3, 1, 0, False, False, False, True, 0),         # batched, hi + lo outputs, K < one tile
    (65, 65, 8, 1, 0, 0, False, True, False, False, 0),           # one row / column past a 64 tile
]


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", TILE_SHAPES)
def test_gemm_nt_tile_sizes(dev, shape, dt, tile):
    """gemm_nt_128<.., 128, 128> and <.., 64, 64> against torch fp64 on the same operands."""
    _gemm_case(dev, shape, dt, tile, f"tile {tile}")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", STREAM_SHAPES)
def test_gemm_nt_stream(dev, shape, dt):
    """The persistent 256x128 streaming kernel (pio_gemm_stream.hip) against torch fp64 on the same operands."""
    _gemm_case(dev, shape, dt, 1 if shape[-1] else 0, "stream")


def _gemm_case(dev, shape, dt, override, what):
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    M, N, K, batch, bias_mode, act, resid, out_f32, lo_w, lo_out, force = shape
    tdt = torch.float16 if dt == "f16" else torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(M * 7 + N + K)
    A = torch.randn(batch, M, K, generator=g).to(tdt).to(dev)
    Bm = (torch.randn(batch, N, K, generator=g) / K ** 0.5).to(dev)
    Bhi = Bm.to(tdt)
    Blo = (Bm - Bhi.float()).to(tdt)
    bias = torch.randn(N, generator=g).to(dev)
    Rm = torch.randn(M, N, generator=g).to(dev)
    ldc = N if out_f32 else (N + 7) // 8 * 8
    Cd = torch.full((batch, M, ldc), float("nan"), dtype=torch.float32 if out_f32 else tdt, device=dev)
    Cl = torch.full_like(Cd, float("nan"))
    alpha = 1.0 if resid else 0.5
    gm = L.Gemm()
    gm.A, gm.B, gm.C = A.data_ptr(), Bhi.data_ptr(), Cd.data_ptr()
    gm.B_lo = Blo.data_ptr() if lo_w else None
    gm.C_lo = Cl.data_ptr() if lo_out else None
    gm.M, gm.N, gm.K = M, N, K
    gm.lda, gm.ldb, gm.ldc = K, K, ldc
    gm.batch, gm.nh = batch, 1
    gm.sAb, gm.sBb, gm.sCb = M * K, N * K, M * ldc
    gm.bias = bias.data_ptr() if bias_mode else None
    gm.bias_mode, gm.act, gm.alpha = bias_mode, act, alpha
    if resid:
        gm.R, gm.ldr = Rm.data_ptr(), N
    gm.out_f32, gm.n_store = int(out_f32), ldc
    gm.dtype = L.PIO_DT_F16 if dt == "f16" else L.PIO_DT_BF16
    prev = lib.pio_gemm_kernel_override(override)
    try:
        L.check(lib.pio_gemm_nt(C.byref(gm), torch.cuda.current_stream().cuda_stream), "pio_gemm_nt")
        torch.cuda.synchronize()
    finally:
        lib.pio_gemm_kernel_override(prev)
    W = Bhi.double() + (Blo.double() if lo_w else 0)
    ref = alpha * torch.bmm(A.double(), W.transpose(1, 2))
    if bias_mode:
        ref = ref + bias.double()[None, None, :]
    if act:
        ref = torch.nn.functional.gelu(ref)
    if resid:
        ref = ref + Rm.double()[None]
    got = Cd.double()
    if lo_out:
        got = got + Cl.double()
    assert torch.isfinite(got[:, :, :N]).all()
    if not out_f32:
        assert (Cd[:, :, N:] == 0).all(), "pad columns must be written as zeros"
    tol = 2e-5 if (out_f32 or lo_out) else (1e-3 if dt == "f16" else 8e-3)
    if lo_out and dt == "bf16":
        tol = 1e-4
    err = ((got[:, :, :N] - ref).abs().max() / ref.abs().max()).item()
    assert err <= tol, f"{what} gemm {shape} {dt}: {err:.3e}"


@pytest.mark.parametrize("C_", [322, 1024, 261, 8, 1280])
@pytest.mark.parametrize("norm", [True, False])
def test_layernorm_cast(dev, C_, norm):
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    lib = L.lib()
    B, T = 3, 37
    g = torch.Generator().manual_seed(C_)
    x = torch.randn(B, T, C_, generator=g) * 3 + 0.5
    gamma = 1 + 0.1 * torch.randn(C_, generator=g)
    beta = 0.1 * torch.randn(C_, generator=g)
    cp = R.pad8(C_)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    y = torch.full((B * T, cp), float("nan"), dtype=torch.float16, device=dev)
    ln = L.LayerNorm(gd.data_ptr(), bd.data_ptr(), C_, 1e-5)
    ylo = torch.full((B * T, cp), float("nan"), dtype=torch.float16, device=dev)
    L.check(lib.pio_layernorm_cast(R.tensor3(xd), C.byref(ln) if norm else None, y.data_ptr(), ylo.data_ptr(), cp,
                                   L.PIO_DT_F16, torch.cuda.current_stream().cuda_stream), "pio_layernorm_cast")
    ref = O.layer_norm(x.numpy().astype(np.float64), gamma.numpy().astype(np.float64),
                       beta.numpy().astype(np.float64)) if norm else x.numpy().astype(np.float64)
    got = y.float().cpu().numpy().reshape(B, T, cp)
    assert (got[..., C_:] == 0).all()
    assert np.abs(got[..., :C_] - ref).max() <= 1e-3 * np.abs(ref).max()      # fp16 rounding of the output
    both = got + ylo.float().cpu().numpy().reshape(B, T, cp)                   # hi + lo ~ fp32 LayerNorm
    assert np.abs(both[..., :C_] - ref).max() <= 2e-6 * np.abs(ref).max()
    # broadcast (stride-0) batch view
    xb = torch.broadcast_to(xd[0:1], (4, T, C_))
    y2 = torch.empty((4 * T, cp), dtype=torch.float16, device=dev)
    L.check(lib.pio_layernorm_cast(R.tensor3(xb), C.byref(ln) if norm else None, y2.data_ptr(), None, cp,
                                   L.PIO_DT_F16, torch.cuda.current_stream().cuda_stream), "pio_layernorm_cast")
    assert torch.equal(y2.view(4, T, cp)[3], y.view(B, T, cp)[0])


@pytest.mark.parametrize("Tk", [13, 512, 3136, 5000])
def test_softmax_rows(dev, Tk):
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    lib = L.lib()
    B, H, Tq = 2, 3, 9
    g = torch.Generator().manual_seed(Tk)
    S = torch.randn(B, H, Tq, Tk, generator=g) * 4
    km = torch.rand(B, Tk, generator=g) > 0.3
    km[1, :] = False if Tk == 13 else km[1, :]
    qm = torch.rand(B, Tq, generator=g) > 0.3
    tkp = R.pad8(Tk)
    Sd = S.to(dev)
    P = torch.full((B, H, Tq, tkp), float("nan"), dtype=torch.float16, device=dev)
    kmd, qmd = km.to(dev).view(torch.uint8), qm.to(dev).view(torch.uint8)
    scale = 0.37
    L.check(lib.pio_softmax_rows(Sd.data_ptr(), Tk, P.data_ptr(), None, tkp, B, H, Tq, Tk, scale, kmd.data_ptr(),
                                 qmd.data_ptr(), None, None, L.PIO_DT_F16, torch.cuda.current_stream().cuda_stream),
            "pio_softmax_rows")
    mask = O.make_cross_attention_mask(qm.numpy(), km.numpy())
    s = S.numpy().astype(np.float64) * scale
    s = np.where(mask[:, None], s, -1e30)
    ref = O.softmax_lastdim(s)
    ref = np.where(np.all(mask == 0, axis=2, keepdims=True)[:, None], 0.0, ref)
    got = P.float().cpu().numpy()
    assert (got[..., Tk:] == 0).all()
    assert np.abs(got[..., :Tk] - ref).max() <= 1e-3 * max(ref.max(), 1e-9)


# ----------------------------------------------------------------------------------------------------
# module-level goldens (reference float32 outputs) through the nn.Module mirror
# ----------------------------------------------------------------------------------------------------
def _mask3(g, dev):
    if "query_mask" in g:
        return _t(O.make_cross_attention_mask(g["query_mask"], g["kv_mask"]), dev)
    return None


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", ATTN)
def test_attention_golden(dev, name, policy):
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    _policy(policy)
    g = load(name)
    B, Tq, Tk, q_in, kv_in, H, qk, v, out = (int(x) for x in g["meta"])
    m = Attention(q_in, kv_in, kv_in, num_heads=H, qk_out_channels=qk, v_out_channels=v, output_channels=out)
    m.load_state_dict(_sd(params(g), "cpu"), strict=True)
    m = m.to(dev).eval()
    xq, xkv = _t(g["xq"], dev), _t(g["xkv"], dev)
    with torch.inference_mode():
        y = m(xq, xkv, xkv, attention_mask=_mask3(g, dev))
    _assert_close(y, g["out"], tol_for(policy, name), what=name)


def test_attention_wiped_rows_equal_final_bias(dev):
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    _policy("fp16x3")
    g = load("attn_h4_fullmask_row")
    B, Tq, Tk, q_in, kv_in, H, qk, v, out = (int(x) for x in g["meta"])
    m = Attention(q_in, kv_in, kv_in, num_heads=H, qk_out_channels=qk, v_out_channels=v, output_channels=out)
    m.load_state_dict(_sd(params(g), "cpu"))
    m = m.to(dev).eval()
    xq, xkv = _t(g["xq"], dev), _t(g["xkv"], dev)
    y = m(xq, xkv, xkv, attention_mask=_mask3(g, dev))
    fb = m.final.bias.detach()
    assert torch.equal(y[1], fb[None, :].expand_as(y[1])), "fully masked sample must give final.bias exactly"


def test_attention_return_matrix_and_bias(dev):
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    _policy("fp16x3")
    g = load("attn_h8_keymask")
    B, Tq, Tk, q_in, kv_in, H, qk, v, out = (int(x) for x in g["meta"])
    p = params(g)
    m = Attention(q_in, kv_in, kv_in, num_heads=H, qk_out_channels=qk, v_out_channels=v, output_channels=out)
    m.load_state_dict(_sd(p, "cpu"))
    m = m.to(dev).eval()
    rng = np.random.default_rng(5)
    bias = rng.standard_normal((B, H, Tq, Tk)).astype(np.float32)
    mask = O.make_cross_attention_mask(g["query_mask"], g["kv_mask"])
    pm, y = m(_t(g["xq"], dev), _t(g["xkv"], dev), _t(g["xkv"], dev), attention_mask=_t(mask, dev),
              attention_bias=_t(bias, dev), return_matrix=True)
    p64 = {k: a.astype(np.float64) for k, a in p.items()}
    rm, ry = O.attention(p64, g["xq"].astype(np.float64), g["xkv"].astype(np.float64), g["xkv"].astype(np.float64),
                         H, mask, bias.astype(np.float64), return_matrix=True)
    _assert_close(y, ry, TIGHT, what="attention with bias")
    assert np.abs(pm.cpu().numpy() - rm).max() <= PROBS_ABS_TOL


FLASH_CASES = [
    # heads, dk, dv, B, Tq, Tk   (per-head widths handled by the fused attention kernel; ragged Tq / Tk tails)
    (8, 128, 128, 2, 512, 512),
    (2, 128, 128, 1, 100, 777),
    (8, 64, 64, 2, 784, 784),
    (16, 32, 32, 1, 2048, 2048),
    (4, 32, 32, 3, 33, 65),
    (8, 32, 160, 1, 256, 256),
    (2, 32, 160, 2, 50, 130),
]


@pytest.mark.parametrize("policy", ["fp16", "fp16x2w", "bf16"])
@pytest.mark.parametrize("case", FLASH_CASES)
def test_fused_attention_vs_oracle(dev, case, policy):
    """Attention.forward on the fused (flash) path against the float64 oracle and against the materialised
    3-sweep path of the same library."""
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    H, dk, dv, B, Tq, Tk = case
    cin = 96
    p = O.gen_attention("", cin, cin, H * dk, H * dv, cin, seed=H * dk + Tq)
    rng = np.random.default_rng(Tk)
    xq = rng.standard_normal((B, Tq, cin)).astype(np.float32)
    xkv = rng.standard_normal((B, Tk, cin)).astype(np.float32)
    m = Attention(cin, cin, cin, num_heads=H, qk_out_channels=H * dk, v_out_channels=H * dv, output_channels=cin)
    m.load_state_dict(_sd(p, "cpu"))
    m = m.to(dev).eval()
    p64 = {k: a.astype(np.float64) for k, a in p.items()}
    ref = O.attention(p64, xq.astype(np.float64), xkv.astype(np.float64), xkv.astype(np.float64), H)
    _policy(policy)
    y = m(_t(xq, dev), _t(xkv, dev), _t(xkv, dev))
    _assert_close(y, ref, TOL if policy != "bf16" else BF16_FUSED_TOL, what=f"fused attention {case} {policy}")
    # a spiky query row forces large running-max jumps between key tiles (the online-softmax rescale branch);
    # compare the fused kernel with the materialised-score path of the SAME policy (return_matrix forces it):
    # identical operand rounding, different algorithm.
    xs = xq.copy()
    xs[0, 0] *= 8.0
    xs[-1, -1] *= -8.0
    yf = m(_t(xs, dev), _t(xkv, dev), _t(xkv, dev))
    _, ym = m(_t(xs, dev), _t(xkv, dev), _t(xkv, dev), return_matrix=True)
    # (the two round P at different points -- un-normalised vs normalised -- so they differ by ~1 ulp16 of P)
    _assert_close(yf, ym.detach().cpu().numpy(), TOL if policy != "bf16" else 8e-3, what=f"fused vs materialised {case} {policy}")
    _policy("fp16x3")
    y3 = m(_t(xq, dev), _t(xkv, dev), _t(xkv, dev))
    _assert_close(y3, ref, TIGHT, what=f"materialised attention {case}")


@pytest.mark.parametrize("shape", [(2, 512, 8), (3, 100, 2), (1, 777, 4),
                                   (16, 600, 8)])  # enough (batch, head, q-tile)s for the 256-row workgroups
def test_fully_fused_self_attention_qkv(dev, shape):
    """inputs_q is inputs_k is inputs_v, 128-wide heads, 1-sweep policy: ONE q|k|v GEMM + the fused attention kernel
    reading V row-major through transposed LDS reads.  Checked against the oracle and against the same module under
    fp16x2s (which takes the separate V^T route)."""
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    B, T, H = shape
    cin = 128
    p = O.gen_attention("", cin, cin, H * 128, H * 128, cin, seed=T)
    x = np.random.default_rng(T).standard_normal((B, T, cin)).astype(np.float32)
    m = Attention(cin, cin, cin, num_heads=H, qk_out_channels=H * 128, v_out_channels=H * 128, output_channels=cin)
    m.load_state_dict(_sd(p, "cpu"))
    m = m.to(dev).eval()
    xt = _t(x, dev)
    ref = O.attention({k: a.astype(np.float64) for k, a in p.items()}, x.astype(np.float64), x.astype(np.float64),
                      x.astype(np.float64), H)
    _policy("fp16")
    y = m(xt, xt, xt)
    _assert_close(y, ref, TOL, what=f"fused qkv {shape}")
    _policy("fp16x2s")
    y2 = m(xt, xt, xt)
    _assert_close(y, y2.detach().cpu().numpy(), TOL, what=f"fused qkv vs separate V^T {shape}")


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", MLP)
def test_mlp_golden(dev, name, policy):
    from perceiverio_pytorch_amd.transformer_primitives import MLP as HipMLP
    _policy(policy)
    g = load(name)
    cin, w = (int(x) for x in g["meta"])
    m = HipMLP(cin, widening_factor=w)
    m.load_state_dict(_sd(params(g), "cpu"), strict=True)
    m = m.to(dev).eval()
    _assert_close(m(_t(g["x"], dev)), g["out"], tol_for(policy, name), what=name)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", SA)
def test_self_attention_golden(dev, name, policy):
    from perceiverio_pytorch_amd.transformer_primitives import SelfAttention
    _policy(policy)
    g = load(name)
    B, N, D, H, w = (int(x) for x in g["meta"])
    m = SelfAttention(D, widening_factor=w, num_heads=H)
    m.load_state_dict(_sd(params(g), "cpu"), strict=True)
    m = m.to(dev).eval()
    _assert_close(m(_t(g["x"], dev)), g["out"], tol_for(policy, name), what=name)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", CA)
def test_cross_attention_golden(dev, name, policy):
    from perceiverio_pytorch_amd.transformer_primitives import CrossAttention
    _policy(policy)
    g = load(name)
    B, Tq, Tk, q_in, kv_in, H, resid, kv = (int(x) for x in g["meta"])
    m = CrossAttention(q_in, kv_in, num_heads=H, shape_for_attn="kv" if kv else "q", use_query_residual=bool(resid))
    m.load_state_dict(_sd(params(g), "cpu"), strict=True)
    m = m.to(dev).eval()
    y = m(_t(g["xq"], dev), _t(g["xkv"], dev), attention_mask=_mask3(g, dev))
    _assert_close(y, g["out"], tol_for(policy, name), what=name)


def build_encdec(cfg, p_enc, p_dec, dev):
    from perceiverio_pytorch_amd.perceiver import PerceiverEncoder, PerceiverDecoder
    enc = PerceiverEncoder(num_input_channels=cfg["C"], num_self_attends_per_block=cfg["L"], num_blocks=cfg["blocks"],
                           num_latents=cfg["N"], num_latent_channels=cfg["D"], qk_channels=cfg.get("qk"),
                           v_channels=cfg.get("v"), num_cross_attend_heads=cfg["xh"],
                           num_self_attend_heads=cfg["sh"], use_query_residual=cfg["enc_resid"])
    dec = PerceiverDecoder(query_channels=cfg["Dq"], final_project_out_channels=cfg["out"] or cfg["Dq"],
                           num_latent_channels=cfg["D"], qk_channels=cfg.get("dqk"), v_channels=cfg.get("dv"),
                           use_query_residual=cfg["dec_resid"], num_heads=cfg["dh"],
                           final_project=cfg["out"] is not None)
    enc.load_state_dict(_sd(p_enc, "cpu"), strict=True)
    dec.load_state_dict(_sd(p_dec, "cpu"), strict=True)
    return enc.to(dev).eval(), dec.to(dev).eval()


def run_encdec(enc, dec, x, qtab, im, qm, dev):
    with torch.inference_mode():
        xt = _t(x, dev)
        z = enc(xt, enc.latents(xt), input_mask=None if im is None else _t(im, dev))
        q = torch.broadcast_to(_t(qtab, dev)[None], (x.shape[0],) + qtab.shape)
        y = dec(q, z, query_mask=None if qm is None else _t(qm, dev))
    return z, y


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", ENCDEC_FULL)
def test_encdec_full_golden(dev, name, policy):
    _policy(policy)
    g = load(name)
    cfg = ENCDEC_CASES[name]
    enc, dec = build_encdec(cfg, params(g, "enc."), params(g, "dec."), dev)
    z, y = run_encdec(enc, dec, g["x"], g["qtab"], g.get("input_mask"), g.get("query_mask"), dev)
    _assert_close(z, g["latents"], tol_for(policy, name), what=name + " latents")
    _assert_close(y, g["out"], tol_for(policy, name), what=name)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", ENCDEC_SUB + ["encdec_imagenet_b2"])
def test_encdec_subsampled_golden(dev, name, policy):
    _policy(policy)
    g = load(name)
    cfg = ENCDEC_CASES[name]
    p_enc, p_dec, qtab, x, im, qm = gen_encdec_inputs(name, cfg, int(g["seed"]))
    enc, dec = build_encdec(cfg, p_enc, p_dec, dev)
    z, y = run_encdec(enc, dec, x, qtab, im, qm, dev)
    ysub = y[:, torch.from_numpy(g["out_rows"]).to(dev), :]
    # error relative to the WHOLE output's magnitude (stored with the golden), reference = float32 run
    d = ysub.cpu().numpy().astype(np.float64) - g["out"].astype(np.float64)
    rmax = np.abs(d).max() / float(g["out_absmax"])
    rl2 = np.sqrt((d * d).sum()) / np.sqrt((g["out"].astype(np.float64) ** 2).sum())
    print(f"{name} [{policy}] relL2={rl2:.3e} max/absmax={rmax:.3e}")
    tol = tol_for(policy, name)
    assert rl2 <= tol and rmax <= tol, f"{name} [{policy}]: relL2={rl2:.3e} max/absmax={rmax:.3e}"
    _assert_close(z[:, ::8, ::8], g["latents_sub"], tol, what=name + " latents")


def test_oracle_same_inputs_mid(dev):
    """HIP path vs the oracle (float64) on the same seeded inputs, a shape with awkward tails."""
    _policy("fp16x3")
    cfg = dict(B=3, M=203, C=45, N=37, D=72, L=2, blocks=2, xh=1, sh=4, enc_resid=True, Q=19, Dq=40, out=11, dh=1,
               dec_resid=False, masks=True)
    p_enc, p_dec, qtab, x, im, qm = gen_encdec_inputs("tails", cfg, 5)
    enc, dec = build_encdec(cfg, p_enc, p_dec, dev)
    z, y = run_encdec(enc, dec, x, qtab, im, qm, dev)
    c64 = lambda d: {k: a.astype(np.float64) for k, a in d.items()}  # noqa: E731
    ref = O.encode_decode(c64(p_enc), c64(p_dec), x.astype(np.float64), qtab.astype(np.float64),
                          **encdec_kwargs(cfg, im, qm))
    _assert_close(y, ref, TIGHT, what="tails")


@pytest.mark.parametrize("policy", ["fp16x3", "fp16x2af", "fp16"])
@pytest.mark.parametrize("Dq,resid,Q", [(1026, False, 2300), (1026, True, 2300), (522, False, 1100), (1022, True, 700)])
def test_decoder_odd_wide_query_channels_vs_oracle(dev, Dq, resid, Q, policy):
    """Decoder query channel counts that are neither multiples of 64 nor of 4 (the multimodal decoder has 1026): the
    16-bit operands run on the channel pitch pio_padc (1088 / 576 / 1024) and the decoder's internal fp32 rows on a
    float4 pitch, which takes the 2 x 2300-row GEMMs to the staged kernels -- against the float64 oracle, with and
    without the query residual (whose rows keep the caller's pitch), query mask included."""
    _policy(policy)
    try:
        cfg = dict(B=2, M=90, C=40, N=96, D=256, L=1, blocks=1, xh=1, sh=4, enc_resid=True, Q=Q, Dq=Dq, out=24, dh=1,
                   dec_resid=resid, masks=True)
        p_enc, p_dec, qtab, x, im, qm = gen_encdec_inputs(f"odd{Dq}", cfg, 9)
        enc, dec = build_encdec(cfg, p_enc, p_dec, dev)
        z, y = run_encdec(enc, dec, x, qtab, im, qm, dev)
        c64 = lambda d: {k: a.astype(np.float64) for k, a in d.items()}  # noqa: E731
        ref = O.encode_decode(c64(p_enc), c64(p_dec), x.astype(np.float64), qtab.astype(np.float64),
                              **encdec_kwargs(cfg, im, qm))
        # (single-sweep "fp16" on a dense decoder is not a shipped combination -- models.DEFAULT_POLICY gives dense
        #  decoders split activations, "x2af" -- it runs here for the single-sweep kernels' pitch handling: 2e-3)
        tol = {"fp16x3": TIGHT, "fp16x2af": TOL, "fp16": 2e-3}[policy]
        _assert_close(y, ref, tol, what=f"decoder Dq={Dq} resid={resid} {policy}")
    finally:
        _policy("fp16x3")


# ----------------------------------------------------------------------------------------------------
# edge cases the reference's semantics define
# ----------------------------------------------------------------------------------------------------
def test_encoder_sample_with_every_input_token_masked(dev):
    """A sample whose key mask is all-false: every latent row is "wiped" -> attention output = final.bias, then the
    residual / MLP as usual (transformer_primitives.py:168-175; SURVEY appendix A "masked-row consequences")."""
    _policy("fp16x3")
    cfg = dict(B=3, M=37, C=24, N=16, D=32, L=1, blocks=1, xh=2, sh=4, enc_resid=True, Q=5, Dq=24, out=None, dh=2,
               dec_resid=False, masks=True, qk=16, v=32, dqk=16, dv=24)
    p_enc, p_dec, qtab, x, im, qm = gen_encdec_inputs("allmasked", cfg, 9)
    im[1, :] = False                     # sample 1: nothing to attend to
    qm[2, :] = False                     # sample 2: every decoder query masked
    enc, dec = build_encdec(cfg, p_enc, p_dec, dev)
    z, y = run_encdec(enc, dec, x, qtab, im, qm, dev)
    c64 = lambda d: {k: a.astype(np.float64) for k, a in d.items()}  # noqa: E731
    ref = O.encode_decode(c64(p_enc), c64(p_dec), x.astype(np.float64), qtab.astype(np.float64),
                          **encdec_kwargs(cfg, im, qm))
    assert torch.isfinite(y).all()
    _assert_close(y, ref, TIGHT, what="fully masked samples")


def test_strided_and_degenerate_inputs(dev):
    from perceiverio_pytorch_amd.transformer_primitives import Attention, SelfAttention
    _policy("fp16x3")
    rng = np.random.default_rng(3)
    # (a) a transposed (non-contiguous) view and a float64 input are accepted like any tensor
    p = O.gen_self_attention("", 32, 4, widening=1)
    m = SelfAttention(32, widening_factor=1, num_heads=4)
    m.load_state_dict(_sd(p, "cpu"))
    m = m.to(dev).eval()
    base = rng.standard_normal((2, 32, 11))                       # [B, C, T]
    xv = _t(base, dev).transpose(1, 2)                            # [B, T, C] view with stride(2) != 1
    ref = O.self_attention({k: a.astype(np.float64) for k, a in p.items()}, base.transpose(0, 2, 1), 4)
    _assert_close(m(xv), ref, TIGHT, what="strided fp64 input")
    # (b) one query, one key
    pa = O.gen_attention("", 16, 16, 16, 16, 16, 5)
    a = Attention(16, 16, 16, num_heads=2)
    a.load_state_dict(_sd(pa, "cpu"))
    a = a.to(dev).eval()
    xq, xk = rng.standard_normal((1, 1, 16)).astype(np.float32), rng.standard_normal((1, 1, 16)).astype(np.float32)
    ref = O.attention({k: v.astype(np.float64) for k, v in pa.items()}, xq.astype(np.float64), xk.astype(np.float64),
                      xk.astype(np.float64), 2)
    _assert_close(a(_t(xq, dev), _t(xk, dev), _t(xk, dev)), ref, TIGHT, what="1x1 attention")
    # (c) inputs_k is not inputs_v (generic Attention signature)
    xv2 = rng.standard_normal((1, 1, 16)).astype(np.float32)
    ref = O.attention({k: v.astype(np.float64) for k, v in pa.items()}, xq.astype(np.float64), xk.astype(np.float64),
                      xv2.astype(np.float64), 2)
    _assert_close(a(_t(xq, dev), _t(xk, dev), _t(xv2, dev)), ref, TIGHT, what="k != v inputs")


def test_errors_are_loud(dev):
    from perceiverio_pytorch_amd import PioError
    from perceiverio_pytorch_amd.transformer_primitives import SelfAttention
    m = SelfAttention(32, widening_factor=1, num_heads=4).to(dev).eval()
    with pytest.raises(PioError, match="PIO_E_SHAPE"):
        m(torch.zeros(1, 4, 24, device=dev))                      # wrong channel count reaches the C-ABI check
    with pytest.raises(ValueError):
        m(torch.zeros(4, 32, device=dev))                         # not [B, T, C]
    m.train()
    m2 = SelfAttention(32, widening_factor=1, num_heads=4, dropout_prob=0.1).to(dev)
    with pytest.raises(NotImplementedError):
        m2(torch.zeros(1, 4, 32, device=dev))                     # training-mode dropout is not on this path


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("M,N2,act", [(4096, 3072, 0), (4000, 1024, 1), (16384, 1024, 1)])
def test_gemm_layernorm_fold(dev, M, N2, act, dt):
    """LayerNorm folded into the two GEMMs around it (pio_gemm_t.X16 / row_part -> ln_part / ln_c, kernel
    gemm_nt_wide): x = R + A W1^T + b1 (fp32, + 16-bit copy + per-row partial sums), then
    y = act(LN(x) W2^T + b2) computed as rstd * (x16 W'^T - mean * c) + b' -- against torch fp64 of the unfolded
    chain (transformer_primitives.py:281-292)."""
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    D, K1 = 1024, 512
    tdt = torch.float16 if dt == "f16" else torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(M + N2 + act)
    A = torch.randn(M, K1, generator=g).to(tdt).to(dev)
    W1 = (torch.randn(D, K1, generator=g) / K1 ** 0.5).to(tdt).to(dev)
    b1 = torch.randn(D, generator=g).to(dev)
    Rm = (torch.randn(M, D, generator=g) * 2 + 0.3).to(dev)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    beta = (0.1 * torch.randn(D, generator=g)).to(dev)
    W2 = (torch.randn(N2, D, generator=g) / D ** 0.5).to(dev)
    b2 = torch.randn(N2, generator=g).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    code = L.PIO_DT_F16 if dt == "f16" else L.PIO_DT_BF16

    # ---- producer
    X = torch.full((M, D), float("nan"), device=dev)
    X16 = torch.full((M, D), float("nan"), dtype=tdt, device=dev)
    part = torch.full((M, D // 128, 2), float("nan"), device=dev)
    gp = L.Gemm()
    gp.A, gp.B, gp.C = A.data_ptr(), W1.data_ptr(), X.data_ptr()
    gp.M, gp.N, gp.K = M, D, K1
    gp.lda, gp.ldb, gp.ldc = K1, K1, D
    gp.batch, gp.nh = 1, 1
    gp.bias, gp.bias_mode, gp.act, gp.alpha = b1.data_ptr(), 1, 0, 1.0
    gp.R, gp.ldr = Rm.data_ptr(), D
    gp.out_f32, gp.n_store, gp.dtype = 1, D, code
    gp.X16, gp.ld16, gp.row_part = X16.data_ptr(), D, part.data_ptr()
    L.check(lib.pio_gemm_nt(C.byref(gp), st), "producer")
    torch.cuda.synchronize()
    xref = A.double() @ W1.double().T + b1.double() + Rm.double()
    assert ((X.double() - xref).abs().max() / xref.abs().max()).item() <= 2e-5
    assert torch.equal(X16, X.to(tdt)), "the 16-bit copy is the rounded fp32 result"
    blocks = X.double().reshape(M, D // 128, 128)
    assert torch.allclose(part[:, :, 0].double(), blocks.sum(-1), rtol=1e-4, atol=1e-3)
    assert torch.allclose(part[:, :, 1].double(), (blocks * blocks).sum(-1), rtol=1e-4, atol=1e-3)

    # ---- the same producer with the residual stream as a 16-bit pair in and out, no fp32 result at all
    Rhi = Rm.to(tdt)
    Rlo = (Rm - Rhi.float()).to(tdt)
    Xh = torch.full((M, D), float("nan"), dtype=tdt, device=dev)
    Xl = torch.full((M, D), float("nan"), dtype=tdt, device=dev)
    part2 = torch.full((M, D // 128, 2), float("nan"), device=dev)
    gq = L.Gemm()
    gq.A, gq.B, gq.C = A.data_ptr(), W1.data_ptr(), None
    gq.M, gq.N, gq.K = M, D, K1
    gq.lda, gq.ldb, gq.ldc = K1, K1, D
    gq.batch, gq.nh = 1, 1
    gq.bias, gq.bias_mode, gq.act, gq.alpha = b1.data_ptr(), 1, 0, 1.0
    gq.out_f32, gq.n_store, gq.dtype = 1, D, code
    gq.X16, gq.ld16, gq.row_part = Xh.data_ptr(), D, part2.data_ptr()
    gq.X16_lo, gq.R16_hi, gq.R16_lo = Xl.data_ptr(), Rhi.data_ptr(), Rlo.data_ptr()
    xref2 = A.double() @ W1.double().T + b1.double() + Rhi.double() + Rlo.double()
    pair_tol = 2e-6 if dt == "f16" else 4e-5
    for kernel in (0,):  # (the two-workgroups-per-CU producer, override 3, lives in tools/experiments)
        Xh.fill_(float("nan")); Xl.fill_(float("nan")); part2.fill_(float("nan"))
        prev = lib.pio_gemm_kernel_override(kernel)
        try:
            L.check(lib.pio_gemm_nt(C.byref(gq), st), "producer (pair)")
            torch.cuda.synchronize()
        finally:
            lib.pio_gemm_kernel_override(prev)
        got2 = Xh.double() + Xl.double()
        assert torch.isfinite(got2).all() and torch.isfinite(part2).all(), f"kernel {kernel}"
        assert ((got2 - xref2).abs().max() / xref2.abs().max()).item() <= pair_tol, f"kernel {kernel}"
        assert torch.allclose(part2[:, :, 0].double(), got2.reshape(M, D // 128, 128).sum(-1), rtol=1e-4, atol=2e-3)
        assert torch.allclose(part2[:, :, 1].double(), (got2 * got2).reshape(M, D // 128, 128).sum(-1), rtol=1e-4,
                              atol=2e-3)

    # ---- consumer
    Wf = (W2 * gamma[None, :]).to(tdt)
    cvec = Wf.float().sum(1).contiguous()
    bf = (W2.double() @ beta.double() + b2.double()).float().contiguous()
    ldc = N2
    Y = torch.full((M, ldc), float("nan"), dtype=tdt, device=dev)
    gc = L.Gemm()
    gc.A, gc.B, gc.C = X16.data_ptr(), Wf.data_ptr(), Y.data_ptr()
    gc.M, gc.N, gc.K = M, N2, D
    gc.lda, gc.ldb, gc.ldc = D, D, ldc
    gc.batch, gc.nh = 1, 1
    gc.bias, gc.bias_mode, gc.act, gc.alpha = bf.data_ptr(), 1, act, 1.0
    gc.out_f32, gc.n_store, gc.dtype = 0, N2, code
    gc.ln_part, gc.ln_c, gc.ln_eps = part.data_ptr(), cvec.data_ptr(), 1e-5
    L.check(lib.pio_gemm_nt(C.byref(gc), st), "consumer")
    torch.cuda.synchronize()
    xd = X.double()
    ln = torch.nn.functional.layer_norm(xd, (D,), gamma.double(), beta.double(), 1e-5)
    ref = ln @ W2.double().T + b2.double()
    if act:
        ref = torch.nn.functional.gelu(ref)
    got = Y.double()
    assert torch.isfinite(got).all()
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    rl2 = ((got - ref).norm() / ref.norm()).item()
    print(f"folded LayerNorm GEMM M={M} N={N2} act={act} {dt}: relL2={rl2:.3e} max/absmax={err:.3e}")
    # fp16 at the north_star's bar against the exact float64 result (measured 3e-4 / 4e-4); bf16 is the range fallback,
    # not a parity policy (8-bit mantissa: 2.4e-3 / 3.2e-3)
    assert max(err, rl2) <= (TOL if dt == "f16" else 5e-3), f"folded LayerNorm GEMM M={M} N={N2} act={act} {dt}: {rl2:.3e} / {err:.3e}"
    # the same roundings in fp64: only the accumulation order and the 16-bit output rounding remain
    mu = xd.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + 1e-5)
    ref2 = rs * (X16.double() @ Wf.double().T - mu * cvec.double()[None, :]) + bf.double()[None, :]
    if act:
        ref2 = torch.nn.functional.gelu(ref2)
    err2 = ((got - ref2).abs().max() / ref2.abs().max()).item()
    assert err2 <= (1e-3 if dt == "f16" else 8e-3), f"folded LayerNorm GEMM vs same-rounding reference: {err2:.3e}"


def _sa_reference64(m, x):
    """SelfAttention.forward of the reference (transformer_primitives.py:281-292) in torch float64."""
    F = torch.nn.functional
    d = lambda t: t.detach().double()  # noqa: E731
    xd = x.double()
    B, N, D = xd.shape
    H = m.attention._num_heads
    a = m.attention
    n1 = F.layer_norm(xd, (D,), d(m.layer_norm1.weight), d(m.layer_norm1.bias), m.layer_norm1.eps)
    q = (n1 @ d(a.proj_q.weight).T + d(a.proj_q.bias)).reshape(B, N, H, -1).permute(0, 2, 1, 3)
    k = (n1 @ d(a.proj_k.weight).T + d(a.proj_k.bias)).reshape(B, N, H, -1).permute(0, 2, 1, 3)
    v = (n1 @ d(a.proj_v.weight).T + d(a.proj_v.bias)).reshape(B, N, H, -1).permute(0, 2, 1, 3)
    p = torch.softmax(q @ k.transpose(-1, -2) / q.shape[-1] ** 0.5, -1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(B, N, -1)
    x1 = xd + o @ d(a.final.weight).T + d(a.final.bias)
    n2 = F.layer_norm(x1, (D,), d(m.layer_norm2.weight), d(m.layer_norm2.bias), m.layer_norm2.eps)
    h = F.gelu(n2 @ d(m.mlp.fc1.weight).T + d(m.mlp.fc1.bias))
    return x1 + h @ d(m.mlp.fc2.weight).T + d(m.mlp.fc2.bias)


@pytest.mark.parametrize("policy", ["fp16", "bf16"])
def test_self_attention_layernorm_fold(dev, policy):
    """A 1024-channel SelfAttention block with the LayerNorms folded into the GEMMs around them (pio_ln_fold_t)
    against torch float64 of the reference's forward, and against the same block with the fold switched off."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd.transformer_primitives import SelfAttention
    lib = L.lib()
    _policy(policy)
    torch.manual_seed(5)
    m = SelfAttention(1024, widening_factor=1, num_heads=8)
    with torch.no_grad():
        for ln in (m.layer_norm1, m.layer_norm2):
            ln.weight.add_(0.1 * torch.randn(1024))
            ln.bias.add_(0.1 * torch.randn(1024))
        for lin in (m.attention.proj_q, m.attention.proj_k, m.attention.proj_v, m.attention.final, m.mlp.fc1, m.mlp.fc2):
            lin.bias.add_(0.05 * torch.randn(lin.bias.shape))
    m = m.to(dev).eval()
    x = (torch.randn(4, 512, 1024) * 1.5 + 0.2).to(dev)
    ref = _sa_reference64(m, x)
    prev = lib.pio_ln_fold_enable(2)       # 2048 rows: below the automatic setting's 6144
    try:
        with torch.inference_mode():
            y_fold = m(x).double()
            lib.pio_ln_fold_enable(0)
            y_plain = m(x).double()
    finally:
        lib.pio_ln_fold_enable(prev)
    scale = ref.abs().max()
    e_fold = ((y_fold - ref).abs().max() / scale).item()
    e_plain = ((y_plain - ref).abs().max() / scale).item()
    assert not torch.equal(y_fold, y_plain), "the fold did not run (identical results)"
    print(f"SA block {policy}: fold relL2={((y_fold - ref).norm() / ref.norm()).item():.3e} max={e_fold:.3e} | "
          f"plain relL2={((y_plain - ref).norm() / ref.norm()).item():.3e} max={e_plain:.3e}")
    tol = TOL if policy == "fp16" else 3e-3     # (measured: fp16 1.8e-4, bf16 -- range fallback, not a parity policy -- 1.4e-3)
    assert e_fold <= tol, f"folded block {policy}: {e_fold:.3e} (unfolded {e_plain:.3e})"
    assert e_fold <= 1.5 * e_plain + 2e-4, f"folded block {policy}: {e_fold:.3e} vs unfolded {e_plain:.3e}"


@pytest.mark.parametrize("shape", [(1, 512), (2, 200), (1, 77)])
def test_self_attention_small_batch(dev, shape):
    """Small batches of the 1024-channel block (8 heads of 128, fused q|k|v, V row-major, ragged last query tile) against
    the float64 restatement of the reference's SelfAttention.forward."""
    from perceiverio_pytorch_amd.transformer_primitives import SelfAttention
    B, T = shape
    _policy("fp16")
    try:
        torch.manual_seed(B * 1000 + T)
        m = SelfAttention(1024, widening_factor=1, num_heads=8).to(dev).eval()
        x = (torch.randn(B, T, 1024) * 1.2 + 0.1).to(dev)
        with torch.inference_mode():
            y = m(x).double()
        ref = _sa_reference64(m, x)
        rl2 = ((y - ref).norm() / ref.norm()).item()
        rmax = ((y - ref).abs().max() / ref.abs().max()).item()
        assert rl2 <= TOL and rmax <= TOL, (shape, rl2, rmax)
    finally:
        _policy("fp16x3")


# (D, rows, slot width): the fold's two kernel families at the channel widths of the shipped stacks -- 128-column slots on
# the 256 x 256-tile kernel (language 1280, flow / multimodal 512 at many rows), 64-column slots on the tile kernels
FOLD_GENERAL = [(512, 4096, 128), (1280, 4096, 128), (1536, 2304, 128), (512, 2048, 64), (512, 784, 64), (1024, 512, 64),
                (1280, 300, 64)]


@pytest.mark.parametrize("D,M,slot_w", FOLD_GENERAL)
def test_gemm_layernorm_fold_other_widths(dev, D, M, slot_w):
    """pio_gemm_t.row_slot_w / ln_slots: producer (residual pair in, result pair out IN PLACE, per-slot row sums) and
    consumer (LayerNorm folded into the GEMM) at 512 / 1280 / 1536 channels on both kernel families, against torch
    float64 of the un-folded chain (transformer_primitives.py:281-292)."""
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    K1, N2 = D, D + 256
    tdt = torch.float16
    g = torch.Generator(device="cpu").manual_seed(D + M + slot_w)
    A = torch.randn(M, K1, generator=g).to(tdt).to(dev)
    W1 = (torch.randn(D, K1, generator=g) / K1 ** 0.5).to(tdt).to(dev)
    b1 = torch.randn(D, generator=g).to(dev)
    Rm = (torch.randn(M, D, generator=g) * 2 + 0.3).to(dev)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    beta = (0.1 * torch.randn(D, generator=g)).to(dev)
    W2 = (torch.randn(N2, D, generator=g) / D ** 0.5).to(dev)
    b2 = torch.randn(N2, generator=g).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    nslots = D // slot_w
    Xh = Rm.to(tdt)                                   # the stream, updated in place by the producer
    Xl = (Rm - Xh.float()).to(tdt)
    xref = A.double() @ W1.double().T + b1.double() + Xh.double() + Xl.double()
    part = torch.full((M, nslots, 2), float("nan"), device=dev)
    gq = L.Gemm()
    gq.A, gq.B, gq.C = A.data_ptr(), W1.data_ptr(), None
    gq.M, gq.N, gq.K = M, D, K1
    gq.lda, gq.ldb, gq.ldc = K1, K1, D
    gq.batch, gq.nh = 1, 1
    gq.bias, gq.bias_mode, gq.act, gq.alpha = b1.data_ptr(), 1, 0, 1.0
    gq.out_f32, gq.n_store, gq.dtype = 1, D, L.PIO_DT_F16
    gq.X16, gq.ld16, gq.row_part = Xh.data_ptr(), D, part.data_ptr()
    gq.X16_lo, gq.R16_hi, gq.R16_lo = Xl.data_ptr(), Xh.data_ptr(), Xl.data_ptr()
    gq.row_slot_w = slot_w
    L.check(lib.pio_gemm_nt(C.byref(gq), st), "producer")
    torch.cuda.synchronize()
    got = Xh.double() + Xl.double()
    assert torch.isfinite(got).all() and torch.isfinite(part).all()
    assert ((got - xref).abs().max() / xref.abs().max()).item() <= 2e-6
    assert torch.allclose(part[:, :, 0].double(), got.reshape(M, nslots, slot_w).sum(-1), rtol=1e-4, atol=2e-3)
    assert torch.allclose(part[:, :, 1].double(), (got * got).reshape(M, nslots, slot_w).sum(-1), rtol=1e-4, atol=2e-3)

    for act in (0, 1):
        Wf = (W2 * gamma[None, :]).to(tdt)
        cvec = Wf.float().sum(1).contiguous()
        bf = (W2.double() @ beta.double() + b2.double()).float().contiguous()
        Y = torch.full((M, N2), float("nan"), dtype=tdt, device=dev)
        gc = L.Gemm()
        gc.A, gc.B, gc.C = Xh.data_ptr(), Wf.data_ptr(), Y.data_ptr()
        gc.M, gc.N, gc.K = M, N2, D
        gc.lda, gc.ldb, gc.ldc = D, D, N2
        gc.batch, gc.nh = 1, 1
        gc.bias, gc.bias_mode, gc.act, gc.alpha = bf.data_ptr(), 1, act, 1.0
        gc.out_f32, gc.n_store, gc.dtype = 0, N2, L.PIO_DT_F16
        gc.ln_part, gc.ln_c, gc.ln_eps, gc.ln_slots = part.data_ptr(), cvec.data_ptr(), 1e-5, nslots
        L.check(lib.pio_gemm_nt(C.byref(gc), st), "consumer")
        torch.cuda.synchronize()
        ln = torch.nn.functional.layer_norm(got, (D,), gamma.double(), beta.double(), 1e-5)
        ref = ln @ W2.double().T + b2.double()
        if act:
            ref = torch.nn.functional.gelu(ref)
        y = Y.double()
        assert torch.isfinite(y).all()
        err = ((y - ref).abs().max() / ref.abs().max()).item()
        rl2 = ((y - ref).norm() / ref.norm()).item()
        print(f"fold D={D} M={M} slot={slot_w} act={act}: relL2={rl2:.3e} max/absmax={err:.3e}")
        assert max(err, rl2) <= TOL, (D, M, slot_w, act, rl2, err)


# (channels, heads, qk_channels, v_channels, B, N): the latent blocks of the language, flow and multimodal models, at row
# counts of both fold families (mode 2: 256 x 256 tiles from 2048 rows, tile kernels below)
SA_SHIPPED = [(1280, 8, 256, 1280, 10, 256, "language, wide"), (1280, 8, 256, 1280, 3, 256, "language, tiles"),
              (512, 16, 512, 512, 1, 2048, "flow, wide"), (512, 16, 512, 512, 1, 1000, "flow-like, tiles"),
              (512, 8, 512, 512, 1, 784, "multimodal, tiles"), (1024, 8, 1024, 1024, 2, 512, "imagenet B=2, tiles")]


@pytest.mark.parametrize("case", SA_SHIPPED, ids=[c[-1].replace(" ", "_").replace(",", "") for c in SA_SHIPPED])
def test_self_attention_fold_shipped_stacks(dev, case):
    """SelfAttention blocks of the other three shipped stacks (and a small ImageNet batch) with the LayerNorm fold, the
    in-place 16-bit-pair stream and ONE q|k|v GEMM feeding the fused attention kernel with V read row-major, against torch
    float64 of the reference's forward (transformer_primitives.py:275-297) -- and against the same block un-folded."""
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd.transformer_primitives import SelfAttention
    Cc, H, qk, vv, B, N, what = case
    lib = L.lib()
    _policy("fp16")
    try:
        torch.manual_seed(Cc + H + N)
        m = SelfAttention(Cc, widening_factor=1, num_heads=H, qk_channels=qk, v_channels=vv)
        with torch.no_grad():
            for ln in (m.layer_norm1, m.layer_norm2):
                ln.weight.add_(0.1 * torch.randn(Cc))
                ln.bias.add_(0.1 * torch.randn(Cc))
            for lin in (m.attention.proj_q, m.attention.proj_k, m.attention.proj_v, m.attention.final, m.mlp.fc1, m.mlp.fc2):
                lin.bias.add_(0.05 * torch.randn(lin.bias.shape))
        m = m.to(dev).eval()
        x = (torch.randn(B, N, Cc) * 1.5 + 0.2).to(dev)
        ref = _sa_reference64(m, x)
        prev = lib.pio_ln_fold_enable(2)
        try:
            with torch.inference_mode():
                y_fold = m(x).double()
                y_again = m(x).double()
                lib.pio_ln_fold_enable(0)
                y_plain = m(x).double()
        finally:
            lib.pio_ln_fold_enable(prev)
        assert torch.equal(y_fold, y_again), "the folded block is not deterministic"
        assert not torch.equal(y_fold, y_plain), f"{what}: the fold did not run (identical results)"
        scale = ref.abs().max()
        e_fold = max(((y_fold - ref).abs().max() / scale).item(), ((y_fold - ref).norm() / ref.norm()).item())
        e_plain = max(((y_plain - ref).abs().max() / scale).item(), ((y_plain - ref).norm() / ref.norm()).item())
        print(f"SA {what}: fold {e_fold:.3e} | un-folded {e_plain:.3e}")
        assert e_fold <= TOL and e_plain <= TOL, (what, e_fold, e_plain)
        assert e_fold <= 1.5 * e_plain + 2e-4, (what, e_fold, e_plain)
    finally:
        _policy("fp16x3")


def test_backward_through_hip_modules_raises(dev):
    """With autograd recording, the output of a HIP module carries a grad_fn whose backward raises -- a training step
    cannot silently skip the encoder / decoder parameters."""
    from perceiverio_pytorch_amd.transformer_primitives import MLP as HipMLP
    m = HipMLP(32, widening_factor=1).to(dev)
    x = torch.randn(2, 5, 32, device=dev)
    with torch.enable_grad():
        y = m(x)
        assert y.requires_grad
        with pytest.raises(NotImplementedError, match="forward / inference"):
            y.sum().backward()
    assert all(p.grad is None for p in m.parameters())


# ----------------------------------------------------------------------------------------------------
# fused cross-attention kernel (pio_xattn.hip): mask VECTORS, wide single heads, dv != dk, key splits
# ----------------------------------------------------------------------------------------------------
XATTN_CASES = [
    # heads, dk, dv, B, Tq, Tk, mask kind, broadcast Q
    (1, 322, 322, 2, 200, 500, "key", False),      # the 322-wide single head of the ImageNet / flow encoders, ragged
    (1, 322, 322, 1, 512, 3136, None, True),       # ImageNet encoder shape, one sample: split over the keys
    (1, 322, 322, 3, 512, 1000, "key_allfalse_b1", True),
    (1, 261, 261, 1, 64, 300, None, False),        # FOURIER_POS_PIXEL width
    (1, 512, 512, 1, 300, 2048, "query", False),   # flow / multimodal decoders: two dv slices
    (1, 704, 704, 1, 130, 1000, "key", False),     # multimodal encoder: two dv slices of 352
    (8, 32, 160, 2, 256, 2048, "key", True),       # language encoder
    (8, 32, 96, 2, 700, 256, "query", False),      # language decoder
    (4, 64, 64, 2, 100, 333, "key", False),        # generic narrow heads on the (128, 128) instantiation
    (2, 128, 128, 1, 77, 150, "query", False),
    (1, 322, 322, 2, 1, 5, "key", False),          # edge: one query row, fewer keys than one 32-key tile
    (8, 32, 96, 1, 3, 33, "query", False),         # edge: a second tile holding a single key
    (1, 512, 512, 2, 129, 31, None, True),         # edge: ragged query tile, Tk = tile - 1, broadcast Q
    # heads wider than the tiled kernel covers, over <= 512 keys: xattn_tall_kernel (pio_xtall.hip; the ImageNet decoder)
    (1, 1024, 1024, 2, 300, 512, None, True),      # the decoder's shape class: broadcast Q, ragged last query tile
    (1, 1024, 1024, 2, 200, 480, "key", False),    # key mask words + a tail past Tk inside the last 32-key block
    (1, 1024, 1024, 2, 77, 100, "query", False),   # Tk far below 512: clamped K rows / V^T columns, wiped query rows
    (1, 768, 512, 3, 130, 257, "key_allfalse_b1", True),   # dk != dv, a key block holding one key, a sample without keys
    (2, 800, 256, 1, 33, 512, None, False),        # two heads, dk = 25 chunks of 32, one dv pass
]


def _attention_vector_masks(m, xq, xkv, kv_mask, q_mask, dev):
    """Attention.forward through the C-ABI with the mask VECTORS (what PerceiverEncoder / PerceiverDecoder pass)."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    lib = P.lib()
    d = m._desc()
    B, Tq = xq.shape[0], xq.shape[1]
    Tk = xkv.shape[1]
    out = torch.empty((B, Tq, m.final.out_features), dtype=torch.float32, device=dev)
    ws = R.workspace(dev, lib.pio_attention_workspace_bytes(d, B, Tq, Tk))
    keep = []
    kp = qp = None
    if kv_mask is not None:
        km = _t(kv_mask, dev).view(torch.uint8)
        keep.append(km)
        kp = km.data_ptr()
    if q_mask is not None:
        qm = _t(q_mask, dev).view(torch.uint8)
        keep.append(qm)
        qp = qm.data_ptr()
    L.check(lib.pio_attention_fwd(d, R.tensor3(xq), R.tensor3(xkv), R.tensor3(xkv), kp, qp, None, None,
                                  out.data_ptr(), None, ws.data_ptr(), ws.numel(), R.stream_ptr(dev)), "pio_attention_fwd")
    torch.cuda.synchronize()
    return out


def _attention_vector_masks_kv(m, xq, xk, xv, kv_mask, q_mask, dev):
    """as _attention_vector_masks, with separate key and value inputs"""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    lib = P.lib()
    d = m._desc()
    B, Tq, Tk = xq.shape[0], xq.shape[1], xk.shape[1]
    out = torch.empty((B, Tq, m.final.out_features), dtype=torch.float32, device=dev)
    ws = R.workspace(dev, lib.pio_attention_workspace_bytes(d, B, Tq, Tk))
    keep = []
    kp = qp = None
    if kv_mask is not None:
        keep.append(_t(kv_mask, dev).view(torch.uint8))
        kp = keep[-1].data_ptr()
    if q_mask is not None:
        keep.append(_t(q_mask, dev).view(torch.uint8))
        qp = keep[-1].data_ptr()
    L.check(lib.pio_attention_fwd(d, R.tensor3(xq), R.tensor3(xk), R.tensor3(xv), kp, qp, None, None,
                                  out.data_ptr(), None, ws.data_ptr(), ws.numel(), R.stream_ptr(dev)), "pio_attention_fwd")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("policy", ["fp16", "fp16x2w", "bf16", "fp16x3f"])
@pytest.mark.parametrize("case", XATTN_CASES)
def test_fused_cross_attention_vs_oracle(dev, case, policy):
    """Attention on the fused cross-attention kernel (mask vectors, wide heads, dv != dk, key splits) against the float64
    oracle with the equivalent full mask, and against the materialised path of the SAME policy (full mask tensor)."""
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    H, dk, dv, B, Tq, Tk, mk, bcast = case
    q_in, kv_in = 64, 96
    p = O.gen_attention("", q_in, kv_in, H * dk, H * dv, q_in, seed=dk + Tq)
    rng = np.random.default_rng(Tk + dk)
    xq = rng.standard_normal((1 if bcast else B, Tq, q_in)).astype(np.float32)
    xkv = rng.standard_normal((B, Tk, kv_in)).astype(np.float32)
    qm = km = None
    if mk in ("key", "key_allfalse_b1"):
        km = rng.random((B, Tk)) > 0.3
        km[:, 0] = True
        if mk == "key_allfalse_b1":
            km[1, :] = False
    elif mk == "query":
        qm = rng.random((B, Tq)) > 0.3
    m = Attention(q_in, kv_in, kv_in, num_heads=H, qk_out_channels=H * dk, v_out_channels=H * dv, output_channels=q_in)
    m.load_state_dict(_sd(p, "cpu"))
    m = m.to(dev).eval()
    xq_full = np.broadcast_to(xq, (B, Tq, q_in))
    mask3 = None
    if mk is not None:
        mask3 = O.make_cross_attention_mask(qm if qm is not None else np.ones((B, Tq), bool),
                                            km if km is not None else np.ones((B, Tk), bool))
    p64 = {k: a.astype(np.float64) for k, a in p.items()}
    ref = O.attention(p64, xq_full.astype(np.float64), xkv.astype(np.float64), xkv.astype(np.float64), H, mask3)
    xq_t = _t(xq, dev)
    if bcast:
        xq_t = torch.broadcast_to(xq_t, (B, Tq, q_in))          # stride-0 batch: Q is projected once
    _policy(policy)
    y = _attention_vector_masks(m, xq_t, _t(xkv, dev), km, qm, dev)
    # (random toy weights on 64 / 96 input channels: operand rounding alone is ~1e-3 here -- the budget of the toy
    #  goldens; the kernel itself is held to TOL against the materialised path of the same policy below, and against the
    #  oracle with real projections at the shipped widths in
    #  test_fused_cross_attention_real_projections_at_shipped_widths_vs_oracle)
    tol = TOL if policy != "bf16" else 1e-2
    if policy == "fp16x3f":
        # split projections around a single-sweep fused core: only q / k / v / p are rounded once -- held to the 1e-3 bar
        # against the oracle even on these toy widths (worst 3.8e-4 / 6.3e-4), and against the fully 3-sweep
        # materialised path below
        _assert_close(y, ref, TOL, what=f"fused cross-attention {case} {policy}")
    else:
        _assert_close(y, ref, FAST_TOY_BUDGET if policy != "bf16" else 2e-2, what=f"fused cross-attention {case} {policy}")
    if mk == "key_allfalse_b1":
        fb = m.final.bias.detach()
        assert torch.equal(y[1], fb[None, :].expand_as(y[1])), "sample without an attendable key must give final.bias"
    # same policy, materialised path (a full mask tensor forces it): same operand rounding, different algorithm
    full = _t(mask3 if mask3 is not None else np.ones((B, Tq, Tk), bool), dev)
    ym = m(xq_t, _t(xkv, dev), _t(xkv, dev), attention_mask=full)
    _assert_close(y, ym.detach().cpu().numpy(), tol, what=f"fused vs materialised {case} {policy}")


# The fused attention KERNELS alone, at the widths of the shipped models, against the float64 oracle at the north_star's
# 1e-3: the projections around the core are identities on fp16-exact inputs (q = xq, k = xk, v = xv, out = core output),
# so nothing but the kernel's own arithmetic (Q K^T in fp32, softmax, P rounded to 16 bits, P V in fp32, one 16-bit
# rounding of the output) separates the result from transformer_primitives.py:138-175 computed in float64.
KERNEL_CASES = [
    # heads, dk, dv, B, Tq, Tk, mask kind, kernel
    (1, 328, 328, 2, 512, 3136, "key", "xattn<352,352> (ImageNet / flow encoder, 322 padded to 328; single pass)"),
    (1, 512, 512, 1, 1024, 784, "query", "xattn<512,512> (multimodal / flow decoder; single pass)"),
    (1, 704, 704, 1, 784, 4096, None, "xattn<704,256> (multimodal encoder, key split)"),
    (8, 32, 160, 2, 256, 2048, "key", "xattn<32,160> (language encoder)"),
    (8, 32, 96, 2, 2048, 256, "query", "xattn<32,96> (language decoder)"),
    (1, 1024, 1024, 2, 1000, 512, None, "xattn_tall (ImageNet decoder)"),
    (8, 128, 128, 4, 512, 512, None, "flash_attn<128,128> (ImageNet latent self-attention)"),
    (16, 32, 32, 1, 2048, 2048, None, "flash_attn<32,32> (flow latent self-attention)"),
    (8, 64, 64, 1, 784, 784, None, "flash_attn<64,64> (multimodal latent self-attention)"),
]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c[-1].split(" ")[0] for c in KERNEL_CASES])
def test_fused_attention_kernels_at_shipped_widths_vs_oracle(dev, case):
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    H, dk, dv, B, Tq, Tk, mk, what = case
    rng = np.random.default_rng(dk * 7 + Tk)
    f16 = lambda a: a.astype(np.float16).astype(np.float32)  # noqa: E731  (fp16-exact inputs: the identity projections are exact)
    xq = f16(rng.standard_normal((B, Tq, H * dk)))
    xk = f16(rng.standard_normal((B, Tk, H * dk)))
    xv = f16(rng.standard_normal((B, Tk, H * dv)))
    qm = km = None
    if mk == "key":
        km = rng.random((B, Tk)) > 0.3
        km[:, 0] = True
    elif mk == "query":
        qm = rng.random((B, Tq)) > 0.3
    m = Attention(H * dk, H * dk, H * dv, num_heads=H, qk_out_channels=H * dk, v_out_channels=H * dv,
                  output_channels=H * dv)
    with torch.no_grad():
        for lin, n in ((m.proj_q, H * dk), (m.proj_k, H * dk), (m.proj_v, H * dv), (m.final, H * dv)):
            lin.weight.copy_(torch.eye(n))
            lin.bias.zero_()
    m = m.to(dev).eval()
    p64 = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    mask3 = None
    if mk is not None:
        mask3 = O.make_cross_attention_mask(qm if qm is not None else np.ones((B, Tq), bool),
                                            km if km is not None else np.ones((B, Tk), bool))
    ref = O.attention(p64, xq.astype(np.float64), xk.astype(np.float64), xv.astype(np.float64), H, mask3)
    _policy("fp16")
    try:
        y = _attention_vector_masks_kv(m, _t(xq, dev), _t(xk, dev), _t(xv, dev), km, qm, dev)
    finally:
        _policy("fp16x3")
    rl2, rmax = _errs(y, ref)
    print(f"{what}: relL2={rl2:.3e} max/absmax={rmax:.3e}")
    assert rl2 <= TOL and rmax <= TOL, f"{what}: relL2={rl2:.3e} max/absmax={rmax:.3e}"


# The same kernels inside whole Attention modules with REAL (non-identity, fan-in-scaled random) projections at the widths
# of the shipped cross-attends, single-sweep fp16, against the float64 oracle at the north_star's 1e-3 -- the bound the
# toy-width cases above cannot carry (FAST_TOY_BUDGET: operand rounding on 64 / 96 input channels alone exceeds 1e-3).
XATTN_SHIPPED = [
    # q_in, kv_in, heads, qk, v, out, B, Tq, Tk, mask kind, the policy this cross-attend ships under, what
    (1024, 322, 1, 322, 322, 1024, 2, 512, 3136, None, "fp16x2w", "imagenet-encoder xattn<352,352>"),
    (1024, 1024, 1, 1024, 1024, 1024, 2, 1000, 512, None, "fp16x3f", "imagenet-decoder xattn_tall"),
    (512, 322, 1, 322, 322, 512, 1, 2048, 6000, None, "fp16", "flow-encoder xattn<352,352> key splits"),
    (322, 512, 1, 512, 512, 322, 1, 4096, 2048, None, "fp16x2af", "flow-decoder xattn<512,512>"),
    (512, 704, 1, 704, 704, 512, 1, 784, 4096, None, "fp16x2w", "multimodal-encoder xattn<704,256>"),
    (1026, 512, 1, 512, 512, 1026, 1, 3000, 784, None, "fp16x3f", "multimodal-decoder xattn<512,512>"),
    (1280, 768, 8, 256, 1280, 1280, 2, 256, 2048, "key", "fp16x3f", "language-encoder xattn<32,160>"),
    (768, 1280, 8, 256, 768, 768, 2, 2048, 256, "query", "fp16x3f", "language-decoder xattn<32,96>"),
]
# single-sweep fp16 around these two cores measures 7.1e-4 / 1.23e-3 and 7.8e-4 / 1.32e-3 (1024- / 1280-deep products
# with 11-bit operands on both sides, un-averaged output rows): the kernels are fine -- the same cores under the shipped
# split-operand projections hold 1e-3 -- but "fp16" is not a parity configuration for them; bound written down here
SINGLE_SWEEP_BUDGET = {"imagenet-decoder": 1.5e-3, "language-decoder": 1.5e-3}


@pytest.mark.parametrize("which", ["single sweep", "shipped policy"])
@pytest.mark.parametrize("case", XATTN_SHIPPED, ids=[c[-1].split(" ")[0] for c in XATTN_SHIPPED])
def test_fused_cross_attention_real_projections_at_shipped_widths_vs_oracle(dev, case, which):
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    q_in, kv_in, H, qk, vv, outc, B, Tq, Tk, mk, shipped, what = case
    policy = "fp16" if which == "single sweep" else shipped
    if which == "shipped policy" and shipped == "fp16":
        pytest.skip("ships single-sweep: covered by the other leg")
    tol = SINGLE_SWEEP_BUDGET.get(what.split(" ")[0], TOL) if which == "single sweep" else TOL
    p = O.gen_attention("", q_in, kv_in, qk, vv, outc, seed=q_in + Tk)
    rng = np.random.default_rng(Tq + kv_in)
    xq = rng.standard_normal((B, Tq, q_in)).astype(np.float32)            # (what the LayerNorms in front deliver)
    xkv = rng.standard_normal((B, Tk, kv_in)).astype(np.float32)
    qm = km = None
    if mk == "key":
        km = rng.random((B, Tk)) > 0.3
        km[:, 0] = True
    elif mk == "query":
        qm = rng.random((B, Tq)) > 0.3
    m = Attention(q_in, kv_in, kv_in, num_heads=H, qk_out_channels=qk, v_out_channels=vv, output_channels=outc)
    m.load_state_dict(_sd(p, "cpu"))
    m = m.to(dev).eval()
    mask3 = None
    if mk is not None:
        mask3 = O.make_cross_attention_mask(qm if qm is not None else np.ones((B, Tq), bool),
                                            km if km is not None else np.ones((B, Tk), bool))
    p64 = {k: a.astype(np.float64) for k, a in p.items()}
    ref = O.attention(p64, xq.astype(np.float64), xkv.astype(np.float64), xkv.astype(np.float64), H, mask3)
    _policy(policy)
    try:
        y = _attention_vector_masks(m, _t(xq, dev), _t(xkv, dev), km, qm, dev)
    finally:
        _policy("fp16x3")
    rl2, rmax = _errs(y, ref)
    print(f"{what} [{policy}]: relL2={rl2:.3e} max/absmax={rmax:.3e}")
    assert rl2 <= tol and rmax <= tol, f"{what} [{policy}]: relL2={rl2:.3e} max/absmax={rmax:.3e} > {tol}"


@pytest.mark.parametrize("policy", ["fp16", "fp16x2af"])
@pytest.mark.parametrize("kv_in,Tq,Tk,B,bcast", [(322, 512, 3136, 3, True), (704, 200, 2500, 1, False),
                                                 (512, 130, 4097, 2, False),
                                                 (1024, 1000, 512, 8, True)])   # the ImageNet decoder's shape: xattn_tall
def test_kv_projection_fold_of_single_head_cross_attention(dev, kv_in, Tq, Tk, B, bcast, policy, monkeypatch):
    """pio_attention_t.kq / vo: a single-head cross-attend over many keys computed as
    softmax((Q Wk) LN(x)^T) LN(x) (Wo Wv)^T + (Wo bv + bo) -- no K / V projection GEMMs -- against the float64 oracle of
    transformer_primitives.py:90-180, and against the un-folded path of the same policy.  With a key mask the fold must
    step aside (a sample without an attendable key comes out as final.bias alone)."""
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    q_in = 256
    p = O.gen_attention("", q_in, kv_in, kv_in, kv_in, q_in, seed=kv_in + Tq)
    rng = np.random.default_rng(Tk)
    xq = rng.standard_normal((1 if bcast else B, Tq, q_in)).astype(np.float32)
    xkv = rng.standard_normal((B, Tk, kv_in)).astype(np.float32)
    m = Attention(q_in, kv_in, kv_in, num_heads=1, qk_out_channels=kv_in, v_out_channels=kv_in, output_channels=q_in)
    m.load_state_dict(_sd(p, "cpu"))
    m = m.to(dev).eval()
    p64 = {k: a.astype(np.float64) for k, a in p.items()}
    xq_full = np.broadcast_to(xq, (B, Tq, q_in))
    ref = O.attention(p64, xq_full.astype(np.float64), xkv.astype(np.float64), xkv.astype(np.float64), 1, None)
    xq_t = _t(xq, dev)
    if bcast:
        xq_t = torch.broadcast_to(xq_t, (B, Tq, q_in))
    _policy(policy)
    try:
        y = _attention_vector_masks(m, xq_t, _t(xkv, dev), None, None, dev)
        monkeypatch.setenv("PIO_KV_FOLD", "0")
        y0 = _attention_vector_masks(m, xq_t, _t(xkv, dev), None, None, dev)
        monkeypatch.delenv("PIO_KV_FOLD")
        rl2, rmax = _assert_close(y, ref, TOL, what=f"K/V fold kv_in={kv_in} {policy}")
        e0 = _errs(y0, ref)
        print(f"kv_in={kv_in} Tq={Tq} Tk={Tk} {policy}: folded {rl2:.3e} / {rmax:.3e}, un-folded {e0[0]:.3e} / {e0[1]:.3e}")
        assert not torch.equal(y, y0), "the fold did not engage"
        # key mask with one sample fully masked: the un-folded path, bit for bit, and final.bias rows
        km = rng.random((B, Tk)) > 0.3
        km[:, 0] = True
        km[B - 1, :] = False
        ym = _attention_vector_masks(m, xq_t, _t(xkv, dev), km, None, dev)
        monkeypatch.setenv("PIO_KV_FOLD", "0")
        ym0 = _attention_vector_masks(m, xq_t, _t(xkv, dev), km, None, dev)
        assert torch.equal(ym, ym0)
        if policy == "fp16":
            fb = m.final.bias.detach()
            assert torch.equal(ym[B - 1], fb[None, :].expand_as(ym[B - 1]))
    finally:
        _policy("fp16x3")


# ----------------------------------------------------------------------------------------------------
# fp16 range: the LayerNorm-folded stack carries the residual stream as an fp16 pair
# ----------------------------------------------------------------------------------------------------
def _fold_stack(dev, scale, offset=0.0, outlier=0.0, policy="fp16"):
    """A 1024-channel PerceiverEncoder (2 shared layers x 2 blocks) on 2048 latent rows whose latent table is scaled /
    shifted: returns (folded fp16, un-folded fp16, fp16x3) outputs and whether the guard re-ran the call."""
    from perceiverio_pytorch_amd import runtime as R
    from perceiverio_pytorch_amd.perceiver import PerceiverEncoder
    import perceiverio_pytorch_amd as P
    lib = P.lib()
    C_, N, D, Lyr = 64, 512, 1024, 2
    p_enc = O.gen_encoder(C_, N, D, Lyr, seed=77)
    lat = p_enc["latent_pos_enc.pos_embs"] * scale + offset
    if outlier:
        lat[:, 7] = outlier                      # one channel far from the others
    p_enc["latent_pos_enc.pos_embs"] = lat.astype(np.float32)
    enc = PerceiverEncoder(C_, Lyr, 2, N, D, num_self_attend_heads=8)
    enc.load_state_dict(_sd(p_enc, "cpu"))
    enc = enc.to(dev).eval()
    x = _t(np.random.default_rng(3).standard_normal((4, 96, C_)).astype(np.float32), dev)
    outs = {}
    prev = lib.pio_ln_fold_enable(2)       # 2048 rows: below the automatic setting's 6144
    try:
        _policy(policy)
        outs["fold"] = enc(x, enc.latents(x)).clone()
        lib.pio_ln_fold_enable(0)
        outs["plain"] = enc(x, enc.latents(x)).clone()
        _policy("fp16x3")
        outs["x3"] = enc(x, enc.latents(x)).clone()
    finally:
        lib.pio_ln_fold_enable(prev)
        _policy("fp16x3")
    return outs


@pytest.mark.parametrize("policy", ["fp16", "fp16x2s", "fp16x2w"])
def test_fold_range_guard_falls_back_on_overflow(dev, policy):
    """Latents beyond the fp16 range (65504): the folded stack alone would return inf / nan; with the guard
    (runtime.range_check, default on: a device word the fold's producer GEMMs report into) the call is re-run un-folded
    and matches the un-folded result bit for bit -- under EVERY policy the fold is offered for."""
    from perceiverio_pytorch_amd import runtime as R
    assert R.range_check()
    outs = _fold_stack(dev, scale=3.0e5, policy=policy)        # |latents| up to ~1e6 >> 65504
    assert torch.isfinite(outs["fold"]).all(), "the guard must have replaced the overflowed result"
    assert torch.equal(outs["fold"], outs["plain"])
    _assert_close(outs["plain"], outs["x3"].cpu().numpy(), TOL, what=f"un-folded {policy} vs fp16x3 at |x| ~ 1e6")
    R.set_range_check(False)
    try:
        raw = _fold_stack(dev, scale=3.0e5, policy=policy)["fold"]
    finally:
        R.set_range_check(True)
    assert not torch.isfinite(raw).all(), "without the guard the fp16-pair stream overflows (documented behaviour)"
    # in-range latents leave the word untouched
    _fold_stack(dev, scale=1.0, policy=policy)
    assert int(R.last_range_flag(dev).item()) == 0


@pytest.mark.parametrize("D,fold", [(1024, True), (72, False)])
def test_per_block_images_path_equals_shared_path_when_images_are_equal(dev, D, fold, monkeypatch):
    """Policy "fp16sd" hands pio_encoder_fwd one descriptor set per block (per_block).  With the error feedback switched off
    (every block gets the round-to-nearest image) the result must equal policy "fp16" bit for bit -- same kernels, same
    order, only the weight pointers differ -- with and without the LayerNorm fold; with the feedback on it must differ
    (the images do) and stay as close to the fp16x3 result."""
    from perceiverio_pytorch_amd import runtime as R
    from perceiverio_pytorch_amd.perceiver import PerceiverEncoder
    import perceiverio_pytorch_amd as P
    lib = P.lib()
    C_, N, Lyr, nblk = 40, 512, 2, 3
    p_enc = O.gen_encoder(C_, N, D, Lyr, seed=21)
    enc = PerceiverEncoder(C_, Lyr, nblk, N, D, num_self_attend_heads=8)
    enc.load_state_dict(_sd(p_enc, "cpu"))
    enc = enc.to(dev).eval()
    x = _t(np.random.default_rng(4).standard_normal((4, 60, C_)).astype(np.float32), dev)
    prev = lib.pio_ln_fold_enable(2 if fold else 0)
    try:
        _policy("fp16")
        y16 = enc(x, enc.latents(x)).clone()
        _policy("fp16sd")
        y_sd = enc(x, enc.latents(x)).clone()
        tdt = torch.float16

        def no_feedback(w, n, dtype):
            hi = w.detach().float().to(tdt).float()
            return [hi for _ in range(n)]
        monkeypatch.setattr(R, "feedback_images", no_feedback)
        R.invalidate_packed_weights(enc)
        y_eq = enc(x, enc.latents(x)).clone()
        monkeypatch.undo()
        R.invalidate_packed_weights(enc)
        _policy("fp16x3")
        y3 = enc(x, enc.latents(x)).clone()
    finally:
        lib.pio_ln_fold_enable(prev)
        _policy("fp16x3")
    assert torch.equal(y_eq, y16), "per-block path with equal images must reproduce the shared-image path"
    assert not torch.equal(y_sd, y16), "error-feedback images must differ from the round-to-nearest ones"
    e16, esd = _errs(y16, y3.cpu().numpy()), _errs(y_sd, y3.cpu().numpy())
    print(f"D={D} fold={fold}: fp16 relL2={e16[0]:.2e} max={e16[1]:.2e} | fp16sd relL2={esd[0]:.2e} max={esd[1]:.2e}")
    assert esd[0] <= TOL and esd[1] <= TOL


def _fold_lib():
    import perceiverio_pytorch_amd as P
    return P.lib()


def test_range_guard_is_deferred_and_graph_capturable(dev):
    """PerceiverIO.forward resolves the range guard once, after the decoder (no synchronisation between encoder and
    decoder), and the whole module forward -- guard ON -- captures into a HIP graph: during capture nothing is read
    from the device, the word stays in runtime.last_range_flag for the owner of the graph."""
    from perceiverio_pytorch_amd import runtime as R
    from perceiverio_pytorch_amd.perceiver import PerceiverIO
    from perceiverio_pytorch_amd.output_queries import TrainableQuery
    assert R.range_check()
    torch.manual_seed(5)
    m = PerceiverIO(num_blocks=2, num_self_attends_per_block=2, num_latents=512, num_latent_channels=1024,
                    final_project=True, final_project_out_channels=16, input_channels=64,
                    output_queries=TrainableQuery(output_index_dims=8, num_channels=1024)).to(dev).eval()
    x = torch.randn(4, 96, 64, device=dev)                       # 4 x 512 = 2048 latent rows: the fold is active
    _policy("fp16")
    prev_fold = _fold_lib().pio_ln_fold_enable(2)                # (forced: automatic starts at 6144 rows)
    try:
        with torch.inference_mode():
            y = m(x).clone()
            assert torch.isfinite(y).all()
            # (a) overflow inside PerceiverIO.forward: deferred check, un-folded repeat of the whole forward
            with torch.no_grad():
                saved = m._encoder.latent_pos_enc.pos_embs.clone()
                m._encoder.latent_pos_enc.pos_embs.mul_(3.0e5 / 0.02)
            y_big = m(x).clone()
            assert torch.isfinite(y_big).all(), "deferred guard must have repeated the forward un-folded"
            with torch.no_grad():
                m._encoder.latent_pos_enc.pos_embs.copy_(saved)
            # (b) capture with the guard on
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    m(x)
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                yg = m(x)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(yg, y), "graph replay must reproduce the eager logits"
            assert int(R.last_range_flag(dev).item()) == 0
    finally:
        _fold_lib().pio_ln_fold_enable(prev_fold)
        _policy("fp16x3")


@pytest.mark.parametrize("kind", ["dc_offset_30sigma", "outlier_channel_1e4"])
def test_fold_on_adversarial_rows(dev, kind):
    """Rows with a DC offset of 30 sigma, or one channel near 1e4: the fold computes var = E[x^2] - mean^2 in fp32 from
    per-128-column partial sums and reads the un-normalised fp16 stream -- held to the same 1e-3 as the un-folded path
    against the float32-grade policy."""
    outs = _fold_stack(dev, scale=1.0, offset=15.0) if kind == "dc_offset_30sigma" else \
        _fold_stack(dev, scale=1.0, outlier=1.0e4)
    ref = outs["x3"].cpu().numpy()
    e_fold, e_plain = _errs(outs["fold"], ref), _errs(outs["plain"], ref)
    print(f"{kind}: fold relL2={e_fold[0]:.2e} max={e_fold[1]:.2e} | un-folded relL2={e_plain[0]:.2e} max={e_plain[1]:.2e}")
    assert e_fold[0] <= TOL and e_fold[1] <= TOL, (kind, e_fold, e_plain)


def test_layernorm_cast_cat_equals_layernorm_of_concatenation(dev):
    """pio_layernorm_cast_cat([x1 | table]) == pio_layernorm_cast(cat(x1, table)) bit for bit, and the oracle's
    LayerNorm of the concatenated row within 16-bit rounding."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    lib = P.lib()
    rng = np.random.default_rng(9)
    B, T, C1, C2 = 3, 50, 64, 258
    x1 = rng.standard_normal((B, T, C1)).astype(np.float32)
    tab = rng.standard_normal((1, T, C2)).astype(np.float32)
    gamma = (1 + 0.1 * rng.standard_normal(C1 + C2)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(C1 + C2)).astype(np.float32)
    cp = R.pad8(C1 + C2)
    t1, t2, tg, tb = _t(x1, dev), _t(tab, dev), _t(gamma, dev), _t(beta, dev)
    cat = torch.cat([t1, t2.expand(B, T, C2)], dim=-1).contiguous()
    ln = L.LayerNorm(tg.data_ptr(), tb.data_ptr(), C1 + C2, 1e-5)
    ya = torch.empty((B * T, cp), dtype=torch.float16, device=dev)
    yb = torch.empty_like(ya)
    la, lb = torch.empty_like(ya), torch.empty_like(ya)
    s = R.stream_ptr(dev)
    L.check(lib.pio_layernorm_cast_cat(R.tensor3(t1), R.tensor3(t2), ln, ya.data_ptr(), la.data_ptr(), cp,
                                       L.PIO_DT_F16, s), "cat")
    L.check(lib.pio_layernorm_cast(R.tensor3(cat), ln, yb.data_ptr(), lb.data_ptr(), cp, L.PIO_DT_F16, s), "plain")
    torch.cuda.synchronize()
    assert torch.equal(ya, yb) and torch.equal(la, lb)
    ref = O.layer_norm(np.concatenate([x1, np.broadcast_to(tab, (B, T, C2))], -1).astype(np.float64),
                       gamma.astype(np.float64), beta.astype(np.float64))
    got = (ya.float() + la.float()).cpu().numpy().reshape(B, T, cp)
    assert np.abs(got[..., :C1 + C2] - ref).max() <= 2e-6 and (got[..., C1 + C2:] == 0).all()


def test_fused_cross_attention_fuzz(dev):
    """Seeded random shapes / masks through the fused cross-attention kernel against the materialised path of the same
    policy (full mask tensor): every instantiation, ragged tiles, key splits, dv slices, broadcast Q."""
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    rng = np.random.default_rng(2024)
    widths = [(1, 322, 322), (1, 264, 264), (1, 512, 512), (1, 704, 704), (1, 400, 320), (8, 32, 160), (8, 32, 96),
              (4, 64, 64), (2, 128, 128), (3, 40, 24), (1, 136, 200)]
    _policy("fp16")
    for it in range(22):
        H, dk, dv = widths[it % len(widths)]
        B = int(rng.integers(1, 4))
        Tq = int(rng.integers(1, 600))
        Tk = int(rng.integers(1, 3000))
        mk = [None, "key", "query"][int(rng.integers(0, 3))]
        bcast = bool(rng.integers(0, 2))
        q_in, kv_in = 64, 96
        p = O.gen_attention("", q_in, kv_in, H * dk, H * dv, q_in, seed=100 + it)
        xq = rng.standard_normal((1 if bcast else B, Tq, q_in)).astype(np.float32)
        xkv = rng.standard_normal((B, Tk, kv_in)).astype(np.float32)
        qm = km = None
        if mk == "key":
            km = rng.random((B, Tk)) > 0.4
            if B > 1:
                km[B - 1, :] = False                 # one sample without any attendable key
        elif mk == "query":
            qm = rng.random((B, Tq)) > 0.4
        m = Attention(q_in, kv_in, kv_in, num_heads=H, qk_out_channels=H * dk, v_out_channels=H * dv,
                      output_channels=q_in)
        m.load_state_dict(_sd(p, "cpu"))
        m = m.to(dev).eval()
        xq_t = _t(xq, dev)
        if bcast:
            xq_t = torch.broadcast_to(xq_t, (B, Tq, q_in))
        y = _attention_vector_masks(m, xq_t, _t(xkv, dev), km, qm, dev)
        mask3 = O.make_cross_attention_mask(qm if qm is not None else np.ones((B, Tq), bool),
                                            km if km is not None else np.ones((B, Tk), bool))
        ym = m(xq_t, _t(xkv, dev), _t(xkv, dev), attention_mask=_t(mask3, dev))
        assert torch.isfinite(y).all(), (it, H, dk, dv, B, Tq, Tk, mk)
        _assert_close(y, ym.detach().cpu().numpy(), TOL, what=f"fuzz {it}: H={H} dk={dk} dv={dv} B={B} Tq={Tq} Tk={Tk} {mk}")


def test_fused_cross_attention_is_deterministic(dev):
    """The cross-attention kernel's LDS ring runs on COUNTED waits and raw barriers: a miscounted wait would show as a
    run-to-run difference.  Thirty launches per shape (ragged piece shares, key splits, every ring depth) under uneven
    load must agree bit for bit."""
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    rng = np.random.default_rng(7)
    _policy("fp16")
    for (H, dk, dv, B, Tq, Tk) in [(1, 322, 322, 3, 300, 3000), (1, 704, 704, 1, 200, 5000), (1, 512, 512, 2, 257, 700),
                                   (8, 32, 160, 2, 256, 2048), (8, 32, 96, 1, 130, 999), (2, 128, 128, 5, 100, 640)]:
        q_in, kv_in = 64, 96
        p = O.gen_attention("", q_in, kv_in, H * dk, H * dv, q_in, seed=dk + Tk)
        m = Attention(q_in, kv_in, kv_in, num_heads=H, qk_out_channels=H * dk, v_out_channels=H * dv,
                      output_channels=q_in)
        m.load_state_dict(_sd(p, "cpu"))
        m = m.to(dev).eval()
        xq = _t(rng.standard_normal((B, Tq, q_in)).astype(np.float32), dev)
        xkv = _t(rng.standard_normal((B, Tk, kv_in)).astype(np.float32), dev)
        km = rng.random((B, Tk)) > 0.2
        first = _attention_vector_masks(m, xq, xkv, km, None, dev).clone()
        noise = torch.randn(4096, 4096, device=dev)
        for it in range(30):
            if it % 3 == 0:
                noise = noise @ noise.T * 1e-4          # something else keeps part of the chip busy
            y = _attention_vector_masks(m, xq, xkv, km, None, dev)
            assert torch.equal(y, first), f"run {it} differs for H={H} dk={dk} dv={dv} B={B} Tq={Tq} Tk={Tk}"


@pytest.mark.gpu
@pytest.mark.parametrize("shape,channels,layers,bn", [((2, 3, 224, 224), 64, 1, True), ((3, 3, 61, 45), 64, 1, True),
                                                      ((2, 3, 64, 50), 32, 1, False), ((2, 3, 96, 96), 96, 2, True),
                                                      ((1, 3, 30, 422), 64, 1, True)])
def test_conv_downsample_fused_tail_matches_torch_ops(dev, shape, channels, layers, bn):
    """pio_bn_relu_maxpool_tokens (BatchNorm(eval) -> ReLU -> 3x3/2 SAME max-pool -> channels-last tokens in one pass)
    against the same network through torch's ops (processor_utils.py:163-180): odd / even maps, channel counts off the
    64-channel group, two layers, no BatchNorm; fp32 rounding of the folded scale / shift only."""
    from perceiverio_pytorch_amd.io_processors import Conv2DDownsample
    torch.manual_seed(5)
    net = Conv2DDownsample(num_layers=layers, num_channels=channels, use_batchnorm=bn).to(dev).eval()
    if bn:
        for m in net.norms:
            m.running_mean.normal_(0, 0.02)
            m.running_var.uniform_(0.5, 2.0)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.02)
    for conv in net.convs:
        conv.weight.data.mul_(10.0)
    x = torch.randn(shape, device=dev)
    want = net(x)
    want = want.movedim(1, -1).reshape(want.shape[0], -1, want.shape[1])
    got = net.forward_tokens(x)
    assert got is not None and got.shape == want.shape
    assert float(want.abs().max()) > 0.1
    torch.testing.assert_close(got, want, rtol=2e-5, atol=2e-6)
    net.train()
    assert (net.forward_tokens(x) is None) == bn          # training-mode BatchNorm is not folded




def test_cpu_plumbing_backend_refuses_gpu_tensors(dev):
    """set_backend("torch") is the CPU plumbing path of BASELINE config 1: a CUDA tensor under it raises instead of
    silently running eager ops on the GPU (and the default backend is restored untouched)."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd.transformer_primitives import MLP as HipMLP
    m = HipMLP(32, widening_factor=1).to(dev).eval()
    x = torch.randn(1, 4, 32, device=dev)
    P.set_backend("torch")
    try:
        with pytest.raises(P.PioError, match="CPU plumbing"):
            m(x)
    finally:
        P.set_backend("hip")
    assert torch.isfinite(m(x)).all()
