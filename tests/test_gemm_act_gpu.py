"""GPU: the exact-erf GELU epilogues of pio_gemm_nt over their whole domain, on every kernel that applies one -- the cases
of tests/gemm_act_cases.py through the raw C-ABI, for fp16 and bf16 operands.

One launch evaluates GELU at every multiple of 2^-6 in [-8, 8) and at the special points (the clamp at +-6 and its
neighbours, the polynomial's worst point, tiny, subnormal, zero, and large arguments up to 3e38), each an fp32 value the
accumulator holds exactly in any summation order, and is compared with float64 0.5 x erfc(-x / sqrt 2) within the bound
gemm_act_cases derives (four times the float32 model's own deviation plus the rounding of the output form); signs,
f(0) == 0, |f(x)| <= |x|, +0 pad columns and the NaN fill of everything outside rows < M x columns < n_store are exact.
Non-finite pre-activations run in cases of their own: NaN gives NaN, +-inf a non-finite result.
tests/test_gemm_act_host.py shows on the CPU that every case reaches the kernel it names on a 256-CU device (asserted
below) and that each of nine planted faults -- tanh-GELU among them -- breaks these checks."""
import ctypes as C
import functools
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_act_cases as AC  # noqa: E402
from test_gemm_addr_gpu import TDT, _bits, _nan_bits, _put  # noqa: E402
from test_primitives_gpu import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    lib = P.lib()
    assert lib.pio_arch_ok() == 1
    # the routing the host test checked: 256 CUs, the default CU budget
    assert torch.cuda.get_device_properties(0).multi_processor_count == AC.N_CU
    prev = lib.pio_set_cu_budget(0)
    if prev:
        lib.pio_set_cu_budget(prev)
    assert prev == 0, "the CU budget must be the default"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=2)
def _reference(cid):
    """(arrays, x, ref) of a case: built once on the CPU, shared by both operand types"""
    c = AC.BY_ID[cid]
    arrays = AC.make_arrays(c)
    assert AC.exact_ok(c, arrays)
    return (arrays,) + AC.reference(c, arrays)


def _launch(dev, c, dt, arrays):
    """One pio_gemm_nt call on guarded, NaN-filled buffers -> (return code, C, C_lo or None, every Guarded)."""
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    tdt = TDT[dt]
    odt = torch.float32 if c["out_f32"] else tdt
    A, B = _put(dev, arrays["A"], tdt), _put(dev, arrays["B"], tdt)
    bias, R = _put(dev, arrays["bias"], torch.float32), _put(dev, arrays["R"], torch.float32)
    n_c = c["M"] * c["ldc"] + AC.TAIL
    Cg = Guarded(dev, (n_c,), odt)
    Cl = Guarded(dev, (n_c,), odt) if c["c_lo"] else None
    g = L.Gemm()
    g.A, g.B, g.C = A.ptr, B.ptr, Cg.ptr
    g.A_lo = g.B_lo = None
    g.C_lo = Cl.ptr if Cl else None
    for k in ("M", "N", "K", "lda", "ldb", "ldc", "batch", "nh", "sAb", "sAh", "sBb", "sBh", "sCb", "sCh", "bias_mode",
              "out_f32", "n_store", "b_lo_n0", "act"):
        setattr(g, k, c[k])
    g.alpha = c["alpha"]
    g.bias = bias.ptr
    if R:
        g.R, g.ldr, g.r_stride_b, g.r_rows_per_batch = R.ptr, c["ldr"], 0, 0
    g.dtype = L.PIO_DT_F16 if dt == "f16" else L.PIO_DT_BF16
    assert all(x.ptr % 256 == 0 for x in (A, B, Cg, bias)) and (Cl is None or Cl.ptr % 256 == 0) and (R is None or R.ptr % 256 == 0)
    prev = lib.pio_gemm_kernel_override(c["override"])
    try:
        rc = lib.pio_gemm_nt(C.byref(g), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        lib.pio_gemm_kernel_override(prev)
    return rc, Cg, Cl, [x for x in (A, B, bias, R, Cg, Cl) if x is not None]


def _image(what, c, g):
    """Guarded C / C_lo -> the written block [M, n_store] as float32; everything else in the payload -- the pitch columns
    [n_store, ldc) of every row and the elements behind row M - 1 -- must still hold the NaN bits it was filled with."""
    flat = g.t.cpu()
    M, ld, ns = c["M"], c["ldc"], c["n_store"]
    rows = flat[:M * ld].view(M, ld)
    stray = (_bits(rows[:, ns:]) != _nan_bits(flat.dtype)).sum().item() + (_bits(flat[M * ld:]) != _nan_bits(flat.dtype)).sum().item()
    assert stray == 0, f"{what}: {stray} elements behind n_store or behind row M - 1 were written"
    return rows[:, :ns].float().numpy()


@pytest.mark.parametrize("case", AC.CASES, ids=[c["id"] for c in AC.CASES])
def test_gemm_gelu_whole_domain(dev, case):
    c = case
    arrays, x, ref = _reference(c["id"])
    for dt in AC.DTYPES:
        what = f"gemm act {c['id']} [{c['kernel']} {c['form']}] {dt}"
        t0 = time.perf_counter()
        rc, Cg, Cl, bufs = _launch(dev, c, dt, arrays)
        assert rc == 0, f"{what}: return code {rc}"
        for b in bufs:
            b.check(what)
        hi = _image(what + " C", c, Cg)
        lo = _image(what + " C_lo", c, Cl) if Cl is not None else None
        e6, x6, einf, xinf = AC.worst(c, hi, lo, x, ref)
        print(f"{what}: max |got - ref| = {e6:.3e} at x = {x6!r} (|x| <= 6), max |got - ref| / |x| = {einf:.3e} at "
              f"x = {xinf!r} (|x| > 6), {time.perf_counter() - t0:.2f} s")
        bad = AC.violation(c, dt, hi, lo, x, ref)
        assert bad is None, f"{what}: {bad}"
