"""GPU: the addressing of pio_gemm_nt, bit for bit, on every kernel csrc/pio_gemm_route.h can pick -- one case per
(kernel, layout) of tests/gemm_addr_cases.py through the raw C-ABI, for fp16 and bf16.

Operands are small integers, so the fp32 accumulators hold the true result in any order and the comparison has NO
tolerance: fp32 outputs equal the float64 reference, 16-bit outputs its round-to-nearest-even image, C_lo the rounded
remainder.  Every buffer, input and output, is guard | payload | guard in one allocation (Guarded of
tests/test_primitives_gpu.py).  Output payloads are NaN before the call and every element the contract does not write --
rows behind M, the pitch columns [n_store, ldc), the gaps between (batch, head) slices, a neighbouring head's columns --
must still be NaN bits afterwards; every input element the contract calls unread (pitch columns of A / B, B_lo rows
below b_lo_n0, residual columns >= N, the bias behind its last entry, gaps) is NaN, so a kernel that reads one of them,
even to multiply it by zero, leaves NaN in the result.  tests/test_gemm_addr_host.py shows on the CPU that every case
reaches the kernel it names on a 256-CU device, which the fixture below asserts this one is."""
import ctypes as C
import functools
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_addr_cases as GC  # noqa: E402
from test_primitives_gpu import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
CODES = {"PIO_E_SHAPE": -1, "PIO_E_ALIGN": -2, "PIO_E_ARG": -6}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    lib = P.lib()
    assert lib.pio_arch_ok() == 1
    # the routing the host test checked: 256 CUs, the default CU budget
    assert torch.cuda.get_device_properties(0).multi_processor_count == GC.N_CU
    prev = lib.pio_set_cu_budget(0)
    if prev:
        lib.pio_set_cu_budget(prev)
    assert prev == 0, "the CU budget must be the default"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=4)
def _reference(cid):
    """(arrays, ref, index, pad) of a case: built once on the CPU, shared by both dtypes"""
    c = next(c for c in GC.CASES + GC.MODEL_CASES + GC.REFUSED if c["id"] == cid)
    arrays = GC.make_arrays(c)
    assert GC.exact_ok(c, arrays)
    return (arrays,) + GC.ref_gemm(c, arrays)


def _put(dev, a, tdt):
    """a float32 payload (or None) -> Guarded holding it as `tdt` (integers and NaN: exact in every type)"""
    if a is None:
        return None
    g = Guarded(dev, (a.size,), tdt)
    g.t.copy_(torch.from_numpy(a).to(dev))
    return g


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _nan_bits(dtype):
    """the bit pattern Guarded fills a payload with"""
    return _bits(torch.full((1,), float("nan"), dtype=dtype))[0].item()


def _launch(dev, c, dt, arrays):
    """One pio_gemm_nt call of the case on guarded buffers -> (return code, C, C_lo or None, every Guarded)."""
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    tdt = TDT[dt]
    odt = torch.float32 if c["out_f32"] else tdt
    A, Al, B, Bl = (_put(dev, arrays[k], tdt) for k in ("A", "A_lo", "B", "B_lo"))
    bias, R = _put(dev, arrays["bias"], torch.float32), _put(dev, arrays["R"], torch.float32)
    n_c = GC.c_elements(c)
    Cg = Guarded(dev, (n_c,), odt)
    Cl = Guarded(dev, (n_c,), odt) if c["c_lo"] else None
    esz = 4 if c["out_f32"] else 2
    g = L.Gemm()
    g.A, g.B, g.C = A.ptr, B.ptr, Cg.ptr + c["c_off"] * esz
    g.A_lo = Al.ptr if Al else None
    g.B_lo = Bl.ptr if Bl else None
    g.C_lo = Cl.ptr + c["c_off"] * esz if Cl else None
    for k in ("M", "N", "K", "lda", "ldb", "ldc", "batch", "nh", "sAb", "sAh", "sBb", "sBh", "sCb", "sCh", "bias_mode",
              "out_f32", "n_store", "b_lo_n0"):
        setattr(g, k, c[k])
    g.alpha, g.act = c["alpha"], 0
    g.bias = bias.ptr + 4 * c["bias_off"] if bias else None
    if R:
        g.R, g.ldr, g.r_stride_b, g.r_rows_per_batch = R.ptr + 4 * c["r_off"], c["ldr"], c["r_stride_b"], c["r_rows"]
    g.dtype = L.PIO_DT_F16 if dt == "f16" else L.PIO_DT_BF16
    assert A.ptr % 256 == 0 and Cg.ptr % 256 == 0 and (bias is None or bias.ptr % 256 == 0) and (R is None or R.ptr % 256 == 0)
    prev = lib.pio_gemm_kernel_override(c["override"])
    try:
        rc = lib.pio_gemm_nt(C.byref(g), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        lib.pio_gemm_kernel_override(prev)
    return rc, Cg, Cl, [x for x in (A, Al, B, Bl, bias, R, Cg, Cl) if x is not None]


def _check_image(what, c, got_g, want, index, pad):
    """got_g: Guarded C / C_lo; want [batch, M, n_store] float32: the written elements bit-equal, the pad columns +0, every
    other element of the payload still the NaN it was filled with."""
    flat = got_g.t.cpu()
    nan_bits = _nan_bits(flat.dtype)
    got = flat[torch.from_numpy(index)]
    want_t = torch.from_numpy(want).to(flat.dtype)
    assert torch.equal(want_t.float(), torch.from_numpy(want)), what          # the expected image is a value of the type
    gb, wb = _bits(got).numpy(), _bits(want_t).numpy()
    bad = np.argwhere(gb != wb)
    if len(bad):
        z, m, n = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} wrong elements, first at (zb, zh, m, n) = ({z // c['nh']}, {z % c['nh']}, "
                             f"{m}, {n}): got {got[z, m, n].item()!r} expected {float(want[z, m, n])!r}")
    assert (gb[:, :, pad] == 0).all(), f"{what}: the pad columns [N, n_store) must be +0"
    untouched = torch.ones(flat.numel(), dtype=torch.bool)
    untouched[torch.from_numpy(index.reshape(-1))] = False
    stray = torch.nonzero(untouched & (_bits(flat) != nan_bits)).reshape(-1)
    if len(stray):
        e = int(stray[0]) - c["c_off"]
        raise AssertionError(f"{what}: {len(stray)} elements outside rows < M x columns < n_store of the slices were written, "
                             f"first at element {e} behind C (row {e // c['ldc']} column {e % c['ldc']} of the first slice's "
                             f"pitch): {flat[int(stray[0])].item()!r}")


def _run_exact(dev, c):
    arrays, ref, index, pad = _reference(c["id"])
    for dt in GC.DTYPES:
        what = f"gemm {c['id']} [{c['kernel']}] {dt}"
        t0 = time.perf_counter()
        rc, Cg, Cl, bufs = _launch(dev, c, dt, arrays)
        assert rc == 0, f"{what}: return code {rc}"
        for b in bufs:
            b.check(what)
        hi, lo = GC.expected_images(c, ref, dt)
        _check_image(what + " C", c, Cg, hi, index, pad)
        if Cl is not None:
            _check_image(what + " C_lo", c, Cl, lo, index, pad)
        print(f"{what}: exact, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("case", GC.CASES, ids=[c["id"] for c in GC.CASES])
def test_gemm_addressing_exact(dev, case):
    _run_exact(dev, case)


@pytest.mark.parametrize("case", GC.MODEL_CASES, ids=[c["id"] for c in GC.MODEL_CASES])
def test_gemm_model_layouts_exact(dev, case):
    """The descriptors materialised_core (csrc/pio_blocks.hip) builds for Q K^T and P V at H = 3, dk = 24, dv = 40,
    Tq = 70, Tk = 77, B = 2: heads interleaved inside the rows of Q / K and of O, tkp / tkv pitches on P and V^T."""
    _run_exact(dev, case)


@pytest.mark.parametrize("case", GC.REFUSED, ids=[c["id"] for c in GC.REFUSED])
def test_gemm_refusals_write_nothing(dev, case):
    assert not case.get("missing_base"), f"{case['id']}: its base case {case['base']} is gone from CASES"
    arrays = _reference(case["id"])[0]
    for dt in GC.DTYPES:
        what = f"gemm {case['id']} {dt}"
        rc, Cg, Cl, bufs = _launch(dev, case, dt, arrays)
        assert rc == CODES[case["expect"]], f"{what}: return code {rc}, expected {case['expect']}"
        for b in bufs:
            b.check(what)
        for g in (Cg, Cl):
            if g is not None:      # bit-untouched: the fill pattern, not just some NaN
                assert (_bits(g.t) == _nan_bits(g.t.dtype)).all().item(), f"{what}: a refused call must not write"
