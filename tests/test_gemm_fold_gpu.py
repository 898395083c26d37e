"""GPU: the LayerNorm fold of pio_gemm_nt on every kernel that runs it -- one raw C-ABI call per case of
tests/gemm_fold_cases.py and type (fp16, bf16).

Every buffer -- operands, bias, residuals, the 16-bit stream, row_part, ln_part, ln_c, C, the flag word -- is
guard | payload | guard in one allocation (Guarded of tests/test_primitives_gpu.py).  Inputs carry NaN wherever the
contract says "unread", output payloads are NaN before the call, and after it every element the contract does not write
must hold the bits it held before (for the in-place stream: the input image's).  The int and exact families are compared
BIT FOR BIT; the pair family's sums, the bounded and the gelu family within the bounds gemm_fold_cases.py derives.
tests/test_gemm_fold_host.py shows on the CPU that every case reaches the kernel it names, which is asserted here to be
a 256-CU device at the default CU budget (8 CUs around the two-tiles-per-workgroup launches, restored in `finally`)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_fold_cases as FC  # noqa: E402
from test_primitives_gpu import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
CODES = {"PIO_E_SHAPE": -1, "PIO_E_ALIGN": -2, "PIO_E_ARG": -6}
FLAG_FILL = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    lib = P.lib()
    assert lib.pio_arch_ok() == 1
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256
    prev = lib.pio_set_cu_budget(0)
    if prev:
        lib.pio_set_cu_budget(prev)
    assert prev == 0, "the CU budget must be the default"
    times = {}
    yield torch.device("cuda:0"), times
    if times:
        worst = max(times, key=times.get)
        print(f"\nfold cases: {len(times)} launches + checks in {sum(times.values()):.2f} s, slowest {worst}: {times[worst]:.2f} s")


def _put(dev, a, tdt):
    """a float32 payload (or None) -> Guarded holding it as `tdt` (every value is one of the type, NaN stays NaN)"""
    if a is None:
        return None
    g = Guarded(dev, (a.size,), tdt)
    g.t.copy_(torch.from_numpy(a).to(dev))
    return g


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


class Out:
    """An output payload: the Guarded, its bits before the call, and the [rows, cols] grid at pitch ld the call writes."""

    def __init__(self, name, g, rows, ld, cols):
        self.name, self.g, self.rows, self.ld, self.cols = name, g, rows, ld, cols
        self.before = _bits(g.t).cpu().clone()

    def after(self):
        flat = self.g.t.cpu()
        return flat, _bits(flat)

    def grid(self, flat):
        return flat[:self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    def check_untouched(self, what, all_of_it=False):
        flat, bits = self.after()
        keep = torch.ones(flat.numel(), dtype=torch.bool)
        if not all_of_it:
            self.grid(keep)[:] = False
        stray = torch.nonzero(keep & (bits != self.before)).reshape(-1)
        if len(stray):
            e = int(stray[0])
            raise AssertionError(f"{what} {self.name}: {len(stray)} elements outside rows < {self.rows} x columns < {self.cols} "
                                 f"were written, first at element {e} (row {e // self.ld} column {e % self.ld} of the pitch "
                                 f"{self.ld}): {flat[e].item()!r}")

    def check_bits(self, what, want, skip_row=None, pos=("m", "n")):
        """want [rows, cols] float32: bit-equal (a skipped row: the planted one of a range case)"""
        flat, _ = self.after()
        got = self.grid(flat)
        if skip_row is not None:
            want = np.array(want, copy=True)
            want[skip_row] = 0
        want_t = torch.from_numpy(np.ascontiguousarray(want)).to(flat.dtype)
        assert torch.equal(want_t.float(), torch.from_numpy(np.ascontiguousarray(want))), f"{what} {self.name}: expectation"
        diff = _bits(got.contiguous()) != _bits(want_t)
        if skip_row is not None:
            diff[skip_row] = False
        bad = torch.nonzero(diff)
        if len(bad):
            m, n = (int(v) for v in bad[0])
            raise AssertionError(f"{what} {self.name}: {len(bad)} wrong elements, first at ({pos[0]}, {pos[1]}) = ({m}, {n}): "
                                 f"got {got[m, n].item()!r} expected {float(want[m, n])!r}")

    def check_bound(self, what, ref, bound, pos=("m", "n")):
        flat, _ = self.after()
        got = self.grid(flat).double().numpy()
        err = np.abs(got - ref)
        bad = np.argwhere(~(err <= bound))
        worst = float(np.nanmax(err / np.maximum(bound, 1e-300)))
        print(f"{what} {self.name}: worst |got - ref| / bound = {worst:.3f}")
        if len(bad):
            m, n = (int(v) for v in bad[0])
            raise AssertionError(f"{what} {self.name}: {len(bad)} elements outside the bound, first at ({pos[0]}, {pos[1]}) = "
                                 f"({m}, {n}): got {got[m, n]!r} reference {ref[m, n]!r} bound {bound[m, n]:.3e}")


def _launch(dev, c, dt, a):
    """One pio_gemm_nt call on guarded buffers -> (return code, dict of Out, flag Guarded or None, every Guarded)."""
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    tdt = TDT[dt]
    M, N = c["M"], c["N"]
    A, Al, B, Bl = (_put(dev, a[k], tdt) for k in ("A", "A_lo", "B", "B_lo"))
    bias = _put(dev, a["bias"], torch.float32)
    bufs = [A, Al, B, Bl, bias]
    g = L.Gemm()
    g.A, g.B = A.ptr, B.ptr
    g.A_lo = Al.ptr if Al else None
    g.B_lo = Bl.ptr if Bl else None
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.batch, g.nh, g.n_store = M, N, c["K"], c["lda"], c["ldb"], c["ldc"], 1, 1, c["n_store"]
    g.alpha, g.act, g.bias_mode = c["alpha"], c["act"], 1 if bias else 0
    g.bias = bias.ptr + 4 * c["bias_off"] if bias else None
    g.dtype = L.PIO_DT_F16 if dt == "f16" else L.PIO_DT_BF16
    outs, flag = {}, None
    if c["role"] == "prod":
        ld16, w = c["ld16"], c["slot_w"]
        g.out_f32, g.ld16, g.row_slot_w = 1, ld16, w
        R = _put(dev, a["R"], torch.float32)
        Rh, Rl = _put(dev, a["R_hi"], tdt), _put(dev, a["R_lo"], tdt)
        if R:
            g.R, g.ldr = R.ptr, c["ldr"]
        else:
            g.R16_hi, g.R16_lo = Rh.ptr, Rl.ptr
        if c["res"] == "inplace":
            X, Xl = Rh, Rl
        else:
            X = Guarded(dev, (M * ld16 + FC.TAIL,), tdt)
            Xl = Guarded(dev, (M * ld16 + FC.TAIL,), tdt) if c["x_lo"] else None
        g.X16, g.X16_lo = X.ptr, (Xl.ptr if Xl else None)
        outs["X16"] = Out("X16", X, M, ld16, N)
        if Xl:
            outs["X16_lo"] = Out("X16_lo", Xl, M, ld16, N)
        if c["c"]:
            Cg = Guarded(dev, (M * c["ldc"] + FC.TAIL,), torch.float32)
            g.C = Cg.ptr
            outs["C"] = Out("C", Cg, M, c["ldc"], N)
            bufs.append(Cg)
        part = Guarded(dev, (M * (N // w) * 2 + FC.TAIL,), torch.float32)
        g.row_part = part.ptr
        outs["row_part"] = Out("row_part", part, M, (N // w) * 2, (N // w) * 2)
        flag = Guarded(dev, (4,), torch.int32)
        assert (flag.t == FLAG_FILL).all().item()
        flag.t[1] = 1 if c["flag"] == "set" else 0
        g.range_flag = flag.ptr + 4 if c["flag"] != "null" else None
        bufs += [R, Rh, Rl, X, Xl, part, flag]
    else:
        part, lnc = _put(dev, a["ln_part"], torch.float32), _put(dev, a["ln_c"], torch.float32)
        g.ln_part, g.ln_c = part.ptr + 4 * c["part_off"], lnc.ptr + 4 * c["lnc_off"]
        g.ln_eps, g.ln_slots, g.out_f32 = FC.EPS, c["ln_slots"], 0
        Cg = Guarded(dev, (M * c["ldc"] + FC.TAIL,), tdt)
        g.C = Cg.ptr
        outs["C"] = Out("C", Cg, M, c["ldc"], c["n_store"])
        if c["c_lo"]:
            Cl = Guarded(dev, (M * c["ldc"] + FC.TAIL,), tdt)
            g.C_lo = Cl.ptr
            outs["C_lo"] = Out("C_lo", Cl, M, c["ldc"], c["n_store"])
            bufs.append(Cl)
        bufs += [part, lnc, Cg]
    bufs = [b for b in bufs if b is not None]
    assert all(b.ptr % 256 == 0 for b in bufs)
    for o in outs.values():       # (taken now: the in-place stream's "before" is the input image)
        o.before = _bits(o.g.t).cpu().clone()
    prev = lib.pio_gemm_kernel_override(c["override"])
    budget = lib.pio_set_cu_budget(c["n_cu"]) if c["n_cu"] != 256 else None
    try:
        rc = lib.pio_gemm_nt(C.byref(g), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        lib.pio_gemm_kernel_override(prev)
        if budget is not None:
            lib.pio_set_cu_budget(budget)
    return rc, outs, flag, bufs


def _check_flag(what, c, flag, want):
    f = flag.t.cpu()
    assert f[0].item() == FLAG_FILL and f[2].item() == FLAG_FILL and f[3].item() == FLAG_FILL, \
        f"{what} range_flag: a word beside the flag was written: {f.tolist()}"
    assert f[1].item() == want, f"{what} range_flag: {f[1].item()}, expected {want}"


@pytest.mark.parametrize("case", FC.CASES, ids=[c["id"] for c in FC.CASES])
def test_gemm_fold(dev, case):
    dev, times = dev
    c = case
    for dt in FC.DTYPES:
        what = f"fold {c['id']} [{c['kernel']}] {dt}"
        t0 = time.perf_counter()
        a = FC.make_arrays(c, dt)
        with np.errstate(over="ignore"):
            assert FC.exact_ok(c, a, dt), what
        rc, outs, flag, bufs = _launch(dev, c, dt, a)
        assert rc == 0, f"{what}: return code {rc}"
        for b in bufs:
            b.check(what)
        for o in outs.values():
            o.check_untouched(what)
        if c["role"] == "prod":
            skip = c["plant"][1] if c["plant"] else None
            with np.errstate(all="ignore"):
                hi, lo, x32, sums = FC.expected_producer(c, a, dt)
            outs["X16"].check_bits(what, hi, skip)
            if "X16_lo" in outs:
                outs["X16_lo"].check_bits(what, lo, skip)
            if "C" in outs:
                outs["C"].check_bits(what, x32, skip)
            S = c["N"] // c["slot_w"]
            if c["family"] == "pair":
                outs["row_part"].check_bound(what, sums.reshape(c["M"], 2 * S), FC.sum_bound(c, a).reshape(c["M"], 2 * S),
                                             pos=("m", "2 * slot + {0: sum, 1: squares}"))
            else:
                s32 = sums.astype(np.float32)
                assert skip is not None or np.array_equal(s32.astype(np.float64), sums)
                outs["row_part"].check_bits(what, s32.reshape(c["M"], 2 * S), skip, pos=("m", "2 * slot + {0: sum, 1: squares}"))
            if c["flag"] == "null":
                _check_flag(what, c, flag, 0)                       # (never handed to the call: every word intact)
            else:
                _check_flag(what, c, flag, 1 if (c["plant"] or c["flag"] == "set") else 0)
        else:
            y = FC.ref_consumer(c, a)[0]
            if c["family"] == "exact":
                hi, lo = FC.expected_consumer(c, y, dt)
                outs["C"].check_bits(what, hi)
                if lo is not None:
                    outs["C_lo"].check_bits(what, lo)
            else:
                assert not c["c_lo"]
                bound = FC.cons_bound(c, a, dt) if c["family"] == "bounded" else FC.gelu_bound(c, y, dt)
                outs["C"].check_bound(what, y, bound)
                flat, bits = outs["C"].after()
                pad = outs["C"].grid(bits)[:, c["N"]:]
                assert not pad.any().item(), f"{what} C: the pad columns [N, n_store) must be +0"
        times[what] = time.perf_counter() - t0
        print(f"{what}: {c['family']}, {times[what]:.2f} s")


@pytest.mark.parametrize("case", FC.REFUSED, ids=[c["id"] for c in FC.REFUSED])
def test_gemm_fold_refusals_write_nothing(dev, case):
    dev, _ = dev
    assert not case.get("missing_base"), f"{case['id']}: its base case {case['base']} is gone from CASES"
    for dt in FC.DTYPES:
        what = f"fold {case['id']} {dt}"
        rc, outs, flag, bufs = _launch(dev, case, dt, FC.make_arrays(case, dt))
        assert rc == CODES[case["expect"]], f"{what}: return code {rc}, expected {case['expect']}"
        for b in bufs:
            b.check(what)
        for o in outs.values():
            o.check_untouched(what, all_of_it=True)
        if flag is not None:
            _check_flag(what, case, flag, 1 if case["flag"] == "set" else 0)
