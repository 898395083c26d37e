"""GPU: pio_rowstats_cast and pio_transpose16 (csrc/pio_elementwise.hip) through the raw C-ABI on the cases of
tests/row_pass_cases.py, both operand types where the kernel has one.

Every output is guard | payload | guard in one allocation (Guarded of tests/test_primitives_gpu.py), its payload NaN / POISON
before the call, with spare elements behind the part the contract writes that must keep their bits; every input holds NaN /
POISON where the contract says unread (pitch columns, rows behind the last).  Integer-valued, residual and non-finite probes
and the transpose are compared BIT FOR BIT; the sums of the other probes within SUM_BOUND, which row_pass_cases.py derives.
Refusals return their code and write nothing.  The chain test hands what pio_rowstats_cast wrote to consumer GEMMs of
tests/gemm_fold_cases.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_fold_cases as FC  # noqa: E402
import row_pass_cases as RC  # noqa: E402
from test_primitives_gpu import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
SPARE = 64      # elements behind the written part of every output payload: must keep their bits


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


def _lib():
    from perceiverio_pytorch_amd import _lib as L
    return L, L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dt(dt):
    return 0 if dt == "f16" else 1


def _bits16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _bits_of(a, dt):
    """float32 image of 16-bit values -> their bit patterns"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(TDT[dt]).view(torch.int16).numpy().view(np.uint16)


# ====================================================================================================
# pio_rowstats_cast
# ====================================================================================================
def _run_rowstats(dev, x, slot_w, dt, with_lo):
    """One call: x with a NaN row behind the last; outputs NaN-filled with SPARE elements behind.  Returns the numpy images
    (y bits [rows, C], y_lo bits or None, part float32 [rows, ns, 2]) after every guard and spare element was checked."""
    L, lib = _lib()
    rows, C_ = x.shape
    ns = C_ // slot_w
    xd = torch.full((rows + 1, C_), float("nan"), dtype=torch.float32, device=dev)
    xd[:rows] = torch.from_numpy(x).to(dev)
    y = Guarded(dev, (rows * C_ + SPARE,), TDT[dt])
    yl = Guarded(dev, (rows * C_ + SPARE,), TDT[dt]) if with_lo else None
    part = Guarded(dev, (rows * ns * 2 + SPARE,), torch.float32)
    what = f"rowstats C={C_} w={slot_w} rows={rows} {dt} lo={int(with_lo)}"
    rc = lib.pio_rowstats_cast(xd.data_ptr(), rows, C_, slot_w, y.ptr, yl.ptr if yl else None, part.ptr, _dt(dt), _stream())
    assert rc == 0, f"{what}: return code {rc}"
    for g in (y, yl, part):
        if g is not None:
            g.check(what)
            n = g.t.numel() - SPARE
            assert torch.isnan(g.t[n:]).all(), f"{what}: elements behind the last row were written"
    return (_bits16(y.t[:rows * C_]).reshape(rows, C_), _bits16(yl.t[:rows * C_]).reshape(rows, C_) if yl else None,
            part.t[:rows * ns * 2].cpu().numpy().reshape(rows, ns, 2), what)


def _assert_bits(got, want, what):
    bad = np.argwhere(got != want)
    assert not len(bad), f"{what}: {len(bad)} wrong elements, first at {tuple(bad[0])}: got 0x{got[tuple(bad[0])]:04X} " \
                         f"expected 0x{want[tuple(bad[0])]:04X}"


def _assert_part(got, part, bound, what, exact):
    if exact:
        want = part.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), part)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert not len(bad), f"{what} part: {len(bad)} wrong entries, first at (row, slot, sum|squares) = {tuple(bad[0])}: got " \
                             f"{got[tuple(bad[0])]!r} expected {want[tuple(bad[0])]!r}"
        return
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - part)
    inf = np.isinf(part)
    assert np.array_equal(got[inf].astype(np.float64), part[inf]), f"{what} part: a non-finite sum of squares must be +inf"
    ratio = np.where(inf, 0.0, err / np.maximum(bound, 1e-300))
    print(f"{what} part: worst |got - ref| / bound = sum {ratio[..., 0].max():.3f}, squares {ratio[..., 1].max():.3f}")
    bad = np.argwhere(~inf & ~(err <= bound))
    assert not len(bad), f"{what} part: {len(bad)} entries outside the bound, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} " \
                         f"reference {part[tuple(bad[0])]!r} bound {bound[tuple(bad[0])]:.3e}"


@pytest.mark.parametrize("shape", RC.RS_SHAPES, ids=["C{}_w{}_r{}".format(*s) for s in RC.RS_SHAPES])
def test_rowstats_cast_integer_probe(dev, shape):
    """Every (C, slot_w, rows), y_lo given and NULL, both types: y, y_lo == +0 and every (sum, sum of squares) bit for bit."""
    C_, w, rows = shape
    for dt in RC.DTYPES:
        x = RC.rs_input(C_, w, rows, "int", dt)
        y, lo, part, bound = RC.rs_reference(x, w, dt)
        for with_lo in (True, False):
            gy, glo, gpart, what = _run_rowstats(dev, x, w, dt, with_lo)
            _assert_bits(gy, _bits_of(y, dt), what + " y")
            if with_lo:
                assert not glo.any(), f"{what}: y_lo must be +0 for values of the type"
            _assert_part(gpart, part, bound, what, exact=True)


@pytest.mark.parametrize("probe", ["residual", "gauss", "big"])
@pytest.mark.parametrize("shape", RC.RS_SHAPES_FEW, ids=["C{}_w{}_r{}".format(*s) for s in RC.RS_SHAPES_FEW])
def test_rowstats_cast_probes(dev, shape, probe):
    C_, w, rows = shape
    for dt in RC.DTYPES:
        x = RC.rs_input(C_, w, rows, probe, dt)
        if probe == "residual":
            x, h, l = x
        y, lo, part, bound = RC.rs_reference(x, w, dt)
        gy, glo, gpart, what = _run_rowstats(dev, x, w, dt, True)
        what += " " + probe
        if probe == "residual":
            _assert_bits(gy, _bits_of(h, dt), what + " y == h")
            _assert_bits(glo, _bits_of(l, dt), what + " y_lo == l")
        _assert_bits(gy, _bits_of(y, dt), what + " y")
        _assert_bits(glo, _bits_of(lo, dt), what + " y_lo")
        if probe == "big":       # one slot: sum within the bound, squares +inf; every other slot as the int probe: exact
            r, c = RC.RS_BIG_AT
            s = c // w
            assert gpart[r, s, 1] == np.inf and abs(float(gpart[r, s, 0]) - part[r, s, 0]) <= bound[r, s, 0], what
            keep = np.ones(part.shape, bool)
            keep[r, s] = False
            xi = RC.rs_input(C_, w, rows, "int", dt)
            pi = RC.rs_reference(xi, w, dt)[2]
            assert np.array_equal(pi[keep], part[keep])
            assert np.array_equal(gpart[keep].astype(np.float64), pi[keep]) and np.isfinite(gpart[keep]).all(), \
                f"{what}: a slot beside the planted one changed"
            yi = _bits_of(RC.rs_reference(xi, w, dt)[0], dt)
            yi[r, c] = _bits_of(y, dt)[r, c]
            _assert_bits(gy, yi, what + " y beside the planted element")
        else:
            _assert_part(gpart, part, bound, what, exact=False)


def _device_bases(dev):
    bufs = {k: Guarded(dev, (4096,), torch.float32) for k in ("x", "y16", "y16_lo", "part", "vt")}
    bufs["x"].t.zero_()
    return bufs, {k: g.ptr for k, g in bufs.items()}


def _no_profiler_record(lib, calls):
    """Runs calls() under the per-launch profiler: a refused call must leave no record of a launch."""
    assert lib.pio_prof_begin(256) == 0
    try:
        calls()
    finally:
        n = lib.pio_prof_end(None, None, None, None)
    assert n == 0, f"{n} profiler records from refused calls"


def test_rowstats_cast_refusals_write_nothing(dev):
    L, lib = _lib()
    bufs, base = _device_bases(dev)
    assert all(p % 256 == 0 for p in base.values())

    def calls():
        for cid, code, change in RC.RS_REFUSED:
            x, rows, C_, w, y, yl, part, dtype = RC.rs_call_args(change, base)
            rc = lib.pio_rowstats_cast(x or None, rows, C_, w, y or None, yl or None, part or None, dtype, _stream())
            assert rc == code, f"{cid}: return code {rc}, expected {code}"

    _no_profiler_record(lib, calls)
    for k in ("y16", "y16_lo", "part"):
        bufs[k].check(f"rowstats refusals {k}")
        assert torch.isnan(bufs[k].t).all(), f"a refused call wrote {k}"


# ---- chain: the consumer GEMMs of the fold read what this kernel wrote -----------------------------------------------
CHAIN = ("t32_c_edges", "wc_k256")     # K = 256: 4 slots of 64 on a tile kernel (lda = K + 8, ln_part 8 bytes off) / 2 of 128 on gemm_nt_wide


@pytest.mark.parametrize("cid", CHAIN)
def test_rowstats_cast_feeds_a_fold_consumer(dev, cid):
    """y16 and part of pio_rowstats_cast (integer probe) as the A operand and ln_part of a consumer case of
    gemm_fold_cases.py whose K the kernel takes: the result equals, bit for bit, the same consumer fed the reference's
    row_part.  (y16_lo is +0 in this probe and the consumers take no A_lo.)"""
    from test_gemm_fold_gpu import _launch
    c = FC.BY_ID[cid]
    M, K, ns = c["M"], c["K"], c["ln_slots"]
    assert K % 256 == 0 and K % ns == 0 and K // ns in (64, 128) and not c["a_lo"]
    w = K // ns
    for dt in RC.DTYPES:
        x = RC.rs_input(K, w, 9, "int", dt)
        x = np.ascontiguousarray(np.resize(x, (M, K)))                       # the nine probe rows, repeated
        y, _, part, bound = RC.rs_reference(x, w, dt)
        gy, glo, gpart, what = _run_rowstats(dev, x, w, dt, True)
        assert not glo.any()
        a = FC.make_arrays(c, dt)
        got_y = torch.from_numpy(gy.view(np.int16)).view(TDT[dt]).float().numpy()
        results = []
        for name, A, P in (("kernel", got_y, gpart), ("reference", y, part.astype(np.float32))):
            b = dict(a)
            b["A"] = FC._matrix(M, c["lda"], K, A)
            b["ln_part"] = FC._vector(c["part_off"], M * ns * 2, P.reshape(-1))
            rc, outs, _, bufs = _launch(dev, c, dt, b)
            assert rc == 0, f"{what} -> {cid} ({name}): return code {rc}"
            for g in bufs:
                g.check(f"{what} -> {cid}")
            for o in outs.values():
                o.check_untouched(f"{what} -> {cid}")
            flat, bits = outs["C"].after()
            assert torch.isfinite(outs["C"].grid(flat).float()).all(), f"{what} -> {cid} ({name})"
            results.append({k: o.after()[1].clone() for k, o in outs.items()})
        for k in results[0]:
            assert torch.equal(results[0][k], results[1][k]), f"{what} -> {cid}: {k} differs from the consumer fed the reference"
        # ... and is the LayerNorm'd product: against float64 of the definition, within the bounded family's bound
        b["ln_part"] = FC._vector(c["part_off"], M * ns * 2, part.astype(np.float32).reshape(-1))
        S, Q, mean, wv, _ = FC.cons_stats(c, b)
        assert ((Q / K + mean * mean) / wv).max() <= 19.0, "the premise of cons_bound"
        outs["C"].check_bound(f"{what} -> {cid}", FC.ref_consumer(c, b)[0], FC.cons_bound(c, b, dt))


# ====================================================================================================
# pio_transpose16
# ====================================================================================================
def _u16(dev, a):
    return torch.from_numpy(a.view(np.int16)).to(dev)


@pytest.mark.parametrize("case", RC.TR_CASES, ids=[RC.tr_id(c) for c in RC.TR_CASES])
def test_transpose16(dev, case):
    L, lib = _lib()
    B, T, C_, ldx, tkv = RC.tr_shape(case)
    xd = _u16(dev, RC.tr_input(case))
    vt = Guarded(dev, (B * C_ * tkv + SPARE,), torch.int16)
    vt.t.fill_(int(np.array([RC.POISON], np.uint16).view(np.int16)[0]))
    what = f"transpose16 {RC.tr_id(case)}"
    rc = lib.pio_transpose16(xd.data_ptr(), ldx, B, T, C_, vt.ptr, tkv, _stream())
    assert rc == 0, f"{what}: return code {rc}"
    vt.check(what)
    got = vt.t.cpu().numpy().view(np.uint16)
    assert (got[B * C_ * tkv:] == RC.POISON).all(), f"{what}: elements behind B * C * tkv were written"
    got = got[:B * C_ * tkv].reshape(B, C_, tkv)
    assert not got[:, :, T:].any(), f"{what}: columns [T, tkv) must be +0"
    want = RC.tr_reference(case)
    bad = np.argwhere(got != want)
    assert not len(bad), f"{what}: {len(bad)} wrong elements, first at (b, c, t) = {tuple(bad[0])}: got 0x{got[tuple(bad[0])]:04X} " \
                         f"expected 0x{want[tuple(bad[0])]:04X}"


def test_transpose16_refusals_write_nothing(dev):
    L, lib = _lib()
    bufs, base = _device_bases(dev)

    def calls():
        for cid, code, change in RC.TR_REFUSED:
            x, ldx, B, T, C_, vt, tkv = RC.tr_call_args(change, base)
            rc = lib.pio_transpose16(x or None, ldx, B, T, C_, vt or None, tkv, _stream())
            assert rc == code, f"{cid}: return code {rc}, expected {code}"

    _no_profiler_record(lib, calls)
    bufs["vt"].check("transpose16 refusals")
    assert torch.isnan(bufs["vt"].t).all(), "a refused call wrote vt"
