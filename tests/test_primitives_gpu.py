"""GPU: the memory-bound primitives of csrc/pio_elementwise.hip through the raw C-ABI, one case per launcher branch
(tests/primitive_cases.py), against float64 references -- and the workspace contract of the block entry points.

Every output lives in a guarded buffer (guard | payload | guard in ONE allocation, the guards hold a fixed pattern and
must come back bit-intact), every output payload and every piece of input memory the contract calls unread is NaN
before the call.  Tolerance: one rounding to the output type, |got - ref| <= ulp |ref| + tiny with ulp = 2^-10 (fp16) /
2^-8 (bf16), i.e. twice the half-ulp, and tiny the type's smallest subnormal; masked entries, wiped rows and pad
columns are compared for exact zero."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import primitive_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
PIO_E_SHAPE, PIO_E_WORKSPACE = -1, -4

# hi + lo of LayerNorm against the reference's abs-max.  fp16: the project's figure (test_parity_gpu.test_layernorm_cast).  A bf16
# pair cannot meet it: lo is the residual (<= 2^-9 |v|) rounded to 8 bits, half an ulp of it is 2^-18 |v| = 3.8e-6 |v|;
# the bound is twice that, as for the single rounding above.
LN_PAIR_TOL = {"f16": 2e-6, "bf16": 2.0 ** -17}
# P + P_lo of softmax against the row's largest probability: largest |P + P_lo - ref| / rowmax(ref) measured over the
# cases below on an MI355X; the test asserts four times it (the fast exponential's error depends on the argument).
#   bf16: 7.33e-6 (tk2048).
#   fp16: 4.19e-5 (tk4100), above 1e-5: a FINDING, not a bound.  It is the fp16 range, not the arithmetic: in a row of
#         thousands of comparable keys P_lo = round(p - P) lies below fp16's smallest normal 6.1e-5, where values are
#         2^-24 apart; that absolute step against a row maximum of 7e-4 is the 4e-5.  Rows where P_lo is a normal number
#         (tk8, tk13) measure 2.1e-7.  fp16 asserts the format's step plus four times the short-row figure:
#         |P + P_lo - ref| <= 2^-24 + 4 * 2.1e-7 * rowmax(ref).
SM_PAIR_MEASURED = {"f16": 2.1e-7, "bf16": 7.33e-6}
SM_PAIR_ABS = {"f16": 2.0 ** -24, "bf16": 0.0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dt(dt):
    from perceiverio_pytorch_amd import _lib as L
    return L.PIO_DT_F16 if dt == "f16" else L.PIO_DT_BF16


class Guarded:
    """guard | payload | guard in one device allocation.  `t` is the payload viewed as `dtype` / `shape`, filled with
    NaN (float types) or 0xA5 bytes; check() asserts both guards are bit-intact."""

    def __init__(self, dev, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.n = n
        self.pattern = ((torch.arange(GUARD, dtype=torch.int64) * 37 + 11) % 251).to(torch.uint8).to(dev)
        self.buf = torch.empty(GUARD + n + GUARD, dtype=torch.uint8, device=dev)
        self.buf[:GUARD] = self.pattern
        self.buf[GUARD + n:] = self.pattern
        self.bytes = self.buf[GUARD:GUARD + n]
        self.t = self.bytes.view(dtype).view(shape)
        if dtype.is_floating_point:
            self.t.fill_(float("nan"))
        else:
            self.bytes.fill_(0xA5)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        torch.cuda.synchronize()
        assert torch.equal(self.buf[:GUARD], self.pattern), f"{what}: bytes in FRONT of the buffer were written"
        assert torch.equal(self.buf[GUARD + self.n:], self.pattern), f"{what}: bytes BEHIND the buffer were written"


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def assert_rounded(got, ref, dt, what):
    err = np.abs(got - ref)
    bound = PC.ULP[dt] * np.abs(ref) + PC.TINY[dt]
    worst = float((err / bound).max())
    print(f"{what}: worst |got - ref| / (ulp |ref| + tiny) = {worst:.3f}")
    if worst > 1.0:
        i = np.unravel_index(np.argmax(err / bound), err.shape)
        raise AssertionError(f"{what}: element {i}: got {got[i]!r} ref {ref[i]!r} err {err[i]:.3e} bound {bound[i]:.3e}")


# ====================================================================================================
# pio_softmax_rows
# ====================================================================================================
def _run_softmax(dev, case, d, dt, with_lo):
    """One call on guarded, NaN-filled outputs and a NaN-pitched S; returns (P, P_lo or None) as device tensors."""
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    B, H, Tq, Tk = PC.SM_B, PC.SM_H, PC.SM_TQ, case["Tk"]
    lds, ldp, off = case["lds"], case["ldp"], case["s_off"]
    rows = B * H * Tq
    sbuf = torch.full((off + rows * lds + 4,), float("nan"), dtype=torch.float32, device=dev)
    sview = sbuf[off:off + rows * lds].view(rows, lds)
    sview[:, :Tk] = torch.from_numpy(d["S"]).to(dev).view(rows, Tk)
    keep = [sbuf]

    def dptr(a):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t.data_ptr()

    P = Guarded(dev, (rows, ldp), TDT[dt])
    Pl = Guarded(dev, (rows, ldp), TDT[dt]) if with_lo else None
    what = f"softmax {case['id']} {dt}"
    L.check(lib.pio_softmax_rows(sbuf.data_ptr() + 4 * off, lds, P.ptr, Pl.ptr if Pl else None, ldp, B, H, Tq, Tk,
                                 d["scale"], dptr(d["kv_mask"]), dptr(d["q_mask"]), dptr(d["full_mask"]), dptr(d["bias"]),
                                 _dt(dt), _stream()), what)
    P.check(what + " P")
    if Pl:
        Pl.check(what + " P_lo")
    return P.t, (Pl.t if Pl else None)


_sm_pair_seen = {"f16": 0.0, "bf16": 0.0}


@pytest.mark.parametrize("form", PC.SM_FORMS)
@pytest.mark.parametrize("case", PC.SOFTMAX_CASES, ids=[c["id"] for c in PC.SOFTMAX_CASES])
def test_softmax_rows_branch(dev, case, form):
    """One case per kernel of softmax_rows_launch, PLAIN and with every optional pointer set; the P + P_lo figures
    measured on an MI355X are beside SM_PAIR_MEASURED."""
    B, H, Tq, Tk, ldp = PC.SM_B, PC.SM_H, PC.SM_TQ, case["Tk"], case["ldp"]
    d = PC.sm_inputs(case, form)
    ref = PC.ref_softmax_rows(d["S"], d["scale"], d["kv_mask"], d["q_mask"], d["full_mask"], d["bias"])
    ok = np.broadcast_to(PC.softmax_valid(ref.shape, d["kv_mask"], d["q_mask"], d["full_mask"]), ref.shape)
    for dt in PC.DTYPES:
        what = f"softmax {case['id']} {form} {dt} [{case['branch']}]"
        P, Pl = _run_softmax(dev, case, d, dt, with_lo=(form == "full"))
        got = _np(P).reshape(B, H, Tq, ldp)
        assert np.isfinite(got).all(), what
        assert (got[..., Tk:] == 0).all(), f"{what}: pad columns must be exact zeros"
        got = got[..., :Tk]
        assert (got[~ok] == 0).all(), f"{what}: masked entries must be exact zeros"
        assert_rounded(got, ref, dt, what)
        if form == "full":
            assert (got[1] == 0).all() and (got[0, :, PC.SM_ROW_QMASKED] == 0).all()
            assert (got[0, :, PC.SM_ROW_FULL_EMPTY] == 0).all()
            assert (got[0, :, PC.SM_ROW_ONE_KEY, Tk - 1] == 1).all(), f"{what}: a single attendable key has probability 1"
            lo = _np(Pl).reshape(B, H, Tq, ldp)
            assert np.isfinite(lo).all() and (lo[..., Tk:] == 0).all() and (lo[..., :Tk][~ok] == 0).all(), what
            rowmax = ref.max(axis=-1, keepdims=True)
            err = np.abs(got + lo[..., :Tk] - ref)
            fig = float(np.where(rowmax > 0, err / np.where(rowmax > 0, rowmax, 1.0), 0.0).max())
            _sm_pair_seen[dt] = max(_sm_pair_seen[dt], fig)
            print(f"{what}: |P + P_lo - ref| / rowmax = {fig:.3e} (largest so far for {dt}: {_sm_pair_seen[dt]:.3e})")
            assert (err <= SM_PAIR_ABS[dt] + 4 * SM_PAIR_MEASURED[dt] * rowmax).all(), f"{what}: P + P_lo {fig:.3e}"


@pytest.mark.parametrize("dt", PC.DTYPES)
@pytest.mark.parametrize("name", PC.SM_MASK_BYTE_CASES)
def test_softmax_rows_mask_bytes(dev, name, dt):
    """A mask byte is true iff non-zero: the same pattern written with 1, 2, 0x80 and 0xFF gives the same bits."""
    case = next(c for c in PC.SOFTMAX_CASES if c["id"] == name)
    d = PC.sm_inputs(case, "full")
    P0, L0 = _run_softmax(dev, case, d, dt, True)
    P0, L0 = _bits(P0), _bits(L0)
    assert (P0 != 0).any()
    bad = []
    for which in ("kv_mask", "q_mask", "full_mask"):
        for v in PC.MASK_TRUE_BYTES:
            e = dict(d)
            e[which] = (d[which].astype(np.uint32) * v).astype(np.uint8)
            P1, L1 = _run_softmax(dev, case, e, dt, True)
            if not (torch.equal(_bits(P1), P0) and torch.equal(_bits(L1), L0)):
                bad.append(f"{which}=0x{v:02X}")
    print(f"softmax mask bytes {name} {dt} [{case['branch']}]: differing from the 0/1 run: {bad or 'none'}")
    assert not bad, f"{name} {dt}: results differ from the 0 / 1 masks for {bad}"


# ====================================================================================================
# pio_layernorm_cast
# ====================================================================================================
def _place_x(dev, x, sb, st, nsamp, x_off):
    """x [nsamp, T, C] placed with element strides (sb, st) at `x_off` floats into a NaN-filled buffer."""
    _, T, Cc = x.shape
    sbm = sb if nsamp > 1 else T * st
    buf = torch.full((x_off + nsamp * max(sbm, T * st) + 16,), float("nan"), dtype=torch.float32, device=dev)
    torch.as_strided(buf, (nsamp, T, Cc), (sbm, st, 1), x_off).copy_(torch.from_numpy(x[:nsamp]).to(dev))
    return buf


def _check_ln(got, lo, ref, C_, dt, what):
    assert np.isfinite(got).all(), what
    assert (got[..., C_:] == 0).all(), f"{what}: pad columns must be exact zeros"
    assert_rounded(got[..., :C_], ref[..., :C_], dt, what)
    if lo is not None:
        assert np.isfinite(lo).all() and (lo[..., C_:] == 0).all(), what
        err, absmax = np.abs(got + lo - ref).max(), np.abs(ref).max()      # (as test_parity_gpu.test_layernorm_cast)
        assert err <= LN_PAIR_TOL[dt] * absmax, f"{what}: hi + lo {err / absmax:.3e}"


@pytest.mark.parametrize("layout", PC.LN_LAYOUTS)
@pytest.mark.parametrize("case", PC.LAYERNORM_CASES, ids=[c["id"] for c in PC.LAYERNORM_CASES])
def test_layernorm_cast_branch(dev, case, layout):
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    B, T, C_, cp = PC.LN_B, PC.LN_T, case["C"], case["c_pad"]
    x, gamma, beta = PC.ln_inputs(case)
    sb, st, nsamp = PC.ln_strides(case, layout)
    xe = x if nsamp == B else np.broadcast_to(x[0:1], x.shape)
    buf = _place_x(dev, x, sb, st, nsamp, case["x_off"])
    gd, bd = torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev)
    ln = L.LayerNorm(gd.data_ptr(), bd.data_ptr(), C_, PC.LN_EPS)
    t3 = L.Tensor3(buf.data_ptr() + 4 * case["x_off"], sb, st, B, T, C_)
    refs = {True: PC.ref_layernorm_cast(xe, gamma, beta, PC.LN_EPS, cp), False: PC.ref_layernorm_cast(xe, None, None, 0.0, cp)}
    for norm in (True, False):
        for dt in PC.DTYPES:
            for with_lo in (True, False):
                what = f"layernorm {case['id']} {layout} ln={int(norm)} {dt} lo={int(with_lo)} [{case['branch']}]"
                y = Guarded(dev, (B * T, cp), TDT[dt])
                yl = Guarded(dev, (B * T, cp), TDT[dt]) if with_lo else None
                L.check(lib.pio_layernorm_cast(C.byref(t3), C.byref(ln) if norm else None, y.ptr, yl.ptr if yl else None,
                                               cp, _dt(dt), _stream()), what)
                y.check(what + " y")
                if yl:
                    yl.check(what + " y_lo")
                got = _np(y.t).reshape(B, T, cp)
                _check_ln(got, _np(yl.t).reshape(B, T, cp) if yl else None, refs[norm], C_, dt, what)
                if norm:        # a constant row and an all-zero row come out as beta
                    for r in (PC.LN_ROW_CONST, PC.LN_ROW_ZERO):
                        assert_rounded(got[0, r, :C_], beta.astype(np.float64), dt, what + f" row {r} == beta")


# ====================================================================================================
# pio_layernorm_cast_cat
# ====================================================================================================
@pytest.mark.parametrize("case", PC.LNCAT_CASES, ids=[c["id"] for c in PC.LNCAT_CASES])
def test_layernorm_cast_cat(dev, case):
    """Bit-identical to pio_layernorm_cast of the materialised concatenation on the float2 kernel whose arithmetic the
    cat kernel restates (the concatenation is placed 8-byte but not 16-byte aligned, so that rows whose width is a
    multiple of 4 take that kernel too), and within one rounding of the float64 reference."""
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    B, T, C1, C2 = PC.LN_B, PC.LN_T, case["C1"], case["C2"]
    C_ = C1 + C2
    cp = PC.pad8(C_)
    x, gamma, beta = PC.ln_inputs(dict(C=C_))
    if case["table"]:
        x[:, :, C1:] = x[0:1, :, C1:]
    st1 = C1 + case["x1_gap"]
    b1 = _place_x(dev, np.ascontiguousarray(x[:, :, :C1]), T * st1, st1, B, 0)
    n2 = 1 if case["table"] else B
    x2 = torch.from_numpy(np.ascontiguousarray(x[:n2, :, C1:])).to(dev)
    cat = _place_x(dev, x, T * C_, C_, B, 2)
    gd, bd = torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev)
    ln = L.LayerNorm(gd.data_ptr(), bd.data_ptr(), C_, PC.LN_EPS)
    t1 = L.Tensor3(b1.data_ptr(), T * st1, st1, B, T, C1)
    t2 = L.Tensor3(x2.data_ptr(), T * C2, C2, n2, T, C2)
    tc = L.Tensor3(cat.data_ptr() + 8, T * C_, C_, B, T, C_)
    ref = PC.ref_layernorm_cast(x, gamma, beta, PC.LN_EPS, cp)
    for dt in PC.DTYPES:
        what = f"layernorm_cat {case['id']} {dt}"
        ya, la = Guarded(dev, (B * T, cp), TDT[dt]), Guarded(dev, (B * T, cp), TDT[dt])
        yb, lb = Guarded(dev, (B * T, cp), TDT[dt]), Guarded(dev, (B * T, cp), TDT[dt])
        L.check(lib.pio_layernorm_cast_cat(C.byref(t1), C.byref(t2), C.byref(ln), ya.ptr, la.ptr, cp, _dt(dt), _stream()), what)
        L.check(lib.pio_layernorm_cast(C.byref(tc), C.byref(ln), yb.ptr, lb.ptr, cp, _dt(dt), _stream()), what + " plain")
        for g in (ya, la, yb, lb):
            g.check(what)
        assert torch.equal(_bits(ya.t), _bits(yb.t)) and torch.equal(_bits(la.t), _bits(lb.t)), \
            f"{what}: differs from pio_layernorm_cast of the concatenation"
        _check_ln(_np(ya.t).reshape(B, T, cp), _np(la.t).reshape(B, T, cp), ref, C_, dt, what)
        yc = Guarded(dev, (B * T, cp), TDT[dt])                      # without y_lo
        L.check(lib.pio_layernorm_cast_cat(C.byref(t1), C.byref(t2), C.byref(ln), yc.ptr, None, cp, _dt(dt), _stream()), what)
        yc.check(what)
        assert torch.equal(_bits(yc.t), _bits(ya.t))


@pytest.mark.parametrize("case", PC.LNCAT_REFUSED, ids=[c["id"] for c in PC.LNCAT_REFUSED])
def test_layernorm_cast_cat_refuses(dev, case):
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    B, T, C1, C2, cp = PC.LN_B, PC.LN_T, case["C1"], case["C2"], case["c_pad"]
    x1 = torch.zeros(B, T, C1 + 1, device=dev)[:, :, :C1]
    x2 = torch.zeros(1, T, C2 + 1, device=dev)[:, :, :C2]
    g = torch.ones(C1 + C2, device=dev)
    ln = L.LayerNorm(g.data_ptr(), g.data_ptr(), C1 + C2, PC.LN_EPS)
    t1 = L.Tensor3(x1.data_ptr(), T * (C1 + 1), C1 + 1, B, T, C1)
    t2 = L.Tensor3(x2.data_ptr(), T * (C2 + 1), C2 + 1, 1, T, C2)
    y = Guarded(dev, (B * T, cp), torch.float16)
    rc = lib.pio_layernorm_cast_cat(C.byref(t1), C.byref(t2), C.byref(ln), y.ptr, None, cp, _dt("f16"), _stream())
    assert rc == PIO_E_SHAPE, rc
    y.check(case["id"])
    assert torch.isnan(y.t).all(), "a refused call must not write"


# ====================================================================================================
# pio_pack_linear
# ====================================================================================================
@pytest.mark.parametrize("dt", PC.DTYPES)
@pytest.mark.parametrize("case", PC.PACK_CASES, ids=["x".join(map(str, c)) for c in PC.PACK_CASES])
def test_pack_linear(dev, case, dt):
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    out, inn, rh, ch = case
    rows_p, cols_used, k_pad, ldw, rows_total = PC.pack_geometry(case)
    w, bias = PC.pack_inputs(case)
    wd = torch.full((out, ldw), float("nan"), dtype=torch.float32, device=dev)
    wd[:, :inn] = torch.from_numpy(w).to(dev)
    bd = torch.from_numpy(bias).to(dev)
    for with_bias in (True, False):
        img, bimg, written = PC.ref_pack_linear(w, bias if with_bias else None, rh, ch, k_pad, PC.PACK_ROW0, rows_total)
        img32 = np.where(written[:, None], img, 0.0).astype(np.float32)       # (exact: the values are fp32 weights)
        hi_ref = PC.round_to(dt, img32)
        lo_ref = PC.round_to(dt, img32 - hi_ref)
        for with_lo in (True, False):
            what = f"pack {case} {dt} bias={int(with_bias)} lo={int(with_lo)}"
            hi = Guarded(dev, (rows_total, k_pad), TDT[dt])
            lo = Guarded(dev, (rows_total, k_pad), TDT[dt]) if with_lo else None
            db = Guarded(dev, (rows_total,), torch.float32)
            L.check(lib.pio_pack_linear(wd.data_ptr(), bd.data_ptr() if with_bias else None, out, inn, ldw, rh, ch, hi.ptr,
                                        lo.ptr if lo else None, db.ptr, PC.PACK_ROW0, k_pad, _dt(dt), _stream()), what)
            for g in (hi, lo, db):
                if g is not None:
                    g.check(what)
            for g, want, nm in ((hi, hi_ref, "hi"), (lo, lo_ref, "lo")):
                if g is None:
                    continue
                got = g.t.float().cpu().numpy()
                assert np.isnan(got[~written]).all(), f"{what}: {nm} rows outside the packed part were written"
                assert np.array_equal(got[written], want[written]), f"{what}: {nm} is not the correctly rounded image"
            gb = db.t.cpu().numpy()
            assert np.isnan(gb[~written]).all(), f"{what}: bias rows outside the packed part were written"
            assert np.array_equal(gb[written].astype(np.float64), bimg[written]), f"{what}: bias"


# ====================================================================================================
# pio_bn_relu_maxpool_tokens
# ====================================================================================================
@pytest.mark.parametrize("hw", PC.POOL_HW, ids=[f"{h}x{w}" for h, w in PC.POOL_HW])
@pytest.mark.parametrize("C_", PC.POOL_C)
def test_bn_relu_maxpool_tokens(dev, C_, hw):
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    H, W = hw
    OH, OW = (H + 1) // 2, (W + 1) // 2
    x, scale, shift = PC.pool_inputs(C_, H, W)
    xd, sd, hd = (torch.from_numpy(a).to(dev) for a in (x, scale, shift))
    for pt, pl in PC.POOL_PADS:
        what = f"maxpool C={C_} {H}x{W} pad=({pt},{pl})"
        y = Guarded(dev, (PC.POOL_B, OH * OW, C_), torch.float32)
        L.check(lib.pio_bn_relu_maxpool_tokens(xd.data_ptr(), sd.data_ptr(), hd.data_ptr(), y.ptr, PC.POOL_B, C_, H, W, pt, pl,
                                               _stream()), what)
        y.check(what)
        got = y.t.cpu().numpy().astype(np.float64)
        ref, mag = PC.ref_bn_relu_maxpool_tokens(x, scale, shift, pt, pl)
        assert np.isfinite(got).all(), what
        assert (np.abs(got - ref) <= 2.0 ** -22 * mag).all(), f"{what}: {np.abs(got - ref).max():.3e}"
        assert (got[1, 0] == 0).all(), f"{what}: a window of negative values must be exactly 0"


# ====================================================================================================
# workspace contract of the block entry points: exactly the promised bytes, cut from the middle of a guarded buffer
# ====================================================================================================
def _workspace_contract(dev, what, need, out_shape, call):
    """call(out_ptr, ws_ptr, ws_bytes) -> return code.  Runs it with exactly `need` bytes between two guards, with a roomy
    workspace (bit-identical result) and one byte short (PIO_E_WORKSPACE, nothing written)."""
    assert need > 0, what
    ws = Guarded(dev, (need,), torch.uint8)
    ws.bytes.zero_()
    out = Guarded(dev, out_shape, torch.float32)
    assert ws.ptr % 256 == 0
    assert call(out.ptr, ws.ptr, need) == 0, what
    ws.check(what + " workspace")
    out.check(what + " out")
    assert torch.isfinite(out.t).all(), what
    roomy = torch.zeros(2 * need + (1 << 16), dtype=torch.uint8, device=dev)
    out2 = Guarded(dev, out_shape, torch.float32)
    assert call(out2.ptr, roomy.data_ptr(), roomy.numel()) == 0, what
    out2.check(what + " out (roomy workspace)")
    assert torch.equal(out.t, out2.t), f"{what}: result depends on the size of the workspace"
    out3 = Guarded(dev, out_shape, torch.float32)
    assert call(out3.ptr, ws.ptr, need - 1) == PIO_E_WORKSPACE, what
    out3.check(what)
    assert torch.isnan(out3.t).all(), f"{what}: a refused call must not write"


@pytest.fixture
def fp16_policy():
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import runtime as R
    prev = R.get_precision_policy()
    P.set_precision_policy("fp16")
    yield
    P.set_precision_policy(prev)


def _randn(dev, *shape, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).to(dev)


def test_workspace_mlp(dev, fp16_policy):
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import MLP
    lib = L.lib()
    torch.manual_seed(1)
    m = MLP(64, widening_factor=4).to(dev).eval()
    d = m._desc()
    x = _randn(dev, 2, 37, 64)
    need = lib.pio_mlp_workspace_bytes(d, 2 * 37)
    _workspace_contract(dev, "pio_mlp_fwd", need, (2, 37, 64),
                        lambda o, w, n: lib.pio_mlp_fwd(d, R.tensor3(x), o, w, n, _stream()))


def test_workspace_self_attention(dev, fp16_policy):
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import SelfAttention
    lib = L.lib()
    torch.manual_seed(2)
    m = SelfAttention(64, widening_factor=1, num_heads=2).to(dev).eval()
    d = m._desc()
    x = _randn(dev, 2, 128, 64)
    need = lib.pio_self_attention_workspace_bytes(d, 2, 128)
    _workspace_contract(dev, "pio_self_attention_fwd", need, (2, 128, 64),
                        lambda o, w, n: lib.pio_self_attention_fwd(d, R.tensor3(x), None, None, None, None, o, None, None, w,
                                                                   n, _stream()))


def test_workspace_cross_attention(dev, fp16_policy):
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import CrossAttention
    lib = L.lib()
    torch.manual_seed(3)
    m = CrossAttention(q_in_channels=64, kv_in_channels=64, num_heads=2).to(dev).eval()
    d = m._desc()
    xq, xkv = _randn(dev, 2, 16, 64, seed=1), _randn(dev, 2, 96, 64, seed=2)
    need = lib.pio_cross_attention_workspace_bytes(d, 2, 16, 96)
    _workspace_contract(dev, "pio_cross_attention_fwd", need, (2, 16, 64),
                        lambda o, w, n: lib.pio_cross_attention_fwd(d, R.tensor3(xq), R.tensor3(xkv), None, None, None, None,
                                                                    o, None, w, n, _stream()))


def test_workspace_decoder(dev, fp16_policy):
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.perceiver import PerceiverDecoder
    lib = L.lib()
    torch.manual_seed(4)
    m = PerceiverDecoder(64, 10, num_latent_channels=64, num_heads=1).to(dev).eval()
    cross, fin = m.decoding_cross_attn._desc(), m._final_desc()
    q, z = _randn(dev, 2, 16, 64, seed=3), _randn(dev, 2, 32, 64, seed=4)
    need = lib.pio_decoder_workspace_bytes(cross, C.byref(fin.desc), 2, 16, 32)
    rec = L.DecoderCall(C.pointer(cross), C.pointer(fin.desc), 10, C.pointer(R.tensor3(q)), None, C.pointer(R.tensor3(z)))

    def call(o, w, n):
        rec.out = o
        return lib.pio_decoder_fwd(C.byref(rec), w, n, _stream())

    _workspace_contract(dev, "pio_decoder_fwd", need, (2, 16, 10), call)


@pytest.mark.parametrize("case", PC.ATTN_WS_CASES, ids=[c[0] for c in PC.ATTN_WS_CASES])
def test_workspace_attention_routes(dev, fp16_policy, case):
    """pio_attention_fwd on each of its routes (launch counts of the profiler classes as tests/test_attn_route_gpu.py:
    5 = fused cores, 3 = softmax_rows); q, k and v are three arrays, the plain call the workspace query sizes."""
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    lib = L.lib()
    name, H, qk, vv, Tq, Tk, mask, want_fused, want_softmax = case
    B, cin = 2, 64
    torch.manual_seed(5)
    m = Attention(cin, cin, cin, num_heads=H, qk_out_channels=qk, v_out_channels=vv, output_channels=cin).to(dev).eval()
    d = m._desc()
    xq, xk, xv = _randn(dev, B, Tq, cin, seed=5), _randn(dev, B, Tk, cin, seed=6), _randn(dev, B, Tk, cin, seed=7)
    rng = np.random.default_rng(Tk)
    km = fm = None
    if mask == "kv":
        k = rng.random((B, Tk)) > 0.3
        k[:, 0] = True
        km = torch.from_numpy(k.astype(np.uint8)).to(dev)
    elif mask == "full":
        f = rng.random((B, Tq, Tk)) > 0.3
        f[:, :, 0] = True
        fm = torch.from_numpy(f.astype(np.uint8)).to(dev)

    def call(o, w, n):
        return lib.pio_attention_fwd(d, R.tensor3(xq), R.tensor3(xk), R.tensor3(xv), km.data_ptr() if km is not None else None,
                                     None, fm.data_ptr() if fm is not None else None, None, o, None, w, n, _stream())

    need = lib.pio_attention_workspace_bytes(d, B, Tq, Tk)
    _workspace_contract(dev, f"pio_attention_fwd {name}", need, (B, Tq, cin), call)
    roomy = torch.zeros(2 * need, dtype=torch.uint8, device=dev)
    out = torch.empty(B, Tq, cin, device=dev)
    L.check(lib.pio_prof_begin(64), "pio_prof_begin")
    try:
        assert call(out.data_ptr(), roomy.data_ptr(), roomy.numel()) == 0
    finally:
        launches = (C.c_int64 * 9)()
        assert lib.pio_prof_end(None, None, None, launches) >= 0
    torch.cuda.synchronize()
    assert launches[5] == want_fused, (name, list(launches))
    assert (launches[3] >= 1) if want_softmax is None else (launches[3] == want_softmax), (name, list(launches))
