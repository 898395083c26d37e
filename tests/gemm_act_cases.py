"""Cases, operands, the float64 reference, the bounds and the planted faults for the exact-erf GELU (act == 1) of
pio_gemm_nt (include/pio_hip.h) on every kernel that applies it: gelu_erf / gelu_erf2 of csrc/pio_gemm_common.h, called
from gemm_nt_wide (packed interior path, per-element edge path), gemm_nt_stream (ACT == 1), the row walk of gemm_nt_128
(T128 / T64 / T32 and their two-team forms) and epilogue_store4 (gemm_nt_256).  gemm_nt_skinny takes no activation.

Numpy only; shared by tests/test_gemm_act_host.py (CPU: routing through csrc/pio_gemm_route.h, coverage, the bounds
shown to hold for a float32 model of the epilogue and to FAIL for every planted fault) and tests/test_gemm_act_gpu.py.

PRE-ACTIVATIONS, exact by construction.  A[m, 0:2] = (a_m / alpha, 1), B[n, 0:2] = (1, b_n / alpha), every other column
zero: alpha * acc[m, n] = a_m + b_n in any summation order.  Rows repeat with period ROW_P = 88: 64 GRID rows, a_m the
multiples of 1/4 in [-8, 8), then 24 BAND rows; columns with period COL_P = 40: 16 grid columns, b_n the multiples of
2^-6 in [0, 1/4), then 24 band columns.  Grid rows x grid columns of one launch are every multiple of 2^-6 in [-8, 8):
1024 points, each exact in fp32, every operand exact in fp16 and bf16 (alpha in {1/2, 1, 2}).
The band rows of A and the band columns of B are ZERO THROUGHOUT (not only a_m = 0 / b_n = 0: A[m, 1] and B[n, 0]
too), so the accumulator is +0 there and the fp32 bias ALONE is the pre-activation -- in every row of a band column
(bias_mode 1) and every column of a band row (bias_mode 2), with no rounding.  (With A[m, 1] = 1 kept, a band row
under a per-row bias would see b_n + bias[m], which fp32 does not hold.)  The band carries SPECIALS:
nextafter(+-6, 0), +-6, nextafter(+-6, +-inf), +-4.2446 (the polynomial's worst point), +-1e-3, +-2^-126, +-2^-140,
+-0, +-20, +-1000, +-65504, +-3e38.  (acc = +0 and bias = -0 add to +0: a -0 pre-activation needs a negative alpha and
is not produced; f(0) == 0 is asserted for whatever sign arrives.)  A 16-bit fp16 result cannot hold what the
kernels make of +-3e38 (3e38 and -3e38 Phi(-6) = -2.96e29): where ref +- bound reaches past the largest finite value
of the output type the infinity of that side is accepted (nothing finite is within the bound of 3e38 in fp16, so +inf
is then the only value that passes; the sign checks still hold).
Non-finite pre-activations (NaN, +-inf in the band) have cases of their own ("nonfinite"), so that every other case
asserts finiteness.

CONTRACT (include/pio_hip.h): C = gelu(alpha acc + bias) + R.  The "order" cases use alpha = 1/2 (operands doubled), a
per-column bias of 0 / +2 / -2 on the grid columns and an fp32 residual of multiples of 16 in +-[16, 64].

REFERENCE: float64 0.5 x erfc(-x / sqrt 2) (math.erfc: no cancellation in the tail) of the exact pre-activation.
BOUND per element: G(x) + [residual: 2^-24 |ref|] + the rounding of the output form, where
    G(x) = 4 max(G6, GINF |x|)   G6   = largest |f32_gelu - ref| over |x| <= 6 of the case set's pre-activations
                                 GINF = largest |f32_gelu - ref| / |x| over |x| > 6 (there E is frozen at Phi(-6), so
                                        the negative tail is x Phi(-6) instead of -> 0)
    (f32_gelu: the numpy float32 restatement of gelu_erf in gemm_fold_cases; the factor 4 is that module's GELU_G
    convention: hardware exp2 good to about an ulp, FMA contraction);
    2^-24 |ref|: the one fp32 rounding of gelu + R (half an ulp), residual cases only;
    fp32 out: nothing more; 16-bit out: ULP[dt] |ref| + TINY[dt]; hi + lo pair: hi as 16-bit out, and hi + lo within
    ULP[dt]^2 / 2 |ref| + TINY[dt] (|lo| <= ULP/2 |ref|, rounded once more: ULP/2 |lo|; twice that).
EXACT, on every case without a residual: f(0) == 0; result <= 0 for x < 0, >= 0 for x > 0; |result| <= |x| (16-bit
out: <= rn(|x|), rounding is monotone); and on every case: pad columns [N, n_store) are +0, everything else in C /
C_lo outside rows < M x columns < n_store keeps its NaN fill.
NON-FINITE: NaN in -> NaN out; +-inf in -> a non-finite result (+inf in gives NaN: fma(-inf, E, +inf); not repaired,
the epilogues are bound by their instruction count).

MEASURED, CPU model f32_gelu over the case set's pre-activations: g6 = 2.551e-7 (at x = 4.2446), ginf = 1.048e-9
(committed as G6 = 2.6e-7, GINF = 1.05e-9).
MEASURED, MI355X (tests/test_gemm_act_gpu.py prints them; a record, not a bound): see DEVICE_RECORD below.
"""
import math
import os
import re

import numpy as np

from gemm_fold_cases import TINY, ULP, f32_gelu  # noqa: F401
from primitive_cases import DTYPES, round_to  # noqa: F401  (re-exported for the two test files)

KERNELS = ("WIDE", "STREAM", "T256", "T128", "T128_KG2", "T64", "T64_KG2", "T32", "T32_KG2")
TILE_N = {"WIDE": 256, "STREAM": 128, "T256": 256, "T128": 128, "T128_KG2": 128, "T64": 64, "T64_KG2": 64, "T32": 64,
          "T32_KG2": 64}
TILE_M = {"WIDE": 256, "STREAM": 256, "T256": 256, "T128": 128, "T128_KG2": 128, "T64": 64, "T64_KG2": 64, "T32": 32,
          "T32_KG2": 32}
F32_ACT = ("T256", "T128", "T128_KG2", "T64", "T64_KG2", "T32", "T32_KG2")   # fp32 out, bias_mode 2, residual with act
FORMS = ("out16", "pair", "f32")
N_CU = 256
TAIL = 8
U32 = 2.0 ** -24
MAXF = {"f16": 65504.0, "bf16": float(np.float32(2.0 ** 127 * (2 - 2.0 ** -7)))}   # largest finite value of the type

# the committed figures of the CPU model (tests/test_gemm_act_host.py measures them and holds them to these)
G6 = 2.6e-7
GINF = 1.05e-9

# Largest |got - ref| seen on an MI355X per (kernel, form), fp16 / bf16 operands, and where: a record, not a bound.
DEVICE_RECORD = """
The same figures on all nine kernels (WIDE, STREAM, T256, T128, T128_KG2, T64, T64_KG2, T32, T32_KG2), fp16 and bf16
operands alike where only one figure is given; (|x| <= 6: largest |got - ref| and its x; |x| > 6: largest |got - ref| / |x|):
  fp32 out              2.551e-7 at x = 4.2446;  1.048e-9 at x = -1000   -- the CPU model's own figures, digit for digit
  fp32 out + residual   3.954e-6 at x = 4.375 (the rounding of gelu + R, |R| <= 64);  7.849e-8 at x = 6
  hi + lo pair   fp16   7.319e-7 at x = 4.2446;  1.073e-9 at x = -1000
                 bf16   2.950e-5 at x = 4.078;   1.758e-6 at x = 3e38
  16-bit out     fp16   1.540e-3 at x = 4.2446;  7.849e-8 at x = 6
                 bf16   1.563e-2 at x = 5.359;   2.597e-3 at x = 6.016
Non-finite cases: NaN -> NaN and +-inf -> a non-finite value on every kernel.
"""

_f = np.float32
_six = _f(6.0)
SPECIALS = np.array(
    [np.nextafter(_six, _f(0)), _six, np.nextafter(_six, _f(np.inf)),
     -np.nextafter(_six, _f(0)), -_six, -np.nextafter(_six, _f(np.inf)),
     4.2446, -4.2446, 1e-3, -1e-3, 2.0 ** -126, -2.0 ** -126, 2.0 ** -140, -2.0 ** -140, 0.0, -0.0,
     20.0, -20.0, 1000.0, -1000.0, 65504.0, -65504.0, 3e38, -3e38], dtype=np.float32)
NONFINITE = np.array([np.nan, np.inf, -np.inf] * 8, dtype=np.float32)
GRID_ROWS, GRID_COLS, BAND = 64, 16, 24
ROW_P, COL_P = GRID_ROWS + BAND, GRID_COLS + BAND
assert len(SPECIALS) == BAND and len(NONFINITE) == BAND
GRID = np.arange(-512, 512) / 64.0          # the 1024 points


def _case(cid, kernel, override, M, N, K, form, **kw):
    c = dict(id=cid, kernel=kernel, override=override, M=M, N=N, K=K, form=form, out_f32=int(form == "f32"),
             c_lo=form == "pair", act=1, bias_mode=1, alpha=1.0, res=False, order=False, nonfinite=False, n_store=N,
             # the dense single-problem descriptor the route driver of tests/test_gemm_addr_host.py is given
             batch=1, nh=1, a_lo=False, b_lo=False, b_lo_n0=0, c_off=0, bias_off=0, r_off=0, r_rows=0, r_stride_b=0, ldr=0)
    c.update(kw)
    c.setdefault("lda", K + 8)
    c.setdefault("ldb", K + 8)
    c.setdefault("ldc", c["n_store"])
    c.update(sAh=M * c["lda"], sBh=N * c["ldb"], sCh=M * c["ldc"])
    c.update(sAb=c["sAh"], sBb=c["sBh"], sCb=c["sCh"])
    if c["res"]:
        c["ldr"] = N + 4
    assert M >= ROW_P and (N >= COL_P or cid.startswith("skinny")), cid
    return c


# (override, M, N, K): the smallest shape of tests/gemm_addr_cases.py that reaches the kernel, M >= 88 and N ragged
# against the kernel's tile; tests/test_gemm_act_host.py re-checks every route with act = 1
SHAPES = {
    "T32": (0, 100, 72, 40), "T32_KG2": (0, 100, 136, 1024), "T64": (64, 150, 72, 72), "T64_KG2": (0, 830, 892, 1024),
    "T128": (128, 200, 136, 72), "T128_KG2": (0, 1660, 1916, 1024), "T256": (256, 300, 264, 40),
    # gemm_nt_wide: K >= 128; 2 x 2 tiles, (0, 0) interior (the packed gelu_erf2 path), the others ragged in M, N or both
    "WIDE": (2, 300, 264, 128),
    # gemm_nt_stream: 16 K steps of 64; 3 x 3 = 9 tiles on persistent_grid(9, 256) = 8 workgroups: one runs two tiles
    "STREAM": (1, 520, 264, 1024),
}


def _cases():
    out = []
    for k in KERNELS:
        ov, M, N, K = SHAPES[k]
        t = k.lower()
        persistent = k in ("WIDE", "STREAM")
        # 16-bit out on the vector store: pad columns and a pitch; alpha = 2 (operands halved)
        out.append(_case(f"{t}_16", k, ov, M, N, K, "out16", n_store=N + 8, ldc=N + 16, alpha=2.0))
        if persistent:
            out.append(_case(f"{t}_pair", k, ov, M, N, K, "pair", n_store=N + 8, ldc=N + 16))
        else:
            # hi + lo pair on the scalar store (odd pitch, one pad column), per-row bias
            out.append(_case(f"{t}_pair", k, ov, M, N, K, "pair", n_store=N + 1, ldc=N + 3, bias_mode=2))
            out.append(_case(f"{t}_f32", k, ov, M, N, K, "f32", ldc=N + 4))
            # (fp32 out: under a 16-bit result the rounding of gelu + R, |R| up to 64, would hide a wrong GELU variant)
            out.append(_case(f"{t}_order", k, ov, M, N, K, "f32", n_store=N + 4, ldc=N + 8, alpha=0.5, res=True,
                             order=True))
        out.append(_case(f"{t}_nonfinite", k, ov, M, N, K, "out16" if persistent else "f32", nonfinite=True))
    # a few columns over many rows: gemm_nt_skinny's shape, which act = 1 keeps away from it (-> the 32 x 64 tile)
    out.append(_case("skinny_shape", "T32", 0, 2051, 2, 72, "out16"))
    return out


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
FINITE = [c for c in CASES if not c["nonfinite"]]


def _variant(cid, base, expect, **change):
    c = dict(BY_ID[base])
    c.update(change)
    c.update(id=cid, expect=expect, base=base)
    if c["res"] and not c["ldr"]:
        c["ldr"] = c["N"] + 4
    return c


# act = 1 descriptors the persistent kernels do not take (gemm_wide_ok / gemm_stream_ok): under their override they
# run on the 128 x 128 tile, so no case above can silently measure another kernel than the one it names
REROUTED = [
    _variant("wide_res_act", "wide_pair", "T128", form="out16", c_lo=False, res=True),
    _variant("wide_pair_res_act", "wide_pair", "T128", res=True),
    _variant("wide_f32_act", "wide_16", "T128", form="f32", out_f32=1),
    _variant("stream_res_act", "stream_pair", "T128", form="out16", c_lo=False, res=True),
    _variant("stream_f32_act", "stream_16", "T128", form="f32", out_f32=1),
    _variant("wide_bias_rows_act", "wide_16", "T128", bias_mode=2),
    _variant("stream_bias_rows_act", "stream_16", "T128", bias_mode=2),
]
# the same shape with act = 0 IS the few-column kernel's (the host test shows it): only the activation moves it
SKINNY_PLAIN = _variant("skinny_shape_act0", "skinny_shape", "SKINNY2", act=0)


# ----------------------------------------------------------------------------------------------------
# operands
# ----------------------------------------------------------------------------------------------------
def row_values(c):
    """(a [M] float64, band index [M] int: -1 on grid rows)"""
    r = np.arange(c["M"]) % ROW_P
    grid = r < GRID_ROWS
    return np.where(grid, (r - 32) / 4.0, 0.0), np.where(grid, -1, r - GRID_ROWS)


def col_values(c):
    r = np.arange(c["N"]) % COL_P
    grid = r < GRID_COLS
    return np.where(grid, r / 64.0, 0.0), np.where(grid, -1, r - GRID_COLS)


def _matrix(rows, ld, cols, values):
    buf = np.full(rows * ld + TAIL, np.nan, dtype=np.float32)
    buf[:rows * ld].reshape(rows, ld)[:, :cols] = values
    return buf


def make_arrays(c):
    """Flat float32 payloads (values exact in fp16 and bf16; the bias and R are fp32 operands); pitch columns and the
    TAIL behind every payload are NaN."""
    M, N, K = c["M"], c["N"], c["K"]
    a, rband = row_values(c)
    b, cband = col_values(c)
    s = 1.0 / c["alpha"]
    A, B = np.zeros((M, K), np.float32), np.zeros((N, K), np.float32)
    A[:, 0], A[:, 1] = a * s, (rband < 0)
    B[:, 0], B[:, 1] = (cband < 0), b * s
    band = NONFINITE if c["nonfinite"] else SPECIALS
    if c["bias_mode"] == 1:
        bias = np.where(cband < 0, 0.0, band[np.maximum(cband, 0)]).astype(np.float32)
        if c["order"]:
            bias = np.where(cband < 0, np.array([0.0, 2.0, -2.0])[(np.arange(N) // COL_P) % 3], bias).astype(np.float32)
    else:
        bias = np.where(rband < 0, 0.0, band[np.maximum(rband, 0)]).astype(np.float32)
    out = dict(A=_matrix(M, c["lda"], K, A), B=_matrix(N, c["ldb"], K, B), A_lo=None, B_lo=None, R=None,
               bias=np.concatenate([bias, np.full(TAIL, np.nan, np.float32)]))
    if c["res"]:
        m, n = np.arange(M)[:, None], np.arange(N)[None, :]
        R = 16.0 * (1 + (3 * m + n) % 4) * np.where((m + 2 * n) % 3 == 0, -1.0, 1.0)
        out["R"] = _matrix(M, c["ldr"], N, R)
    return out


def _view(buf, rows, ld, cols):
    return buf[:rows * ld].reshape(rows, ld)[:, :cols]


def preact(c, arrays):
    """x [M, N] float64 = alpha A B^T + bias, from the payloads; exact (exact_ok)."""
    M, N, K = c["M"], c["N"], c["K"]
    A, B = _view(arrays["A"], M, c["lda"], K).astype(np.float64), _view(arrays["B"], N, c["ldb"], K).astype(np.float64)
    assert not A[:, 2:].any() and not B[:, 2:].any()
    x = c["alpha"] * (A[:, :2] @ B[:, :2].T)
    bias = arrays["bias"][:N if c["bias_mode"] == 1 else M].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return x + (bias[None, :] if c["bias_mode"] == 1 else bias[:, None])


def residual(c, arrays):
    return _view(arrays["R"], c["M"], c["ldr"], c["N"]).astype(np.float64) if c["res"] else None


def exact_ok(c, arrays):
    """every operand a value of fp16 and of bf16, every pre-activation a value of fp32, and every partial result on
    the way (alpha acc, acc + bias / alpha: gemm_nt_stream adds the bias to the accumulators) as well"""
    ok = True
    for k in ("A", "B"):
        v = arrays[k][np.isfinite(arrays[k])]
        ok = ok and all(np.array_equal(round_to(d, v), v) for d in DTYPES)
    x = preact(c, arrays)
    fin = np.isfinite(x)
    ok = ok and np.array_equal(x[fin].astype(np.float32).astype(np.float64), x[fin])
    if c["kernel"] == "STREAM":
        b = arrays["bias"][np.isfinite(arrays["bias"])].astype(np.float64) / c["alpha"]
        ok = ok and np.abs(b).max() < 3.4e38 and np.array_equal(b.astype(np.float32).astype(np.float64), b)
    if c["res"]:
        r = residual(c, arrays)
        ok = ok and bool((np.abs(r) >= 16).all() and (np.abs(r) <= 64).all() and (r == np.rint(r)).all())
    return bool(ok)


# ----------------------------------------------------------------------------------------------------
# reference and bounds
# ----------------------------------------------------------------------------------------------------
def gelu64(x):
    """float64 0.5 x erfc(-x / sqrt 2); NaN where x is not finite (those elements have their own contract)"""
    vals, inv = np.unique(x, return_inverse=True)
    g = np.array([0.5 * v * math.erfc(-v / math.sqrt(2.0)) if math.isfinite(v) else math.nan for v in vals])
    return g[inv].reshape(x.shape)


def reference(c, arrays):
    """-> (x [M, N], ref [M, n_store]) float64; ref = gelu(x) + R, +0 in the pad columns"""
    x = preact(c, arrays)
    y = gelu64(x)
    if c["res"]:
        y = y + residual(c, arrays)
    ref = np.zeros((c["M"], c["n_store"]))
    ref[:, :c["N"]] = y + 0.0
    return x, ref


def G(x):
    return 4.0 * np.maximum(G6, GINF * np.abs(x))


def bounds(c, dt, x, ref):
    """-> (bound on |hi - ref|, bound on |hi + lo - ref| or None), [M, N]"""
    r = np.abs(ref[:, :c["N"]])
    base = G(x) + (U32 * r if c["res"] else 0.0)
    if c["out_f32"]:
        return base, None
    return base + ULP[dt] * r + TINY[dt], (base + 0.5 * ULP[dt] ** 2 * r + TINY[dt]) if c["c_lo"] else None


def out_type_round(c, dt, v):
    return np.asarray(v, np.float32) if c["out_f32"] else round_to(dt, v)


def violation(c, dt, hi, lo, x, ref):
    """hi, lo: the C / C_lo images [M, n_store] as float32 (lo None without C_lo).  Returns None when the images meet
    every requirement of the module docstring, else a one-line description of the first that fails."""
    N = c["N"]
    hi = hi.astype(np.float64)
    pad = hi[:, N:]
    if pad.size and not ((pad == 0).all() and not np.signbit(pad).any()):
        return "pad columns [N, n_store) of C are not +0"
    if lo is not None:
        lo = lo.astype(np.float64)
        if lo[:, N:].size and not ((lo[:, N:] == 0).all() and not np.signbit(lo[:, N:]).any()):
            return "pad columns [N, n_store) of C_lo are not +0"
        lo = lo[:, :N]
    h, r = hi[:, :N], ref[:, :N]
    fin = np.isfinite(x)
    if c["nonfinite"]:
        if not np.isnan(h[np.isnan(x)]).all():
            return "NaN in did not give NaN out"
        if np.isfinite(h[np.isinf(x)]).any():
            return "an infinite pre-activation gave a finite result"
    elif not fin.all():
        return "a finite case with a non-finite pre-activation"
    b_hi, b_pair = bounds(c, dt, x, ref)
    # a 16-bit result whose bound reaches past the type's largest finite value may leave as the infinity of that side
    top = np.inf if c["out_f32"] else MAXF[dt]
    with np.errstate(invalid="ignore"):
        over = fin & (((h == np.inf) & (r + b_hi > top)) | ((h == -np.inf) & (r - b_hi < -top)))
    cmp = fin & ~over
    if not np.isfinite(h[cmp]).all():
        m, n = np.argwhere(cmp & ~np.isfinite(h))[0]
        return f"non-finite result {h[m, n]!r} at ({m}, {n}), x = {x[m, n]!r}"
    with np.errstate(invalid="ignore"):
        err = np.where(cmp, np.abs(h - r), 0.0)
        bad = err > np.where(cmp, b_hi, np.inf)
    if bad.any():
        m, n = np.argwhere(bad)[0]
        return f"|C - ref| = {err[m, n]:.3e} > {b_hi[m, n]:.3e} at ({m}, {n}), x = {x[m, n]!r}: got {h[m, n]!r} ref {r[m, n]!r}"
    if lo is not None:
        if not np.isfinite(lo[cmp]).all():
            return "non-finite C_lo"
        with np.errstate(invalid="ignore"):
            err = np.where(cmp, np.abs(h + lo - r), 0.0)
            bad = err > np.where(cmp, b_pair, np.inf)
        if bad.any():
            m, n = np.argwhere(bad)[0]
            return f"|C + C_lo - ref| = {err[m, n]:.3e} > {b_pair[m, n]:.3e} at ({m}, {n}), x = {x[m, n]!r}"
    if not c["res"]:
        xc, hc = x[cmp], h[cmp]
        if (hc[xc == 0] != 0).any():
            return "f(0) != 0"
        if (hc[xc < 0] > 0).any() or (hc[xc > 0] < 0).any():
            return "the result has the wrong sign"
        lim = out_type_round(c, dt, np.abs(xc).astype(np.float32)).astype(np.float64)
        if (np.abs(hc) > lim).any():
            i = int(np.argmax(np.abs(hc) > lim))
            return f"|result| > |x|: x = {xc[i]!r}, got {hc[i]!r}"
    return None


def worst(c, hi, lo, x, ref):
    """The figures the GPU test prints, over the finite results: (largest |got - ref| over |x| <= 6, its x, largest
    |got - ref| / |x| over |x| > 6, its x); got = C (+ C_lo)."""
    N = c["N"]
    with np.errstate(invalid="ignore"):
        got = hi[:, :N].astype(np.float64) + (lo[:, :N].astype(np.float64) if lo is not None else 0.0)
        err = np.where(np.isfinite(x) & np.isfinite(got), np.abs(got - ref[:, :N]), 0.0)
        inner = np.where(np.abs(x) <= 6, err, 0.0)
        outer = np.where(np.abs(x) > 6, err / np.maximum(np.abs(x), 1.0), 0.0)
    i, o = np.unravel_index(int(np.argmax(inner)), err.shape), np.unravel_index(int(np.argmax(outer)), err.shape)
    return float(inner[i]), float(x[i]), float(outer[o]), float(x[o])


# ----------------------------------------------------------------------------------------------------
# a float32 model of the epilogue, and the faults planted in it
# ----------------------------------------------------------------------------------------------------
FAULTS = ("tanh", "no_clamp", "clamp_x", "res_before_act", "bias_after_act", "no_alpha", "pair_swapped", "no_max",
          "edge_no_act")


def header_coefficients():
    """the polynomial of gelu_erf as csrc/pio_gemm_common.h states it, highest degree first"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "perceiverio_pytorch_amd", "csrc",
                        "pio_gemm_common.h")
    body = re.search(r"float gelu_erf\(float x\) \{(.*?)\n\}", open(path).read(), re.S).group(1)
    first = re.search(r"float q = ([-+0-9.e]+)f;", body).group(1)
    rest = re.findall(r"q = fmaf\(q, a, ([-+0-9.e]+)f\);", body)
    return [float(first)] + [float(v) for v in rest]


def gelu_from_header(x, clamp=True):
    """gelu_erf restated from the header's own coefficients (numpy float32, np.exp2); clamp=False: the polynomial at |x|"""
    f = np.float32
    x = x.astype(f)
    a = np.minimum(np.abs(x), f(6.0)) if clamp else np.abs(x)
    co = header_coefficients()
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.full(x.shape, co[0], f)
        for k in co[1:]:
            q = q * a + f(k)
        return -np.abs(x) * np.exp2(q) + np.maximum(x, f(0))


def sees(c, fault):
    """can the case tell the fault from the contract?"""
    if c["nonfinite"]:
        return False
    band = c["N"] >= COL_P      # (only the band holds |x| > 6 and a non-zero bias: the two-column case has none)
    return {"res_before_act": c["res"], "no_alpha": c["alpha"] != 1.0, "edge_no_act": c["N"] % TILE_N[c["kernel"]] != 0,
            "pair_swapped": c["N"] >= 2, "no_clamp": band, "bias_after_act": band}.get(fault, True)


def model(c, arrays, dt, fault=None):
    """The epilogue in numpy float32 -> (C, C_lo or None) images [M, n_store] float32.  fault: one of FAULTS."""
    f = np.float32
    M, N = c["M"], c["N"]
    A, B = _view(arrays["A"], M, c["lda"], 2), _view(arrays["B"], N, c["ldb"], 2)
    acc = (A.astype(np.float64) @ B.astype(np.float64).T).astype(f)
    bias = arrays["bias"][:N if c["bias_mode"] == 1 else M]
    bias = bias[None, :] if c["bias_mode"] == 1 else bias[:, None]
    R = _view(arrays["R"], M, c["ldr"], N) if c["res"] else None
    with np.errstate(invalid="ignore", over="ignore"):
        x = acc * f(1.0 if fault == "no_alpha" else c["alpha"])
        if fault != "bias_after_act":
            x = x + bias
        if fault == "res_before_act":
            x = x + R
        if fault == "tanh":
            y = f(0.5) * x * (f(1) + np.tanh(f(0.7978845608028654) * (x + f(0.044715) * x * x * x)))
        elif fault == "no_clamp":
            y = gelu_from_header(x, clamp=False)
        elif fault == "clamp_x":
            y = f32_gelu(np.clip(x, f(-6), f(6)))
        elif fault == "no_max":
            y = f32_gelu(x) - np.maximum(x, f(0))
        else:
            y = f32_gelu(x)
        if fault == "pair_swapped":
            n2 = N & ~1
            y[:, :n2] = y[:, :n2].reshape(M, n2 // 2, 2)[:, :, ::-1].reshape(M, n2)
        if fault == "edge_no_act":
            n0 = N // TILE_N[c["kernel"]] * TILE_N[c["kernel"]]
            y[:, n0:] = x[:, n0:]
        if fault == "bias_after_act":
            y = y + bias
        if R is not None and fault != "res_before_act":
            y = y + R
        v = np.zeros((M, c["n_store"]), f)
        v[:, :N] = y.astype(f) + f(0)
        if c["out_f32"]:
            return v, None
        hi = round_to(dt, v)
        return hi, (round_to(dt, v - hi) if c["c_lo"] else None)
