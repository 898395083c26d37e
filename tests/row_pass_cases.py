"""Cases, probes and references for the two row kernels of the folded paths that no exported primitive reached
(csrc/pio_elementwise.hip; include/pio_hip.h: pio_rowstats_cast, pio_transpose16).  Numpy only.

tests/test_row_pass_host.py proves on the CPU that the references are right, that the case tables reject every fault these
kernels can have (each fault is a mutation of the models below) and that the refusal tables are what a restatement of the
launchers' checks gives; tests/test_row_pass_gpu.py launches the kernels on guarded, NaN-surrounded buffers and runs the
refusal tables against the launchers themselves.

pio_rowstats_cast   x fp32 [rows, C] -> y = rn(x), y_lo = rn(x - y), part[row][C / slot_w][2] = (sum, sum of squares) per slot.
  int       x = small integers / 4 (|4 x| <= 256: exact in fp16 and bf16): y == x, y_lo == +0 and every sum exact in fp32 in
            any order (the largest sum of squares is below 2^24 / 16): EVERYTHING bit for bit.  The first column of every
            slot is chosen so that all (row, slot) of a case differ in their sum AND in their sum of squares: a slot that
            lands elsewhere is an O(1) error.
  residual  x = h + l: h in +-[128, 256) on the type's grid there (fp16: multiples of 1/8, bf16: integers), l = k 2^-8 (fp16) /
            k 2^-5 (bf16) with 1 <= |k| <= 12 -- below half an ulp of h, a value of the type itself, h + l exact in fp32:
            y == h and y_lo == l bit for bit.  The sums are held to SUM_BOUND.
  gauss     standard normal x: y and y_lo are casts, hence exact (x - y is exact in fp32); sums within SUM_BOUND.
  big       the int probe with ONE element 2^70: the sum of squares of its slot is +inf, its sum 2^70 within SUM_BOUND, its
            16-bit image +inf / -inf (y / y_lo) in fp16 and 2^70 / +0 in bf16; every other slot and row bit for bit.
SUM_BOUND   An fp32 sum of n terms in ANY order -- sequential, tree, four per lane and then shuffles -- has n - 1 additions,
            each off by at most u = 2^-24 relative, so it differs from the exact sum by at most gamma(n - 1) sum |term| with
            gamma(k) = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2): (n - 1) 2^-24
            sum |term| to first order.  The squares are products rounded once more (not at all under an FMA): gamma(n) sum x^2.
            n = slot_w.  The float64 reference's own error (2^-53 n) is five orders below and not counted.

pio_transpose16     x 16-bit [B][T][ldx] -> vt [B][C][tkv], vt[b][c][t] = x[b][t][c], columns [T, tkv) = +0.  Bit patterns only:
            element (b, t, c) holds hash16(b, t, c) (NaN patterns, infinities and -0 among them).  Pitch columns, the rows
            behind the last and the output payload hold POISON.
"""
import numpy as np

from primitive_cases import DTYPES, round_to  # noqa: F401  (re-exported)

U32 = 2.0 ** -24
POISON = 0x7E7B          # a NaN of fp16 and of bf16
E_SHAPE, E_ALIGN, E_ARG = -1, -2, -6
PTR = 0x7F0000001000     # an aligned address for the CPU restatement of the launchers' checks (arithmetic only)


def padc(c):
    return (c + 63) & ~63 if c >= 256 else (c + 7) & ~7


def gamma(k):
    return k * U32 / (1.0 - k * U32)


# ====================================================================================================
# pio_rowstats_cast
# ====================================================================================================
RS_C = (256, 512, 1024, 1280)
RS_SLOT_W = (64, 128)
RS_ROWS = (1, 3, 4, 5, 9)
RS_PROBES = ("int", "residual", "gauss", "big")
# every (C, slot_w, rows) with the int probe -- 40 launches of a few rows each; the other probes on a pairwise selection
RS_SHAPES = [(C, w, r) for C in RS_C for w in RS_SLOT_W for r in RS_ROWS]
RS_SHAPES_FEW = [(256, 64, 5), (512, 128, 3), (1024, 64, 9), (1280, 128, 1), (1280, 64, 4)]
RS_BIG_AT = (-1, 130)     # (row, column) of the 2^70 element: last row, slot 2 of 64 / slot 1 of 128


def rs_input(C, slot_w, rows, probe, dt):
    """x [rows, C] float32 of one probe (module docstring); for `residual` also (h, l)."""
    base = "int" if probe == "big" else probe           # (big: the int probe of the same shape around one planted element)
    rng = np.random.default_rng(C * 1000 + slot_w * 10 + rows + 7 * RS_PROBES.index(base) + (dt == "bf16"))
    ns = C // slot_w
    if probe in ("int", "big"):
        # columns 2 .. of a slot: random in [-2, 2]; column 0 makes the slot's sum its target (a permutation of the (row, slot)
        # indices: distinct); column 1 is the first value that gives a sum of squares no earlier slot of the case has
        k = rng.integers(-2, 3, (rows, C))
        ks = k.reshape(rows, ns, slot_w)
        target = (np.arange(rows * ns).reshape(rows, ns) * 37) % (rows * ns) - (rows * ns) // 2
        seen = set()
        for r in range(rows):
            for s in range(ns):
                rest, rest_q = int(ks[r, s, 2:].sum()), int((ks[r, s, 2:] ** 2).sum())
                for b in range(-3, 100):
                    a = int(target[r, s]) - rest - b
                    q = a * a + b * b + rest_q
                    if q not in seen and abs(a) <= 256:
                        break
                else:
                    raise AssertionError("no integer probe with distinct sums of squares")
                seen.add(q)
                ks[r, s, 0], ks[r, s, 1] = a, b
        x = (k / 4.0).astype(np.float32)
        if probe == "big":
            x[RS_BIG_AT] = np.float32(2.0 ** 70)
        return x
    if probe == "residual":
        sign = rng.choice([-1.0, 1.0], (rows, C))
        step, lstep = (0.125, 2.0 ** -8) if dt == "f16" else (1.0, 2.0 ** -5)
        h = sign * (128.0 + step * rng.integers(1, int(128 / step), (rows, C)))     # (not 128 itself: finer grid below it)
        kk = rng.integers(1, 13, (rows, C)) * rng.choice([-1, 1], (rows, C))
        l = kk * lstep
        x = (h + l).astype(np.float32)
        assert np.array_equal(x.astype(np.float64), h + l)
        return x, h.astype(np.float32), l.astype(np.float32)
    if probe == "gauss":
        return rng.standard_normal((rows, C)).astype(np.float32)
    raise KeyError(probe)


def rs_reference(x, slot_w, dt):
    """-> y, y_lo (float32 images of the 16-bit values), part [rows, C / slot_w, 2] float64, bound of the same shape."""
    x = np.asarray(x, np.float32)
    rows, C = x.shape
    with np.errstate(all="ignore"):
        y = round_to(dt, x)
        lo = round_to(dt, x - y)
        xs = x.astype(np.float64).reshape(rows, C // slot_w, slot_w)
        part = np.stack([xs.sum(axis=2), (xs * xs).sum(axis=2)], axis=2)
        part[..., 1] = np.where(part[..., 1] >= 2.0 ** 128, np.inf, part[..., 1])      # beyond fp32: +inf
        bound = np.stack([gamma(slot_w - 1) * np.abs(xs).sum(axis=2), gamma(slot_w) * (xs * xs).sum(axis=2)], axis=2)
    return y, lo, part, bound


RS_FAULTS = ("other_slot_w", "swap_sum_sq", "ragged_rows_unwritten", "lo_copy_of_y", "part_pitch_128")
RS_TAIL = 64         # floats of `part` behind the last slot that the models may (wrongly) reach


def rs_model(x, slot_w, dt, with_lo=True, fault=None):
    """What the kernel leaves in NaN-filled buffers -- y [rows, C], y_lo (None without), part as a FLAT float64 array of
    rows * (C / slot_w) * 2 + RS_TAIL elements -- with one `fault` of RS_FAULTS, or none."""
    rows, C = x.shape
    ns = C // slot_w
    y, lo, part, _ = rs_reference(x, slot_w, dt)
    y, lo = y.copy(), lo.copy()
    flat = np.full(rows * ns * 2 + RS_TAIL, np.nan)
    live = rows if fault != "ragged_rows_unwritten" else 4 * (rows // 4)      # the last, partial workgroup does nothing
    if fault == "lo_copy_of_y":
        lo = y.copy()
    if fault == "swap_sum_sq":
        part = part[..., ::-1]
    y[live:] = np.nan
    lo[live:] = np.nan
    other = 192 - slot_w
    for r in range(live):
        for s in range(ns):
            slot = (s * slot_w) // other if fault == "other_slot_w" else s
            pitch = C // 128 if (fault == "part_pitch_128" and slot_w == 64) else ns
            at = (r * pitch + slot) * 2
            if at + 2 <= flat.size:
                flat[at:at + 2] = part[r, s]
    return y, (lo if with_lo else None), flat


def rs_rejects(x, slot_w, dt, with_lo, got):
    """Does the comparison the GPU test makes (bit for bit on an int probe) reject the model output `got`?"""
    y, lo, part, _ = rs_reference(x, slot_w, dt)
    gy, glo, gflat = got
    n = part.size
    same = np.array_equal(gy, y, equal_nan=True) and np.array_equal(gflat[:n], part.reshape(-1), equal_nan=True) and \
        np.isnan(gflat[n:]).all()
    if with_lo:
        same = same and np.array_equal(glo, lo, equal_nan=True) and \
            np.array_equal(np.signbit(glo), np.signbit(lo))
    return not same


def rowstats_refusal(x, rows, C, slot_w, y16, y16_lo, part, dtype):
    """The checks of rowstats_cast_launch, in its order, on integer addresses (0 = NULL): 0 or the PIO_E_* code."""
    if not x or not y16 or not part or rows <= 0:
        return E_ARG
    if C <= 0 or C % 256 or slot_w not in (64, 128):
        return E_SHAPE
    if x & 15 or y16 & 7 or part & 7 or y16_lo & 7:
        return E_ALIGN
    return 0 if dtype in (0, 1) else E_ARG


# (id, expected code, arguments that differ from the well-formed call x = y16 = y16_lo = part = aligned, rows 4, C 256, slot_w
# 64, dtype fp16).  Pointer entries are byte offsets from an aligned buffer ("null": NULL).
RS_REFUSED = [
    ("x_null", E_ARG, dict(x="null")), ("y16_null", E_ARG, dict(y16="null")), ("part_null", E_ARG, dict(part="null")),
    ("rows_0", E_ARG, dict(rows=0)), ("rows_negative", E_ARG, dict(rows=-4)), ("dtype_2", E_ARG, dict(dtype=2)),
    ("dtype_negative", E_ARG, dict(dtype=-1)), ("x_null_wins_over_shape", E_ARG, dict(x="null", C=100)),
    ("c_0", E_SHAPE, dict(C=0)), ("c_negative", E_SHAPE, dict(C=-256)), ("c_128", E_SHAPE, dict(C=128)),
    ("c_320", E_SHAPE, dict(C=320)), ("c_1028", E_SHAPE, dict(C=1028)), ("slot_w_32", E_SHAPE, dict(slot_w=32)),
    ("slot_w_0", E_SHAPE, dict(slot_w=0)), ("slot_w_256", E_SHAPE, dict(slot_w=256)), ("slot_w_96", E_SHAPE, dict(slot_w=96)),
    ("shape_wins_over_align", E_SHAPE, dict(C=320, x=4)),
    ("x_off_4", E_ALIGN, dict(x=4)), ("x_off_8", E_ALIGN, dict(x=8)), ("y16_off_2", E_ALIGN, dict(y16=2)),
    ("y16_off_4", E_ALIGN, dict(y16=4)), ("y16_lo_off_4", E_ALIGN, dict(y16_lo=4)), ("y16_lo_off_2", E_ALIGN, dict(y16_lo=2)),
    ("part_off_4", E_ALIGN, dict(part=4)), ("align_wins_over_dtype", E_ALIGN, dict(part=4, dtype=7)),
]
RS_ACCEPTED = [("y16_off_8", dict(y16=8)), ("part_off_8", dict(part=8)), ("y16_lo_null", dict(y16_lo="null")), ("x_off_16", dict(x=16))]


def rs_call_args(change, base):
    """(x, rows, C, slot_w, y16, y16_lo, part, dtype) as integers for a table entry; base: {name: aligned address}."""
    a = dict(rows=4, C=256, slot_w=64, dtype=0, x=0, y16=0, y16_lo=0, part=0)
    a.update(change)
    ptr = {k: (0 if a[k] == "null" else base[k] + a[k]) for k in ("x", "y16", "y16_lo", "part")}
    return ptr["x"], a["rows"], a["C"], a["slot_w"], ptr["y16"], ptr["y16_lo"], ptr["part"], a["dtype"]


# ====================================================================================================
# pio_transpose16
# ====================================================================================================
TR_T = (1, 7, 63, 64, 65, 100, 129)
TR_C = (8, 40, 64, 72, 328)
TR_LDX = ("c", "c8", "padc")
TR_TKV = ("r8", "r32", "r32_128")
TR_B = (1, 3)
# a selection that reaches every value of every axis, and every pair (T off / on the tile) x (C off / on the tile)
TR_CASES = [
    # T, C, ldx, tkv, B
    (1, 8, "c", "r8", 1), (7, 40, "c8", "r32", 3), (63, 64, "padc", "r32_128", 1), (64, 72, "c8", "r8", 3),
    (65, 328, "padc", "r32", 3), (100, 328, "c", "r32_128", 1), (129, 328, "c8", "r8", 3), (129, 64, "c", "r32", 1),
    (64, 64, "c", "r8", 1), (100, 40, "padc", "r32_128", 3), (65, 8, "c8", "r32_128", 3), (7, 72, "c", "r32", 1),
    (1, 328, "padc", "r32_128", 3), (63, 72, "padc", "r8", 3), (129, 8, "padc", "r8", 1),
]


def tr_shape(case):
    """-> (B, T, C, ldx, tkv)"""
    T, C, ldx, tkv, B = case
    ld = {"c": C, "c8": C + 8, "padc": padc(C)}[ldx]
    tk = {"r8": (T + 7) & ~7, "r32": (T + 31) & ~31, "r32_128": ((T + 31) & ~31) + 128}[tkv]
    return B, T, C, ld, tk


def tr_id(case):
    return "T{}_C{}_ldx-{}_tkv-{}_B{}".format(*case)


def hash16(b, t, c):
    """16 bits that name (b, t, c): odd multipliers, so that a step in any one index -- and a swap of t and c -- changes them."""
    return ((np.asarray(b, np.int64) * 40503 + np.asarray(t, np.int64) * 30011 + np.asarray(c, np.int64) * 10007 + 12345)
            & 0xFFFF).astype(np.uint16)


TR_XTAIL = 4096      # poison elements behind the last row: what a too-long stride or pitch reads


def tr_input(case):
    """flat uint16 payload of x: [B][T][ldx] with hash16 in the C columns, POISON in the pitch columns and in the tail."""
    B, T, C, ldx, _ = tr_shape(case)
    x = np.full(B * T * ldx + TR_XTAIL, POISON, np.uint16)
    b, t, c = np.ogrid[:B, :T, :C]
    x[:B * T * ldx].reshape(B, T, ldx)[:, :, :C] = hash16(b, t, c)
    return x


def tr_reference(case):
    """vt [B, C, tkv] uint16, from the definition by index (not from the input payload)."""
    B, T, C, _, tkv = tr_shape(case)
    vt = np.zeros((B, C, tkv), np.uint16)
    b, c, t = np.ogrid[:B, :C, :T]
    vt[:, :, :T] = hash16(b, t, c)
    return vt


TR_FAULTS = ("swap_tc_in_tile", "tail_unwritten", "batch_stride_tkv_ldx", "batch_stride_T_C", "pitch_C", "drop_last_row",
             "clip_last_c_tile")


def tr_model(case, x, fault=None):
    """What the kernel leaves in a POISON-filled vt [B, C, tkv], tile by tile as it works, with one fault of TR_FAULTS."""
    B, T, C, ldx, tkv = tr_shape(case)
    vt = np.full((B, C, tkv), POISON, np.uint16)
    pitch = C if fault == "pitch_C" else ldx
    sb = {"batch_stride_tkv_ldx": tkv * ldx, "batch_stride_T_C": T * C}.get(fault, T * ldx)
    rows = T - 1 if fault == "drop_last_row" else T
    ctiles = C // 64 if fault == "clip_last_c_tile" else (C + 63) // 64

    T64, C64 = (tkv + 63) & ~63, (C + 63) & ~63
    t, c = np.ogrid[:rows, :C]
    for b in range(B):
        at = b * sb + t * pitch + c
        full = np.zeros((T64, C64), np.uint16)                   # the LDS tiles side by side, [t][c]: zeros where t >= T
        full[:rows, :C] = np.where(at < x.size, x[np.minimum(at, x.size - 1)], POISON)
        if fault == "swap_tc_in_tile":                           # element (r, cc) of tile (ti, ci) lands at row ci 64 + r
            out = full.reshape(T64 // 64, 64, C64 // 64, 64).transpose(2, 1, 0, 3).reshape(C64, T64)
        else:
            out = full.T
        nc = min(C, 64 * ctiles)
        vt[b, :nc, :] = out[:nc, :tkv]
        if fault == "tail_unwritten":
            vt[b, :, T:] = POISON
    return vt


def transpose_refusal(x, ldx, B, T, C, vt, tkv):
    """The checks of transpose16_launch, in its order, on integer addresses."""
    if not x or not vt or B <= 0 or T <= 0 or C <= 0:
        return E_ARG
    if C & 7 or ldx & 7 or tkv & 7 or tkv < T or B > 65535:
        return E_SHAPE
    if x & 15 or vt & 15:
        return E_ALIGN
    return 0


# well-formed call: B 2, T 20, C 16, ldx 24, tkv 32, aligned pointers
TR_REFUSED = [
    ("x_null", E_ARG, dict(x="null")), ("vt_null", E_ARG, dict(vt="null")), ("b_0", E_ARG, dict(B=0)),
    ("t_0", E_ARG, dict(T=0)), ("c_0", E_ARG, dict(C=0)), ("t_negative", E_ARG, dict(T=-8)),
    ("null_wins_over_shape", E_ARG, dict(vt="null", C=12)),
    ("c_12", E_SHAPE, dict(C=12)), ("c_20", E_SHAPE, dict(C=20, ldx=24)), ("ldx_20", E_SHAPE, dict(ldx=20)),
    ("ldx_28", E_SHAPE, dict(ldx=28)), ("tkv_28", E_SHAPE, dict(tkv=28)), ("tkv_below_t", E_SHAPE, dict(tkv=16)),
    ("tkv_t_minus_4", E_SHAPE, dict(T=24, tkv=20)), ("b_65536", E_SHAPE, dict(B=65536)),
    ("shape_wins_over_align", E_SHAPE, dict(C=12, x=2)),
    ("x_off_2", E_ALIGN, dict(x=2)), ("x_off_8", E_ALIGN, dict(x=8)), ("vt_off_2", E_ALIGN, dict(vt=2)),
    ("vt_off_8", E_ALIGN, dict(vt=8)),
]
TR_ACCEPTED = [("tkv_equals_t", dict(T=32, tkv=32)), ("x_off_16", dict(x=16)), ("vt_off_16", dict(vt=16))]


def tr_call_args(change, base):
    """(x, ldx, B, T, C, vt, tkv) as integers for a table entry; base: {name: aligned address}."""
    a = dict(B=2, T=20, C=16, ldx=24, tkv=32, x=0, vt=0)
    a.update(change)
    ptr = {k: (0 if a[k] == "null" else base[k] + a[k]) for k in ("x", "vt")}
    return ptr["x"], a["ldx"], a["B"], a["T"], a["C"], ptr["vt"], a["tkv"]
