"""Cases and float64 references for the memory-bound primitive kernels of csrc/pio_elementwise.hip:
pio_pack_linear, pio_layernorm_cast(_cat), pio_softmax_rows, pio_bn_relu_maxpool_tokens.

Numpy only; shared by tests/test_primitive_cases_host.py (CPU: the references against torch's float64 ops, branch
coverage of the tables) and tests/test_primitives_gpu.py (MI355X: the kernels against the references).

The references restate the DEFINITIONS of include/pio_hip.h in float64, not the kernels.  Each case names the launcher
branch it is meant to reach; tests/test_rows_route.py asks the launchers' own routing header (csrc/pio_rows_route.h) that
it does.
"""
import numpy as np

DTYPES = ("f16", "bf16")
ULP = {"f16": 2.0 ** -10, "bf16": 2.0 ** -8}          # twice the half-ulp one rounding to the type may cost
TINY = {"f16": 2.0 ** -24, "bf16": 2.0 ** -133}       # smallest subnormal of the type


def pad8(c):
    return (c + 7) & ~7


# ----------------------------------------------------------------------------------------------------
# rounding to the operand types (round to nearest even, subnormals kept), for the EXACT comparisons of pack_linear
# ----------------------------------------------------------------------------------------------------
def round_to(dtype, a):
    """float32 array -> the nearest value of `dtype`, returned as float32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "f16":
        return a.astype(np.float16).astype(np.float32)
    bits = a.view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).reshape(a.shape)


# ----------------------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------------------
def ref_pack_linear(w, bias, row_heads, col_heads, k_pad, dst_row0, rows_total):
    """W [out, in] -> (image [rows_total, k_pad] float64, bias image [rows_total] float64, written [rows_total] bool).
    Rows are `row_heads` groups of out / row_heads, each padded to a multiple of 8; columns likewise.  The packed rows
    start at `dst_row0`; padding inside them is zero, rows outside are NaN in the images and False in `written`.  The
    image holds the UN-rounded values: hi = round(image), lo = round(image - hi)."""
    w = np.asarray(w, dtype=np.float64)
    out, inn = w.shape
    dr, dc = out // row_heads, inn // col_heads
    drp, dcp = pad8(dr), pad8(dc)
    rows_p = row_heads * drp
    img = np.full((rows_total, k_pad), np.nan)
    bimg = np.full((rows_total,), np.nan)
    written = np.zeros(rows_total, dtype=bool)
    img[dst_row0:dst_row0 + rows_p] = 0.0
    bimg[dst_row0:dst_row0 + rows_p] = 0.0
    written[dst_row0:dst_row0 + rows_p] = True
    for r in range(out):
        pr = dst_row0 + (r // dr) * drp + r % dr
        for hc in range(col_heads):
            img[pr, hc * dcp:hc * dcp + dc] = w[r, hc * dc:(hc + 1) * dc]
        if bias is not None:
            bimg[pr] = float(bias[r])
    return img, bimg, written


def ref_layernorm_cast(x, gamma, beta, eps, c_pad):
    """x [..., C] -> [..., c_pad] float64: LayerNorm over the last axis (biased variance), zeros in [C, c_pad).
    gamma is None: plain copy."""
    x = np.asarray(x, dtype=np.float64)
    C = x.shape[-1]
    if gamma is None:
        y = x
    else:
        mean = x.mean(axis=-1, keepdims=True)
        var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
        y = (x - mean) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    out = np.zeros(x.shape[:-1] + (c_pad,))
    out[..., :C] = y
    return out


def softmax_valid(shape, kv_mask, q_mask, full_mask):
    """[B, 1 or H, Tq, Tk] bool: a mask entry counts as true iff its byte is non-zero."""
    B, H, Tq, Tk = shape
    ok = np.ones((B, 1, Tq, Tk), dtype=bool)
    if kv_mask is not None:
        ok &= (np.asarray(kv_mask) != 0)[:, None, None, :]
    if q_mask is not None:
        ok &= (np.asarray(q_mask) != 0)[:, None, :, None]
    if full_mask is not None:
        ok &= (np.asarray(full_mask) != 0)[:, None, :, :]
    return ok


def ref_softmax_rows(S, scale, kv_mask, q_mask, full_mask, bias):
    """S [B, H, Tq, Tk] -> softmax over the attendable keys of (S + bias) * scale, float64; masked entries are zero and
    rows with no attendable key are zeros."""
    s = np.asarray(S, dtype=np.float64)
    if bias is not None:
        s = s + np.asarray(bias, dtype=np.float64)
    s = s * np.float64(np.float32(scale))
    ok = np.broadcast_to(softmax_valid(s.shape, kv_mask, q_mask, full_mask), s.shape)
    m = np.where(ok, s, -np.inf).max(axis=-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    e = np.where(ok, np.exp(np.where(ok, s - m, 0.0)), 0.0)
    z = e.sum(axis=-1, keepdims=True)
    return np.where(z > 0, e / np.where(z > 0, z, 1.0), 0.0)


def ref_bn_relu_maxpool_tokens(x, scale, shift, pad_top, pad_left):
    """x [B, C, H, W] -> (y, mag), both [B, OH*OW, C] float64: y = max over the 3x3 stride-2 window (rows 2 oh - pad_top
    + 0..2, columns 2 ow - pad_left + 0..2; cells outside the image count as 0) of relu(x * scale[c] + shift[c]);
    mag = |x * scale| + |shift| of the winning cell (of the largest pre-ReLU cell when the result is the ReLU's 0)."""
    x = np.asarray(x, dtype=np.float64)
    B, C, H, W = x.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    sc = np.asarray(scale, np.float64)[None, :, None, None]
    sh = np.asarray(shift, np.float64)[None, :, None, None]
    val = x * sc + sh
    mag = np.abs(x * sc) + np.abs(sh)
    best = np.full((B, C, OH, OW), -np.inf)
    bmag = np.zeros((B, C, OH, OW))
    for r in range(3):
        for d in range(3):
            ih = 2 * np.arange(OH) - pad_top + r
            iw = 2 * np.arange(OW) - pad_left + d
            okh, okw = (ih >= 0) & (ih < H), (iw >= 0) & (iw < W)
            ihc, iwc = np.clip(ih, 0, H - 1), np.clip(iw, 0, W - 1)
            ok = (okh[:, None] & okw[None, :])[None, None]
            v = np.where(ok, val[:, :, ihc][:, :, :, iwc], -np.inf)
            g = np.where(ok, mag[:, :, ihc][:, :, :, iwc], 0.0)
            take = v > best
            best = np.where(take, v, best)
            bmag = np.where(take, g, bmag)
    y = np.maximum(best, 0.0)
    return (y.transpose(0, 2, 3, 1).reshape(B, OH * OW, C), bmag.transpose(0, 2, 3, 1).reshape(B, OH * OW, C))


# ----------------------------------------------------------------------------------------------------
# pio_softmax_rows
# ----------------------------------------------------------------------------------------------------
SM_B, SM_H, SM_TQ = 2, 3, 7          # 42 rows: not a multiple of the 4 rows a workgroup takes
SM_SCALE = 0.125                      # 1 / sqrt(64): a power of two, so that s * scale is exact in fp32 (see sm_inputs)
SM_FORMS = ("plain", "full")          # every optional pointer NULL | kv_mask, q_mask, full_mask, bias, P_lo together
SM_BRANCHES = ("reg_nv2", "reg_nv8", "reg_nv16", "gen_w1", "gen_w4")


def _sm(name, branch, Tk, lds=None, ldp=None, s_off=0):
    return dict(id=name, branch=branch, Tk=Tk, lds=Tk if lds is None else lds, ldp=pad8(Tk) if ldp is None else ldp,
                s_off=s_off)


SOFTMAX_CASES = [
    _sm("tk8", "reg_nv2", 8),
    _sm("tk512", "reg_nv2", 512),
    _sm("tk500_ldp512", "reg_nv2", 500, ldp=512),
    _sm("tk512_lds516_gap", "reg_nv2", 512, lds=516),            # pitched S: the gap columns hold NaN
    _sm("tk516", "reg_nv8", 516),
    _sm("tk2048", "reg_nv8", 2048),
    _sm("tk2052", "reg_nv16", 2052),
    _sm("tk4096", "reg_nv16", 4096),
    _sm("tk13", "gen_w1", 13),
    _sm("tk2046", "gen_w1", 2046),
    _sm("tk512_s_off1", "gen_w1", 512, s_off=1),                 # S one float past a 16-byte boundary
    _sm("tk512_lds513_gap", "gen_w1", 512, lds=513),
    _sm("tk2050", "gen_w4", 2050),
    _sm("tk4100", "gen_w4", 4100),                               # ldp = 4104 > 4096
]
SM_MASK_BYTE_CASES = ("tk512", "tk13")     # one register-kernel shape, one generic shape
MASK_TRUE_BYTES = (1, 2, 0x80, 0xFF)


# rows planted in every case (sample 0; in the masked form sample 1 has every key masked by kv_mask)
SM_ROW_QMASKED, SM_ROW_FULL_EMPTY, SM_ROW_ONE_KEY, SM_ROW_LARGE, SM_ROW_CONST = 1, 2, 3, 4, 5


def sm_inputs(case, form, seed=0):
    """S (float32 [B, H, Tq, Tk], N(0, 4^2)), scale and, for the masked form, kv_mask / q_mask / full_mask (uint8, 0 / 1)
    and bias.  Query row SM_ROW_LARGE of sample 0 is scaled so that max |s * scale| = 1e4 and row SM_ROW_CONST holds one
    value.  The scale is a power of two and the bias of the large row is zero: (s + bias) * scale is then exact in fp32
    for that row, so it tests the max subtraction and not the 1e4 * 2^-24 = 6e-4 rounding of an fp32 sum at that
    magnitude, which no fp32 softmax can avoid and which would show as a 1e-3 relative error in the probabilities."""
    B, H, Tq, Tk = SM_B, SM_H, SM_TQ, case["Tk"]
    rng = np.random.default_rng(1000 + Tk + seed)
    S = (rng.standard_normal((B, H, Tq, Tk)) * 4).astype(np.float32)
    big = S[0, :, SM_ROW_LARGE, :]
    S[0, :, SM_ROW_LARGE, :] = (big * (1e4 / SM_SCALE / np.abs(big).max(axis=-1, keepdims=True))).astype(np.float32)
    S[0, :, SM_ROW_CONST, :] = np.float32(-3.25)
    d = dict(S=S, scale=SM_SCALE, kv_mask=None, q_mask=None, full_mask=None, bias=None)
    if form == "plain":
        _clear_flush_window(S, np.ones(Tk, dtype=bool))
        return d
    kv = (rng.random((B, Tk)) > 0.3).astype(np.uint8)
    kv[0, Tk - 1] = 1
    kv[1, :] = 0                                            # a sample whose keys are all masked
    qm = np.ones((B, Tq), dtype=np.uint8)
    qm[0, SM_ROW_QMASKED] = 0
    qm[1, 0] = 0
    fm = (rng.random((B, Tq, Tk)) > 0.3).astype(np.uint8)
    fm[0, SM_ROW_FULL_EMPTY, :] = 0
    fm[0, SM_ROW_ONE_KEY, :] = 0
    fm[0, SM_ROW_ONE_KEY, Tk - 1] = 1                       # exactly one attendable key, the last: probability 1
    fm[0, SM_ROW_LARGE, :] = 1
    bias = rng.standard_normal((B, H, Tq, Tk)).astype(np.float32)
    bias[0, :, SM_ROW_LARGE, :] = 0.0
    _clear_flush_window(S, kv[0] != 0)
    d.update(kv_mask=kv, q_mask=qm, full_mask=fm, bias=bias)
    return d


def _clear_flush_window(S, valid):
    """The large row spreads its logits over +-1e4, so some land where the probability is a bf16 SUBNORMAL:
    exp(x - max) in [2^-133, 2^-126).  The kernels' fast exponential returns 0 below fp32's smallest normal 2^-126, so
    those come out as 0 where float64 says up to 1.2e-38 -- measured on the MI355X, reported in the pull request that
    added this file, and not what this row is for (the max subtraction).  Entries of the large row inside that window
    are moved 8 further down, where the reference is below half of bf16's smallest subnormal too."""
    for h in range(S.shape[1]):
        row = S[0, h, SM_ROW_LARGE]
        x = row.astype(np.float64) * SM_SCALE
        rel = x - x[valid].max()
        row[(rel < -87.0) & (rel > -93.0)] -= np.float32(8.0 / SM_SCALE)


# ----------------------------------------------------------------------------------------------------
# pio_layernorm_cast
# ----------------------------------------------------------------------------------------------------
LN_B, LN_T = 3, 5
LN_EPS = 1e-5
LN_BRANCHES = ("reg_nv4", "reg_nv8", "reg2", "gen_vec", "gen_scalar")
LN_LAYOUTS = ("contiguous", "row_slice", "batch_broadcast", "uneven_batch")


def _ln(name, branch, C, c_pad=None, x_off=0):
    return dict(id=name, branch=branch, C=C, c_pad=pad8(C) if c_pad is None else c_pad, x_off=x_off)


LAYERNORM_CASES = [
    _ln("c8", "reg_nv4", 8),
    _ln("c1024", "reg_nv4", 1024),
    _ln("c600_pad640", "reg_nv4", 600, c_pad=640),               # 40 zero-filled columns
    _ln("c1028", "reg_nv8", 1028),
    _ln("c2048", "reg_nv8", 2048),
    _ln("c322", "reg2", 322),
    _ln("c1026", "reg2", 1026),
    _ln("c2052", "gen_vec", 2052),                               # c_pad = 2056 > 2048
    _ln("c261", "gen_scalar", 261),
    _ln("c1024_x_off1", "gen_scalar", 1024, x_off=1),            # x one float past a 16-byte boundary
]
LN_GAP = 8      # unread floats behind every row (row_slice) / behind every sample (uneven_batch): keeps C's alignment class


def ln_strides(case, layout):
    """(stride_b, stride_t, number of distinct samples in memory) in elements."""
    C = case["C"]
    st = C + LN_GAP if layout == "row_slice" else C
    if layout == "batch_broadcast":
        return 0, st, 1
    sb = LN_T * st + (LN_GAP if layout == "uneven_batch" else 0)
    return sb, st, LN_B


LN_ROW_CONST, LN_ROW_MEAN1E3, LN_ROW_OUTLIER, LN_ROW_ZERO = 0, 1, 2, 3     # rows t of sample 0


def _mirrored(rng, C, centre, spread, grid):
    """C values on a `grid`, mirrored about `centre`: their mean is exactly `centre` and every partial sum is exact in
    fp32, whatever the order of summation."""
    half = np.round(rng.standard_normal(C // 2) * spread / grid) * grid
    dev = np.concatenate([half, -half] + ([[0.0]] if C % 2 else []))
    return (centre + rng.permutation(dev)).astype(np.float32)


def ln_inputs(case, seed=0):
    """x [B, T, C] float32, gamma, beta.  Every row is mirrored about a centre that fp32 represents, on a dyadic grid:
    the row sums and the mean are then EXACT in fp32 in any summation order, and x - mean is exact too.  What is left of
    the kernel's fp32 arithmetic is relative noise of a few 2^-24 on (x - mean) * rstd * gamma, far inside the rounding
    bound; without this the bound would judge the rounding of the fp32 mean (|mean| 2^-24 absolute on every element, a
    large RELATIVE error on the elements near zero) rather than the kernel.  beta is small against gamma for the same
    reason: where (x - mean) * rstd * gamma and beta cancel, the fp32 rounding of the terms (2^-24 of THEIR size) is a
    relative error of the sum that no fp32 LayerNorm avoids; |beta| <= 0.008 stays below every |term| of the outlier row
    (>= 0.009 for C <= 2052) and makes such an element rare elsewhere.  The constant and the all-zero row still pin beta:
    they must come out as beta itself."""
    C = case["C"]
    rng = np.random.default_rng(2000 + C)
    x = np.stack([np.stack([_mirrored(rng, C, 0.5, 3.0, 2.0 ** -6) for _ in range(LN_T)]) for _ in range(LN_B)])
    x[0, LN_ROW_CONST] = 2.5                                   # LN of a constant row is beta
    x[0, LN_ROW_MEAN1E3] = _mirrored(rng, C, 1000.0, 1.0, 2.0 ** -3)   # E[x^2] - mean^2 in fp32 has no digits left here
    m = np.round(1e4 / C * 64) / 64                            # one outlier of C * m ~ 1e4 among N(0, 1) values that sum
    half = np.round(rng.standard_normal((C - 1) // 2) * 64) / 64      # to zero: the mean is m, exactly
    out = np.concatenate([[C * m], half, -half] + ([[0.0]] if C % 2 == 0 else []))
    x[0, LN_ROW_OUTLIER] = out.astype(np.float32)
    x[0, LN_ROW_ZERO] = 0.0
    gamma = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    beta = np.clip(0.004 * rng.standard_normal(C), -0.008, 0.008).astype(np.float32)
    return x.astype(np.float32), gamma, beta


# pio_layernorm_cast_cat: ONE kernel (float2 lanes over the virtual concatenation); the launcher's branches are the operand
# dtype, x2 per sample or one table, and its refusals
LNCAT_CASES = [
    dict(id="c64_258_table", C1=64, C2=258, table=True, x1_gap=0),          # (C1 + C2) % 4 != 0: the ImageNet shapes
    dict(id="c64_258_per_batch", C1=64, C2=258, table=False, x1_gap=0),
    dict(id="c6_2_strided_x1", C1=6, C2=2, table=True, x1_gap=6),            # x1 a column slice of a wider array
    dict(id="c1000_1040_table", C1=1000, C2=1040, table=True, x1_gap=0),     # 2040: c_pad 2040, the widest row
    dict(id="c64_192_mult4", C1=64, C2=192, table=False, x1_gap=2),          # (C1 + C2) % 4 == 0
]
LNCAT_REFUSED = [
    dict(id="c_pad_above_2048", C1=1026, C2=1026, c_pad=2056),
    dict(id="odd_c1", C1=63, C2=259, c_pad=328),
]

# ----------------------------------------------------------------------------------------------------
# pio_pack_linear
# ----------------------------------------------------------------------------------------------------
# (out, in, row_heads, col_heads); the last has per-head widths of 10, padded to 16
PACK_CASES = [(24, 40, 1, 1), (60, 36, 4, 1), (36, 60, 1, 4), (66, 322, 1, 1), (20, 20, 2, 2)]
PACK_K_EXTRA = 8      # k_pad = used columns + 8
PACK_LDW_EXTRA = 3    # ldw = in + 3, NaN behind `in`
PACK_ROW0 = 8         # dst_row0; the image has 16 more rows than the part
PACK_ROWS_EXTRA = 16


def pack_geometry(case):
    out, inn, rh, ch = case
    rows_p = rh * pad8(out // rh)
    cols_used = ch * pad8(inn // ch)
    return rows_p, cols_used, cols_used + PACK_K_EXTRA, inn + PACK_LDW_EXTRA, rows_p + PACK_ROWS_EXTRA


def pack_inputs(case):
    out, inn, _, _ = case
    rng = np.random.default_rng(3000 + out * inn)
    w = (rng.standard_normal((out, inn)) * 0.3).astype(np.float32)
    w[0, 0], w[-1, -1] = 3.0e-8, 60000.0        # half of fp16's smallest subnormal / close to its largest finite value
    bias = rng.standard_normal(out).astype(np.float32)
    return w, bias


# ----------------------------------------------------------------------------------------------------
# pio_bn_relu_maxpool_tokens
# ----------------------------------------------------------------------------------------------------
POOL_B = 2
POOL_C = (1, 64, 65, 100)
POOL_HW = ((1, 1), (2, 3), (7, 130), (5, 257))      # W = 257: OW = 129, more than one wave of output columns
POOL_PADS = ((0, 0), (0, 1), (1, 0), (1, 1))


def pool_inputs(C, H, W):
    """x [B, C, H, W], scale (negative on every third channel), shift.  The window of output (0, 0) of sample 1 holds
    only cells with x * scale + shift < 0 in every channel: it must come out as exactly 0."""
    rng = np.random.default_rng(4000 + C * 1000 + H * W)
    x = rng.standard_normal((POOL_B, C, H, W)).astype(np.float32) * 2
    scale = (0.5 + rng.random(C)).astype(np.float32)
    scale[::3] *= -1
    shift = (0.3 * rng.standard_normal(C)).astype(np.float32)
    sgn = np.sign(scale)[:, None, None]
    x[1, :, :3, :3] = (-(np.abs(x[1, :, :3, :3]) + 2.0) * sgn).astype(np.float32)     # |x * scale| >= 1 > |shift|
    return x, scale, shift


# ----------------------------------------------------------------------------------------------------
# block entry points with a workspace of exactly the promised size (shapes: the smallest of tests/test_attn_route_gpu.py
# that reach each route of pio_attention_fwd)
# ----------------------------------------------------------------------------------------------------
ATTN_WS_CASES = [
    # id, heads, qk channels, v channels, Tq, Tk, mask, fused-core launches, softmax_rows launches (None: >= 1)
    ("self_core", 2, 64, 64, 128, 128, None, 1, 0),
    ("cross_core_kv_mask_key_split", 2, 64, 64, 128, 512, "kv", 1, 0),      # 16 key tiles: two key splits
    ("tall_core", 1, 1024, 1024, 128, 96, None, 1, 0),
    ("materialised_full_mask", 2, 64, 64, 128, 128, "full", 0, None),
]
