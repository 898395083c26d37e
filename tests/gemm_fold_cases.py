"""Cases and float64 references for the LayerNorm FOLD of pio_gemm_nt (include/pio_hip.h, pio_gemm_t: X16, X16_lo, ld16,
row_part, row_slot_w, R16_hi, R16_lo, range_flag, ln_part, ln_slots, ln_c, ln_eps) on every kernel that runs it:
gemm_nt_wide (both producer epilogues, the consumer) and the six tile kernels of gemm_nt_128.

Numpy only; shared by tests/test_gemm_fold_host.py (CPU: routing through csrc/pio_gemm_route.h, coverage of the
(role, kernel, feature) matrix, every bound shown to hold for a float32 restatement) and tests/test_gemm_fold_gpu.py
(MI355X: the kernels on guarded, NaN-surrounded buffers).

A case is a dict of the fields that matter plus
    role      "prod" (row_part set) or "cons" (ln_part / ln_c set)
    override  value passed to pio_gemm_kernel_override
    kernel    the GemmKernel enumerator the launch must reach at its n_cu
    n_cu      256 (the default CU budget) or 8 (pio_set_cu_budget(8) around the launch)
    bias_off / part_off / lnc_off   element offsets of the bias / ln_part / ln_c pointers inside their 256-byte aligned payloads
    family    how the result is compared (below): derived from the fields (family_of)
    features  what the layout exercises (features_of: derived from the fields, never claimed by hand)

PRODUCER   x = alpha (A B^T [+ A B_lo^T] [+ A_lo B^T]) + bias + residual, residual = fp32 R or the pair R16_hi + R16_lo;
           X16 = rn(x), X16_lo = rn(x - X16), C = x (when given), row_part[m][s] = (sum, sum of squares) of x over slot s.
  int    every operand a small integer with |x| <= 256: x is a value of fp16 and of bf16, X16_lo is +0 bit for bit, and
         every slot sum is an integer below 2^24 -- exact in fp32 in any order.  Everything is compared BIT FOR BIT.  The
         residual pair has a non-zero lo half (hi: multiples of 8): a kernel that drops it fails.
  pair   x holds more bits than the type (fp16: multiples of 1/16 -- 1/32 under alpha = 1/2 -- up to 256; bf16: integers
         or halves up to 2048), still exact in fp32 in any order (exact_ok), so X16, X16_lo (both non-zero) and C are
         compared bit for bit.  The slot sums are not exact: row_part is compared with float64 within
             SUM_BOUND = slot_w * 2^-23 * sum |term|
         -- an fp32 sum of n terms in ANY order (sequential, tree, lanes then shuffles) is off by at most
         (n - 1) 2^-24 sum |term| (1 + O(2^-24)) and each square by one more rounding (none under an FMA): n 2^-24
         sum |term|; the factor two covers the second-order tail generously.
  range  the int family with ONE planted element (+inf in R16_hi, 1e20 in R, 1e20 in R16_hi) that makes one row's sum of
         squares non-finite: the flag word becomes 1, every OTHER row is still bit-exact (the planted row is not compared).
  Every other case starts with the flag word at 0 (must stay 0), one at 1 (must stay 1: the kernel ORs), one with NULL.

CONSUMER   (pio_hip.h) S, Q = sums of row m's ln_slots (sum, sum of squares) pairs; mean = S / K;
           var = max(Q / K - mean^2, 0); rstd = 1 / sqrt(var + eps); y = act(rstd (A B^T)[m,n] - rstd mean c[n] + bias[n]).
           ln_part and ln_c are INPUTS and hand-built: they need not come from a producer or from B.
  exact  K in {256, 512, 1024} (1 / K exact), eps = 0.25; per row an integer mean mu and j in {0, 1, 2}: S = K mu,
         Q = K (mu^2 + 4^j - 1/4), spread over the slots as DISTINCT integers (negative ones among them), so that a slot
         skipped, repeated or taken from the neighbouring row changes S or Q.  Then var + eps = 4^j and rstd = 2^-j exactly,
         and with integer A, B, c, bias every intermediate is a multiple of 1/4 far below 2^24: y is exact in fp32 with or
         without FMA contraction and in both orders the kernels use -- (v rs + nm c) + b on the tiles, a rs + (nm c + b)
         on the wide kernel.  16-bit C = rn(y), C_lo = rn(y - C): BIT FOR BIT, no tolerance.
  bounded  K in {768, 1280, 1536, 1664} (1 / K inexact), same construction, float64 of the definition as reference and
         CONS_BOUND (derived at cons_bound) per element.
  gelu   the exact family's construction with act = 1 and operands chosen so that every pre-activation is a multiple of
         1/4 in [-2, 8] (exact in fp32); reference = float64 erf-GELU of it; bound ULP |ref| + TINY + GELU_G.

UNREAD AND UNWRITTEN ELEMENTS -- the contract both tests hold the kernels to:
  NaN in the inputs (one stray read poisons a result or a statistic): the pitch columns of A, B, R16_* and R; rows of
  R16_* and ln_part behind M - 1; ln_c and bias entries behind N - 1 (and in front of an offset pointer); the slots behind
  ln_slots - 1 of the last row.
  Written: rows < M x columns < N of X16, X16_lo and C; row_part[m < M][s < N / w][2]; rows < M x columns < n_store of a
  consumer's C (and C_lo), [N, n_store) as +0; the flag word.  Everything else in every payload keeps its bits.
"""
import math
import zlib

import numpy as np

from primitive_cases import DTYPES, TINY, ULP, round_to  # noqa: F401  (re-exported for the two test files)

TILE_KERNELS = ("T128", "T128_KG2", "T64", "T64_KG2", "T32", "T32_KG2")
KERNELS = ("WIDE",) + TILE_KERNELS
TILE_OF = {"WIDE": (256, 256), "T128": (128, 128), "T128_KG2": (128, 128), "T64": (64, 64), "T64_KG2": (64, 64),
           "T32": (32, 64), "T32_KG2": (32, 64)}
TAIL = 8             # unread (NaN) / unwritten elements behind the last element of every payload
EPS = 0.25
U = 2.0 ** -24       # unit roundoff of fp32
# GELU_G: allowance for the fp32 evaluation of gelu_erf (csrc/pio_gemm_common.h: degree-7 polynomial around exp2).
# tests/test_gemm_fold_host.py restates the polynomial in numpy float32 with np.exp2 and measures its largest deviation
# from float64 erf-GELU over every gelu case's pre-activations: 1.27e-7 (at x = 4.25).  Four times that: the hardware exp2
# is accurate to about one ulp rather than correctly rounded, and the FMAs may contract differently.
GELU_MEASURED = 1.3e-7
GELU_G = 4 * GELU_MEASURED

PROD_FEATURES = ("ld16_pitch", "c_null", "c_given", "ldc_pitch", "in_place", "res_pair_separate", "res_f32", "ragged_m",
                 "half_tile_n", "two_tiles_per_wg", "bias_none", "bias_unaligned", "alpha", "b_lo", "a_lo", "flag_set",
                 "flag_clear", "flag_null")
CONS_FEATURES = ("slots_128", "slots_64", "slots_gt8", "slots_le8", "slots_gt24", "ln_part_8B", "ln_c_unaligned", "ragged_n",
                 "n_store_pad", "ldc_pitch", "lda_pitch", "ragged_m", "act", "c_lo", "bias_none", "bias_unaligned", "b_lo")
# beside the matrix: the comparison family and the forms the matrix cannot name
EXTRAS = ("int", "pair", "range", "exact", "bounded", "gelu", "x_lo_null", "ln_part_4B", "staged", "direct", "staged_only",
          "two_tiles_whole", "two_tiles_ragged", "range_hi_inf", "range_r_1e20", "range_hi_1e20") + \
    tuple(f"slots_{n}" for n in range(2, 13, 2))


def persistent_grid(tiles, n_cu):
    g = min(tiles, n_cu)
    return g & ~7 if g >= 8 else g


def family_of(c):
    if c["role"] == "prod":
        return "range" if c["plant"] else ("pair" if c["pair"] else "int")
    if c["act"]:
        return "gelu"
    return "exact" if c["K"] in (256, 512, 1024) else "bounded"


def features_of(c):
    tm, tn = TILE_OF[c["kernel"]]
    wide = c["kernel"] == "WIDE"
    f = set()
    if c["M"] % tm:
        f.add("ragged_m")
    if not c["bias"]:
        f.add("bias_none")
    elif c["bias_off"] % 4:
        f.add("bias_unaligned")
    if c["b_lo"]:
        f.add("b_lo")
    if c["role"] == "prod":
        if c["ld16"] > c["N"]:
            f.add("ld16_pitch")
        f.add("c_given" if c["c"] else "c_null")
        if c["c"] and c["ldc"] > c["N"]:
            f.add("ldc_pitch")
        f.add({"inplace": "in_place", "pair": "res_pair_separate", "f32": "res_f32"}[c["res"]])
        if wide and c["N"] % 256 == 128:
            f.add("half_tile_n")
        tiles = -(-c["M"] // 256) * -(-c["N"] // 256)
        if wide and not c["c"] and c["x_lo"] and c["res"] != "f32" and tiles >= 2 * persistent_grid(tiles, c["n_cu"]):
            f.add("two_tiles_per_wg")
        if c["alpha"] != 1.0:
            f.add("alpha")
        if c["a_lo"]:
            f.add("a_lo")
        f.add("flag_" + c["flag"])
    else:
        if c["K"] % 128 == 0 and c["ln_slots"] == c["K"] // 128:
            f.add("slots_128")
        if c["ln_slots"] == c["K"] // 64:
            f.add("slots_64")
        if wide:
            f.add("slots_gt8" if c["ln_slots"] > 8 else "slots_le8")
        elif c["ln_slots"] > 24:
            f.add("slots_gt24")
        if c["part_off"] % 4 == 2:
            f.add("ln_part_8B")
        if c["lnc_off"] % 4:
            f.add("ln_c_unaligned")
        if c["N"] % tn:
            f.add("ragged_n")
        if c["n_store"] > c["N"]:
            f.add("n_store_pad")
        if c["ldc"] > c["n_store"]:
            f.add("ldc_pitch")
        if c["lda"] > c["K"]:
            f.add("lda_pitch")
        if c["act"]:
            f.add("act")
        if c["c_lo"]:
            f.add("c_lo")
    return frozenset(f)


def extras_of(c):
    e = {family_of(c)}
    if c["role"] == "prod":
        if not c["x_lo"]:
            e.add("x_lo_null")
        if c["kernel"] == "WIDE":
            # the staged epilogue: no fp32 C, the pair out, the 16-bit residual pair, an interior tile that is its
            # workgroup's last; every other tile leaves through the direct one
            stg = not c["c"] and c["x_lo"] and c["res"] != "f32"
            tiles = -(-c["M"] // 256) * -(-c["N"] // 256)
            interior = (c["M"] // 256) * (c["N"] // 256)
            if stg and interior:
                e.add("staged")
            if not stg or interior < tiles or tiles > persistent_grid(tiles, c["n_cu"]):
                e.add("direct")
            if "two_tiles_per_wg" in features_of(c):     # whole tiles: every workgroup runs direct, then staged
                e.add("two_tiles_ragged" if c["M"] % 256 or c["N"] % 256 else "two_tiles_whole")
            if "staged" in e and "direct" not in e:
                e.add("staged_only")
        if c["plant"]:
            e.add("range_" + c["plant"][0])
    elif c["kernel"] == "WIDE":
        e.add(f"slots_{c['ln_slots']}")
    if c["role"] == "cons" and c["part_off"] % 2:
        e.add("ln_part_4B")
    return frozenset(e)


def _finish(c):
    c["family"] = family_of(c)
    c["features"] = features_of(c)
    c["extras"] = extras_of(c)
    return c


def _prod(cid, kernel, override, M, N, K, **kw):
    """Producer, defaults = the dense in-place form of the blocks (R16_* == X16*, no fp32 C, 128-column slots)."""
    c = dict(id=cid, role="prod", kernel=kernel, override=override, n_cu=256, M=M, N=N, K=K, slot_w=128, alpha=1.0,
             bias=True, bias_off=0, a_lo=False, b_lo=False, c=False, res="inplace", x_lo=True, flag="clear", plant=None,
             pair=False, act=0, n_store=N)
    c.update(kw)
    for k, v in (("lda", K), ("ldb", K), ("ld16", N), ("ldc", N), ("ldr", N)):
        c.setdefault(k, v)
    return _finish(c)


def _cons(cid, kernel, override, M, N, K, **kw):
    """Consumer, defaults = the dense layout with K / 128 slots."""
    c = dict(id=cid, role="cons", kernel=kernel, override=override, n_cu=256, M=M, N=N, K=K, ln_slots=K // 128, part_off=0,
             lnc_off=0, n_store=N, act=0, c_lo=False, bias=True, bias_off=0, a_lo=False, b_lo=False, alpha=1.0)
    c.update(kw)
    for k, v in (("lda", K), ("ldb", K), ("ldc", c["n_store"])):
        c.setdefault(k, v)
    return _finish(c)


# ----------------------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------------------
# shapes that reach each tile kernel on 256 CUs (csrc/pio_gemm_route.h: tiles per CU; two K teams from K = 1024 on when
# the grid fits the CUs; overrides 64 / 128 force the tile and switch the teams off): (override, M, N of a producer,
# N of a consumer, K of the exact family)
TILE_SHAPES = {
    "T32": (0, 70, 128, 70, 256), "T32_KG2": (0, 70, 128, 70, 1024),
    "T64": (64, 150, 128, 70, 512), "T64_KG2": (0, 830, 896, 890, 1024),
    "T128": (128, 300, 192, 134, 256), "T128_KG2": (0, 1660, 1920, 1914, 1024),
}


def _tile_cases():
    out = []
    for i, k in enumerate(TILE_KERNELS):
        ov, M, Np, Nc, K = TILE_SHAPES[k]
        t = k.lower()
        Kp = K if k.endswith("KG2") else 64
        # producer: the blocks' in-place form, dense bias-free; and everything else at once
        out.append(_prod(f"{t}_p_inplace", k, ov, M, Np, Kp, slot_w=64, ld16=Np + 4, bias=False))
        out.append(_prod(f"{t}_p_sep", k, ov, M, Np, Kp, slot_w=64, res="pair", c=True, ldc=Np + 4, bias_off=1, alpha=0.5,
                         pair=True, flag="set" if i % 2 else "null"))
        # consumer: K / 64 slots 8 bytes off, every pitch and pad, unaligned column constants, the hi + lo result
        ns = Nc + 2
        out.append(_cons(f"{t}_c_edges", k, ov, M, Nc, K, ln_slots=K // 64, part_off=2, lnc_off=1, bias_off=3, n_store=ns,
                         ldc=ns + 3, lda=K + 8, c_lo=True))
        # ... 26 slots (the loop path), 4 bytes off, no bias
        out.append(_cons(f"{t}_c_loop", k, ov, M, Nc, K, ln_slots=26, part_off=1, bias=False))
        # ... K / 128 slots, GELU
        out.append(_cons(f"{t}_c_gelu", k, ov, M, Nc, K, act=1))
    return out


CASES = [
    # ---- gemm_nt_wide, producer (128-column slots, no row minimum).  One tile per workgroup on 256 CUs: the staged
    # epilogue on interior tiles when there is no fp32 C, the direct one everywhere else.
    _prod("wp_staged", "WIDE", 0, 512, 256, 128, ld16=264),                                   # 2 interior tiles: staged
    _prod("wp_half_ragged", "WIDE", 0, 300, 384, 128, ld16=392, c=True, ldc=392, flag="set"),  # direct; N = 1.5 tiles
    _prod("wp_two_tiles", "WIDE", 0, 512, 2048, 128, n_cu=8, ld16=2056),           # 16 tiles on 8 workgroups: direct, staged
    _prod("wp_two_tiles_ragged", "WIDE", 0, 500, 2048, 128, n_cu=8, ld16=2056, bias=False),   # ... the last tile row ragged
    _prod("wp_res_f32", "WIDE", 0, 300, 128, 128, res="f32", ldr=132, c=True, a_lo=True, b_lo=True, alpha=2.0, flag="null"),
    _prod("wp_res_f32_b_lo", "WIDE", 0, 300, 256, 128, res="f32", x_lo=False, c=True, b_lo=True, pair=True),
    _prod("wp_sep_b_lo", "WIDE", 0, 300, 128, 128, res="pair", b_lo=True, pair=True, alpha=0.5),
    _prod("wp_range_hi_inf", "WIDE", 0, 300, 256, 128, plant=("hi_inf", 40, 130)),            # staged tile, +inf in R16_hi
    _prod("wp_range_r_1e20", "WIDE", 0, 300, 128, 128, res="f32", c=True, plant=("r_1e20", 299, 127)),
    _prod("t64_p_range_hi_1e20", "T64", 64, 150, 128, 64, slot_w=64, plant=("hi_1e20", 149, 64)),
    # ---- gemm_nt_wide, consumer (from 2048 rows; K / 128 slots, an even number of them)
    _cons("wc_k256", "WIDE", 0, 2100, 264, 256, n_store=272, ldc=280, lda=264),               # 2 slots
    _cons("wc_k512_b_lo", "WIDE", 0, 2100, 256, 512, b_lo=True, bias=False),
    _cons("wc_k1024_gelu", "WIDE", 0, 2100, 136, 1024, act=1),                                # 8 slots: part full, part2 empty
    _cons("wc_k768", "WIDE", 0, 2100, 128, 768),                                              # 6 slots
    _cons("wc_k1280", "WIDE", 0, 2100, 128, 1280, bias=False),                                # 10: part2 half full
    _cons("wc_k1536", "WIDE", 0, 2100, 264, 1536, n_store=272, ldc=280),                      # 12
    # ---- the tile kernels: bounded cases beside the table below
    _cons("t32kg2_c_k1664", "T32_KG2", 0, 70, 70, 1664, ln_slots=26, part_off=2),  # 26 slots of 64: the loop path
    _cons("t64_c_k768", "T64", 64, 150, 70, 768, ln_slots=12, lnc_off=1),
] + _tile_cases()
BY_ID = {c["id"]: c for c in CASES}

# Two or three CONSISTENT cases (CPU only): ln_part from the rows of A, ln_c[n] = sum_k B[n, k]; the host test compares the
# reference with torch float64 layer_norm(x) @ W.T + b.
CONSISTENT = [dict(id="consistent_128", M=37, N=24, K=256, slot_w=128), dict(id="consistent_64", M=21, N=40, K=192, slot_w=64),
              dict(id="consistent_gelu", M=19, N=16, K=128, slot_w=64, act=1)]


def _variant(role, kernel, feature, base, expect, **change):
    """`base` with `change` applied: a descriptor that asks `kernel` (the base case's kernel) for `feature`."""
    cid = f"{kernel.lower()}_{role}_no_{feature}"
    if base not in BY_ID:
        return dict(id=cid, role=role, kernel=kernel, expect=expect, feature=feature, base=base, missing_base=True,
                    features=frozenset(), extras=frozenset(), n_cu=256)
    c = dict(BY_ID[base])
    c.update(change)
    c.update(id=cid, kernel=kernel, expect=expect, feature=feature, base=base)
    c["family"], c["features"], c["extras"] = family_of(c), features_of(c), extras_of(c)
    assert c["role"] == role and (feature in c["features"] or feature in NOT_A_FEATURE), (cid, sorted(c["features"]))
    return c


# refusals that are no cell of the matrix (no feature names them) but that the issue names
NOT_A_FEATURE = ("slot128_n_not_128", "slots_odd")

# (role, kernel, feature) the predicates turn away with an error code: the launch never happens.
REFUSED = [
    # gemm_wide_ok: the bias is fetched by 16-byte DMAs
    _variant("prod", "WIDE", "bias_unaligned", "wp_staged", "PIO_E_SHAPE", bias_off=1),
    # 128-column slots on an N that is no multiple of 128
    _variant("prod", "WIDE", "slot128_n_not_128", "wp_staged", "PIO_E_SHAPE", N=192, n_store=192, ld16=200),
]
for _k in TILE_KERNELS:
    _b = f"{_k.lower()}_p_inplace"
    REFUSED += [
        # the small-tile producer takes the 16-bit residual pair only, and one K sweep
        _variant("prod", _k, "res_f32", _b, "PIO_E_SHAPE", res="f32", c=True),
        _variant("prod", _k, "b_lo", _b, "PIO_E_SHAPE", b_lo=True),
        _variant("prod", _k, "a_lo", _b, "PIO_E_SHAPE", a_lo=True),
        _variant("cons", _k, "b_lo", f"{_k.lower()}_c_loop", "PIO_E_SHAPE", b_lo=True),
    ]

# ... that the predicates hand to ANOTHER kernel: what gemm_wide_ok does not take of a wide-shaped consumer runs on a tile
# kernel (2100 x 264: 165 tiles of 64 x 64 -> the 32 x 64 tile)
REROUTED = [
    _variant("cons", "WIDE", "ln_c_unaligned", "wc_k256", "T32", lnc_off=1),
    _variant("cons", "WIDE", "ln_part_8B", "wc_k256", "T32", part_off=2),
    _variant("cons", "WIDE", "bias_unaligned", "wc_k256", "T32", bias_off=1),
    _variant("cons", "WIDE", "c_lo", "wc_k256", "T32", c_lo=True),
    _variant("cons", "WIDE", "slots_64", "wc_k256", "T32", ln_slots=4),
    _variant("cons", "WIDE", "slots_odd", "wc_k256", "T32", K=384, lda=392, ln_slots=3),
]


def required_cells():
    """Every (role, kernel, feature) the predicates admit; "ANY" = once on some kernel of the group (the pre-set and the
    NULL flag word differ from the cleared one in the pointer's target alone, not in the code that runs)."""
    cells = set()
    tile_p = set(PROD_FEATURES) - {"res_f32", "half_tile_n", "two_tiles_per_wg", "b_lo", "a_lo", "flag_set", "flag_null"}
    wide_p = set(PROD_FEATURES) - {"bias_unaligned", "flag_set", "flag_null"}
    tile_c = set(CONS_FEATURES) - {"slots_gt8", "slots_le8", "b_lo"}
    wide_c = set(CONS_FEATURES) - {"slots_64", "slots_gt24", "ln_part_8B", "ln_c_unaligned", "c_lo", "bias_unaligned"}
    cells |= {("prod", "WIDE", f) for f in wide_p} | {("cons", "WIDE", f) for f in wide_c}
    for k in TILE_KERNELS:
        cells |= {("prod", k, f) for f in tile_p} | {("cons", k, f) for f in tile_c}
    cells |= {("prod", g, f) for g in ("ANY_WIDE", "ANY_TILE") for f in ("flag_set", "flag_null")}
    # the comparison families and the forms beside the matrix
    cells |= {("prod", "WIDE", e) for e in ("int", "pair", "range", "staged", "direct", "x_lo_null", "staged_only",
                                            "two_tiles_whole", "two_tiles_ragged", "range_hi_inf", "range_r_1e20")}
    cells |= {("cons", "WIDE", e) for e in ("exact", "bounded", "gelu")} | {("cons", "WIDE", f"slots_{n}") for n in range(2, 13, 2)}
    for k in TILE_KERNELS:
        cells |= {("prod", k, "int"), ("prod", k, "pair"), ("cons", k, "exact"), ("cons", k, "gelu"), ("cons", k, "ln_part_4B")}
    cells |= {("prod", "T64", "range_hi_1e20"), ("cons", "T32_KG2", "bounded"), ("cons", "T64", "bounded")}
    return cells


def provides(c):
    out = {(c["role"], c["kernel"], f) for f in c["features"] | c["extras"]}
    grp = "ANY_WIDE" if c["kernel"] == "WIDE" else "ANY_TILE"
    out |= {(c["role"], grp, f) for f in c["features"] if f in ("flag_set", "flag_null")}
    return out & required_cells()


# ----------------------------------------------------------------------------------------------------
# buffers
# ----------------------------------------------------------------------------------------------------
def _rng(c):
    return np.random.default_rng(zlib.crc32(c["id"].encode()))


def _matrix(rows, ld, cols, values):
    """flat payload of a [rows, cols] matrix with row pitch ld: pitch columns and TAIL are NaN"""
    buf = np.full(rows * ld + TAIL, np.nan, dtype=np.float32)
    buf[:rows * ld].reshape(rows, ld)[:, :cols] = values
    return buf


def _view(buf, rows, ld, cols, off=0):
    return buf[off:off + rows * ld].reshape(rows, ld)[:, :cols]


def _vector(off, n, values):
    buf = np.full(off + n + TAIL, np.nan, dtype=np.float32)
    buf[off:off + n] = values
    return buf


def _sparse_rows(rng, rows, K, nnz, values):
    """[rows, K]: nnz entries of `values` per row, zeros elsewhere"""
    out = np.zeros((rows, K), dtype=np.float32)
    cols = np.argsort(rng.random((rows, K)), axis=1)[:, :nnz]
    out[np.arange(rows)[:, None], cols] = rng.choice(values, (rows, nnz))
    return out


def make_arrays(c, dt):
    """Inputs as flat float32 payloads, every value exact in `dt`; unread elements are NaN (see the module docstring)."""
    return _prod_arrays(c, dt) if c["role"] == "prod" else _cons_arrays(c)


def _prod_arrays(c, dt):
    rng = _rng(c)
    M, N, K = c["M"], c["N"], c["K"]
    # int family: grid 1, |x| <= 3 * 12 * 2 * 2 + 8 + 64 + 3 = 219.  pair family (at most two sweeps): fp16 bias / lo on a
    # 1/16 grid, |hi| in [128, 176], |x| <= 48 + 8 + 176 + 3 = 235; bf16 everything eight times larger -- integers up to 1880
    fine = 1.0 / 16 if (c["pair"] and dt == "f16") else 1.0
    big = 8.0 if (c["pair"] and dt == "bf16") else 1.0
    bvals = np.array([-2, -1, 1, 2], dtype=np.float32) * big
    out = {}
    for name, on in (("A", True), ("A_lo", c["a_lo"])):
        out[name] = _matrix(M, c["lda"], K, rng.integers(-1, 2, (M, K))) if on else None
    for name, on in (("B", True), ("B_lo", c["b_lo"])):
        out[name] = _matrix(N, c["ldb"], K, _sparse_rows(rng, N, K, 12, bvals)) if on else None
    kb, klo = rng.integers(-128, 129, N), rng.integers(-48, 49, (M, N))
    if fine < 1:
        b, lo = kb / 16.0, klo / 16.0                    # multiples of 1/16 in [-8, 8] and [-3, 3]
    elif big > 1:
        b, lo = np.rint(kb / 2.0), np.rint(klo / 2.0)    # integers in [-64, 64] and [-24, 24]
    else:
        b, lo = np.rint(kb / 16.0), np.rint(klo / 16.0)  # integers in [-8, 8] and [-3, 3] ...
        lo[lo == 0] = 1.0                                # ... the lo half never zero
    out["bias"] = _vector(c["bias_off"], N, b) if c["bias"] else None
    hi = rng.integers(-8, 9, (M, N)) * 8.0
    if c["pair"]:   # |x| mostly in [128, 256) (bf16: [1024, 2048)), where the type's ulp is coarser than the grid of x
        hi = rng.choice([-1.0, 1.0], (M, N)) * (128.0 + 8.0 * rng.integers(0, 7, (M, N))) * big
    out["R"] = out["R_hi"] = out["R_lo"] = None
    if c["res"] == "f32":
        out["R"] = _matrix(M, c["ldr"], N, hi + lo)
    else:
        out["R_hi"], out["R_lo"] = _matrix(M, c["ld16"], N, hi), _matrix(M, c["ld16"], N, lo)
    if c["plant"]:
        what, m, n = c["plant"]
        if what == "hi_inf":
            _view(out["R_hi"], M, c["ld16"], N)[m, n] = np.inf
        elif what == "r_1e20":
            _view(out["R"], M, c["ldr"], N)[m, n] = 1e20
        else:
            _view(out["R_hi"], M, c["ld16"], N)[m, n] = round_to(dt, np.float32(1e20))
    return out


def _spread(rng, total, ns):
    """[M] integer totals -> [M, ns] DISTINCT integers per row (negative ones among them) with that sum"""
    M = len(total)
    pool = np.tile(np.arange(-2000, 2001, dtype=np.int64), (M, 1))
    first = rng.permuted(pool, axis=1)[:, :ns - 1]
    for _ in range(64):
        last = total - first.sum(axis=1)
        clash = (first == last[:, None]).any(axis=1)
        if not clash.any():
            break
        first[clash, 0] += 4001          # (outside the pool: distinct from every other slot)
    out = np.concatenate([first, last[:, None]], axis=1)
    assert all(len(set(r)) == ns for r in out[:64]) and (out < 0).any()
    return out


def _cons_arrays(c):
    rng = _rng(c)
    M, N, K, ns = c["M"], c["N"], c["K"], c["ln_slots"]
    gelu = bool(c["act"])
    out = {"A_lo": None}
    if gelu:   # pre-activation = rstd (acc - mu c) + b in [-2, 8]: |acc| <= 2, |mu c| <= 1, b in [1, 5]
        assert not c["b_lo"] and c["bias"]
        A, B = _sparse_rows(rng, M, K, 2, np.array([-1, 1], dtype=np.float32)), rng.integers(-1, 2, (N, K))
        mu, cn, b = rng.integers(-1, 2, M), rng.integers(-1, 2, N), rng.integers(1, 6, N)
    else:
        A, B = rng.integers(-3, 4, (M, K)), rng.integers(-3, 4, (N, K))
        mu, cn, b = rng.integers(-3, 4, M), rng.integers(-4, 5, N), rng.integers(-8, 9, N)
    out["A"], out["B"] = _matrix(M, c["lda"], K, A), _matrix(N, c["ldb"], K, B)
    out["B_lo"] = _matrix(N, c["ldb"], K, rng.integers(-1, 2, (N, K))) if c["b_lo"] else None
    out["bias"] = _vector(c["bias_off"], N, b) if c["bias"] else None
    out["ln_c"] = _vector(c["lnc_off"], N, cn)
    j = rng.integers(0, 3, M)
    S = K * mu.astype(np.int64)
    Q = (K // 4) * (4 * mu.astype(np.int64) ** 2 + 4 * 4 ** j - 1)        # K (mu^2 + 4^j - 1/4)
    part = np.stack([_spread(rng, S, ns), _spread(rng, Q, ns)], axis=2)   # [M, ns, 2]
    out["ln_part"] = _vector(c["part_off"], M * ns * 2, part.reshape(-1))
    out["mu"], out["j"] = mu, j
    return out


# ----------------------------------------------------------------------------------------------------
# references (float64)
# ----------------------------------------------------------------------------------------------------
def _acc(c, a, f=lambda v: v.astype(np.float64)):
    M, N, K = c["M"], c["N"], c["K"]
    A, B = f(_view(a["A"], M, c["lda"], K)), f(_view(a["B"], N, c["ldb"], K))
    acc = A @ B.T
    if c["b_lo"]:
        acc += A @ f(_view(a["B_lo"], N, c["ldb"], K)).T
    if c["a_lo"]:
        acc += f(_view(a["A_lo"], M, c["lda"], K)) @ B.T
    return acc


def ref_producer(c, a, magnitude=False):
    """-> (x [M, N], sums [M, N / w, 2]) in float64; magnitude=True: the same over absolute values (the bounds)."""
    M, N, w = c["M"], c["N"], c["slot_w"]
    f = (lambda v: np.abs(v.astype(np.float64))) if magnitude else (lambda v: v.astype(np.float64))
    x = abs(c["alpha"]) * _acc(c, a, f) if magnitude else c["alpha"] * _acc(c, a)
    if c["bias"]:
        x = x + f(a["bias"][c["bias_off"]:c["bias_off"] + N])[None, :]
    if c["res"] == "f32":
        x = x + f(_view(a["R"], M, c["ldr"], N))
    else:
        x = x + f(_view(a["R_hi"], M, c["ld16"], N)) + f(_view(a["R_lo"], M, c["ld16"], N))
    x = x + 0.0
    xs = x.reshape(M, N // w, w)
    return x, np.stack([xs.sum(axis=2), (xs * xs).sum(axis=2)], axis=2)


def sum_bound(c, a):
    """[M, N / w, 2]: slot_w * 2^-23 * sum |term| (module docstring) for the sum and the sum of squares of every slot"""
    x = ref_producer(c, a)[0]
    xs = np.abs(x).reshape(c["M"], c["N"] // c["slot_w"], c["slot_w"])
    return c["slot_w"] * 2.0 ** -23 * np.stack([xs.sum(axis=2), (xs * xs).sum(axis=2)], axis=2)


def _erf_gelu(x):
    vals, inv = np.unique(x, return_inverse=True)
    g = np.array([0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0))) for v in vals])
    return g[inv].reshape(x.shape)


def cons_stats(c, a):
    """float64 (S, Q, mean, var + eps, rstd) per row from the ln_part payload"""
    M, ns, K = c["M"], c["ln_slots"], c["K"]
    part = a["ln_part"][c["part_off"]:c["part_off"] + M * ns * 2].astype(np.float64).reshape(M, ns, 2)
    S, Q = part[:, :, 0].sum(axis=1), part[:, :, 1].sum(axis=1)
    mean = S / K
    w = np.maximum(Q / K - mean * mean, 0.0) + EPS
    return S, Q, mean, w, 1.0 / np.sqrt(w)


def ref_consumer(c, a):
    """-> (y [M, n_store] float64 with [N, n_store) = 0, pre [M, N] the pre-activation, terms (T1, T2, b))"""
    M, N = c["M"], c["N"]
    _, _, mean, _, rstd = cons_stats(c, a)
    cn = a["ln_c"][c["lnc_off"]:c["lnc_off"] + N].astype(np.float64)
    b = a["bias"][c["bias_off"]:c["bias_off"] + N].astype(np.float64) if c["bias"] else np.zeros(N)
    t1, t2 = rstd[:, None] * _acc(c, a), (rstd * mean)[:, None] * cn[None, :]
    pre = t1 - t2 + b[None, :]
    y = np.zeros((M, c["n_store"]))
    y[:, :N] = (_erf_gelu(pre) if c["act"] else pre) + 0.0
    return y, pre, (np.abs(t1), np.abs(t2), np.abs(b)[None, :] + 0 * t1)


def cons_bound(c, a, dt):
    """Per-element bound of the BOUNDED family, u = 2^-24.  S and Q are integers below 2^24: exact sums.  The device has
    ik = fl(1 / K) (relative error u), mean^ = fl(S ik) (2 u), q^ = fl(Q ik) (2 u), var^ = fl(q^ - mean^2) with or without
    a fused product: |var^ - var| <= 2 u Q/K + 5 u mu^2 + u var <= 5 u (Q/K + mu^2) + u w, and w^ = fl(var^ + eps) one more
    u w, with w = var + eps.  rstd = 1 / sqrt(w): half the relative error of w plus the square root and the division, each
    allowed 2 u (about one ulp, not necessarily correctly rounded):
        rho = 2.5 u (Q/K + mu^2) / w + 5 u.
    nm^ = fl(-mean^ rstd^): rho + 3 u.  y^ = (T1^ + T2^) + b in either order, T1 = rstd acc, T2 = rstd mu c: products
    rho + u and rho + 4 u, two additions of at most u (|T1| + |T2| + |b|) each (FMA contraction only removes roundings):
        |y^ - y| <= E = 13 u (|T1| + |T2| + |b|)  +  2.5 u (Q/K + mu^2) / w * (|T1| + |T2|)
    and the rounding to the type adds ULP (|y| + E) + TINY.  The rows keep (Q/K + mu^2) / w <= 2 mu^2 / 4^j + 1 <= 19."""
    S, Q, mean, w, _ = cons_stats(c, a)
    y, _, (t1, t2, b) = ref_consumer(c, a)
    amp = (Q / c["K"] + mean * mean) / w
    assert amp.max() <= 19.0
    E = 13 * U * (t1 + t2 + b) + 2.5 * U * amp[:, None] * (t1 + t2)
    out = np.zeros_like(y)
    out[:, :c["N"]] = E * (1 + ULP[dt]) + ULP[dt] * np.abs(y[:, :c["N"]]) + TINY[dt]
    return out


def gelu_bound(c, y, dt):
    out = ULP[dt] * np.abs(y) + TINY[dt] + GELU_G
    out[:, c["N"]:] = 0.0
    return out


def exact_ok(c, a, dt):
    """The premises of the bit-for-bit comparisons (module docstring), asserted; True when the case's family needs none."""
    M, N, K = c["M"], c["N"], c["K"]
    if c["role"] == "prod":
        if c["plant"]:       # the int family around one planted element: judge the case without it
            a = dict(a)
            for k in ("R", "R_hi"):
                if a[k] is not None:
                    a[k] = np.where(np.isfinite(a[k]) & (np.abs(a[k]) < 1e19), a[k], np.where(np.isnan(a[k]), np.nan, 8.0)).astype(np.float32)
        mag, msum = ref_producer(c, a, magnitude=True)
        x, sums = ref_producer(c, a)
        q = 1.0 / 32      # every term is a multiple of q and the sum of magnitudes / q < 2^24: exact in any order
        ok = c["alpha"] in (0.5, 1.0, 2.0) and bool(np.isfinite(mag).all()) and mag.max() / q < 2.0 ** 24
        ok = ok and bool((x == np.rint(x / q) * q).all())
        if c["family"] in ("int", "range"):
            ok = ok and bool((x == np.rint(x)).all()) and np.abs(x).max() <= 256 and msum.max() < 2.0 ** 24
            ok = ok and all(bool((round_to(d, x.astype(np.float32)) == x).all()) for d in DTYPES)
        else:
            hi = round_to(dt, x.astype(np.float32))
            lo = round_to(dt, x.astype(np.float32) - hi)
            ok = ok and np.abs(x).max() <= (256 if dt == "f16" else 2048) and bool((hi + lo.astype(np.float64) == x).all())
            ok = ok and (lo != 0).mean() > 0.25
        return bool(ok)
    if c["family"] == "bounded":
        return True
    S, Q, mean, w, rstd = cons_stats(c, a)
    part = a["ln_part"][c["part_off"]:c["part_off"] + M * c["ln_slots"] * 2].astype(np.float64)
    ok = K in (256, 512, 1024) and bool((part == np.rint(part)).all()) and np.abs(part).reshape(M, -1).sum(axis=1).max() < 2.0 ** 24
    ok = ok and bool((mean == a["mu"]).all()) and bool((w == 4.0 ** a["j"]).all()) and bool((rstd == 0.5 ** a["j"]).all())
    y, pre, (t1, t2, b) = ref_consumer(c, a)
    ok = ok and bool((pre == np.rint(pre * 4) / 4).all()) and (4 * (t1 + t2 + b)).max() < 2.0 ** 24
    if c["act"]:
        ok = ok and pre.min() >= -2.0 and pre.max() <= 8.0
    return bool(ok)


def expected_producer(c, a, dt):
    """float32 images the kernel must store: (X16, X16_lo, C, row_part [M, N / w, 2]) -- row_part as float64 sums"""
    x, sums = ref_producer(c, a)
    x32 = x.astype(np.float32)
    hi = round_to(dt, x32)
    return hi, round_to(dt, x32 - hi), x32, sums


def expected_consumer(c, y, dt):
    y32 = y.astype(np.float32)
    hi = round_to(dt, y32)
    return hi, (round_to(dt, y32 - hi) if c["c_lo"] else None)


# ----------------------------------------------------------------------------------------------------
# float32 restatements (the host test shows that every bound holds for them)
# ----------------------------------------------------------------------------------------------------
def f32_sums_three_orders(x):
    """x [M, S, w] float64 (exact in fp32) -> three [M, S, 2] float32 results: forward, reverse, pairwise"""
    x = x.astype(np.float32)
    out = []
    for order in ("fwd", "rev", "pair"):
        v = x[..., ::-1] if order == "rev" else x
        if order == "pair":
            s, q = v.copy(), v * v
            while s.shape[-1] > 1:
                s, q = s[..., 0::2] + s[..., 1::2], q[..., 0::2] + q[..., 1::2]
            out.append(np.stack([s[..., 0], q[..., 0]], axis=-1))
        else:
            s, q = np.zeros(v.shape[:-1], np.float32), np.zeros(v.shape[:-1], np.float32)
            for i in range(v.shape[-1]):
                s, q = s + v[..., i], q + v[..., i] * v[..., i]
            out.append(np.stack([s, q], axis=-1))
    return out


def f32_consumer_two_orders(c, a):
    """The consumer's formula in numpy float32, in the tile kernels' order and in the wide kernel's: [2][M, N]"""
    f = np.float32
    M, N, ns, K = c["M"], c["N"], c["ln_slots"], c["K"]
    part = a["ln_part"][c["part_off"]:c["part_off"] + M * ns * 2].reshape(M, ns, 2)
    sm, sq = np.zeros(M, f), np.zeros(M, f)
    for i in range(ns):
        sm, sq = sm + part[:, i, 0], sq + part[:, i, 1]
    ik = f(1.0) / f(K)
    mean = sm * ik
    var = np.maximum(sq * ik - mean * mean, f(0))
    rs = f(1.0) / np.sqrt(var + f(EPS))
    nm = -mean * rs
    acc = _acc(c, a).astype(f)
    cn = a["ln_c"][c["lnc_off"]:c["lnc_off"] + N]
    b = a["bias"][c["bias_off"]:c["bias_off"] + N] if c["bias"] else np.zeros(N, f)
    tile = (acc * rs[:, None] + nm[:, None] * cn[None, :]) + b[None, :]
    wide = acc * rs[:, None] + (nm[:, None] * cn[None, :] + b[None, :])
    assert tile.dtype == f and wide.dtype == f
    return tile, wide


def f32_gelu(x):
    """gelu_erf of csrc/pio_gemm_common.h in numpy float32 (np.exp2 for the hardware exp2)"""
    f = np.float32
    x = x.astype(f)
    a = np.minimum(np.abs(x), f(6.0))
    q = np.full(x.shape, 3.152013050566893e-06, f)
    for k in (2.9346412588893145e-07, -0.0006359288236126304, 0.007810706272721291, -0.05312380567193031,
              -0.45892834663391113, -1.15116286277771, -0.9999961256980896):
        q = q * a + f(k)
    return -np.abs(x) * np.exp2(q) + np.maximum(x, f(0))
