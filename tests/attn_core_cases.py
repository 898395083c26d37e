"""Cases, probes and the float64 reference for the three fused attention cores (numpy only):

    flash_attn_kernel  (csrc/pio_flash.hip,  pio_flash_attention / pio_flash_attention_pair core 1)   key tile 64
    xattn_kernel + xattn_reduce_kernel (csrc/pio_xattn.hip, pio_flash_attention_pair core 2)          key tile 32
    xattn_tall_kernel  (csrc/pio_xtall.hip,  pio_flash_attention_pair core 3)                         key block 32

tests/test_attn_core_cases_host.py proves on the CPU that the reference is right, that every case detects the faults these
kernels can have, and that every case reaches the branch it is labelled with; tests/test_attn_cores_gpu.py launches them.

Operands.  Planted, uniform and staircase operands are small integers (|n| <= 256 = an exact 8-bit significand) times a
power of two: exact in fp16 AND bf16, every product and every partial sum of a logit exact in fp32.  The random probe is
Gaussian, rounded to the case's 16-bit type here.  The reference runs in float64 on those same 16-bit operands, so it
differs from a kernel only by the kernel's documented roundings.

Probes (each case runs all that apply):
  planted    query row i leads one target key t(i) by >= 16 nats over every other attendable key, |s| <= 30: the output
             row is V[t(i), :] and a misplaced / dropped / extra key is an O(1) error.  Targets cycle over the edge list
             of the case (edges()).  Target keys carry signed rows of a Hadamard matrix (mutually orthogonal or opposite),
             the other keys entries of {-1, 0, 1} / 4; a MASKED key next to a target carries the target's own code, so
             that attending it halves the row.
  uniform    Q = 0: p = 1 exactly for every attendable key, the output is the mean of V over them.
  staircase  every key of a tile leads every key of the tile before by >= 8 nats (every tile moves the running maximum), or fall (mirrored: only the
             first tile does); on the masked cores the rising form also with the two leading tiles masked.
  random     Gaussian Q, K, V, |s| <~ 6.
V[j, c] = ((37 j + 11 c + 17 (b H + h)) mod 251 - 125) / 128 names key, channel and head (random probe: Gaussian).

Bound (bound()), per output element, derived -- not tuned.  u = 2^-11 (fp16) / 2^-8 (bf16) is half an ulp: Op<DT>::from_f32
(csrc/pio_internal.h) is a plain cast, round to nearest even, in both types, so r = 1.  With p_j the un-normalised
probabilities in fp32, l = sum_j p_j accumulated in fp32 from the UNROUNDED p_j, and o = (sum_j round16(p_j) v_j) / l:
  P     every p_j is rounded once to 16 bits: |round16(p_j) - p_j| <= u p_j, so the numerator moves by at most
        u sum_j p_j |v_j| <= u l max|V|: u max|V| after the division.
  O     the quotient is rounded once to 16 bits: u |o| <= u max|V|.  (Dropped where O + O_lo is compared.)
  fp16  a p_j below 2^-14 is subnormal in fp16 and carries an ABSOLUTE error of up to 2^-25; l >= 1 (the reference point
        of the exponent never exceeds the row maximum, so the largest p_j is >= 1): at most Tk 2^-25 max|V| in all.
  fp32  the sums (fp32 MFMA accumulation of exact products, the running l), the scale FMA and v_exp_f32: a few 2^-24
        relative each plus ~2^-23 |x| ln 2 from the exponent's argument near the row maximum: 2^-16 max|V| covers them.
=> |o - ref| <= (u + u + [fp16] Tk 2^-25 + 2^-16) max|V|, max|V| over the attendable keys of that (sample, head).
Exactly-zero rows, bit-identity claims and untouched memory are asserted exactly."""
import math

import numpy as np

U = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
ROUNDINGS = 1          # r: round to nearest (Op<DT>::from_f32 is `(T)x` for __half and __hip_bfloat16)
KEY_TILE = {"flash": 64, "xattn": 32, "xtall": 32}
PROBES = ("planted", "uniform", "stair_up", "stair_down", "stair_up_masked_lead", "random")
FAULTS = ("drop_last", "extra", "flip_mask", "swap23", "drop_tile", "skip_rescale", "drop_lo")


def bound(dt, Tk, vmax, pair_sum=False):
    """The element-wise bound of the module docstring; vmax may be an array."""
    terms = ROUNDINGS * U[dt] + (0.0 if pair_sum else ROUNDINGS * U[dt]) + (Tk * 2.0 ** -25 if dt == "f16" else 0.0)
    return (terms + 2.0 ** -16) * vmax


# ====================================================================================================
# cases: the smallest shape that reaches each branch.  label: the branch, as LITERALS (checked against
# csrc/pio_attn_route.h by the host test): flash (NW, KS); xattn (dkl, dvs, dv slices, key splits);
# xtall (xtall_supported, xattn_supported)
# ====================================================================================================
def _case(id, kern, dkp, dvp, B, H, Tq, Tk, label, **kw):
    c = dict(id=id, kern=kern, dkp=dkp, dvp=dvp, dk=dkp, B=B, H=H, Tq=Tq, Tk=Tk, label=label, vrow=False, pair=False,
             olo=False, ldo_gap=8, kmask=None, qmask=False, sqb0=False, dts=("f16", "bf16"), mask_bytes=False,
             twice=False, fwd=False)
    assert set(kw) <= set(c), kw
    c.update(kw)
    if c["pair"]:
        c["dts"] = ("f16",)
    return c


CASES = [
    # ---- flash_attn_kernel: four head shapes x {V^T, row-major V}; NW = 4 / KS = 1 on ragged shapes ----
    _case("flash_128_vt_tq127_tk63", "flash", 128, 128, 1, 2, 127, 63, (4, 1)),
    _case("flash_128_row_tq129_tk65", "flash", 128, 128, 1, 2, 129, 65, (4, 1), vrow=True),
    _case("flash_64_vt_tq200_tk133", "flash", 64, 64, 2, 1, 200, 133, (4, 1)),
    _case("flash_64_row_tq1_tk1", "flash", 64, 64, 2, 2, 1, 1, (4, 1), vrow=True),
    _case("flash_32_vt_tq129_tk1", "flash", 32, 32, 1, 3, 129, 1, (4, 1)),
    _case("flash_32_row_tq127_tk133_lane_stores", "flash", 32, 32, 2, 2, 127, 133, (4, 1), vrow=True, ldo_gap=4),
    _case("flash_32x160_vt_tq200_tk65", "flash", 32, 160, 1, 2, 200, 65, (4, 1)),
    _case("flash_32x160_row_tq1_tk63_lane_stores", "flash", 32, 160, 2, 1, 1, 63, (4, 1), vrow=True, ldo_gap=4),
    _case("flash_128_vt_tq1_tk133_lane_stores", "flash", 128, 128, 1, 2, 1, 133, (4, 1), ldo_gap=4),
    # 256-row workgroups: B H ceil(Tq / 256) >= 256 with Tq >= 256, row-major V
    _case("flash_32_row_nw8", "flash", 32, 32, 16, 16, 259, 65, (8, 1), vrow=True),
    # key parts over wave groups
    _case("flash_128_row_ks2_tk256", "flash", 128, 128, 1, 2, 130, 256, (8, 2), vrow=True),
    _case("flash_128_row_ks2_tk384", "flash", 128, 128, 1, 2, 130, 384, (8, 2), vrow=True),
    _case("flash_32x160_row_ks2_tk256_lane_stores", "flash", 32, 160, 1, 2, 130, 256, (8, 2), vrow=True, ldo_gap=4),
    _case("flash_32_row_ks4_tk1024", "flash", 32, 32, 1, 2, 130, 1024, (16, 4), vrow=True),
    _case("flash_64_row_ks4_tk1024", "flash", 64, 64, 1, 2, 130, 1024, (16, 4), vrow=True),
    # pair operands (fp16): Q_lo / K_lo non-zero, output as a pair (per-lane stores)
    _case("flash_32_row_pair_olo", "flash", 32, 32, 1, 2, 129, 133, (4, 1), vrow=True, pair=True, olo=True),
    _case("flash_32x160_vt_pair_olo", "flash", 32, 160, 1, 2, 33, 65, (4, 1), pair=True, olo=True),
    _case("flash_32_row_pair_ks4", "flash", 32, 32, 1, 1, 130, 1024, (16, 4), vrow=True, pair=True),
    # batch-invariant Q, logical dk < dkp
    _case("flash_64_vt_sqb0", "flash", 64, 64, 3, 2, 129, 65, (4, 1), sqb0=True),
    _case("flash_32_row_dk25", "flash", 32, 32, 1, 2, 33, 133, (4, 1), vrow=True, dk=25),

    # ---- xattn_kernel: six instantiations at the edges of the table; masks; key splits ----
    _case("xattn_32x96_dk8_dv8_singles", "xattn", 8, 8, 5, 2, 33, 100, (32, 96, 1, 1), kmask="singles", olo=True),
    _case("xattn_32x96_pair_both_masks", "xattn", 32, 96, 2, 2, 129, 100, (32, 96, 1, 1), pair=True, olo=True,
          kmask="scatter", qmask=True, mask_bytes=True),
    _case("xattn_32x96_tq1_tk1", "xattn", 32, 96, 2, 1, 1, 1, (32, 96, 1, 1)),
    _case("xattn_32x160_pair_tq1_tk33", "xattn", 32, 160, 2, 2, 1, 33, (32, 160, 1, 1), pair=True, olo=True),
    _case("xattn_32x160_dk16_dv104_tk31_qmask", "xattn", 16, 104, 2, 1, 33, 31, (32, 160, 1, 1), qmask=True),
    _case("xattn_32x160_lead2", "xattn", 32, 160, 1, 2, 33, 100, (32, 160, 1, 1), kmask="lead2", olo=True),
    _case("xattn_128_middle", "xattn", 128, 128, 1, 2, 129, 100, (128, 128, 1, 1), kmask="middle"),
    _case("xattn_128_dk40_dv8_dead_sample", "xattn", 40, 8, 2, 2, 33, 33, (128, 128, 1, 1), kmask="dead1", olo=True),
    _case("xattn_352_at_328", "xattn", 328, 328, 1, 1, 129, 100, (352, 352, 1, 1), kmask="scatter"),
    _case("xattn_352_tk31_sqb0", "xattn", 352, 352, 2, 1, 33, 31, (352, 352, 1, 1), sqb0=True),
    _case("xattn_512", "xattn", 512, 512, 1, 1, 33, 33, (512, 512, 1, 1), olo=True),
    _case("xattn_512_dk360_qmask", "xattn", 360, 360, 1, 1, 129, 100, (512, 512, 1, 1), qmask=True),
    _case("xattn_704_three_slices", "xattn", 704, 704, 1, 1, 33, 100, (704, 256, 3, 1), kmask="lead2"),
    _case("xattn_704_dk520_dv264_two_slices", "xattn", 520, 264, 1, 1, 33, 33, (704, 256, 2, 1), olo=True),
    # key splits (xattn_reduce_kernel)
    _case("xattn_split2_tk520", "xattn", 32, 96, 1, 1, 129, 520, (32, 96, 1, 2), twice=True),
    _case("xattn_split2_tk520_pair_olo_qmask", "xattn", 32, 160, 1, 1, 33, 520, (32, 160, 1, 2), pair=True, olo=True,
          qmask=True, twice=True),
    _case("xattn_split4_tk1000_scatter", "xattn", 128, 128, 1, 1, 129, 1000, (128, 128, 1, 4), kmask="scatter", olo=True),
    _case("xattn_split2_last_split_masked", "xattn", 32, 96, 1, 1, 33, 520, (32, 96, 1, 2), kmask="split1_dead"),
    _case("xattn_split2_first_split_masked", "xattn", 32, 96, 1, 1, 33, 520, (32, 96, 1, 2), kmask="split0_dead",
          qmask=True),
    _case("xattn_split10_empty_split_tk2575", "xattn", 32, 96, 1, 1, 128, 2575, (32, 96, 1, 10), olo=True, twice=True),
    _case("xattn_512_split2_tk520", "xattn", 512, 512, 1, 1, 33, 520, (512, 512, 1, 2), qmask=True),
    _case("xattn_704_split_two_slices", "xattn", 520, 264, 1, 1, 33, 520, (704, 256, 2, 2)),

    # ---- xattn_tall_kernel ----
    _case("xtall_64x256_tk33", "xtall", 64, 256, 2, 2, 129, 33, (1, 1), olo=True),
    _case("xtall_64x768_tk1", "xtall", 64, 768, 1, 2, 1, 1, (1, 0)),
    _case("xtall_64x768_tk257_mask", "xtall", 64, 768, 2, 1, 129, 257, (1, 0), kmask="tall", mask_bytes=True),
    _case("xtall_736x512_tk480_qmask", "xtall", 736, 512, 1, 1, 129, 480, (1, 0), qmask=True, olo=True),
    _case("xtall_736x512_tk512_dead_sample", "xtall", 736, 512, 2, 2, 1, 512, (1, 0), kmask="dead1", mask_bytes=True),
    _case("xtall_1024_tk512_sqb0", "xtall", 1024, 1024, 2, 1, 129, 512, (1, 0), sqb0=True),
    _case("xtall_1024_tk257_fwd", "xtall", 1024, 1024, 1, 1, 33, 257, (1, 0), fwd=True, dts=("f16",)),
]
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def key_parts(c):
    """[(first key, end key)] of the key splits (xattn: label's split count) / key parts (flash: KS) that own keys."""
    Tk, kt = c["Tk"], KEY_TILE[c["kern"]]
    ntiles = (Tk + kt - 1) // kt
    n = c["label"][3] if c["kern"] == "xattn" else (c["label"][1] if c["kern"] == "flash" else 1)
    per = (ntiles + n - 1) // n
    out = []
    for s in range(n):
        a, b = s * per * kt, min((s + 1) * per * kt, Tk)
        if a < b:
            out.append((a, b))
    return out


def key_mask(c):
    """bool [B, Tk] (True = attendable) or None."""
    B, Tk, kind = c["B"], c["Tk"], c["kmask"]
    if kind is None:
        return None
    j = np.arange(Tk)
    m = np.ones((B, Tk), bool)
    if kind == "singles":                       # isolated attendable keys at 0, 31, 32, Tk - 1
        pos = [0, 31, 32, Tk - 1]
        m[:] = False
        m[0, pos + [4]] = True
        for b in range(1, B):
            m[b, pos[(b - 1) % 4]] = True
    elif kind == "lead2":
        m[:, :64] = False
    elif kind == "middle":
        m[:, 32:64] = False
    elif kind == "scatter":
        m[:, (j % 7) == 3] = False
        m[-1, 0] = False
    elif kind == "dead1":                       # sample 1 has no attendable key
        m[:, (j % 5) == 3] = False
        m[1, :] = False
    elif kind == "split1_dead":
        m[:, key_parts(c)[1][0]:] = False
    elif kind == "split0_dead":
        m[:, :key_parts(c)[1][0]] = False
    elif kind == "tall":                        # a fully masked 32-block and a single key in the last block
        m[:, 32:64] = False
        last0 = 32 * ((Tk - 1) // 32)
        m[:, last0:] = False
        m[:, min(last0 + 5, Tk - 1)] = True
    else:
        raise KeyError(kind)
    return m


def query_mask(c):
    if not c["qmask"]:
        return None
    i = np.arange(c["Tq"])
    m = np.ones((c["B"], c["Tq"]), bool)
    m[:, (i % 5) == 1] = False
    m[-1, 0] = False
    return m


def edges(c, att):
    """Planted targets of one sample (att: bool [Tk], its attendable keys): the positions inside a 32-key tile that expose
    the bit-2/3 row permutation, 31 | 32, first and last key of the kernel's leading and last tiles and of every key split
    / part, the last attendable key, Tk - 1, and the attendable neighbours of masked keys."""
    Tk, kt = c["Tk"], KEY_TILE[c["kern"]]
    idx = np.flatnonzero(att)
    e = ([int(idx[-1])] if idx.size else []) + [4, Tk - 1]      # (first: a case with a single query row still gets these)
    for a, b in key_parts(c):                                   # first and last attendable key of every key split / part
        own = idx[(idx >= a) & (idx < b)]
        if own.size:
            e += [int(own[0]), int(own[-1])]
    e += [0, 3, 7, 8, 11, 12, 15, 31, 32, kt - 1, kt, 2 * kt - 1, 2 * kt, kt * ((Tk - 1) // kt), Tk - 1]
    for a, b in key_parts(c):
        e += [a, a + 31, b - 32, b - 1, kt * ((b - 1) // kt)]
    if idx.size:
        e.append(int(idx[0]))
    masked = np.flatnonzero(~att)
    near = [int(k) + d for k in masked for d in (-1, 1)]
    e += near[:8] + near[-8:]
    seen, out = set(), []
    for k in e:
        if 0 <= k < Tk and att[k] and k not in seen:
            seen.add(k)
            out.append(k)
    return out


# ====================================================================================================
# operands
# ====================================================================================================
def round16(a, dt):
    """float -> nearest value of the 16-bit type (ties to even), as float32."""
    a = np.asarray(a, np.float32)
    if dt == "f16":
        return a.astype(np.float16).astype(np.float32)
    bits = a.view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32)


def _hadamard(n):
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def _quant(x):
    """x rounded down to m 2^-e with 64 <= m <= 128: returns (m, e)."""
    e = 0
    while x * 2.0 ** e < 64:
        e += 1
    while x * 2.0 ** e > 128:
        e -= 1
    return int(math.floor(x * 2.0 ** e)), e


def _v_code(c):
    B, H, Tk, dv = c["B"], c["H"], c["Tk"], c["dvp"]
    b, j, h, ch = np.ogrid[:B, :Tk, :H, :dv]
    return (((37 * j + 11 * ch + 17 * (b * H + h)) % 251) - 125) / 128.0


def _lo_pattern(shape, mul):
    idx = np.indices(shape).astype(np.int64)
    return ((idx[-3] * 7 + idx[-1] * 3 + idx[-2] * mul + 1) % 5 - 2) * 2.0 ** -5


def make(c, probe, dt):
    """Operands of one probe as float64 arrays holding values exact in `dt`:
    qh [Bq, Tq, H, dkp] (Bq = 1: batch-invariant), kh [B, Tk, H, dkp], v [B, Tk, H, dvp], ql / kl (pair cases, else None),
    km [B, Tk] / qm [B, Tq] bool or None, targets [B, H, Tq] (planted) or None.  None when the probe does not apply."""
    B, H, Tq, Tk, dkp, dk = c["B"], c["H"], c["Tq"], c["Tk"], c["dkp"], c["dk"]
    kt = KEY_TILE[c["kern"]]
    Bq = 1 if c["sqb0"] else B
    km, qm = key_mask(c), query_mask(c)
    rng = np.random.default_rng(sum(ord(x) * (i + 1) for i, x in enumerate(c["id"] + probe)))
    qh = np.zeros((Bq, Tq, H, dkp))
    kh = np.zeros((B, Tk, H, dkp))
    kh[..., :dk] = rng.integers(-1, 2, (B, Tk, H, dk)) / 4.0
    v = _v_code(c)
    targets = None
    ntile = (Tk + kt - 1) // kt
    if probe == "planted":
        n = 1
        while 2 * n <= min(dk, 64):
            n *= 2
        had = _hadamard(n)
        used = n * (dk // n)
        m, e = _quant(28.0 * math.sqrt(dk) / used)
        a = m * 2.0 ** -e
        targets = np.full((B, H, Tq), -1)
        for b in range(B):
            att = km[b] if km is not None else np.ones(Tk, bool)
            ed = edges(c, att)
            if not ed:
                continue
            for h in range(H):
                # head h continues in the edge list where head h - 1 stopped, so that the heads of ONE sample cover it
                # (a (sample, head) has 2 n codes and Tq rows); samples start at different edges, unless Q is shared
                width = min(2 * n, len(ed), Tq)
                off = h * width + (0 if c["sqb0"] else 5 * b)
                win = [ed[(off + r) % len(ed)] for r in range(width)]
                codes = [np.tile((1 if r < n else -1) * had[r % n], dk // n) for r in range(len(win))]
                for r, key in enumerate(win):
                    kh[b, key, h, :] = 0
                    kh[b, key, h, :used] = codes[r]
                    for nb in (key - 1, key + 1):                      # masked neighbours: decoys with the target's code
                        if 0 <= nb < Tk and not att[nb]:
                            kh[b, nb, h, :] = kh[b, key, h, :]
                for i in range(Tq):
                    r = i % len(win)
                    targets[b, h, i] = win[r]
                    if b < Bq:
                        qh[b, i, h, :] = 0
                        qh[b, i, h, :used] = a * codes[r]
    elif probe == "uniform":
        pass
    elif probe.startswith("stair"):
        if probe == "stair_up_masked_lead":
            if c["kern"] == "flash" or Tk <= 2 * kt or km is not None:
                return None
            km = np.ones((B, Tk), bool)
            km[:, :2 * kt] = False
        if ntile < 2:
            return None
        na = max(dk // 2, 1)
        nb = dk - na
        sig = np.where(np.arange(dk) % 3 == 0, -1.0, 1.0)
        ma, e = _quant(12.0 * math.sqrt(dk) / na)      # ~12 nats per tile, ~0.5 per jitter step (<= 3 steps)
        mb = max(int(round(0.5 * math.sqrt(dk) / max(nb, 1) * 2.0 ** e)), 1)
        level = np.arange(Tk) // kt
        if probe == "stair_down":
            level = ntile - 1 - level
        jit = np.arange(Tk) % 4
        kh[:] = 0
        kh[..., :na] = level[None, :, None, None] * sig[:na]
        if nb:
            kh[..., na:dk] = ((jit[None, :, None] + np.arange(H)[None, None, :]) % 4)[..., None] * sig[na:]
        row = 1 + (np.arange(Tq) % 2)
        qh[..., :na] = (ma * 2.0 ** -e) * sig[:na] * row[None, :, None, None]
        if nb:
            qh[..., na:dk] = (mb * 2.0 ** -e) * sig[na:] * row[None, :, None, None]
    elif probe == "random":
        qh[..., :dk] = rng.standard_normal((Bq, Tq, H, dk))
        kh[..., :dk] = rng.standard_normal((B, Tk, H, dk))
        v = rng.standard_normal(v.shape)
    else:
        raise KeyError(probe)
    ql = kl = None
    if probe == "random":
        q32, k32 = qh.astype(np.float32), kh.astype(np.float32)
        qh, kh, v = (round16(x, dt).astype(np.float64) for x in (qh, kh, v))
        if c["pair"]:
            ql = round16(q32 - qh.astype(np.float32), dt).astype(np.float64)
            kl = round16(k32 - kh.astype(np.float32), dt).astype(np.float64)
    elif c["pair"]:
        # (not rounding residuals: large enough that a core that drops Q_lo K_hi + Q_hi K_lo misses the bound)
        ql = np.zeros_like(qh) if probe == "uniform" else _lo_pattern(qh.shape, 1)
        kl = _lo_pattern(kh.shape, 2)
        ql[..., dk:] = 0
        kl[..., dk:] = 0
    for x in (qh, kh, v, ql, kl):
        assert x is None or np.array_equal(round16(x, dt), x), "operands must be exact in the 16-bit type"
    return dict(qh=qh, ql=ql, kh=kh, kl=kl, v=v, km=km, qm=qm, targets=targets, dk=dk)


# ====================================================================================================
# float64 reference, and the same with one fault of the kind these kernels can have
# ====================================================================================================
def logits(d):
    """[B, H, Tq, Tk] float64: (Q_hi K_hi + Q_lo K_hi + Q_hi K_lo) / sqrt(dk), masked keys -inf."""
    B = d["kh"].shape[0]
    def qk(q, k):
        return np.broadcast_to(q, (B,) + q.shape[1:]).transpose(0, 2, 1, 3) @ k.transpose(0, 2, 3, 1)
    s = qk(d["qh"], d["kh"])
    if d["ql"] is not None:
        s = s + qk(d["ql"], d["kh"]) + qk(d["qh"], d["kl"])
    s = s / math.sqrt(d["dk"])
    if d["km"] is not None:
        s = np.where(d["km"][:, None, None, :], s, -np.inf)
    return s


def _finish(o, d):
    """[B, H, Tq, dv] -> [B, Tq, H, dv], rows with query mask 0 wiped."""
    o = o.transpose(0, 2, 1, 3)
    if d["qm"] is not None:
        o = np.where(d["qm"][:, :, None, None], o, 0.0)
    return o


def reference(d):
    """O [B, Tq, H, dv] float64.  Rows without an attendable key and rows with query mask 0 are zero."""
    s = logits(d)
    m = s.max(axis=-1, keepdims=True)
    p = np.exp(s - np.where(np.isfinite(m), m, 0.0))
    l = p.sum(axis=-1, keepdims=True)
    o = (p @ d["v"].transpose(0, 2, 1, 3)) / np.where(l > 0, l, 1.0)
    return _finish(o, d)


def reference_online(d, kt, skip_tile=None):
    """The same by online softmax over key tiles of kt; skip_tile: that tile's rescale of the running sums is left out."""
    s = logits(d)
    B, H, Tq, Tk = s.shape
    m = np.full((B, H, Tq, 1), -np.inf)
    l = np.zeros((B, H, Tq, 1))
    o = np.zeros((B, H, Tq, d["v"].shape[-1]))
    for t in range((Tk + kt - 1) // kt):
        st = s[..., t * kt:(t + 1) * kt]
        mn = np.maximum(m, st.max(axis=-1, keepdims=True))
        mu = np.where(np.isfinite(mn), mn, 0.0)
        alpha = np.where(np.isfinite(m), np.exp(m - mu), 1.0)
        if t == skip_tile:
            alpha = np.ones_like(alpha)
        p = np.exp(st - mu)
        l = l * alpha + p.sum(axis=-1, keepdims=True)
        o = o * alpha + p @ d["v"][:, t * kt:(t + 1) * kt].transpose(0, 2, 1, 3)
        m = mn
    return _finish(o / np.where(l > 0, l, 1.0), d)


def _swap23(j):
    return (j & ~12) | ((j & 4) << 1) | ((j & 8) >> 1)


def faulty(c, d, fault):
    """reference(d) as a kernel with `fault` would compute it, or None where the fault does not apply to the case."""
    B, Tk = d["kh"].shape[:2]
    kt = KEY_TILE[c["kern"]]
    km = d["km"] if d["km"] is not None else np.ones((B, Tk), bool)
    e = dict(d)
    if fault == "drop_last":                    # the last attendable key of every sample is dropped
        km = km.copy()
        for b in range(B):
            idx = np.flatnonzero(km[b])
            if idx.size:
                km[b, idx[-1]] = False
        e["km"] = km
    elif fault == "extra":                      # key Tk is attended too: garbage as good as the last attendable key's row
        last = [int(np.flatnonzero(km[b])[-1]) if km[b].any() else Tk - 1 for b in range(B)]
        e["kh"] = np.concatenate([d["kh"], d["kh"][np.arange(B), last][:, None]], axis=1)
        if d["kl"] is not None:
            e["kl"] = np.concatenate([d["kl"], d["kl"][np.arange(B), last][:, None]], axis=1)
        vx = (d["v"][:, -1:] + 0.75) % 1.0 - 0.5
        e["v"] = np.concatenate([d["v"], vx], axis=1)
        e["km"] = np.concatenate([km, km.any(axis=1, keepdims=True)], axis=1)
    elif fault == "flip_mask":                  # one masked key next to an attendable one is attended
        if c["kmask"] is None:
            return None
        km = km.copy()
        for b in range(B):
            for k in np.flatnonzero(~km[b]):
                if (k > 0 and km[b, k - 1]) or (k + 1 < Tk and km[b, k + 1]):
                    km[b, k] = True
                    break
        e["km"] = km
    elif fault == "swap23":                     # a key lands on the V^T column of its bit-2/3 partner
        j = np.arange(Tk)
        sw = _swap23(j)
        if Tk <= 8:
            return None
        e["v"] = d["v"][:, np.where(sw < Tk, sw, j)]
    elif fault == "drop_tile":                  # every key split / part loses its last tile
        km = km.copy()
        for a, b_ in key_parts(c):
            km[:, kt * ((b_ - 1) // kt):b_] = False
        e["km"] = km
    elif fault == "skip_rescale":               # the last tile that moves the running maximum does not rescale
        live = [t for t in range((Tk + kt - 1) // kt) if km[:, t * kt:(t + 1) * kt].any()]
        if len(live) < 2 or c["kern"] == "xtall":   # (the tall-head kernel takes the exact maximum: no rescale exists)
            return None
        return reference_online(d, kt, skip_tile=live[-1])
    elif fault == "drop_lo":                    # pair cases: S = Q_hi K_hi alone
        if d["ql"] is None:
            return None
        e["ql"] = e["kl"] = None
    else:
        raise KeyError(fault)
    return reference(e)


def vmax_of(d):
    """max |V| over the attendable keys, [B, 1, H, 1] (0 where a sample has none)."""
    B, Tk = d["kh"].shape[:2]
    km = d["km"] if d["km"] is not None else np.ones((B, Tk), bool)
    return np.where(km[:, :, None, None], np.abs(d["v"]), 0.0).max(axis=(1, 3), keepdims=True)
