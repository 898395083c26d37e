"""Cases and the float64 reference for the ADDRESSING of pio_gemm_nt (include/pio_hip.h, pio_gemm_t): every stride, pitch,
offset and alignment class of the descriptor on every kernel csrc/pio_gemm_route.h can pick.

Numpy only; shared by tests/test_gemm_addr_host.py (CPU: routing of every case through pio_gemm_route.h, coverage of the
kernel x feature matrix, the reference against torch) and tests/test_gemm_addr_gpu.py (MI355X: the kernels, bit for bit).

Operands are small integers: every product and every partial sum is an integer far below 2^24, so the fp32 accumulator of
any kernel holds the true result in any summation order and the comparison needs no tolerance (exact_ok).  act == 0 and
no LayerNorm-fold fields throughout: the fold and GELU under it have tests/gemm_fold_cases.py, test_gemm_fold_host.py / _gpu.py.

A case is a dict of the pio_gemm_t fields that matter plus
    override  value passed to pio_gemm_kernel_override
    kernel    the GemmKernel enumerator the launch must reach on 256 CUs
    c_off / bias_off / r_off   element offsets of the C / bias / R pointers inside their (256-byte aligned) payloads
    features  the addressing features the layout exercises (features_of: derived from the fields, never claimed by hand)
"""
import zlib

import numpy as np

from primitive_cases import DTYPES, round_to  # noqa: F401  (re-exported for the two test files)

KERNELS = ("SKINNY2", "SKINNY4", "WIDE", "STREAM", "T256", "T128", "T128_KG2", "T64", "T64_KG2", "T32", "T32_KG2")
FEATURES = ("lda_pitch", "ldb_pitch", "ldc_pitch", "n_store_pad", "ldr_pitch", "heads_in_row_A", "heads_in_row_B",
            "heads_in_row_C", "batch_gap", "res_rows", "res_unaligned", "c_unaligned", "bias_unaligned", "bias_rows",
            "b_lo_from", "a_lo", "b_lo", "c_lo", "alpha")
N_CU = 256          # the routing below holds for a 256-CU device with the default CU budget
TAIL = 8            # unread (NaN) elements behind the last element of every input


def _case(cid, kernel, override, M, N, K, **kw):
    """Defaults = the dense layout; every keyword overrides one field."""
    c = dict(id=cid, kernel=kernel, override=override, M=M, N=N, K=K, batch=1, nh=1, n_store=N, out_f32=1, alpha=1.0,
             a_lo=False, b_lo=False, c_lo=False, b_lo_n0=0, bias_mode=0, bias_off=0, c_off=0,
             res=False, ldr=0, r_rows=0, r_stride_b=0, r_off=0)
    c.update(kw)
    c.setdefault("lda", K)
    c.setdefault("ldb", K)
    c.setdefault("ldc", c["n_store"])
    c.setdefault("sAh", M * c["lda"])
    c.setdefault("sBh", N * c["ldb"])
    c.setdefault("sCh", M * c["ldc"])
    c.setdefault("sAb", c["nh"] * c["sAh"])
    c.setdefault("sBb", c["nh"] * c["sBh"])
    c.setdefault("sCb", c["nh"] * c["sCh"])
    if c["res"] and not c["ldr"]:
        c["ldr"] = N
    c["features"] = features_of(c)
    c["extras"] = extras_of(c)
    return c


# ----------------------------------------------------------------------------------------------------
# what gemm_params derives (restated; the host test compares it with the C++)
# ----------------------------------------------------------------------------------------------------
def derived(c):
    esz, valign = (4, 16) if c["out_f32"] else (2, 8)
    vec = all((v * esz) % valign == 0 for v in (c["c_off"], c["ldc"], c["sCb"], c["sCh"]))
    r_rows = c["r_rows"] if c["res"] else 0
    if c["res"] and r_rows > 0 and c["r_stride_b"] == r_rows * c["ldr"]:
        r_rows = 0          # contiguous batches: one flat matrix
    return dict(vec_ok=int(vec),
                r_vec=int(bool(c["res"]) and c["r_off"] % 4 == 0 and c["ldr"] % 4 == 0 and c["r_stride_b"] % 4 == 0),
                bias_vec=int(c["bias_mode"] != 0 and c["bias_off"] % 4 == 0),
                npass=1 + int(c["a_lo"]) + int(c["b_lo"]), lo_n0=c["b_lo_n0"] if c["b_lo"] else 0, r_rows=r_rows)


def features_of(c):
    d = derived(c)
    nh, nb = c["nh"], c["batch"] // c["nh"]
    a_mat, b_mat = (c["M"] - 1) * c["lda"] + c["K"], (c["N"] - 1) * c["ldb"] + c["K"]
    hA = nh > 1 and 0 < c["sAh"] < a_mat
    hB = nh > 1 and 0 < c["sBh"] < b_mat
    hC = nh > 1 and 0 < c["sCh"] < c["ldc"]
    f = set()
    if c["lda"] > (nh * c["K"] if hA else c["K"]):
        f.add("lda_pitch")
    if c["ldb"] > (nh * c["K"] if hB else c["K"]):
        f.add("ldb_pitch")
    if c["ldc"] > (nh * c["n_store"] if hC else c["n_store"]):
        f.add("ldc_pitch")
    if c["n_store"] > c["N"]:
        f.add("n_store_pad")
    if hA:
        f.add("heads_in_row_A")
    if hB:
        f.add("heads_in_row_B")
    if hC:
        assert c["n_store"] == c["N"], "pad columns would land in the neighbouring head"
        f.add("heads_in_row_C")
    if nb > 1 and c["sAb"] > (c["lda"] * c["M"] if hA else nh * c["sAh"]) and \
            c["sBb"] > (c["ldb"] * c["N"] if hB else nh * c["sBh"]) and c["sCb"] > (c["ldc"] * c["M"] if hC else nh * c["sCh"]):
        f.add("batch_gap")
    if c["res"]:
        if c["ldr"] > c["N"]:
            f.add("ldr_pitch")
        if d["r_rows"] > 0:
            f.add("res_rows")
        if not d["r_vec"]:
            f.add("res_unaligned")
    if not d["vec_ok"]:
        f.add("c_unaligned")
    if c["bias_mode"] == 1 and not d["bias_vec"]:
        f.add("bias_unaligned")
    if c["bias_mode"] == 2:
        f.add("bias_rows")
    if d["lo_n0"]:
        f.add("b_lo_from")
    for k in ("a_lo", "b_lo"):
        if c[k]:
            f.add(k)
    if c["c_lo"] and not c["out_f32"]:      # (beside an fp32 result C_lo is ignored)
        f.add("c_lo")
    if c["alpha"] != 1.0:
        f.add("alpha")
    return frozenset(f)


# Forms of the epilogue beside the addressing features: asked of the kernels REQUIRED_EXTRA names, not of all eleven.
EXTRAS = ("out_f32", "out_16", "out_16_plain", "res_vec", "res_stride0", "res_16", "res_batched", "c16_scalar")


def extras_of(c):
    d = derived(c)
    e = {"out_f32" if c["out_f32"] else "out_16"}
    if not c["out_f32"] and not c["res"] and not c["c_lo"]:
        e.add("out_16_plain")                 # one 16-bit image, nothing added behind the bias
    if c["res"]:
        if d["r_vec"]:
            e.add("res_vec")                  # the 16-byte residual load
        if d["r_rows"] > 0 and c["r_stride_b"] == 0:
            e.add("res_stride0")              # every batch of rows reads the same residual rows
        if not c["out_f32"]:
            e.add("res_16")                   # a residual under a 16-bit result
        if c["batch"] > 1:
            e.add("res_batched")              # one residual for every (zb, zh) slice
    if not c["out_f32"] and not d["vec_ok"]:
        e.add("c16_scalar")                   # the element-by-element 16-bit store of C (and C_lo)
    return frozenset(e)


# ----------------------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------------------
def _heads(cid, kernel, override, M, N, K, nb, nh, **kw):
    """(b, h) slices with the heads interleaved INSIDE a row of all three matrices -- A / B as the materialised Q K^T of
    csrc/pio_blocks.hip reads them, C as its P V writes them --, a pitch behind the heads, a gap between batches, all three
    K sweeps, the hi + lo result, a per-row bias and alpha = 1/2."""
    lda, ldb, ldc = nh * K + 8, nh * K + 16, nh * N + 8
    d = dict(batch=nb * nh, nh=nh, lda=lda, ldb=ldb, ldc=ldc, sAh=K, sBh=K, sCh=N, sAb=M * lda + 24, sBb=N * ldb + 8,
             sCb=M * ldc + 16, out_f32=0, a_lo=True, b_lo=True, c_lo=True, bias_mode=2, alpha=0.5)
    d.update(kw)
    return _case(cid, kernel, override, M, N, K, **d)


def _flat_scalar(cid, kernel, override, M, N, K, r_rows, **kw):
    """One flat problem on the SCALAR epilogue paths: fp32 C 8 bytes off a 16-byte boundary, a residual 4 bytes off with an
    odd pitch given as (stride_b, rows_per_batch), a bias 4 bytes off, zero columns behind N, pitches everywhere."""
    n_store = N + 2
    d = dict(n_store=n_store, lda=K + 8, ldb=K + 16, ldc=n_store + 3, c_off=2, bias_mode=1, bias_off=1, alpha=0.5,
             res=True, ldr=N + 3, r_off=1, r_rows=r_rows, r_stride_b=r_rows * (N + 3) + 5)
    d.update(kw)
    return _case(cid, kernel, override, M, N, K, **d)


def _flat_vector(cid, kernel, override, M, N, K, r_rows, **kw):
    """One flat problem on the VECTOR epilogue paths: 16-bit hi + lo result with zero columns and a pitch, a 16-byte aligned
    residual with a pitch whose batches all read the SAME rows (r_stride_b == 0), an aligned bias."""
    n_store = N + 4
    d = dict(n_store=n_store, out_f32=0, c_lo=True, lda=K + 8, ldb=K + 8, ldc=n_store + 4, bias_mode=1, alpha=2.0,
             res=True, ldr=N + 4, r_rows=r_rows, r_stride_b=0)
    d.update(kw)
    return _case(cid, kernel, override, M, N, K, **d)


def _batched_scalar16(cid, kernel, override, M, N, K, **kw):
    """Two dense slices on the SCALAR 16-bit store: hi + lo result with an odd pitch and one zero column, so that no row of
    C or C_lo is 8-byte aligned and n_store is no multiple of 4; ONE residual (odd pitch) added to both slices."""
    n_store = N + 1
    ldc = n_store + 3 - (n_store & 1)
    assert ldc % 2 == 1
    d = dict(batch=2, n_store=n_store, out_f32=0, c_lo=True, ldc=ldc, sCb=M * ldc + 1, lda=K + 8, bias_mode=1,
             res=True, ldr=N + 3)
    d.update(kw)
    return _case(cid, kernel, override, M, N, K, **d)


CASES = [
    # ---- gemm_nt_128 on its three tiles, with and without the two K teams (route: tiles per CU; KG2: npass * K >= 1024)
    _heads("t32_heads", "T32", 0, 70, 72, 40, 2, 3),
    _flat_scalar("t32_scalar", "T32", 0, 70, 70, 40, 16),
    _heads("t32kg2_heads", "T32_KG2", 0, 40, 72, 344, 2, 2),                  # 3 sweeps x 344 = 1032
    _flat_scalar("t32kg2_scalar", "T32_KG2", 0, 100, 134, 1024, 32),
    _heads("t64_heads", "T64", 64, 65, 68, 72, 2, 2),
    _flat_scalar("t64_scalar", "T64", 64, 65, 65, 72, 16),
    _flat_vector("t64_vector", "T64", 64, 65, 68, 72, 16),
    _batched_scalar16("t64_scalar16", "T64", 64, 65, 66, 72),
    _heads("t64kg2_heads", "T64_KG2", 0, 390, 444, 344, 2, 2),                # 7 x 7 x 4 = 196 tiles of 64 x 64
    _flat_scalar("t64kg2_scalar", "T64_KG2", 0, 830, 890, 1024, 100),         # 13 x 14 = 182 tiles
    _heads("t128_heads", "T128", 128, 200, 136, 72, 2, 2),
    _flat_scalar("t128_scalar", "T128", 128, 200, 134, 72, 64),
    _flat_vector("t128_vector", "T128", 128, 200, 132, 72, 50),
    _batched_scalar16("t128_scalar16", "T128", 128, 200, 134, 72),
    _heads("t128kg2_heads", "T128_KG2", 0, 129, 132, 520, 6, 8),              # 2 x 2 x 48 = 192 tiles of 128 x 128
    _flat_scalar("t128kg2_scalar", "T128_KG2", 0, 1660, 1914, 1024, 256),     # 13 x 15 = 195 tiles
    # ---- gemm_nt_256
    _heads("t256_heads", "T256", 256, 300, 264, 40, 2, 2),
    _flat_scalar("t256_scalar", "T256", 256, 300, 262, 40, 128),
    _flat_vector("t256_vector", "T256", 256, 300, 260, 40, 75),
    _batched_scalar16("t256_scalar16", "T256", 256, 300, 262, 40),
    # ---- gemm_nt_stream: K % 64 == 0, >= 16 K steps, 4-column groups, aligned C / R / bias, alpha == 1 with a residual
    _case("stream_res_f32", "STREAM", 1, 300, 264, 1024, n_store=268, lda=1032, ldb=1040, ldc=272, bias_mode=1,
          res=True, ldr=268),
    _heads("stream_heads", "STREAM", 1, 300, 136, 512, 2, 2, bias_mode=1),
    _case("stream_res_16", "STREAM", 1, 300, 132, 512, out_f32=0, n_store=136, ldc=144, lda=520, b_lo=True, bias_mode=1,
          res=True, ldr=136),
    # ---- gemm_nt_wide: one flat problem, K % 64 == 0, 8-column groups
    _case("wide_16", "WIDE", 2, 300, 264, 128, out_f32=0, n_store=272, lda=136, ldb=144, ldc=280, bias_mode=1, alpha=0.5),
    _case("wide_b_lo_from", "WIDE", 2, 300, 520, 192, out_f32=0, b_lo=True, b_lo_n0=256, c_lo=True, lda=200, ldb=200,
          ldc=528, bias_mode=1),
    _case("wide_a_lo_res_f32", "WIDE", 2, 300, 264, 128, a_lo=True, b_lo=True, lda=136, ldb=136, ldc=272, bias_mode=1,
          res=True, ldr=268, alpha=2.0),
    _case("wide_c_lo_res", "WIDE", 2, 300, 264, 128, out_f32=0, c_lo=True, a_lo=True, n_store=272, ldc=280, bias_mode=1,
          res=True, ldr=272),
    # ---- gemm_nt_skinny: >= 2048 rows, <= 4 stored columns; scalar loads and stores throughout (no alignment asked)
    _case("skinny2", "SKINNY2", 0, 2051, 1, 72, n_store=2, lda=80, ldb=88, ldc=3, c_off=2, bias_mode=1, bias_off=1,
          a_lo=True, b_lo=True, alpha=0.5),
    _case("skinny2_dense", "SKINNY2", 0, 2051, 2, 72, out_f32=0, lda=80, ldb=88, ldc=6),
    _case("skinny4", "SKINNY4", 0, 2051, 3, 1032, out_f32=0, n_store=4, lda=1040, ldb=1048, ldc=5, bias_mode=1,
          bias_off=3, a_lo=True, b_lo=True, alpha=2.0),
]
BY_ID = {c["id"]: c for c in CASES}


def model_layout_cases(H=3, dk=24, dv=40, Tq=70, Tk=77, B=2):
    """The two descriptors materialised_core (csrc/pio_blocks.hip) builds for S = Q K^T and O = P V, field for field, on
    the operands a fused q|k projection leaves (row pitch 2 H dkp, K behind Q) and split activations throughout."""
    pad8 = lambda v: (v + 7) & ~7                                                                    # noqa: E731
    dkp, dvp, tkp, tkv = pad8(dk), pad8(dv), pad8(Tk), (Tk + 31) // 32 * 32
    ldq, ldo = 2 * H * dkp, H * dvp
    qk = _case("model_qk", "T32", 0, Tq, Tk, dkp, batch=B * H, nh=H, lda=ldq, ldb=ldq, ldc=Tk, sAb=Tq * ldq, sAh=dkp,
               sBb=Tk * ldq, sBh=dkp, sCb=H * Tq * Tk, sCh=Tq * Tk, a_lo=True, b_lo=True)
    pv = _case("model_pv", "T32", 0, Tq, dvp, tkp, batch=B * H, nh=H, out_f32=0, lda=tkp, ldb=tkv, ldc=ldo,
               sAb=H * Tq * tkp, sAh=Tq * tkp, sBb=ldo * tkv, sBh=dvp * tkv, sCb=Tq * ldo, sCh=dvp, a_lo=True, b_lo=True,
               c_lo=True)
    return [qk, pv]


MODEL_CASES = model_layout_cases()


def _variant(kernel, feature, base, expect, **change):
    """`base` with `change` applied: a descriptor that asks `kernel` (through the base case's override) for `feature`.
    A base that is no longer in CASES leaves a stub the host test fails on (an assertion, not an import error)."""
    cid = f"{kernel.lower()}_no_{feature}"
    if base not in BY_ID:
        return dict(id=cid, kernel=kernel, expect=expect, feature=feature, base=base, missing_base=True,
                    features=frozenset(), extras=frozenset())
    c = dict(BY_ID[base])
    c.update(change)
    c.update(id=cid, kernel=kernel, expect=expect, feature=feature, base=base)
    c["features"], c["extras"] = features_of(c), extras_of(c)
    assert feature in c["features"], (c["id"], sorted(c["features"]))
    return c


# Pairs a kernel's predicate turns away with an error code (the launch never happens): a partial B_lo is a gemm_nt_wide
# feature, every other route answers PIO_E_SHAPE.
REFUSED = [_variant(k, "b_lo_from", b, "PIO_E_SHAPE", b_lo=True, a_lo=False, b_lo_n0=256) for k, b in (
    ("SKINNY2", "skinny2_dense"), ("SKINNY4", "skinny4"), ("STREAM", "stream_res_f32"), ("T256", "t256_scalar"),
    ("T128", "t128_scalar"), ("T128_KG2", "t128kg2_scalar"), ("T64", "t64_scalar"), ("T64_KG2", "t64kg2_scalar"),
    ("T32", "t32_scalar"), ("T32_KG2", "t32kg2_scalar"))]


def _rerouted():
    """Pairs a kernel's predicate hands to ANOTHER kernel (the same override, the kernel the driver then reports: under a
    non-zero override gemm_nt_128 on its 128 x 128 tile)."""
    out = [
        # gemm_nt_stream (gemm_stream_ok): flat residual rows only, vector epilogue only, per-column bias only
        _variant("STREAM", "res_rows", "stream_res_f32", "T128", r_rows=100, r_stride_b=100 * 268 + 8),
        _variant("STREAM", "res_unaligned", "stream_res_f32", "T128", r_off=1),
        _variant("STREAM", "c_unaligned", "stream_res_f32", "T128", c_off=2),
        _variant("STREAM", "bias_unaligned", "stream_res_f32", "T128", bias_off=1),
        _variant("STREAM", "bias_rows", "stream_res_f32", "T128", bias_mode=2),
        # gemm_nt_wide (gemm_wide_ok): one flat problem, the same epilogue limits
        _variant("WIDE", "heads_in_row_A", "stream_heads", "T128", override=2),
        _variant("WIDE", "heads_in_row_B", "stream_heads", "T128", override=2),
        _variant("WIDE", "heads_in_row_C", "stream_heads", "T128", override=2),
        _variant("WIDE", "batch_gap", "stream_heads", "T128", override=2),
        _variant("WIDE", "res_rows", "wide_a_lo_res_f32", "T128", r_rows=100, r_stride_b=100 * 268 + 8),
        _variant("WIDE", "res_unaligned", "wide_a_lo_res_f32", "T128", r_off=1),
        _variant("WIDE", "c_unaligned", "wide_16", "T128", c_off=2),
        _variant("WIDE", "bias_unaligned", "wide_16", "T128", bias_off=1),
        _variant("WIDE", "bias_rows", "wide_16", "T128", bias_mode=2),
    ]
    # the few-column kernel takes plain flat products only (gemm_route: `plain`, batch == 1)
    for k, b, M, K, ns in (("SKINNY2", "skinny2_dense", 2051, 72, 2), ("SKINNY4", "skinny4", 2051, 1032, 4)):
        r = dict(res=True, ldr=8, r_off=1, r_rows=100, r_stride_b=100 * 8 + 1)
        to = "T32" if K < 1024 else "T32_KG2"       # (one tile row of 32 x 64 tiles per 32 rows: K decides the teams)
        out += [_variant(k, f, b, to, **r) for f in ("ldr_pitch", "res_rows", "res_unaligned")]
        out += [_variant(k, "bias_rows", b, to, bias_mode=2), _variant(k, "c_lo", b, to, c_lo=True)]
        # two samples x two heads of the same few columns, heads inside a row, a gap between the samples
        h = dict(batch=4, nh=2, N=ns, lda=2 * K + 8, ldb=2 * K + 8, sAh=K, sBh=K, ldc=2 * ns + 4, sCh=ns, c_off=0, bias_off=0)
        h.update(sAb=M * h["lda"] + 8, sBb=ns * h["ldb"] + 8, sCb=M * h["ldc"] + 8)
        out += [_variant(k, f, b, "T32", **h) for f in ("heads_in_row_A", "heads_in_row_B", "heads_in_row_C", "batch_gap")]
    return out


REROUTED = _rerouted()

# (kernel, extra) pairs that must have a case: both copies of the epilogue (gemm_nt_128: T64 / T128; epilogue_store4:
# T256) on the vector residual load, the shared residual rows, a residual under 16-bit results and beside batched slices,
# the scalar 16-bit store; the persistent kernels' residual forms; both output types of the few-column kernel.
REQUIRED_EXTRA = [(k, e) for k in ("T64", "T128", "T256") for e in ("res_vec", "res_stride0", "res_16", "res_batched", "c16_scalar")]
REQUIRED_EXTRA += [("STREAM", "res_vec"), ("STREAM", "res_16"), ("STREAM", "out_f32"), ("WIDE", "res_vec"), ("WIDE", "res_16"),
                   ("WIDE", "out_f32"), ("WIDE", "out_16_plain"), ("SKINNY2", "out_f32"), ("SKINNY2", "out_16")]


# ----------------------------------------------------------------------------------------------------
# buffers
# ----------------------------------------------------------------------------------------------------
def slice_offsets(c, sb, sh):
    z = np.arange(c["batch"], dtype=np.int64)
    return (z // c["nh"]) * sb + (z % c["nh"]) * sh


def _index(offs, rows, ld, cols):
    """flat element index [Z, rows, cols] of a strided stack of matrices"""
    return offs[:, None, None] + np.arange(rows, dtype=np.int64)[None, :, None] * ld + np.arange(cols, dtype=np.int64)[None, None, :]


def residual_rows(c):
    """element offset of residual row m (pio_hip.h: the (stride_b, rows_per_batch) form, else m * ldr)"""
    m = np.arange(c["M"], dtype=np.int64)
    if c["r_rows"] > 0:
        return (m // c["r_rows"]) * c["r_stride_b"] + (m % c["r_rows"]) * c["ldr"]
    return m * c["ldr"]


def c_elements(c):
    """size of the C payload in elements: every slice's M whole pitches behind the pointer's offset"""
    return int(c["c_off"] + slice_offsets(c, c["sCb"], c["sCh"]).max() + c["M"] * c["ldc"]) + TAIL


def make_arrays(c):
    """The inputs as flat float32 payloads (integers, exact in fp16 and bf16); every element the contract calls unread --
    pitch columns, gaps between slices, B_lo rows below b_lo_n0, residual columns >= N, the bias behind its last entry,
    everything in front of an offset pointer -- is NaN."""
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    M, N, K = c["M"], c["N"], c["K"]
    out = {}
    ia = _index(slice_offsets(c, c["sAb"], c["sAh"]), M, c["lda"], K)
    ib = _index(slice_offsets(c, c["sBb"], c["sBh"]), N, c["ldb"], K)
    for name, idx, on in (("A", ia, True), ("A_lo", ia, c["a_lo"]), ("B", ib, True), ("B_lo", ib, c["b_lo"])):
        if not on:
            out[name] = None
            continue
        buf = np.full(int(idx.max()) + 1 + TAIL, np.nan, dtype=np.float32)
        buf[idx] = rng.integers(-3, 4, idx.shape).astype(np.float32)
        if name == "B_lo" and c["b_lo_n0"]:
            buf[idx[:, :c["b_lo_n0"], :]] = np.nan
        out[name] = buf
    out["bias"] = None
    if c["bias_mode"]:
        n = N if c["bias_mode"] == 1 else M
        out["bias"] = np.full(c["bias_off"] + n + TAIL, np.nan, dtype=np.float32)
        out["bias"][c["bias_off"]:c["bias_off"] + n] = rng.integers(-8, 9, n)
    out["R"] = None
    if c["res"]:
        ir = c["r_off"] + residual_rows(c)[:, None] + np.arange(N, dtype=np.int64)[None, :]
        out["R"] = np.full(int(ir.max()) + 1 + TAIL, np.nan, dtype=np.float32)
        out["R"][ir] = rng.integers(-16, 17, ir.shape)
    return out


# ----------------------------------------------------------------------------------------------------
# the reference: include/pio_hip.h, pio_gemm_t, restated in float64 from the strided buffers
# ----------------------------------------------------------------------------------------------------
def ref_gemm(c, arrays, magnitude=False):
    """-> (ref [batch, M, n_store] float64, index [batch, M, n_store] int64, pad [n_store] bool)
    ref: alpha * (A B^T + A B_lo^T [columns >= b_lo_n0] + A_lo B^T) + bias + R for columns < N (the A_lo B_lo^T term is
    dropped), 0 for the pad columns [N, n_store); slice z = zb * nh + zh, the residual indexed by the row alone.
    index: the element of the C payload each entry lives in -- exactly the elements the contract writes.
    magnitude=True: the same sum over absolute values (the bound exact_ok needs)."""
    M, N, K, ns = c["M"], c["N"], c["K"], c["n_store"]
    f = (lambda a: np.abs(a.astype(np.float64))) if magnitude else (lambda a: a.astype(np.float64))
    ia = _index(slice_offsets(c, c["sAb"], c["sAh"]), M, c["lda"], K)
    ib = _index(slice_offsets(c, c["sBb"], c["sBh"]), N, c["ldb"], K)
    A, B = f(arrays["A"][ia]), f(arrays["B"][ib])
    acc = A @ B.transpose(0, 2, 1)
    if c["b_lo"]:
        n0 = c["b_lo_n0"]
        acc[:, :, n0:] += A @ f(arrays["B_lo"][ib[:, n0:]]).transpose(0, 2, 1)
    if c["a_lo"]:
        acc += f(arrays["A_lo"][ia]) @ B.transpose(0, 2, 1)
    x = abs(c["alpha"]) * acc if magnitude else c["alpha"] * acc
    if c["bias_mode"] == 1:
        x += f(arrays["bias"][c["bias_off"]:c["bias_off"] + N])[None, None, :]
    elif c["bias_mode"] == 2:
        x += f(arrays["bias"][c["bias_off"]:c["bias_off"] + M])[None, :, None]
    if c["res"]:
        x += f(arrays["R"][c["r_off"] + residual_rows(c)[:, None] + np.arange(N)[None, :]])[None]
    ref = np.zeros((c["batch"], M, ns), dtype=np.float64)
    ref[:, :, :N] = x + 0.0          # (a zero result is +0 in every kernel: x - x and 0 * x + 0 round to +0)
    index = c["c_off"] + _index(slice_offsets(c, c["sCb"], c["sCh"]), M, c["ldc"], ns)
    return ref, index, np.arange(ns) >= N


def exact_ok(c, arrays):
    """|alpha| sum_k |a| |b| over all sweeps + |bias| + |R| < 2^24 for every element: every partial sum of every kernel is
    then an integer multiple of min(|alpha|, 1) that fp32 holds exactly -- also where a kernel adds bias / alpha and the
    residual BEFORE the products (gemm_nt_stream): alpha is a power of two and the same bound divided by it holds."""
    mag = ref_gemm(c, arrays, magnitude=True)[0]
    a = abs(c["alpha"])
    return a in (0.5, 1.0, 2.0) and bool(np.isfinite(mag).all()) and float(mag.max()) / min(a, 1.0) < 2.0 ** 24


def expected_images(c, ref, dt):
    """(C, C_lo or None) as float32 arrays holding the values the kernel must store: fp32 exactly, 16-bit the round-to-
    nearest-even image, C_lo the rounded remainder."""
    r32 = ref.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), ref)
    if c["out_f32"]:
        return r32, None
    hi = round_to(dt, r32)
    return hi, (round_to(dt, r32 - hi) if c["c_lo"] else None)
