"""Cases and the definition of the output heads (pio_project_heads, csrc/pio_heads.hip).

Numpy only; shared by tests/test_heads_host.py (CPU: the header, the struct, the refusal table, eligibility, the chain on
CPU tensors against the definition) and tests/test_heads_gpu.py (MI355X: the kernel against the definition).

The definition restates the formula of include/pio_hip.h in float64 on the exact fp32 inputs:

    y_s[b, r, j] = bias_s[j] + sum_k w_s[j, k] x[b, row0_s + r, k]

Bound (derived, not measured): an fp32 dot product of K terms plus the bias, summed in ANY order, with or without FMA,
satisfies |y - ref| <= gamma_(K+1) mag,  gamma_n = n u / (1 - n u),  u = 2^-24,  mag = sum_k |w_k x_k| + |bias|
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).

Every input lives inside a larger array that is NaN around it: x is a row range of a [B, Q + 2, ldx] NaN array (x_sb >
Q ldx), NaN in the columns [K, ldx) and in every row no segment covers; the weights have NaN rows around them and NaN in
[K, ldw); the bias has NaN neighbours.  A kernel that reads one element outside what the formula addresses, even to multiply
it by zero, makes an output NaN.  y of a segment is a row range of a larger [B, rows + 3, y_rs] buffer."""
import numpy as np

PIO_OK, PIO_E_SHAPE, PIO_E_ALIGN, PIO_E_ARG = 0, -1, -2, -6
STRIP = 64          # rows per workgroup strip in csrc/pio_heads.hip (HD_TS): cases cross it on purpose
U = 2.0 ** -24


def seg(row0, rows, n_out, bias=True, y_rs=None, ldw_gap=0):
    return dict(row0=row0, rows=rows, n_out=n_out, bias=bias, y_rs=y_rs if y_rs is not None else n_out, ldw_gap=ldw_gap)


def _case(B, Q, K, segs, ldx=None):
    return dict(B=B, Q=Q, K=K, ldx=ldx if ldx is not None else K, segs=segs)


# name -> case.  K = 4, 8, 260 (a partial last sweep of the 64 lanes), 512, 1024; n_out = 1, 2, 3, 5, 16; B = 1 and 2;
# rows = 1, STRIP - 1, STRIP + 1, 257; ldx > K; three segments in one call, out of row order, with rows nobody covers;
# a zero-row segment; y_rs > n_out; bias = NULL.
CASES = {
    "k4_one_row": _case(1, 1, 4, [seg(0, 1, 1)]),
    "k8_n2_63": _case(2, STRIP - 1, 8, [seg(0, STRIP - 1, 2, y_rs=5)], ldx=12),
    "k260_n5_65": _case(2, STRIP + 1, 260, [seg(0, STRIP + 1, 5, bias=False, ldw_gap=4)], ldx=264),
    "k512_three": _case(2, 340, 512, [seg(70, 257, 3, y_rs=4), seg(2, STRIP, 16, ldw_gap=8), seg(339, 1, 1, bias=False)],
                        ldx=516),
    "k1024_n16": _case(1, 7, 1024, [seg(1, 5, 16, y_rs=20, ldw_gap=4)]),
    "zero_rows": _case(2, 6, 8, [seg(3, 0, 3), seg(1, 4, 2)]),
    "planted_nan": _case(2, 9, 260, [seg(0, 9, 3)], ldx=264),
}
PLANTED = {"planted_nan": (1, 4, 257)}      # case -> (b, row of x, k): one NaN element


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


def covered_rows(c):
    m = np.zeros(c["Q"], dtype=bool)
    for g in c["segs"]:
        m[g["row0"]:g["row0"] + g["rows"]] = True
    return m


def gen(name):
    """Inputs of a case: x_full [B, Q + 2, ldx] (x starts at element x_off: one row in), x_sb; per segment w_full
    [n_out + 2, ldw] (w_off: one row in), w [n_out, K], bias_full [n_out + 2] / bias (None without), ldw."""
    c = CASES[name]
    rng = np.random.default_rng(_seed(name))
    B, Q, K, ldx = c["B"], c["Q"], c["K"], c["ldx"]
    x_full = np.full((B, Q + 2, ldx), np.nan, dtype=np.float32)
    x = rng.standard_normal((B, Q, K)).astype(np.float32)
    x[:, ~covered_rows(c), :] = np.nan
    if name in PLANTED:
        b, r, k = PLANTED[name]
        x[b, r, k] = np.nan
    x_full[:, 1:1 + Q, :K] = x
    segs = []
    for g in c["segs"]:
        n, ldw = g["n_out"], K + g["ldw_gap"]
        w = (rng.standard_normal((n, K)) / np.sqrt(K)).astype(np.float32)
        w_full = np.full((n + 2, ldw), np.nan, dtype=np.float32)
        w_full[1:1 + n, :K] = w
        d = dict(w=w, w_full=w_full, w_off=ldw, ldw=ldw, bias=None, bias_full=None, bias_off=0)
        if g["bias"]:
            bias = rng.standard_normal(n).astype(np.float32)
            bf = np.full(n + 2, np.nan, dtype=np.float32)
            bf[1:1 + n] = bias
            d.update(bias=bias, bias_full=bf, bias_off=1)
        segs.append(d)
    return dict(x=x, x_full=x_full, x_off=ldx, x_sb=(Q + 2) * ldx, segs=segs)


def definition(x, w, bias):
    """(ref, mag) float64 [.., rows, n_out] of fp32 x [.., rows, K], w [n_out, K], bias [n_out] or None."""
    x64, w64 = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ref = x64 @ w64.T
        mag = np.abs(x64) @ np.abs(w64).T
        if bias is not None:
            ref = ref + np.asarray(bias, dtype=np.float64)
            mag = mag + np.abs(np.asarray(bias, dtype=np.float64))
    return ref, mag


def reference(name, data):
    """Per segment (ref, mag) [B, rows, n_out] float64; a planted NaN makes exactly that row NaN."""
    c = CASES[name]
    return [definition(data["x"][:, g["row0"]:g["row0"] + g["rows"]], d["w"], d["bias"])
            for g, d in zip(c["segs"], data["segs"])]


def bound(K, mag):
    n = K + 1
    return n * U / (1.0 - n * U) * mag


def assert_within_bound(got, ref, mag, K, what):
    """got [.., n_out] (numpy, any float type) against the float64 definition: element-wise derived bound; NaN exactly where
    the definition is NaN.  Prints the worst |y - ref| / bound."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN outputs differ from the definition's"
    assert np.isfinite(got[~nan]).all(), f"{what}: non-finite outputs (a read outside an input?)"
    err, bnd = np.abs(got - ref)[~nan], bound(K, mag)[~nan]
    if err.size == 0:
        return 0.0
    ratio = float((err / np.where(bnd > 0, bnd, 1.0))[bnd > 0].max()) if (bnd > 0).any() else 0.0
    print(f"{what}: max |y - ref| = {err.max():.3e}, worst |y - ref| / bound = {ratio:.3f}")
    bad = err > bnd
    if bad.any():
        i = int(np.argmax(err - bnd))
        raise AssertionError(f"{what}: element {i} of the finite ones: err {err[i]:.3e} bound {bnd[i]:.3e}")
    return ratio


Y_FRONT, Y_BACK = 2, 1      # rows of the enclosing y buffer in front of and behind a segment's rows, per sample


def y_rows(g):
    return Y_FRONT + g["rows"] + Y_BACK


def call_fields(name, data, addr):
    """The call of a case as plain values: (list of per-segment field dicts of pio_head_segment_t, keyword arguments).
    addr(what) -> byte address of the enclosing array: "x", or (segment index, "w" / "bias" / "y"); y of segment i is a
    [B, y_rows, y_rs] buffer whose rows [Y_FRONT, Y_FRONT + rows) of every sample the call writes."""
    c = CASES[name]
    segs = []
    for i, (g, d) in enumerate(zip(c["segs"], data["segs"])):
        segs.append(dict(row0=g["row0"], rows=g["rows"], n_out=g["n_out"], w=addr((i, "w")) + 4 * d["w_off"], ldw=d["ldw"],
                         bias=None if d["bias"] is None else addr((i, "bias")) + 4 * d["bias_off"],
                         y=addr((i, "y")) + 4 * Y_FRONT * g["y_rs"], y_sb=y_rows(g) * g["y_rs"], y_rs=g["y_rs"]))
    return segs, dict(x=addr("x") + 4 * data["x_off"], x_sb=data["x_sb"], ldx=c["ldx"], B=c["B"], Q=c["Q"], K=c["K"])


# ----------------------------------------------------------------------------------------------------
# refusals: (name, ONE change to the valid call, expected code).  The valid call: B = 2, Q = 12, K = 8, ldx = 8, x_sb = 104;
# segment 0 rows [0, 5) -> 3 columns (y_rs 4), segment 1 rows [6, 10) -> 16 columns (ldw 12), both with a bias.  A change is
# keyed by an argument name, or by (segment, field); "ptr+<b>": that pointer moved by b bytes; None: a NULL pointer.
# ----------------------------------------------------------------------------------------------------
VALID_ARGS = dict(nseg=2, x_sb=104, ldx=8, B=2, Q=12, K=8)
VALID_SEGS = [
    dict(row0=0, rows=5, n_out=3, ldw=8, y_sb=40, y_rs=4),
    dict(row0=6, rows=4, n_out=16, ldw=12, y_sb=64, y_rs=16),
]
POINTER_FIELDS = ("w", "bias", "y")
REFUSALS = [
    ("x NULL", {"x": None}, PIO_E_ARG),
    ("w NULL", {(0, "w"): None}, PIO_E_ARG),
    ("y NULL", {(1, "y"): None}, PIO_E_ARG),
    ("nseg=0", {"nseg": 0}, PIO_E_ARG),
    ("nseg=5", {"nseg": 5}, PIO_E_ARG),
    ("B=0", {"B": 0}, PIO_E_SHAPE),
    ("Q=0", {"Q": 0}, PIO_E_SHAPE),
    ("K=0", {"K": 0}, PIO_E_SHAPE),
    ("K=6", {"K": 6}, PIO_E_SHAPE),
    ("K=1028", {"K": 1028}, PIO_E_SHAPE),
    ("ldx<K", {"ldx": 4}, PIO_E_SHAPE),
    ("n_out=0", {(0, "n_out"): 0}, PIO_E_SHAPE),
    ("n_out=17", {(1, "n_out"): 17}, PIO_E_SHAPE),
    ("rows=-1", {(0, "rows"): -1}, PIO_E_SHAPE),
    ("row0=-1", {(0, "row0"): -1}, PIO_E_SHAPE),
    ("segment past Q", {(1, "row0"): 9}, PIO_E_SHAPE),
    ("ldw<K", {(0, "ldw"): 4}, PIO_E_SHAPE),
    ("y_rs<n_out", {(0, "y_rs"): 2}, PIO_E_SHAPE),
    ("segments overlap", {(1, "row0"): 4}, PIO_E_SHAPE),
    ("x 8-byte aligned", {"x": "ptr+8"}, PIO_E_ALIGN),
    ("w 4-byte aligned", {(1, "w"): "ptr+4"}, PIO_E_ALIGN),
    ("ldx % 4", {"ldx": 10}, PIO_E_ALIGN),
    ("ldw % 4", {(0, "ldw"): 10}, PIO_E_ALIGN),
    ("x_sb % 4", {"x_sb": 106}, PIO_E_ALIGN),
    ("y misaligned", {(0, "y"): "ptr+2"}, PIO_E_ALIGN),
    ("bias misaligned", {(1, "bias"): "ptr+2"}, PIO_E_ALIGN),
]


def refusal_fields(ptrs, changes):
    """The valid call with `changes` applied: (segment field dicts, keyword arguments).  ptrs: "x" -> address,
    (segment, field) -> address for every field of POINTER_FIELDS."""
    args = dict(VALID_ARGS, x=ptrs["x"])
    segs = [dict(g, **{f: ptrs[(i, f)] for f in POINTER_FIELDS}) for i, g in enumerate(VALID_SEGS)]

    def moved(p, v):
        return None if v is None else p + int(v[4:])
    for k, v in changes.items():
        if k == "x":
            args["x"] = moved(args["x"], v)
        elif isinstance(k, tuple):
            segs[k[0]][k[1]] = moved(segs[k[0]][k[1]], v) if k[1] in POINTER_FIELDS else v
        else:
            args[k] = v
    return segs, args
