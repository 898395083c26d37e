"""Case tables of the range-probe tests (shared by tests/test_range_probe_host.py, which checks the tables and the CPU
backend, and tests/test_range_probe_gpu.py, which runs them on the kernels).  Seeded numpy / torch only.

Primitive cases.  pio_absmax16 reads rows x cols elements with row pitch ld (x batch, batch stride stride_b).  Every case
is laid out inside one allocation that is +inf wherever the kernel must not read: FENCE elements in front of x, the slack
columns [cols, ld) of every row (the last one included), the gap between two batches, and FENCE elements behind the last
row.  A single stray read turns the result into inf.
"""
import numpy as np

FENCE = 64
PLANT = -2048.0          # exact in fp16 and in bf16; far above the data (|N(0,1)| * 3 < 20)

# (rows, cols, ld): one element; fewer columns than one 16-byte piece; whole pieces with slack; the flow decoder's 328-wide
# rows contiguous (collapsed into one long row) and with 322 logical columns; more than one workgroup with a ragged tail
SHAPES = [(1, 1, 8), (3, 7, 8), (5, 8, 24), (64, 328, 328), (130, 322, 328), (257, 1030, 1088)]
# name: (batch, batch stride as a function of rows * ld, element offset of x from a 16-byte boundary)
LAYOUTS = {
    "plain": (1, lambda n: n, 0),
    "batch3": (3, lambda n: n + 13, 0),      # a stride larger than rows * ld (odd: every batch starts at another alignment)
    "stride0": (3, lambda n: 0, 0),          # stride_b = 0: one batch is read
    "offset2": (1, lambda n: n, 1),          # x two bytes behind a 16-byte boundary: the scalar head of every row
}
DTYPES = ("f16", "bf16")


def layout(shape, name):
    """dict(rows, cols, ld, batch, stride_b, base, total, nb): base = element offset of x inside the allocation (the
    allocation itself is at least 16-byte aligned), total = elements allocated, nb = batches actually read."""
    rows, cols, ld = shape
    batch, stride_of, mis = LAYOUTS[name]
    stride_b = stride_of(rows * ld)
    nb = batch if stride_b else 1
    base = FENCE + mis
    extent = (nb - 1) * stride_b + rows * ld
    return dict(rows=rows, cols=cols, ld=ld, batch=batch, stride_b=stride_b, base=base, total=base + extent + FENCE, nb=nb)


def index(lay, b, r, c):
    return lay["base"] + b * lay["stride_b"] + r * lay["ld"] + c


def fill(lay, seed, zero=False):
    """float32 image of the allocation: +inf everywhere, N(0,1) * 3 (or zeros) at the elements pio_absmax16 may read."""
    rng = np.random.default_rng(seed)
    buf = np.full(lay["total"], np.inf, np.float32)
    for b in range(lay["nb"]):
        for r in range(lay["rows"]):
            i = index(lay, b, r, 0)
            buf[i:i + lay["cols"]] = 0.0 if zero else rng.standard_normal(lay["cols"]).astype(np.float32) * 3
    return buf


def plant_positions(lay):
    """The four (b, r, c) the maximum is planted at in turn: first element, last element, last element of the first row,
    first element of the last batch."""
    return [(0, 0, 0), (lay["nb"] - 1, lay["rows"] - 1, lay["cols"] - 1), (0, 0, lay["cols"] - 1), (lay["nb"] - 1, 0, 0)]


# ---- block level ---------------------------------------------------------------------------------------------------------
POLICIES = ("fp16x3", "bf16x3")
# name: kind of block, then its shape
BLOCKS = {
    "self": dict(kind="self", D=64, H=2, N=64, B=2),
    "cross": dict(kind="cross", Cq=64, Ckv=40, H=2, Tq=32, Tk=96, B=2, mask=False),
    "cross_keymask": dict(kind="cross", Cq=64, Ckv=40, H=2, Tq=32, Tk=96, B=2, mask=True),
}
# One 16-bit rounding is 2^-9 (bf16) / 2^-12 (fp16) relative, the policies deviate by <= 1e-3 ~ 2^-10 on top: 2^-7 covers both
FIGURE_RTOL = 2.0 ** -7
# the CPU-backend hidden abs-max the overflow tests plant: beyond fp16 (65 504), far inside bf16
OVERFLOW_WINDOW = (1e5, 1e6)


def align(gpu, cpu):
    """Pair the HIP backend's records with the CPU backend's of the same forward: [(part, kind, gpu figure, cpu figure)].
    Both are lists of (part, kind, absmax) in call order.  The CPU backend records q, k and v one by one; a stacked q|k or
    q|k|v GEMM is ONE "q" record on the HIP backend, compared with the max over the CPU figures it covers.  Raises
    AssertionError when the sequences do not match."""
    out, j = [], 0
    for i, (part, kind, v) in enumerate(gpu):
        assert j < len(cpu), (i, part, kind, "the CPU backend has no record left")
        cpart, ckind, cv = cpu[j]
        assert (cpart, ckind) == (part, kind), (i, (part, kind), j, (cpart, ckind))
        j += 1
        nxt = gpu[i + 1][1] if i + 1 < len(gpu) else None
        if kind == "q" and nxt != "k":                  # stacked: q|k (a "v" record follows) or q|k|v (none does)
            take = 1 if nxt == "v" else 2
            assert [c[1] for c in cpu[j:j + take]] == ["k", "v"][:take], (i, cpu[j:j + take])
            cv = max([cv] + [c[2] for c in cpu[j:j + take]])
            j += take
        out.append((part, kind, v, cv))
    assert j == len(cpu), ("unmatched CPU records", cpu[j:])
    return out
