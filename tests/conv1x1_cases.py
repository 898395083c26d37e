"""The 1x1-conv front end (pio_conv1x1_tokens) as numpy: its float64 definition, the error bound any order of C fused
multiply-adds plus the bias term satisfies, the argument order of the entry point, its refusal table, and the shapes and
sources the GPU tests run.  Shapes are written (B, C, H, W, s, N)."""
import numpy as np

N_CAP = 1024            # _lib.PIO_CONV1X1_MAX_N (test_conv1x1_front_host.py holds the two equal)

ARG_ORDER = ("x", "sb", "sc", "sy", "sx", "w", "ldw", "bias", "y", "ldy", "sYb", "B", "C", "H", "W", "s", "N")
PIO_OK, E_SHAPE, E_ALIGN, E_ARG = 0, -1, -2, -6

# exact addressing: the smallest shapes that can still go wrong -- one pixel; one output pixel behind a stride of 8; an
# image row longer than a wave and no multiple of it; more than one strip per sample with the widest row the entry takes
EXACT_SHAPES = ((2, 3, 5, 7, 1, 8), (1, 1, 1, 1, 1, 4), (3, 4, 6, 10, 2, 12), (1, 3, 8, 8, 8, 4), (2, 3, 3, 67, 1, 256),
                (1, 2, 2, 130, 1, N_CAP))
SOURCES = ("contiguous", "channels_last", "batch_slice", "offset_one", "stride0_batch")


def gamma(k: int) -> float:
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


def reference(x, w, bias, s):
    """(y [B, OH*OW, N] float64, magnitude [B, OH*OW, N] = |bias| + sum |w x|) of the definition on float32 arrays
    x [B, C, H, W], w [N, C], bias [N] or None."""
    b, c, h, wd = x.shape
    assert h % s == 0 and wd % s == 0 and w.shape[1] == c
    px = x[:, :, ::s, ::s].astype(np.float64).reshape(b, c, -1)             # [B, C, M]
    w64 = w.astype(np.float64)
    y = np.einsum("nc,bcm->bmn", w64, px)
    mag = np.einsum("nc,bcm->bmn", np.abs(w64), np.abs(px))
    if bias is not None:
        y = y + bias.astype(np.float64)
        mag = mag + np.abs(bias.astype(np.float64))
    return y, mag


def exact_params(c, n):
    """w[n, c] = (c == n % C), bias[n] = n: y == x[b, n % C, i s, j s] + n, exactly, for small integer pixels."""
    w = np.zeros((n, c), dtype=np.float32)
    w[np.arange(n), np.arange(n) % c] = 1.0
    return w, np.arange(n, dtype=np.float32)


def exact_pixels(b, c, h, w):
    """Small distinct integers: every pixel of every plane of every sample its own value (sums with n <= 1023 stay far below
    2^24, where fp32 still counts)."""
    return np.arange(1, b * c * h * w + 1, dtype=np.float32).reshape(b, c, h, w)


def exact_expected(x, s, n):
    b, c = x.shape[:2]
    px = x[:, :, ::s, ::s].reshape(b, c, -1)                                 # [B, C, M]
    idx = np.arange(n)
    return (px[:, idx % c, :].transpose(0, 2, 1) + idx.astype(np.float32)[None, None, :]).astype(np.float32)


def _signed_pow10(rng, shape, lo, hi, zeros):
    v = np.power(10.0, rng.uniform(lo, hi, size=shape)) * rng.choice([-1.0, 1.0], size=shape)
    v[rng.random(size=shape) < zeros] = 0.0
    return v.astype(np.float32)


def accuracy_data(kind, shape, seed):
    """(x, w, bias) float32.  "wide": weights and pixels +-10^[-15, 15], the bias +-10^[-30, 30], a tenth of each zero -- every
    product and the bias lie in 1e-30 .. 1e30 or are zero, so no term underflows or overflows and the bound is one of
    rounding alone (a sum that cancels into the subnormal range is off by at most 2^-150 there, far below gamma * 1e-30).
    "image": normalised pixels in [-2.2, 2.7], the weights the module's initialiser draws (truncated normal, std 0.01),
    a small bias."""
    b, c, h, w, _, n = shape
    rng = np.random.default_rng(seed)
    if kind == "wide":
        return (_signed_pow10(rng, (b, c, h, w), -15, 15, 0.1), _signed_pow10(rng, (n, c), -15, 15, 0.1),
                _signed_pow10(rng, (n,), -30, 30, 0.1))
    x = rng.uniform(-2.2, 2.7, size=(b, c, h, w)).astype(np.float32)
    wt = np.clip(rng.normal(0.0, 0.01, size=(n, c)), -2.0, 2.0).astype(np.float32)
    return x, wt, rng.normal(0.0, 0.02, size=(n,)).astype(np.float32)


ACCURACY_CASES = (("wide", (2, 3, 5, 7, 1, 8)), ("wide", (1, 4, 6, 10, 2, 12)), ("wide", (1, 1, 3, 67, 1, 256)),
                  ("wide", (1, 2, 2, 130, 1, N_CAP)), ("image", (2, 3, 9, 71, 1, 256)), ("image", (1, 3, 16, 16, 4, 260)))


# refusal table: (what, {argument: value} over a valid call, code).  The valid call: B = 2, C = 3, H = 6, W = 8, s = 2,
# N = 8 -- OH*OW = 12 rows per sample.
VALID = dict(sb=144, sc=48, sy=8, sx=1, ldw=3, ldy=8, sYb=96, B=2, C=3, H=6, W=8, s=2, N=8)
REFUSALS = (
    ("x NULL", dict(x=None), E_ARG), ("w NULL", dict(w=None), E_ARG), ("y NULL", dict(y=None), E_ARG),
    ("B 0", dict(B=0), E_SHAPE), ("H 0", dict(H=0), E_SHAPE), ("W 0", dict(W=0), E_SHAPE),
    ("C 0", dict(C=0), E_SHAPE), ("C 5", dict(C=5, ldw=5), E_SHAPE),
    ("s 0", dict(s=0), E_SHAPE), ("s 9", dict(s=9, H=9, W=9), E_SHAPE),
    ("H % s", dict(H=7), E_SHAPE), ("W % s", dict(W=9), E_SHAPE),
    ("N 0", dict(N=0), E_SHAPE), ("N % 4", dict(N=6), E_SHAPE), ("N above the cap", dict(N=N_CAP + 4, ldy=N_CAP + 4,
                                                                                          sYb=12 * (N_CAP + 4)), E_SHAPE),
    ("ldw < C", dict(ldw=2), E_SHAPE), ("ldy < N", dict(ldy=4), E_SHAPE),
    ("sYb < rows * ldy", dict(sYb=92), E_SHAPE),
    ("2^31 rows", dict(B=2 ** 17, H=128, W=128, s=1, sYb=128 * 128 * 8), E_SHAPE),
    ("ldy % 4", dict(ldy=10, sYb=120), E_ALIGN), ("sYb % 4", dict(sYb=98), E_ALIGN),
    ("y 8-byte aligned", dict(y=0x50008), E_ALIGN), ("x 2-byte aligned", dict(x=0x10002), E_ALIGN),
    ("w 2-byte aligned", dict(w=0x30002), E_ALIGN), ("bias 2-byte aligned", dict(bias=0x40002), E_ALIGN),
)


def refusal_call(lib, changes):
    """pio_conv1x1_tokens on VALID with `changes` and made-up (aligned, non-NULL) addresses: a refused call returns before
    it touches a device or a pointer."""
    f = dict(VALID, x=0x10000, w=0x30000, bias=0x40000, y=0x50000)
    f.update(changes)
    return lib.pio_conv1x1_tokens(*[f[k] for k in ARG_ORDER], None)
