"""Seeded cases of the media samples (perceiverio_pytorch_amd.to_frames / to_pcm16, media.restatement and pio_finish_media
behind them), shared by tests/test_media_host.py and tests/test_media_gpu.py.  numpy only.

THE RULE is equality of bytes.  `numpy_formula` is what example_multimodal.py computes on the host --
(np.clip(a, 0, 1) * 255).astype(np.uint8) and (a * 2**15).astype(np.int16) -- and is defined for `in_range` values (U8: no
NaN; S16: trunc(a * 2**15) inside int16).  `definition` is the entry's own formula in numpy, which adds the documented
values where numpy is undefined: a NaN gives 0, an int16 sample saturates.

Every case is a logical fp32 array [n, h, w, C] that begins with the special values of its kind and goes on with seeded
random ones, a layout that says how it sits in memory (`place`), and for U8 whether the channels are reversed."""
import numpy as np

U8, S16 = 0, 1
ULP1 = np.float32(2.0 ** -23)            # ulp of 1.0


def _f32(vals):
    return np.array(vals, np.float32)


def u8_values():
    """+-0, a denormal, j / 255 and its two fp32 neighbours for a handful of j, 1 - ulp, 1, 1 + ulp, negatives, 1e30, +-inf, NaN."""
    vals = [0.0, -0.0, 1e-40, -1e-40]
    for j in (1, 2, 3, 64, 127, 128, 200, 254):
        x = np.float32(j) / np.float32(255)
        vals += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(2))]
    vals += [np.nextafter(np.float32(1), np.float32(0)), 1.0, np.float32(1) + ULP1, -0.25, -3.0, -1e30, 1e30, np.inf, -np.inf,
             np.nan]
    return _f32(vals)


def s16_values():
    """+-0, +-1, -1 - ulp, 32767 / 32768, 32767.5 / 32768, +-(1 + ulp), +-inf, NaN, and a few plain ones."""
    one = np.float32(1)
    return _f32([0.0, -0.0, 1.0, -1.0, -one - ULP1, 32767.0 / 32768.0, 32767.5 / 32768.0, one + ULP1, -(one + ULP1), np.inf,
                 -np.inf, np.nan, 0.5, -0.5, 1.0 / 32768.0, -1.0 / 32768.0, 0.9 / 32768.0, -0.9 / 32768.0, 1e-40, 3.0, -3.0,
                 1e30, -1e30])


def in_range(a, kind):
    """Where numpy's own formula is defined."""
    a = np.asarray(a, np.float32)
    if kind == U8:
        return ~np.isnan(a)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.trunc(a.astype(np.float64) * 32768.0)
    return np.isfinite(a) & (t >= -32768) & (t <= 32767)


def numpy_formula(a, kind):
    """The example's expression, fp32 throughout.  Only meaningful where in_range."""
    a = np.asarray(a, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == U8:
            return (np.clip(a, 0, 1) * 255).astype(np.uint8)
        return (a * 2 ** 15).astype(np.int16)


def definition(a, kind, reverse=False):
    """pio_finish_media's formula in numpy: contiguous uint8 / int16 of a's shape."""
    a = np.asarray(a, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == U8:
            v = np.where(a > 0, np.where(a > 1, np.float32(1), a), np.float32(0)).astype(np.float32)
            y = (v * np.float32(255)).astype(np.float32).astype(np.int32).astype(np.uint8)
            return np.ascontiguousarray(y[..., ::-1] if reverse else y)
        assert not reverse
        t = (a * np.float32(32768)).astype(np.float32)
        c = np.where(np.isnan(t), np.float32(0), np.clip(t, np.float32(-32768), np.float32(32767)))
        return np.ascontiguousarray(c.astype(np.int32).astype(np.int16))


# name -> kind, shape (n, h, w, C), layout, reverse, x_off (elements in front of the array: 1 breaks the 16-byte alignment)
#   flat       contiguous [n, h, w, C]
#   batch_gap  contiguous images, 7 elements between two of them (a batch stride larger than the image)
#   chw        channels-first storage [n, C, h, w] seen as [n, h, w, C]
#   crop       rows of w + 3 pixels of which w are read (rows not adjacent: nothing collapses)
CASES = {
    "u8_p1": dict(kind=U8, shape=(1, 1, 1, 3)),                                 # one pixel: the tail group alone
    "u8_p3_w1": dict(kind=U8, shape=(1, 3, 1, 3)),                              # w = 1
    "u8_p4_c4": dict(kind=U8, shape=(1, 2, 2, 4)),                              # exactly one full group
    "u8_p5_c1": dict(kind=U8, shape=(1, 1, 5, 1)),                              # a full group and a tail
    "u8_c2": dict(kind=U8, shape=(1, 5, 9, 2), reverse=True),
    "u8_p1027": dict(kind=U8, shape=(1, 13, 79, 3)),                            # 1027 pixels: a second workgroup, a tail of 3
    "u8_p1027_c4": dict(kind=U8, shape=(1, 13, 79, 4), reverse=True),
    "u8_p1027_off": dict(kind=U8, shape=(1, 13, 79, 3), x_off=1),               # x 4-byte but not 16-byte aligned
    "u8_n3_flat": dict(kind=U8, shape=(3, 7, 49, 3), reverse=True),             # images adjacent, 1029 pixels
    "u8_n3_gap": dict(kind=U8, shape=(3, 5, 7, 3), layout="batch_gap"),
    "u8_n3_gap_big": dict(kind=U8, shape=(3, 19, 23, 1), layout="batch_gap"),   # 1311 pixels through the strided walk
    "u8_chw": dict(kind=U8, shape=(3, 9, 11, 3), layout="chw", reverse=True),
    "u8_chw_w1": dict(kind=U8, shape=(2, 5, 1, 4), layout="chw"),
    "u8_crop": dict(kind=U8, shape=(2, 6, 10, 4), layout="crop"),
    "s16_p1": dict(kind=S16, shape=(1, 1, 1, 1)),
    "s16_p3": dict(kind=S16, shape=(1, 1, 3, 1)),
    "s16_p4": dict(kind=S16, shape=(1, 1, 4, 1)),
    "s16_p5_w1": dict(kind=S16, shape=(1, 5, 1, 1)),
    "s16_p1027": dict(kind=S16, shape=(1, 1, 1027, 1)),
    "s16_p1027_c3": dict(kind=S16, shape=(1, 13, 79, 3)),
    "s16_p1027_off": dict(kind=S16, shape=(1, 1, 1027, 1), x_off=1),
    "s16_n3_gap_c4": dict(kind=S16, shape=(3, 5, 7, 4), layout="batch_gap"),
    "s16_chw_c2": dict(kind=S16, shape=(2, 9, 11, 2), layout="chw"),
    "s16_crop": dict(kind=S16, shape=(3, 8, 45, 1), layout="crop"),             # 1080 pixels
}
# byte offsets of y inside its buffer that the GPU test runs a case at (0: 16-byte aligned): every alignment class
Y_OFFSETS = {"u8_p1027": (0, 1, 2, 4), "u8_p1027_c4": (0, 1, 2, 4, 8), "u8_p5_c1": (0, 1, 2), "u8_c2": (0, 4, 8),
             "s16_p1027": (0, 2, 4, 8), "s16_p1027_c3": (0, 2, 4, 8), "s16_n3_gap_c4": (0, 2, 4, 8), "s16_chw_c2": (0, 2, 8),
             "s16_p5_w1": (0, 2)}
_DATA = {}


def gen(name):
    """The case's (read-only) logical array [n, h, w, C], made once: the special values of its kind, then seeded random ones
    (U8: uniform in [-0.25, 1.25]; S16: uniform in [-1, 1), every one in range)."""
    if name not in _DATA:
        c = CASES[name]
        size = int(np.prod(c["shape"]))
        rng = np.random.default_rng(sum(name.encode()) * 7919 + 17)
        if c["kind"] == U8:
            special, rest = u8_values(), rng.uniform(-0.25, 1.25, size).astype(np.float32)
        else:
            special, rest = s16_values(), rng.uniform(-1.0, 1.0, size).astype(np.float32)
            rest = np.minimum(rest, np.nextafter(np.float32(1), np.float32(0)))
        k = min(size, len(special))
        rest[:k] = special[:k]
        a = rest.reshape(c["shape"])
        a.setflags(write=False)
        _DATA[name] = a
    return _DATA[name]


def place(name):
    """(storage, offset, strides): a 1-D fp32 array of junk in which the case's array sits as its layout says -- element
    (i, r, p, c) at storage[offset + i*sn + r*sy + p*sx + c*sc], strides = (sn, sy, sx, sc) in elements."""
    c, a = CASES[name], gen(name)
    n, h, w, ch = a.shape
    layout, x_off = c.get("layout", "flat"), c.get("x_off", 0)
    if layout == "flat":
        shape, view = (n, h, w, ch), lambda s: s
    elif layout == "batch_gap":
        shape, view = (n, h * w * ch + 7), None             # (a strided view of the rows' heads, made below)
    elif layout == "chw":
        shape, view = (n, ch, h, w), lambda s: s.transpose(0, 2, 3, 1)
    elif layout == "crop":
        shape, view = (n, h, w + 3, ch), lambda s: s[:, :, :w]
    else:
        raise KeyError(layout)
    rng = np.random.default_rng(5)
    storage = rng.uniform(0.3, 0.6, x_off + int(np.prod(shape))).astype(np.float32)      # junk that is no special value
    body = storage[x_off:].reshape(shape)
    if layout == "batch_gap":
        v = np.lib.stride_tricks.as_strided(body, (n, h, w, ch), (body.strides[0], 4 * w * ch, 4 * ch, 4))
    else:
        v = view(body)
    v[...] = a
    off = (v.__array_interface__["data"][0] - storage.__array_interface__["data"][0]) // 4
    return storage, int(off), tuple(int(s) // 4 for s in v.strides)


def reverse_of(name):
    return bool(CASES[name].get("reverse", False))


def kind_of(name):
    return CASES[name]["kind"]


# ---- the raw entry -------------------------------------------------------------------------------------------------------
PIO_OK, PIO_E_SHAPE, PIO_E_ALIGN, PIO_E_ARG = 0, -1, -2, -6


def raw(L, x_ptr, strides, shape, kind, reverse, y_ptr, stream):
    """pio_finish_media on raw pointers; strides = (sn, sy, sx, sc) in elements, shape = (n, h, w, C).  Returns the code."""
    sn, sy, sx, sc = strides
    n, h, w, c = shape
    return L.lib().pio_finish_media(x_ptr, sn, sy, sx, sc, n, h, w, c, kind, int(reverse), y_ptr, stream)


# (what, changes to the valid call of a contiguous [1, R_H, R_W, 3] array as PIO_MEDIA_U8, code)
R_H, R_W, R_C = 6, 10, 3
REFUSALS = [
    ("null x", dict(x=None), PIO_E_ARG),
    ("null y", dict(y=None), PIO_E_ARG),
    ("unknown kind", dict(kind=2), PIO_E_ARG),
    ("negative kind", dict(kind=-1), PIO_E_ARG),
    ("reverse with int16", dict(kind=S16, reverse=1), PIO_E_ARG),
    ("n = 0", dict(n=0), PIO_E_SHAPE),
    ("h < 0", dict(h=-3), PIO_E_SHAPE),
    ("w = 0", dict(w=0), PIO_E_SHAPE),
    ("C = 0", dict(C=0), PIO_E_SHAPE),
    ("C = 5", dict(C=5), PIO_E_SHAPE),
    ("h w beyond 2^31 - 1", dict(h=1 << 16, w=1 << 15), PIO_E_SHAPE),
    ("grid beyond 2^31 - 1", dict(n=0x7fffffff, h=1 << 15, w=1 << 15), PIO_E_SHAPE),
    ("x not 4-byte aligned", dict(x_offset=2), PIO_E_ALIGN),
    ("int16 y not 2-byte aligned", dict(kind=S16, y_offset=1), PIO_E_ALIGN),
]
