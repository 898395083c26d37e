"""Seeded cases and the acceptance rule of flow_to_image (utils/flow_utils.py; perceiverio_pytorch_amd.flow_to_image and
pio_flow_to_image behind it), shared by tests/test_flow_image_host.py and tests/test_flow_image_gpu.py.  numpy only.

THE RULE.  steps123 reproduces the fp32 part of the definition with numpy's own separately rounded operations (clip with
the lower bound 0, radius, the maximum of every image on its own, + 1e-5, two divisions, radius again): u_n, v_n and rad_n
are exact, and so is the decision rad_n <= 1, which gets no tolerance.  From them reference_c evaluates the wheel position
and the colour in float64: c = 255 col, before the floor.  A byte y is accepted iff floor(c - DELTA) <= y <= floor(c + DELTA):
where c lies further than DELTA from an integer the byte must match exactly.

DELTA = 2e-3.  |dc/dfk| <= 64 (the steepest wheel segment changes by 255 in 4 steps); an fp32 evaluation of fk (up to 54,
ulp 3.8e-6) through an atan2f of a few ulp, a division and two more operations leaves a few ulp(54) of error in fk, about
1e-3 in c; DELTA is twice that.

So that the band cannot hide a wrong implementation, every case that is not planted must have fewer than 2 % of its channel
values inside the band (generic values: about 2 DELTA = 0.4 %).  One class of values is left out of that share because it
sits on an integer by construction, for every input: a channel whose wheel entries at k0 and k1 are both 255 has col = 1
and, inside the unit circle, c = 255 (1 - rad_n 0) = 255 exactly -- one channel of nearly every pixel -- and so has a pixel of
radius 0.  Rounding decides between 254 and 255 there (numpy's own float64 chain gives both); the rule accepts those two and
nothing else, and `share` counts the band over all OTHER values."""
import numpy as np

DELTA = 2e-3
BAND_CAP = 0.02
SEGMENTS = (15, 6, 4, 11, 13, 6)      # RY YG GC CB BM MR


def wheel():
    """[55, 3] float64, built here from the segment table (the host test compares it with utils.flow_utils')."""
    rows = []
    for s, n in enumerate(SEGMENTS):
        full, ramping = ((s + 1) // 2) % 3, (1 + 2 * s) % 3
        for i in range(n):
            ramp = np.floor(255 * i / n)
            row = [0.0, 0.0, 0.0]
            row[full] = 255.0
            row[ramping] = 255.0 - ramp if s % 2 else ramp
            rows.append(row)
    return np.array(rows, np.float64)


WHEEL = wheel()


def steps123(flow, clip=None, batch_wide_max=False):
    """(u_n, v_n, rad_n, s) in fp32 of a [b, h, w, 2] flow, every operation rounded on its own as numpy does.
    batch_wide_max: the WRONG maximum (one for the batch), for the test that tells the two apart."""
    flow = np.asarray(flow, np.float32)
    assert flow.ndim == 4 and flow.dtype == np.float32
    if clip is not None:
        flow = np.clip(flow, 0, clip)
    u, v = flow[..., 0], flow[..., 1]
    rad = np.sqrt(u * u + v * v)
    rmax = rad.max(axis=None if batch_wide_max else (1, 2), keepdims=True)
    s = (rmax + np.float32(1e-5)).astype(np.float32)
    un, vn = u / s, v / s
    radn = np.sqrt(un * un + vn * vn)
    assert un.dtype == vn.dtype == radn.dtype == np.float32
    return un, vn, radn, np.broadcast_to(s, (flow.shape[0], 1, 1))


def reference_c(flow, clip=None, batch_wide_max=False):
    """(c, white): c = 255 col in float64, RGB order, [b, h, w, 3]; white = the values that are 255 by construction."""
    un, vn, radn, _ = steps123(flow, clip, batch_wide_max)
    a = np.arctan2(-vn.astype(np.float64), -un.astype(np.float64)) / np.pi
    fk = (a + 1) / 2 * 54
    k0 = np.clip(np.floor(fk), 0, 54).astype(np.int64)
    k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
    f = (fk - k0)[..., None]
    col = (1 - f) * WHEEL[k0] / 255.0 + f * WHEEL[k1] / 255.0
    inside = (radn <= np.float32(1))[..., None]          # from the exact fp32 rad_n: no tolerance
    r = radn.astype(np.float64)[..., None]
    col = np.where(inside, 1 - r * (1 - col), col * 0.75)
    white = inside & (((WHEEL[k0] == 255) & (WHEEL[k1] == 255)) | (r == 0))
    return 255 * col, white


def bounds(c):
    return np.floor(c - DELTA), np.floor(c + DELTA)


def share(c, white):
    """Fraction of the values outside `white` that lie inside the band."""
    lo, hi = bounds(c)
    free = ~white
    return float(((lo != hi) & free).sum()) / max(1, int(free.sum()))


def check(img, flow, clip=None, bgr=False, what=""):
    """Assert the rule for the uint8 image(s) of flow ([b, h, w, 2] with [b, h, w, 3], or both without b); prints the
    figures first.  Returns the number of bytes that differ from floor(c)."""
    img, flow = np.asarray(img), np.asarray(flow, np.float32)
    if flow.ndim == 3:
        img, flow = img[None], flow[None]
    assert img.dtype == np.uint8 and img.shape == flow.shape[:3] + (3,), (what, img.dtype, img.shape, flow.shape)
    c, white = reference_c(flow, clip)
    y = (img[..., ::-1] if bgr else img).astype(np.float64)
    lo, hi = bounds(c)
    bad = (y < lo) | (y > hi)
    off = int((y != np.floor(c)).sum())
    print(f"{what}: {y.size} values, {int((lo != hi).sum())} in the band ({int(((lo != hi) & ~white).sum())} outside the "
          f"values that are 255 by construction), {off} differ from floor(c), {int(bad.sum())} rejected")
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {y.size} bytes outside the rule; first at {i}: got {y[i]:.0f}, "
                             f"c = {c[i]:.6f}")
    return off


def _randn(seed, shape, scale):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def _unit(seed, h, w):
    t = np.random.default_rng(seed).uniform(0, 2 * np.pi, (h, w))
    return np.stack([np.cos(t), np.sin(t)], axis=-1).astype(np.float32)


def _big():
    """Unit radii and ONE pixel of radius about 1e4 per image: s = fl(rad_max + 1e-5) = rad_max, so that pixel's rad_n lands
    above, on or below 1 by rounding alone -- image 0: (8418, 5398), rad_n = 1 + 2^-23 (the 0.75 branch); image 1:
    (10000, 0), rad_n = 1 exactly (the other branch); image 2: (-1240, 9923), rad_n = 1 - 2^-24."""
    f = np.stack([_unit(21, 9, 12), _unit(22, 9, 12), _unit(23, 9, 12)])
    f[0, 4, 5] = (8418.0, 5398.0)
    f[1, 2, 7] = (10000.0, 0.0)
    f[2, 8, 11] = (-1240.0, 9923.0)
    return f


def _signed_zero():
    """Row 0: v = +0.0, row 1: v = -0.0, u > 0 in both: atan2(-0, -u) = -pi (wheel entry 0) and atan2(+0, -u) = +pi (entry 54)."""
    f = np.zeros((1, 2, 8, 2), np.float32)
    f[0, :, :, 0] = np.linspace(0.5, 4.0, 8, dtype=np.float32)
    f[0, 1, :, 1] = -0.0
    assert not np.signbit(f[0, 0, :, 1]).any() and np.signbit(f[0, 1, :, 1]).all()
    return f


def _directions():
    """The eight axis and diagonal directions at radii 1, 2 and 3."""
    d = np.array([(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)], np.float32)
    return (d[None, :, :] * np.array([1, 2, 3], np.float32)[:, None, None])[None]


def _clip():
    """A field with negative components and components above 3, and two pixels with v = -0.0 and v = +0.0: np.clip leaves
    the sign of a zero alone."""
    f = _randn(5, (1, 12, 21, 2), 1.5)
    f[0, 3, 4] = (2.0, -0.0)
    f[0, 3, 5] = (2.0, 0.0)
    return f


def _batch3():
    f = _randn(31, (3, 17, 40, 2), 2.0)
    f[1] *= np.float32(50.0)
    f[2] *= np.float32(0.01)
    return f


# name -> flow [b, h, w, 2] fp32, clip, bgr, planted (exempt from the band-share cap), chw (handed over as a [2, h, w]
# array seen through .permute(1, 2, 0); b = 1)
CASES = {
    "5x7": dict(flow=lambda: _randn(3, (1, 5, 7, 2), 3.0)),                 # less than one wave, byte-store tail
    "33x130": dict(flow=lambda: _randn(2, (1, 33, 130, 2), 3.0)),           # row ends inside 4-pixel groups, several waves
    "64x256": dict(flow=lambda: _randn(3, (1, 64, 256, 2), 3.0)),           # whole groups only
    "batch3": dict(flow=_batch3),                                           # radii x1, x50, x0.01: one maximum per image
    "zero": dict(flow=lambda: np.zeros((1, 6, 9, 2), np.float32), planted=True),
    "signed_zero": dict(flow=_signed_zero, planted=True),
    "directions": dict(flow=_directions, planted=True),
    "big": dict(flow=_big, planted=True),
    "clip": dict(flow=_clip, clip=3.0),                                     # negative components: the lower bound is 0
    "bgr": dict(flow=lambda: _randn(6, (1, 8, 13, 2), 3.0), bgr=True),
    "permuted": dict(flow=lambda: _randn(7, (1, 11, 19, 2), 3.0), chw=True),
}
_DATA = {}


def gen(name):
    """The case's (read-only) flow, made once."""
    if name not in _DATA:
        f = np.ascontiguousarray(CASES[name]["flow"](), np.float32)
        f.setflags(write=False)
        _DATA[name] = f
    return _DATA[name]


def clip_of(name):
    return CASES[name].get("clip")


def bgr_of(name):
    return bool(CASES[name].get("bgr", False))


def planted(name):
    return bool(CASES[name].get("planted", False))


# ---- the raw entry -------------------------------------------------------------------------------------------------------
PIO_OK, PIO_E_SHAPE, PIO_E_ALIGN, PIO_E_ARG = 0, -1, -2, -6


def raw(L, flow_ptr, strides, b, h, w, out_ptr, rad_ptr, stream, clip=None, bgr=False):
    """pio_flow_to_image on raw pointers; strides = (sn, sy, sx, sc) in elements.  Returns the code."""
    sn, sy, sx, sc = strides
    return L.lib().pio_flow_to_image(flow_ptr, sn, sy, sx, sc, b, h, w, 0.0 if clip is None else float(clip),
                                     clip is not None, bool(bgr), out_ptr, rad_ptr, stream)


# (what, changes to the valid call of an [1, R_H, R_W, 2] flow, code): refused before anything is launched
R_H, R_W = 6, 10
REFUSALS = [
    ("null flow", dict(flow=None), PIO_E_ARG),
    ("null out", dict(out=None), PIO_E_ARG),
    ("null maxima", dict(rad=None), PIO_E_ARG),
    ("b = 0", dict(b=0), PIO_E_SHAPE),
    ("h < 0", dict(h=-3), PIO_E_SHAPE),
    ("w = 0", dict(w=0), PIO_E_SHAPE),
    ("h w beyond 2^31 - 1", dict(h=1 << 16, w=1 << 15), PIO_E_SHAPE),
    ("grid beyond 2^31 - 1", dict(b=0x7fffffff, h=1 << 15, w=1 << 15), PIO_E_SHAPE),
    ("flow not 4-byte aligned", dict(flow_offset=2), PIO_E_ALIGN),
]
