"""Cases, tolerance and the float64 definition of pio_prepare_images / prepare_images (include/pio_hip.h), shared by
tests/test_image_prep_host.py and tests/test_image_prep_gpu.py.

The definition: per axis a weight matrix W [out, in] (`axis_weights`: indices and numerators in integer arithmetic, which
is exact, one float64 division per weight), then v = Wy . crop . Wx^T per channel, the channel reversal, (v - mean) / std."""
import numpy as np

MAX_SOURCES = 32        # _lib.PIO_MAX_IMAGE_SOURCES (test_image_prep_host.py holds the two equal)
MAX_REDUCTION = 40      # _lib.PIO_IMAGE_MAX_REDUCTION
U = 2.0 ** -24          # unit roundoff of fp32


def axis_weights(n_in, n_out, antialias):
    """(W float64 [n_out, n_in], the largest tap count)."""
    W = np.zeros((n_out, n_in), np.float64)
    taps = 0
    for i in range(n_out):
        c2 = (2 * i + 1) * n_in
        if antialias:
            d = 2 * max(n_in, n_out)
            a, b = c2 - d + n_out, c2 + d + n_out
            lo = a // (2 * n_out) if a > 0 else 0
            hi = min(n_in, b // (2 * n_out))
            j = np.arange(lo, hi)
            r = np.maximum(0.0, 1.0 - np.abs((2 * j + 1) * n_out - c2) / d)
            W[i, lo:hi] = r / r.sum()
            taps = max(taps, hi - lo)
        else:
            q = max(0, c2 - n_out)
            j0 = min(q // (2 * n_out), n_in - 1)
            j1 = min(j0 + 1, n_in - 1)
            lam = (q - 2 * n_out * j0) / (2 * n_out)
            W[i, j0] += 1.0 - lam
            W[i, j1] += lam
            taps = max(taps, 2)
    return W, taps


def axis_windows(n_in, n_out, antialias):
    """(lo, hi) arrays: output index i has its taps on the crop indices [lo[i], hi[i])."""
    W, _ = axis_weights(n_in, n_out, antialias)
    if not antialias:
        return np.array([np.flatnonzero(r)[0] for r in W]), np.array([min(np.flatnonzero(r)[0] + 2, n_in) for r in W])
    i = np.arange(n_out)
    d, c2 = 2 * max(n_in, n_out), (2 * i + 1) * n_in
    return np.maximum(0, c2 - d + n_out) // (2 * n_out), np.minimum(n_in, (c2 + d + n_out) // (2 * n_out))


def axis_weights_literal(n_in, n_out, antialias):
    """The same matrix from the formulas as they are usually written, in float64 (scale * (i + 0.5) and so on): what
    axis_weights restates in integers.  Differs from it by float64 rounding only (test_image_prep_host.py)."""
    W = np.zeros((n_out, n_in), np.float64)
    scale = n_in / n_out
    for i in range(n_out):
        if antialias:
            support, centre = max(scale, 1.0), scale * (i + 0.5)
            lo, hi = max(0, int(centre - support + 0.5)), min(n_in, int(centre + support + 0.5))
            j = np.arange(lo, hi)
            r = np.maximum(0.0, 1.0 - np.abs(j + 0.5 - centre) / support)
            W[i, lo:hi] = r / r.sum()
        else:
            s = max(0.0, (2 * i + 1) * n_in / (2 * n_out) - 0.5)
            j0 = min(int(np.floor(s)), n_in - 1)
            j1 = min(j0 + 1, n_in - 1)
            W[i, j0] += 1.0 - (s - j0)
            W[i, j1] += s - j0
    return W


def restate(x, box, size, antialias, reverse, mean, std):
    """x [C, H, W] (any numeric dtype) -> (float64 [C, oh, ow], t_y, t_x)."""
    top, left, ch, cw = box
    oh, ow = size if size is not None else (ch, cw)
    Wy, ty = axis_weights(ch, oh, antialias)
    Wx, tx = axis_weights(cw, ow, antialias)
    crop = np.asarray(x, np.float64)[:, top:top + ch, left:left + cw]
    v = np.matmul(np.matmul(Wy, crop), Wx.T)
    if reverse:
        v = v[::-1]
    m = np.asarray(np.float32(mean), np.float64).reshape(-1, 1, 1)
    s = np.asarray(np.float32(std), np.float64).reshape(-1, 1, 1)
    return (v - m) / s, ty, tx


def tolerance(r64, ty, tx, xmax, std):
    """|r - r64| <= gamma_n max|x| / |std| + 2 u |r64|, n = 2 (t_y + t_x) + 8: at most t + 3 roundings in a normalised weight
    (one division, one subtraction, t - 1 additions of the normaliser, one division) and t in a pass (one fmaf per tap), for
    both passes, with non-negative weights that sum to one; the two roundings of the subtraction and the division behind
    them are the second term.  The kernel's chains are the ones counted, so n is the issue's."""
    n = 2 * (ty + tx) + 8
    gamma = n * U / (1.0 - n * U)
    s = np.abs(np.asarray(np.float32(std), np.float64)).reshape(-1, 1, 1)
    return gamma * xmax / s + 2 * U * np.abs(r64)


def center_box(h, w):
    m = min(h, w)
    return int(h / 2 - m / 2), int(w / 2 - m / 2), m, m


# name -> dict(imgs=[(H, W, dtype, layout)], C, size, crop, aa, rev, mean, std, batch (one [N, ..] tensor), window (the
# source is a strided view: rows 3 .., every second column of a larger array))
_D = dict(C=3, size=(16, 24), crop=None, aa=True, rev=False, mean=None, std=None, batch=False, window=False)
CLS_MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)
CLS_STD = (0.229 * 255, 0.224 * 255, 0.225 * 255)


def _case(**kw):
    return dict(_D, **kw)


CASES = {
    "ident_u8": _case(imgs=[(5, 7, "u8", "cl")], size=None, mean=(1.0, 2.0, 3.0), std=(2.0, 3.0, 7.0)),
    "ident_f32": _case(imgs=[(5, 7, "f32", "cf")], size=None, aa=False, mean=0.25, std=3.0),
    "ident_sized": _case(imgs=[(5, 7, "u8", "cf")], size=(5, 7), mean=127.5, std=127.5),
    "down_aa": _case(imgs=[(37, 53, "u8", "cl")]),
    "down_noaa": _case(imgs=[(37, 53, "u8", "cf")], aa=False),
    "up_aa": _case(imgs=[(7, 5, "f32", "cf")], C=1),
    "up_noaa": _case(imgs=[(7, 5, "u8", "cl")], C=4, aa=False),
    "c4_f32_cl": _case(imgs=[(37, 53, "f32", "cl")], C=4, rev=True, mean=(1.0, 2.0, 3.0, 4.0), std=(2.0, 4.0, 8.0, 255.0)),
    "c4_u8_cl_box": _case(imgs=[(37, 53, "u8", "cl")], C=4, crop=(1, 3, 30, 41)),
    "c1_u8": _case(imgs=[(37, 53, "u8", "cf")], C=1, std=255.0),
    "taps_33_65": _case(imgs=[(130, 257, "u8", "cl")], size=(8, 8)),
    "ragged": _case(imgs=[(40, 150, "u8", "cl")], size=(13, 70)),
    "real_center": _case(imgs=[(500, 375, "u8", "cl")], size=(224, 224), crop="center", mean=CLS_MEAN, std=CLS_STD),
    "reverse": _case(imgs=[(37, 53, "u8", "cl")], rev=True, mean=(10.0, 20.0, 30.0), std=(1.0, 2.0, 4.0)),
    "window": _case(imgs=[(37, 53, "u8", "cl")], window=True),
    "window_f32_cf": _case(imgs=[(37, 53, "f32", "cf")], window=True, aa=False),
    "box_top_left": _case(imgs=[(20, 30, "u8", "cl")], crop=(0, 0, 9, 11), size=(4, 4)),
    "box_bottom_right": _case(imgs=[(20, 30, "u8", "cl")], crop=(11, 19, 9, 11), size=(4, 4)),
    "box_1x1": _case(imgs=[(20, 30, "f32", "cf")], crop=(7, 9, 1, 1), size=(4, 4)),
    # (a one-pixel-WIDE antialiased output is left out of the table: there ATen's CPU kernel departs from the definition --
    #  14.6 of 255 at 37 x 53 -> 16 x 1 -- so the chain cannot be held to it; test_image_prep_gpu.py holds the kernel to it)
    "one_wide_noaa": _case(imgs=[(37, 53, "u8", "cl")], crop=(0, 5, 37, 33), size=(16, 1), aa=False),
    "one_high": _case(imgs=[(37, 53, "u8", "cl")], size=(1, 24)),
    "batch3": _case(imgs=[(37, 53, "u8", "cl")] * 3, batch=True, crop="center"),
    "batch3_boxes": _case(imgs=[(20, 30, "f32", "cf")] * 3, batch=True, crop=[(0, 0, 20, 30), (2, 3, 10, 9), (5, 0, 15, 30)]),
    "list3": _case(imgs=[(37, 53, "u8", "cl"), (20, 64, "f32", "cf"), (61, 33, "u8", "cf")], crop="center"),
    "many": _case(imgs=[(4, 4, "u8", "cl")] * (MAX_SOURCES + 1), size=(3, 5)),
}


def gen(name):
    """The case's images as numpy arrays in the logical [C, H, W] order (uint8, or float32 values in [0, 255])."""
    spec = CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 7)
    imgs = []
    for h, w, dt, _ in spec["imgs"]:
        if dt == "u8":
            imgs.append(rng.integers(0, 256, (spec["C"], h, w)).astype(np.uint8))
        else:
            imgs.append((rng.random((spec["C"], h, w)) * 255).astype(np.float32))
    return imgs


def boxes_of(name):
    spec, crop = CASES[name], CASES[name]["crop"]
    shapes = [(h, w) for h, w, _, _ in spec["imgs"]]
    if crop is None:
        return [(0, 0, h, w) for h, w in shapes]
    if crop == "center":
        return [center_box(h, w) for h, w in shapes]
    return [tuple(crop)] * len(shapes) if isinstance(crop[0], int) else [tuple(b) for b in crop]


def per_channel(v, c, default):
    return [default] * c if v is None else [float(v)] * c if isinstance(v, (int, float)) else list(v)


def expected(name):
    """[(r64 [C, oh, ow], tolerance array)] per image of the case."""
    spec = CASES[name]
    c = spec["C"]
    mean, std = per_channel(spec["mean"], c, 0.0), per_channel(spec["std"], c, 1.0)
    out = []
    for x, box in zip(gen(name), boxes_of(name)):
        r64, ty, tx = restate(x, box, spec["size"], spec["aa"], spec["rev"], mean, std)
        out.append((r64, tolerance(r64, ty, tx, float(np.abs(x.astype(np.float64)).max()), std)))
    return out


def torch_inputs(name, device):
    """What the case passes to prepare_images: (images, kwargs).  Every image in the layout the case names; `window`: seen
    through a view of a larger array (rows 3 .., every second column)."""
    import torch
    spec = CASES[name]
    tens = []
    for x, (_, _, _, layout) in zip(gen(name), spec["imgs"]):
        t = torch.from_numpy(x)
        if spec["window"]:
            big = torch.zeros((x.shape[0], x.shape[1] + 5, 2 * x.shape[2] + 3), dtype=t.dtype)
            big[:, 3:3 + x.shape[1], 1:1 + 2 * x.shape[2]:2] = t
            big = big.permute(1, 2, 0).contiguous().to(device) if layout == "cl" else big.to(device)
            big = big.permute(2, 0, 1) if layout == "cl" else big
            t = big[:, 3:3 + x.shape[1], 1:1 + 2 * x.shape[2]:2]
            t = t.permute(1, 2, 0) if layout == "cl" else t
        else:
            t = t.permute(1, 2, 0).contiguous().to(device) if layout == "cl" else t.contiguous().to(device)
        tens.append(t)
    images = torch.stack(tens) if spec["batch"] else tens[0] if len(tens) == 1 else tens
    kw = dict(size=spec["size"], crop=spec["crop"], antialias=spec["aa"], reverse_channels=spec["rev"], mean=spec["mean"],
              std=spec["std"], channels_last=spec["imgs"][0][3] == "cl" if len({i[3] for i in spec["imgs"]}) == 1 else None)
    return images, kw
