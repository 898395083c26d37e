"""Cases and the float64 definition of the flow front end (pio_flow_patch_tokens, csrc/pio_flowprep.hip).

Numpy only; shared by tests/test_flow_front_host.py (CPU: the definition against patches_for_flow -> space_to_depth ->
Linear in float64, and the refusal table) and tests/test_flow_front_gpu.py (MI355X: the kernel against the definition).

The definition restates the formula of include/pio_hip.h, not the torch functions and not the kernel:

    y[n, r W + x, o] = bias[o] + sum_{t<2} sum_{py,px<3} sum_{c<C} w[o, t 9C + (py 3 + px) C + c]
                                                                   * frame_t[n, c, r + py - 1, x + px - 1]    (0 outside)

Every frame lives inside a larger image that is NaN outside the addressed region (`full` / `origin` per frame): a kernel
that reads one cell outside [0, H) x [0, W) -- even to multiply it by zero -- makes its output non-finite.
"""
import numpy as np

PIO_OK, PIO_E_SHAPE, PIO_E_ALIGN, PIO_E_ARG = 0, -1, -2, -6
BORDER = 2          # NaN rows / columns around a frame that has no `full` image of its own


def _case(N, C, H, W, out, raw=False, ldy=None, full0=None, origin0=None, full1=None, origin1=None):
    full0 = full0 or (H + 2 * BORDER, W + 2 * BORDER)
    full1 = full1 or (H + 2 * BORDER, W + 2 * BORDER)
    return dict(N=N, C=C, H=H, W=W, out=out, raw=raw, ldy=ldy if ldy is not None else (out + 3) // 4 * 4,
                full=(full0, full1), origin=(origin0 or (BORDER, BORDER), origin1 or (BORDER, BORDER)))


# name -> case; what each one probes: the table of the kernel's issue
CASES = {
    "one_pixel": _case(1, 3, 1, 1, 64),               # every neighbour is padding
    "thin_row": _case(2, 3, 1, 70, 64),               # one-row image crossing a column-tile seam (64)
    "thin_col": _case(2, 3, 70, 1, 64),               # one-column image crossing many row-tile seams (4)
    "odd": _case(2, 3, 17, 70, 64),                   # no multiple of the 4 x 64 tile in either axis, N > 1
    "train": _case(1, 3, 48, 64, 64),                 # the small flow golden's size: exact tiles
    "c1_out4": _case(1, 1, 9, 33, 4),                 # the ends of the supported range
    "c4_out128": _case(1, 4, 9, 33, 128),
    "raw": _case(2, 3, 17, 70, 54, raw=True),         # w == NULL: the 18 C patch channels, ldy = 56
    # a 17 x 70 crop of a 40 x 100 image (frame 1: of a 44 x 104 image at another place): row / plane / sample strides
    # that differ between the two frames, and an output pitch wider than the row
    "strided": _case(2, 3, 17, 70, 64, ldy=72, full0=(40, 100), origin0=(11, 13), full1=(44, 104), origin1=(5, 29)),
}


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


def gen(name):
    """Inputs of a case: `full` -- the two enclosing images [N, C, Hf, Wf] float32, N(0, 1) inside the addressed region and
    NaN outside; `frames` -- the two regions themselves [N, C, H, W] (copies); `w` [out, 18 C] LeCun-normal (variance
    1 / fan_in, truncated at two standard deviations, as the module initialises it) and `bias` [out] (None for raw)."""
    c = CASES[name]
    rng = np.random.default_rng(_seed(name))
    N, C, H, W, out = c["N"], c["C"], c["H"], c["W"], c["out"]
    full, frames = [], []
    for t in range(2):
        hf, wf = c["full"][t]
        oy, ox = c["origin"][t]
        img = np.full((N, C, hf, wf), np.nan, dtype=np.float32)
        fr = rng.standard_normal((N, C, H, W)).astype(np.float32)
        img[:, :, oy:oy + H, ox:ox + W] = fr
        full.append(img)
        frames.append(fr)
    d = dict(full=full, frames=frames, w=None, bias=None)
    if not c["raw"]:
        K = 18 * C
        g = np.clip(rng.standard_normal((out, K)), -2.0, 2.0) / 0.87962566103423978     # unit variance after truncation
        d["w"] = (g / np.sqrt(K)).astype(np.float32)
        d["bias"] = (0.1 * rng.standard_normal(out)).astype(np.float32)
    return d


def patches(frames):
    """[N, H, W, 18 C] float64: the zero-padded 3x3 neighbourhoods of both frames in the channel order of the formula."""
    f0 = np.asarray(frames[0], dtype=np.float64)
    N, C, H, W = f0.shape
    p = np.zeros((N, H, W, 18 * C))
    for t in range(2):
        padded = np.zeros((N, C, H + 2, W + 2))
        padded[:, :, 1:H + 1, 1:W + 1] = np.asarray(frames[t], dtype=np.float64)
        for py in range(3):
            for px in range(3):
                for ch in range(C):
                    p[..., t * 9 * C + (py * 3 + px) * C + ch] = padded[:, ch, py:py + H, px:px + W]
    return p


def reference(d):
    """(y, mag) float64 [N, H W, out]: the definition and sum_k |w_k x_k| + |b| (the scale of the error bound).  Raw
    (w is None): y = the patches, mag = 0 -- the kernel only moves values."""
    p = patches(d["frames"])
    N, H, W, K = p.shape
    p = p.reshape(N, H * W, K)
    if d["w"] is None:
        return p, np.zeros_like(p)
    w, b = d["w"].astype(np.float64), d["bias"].astype(np.float64)
    return p @ w.T + b, np.abs(p) @ np.abs(w).T + np.abs(b)


def bound(C, mag):
    """|y - ref| <= (K + 1) 2^-24 (sum_k |w_k x_k| + |b|), K = 18 C: K fp32 FMAs, each one rounding of relative size
    2^-24, in ANY summation order (gamma_K = K u / (1 - K u) <= (K + 1) u for K^2 u <= 1)."""
    return (18 * C + 1) * 2.0 ** -24 * mag


# ----------------------------------------------------------------------------------------------------
# refusals: (name, changes to a valid call, expected code).  The valid call: C = 3, H x W = 5 x 6, N = 1, out = 64,
# ldy = 64, every pointer present and aligned.  "ptr+<b>": that pointer moved by b bytes; None: a NULL pointer.
# ----------------------------------------------------------------------------------------------------
VALID = dict(N=1, C=3, H=5, W=6, out=64, ldy=64)
REFUSALS = [
    ("C=5", dict(C=5), PIO_E_SHAPE),
    ("C=0", dict(C=0), PIO_E_SHAPE),
    ("out=6", dict(out=6, ldy=8), PIO_E_SHAPE),
    ("out=132", dict(out=132, ldy=132), PIO_E_SHAPE),
    ("out=0", dict(out=0), PIO_E_SHAPE),
    ("N=0", dict(N=0), PIO_E_SHAPE),
    ("H=0", dict(H=0), PIO_E_SHAPE),
    ("W=-1", dict(W=-1), PIO_E_SHAPE),
    ("N=65536", dict(N=65536), PIO_E_SHAPE),
    ("ldy<out", dict(ldy=60), PIO_E_SHAPE),
    ("raw, out != 18 C", dict(w=None, bias=None), PIO_E_SHAPE),
    ("ldy=out+2", dict(ldy=66), PIO_E_ALIGN),
    ("y misaligned", dict(y="ptr+4"), PIO_E_ALIGN),
    ("frame0 misaligned", dict(frame0="ptr+2"), PIO_E_ALIGN),
    ("frame1 misaligned", dict(frame1="ptr+1"), PIO_E_ALIGN),
    ("w misaligned", dict(w="ptr+2"), PIO_E_ALIGN),
    ("frame0 NULL", dict(frame0=None), PIO_E_ARG),
    ("frame1 NULL", dict(frame1=None), PIO_E_ARG),
    ("y NULL", dict(y=None), PIO_E_ARG),
    ("w without bias", dict(bias=None), PIO_E_ARG),
]


def refusal_call(lib, ptrs, changes, stream=None):
    """The valid call with `changes` applied; ptrs: name -> address for frame0, frame1, w, bias, y."""
    a = dict(VALID)
    p = dict(ptrs)
    for k, v in changes.items():
        if k in p:
            p[k] = None if v is None else p[k] + int(v[4:])
        else:
            a[k] = v
    H, W, C = max(a["H"], 1), max(a["W"], 1), max(a["C"], 1)
    return lib.pio_flow_patch_tokens(p["frame0"], p["frame1"], C * H * W, H * W, W, C * H * W, H * W, W, p["w"], p["bias"],
                                     p["y"], a["ldy"], a["N"], a["C"], a["H"], a["W"], a["out"], stream)
