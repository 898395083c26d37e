"""Cases, refusals and the fp32 numpy definition of pio_flow_blend_tiles (include/pio_hip.h), shared by
tests/test_flow_blend_host.py and tests/test_flow_blend_gpu.py.

The definition is the vectorised restatement of the tile blend of FlowPerceiver.forward(test_mode=True): a zero accumulator,
and for each tile in order acc[region] = acc[region] + flow * ramp, wsum[region] += ramp, then one divide -- every operation
a separately rounded fp32 one.  A tile that hangs over the lower or right edge of the image is cut at the edge, as the
chain's negative padding cuts it (compute_grid_indices makes such tiles whenever an inner corner lies behind h - H: the
cases `odd`, `dup`, `column` and `wide` have them).

`wide` runs with overlap 3: the 20 of the case list is not below its tile height of 4, and compute_grid_indices raises for
such an overlap; 3 is the largest it takes.  Everything else of that case is as listed (rows of 700 pixels over 300-pixel
tiles: wider than a workgroup's span, no multiple of 64)."""
import itertools
import zlib

import numpy as np

PIO_OK, PIO_E_SHAPE, PIO_E_ALIGN, PIO_E_ARG = 0, -1, -2, -6
MAX_AXIS = MAX_GROUPS = 64
SPAN = 256                                  # pixels of an image row per workgroup (csrc/pio_flowblend.hip FB_SPAN)

# layout "perm": the permuted view of [B, H, W, 2] that FlowPostprocessor returns (sc = 1, sx = 2); "contig": [B, 2, H, W].
# pad: extra rows / columns of NaN inside every sample of the allocation (0: the dense, shipped strides).
CASES = {
    "single": dict(H=6, W=8, h=6, w=8, overlap=1, N=1, tpg=1, layout="contig", pad=1, ys=[0], xs=[0]),
    "odd": dict(H=5, W=7, h=9, w=16, overlap=2, N=2, tpg=2, layout="perm", pad=1, ys=[0, 3, 4], xs=[0, 5, 10, 9]),
    "dup": dict(H=5, W=6, h=11, w=19, overlap=3, N=1, tpg=4, layout="contig", pad=1, ys=[0, 2, 4, 6, 8, 6],
                xs=[0, 3, 6, 9, 12, 15, 13]),
    "column": dict(H=6, W=8, h=13, w=8, overlap=3, N=1, tpg=1, layout="perm", pad=1, ys=[0, 3, 6, 9, 7], xs=[0]),
    "wide": dict(H=4, W=300, h=7, w=700, overlap=3, N=1, tpg=3, layout="perm", pad=1, ys=[0, 1, 2, 3, 4, 5, 3],
                 xs=[0, 297, 400]),
    "small_golden": dict(H=48, W=64, h=60, w=80, overlap=10, N=1, tpg=4, layout="perm", pad=0, ys=[0, 12], xs=[0, 16]),
    "sintel": dict(H=368, W=496, h=436, w=1024, overlap=20, N=1, tpg=4, layout="perm", pad=0, ys=[0, 68],
                   xs=[0, 476, 528]),
}
HOST_CASES = sorted(n for n in CASES if n != "sintel")


def axes(c):
    """(ys, xs) by the arithmetic of FlowPerceiver.compute_grid_indices, written out once more."""
    out = []
    for tile, size in ((c["H"], c["h"]), (c["W"], c["w"])):
        a = list(range(0, size, tile - c["overlap"]))
        a[-1] = size - tile
        out.append([0] if size == tile else a)
    return out


def group_sizes(c):
    tiles = len(c["ys"]) * len(c["xs"])
    return [min(c["tpg"], tiles - i) for i in range(0, tiles, c["tpg"])]


def strides(c):
    """Element strides (sn, sc, sy, sx) of every group's [tiles * N, 2, H, W] view, and the shape of one sample of its
    allocation."""
    Hp, Wp = c["H"] + c["pad"], c["W"] + 3 * c["pad"]
    if c["layout"] == "perm":
        return (Hp * Wp * 2, 1, Wp * 2, 2), (Hp, Wp, 2)
    return (2 * Hp * Wp, Hp * Wp, Wp, 1), (2, Hp, Wp)


def out_layout(c):
    """(first element, on, oc, oy, elements) of the output inside its NaN-filled allocation: oy > w, gaps behind every
    plane and sample, a first element that is 4- but not 8-byte aligned."""
    oy = c["w"] + 3
    oc = c["h"] * oy + 5
    on = 2 * oc + 7
    off = 1
    return off, on, oc, oy, off + c["N"] * on + 4


def gen(name):
    """The case's inputs: per group a NaN-filled allocation `full[i]` ([tiles * N + 2 samples]: one guard sample in front,
    one behind, NaN pad rows / columns inside) whose view begins `first` elements in, and `flows[i]`, that view as a dense
    [tiles * N, 2, H, W] array.  Random normal values, about 10 % exact zeros, half of them negative."""
    c = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    (sn, sc, sy, sx), sample = strides(c)
    full, flows = [], []
    for g in group_sizes(c):
        rows = g * c["N"]
        v = rng.standard_normal((rows, 2, c["H"], c["W"])).astype(np.float32)
        u = rng.random(v.shape)
        v[u < 0.05] = 0.0
        v[(u >= 0.05) & (u < 0.10)] = -0.0
        a = np.full((rows + 2,) + sample, np.nan, dtype=np.float32)
        if c["layout"] == "perm":
            a[1:-1, :c["H"], :c["W"], :] = v.transpose(0, 2, 3, 1)
        else:
            a[1:-1, :, :c["H"], :c["W"]] = v
        full.append(a)
        flows.append(v)
    return {"full": full, "flows": flows, "first": sn, "strides": (sn, sc, sy, sx)}


def tile_flow(c, data, k):
    """[N, 2, H, W]: the flow of tile k."""
    g, j = divmod(k, c["tpg"])
    return data["flows"][g][j * c["N"]:(j + 1) * c["N"]]


def reference(name, data, xs=None):
    """The definition on the case's tiles ([N, 2, h, w] fp32), with the case's xs or the given list."""
    c = CASES[name]
    H, W, h, w = c["H"], c["W"], c["h"], c["w"]
    xs = c["xs"] if xs is None else xs
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ramp = np.minimum(np.minimum(xx + 1, W - xx), np.minimum(yy + 1, H - yy))
    assert int(ramp.max()) == min((W + 1) // 2, (H + 1) // 2)
    ramp = ramp.astype(np.float32) / np.float32(ramp.max())
    acc = np.zeros((c["N"], 2, h, w), dtype=np.float32)
    wsum = np.zeros((h, w), dtype=np.float32)
    for k, (y, x) in enumerate(itertools.product(c["ys"], xs)):
        hh, ww = min(H, h - y), min(W, w - x)
        r = ramp[:hh, :ww]
        acc[:, :, y:y + hh, x:x + ww] = acc[:, :, y:y + hh, x:x + ww] + tile_flow(c, data, k)[:, :, :hh, :ww] * r
        wsum[y:y + hh, x:x + ww] += r
    assert (wsum > 0).all()
    out = acc / wsum
    assert out.dtype == np.float32
    return out


def expected_full(name, ref):
    """The whole output allocation after the call: the definition where out lives, NaN everywhere else."""
    c = CASES[name]
    off, on, oc, oy, total = out_layout(c)
    full = np.full(total, np.nan, dtype=np.float32)
    for n in range(c["N"]):
        for ch in range(2):
            for y in range(c["h"]):
                o = off + n * on + ch * oc + y * oy
                full[o:o + c["w"]] = ref[n, ch, y]
    return full


def fill_struct(L, f):
    """The ctypes pio_flow_blend_t of a field dict (keys of base_fields)."""
    p = L.FlowBlend()
    for i, a in enumerate(f["group"][:MAX_GROUPS]):
        p.group[i] = a
    for k in ("sn", "sc", "sy", "sx", "ngroups", "tiles_per_group", "ny", "nx", "N", "H", "W", "h", "w"):
        setattr(p, k, f[k])
    p.ys[:len(f["ys"])] = f["ys"]
    p.xs[:len(f["xs"])] = f["xs"]
    return p


def blend(L, f, stream=None):
    """pio_flow_blend_tiles on a field dict; f["p"] is None passes a NULL struct."""
    p = None if f.get("p", True) is None else fill_struct(L, f)
    return L.lib().pio_flow_blend_tiles(p, f["out"], f["on"], f["oc"], f["oy"], stream)


def case_fields(name, data, group_ptrs, out_ptr, xs=None):
    c = CASES[name]
    sn, sc, sy, sx = data["strides"]
    off, on, oc, oy, _ = out_layout(c)
    xs = c["xs"] if xs is None else xs
    return dict(group=[a + 4 * data["first"] for a in group_ptrs], sn=sn, sc=sc, sy=sy, sx=sx, ngroups=len(group_ptrs),
                tiles_per_group=c["tpg"], ny=len(c["ys"]), nx=len(xs), ys=c["ys"], xs=xs, N=c["N"], H=c["H"], W=c["W"],
                h=c["h"], w=c["w"], out=out_ptr + 4 * off, on=on, oc=oc, oy=oy)


# ---- refusals: one valid call (4 x 6 tiles at ys x xs = [0, 2] x [0, 3] of a 6 x 9 image, two groups of two tiles, dense
# [B, 2, H, W] flows) and what each row changes in it
R_H, R_W, R_h, R_w = 4, 6, 6, 9
R_GROUP_ELEMS = 2 * 2 * R_H * R_W
R_OUT_ELEMS = 2 * R_h * R_w


def base_fields(ptrs):
    return dict(group=[ptrs["g0"], ptrs["g1"]], sn=2 * R_H * R_W, sc=R_H * R_W, sy=R_W, sx=1, ngroups=2, tiles_per_group=2,
                ny=2, nx=2, ys=[0, 2], xs=[0, 3], N=1, H=R_H, W=R_W, h=R_h, w=R_w, out=ptrs["out"], on=2 * R_h * R_w,
                oc=R_h * R_w, oy=R_w)


def refusal_fields(ptrs, changes):
    f = base_fields(ptrs)
    for k, v in changes.items():
        if k == "group1":
            f["group"] = [f["group"][0], v(ptrs) if callable(v) else v]
        elif k == "group0":
            f["group"] = [v(ptrs) if callable(v) else v, f["group"][1]]
        else:
            f[k] = v(ptrs) if callable(v) else v
    if f["ngroups"] > len(f["group"]):
        f["group"] = (f["group"] * MAX_GROUPS)[:MAX_GROUPS]
    return f


REFUSALS = [
    ("null_p", {"p": None}, PIO_E_ARG),
    ("null_out", {"out": None}, PIO_E_ARG),
    ("null_group1", {"group1": None}, PIO_E_ARG),
    ("N_0", {"N": 0}, PIO_E_SHAPE),
    ("H_0", {"H": 0}, PIO_E_SHAPE),
    ("W_0", {"W": 0}, PIO_E_SHAPE),
    ("h_below_H", {"h": R_H - 1}, PIO_E_SHAPE),
    ("w_below_W", {"w": R_W - 1}, PIO_E_SHAPE),
    ("ny_0", {"ny": 0}, PIO_E_SHAPE),
    ("ny_65", {"ny": 65}, PIO_E_SHAPE),
    ("nx_0", {"nx": 0}, PIO_E_SHAPE),
    ("nx_65", {"nx": 65}, PIO_E_SHAPE),
    ("ngroups_0", {"ngroups": 0}, PIO_E_SHAPE),
    ("ngroups_65", {"ngroups": 65, "tiles_per_group": 1}, PIO_E_SHAPE),
    ("tiles_per_group_0", {"tiles_per_group": 0}, PIO_E_SHAPE),
    ("ngroups_too_few", {"tiles_per_group": 1}, PIO_E_SHAPE),
    ("ngroups_too_many", {"tiles_per_group": 4}, PIO_E_SHAPE),
    ("y_corner_negative", {"ys": [-1, 2]}, PIO_E_SHAPE),
    ("y_corner_behind_image", {"ys": [0, R_h]}, PIO_E_SHAPE),
    ("x_corner_negative", {"xs": [-1, 3]}, PIO_E_SHAPE),
    ("x_corner_behind_image", {"xs": [0, R_w]}, PIO_E_SHAPE),
    ("last_rows_uncovered", {"ys": [0, 0]}, PIO_E_SHAPE),
    ("first_row_uncovered", {"ys": [1, 2]}, PIO_E_SHAPE),
    ("last_columns_uncovered", {"xs": [0, 2]}, PIO_E_SHAPE),
    ("middle_column_uncovered", {"w": 14, "oy": 14, "xs": [0, 8]}, PIO_E_SHAPE),
    ("oy_below_w", {"oy": R_w - 1}, PIO_E_SHAPE),
    ("grid_beyond_31_bits", {"N": 2 ** 30}, PIO_E_SHAPE),
    ("out_misaligned", {"out": lambda p: p["out"] + 2}, PIO_E_ALIGN),
    ("group0_misaligned", {"group0": lambda p: p["g0"] + 1}, PIO_E_ALIGN),
    ("group1_misaligned", {"group1": lambda p: p["g1"] + 3}, PIO_E_ALIGN),
]
