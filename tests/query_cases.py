"""Cases and the definition of the decoder query builder (pio_build_queries, csrc/pio_queries.hip).

Numpy only; shared by tests/test_queries_host.py (CPU: the definition against PerceiverIO.decoder_query's chain of torch
ops, the refusal table, eligibility) and tests/test_queries_gpu.py (MI355X: the kernel against the definition).

The definition restates the formulas of include/pio_hip.h by plain indexing -- not the torch functions, not the kernel:

    FOURIER  i = (points ? points[m] : start + m) mod prod(dims),  coord = row-major unravel of i,  p_j = axis[j][coord_j]
             phase(j, k) = fl32(fl32(p_j * bands[j, k]) * fl32(pi))
             x[0 : d] = p (concat_pos)   x[c0 + j K + k] = sin(phase)   x[c0 + d K + j K + k] = cos(phase) (not sine_only)
             x[width : Cq] = pad
    TABLE    x[0 : C] = table[m, :]   x[C : Cq] = pad
    y[row0 + m, c] = x[c]

Position, table and padding channels are moves: compared bit for bit.  Sine and cosine channels are compared against the
float64 sine / cosine of the fp32 phase within SINCOS_BOUND.

Every input lives inside a larger array that is NaN around it: axis tables have a NaN in front and behind, band tables
have row gaps (ldb > K) and NaN rows around them, learned tables have ldt > C, padding vectors NaN neighbours; the index
points sit inside a longer int64 array whose other entries are valid indices of OTHER grid points (a row built from one of
them differs visibly from the definition).  The output is NaN before the call.
"""
import numpy as np

PIO_OK, PIO_E_SHAPE, PIO_E_ALIGN, PIO_E_ARG = 0, -1, -2, -6
FOURIER, TABLE = 0, 1
STRIP = 32          # rows per workgroup strip in csrc/pio_queries.hip (QR_TS): cases cross it on purpose

# Largest |got - float64 sin / cos of the fp32 phase| allowed on a sine / cosine channel: TWICE the largest error of the
# torch chain itself (torch.sin / torch.cos of the same fp32 phases on an MI355X) over all cases below, as recorded in
# profiles/decoder_queries.json ("sincos_error": chain 6.432e-08, reached in big_phase; the kernel's sincosf measured the
# same 6.432e-08 -- about one ulp of a value near 1 plus the fp32 rounding of the result).  The factor covers sincosf against
# separate sinf / cosf calls.  A phase that was contracted, reassociated or rebuilt from the index errs by |phase| 2^-24: up to
# 3e-3 in big_phase, 5e-6 at 88 rad.
SINCOS_BOUND = 2 * 6.432e-08


def fourier(dims, K, res, points=None, start=0, M=None, concat_pos=True, sine_only=False, row0=None):
    pts = None if points is None else np.array(points, dtype=np.int64)
    return dict(kind=FOURIER, dims=tuple(dims), d=len(dims), K=K, res=tuple(res), points=pts, start=start,
                M=len(pts) if pts is not None else M, concat_pos=concat_pos, sine_only=sine_only, row0=row0,
                width=(len(dims) if concat_pos else 0) + len(dims) * K * (1 if sine_only else 2))


def table(M, C, row0=None):
    return dict(kind=TABLE, M=M, C=C, width=C, row0=row0)


def _case(Cq, segs, ldy=None, Qtot=None):
    """Segments are placed one after the other in the given order unless they carry their own row0."""
    r = 0
    for g in segs:
        if g["row0"] is None:
            g["row0"] = r
        r = g["row0"] + g["M"]
    return dict(Cq=Cq, ldy=ldy if ldy is not None else Cq, Qtot=Qtot if Qtot is not None else r, segs=segs)


def _mini(chunk):
    """The small multimodal golden's queries (MultiModalPerceiver(img_size=(16, 16), num_frames=2, num_classes=10,
    audio_samples_per_frame=32, audio_samples_per_patch=16), n_chunks = 2), chunk 0 or 1: audio | image | label."""
    return _case(1026, [fourier((4,), 192, (64,), points=np.arange(2 * chunk, 2 * chunk + 2)),
                        fourier((2, 16, 16), 32, (2, 4, 4), points=np.arange(256 * chunk, 256 * chunk + 256)),
                        table(1, 1024)])


_rng = np.random.default_rng(20261)
# name -> case; widths: Cq odd (11, 13), Cq % 4 == 2 (22, 386, 1026), Cq % 4 == 0 (8, 12, 16), each also with ldy > Cq
CASES = {
    # M = 1 three times, Cq odd; the table fills the row: a zero-width pad
    "one_row": _case(11, [fourier((5,), 2, (5,), points=[3]), fourier((2, 3), 1, (2, 3), points=[4]), table(1, 11)]),
    "mini_model_c0": _mini(0),
    "mini_model_c1": _mini(1),
    # 180 consecutive points from the middle of an image row: strips of 32 cross rows of 70, runs of equal y end mid-strip
    "seams": _case(22, [fourier((3, 70), 4, (3, 70), points=np.arange(20, 200))]),
    # permuted, repeated, >= total (15) and negative indices
    "wrap": _case(16, [fourier((3, 5), 3, (6, 10), points=np.concatenate([_rng.permutation(15), [7, 7, 7, 15, 29, 44, 1000, -1,
                                                                                                  -16, 14, 0]]))]),
    "sine_only": _case(12, [fourier((2, 3, 4), 2, (2, 3, 4), points=np.arange(24)[::-1], sine_only=True)], ldy=16),
    "no_pos": _case(13, [fourier((2, 3, 4), 2, (4, 6, 8), points=np.arange(3, 21), concat_pos=False)], ldy=15),
    # the audio query of the full model: the phase reaches 48 255 rad -- THE accuracy case
    "big_phase": _case(386, [fourier((1920,), 192, (30720,), points=np.concatenate([np.arange(64), np.arange(1856, 1920)]))],
                       ldy=388),
    # points = NULL: rows are start + m; Cq even on an odd pitch (dword stores)
    "start_only": _case(22, [fourier((3, 70), 4, (3, 70), start=37, M=50)], ldy=23),
    # segments given out of row order that leave rows 0, 1, 5, 6, 10, 11 alone; Cq % 4 == 0 on a pitch that is only even
    "holes": _case(8, [table(3, 4, row0=7), fourier((6,), 1, (6,), points=[5, 0, 3], row0=2)], ldy=10, Qtot=12),
}


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


def axis_table(n):
    """-1 + 2 i / n in fp32, operation by operation as BasicQuery._encode computes it: (2 i) exact, one rounded division,
    one rounded addition."""
    i2 = (2 * np.arange(n, dtype=np.int64)).astype(np.float32)
    return (np.float32(-1) + i2 / np.float32(n)).astype(np.float32)


def band_table(res, K):
    """K linearly spaced fp32 bands from 1 to res / 2 per axis (step = (end - start) / (K - 1); the first half counts up from
    the start, the second half down from the end).  torch.linspace rounds some of them differently: where a case stands for a
    module, the module's own bands are passed to gen()."""
    rows = []
    for r in res:
        start, end = np.float32(1.0), np.float32(r / 2)
        step = np.float32((end - start) / np.float32(K - 1)) if K > 1 else np.float32(0)
        idx = np.arange(K)
        up = (start + step * idx.astype(np.float32)).astype(np.float32)
        down = (end - step * (K - 1 - idx).astype(np.float32)).astype(np.float32)
        rows.append(np.where((idx < K // 2) | (K == 1), up, down).astype(np.float32))
    return np.stack(rows)


def _framed(a, gap):
    """a [R, C] inside a NaN array [R + 2, C + gap] at [1:, 1:]: (full, element offset of a[0, 0], row pitch)."""
    full = np.full((a.shape[0] + 2, a.shape[1] + gap), np.nan, dtype=np.float32)
    full[1:1 + a.shape[0], 1:1 + a.shape[1]] = a
    return full, full.shape[1] + 1, full.shape[1]


def gen(name, bands=None):
    """Inputs of a case, per segment a dict of  <what>_full (the enclosing array), <what>_off (element offset of the first
    addressed element in it) and <what> (the values themselves; None where the segment has none) for what in
      axis0 / axis1 / axis2 [dims[j]], bands [d, K] (+ ldb), points [M] int64, table [M, C] (+ ldt), pad [Cq - width]
    bands: optional {segment index: [d, K] float32} to use instead of band_table (a module's own torch.linspace values)."""
    c = CASES[name]
    rng = np.random.default_rng(_seed(name))
    out = []
    for i, g in enumerate(c["segs"]):
        d = {}
        for what in ("axis0", "axis1", "axis2", "bands", "points", "table", "pad"):
            d.update({what + "_full": None, what + "_off": 0, what: None})
        d.update(ldb=0, ldt=0)
        if g["kind"] == FOURIER:
            for j, n in enumerate(g["dims"]):
                ax = axis_table(n)
                full, off, _ = _framed(ax[None], 2)
                d.update({f"axis{j}_full": full, f"axis{j}_off": off, f"axis{j}": ax})
            b = np.asarray(bands[i], dtype=np.float32) if bands and i in bands else band_table(g["res"], g["K"])
            assert b.shape == (g["d"], g["K"])
            full, off, ldb = _framed(b, 3)
            d.update(bands_full=full, bands_off=off, ldb=ldb, bands=b)
            if g["points"] is not None:
                total = int(np.prod(g["dims"]))
                pts = g["points"]
                # surroundings: valid indices of grid points half the grid away from the neighbouring entry
                front = (pts[:3][::-1] + total // 2 + 1) % total
                pf = np.concatenate([front, pts, (pts[-3:] + total // 2 + 1) % total])
                d.update(points_full=pf.astype(np.int64), points_off=len(front), points=pts)
        else:
            t = (0.02 * rng.standard_normal((g["M"], g["C"]))).astype(np.float32)
            full, off, ldt = _framed(t, 3)
            d.update(table_full=full, table_off=off, ldt=ldt, table=t)
        if c["Cq"] > g["width"]:
            v = (0.02 * rng.standard_normal(c["Cq"] - g["width"])).astype(np.float32)
            full, off, _ = _framed(v[None], 2)
            d.update(pad_full=full, pad_off=off, pad=v)
        out.append(d)
    return out


def _at(d, what, i):
    return d[what + "_full"].reshape(-1)[d[what + "_off"] + i]


PI_F = np.float32(np.pi)
MOVE, SIN, COS = 0, 1, 2


def reference(name, data):
    """(y [Qtot, ldy] float32, exact [Qtot, ldy] float64, kind [Qtot, ldy] int8): the definition.  y and exact are NaN
    wherever the call must not write (ldy gaps, uncovered rows); kind is MOVE where y is the bit-exact expectation, SIN / COS
    where `exact` is the float64 sine / cosine of the fp32 phase (y holds it rounded to fp32)."""
    c = CASES[name]
    Cq = c["Cq"]
    y = np.full((c["Qtot"], c["ldy"]), np.nan, dtype=np.float32)
    exact = np.full((c["Qtot"], c["ldy"]), np.nan, dtype=np.float64)
    kind = np.zeros((c["Qtot"], c["ldy"]), dtype=np.int8)
    for g, d in zip(c["segs"], data):
        width = g["width"]
        for m in range(g["M"]):
            row = g["row0"] + m
            x = np.empty(Cq, dtype=np.float64)
            if g["kind"] == TABLE:
                for ch in range(g["C"]):
                    x[ch] = _at(d, "table", m * d["ldt"] + ch)
            else:
                nd, K = g["d"], g["K"]
                total = int(np.prod(g["dims"]))
                i = (int(_at(d, "points", m)) if g["points"] is not None else g["start"] + m) % total    # (Python's %: >= 0)
                coord = [0] * nd
                for j in reversed(range(nd)):
                    coord[j] = i % g["dims"][j]
                    i //= g["dims"][j]
                p = [np.float32(_at(d, f"axis{j}", coord[j])) for j in range(nd)]
                c0 = nd if g["concat_pos"] else 0
                for j in range(c0):
                    x[j] = p[j]
                for j in range(nd):
                    for k in range(K):
                        band = np.float32(_at(d, "bands", j * d["ldb"] + k))
                        phase = np.float64(np.float32(np.float32(p[j] * band) * PI_F))
                        ch = c0 + j * K + k
                        x[ch], kind[row, ch] = np.sin(phase), SIN
                        if not g["sine_only"]:
                            ch += nd * K
                            x[ch], kind[row, ch] = np.cos(phase), COS
            for ch in range(width, Cq):
                x[ch] = _at(d, "pad", ch - width)
            exact[row, :Cq] = x
            y[row, :Cq] = x.astype(np.float32)
    return y, exact, kind


def max_phase(name, data):
    """Largest |phase| of a case in rad (fp32 arithmetic as the definition's)."""
    worst = 0.0
    for g, d in zip(CASES[name]["segs"], data):
        if g["kind"] == FOURIER:
            for j in range(g["d"]):
                p = np.abs(d[f"axis{j}"]).max()
                worst = max(worst, float(np.float32(np.float32(p * np.abs(d["bands"][j]).max()) * PI_F)))
    return worst


def covered(name):
    """bool [Qtot, ldy]: the elements the call writes."""
    c = CASES[name]
    w = np.zeros((c["Qtot"], c["ldy"]), dtype=bool)
    for g in c["segs"]:
        w[g["row0"]:g["row0"] + g["M"], :c["Cq"]] = True
    return w


def compare(got, ref, what, bound=None):
    """got [Qtot, ldy] float32 against reference(): NaN (untouched) outside the covered elements, moves bit for bit, sine and
    cosine within `bound` (default SINCOS_BOUND) of the float64 value.  Returns the largest sine / cosine error."""
    y, exact, kind = ref
    got = np.ascontiguousarray(got, dtype=np.float32)
    assert got.shape == y.shape, (what, got.shape, y.shape)
    cov = ~np.isnan(exact)
    assert np.isnan(got[~cov]).all(), f"{what}: an ldy gap or a row no segment covers was written"
    assert np.isfinite(got[cov]).all(), f"{what}: non-finite outputs (a read outside an input?)"
    move = cov & (kind == MOVE)
    same = got.view(np.int32) == y.view(np.int32)
    if not same[move].all():
        i = tuple(int(v[0]) for v in np.nonzero(move & ~same))
        raise AssertionError(f"{what}: {int((move & ~same).sum())} moved elements differ, first at {i}: got {got[i]!r} "
                             f"ref {y[i]!r}")
    trig = cov & (kind != MOVE)
    if not trig.any():
        return 0.0
    err = np.abs(got.astype(np.float64) - exact)
    err[~trig] = 0.0
    worst = float(err.max())
    print(f"{what}: max sine / cosine error {worst:.3e}")
    i = np.unravel_index(int(err.argmax()), err.shape)
    assert worst <= (SINCOS_BOUND if bound is None else bound), \
        f"{what}: sine / cosine error {worst:.3e} at {tuple(int(v) for v in i)}: got {got[i]!r}, exact {exact[i]!r}"
    return worst


def call_fields(name, data, addr):
    """The call of a case as plain values: (list of per-segment field dicts of pio_query_segment_t, keyword arguments).
    addr(segment index, what) -> byte address of the enclosing array `what`."""
    c = CASES[name]
    segs = []
    for i, (g, d) in enumerate(zip(c["segs"], data)):
        def ptr(what, size=4):
            return None if d[what] is None else addr(i, what) + size * d[what + "_off"]
        f = dict(kind=g["kind"], row0=g["row0"], M=g["M"], ldb=d["ldb"], ldt=d["ldt"], pad=ptr("pad"))
        if g["kind"] == FOURIER:
            f.update(d=g["d"], dims=list(g["dims"]), K=g["K"], concat_pos=int(g["concat_pos"]), sine_only=int(g["sine_only"]),
                     start=g["start"], axis=[ptr(f"axis{j}") for j in range(g["d"])], bands=ptr("bands"),
                     points=ptr("points", 8))
        else:
            f.update(C=g["C"], table=ptr("table"))
        segs.append(f)
    return segs, dict(ldy=c["ldy"], Qtot=c["Qtot"], Cq=c["Cq"])


# ----------------------------------------------------------------------------------------------------
# refusals: (name, changes to a valid call, expected code).  The valid call: Cq = 8, ldy = 8, Qtot = 5; segment 0 FOURIER
# rows [0, 3): d = 2, dims (3, 4), K = 1, positions -> 2 | 2 sines | 2 cosines | 2 pad, with points; segment 1 TABLE rows
# [3, 5): C = 8, ldt = 8, no pad.  A change is keyed by an argument name, by (segment, field) or by (segment, "axis" /
# "dims", j); "ptr+<b>": that pointer moved by b bytes; "ptr": a valid pointer where the valid call has none; None: NULL.
# (A grid beyond 32 bits cannot be reached: 4 segments of at most 2^31 - 1 rows are 2^28 strips.)
# ----------------------------------------------------------------------------------------------------
VALID_ARGS = dict(nseg=2, ldy=8, Qtot=5, Cq=8)
VALID_SEGS = [
    dict(kind=FOURIER, row0=0, M=3, d=2, dims=[3, 4, 0], K=1, concat_pos=1, sine_only=0, start=0, ldb=1, ldt=0, C=0),
    dict(kind=TABLE, row0=3, M=2, d=0, dims=[0, 0, 0], K=0, concat_pos=0, sine_only=0, start=0, ldb=0, ldt=8, C=8),
]
VALID_PTRS = [("axis0", "axis1", "bands", "points", "pad"), ("table",)]       # the pointers each segment carries
REFUSALS = [
    ("y NULL", {"y": None}, PIO_E_ARG),
    ("nseg=0", {"nseg": 0}, PIO_E_ARG),
    ("nseg=5", {"nseg": 5}, PIO_E_ARG),
    ("kind=2", {(0, "kind"): 2}, PIO_E_ARG),
    ("d=0", {(0, "d"): 0}, PIO_E_ARG),
    ("d=4", {(0, "d"): 4}, PIO_E_ARG),
    ("K=0", {(0, "K"): 0}, PIO_E_ARG),
    ("axis[0] NULL", {(0, "axis0"): None}, PIO_E_ARG),
    ("axis[1] NULL", {(0, "axis1"): None}, PIO_E_ARG),
    ("axis[2] NULL, d=3", {(0, "d"): 3, (0, "dims", 2): 1, "Cq": 9, "ldy": 9, (1, "C"): 9, (1, "ldt"): 9}, PIO_E_ARG),
    ("bands NULL", {(0, "bands"): None}, PIO_E_ARG),
    ("table NULL, C > 0", {(1, "table"): None}, PIO_E_ARG),
    ("FOURIER pad NULL, width < Cq", {(0, "pad"): None}, PIO_E_ARG),
    ("TABLE pad NULL, C < Cq", {(1, "C"): 7}, PIO_E_ARG),
    ("Qtot=0", {"Qtot": 0}, PIO_E_SHAPE),
    ("Cq=0", {"Cq": 0}, PIO_E_SHAPE),
    ("ldy<Cq", {"ldy": 7}, PIO_E_SHAPE),
    ("M=0", {(0, "M"): 0}, PIO_E_SHAPE),
    ("M=-1", {(1, "M"): -1}, PIO_E_SHAPE),
    ("dims[1]=0", {(0, "dims", 1): 0}, PIO_E_SHAPE),
    ("prod(dims) >= 2^31", {(0, "dims", 0): 1 << 16, (0, "dims", 1): 1 << 15}, PIO_E_SHAPE),
    ("ldb<K", {(0, "ldb"): 0}, PIO_E_SHAPE),
    ("width>Cq", {(0, "K"): 2, (0, "ldb"): 2}, PIO_E_SHAPE),
    ("width>Cq, sine_only", {(0, "K"): 4, (0, "ldb"): 4, (0, "sine_only"): 1}, PIO_E_SHAPE),
    ("C<0", {(1, "C"): -1}, PIO_E_SHAPE),
    ("C>Cq", {(1, "C"): 9, (1, "ldt"): 9}, PIO_E_SHAPE),
    ("ldt<C", {(1, "ldt"): 7}, PIO_E_SHAPE),
    ("feature rows beyond the LDS", {(0, "K"): 124, (0, "ldb"): 124, "Cq": 1024, "ldy": 1024, (1, "pad"): "ptr"}, PIO_E_SHAPE),
    ("row0<0", {(0, "row0"): -1}, PIO_E_SHAPE),
    ("segment past Qtot", {(1, "row0"): 4}, PIO_E_SHAPE),
    ("segments overlap", {(1, "row0"): 2}, PIO_E_SHAPE),
    ("y misaligned", {"y": "ptr+2"}, PIO_E_ALIGN),
    ("axis misaligned", {(0, "axis1"): "ptr+2"}, PIO_E_ALIGN),
    ("bands misaligned", {(0, "bands"): "ptr+1"}, PIO_E_ALIGN),
    ("points 4-byte aligned", {(0, "points"): "ptr+4"}, PIO_E_ALIGN),
    ("table misaligned", {(1, "table"): "ptr+2"}, PIO_E_ALIGN),
    ("pad misaligned", {(0, "pad"): "ptr+3"}, PIO_E_ALIGN),
]
# changes that stay VALID (the call runs): the fall-backs of the vector paths are not refusals
ACCEPTED = [
    ("the valid call", {}),
    ("y 8-byte aligned", {"y": "ptr+8"}),
    ("y 4-byte aligned", {"y": "ptr+4"}),
    ("ldy=10", {"ldy": 10}),
    ("ldy=9", {"ldy": 9}),
    ("the largest feature rows", {(0, "K"): 123, (0, "ldb"): 123, "Cq": 1024, "ldy": 1024, (1, "pad"): "ptr"}),
]
POINTER_FIELDS = ("axis0", "axis1", "axis2", "bands", "points", "table", "pad")


def refusal_fields(ptrs, changes):
    """The valid call with `changes` applied: (segment field dicts, keyword arguments, y address).  ptrs: "y" -> address,
    (segment, field) -> address for every pointer field of both segments (those VALID_PTRS does not list start as NULL)."""
    args = dict(VALID_ARGS)
    segs = [dict(g, dims=list(g["dims"])) for g in VALID_SEGS]
    for i, fields in enumerate(VALID_PTRS):
        for f in POINTER_FIELDS:
            segs[i][f] = ptrs[(i, f)] if f in fields else None
    y = ptrs["y"]
    for k, v in changes.items():
        if k == "y":
            y = None if v is None else y + int(v[4:])
        elif isinstance(k, tuple) and k[1] == "dims":
            segs[k[0]]["dims"][k[2]] = v
        elif isinstance(k, tuple) and k[1] in POINTER_FIELDS:
            base = ptrs[(k[0], k[1])]
            segs[k[0]][k[1]] = None if v is None else base if v == "ptr" else base + int(v[4:])
        elif isinstance(k, tuple):
            segs[k[0]][k[1]] = v
        else:
            args[k] = v
    for g in segs:
        g["axis"] = [g.pop("axis0"), g.pop("axis1"), g.pop("axis2")]
    return segs, args, y
