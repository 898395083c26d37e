"""Cases and the definition of the multimodal front end (pio_assemble_tokens, csrc/pio_tokens.hip).

Numpy only; shared by tests/test_mm_front_host.py (CPU: the definition against MultimodalPreprocessor's chain of copies,
the refusal table, eligibility) and tests/test_mm_front_gpu.py (MI355X: the kernel against the definition, bit for bit).

The definition restates the formulas of include/pio_hip.h by plain indexing -- not the torch functions, not the kernel:

    x[0 : C1] = feature(b, m, :)    x[C1 : C1 + C2] = table[m, :]    x[C1 + C2 : Cc] = pad[:]
    y[b, row0 + m, c] = x[c]                       unmasked
                      = token[c] + 0.0f * x[c]     masked
    ROWS: feature(b, m, j) = f[b sb + m sm + j]
    S2D:  m = (t H/s + y) W/s + x,  j = (dy s + dx) C + c,  feature = frame[b, t, c, y s + dy, x s + dx]

Every input lives inside a larger array that is NaN around it: frames are crops (in t, c, y and x) of NaN videos, ROWS
features have NaN gaps between rows (sm > C1) and NaN rows around them, tables have ldt > C2 with NaN gaps, padding and
token vectors have NaN neighbours.  A kernel that reads one element outside what the formulas address makes an unmasked
output non-finite.
"""
import numpy as np

PIO_OK, PIO_E_SHAPE, PIO_E_ALIGN, PIO_E_ARG = 0, -1, -2, -6
ROWS, S2D = 0, 1
STRIP = 32          # tokens per workgroup strip in csrc/pio_tokens.hip (TK_TS): cases cross it on purpose


def rows(M, C1, C2, sm=None, masked=False, row0=None):
    return dict(kind=ROWS, M=M, C1=C1, C2=C2, sm=sm if sm is not None else C1 + 3, masked=masked, row0=row0)


def s2d(T, C, H, W, s, C2, masked=False, row0=None, four_d=False):
    return dict(kind=S2D, T=T, C=C, H=H, W=W, s=s, M=T * (H // s) * (W // s), C1=s * s * C, C2=C2, masked=masked,
                row0=row0, four_d=four_d)


def _case(B, Cc, segs, ldy=None, Mtot=None):
    """Segments are placed one after the other in the given order unless they carry their own row0."""
    r = 0
    for g in segs:
        if g["row0"] is None:
            g["row0"] = r
        r = g["row0"] + g["M"]
    return dict(B=B, Cc=Cc, ldy=ldy if ldy is not None else Cc, Mtot=Mtot if Mtot is not None else r, segs=segs)


# name -> case; what each one probes: the table of the kernel's issue
CASES = {
    "one_token": _case(2, 11, [rows(1, 3, 2), s2d(1, 1, 1, 1, 1, C2=4), rows(1, 11, 0)]),      # M = 1 three times, Cc odd
    "s2d_small": _case(2, 60, [s2d(2, 3, 8, 8, 4, C2=7)]),                  # 8 tokens, 48 | 7 | 5: the vector path
    "s2d_seams": _case(2, 8, [s2d(1, 3, 3, 70, 1, C2=2)]),                  # pixels form: 210 tokens, strips of 32 cross rows of 70
    "s2d_c1_s2": _case(2, 9, [s2d(1, 1, 6, 10, 2, C2=3, four_d=True)]),     # 4-D image, C = 1, s = 2, cropped in every axis
    "s2d_c4_s8": _case(1, 260, [s2d(1, 4, 8, 16, 8, C2=1)]),                # the upper ends: C = 4, s = 8, C1 = 256
    "rows_strided": _case(2, 28, [rows(37, 16, 9, sm=24)]),                 # sm = 24, sb != M sm, 37 rows: two strips
    "no_pos_no_pad": _case(2, 12, [rows(5, 12, 0), rows(3, 8, 4)]),         # C2 = 0 and Cp = 0 in one segment, Cp = 0 in the other
    "masked": _case(2, 27, [rows(4, 16, 9), rows(1, 10, 0, masked=True)]),  # the label's form; inf / NaN planted in its x
    "masked_vec": _case(2, 28, [rows(3, 10, 2, masked=True), s2d(1, 2, 2, 4, 2, C2=5, masked=True)]),   # both kinds, 16-byte rows
    "dword_path": _case(2, 405, [rows(3, 16, 385)]),                        # Cc = 405, ldy = 405
    "dword_path_ld412": _case(2, 405, [rows(3, 16, 385)], ldy=412),         # ... and ldy = 412
    # audio | image | label with the small golden's widths (MultiModalPerceiver(img_size=(16, 16), num_frames=2,
    # num_classes=10, audio_samples_per_frame=32)): 16 | 385 | 4,  48 | 195 | 162,  10 | 0 | 395 masked
    "mini_model": _case(2, 405, [rows(4, 16, 385, sm=16), s2d(2, 3, 16, 16, 4, C2=195), rows(1, 10, 0, sm=10, masked=True)]),
    # segments that leave rows 0, 1, 5, 6 and 11 alone, given out of row order
    "holes": _case(2, 8, [s2d(1, 2, 4, 4, 2, C2=0, row0=7), rows(3, 4, 2, row0=2)], Mtot=12),
}
PLANTED = {"masked": (1, [(0, 0, 3, np.inf), (1, 0, 7, np.nan), (1, 0, 8, -np.inf)])}   # case -> (segment, [(b, m, j, value)])


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


def gen(name, tables=None):
    """Inputs of a case, per segment a dict of
      feat_full   the enclosing fp32 array, NaN outside the addressed elements; feat_off: element offset of feature(0, 0, 0)
                  (ROWS) or of frame[0, 0, 0, 0, 0] (S2D) in it; sb / sm / st / sc / sy: element strides
      feat        the features themselves: ROWS [B, M, C1]; S2D the frames [B, T, C, H, W] ([B, C, H, W] for four_d)
      table_full  [M + 2, ldt] with the table [M, C2] at [1:, 1:]; table_off, ldt, table   (None for C2 == 0)
      pad_full / pad_off / pad [Cp], token_full / token_off / token [Cc]                  (None where absent)
    tables: optional {segment index: [M, C2] float32} to use instead of random tables (a module's Fourier features)."""
    c = CASES[name]
    rng = np.random.default_rng(_seed(name))
    B, Cc = c["B"], c["Cc"]
    out = []
    for i, g in enumerate(c["segs"]):
        M, C1, C2 = g["M"], g["C1"], g["C2"]
        d = {}
        if g["kind"] == ROWS:
            sm, Mf = g["sm"], M + 2
            full = np.full((B, Mf, sm), np.nan, dtype=np.float32)
            feat = rng.standard_normal((B, M, C1)).astype(np.float32)
            if name in PLANTED and PLANTED[name][0] == i:
                for (b, m, j, v) in PLANTED[name][1]:
                    feat[b, m, j] = v
            full[:, 1:1 + M, :C1] = feat
            d.update(feat_full=full, feat_off=sm, sb=Mf * sm, sm=sm, st=0, sc=0, sy=0, feat=feat)
        else:
            T, C, H, W = g["T"], g["C"], g["H"], g["W"]
            Tf, Cf, Hf, Wf = T + 2, C + 2, H + 4, W + 6
            full = np.full((B, Tf, Cf, Hf, Wf), np.nan, dtype=np.float32)
            fr = rng.standard_normal((B, T, C, H, W)).astype(np.float32)
            full[:, 1:1 + T, 1:1 + C, 2:2 + H, 3:3 + W] = fr
            st, sc, sy = Cf * Hf * Wf, Hf * Wf, Wf
            d.update(feat_full=full, feat_off=st + sc + 2 * sy + 3, sb=Tf * st, sm=0, st=st, sc=sc, sy=sy,
                     feat=fr[:, 0] if g["four_d"] else fr)
        if C2 > 0:
            ldt = C2 + 3
            table = np.asarray(tables[i], dtype=np.float32) if tables and i in tables else \
                rng.standard_normal((M, C2)).astype(np.float32)
            assert table.shape == (M, C2)
            tf = np.full((M + 2, ldt), np.nan, dtype=np.float32)
            tf[1:1 + M, 1:1 + C2] = table
            d.update(table_full=tf, table_off=ldt + 1, ldt=ldt, table=table)
        else:
            d.update(table_full=None, table_off=0, ldt=0, table=None)
        for what, width, on in (("pad", Cc - C1 - C2, True), ("token", Cc, g["masked"])):
            if on and width > 0:
                v = (0.02 * rng.standard_normal(width)).astype(np.float32)
                vf = np.full(width + 2, np.nan, dtype=np.float32)
                vf[1:1 + width] = v
                d.update({what + "_full": vf, what + "_off": 1, what: v})
            else:
                d.update({what + "_full": None, what + "_off": 0, what: None})
        out.append(d)
    return out


def feature(g, d, b, m, j):
    """feature(b, m, j) of the header's formulas, read from the ENCLOSING array through offset and strides."""
    flat = d["feat_full"].reshape(-1)
    if g["kind"] == ROWS:
        return flat[d["feat_off"] + b * d["sb"] + m * d["sm"] + j]
    s, C, Hs, Ws = g["s"], g["C"], g["H"] // g["s"], g["W"] // g["s"]
    x, q = m % Ws, m // Ws
    y, t = q % Hs, q // Hs
    ch, q = j % C, j // C
    dx, dy = q % s, q // s
    return flat[d["feat_off"] + b * d["sb"] + t * d["st"] + ch * d["sc"] + (y * s + dy) * d["sy"] + x * s + dx]


def reference(name, data):
    """y [B, Mtot, ldy] float32: the definition; NaN wherever the call must not write (ldy gaps, uncovered rows)."""
    c = CASES[name]
    B, Cc = c["B"], c["Cc"]
    y = np.full((B, c["Mtot"], c["ldy"]), np.nan, dtype=np.float32)
    zero = np.float32(0.0)
    for g, d in zip(c["segs"], data):
        C1, C2 = g["C1"], g["C2"]
        for b in range(B):
            for m in range(g["M"]):
                x = np.empty(Cc, dtype=np.float32)
                for j in range(C1):
                    x[j] = feature(g, d, b, m, j)
                if C2:
                    x[C1:C1 + C2] = d["table_full"].reshape(-1)[d["table_off"] + m * d["ldt"]:][:C2]
                if Cc - C1 - C2:
                    x[C1 + C2:] = d["pad_full"][d["pad_off"]:][:Cc - C1 - C2]
                if g["masked"]:
                    with np.errstate(invalid="ignore"):
                        x = d["token"] + zero * x
                y[b, g["row0"] + m, :Cc] = x
    return y


def covered(name):
    """bool [Mtot, ldy]: the elements of a sample the call writes."""
    c = CASES[name]
    w = np.zeros((c["Mtot"], c["ldy"]), dtype=bool)
    for g in c["segs"]:
        w[g["row0"]:g["row0"] + g["M"], :c["Cc"]] = True
    return w


def masked_rows(name):
    c = CASES[name]
    w = np.zeros(c["Mtot"], dtype=bool)
    for g in c["segs"]:
        if g["masked"]:
            w[g["row0"]:g["row0"] + g["M"]] = True
    return w


def call_fields(name, data, addr):
    """The call of a case as plain values: (list of per-segment field dicts of pio_token_segment_t, keyword arguments).
    addr(segment index, what) -> byte address of the enclosing array `what` ("feat", "table", "pad", "token")."""
    c = CASES[name]
    segs = []
    for i, (g, d) in enumerate(zip(c["segs"], data)):
        f = dict(kind=g["kind"], row0=g["row0"], M=g["M"], C1=g["C1"], C2=g["C2"], sb=d["sb"], sm=d["sm"], st=d["st"],
                 sc=d["sc"], sy=d["sy"], ldt=d["ldt"], T=g.get("T", 0), C=g.get("C", 0), H=g.get("H", 0), W=g.get("W", 0),
                 s=g.get("s", 0), feature=addr(i, "feat") + 4 * d["feat_off"])
        for what, field in (("table", "table"), ("pad", "pad"), ("token", "token")):
            f[field] = None if d[what] is None else addr(i, what) + 4 * d[what + "_off"]
        segs.append(f)
    return segs, dict(ldy=c["ldy"], sYb=c["Mtot"] * c["ldy"], B=c["B"], Mtot=c["Mtot"], Cc=c["Cc"])


# ----------------------------------------------------------------------------------------------------
# refusals: (name, changes to a valid call, expected code).  The valid call: B = 2, Cc = 8 (vector path), ldy = 8,
# Mtot = 7, sYb = 56; segment 0 ROWS rows [0, 3): 4 | 3 | 1 with a token; segment 1 S2D rows [3, 7): C = 2, s = 2, T = 1,
# 4 x 4 -> 8 | 0 | 0.  A change is keyed by an argument name, or by (segment, field); "ptr+<b>": that pointer moved by b
# bytes; None: a NULL pointer.
# ----------------------------------------------------------------------------------------------------
VALID_ARGS = dict(nseg=2, ldy=8, sYb=56, B=2, Mtot=7, Cc=8)
VALID_SEGS = [
    dict(kind=ROWS, row0=0, M=3, C1=4, C2=3, sb=21, sm=7, st=0, sc=0, sy=0, ldt=3, T=0, C=0, H=0, W=0, s=0),
    dict(kind=S2D, row0=3, M=4, C1=8, C2=0, sb=32, sm=0, st=32, sc=16, sy=4, ldt=0, T=1, C=2, H=4, W=4, s=2),
]
VALID_PTRS = [("feature", "table", "pad", "token"), ("feature",)]       # the pointers each segment carries
REFUSALS = [
    ("y NULL", {"y": None}, PIO_E_ARG),
    ("nseg=0", {"nseg": 0}, PIO_E_ARG),
    ("nseg=9", {"nseg": 9}, PIO_E_ARG),
    ("kind=2", {(0, "kind"): 2}, PIO_E_ARG),
    ("ROWS feature NULL", {(0, "feature"): None}, PIO_E_ARG),
    ("S2D feature NULL", {(1, "feature"): None}, PIO_E_ARG),
    ("table NULL, C2 > 0", {(0, "table"): None}, PIO_E_ARG),
    ("pad NULL, Cp > 0", {(0, "pad"): None}, PIO_E_ARG),
    ("B=0", {"B": 0}, PIO_E_SHAPE),
    ("Mtot=0", {"Mtot": 0}, PIO_E_SHAPE),
    ("Cc=0", {"Cc": 0}, PIO_E_SHAPE),
    ("M=0", {(0, "M"): 0}, PIO_E_SHAPE),
    ("M=-1", {(0, "M"): -1}, PIO_E_SHAPE),
    ("C1=-1", {(0, "C1"): -1}, PIO_E_SHAPE),
    ("C2=-1", {(0, "C2"): -1}, PIO_E_SHAPE),
    ("C1+C2>Cc", {(0, "C2"): 5}, PIO_E_SHAPE),
    ("ldy<Cc", {"ldy": 4}, PIO_E_SHAPE),
    ("sYb inside a sample", {"sYb": 52}, PIO_E_SHAPE),
    ("S2D C1 != s s C", {(1, "C"): 1}, PIO_E_SHAPE),
    ("S2D M != T H/s W/s", {(1, "M"): 3}, PIO_E_SHAPE),
    ("S2D s=0", {(1, "s"): 0}, PIO_E_SHAPE),
    ("S2D s=9", {(1, "s"): 9}, PIO_E_SHAPE),
    ("S2D C=5", {(1, "C"): 5, (1, "C1"): 20, "Cc": 20, "ldy": 20, "sYb": 140}, PIO_E_SHAPE),
    ("S2D C=0", {(1, "C"): 0}, PIO_E_SHAPE),
    ("S2D T=0", {(1, "T"): 0}, PIO_E_SHAPE),
    ("S2D H % s", {(1, "H"): 5}, PIO_E_SHAPE),
    ("S2D W % s", {(1, "W"): 3}, PIO_E_SHAPE),
    ("row0<0", {(0, "row0"): -1}, PIO_E_SHAPE),
    ("segment past Mtot", {(1, "row0"): 4}, PIO_E_SHAPE),
    ("segments overlap", {(1, "row0"): 2}, PIO_E_SHAPE),
    ("y 4-byte aligned, vector path", {"y": "ptr+4"}, PIO_E_ALIGN),
    ("y misaligned", {"y": "ptr+2"}, PIO_E_ALIGN),
    ("ldy % 4", {"ldy": 10, "sYb": 72}, PIO_E_ALIGN),
    ("sYb % 4", {"sYb": 58}, PIO_E_ALIGN),
    ("ROWS feature misaligned", {(0, "feature"): "ptr+2"}, PIO_E_ALIGN),
    ("S2D feature misaligned", {(1, "feature"): "ptr+1"}, PIO_E_ALIGN),
    ("table misaligned", {(0, "table"): "ptr+2"}, PIO_E_ALIGN),
    ("pad misaligned", {(0, "pad"): "ptr+3"}, PIO_E_ALIGN),
    ("token misaligned", {(0, "token"): "ptr+2"}, PIO_E_ALIGN),
]


def refusal_fields(ptrs, changes):
    """The valid call with `changes` applied: (segment field dicts, keyword arguments, y address).  ptrs: "y" -> address,
    (segment, field) -> address for every pointer of VALID_PTRS."""
    args = dict(VALID_ARGS)
    segs = [dict(g) for g in VALID_SEGS]
    for i, fields in enumerate(VALID_PTRS):
        for f in ("feature", "table", "pad", "token"):
            segs[i][f] = ptrs[(i, f)] if f in fields else None
    y = ptrs["y"]

    def moved(p, v):
        return None if v is None else p + int(v[4:])
    for k, v in changes.items():
        if k == "y":
            y = moved(y, v)
        elif isinstance(k, tuple):
            segs[k[0]][k[1]] = moved(segs[k[0]][k[1]], v) if k[1] in ("feature", "table", "pad", "token") else v
        else:
            args[k] = v
    return segs, args, y
