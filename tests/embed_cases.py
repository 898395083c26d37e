"""Cases and the definition of the language front end (pio_embed_tokens, csrc/pio_embed.hip).

Numpy only; shared by tests/test_embed_front_host.py (CPU: the definition against `embed(ids) + pos` in torch, the refusal
table, routing) and tests/test_embed_front_gpu.py (MI355X: the kernel against the definition).

The definition restates include/pio_hip.h by plain indexing -- not the torch functions, not the kernel.  With
id = ids[b ids_sb + t]:

    0 <= id < V:   y[b y_sb + t ldy + c] = fl32(table[id ldt + c] + pos[t ldp + c])     tokens[b tok_sb + t ldtok + c] = table[id ldt + c]
    otherwise:     both rows NaN in [0, C), the flag word 1

Everything is compared as int32 bit patterns where the definition is finite, and must be NaN everywhere else: on the rows of
bad ids, in the pitch gaps [C, ld), between samples (y_sb > T ldy) and in front of a shifted output.

Memory safety by construction:
  * table sits between GUARD_ROWS (>= 2) NaN rows in front and behind and has NaN pitch gaps, pos between NaN rows, both
    optionally shifted by one element (col_off): a read outside them gives a NaN where the definition is finite;
  * the ids of a sliced id matrix (ids_sb > T) that the call must skip, and the entries around the matrix, name OTHER valid
    rows: a row built from one of them differs visibly;
  * bad ids are -1, V and V + 1 (a kernel that indexed with them would still land in the NaN guard rows) and, for int64,
    2^32 + k and -2^32 + k with 0 <= k < V (a kernel that narrowed before the range test would read the valid row k and
    produce a finite row);
  * outputs are NaN before the call and sit between 4 KiB guard bands (tests/test_flow_front_gpu.py GuardedOut).
"""
import numpy as np

PIO_OK, PIO_E_SHAPE, PIO_E_ALIGN, PIO_E_ARG = 0, -1, -2, -6
STRIP = 32          # tokens per workgroup strip in csrc/pio_embed.hip (EM_TS): cases cross it on purpose
GUARD_ROWS = 3      # NaN rows in front of and behind the table


def _case(B, T, C, V, id_bytes=8, ids_sb=None, ldt=None, ldp=None, ldy=None, y_sb=None, ldtok=None, tok_sb=None,
          tokens=False, y_off=0, col_off=0, bad=None, flag=True):
    """ld* default to dense (C, + col_off for the inputs), sample strides to T * ld.  y_off: elements the output pointer is
    shifted by; col_off: elements table and pos are shifted by inside their rows; bad: {(b, t): id}; flag: pass bad_ids."""
    ldy = C if ldy is None else ldy
    ldtok = C if ldtok is None else ldtok
    return dict(B=B, T=T, C=C, V=V, id_bytes=id_bytes, ids_sb=T if ids_sb is None else ids_sb,
                ldt=C + col_off if ldt is None else ldt, ldp=C + col_off if ldp is None else ldp, ldy=ldy,
                y_sb=T * ldy if y_sb is None else y_sb, tokens=tokens, ldtok=ldtok,
                tok_sb=T * ldtok if tok_sb is None else tok_sb, y_off=y_off, col_off=col_off, bad=dict(bad or {}), flag=flag)


P32 = 2 ** 32
CASES = {
    # the smallest call; V = 1: every id is row 0
    "c1": _case(1, 1, 1, 1, id_bytes=4, tokens=True),
    # dword path: C odd, every pitch larger than C and odd, a sliced id matrix, a gap between samples, shifted inputs
    "c3_pitches": _case(3, 5, 3, 2, ids_sb=8, ldt=5, ldp=7, ldy=7, y_sb=5 * 7 + 6, tokens=True, ldtok=5, tok_sb=5 * 5 + 3,
                        col_off=1),
    # one 16-byte vector per row, everything dense, tokens NULL
    "c4_vec": _case(1, 5, 4, 2, id_bytes=4),
    # C % 4 != 0 behind aligned pitches: dwords
    "c6_pitch8": _case(3, 5, 6, 262, id_bytes=4, ldt=8, ldp=8, ldy=8, tokens=True, ldtok=8),
    # C % 4 == 0, y shifted by 4 bytes: alignment demotes the call to dwords (tokens stay aligned); one more than a strip
    "c8_y_off4": _case(1, STRIP + 1, 8, 262, tokens=True, y_off=1),
    # 65 vectors: a second trip of the lane loop; vector path with every pitch larger than C
    "c260_trip2": _case(1, 5, 260, 262, ldt=264, ldp=268, ldy=264, tokens=True, ldtok=272),
    # the shipped model's row: 192 vectors, V = 262
    "c768": _case(1, 5, 768, 262, id_bytes=4),
    # vector path, several workgroups per sample (3 strips), a sliced id matrix, a gap between samples
    "strips": _case(3, 2 * STRIP + 6, 4, 262, ids_sb=2 * STRIP + 11, ldy=8, y_sb=(2 * STRIP + 6) * 8 + 8),
    # vector path, one more than a strip, tokens with a pitch and a sample stride of their own
    "t33_tokens": _case(3, STRIP + 1, 8, 2, id_bytes=4, ids_sb=STRIP + 4, tokens=True, ldtok=12,
                        tok_sb=(STRIP + 1) * 12 + 4),
    # bad ids, int32, vector path, no tokens
    "bad_i32": _case(3, 5, 4, 262, id_bytes=4, bad={(0, 1): -1, (1, 0): 262, (2, 4): 263}),
    # bad ids, int64, vector path, tokens: the narrowing cases
    "bad_i64": _case(1, STRIP + 1, 8, 262, tokens=True,
                     bad={(0, 0): -1, (0, 3): 262, (0, 7): 263, (0, 8): P32 + 5, (0, 31): -P32 + 261, (0, 32): P32,
                          (0, 20): 2 ** 31 + 7}),
    # bad ids on the dword path
    "bad_dwords": _case(3, 5, 3, 2, ldy=4, tokens=True, bad={(0, 0): 2, (1, 2): -1, (2, 4): P32 + 1, (2, 0): -P32}),
    # bad ids without a flag word: the rows are NaN all the same
    "bad_no_flag": _case(1, 5, 4, 2, tokens=True, bad={(0, 2): 3, (0, 4): -1}, flag=False),
}


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


def gen(name):
    """Inputs of a case: <what>_full (the enclosing array), <what>_off (element offset of the first addressed element) for
    what in ids (int32 / int64), table, pos (float32); `ids` [B, T] the addressed ids themselves (int64)."""
    c = CASES[name]
    B, T, C, V = c["B"], c["T"], c["C"], c["V"]
    rng = np.random.default_rng(_seed(name))
    ids = rng.integers(0, V, size=(B, T), dtype=np.int64)
    free = [(b, t) for b in range(B) for t in range(T) if (b, t) not in c["bad"]]
    ids[free[0]] = 0                             # row 0, row V - 1 and a repeat, wherever there is room for them
    if len(free) > 1:
        ids[free[-1]] = V - 1
    if len(free) > 3:
        ids[free[2]] = ids[free[1]]
    for (b, t), v in c["bad"].items():
        ids[b, t] = v
    front = 3
    mat = np.empty((B, c["ids_sb"]), dtype=np.int64)
    mat[:, :T] = ids
    for j in range(T, c["ids_sb"]):              # skipped entries: another valid row than their left neighbour's
        mat[:, j] = (np.clip(mat[:, j - 1], 0, V - 1) + V // 2 + 1) % V
    ids_full = np.concatenate([(np.clip(ids[0, :1], 0, V - 1) + V // 2 + 1) % V * np.ones(front, dtype=np.int64),
                               mat.reshape(-1), np.full(front, (V // 2) % V, dtype=np.int64)])
    ids_full = ids_full.astype(np.int32 if c["id_bytes"] == 4 else np.int64)
    out = dict(ids=ids, ids_full=ids_full, ids_off=front)
    for what, rows, ld, guard in (("table", V, c["ldt"], GUARD_ROWS), ("pos", T, c["ldp"], 1)):
        assert ld >= C + c["col_off"]
        full = np.full((rows + 2 * guard, ld), np.nan, dtype=np.float32)
        full[guard:guard + rows, c["col_off"]:c["col_off"] + C] = (0.02 * rng.standard_normal((rows, C))).astype(np.float32)
        out.update({what + "_full": full, what + "_off": guard * ld + c["col_off"]})
    return out


def out_elems(c, which):
    """Elements of the array an output lives in: everything the call may address, with the shift in front and a tail."""
    ld, sb = (c["ldy"], c["y_sb"]) if which == "y" else (c["ldtok"], c["tok_sb"])
    off = c["y_off"] if which == "y" else 0
    return off + (c["B"] - 1) * sb + c["T"] * ld + 5


def reference(name, data):
    """(y, tokens or None, flag): the definition as flat float32 arrays of out_elems() elements, NaN wherever the call must
    not write or must write NaN; flag 1 if any id is out of range (what the word holds when it was 0 before the call and
    the case passes it)."""
    c = CASES[name]
    B, T, C, V = c["B"], c["T"], c["C"], c["V"]
    ids, table, pos = data["ids_full"].reshape(-1), data["table_full"].reshape(-1), data["pos_full"].reshape(-1)
    y = np.full(out_elems(c, "y"), np.nan, dtype=np.float32)
    tok = np.full(out_elems(c, "tokens"), np.nan, dtype=np.float32) if c["tokens"] else None
    flag = 0
    for b in range(B):
        for t in range(T):
            i = int(ids[data["ids_off"] + b * c["ids_sb"] + t])
            if not 0 <= i < V:
                flag = 1
                continue
            e = table[data["table_off"] + i * c["ldt"]:][:C]
            p = pos[data["pos_off"] + t * c["ldp"]:][:C]
            o = c["y_off"] + b * c["y_sb"] + t * c["ldy"]
            y[o:o + C] = e + p                   # (float32 + float32: one rounded add per element)
            if tok is not None:
                o = b * c["tok_sb"] + t * c["ldtok"]
                tok[o:o + C] = e
    return y, tok, flag


def compare(got, ref, what):
    """A flat float32 output against the definition: equal int32 bit patterns where the definition is finite, NaN elsewhere."""
    got = np.ascontiguousarray(got, dtype=np.float32).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.isnan(got[~fin]).all(), \
        f"{what}: {int((~np.isnan(got[~fin])).sum())} elements that must stay / be NaN are not (a pitch gap, a sample gap or a " \
        f"bad id's row), first at {int(np.nonzero(~fin & ~np.isnan(got))[0][0])}"
    same = got.view(np.int32) == ref.view(np.int32)
    if not same[fin].all():
        i = int(np.nonzero(fin & ~same)[0][0])
        raise AssertionError(f"{what}: {int((fin & ~same).sum())} elements differ, first at {i}: got {got[i]!r} ref {ref[i]!r}")


def call_fields(name, data, addr):
    """The call of a case as plain values (keyword arguments of pio_embed_tokens without the stream).  addr(what) -> byte
    address of the enclosing array `what` in ids / table / pos / y / tokens / bad_ids."""
    c = CASES[name]
    return dict(ids=addr("ids") + c["id_bytes"] * data["ids_off"], id_bytes=c["id_bytes"], ids_sb=c["ids_sb"],
                table=addr("table") + 4 * data["table_off"], ldt=c["ldt"], V=c["V"],
                pos=addr("pos") + 4 * data["pos_off"], ldp=c["ldp"],
                y=addr("y") + 4 * c["y_off"], y_sb=c["y_sb"], ldy=c["ldy"],
                tokens=addr("tokens") if c["tokens"] else None, tok_sb=c["tok_sb"], ldtok=c["ldtok"],
                bad_ids=addr("bad_ids") if c["flag"] else None, B=c["B"], T=c["T"], C=c["C"])


ARG_ORDER = ("ids", "id_bytes", "ids_sb", "table", "ldt", "V", "pos", "ldp", "y", "y_sb", "ldy", "tokens", "tok_sb", "ldtok",
             "bad_ids", "B", "T", "C")
POINTERS = ("ids", "table", "pos", "y", "tokens", "bad_ids")

# ----------------------------------------------------------------------------------------------------
# refusals: (name, changes to a valid call, expected code).  The valid call: B = 2, T = 3, C = 4, V = 5, int64 ids, every
# array dense, tokens and the flag word given.  A change is keyed by an argument name; for a pointer "ptr+<b>" moves it by b
# bytes, None is NULL, "=y" aliases y.  Each row launches nothing and leaves y NaN.
# ----------------------------------------------------------------------------------------------------
VALID = dict(id_bytes=8, ids_sb=3, ldt=4, V=5, ldp=4, y_sb=12, ldy=4, tok_sb=12, ldtok=4, B=2, T=3, C=4)
I31 = 2 ** 31 - 1
REFUSALS = [
    ("ids NULL", {"ids": None}, PIO_E_ARG),
    ("table NULL", {"table": None}, PIO_E_ARG),
    ("pos NULL", {"pos": None}, PIO_E_ARG),
    ("y NULL", {"y": None}, PIO_E_ARG),
    ("id_bytes=2", {"id_bytes": 2}, PIO_E_ARG),
    ("id_bytes=16", {"id_bytes": 16}, PIO_E_ARG),
    ("id_bytes=0", {"id_bytes": 0}, PIO_E_ARG),
    ("int64 ids 4-byte aligned", {"ids": "ptr+4"}, PIO_E_ARG),
    ("int32 ids 2-byte aligned", {"ids": "ptr+2", "id_bytes": 4}, PIO_E_ARG),
    ("table misaligned", {"table": "ptr+2"}, PIO_E_ARG),
    ("pos misaligned", {"pos": "ptr+1"}, PIO_E_ARG),
    ("y misaligned", {"y": "ptr+2"}, PIO_E_ARG),
    ("tokens misaligned", {"tokens": "ptr+3"}, PIO_E_ARG),
    ("bad_ids misaligned", {"bad_ids": "ptr+2"}, PIO_E_ARG),
    ("B=0", {"B": 0}, PIO_E_SHAPE),
    ("B=-1", {"B": -1}, PIO_E_SHAPE),
    ("T=0", {"T": 0}, PIO_E_SHAPE),
    ("C=0", {"C": 0}, PIO_E_SHAPE),
    ("V=0", {"V": 0}, PIO_E_SHAPE),
    ("ldt<C", {"ldt": 3}, PIO_E_SHAPE),
    ("ldp<C", {"ldp": 3}, PIO_E_SHAPE),
    ("ldy<C", {"ldy": 3, "y_sb": 9}, PIO_E_SHAPE),
    ("ldtok<C", {"ldtok": 3, "tok_sb": 9}, PIO_E_SHAPE),
    ("ids_sb<T, B>1", {"ids_sb": 2}, PIO_E_SHAPE),
    ("y_sb<T*ldy, B>1", {"y_sb": 11}, PIO_E_SHAPE),
    ("tok_sb<T*ldtok, B>1", {"tok_sb": 11}, PIO_E_SHAPE),
    ("T*ldy beyond 64 bits", {"ldy": 2 ** 62, "y_sb": 2 ** 62}, PIO_E_SHAPE),
    ("tokens == y", {"tokens": "=y"}, PIO_E_SHAPE),
    ("B * strips beyond the grid", {"B": I31, "T": I31, "ids_sb": I31, "y_sb": 4 * I31, "tok_sb": 4 * I31}, PIO_E_SHAPE),
]
# changes that stay VALID (the call runs): the fall-backs of the vector path and the optional arguments are not refusals
ACCEPTED = [
    ("the valid call", {}),
    ("tokens NULL", {"tokens": None}),
    ("tokens NULL, its pitch and stride not looked at", {"tokens": None, "ldtok": 0, "tok_sb": 0}),
    ("bad_ids NULL", {"bad_ids": None}),
    ("int32 ids", {"id_bytes": 4}),
    ("int32 ids 4-byte aligned", {"id_bytes": 4, "ids": "ptr+4"}),
    ("y 4-byte aligned", {"y": "ptr+4"}),
    ("tokens 8-byte aligned", {"tokens": "ptr+8"}),
    ("ldy=5", {"ldy": 5, "y_sb": 15}),
    ("y_sb=13", {"y_sb": 13}),
    ("ids_sb=5", {"ids_sb": 5}),
    ("B=1: sample strides not read", {"B": 1, "ids_sb": 0, "y_sb": 0, "tok_sb": 0}),
]


def refusal_fields(ptrs, changes):
    """The valid call with `changes` applied, as keyword arguments.  ptrs: pointer argument -> address."""
    f = dict(VALID)
    f.update({k: ptrs[k] for k in POINTERS})
    for k, v in changes.items():
        if k in POINTERS:
            f[k] = None if v is None else ptrs["y"] if v == "=y" else ptrs[k] + int(v[4:])
        else:
            f[k] = v
    return f


def written(f, which):
    """bool mask over the flat elements behind the (possibly moved) output pointer of an ACCEPTED call: what it writes."""
    ld, sb = (f["ldy"], f["y_sb"]) if which == "y" else (f["ldtok"], f["tok_sb"])
    n = (f["B"] - 1) * sb + f["T"] * ld
    m = np.zeros(n, dtype=bool)
    for b in range(f["B"]):
        for t in range(f["T"]):
            o = b * sb + t * ld
            m[o:o + f["C"]] = True
    return m
