"""CPU: libpio_hip.so loads and exports EVERY function include/pio_hip.h declares (no compute calls)."""
import ctypes
import keyword
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pio_hip.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(pio_[a-z0-9_]+)\s*\(", src)
    return sorted(set(n for n in names if not n.endswith("_t")))


def test_header_declares_something():
    fns = declared_functions()
    assert len(fns) >= 20 and "pio_encoder_fwd" in fns and "pio_gemm_nt" in fns


def test_library_exports_every_declared_symbol():
    from perceiverio_pytorch_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    missing = [f for f in declared_functions() if not hasattr(lib, f)]
    assert not missing, f"declared in pio_hip.h but not exported: {missing}"


def test_ctypes_table_matches_header():
    from perceiverio_pytorch_amd import _lib as L
    assert sorted(L.SIGNATURES) == declared_functions()


def test_host_side_queries_need_no_gpu():
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    assert lib.pio_version() == 101
    assert lib.pio_pad8(322) == 328 and lib.pio_pad8(8) == 8
    assert [lib.pio_padc(c) for c in (96, 250, 322, 504, 512, 1026, 1280)] == [96, 256, 384, 512, 512, 1088, 1280]
    assert lib.pio_packed_weight_bytes(1024, 1024, 8, 1) == 1024 * 1024 * 2
    assert lib.pio_packed_weight_bytes(322, 322, 1, 1) == 328 * 328 * 2
    assert lib.pio_packed_weight_bytes(10, 10, 3, 1) == 0          # not divisible by the head count
    assert lib.pio_error_string(-4) == b"workspace too small"


def _gcc(source, *flags, run=False):
    """Compile `source` against the real header (-Werror); with run=True also run it and return its output lines."""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c, out = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(source)
        r = subprocess.run(["gcc", "-std=c11", "-Werror", "-I", os.path.join(ROOT, "include"), *flags, c, "-o", out],
                           capture_output=True, text=True)
        if not run or r.returncode:
            return r
        return subprocess.check_output([out], text=True).splitlines()


def _c_name(field):
    """The header's spelling of a ctypes field name (in_ -> in)."""
    return field[:-1] if field.endswith("_") and keyword.iskeyword(field[:-1]) else field


def test_every_struct_matches_the_c_layout():
    """sizeof of EVERY struct of the header, and offsetof and sizeof of every one of its fields, as a C compiler has them,
    against the ctypes classes the reader built."""
    from perceiverio_pytorch_amd import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    in_header = re.findall(r"\}\s*(pio_\w+_t)\s*;", src)
    assert len(in_header) >= 17 and sorted(in_header) == sorted(L.CLASS_NAMES)
    lines, want = [], []
    for alias, name in L.CLASS_NAMES.items():
        cls = getattr(L, name)
        assert issubclass(cls, ctypes.Structure) and cls.__name__ == name
        lines.append(f'printf("{alias} %zu\\n", sizeof({alias}));')
        want.append(f"{alias} {ctypes.sizeof(cls)}")
        for field, _ in cls._fields_:
            f = _c_name(field)
            lines.append(f'printf("{alias}.{f} %zu %zu\\n", offsetof({alias}, {f}), sizeof((({alias} *)0)->{f}));')
            want.append(f"{alias}.{f} {getattr(cls, field).offset} {getattr(cls, field).size}")
    assert len(want) > 200 and "pio_mlp_t.in 80 4" in want
    got = _gcc('#include <stdio.h>\n#include "pio_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n",
               run=True)
    assert got == want


def _prototype_unit(decls, signatures):
    """One translation unit that holds every parsed prototype against the declared function: a function-pointer
    initialisation per function (an incompatible type is an error), and per scalar type what the ctypes type stands for
    -- its size, whether it is signed, whether it is a floating type."""
    from perceiverio_pytorch_amd import _lib as L
    out = ['#include "pio_hip.h"']
    for name, (ret, params) in decls.items():
        args = ", ".join(L.c_type(t) for t, _ in params) or "void"
        out.append(f"static {L.c_type(ret)} (*const check_{name})({args}) = {name};")
        restype, argtypes = signatures[name]
        for t, ct in zip([ret] + [t for t, _ in params], [restype] + list(argtypes)):
            c = L.c_type(t)
            out.append(f'_Static_assert(sizeof({c}) == {ctypes.sizeof(ct)}, "{name}: {c}");')
            if not t[2]:
                signed, floating = int(ct(-1).value < 0), int(ct in (ctypes.c_float, ctypes.c_double))
                out.append(f'_Static_assert((({c})-1 < 0) == {signed} && (({c})0.5 != 0) == {floating}, "{name}: {c}");')
    return "\n".join(out) + "\nint main(void) { return 0; }\n"


def test_every_prototype_matches_the_declared_function():
    """What the reader parsed of EVERY prototype -- return type, parameter types, const included -- rebuilt as a function
    pointer that the compiler accepts for the declared function; one int64_t read as int32_t is refused."""
    from perceiverio_pytorch_amd import _lib as L
    assert sorted(L.DECLS) == sorted(L.SIGNATURES) == sorted(L.PARAMS) == declared_functions() and len(L.DECLS) >= 53
    for name, (_, params) in L.DECLS.items():
        assert len(params) == len(L.SIGNATURES[name][1]) == len(L.PARAMS[name])
    assert L.PARAMS["pio_pack_linear"][:4] == ("w", "bias", "out", "in_")
    assert L.SIGNATURES["pio_error_string"] == (ctypes.c_char_p, [ctypes.c_int])
    ok = _gcc(_prototype_unit(L.DECLS, L.SIGNATURES), "-c")
    assert ok.returncode == 0, ok.stderr[-2000:]
    # the control: ids_sb of pio_embed_tokens mis-read as int32_t, and a dropped const, must not compile
    for name, i, wrong in (("pio_embed_tokens", 2, (False, "int32_t", False)), ("pio_vocab_topk", 0, (False, "float", True))):
        ret, params = L.DECLS[name]
        assert params[i][0] != wrong
        bad = dict(L.DECLS)
        bad[name] = (ret, params[:i] + ((wrong, params[i][1]),) + params[i + 1:])
        r = _gcc(_prototype_unit({name: bad[name]}, {name: L.SIGNATURES[name]}), "-c")
        assert r.returncode != 0 and "incompatible" in r.stderr, r.stderr[-2000:]


_SNIPPET = "typedef struct pio_linear_t {\n    const void *w_hi;\n    %s;\n} pio_linear_t;\n"


@pytest.mark.parametrize("text, line, names", [
    (_SNIPPET % "uint16_t n", 3, ("unknown type", "uint16_t")),
    (_SNIPPET % "void (*done)(int32_t code)", 3, ("unsupported field", "(*done)")),
    (_SNIPPET % "int32_t n : 3", 3, ("unsupported field", "n : 3")),
    (_SNIPPET % "struct { int32_t a; } inner", 1, ("unsupported construct", "typedef struct pio_linear_t")),
    ("\ntypedef struct pio_tile_t {\n    int32_t n;\n} pio_tile_t;\n", 4, ("pio_tile_t", "CLASS_NAMES")),
    (_SNIPPET % "int32_t ys[PIO_MAX_TILES]", 3, ("ys[PIO_MAX_TILES]", "undefined macro")),
    ("#define PIO_SCALE 1.5f\n", 1, ("PIO_SCALE", "not an integer")),
    ("int pio_version(void);\nint pio_apply(int32_t n, int (*fn)(int));\n", 2, ("unsupported", "pio_apply")),
    ("int pio_sum(pio_missing_t *p, void *stream);\n", 1, ("unknown type", "pio_missing_t *")),
])
def test_reader_refuses_what_it_does_not_cover(text, line, names):
    from perceiverio_pytorch_amd import _lib as L
    with pytest.raises(L.PioError) as e:
        L.read_header(text, "snippet.h")
    assert str(e.value).startswith(f"snippet.h:{line}: ") and all(n in str(e.value) for n in names), str(e.value)


def test_reader_on_a_snippet_and_a_missing_header(monkeypatch):
    from perceiverio_pytorch_amd import _lib as L
    h = L.read_header("#define PIO_MAX_TILES 3 /* c */\nenum { PIO_A = 0, PIO_E_X = -9 };\n" + _SNIPPET % "int32_t in, ys[PIO_MAX_TILES]"
                      + "size_t pio_bytes(const pio_linear_t *l, pio_linear_t by_value, const float *x, void *stream);\n")
    assert h.constants == {"PIO_MAX_TILES": 3, "PIO_A": 0, "PIO_E_X": -9}
    cls = h.structs["pio_linear_t"]
    assert [(n, t) for n, t in cls._fields_] == [("w_hi", ctypes.c_void_p), ("in_", ctypes.c_int32), ("ys", ctypes.c_int32 * 3)]
    assert h.signatures == {"pio_bytes": (ctypes.c_size_t, [ctypes.POINTER(cls), cls, ctypes.c_void_p, ctypes.c_void_p])}
    assert h.decls["pio_bytes"][1][2] == ((True, "float", True), "x")
    monkeypatch.setattr(L, "HEADER", os.path.join(ROOT, "include", "no_such.h"))
    with pytest.raises(L.PioError, match="no_such.h"):
        L._load()


class _NoCalls:
    """In place of the library: any entry point looked up on it is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was looked up on the library")


@pytest.mark.parametrize("args, named, names", [
    ((1, 2, 3), dict(Cq=4), ("pio_build_queries", "missing ldy, Qtot")),                             # a missing name
    ((), dict(segs=1, nseg=2, y=3, ldy=4, Qtot=5, Cq=6, ldx=7), ("pio_build_queries", "no parameter 'ldx'")),
    ((1, 2), dict(nseg=2, y=3, ldy=4, Qtot=5, Cq=6), ("pio_build_queries", "'nseg' given twice")),   # both ways
    ((1, 2, 3, 4, 5, 6, 7, 8), {}, ("pio_build_queries", "positional")),
])
def test_call_refuses_wrong_names_before_anything_runs(monkeypatch, args, named, names):
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    monkeypatch.setattr(L, "lib", lambda: _NoCalls())
    monkeypatch.setattr(R, "call", lambda *a, **k: pytest.fail("runtime.call was reached"))
    with pytest.raises(L.PioError) as e:
        R.call_named("cuda:0", "pio_build_queries", *args, **named)
    assert all(n in str(e.value) for n in names), str(e.value)


def test_arguments_refuses_a_repeated_name_and_an_unknown_entry():
    from perceiverio_pytorch_amd import _lib as L
    with pytest.raises(L.PioError, match="pio_range_probe_mark: parameter 'part' given twice"):
        L.arguments("pio_range_probe_mark", (), [("part", 1), ("part", 2)])
    with pytest.raises(L.PioError, match="pio_no_such_entry"):
        L.arguments("pio_no_such_entry", (1,), {})
    assert L.arguments("pio_range_probe_mark", (), [("part", 1)]) == L.arguments("pio_range_probe_mark", (1,), {}) == (1,)


def test_named_arguments_lay_out_as_the_positional_calls_did():
    """A fully named pio_conv1x1_tokens and pio_vocab_topk against the positional tuples of the call sites before names:
    fused_io.conv1x1_tokens passed (x, x.stride(0..3), w2, w2.stride(0), bias, y, n, m * n, b, c, h, w, s, n), vocab_topk in
    its selection mode (None, 0, 0, None, 0, None, b, p, v, 0, k, ids, logprob, None, logits, v), each then the stream."""
    from perceiverio_pytorch_amd import _lib as L
    x, w2, y, st, (b, c, h, w, s, n, m) = 0x1000, 0x2000, 0x3000, (9408, 3136, 56, 1), (2, 3, 56, 56, 2, 64, 784)
    got = L.arguments("pio_conv1x1_tokens", (), dict(
        x=x, sb=st[0], sc=st[1], sy=st[2], sx=st[3], w=w2, ldw=c, bias=None, y=y, ldy=n, sYb=m * n, B=b, C=c, H=h, W=w, s=s,
        N=n, stream=0x77))
    assert got == (x, 9408, 3136, 56, 1, w2, c, None, y, n, m * n, b, c, h, w, s, n, 0x77)
    ids, logprob, logits, (b, p, v, k) = 0x4000, 0x5000, 0x6000, (2, 5, 262, 3)
    named = dict(x=None, x_sb=0, ldx=0, w=None, ldw=0, bias=None, B=b, Q=p, V=v, K=0, k=k, ids=ids, logprob=logprob, lse=None,
                 logits=logits, ldl=v, stream=0x77)
    want = (None, 0, 0, None, 0, None, b, p, v, 0, k, ids, logprob, None, logits, v, 0x77)
    assert L.arguments("pio_vocab_topk", (), named) == want
    assert L.arguments("pio_vocab_topk", want[:6], {k_: v_ for k_, v_ in named.items() if k_ not in L.PARAMS["pio_vocab_topk"][:6]}) == want
    assert L.arguments("pio_vocab_topk", want, {}) == want
