"""ctypes binding of libpio_hip.so, read from include/pio_hip.h: the header is the only statement of the C-ABI.

At import the header is parsed once (read_header) and gives every PIO_* constant, one ctypes.Structure per struct
(CLASS_NAMES), SIGNATURES and PARAMS.  A new entry point or constant needs no edit here; a new struct needs its line in
CLASS_NAMES.  The reader covers the C subset the header is written in and refuses anything else, naming the line.

The library is built in-tree (``perceiverio_pytorch_amd/libpio_hip.so``) by ``__graft_entry__.build()``
or ``make -C perceiverio_pytorch_amd/csrc``.  There is NO fallback: if the shared object is missing or
fails to load, importing the compute modules raises -- the hot path only exists as HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import keyword
import os
import re
import subprocess
from types import SimpleNamespace

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PIO_LIB_PATH", os.path.join(_HERE, "libpio_hip.so"))  # override: A/B builds only
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "pio_hip.h")


class PioError(RuntimeError):
    pass


# pio_*_t -> Python class.  Every struct of the header needs its line: several names cannot be derived.
CLASS_NAMES = {
    "pio_linear_t": "Linear", "pio_layernorm_t": "LayerNorm", "pio_attention_t": "Attention", "pio_mlp_t": "Mlp",
    "pio_ln_fold_t": "LnFold", "pio_self_attention_t": "SelfAttention", "pio_cross_attention_t": "CrossAttention",
    "pio_tensor3_t": "Tensor3", "pio_call_opts_t": "CallOpts", "pio_encoder_call_t": "EncoderCall",
    "pio_decoder_call_t": "DecoderCall", "pio_token_segment_t": "TokenSegment", "pio_query_segment_t": "QuerySegment",
    "pio_head_segment_t": "HeadSegment", "pio_flow_blend_t": "FlowBlend", "pio_image_src_t": "ImageSource",
    "pio_gemm_t": "Gemm"}

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float,
            "double": C.c_double, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32}

# one top-level construct of the comment-stripped header
_ITEM = re.compile(r"""\s*(?:
      \#[ \t]*define[ \t]+(?P<macro>\w+)(?P<value>[^\n]*)
    | \#[ \t]*ifdef[ \t]+__cplusplus\b.*?\#[ \t]*endif\b           # the extern "C" brackets
    | \#[ \t]*(?:include|ifndef|endif)\b[^\n]*
    | enum\s*\{(?P<enum>[^{};]*)\}\s*;
    | typedef\s+struct\s+\w+\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)\s*;
    | (?P<proto>[^;{}\#]*\))\s*;
    )""", re.S | re.X)
_ENUMERATOR = re.compile(r"(\w+)\s*=\s*(-?\d+)$")
_FIELDS = re.compile(r"(const\s+)?(\w+)\b\s*(.*)$", re.S)                           # type, then declarators
_DECLARATOR = re.compile(r"(\*?)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?$")
_PROTO = re.compile(r"(const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*\((.*)\)$", re.S)
_PARAM = re.compile(r"(const\s+)?(\w+)\s*(\*?)\s*(\w+)$")


def py_name(name: str) -> str:
    """A field or parameter name of the header as Python spells it: a keyword gets a trailing underscore (in -> in_)."""
    return name + "_" * keyword.iskeyword(name)


def c_type(t) -> str:
    """The C spelling of a parsed type (const, base, pointer)."""
    return ("const " if t[0] else "") + t[1] + (" *" if t[2] else "")


def read_header(text: str, path: str = HEADER) -> SimpleNamespace:
    """What header `text` declares: .constants {PIO_X: int} of every integer #define and enumerator; .structs {pio_x_t:
    ctypes class}, built in header order; .decls {function: (return type, ((parameter type, parameter name), ..))} with
    types as (const, base, pointer) -- see c_type; .signatures {function: (restype, argtypes)}.  PioError, naming `path`,
    the line and the construct, for anything outside the subset."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: "\n" * m.group().count("\n"), text, flags=re.S)
    constants, structs, decls, signatures = {}, {}, {}, {}

    def fail(pos, what):
        raise PioError(f"{path}:{text.count(chr(10), 0, pos) + 1}: {what}")

    def ctype(t, pos, ret=False):
        _, base, ptr = t
        if base in structs:
            return C.POINTER(structs[base]) if ptr else structs[base]
        if ptr and (base in _SCALARS or base in ("void", "char")):
            return C.c_char_p if ret and base == "char" else C.c_void_p
        if not ptr and base in _SCALARS:
            return _SCALARS[base]
        fail(pos, f"unknown type {c_type(t)!r}")

    def pieces(chunk, start, sep):
        """(position, stripped text) of the non-empty `sep`-separated pieces of `chunk`, which begins at `start`."""
        for part in chunk.split(sep):
            if part.strip():
                yield start + len(part) - len(part.lstrip()), part.strip()
            start += len(part) + 1

    pos = 0
    while text[pos:].strip():
        m = _ITEM.match(text, pos)
        if m is None:
            rest = text[pos:].lstrip()
            fail(len(text) - len(rest), f"unsupported construct {rest.splitlines()[0]!r}")
        pos = m.end()
        if m["macro"] and m["value"].strip():
            if not re.fullmatch(r"-?\d+", m["value"].strip()):
                fail(m.start("macro"), f"#define {m['macro']} is not an integer constant")
            constants[m["macro"]] = int(m["value"])
        elif m["enum"] is not None:
            for p, item in pieces(m["enum"], m.start("enum"), ","):
                e = _ENUMERATOR.match(item)
                if e is None:
                    fail(p, f"enumerator {item!r} without an integer value")
                constants[e[1]] = int(e[2])
        elif m["struct"]:
            alias, fields = m["struct"], []
            if alias not in CLASS_NAMES:
                fail(m.start("struct"), f"struct {alias} has no entry in CLASS_NAMES")
            for p, decl in pieces(m["body"], m.start("body"), ";"):
                f = _FIELDS.match(decl)
                names = [_DECLARATOR.match(item) for _, item in pieces(f[3], 0, ",")] if f else []
                if not names or None in names:
                    fail(p, f"unsupported field {decl!r} of {alias}")
                for d in names:
                    t = ctype((bool(f[1]), f[2], bool(d[1])), p)
                    if d[3] is not None:
                        if not d[3].isdigit() and d[3] not in constants:
                            fail(p, f"array {d[2]}[{d[3]}] of {alias} is sized by an undefined macro")
                        t = t * int(constants.get(d[3], d[3]))
                    fields.append((py_name(d[2]), t))
            structs[alias] = type(CLASS_NAMES[alias], (C.Structure,), {"_fields_": fields, "__doc__": alias})
        elif m["proto"]:
            f = _PROTO.match(m["proto"].strip())
            if f is None:
                fail(m.start("proto"), f"unsupported declaration {' '.join(m['proto'].split())!r}")
            name, ret, params, argtypes = f[4], (bool(f[1]), f[2], bool(f[3])), [], []
            for p, item in pieces(f[5] if f[5].strip() != "void" else "", m.start("proto") + f.start(5), ","):
                a = _PARAM.match(item)
                if a is None:
                    fail(p, f"unsupported parameter {item!r} of {name}")
                params.append(((bool(a[1]), a[2], bool(a[3])), a[4]))
                argtypes.append(ctype(params[-1][0], p))
            decls[name] = (ret, tuple(params))
            signatures[name] = (ctype(ret, m.start("proto"), ret=True), argtypes)
    return SimpleNamespace(constants=constants, structs=structs, decls=decls, signatures=signatures)


def _load() -> SimpleNamespace:
    try:
        with open(HEADER) as f:
            text = f.read()
    except OSError as e:
        raise PioError(f"{HEADER}: cannot read the C-ABI header ({e.strerror})") from None
    return read_header(text)


_header = _load()
globals().update(_header.constants)                                                   # PIO_OK, PIO_DT_F16, PIO_MAX_* ...
globals().update({CLASS_NAMES[alias]: cls for alias, cls in _header.structs.items()})     # Linear, LayerNorm, ...
_ERRORS = {v: k for k, v in _header.constants.items() if k.startswith("PIO_E_")}
# name -> (restype, argtypes), the parsed C types (see read_header) and the parameter names (py_name) of EVERY function of
# the header
SIGNATURES, DECLS = _header.signatures, _header.decls
PARAMS = {name: tuple(py_name(p) for _, p in params) for name, (_, params) in DECLS.items()}


def arguments(name: str, args, named) -> tuple:
    """The argument tuple of entry point `name` in the header's order, from leading positional `args` and `named` (a
    mapping, or (parameter, value) pairs).  PioError -- before anything is called -- for an unknown entry point or
    parameter, a parameter given twice or both ways, and a parameter left out."""
    if name not in PARAMS:
        raise PioError(f"{name}: not declared in {HEADER}")
    params, given = PARAMS[name], {}
    if len(args) > len(params):
        raise PioError(f"{name}: {len(args)} positional arguments for {len(params)} parameters")
    for k, v in named.items() if hasattr(named, "items") else named:
        if k not in params:
            raise PioError(f"{name}: no parameter {k!r} (the header has {', '.join(params)})")
        if k in given or k in params[:len(args)]:
            raise PioError(f"{name}: parameter {k!r} given twice")
        given[k] = v
    missing = [p for p in params[len(args):] if p not in given]
    if missing:
        raise PioError(f"{name}: missing {', '.join(missing)}")
    return tuple(args) + tuple(given[p] for p in params[len(args):])


_lib = None


def build(verbose: bool = False) -> str:
    """Compile libpio_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    out = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if verbose or out.returncode:
        print(out.stdout[-4000:])
        print(out.stderr[-4000:])
    if out.returncode:
        raise PioError("building libpio_hip.so failed")
    return LIB_PATH


def lib() -> C.CDLL:
    """The loaded library with argtypes set.  Raises loudly if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PioError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU / eager fallback for the PerceiverIO hot path)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)      # AttributeError => stale .so: fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(code: int, what: str = "") -> None:
    if code != PIO_OK:  # noqa: F821  (from the header)
        raise PioError(f"{what}: {_ERRORS.get(code, code)}")
