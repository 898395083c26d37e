"""CPU: the case table of the stale-workspace tests (tests/workspace_stale_cases.py) against the pure routing headers.

Every AttnCore of csrc/pio_attn_route.h, every SelfFold family and every plan struct of csrc/pio_block_route.h has a case,
and the route a case is LABELLED with is the one the headers return for its shape: the headers are compiled with g++ into
a small driver (as tests/test_attn_route.py and tests/test_block_route.py do), which carves the entry point's plan on a
fake base pointer -- never dereferenced -- states the call facts the way pio_blocks.hip does (adjacent carves included) and
prints attn_route / self_fold_route.  What the Python front end offers in a descriptor (stacked q|k / q|k|v images, the
K / V fold, the LayerNorm fold) is restated here from transformer_primitives.py; the GPU test's launch counts catch a
restatement that has gone stale."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workspace_stale_cases as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc")

DRIVER_HEAD = r'''
#include <stdio.h>
#include "pio_block_route.h"
using namespace pio;

static const char *name(AttnCore k) {
    switch (k) {
    case AttnCore::QKV_FLASH: return "QKV_FLASH";
    case AttnCore::KVFOLD_XATTN: return "KVFOLD_XATTN";
    case AttnCore::KVFOLD_XTALL: return "KVFOLD_XTALL";
    case AttnCore::PAIR_FLASH: return "PAIR_FLASH";
    case AttnCore::PAIR_XATTN: return "PAIR_XATTN";
    case AttnCore::FLASH: return "FLASH";
    case AttnCore::XATTN: return "XATTN";
    case AttnCore::XTALL: return "XTALL";
    case AttnCore::MATERIALISED: return "MATERIALISED";
    }
    return "?";
}
static const void *W = (const void *)(uintptr_t)0x10000000;   // fake, aligned, never dereferenced
static void *BASE = (void *)(uintptr_t)0x40000000;

// the descriptor as Attention._build_desc packs it; qk / qkv / kvf: which optional images it offers
static pio_attention_t attn(int heads, int dk, int dv, int act_split, int dtype, int q_in, int kv_in, int out, int qk,
                            int qkv, int qkv_lo, int kvf) {
    pio_attention_t a = {};
    a.heads = heads; a.dk = dk; a.dv = dv; a.dkp = pad8(dk); a.dvp = pad8(dv); a.dtype = dtype; a.act_split = act_split;
    a.q_in = q_in; a.k_in = a.v_in = kv_in; a.out = out;
    const int hdk = heads * a.dkp, ldo = heads * a.dvp;
    a.q.w_hi = a.k.w_hi = a.v.w_hi = a.o.w_hi = W;
    a.q.n = a.k.n = hdk; a.v.n = ldo; a.q.k = padc(q_in); a.k.k = a.v.k = padc(kv_in); a.o.k = ldo; a.o.n = pad8(out);
    if (qk) { a.qk.w_hi = W; a.qk.n = 2 * hdk; a.qk.k = padc(q_in); }
    if (qkv) { a.qkv.w_hi = W; a.qkv.n = 2 * hdk + ldo; a.qkv.k = padc(q_in); if (qkv_lo) { a.qkv.w_lo = W; a.qkv.lo_row0 = 2 * hdk; } }
    if (kvf) { a.kq.w_hi = a.vo.w_hi = W; a.kq.k = hdk; a.kq.n = a.vo.k = pad8(kv_in); a.vo.n = pad8(out); }
    return a;
}
static pio_mlp_t mlp(int c, int hidden, int dtype, int act_split) {
    pio_mlp_t m = {};
    m.in = m.out = c; m.hidden = hidden; m.dtype = dtype; m.act_split = act_split;
    m.fc1.w_hi = m.fc2.w_hi = W; m.fc1.k = padc(c); m.fc1.n = padc(hidden); m.fc2.k = m.fc1.n; m.fc2.n = padc(c);
    return m;
}
// attention_core's call facts on a carved scratch (pio_blocks.hip), then the route
static void route(const char *id, const pio_attention_t &a, const AttnScratch &w, AttnCall c) {
    const int64_t hdk = (int64_t)a.heads * a.dkp, ldo = (int64_t)a.heads * a.dvp, ld3 = 2 * hdk + ldo, tkv = round_up(c.Tk, 32);
    c.kv_fold_on = true;
    c.qkv_adjacent = (char *)w.q16.hi < (char *)w.k16.hi && (char *)w.k16.hi < (char *)w.vt16.hi &&
                     (size_t)((char *)w.vt16.hi - (char *)w.q16.hi) + (size_t)c.B * ldo * tkv * 2 >= (size_t)c.B * c.Tq * ld3 * 2;
    c.qk_adjacent = (char *)w.q16.hi + (size_t)c.B * c.Tq * hdk * 2 <= (char *)w.k16.hi;
    const AttnRoute r = attn_route(a, c);
    if (r.err) { printf("route %s error%d\n", id, r.err); return; }
    printf("route %s %s %d %d\n", id, name(r.core), r.fuse_qk, (int)(r.need_scores && !w.scores));
}
static AttnCall call(int B, int Bq, int Tq, int Tk, int same_qk, int same_kv, int kv, int q, int full, int bias, int probs,
                     int qcache) {
    AttnCall c = {};
    c.B = B; c.Bq = Bq; c.Tq = Tq; c.Tk = Tk; c.q_bcast = Bq != B; c.same_qk = same_qk; c.same_kv = same_kv;
    c.kv_mask = kv; c.q_mask = q; c.full_mask = full; c.bias = bias; c.probs = probs; c.qcache = qcache;
    return c;
}
static void attention_entry(const char *id, const pio_attention_t &a, AttnCall c) {
    AttentionPlan p;
    p.carve(BASE, a, c.B, c.Tq, c.Tk, c.q_bcast, c.same_kv);
    c.same_qk = false;  // pio_attention_fwd casts q and k into two carves
    route(id, a, p.core, c);
}
static void cross_entry(const char *id, const pio_attention_t &a, AttnCall c, int lean, int final_k) {
    pio_cross_attention_t ca = {};
    ca.attn = a; ca.mlp = mlp(a.q_in, a.q_in, a.dtype, a.act_split != 0);
    if (final_k >= 0) {  // a decoder; final_k: K of the final Linear's image (0: none)
        pio_linear_t fin = {};
        fin.w_hi = W; fin.k = final_k;
        DecoderPlan p;
        p.carve(BASE, ca, final_k ? &fin : nullptr, c.B, c.Tq, c.Tk, c.q_bcast);
        printf("y16 %s %d\n", id, (int)decoder_y16_direct(final_k ? &fin : nullptr, a.q_in));
        route(id, a, p.cp.core, c);
        return;
    }
    CrossPlan p;
    p.carve(BASE, ca, c.B, c.Tq, c.Tk, c.q_bcast, lean);
    route(id, a, p.core, c);
}
// fold_offered: SelfAttention._build_ln_fold packed the fold's images; ln_fold: pio_call_opts_t.ln_fold (the knobs
// as pio_blocks.hip derives them from it, process-wide setting 1, no environment)
static void self_entry(const char *id, const pio_attention_t &a, int B, int N, int fold_offered, int ln_fold, int lean) {
    pio_self_attention_t sa = {};
    const int C = a.q_in;
    sa.attn = a; sa.mlp = mlp(C, C, a.dtype, a.act_split != 0);
    if (fold_offered) {
        sa.fold.qkv.w_hi = sa.fold.fc1.w_hi = W;
        sa.fold.qkv.n = a.qkv.n; sa.fold.qkv.k = C; sa.fold.fc1.n = sa.mlp.fc1.n; sa.fold.fc1.k = C;
    }
    const int choice = ln_fold > 0 ? ln_fold - 1 : 1;
    const FoldKnobs knobs{choice, choice == 2 ? 2048 : 6144, choice == 2 ? 128 : 512, 4096};
    SelfPlan p;
    p.carve(BASE, sa, B, N, lean);
    SelfCall sc = {};
    sc.B = B; sc.N = N; sc.C = C; sc.stride_t = C; sc.stride_b = (int64_t)N * C; sc.x_aligned16 = true;
    sc.has_fold_buffers = p.x16b != nullptr;
    const SelfFold f = self_fold_route(sa, sc, knobs);
    printf("fold %s %s\n", id, f.family == SelfFold::NONE ? "NONE" : f.family == SelfFold::SMALL ? "SMALL" : "WIDE");
    AttnCall c = call(B, B, N, N, 1, 1, 0, 0, 0, 0, 0, 0);
    c.fold_in = c.fold_out = f.family != SelfFold::NONE;
    c.fold_qkv = c.fold_in ? &sa.fold.qkv : nullptr;
    route(id, a, p.core, c);
}
int main() {
'''


def _attn_expr(policy, H, qk, v, q_in, kv_in, out):
    """The C++ expression of the descriptor Attention._build_desc packs (transformer_primitives.py)."""
    from perceiverio_pytorch_amd import runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import FUSED_SELF_HEADS
    dtype, split = R.policy_dtype(policy)
    dk, dv = qk // H, v // H
    pad8 = lambda c: (c + 7) & ~7  # noqa: E731
    v_two = R.splits("proj_v", policy)
    kvf = H == 1 and dk == kv_in and dv == kv_in and R.kv_fold_offered(policy)
    has_qk = q_in == kv_in and not split
    has_qkv = (has_qk and R.qkv_stack_allowed(policy) and (pad8(dk), pad8(dv)) in FUSED_SELF_HEADS
               and (not v_two or (2 * H * pad8(dk)) % 256 == 0))
    return (f"attn({H}, {dk}, {dv}, {R.attention_act_split(policy)}, {dtype}, {q_in}, {kv_in}, {out}, {int(has_qk)}, "
            f"{int(has_qkv)}, {int(has_qkv and v_two)}, {int(kvf)})"), has_qkv


def _fold_offered(policy, C, has_qkv):
    """SelfAttention._build_ln_fold (widening factor 1 throughout the table)."""
    from perceiverio_pytorch_amd import runtime as R
    return not (not R.ln_fold_offered(policy) or C % 256 or not 512 <= C <= 1536 or not has_qkv)


def _lines(c):
    """The driver statements of one case: one per attention call, in the order of c["cores"]."""
    e, m = c["entry"], set(c.get("masks", ()))
    flags = lambda kv=0, q=0: f"{int(kv or 'kv' in m)}, {int(q or 'q' in m)}, {int('full' in m)}, {int('bias' in m)}, {int('probs' in m)}"  # noqa: E731
    B = c["B"]
    if e == "mlp_fwd":
        return []
    if e == "attention_fwd":
        a, _ = _attn_expr(c["policy"], c["H"], c["qk"], c["v"], c["q_in"], c["kv_in"], c["out"])
        Bq = 1 if c.get("q_bcast") else B
        return [f'attention_entry("{c["id"]}", {a}, call({B}, {Bq}, {c["Tq"]}, {c["Tk"]}, 0, {int(c["inputs"] != "three")}, '
                f'{flags()}, 0));']
    if e == "self_attention_fwd":
        a, has_qkv = _attn_expr(c["policy"], c["H"], c["C"], c["C"], c["C"], c["C"], c["C"])
        return [f'self_entry("{c["id"]}", {a}, {B}, {c["N"]}, {int(_fold_offered(c["policy"], c["C"], has_qkv))}, '
                f'{c["ln_fold"]}, 0);']
    if e == "cross_attention_fwd":
        a, _ = _attn_expr(c["policy"], c["H"], c["kv_in"], c["kv_in"], c["q_in"], c["kv_in"], c["q_in"])
        Bq = 1 if c.get("q_bcast") else B
        return [f'cross_entry("{c["id"]}", {a}, call({B}, {Bq}, {c["Tq"]}, {c["Tk"]}, 0, 1, {flags()}, 0), 0, -1);']
    if e.startswith("encoder"):
        a, _ = _attn_expr(c["policy"], 1, c["C_in"], c["C_in"], c["D"], c["C_in"], c["D"])
        s, has_qkv = _attn_expr(c["policy"], c["H"], c["D"], c["D"], c["D"], c["D"], c["D"])
        return [f'cross_entry("{c["id"]}", {a}, call({B}, 1, {c["N"]}, {c["M"]}, 0, 1, {flags(kv=c.get("input_mask"))}, 0), 1, -1);',
                f'self_entry("{c["id"]}", {s}, {B}, {c["N"]}, {int(_fold_offered(c["policy"], c["D"], has_qkv))}, '
                f'{c.get("ln_fold", 0)}, 1);']
    assert e.startswith("decoder"), e
    a, _ = _attn_expr(c["policy"], 1, c["D"], c["D"], c["Dq"], c["D"], c["Dq"])
    Bq = 1 if c.get("q_bcast") else B
    padc = lambda ch: (ch + 63) & ~63 if ch >= 256 else (ch + 7) & ~7  # noqa: E731
    return [f'cross_entry("{c["id"]}", {a}, call({B}, {Bq}, {c["Q"]}, {c["N"]}, 0, 1, {flags(q=c.get("query_mask"))}, '
            f'{int(bool(c.get("qcache")))}), 1, {padc(c["Dq"]) if c["final"] else 0});']


ALL = W.CASES + [W.SEQUENCE_FIRST]
_GOT = None


def _got():
    global _GOT
    if _GOT is None:
        body = "\n".join("    " + ln for c in ALL for ln in _lines(c))
        with tempfile.TemporaryDirectory() as d:
            src, exe = os.path.join(d, "stale.cpp"), os.path.join(d, "stale")
            open(src, "w").write(DRIVER_HEAD + body + "\n    return 0;\n}\n")
            subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                   src, "-o", exe])
            out = subprocess.check_output([exe]).decode().split("\n")
        _GOT = {"route": {}, "fold": {}, "y16": {}}
        for f in (ln.split() for ln in out if ln):
            _GOT[f[0]].setdefault(f[1], []).append(f[2:])
    return _GOT


def test_ids_are_unique_and_fields_present():
    ids = [c["id"] for c in ALL]
    assert len(ids) == len(set(ids))
    assert W.SEQUENCE_SECOND in W.BY_ID
    for c in ALL:
        assert len(c["launches"]) == 9 and all(isinstance(n, int) for n in c["launches"]), c["id"]
        assert all(core in W.ATTN_CORES for core in c["cores"]), c["id"]
        assert c["fold"] in W.FOLD_FAMILIES + (None,), c["id"]
        why = c.get("ragged") or c.get("no_ragged")
        assert isinstance(why, str) and len(why) > 10, f"{c['id']}: a ragged extent, or the reason there is none"


def test_every_attention_primitive_row_is_reused():
    import primitive_cases as PC
    assert {"ws_" + r[0] for r in PC.ATTN_WS_CASES} <= set(W.BY_ID)


def test_every_core_of_the_header_has_a_case():
    src = open(os.path.join(CSRC, "pio_attn_route.h")).read()
    body = re.search(r"enum class AttnCore \{(.*?)\};", src, re.S).group(1)
    cores = re.findall(r"^\s*([A-Z_]+),", body, re.M)
    assert sorted(cores) == sorted(W.ATTN_CORES), "AttnCore changed: extend workspace_stale_cases.ATTN_CORES and the cases"
    used = {core for c in W.CASES for core in c["cores"]}
    assert used == set(cores), set(cores) - used


def test_every_plan_and_fold_family_has_a_case():
    src = open(os.path.join(CSRC, "pio_block_route.h")).read()
    plans = re.findall(r"^struct (\w+Plan) \{", src, re.M)
    assert sorted(plans) == sorted(W.PLANS)
    assert {p for c in W.CASES for p in c["plan"].split("+")} == set(plans)
    fams = re.search(r"enum \{ (.*?) \} family;", src).group(1).split(", ")
    assert sorted(fams) == sorted(W.FOLD_FAMILIES)
    assert {c["fold"] for c in W.CASES if c["fold"]} == set(fams)


def test_labelled_routes_are_what_the_headers_return():
    got = _got()
    for c in ALL:
        routes = got["route"].get(c["id"], [])
        assert tuple(r[0] for r in routes) == tuple(c["cores"]), (c["id"], routes)
        assert all(r[2] == "0" for r in routes), f"{c['id']}: the plan carved no score buffers for a route that needs them"
        folds = got["fold"].get(c["id"], [])
        assert [f[0] for f in folds] == ([c["fold"]] if c["fold"] else []), (c["id"], folds)
    # the q|k form is out of reach of every entry point but the SelfAttention block's (see cross_same_input)
    assert all(r[1] == "0" for c in ALL for r in got["route"].get(c["id"], []))
    # every decoder case with a final Linear takes fc2's direct 16-bit rows (pitch padc(Dq) != Dq)
    for c in W.CASES:
        if c["entry"].startswith("decoder"):
            assert got["y16"][c["id"]] == [["1" if c["final"] else "0"]], c["id"]


def _fake_decoder(resid):
    """pio_cross_attention_t of the smallest decoder cases (Dq 60, D 44, one head) on fake, aligned pointers."""
    from perceiverio_pytorch_amd import _lib as L
    W_, Dq, D = 0x10000000, 60, 44
    pad8 = lambda c: (c + 7) & ~7  # noqa: E731
    ca = L.CrossAttention()
    a, m = ca.attn, ca.mlp
    a.heads, a.dk, a.dv, a.dkp, a.dvp = 1, D, D, pad8(D), pad8(D)
    a.q_in, a.k_in, a.v_in, a.out, a.dtype = Dq, D, D, Dq, L.PIO_DT_F16
    for lin, n, k in ((a.q, pad8(D), pad8(Dq)), (a.k, pad8(D), pad8(D)), (a.v, pad8(D), pad8(D)), (a.o, pad8(Dq), pad8(D)),
                      (m.fc1, pad8(Dq), pad8(Dq)), (m.fc2, pad8(Dq), pad8(Dq))):
        lin.w_hi, lin.n, lin.k = W_, n, k
    m.in_, m.hidden, m.out, m.dtype = Dq, Dq, Dq, L.PIO_DT_F16
    ca.use_query_residual = int(resid)
    return ca


def test_decoder_refuses_a_query_tail_with_a_cache_or_a_residual_before_any_launch():
    """pio_decoder_fwd: query_tail together with q16_hi -- which no entry point could express before the call record --
    and query_tail with use_query_residual are PIO_E_ARG, as is a NULL record.  Fake aligned pointers throughout: the
    refusals come before the first launch (a launch would read them), and the library loads without a device."""
    import ctypes as C
    from perceiverio_pytorch_amd import _lib as L
    lib = L.lib()
    B, Q, N, Dq, D, tail = 2, 33, 13, 60, 44, 6
    X, WS, Q16 = 0x20000000, 0x40000000, 0x30000000
    query = L.Tensor3(X, Q * (Dq - tail), Dq - tail, B, Q, Dq - tail)
    table = L.Tensor3(X + 0x100000, Q * tail, tail, 1, Q, tail)
    latents = L.Tensor3(X + 0x200000, N * D, D, B, N, D)
    stream = None
    for resid, q16_hi in ((0, Q16), (1, None)):
        ca = _fake_decoder(resid)
        need = lib.pio_decoder_workspace_bytes(ca, None, B, Q, N)
        assert need > 0
        rec = L.DecoderCall(C.pointer(ca), None, Dq, C.pointer(query), C.pointer(table), C.pointer(latents), None,
                            X + 0x300000, q16_hi, None, 0)
        assert lib.pio_decoder_fwd(C.byref(rec), WS, need, stream) == -6, (resid, q16_hi)       # PIO_E_ARG
        # (the record is otherwise in order: one byte less of workspace is what the call objects to first)
        assert lib.pio_decoder_fwd(C.byref(rec), WS, need - 1, stream) == -4                    # PIO_E_WORKSPACE
    assert lib.pio_decoder_fwd(None, WS, need, stream) == -6
    assert lib.pio_encoder_fwd(None, WS, need, stream) == -6
