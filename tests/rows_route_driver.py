"""perceiverio_pytorch_amd/csrc/pio_rows_route.h compiled with g++ into a small driver that answers calls read from its
standard input: which kernel a pio_layernorm_cast / pio_softmax_rows call goes to, or the error code of a refused call.
Shared by tests/test_rows_route.py and tests/test_primitive_cases_host.py; the calls of the case tables of
tests/primitive_cases.py are built here exactly as tests/test_primitives_gpu.py places the buffers (every allocation
16-byte aligned, x / S shifted by the case's x_off / s_off floats)."""
import atexit
import os
import shutil
import subprocess
import tempfile

import primitive_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc", "pio_rows_route.h")

DRIVER = r'''
#include <stdio.h>
#include <string.h>
#include "pio_rows_route.h"
using namespace pio;

static int dtype_of(const char *s) { return !strcmp(s, "f16") ? PIO_DT_F16 : !strcmp(s, "bf16") ? PIO_DT_BF16 : 99; }
static const char *err_name(int e) {
    return e == PIO_E_SHAPE ? "PIO_E_SHAPE" : e == PIO_E_ALIGN ? "PIO_E_ALIGN" : e == PIO_E_ARG ? "PIO_E_ARG" : "error";
}

int main() {
    char what[8], id[128], dt[8];
    while (scanf("%7s %127s %7s", what, id, dt) == 3) {
        if (!strcmp(what, "ln")) {
            LnCall c = {};
            long long sb, st;
            int has_ln;
            if (scanf("%d %d %d %d %lld %lld %d %u %u %u %u %u", &c.B, &c.T, &c.C, &c.c_pad, &sb, &st, &has_ln, &c.x, &c.y,
                      &c.y_lo, &c.gamma, &c.beta) != 12) return 2;
            c.stride_b = sb; c.stride_t = st; c.has_ln = has_ln != 0; c.dtype = dtype_of(dt);
            const LnRoute r = ln_route(c);
            if (r.err) printf("%s %s\n", id, err_name(r.err));
            else if (r.kind == LnKind::REG4) printf("%s reg_nv%d %u %d\n", id, r.nv, r.blocks, (int)r.even_rows);
            else printf("%s %s %u %d\n", id, r.kind == LnKind::REG2 ? "reg2" : r.kind == LnKind::GEN_VEC ? "gen_vec" : "gen_scalar",
                        r.blocks, (int)r.even_rows);
        } else if (!strcmp(what, "cat")) {
            LnCatCall c = {};
            long long s[4];
            if (scanf("%d %d %d %d %d %d %d %d %lld %lld %lld %lld %u %u %u %u %u %u", &c.B1, &c.T1, &c.C1, &c.B2, &c.T2, &c.C2,
                      &c.ln_c, &c.c_pad, &s[0], &s[1], &s[2], &s[3], &c.x1, &c.x2, &c.y, &c.y_lo, &c.gamma, &c.beta) != 18)
                return 2;
            c.sb1 = s[0]; c.st1 = s[1]; c.sb2 = s[2]; c.st2 = s[3]; c.dtype = dtype_of(dt);
            const int e = ln_cat_check(c);
            printf("%s %s\n", id, e ? err_name(e) : "cat2");
        } else if (!strcmp(what, "sm")) {
            SoftmaxCall c = {};
            long long lds, ldp;
            int has[6];
            if (scanf("%d %d %d %d %lld %lld %d %d %d %d %d %d %u %u %u %u %u %u %u", &c.B, &c.H, &c.Tq, &c.Tk, &lds, &ldp,
                      &has[0], &has[1], &has[2], &has[3], &has[4], &has[5], &c.S, &c.P, &c.P_lo, &c.bias, &c.probs,
                      &c.kv_mask, &c.full_mask) != 19) return 2;
            c.lds = lds; c.ldp = ldp; c.dtype = dtype_of(dt);
            c.has_P_lo = has[0]; c.has_bias = has[1]; c.has_probs = has[2];
            c.has_kv_mask = has[3]; c.has_q_mask = has[4]; c.has_full_mask = has[5];
            const SoftmaxRoute r = softmax_route(c);
            if (r.err) printf("%s %s\n", id, err_name(r.err));
            else if (r.kind == SoftmaxKind::REG) printf("%s reg_nv%d_%s %u\n", id, r.nv4, r.plain ? "plain" : "masked", r.blocks);
            else printf("%s %s %u\n", id, r.kind == SoftmaxKind::GEN_W1 ? "gen_w1" : "gen_w4", r.blocks);
        } else {
            return 2;
        }
    }
    return 0;
}
'''

_exe = None


def _driver():
    global _exe
    if _exe is None:
        d = tempfile.mkdtemp(prefix="rows_route_")
        atexit.register(shutil.rmtree, d, True)
        src = os.path.join(d, "rows_route.cpp")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                               os.path.dirname(HEADER), src, "-o", os.path.join(d, "rows_route")])
        _exe = os.path.join(d, "rows_route")
    return _exe


def ask(calls):
    """calls: lines "ln|cat|sm <id> <dtype> <numbers ...>" (ln_call / cat_call / sm_call) -> {id: answer fields}: the kernel's
    label and its workgroups (layernorm_cast: and even_rows), or the error code's name."""
    out = subprocess.run([_driver()], input="\n".join(calls) + "\n", capture_output=True, text=True, check=True).stdout
    got = {}
    for line in filter(None, out.split("\n")):
        f = line.split()
        got[f[0]] = f[1] if len(f) == 2 else (f[1],) + tuple(int(v) for v in f[2:])
    assert len(got) == len(calls), "ids must be distinct and every call answered"
    return got


def ln_call(name, dt, B, T, C, c_pad, sb, st, has_ln=True, x=0, y=0, y_lo=0, gamma=0, beta=0):
    return f"ln {name} {dt} {B} {T} {C} {c_pad} {sb} {st} {int(has_ln)} {x} {y} {y_lo} {gamma} {beta}"


def cat_call(name, dt, B1, T1, C1, B2, T2, C2, ln_c, c_pad, sb1, st1, sb2, st2, x1=0, x2=0, y=0, y_lo=0, gamma=0, beta=0):
    return (f"cat {name} {dt} {B1} {T1} {C1} {B2} {T2} {C2} {ln_c} {c_pad} {sb1} {st1} {sb2} {st2} {x1} {x2} {y} {y_lo} "
            f"{gamma} {beta}")


def sm_call(name, dt, B, H, Tq, Tk, lds, ldp, full=False, S=0, P=0, P_lo=0, bias=0, probs=0, kv_mask=0, full_mask=0):
    """full: kv_mask, q_mask, full_mask, bias and P_lo present (primitive_cases.SM_FORMS); never a probability output."""
    has = f"{int(full)} {int(full)} 0 {int(full)} {int(full)} {int(full)}"
    return f"sm {name} {dt} {B} {H} {Tq} {Tk} {lds} {ldp} {has} {S} {P} {P_lo} {bias} {probs} {kv_mask} {full_mask}"


def ln_case_call(name, case, layout, dt="f16", has_ln=True):
    sb, st, _ = PC.ln_strides(case, layout)
    return ln_call(name, dt, PC.LN_B, PC.LN_T, case["C"], case["c_pad"], sb, st, has_ln, x=(4 * case["x_off"]) & 15)


def sm_case_call(name, case, form, dt="f16"):
    return sm_call(name, dt, PC.SM_B, PC.SM_H, PC.SM_TQ, case["Tk"], case["lds"], case["ldp"], full=(form == "full"),
                   S=(4 * case["s_off"]) & 15)


def ln_variants():
    """{(case id, layout): kernel label} of every LAYERNORM_CASES x LN_LAYOUTS call."""
    keys = [(c, layout) for c in PC.LAYERNORM_CASES for layout in PC.LN_LAYOUTS]
    got = ask([ln_case_call(f"{c['id']}/{layout}", c, layout) for c, layout in keys])
    return {(c["id"], layout): got[f"{c['id']}/{layout}"][0] for c, layout in keys}


def softmax_variants():
    """{(case id, form): kernel label} of every SOFTMAX_CASES x SM_FORMS call."""
    keys = [(c, form) for c in PC.SOFTMAX_CASES for form in PC.SM_FORMS]
    got = ask([sm_case_call(f"{c['id']}/{form}", c, form) for c, form in keys])
    return {(c["id"], form): got[f"{c['id']}/{form}"][0] for c, form in keys}
