"""CPU: pair-operand Q.K^T on the 128-wide head of the self-attention core -- the SELECTION of the raw-core cases the GPU
tests run (tests/qk_pair_wide_cases.py), done with the project's numerics model so that it can be reproduced without a
GPU, and the routing (perceiverio_pytorch_amd/csrc/pio_attn_route.h compiled with g++ into a small driver, as
tests/test_attn_route.py does)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import perceiver_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numerics_model as NM  # noqa: E402
import qk_pair_cases as QC  # noqa: E402
import qk_pair_wide_cases as WC  # noqa: E402

TOL = 1e-3          # the project's bar


@pytest.mark.parametrize("name", sorted(WC.CASES))
def test_case_selection_single_rounding_fails_pair_passes(name):
    """The rule of tests/test_qk_pair_host.py: the numpy emulation of the fused core against the float64 oracle, with q / k
    rounded once (above 2 TOL on at least one project figure) and as hi + fp16(residual) (below TOL / 2 on both), |s| <= 20.
    No case is exempt."""
    c = WC.CASES[name]
    q, k, v, ref, smax = WC.oracle(name)
    pts = ["q", "k", "v", "p", "o"]
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    one = NM.core(f64(q), f64(k), f64(v), c["H"], NM.Rounder("f16", pts), None)
    two = NM.core(f64(q), f64(k), f64(v), c["H"], NM.Rounder("f16", pts, pair=("q", "k")), None)
    e1, e2 = O.rel_errors(one, ref), O.rel_errors(two, ref)
    print(f"{name}: max|s|={smax:.2f} single {e1[0]:.3e} / {e1[1]:.3e}  pair {e2[0]:.3e} / {e2[1]:.3e}")
    assert smax <= 20.0
    assert max(e2) < TOL / 2, (name, e2)
    assert max(e1) > 2 * TOL, (name, e1)


def test_small_logit_variant_stays_below_one():
    """(a property of the test inputs: the GPU test's small-logit leg relies on it)"""
    for name in ("w128_256", "w128_200x300", "w128_1024"):
        assert WC.oracle(name, small=True)[4] <= 1.0


DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include "pio_attn_route.h"
using namespace pio;

static const char *name(AttnCore k) {
    switch (k) {
    case AttnCore::PAIR_FLASH: return "PAIR_FLASH";
    case AttnCore::PAIR_XATTN: return "PAIR_XATTN";
    case AttnCore::FLASH: return "FLASH";
    case AttnCore::XATTN: return "XATTN";
    case AttnCore::MATERIALISED: return "MATERIALISED";
    default: return "other";
    }
}
static const void *W = (const void *)(uintptr_t)0x10000000;   // a fake, aligned pointer: never dereferenced
static pio_attention_t attn(int heads, int dk, int dv, int act_split, int dtype = PIO_DT_F16) {
    pio_attention_t a = {};
    a.heads = heads; a.dk = dk; a.dv = dv; a.dkp = dk; a.dvp = dv; a.dtype = dtype; a.act_split = act_split;
    a.q_in = a.out = a.k_in = a.v_in = heads * dv;
    a.q.w_hi = a.k.w_hi = a.v.w_hi = a.o.w_hi = W;
    a.qk.w_hi = W; a.qk.n = 2 * heads * dk;
    a.qkv.w_hi = W; a.qkv.n = 2 * heads * dk + heads * dv;
    return a;
}
static void show(const char *id, const pio_attention_t &a, bool kv_mask) {
    AttnCall c = {};
    c.B = c.Bq = 2; c.Tq = c.Tk = 256; c.same_qk = c.same_kv = true; c.kv_fold_on = true;
    c.qkv_adjacent = c.qk_adjacent = true; c.kv_mask = kv_mask;
    const AttnRoute r = attn_route(a, c);
    const AttnRoute lean = attn_plan(a, 2, 2, 256, 256, true), cross = attn_plan(a, 2, 2, 256, 256, true, true);
    printf("route %s %d %s %d %d %d %d %d\n", id, r.err, name(r.core), r.qk_pair, r.out_pair, r.need_scores,
           lean.need_scores, cross.need_scores);
}
static void route(const char *id, char **argv, int i) {
    const int dkp = atoi(argv[i]), dvp = atoi(argv[i + 1]), B = atoi(argv[i + 2]), H = atoi(argv[i + 3]);
    const int Tq = atoi(argv[i + 4]), Tk = atoi(argv[i + 5]), vrow = atoi(argv[i + 6]);
    for (int ks = 0; ks < 2; ++ks) {
        const FlashRoute p = flash_pair_route(dkp, dvp, B, H, Tq, Tk, vrow, ks, 256);
        const FlashRoute f = flash_route(dkp, dvp, B, H, Tq, Tk, vrow, ks, 256);
        printf("flash %s/%d %d %d %d %d %d | %d %d %d %d %d\n", id, ks, p.v_rowmajor, p.NW, p.KS, p.nqt, p.threads,
               f.v_rowmajor, f.NW, f.KS, f.nqt, f.threads);
    }
}
int main(int argc, char **argv) {
    printf("supported %d %d %d %d %d\n", flash_pair_supported(PIO_DT_F16, 128, 128), flash_pair_supported(PIO_DT_F16, 64, 64),
           flash_pair_supported(PIO_DT_BF16, 128, 128), flash_pair_supported(PIO_DT_F16, 32, 160),
           xattn_pair_supported(PIO_DT_F16, 128, 128));
    show("plain_3", attn(8, 128, 128, 3), false);
    show("kv_mask_3", attn(8, 128, 128, 3), true);
    show("plain_2", attn(8, 128, 128, 2), false);
    show("kv_mask_2", attn(8, 128, 128, 2), true);
    show("plain_3_bf16", attn(8, 128, 128, 3, PIO_DT_BF16), false);
    show("plain_3_64", attn(8, 64, 64, 3), false);
    show("narrow_plain_3", attn(8, 32, 160, 3), false);
    show("narrow_kv_mask_3", attn(8, 32, 160, 3), true);
    for (int i = 1; i + 7 < argc; i += 8) route(argv[i], argv, i + 1);
    return 0;
}
'''

GOT = None


def _got():
    """Runs the driver once: the predicates, the attn_route lines and, for every raw-core case of both case files (passed
    on the command line: id dkp dvp B H Tq Tk vrow), flash_pair_route next to flash_route with the key split on and off."""
    global GOT
    if GOT is not None:
        return GOT
    argv = []
    for n, c in sorted(QC.CASES.items()):
        if c["core"] == "flash":
            argv += [n, QC.DK, c["dv"], c["B"], c["H"], c["Tq"], c["Tk"], int(bool(c.get("vrow")))]
    for n, c in sorted(WC.CASES.items()):
        argv += [n, WC.DK, WC.DV, c["B"], c["H"], c["Tq"], c["Tk"], int(c["vrow"])]
    inc = os.path.join(ROOT, "include")
    csrc = os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "route.cpp")
        open(src, "w").write(DRIVER)
        exe = os.path.join(d, "route")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", inc, "-I", csrc, src, "-o", exe])
        out = subprocess.check_output([exe] + [str(a) for a in argv]).decode().split("\n")
    got = {"supported": None, "route": {}, "flash": {}}
    for line in filter(None, out):
        f = line.split()
        if f[0] == "supported":
            got["supported"] = tuple(int(x) for x in f[1:])
        elif f[0] == "route":
            got["route"][f[1]] = tuple(int(x) if x.lstrip("-").isdigit() else x for x in f[2:])
        else:
            bar = f.index("|")
            got["flash"][f[1]] = (tuple(int(x) for x in f[2:bar]), tuple(int(x) for x in f[bar + 1:]))
    GOT = got
    return got


def test_pair_support_table():
    # (F16, 128, 128) yes; (F16, 64, 64) no; (BF16, 128, 128) no; the narrow head as before; no xattn pair core at 128
    assert _got()["supported"] == (1, 0, 0, 1, 0)


def test_attn_route_of_the_wide_pair_head():
    r = _got()["route"]
    # err, core, qk_pair, out_pair, need_scores | score buffers of the lean plan of a stack / of a cross-attend (which may
    # be called with mask vectors: the masked 128-wide pair request is MATERIALISED and needs them)
    assert r["plain_3"] == (0, "PAIR_FLASH", 1, 1, 0, 0, 1)
    assert r["kv_mask_3"] == (0, "MATERIALISED", 1, 1, 1, 0, 1)
    # act_split 2: as on the parent commit (single-operand cross-attention kernel on the hi halves, output pair)
    assert r["plain_2"] == (0, "XATTN", 0, 1, 0, 0, 0)
    assert r["kv_mask_2"] == (0, "XATTN", 0, 1, 0, 0, 0)
    # still without a pair core: materialised, never a single-operand run
    assert r["plain_3_bf16"] == (0, "MATERIALISED", 1, 1, 1, 1, 1)
    assert r["plain_3_64"] == (0, "MATERIALISED", 1, 1, 1, 1, 1)
    # the narrow heads: both families, as before
    assert r["narrow_plain_3"] == (0, "PAIR_FLASH", 1, 1, 0, 0, 0)
    assert r["narrow_kv_mask_3"] == (0, "PAIR_XATTN", 1, 1, 0, 0, 0)


def test_flash_pair_route():
    f = _got()["flash"]
    narrow = [n for n, c in QC.CASES.items() if c["core"] == "flash"]
    assert len(narrow) >= 11
    for n in narrow:                                   # dkp = 32: exactly flash_route
        for ks in (0, 1):
            pair, single = f[f"{n}/{ks}"]
            assert pair == single, n
    assert f["self_rm_ks2/1"][0][1:3] == (8, 2) and f["self32_rm_ks4/1"][0][1:3] == (16, 4)   # (the table has the splits)
    for n, c in WC.CASES.items():                      # dkp = 128: never a key split; 8 waves under the "wide" rule
        for ks in (0, 1):
            pair, single = f[f"{n}/{ks}"]
            rows = 256 if c["NW"] == 8 else 128
            assert pair == (int(c["vrow"]), c["NW"], c["KS"], (c["Tq"] + rows - 1) // rows, 64 * c["NW"]), (n, pair)
            assert pair[3] == single[3], n             # the same query tiling as the single-operand launch
    assert f["w128_rm_256/1"][1][1:3] == (8, 2)        # the single-operand route splits the keys here
    assert f["w128_rm_nw8/1"][1][1:3] == (8, 1)
