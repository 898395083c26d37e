"""CPU: the cases of tests/kv_fold_cases.py (the K / V-projection fold as a composition).

1. the reference against torch float64 of the un-folded formula and against the folded algebra;
2. the reference pushed through a numpy model of the cores' documented roundings stays inside the bound, folded and un-folded;
3. the faults the composition can have (a scale of sqrt(kvp), a dropped Wo bv, a lost last key, a batch stride that is wrong
   under batch-invariant queries) each move some element of at least one case and probe by more than FAULT_MARGIN = 8
   times the folded run's bound -- the GPU test lets the kernel use one bound, so such a fault cannot pass it (printed: which);
4. every case carries the route csrc/pio_attn_route.h gives it (a small driver compiled with g++, as tests/test_attn_route.py)."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_fold_cases as KC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c["id"] for c in KC.CASES]


def _probes(c, dt):
    for probe in KC.PROBES:
        d = KC.make(c, probe, dt)
        if d is not None:
            yield probe, d


@pytest.mark.parametrize("case", KC.CASES, ids=IDS)
def test_reference_and_bound(case):
    c = case
    for policy in c["policies"]:
        dt, pair = KC.DT_OF[policy], policy == "fp16x2af"
        n = 0
        for probe, d in _probes(c, dt):
            n += 1
            ref = KC.reference(c, d)
            t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items() if isinstance(v, np.ndarray)}
            xq = t["xq"].expand(c["B"], -1, -1)
            q = xq @ t["Wq"].T + t["bq"]
            k = t["x"] @ t["Wk"].T + t["bk"]
            v = t["x"] @ t["Wv"].T + t["bv"]
            p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(c["k_in"]), dim=-1)
            tor = ((p @ v) @ t["Wo"].T + t["bo"]).numpy()
            assert np.abs(tor - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (c["id"], probe)
            # the fold's algebra, in float64
            s = (q.numpy() @ d["Wk"]) @ d["x"].transpose(0, 2, 1) / math.sqrt(c["k_in"])
            e = np.exp(s - s.max(axis=-1, keepdims=True))
            alg = ((e / e.sum(axis=-1, keepdims=True)) @ d["x"]) @ (d["Wo"] @ d["Wv"]).T + (d["Wo"] @ d["bv"] + d["bo"])
            assert np.abs(alg - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max()), (c["id"], probe)
            for folded in (True, False):
                bound = KC.bound(c, d, dt, pair, folded)
                err = np.abs(KC.rounded_model(c, d, dt, pair, folded) - ref)
                assert (err <= bound).all(), (c["id"], policy, probe, folded, float((err / bound).max()))
            if probe == "planted":      # the output is the target key's row through the projections
                tg = d["targets"][:, 0]
                for b in range(c["B"]):
                    want = (d["x"][b, tg[b]] @ d["Wv"].T + d["bv"]) @ d["Wo"].T + d["bo"]
                    assert np.abs(ref[b] - want).max() <= 1e-5
            # masked: a sample without attendable key is final.bias; every other sample keeps attendable keys
            km = KC.key_mask(c)
            rm = KC.reference(c, d, km)
            assert km[0].any() and not km[0].all() and (c["B"] == 1 or not km[c["B"] - 1].any())
            if c["B"] > 1:
                assert np.array_equal(rm[c["B"] - 1], np.broadcast_to(d["bo"], rm[c["B"] - 1].shape))
            assert not np.array_equal(rm[0], ref[0]) or probe == "planted"
        assert n >= 3, c["id"]


@pytest.mark.parametrize("fault", KC.FAULTS)
def test_fault_is_rejected(fault):
    caught = []
    for c in KC.CASES:
        if not c["fold"]:
            continue
        policy = c["policies"][0]
        dt, pair = KC.DT_OF[policy], policy == "fp16x2af"
        for probe, d in _probes(c, dt):
            err = np.abs(KC.reference(c, d, fault=fault) - KC.reference(c, d))
            ratio = float((err / KC.bound(c, d, dt, pair, True)).max())
            if ratio > KC.FAULT_MARGIN:
                caught.append(f"{c['id']}/{probe} ({ratio:.0f}x)")
    print(f"K/V-fold fault {fault}: more than {KC.FAULT_MARGIN:.0f} bounds on {caught}")
    assert caught, f"no case rejects {fault}"
    if fault in ("scale_kvp", "bstride_bq1"):
        assert any(x.startswith("k322_b2_bq1/") for x in caught), "the 322-channel case must catch it"


# ---- 4. routes -------------------------------------------------------------------------------------------------------
DRIVER_HEAD = r'''
#include <stdio.h>
#include "pio_attn_route.h"
using namespace pio;
static const char *name(AttnCore k) {
    switch (k) {
    case AttnCore::KVFOLD_XATTN: return "KVFOLD_XATTN";
    case AttnCore::KVFOLD_XTALL: return "KVFOLD_XTALL";
    case AttnCore::XATTN: return "XATTN";
    case AttnCore::XTALL: return "XTALL";
    default: return "OTHER";
    }
}
static const void *W = (const void *)(uintptr_t)0x10000000;   // a fake, aligned pointer: never dereferenced
static void show(const char *id, int c, int act_split, int B, int Bq, int Tq, int Tk, int masked, int fold_on) {
    pio_attention_t a = {};
    const int p = (c + 7) & ~7;
    a.heads = 1; a.dk = a.dv = c; a.dkp = a.dvp = p; a.dtype = PIO_DT_F16; a.act_split = act_split;
    a.q_in = a.k_in = a.v_in = c; a.out = 24;
    a.q.w_hi = a.k.w_hi = a.v.w_hi = a.o.w_hi = a.kq.w_hi = a.vo.w_hi = W;
    a.kq.k = p; a.kq.n = a.vo.k = p;
    AttnCall call = {};
    call.B = B; call.Bq = Bq; call.Tq = Tq; call.Tk = Tk; call.q_bcast = Bq == 1 && B > 1; call.same_kv = true;
    call.kv_fold_on = fold_on; call.kv_mask = masked; call.qk_adjacent = true;
    const AttnRoute r = attn_route(a, call);
    const XCfg *x = xattn_cfg(p, p);
    const bool tall = r.core == AttnCore::KVFOLD_XTALL || r.core == AttnCore::XTALL;
    printf("%s %s %d %d %d %d %d %d\n", id, name(r.core), tall || !x ? 0 : x->dkl, tall || !x ? 0 : x->dvs,
           tall || !x ? 1 : (p + x->dvs - 1) / x->dvs, tall ? 1 : xattn_splits(p, p, B, 1, Tq, Tk), r.out_pair, r.need_scores);
}
int main() {
'''


def _routes():
    lines = []
    for c in KC.CASES:
        for policy in c["policies"]:
            a = 2 if policy == "fp16x2af" else 0
            for tag, masked, on in (("fold", 0, 1), ("off", 0, 0), ("mask", 1, 1)):
                lines.append(f'    show("{c["id"]}|{policy}|{tag}", {c["k_in"]}, {a}, {c["B"]}, {c["Bq"]}, {c["Tq"]}, {c["Tk"]}, {masked}, {on});')
    e = KC.BY_ID[KC.SPLIT_EDGE[0]]
    lines.append(f'    show("edge|fp16|fold", {e["k_in"]}, 0, {e["B"]}, {e["Bq"]}, {e["Tq"]}, {KC.SPLIT_EDGE[1]}, 0, 1);')
    src = DRIVER_HEAD + "\n".join(lines) + "\n    return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        path, exe = os.path.join(d, "kvroute.cpp"), os.path.join(d, "kvroute")
        open(path, "w").write(src)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                               os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc"), path, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    got = {}
    for line in filter(None, out):
        f = line.split()
        got[f[0]] = (f[1],) + tuple(int(v) for v in f[2:])
    return got


def test_every_case_carries_its_route():
    got = _routes()
    for c in KC.CASES:
        for policy in c["policies"]:
            pair = int(policy == "fp16x2af")
            core, dkl, dvs, slices, splits, out_pair, scores = got[f"{c['id']}|{policy}|fold"]
            cfg = c["cfg"] or (0, 0)
            assert (core, (dkl, dvs), slices, splits) == (c["core"], cfg, c["slices"], c["splits"]), (c["id"], got[f"{c['id']}|{policy}|fold"])
            assert (core.startswith("KVFOLD")) == c["fold"] and out_pair == pair and scores == 0, c["id"]
            for tag in ("off", "mask"):      # the switch and a key mask leave the un-folded fused core of the same family
                ucore = got[f"{c['id']}|{policy}|{tag}"]
                assert ucore[0] == c["core"].replace("KVFOLD_", "") and ucore[6] == 0, (c["id"], tag, ucore)
    assert got["edge|fp16|fold"][4] == 1 and KC.BY_ID[KC.SPLIT_EDGE[0]]["splits"] == 2, "the split case is the smallest Tk that splits"
    assert (KC.BY_ID["k104_tk131_below"]["B"] * 131 < 4 * 33 <= KC.BY_ID["k104_tk132_at"]["B"] * 132)
    cores = {c["core"] for c in KC.CASES}
    assert {"KVFOLD_XATTN", "KVFOLD_XTALL"} <= cores
    assert {c["cfg"] for c in KC.CASES if c["cfg"]} == {(32, 96), (128, 128), (352, 352), (512, 512), (704, 256)}
