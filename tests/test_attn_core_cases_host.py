"""CPU: the cases of tests/attn_core_cases.py mean what they claim -- the float64 reference agrees with the oracle's
`attend` and with torch, the planted probe really isolates one key per row, every case detects every fault that applies to
it (a fault moves some element by more than 8 times the bound the GPU test asserts), and every case reaches the kernel
branch it is labelled with (csrc/pio_attn_route.h compiled with g++, as tests/test_attn_route.py does)."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import perceiver_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_core_cases as AC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c["id"] for c in AC.CASES]
_cache = {}


def probes(c):
    """{probe: (operands, reference)} of the case's first dtype, computed once."""
    if c["id"] not in _cache:
        out = {}
        for pr in AC.PROBES:
            d = AC.make(c, pr, c["dts"][0])
            if d is not None:
                out[pr] = (d, AC.reference(d))
        _cache.clear()                              # (one case at a time: the big ones hold tens of MB)
        _cache[c["id"]] = out
    return _cache[c["id"]]


def _mask3(d, B, Tq, Tk):
    if d["km"] is None and d["qm"] is None:
        return None
    km = d["km"] if d["km"] is not None else np.ones((B, Tk), bool)
    qm = d["qm"] if d["qm"] is not None else np.ones((B, Tq), bool)
    return O.make_cross_attention_mask(qm, km)


@pytest.mark.parametrize("cid", IDS)
def test_reference_equals_oracle_and_torch(cid):
    c = AC.BY_ID[cid]
    B, Tq, Tk, dk = c["B"], c["Tq"], c["Tk"], c["dk"]
    for pr, (d, ref) in probes(c).items():
        qh = np.broadcast_to(d["qh"], (B,) + d["qh"].shape[1:])[..., :dk]
        kh = d["kh"][..., :dk]
        if d["ql"] is None:
            q, k = qh, kh
        else:   # S = Q_hi K_hi + Q_lo K_hi + Q_hi K_lo as ONE product over 3 dk channels (the oracle scales by sqrt(3 dk))
            ql = np.broadcast_to(d["ql"], qh.shape[:3] + (d["ql"].shape[-1],))[..., :dk]
            q = np.concatenate([qh, ql, qh], axis=-1) * math.sqrt(3.0)
            k = np.concatenate([kh, kh, d["kl"][..., :dk]], axis=-1)
        m3 = _mask3(d, B, Tq, Tk)
        want = O.attend(q, k, d["v"], m3).reshape(ref.shape)
        scale = max(np.abs(d["v"]).max(), 1.0)
        assert np.abs(ref - want).max() <= 1e-12 * scale, (cid, pr, "oracle")
        tq, tk, tv = (torch.from_numpy(np.array(x)).permute(0, 2, 1, 3) for x in (q, k, d["v"]))
        s = tq @ tk.transpose(-1, -2) / math.sqrt(q.shape[-1])
        if m3 is not None:
            s = s.masked_fill(~torch.from_numpy(m3)[:, None], -1e30)
        got = (torch.softmax(s, dim=-1) @ tv).permute(0, 2, 1, 3)
        if m3 is not None:
            got = got.masked_fill(~torch.from_numpy(m3).any(dim=2)[:, :, None, None], 0.0)
        assert got.dtype == torch.float64
        assert np.abs(ref - got.numpy()).max() <= 1e-12 * scale, (cid, pr, "torch")
        online = AC.reference_online(d, AC.KEY_TILE[c["kern"]])
        assert np.abs(ref - online).max() <= 1e-12 * scale, (cid, pr, "online form")


@pytest.mark.parametrize("cid", IDS)
def test_planted_rows_isolate_their_target(cid):
    """The target leads every other attendable key by >= 16 nats, |s| <= 30, the row is V[target] to exp(-16) Tk; and the
    staircases step by >= 8 nats per key tile."""
    c = AC.BY_ID[cid]
    B, H, Tq, Tk = c["B"], c["H"], c["Tq"], c["Tk"]
    d, ref = probes(c)["planted"]
    s = AC.logits(d)
    live = np.isfinite(s).any(axis=-1)
    if d["qm"] is not None:
        live &= d["qm"][:, None, :]
    assert np.abs(s[np.isfinite(s)]).max() <= 30.0
    t = d["targets"]
    seen = set()
    for b in range(B):
        for h in range(H):
            for i in range(Tq):
                if not live[b, h, i]:
                    assert (ref[b, i, h] == 0).all()
                    continue
                row = s[b, h, i].copy()
                top = row[t[b, h, i]]
                row[t[b, h, i]] = -np.inf
                assert top - row.max() >= 16.0, (cid, b, h, i, top, row.max())
                assert np.abs(ref[b, i, h] - d["v"][b, t[b, h, i], h]).max() <= 2 * Tk * math.exp(-16.0)
                seen.add(int(t[b, h, i]))
    if live.any():
        assert seen, cid
    if Tq > 1:      # every edge of every sample is some row's target (a target list cut short is rejected, not kept)
        for b in range(B):
            att = d["km"][b] if d["km"] is not None else np.ones(Tk, bool)
            want = set(AC.edges(c, att))
            for a, e in AC.key_parts(c):
                own = np.flatnonzero(att[a:e]) + a
                assert own.size == 0 or {int(own[0]), int(own[-1])} <= want, (cid, b, a, e)
            have = {int(k) for k in t[b].ravel() if k >= 0}
            assert want <= have, (cid, b, sorted(want - have))
    for pr in ("stair_up", "stair_down", "stair_up_masked_lead"):
        if pr not in probes(c):
            continue
        ds = probes(c)[pr][0]
        s = AC.logits(ds)
        kt = AC.KEY_TILE[c["kern"]]
        for b in range(B):                          # over the tiles of a sample that hold an attendable key, in order
            sb = s[b]
            tiles = [sb[..., a:a + kt] for a in range(0, Tk, kt) if np.isfinite(sb[..., a:a + kt]).any()]
            tmax = [t.max(axis=-1) for t in tiles]
            tmin = [np.where(np.isfinite(t), t, np.inf).min(axis=-1) for t in tiles]
            for a in range(len(tiles) - 1):
                lo, hi = (a, a + 1) if pr != "stair_down" else (a + 1, a)
                assert (tmin[hi] - tmax[lo] >= 8.0).all(), (cid, pr, b, a)


@pytest.mark.parametrize("cid", IDS)
def test_every_case_has_teeth(cid):
    """Each fault that applies moves at least one element of at least one probe by more than 8 x the asserted bound (the
    widest one the case is run with: its last dtype)."""
    c = AC.BY_ID[cid]
    dt = c["dts"][-1]
    applied = 0
    for fault in AC.FAULTS:
        worst, applies = 0.0, False
        for pr, (d, ref) in probes(c).items():
            bad = AC.faulty(c, d, fault)
            if bad is None:
                continue
            applies = True
            bnd = AC.bound(dt, c["Tk"], np.maximum(AC.vmax_of(d), 2.0 ** -7))
            worst = max(worst, float((np.abs(bad - ref) / bnd).max()))
            if worst > 8.0:
                break
        if applies:
            applied += 1
            assert worst > 8.0, f"{cid}: fault {fault} would pass ({worst:.2f} x bound)"
    assert applied >= 3, cid


# ---- branch labels -------------------------------------------------------------------------------------------------
DRIVER_HEAD = r'''
#include <stdio.h>
#include "pio_attn_route.h"
using namespace pio;
static void flash(const char *id, int dkp, int dvp, int B, int H, int Tq, int Tk, int vrow) {
    const FlashRoute r = flash_route(dkp, dvp, B, H, Tq, Tk, vrow != 0, true, 256);
    printf("%s %d %d\n", id, r.NW, r.KS);
}
static void xattn(const char *id, int dkp, int dvp, int B, int H, int Tq, int Tk) {
    const XCfg *c = xattn_cfg(dkp, dvp);
    const int ns = xattn_splits(dkp, dvp, B, H, Tq, Tk), nt = (Tk + 31) / 32, tps = (nt + ns - 1) / ns;
    int empty = 0;
    for (int s = 0; s < ns; ++s) empty += s * tps >= nt;
    printf("%s %d %d %d %d %d\n", id, c ? c->dkl : 0, c ? c->dvs : 0, c ? (dvp + c->dvs - 1) / c->dvs : 0, ns, empty);
}
static void xtall(const char *id, int dkp, int dvp, int Tk) {
    printf("%s %d %d\n", id, (int)xtall_supported(dkp, dvp, Tk), (int)xattn_supported(dkp, dvp));
}
int main() {
    printf("refuse513 %d %d\n", (int)xtall_supported(1024, 1024, 513), 0);
'''


def test_branch_labels_are_true():
    body = []
    for c in AC.CASES:
        a = (c["id"], c["dkp"], c["dvp"], c["B"], c["H"], c["Tq"], c["Tk"])
        if c["kern"] == "flash":
            body.append('    flash("%s", %d, %d, %d, %d, %d, %d, %d);' % (a + (int(c["vrow"]),)))
        elif c["kern"] == "xattn":
            body.append('    xattn("%s", %d, %d, %d, %d, %d, %d);' % a)
        else:
            body.append('    xtall("%s", %d, %d, %d);' % (c["id"], c["dkp"], c["dvp"], c["Tk"]))
    src_text = DRIVER_HEAD + "\n".join(body) + "\n    return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "labels.cpp"), os.path.join(d, "labels")
        open(src, "w").write(src_text)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                               os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc"), src, "-o", exe])
        got = {f[0]: tuple(int(x) for x in f[1:]) for f in
               (line.split() for line in subprocess.check_output([exe]).decode().splitlines() if line)}
    assert got.pop("refuse513") == (0, 0)
    for c in AC.CASES:
        g = got[c["id"]]
        if c["kern"] == "xattn":
            empty = 1 if c["id"] == "xattn_split10_empty_split_tk2575" else 0
            assert g == tuple(c["label"]) + (empty,), (c["id"], g)
            assert len(AC.key_parts(c)) == c["label"][3] - empty
        else:
            assert g == tuple(c["label"]), (c["id"], g)
    # every instantiation and route the issue names is reached by some case
    assert {c["label"] for c in AC.CASES if c["kern"] == "flash"} == {(4, 1), (8, 1), (8, 2), (16, 4)}
    assert {c["label"][:2] for c in AC.CASES if c["kern"] == "xattn"} == {(32, 96), (32, 160), (128, 128), (352, 352),
                                                                          (512, 512), (704, 256)}
    assert {(c["dkp"], c["dvp"]) for c in AC.CASES if c["kern"] == "flash"} == {(128, 128), (64, 64), (32, 32), (32, 160)}
    assert {(c["dkp"], c["dvp"]) for c in AC.CASES if c["kern"] == "xtall"} == {(64, 256), (64, 768), (736, 512), (1024, 1024)}
