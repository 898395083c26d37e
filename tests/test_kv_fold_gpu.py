"""GPU: the K / V-projection fold of a single-head cross-attend as a composition -- pio_attention_fwd on descriptors built by
transformer_primitives.Attention, at the cases and exact operands of tests/kv_fold_cases.py.

Each case and probe runs three ways, every time on a fresh workspace of exactly the promised bytes between guards, poisoned
as tests/test_workspace_stale_gpu.py poisons it (0x7B: finite and huge; the folded run also on 0xFF: NaN everywhere, bit-identical):
  1. folded;  2. with PIO_KV_FOLD=0;  3. with a key mask, where the fold must step aside.
(1) and (2) each meet their derived bound (kv_fold_cases.bound: the values the run's own core reads) against the float64
reference of the UN-FOLDED formula; (3) is bit-identical to the same call with PIO_KV_FOLD=0 and meets the bound of the masked
reference on a scattered key mask; where a case has two samples the last has no attendable key and equals final.bias exactly.  Engagement is read from the profiler's launch accounting: the folded run launches
three GEMMs (Q, Q Wk, Wo Wv) and one fused core, the un-folded run four (Q, K, V^T, Wo) and one fused core; neither a softmax."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_fold_cases as KC  # noqa: E402
from test_primitives_gpu import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

GEMM_CLASSES = (0, 1, 6, 7, 8)
worst_ratio = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256, "the key-split labels are those of 256 CUs"
    yield torch.device("cuda:0")
    for k, v in worst_ratio.items():
        print(f"K/V fold {k}: worst |out - ref| / bound = folded {v[0]:.3f}, un-folded {v[1]:.3f}")


def _module(c, d, dev):
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    k = c["k_in"]
    m = Attention(k, k, k, num_heads=1, qk_out_channels=k, v_out_channels=k, output_channels=KC.OUT)
    sd = {"proj_q.weight": d["Wq"], "proj_q.bias": d["bq"], "proj_k.weight": d["Wk"], "proj_k.bias": d["bk"],
          "proj_v.weight": d["Wv"], "proj_v.bias": d["bv"], "final.weight": d["Wo"], "final.bias": d["bo"]}
    m.load_state_dict({n: torch.from_numpy(np.ascontiguousarray(a, np.float32)) for n, a in sd.items()})
    for n, a in sd.items():
        assert np.array_equal(np.asarray(a, np.float32).astype(np.float64), a), n
    return m.to(dev).eval()


def _run(dev, desc, c, xq, xkv, km, fill):
    """One pio_attention_fwd on a poisoned workspace of exactly the promised size -> (out, launches per profiler class)."""
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    lib = L.lib()
    B, Tq, Tk = c["B"], c["Tq"], c["Tk"]
    need = lib.pio_attention_workspace_bytes(desc, B, Tq, Tk)
    ws = Guarded(dev, (need,), torch.uint8)
    ws.bytes.fill_(fill)
    out = Guarded(dev, (B, Tq, KC.OUT), torch.float32)
    launches = (C.c_int64 * 9)()
    L.check(lib.pio_prof_begin(64), "pio_prof_begin")
    try:
        rc = lib.pio_attention_fwd(desc, R.tensor3(xq), R.tensor3(xkv), R.tensor3(xkv), km.data_ptr() if km is not None else None,
                                   None, None, None, out.ptr, None, ws.ptr, need, R.stream_ptr(dev))
    finally:
        assert lib.pio_prof_end(None, None, None, launches) >= 0
    assert rc == 0, f"pio_attention_fwd: return code {rc}"
    ws.check("workspace")
    out.check("out")
    return out.t.clone(), list(launches)


def _check(what, got, ref, bound):
    err = np.abs(got.double().cpu().numpy() - ref)
    bound = np.broadcast_to(bound, err.shape)
    live = bound > 0                      # (a sample without attendable key: bound 0, compared exactly below)
    ratio = float((err[live] / bound[live]).max())
    if not (err <= bound).all():
        i = np.unravel_index(np.argmax(err - bound), err.shape)
        raise AssertionError(f"{what}: worst |out - ref| / bound = {ratio:.3f} at (b, i, n) = {i}: got "
                             f"{got[i].item()!r} reference {ref[i]!r} bound {bound[i]:.3e}")
    return ratio


@pytest.mark.parametrize("case", KC.CASES, ids=[c["id"] for c in KC.CASES])
def test_kv_fold_composition(dev, case, monkeypatch):
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import runtime as R
    c = case
    prev = R.get_precision_policy()
    monkeypatch.delenv("PIO_KV_FOLD", raising=False)
    try:
        for policy in c["policies"]:
            P.set_precision_policy(policy)
            dt = KC.DT_OF[policy]
            assert R.kv_fold_offered()
            for probe in KC.PROBES:
                d = KC.make(c, probe, dt)
                if d is None:
                    continue
                what = f"K/V fold {c['id']} {policy} {probe}"
                m = _module(c, d, dev)
                desc = m._desc()
                pair = desc.act_split == 2
                assert pair == (policy == "fp16x2af") and desc.kq.w_hi and desc.vo.w_hi, what
                xq = torch.from_numpy(np.ascontiguousarray(d["xq"], np.float32)).to(dev)
                if c["Bq"] == 1 and c["B"] > 1:
                    xq = torch.broadcast_to(xq, (c["B"],) + tuple(xq.shape[1:]))
                xkv = torch.from_numpy(np.ascontiguousarray(d["x"], np.float32)).to(dev)
                ref = KC.reference(c, d)
                # 1. folded (where the route folds), on both poisons
                y, n1 = _run(dev, desc, c, xq, xkv, None, 0x7B)
                yff, _ = _run(dev, desc, c, xq, xkv, None, 0xFF)
                assert torch.equal(y.view(torch.int32), yff.view(torch.int32)), f"{what}: the result depends on stale workspace bytes"
                # 2. un-folded
                monkeypatch.setenv("PIO_KV_FOLD", "0")
                y0, n0 = _run(dev, desc, c, xq, xkv, None, 0x7B)
                monkeypatch.delenv("PIO_KV_FOLD")
                gemms1, gemms0 = sum(n1[k] for k in GEMM_CLASSES), sum(n0[k] for k in GEMM_CLASSES)
                print(f"{what}: launches per class folded {n1} un-folded {n0}")
                assert gemms0 == 4 and n0[5] == 1 and n0[3] == 0, f"{what}: un-folded launches {n0}"
                if c["fold"]:
                    assert gemms1 == 3 and n1[5] == 1 and n1[3] == 0, f"{what}: the fold did not engage: launches {n1}"
                    assert n1[2] == n0[2] + 1, f"{what}: one transpose beside the two casts: {n1} / {n0}"
                else:
                    assert n1 == n0 and torch.equal(y.view(torch.int32), y0.view(torch.int32)), f"{what}: below the threshold the fold is off"
                r1 = _check(what + " folded", y, ref, KC.bound(c, d, dt, pair, c["fold"]))
                r0 = _check(what + " un-folded", y0, ref, KC.bound(c, d, dt, pair, False))
                key = f"{c['id']} {policy}"
                w = worst_ratio.get(key, (0.0, 0.0))
                worst_ratio[key] = (max(w[0], r1), max(w[1], r0))
                print(f"{what}: worst |out - ref| / bound = folded {r1:.3f}, un-folded {r0:.3f}")
                # 3. a key mask: the fold steps aside
                kmn = KC.key_mask(c)
                km = torch.from_numpy(kmn.astype(np.uint8)).to(dev)
                ym, nm = _run(dev, desc, c, xq, xkv, km, 0x7B)
                monkeypatch.setenv("PIO_KV_FOLD", "0")
                ym0, nm0 = _run(dev, desc, c, xq, xkv, km, 0x7B)
                monkeypatch.delenv("PIO_KV_FOLD")
                assert nm == nm0 and sum(nm[k] for k in GEMM_CLASSES) == 4, f"{what}: masked launches {nm} / {nm0}"
                assert torch.equal(ym.view(torch.int32), ym0.view(torch.int32)), f"{what}: with a key mask the fold must step aside"
                assert kmn[0].any() and not kmn[0].all()
                _check(what + " masked", ym, KC.reference(c, d, kmn), KC.bound(c, d, dt, pair, False, kmn))
                if dt == "f16" and c["B"] > 1:
                    fb = m.final.bias.detach()
                    dead = ym[c["B"] - 1]
                    assert torch.equal(dead, fb[None, :].expand_as(dead)), f"{what}: a sample without attendable key must be final.bias"
    finally:
        P.set_precision_policy(prev)
