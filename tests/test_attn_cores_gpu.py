"""GPU: the three fused attention cores through the raw C-ABI (pio_flash_attention, pio_flash_attention_pair cores 1 / 2 /
3), one case per kernel branch (tests/attn_core_cases.py), four probes per case, against the float64 reference on the same
16-bit operands, element by element, at the DERIVED bound of attn_core_cases.bound().

Every launch: O (and O_lo) between 4 KiB guards, NaN-prefilled, two spare rows behind every sample's Tq; row pitches wider
than the data (ldq = H dkp + 8, ldk = H dkp + 16, ldo = H dvp + 8, or + 4 for the per-lane 8-byte epilogue of the
self-attention kernel), the gap columns of Q / K / row-major V holding NaN; 32 NaN rows of K behind the last sample (the
cross-attention kernel reads whole tiles); V^T columns behind Tk zero; the workspace exactly as large as the library asks,
guarded too.  Gap columns, spare rows and guards must come back untouched.

Measured on an MI355X, worst |o - ref| / bound over all cases and probes: the docstring of test_report."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_core_cases as AC  # noqa: E402
from test_primitives_gpu import Guarded, TDT, _dt, _stream  # noqa: E402

pytestmark = pytest.mark.gpu

PIO_E_SHAPE, PIO_E_ALIGN, PIO_E_WORKSPACE, PIO_E_ARG = -1, -2, -4, -6
CORE = {"flash": 1, "xattn": 2, "xtall": 3}
WORST = {}          # (kernel, dtype) -> (worst |o - ref| / bound, worst |o - ref| / max|V|, case, probe)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


def _rows16(a, rows_extra, ld, dt, dev):
    """float64 [R, C] -> device [R + rows_extra, ld] of the 16-bit type, NaN everywhere but [:R, :C]."""
    R, C = a.shape
    t = torch.full((R + rows_extra, ld), float("nan"), dtype=TDT[dt], device=dev)
    t[:R, :C] = torch.from_numpy(a.astype(np.float32)).to(dev).to(TDT[dt])
    return t


class Launch:
    """Device operands of one (case, probe, dtype); run() launches on fresh guarded outputs."""

    def __init__(self, dev, c, d, dt, replicate_q=False):
        self.dev, self.c, self.d, self.dt = dev, c, d, dt
        B, H, Tq, Tk, dkp, dvp = c["B"], c["H"], c["Tq"], c["Tk"], c["dkp"], c["dvp"]
        self.ldq, self.ldk, self.ldo = H * dkp + 8, H * dkp + 16, H * dvp + c["ldo_gap"]
        qh, ql = d["qh"], d["ql"]
        if replicate_q:
            qh = np.broadcast_to(qh, (B,) + qh.shape[1:])
            ql = None if ql is None else np.broadcast_to(ql, (B,) + ql.shape[1:])
        Bq = qh.shape[0]
        self.sQb = Tq * self.ldq if Bq == B else 0
        self.q = _rows16(qh.reshape(Bq * Tq, H * dkp), 0, self.ldq, dt, dev)
        self.k = _rows16(d["kh"].reshape(B * Tk, H * dkp), 32, self.ldk, dt, dev)
        self.ql = self.kl = None
        if ql is not None:
            self.ql = _rows16(ql.reshape(Bq * Tq, H * dkp), 0, self.ldq, dt, dev)
            self.kl = _rows16(d["kl"].reshape(B * Tk, H * dkp), 32, self.ldk, dt, dev)
        if c["vrow"]:
            self.ldv = H * dvp + 8
            self.v = _rows16(d["v"].reshape(B * Tk, H * dvp), 0, self.ldv, dt, dev)
            self.sVb = Tk * self.ldv
        else:                                           # V^T [B][H dvp][ldv], zeros behind Tk
            self.ldv = max(64, (Tk + 31) // 32 * 32)
            vt = np.zeros((B, H * dvp, self.ldv), np.float32)
            vt[:, :, :Tk] = d["v"].reshape(B, Tk, H * dvp).transpose(0, 2, 1)
            self.v = torch.from_numpy(vt).to(dev).to(TDT[dt])
            self.sVb = H * dvp * self.ldv
        self.km = None if d["km"] is None else d["km"].astype(np.uint8)
        self.qm = None if d["qm"] is None else d["qm"].astype(np.uint8)

    def run(self, entry="pair", mask_byte=1, core=None, ws_short=0, expect=0, v_rowmajor=None, ldv=None, misalign=None,
            olo=None):
        """One launch; returns (O tensor [B, Tq, H dvp], O_lo tensor or None) after the memory checks, or None when
        `expect` is an error code (then the outputs must still be all NaN)."""
        from perceiverio_pytorch_amd import _lib as L
        lib = L.lib()
        c, dev, dt = self.c, self.dev, self.dt
        B, H, Tq, Tk, dkp, dvp = c["B"], c["H"], c["Tq"], c["Tk"], c["dkp"], c["dvp"]
        rows = Tq + 2
        want_lo = c["olo"] if olo is None else olo
        o = Guarded(dev, (B, rows, self.ldo), TDT[dt])
        ol = Guarded(dev, (B, rows, self.ldo), TDT[dt]) if want_lo else None
        keep = []

        def mask(m):
            if m is None:
                return None
            keep.append(torch.from_numpy(m * np.uint8(mask_byte)).to(dev))
            return keep[-1].data_ptr()

        vrow = int(c["vrow"]) if v_rowmajor is None else v_rowmajor
        strides = (self.ldq, self.ldk, self.ldv if ldv is None else ldv, self.ldo, self.sQb, Tk * self.ldk, self.sVb,
                   rows * self.ldo)
        what = f"{c['id']} {dt} {entry}"
        off = {"Q": 0, "K": 0, "O": 0}
        if misalign:
            off[misalign] = 2
        if entry == "flash":
            rc = lib.pio_flash_attention(_dt(dt), dkp, dvp, c["dk"], self.q.data_ptr(), self.k.data_ptr(), self.v.data_ptr(),
                                         o.ptr, B, H, Tq, Tk, *strides, vrow, _stream())
            ws = None
        else:
            nb = lib.pio_flash_attention_pair_workspace_bytes(dkp, dvp, B, H, Tq, Tk)
            nb = max(nb - ws_short, 0)
            ws = Guarded(dev, (max(nb, 16),), torch.uint8) if nb else None
            ws_ptr = None
            if ws is not None:                          # exactly nb bytes, ending at the rear guard
                ws_ptr = ws.ptr + (max(nb, 16) - nb)
                assert ws_ptr % 16 == 0 or nb < 16
            rc = lib.pio_flash_attention_pair(
                _dt(dt), dkp, dvp, c["dk"], self.q.data_ptr() + off["Q"], None if self.ql is None else self.ql.data_ptr(),
                self.k.data_ptr() + off["K"], None if self.kl is None else self.kl.data_ptr(), self.v.data_ptr(),
                o.ptr + off["O"], ol.ptr if ol else None, B, H, Tq, Tk, *strides, vrow, mask(self.km), mask(self.qm),
                CORE[c["kern"]] if core is None else core, ws_ptr, nb, _stream())
        torch.cuda.synchronize()
        o.check(what + " O")
        if ol:
            ol.check(what + " O_lo")
        if ws is not None:
            ws.check(what + " workspace")
        if expect != 0:
            assert rc == expect, f"{what}: returned {rc}, expected {expect}"
            assert torch.isnan(o.t).all() and (ol is None or torch.isnan(ol.t).all()), f"{what}: a refused call wrote"
            return None
        L.check(rc, what)
        out = []
        for g, name in ((o, "O"), (ol, "O_lo")):
            if g is None:
                out.append(None)
                continue
            assert torch.isnan(g.t[:, :, H * dvp:]).all(), f"{what}: gap columns of {name} were written"
            assert torch.isnan(g.t[:, Tq:, :]).all(), f"{what}: rows behind Tq of {name} were written"
            out.append(g.t[:, :Tq, :H * dvp].clone())
        return out


def _f64(t, c):
    return t.float().cpu().numpy().astype(np.float64).reshape(c["B"], c["Tq"], c["H"], c["dvp"])


def _compare(c, d, ref, dt, probe, o, ol):
    B, Tk = c["B"], c["Tk"]
    got = _f64(o, c)
    assert np.isfinite(got).all(), f"{c['id']} {dt} {probe}: non-finite output"
    vmax = AC.vmax_of(d)                                        # [B, 1, H, 1]
    km = d["km"] if d["km"] is not None else np.ones((B, Tk), bool)
    live = np.broadcast_to(km.any(axis=1)[:, None], (B, c["Tq"])).copy()
    if d["qm"] is not None:
        live &= d["qm"]
    dead = ~live
    if dead.any():
        assert (got[dead] == 0).all(), f"{c['id']} {dt} {probe}: wiped rows must be exactly zero"
    figs = [(got, False)]
    if ol is not None:
        lo = _f64(ol, c)
        assert np.isfinite(lo).all()
        if dead.any():
            assert (lo[dead] == 0).all(), f"{c['id']} {dt} {probe}: wiped rows of O_lo must be exactly zero"
        figs.append((got + lo, True))
    for y, pair_sum in figs:
        err = np.abs(y - ref)
        bnd = AC.bound(dt, Tk, np.maximum(vmax, 2.0 ** -20), pair_sum)
        ratio = err / bnd
        w = float(ratio.max())
        rel = float((err / np.maximum(vmax, 2.0 ** -20)).max())
        key = (c["kern"] + ("+lo" if pair_sum else ""), dt)
        if key not in WORST or w > WORST[key][0]:
            WORST[key] = (w, rel, c["id"], probe)
        print(f"{c['id']} {dt} {probe}{' O+O_lo' if pair_sum else ''}: worst |o - ref| / bound = {w:.3f} "
              f"(|o - ref| / max|V| = {rel:.3e}, bound / max|V| = {float(AC.bound(dt, Tk, 1.0, pair_sum)):.3e})")
        if w > 1.0:
            i = np.unravel_index(np.argmax(ratio), ratio.shape)
            t = None if d["targets"] is None else int(d["targets"][i[0], i[2], i[1]])
            raise AssertionError(f"{c['id']} {dt} {probe}: element (b, q, h, c) = {i} (planted target {t}): got {y[i]!r} "
                                 f"ref {ref[i]!r} err {err[i]:.3e} bound {np.broadcast_to(bnd, err.shape)[i]:.3e}")


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, b))


def _run_case(dev, c):
    refs = {}
    for dt in c["dts"]:
        for probe in AC.PROBES:
            d = AC.make(c, probe, dt)
            if d is None:
                continue
            if probe == "random" or probe not in refs:      # (the other probes' operands are the same in both types)
                refs[probe] = AC.reference(d)
            ref = refs[probe]
            ln = Launch(dev, c, d, dt)
            o, ol = ln.run()
            _compare(c, d, ref, dt, probe, o, ol)
            if probe not in ("planted", "stair_up", "random"):
                continue
            # ---- exact claims: on the planted probe, and on two whose rows are sums over many keys (there a changed
            # summation order, another route or a mis-read mask byte changes bits)
            if c["twice"] or c["label"][-1] > 1:
                assert _same((o, ol), ln.run()), f"{c['id']} {dt}: two runs must be bit-identical"
            if c["kern"] == "flash" and not c["pair"]:
                assert _same((o,), ln.run(entry="flash")[:1]), \
                    f"{c['id']} {dt}: core 1 with NULL lo operands must be bit-identical to pio_flash_attention"
            if c["sqb0"]:
                assert _same((o, ol), Launch(dev, c, d, dt, replicate_q=True).run()), \
                    f"{c['id']} {dt}: batch-invariant Q (sQb = 0) must be bit-identical to the same Q replicated"
            if c["mask_bytes"]:
                for byte in (0x02, 0x80, 0xFF):
                    assert _same((o, ol), ln.run(mask_byte=byte)), f"{c['id']} {dt}: mask byte {byte:#x} must act as 0x01"


def _ids(kern):
    return [c["id"] for c in AC.CASES if c["kern"] == kern]


@pytest.mark.parametrize("cid", _ids("flash"))
def test_flash_attn_kernel(dev, cid):
    _run_case(dev, AC.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("xattn"))
def test_xattn_kernel(dev, cid):
    _run_case(dev, AC.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("xtall"))
def test_xattn_tall_kernel(dev, cid):
    c = AC.BY_ID[cid]
    _run_case(dev, c)
    if c["fwd"]:
        _tall_through_attention_fwd(dev, c)


def _tall_through_attention_fwd(dev, c):
    """The raw core-3 launch and the routed one (pio_attention_fwd, identity projections, policy "fp16": q = xq, k = xk,
    v = xv, out = float(core output) exactly) give the same bits, on the planted and on the random probe, and the routed
    call runs exactly one fused core and no materialised softmax (launch accounting of pio_prof_begin / pio_prof_end:
    class 5 = fused attention cores, class 3 = softmax_rows)."""
    import ctypes as C
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    B, H, Tq, Tk, dk, dv = c["B"], c["H"], c["Tq"], c["Tk"], c["dkp"], c["dvp"]
    m = Attention(H * dk, H * dk, H * dv, num_heads=H, qk_out_channels=H * dk, v_out_channels=H * dv, output_channels=H * dv)
    for lin, n in ((m.proj_q, H * dk), (m.proj_k, H * dk), (m.proj_v, H * dv), (m.final, H * dv)):
        lin.weight.copy_(torch.eye(n))
        lin.bias.zero_()
    m = m.to(dev).eval()
    lib = P.lib()
    prev = R.get_precision_policy()
    P.set_precision_policy("fp16")
    try:
        desc = m._desc()
        ws = R.workspace(dev, lib.pio_attention_workspace_bytes(desc, B, Tq, Tk))
        for probe in ("planted", "random"):
            d = AC.make(c, probe, "f16")
            raw = Launch(dev, c, d, "f16").run()[0].float()
            xq, xk, xv = (torch.from_numpy(x.reshape(B, -1, x.shape[2] * x.shape[3]).astype(np.float32)).to(dev)
                          for x in (d["qh"], d["kh"], d["v"]))
            out = torch.empty((B, Tq, H * dv), dtype=torch.float32, device=dev)
            L.check(lib.pio_prof_begin(64), "pio_prof_begin")
            rc = lib.pio_attention_fwd(desc, R.tensor3(xq), R.tensor3(xk), R.tensor3(xv), None, None, None, None,
                                       out.data_ptr(), None, ws.data_ptr(), ws.numel(), R.stream_ptr(dev))
            launches = (C.c_int64 * 9)()
            assert lib.pio_prof_end(None, None, None, launches) >= 0
            L.check(rc, "pio_attention_fwd")
            torch.cuda.synchronize()
            assert launches[5] == 1 and launches[3] == 0, f"the routed call must run one fused core: {list(launches)}"
            assert torch.equal(out, raw), \
                f"{probe}: routed and raw tall-head launches differ: max {float((out - raw).abs().max()):.3e}"
    finally:
        P.set_precision_policy(prev)


def test_refusals_launch_nothing(dev):
    """Every refused call returns its code and leaves the NaN-prefilled outputs untouched."""
    x = AC.BY_ID["xattn_split2_tk520"]
    d = AC.make(x, "planted", "f16")
    ln = Launch(dev, x, d, "f16")
    ln.run(ldv=ln.ldv + 8, expect=PIO_E_ALIGN)              # ldv % 32 != 0
    ln.run(misalign="Q", expect=PIO_E_ALIGN)
    ln.run(misalign="K", expect=PIO_E_ALIGN)
    ln.run(misalign="O", expect=PIO_E_ALIGN)
    ln.run(ws_short=1, expect=PIO_E_WORKSPACE)              # one byte short; the exact size runs in test_xattn_kernel
    ln.run(v_rowmajor=1, expect=PIO_E_ARG)
    m = AC.BY_ID["xattn_32x160_lead2"]                      # (32, 160): the self-attention kernel covers the shape ...
    lm = Launch(dev, m, AC.make(m, "planted", "f16"), "f16")
    lm.run(core=1, olo=False, expect=PIO_E_ARG)             # ... but takes no mask
    t = AC.BY_ID["xtall_1024_tk512_sqb0"]
    t513 = dict(t, Tk=513)
    lt = Launch(dev, t513, AC.make(t513, "uniform", "f16"), "f16")
    lt.run(core=3, expect=PIO_E_SHAPE)                      # the tall-head kernel covers 512 keys
    k = AC.BY_ID["xtall_64x768_tk257_mask"]
    lk = Launch(dev, k, AC.make(k, "uniform", "f16"), "f16")
    lk.run(ws_short=1, expect=PIO_E_WORKSPACE)
    lk.run(core=2, expect=PIO_E_SHAPE)                      # (64, 768): not a shape of the tiled kernel


def test_report():
    """Worst figures of this run per kernel and dtype (run with -s).  Measured on an MI355X, as a fraction of the derived
    bound and as |o - ref| / max|V| next to bound / max|V| ("+lo": O + O_lo compared, the O term dropped):
        flash     f16  0.264  2.63e-4 / 9.96e-4  (flash_32_row_pair_olo, stair_up)
                  bf16 0.266  2.08e-3 / 7.83e-3  (flash_32_row_dk25, stair_up)
        flash+lo  f16  0.140  7.06e-5 / 5.05e-4  (flash_32x160_vt_pair_olo, stair_down)
        xattn     f16  0.299  2.97e-4 / 9.95e-4  (xattn_32x96_pair_both_masks, stair_up)
                  bf16 0.345  2.70e-3 / 7.83e-3  (xattn_32x96_dk8_dv8_singles, random)
        xattn+lo  f16  0.363  1.84e-4 / 5.07e-4  bf16  0.383  1.50e-3 / 3.92e-3  (xattn_32x96_dk8_dv8_singles, random)
        xtall     f16  0.250  2.48e-4 / 9.93e-4  (xtall_64x256_tk33, stair_up)   bf16  0.152  1.19e-3 / 7.83e-3
        xtall+lo  f16  0.137  6.91e-5 / 5.05e-4  bf16  0.144  5.64e-4 / 3.92e-3  (xtall_64x256_tk33, random)
    The planted probe measures <= 3.4e-9 max|V| on every case (exp(-16) weights on the other keys): no key is misplaced,
    dropped or added on any branch.  No case exceeded the bound; the kernels needed no change."""
    for key in sorted(WORST):
        w, rel, cid, probe = WORST[key]
        print(f"{key[0]:10s} {key[1]:5s} worst |o - ref| / bound = {w:.3f}   |o - ref| / max|V| = {rel:.3e}   ({cid}, {probe})")
    assert all(v[0] <= 1.0 for v in WORST.values())
