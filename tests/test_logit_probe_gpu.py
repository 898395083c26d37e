"""GPU: the logit probe -- qk_absmax_kernel through pio_qk_logit_absmax against float64 on the same 16-bit values, the
hook in attention_core on every reachable core (pio_logit_probe_begin / _end), and recommend_precision_policy on the
language goldens.  Measured figures: profiles/logit_probe.json."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAD_ROWS = 40          # allocated rows behind Tq / Tk (more than the 31 a 32-key tile could reach), filled with PAD_VALUE
PAD_VALUE = 6e4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- raw primitive ---------------------------------------------------------------------------------------------------
RAW_CASES = {
    # name: dtype, dkp, dk, H, B, Tq, Tk, batch-invariant queries
    "f16_dk8": ("f16", 8, 8, 2, 1, 17, 33, False),
    "f16_dk32_tails": ("f16", 32, 32, 8, 2, 130, 70, False),
    "f16_dk328_bcast": ("f16", 328, 322, 1, 3, 64, 1000, True),
    "f16_dk1024": ("f16", 1024, 1024, 1, 2, 100, 512, False),
    "f16_stacked_qkv": ("f16", 32, 32, 4, 2, 96, 96, False),
    "bf16_dk64": ("bf16", 64, 64, 4, 1, 128, 128, False),
}


def _round16(a, dtype):
    t = torch.from_numpy(a.astype(np.float32)).to(torch.float16 if dtype == "f16" else torch.bfloat16)
    return t, t.double().numpy()


def _gen_raw(name):
    """q [Bq,Tq,H,dkp], k [B,Tk,H,dkp] as float64 values that are exact in the operand dtype (channels behind dk zero)."""
    dtype, dkp, dk, H, B, Tq, Tk, bcast = RAW_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    q = rng.standard_normal((1 if bcast else B, Tq, H, dkp))
    k = rng.standard_normal((B, Tk, H, dkp))
    q[..., dk:] = 0
    k[..., dk:] = 0
    return _round16(q, dtype)[1], _round16(k, dtype)[1]


def _ref_raw(q, k, dk, km=None, qm=None, fm=None):
    """(max |s|, bound unit max sum_c |q_c k_c| * scale) over the attendable positions, float64."""
    B = k.shape[0]
    qb = np.broadcast_to(q, (B,) + q.shape[1:])
    scale = 1.0 / np.sqrt(dk)
    s = np.abs(np.einsum("bihc,bjhc->bhij", qb, k)) * scale
    u = np.einsum("bihc,bjhc->bhij", np.abs(qb), np.abs(k)) * scale
    live = np.ones(s.shape, bool)
    if km is not None:
        live &= km[:, None, None, :] != 0
    if qm is not None:
        live &= qm[:, None, :, None] != 0
    if fm is not None:
        live &= fm[:, None, :, :] != 0
    s, u = np.where(live, s, 0.0), np.where(live, u, 0.0)
    return float(s.max()), float(u.max()), np.unravel_index(np.argmax(s), s.shape)


def _launch_raw(dev, name, q, k, km=None, qm=None, fm=None):
    """Lay q / k out as the fused cores read them -- PAD_ROWS rows of PAD_VALUE behind Tq and Tk of EVERY sample -- and run
    pio_qk_logit_absmax once."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L
    dtype, dkp, dk, H, B, Tq, Tk, bcast = RAW_CASES[name]
    tdt = torch.float16 if dtype == "f16" else torch.bfloat16
    Bq = q.shape[0]
    if name == "f16_stacked_qkv":                       # one [B][T][q | k | v] buffer, Q and K its column ranges
        assert Tq == Tk and Bq == B
        ld = H * (2 * dkp + 32)
        buf = torch.full((B, Tq + PAD_ROWS, ld), PAD_VALUE, dtype=tdt)
        buf[:, :Tq, :H * dkp] = torch.from_numpy(q.reshape(B, Tq, H * dkp)).to(tdt)
        buf[:, :Tk, H * dkp:2 * H * dkp] = torch.from_numpy(k.reshape(B, Tk, H * dkp)).to(tdt)
        buf = buf.to(dev)
        qp, kp = buf.data_ptr(), buf.data_ptr() + 2 * H * dkp
        ldq = ldk = ld
        sq = sk = (Tq + PAD_ROWS) * ld
        keep = [buf]
    else:
        qa = torch.full((Bq, Tq + PAD_ROWS, H * dkp), PAD_VALUE, dtype=tdt)
        ka = torch.full((B, Tk + PAD_ROWS, H * dkp), PAD_VALUE, dtype=tdt)
        qa[:, :Tq] = torch.from_numpy(q.reshape(Bq, Tq, H * dkp)).to(tdt)
        ka[:, :Tk] = torch.from_numpy(k.reshape(B, Tk, H * dkp)).to(tdt)
        qa, ka = qa.to(dev), ka.to(dev)
        qp, kp, ldq, ldk = qa.data_ptr(), ka.data_ptr(), H * dkp, H * dkp
        sq, sk = (0 if bcast else (Tq + PAD_ROWS) * ldq), (Tk + PAD_ROWS) * ldk
        keep = [qa, ka]
    masks = [(_t(m.astype(np.uint8), dev) if m is not None else None) for m in (km, qm, fm)]
    out = torch.zeros(1, dtype=torch.float32, device=dev)
    code = P.lib().pio_qk_logit_absmax(L.PIO_DT_F16 if dtype == "f16" else L.PIO_DT_BF16, dkp, dk, qp, kp, B, H, Tq, Tk, ldq,
                                       ldk, sq, sk, *[m.data_ptr() if m is not None else None for m in masks],
                                       out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    L.check(code, "pio_qk_logit_absmax")
    torch.cuda.synchronize()
    del keep
    return float(out.item())


def _bound(name, unit):
    """fp32 accumulation of dkp products plus headroom: dkp * 2^-23 * scale * max_ij sum_c |q_ic k_jc| (the issue's bound)."""
    return RAW_CASES[name][1] * 2.0 ** -23 * unit


@pytest.mark.parametrize("name", sorted(RAW_CASES))
def test_raw_primitive_vs_float64(dev, name):
    dtype, dkp, dk, H, B, Tq, Tk, bcast = RAW_CASES[name]
    q, k = _gen_raw(name)
    ref, unit, _ = _ref_raw(q, k, dk)
    got = _launch_raw(dev, name, q, k)
    print(f"{name}: absmax {got:.6f} float64 {ref:.6f} |diff| {abs(got - ref):.3e} bound {_bound(name, unit):.3e}")
    assert abs(got - ref) <= _bound(name, unit), (name, got, ref)


@pytest.mark.parametrize("corner", ["last", "first"])
@pytest.mark.parametrize("name", ["f16_dk32_tails", "f16_dk328_bcast", "bf16_dk64"])
def test_planted_maximum_at_the_corners(dev, name, corner):
    """The true maximum once at (Tq - 1, Tk - 1) of the last batch / head, once at (0, 0) of the first."""
    dtype, dkp, dk, H, B, Tq, Tk, bcast = RAW_CASES[name]
    q, k = _gen_raw(name)
    b, h, i, j = (B - 1, H - 1, Tq - 1, Tk - 1) if corner == "last" else (0, 0, 0, 0)
    pat = np.where(np.arange(dkp) % 2 == 0, 4.0, -4.0) * (np.arange(dkp) < dk)
    q[0 if bcast else b, i, h] = pat
    k[b, j, h] = pat
    ref, unit, where = _ref_raw(q, k, dk)
    assert tuple(where) == (b, h, i, j) and ref == pytest.approx(16.0 * dk / np.sqrt(dk))
    got = _launch_raw(dev, name, q, k)
    assert abs(got - ref) <= _bound(name, unit), (name, corner, got, ref)


@pytest.mark.parametrize("which", ["kv_mask", "q_mask", "full_mask"])
@pytest.mark.parametrize("name", ["f16_dk32_tails", "f16_dk328_bcast"])
def test_planted_value_under_a_mask_is_ignored(dev, name, which):
    dtype, dkp, dk, H, B, Tq, Tk, bcast = RAW_CASES[name]
    q, k = _gen_raw(name)
    rng = np.random.default_rng(7)
    b, h, i, j = B - 1, H - 1, Tq - 2, Tk - 3
    pat = np.where(np.arange(dkp) % 2 == 0, 8.0, -8.0) * (np.arange(dkp) < dk)
    km = (rng.random((B, Tk)) > 0.2).astype(np.uint8)
    qm = (rng.random((B, Tq)) > 0.2).astype(np.uint8)
    fm = (rng.random((B, Tq, Tk)) > 0.2).astype(np.uint8)
    if which == "kv_mask":
        k[b, j, h] = pat * 8
        km[b, j] = 0
        masks = dict(km=km)
    elif which == "q_mask":
        if bcast:
            qm[:, i] = 0                               # (batch-invariant queries: the planted row is every sample's)
        q[0 if bcast else b, i, h] = pat * 8
        qm[b, i] = 0
        masks = dict(qm=qm)
    else:
        q[0 if bcast else b, i, h] = pat
        k[b, j, h] = pat
        fm[:, i, j] = 0
        masks = dict(fm=fm)
    ref_open, _, _ = _ref_raw(q, k, dk)
    ref, unit, _ = _ref_raw(q, k, dk, **masks)
    assert ref_open > 2 * ref > 0, "the planted value must dominate when nothing is masked"
    got = _launch_raw(dev, name, q, k, **masks)
    print(f"{name} {which}: absmax {got:.5f} float64 {ref:.5f} (unmasked {ref_open:.2f})")
    assert abs(got - ref) <= _bound(name, unit), (name, which, got, ref, ref_open)


def test_nothing_attendable_is_zero_and_nan_is_inf(dev):
    name = "f16_dk32_tails"
    dtype, dkp, dk, H, B, Tq, Tk, bcast = RAW_CASES[name]
    q, k = _gen_raw(name)
    assert _launch_raw(dev, name, q, k, km=np.zeros((B, Tk), np.uint8)) == 0.0
    k[1, Tk - 1, 3, 5] = np.nan
    km = np.ones((B, Tk), np.uint8)
    assert _launch_raw(dev, name, q, k, km=km) == float("inf")          # a NaN in an attendable key
    km[1, Tk - 1] = 0
    ref, unit, _ = _ref_raw(np.nan_to_num(q), np.nan_to_num(k), dk, km=km)
    got = _launch_raw(dev, name, q, k, km=km)                            # ... and the same key masked out
    assert abs(got - ref) <= _bound(name, unit)
    k[1, Tk - 1, 3, 5] = np.inf
    assert _launch_raw(dev, name, q, k) == float("inf")


def test_error_codes(dev):
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L
    lib = P.lib()
    z = torch.zeros(4096, dtype=torch.float16, device=dev)
    o = torch.zeros(1, dtype=torch.float32, device=dev)
    p = z.data_ptr()
    call = lambda dt, dkp, dk, qp, ldq, op: lib.pio_qk_logit_absmax(dt, dkp, dk, qp, p, 1, 1, 4, 4, ldq, 32, 0, 0, None, None,  # noqa: E731
                                                                    None, op, 0)
    assert call(L.PIO_DT_F16, 12, 12, p, 32, o.data_ptr()) == -1       # PIO_E_SHAPE: dkp % 8
    assert call(L.PIO_DT_F16, 32, 40, p, 32, o.data_ptr()) == -1       # dk > dkp
    assert call(L.PIO_DT_F16, 32, 32, p + 2, 32, o.data_ptr()) == -2   # PIO_E_ALIGN: pointer
    assert call(L.PIO_DT_F16, 32, 32, p, 36, o.data_ptr()) == -2       # row pitch
    assert call(L.PIO_DT_F16, 32, 32, None, 32, o.data_ptr()) == -6    # PIO_E_ARG
    assert call(L.PIO_DT_F16, 32, 32, p, 32, None) == -6
    assert call(7, 32, 32, p, 32, o.data_ptr()) == -6
    assert lib.pio_logit_probe_begin(None, 4) == -6 and lib.pio_logit_probe_begin(o.data_ptr(), 0) == -6
    assert lib.pio_logit_probe_end() == 0                              # not active
    torch.cuda.synchronize()
    assert float(o.item()) == 0.0


# ---- the hook in attention_core, one small shape per reachable core -----------------------------------------------------
BLOCK_CASES = {
    # name: policy, H, q_in, kv_in, qk, v, B, Tq, Tk, mask, extra
    "qkv_flash": ("fp16", 4, 128, 128, 128, 128, 2, 96, 96, None, "self"),
    "pair_flash": ("fp16x3fq", 4, 64, 64, 128, 128, 2, 70, 90, None, None),
    "pair_xattn_keymask": ("fp16x3fq", 4, 64, 64, 128, 128, 2, 70, 90, "key", None),
    "xattn_querymask": ("fp16", 2, 64, 64, 64, 192, 2, 70, 90, "query", None),
    "kvfold_xattn": ("fp16", 1, 48, 64, 64, 64, 2, 16, 200, None, "kvfold"),
    # (the tall-head kernel takes heads beyond the tiled kernel's tables: a 256-wide head with dv = 256 runs on the cross-
    #  attention kernel's <352, 352> instantiation whatever the key count -- tests/test_attn_route_gpu.py -- hence 1024)
    "xtall": ("fp16", 1, 64, 64, 1024, 1024, 2, 128, 100, None, None),
    "materialised_bias": ("fp16x3", 2, 32, 32, 32, 32, 2, 20, 30, None, "bias"),
}
SPLIT_OPERAND = ("fp16x3", "fp16x3fq")
# Gap of a block-level record to the float64 figure from the module's weights, in units of scale * max sum_c |q_c k_c|.
#   split-operand policies: q and k are exact up to ONE rounding each at 2^-11, times a factor of two: 2^-9;
#   single-sweep policies: inputs AND weights are rounded in front of the projections as well -- measured on the MI355X
#   (profiles/logit_probe.json "block_gaps": worst SINGLE_SWEEP_WORST), allowed 4 x that for other rounding realisations.
SPLIT_TOL_UNITS = 2.0 ** -9
#   Measured: qkv_flash 1.98e-5, kvfold_xattn 4.00e-5 (un-folded 4.69e-5), xtall 3.05e-5, xattn_querymask 2.385e-4.
SINGLE_SWEEP_WORST = 2.385e-4
SINGLE_SWEEP_TOL_UNITS = 4 * SINGLE_SWEEP_WORST


def _np64(t):
    return t.detach().double().cpu().numpy()


def _block(dev, name):
    """Build the module + inputs of one case; returns run(probe_records) -> (out, records, calls, launches) and the float64
    figure / unit from the module's weights."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import Attention, SelfAttention
    policy, H, q_in, kv_in, qk, vv, B, Tq, Tk, mk, extra = BLOCK_CASES[name]
    torch.manual_seed(sum(map(ord, name)))
    rng = np.random.default_rng(sum(map(ord, name)))
    lib = P.lib()
    km = qm = None
    if mk == "key":
        km = rng.random((B, Tk)) > 0.3
        km[:, 0] = True
    elif mk == "query":
        qm = rng.random((B, Tq)) > 0.3
    xq = torch.randn(B, Tq, q_in) * 2
    xkv = xq if extra == "self" else torch.randn(B, Tk, kv_in) * 2
    bias = torch.randn(B, H, Tq, Tk).to(dev) if extra == "bias" else None
    if extra == "self":
        m = SelfAttention(q_in, widening_factor=1, num_heads=H).eval()
        with torch.no_grad():
            m.layer_norm1.weight.uniform_(0.5, 3.0)
        att = m.attention
        ln = m.layer_norm1
        x64 = _np64(xq)
        mu = x64.mean(-1, keepdims=True)
        n64 = (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + ln.eps) * _np64(ln.weight) + _np64(ln.bias)
        nq = nk = n64
    else:
        m = att = Attention(q_in, kv_in, kv_in, num_heads=H, qk_out_channels=qk, v_out_channels=vv,
                            output_channels=q_in).eval()
        nq, nk = _np64(xq), _np64(xkv)
    q = (nq @ _np64(att.proj_q.weight).T + _np64(att.proj_q.bias)).reshape(B, Tq, H, -1)
    k = (nk @ _np64(att.proj_k.weight).T + _np64(att.proj_k.bias)).reshape(B, Tk, H, -1)
    ref, unit, _ = _ref_raw(q, k, q.shape[-1], km=km, qm=qm)
    m = m.to(dev)
    xq_t, xkv_t = xq.to(dev), xkv.to(dev)
    kmt = _t(km, dev).view(torch.uint8) if km is not None else None
    qmt = _t(qm, dev).view(torch.uint8) if qm is not None else None

    def run(max_records):
        prev = R.get_precision_policy()
        P.set_precision_policy(policy)
        try:
            d = m._desc()
            out = torch.full((B, Tq, q_in), float("nan"), dtype=torch.float32, device=dev)
            rec = torch.zeros(8, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            s = R.stream_ptr(dev)
            L.check(lib.pio_prof_begin(64), "pio_prof_begin")
            if max_records:
                L.check(lib.pio_logit_probe_begin(rec.data_ptr(), max_records), "pio_logit_probe_begin")
            try:
                if extra == "self":
                    ws = R.workspace(dev, lib.pio_self_attention_workspace_bytes(d, B, Tq))
                    code = lib.pio_self_attention_fwd(d, R.tensor3(xq_t), None, None, None, None, out.data_ptr(), None,
                                                      None, ws.data_ptr(), ws.numel(), s)
                else:
                    ws = R.workspace(dev, lib.pio_attention_workspace_bytes(d, B, Tq, Tk))
                    code = lib.pio_attention_fwd(d, R.tensor3(xq_t), R.tensor3(xkv_t), R.tensor3(xkv_t),
                                                 kmt.data_ptr() if kmt is not None else None,
                                                 qmt.data_ptr() if qmt is not None else None, None,
                                                 bias.data_ptr() if bias is not None else None, out.data_ptr(), None,
                                                 ws.data_ptr(), ws.numel(), s)
            finally:
                calls = lib.pio_logit_probe_end()
                launches = (C.c_int64 * 9)()
                assert lib.pio_prof_end(None, None, None, launches) >= 0
            L.check(code, name)
            torch.cuda.synchronize()
            return out, rec.cpu().tolist(), calls, list(launches)
        finally:
            P.set_precision_policy(prev)

    return run, ref, unit


@pytest.mark.parametrize("name", sorted(BLOCK_CASES))
def test_probe_hook_on_every_core(dev, name):
    policy, H, q_in, kv_in, qk, vv, B, Tq, Tk, mk, extra = BLOCK_CASES[name]
    run, ref, unit = _block(dev, name)
    out_off, rec_off, calls_off, launches_off = run(0)
    out_on, rec, calls, launches = run(4)
    gap = abs(rec[0] - ref) / unit
    print(f"{name} [{policy}]: record {rec[0]:.6f} float64 {ref:.6f} gap {gap:.3e} units (2^-9 = {2.0 ** -9:.3e}) "
          f"launches {launches}")
    # nothing but the probe's own kernel is added: same result bits, same launches per profiler class, one record
    assert calls_off == 0 and rec_off == [0.0] * 8
    assert calls == 1 and rec[1:] == [0.0] * 7
    assert torch.isfinite(out_off).all() and torch.equal(out_on, out_off), "the probe changed the block's output"
    assert launches == launches_off, "the probe changed what the block launches"
    if name == "materialised_bias":
        assert launches[5] == 0 and launches[3] >= 1
    else:
        assert launches[5] == 1 and launches[3] == 0, "the case must run on a fused core"
    if extra == "kvfold":
        # the K / V fold really is the route: with it switched off (PIO_KV_FOLD is read per call) the core multiplies other
        # operands -- q k^T instead of (q Wk) x^T -- and the record moves in its last bits
        os.environ["PIO_KV_FOLD"] = "0"
        try:
            _, rec_unfolded, _, _ = run(4)
        finally:
            del os.environ["PIO_KV_FOLD"]
        print(f"{name}: un-folded record {rec_unfolded[0]:.6f}")
        assert rec_unfolded[0] != rec[0] and abs(rec_unfolded[0] - ref) / unit <= SINGLE_SWEEP_TOL_UNITS
    # calls past max_records are counted, not recorded
    _, rec1, calls1, _ = run(1)
    assert calls1 == 1 and rec1[0] == rec[0]
    tol = SPLIT_TOL_UNITS if policy in SPLIT_OPERAND else SINGLE_SWEEP_TOL_UNITS
    assert gap <= tol, (name, rec[0], ref, gap, tol)


def test_records_past_max_records_are_counted_not_written(dev):
    """Two attention calls with max_records = 1: pio_logit_probe_end returns 2, the second record stays zero."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    torch.manual_seed(5)
    m = Attention(32, 32, 32, num_heads=2).to(dev).eval()
    x = torch.randn(1, 24, 32, device=dev)
    lib = P.lib()
    rec = torch.zeros(4, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    L.check(lib.pio_logit_probe_begin(rec.data_ptr(), 1), "pio_logit_probe_begin")
    try:
        y1, y2 = m(x, x, x), m(x, x, x)
    finally:
        n = lib.pio_logit_probe_end()
    torch.cuda.synchronize()
    vals = rec.cpu().tolist()
    assert n == 2 and vals[0] > 0 and vals[1:] == [0.0, 0.0, 0.0] and torch.equal(y1, y2)


def test_python_api_labels_and_capture_guard(dev):
    """logit_probe() on the HIP backend: labels of a small PerceiverIO (L = 2, 2 blocks) and of a raw module, outputs
    bit-identical with the probe on and off, and entering during stream capture raises."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd.output_queries import TrainableQuery
    from perceiverio_pytorch_amd.perceiver import PerceiverIO
    from perceiverio_pytorch_amd.transformer_primitives import SelfAttention
    torch.manual_seed(2)
    model = PerceiverIO(num_blocks=2, num_self_attends_per_block=2, num_latents=64, num_latent_channels=128,
                        input_channels=48, final_project_out_channels=5,
                        perceiver_encoder_kwargs=dict(num_self_attend_heads=4, num_cross_attend_heads=1),
                        output_queries=TrainableQuery(output_index_dims=10, num_channels=128)).to(dev).eval()
    sa = SelfAttention(128, num_heads=4).to(dev).eval()
    x = torch.randn(2, 150, 48, device=dev)
    y0 = model(x)
    with P.logit_probe() as probe:
        y1 = model(x)
        sa(y1.new_zeros(1, 8, 128))
    assert [p for p, _ in probe.records] == ["cross"] + 4 * ["stack"] + ["decoder", "attention"] and probe.calls == 7
    assert all(np.isfinite(v) for _, v in probe.records) and all(v > 0 for _, v in probe.records[:6])
    assert torch.equal(y0, y1) and torch.equal(y0, model(x))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        model(x)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        with pytest.raises(P.PioError, match="stream capture"):
            with P.logit_probe():
                pass
        model(x)
    from perceiverio_pytorch_amd import probe as LP
    assert not LP.active() and P.lib().pio_logit_probe_end() == 0


@pytest.mark.parametrize("name", ["model_language_trained", "model_language"])
def test_recommendation_on_the_language_goldens(dev, name):
    """With the SHIPPED default threshold (profiles/logit_probe.json: the goldens separate, 49.6 against 63.2):
    model_language_trained gets at least one part turned into "fp16x3fq", model_language keeps the class default."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import models as M, probe as LP
    from cases import MODEL_CASES, gen_state_dict, model_inputs, model_seed, model_stats
    from _golden import load
    g = load(name)
    spec = [(str(n), tuple(int(d) for d in str(s).split(",") if d != "")) for n, s in zip(g["spec_names"], g["spec_shapes"])]
    model = getattr(M, MODEL_CASES[name]["cls"])(**dict(MODEL_CASES[name]["kw"]))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in
                           gen_state_dict(spec, model_seed(name), model_stats(name)).items()}, strict=True)
    model = model.to(dev).eval()
    ins = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]
    default = M.DEFAULT_POLICY["LanguagePerceiver"]
    assert model.precision_policy == default and LP.DEFAULT_THRESHOLD is not None
    policy, report = P.recommend_precision_policy(model, ins[0], ins[1])
    print(f"{name}: {report['absmax']} threshold {report['threshold']} -> {policy}")
    assert report["threshold"] == LP.DEFAULT_THRESHOLD and report["calls"] == 28 and model.precision_policy == default
    parts = policy.split("/")
    if name == "model_language_trained":
        assert len(parts) == 3 and "fp16x3fq" in parts
        assert all(p == "fp16x3fq" or p == d for p, d in zip(parts, default.split("/")))
    else:
        assert policy == default
