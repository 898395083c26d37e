"""GPU: pair-operand Q.K^T in the fused attention cores (policy "fp16x3fq", pio_attention_t.act_split = 3) -- the raw
kernels of both families against the float64 oracle on the cases tests/test_qk_pair_host.py selects, the Attention module
with trained-like statistics, the fallback for a shape without a pair core, and the LanguagePerceiver goldens."""
import os
import sys

import numpy as np
import pytest
import torch

import perceiver_oracle as O
from cases import MODEL_CASES, gen_state_dict, model_inputs, model_seed, model_stats
from _golden import load

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qk_pair_cases as QC  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _pair16(a, dev, pad_rows=0):
    """fp32 [B,T,C] -> (hi, lo) fp16 device tensors, `pad_rows` readable zero rows behind the last sample."""
    hi = a.astype(np.float16)
    lo = (a - hi.astype(np.float32)).astype(np.float16)
    out = []
    for h in (hi, lo):
        flat = np.concatenate([h.reshape(-1, h.shape[-1]), np.zeros((pad_rows, h.shape[-1]), np.float16)])
        out.append(_t(flat, dev))
    return out


def _run_core(dev, name, q, k, v, km, qm, pair, entry="pair"):
    """One raw launch.  entry "pair": pio_flash_attention_pair (pair=False: Q_lo = K_lo = NULL, the single-operand sibling);
    entry "flash": the pre-existing pio_flash_attention on the hi halves.  Returns O (hi half, float64) and O_lo or None."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L
    lib = P.lib()
    c = QC.CASES[name]
    B, H, Tq, Tk, dv = c["B"], c["H"], c["Tq"], c["Tk"], c["dv"]
    tkv = (Tk + 31) // 32 * 32
    qh, ql = _pair16(q, dev)
    kh, kl = _pair16(k, dev, pad_rows=32)          # the cross-attention kernel reads whole 32-key tiles
    vrow = 1 if c.get("vrow") else 0
    if vrow:                                       # V row-major [B][Tk][H*dv]
        vt = _t(v.astype(np.float16), dev)
    else:                                          # V^T [B][H*dv][keys], zero-filled to whole 32-key tiles
        vt = np.zeros((B, H * dv, tkv), np.float16)
        vt[:, :, :Tk] = v.astype(np.float16).transpose(0, 2, 1)
        vt = _t(vt, dev)
    o = torch.full((B, Tq, H * dv), float("nan"), dtype=torch.float16, device=dev)
    olo = torch.full_like(o, float("nan"))
    ldq, ldo = H * QC.DK, H * dv
    strides = (ldq, ldq, ldo if vrow else tkv, ldo, Tq * ldq, Tk * ldq, Tk * ldo if vrow else H * dv * tkv, Tq * ldo)
    s = torch.cuda.current_stream(dev).cuda_stream
    if entry == "flash":
        L.check(lib.pio_flash_attention(L.PIO_DT_F16, QC.DK, dv, QC.DK, qh.data_ptr(), kh.data_ptr(), vt.data_ptr(),
                                        o.data_ptr(), B, H, Tq, Tk, *strides, vrow, s), "pio_flash_attention")
        torch.cuda.synchronize()
        return o.double().cpu().numpy(), None
    kmt = _t(km, dev).view(torch.uint8) if km is not None else None
    qmt = _t(qm, dev).view(torch.uint8) if qm is not None else None
    nb = lib.pio_flash_attention_pair_workspace_bytes(QC.DK, dv, B, H, Tq, Tk)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
    core = 1 if c["core"] == "flash" else 2
    want_lo = pair or core == 2
    L.check(lib.pio_flash_attention_pair(L.PIO_DT_F16, QC.DK, dv, QC.DK, qh.data_ptr(), ql.data_ptr() if pair else None,
                                         kh.data_ptr(), kl.data_ptr() if pair else None, vt.data_ptr(), o.data_ptr(),
                                         olo.data_ptr() if want_lo else None, B, H, Tq, Tk, *strides, vrow,
                                         kmt.data_ptr() if kmt is not None else None,
                                         qmt.data_ptr() if qmt is not None else None, core, ws.data_ptr(), ws.numel(), s),
            "pio_flash_attention_pair")
    torch.cuda.synchronize()
    return o.double().cpu().numpy(), (olo.double().cpu().numpy() if want_lo else None)


@pytest.mark.parametrize("name", sorted(QC.CASES))
def test_raw_pair_cores_vs_oracle(dev, name):
    """Step 4 of the issue.  Figures (relL2, max-abs / abs-max) against the float64 oracle; measured on the MI355X:
    see profiles/qk_pair.json "raw_core_errors"."""
    c = QC.CASES[name]
    q, k, v, km, qm = QC.gen(name)
    ref, smax = QC.oracle(name, q, k, v, km, qm)
    y, ylo = _run_core(dev, name, q, k, v, km, qm, pair=True)
    y2, ylo2 = _run_core(dev, name, q, k, v, km, qm, pair=True)
    # the single-operand core on the hi halves of the same inputs: the PRE-EXISTING entry point for the self-attention
    # kernel; the cross-attention kernel had no raw entry point before, its single-operand instantiation is reached with
    # Q_lo = K_lo = NULL
    ys, _ = (_run_core(dev, name, q, k, v, km, qm, pair=False, entry="flash") if c["core"] == "flash"
             else _run_core(dev, name, q, k, v, km, qm, pair=False))
    ep, es = O.rel_errors(y, ref), O.rel_errors(ys, ref)
    epl = O.rel_errors(y + ylo, ref)
    print(f"{name}: max|s|={smax:.2f} pair {ep[0]:.3e} / {ep[1]:.3e} (hi + lo: {epl[0]:.3e} / {epl[1]:.3e}) "
          f"single {es[0]:.3e} / {es[1]:.3e}")
    assert np.isfinite(y).all() and np.isfinite(ylo).all() and np.isfinite(ys).all()
    assert np.array_equal(y, y2) and np.array_equal(ylo, ylo2), "two runs must be bit-identical"
    m3 = QC.mask3(name, km, qm)
    if m3 is not None:
        dead = ~m3.any(axis=2)                              # rows without an attendable key / with query mask 0
        assert dead.any() and (y[dead] == 0).all() and (ylo[dead] == 0).all(), "masked rows must be exactly zero"
    assert max(ep) <= TOL, (name, ep)
    if name not in QC.NO_TEETH:             # the issue's MUST_FAIL shapes and every other selected case
        assert max(es) > TOL, f"{name}: the single-operand core passes ({es}): the case has no teeth"
    # small logits (|s| <= 1): the pair core is no worse than the single core on the same inputs
    q, k, v, km, qm = QC.gen(name, small=True)
    ref, smax = QC.oracle(name, q, k, v, km, qm)
    assert smax <= 1.0
    y, _ = _run_core(dev, name, q, k, v, km, qm, pair=True)
    ys, _ = (_run_core(dev, name, q, k, v, km, qm, pair=False, entry="flash") if c["core"] == "flash"
             else _run_core(dev, name, q, k, v, km, qm, pair=False))
    ep, es = O.rel_errors(y, ref), O.rel_errors(ys, ref)
    print(f"{name} small logits: max|s|={smax:.2f} pair {ep[0]:.3e} / {ep[1]:.3e} single {es[0]:.3e} / {es[1]:.3e}")
    # Asserted on relL2.  The second figure is the error of ONE output element -- the extreme of ~10^5 rounding
    # realisations of p, v and o, which the two cores share in distribution but not element by element (another S changes
    # which way individual p round): at |s| <= 1 the q / k rounding is ~1e-5 of that element's error, so which core's
    # extreme element is larger is a coin toss (measured: pair larger on 2 of 7 cases, by <= 2 %).  It is held to the
    # half-ulp scale of the fp16 output instead: the two maxima differ by less than 2^-11 of the abs-max.
    assert ep[0] <= es[0], (name, ep, es)
    assert ep[1] <= es[1] + 2.0 ** -11, (name, ep, es)


def test_pair_request_without_a_pair_core_is_an_error_not_a_single_operand_run(dev):
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L
    lib = P.lib()
    z = torch.zeros(1 << 16, dtype=torch.float16, device=dev)
    p = z.data_ptr()
    args = lambda dt, dk, dv, core: (dt, dk, dv, dk, p, p, p, p, p, p, p, 1, 1, 64, 64, dk, dk, 64, dv, 64 * dk, 64 * dk,  # noqa: E731
                                     dv * 64, 64 * dv, 0, None, None, core, p, 1 << 16, 0)
    assert lib.pio_flash_attention_pair(*args(L.PIO_DT_BF16, 32, 32, 1)) == -1       # PIO_E_SHAPE: no bf16 pair core
    assert lib.pio_flash_attention_pair(*args(L.PIO_DT_BF16, 32, 96, 2)) == -1
    assert lib.pio_flash_attention_pair(*args(L.PIO_DT_F16, 64, 64, 1)) == -1        # dk = 64: no pair instantiation
    assert lib.pio_flash_attention_pair(*args(L.PIO_DT_F16, 128, 128, 2)) == -1


def _trained_attention(q_in, kv_in, H, qk, vv, outc, seed):
    """Attention parameters + inputs with trained-like statistics, re-derived from oracle/cases.py stats="trained": the
    inputs are what LayerNorms with gains drawn up to 5 deliver."""
    p = O.gen_attention("", q_in, kv_in, qk, vv, outc, seed=seed)
    r = np.random.default_rng(seed + 1)
    gq = np.exp(r.uniform(np.log(0.2), np.log(5.0), q_in)).astype(np.float32)
    gk = np.exp(r.uniform(np.log(0.2), np.log(5.0), kv_in)).astype(np.float32)
    return p, gq, gk


ATTN_CASES = [
    # q_in, kv_in, heads, qk, v, out, B, Tq, Tk, mask, what
    (1280, 768, 8, 256, 1280, 1280, 2, 256, 2048, "key", "language-encoder cross xattn<32,160>"),
    (1280, 1280, 8, 256, 1280, 1280, 2, 256, 256, None, "language-stack self flash<32,160>"),
    (768, 1280, 8, 256, 768, 768, 2, 2048, 256, "query", "language-decoder cross xattn<32,96>"),
    (512, 512, 1, 512, 512, 512, 2, 384, 1024, None, "wide single head: no pair core, materialised fallback"),
]


@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[-1].split(":")[0].replace(" ", "-") for c in ATTN_CASES])
def test_attention_module_trained_like_under_fp16x3fq(dev, case):
    """Step 5 (Attention at the language widths + the wide single head).  The fallback is checked with the library's
    pio_prof_begin / pio_prof_end launch accounting: class 5 counts the fused attention kernels -- none may run for the
    wide head, exactly one for the others."""
    import ctypes as C
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    q_in, kv_in, H, qk, vv, outc, B, Tq, Tk, mk, what = case
    p, gq, gk = _trained_attention(q_in, kv_in, H, qk, vv, outc, q_in + Tk)
    rng = np.random.default_rng(Tq + kv_in)
    xq = (rng.standard_normal((B, Tq, q_in)) * gq).astype(np.float32)
    xkv = (rng.standard_normal((B, Tk, kv_in)) * gk).astype(np.float32)
    km = qm = mask3 = None
    if mk == "key":
        km = rng.random((B, Tk)) > 0.3
        km[:, 0] = True
    elif mk == "query":
        qm = rng.random((B, Tq)) > 0.3
    if mk:
        mask3 = O.make_cross_attention_mask(qm if qm is not None else np.ones((B, Tq), bool),
                                            km if km is not None else np.ones((B, Tk), bool))
    m = Attention(q_in, kv_in, kv_in, num_heads=H, qk_out_channels=qk, v_out_channels=vv, output_channels=outc)
    m.load_state_dict({k: torch.from_numpy(a) for k, a in p.items()})
    m = m.to(dev).eval()
    p64 = {k: a.astype(np.float64) for k, a in p.items()}
    ref = O.attention(p64, xq.astype(np.float64), xkv.astype(np.float64), xkv.astype(np.float64), H, mask3)
    lib = P.lib()
    prev = R.get_precision_policy()
    P.set_precision_policy("fp16x3fq")
    try:
        d = m._desc()
        assert d.act_split == 3
        out = torch.empty((B, Tq, outc), dtype=torch.float32, device=dev)
        ws = R.workspace(dev, lib.pio_attention_workspace_bytes(d, B, Tq, Tk))
        kmt = _t(km, dev).view(torch.uint8) if km is not None else None
        qmt = _t(qm, dev).view(torch.uint8) if qm is not None else None
        xq_t, xkv_t = _t(xq, dev), _t(xkv, dev)
        L.check(lib.pio_prof_begin(64), "pio_prof_begin")
        L.check(lib.pio_attention_fwd(d, R.tensor3(xq_t), R.tensor3(xkv_t), R.tensor3(xkv_t),
                                      kmt.data_ptr() if kmt is not None else None,
                                      qmt.data_ptr() if qmt is not None else None, None, None, out.data_ptr(), None,
                                      ws.data_ptr(), ws.numel(), R.stream_ptr(dev)), "pio_attention_fwd")
        launches = (C.c_int64 * 9)()
        assert lib.pio_prof_end(None, None, None, launches) >= 0
        torch.cuda.synchronize()
    finally:
        P.set_precision_policy(prev)
    e = O.rel_errors(out.cpu().numpy(), ref)
    print(f"{what} [fp16x3fq]: relL2={e[0]:.3e} max/absmax={e[1]:.3e} fused-core launches={launches[5]} "
          f"batched score GEMMs={launches[1]} softmax={launches[3]}")
    if H == 1:
        assert launches[5] == 0 and launches[3] >= 1, "a shape without a pair core must take the materialised path"
    else:
        assert launches[5] == 1 and launches[3] == 0
    assert max(e) <= TOL, (what, e)


def _trained_ln(p, rng):
    """LayerNorm statistics of oracle/cases.py stats="trained", re-derived: gains log-uniform in [0.2, 5], biases N(0, 0.3)."""
    for k in p:
        if "layer_norm" in k:
            n = p[k].shape
            p[k] = (np.exp(rng.uniform(np.log(0.2), np.log(5.0), n)) if k.endswith("weight")
                    else 0.3 * rng.standard_normal(n)).astype(np.float32)
    return p


def _profiled(lib, fn):
    """fn() between pio_prof_begin / pio_prof_end: launches per profiler class (5 = fused attention cores, 3 = softmax_rows
    of the materialised path, 1 = batched GEMMs)."""
    import ctypes as C
    from perceiverio_pytorch_amd import _lib as L
    L.check(lib.pio_prof_begin(256), "pio_prof_begin")
    try:
        fn()
    finally:
        launches = (C.c_int64 * 9)()
        assert lib.pio_prof_end(None, None, None, launches) >= 0
    torch.cuda.synchronize()
    return list(launches)


def _check_block(what, out, ref, launches, wide):
    e = O.rel_errors(out.cpu().numpy(), ref)
    print(f"{what} [fp16x3fq]: relL2={e[0]:.3e} max/absmax={e[1]:.3e} fused-core launches={launches[5]} "
          f"softmax={launches[3]}")
    if wide:
        assert launches[5] == 0 and launches[3] >= 1, "a shape without a pair core must take the materialised path"
    else:
        assert launches[5] == 1 and launches[3] == 0, "the pair core must run, and no materialised softmax"
    assert max(e) <= TOL, (what, e)


def test_self_attention_block_trained_like_under_fp16x3fq(dev):
    """Step 5: SelfAttention at the language stack's widths (1280 channels, 8 heads, qk 256: heads of (32, 160)) through
    pio_self_attention_fwd, LayerNorm gains up to 5.  Launch accounting (pio_prof_begin / pio_prof_end): one fused core --
    the pair flash_attn_kernel -- and no softmax_rows launch."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import SelfAttention
    D, H, B, N = 1280, 8, 2, 256
    rng = np.random.default_rng(77)
    p = _trained_ln(O.gen_self_attention("", D, seed=77, widening=1, qk=256, v=D), rng)
    x = rng.standard_normal((B, N, D)).astype(np.float32)
    m = SelfAttention(D, widening_factor=1, num_heads=H, qk_channels=256, v_channels=D)
    m.load_state_dict({k: torch.from_numpy(a) for k, a in p.items()}, strict=True)
    m = m.to(dev).eval()
    ref = O.self_attention({k: a.astype(np.float64) for k, a in p.items()}, x.astype(np.float64), H)
    lib = P.lib()
    prev = R.get_precision_policy()
    P.set_precision_policy("fp16x3fq")
    try:
        d = m._desc()
        assert d.attn.act_split == 3
        xt = _t(x, dev)
        out = torch.empty((B, N, D), dtype=torch.float32, device=dev)
        ws = R.workspace(dev, lib.pio_self_attention_workspace_bytes(d, B, N))
        launches = _profiled(lib, lambda: L.check(lib.pio_self_attention_fwd(
            d, R.tensor3(xt), None, None, None, None, out.data_ptr(), None, None, ws.data_ptr(), ws.numel(), R.stream_ptr(dev)),
            "pio_self_attention_fwd"))
        with torch.inference_mode():
            assert torch.equal(m(xt), out)                # the nn.Module front end runs the same call
    finally:
        P.set_precision_policy(prev)
    _check_block("SelfAttention 1280 / 8 heads (32,160)", out, ref, launches, wide=False)


CROSS_CASES = [
    # q_in, kv_in, heads, qk, v, B, Tq, Tk, mask vector, query residual, batch-invariant queries, what
    (1280, 768, 8, 256, 1280, 2, 256, 2048, "key", True, True, "language-encoder xattn<32,160> key mask, broadcast latents"),
    (768, 1280, 8, 256, 768, 2, 2048, 256, "query", False, False, "language-decoder xattn<32,96> query mask"),
    (512, 512, 1, 512, 512, 2, 384, 1024, None, True, False, "wide single head: no pair core, materialised fallback"),
]


@pytest.mark.parametrize("case", CROSS_CASES, ids=[c[-1].split(" ")[0] + ("-wide" if c[2] == 1 else "") for c in CROSS_CASES])
def test_cross_attention_block_trained_like_under_fp16x3fq(dev, case):
    """Step 5: CrossAttention at the language encoder / decoder widths with the mask VECTORS the encoder / decoder pass
    (pio_cross_attention_fwd), LayerNorm gains up to 5, and a wide single-head CrossAttention, for which no fused core
    may run (launch accounting as above: class 5 == 0, softmax_rows >= 1) and the result must still meet TOL."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import CrossAttention
    q_in, kv_in, H, qk, vv, B, Tq, Tk, mk, resid, bcast, what = case
    rng = np.random.default_rng(q_in + Tk)
    p = _trained_ln(O.gen_cross_attention("", q_in, kv_in, seed=q_in + Tk, widening=1, qk=qk, v=vv), rng)
    xq = rng.standard_normal((1 if bcast else B, Tq, q_in)).astype(np.float32)
    xkv = rng.standard_normal((B, Tk, kv_in)).astype(np.float32)
    km = qm = mask3 = None
    if mk == "key":
        km = rng.random((B, Tk)) > 0.3
        km[:, 0] = True
    elif mk == "query":
        qm = rng.random((B, Tq)) > 0.3
    if mk:
        mask3 = O.make_cross_attention_mask(qm if qm is not None else np.ones((B, Tq), bool),
                                            km if km is not None else np.ones((B, Tk), bool))
    m = CrossAttention(q_in, kv_in, widening_factor=1, num_heads=H, use_query_residual=resid, qk_channels=qk,
                       v_channels=vv)
    m.load_state_dict({k: torch.from_numpy(a) for k, a in p.items()}, strict=True)
    m = m.to(dev).eval()
    xq_full = np.broadcast_to(xq, (B, Tq, q_in))
    ref = O.cross_attention({k: a.astype(np.float64) for k, a in p.items()}, xq_full.astype(np.float64),
                            xkv.astype(np.float64), H, resid, mask3)
    lib = P.lib()
    prev = R.get_precision_policy()
    P.set_precision_policy("fp16x3fq")
    try:
        d = m._desc()
        assert d.attn.act_split == 3
        xq_t, xkv_t = _t(xq, dev), _t(xkv, dev)
        if bcast:
            xq_t = torch.broadcast_to(xq_t, (B, Tq, q_in))       # stride_b = 0: projected once (q_bcast)
        kmt = _t(km, dev).view(torch.uint8) if km is not None else None
        qmt = _t(qm, dev).view(torch.uint8) if qm is not None else None
        out = torch.empty((B, Tq, q_in), dtype=torch.float32, device=dev)
        ws = R.workspace(dev, lib.pio_cross_attention_workspace_bytes(d, B, Tq, Tk))
        launches = _profiled(lib, lambda: L.check(lib.pio_cross_attention_fwd(
            d, R.tensor3(xq_t), R.tensor3(xkv_t), kmt.data_ptr() if kmt is not None else None,
            qmt.data_ptr() if qmt is not None else None, None, None, out.data_ptr(), None, ws.data_ptr(), ws.numel(),
            R.stream_ptr(dev)), "pio_cross_attention_fwd"))
    finally:
        P.set_precision_policy(prev)
    _check_block(what, out, ref, launches, wide=H == 1)


def _build(name):
    from perceiverio_pytorch_amd import models as M
    return getattr(M, MODEL_CASES[name]["cls"])(**dict(MODEL_CASES[name]["kw"]))


def _spec(g):
    return [(str(n), tuple(int(d) for d in str(s).split(",") if d != "")) for n, s in zip(g["spec_names"], g["spec_shapes"])]


def _lang_errs(out, g):
    def fig(y, ref):
        d = y.detach().float().cpu().numpy().astype(np.float64) - ref.astype(np.float64)
        return (float(np.sqrt((d * d).sum()) / np.sqrt((ref.astype(np.float64) ** 2).sum())),
                float(np.abs(d).max() / float(g["out_absmax"])))
    a, b = fig(out[:, :96], g["out"]), fig(out[:, 640:704], g["out_tail"])
    return max(a[0], b[0]), max(a[1], b[1])


@pytest.mark.parametrize("name", ["model_language_trained", "model_language", "model_language_s32", "model_language_s33"])
def test_language_goldens_under_fp16x3fq(dev, name):
    """Step 6.  model_language_trained: "fp16x3fq" in all three parts must meet TOL, "fp16x3f" in all three must NOT (the
    recorded known limit 2.6e-3 / 4.1e-3) -- otherwise this feature is not what fixes the golden."""
    g = load(name)
    params = gen_state_dict(_spec(g), model_seed(name), model_stats(name))
    model = _build(name)
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    model.load_state_dict(sd, strict=True)
    back = model.state_dict()
    assert set(back) == set(sd)
    twin = _build(name)                                   # strict round trip: what the model gives back loads again
    twin.load_state_dict(back, strict=True)
    assert all(torch.equal(v, back[k]) for k, v in twin.state_dict().items())
    del twin
    model = model.to(dev).eval()
    ins = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]
    model.precision_policy = "fp16x3fq/fp16x3fq/fp16x3fq"
    with torch.inference_mode():
        y = model(ins[0], ins[1]).clone()
        e = _lang_errs(y, g)
        print(f"{name} [fp16x3fq]: relL2={e[0]:.3e} max/absmax={e[1]:.3e}")
        if name == "model_language_trained":
            model.precision_policy = "fp16x3f/fp16x3f/fp16x3f"
            e0 = _lang_errs(model(ins[0], ins[1]), g)
            print(f"{name} [fp16x3f]: relL2={e0[0]:.3e} max/absmax={e0[1]:.3e}")
            assert max(e0) > TOL, f"fp16x3f already meets the bar on {name} ({e0}): pair Q.K^T is NOT what fixes it"
            model.precision_policy = "fp16x3fq/fp16x3fq/fp16x3fq"
        assert max(e) <= TOL, (name, e)
        if name != "model_language_trained":
            return
        # the forward captures into a HIP graph and replays bit-identically (default queue count)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                model(ins[0], ins[1])
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            yg = model(ins[0], ins[1])
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(yg, y), "graph replay must reproduce the eager output"
