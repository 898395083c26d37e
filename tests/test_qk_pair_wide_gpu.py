"""GPU: pair-operand Q.K^T on the 128-wide head of the self-attention core (policy "fp16x3fq" in the classifier's latent
stack) -- the raw kernel against the float64 oracle on the cases tests/test_qk_pair_wide_host.py selects, the refusals
that stay, the SelfAttention block and the Attention module at 8 heads of (128, 128) with launch accounting, and the
ClassificationPerceiver goldens under "fp16x2w/fp16x3fq/fp16x2af"."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import perceiver_oracle as O
from cases import MODEL_CASES, gen_state_dict, model_inputs, model_seed, model_stats
from _golden import load

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qk_pair_wide_cases as WC  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-3
GUARD = 2                                   # NaN rows behind Tq of the last sample that no launch may touch
POLICY = "fp16x2w/fp16x3fq/fp16x2af"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _pair16(a, dev):
    hi = a.astype(np.float16)
    lo = (a - hi.astype(np.float32)).astype(np.float16)
    return _t(hi, dev), _t(lo, dev)


def _run_core(dev, name, q, k, v, pair, entry="pair", cu_budget=0):
    """One raw launch on core 1 (flash_attn_kernel).  entry "pair": pio_flash_attention_pair (pair=False: Q_lo = K_lo =
    O_lo = NULL, the single-operand sibling); entry "flash": pio_flash_attention on the hi halves.  cu_budget: the value of
    the library's A/B switch pio_set_cu_budget around the launch (1: flash_route never splits the keys).  O and O_lo are
    NaN-prefilled with GUARD rows behind the last sample's Tq; returns (O, O_lo or None) as float64 [B, Tq, H*dv] after
    checking that the guard rows are still NaN."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L
    lib = P.lib()
    c = WC.CASES[name]
    B, H, Tq, Tk, dk, dv = c["B"], c["H"], c["Tq"], c["Tk"], WC.DK, WC.DV
    tkv = (Tk + 31) // 32 * 32
    qh, ql = _pair16(q, dev)
    kh, kl = _pair16(k, dev)
    vrow = 1 if c["vrow"] else 0
    if vrow:                                       # V row-major [B][Tk][H*dv]
        vt = _t(v.astype(np.float16), dev)
    else:                                          # V^T [B][H*dv][keys], zero-filled to whole 32-key tiles
        vt = np.zeros((B, H * dv, tkv), np.float16)
        vt[:, :, :Tk] = v.astype(np.float16).transpose(0, 2, 1)
        vt = _t(vt, dev)
    ldq, ldo = H * dk, H * dv
    o = torch.full((B * Tq + GUARD, ldo), float("nan"), dtype=torch.float16, device=dev)
    olo = torch.full_like(o, float("nan"))
    strides = (ldq, ldq, ldo if vrow else tkv, ldo, Tq * ldq, Tk * ldq, Tk * ldo if vrow else H * dv * tkv, Tq * ldo)
    s = torch.cuda.current_stream(dev).cuda_stream
    prev = lib.pio_set_cu_budget(cu_budget)
    try:
        if entry == "flash":
            L.check(lib.pio_flash_attention(L.PIO_DT_F16, dk, dv, dk, qh.data_ptr(), kh.data_ptr(), vt.data_ptr(),
                                            o.data_ptr(), B, H, Tq, Tk, *strides, vrow, s), "pio_flash_attention")
        else:
            L.check(lib.pio_flash_attention_pair(L.PIO_DT_F16, dk, dv, dk, qh.data_ptr(), ql.data_ptr() if pair else None,
                                                 kh.data_ptr(), kl.data_ptr() if pair else None, vt.data_ptr(),
                                                 o.data_ptr(), olo.data_ptr() if pair else None, B, H, Tq, Tk, *strides,
                                                 vrow, None, None, 1, None, 0, s), "pio_flash_attention_pair")
    finally:
        lib.pio_set_cu_budget(prev)
    torch.cuda.synchronize()
    assert torch.isnan(o[B * Tq:]).all() and torch.isnan(olo[B * Tq:]).all(), "rows behind Tq were written"
    if not pair:
        assert torch.isnan(olo).all()
    y = o[:B * Tq].double().cpu().numpy().reshape(B, Tq, ldo)
    return y, (olo[:B * Tq].double().cpu().numpy().reshape(B, Tq, ldo) if pair else None)


@pytest.mark.parametrize("name", sorted(WC.CASES))
def test_raw_wide_pair_core_vs_oracle(dev, name):
    """The pair instantiations of flash_attn_kernel<128, 128> -- (V^T, 4 waves), (row-major V, 4 waves), (row-major V, 8
    waves) -- against the float64 oracle; the single-operand core on the hi halves of the same inputs must miss TOL (the
    case's teeth).
    The small-logit leg compares the pair core with the single-operand instantiation of the SAME kernel variant.  For
    every case but one, flash_route and flash_pair_route name the same variant anyway.  For w128_rm_256 the single-operand
    launch would split the keys over two wave groups (two independent online softmaxes, merged in fp32), which the pair
    launch cannot; the test holds the CU budget at 1 around the single-operand launch, under which flash_route never splits
    (for the other cases the output is bit-identical with and without it).  Measured on the MI355X, small-logit relL2:
    pair 2.2156e-4, single-operand un-split 2.2292e-4, single-operand key-split 2.2141e-4 -- the split kernel rounds p
    against two maxima and differs from BOTH un-split kernels by more than they differ from each other; on the six cases the
    pair core is 0.3 - 0.6 % below its own single-operand variant.  The key-split figure is printed, and the one-element
    figure is held against it too."""
    q, k, v, ref, smax = WC.oracle(name)
    y, ylo = _run_core(dev, name, q, k, v, pair=True)
    y2, ylo2 = _run_core(dev, name, q, k, v, pair=True)
    ys, _ = _run_core(dev, name, q, k, v, pair=False)                     # the same entry with Q_lo = K_lo = NULL
    yf, _ = _run_core(dev, name, q, k, v, pair=False, entry="flash")     # the pre-existing single-operand entry
    ep, es, ef = O.rel_errors(y, ref), O.rel_errors(ys, ref), O.rel_errors(yf, ref)
    epl = O.rel_errors(y + ylo, ref)
    print(f"{name}: max|s|={smax:.2f} pair {ep[0]:.3e} / {ep[1]:.3e} (hi + lo: {epl[0]:.3e} / {epl[1]:.3e}) "
          f"single {es[0]:.3e} / {es[1]:.3e} (pio_flash_attention: {ef[0]:.3e} / {ef[1]:.3e})")
    assert np.isfinite(y).all() and np.isfinite(ylo).all() and np.isfinite(ys).all() and np.isfinite(yf).all()
    assert np.array_equal(y, y2) and np.array_equal(ylo, ylo2), "two runs must be bit-identical"
    assert max(ep) <= TOL, (name, ep)
    assert max(epl) <= TOL, (name, epl)
    assert max(es) > TOL and max(ef) > TOL, f"{name}: the single-operand core passes ({es}, {ef}): the case has no teeth"
    # small logits (|s| <= 1): the pair core is no worse than the single core on the same inputs -- relL2 compared, the
    # one-element figure held to the half-ulp scale of the fp16 output (tests/test_qk_pair_gpu.py says why)
    q, k, v, ref, smax = WC.oracle(name, small=True)
    assert smax <= 1.0
    y, _ = _run_core(dev, name, q, k, v, pair=True)
    ys, _ = _run_core(dev, name, q, k, v, pair=False, entry="flash", cu_budget=1)    # the pair launch's variant
    yr, _ = _run_core(dev, name, q, k, v, pair=False, entry="flash")                 # as flash_route picks it
    ep, es, er = O.rel_errors(y, ref), O.rel_errors(ys, ref), O.rel_errors(yr, ref)
    print(f"{name} small logits: max|s|={smax:.2f} pair {ep[0]:.4e} / {ep[1]:.3e} single {es[0]:.4e} / {es[1]:.3e} "
          f"(single as routed: {er[0]:.4e} / {er[1]:.3e})")
    assert ep[0] <= es[0], (name, ep, es)
    assert ep[1] <= es[1] + 2.0 ** -11, (name, ep, es)
    assert ep[1] <= er[1] + 2.0 ** -11, (name, ep, er)


def test_refusals_kept_and_outputs_untouched(dev):
    """No bf16 pair core and no cross-attention pair core at 128: PIO_E_SHAPE, nothing launched, O / O_lo as they were."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L
    lib = P.lib()
    z = torch.zeros(1 << 16, dtype=torch.float16, device=dev)
    o = torch.full((64, 128), float("nan"), dtype=torch.float16, device=dev)
    olo = torch.full_like(o, float("nan"))
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    p = z.data_ptr()
    args = lambda dt, core: (dt, 128, 128, 128, p, p, p, p, p, o.data_ptr(), olo.data_ptr(), 1, 1, 64, 64, 128, 128, 64,  # noqa: E731
                             128, 64 * 128, 64 * 128, 128 * 64, 64 * 128, 0, None, None, core, ws.data_ptr(), ws.numel(), 0)
    assert lib.pio_flash_attention_pair(*args(L.PIO_DT_BF16, 1)) == -1       # PIO_E_SHAPE
    assert lib.pio_flash_attention_pair(*args(L.PIO_DT_F16, 2)) == -1
    torch.cuda.synchronize()
    assert torch.isnan(o).all() and torch.isnan(olo).all()


def _trained_ln(p, rng):
    """LayerNorm statistics of oracle/cases.py stats="trained", re-derived: gains log-uniform in [0.2, 5], biases N(0, 0.3)."""
    for k in p:
        if "layer_norm" in k:
            n = p[k].shape
            p[k] = (np.exp(rng.uniform(np.log(0.2), np.log(5.0), n)) if k.endswith("weight")
                    else 0.3 * rng.standard_normal(n)).astype(np.float32)
    return p


def _profiled(lib, fn, max_records=256):
    """fn() between pio_prof_begin / pio_prof_end: launches per profiler class (5 = fused attention cores, 3 = softmax_rows
    of the materialised path)."""
    from perceiverio_pytorch_amd import _lib as L
    L.check(lib.pio_prof_begin(max_records), "pio_prof_begin")
    try:
        fn()
    finally:
        launches = (C.c_int64 * 9)()
        n = lib.pio_prof_end(None, None, None, launches)
    assert 0 <= n < max_records
    torch.cuda.synchronize()
    return list(launches)


def test_self_attention_block_wide_heads_under_fp16x3fq(dev):
    """SelfAttention at the classifier stack's widths (1024 channels, 8 heads of (128, 128)) through pio_self_attention_fwd,
    LayerNorm gains up to 5: one fused core -- the pair flash_attn_kernel<128, 128> -- and no softmax_rows launch; with a
    key mask the block stays on the materialised split-operand path (no pair core takes mask vectors at this width)."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import SelfAttention
    D, H, B, N = 1024, 8, 2, 256
    rng = np.random.default_rng(78)
    p = _trained_ln(O.gen_self_attention("", D, seed=78, widening=1), rng)
    x = rng.standard_normal((B, N, D)).astype(np.float32)
    km = rng.random((B, N)) > 0.3
    km[:, 0] = True
    m = SelfAttention(D, widening_factor=1, num_heads=H)
    m.load_state_dict({k: torch.from_numpy(a) for k, a in p.items()}, strict=True)
    m = m.to(dev).eval()
    p64 = {k: a.astype(np.float64) for k, a in p.items()}
    ref = O.self_attention(p64, x.astype(np.float64), H)
    ref_m = O.self_attention(p64, x.astype(np.float64), H, np.broadcast_to(km[:, None, :], (B, N, N)))
    lib = P.lib()
    prev = R.get_precision_policy()
    P.set_precision_policy("fp16x3fq")
    try:
        d = m._desc()
        assert d.attn.act_split == 3 and (d.attn.dkp, d.attn.dvp) == (128, 128)
        xt, kmt = _t(x, dev), _t(km, dev).view(torch.uint8)
        out, out_m = (torch.empty((B, N, D), dtype=torch.float32, device=dev) for _ in range(2))
        ws = R.workspace(dev, lib.pio_self_attention_workspace_bytes(d, B, N))
        launches = _profiled(lib, lambda: L.check(lib.pio_self_attention_fwd(
            d, R.tensor3(xt), None, None, None, None, out.data_ptr(), None, None, ws.data_ptr(), ws.numel(), R.stream_ptr(dev)),
            "pio_self_attention_fwd"))
        with torch.inference_mode():
            assert torch.equal(m(xt), out)                # the nn.Module front end runs the same call
        launches_m = _profiled(lib, lambda: L.check(lib.pio_self_attention_fwd(
            d, R.tensor3(xt), kmt.data_ptr(), None, None, None, out_m.data_ptr(), None, None, ws.data_ptr(), ws.numel(),
            R.stream_ptr(dev)), "pio_self_attention_fwd"))
    finally:
        P.set_precision_policy(prev)
    e, em = O.rel_errors(out.cpu().numpy(), ref), O.rel_errors(out_m.cpu().numpy(), ref_m)
    print(f"SelfAttention 1024 / 8 heads (128,128) [fp16x3fq]: relL2={e[0]:.3e} max/absmax={e[1]:.3e} fused-core "
          f"launches={launches[5]} softmax={launches[3]}; key mask: {em[0]:.3e} / {em[1]:.3e} fused={launches_m[5]} "
          f"softmax={launches_m[3]}")
    assert launches[5] == 1 and launches[3] == 0, "the pair core must run, and no materialised softmax"
    assert launches_m[5] == 0 and launches_m[3] >= 1, "a masked 128-wide pair request takes the materialised path"
    assert max(e) <= TOL, e
    assert max(em) <= TOL, em


def test_attention_module_wide_heads_under_fp16x3fq(dev):
    """Attention 1024 -> 8 heads of (128, 128), Tq = 256 != Tk = 384, no mask, trained-like input statistics: one fused
    launch (V^T form of the pair core), no softmax_rows."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, runtime as R
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    D, H, B, Tq, Tk = 1024, 8, 2, 256, 384
    p = O.gen_attention("", D, D, D, D, D, seed=79)
    rng = np.random.default_rng(80)
    gq = np.exp(rng.uniform(np.log(0.2), np.log(5.0), D)).astype(np.float32)
    gk = np.exp(rng.uniform(np.log(0.2), np.log(5.0), D)).astype(np.float32)
    xq = (rng.standard_normal((B, Tq, D)) * gq).astype(np.float32)
    xkv = (rng.standard_normal((B, Tk, D)) * gk).astype(np.float32)
    m = Attention(D, D, D, num_heads=H, qk_out_channels=D, v_out_channels=D, output_channels=D)
    m.load_state_dict({k: torch.from_numpy(a) for k, a in p.items()})
    m = m.to(dev).eval()
    p64 = {k: a.astype(np.float64) for k, a in p.items()}
    ref = O.attention(p64, xq.astype(np.float64), xkv.astype(np.float64), xkv.astype(np.float64), H, None)
    lib = P.lib()
    prev = R.get_precision_policy()
    P.set_precision_policy("fp16x3fq")
    try:
        d = m._desc()
        assert d.act_split == 3 and (d.dkp, d.dvp) == (128, 128)
        out = torch.empty((B, Tq, D), dtype=torch.float32, device=dev)
        ws = R.workspace(dev, lib.pio_attention_workspace_bytes(d, B, Tq, Tk))
        xq_t, xkv_t = _t(xq, dev), _t(xkv, dev)
        launches = _profiled(lib, lambda: L.check(lib.pio_attention_fwd(
            d, R.tensor3(xq_t), R.tensor3(xkv_t), R.tensor3(xkv_t), None, None, None, None, out.data_ptr(), None,
            ws.data_ptr(), ws.numel(), R.stream_ptr(dev)), "pio_attention_fwd"))
    finally:
        P.set_precision_policy(prev)
    e = O.rel_errors(out.cpu().numpy(), ref)
    print(f"Attention 1024 / 8 heads (128,128) 256 x 384 [fp16x3fq]: relL2={e[0]:.3e} max/absmax={e[1]:.3e} fused-core "
          f"launches={launches[5]} softmax={launches[3]}")
    assert launches[5] == 1 and launches[3] == 0
    assert max(e) <= TOL, e


def _classifier(name, dev):
    from perceiverio_pytorch_amd import models as M
    g = load(name)
    spec = [(str(n), tuple(int(d) for d in str(s).split(",") if d != "")) for n, s in zip(g["spec_names"], g["spec_shapes"])]
    kw = dict(MODEL_CASES[name]["kw"])
    model = M.ClassificationPerceiver(prep_type=M.PrepType[kw.pop("prep")])
    params = gen_state_dict(spec, model_seed(name), model_stats(name))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return model.to(dev).eval(), g


@pytest.mark.parametrize("name", ["model_classify_b4_trained1", "model_classify_b4_trained2", "model_classify_b4_s31"])
def test_classifier_goldens_with_the_pair_core_in_the_stack(dev, name):
    """ClassificationPerceiver under "fp16x2w/fp16x3fq/fp16x2af": the reference logits within TOL, every one of the 48 latent
    self-attends on the fused pair core (no softmax_rows launch in the whole forward); on trained1 also: the forward
    captured into a graph replays bit-identically, and the logit probe changes neither the output nor its record count."""
    import perceiverio_pytorch_amd as P
    model, g = _classifier(name, dev)
    x = torch.from_numpy(model_inputs(name)[0]).to(dev)
    model.precision_policy = POLICY
    lib = P.lib()
    with torch.inference_mode():
        model(x)                                              # (packs the weights for the policy)
        out = {}
        launches = _profiled(lib, lambda: out.__setitem__("y", model(x).clone()), max_records=8192)
        y = out["y"]
        e = O.rel_errors(y.float().cpu().numpy(), g["out"])
        print(f"{name} [{POLICY}]: relL2={e[0]:.3e} max/absmax={e[1]:.3e} fused-core launches={launches[5]} "
              f"softmax={launches[3]}")
        assert launches[3] == 0 and launches[5] >= 48, launches
        assert max(e) <= TOL, (name, e)
        if name != "model_classify_b4_trained1":
            return
        with P.logit_probe() as probe:
            yp = model(x)
        assert torch.equal(yp, y), "the logit probe must not change the output"
        labels = [part for part, _ in probe.records]
        assert probe.calls == 50 and labels == ["cross"] + 48 * ["stack"] + ["decoder"], (probe.calls, labels[:3])
        assert all(np.isfinite(v) and v > 0 for _, v in probe.records)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                model(x)
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            yg = model(x)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(yg, y), "graph replay must reproduce the eager output"
