"""GPU: no result of a block entry point depends on what its workspace held on entry.

The hot path reuses one never-cleared scratch buffer per (device, stream) (runtime.workspace), so every production call
starts on the bytes an earlier, usually larger, call left: 16-bit activations, fp32 scores, key-bit words, key-split
partials.  Every case of tests/workspace_stale_cases.py -- one per (entry point, route) at ragged extents -- runs three
times through the raw C-ABI on exactly pio_*_workspace_bytes() bytes between two guard bands, the workspace pre-filled
with
  0x00  the baseline the rest of the suite runs on,
  0xFF  every 16-bit and fp32 word a NaN, every mask byte "attend", every key-bit word "all keys",
  0x7B  fp16 61 280, bf16 / fp32 about 1.3e36: finite and huge -- v_max_f32 / fmaxf drop a NaN operand, so a stale NaN
        that reaches a running row maximum can vanish; a stale huge value cannot,
and the three results (probability outputs included) must be bit-identical, the guards intact, the launches per
profiler class the literals of the case, and the baseline within the project's tolerance for the policy of the float64
oracle (oracle/perceiver_oracle.py) -- three runs that are identically wrong do not pass.  Caller-owned scratch (the
projected-query cache, pio_decoder_call_t.q16_hi, while q16_valid == 0) is poisoned the same way.  Poison values are data:
no kernel reads an index or an offset from its scratch (the key-bit words are bit masks, the partials fp32 numbers;
csrc/pio_xattn.hip, pio_xtall.hip), so a poisoned run reads and writes the addresses of the zeroed one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import perceiver_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workspace_stale_cases as W  # noqa: E402
from test_parity_gpu import BF16_FUSED_TOL, FAST_TOY_BUDGET, PROBS_ABS_TOL, TIGHT, TOL  # noqa: E402  (the project's bars)
from test_primitives_gpu import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu


def tol_for(case):
    """test_parity_gpu.tol_for: "fp16x3" is held to TIGHT; the other policies to TOL at realistic widths (every channel
    count >= 256) and to FAST_TOY_BUDGET on toy-sized ones, where rounding the operands to 11 bits alone is ~1e-3."""
    if case["policy"] == "fp16x3":
        return TIGHT
    if case["policy"] == "bf16":
        return BF16_FUSED_TOL
    widths = [case[k] for k in ("C", "q_in", "kv_in", "C_in", "D", "Dq") if k in case]
    return TOL if min(widths) >= 256 else FAST_TOY_BUDGET


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f64(p):
    return {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}


def _load(mod, p, dev):
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    return mod.to(dev).eval()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ptr(t):
    return t.data_ptr() if t is not None else None


class Prepared:
    """One case ready to run: call(out_ptrs, ws_ptr, ws_bytes, scratch_ptrs, valid) -> return code."""

    def __init__(self, need, outs, call, ref, keep, scratch=(), pre=None):
        self.need, self.outs, self.call, self.ref, self.keep = need, outs, call, ref, keep
        self.scratch = scratch      # byte sizes of caller-owned scratch poisoned like the workspace
        self.pre = pre              # pre(out tensors): what an output buffer holds before the call (`out` aliasing `x`)


def _masks(case, rng, B, Tq, Tk, dev):
    m = set(case.get("masks", ()))
    kv = q = full = bias = None
    if "kv" in m:
        kv = rng.random((B, Tk)) > 0.3
        kv[:, 0] = True
        if case.get("kv_dead"):
            kv[1, :] = False
    if "q" in m:
        q = rng.random((B, Tq)) > 0.3
        q[:, 0] = True
        q[0, Tq - 1] = False
    if "full" in m:
        full = rng.random((B, Tq, Tk)) > 0.3
        full[:, :, 0] = True
        full[0, Tq - 1, :] = False            # a row without an attendable key
    if "bias" in m:
        bias = rng.standard_normal((B, case["H"], Tq, Tk)).astype(np.float32)
    mask = None
    if kv is not None or q is not None or full is not None:
        mask = np.ones((B, Tq, Tk), dtype=bool)
        if kv is not None:
            mask &= kv[:, None, :]
        if q is not None:
            mask &= q[:, :, None]
        if full is not None:
            mask &= full
    d = {k: (_dev(v.astype(np.uint8), dev) if v is not None else None) for k, v in (("kv", kv), ("q", q), ("full", full))}
    d["bias"] = _dev(bias, dev) if bias is not None else None
    return d, mask, bias


def _bcast(a, B, dev):
    """[1, T, C] on the device, viewed as a stride-0 batch of B."""
    t = _dev(a[:1], dev)
    return t.expand(B, -1, -1)


def _prep_mlp(case, dev, lib, R):
    from perceiverio_pytorch_amd.transformer_primitives import MLP
    B, T, Cc = case["B"], case["T"], case["C"]
    p = O.gen_mlp("", Cc, case["widening"], Cc, seed=11)
    m = _load(MLP(Cc, widening_factor=case["widening"]), p, dev)
    d = m._desc()
    x = W.rng_for(case).standard_normal((B, T, Cc)).astype(np.float32)
    xd = _dev(x, dev)
    need = lib.pio_mlp_workspace_bytes(d, B * T)
    return Prepared(need, [("out", (B, T, Cc))],
                    lambda o, w, n, s, valid: lib.pio_mlp_fwd(d, R.tensor3(xd), o[0], w, n, _stream()),
                    {"out": O.mlp(_f64(p), x.astype(np.float64))}, [m, xd])


def _prep_attention(case, dev, lib, R):
    from perceiverio_pytorch_amd.transformer_primitives import Attention
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    q_in, kv_in, out = case["q_in"], case["kv_in"], case["out"]
    p = O.gen_attention("", q_in, kv_in, case["qk"], case["v"], out, seed=12)
    m = _load(Attention(q_in, kv_in, kv_in, num_heads=H, qk_out_channels=case["qk"], v_out_channels=case["v"],
                        output_channels=out), p, dev)
    d = m._desc()
    rng = W.rng_for(case)
    xk = rng.standard_normal((B, Tk, kv_in)).astype(np.float32)
    xv = xk if case["inputs"] != "three" else rng.standard_normal((B, Tk, kv_in)).astype(np.float32)
    xq = xk if case["inputs"] == "self" else rng.standard_normal((B, Tq, q_in)).astype(np.float32)
    if case.get("q_bcast"):
        xq = np.broadcast_to(xq[:1], xq.shape)
    kd = _dev(xk, dev)
    vd = kd if case["inputs"] != "three" else _dev(xv, dev)
    qd = kd if case["inputs"] == "self" else (_bcast(xq, B, dev) if case.get("q_bcast") else _dev(xq, dev))
    md, mask, bias = _masks(case, rng, B, Tq, Tk, dev)
    probs = "probs" in case.get("masks", ())
    outs = [("out", (B, Tq, out))] + ([("probs", (B, H, Tq, Tk))] if probs else [])
    need = lib.pio_attention_workspace_bytes(d, B, Tq, Tk)

    def call(o, w, n, s, valid):
        return lib.pio_attention_fwd(d, R.tensor3(qd), R.tensor3(kd), R.tensor3(vd), _ptr(md["kv"]), _ptr(md["q"]),
                                     _ptr(md["full"]), _ptr(md["bias"]), o[0], o[1] if probs else None, w, n, _stream())

    r = O.attention(_f64(p), xq.astype(np.float64), xk.astype(np.float64), xv.astype(np.float64), H, mask,
                    bias.astype(np.float64) if bias is not None else None, return_matrix=probs)
    ref = {"out": r[1], "probs": r[0]} if probs else {"out": r}
    return Prepared(need, outs, call, ref, [m, qd, kd, vd, md])


def _prep_self(case, dev, lib, R):
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd.transformer_primitives import SelfAttention
    B, N, Cc, H = case["B"], case["N"], case["C"], case["H"]
    p = O.gen_self_attention("", Cc, seed=13)
    m = _load(SelfAttention(Cc, widening_factor=1, num_heads=H), p, dev)
    d = m._desc()
    x = W.rng_for(case).standard_normal((B, N, Cc)).astype(np.float32)
    xd = _dev(x, dev)
    opts = L.CallOpts(case["ln_fold"], 0)
    need = lib.pio_self_attention_workspace_bytes(d, B, N)
    alias = bool(case.get("alias"))

    def call(o, w, n, s, valid):
        src = L.Tensor3(o[0], N * Cc, Cc, B, N, Cc) if alias else R.tensor3(xd)
        return lib.pio_self_attention_fwd(d, src, None, None, None, None, o[0], None, C.byref(opts), w, n, _stream())

    return Prepared(need, [("out", (B, N, Cc))], call, {"out": O.self_attention(_f64(p), x.astype(np.float64), H)},
                    [m, xd, opts], pre=(lambda ts: ts[0].copy_(xd)) if alias else None)


def _prep_cross(case, dev, lib, R):
    from perceiverio_pytorch_amd.transformer_primitives import CrossAttention
    B, H, Tq, Tk, q_in, kv_in = case["B"], case["H"], case["Tq"], case["Tk"], case["q_in"], case["kv_in"]
    p = O.gen_cross_attention("", q_in, kv_in, seed=14)
    m = _load(CrossAttention(q_in, kv_in, num_heads=H, use_query_residual=case["resid"]), p, dev)
    d = m._desc()
    rng = W.rng_for(case)
    xkv = rng.standard_normal((B, Tk, kv_in)).astype(np.float32)
    xq = xkv if case.get("same_input") else rng.standard_normal((B, Tq, q_in)).astype(np.float32)
    if case.get("q_bcast"):
        xq = np.broadcast_to(xq[:1], xq.shape)
    kd = _dev(xkv, dev)
    qd = kd if case.get("same_input") else (_bcast(xq, B, dev) if case.get("q_bcast") else _dev(xq, dev))
    md, mask, _ = _masks(case, rng, B, Tq, Tk, dev)
    need = lib.pio_cross_attention_workspace_bytes(d, B, Tq, Tk)

    def call(o, w, n, s, valid):
        return lib.pio_cross_attention_fwd(d, R.tensor3(qd), R.tensor3(kd), _ptr(md["kv"]), _ptr(md["q"]), None, None, o[0],
                                           None, w, n, _stream())

    ref = O.cross_attention(_f64(p), xq.astype(np.float64), xkv.astype(np.float64), H, case["resid"], mask)
    return Prepared(need, [("out", (B, Tq, q_in))], call, {"out": ref}, [m, qd, kd, md])


def _prep_encoder(case, dev, lib, R):
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd.perceiver import PerceiverEncoder
    B, M, N, D, H, Ly, nblk, C_in = (case[k] for k in ("B", "M", "N", "D", "H", "L", "blocks", "C_in"))
    p = O.gen_encoder(C_in, N, D, Ly, seed=15)
    enc = _load(PerceiverEncoder(C_in, Ly, nblk, N, D, num_cross_attend_heads=1, num_self_attend_heads=H), p, dev)
    cross = enc.cross_attend._desc()
    per_block = case.get("per_block", 0)
    nset = nblk if per_block else 1
    layers = (L.SelfAttention * (Ly * nset))()
    for b in range(nset):                    # (per_block: every block gets the images of the shared parameters)
        for i, sa in enumerate(enc.self_attends):
            layers[b * Ly + i] = sa._desc()
    rng = W.rng_for(case)
    x = rng.standard_normal((B, M, C_in)).astype(np.float32)
    tail = case.get("tail", 0)
    if tail:
        x[:, :, C_in - tail:] = x[:1, :, C_in - tail:]          # the last `tail` channels are one [1, M, tail] table
    xd = _dev(x[:, :, :C_in - tail], dev)
    td = _dev(x[:1, :, C_in - tail:], dev) if tail else None
    zd = _bcast(p["latent_pos_enc.pos_embs"][None], B, dev)
    im = None
    if case.get("input_mask"):
        im = rng.random((B, M)) > 0.3
        im[:, 0] = True
    imd = _dev(im.astype(np.uint8), dev) if im is not None else None
    opts = L.CallOpts(case.get("ln_fold", 0), 0)
    need = lib.pio_encoder_workspace_bytes(cross, layers, Ly, B, M, N)
    tx, tz = R.tensor3(xd), R.tensor3(zd)
    tt = R.tensor3(td) if tail else None
    rec = L.EncoderCall(C.pointer(cross), C.cast(layers, C.POINTER(L.SelfAttention)), Ly, nblk, per_block, C.pointer(tx),
                        C.pointer(tt) if tail else None, C.pointer(tz), _ptr(imd), None, opts)

    def call(o, w, n, s, valid):
        rec.out = o[0]
        return lib.pio_encoder_fwd(C.byref(rec), w, n, _stream())

    ref = O.encoder(_f64(p), x.astype(np.float64), num_blocks=nblk, num_self_attends_per_block=Ly, num_cross_attend_heads=1,
                    num_self_attend_heads=H, input_mask=im)
    return Prepared(need, [("out", (B, N, D))], call, {"out": ref}, [enc, layers, xd, td, zd, imd, rec])


def _prep_decoder(case, dev, lib, R):
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd.perceiver import PerceiverDecoder
    B, Q, N, Dq, D, final, resid = (case[k] for k in ("B", "Q", "N", "Dq", "D", "final", "resid"))
    p = O.gen_decoder(Dq, D, case["out"] if final else None, seed=16)
    dec = _load(PerceiverDecoder(Dq, case["out"], num_latent_channels=D, num_heads=1, use_query_residual=resid,
                                 final_project=final), p, dev)
    cross = dec.decoding_cross_attn._desc()
    fin = dec._final_desc() if final else None
    fin_ptr = C.pointer(fin.desc) if fin is not None else None
    rng = W.rng_for(case)
    q = rng.standard_normal((B, Q, Dq)).astype(np.float32)
    z = rng.standard_normal((B, N, D)).astype(np.float32)
    tail = case.get("tail", 0)
    if tail:
        q[:, :, Dq - tail:] = q[:1, :, Dq - tail:]
    if case.get("q_bcast"):
        q = np.ascontiguousarray(np.broadcast_to(q[:1], q.shape))
    qd = _bcast(q, B, dev) if case.get("q_bcast") else _dev(q[:, :, :Dq - tail], dev)
    td = _dev(q[:1, :, Dq - tail:], dev) if tail else None
    zd = _dev(z, dev)
    qm = None
    if case.get("query_mask"):
        qm = rng.random((B, Q)) > 0.3
        qm[:, 0] = True
        qm[0, Q - 1] = False
    qmd = _dev(qm.astype(np.uint8), dev) if qm is not None else None
    need = lib.pio_decoder_workspace_bytes(cross, fin_ptr, B, Q, N)
    out_ch = case["out"]
    scratch = ()
    if case.get("qcache"):
        nb = lib.pio_decoder_qcache_bytes(cross, 1 if case.get("q_bcast") else B, Q)
        assert nb > 0 and cross.attn.act_split != 0            # (a policy with split activations: hi AND lo are cached)
        scratch = (nb, nb)
        used = (1 if case.get("q_bcast") else B) * Q * cross.attn.heads * cross.attn.dkp * 2
        assert used <= nb < used + 256

    rec = L.DecoderCall(C.pointer(cross), fin_ptr, out_ch, C.pointer(R.tensor3(qd)), C.pointer(R.tensor3(td)) if tail else None,
                        C.pointer(R.tensor3(zd)), _ptr(qmd))

    def call(o, w, n, s, valid):
        rec.out = o[0]
        if scratch:
            rec.q16_hi, rec.q16_lo, rec.q16_valid = s[0], s[1], valid
        return lib.pio_decoder_fwd(C.byref(rec), w, n, _stream())

    ref = O.decoder(_f64(p), q.astype(np.float64), z.astype(np.float64), num_heads=1, use_query_residual=resid,
                    final_project=final, query_mask=qm)
    pr = Prepared(need, [("out", (B, Q, out_ch))], call, {"out": ref}, [dec, fin, qd, td, zd, qmd, rec], scratch=scratch)
    pr.scratch_used = used if scratch else 0
    return pr


def _prepare(case, dev):
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import runtime as R
    lib = P.lib()
    e = case["entry"]
    prep = (_prep_mlp if e == "mlp_fwd" else _prep_attention if e == "attention_fwd" else
            _prep_self if e.startswith("self") else _prep_cross if e.startswith("cross") else
            _prep_encoder if e.startswith("encoder") else _prep_decoder)
    return prep(case, dev, lib, R)


class policy:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        import perceiverio_pytorch_amd as P
        from perceiverio_pytorch_amd import runtime as R
        self.prev = R.get_precision_policy()
        P.set_precision_policy(self.name)

    def __exit__(self, *exc):
        import perceiverio_pytorch_amd as P
        P.set_precision_policy(self.prev)
        return False


def _filled(dev, nbytes, fill):
    g = Guarded(dev, (nbytes,), torch.uint8)
    if fill == 0:
        g.bytes.zero_()            # the baseline run
    else:
        g.bytes.fill_(fill)
    return g


def _run(dev, case, pr, fill, what, ws=None, scratch=None, valid=0, count=False):
    """One call on guarded outputs; returns ({name: tensor}, workspace, scratch buffers, launches per class or None)."""
    import perceiverio_pytorch_amd as P
    lib = P.lib()
    ws = ws if ws is not None else _filled(dev, pr.need, fill)
    scratch = scratch if scratch is not None else [_filled(dev, n, fill) for n in pr.scratch]
    outs = [Guarded(dev, shape, torch.float32) for _, shape in pr.outs]
    if pr.pre:
        pr.pre([g.t for g in outs])
    assert ws.ptr % 256 == 0
    launches = None
    if count:
        assert lib.pio_prof_begin(256) == 0
    try:
        rc = pr.call([g.ptr for g in outs], ws.ptr, pr.need, [g.ptr for g in scratch] or [None, None], valid)
    finally:
        if count:
            launches = (C.c_int64 * 9)()
            assert lib.pio_prof_end(None, None, None, launches) >= 0
            launches = list(launches)
    assert rc == 0, f"{what}: return code {rc}"
    ws.check(what + " workspace")
    for g in scratch:
        g.check(what + " caller-owned scratch")
    for (name, _), g in zip(pr.outs, outs):
        g.check(f"{what} {name}")
    return {name: g.t for (name, _), g in zip(pr.outs, outs)}, ws, scratch, launches


def _assert_oracle(case, pr, got, what):
    tol = tol_for(case)
    for name, ref in pr.ref.items():
        if name == "probs":     # (the figure of test_parity_gpu.test_attention_return_matrix_and_bias, policy "fp16x3")
            err = float(np.abs(got[name].cpu().numpy() - ref).max())
            print(f"{what} probs: max |p - ref| = {err:.3e} (bar {PROBS_ABS_TOL:g})")
            assert case["policy"] == "fp16x3" and err <= PROBS_ABS_TOL, f"{what} probs: {err:.3e}"
            continue
        rl2, rmax = O.rel_errors(got[name].cpu().numpy(), ref)
        print(f"{what} {name}: relL2={rl2:.3e} max/absmax={rmax:.3e} (bar {tol:g})")
        assert rl2 <= tol and rmax <= tol, f"{what} {name}: relL2={rl2:.3e} max/absmax={rmax:.3e} > {tol}"


def _same(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


@pytest.mark.parametrize("case", W.CASES, ids=[c["id"] for c in W.CASES])
def test_result_does_not_depend_on_stale_workspace(dev, case):
    with policy(case["policy"]):
        pr = _prepare(case, dev)
        base, _, _, launches = _run(dev, case, pr, 0x00, f"{case['id']} zeroed", count=True)
        print(f"{case['id']}: workspace {pr.need} bytes, launches per class = {launches}")
        differ = []
        for fill in W.FILLS[1:]:
            got, _, _, _ = _run(dev, case, pr, fill, f"{case['id']} 0x{fill:02X}")
            for k in base:
                if not torch.equal(got[k].view(torch.int32), base[k].view(torch.int32)):
                    n = int((got[k].view(torch.int32) != base[k].view(torch.int32)).sum())
                    differ.append(f"{k} on 0x{fill:02X} bytes: {n} of {got[k].numel()} words, "
                                  f"{int(torch.isnan(got[k]).sum())} NaN")
    print(f"{case['id']}: differing from the zeroed run: {differ or 'none'}")
    assert launches == case["launches"], (case["id"], launches)
    _assert_oracle(case, pr, base, case["id"])
    assert not differ, f"{case['id']} [{'/'.join(case['cores'])}]: the result depends on stale workspace bytes: {differ}"


def test_query_cache_is_scratch_until_valid(dev):
    """q16_hi / q16_lo of pio_decoder_call_t: with q16_valid == 0 their content is undefined on entry (the parametrised
    test above poisons them with the workspace); what the call leaves there serves a q16_valid == 1 call on a freshly
    poisoned workspace, which skips LayerNorm_q and proj_q and returns the same bits."""
    case = W.BY_ID["decoder_qcache"]
    with policy(case["policy"]):
        pr = _prepare(case, dev)
        caches = {}
        for fill in W.FILLS:
            out, _, scratch, _ = _run(dev, case, pr, fill, f"qcache 0x{fill:02X} valid=0")
            caches[fill] = (out, scratch)
        base = caches[0x00][0]
        for fill in W.FILLS[1:]:
            assert _same(caches[fill][0], base), f"q16_valid = 0 on 0x{fill:02X} caches: the result depends on their content"
            used = pr.scratch_used      # (pio_decoder_qcache_bytes rounds up to 256: the bytes behind the rows stay unwritten)
            for a, b in zip(caches[fill][1], caches[0x00][1]):
                assert torch.equal(a.bytes[:used], b.bytes[:used]), "the projected queries left in the cache depend on its old content"
                assert bool((a.bytes[used:] == fill).all()), "bytes behind the projected queries were written"
        for fill in W.FILLS[1:]:
            out, _, _, launches = _run(dev, case, pr, fill, f"qcache 0x{fill:02X} valid=1", scratch=caches[0xFF][1], valid=1,
                                       count=True)
            assert launches == case["launches_valid"], launches
            assert _same(out, base), f"q16_valid = 1 on a 0x{fill:02X} workspace differs from the q16_valid = 0 call"
    _assert_oracle(case, pr, base, "decoder_qcache")


def test_small_call_after_a_larger_masked_key_split_call(dev):
    """Real reuse: ONE buffer, first a larger masked cross-attend in four key splits (key-bit words, fp32 partials, wider
    carves), then the small un-masked two-split case on its first bytes; the second result is its zero-workspace result."""
    first, second = W.SEQUENCE_FIRST, W.BY_ID[W.SEQUENCE_SECOND]
    with policy(first["policy"]):
        p1, p2 = _prepare(first, dev), _prepare(second, dev)
        assert p1.need > p2.need
        base, _, _, _ = _run(dev, second, p2, 0x00, "second call, zeroed workspace")
        ws = _filled(dev, p1.need, 0xFF)
        big, _, _, launches = _run(dev, first, p1, None, "first call", ws=ws, count=True)
        assert launches == first["launches"], launches
        _assert_oracle(first, p1, big, "first call")
        got, _, _, _ = _run(dev, second, p2, None, "second call, reused workspace", ws=ws)
    _assert_oracle(second, p2, base, "second call")
    assert _same(got, base), "the small call's result depends on what the larger call left in the workspace"
