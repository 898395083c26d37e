"""GPU: the vocabulary head -- pio_vocab_topk through the raw C-ABI against the float64 definition (tests/vocab_cases.py: the
derived logit and lse bounds, the exact order of ids, logprob bit for bit), planted winners, row independence, the selection
mode, the refusal table; LanguagePerceiver.predict on the full-size goldens.

Memory safety by construction: every output sits between guard bands and is NaN before the call; the columns [V, ldl) of the
logits must still be NaN afterwards; x, w and bias are surrounded by NaN (rows around them, the columns [K, ld)), and every
result must be finite."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vocab_cases as VC  # noqa: E402
from test_flow_front_gpu import GuardedOut  # noqa: E402
from test_models import TOL, _cached_model, _close  # noqa: E402
from _golden import load  # noqa: E402
from cases import model_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
S = VC.STRIP


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


def _framed(a, ld, dev):
    """A 2-D fp32 array as rows 1 .. of a NaN array with row pitch ld and a NaN row on either side; (tensor, address)."""
    full = np.full((a.shape[0] + 2, ld), np.nan, dtype=np.float32)
    full[1:-1, :a.shape[1]] = a
    t = torch.from_numpy(full).to(dev)
    return t, t.data_ptr() + 4 * ld


def run(dev, k, x=None, w=None, bias=None, given=None, ldx_gap=0, ldw_gap=0, ldl_gap=0, want_logits=True, what=""):
    """One call of the raw entry.  Computing: x [B, Q, K], w [V, K], bias [V] or None (numpy fp32), each NaN-framed with its
    pitch; selection alone: given [B Q, V] logits.  Returns numpy ids [R, k], logprob [R, k], lse [R], logits [R, V] or None."""
    from perceiverio_pytorch_amd import _lib as L
    f = dict(x=None, x_sb=0, ldx=0, w=None, ldw=0, bias=None, K=0, k=k)
    keep = []
    if given is None:
        B, Q, K = x.shape
        V = w.shape[0]
        ldx, ldw = K + ldx_gap, K + ldw_gap
        xf = np.full((B, Q + 2, ldx), np.nan, dtype=np.float32)
        xf[:, 1:-1, :K] = x
        xt = torch.from_numpy(xf).to(dev)
        wt, wp = _framed(w, ldw, dev)
        f.update(x=xt.data_ptr() + 4 * ldx, x_sb=(Q + 2) * ldx, ldx=ldx, w=wp, ldw=ldw, K=K)
        keep += [xt, wt]
        if bias is not None:
            bt, bp = _framed(bias[:, None], 1, dev)
            f["bias"] = bp
            keep.append(bt)
    else:
        B, (Q, V) = 1, given.shape
    R, ldl = B * Q, V + ldl_gap
    ids, lp, lse = GuardedOut(dev, R, k), GuardedOut(dev, R, k), GuardedOut(dev, R, 1)
    lg = GuardedOut(dev, R, ldl) if (want_logits or given is not None) else None
    if given is not None:
        lg.t[:, :V] = torch.from_numpy(np.ascontiguousarray(given)).to(dev)
    f.update(B=B, Q=Q, V=V, ids=ids.t.data_ptr(), logprob=lp.t.data_ptr(), lse=lse.t.data_ptr(),
             logits=None if lg is None else lg.t.data_ptr(), ldl=ldl)
    L.check(VC.call(L, f, torch.cuda.current_stream().cuda_stream), f"pio_vocab_topk[{what}]")
    for g in (ids, lp, lse) + ((lg,) if lg is not None else ()):
        g.check(what)
    if lg is not None:
        assert bool(torch.isnan(lg.t[:, V:]).all()), f"{what}: the columns [V, ldl) of the logits were written"
    out = dict(ids=ids.t.view(torch.int32).cpu().numpy(), logprob=lp.t.cpu().numpy(), lse=lse.t[:, 0].cpu().numpy(),
               logits=None if lg is None else lg.t[:, :V].cpu().numpy())
    assert ((out["ids"] >= 0) & (out["ids"] < V)).all(), f"{what}: an id outside [0, V) (or one never written)"
    return out


def check_selection(out, k, what):
    """ids, lse and logprob of a call against ITS OWN logits: the exact order, the derived lse bound, logprob bit for bit."""
    lg = out["logits"]
    assert np.isfinite(lg).all() and np.isfinite(out["lse"]).all() and np.isfinite(out["logprob"]).all(), what
    want = VC.stable_topk(lg, k)
    assert np.array_equal(out["ids"], want), f"{what}: ids differ from a stable descending sort of the kernel's logits"
    ratio = VC.lse_ratio(out["lse"], lg, what)
    top = np.take_along_axis(lg, out["ids"].astype(np.int64), axis=1)
    lp = (top.astype(np.float32) + (-out["lse"].astype(np.float32))[:, None]).astype(np.float32)
    assert np.array_equal(lp.view(np.int32), out["logprob"].view(np.int32)), f"{what}: logprob != fadd(logit, -lse)"
    assert (np.diff(out["logprob"], axis=1) <= 0).all(), f"{what}: values not descending"
    return ratio


def same_bits(a, b, fields=("ids", "logprob", "lse")):
    return all(np.array_equal(a[f].view(np.int32), b[f].view(np.int32)) for f in fields)


# name: B, Q, V, K, k, bias, ldx_gap, ldw_gap.  Rows B Q = 1, STRIP - 1, STRIP + 1, 3 STRIP + 2; V = 1, 5, 64, 65, 262, 1024;
# K = 4, 256, 260 (a partial last sweep of the 64 lanes), 768, 1024; k = 1, 5, 8; ldx > K, ldw > K, B > 1 (a batch stride that is
# not Q ldx: run() frames every sample); bias present and NULL.
CASES = {
    "one_row_v1_k4": (1, 1, 1, 4, 1, True, 0, 0),
    "strip-1_v5_k256": (1, S - 1, 5, 256, 5, False, 4, 0),
    "strip+1_v64_k260": (3, 3, 64, 260, 8, True, 0, 8),
    "3strips+2_v65_k768": (2, (3 * S + 2) // 2, 65, 768, 5, True, 8, 4),
    "shipped_v262_k768": (1, S + 1, 262, 768, 5, True, 0, 0),
    "v1024_k1024": (1, S - 1, 1024, 1024, 8, True, 4, 4),
    "v262_k4_nobias": (2, (3 * S + 2) // 2, 262, 4, 1, False, 4, 0),
    "v1024_k256_k1": (1, 3 * S + 2, 1024, 256, 1, False, 0, 12),
}
RATIOS = {}


@pytest.mark.parametrize("name", sorted(CASES))
def test_raw_entry_against_the_definition(dev, name):
    B, Q, V, K, k, has_bias, gx, gw = CASES[name]
    rng = np.random.default_rng(sum((i + 1) * ord(c) for i, c in enumerate(name)))
    x = rng.standard_normal((B, Q, K)).astype(np.float32)
    w = (rng.standard_normal((V, K)) * (2.0 / np.sqrt(K))).astype(np.float32)
    bias = rng.standard_normal(V).astype(np.float32) if has_bias else None
    out = run(dev, k, x, w, bias, ldx_gap=gx, ldw_gap=gw, ldl_gap=3, what=name)
    ref, mag = VC.definition(x.reshape(B * Q, K), w, bias)
    RATIOS[name] = (VC.logit_ratio(out["logits"], ref, mag, K, name), check_selection(out, k, name))
    print(f"{name}: worst ratios so far: logits {max(r[0] for r in RATIOS.values()):.3f}, "
          f"lse {max(r[1] for r in RATIOS.values()):.3f}")
    # without the logits: the same small results; the selection alone on the returned logits: the same bits again
    lean = run(dev, k, x, w, bias, ldx_gap=gx, ldw_gap=gw, want_logits=False, what=name + ", no logits")
    assert lean["logits"] is None and same_bits(out, lean), f"{name}: asking for the logits changed the results"
    sel = run(dev, k, given=out["logits"], ldl_gap=5, what=name + ", selection")
    assert same_bits(out, sel), f"{name}: the selection mode differs from the computing mode on the same logits"
    assert np.array_equal(sel["logits"].view(np.int32), out["logits"].view(np.int32))     # (an input: untouched)


def _planted(V, k):
    """Rows of logits [rows, V] with planted winners over a seeded background below -1, and what each row is about.  A lane
    of the selecting wave owns the ids l, l + 64, ...: ids 63 | 64 and 127 | 128 sit on either side of a sweep of the wave, id
    V - 1 is the last id of the last lane's share."""
    rng = np.random.default_rng(V * 131 + k)
    base = (-1.0 - rng.random(V)).astype(np.float32)
    rows, names = [], []

    def add(name, **planted):
        r = base.copy()
        for j, v in planted.items():
            r[int(j[1:])] = v
        rows.append(r)
        names.append(name)
    add("maximum at id 0", j0=3.0)
    add("maximum at id V - 1", **{f"j{V - 1}": 3.0})
    add("maximum at id 63", j63=3.0)
    add("maximum at id 64", j64=3.0)
    add("two equal maxima, 63 | 64", j63=2.5, j64=2.5)
    add("two equal maxima, 127 | 128, a higher id first in lane order", j128=2.5, j127=2.5)
    add("two equal maxima in ONE lane's share", j5=2.5, **{f"j{5 + 64}": 2.5})
    ties = sorted(set([0, 63, 64, 127, 128, V - 1] + list(range(60, 60 + k + 1))))[:k + 1]
    add("k + 1 equal maxima across the sweeps", **{f"j{j}": 2.0 for j in ties})
    rows.append(np.full(V, 0.75, dtype=np.float32))
    names.append("all logits equal")
    z = np.where(rng.random(V) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    z[0], z[1], z[64] = -0.0, 0.0, -0.0
    rows.append(z)
    names.append("+0.0 against -0.0: equal, the lower id first")
    zz = base.copy()
    zz[[7, 70, 130]] = [0.0, -0.0, 0.0]
    rows.append(zz)
    names.append("signed zeros as the three maxima")
    return np.stack(rows), names


@pytest.mark.parametrize("V,k", [(200, 1), (200, 5), (262, 8)])
def test_planted_winners(dev, V, k):
    lg, names = _planted(V, k)
    out = run(dev, k, given=lg, what=f"planted V={V} k={k}")
    want = VC.stable_topk(lg, k)
    for r, name in enumerate(names):
        assert out["ids"][r].tolist() == want[r].tolist(), f"{name}: got {out['ids'][r].tolist()}, want {want[r].tolist()}"
    assert out["ids"][0, 0] == 0 and out["ids"][1, 0] == V - 1 and out["ids"][2, 0] == 63 and out["ids"][3, 0] == 64
    assert out["ids"][4, 0] == 63 and out["ids"][5, 0] == 127 and out["ids"][6, 0] == 5
    assert out["ids"][8].tolist() == list(range(k)) and out["ids"][9].tolist() == list(range(k))
    assert out["ids"][10].tolist() == [7, 70, 130][:k] + ([] if k <= 3 else want[10, 3:].tolist())
    check_selection(out, k, f"planted V={V} k={k}")
    # the same rows (but the signed zeros: a product plus +0 is +0) through the computing mode: x[r] = e_r, w[j, r] = logit[r, j]
    n = 9
    K = 12
    x = np.zeros((1, n, K), dtype=np.float32)
    x[0, np.arange(n), np.arange(n)] = 1.0
    w = np.zeros((V, K), dtype=np.float32)
    w[:, :n] = lg[:n].T
    comp = run(dev, k, x, w, None, what=f"planted V={V} k={k}, computed")
    assert np.array_equal(comp["logits"], lg[:n]) and np.array_equal(comp["ids"], out["ids"][:n])
    assert same_bits({f: v[:n] for f, v in out.items() if v is not None}, comp)


def test_nan_rows_stay_in_bounds_and_alone(dev):
    """A row holding a NaN: ids inside [0, V) (run() asserts it), nothing said about its values; its neighbours are exact."""
    rng = np.random.default_rng(9)
    lg = rng.standard_normal((S + 3, 100)).astype(np.float32)
    clean = run(dev, 8, given=lg, what="before the NaN")
    lg2 = lg.copy()
    lg2[2, 5] = np.nan
    lg2[S + 1, :] = np.nan
    out = run(dev, 8, given=lg2, what="NaN rows")
    good = [r for r in range(S + 3) if r not in (2, S + 1)]
    assert same_bits({f: clean[f][good] for f in ("ids", "logprob", "lse")}, {f: out[f][good] for f in ("ids", "logprob", "lse")})


def test_rows_do_not_depend_on_where_they_run(dev):
    """The same 5 rows as one call at B = 1, and spread over other strips, samples, pitches and row counts: equal bits."""
    rng = np.random.default_rng(17)
    V, K, k = 262, 768, 5
    rows = rng.standard_normal((5, K)).astype(np.float32)
    w = (rng.standard_normal((V, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(V).astype(np.float32)
    one = run(dev, k, rows[None], w, bias, what="alone")
    B, Q = 3, 2 * S + 5
    x = rng.standard_normal((B, Q, K)).astype(np.float32)
    where = [(0, 0), (0, S), (1, 3), (2, Q - 1), (2, S - 1)]          # (sample, row): other strips, lanes of the strip, samples
    for i, (b, q) in enumerate(where):
        x[b, q] = rows[i]
    many = run(dev, k, x, w, bias, ldx_gap=8, ldw_gap=4, ldl_gap=2, what="spread")
    pick = [b * Q + q for b, q in where]
    assert same_bits(one, {f: v[pick] for f, v in many.items()}, fields=("ids", "logprob", "lse", "logits"))
    again = run(dev, k, x, w, bias, ldx_gap=8, ldw_gap=4, ldl_gap=2, what="spread, again")
    assert same_bits(many, again, fields=("ids", "logprob", "lse", "logits")), "two launches differ"


@pytest.mark.parametrize("what,changes,code", VC.REFUSALS, ids=[r[0] for r in VC.REFUSALS])
def test_refusals_launch_nothing(dev, what, changes, code):
    from perceiverio_pytorch_amd import _lib as L
    v = VC.VALID
    bufs = {"x": torch.randn(2 * v["x_sb"] + 64, device=dev), "w": torch.randn(v["V"] * v["ldw"] + 64, device=dev),
            "bias": torch.randn(64, device=dev)}
    outs = {"ids": GuardedOut(dev, 8, 8), "logprob": GuardedOut(dev, 8, 8), "lse": GuardedOut(dev, 8, 8),
            "logits": GuardedOut(dev, 8, 8)}
    ptrs = {**{n: t.data_ptr() for n, t in bufs.items()}, **{n: g.t.data_ptr() for n, g in outs.items()}}
    assert VC.call(L, VC.refusal_fields(ptrs, {}), torch.cuda.current_stream().cuda_stream) == VC.PIO_OK
    for n, g in outs.items():
        g.check("valid call")
        g.t.fill_(float("nan"))
    assert VC.call(L, VC.refusal_fields(ptrs, changes), torch.cuda.current_stream().cuda_stream) == code
    for n, g in outs.items():
        g.check(what)
        assert bool(torch.isnan(g.t).all()), f"{what}: a refused call wrote to {n}"


# ----------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------
WINDOW = list(range(96)) + list(range(640, 704))          # the rows the language goldens store


def _golden_rows(g, pos):
    """[B, P, V] golden logits at positions pos [B, P] (inside the stored windows)."""
    both = np.concatenate([g["out"], g["out_tail"]], axis=1)
    col = np.where(pos < 96, pos, pos - 640 + 96)
    return np.take_along_axis(both, col[:, :, None], axis=1)


@pytest.fixture(scope="module", params=["model_language", "model_language_s33"])
def lang(request, dev):
    name = request.param
    g = load(name)
    model = _cached_model(name, g, dev)
    from perceiverio_pytorch_amd.models import DEFAULT_POLICY
    assert model.precision_policy == DEFAULT_POLICY["LanguagePerceiver"] and model.fused_predict is True
    ins = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]
    # every stored row of both samples, in another order per sample: at every p the two samples ask for different positions
    pos = np.stack([np.array(WINDOW), np.array(WINDOW[::-1])])
    return name, g, model, ins, pos


@pytest.mark.parametrize("route", ["shipped routing", "the kernel multiplies"])
def test_predict_against_the_golden(dev, lang, monkeypatch, route):
    name, g, model, ins, pos = lang
    from perceiverio_pytorch_amd import fused_io as FIO
    if route != "shipped routing":
        monkeypatch.setattr(FIO, "VOCAB_FUSED_MAX_ROWS", 2 ** 31)
    post = model.perceiver._output_postprocessors["__default"]
    assert FIO.vocab_plan(post, torch.empty(2, 160, 768, device=dev), 5) == ("select" if route == "shipped routing" else "fused")
    name = f"{name}, {route}"
    with torch.inference_mode():
        got = model.predict(ins[0], ins[1], torch.from_numpy(pos), k=5, return_logits=True)
        full = model(ins[0], ins[1])
    assert got.ids.shape == (2, 160, 5) and got.ids.dtype == torch.int64 and got.logits.shape == (2, 160, 262)
    ref = _golden_rows(g, pos)
    head = pos < 96
    for b in range(2):
        _close(got.logits[b][torch.from_numpy(head[b]).to(dev)], ref[b][head[b]], f"{name} predict, sample {b} head", TOL,
               absmax=g["out_absmax"])
        _close(got.logits[b][torch.from_numpy(~head[b]).to(dev)], ref[b][~head[b]], f"{name} predict, sample {b} tail", TOL,
               absmax=g["out_absmax"])
    rows = torch.gather(full, 1, torch.from_numpy(pos).to(dev)[:, :, None].expand(-1, -1, 262))
    print(f"{name}: max |predict logits - forward rows| / absmax = "
          f"{float((got.logits - rows).abs().max()) / float(g['out_absmax']):.3e}")
    assert np.array_equal(got.ids[..., 0].cpu().numpy(), ref.argmax(axis=-1)), f"{name}: top-1 differs from the golden's argmax"
    out = dict(ids=got.ids.reshape(-1, 5).cpu().numpy().astype(np.int32), logprob=got.logprobs.reshape(-1, 5).cpu().numpy(),
               logits=got.logits.reshape(-1, 262).cpu().numpy())
    assert np.array_equal(out["ids"], VC.stable_topk(out["logits"], 5))
    lse = torch.logsumexp(got.logits.double(), dim=-1, keepdim=True)
    assert float((torch.gather(got.logits, 2, got.ids).double() - lse - got.logprobs.double()).abs().max()) < 1e-5


def test_chain_and_selection_route_agree_with_the_fused_path(dev, lang, monkeypatch):
    name, g, model, ins, pos = lang
    from perceiverio_pytorch_amd import fused_io as FIO
    p = torch.from_numpy(pos)
    with torch.inference_mode():
        monkeypatch.setattr(FIO, "VOCAB_FUSED_MAX_ROWS", 2 ** 31)     # the kernel's own fp32 multiply
        fused = model.predict(ins[0], ins[1], p, k=5, return_logits=True)
        model.fused_predict = False
        try:
            chain = model.predict(ins[0], ins[1], p, k=5, return_logits=True)
        finally:
            model.fused_predict = True
        monkeypatch.setattr(FIO, "VOCAB_FUSED_MAX_ROWS", 0)           # hip_linear's logits, the kernel's selection
        select = model.predict(ins[0], ins[1], p, k=5, return_logits=True)
    _close(chain.logits, fused.logits.cpu().numpy(), f"{name}: chain against fused", TOL, absmax=g["out_absmax"])
    assert torch.equal(chain.ids[..., 0], fused.ids[..., 0]) and torch.equal(select.ids[..., 0], fused.ids[..., 0])
    assert torch.equal(select.logits, chain.logits), "the selection route multiplies with the chain's hip_linear"
    assert np.array_equal(select.ids.reshape(-1, 5).cpu().numpy(), VC.stable_topk(select.logits.reshape(-1, 262).cpu().numpy(), 5))
    assert float((select.logprobs - chain.logprobs).abs().max()) < 1e-5


def test_shared_positions_equal_repeated_positions(dev, lang):
    name, g, model, ins, pos = lang
    shared = torch.tensor([51, 52, 59, 0, 95, 640, 703, 2047, 1000])
    seen = []
    hook = model.perceiver._decoder.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    try:
        with torch.inference_mode():
            a = model.predict(ins[0], ins[1], shared, k=8, return_logits=True)
            b = model.predict(ins[0], ins[1], shared[None].expand(2, -1).contiguous().to(dev), k=8, return_logits=True)
            c = model.predict(ins[0], ins[1], shared.tolist(), k=8, return_logits=True)
    finally:
        hook.remove()
    assert seen[0].shape == (2, 9, 768) and seen[0].stride(0) == 0 and seen[1].stride(0) != 0       # projected once / per sample
    for f in ("ids", "logprobs", "logits"):
        assert torch.equal(getattr(a, f), getattr(b, f)) and torch.equal(getattr(a, f), getattr(c, f)), f


def test_predict_leaves_forward_alone(dev, lang):
    name, g, model, ins, pos = lang
    with torch.inference_mode():
        before = model(ins[0], ins[1])
        model.predict(ins[0], ins[1], [51, 52, 53], k=5)
        model.predict(ins[0], ins[1], None, k=1)
        after = model(ins[0], ins[1])
    assert torch.equal(before, after)
    assert model.perceiver.decoder_query_rows is None and model.perceiver.decoder_policy is None
