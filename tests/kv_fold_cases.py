"""Cases, exact operands, the float64 reference and the bound for the K / V-projection fold of a single-head cross-attend AS
A COMPOSITION (csrc/pio_blocks.hip, attention_core, the kv_fold branch; routes KVFOLD_XATTN / KVFOLD_XTALL of
csrc/pio_attn_route.h): pio_attention_fwd on descriptors built by transformer_primitives.Attention.  Numpy only.

The fold is algebra: q (x Wk^T + bk)^T = (q Wk) x^T + const and P (x Wv^T + bv) Wo^T + bo = (P x)(Wo Wv)^T + (Wo bv + bo).

Operands.  Every intermediate is exactly representable except the core's documented roundings of P and O:
  x      the keys of a probe of attn_core_cases.make (planted / uniform / staircase) for one head of k_in channels: small
         integers times a power of two.  The values of the folded core are these rows themselves.
  Wk, Wq, Wv   signed permutations (one entry of +-1 per row and column): Q' = Q Wk is the probe's query array, so
         Q = Q' Wk^T and xq = (Q - bq) Wq exactly; V = x Wv^T + bv is a signed permutation of x plus bv.
  Wo     [out, k_in], three entries of {-2, -1, 1, 2} per row: Wo Wv has the same entries in other columns, and
         |Wo| |Wv| = |Wo Wv| (nothing cancels).
  bq     +-2 grid steps of Q; bk, bv multiples of 1/4 (|bv| <= 1/4), bo multiples of 1/2: all non-zero.  The folded bias
         Wo bv + bo is a multiple of 1/4: exact in fp32.
Reference: the un-folded formula (transformer_primitives.py: proj_q / proj_k / proj_v, softmax(q k^T / sqrt(dk)) v, final) in
float64 on these operands; with a key mask, masked keys are left out and a sample without attendable key gives final.bias.

Bound per output element n:  sum_c |(Wo Wv)[n, c]| * attn_core_cases.bound(dt, Tk, vmax)  (pair_sum form where the core returns
O as a pair).  The out projection multiplies a 16-bit O by small integers and accumulates in fp32 -- exact to 2^-24, inside
the 2^-16 term of bound() -- so only the core's error is carried through it: |out - ref|[n] <= sum_c |W[n, c]| |O - o|[c].
vmax is the largest magnitude among the values THAT run's core multiplies P with, over the attendable keys of the sample:
max |x| for the folded run, max |V| with V = x Wv^T + bv (at most |bv| <= 1/4 more) for the un-folded one, whose O has
dv = k_in channels that pass through |Wo| with sum_d |Wo[n, d]| = sum_c |(Wo Wv)[n, c]|.

The graded probe (here, not in attn_core_cases) is the one a wrong softmax scale cannot pass.  One key in 64 (j % 64 == 5)
carries level 1 on the first half of the channels and +h on the rest, every other key level 0 and -h (h: a +-1 pattern of
channel and sample); the query weighs the level channels alone, so that a level key leads by S ~ ln(others / level keys)
nats (twice that on odd rows): the two groups hold about half of the probability each, and a relative change eps of the
scale moves it by p (1 - p) eps S -- 0.9 % of the scale (sqrt(328) for sqrt(322)) is 1e-2 of the output's contrast 2 h,
FAULT_MARGIN times the fp16 bound and more (the host test asserts it).  The planted probe leads by 16 nats and a staircase by
12 per tile: they are blind to the scale by construction."""
import math

import numpy as np

import attn_core_cases as AC

PROBES = ("planted", "uniform", "stair_up", "stair_down", "graded")
FAULT_MARGIN = 8.0            # a modelled fault must move some element by more than this many bounds (the kernel may use one)
OUT = 24                      # output channels of `final`
DT_OF = {"fp16": "f16", "fp16x2af": "f16", "bf16": "bf16"}


def _case(id, k_in, B, Bq, Tq, Tk, core, cfg, slices, splits, policies=("fp16", "bf16"), fold=True):
    """core / cfg / slices / splits: the route as LITERALS (checked against csrc/pio_attn_route.h by the host test):
    AttnCore name, xattn instantiation (dkl, dvs) or None on the tall-head kernel, dv slices, key splits on 256 CUs."""
    return dict(id=id, k_in=k_in, kvp=(k_in + 7) & ~7, B=B, Bq=Bq, Tq=Tq, Tk=Tk, core=core, cfg=cfg, slices=slices, splits=splits,
                policies=policies, fold=fold)


CASES = [
    _case("k8_tq1_tk31", 8, 1, 1, 1, 31, "KVFOLD_XATTN", (32, 96), 1, 1),
    _case("k104_tq33_tk133", 104, 1, 1, 33, 133, "KVFOLD_XATTN", (128, 128), 1, 1),
    # kvp = 328 in rows of padc(322) = 384, two samples under batch-invariant queries: a scale of sqrt(328), a pitch of 328
    _case("k322_b2_bq1", 322, 2, 1, 33, 133, "KVFOLD_XATTN", (352, 352), 1, 1),
    _case("k512_tk520", 512, 1, 1, 33, 520, "KVFOLD_XATTN", (512, 512), 1, 2),
    # (512, 512) has an instantiation of the tiled kernel, which fused_core asks first: by the route header this shape is
    # KVFOLD_XATTN; the tall-head kernel takes the fold from kvp = 768 on (no tiled instantiation beyond 704)
    _case("k512_tk100", 512, 1, 1, 17, 100, "KVFOLD_XATTN", (512, 512), 1, 1),
    _case("k768_tk100_tall", 768, 1, 1, 17, 100, "KVFOLD_XTALL", None, 1, 1),
    _case("k704_three_slices", 704, 1, 1, 33, 133, "KVFOLD_XATTN", (704, 256), 3, 1),
    # key split: ntiles >= 16 is the first condition xattn_splits can meet for a head with one workgroup: Tk = 481
    _case("k8_split2_tk481", 8, 1, 1, 1, 481, "KVFOLD_XATTN", (32, 96), 1, 2),
    _case("k104_x2af_pair", 104, 1, 1, 33, 133, "KVFOLD_XATTN", (128, 128), 1, 1, policies=("fp16x2af",)),
    # the route's threshold B Tk >= 4 Bq Tq = 132: one below (fold off) and at it (fold on)
    _case("k104_tk131_below", 104, 1, 1, 33, 131, "XATTN", (128, 128), 1, 1, fold=False),
    _case("k104_tk132_at", 104, 1, 1, 33, 132, "KVFOLD_XATTN", (128, 128), 1, 1),
]
BY_ID = {c["id"]: c for c in CASES}
SPLIT_EDGE = ("k8_split2_tk481", 480)      # one key fewer: no split


def core_case(c):
    """The case as attn_core_cases sees its core: one head of kvp x kvp, logical dk = k_in."""
    kern = "xtall" if c["core"].endswith("XTALL") else "xattn"
    label = (1, 0) if kern == "xtall" else c["cfg"] + (c["slices"], c["splits"])
    cc = AC._case("kvfold_" + c["id"], kern, c["kvp"], c["kvp"], c["B"], 1, c["Tq"], c["Tk"], label, sqb0=c["Bq"] == 1 and c["B"] > 1)
    cc["dk"] = c["k_in"]
    return cc


def _signed_perm(rng, n):
    return rng.permutation(n), rng.choice([-1.0, 1.0], n)


def _perm_matrix(p, s):
    w = np.zeros((len(p), len(p)))
    w[np.arange(len(p)), p] = s
    return w


def _graded(c):
    """The graded probe (module docstring) in the form of attn_core_cases.make: qh [Bq, Tq, 1, kvp], kh [B, Tk, 1, kvp]."""
    B, Bq, Tq, Tk, k, kvp = c["B"], c["Bq"], c["Tq"], c["Tk"], c["k_in"], c["kvp"]
    na = k // 2
    lead = (np.arange(Tk) % 64) == 5
    S = math.log((Tk - lead.sum()) / lead.sum())
    m, e = AC._quant(S * math.sqrt(k) / na)
    sig = np.where(np.arange(k) % 3 == 0, -1.0, 1.0)
    b, ch = np.ogrid[:B, :k - na]
    h = np.where((ch * 7 + b * 3) % 5 < 2, -1.0, 1.0)                     # [B, k - na]
    kh = np.zeros((B, Tk, 1, kvp))
    kh[:, :, 0, :na] = lead[None, :, None] * sig[:na]
    kh[:, :, 0, na:k] = np.where(lead[None, :, None], 1.0, -1.0) * h[:, None, :]
    qh = np.zeros((Bq, Tq, 1, kvp))
    qh[:, :, 0, :na] = (m * 2.0 ** -e) * sig[:na] * (1 + np.arange(Tq) % 2)[None, :, None]
    return dict(qh=qh, kh=kh, targets=None)


def make(c, probe, dt):
    """-> dict: xq [Bq, Tq, k_in], x [B, Tk, k_in], the eight parameters (float64, exact in `dt` / fp32), the probe's
    targets; None where the probe does not apply (a staircase needs two key tiles)."""
    d = _graded(c) if probe == "graded" else AC.make(core_case(c), probe, dt)
    if d is None:
        return None
    k = c["k_in"]
    rng = np.random.default_rng(k * 131 + c["Tk"])
    x = d["kh"][:, :, 0, :k]
    qp = d["qh"][:, :, 0, :k]                              # Q' = Q Wk
    (pk, sk), (pq, sq), (pv, sv) = (_signed_perm(rng, k) for _ in range(3))
    Wk, Wq, Wv = _perm_matrix(pk, sk), _perm_matrix(pq, sq), _perm_matrix(pv, sv)
    Q = qp @ Wk.T
    g = 2.0 ** -12                                         # the grid of Q: the largest power of two that divides it (<= 1/8)
    while g < 0.125 and np.array_equal(Q / (2 * g), np.rint(Q / (2 * g))):
        g *= 2
    i = np.arange(k)
    bq = 2 * g * ((i % 3) - 1.0)
    bk = np.where(i % 5 == 0, ((i % 7) - 3) / 4.0, 0.0)
    bk[0] = 0.5
    bv = ((i % 3) - 1) / 4.0
    bv[0] = 0.25
    xq = (Q - bq) @ Wq
    Wo = np.zeros((OUT, k))
    for n in range(OUT):
        Wo[n, rng.choice(k, 3, replace=False)] = rng.choice([-2.0, -1.0, 1.0, 2.0], 3)
    bo = (1 + np.arange(OUT) % 4) / 2.0 * np.where(np.arange(OUT) % 2, -1.0, 1.0)
    out = dict(xq=xq, x=x, Wq=Wq, bq=bq, Wk=Wk, bk=bk, Wv=Wv, bv=bv, Wo=Wo, bo=bo, targets=d["targets"], dk=k)
    V = x @ Wv.T + bv
    K = x @ Wk.T + bk
    for a in (xq, x, Q, qp, K, V):
        assert np.array_equal(AC.round16(a, dt), a), "operands and projections must be exact in the 16-bit type"
    assert np.array_equal(xq @ Wq.T + bq, Q) and np.array_equal(Q @ Wk, qp)
    assert np.abs(Wo @ Wv).max() < 2 ** 11 and np.abs(qp).max() < 2 ** 11
    assert np.array_equal(np.abs(Wo) @ np.abs(Wv), np.abs(Wo @ Wv))
    assert bq.any() and bk.any() and bv.any() and bo.all()
    return out


def key_mask(c):
    """[B, Tk] bool for the masked run: scattered keys out; where there is more than one sample, the LAST one without any
    attendable key (with one sample the scattered mask itself is what the run is compared on)."""
    j = np.arange(c["Tk"])
    m = np.ones((c["B"], c["Tk"]), bool)
    m[:, (j % 7) == 3] = False
    if c["B"] > 1:
        m[c["B"] - 1, :] = False
    return m


def _softmax(s, km):
    if km is not None:
        s = np.where(km[:, None, :], s, -np.inf)
    m = s.max(axis=-1, keepdims=True)
    p = np.exp(s - np.where(np.isfinite(m), m, 0.0))
    return p, p.sum(axis=-1, keepdims=True)


def reference(c, d, km=None, fault=None):
    """out [B, Tq, OUT] float64 by the UN-FOLDED formula; fault: one of FAULTS, as a folded path with it would compute."""
    B, k = c["B"], d["dk"]
    xq = np.broadcast_to(d["xq"], (B,) + d["xq"].shape[1:])
    x = d["x"]
    Q = xq @ d["Wq"].T + d["bq"]
    if fault == "bstride_bq1" and c["Bq"] == 1:            # every sample reads the keys of sample 0
        x = np.broadcast_to(x[0:1], x.shape)
    K = x @ d["Wk"].T + d["bk"]
    V = x @ d["Wv"].T + d["bv"]
    s = Q @ K.transpose(0, 2, 1) / math.sqrt(c["kvp"] if fault == "scale_kvp" else k)
    if fault == "drop_last_key":
        s[:, :, -1] = -np.inf
    p, l = _softmax(s, km)
    o = (p @ V) / np.where(l > 0, l, 1.0)
    if fault == "drop_wo_bv":
        o = o - d["bv"]
    out = o @ d["Wo"].T + d["bo"]
    return np.where(l > 0, out, d["bo"])                   # no attendable key: final.bias alone


FAULTS = ("scale_kvp", "drop_wo_bv", "drop_last_key", "bstride_bq1")


def vmax_of(d, folded, km=None):
    """[B, 1, 1]: the largest |value| the run's core multiplies P with, over the attendable keys of the sample: x folded,
    V = x Wv^T + bv un-folded."""
    vals = d["x"] if folded else d["x"] @ d["Wv"].T + d["bv"]
    v = np.abs(vals).max(axis=2)                                           # [B, Tk]
    if km is not None:
        v = np.where(km, v, 0.0)
    return v.max(axis=1)[:, None, None]


def bound(c, d, dt, pair, folded, km=None):
    """[B, 1, OUT] (module docstring); folded: the run whose core reads x itself (a masked run is never folded)."""
    w = np.abs(d["Wo"] @ d["Wv"]).sum(axis=1)
    return w[None, None, :] * AC.bound(dt, c["Tk"], vmax_of(d, folded, km), pair_sum=pair)


def rounded_model(c, d, dt, pair, folded):
    """The reference pushed through the documented roundings of one core: P rounded once to 16 bits against an un-rounded
    denominator, O rounded once (or kept as hi + lo), every projection exact."""
    B = c["B"]
    xq = np.broadcast_to(d["xq"], (B,) + d["xq"].shape[1:])
    Q = xq @ d["Wq"].T + d["bq"]
    x = d["x"]
    if folded:
        s = (Q @ d["Wk"]) @ x.transpose(0, 2, 1) / math.sqrt(d["dk"])
        vals, w, b = x, d["Wo"] @ d["Wv"], d["Wo"] @ d["bv"] + d["bo"]
    else:
        s = Q @ (x @ d["Wk"].T + d["bk"]).transpose(0, 2, 1) / math.sqrt(d["dk"])
        vals, w, b = x @ d["Wv"].T + d["bv"], d["Wo"], d["bo"]
    p, l = _softmax(s, None)
    o = (AC.round16(p, dt).astype(np.float64) @ vals) / l
    hi = AC.round16(o, dt).astype(np.float64)
    if pair:
        hi = hi + AC.round16(o - hi, dt).astype(np.float64)
    return hi @ w.T + b
