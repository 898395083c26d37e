"""Definition, bounds and the refusal table of the vocabulary head (pio_vocab_topk, csrc/pio_vocab.hip).

Numpy only; shared by tests/test_vocab_topk_host.py (CPU) and tests/test_vocab_topk_gpu.py (MI355X).

    logit[r, j] = bias[j] + sum_k w[j, k] x[r, k]
    lse[r]      = m + log(sum_j exp(logit[r, j] - m)),  m = max_j logit[r, j]
    ids[r, :]   = the first k ids in the order (logit descending, id ascending among equal logits, -0.0 == +0.0)
    logprob     = fadd_rn(logit[ids], -lse)

Logit bound (derived, the one of tests/heads_cases.py with this kernel's term count): an fp32 dot product of K terms plus the
bias, in any order, with or without FMA:  |logit - ref| <= gamma_(K+1) (|bias| + sum_k |w_k x_k|),  gamma_n = n u / (1 - n u),
u = 2^-24.

lse bound (derived), against the float64 log-sum-exp of the kernel's OWN fp32 logits l_j; d_j = l_j - m <= 0, m exact (a
maximum rounds nothing), S = sum_j exp(d_j) >= 1:
  * a_j = fsub_rn(l_j, m) = d_j (1 + delta), |delta| <= u, so exp(a_j) = exp(d_j) exp(d_j delta): relative error at most
    exp(|d_j| u) - 1;
  * expf is within 1 ulp of exp (HIP math API, single-precision accuracy table: expf 1 ulp, logf 1 ulp): a relative error of
    at most 2^-23 = 2 u, hence term j carries at most tau_j = exp(|d_j| u) (1 + 2 u) - 1; a term (or a partial sum) too small
    for a normal fp32 may lose up to 2^-126 absolutely, V of them at most;
  * the V non-negative terms are added in some fixed order with rounding: relative error at most gamma_(V-1) <= gamma_V of the
    sum of the computed terms;
  so S_c = S (1 + eta),  |eta| <= (1 + gamma_V) (1 + tau) - 1 + V 2^-126,  tau = sum_j exp(d_j) tau_j / S, and
  A = |log S_c - log S| <= -log(1 - eta);
  * logf within 1 ulp:  B = 2 u (|log S| + A);
  * the final fadd_rn(m, .):  C = u (|ref| + A + B).
  |lse - ref| <= A + B + C."""
import numpy as np

PIO_OK, PIO_E_SHAPE, PIO_E_ALIGN, PIO_E_ARG = 0, -1, -2, -6
STRIP = 8           # rows per workgroup strip in csrc/pio_vocab.hip (VT_TS): cases cross it on purpose
U = 2.0 ** -24

ARG_ORDER = ("x", "x_sb", "ldx", "w", "ldw", "bias", "B", "Q", "V", "K", "k", "ids", "logprob", "lse", "logits", "ldl")
POINTERS = ("x", "w", "bias", "ids", "logprob", "lse", "logits")


def gamma(n):
    return n * U / (1.0 - n * U)


def definition(x, w, bias):
    """(ref, mag) float64 [.., V] of fp32 x [.., K], w [V, K], bias [V] or None."""
    x64, w64 = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    ref, mag = x64 @ w64.T, np.abs(x64) @ np.abs(w64).T
    if bias is not None:
        ref, mag = ref + np.asarray(bias, dtype=np.float64), mag + np.abs(np.asarray(bias, dtype=np.float64))
    return ref, mag


def logit_ratio(got, ref, mag, K, what):
    """Worst |logit - ref| / bound over finite elements; asserts the bound."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite logits (a read outside an input?)"
    err, bnd = np.abs(got - ref), gamma(K + 1) * mag
    ratio = float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0
    print(f"{what}: max |logit - ref| = {err.max():.3e}, worst |logit - ref| / bound = {ratio:.3f}")
    assert (err <= bnd).all(), f"{what}: worst err / bound = {ratio:.3f}"
    return ratio


def lse_reference(logits):
    """(ref, bound) float64 [rows] of fp32 logits [rows, V] -- the derivation in the module docstring."""
    l64 = np.asarray(logits, dtype=np.float64)
    v = l64.shape[-1]
    m = l64.max(axis=-1, keepdims=True)
    d = l64 - m
    e = np.exp(d)
    s = e.sum(axis=-1)
    ref = m[..., 0] + np.log(s)
    tau = (e * (np.exp(np.abs(d) * U) * (1 + 2 * U) - 1)).sum(axis=-1) / s
    eta = (1 + gamma(v)) * (1 + tau) - 1 + v * 2.0 ** -126
    a = -np.log1p(-eta)
    b = 2 * U * (np.abs(np.log(s)) + a)
    c = U * (np.abs(ref) + a + b)
    return ref, a + b + c


def lse_ratio(got, logits, what):
    ref, bnd = lse_reference(logits)
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(ref.shape) - ref)
    ratio = float((err / bnd).max())
    print(f"{what}: max |lse - ref| = {err.max():.3e}, worst |lse - ref| / bound = {ratio:.3f}")
    assert (err <= bnd).all(), f"{what}: worst err / bound = {ratio:.3f}"
    return ratio


def stable_topk(logits, k):
    """ids [rows, k] of fp32 logits [rows, V]: a stable descending sort (the lower id first among equals; -0.0 + 0.0 folds the
    zero signs, so the two zeros are equal keys)."""
    key = -(np.asarray(logits, dtype=np.float32) + np.float32(0.0))
    return np.argsort(key, axis=-1, kind="stable")[..., :k]


# ----------------------------------------------------------------------------------------------------
# refusals: (name, ONE change to the valid call, expected code).  The valid call: B = 2, Q = 3, V = 5, K = 8, k = 2, ldx = 8,
# x_sb = 24, ldw = 8, ldl = 5, every pointer given.  "ptr+<b>": that pointer moved by b bytes; None: a NULL pointer.
# ----------------------------------------------------------------------------------------------------
VALID = dict(x_sb=24, ldx=8, ldw=8, B=2, Q=3, V=5, K=8, k=2, ldl=5)
REFUSALS = [
    ("x NULL alone", {"x": None}, PIO_E_ARG),
    ("w NULL alone", {"w": None}, PIO_E_ARG),
    ("selection without logits", {"x": None, "w": None, "bias": None, "logits": None}, PIO_E_ARG),
    ("selection with a bias", {"x": None, "w": None}, PIO_E_ARG),
    ("no output", {"ids": None, "logprob": None, "lse": None, "logits": None}, PIO_E_ARG),
    ("selection, no output", {"x": None, "w": None, "bias": None, "ids": None, "logprob": None, "lse": None}, PIO_E_ARG),
    ("B=0", {"B": 0}, PIO_E_SHAPE),
    ("Q=0", {"Q": 0}, PIO_E_SHAPE),
    ("B*Q=2^32", {"B": 65536, "Q": 65536}, PIO_E_SHAPE),
    ("V=0", {"V": 0}, PIO_E_SHAPE),
    ("V=1025", {"V": 1025, "ldl": 1025}, PIO_E_SHAPE),
    ("k=0", {"k": 0}, PIO_E_SHAPE),
    ("k=9", {"k": 9, "V": 16, "ldl": 16}, PIO_E_SHAPE),
    ("k>V", {"k": 6}, PIO_E_SHAPE),
    ("K=0", {"K": 0}, PIO_E_SHAPE),
    ("K=6", {"K": 6}, PIO_E_SHAPE),
    ("K=1028", {"K": 1028, "ldx": 1028, "ldw": 1028}, PIO_E_SHAPE),
    ("ldx<K", {"ldx": 4}, PIO_E_SHAPE),
    ("ldw<K", {"ldw": 4}, PIO_E_SHAPE),
    ("ldl<V", {"ldl": 4}, PIO_E_SHAPE),
    ("selection, ldl<V", {"x": None, "w": None, "bias": None, "ldl": 4}, PIO_E_SHAPE),
    ("x 8-byte aligned", {"x": "ptr+8"}, PIO_E_ALIGN),
    ("w 4-byte aligned", {"w": "ptr+4"}, PIO_E_ALIGN),
    ("ldx % 4", {"ldx": 10}, PIO_E_ALIGN),
    ("ldw % 4", {"ldw": 10}, PIO_E_ALIGN),
    ("x_sb % 4", {"x_sb": 26}, PIO_E_ALIGN),
    ("bias misaligned", {"bias": "ptr+2"}, PIO_E_ALIGN),
    ("ids misaligned", {"ids": "ptr+2"}, PIO_E_ALIGN),
    ("logprob misaligned", {"logprob": "ptr+2"}, PIO_E_ALIGN),
    ("lse misaligned", {"lse": "ptr+2"}, PIO_E_ALIGN),
    ("logits misaligned", {"logits": "ptr+2"}, PIO_E_ALIGN),
]


def refusal_fields(ptrs, changes):
    """The valid call with `changes` applied, as {argument: value}; ptrs: pointer argument -> address."""
    f = dict(VALID, **{p: ptrs[p] for p in POINTERS})
    for key, v in changes.items():
        f[key] = (None if v is None else f[key] + int(v[4:])) if key in POINTERS else v
    return f


def call(L, f, stream=None):
    """pio_vocab_topk on the plain keyword values of refusal_fields / the GPU tests."""
    return L.lib().pio_vocab_topk(*[f[a] for a in ARG_ORDER], stream)
