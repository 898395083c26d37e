"""Raw attention-core cases of the pair-operand Q.K^T tests (shared by tests/test_qk_pair_host.py, which SELECTS them on
the CPU with tools/numerics_model.py, and tests/test_qk_pair_gpu.py, which runs them on the kernels).  Seeded numpy only.

Why these inputs.  One fp16 rounding of q and k puts an error of about 2^-11 sqrt(sum_i q_i^2 k_i^2 / dk) into a logit:
what counts is the size of the PRODUCTS q_i k_i, not of their sum.  Trained models (LayerNorm gains up to 5 in front of
the projections) carry large common-mode components in q and k that cancel inside the logit; the cases do the same in the
open: q = A + sigma n, k = A (+1, -1, +1, ...) + sigma n', so that the logits stay small (|s| <= 6, far inside the
|s| <= 20 the issue allows) while the products are A^2 = 36.  The values are uniform in (-1, 1) with one constant channel
per head (what a proj_v bias produces): it fixes the abs-max the second project figure divides by, so that the figure does
not hinge on where the largest output happens to fall between two powers of two.
"""
import numpy as np

A, SIGMA, DC = 6.0, 0.1, 0.46875        # common-mode amplitude, spread, constant value channel (exact in fp16)
DK = 32

# name: core ("flash": flash_attn_kernel, "xattn": xattn_kernel), B, H, Tq, Tk, dv, key mask, query mask
#   key mask "ragged": ~30 % of the keys masked at random; sample B-1 of "ragged+dead" has NO attendable key (its rows are
#   wiped to zeros); query mask: ~30 % of the rows masked (written as zeros)
CASES = {
    "self_256": dict(core="flash", B=2, H=8, Tq=256, Tk=256, dv=160, km=None, qm=False),
    "self_512": dict(core="flash", B=1, H=8, Tq=512, Tk=512, dv=160, km=None, qm=False),
    # rows not a multiple of 128, keys not a multiple of 64: the tail paths of the self-attention kernel
    "self_200x300": dict(core="flash", B=1, H=8, Tq=200, Tk=300, dv=160, km=None, qm=False),
    # 2 x 8 x 2 = 32 workgroups over 64 key tiles: the key split (8 parts) and xattn_reduce_kernel
    "enc_256x2048": dict(core="xattn", B=2, H=8, Tq=256, Tk=2048, dv=160, km="ragged", qm=True),
    # ragged Tk (not a multiple of 32), 200 rows, one sample without an attendable key, key split
    "enc_200x2029": dict(core="xattn", B=2, H=8, Tq=200, Tk=2029, dv=160, km="ragged+dead", qm=True),
    "dec_2048x256": dict(core="xattn", B=1, H=8, Tq=2048, Tk=256, dv=96, km=None, qm=True),
    "dec_300x250": dict(core="xattn", B=2, H=8, Tq=300, Tk=250, dv=96, km="ragged+dead", qm=True),
    # the remaining pair instantiations of flash_attn_kernel, chosen by the launcher from the shape ("vrow": V row-major,
    # the layout of a fused q|k|v buffer): 32 workgroups <= CUs and Tk % 128 == 0 -> the key axis split over two wave groups
    # (KS = 2, merge through LDS); (32, 32) heads over 1024 keys -> four wave groups (KS = 4); >= 256 workgroups of 256
    # rows -> 8 waves (NW = 8); otherwise 4 waves; and the (32, 32) head on V^T
    "self_rm_ks2": dict(core="flash", B=2, H=8, Tq=256, Tk=256, dv=160, km=None, qm=False, vrow=True),
    "self_rm_nw8": dict(core="flash", B=4, H=8, Tq=2048, Tk=256, dv=160, km=None, qm=False, vrow=True),
    "self_rm_nw4": dict(core="flash", B=2, H=8, Tq=200, Tk=320, dv=160, km=None, qm=False, vrow=True),
    "self32_rm_ks4": dict(core="flash", B=1, H=8, Tq=256, Tk=1024, dv=32, km=None, qm=False, vrow=True),
    "self32_rm_ks2": dict(core="flash", B=2, H=8, Tq=256, Tk=256, dv=32, km=None, qm=False, vrow=True),
    "self32_rm_nw8": dict(core="flash", B=4, H=8, Tq=2048, Tk=192, dv=32, km=None, qm=False, vrow=True),
    "self32_rm_nw4": dict(core="flash", B=2, H=8, Tq=200, Tk=320, dv=32, km=None, qm=False, vrow=True),
    "self32_vt": dict(core="flash", B=2, H=8, Tq=256, Tk=256, dv=32, km=None, qm=False),
}
# the shapes the issue names; every one of them is in the "must fail without the feature" set (none had to be dropped)
MUST_FAIL = ["self_256", "self_512", "enc_256x2048", "dec_2048x256"]
# Covered for correctness only: with 1024 keys averaged into a 32-wide head the single-rounding emulation reaches
# 1.6e-3 / 1.1e-3 -- above TOL, below the 2 TOL the selection demands -- so the case carries no "single-operand must
# fail" claim (the bound is not loosened for it; the KS = 4 kernel is the same code as KS = 2, which has one).
NO_TEETH = ["self32_rm_ks4"]


def gen(name, small=False):
    """q [B,Tq,H*32], k [B,Tk,H*32], v [B,Tk,H*dv] (float32), kv_mask [B,Tk] / q_mask [B,Tq] (bool or None).
    small=True: plain N(0, 0.35^2) q and k -- logits |s| <= 1."""
    c = CASES[name]
    B, H, Tq, Tk, dv = c["B"], c["H"], c["Tq"], c["Tk"], c["dv"]
    r = np.random.default_rng(sum(map(ord, name)))
    nq, nk = r.standard_normal((B, Tq, H * DK)), r.standard_normal((B, Tk, H * DK))
    if small:
        q, k = 0.35 * nq, 0.35 * nk
    else:
        sign = np.tile(np.array([1.0, -1.0]), H * DK // 2)
        q, k = A + SIGMA * nq, A * sign + SIGMA * nk
    v = r.uniform(-1.0, 1.0, (B, Tk, H * dv))
    v[:, :, ::dv] = DC
    km = qm = None
    if c["km"]:
        km = r.random((B, Tk)) > 0.3
        km[:, 0] = True
        if c["km"].endswith("dead"):
            km[B - 1, :] = False
    if c["qm"]:
        qm = r.random((B, Tq)) > 0.3
    return q.astype(np.float32), k.astype(np.float32), v.astype(np.float32), km, qm


def mask3(name, km, qm):
    c = CASES[name]
    if km is None and qm is None:
        return None
    qv = qm if qm is not None else np.ones((c["B"], c["Tq"]), bool)
    kv = km if km is not None else np.ones((c["B"], c["Tk"]), bool)
    return np.logical_and(qv[:, :, None], kv[:, None, :])


def oracle(name, q, k, v, km, qm):
    """float64 oracle of the core (oracle/perceiver_oracle.py attend) and the largest |logit|."""
    import perceiver_oracle as O
    c = CASES[name]
    B, H, Tq, Tk, dv = c["B"], c["H"], c["Tq"], c["Tk"], c["dv"]
    q4 = q.astype(np.float64).reshape(B, Tq, H, DK)
    k4 = k.astype(np.float64).reshape(B, Tk, H, DK)
    smax = float(np.abs(np.einsum("bqhd,bkhd->bhqk", q4, k4)).max() / np.sqrt(DK))
    return O.attend(q4, k4, v.astype(np.float64).reshape(B, Tk, H, dv), mask3(name, km, qm)), smax
