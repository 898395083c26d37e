"""Raw attention-core cases of the pair-operand Q.K^T tests on the 128-wide head (dk = dv = 128: the latent stack of the
classifier), shared by tests/test_qk_pair_wide_host.py, which SELECTS them on the CPU with tools/numerics_model.py, and
tests/test_qk_pair_wide_gpu.py, which runs them on flash_attn_kernel.  Seeded numpy only.

The inputs are built as in tests/qk_pair_cases.py (which says why): q = A + sigma n, k = A (+1, -1, ...) + sigma n', so
the products q_i k_i are A^2 = 36 while the logits stay small; v uniform in (-1, 1) with one constant channel per head.
"""
import numpy as np

A, SIGMA, DC = 6.0, 0.1, 0.46875        # as qk_pair_cases.py
DK = DV = 128

# name: B, H, Tq, Tk, V layout (vrow: row-major [keys][H*dv], else V^T), and the variant flash_pair_route must name at 256
# CUs (waves per workgroup, key parts).  The single-operand route would split the keys of "w128_rm_256" (KS = 2).
CASES = {
    "w128_256": dict(B=1, H=2, Tq=256, Tk=256, vrow=False, NW=4, KS=1),
    "w128_200x300": dict(B=1, H=2, Tq=200, Tk=300, vrow=False, NW=4, KS=1),            # row and key tails
    "w128_rm_256": dict(B=2, H=8, Tq=256, Tk=256, vrow=True, NW=4, KS=1),
    "w128_rm_200x320": dict(B=2, H=8, Tq=200, Tk=320, vrow=True, NW=4, KS=1),          # tails
    "w128_rm_nw8": dict(B=4, H=8, Tq=2048, Tk=192, vrow=True, NW=8, KS=1),             # 256 workgroups of 256 rows
    "w128_1024": dict(B=1, H=2, Tq=128, Tk=1024, vrow=False, NW=4, KS=1),              # 16 key tiles
}


def gen(name, small=False):
    """q [B,Tq,H*128], k [B,Tk,H*128], v [B,Tk,H*128] (float32).  small=True: plain N(0, 0.35^2) q and k."""
    c = CASES[name]
    B, H, Tq, Tk = c["B"], c["H"], c["Tq"], c["Tk"]
    r = np.random.default_rng(sum(map(ord, name)))
    nq, nk = r.standard_normal((B, Tq, H * DK)), r.standard_normal((B, Tk, H * DK))
    if small:
        q, k = 0.35 * nq, 0.35 * nk
    else:
        sign = np.tile(np.array([1.0, -1.0]), H * DK // 2)
        q, k = A + SIGMA * nq, A * sign + SIGMA * nk
    v = r.uniform(-1.0, 1.0, (B, Tk, H * DV))
    v[:, :, ::DV] = DC
    return q.astype(np.float32), k.astype(np.float32), v.astype(np.float32)


_ORACLE = {}


def oracle(name, small=False):
    """(q, k, v, float64 oracle of the core -- oracle/perceiver_oracle.py attend --, largest |logit|); computed once."""
    key = (name, small)
    if key not in _ORACLE:
        import perceiver_oracle as O
        c = CASES[name]
        B, H, Tq, Tk = c["B"], c["H"], c["Tq"], c["Tk"]
        q, k, v = gen(name, small)
        q4 = q.astype(np.float64).reshape(B, Tq, H, DK)
        k4 = k.astype(np.float64).reshape(B, Tk, H, DK)
        smax = float(np.abs(np.einsum("bqhd,bkhd->bhqk", q4, k4)).max() / np.sqrt(DK))
        ref = O.attend(q4, k4, v.astype(np.float64).reshape(B, Tk, H, DV), None)
        for a in (q, k, v, ref):
            a.setflags(write=False)
        _ORACLE[key] = (q, k, v, ref, smax)
    return _ORACLE[key]
