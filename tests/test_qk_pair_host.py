"""CPU: the "fp16x3fq" policy (pair-operand Q.K^T in the fused attention cores) on the host side -- policy plumbing, the
C-ABI declarations, and the SELECTION of the raw-core cases the GPU tests run (tests/qk_pair_cases.py), done with the
project's numerics model so that it can be reproduced without a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import perceiver_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numerics_model as NM  # noqa: E402
import qk_pair_cases as QC  # noqa: E402

TOL = 1e-3          # the project's bar (tests/test_parity_gpu.py, tests/test_models.py)
NAMES = ("proj_q", "proj_k", "proj_v", "final", "fc1", "fc2", "final_layer", "post")    # the linears a policy can split


def test_policy_is_known_through_every_selection_route():
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, models as M, runtime as R
    prev = R.get_precision_policy()
    try:
        P.set_precision_policy("fp16x3fq")                                   # 1: the setter
        assert R.get_precision_policy() == "fp16x3fq"
        P.set_precision_policy(prev)
        with R.precision("fp16x3fq"):                                        # 2: the context manager
            assert R.get_precision_policy() == "fp16x3fq"
            assert R.policy_dtype() == (L.PIO_DT_F16, True) == R.policy_dtype("fp16x3f")      # GEMMs as under "fp16x3f":
            assert R.policy().split == R.policy("fp16x3f").split == frozenset(NAMES)           # every weight a pair
            assert all(R.splits(n) and R.splits(n, "fp16x3f") for n in NAMES)
            assert R.policy()._replace(core="fused") == R.policy("fp16x3f")                    # the core alone differs
            assert R.policy().core == "fused_pair" and R.attention_act_split() == 3
        assert R.get_precision_policy() == prev
    finally:
        P.set_precision_policy(prev)
    # 3: the environment variable, in a fresh interpreter (read at import)
    code = "import perceiverio_pytorch_amd.runtime as R; print(R.get_precision_policy(), R.attention_act_split())"
    env = dict(os.environ, PIO_PRECISION="fp16x3fq", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["fp16x3fq", "3"]
    # 4: any part of a model's "cross/stack/decoder" string
    assert M.split_policy3("fp16x3fq/fp16x2o/fp16x3fq") == ("fp16x3fq", "fp16x2o", "fp16x3fq")
    assert [n for n, p in R._POLICIES.items() if p.core == "fused_pair"] == ["fp16x3fq"]
    assert "bf16x3fq" not in R._POLICIES                                     # no bf16 pair core, no bf16 policy name
    # the other policies map as before
    assert [R.attention_act_split(n) for n in ("fp16", "fp16x2w", "fp16x3", "fp16x3f", "fp16x2af", "bf16x3f")] == \
        [0, 0, 1, 2, 2, 2]


def test_c_abi_declares_the_pair_entry_point():
    from perceiverio_pytorch_amd import _lib as L
    for name in ("pio_flash_attention_pair", "pio_flash_attention_pair_workspace_bytes"):
        assert name in L.SIGNATURES
    res, args = L.SIGNATURES["pio_flash_attention_pair"]
    base = L.SIGNATURES["pio_flash_attention"][1]
    assert len(args) == len(base) + 8        # + Q_lo, K_lo, O_lo, kv_mask, q_mask, core, workspace, workspace_bytes
    lib = L.lib()
    assert hasattr(lib, "pio_flash_attention_pair")
    header = open(os.path.join(ROOT, "include", "pio_hip.h")).read()
    assert "pio_flash_attention_pair(" in header and "transformer_primitives.py:138-166" in header
    # host-side answers need no GPU: the key-split partials of the encoder cross-attend shape, nothing for a shape the
    # cross-attention kernel does not cover
    assert lib.pio_flash_attention_pair_workspace_bytes(32, 160, 2, 8, 256, 2048) > 2 * 8 * 256 * 160 * 4
    assert ctypes.sizeof(L.Attention) == ctypes.sizeof(L.Linear) * 8 + 11 * 4 + 4   # layout unchanged (act_split: a value)


@pytest.mark.parametrize("name", sorted(QC.CASES))
def test_case_selection_single_rounding_fails_pair_passes(name):
    """For every raw-core case of the GPU tests: the numpy emulation of the fused core (tools/numerics_model.py core():
    p, v, o rounded once as the kernels do) against the float64 oracle, with q / k rounded once and with q / k as
    hi + fp16(residual).  The cases were chosen (see qk_pair_cases.py) so that the single rounding is above 2 TOL on at
    least one of the two project figures and the pair below TOL / 2 on both, with |s| <= 20; both are asserted."""
    q, k, v, km, qm = QC.gen(name)
    c = QC.CASES[name]
    ref, smax = QC.oracle(name, q, k, v, km, qm)
    m3 = QC.mask3(name, km, qm)
    pts = ["q", "k", "v", "p", "o"]
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    one = NM.core(f64(q), f64(k), f64(v), c["H"], NM.Rounder("f16", pts), m3)
    two = NM.core(f64(q), f64(k), f64(v), c["H"], NM.Rounder("f16", pts, pair=("q", "k")), m3)
    e1, e2 = O.rel_errors(one, ref), O.rel_errors(two, ref)
    print(f"{name}: max|s|={smax:.2f} single {e1[0]:.3e} / {e1[1]:.3e}  pair {e2[0]:.3e} / {e2[1]:.3e}")
    assert smax <= 20.0
    assert max(e2) < TOL / 2, (name, e2)
    if name not in QC.NO_TEETH:               # (qk_pair_cases.py says why that one is exempt; none of the issue's shapes is)
        assert max(e1) > 2 * TOL, (name, e1)
    assert not set(QC.MUST_FAIL) & set(QC.NO_TEETH)


def test_small_logit_variant_stays_below_one():
    """(a property of the test inputs, not of the feature: the GPU test's small-logit leg relies on it)"""
    for name in QC.MUST_FAIL:
        q, k, v, km, qm = QC.gen(name, small=True)
        assert QC.oracle(name, q, k, v, km, qm)[1] <= 1.0
