"""CPU: the case table of tests/gemm_act_cases.py (the exact-erf GELU epilogues of pio_gemm_nt) against
csrc/pio_gemm_route.h -- compiled into the driver of tests/test_gemm_addr_host.py -- and against a numpy float32 model
of the epilogue:
  * every case routes, on 256 CUs and with act = 1, to the kernel it names; the act = 1 descriptors the persistent kernels
    do not take (a residual, an fp32 result, a per-row bias) and the few-column shape run on a tile kernel instead;
  * the kernel x output form matrix has no empty cell the route allows (both operand types run every case);
  * every case is exact (operands values of fp16 and bf16, pre-activations values of fp32), covers the 1024-point grid and
    every special point;
  * f32_gelu (gemm_fold_cases) is the header's polynomial, coefficient for coefficient; its deviation from the float64
    reference over the case set's pre-activations stays within the committed G6 / GINF; the reference is torch's
    float64 F.gelu;
  * the model meets every requirement of gemm_act_cases.violation on every case and form, and with any one of the FAULTS
    planted it fails on every case that can see the fault."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_act_cases as AC  # noqa: E402
from test_gemm_addr_host import DRIVER_HEAD, ROOT, descriptor_cpp  # noqa: E402

ROUTED = AC.CASES + AC.REROUTED + [AC.SKINNY_PLAIN]
IDS = [c["id"] for c in AC.CASES]


@functools.lru_cache(maxsize=None)
def routed():
    """id -> kernel (or error code) the route of pio_gemm_route.h answers on 256 CUs"""
    body = [descriptor_cpp(c).replace("show(", f"g.act = {c['act']}; show(") for c in ROUTED]
    src_text = DRIVER_HEAD + "    " + "\n    ".join(body) + "\n    return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "act.cpp"), os.path.join(d, "act")
        with open(src, "w") as f:
            f.write(src_text)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                               os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode()
    return {line.split()[0]: line.split()[1] for line in filter(None, out.split("\n"))}


@functools.lru_cache(maxsize=8)
def _built(cid):
    c = AC.BY_ID[cid]
    arrays = AC.make_arrays(c)
    return (arrays,) + AC.reference(c, arrays)


def test_ids_are_unique():
    ids = [c["id"] for c in ROUTED]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("case", AC.CASES, ids=IDS)
def test_case_routes_to_its_kernel(case):
    assert case["act"] == 1
    assert routed()[case["id"]] == case["kernel"], (case["id"], routed()[case["id"]])


@pytest.mark.parametrize("case", AC.REROUTED, ids=[c["id"] for c in AC.REROUTED])
def test_untaken_act_descriptors_run_elsewhere(case):
    """what gemm_wide_ok / gemm_stream_ok turn away of an act = 1 descriptor reaches a tile kernel under the same override"""
    base = AC.BY_ID[case["base"]]
    got = routed()[case["id"]]
    assert case["act"] == 1 and got == case["expect"] and got != base["kernel"], (case["id"], got)


def test_skinny_shape_is_routed_away_by_the_activation():
    c = AC.BY_ID["skinny_shape"]
    assert routed()[AC.SKINNY_PLAIN["id"]] in ("SKINNY2", "SKINNY4")      # the same descriptor with act = 0
    assert routed()[c["id"]] == c["kernel"] == "T32"


def test_matrix_has_no_empty_cell():
    have = {(c["kernel"], c["form"]) for c in AC.FINITE}
    want = {(k, f) for k in AC.KERNELS for f in AC.FORMS if f != "f32" or k in AC.F32_ACT}
    assert have == want, sorted(want ^ have)
    assert AC.DTYPES == ("f16", "bf16")
    for k in AC.KERNELS:
        mine = [c for c in AC.CASES if c["kernel"] == k]
        assert any(c["nonfinite"] for c in mine)
        assert any(c["n_store"] > c["N"] and c["ldc"] > c["n_store"] for c in mine)
        assert all(c["M"] % AC.TILE_M[k] and c["N"] % AC.TILE_N[k] for c in mine)          # ragged edges on both sides
        if k in AC.F32_ACT:
            assert any(c["order"] and c["res"] and c["alpha"] == 0.5 and c["bias_mode"] == 1 for c in mine)
            assert any(c["bias_mode"] == 2 for c in mine)
        else:
            assert not any(c["res"] or c["out_f32"] or c["bias_mode"] == 2 for c in mine)
        assert any(c["alpha"] != 1.0 for c in mine)
    # gemm_nt_wide: an interior tile beside ragged M and N edges; gemm_nt_stream: more tiles than workgroups
    for c in AC.CASES:
        if c["kernel"] == "WIDE":
            assert c["M"] >= 256 and c["N"] >= 256 and c["M"] % 256 and c["N"] % 256 and c["K"] == 128
        if c["kernel"] == "STREAM":
            tiles = -(-c["M"] // 256) * -(-c["n_store"] // 128)
            grid = min(tiles, AC.N_CU)
            grid = grid & ~7 if grid >= 8 else grid
            assert tiles > grid and c["K"] == 1024


@pytest.mark.parametrize("case", AC.CASES, ids=IDS)
def test_case_is_exact_and_covers_the_domain(case):
    c = case
    arrays, x, ref = _built(c["id"])
    assert AC.exact_ok(c, arrays)
    seen = np.unique(x[np.isfinite(x)])
    if c["id"] == "skinny_shape":       # two columns: every a_m, two b_n (the kernel's domain sweep has its own cases)
        assert len(seen) == 128
        return
    assert np.isin(AC.GRID, seen).all()
    band = AC.NONFINITE if c["nonfinite"] else AC.SPECIALS
    bits = set(x.astype(np.float32).view(np.uint32).reshape(-1).tolist())
    for v in band:
        v = np.float32(0.0) if v == 0 else v       # (+0 acc + -0 bias = +0)
        assert int(np.float32(v).view(np.uint32)) in bits, (c["id"], v)
    if c["nonfinite"]:
        assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any()
    else:
        assert np.isfinite(x).all() and np.isfinite(ref).all()


def test_f32_gelu_is_the_headers_polynomial():
    co = AC.header_coefficients()
    assert len(co) == 8
    x = np.concatenate([AC.GRID, AC.SPECIALS.astype(np.float64), np.linspace(-10, 10, 4001)]).astype(np.float32)
    a, b = AC.f32_gelu(x), AC.gelu_from_header(x)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_model_deviation_is_within_the_committed_constants():
    xs = np.unique(np.concatenate([np.unique(_built(c["id"])[1]) for c in AC.FINITE if c["M"] <= 600]))
    assert np.isin(AC.GRID, xs).all() and np.isin(AC.SPECIALS.astype(np.float64), xs).all()
    dev = np.abs(AC.f32_gelu(xs).astype(np.float64) - AC.gelu64(xs))
    inner = np.abs(xs) <= 6
    g6, at = dev[inner].max(), xs[inner][np.argmax(dev[inner])]
    ginf = (dev[~inner] / np.abs(xs[~inner])).max()
    print(f"f32_gelu against float64: g6 = {g6:.3e} at x = {at!r}, ginf = {ginf:.3e}")
    assert 0.5 * AC.G6 < g6 <= AC.G6 and 0.5 * AC.GINF < ginf <= AC.GINF
    # signs and the non-finite contract of the model
    y = AC.f32_gelu(xs)
    assert (y[xs < 0] <= 0).all() and (y[xs > 0] >= 0).all() and (y[xs == 0] == 0).all() and (np.abs(y) <= np.abs(xs)).all()
    with np.errstate(invalid="ignore"):
        nf = AC.f32_gelu(np.array([np.nan, np.inf, -np.inf], np.float32))
    assert np.isnan(nf[0]) and not np.isfinite(nf[1]) and nf[2] == -np.inf


def test_reference_is_torch_float64_gelu():
    xs = np.concatenate([AC.GRID, AC.SPECIALS.astype(np.float64)])
    want = torch.nn.functional.gelu(torch.from_numpy(xs)).numpy()
    got = AC.gelu64(xs)
    # (torch evaluates 0.5 x (1 + erf(x / sqrt 2)): it cancels in the negative tail, absolutely harmless at 1e-16 |x|)
    assert np.abs(got - want).max() <= 1e-15 * np.maximum(1.0, np.abs(xs)).max() and np.abs(got - want)[np.abs(xs) <= 8].max() < 1e-15


@pytest.mark.parametrize("case", AC.CASES, ids=IDS)
def test_model_passes_and_every_fault_fails(case):
    c = case
    arrays, x, ref = _built(c["id"])
    # the faults on the first two row periods (every row period holds the same pre-activations and no fault looks at
    # the row): the same verdicts as on all M rows of the large cases, in a tenth of the time
    cf = dict(c, M=min(c["M"], 2 * AC.ROW_P))
    arrays_f = AC.make_arrays(cf)
    x_f, ref_f = AC.reference(cf, arrays_f)
    assert np.array_equal(x_f, x[:cf["M"]], equal_nan=True) and np.array_equal(ref_f, ref[:cf["M"]], equal_nan=True)
    for dt in AC.DTYPES:
        hi, lo = AC.model(c, arrays, dt)
        assert (lo is not None) == c["c_lo"]
        assert AC.violation(c, dt, hi, lo, x, ref) is None, (c["id"], dt, AC.violation(c, dt, hi, lo, x, ref))
        for fault in AC.FAULTS:
            if AC.sees(c, fault):
                hi, lo = AC.model(cf, arrays_f, dt, fault)
                assert AC.violation(cf, dt, hi, lo, x_f, ref_f) is not None, f"{c['id']} {dt}: fault {fault} goes unnoticed"


def test_every_fault_is_seen_on_every_kernel():
    for k in AC.KERNELS:
        for fault in AC.FAULTS:
            if fault == "res_before_act" and k not in AC.F32_ACT:
                continue        # (no residual beside act = 1 on the persistent kernels: REROUTED)
            assert any(AC.sees(c, fault) for c in AC.CASES if c["kernel"] == k), (k, fault)


def test_checks_notice_stray_and_missing_values():
    """violation() itself: a non-zero or -0 pad column, a finite result for an infinite input, a finite NaN"""
    c = AC.BY_ID["t32_16"]
    arrays, x, ref = _built(c["id"])
    hi, lo = AC.model(c, arrays, "f16")
    for v in (1.0, -0.0):
        bad = hi.copy()
        bad[3, c["N"] + 1] = v
        assert "pad" in AC.violation(c, "f16", bad, lo, x, ref)
    c = AC.BY_ID["t32_nonfinite"]
    arrays, x, ref = _built(c["id"])
    hi, lo = AC.model(c, arrays, "f16")
    assert AC.violation(c, "f16", hi, lo, x, ref) is None
    for sel in (np.isnan(x), np.isinf(x)):
        bad = hi.copy()
        bad[:, :c["N"]][sel] = 1.0
        assert AC.violation(c, "f16", bad, lo, x, ref) is not None
