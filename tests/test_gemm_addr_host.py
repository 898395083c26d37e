"""CPU: the case table of tests/gemm_addr_cases.py against csrc/pio_gemm_route.h (compiled with g++ into a driver, as
tests/test_gemm_route.py does) and against torch:
  * every case routes, on 256 CUs, to the kernel it names, and gemm_params derives the alignment classes, sweep count,
    B_lo start and residual form the case's layout implies (the fake pointers carry the real offsets' low bits);
  * every GemmKernel enumerator has a case, every (kernel, feature) pair has a case or an entry in REFUSED / REROUTED
    whose outcome the driver confirms; the required pairs include the epilogue forms of REQUIRED_EXTRA, and
    test_no_entry_can_be_removed shows that the coverage fails without any one case or entry;
  * every case is exact (exact_ok) and its result is representable in fp32;
  * ref_gemm equals a float64 einsum over torch.as_strided views of the same buffers."""
import functools
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_addr_cases as GC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER_HEAD = r'''
#include <stdio.h>
#include "pio_gemm_route.h"
using namespace pio;
static char *ptr(int i, long bytes) { return (char *)(uintptr_t)(0x10000000ull * (uint64_t)i + (uint64_t)bytes); }
static const char *name(GemmKernel k) {
    switch (k) {
    case GemmKernel::NONE: return "NONE";
    case GemmKernel::SKINNY2: return "SKINNY2";
    case GemmKernel::SKINNY4: return "SKINNY4";
    case GemmKernel::WIDE: return "WIDE";
    case GemmKernel::STREAM: return "STREAM";
    case GemmKernel::T256: return "T256";
    case GemmKernel::T128: return "T128";
    case GemmKernel::T128_KG2: return "T128_KG2";
    case GemmKernel::T64: return "T64";
    case GemmKernel::T64_KG2: return "T64_KG2";
    case GemmKernel::T32: return "T32";
    case GemmKernel::T32_KG2: return "T32_KG2";
    }
    return "?";
}
static void show(const char *id, const pio_gemm_t &g, int forced) {
    GemmParams p = {};
    int err = gemm_params(g, &p);
    GemmRoute r = {};
    if (!err) {
        r = gemm_route(g, p, forced, 256);
        err = r.err;
    }
    const char *what = err == PIO_E_SHAPE ? "PIO_E_SHAPE" : err == PIO_E_ALIGN ? "PIO_E_ALIGN" : err == PIO_E_ARG ? "PIO_E_ARG"
                       : err ? "error" : name(r.kernel);
    printf("%s %s %d %d %d %d %d %d\n", id, what, p.vec_ok, p.r_vec, p.bias_vec, p.npass, p.lo_n0, p.r_rows);
}
int main() {
    pio_gemm_t g;
'''


def descriptor_cpp(c):
    """C++ statements filling `g` for the case: fake pointers with the low bits of the real ones."""
    esz = 4 if c["out_f32"] else 2
    s = ["g = pio_gemm_t{};",
         "g.A = ptr(1, 0); g.B = ptr(3, 0);",
         f"g.C = ptr(5, {c['c_off'] * esz});"]
    if c["a_lo"]:
        s.append("g.A_lo = ptr(2, 0);")
    if c["b_lo"]:
        s.append("g.B_lo = ptr(4, 0);")
    if c["c_lo"]:
        s.append(f"g.C_lo = ptr(6, {c['c_off'] * esz});")
    if c["bias_mode"]:
        s.append(f"g.bias = (const float *)ptr(7, {c['bias_off'] * 4});")
    if c["res"]:
        s.append(f"g.R = (const float *)ptr(8, {c['r_off'] * 4}); g.ldr = {c['ldr']}; g.r_stride_b = {c['r_stride_b']}; "
                 f"g.r_rows_per_batch = {c['r_rows']};")
    for k in ("M", "N", "K", "lda", "ldb", "ldc", "batch", "nh", "sAb", "sAh", "sBb", "sBh", "sCb", "sCh", "bias_mode",
              "out_f32", "n_store", "b_lo_n0"):
        s.append(f"g.{k} = {c[k]};")
    s.append(f"g.alpha = {c['alpha']!r}f; g.dtype = PIO_DT_F16;")
    s.append(f'show("{c["id"]}", g, {c["override"]});')
    return "\n    ".join(s)


ALL = [c for c in GC.CASES + GC.MODEL_CASES + GC.REFUSED + GC.REROUTED if not c.get("missing_base")]


@functools.lru_cache(maxsize=None)
def routed():
    src_text = DRIVER_HEAD + "    " + "\n    ".join(descriptor_cpp(c) for c in ALL) + "\n    return 0;\n}\n"
    inc = os.path.join(ROOT, "include")
    csrc = os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "addr.cpp")
        with open(src, "w") as f:
            f.write(src_text)
        exe = os.path.join(d, "addr")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", inc, "-I", csrc, src, "-o", exe])
        out = subprocess.check_output([exe]).decode()
    got = {}
    for line in filter(None, out.split("\n")):
        f = line.split()
        got[f[0]] = (f[1], dict(zip(("vec_ok", "r_vec", "bias_vec", "npass", "lo_n0", "r_rows"), map(int, f[2:]))))
    return got


def test_ids_are_unique():
    ids = [c["id"] for c in ALL]
    assert len(ids) == len(set(ids))


def test_driver_names_every_enumerator():
    """the driver's switch (compiled with -Wall -Werror: an enumerator it misses fails the build) and KERNELS agree with
    the enum of pio_gemm_route.h"""
    text = open(os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc", "pio_gemm_route.h")).read()
    body = re.search(r"enum class GemmKernel \{(.*?)\n\};", text, re.S).group(1).split("#ifdef")[0]
    names = re.findall(r"^\s*([A-Z][A-Z0-9_]*),", body, re.M)
    assert set(names) == set(GC.KERNELS) | {"NONE"}


@pytest.mark.parametrize("case", GC.CASES + GC.MODEL_CASES, ids=[c["id"] for c in GC.CASES + GC.MODEL_CASES])
def test_case_routes_to_its_kernel(case):
    kernel, flags = routed()[case["id"]]
    assert kernel == case["kernel"], (case["id"], kernel)
    assert flags == GC.derived(case), (case["id"], flags, GC.derived(case))
    assert case["features"] == GC.features_of(case)
    # a case meant for the (stride_b, rows_per_batch) form survives gemm_params' collapse of contiguous batches
    assert ("res_rows" in case["features"]) == (flags["r_rows"] > 0)
    assert ("c_unaligned" in case["features"]) == (flags["vec_ok"] == 0)
    if case["res"]:
        assert ("res_unaligned" in case["features"]) == (flags["r_vec"] == 0)
    if case["bias_mode"] == 1:
        assert ("bias_unaligned" in case["features"]) == (flags["bias_vec"] == 0)
    assert ("b_lo_from" in case["features"]) == (flags["lo_n0"] > 0)


@pytest.mark.parametrize("case", GC.REFUSED + GC.REROUTED, ids=[c["id"] for c in GC.REFUSED + GC.REROUTED])
def test_refused_pairs_are_refused(case):
    """The variant asks the base case's kernel for one more feature: the driver answers with the error code (REFUSED) or
    with another kernel (REROUTED) -- never with the kernel the pair names."""
    assert not case.get("missing_base"), f"{case['id']}: its base case {case['base']} is gone from CASES"
    got, flags = routed()[case["id"]]
    base = GC.BY_ID[case["base"]]
    assert case["feature"] in case["features"]
    if base["kernel"] == case["kernel"]:        # (else the base is another kernel's case that already has the feature)
        assert case["feature"] not in base["features"]
    assert got == case["expect"] and got != case["kernel"], (case["id"], got)
    if case in GC.REFUSED:
        assert got.startswith("PIO_E_")
    else:
        assert got in GC.KERNELS and flags == GC.derived(case)


def _required():
    return {(k, f) for k in GC.KERNELS for f in GC.FEATURES} | set(GC.REQUIRED_EXTRA)


def _provides(c):
    return {(c["kernel"], f) for f in c["features"] | c["extras"]} & _required()


def test_kernel_feature_matrix_is_covered():
    assert {c["kernel"] for c in GC.CASES} == set(GC.KERNELS)
    have = set().union(*[_provides(c) for c in GC.CASES])
    away = {(c["kernel"], c["feature"]) for c in GC.REFUSED + GC.REROUTED}
    assert not (have & away), sorted(have & away)
    missing = _required() - have - away
    assert not missing, sorted(missing)
    assert len(away) == len(GC.REFUSED) + len(GC.REROUTED)                     # no entry twice
    for c in GC.CASES:
        assert c["features"] <= set(GC.FEATURES) and c["extras"] <= set(GC.EXTRAS)
    assert {e for _, e in GC.REQUIRED_EXTRA} <= set(GC.EXTRAS) and {k for k, _ in GC.REQUIRED_EXTRA} <= set(GC.KERNELS)
    # what the pair matrix cannot say
    res_rows = [c for c in GC.CASES if "res_rows" in c["features"]]
    assert any(c["r_stride_b"] == 0 for c in res_rows) and any(c["r_stride_b"] % 4 for c in res_rows)
    assert any(c["out_f32"] and c["c_off"] % 4 == 2 for c in GC.CASES)          # fp32 C 8 bytes off
    assert any(c["ldc"] % 2 for c in GC.CASES)                                   # an odd pitch
    assert any(c["b_lo_n0"] == 256 for c in GC.CASES)
    assert any(c["kernel"] == "T256" and c["batch"] > 1 for c in GC.CASES)
    assert any(c["kernel"] == "STREAM" and c["batch"] > 1 and c["b_lo"] for c in GC.CASES)
    assert any(c["kernel"] == "WIDE" and c["c_lo"] and c["res"] for c in GC.CASES)
    assert any(c["alpha"] not in (0.0, 1.0) for c in GC.CASES)
    assert {c["id"] for c in GC.MODEL_CASES} == {"model_qk", "model_pv"}


@pytest.mark.parametrize("gone", GC.CASES + GC.REFUSED + GC.REROUTED,
                         ids=[c["id"] for c in GC.CASES + GC.REFUSED + GC.REROUTED])
def test_no_entry_can_be_removed(gone):
    """Every case is the only provider of at least one required (kernel, feature) pair, and every REFUSED / REROUTED entry
    the only one that accounts for its pair: the coverage above fails without it."""
    cases = [c for c in GC.CASES if c is not gone]
    away = {(c["kernel"], c["feature"]) for c in GC.REFUSED + GC.REROUTED if c is not gone}
    have = set().union(*[_provides(c) for c in cases])
    assert _required() - have - away, f"{gone['id']} could be deleted without the coverage noticing"


@functools.lru_cache(maxsize=None)
def _arrays_and_ref(cid):
    c = next(c for c in GC.CASES + GC.MODEL_CASES if c["id"] == cid)
    arrays = GC.make_arrays(c)
    return arrays, GC.ref_gemm(c, arrays)


@pytest.mark.parametrize("case", GC.CASES + GC.MODEL_CASES, ids=[c["id"] for c in GC.CASES + GC.MODEL_CASES])
def test_case_is_exact_and_reference_matches_torch(case):
    c = case
    arrays, (ref, index, pad) = _arrays_and_ref(c["id"])
    assert GC.exact_ok(c, arrays)
    assert np.isfinite(ref).all() and (ref == np.rint(ref * 2) / 2).all()
    for dt in GC.DTYPES:
        hi, lo = GC.expected_images(c, ref, dt)
        assert np.isfinite(hi).all()
        if c["out_f32"]:
            assert np.array_equal(hi.astype(np.float64), ref)
        elif lo is not None:       # hi + lo of a 16-bit pair: lo is the correctly rounded remainder
            assert np.abs(hi.astype(np.float64) + lo - ref).max() <= np.abs(ref).max() * 2.0 ** (-16 if dt == "bf16" else -21)
    # the written set: distinct elements inside the payload, the pad columns among them
    assert len(np.unique(index)) == index.size and index.min() >= c["c_off"] and index.max() < GC.c_elements(c)
    assert (ref[:, :, pad] == 0).all() and pad.sum() == c["n_store"] - c["N"]

    # float64 einsum over as_strided views of the same payloads
    nh, nb, M, N, K = c["nh"], c["batch"] // c["nh"], c["M"], c["N"], c["K"]

    def view(buf, sb, sh, rows, ld):
        return torch.as_strided(torch.from_numpy(buf), (nb, nh, rows, K), (sb, sh, ld, 1)).double()

    A, B = view(arrays["A"], c["sAb"], c["sAh"], M, c["lda"]), view(arrays["B"], c["sBb"], c["sBh"], N, c["ldb"])
    assert torch.isfinite(A).all() and torch.isfinite(B).all()
    want = torch.einsum("bhmk,bhnk->bhmn", A, B)
    if c["a_lo"]:
        want += torch.einsum("bhmk,bhnk->bhmn", view(arrays["A_lo"], c["sAb"], c["sAh"], M, c["lda"]), B)
    if c["b_lo"]:
        n0 = c["b_lo_n0"]
        Bl = view(arrays["B_lo"], c["sBb"], c["sBh"], N, c["ldb"])
        assert torch.isnan(Bl[:, :, :n0]).all() and torch.isfinite(Bl[:, :, n0:]).all()
        want[..., n0:] += torch.einsum("bhmk,bhnk->bhmn", A, Bl[:, :, n0:])
    want *= c["alpha"]
    if c["bias_mode"] == 1:
        want += torch.from_numpy(arrays["bias"][c["bias_off"]:c["bias_off"] + N]).double()
    elif c["bias_mode"] == 2:
        want += torch.from_numpy(arrays["bias"][c["bias_off"]:c["bias_off"] + M]).double()[:, None]
    if c["res"]:
        rr = c["r_rows"] if c["r_rows"] > 0 else M
        sb = c["r_stride_b"] if c["r_rows"] > 0 else 0
        nbat = (M + rr - 1) // rr
        Rbuf = torch.from_numpy(arrays["R"])
        rows = [torch.as_strided(Rbuf, (min(rr, M - b * rr), N), (c["ldr"], 1), c["r_off"] + b * sb) for b in range(nbat)]
        want += torch.cat(rows).double()
    assert np.array_equal(want.reshape(c["batch"], M, N).numpy(), ref[:, :, :N])
