"""CPU: the case table of tests/gemm_fold_cases.py against csrc/pio_gemm_route.h (compiled with g++ into a driver, as
tests/test_gemm_addr_host.py does) and the references against torch and against float32 restatements:
  * every case routes, at its n_cu, to the kernel it names; every REFUSED / REROUTED entry gets the answer it expects;
  * every (role, kernel, feature) cell the predicates admit has a case, every other one a confirmed refusal; the fold
    reaches gemm_nt_wide and the six tile kernels and no other kernel (a sweep of small descriptors shows it);
  * test_no_entry_can_be_removed: the coverage fails without any one case or entry;
  * the premises of the bit-for-bit families hold (exact_ok); the consumer's formula is the LayerNorm of
    transformer_primitives.py:281-292 (consistent cases against torch float64);
  * every bound holds for a float32 restatement of the reference alone: SUM_BOUND in three summation orders, CONS_BOUND
    for both evaluation orders within half the bound, GELU_G against the measured deviation of the polynomial."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_fold_cases as FC  # noqa: E402
from test_gemm_addr_host import DRIVER_HEAD  # noqa: E402  (pio_gemm_route.h, ptr(), name())

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the addressing driver's head up to its show(): ptr() and name() are shared, show() here takes the CU count
HEAD = DRIVER_HEAD[:DRIVER_HEAD.index("static void show(")] + r'''
static void show(const char *id, const pio_gemm_t &g, int forced, int n_cu) {
    GemmParams p = {};
    int err = gemm_params(g, &p);
    GemmRoute r = {};
    if (!err) {
        r = gemm_route(g, p, forced, n_cu);
        err = r.err;
    }
    const char *what = err == PIO_E_SHAPE ? "PIO_E_SHAPE" : err == PIO_E_ALIGN ? "PIO_E_ALIGN" : err == PIO_E_ARG ? "PIO_E_ARG"
                       : err ? "error" : name(r.kernel);
    printf("%s %s %u\n", id, what, r.grid_x);
}
// every kernel a fold descriptor of a small sweep reaches, per role: "sweep <role> <kernel>" lines
static void sweep() {
    static const int Ms[] = {40, 300, 1100, 2100, 4200}, Ns[] = {64, 128, 256, 384, 1024, 2048}, Ks[] = {128, 256, 1024, 1536};
    static const int Fs[] = {0, 1, 2, 64, 128, 256}, CUs[] = {256, 8};
    for (int role = 0; role < 2; ++role)
    for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int f : Fs) for (int cu : CUs) for (int form = 0; form < 2; ++form) {
        pio_gemm_t g = pio_gemm_t{};
        g.A = ptr(1, 0); g.B = ptr(3, 0);
        g.M = M; g.N = N; g.K = K; g.lda = g.ldb = K; g.ldc = N; g.batch = g.nh = 1; g.n_store = N; g.alpha = 1.0f;
        g.dtype = PIO_DT_F16;
        if (role == 0) {
            g.out_f32 = 1; g.X16 = ptr(9, 0); g.X16_lo = ptr(10, 0); g.R16_hi = ptr(9, 0); g.R16_lo = ptr(10, 0); g.ld16 = N;
            g.row_part = (float *)ptr(11, 0); g.row_slot_w = form ? 64 : 128;
        } else {
            g.C = ptr(5, 0); g.ln_part = (const float *)ptr(12, 0); g.ln_c = (const float *)ptr(13, 0); g.ln_eps = 0.25f;
            g.ln_slots = form ? K / 64 : K / 128;
        }
        GemmParams p = {};
        if (gemm_params(g, &p)) continue;
        GemmRoute r = gemm_route(g, p, f, cu);
        if (!r.err) printf("sweep %s %s 0\n", role ? "cons" : "prod", name(r.kernel));
    }
}
int main() {
    pio_gemm_t g;
    sweep();
'''


def descriptor_cpp(c):
    """C++ statements filling `g` for the case: fake pointers with the low bits of the real ones."""
    prod = c["role"] == "prod"
    s = ["g = pio_gemm_t{};", "g.A = ptr(1, 0); g.B = ptr(3, 0);"]
    if c["a_lo"]:
        s.append("g.A_lo = ptr(2, 0);")
    if c["b_lo"]:
        s.append("g.B_lo = ptr(4, 0);")
    if c["bias"]:
        s.append(f"g.bias = (const float *)ptr(7, {c['bias_off'] * 4}); g.bias_mode = 1;")
    for k in ("M", "N", "K", "lda", "ldb", "ldc", "n_store"):
        s.append(f"g.{k} = {c[k]};")
    s.append(f"g.batch = 1; g.nh = 1; g.alpha = {c['alpha']!r}f; g.dtype = PIO_DT_F16; g.act = {c['act']};")
    if prod:
        s.append(f"g.out_f32 = 1; g.X16 = ptr(9, 0); g.ld16 = {c['ld16']}; g.row_part = (float *)ptr(11, 0); "
                 f"g.row_slot_w = {c['slot_w']};")
        if c["c"]:
            s.append("g.C = ptr(5, 0);")
        if c["x_lo"]:
            s.append("g.X16_lo = ptr(10, 0);")
        if c["res"] == "f32":
            s.append(f"g.R = (const float *)ptr(8, 0); g.ldr = {c['ldr']};")
        else:
            same = c["res"] == "inplace"
            s.append(f"g.R16_hi = ptr({9 if same else 14}, 0); g.R16_lo = ptr({10 if same else 15}, 0);")
        if c["flag"] != "null":
            s.append("g.range_flag = (int32_t *)ptr(16, 0);")
    else:
        s.append(f"g.C = ptr(5, 0); g.ln_part = (const float *)ptr(12, {c['part_off'] * 4}); "
                 f"g.ln_c = (const float *)ptr(13, {c['lnc_off'] * 4}); g.ln_eps = {FC.EPS}f; g.ln_slots = {c['ln_slots']};")
        if c["c_lo"]:
            s.append("g.C_lo = ptr(6, 0);")
    s.append(f'show("{c["id"]}", g, {c["override"]}, {c["n_cu"]});')
    return "\n    ".join(s)


ALL = [c for c in FC.CASES + FC.REFUSED + FC.REROUTED if not c.get("missing_base")]


@functools.lru_cache(maxsize=None)
def routed():
    src_text = HEAD + "    " + "\n    ".join(descriptor_cpp(c) for c in ALL) + "\n    return 0;\n}\n"
    inc = os.path.join(ROOT, "include")
    csrc = os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "fold.cpp")
        with open(src, "w") as f:
            f.write(src_text)
        exe = os.path.join(d, "fold")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", inc, "-I", csrc, src, "-o", exe])
        out = subprocess.check_output([exe]).decode()
    got, swept = {}, set()
    for line in filter(None, out.split("\n")):
        f = line.split()
        if f[0] == "sweep":
            swept.add((f[1], f[2]))
        else:
            got[f[0]] = (f[1], int(f[2]))
    return got, swept


def test_ids_are_unique():
    ids = [c["id"] for c in ALL]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("case", FC.CASES, ids=[c["id"] for c in FC.CASES])
def test_case_routes_to_its_kernel(case):
    kernel, grid = routed()[0][case["id"]]
    assert kernel == case["kernel"], (case["id"], kernel)
    assert case["features"] == FC.features_of(case) and case["extras"] == FC.extras_of(case)
    assert case["family"] == FC.family_of(case)
    assert case["features"] <= set(FC.PROD_FEATURES if case["role"] == "prod" else FC.CONS_FEATURES)
    assert case["extras"] <= set(FC.EXTRAS)
    assert case["n_cu"] in (256, 8)
    if kernel == "WIDE":   # the grid the staged / direct bookkeeping of extras_of assumes
        tiles = -(-case["M"] // 256) * -(-case["N"] // 256)
        assert grid == FC.persistent_grid(tiles, case["n_cu"])
    if "two_tiles_per_wg" in case["features"]:
        # 16 or more tiles on the 8-CU budget, no fp32 C: every workgroup runs the direct epilogue, then the staged one
        assert case["n_cu"] == 8 and grid == 8 and not case["c"] and case["N"] % 256 == 0
        assert -(-case["M"] // 256) * (case["N"] // 256) >= 16
    if case["kernel"].startswith("T32") and case["role"] == "cons":
        # the register prefetch of the statistics (pre_stat): up to 24 slots, ln_part 8-byte aligned
        assert (case["ln_slots"] <= 24 and case["part_off"] % 2 == 0) == ("slots_gt24" not in case["features"]
                                                                          and "ln_part_4B" not in case["extras"])


@pytest.mark.parametrize("case", FC.REFUSED + FC.REROUTED, ids=[c["id"] for c in FC.REFUSED + FC.REROUTED])
def test_refused_cells_are_refused(case):
    """The variant asks the base case's kernel for one more feature: the driver answers with the error code (REFUSED) or
    with another kernel (REROUTED) -- never with the kernel the cell names."""
    assert not case.get("missing_base"), f"{case['id']}: its base case {case['base']} is gone from CASES"
    got = routed()[0][case["id"]][0]
    base = FC.BY_ID[case["base"]]
    assert base["kernel"] == case["kernel"] and case["feature"] not in base["features"]
    assert got == case["expect"] and got != case["kernel"], (case["id"], got)
    assert got.startswith("PIO_E_") if case in FC.REFUSED else got in FC.TILE_KERNELS


def _away(entries):
    return {(c["role"], c["kernel"], c["feature"]) for c in entries}


def _matrix():
    """every (role, kernel, feature) cell: the union of what is required and what must be turned away"""
    cells = {("prod", k, f) for k in FC.KERNELS for f in FC.PROD_FEATURES} | \
            {("cons", k, f) for k in FC.KERNELS for f in FC.CONS_FEATURES}
    # features that name a property of ONE kernel's tiling have no meaning on the others
    na = {("prod", k, f) for k in FC.TILE_KERNELS for f in ("half_tile_n", "two_tiles_per_wg")} | \
         {("cons", k, f) for k in FC.TILE_KERNELS for f in ("slots_gt8", "slots_le8")} | {("cons", "WIDE", "slots_gt24")}
    # the pre-set / NULL flag word: once per kernel group (required_cells)
    na |= {("prod", k, f) for k in FC.KERNELS for f in ("flag_set", "flag_null")}
    return cells - na


def test_role_kernel_feature_matrix_is_covered():
    required = FC.required_cells()
    have = set().union(*[FC.provides(c) for c in FC.CASES])
    away = _away(FC.REFUSED + FC.REROUTED)
    assert not (have & away), sorted(have & away)
    assert not (required - have), sorted(required - have)
    named = {a for a in away if a[2] not in FC.NOT_A_FEATURE}
    # a passing case or a confirmed refusal for every cell, and nothing refused that is also required
    assert _matrix() == (required & _matrix()) | named, sorted(_matrix() ^ ((required & _matrix()) | named))
    assert len(away) == len(FC.REFUSED) + len(FC.REROUTED)                     # no entry twice
    # what the issue names beside the matrix
    assert {c["feature"] for c in FC.REFUSED + FC.REROUTED} >= {"slot128_n_not_128", "slots_odd", "res_f32", "b_lo",
                                                                "ln_c_unaligned"}
    flags = [c["flag"] for c in FC.CASES if c["role"] == "prod" and not c["plant"]]
    assert "set" in flags and "null" in flags and flags.count("clear") >= 7
    assert {c["plant"][0] for c in FC.CASES if c["role"] == "prod" and c["plant"]} == {"hi_inf", "r_1e20", "hi_1e20"}
    assert all(c["flag"] == "clear" for c in FC.CASES if c["role"] == "prod" and c["plant"])


def test_fold_reaches_these_kernels_only():
    """(kernel, role) pairs no descriptor reaches: the fold never runs on the few-column, the streaming or the 256 x 256
    tile kernel (gemm_route: `plain` excludes the fold, fold_small switches `stream` and `big` off, every other fold is
    gemm_nt_wide or refused) -- no shape of the driver's sweep (5 x 6 x 4 shapes, six overrides, 256 and 8 CUs, both slot
    forms) reaches one, and every pair the table has cases for is reached."""
    swept = routed()[1]
    assert {k for _, k in swept} <= set(FC.KERNELS), sorted(swept)
    assert {(c["role"], c["kernel"]) for c in FC.CASES} == {(r, k) for r in ("prod", "cons") for k in FC.KERNELS}
    assert {("prod", "WIDE"), ("cons", "WIDE")} <= swept and len(swept) >= 8


@pytest.mark.parametrize("gone", FC.CASES + FC.REFUSED + FC.REROUTED,
                         ids=[c["id"] for c in FC.CASES + FC.REFUSED + FC.REROUTED])
def test_no_entry_can_be_removed(gone):
    """Every case is the only provider of at least one required cell, every REFUSED / REROUTED entry the only one that
    accounts for its cell: the coverage above fails without it."""
    have = set().union(*[FC.provides(c) for c in FC.CASES if c is not gone])
    away = _away([c for c in FC.REFUSED + FC.REROUTED if c is not gone])
    named = {a for a in away if a[2] not in FC.NOT_A_FEATURE}
    required = FC.required_cells()
    issue_names = {"slot128_n_not_128", "slots_odd"} <= {a[2] for a in away}
    ok = not (required - have) and _matrix() == (required & _matrix()) | named and issue_names
    assert not ok, f"{gone['id']} could be deleted without the coverage noticing"


# ----------------------------------------------------------------------------------------------------
# the references
# ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _arrays(cid, dt):
    return FC.make_arrays(FC.BY_ID[cid], dt)


@pytest.mark.parametrize("case", FC.CASES, ids=[c["id"] for c in FC.CASES])
def test_case_premises(case):
    """exact_ok for both types; the producer's sums inside SUM_BOUND in three fp32 orders (bit-equal in the int family); the
    bounded consumer's fp32 restatement, in both evaluation orders, inside HALF of CONS_BOUND (equal to the reference in the
    exact family)."""
    c = case
    for dt in FC.DTYPES:
        a = _arrays(c["id"], dt)
        with np.errstate(over="ignore"):
            assert FC.exact_ok(c, a, dt), (c["id"], dt)
        if c["role"] == "prod":
            if c["plant"]:
                continue
            x, sums = FC.ref_producer(c, a)
            hi, lo, x32, _ = FC.expected_producer(c, a, dt)
            assert np.array_equal(x32.astype(np.float64), x)
            if c["family"] == "int":
                assert not lo.any() and not np.signbit(lo).any() and np.array_equal(hi, x32)
                assert (_view_lo(c, a) != 0).all()
            xs = x.reshape(c["M"], c["N"] // c["slot_w"], c["slot_w"])[:64]
            bound = FC.sum_bound(c, a)[:64]
            for got in FC.f32_sums_three_orders(xs):
                err = np.abs(got.astype(np.float64) - sums[:64])
                assert (err <= bound).all(), (c["id"], dt, float((err / bound).max()))
                if c["family"] == "int":
                    assert not err.any()
        else:
            y, pre, _ = FC.ref_consumer(c, a)
            assert np.isfinite(y).all() and not y[:, c["N"]:].any()
            tile, wide = FC.f32_consumer_two_orders(c, a)
            if c["family"] == "bounded":
                half = 0.5 * (FC.cons_bound(c, a, dt) - FC.ULP[dt] * np.abs(y) - FC.TINY[dt])[:, :c["N"]]
                for got in (tile, wide):
                    err = np.abs(got.astype(np.float64) - pre)
                    assert (err <= half).all(), (c["id"], float((err / half).max()))
            else:
                assert np.array_equal(tile.astype(np.float64), pre) and np.array_equal(wide.astype(np.float64), pre)
            if dt == "f16":
                assert np.abs(y).max() < 60000
            break   # (the consumer's inputs do not depend on the type)


def _view_lo(c, a):
    if c["res"] == "f32":
        return np.ones(1)
    return a["R_lo"][:c["M"] * c["ld16"]].reshape(c["M"], c["ld16"])[:, :c["N"]]


def test_gelu_allowance_is_four_times_the_measured_deviation():
    """G: the polynomial of csrc/pio_gemm_common.h restated in numpy float32 against float64 erf-GELU over every gelu case's
    pre-activations; the constant in gemm_fold_cases.py records the figure."""
    worst, at = 0.0, None
    for c in FC.CASES:
        if c["family"] != "gelu":
            continue
        y, pre, _ = FC.ref_consumer(c, _arrays(c["id"], "f16"))
        vals = np.unique(pre)
        assert vals.min() >= -2.0 and vals.max() <= 8.0 and np.array_equal(vals, np.rint(vals * 4) / 4)
        err = np.abs(FC.f32_gelu(vals).astype(np.float64) - FC._erf_gelu(vals))
        if err.max() > worst:
            worst, at = float(err.max()), float(vals[np.argmax(err)])
    print(f"gelu_erf in float32: largest deviation {worst:.3e} at x = {at}")
    assert worst <= FC.GELU_MEASURED <= 1.25 * worst + 1e-9, (worst, at)
    assert FC.GELU_G == 4 * FC.GELU_MEASURED
    # the coefficients restated in gemm_fold_cases.py are those of the header
    text = open(os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc", "pio_gemm_common.h")).read()
    for k in ("3.152013050566893e-06f", "2.9346412588893145e-07f", "-0.0006359288236126304f", "0.007810706272721291f",
              "-0.05312380567193031f", "-0.45892834663391113f", "-1.15116286277771f", "-0.9999961256980896f"):
        assert k in text


@pytest.mark.parametrize("case", FC.CONSISTENT, ids=[c["id"] for c in FC.CONSISTENT])
def test_consumer_formula_is_layernorm(case):
    """ln_part from the rows of A (as a producer leaves it), ln_c[n] = sum_k B[n, k]: the reference of the consumer equals
    torch float64 layer_norm(x) @ W.T + b (transformer_primitives.py:281-292 with gamma, beta folded into W, b)."""
    M, N, K, w = case["M"], case["N"], case["K"], case["slot_w"]
    rng = np.random.default_rng(7)
    x, W, b = rng.integers(-5, 6, (M, K)).astype(np.float32), rng.integers(-3, 4, (N, K)).astype(np.float32), \
        rng.integers(-4, 5, N).astype(np.float32)
    c = FC._cons(case["id"], "T32", 0, M, N, K, ln_slots=K // w, act=case.get("act", 0))
    xs = x.astype(np.float64).reshape(M, K // w, w)
    part = np.stack([xs.sum(axis=2), (xs * xs).sum(axis=2)], axis=2).astype(np.float32)
    a = dict(A=FC._matrix(M, K, K, x), B=FC._matrix(N, K, K, W), A_lo=None, B_lo=None, bias=FC._vector(0, N, b),
             ln_c=FC._vector(0, N, W.sum(axis=1)), ln_part=FC._vector(0, M * (K // w) * 2, part.reshape(-1)))
    y = FC.ref_consumer(c, a)[0]
    xt = torch.from_numpy(x).double()
    want = torch.nn.functional.layer_norm(xt, (K,), eps=FC.EPS) @ torch.from_numpy(W).double().T + torch.from_numpy(b).double()
    if case.get("act"):
        want = torch.nn.functional.gelu(want)
    assert np.abs(y - want.numpy()).max() <= 1e-12 * max(1.0, float(want.abs().max()))
