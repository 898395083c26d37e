"""CPU: which kernel every pio_gemm_nt launch goes to (perceiverio_pytorch_amd/csrc/pio_gemm_route.h, compiled with g++
into a small driver; the descriptors carry fake, aligned pointers that are never dereferenced)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
#include <stdio.h>
#include "pio_gemm_route.h"
using namespace pio;

static const void *ptr(int i) { return (const void *)(uintptr_t)(0x10000000ull * (uint64_t)i); }   // 256-byte aligned

// one flat [M,K] x [N,K] linear, bias, 16-bit out
static pio_gemm_t linear(int M, int N, int K) {
    pio_gemm_t g = {};
    g.A = ptr(1); g.B = ptr(2); g.C = (void *)ptr(3);
    g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldb = K; g.ldc = N;
    g.batch = 1; g.nh = 1;
    g.bias = (const float *)ptr(4); g.bias_mode = 1; g.alpha = 1.0f;
    g.dtype = PIO_DT_F16;
    return g;
}
static pio_gemm_t residual(pio_gemm_t g) { g.R = (const float *)ptr(5); g.ldr = g.N; return g; }
static pio_gemm_t pair_out(pio_gemm_t g) { g.C_lo = (void *)ptr(6); return g; }
static pio_gemm_t split_act(pio_gemm_t g) { g.A_lo = ptr(7); return g; }
// LayerNorm-fold producer: residual and result as 16-bit pairs, row statistics in slots of w columns, no fp32 C
static pio_gemm_t producer(int M, int N, int K, int w) {
    pio_gemm_t g = linear(M, N, K);
    g.C = nullptr; g.out_f32 = 1;
    g.X16 = (void *)ptr(8); g.X16_lo = (void *)ptr(9); g.ld16 = N;
    g.R16_hi = ptr(10); g.R16_lo = ptr(11);
    g.row_part = (float *)ptr(12); g.row_slot_w = w;
    return g;
}
// LayerNorm-fold consumer with slots per row of ln_part
static pio_gemm_t consumer(int M, int N, int K, int slots) {
    pio_gemm_t g = linear(M, N, K);
    g.ln_part = (const float *)ptr(13); g.ln_c = (const float *)ptr(14); g.ln_eps = 1e-5f; g.ln_slots = slots;
    return g;
}

static const char *name(GemmKernel k) {
    switch (k) {
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
    default: return "NONE";
    }
}

static void show(const char *id, const pio_gemm_t &g, int forced = 0) {
    GemmParams p;
    int err = gemm_params(g, &p);
    GemmRoute r = {};
    if (!err) {
        r = gemm_route(g, p, forced, 256);
        err = r.err;
    }
    if (err == PIO_E_SHAPE) printf("%s PIO_E_SHAPE\n", id);
    else if (err == PIO_E_ALIGN) printf("%s PIO_E_ALIGN\n", id);
    else if (err == PIO_E_ARG) printf("%s PIO_E_ARG\n", id);
    else if (err) printf("%s error %d\n", id, err);
    else printf("%s %s %s %u %u\n", id, name(r.kernel), r.label, r.grid_x, r.grid_y);
}

int main() {
    pio_gemm_t g = split_act(linear(182528, 2, 328));
    g.out_f32 = 1; g.ldc = 2;
    show("flow_final_linear", g);
    g = split_act(linear(100352, 3, 512));
    g.out_f32 = 1; g.ldc = 4;
    show("three_columns", g);
    g = pair_out(split_act(linear(182528, 384, 384)));
    g.act = 1;
    show("flow_decoder_384", g);
    show("proj_16384", linear(16384, 1024, 1024));
    g = residual(linear(16384, 1024, 1024));
    g.out_f32 = 1;
    show("proj_16384_f32_res", g);
    show("proj_16384_pair_res", pair_out(residual(linear(16384, 1024, 1024))));
    show("language_8192", linear(8192, 1280, 1280));
    show("fold_consumer", consumer(16384, 3072, 1024, 1024 / 128));
    show("fold_producer", producer(16384, 1024, 1024, 128));
    show("fold_producer_small", producer(2048, 512, 512, 64));
    g = producer(2048, 512, 512, 64);
    g.B_lo = ptr(15);
    show("fold_producer_small_npass2", g);
    show("fold_consumer_small", consumer(2048, 512, 512, 512 / 64));
    g = linear(512, 1024, 1024);
    g.B_lo = ptr(15); g.b_lo_n0 = 256;
    show("partial_b_lo_refused", g);
    show("imagenet_b1", linear(512, 1024, 1024));
    show("imagenet_b2_qkv", linear(1024, 3072, 1024));
    show("imagenet_b8", linear(4096, 1024, 1024));
    show("flow_qkv", linear(2048, 1536, 512));
    show("flow_stack_proj", linear(2048, 512, 512));
    g = linear(512, 512, 128);
    g.bias_mode = 0; g.batch = 256; g.nh = 8;
    g.sAh = 512 * 128; g.sAb = 8 * g.sAh; g.sBh = 512 * 128; g.sBb = 8 * g.sBh; g.sCh = 512 * 512; g.sCb = 8 * g.sCh;
    show("attention_product", g);
    show("auto_t256", linear(1024, 8192, 1024));
    show("override_1", linear(16384, 1024, 1024), 1);
    show("override_2", linear(16384, 1024, 1024), 2);
    show("override_128", linear(16384, 1024, 1024), 128);
    show("override_256", linear(16384, 1024, 1024), 256);
    show("override_64_imagenet_b2_qkv", linear(1024, 3072, 1024), 64);
    show("override_64_proj_16384", linear(16384, 1024, 1024), 64);
    show("override_2_res_16bit", residual(linear(16384, 1024, 1024)), 2);
    g = linear(16384, 1024, 1024);
    g.out_f32 = 1; g.act = 1;
    show("override_2_f32_gelu", g, 2);
    show("override_2_k1000", linear(512, 1024, 1000), 2);
    show("override_128_fold_consumer", consumer(16384, 3072, 1024, 1024 / 128), 128);
    show("override_256_fold_producer", producer(16384, 1024, 1024, 128), 256);
    show("k_not_multiple_of_8", linear(512, 1024, 1020));
    g = linear(512, 1024, 1024);
    g.A = (const char *)g.A + 8;
    show("a_misaligned", g);
    g = linear(512, 1024, 1024);
    g.bias = nullptr;
    show("bias_missing", g);
    return 0;
}
'''

# id -> (kernel, PIO_GEMM_LOG label) or error code.  n_cu = 256.
EXPECTED = {
    "flow_final_linear": ("SKINNY2", "skinny"),             # 182 528 x 2 x 328, split activations, fp32 out
    "three_columns": ("SKINNY4", "skinny"),
    "flow_decoder_384": ("WIDE", "wide"),                   # N = 384: the 1.34 fill rule
    "proj_16384": ("WIDE", "wide"),
    "proj_16384_f32_res": ("STREAM", "stream"),             # a residual is not sent to the wide kernel at >= 224 tiles
    "proj_16384_pair_res": ("WIDE", "wide"),                # ... unless the result leaves as a hi + lo pair
    "language_8192": ("WIDE", "wide"),                      # 160 tiles of 256 x 256
    "fold_consumer": ("WIDE", "wide"),
    "fold_producer": ("WIDE", "wide"),
    "fold_producer_small": ("T64", "t64"),                  # 64-column slots: the small-tile fold (flow stack)
    "fold_producer_small_npass2": "PIO_E_SHAPE",
    "fold_consumer_small": ("T64", "t64"),
    "partial_b_lo_refused": "PIO_E_SHAPE",                  # a partial B_lo is a gemm_nt_wide feature
    "imagenet_b1": ("T32_KG2", "t32"),
    "imagenet_b2_qkv": ("T128_KG2", "t128"),
    "imagenet_b8": ("T64", "t64"),
    "flow_qkv": ("T64", "t64"),
    "flow_stack_proj": ("T64", "t64"),                      # K = 512: no K teams
    "attention_product": ("T128", "t128"),
    "auto_t256": ("T256", "t256"),
    "override_1": ("STREAM", "stream"),
    "override_2": ("WIDE", "wide"),
    "override_128": ("T128", "t128"),
    "override_256": ("T256", "t256"),
    "override_64_imagenet_b2_qkv": ("T64", "t64"),          # no K teams, no 32-row tile under an override
    "override_64_proj_16384": ("WIDE", "wide"),             # 64 does not keep a GEMM off the persistent kernels
    "override_2_res_16bit": ("STREAM", "stream"),           # the wide kernel refuses: falls through ...
    "override_2_f32_gelu": ("T256", "t256"),
    "override_2_k1000": ("T128", "t128"),
    "override_128_fold_consumer": ("WIDE", "wide"),         # 128 / 256 do not apply to the fold GEMMs
    "override_256_fold_producer": ("WIDE", "wide"),
    "k_not_multiple_of_8": "PIO_E_SHAPE",
    "a_misaligned": "PIO_E_ALIGN",
    "bias_missing": "PIO_E_ARG",
}

# grids of the persistent and few-column kernels (one workgroup per CU, 8 rows a workgroup) and of the tile kernels
GRIDS = {
    "flow_final_linear": (2048, 1),
    "proj_16384": (256, 1),
    "proj_16384_f32_res": (256, 1),
    "language_8192": (160, 1),
    "imagenet_b1": (256, 1),
    "imagenet_b2_qkv": (192, 1),
    "imagenet_b8": (1024, 1),
    "attention_product": (16, 256),
    "auto_t256": (128, 1),
}


def test_gemm_routing_table():
    inc = os.path.join(ROOT, "include")
    csrc = os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "route.cpp")
        open(src, "w").write(DRIVER)
        exe = os.path.join(d, "route")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", inc, "-I", csrc, src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    got, grids = {}, {}
    for line in filter(None, out):
        f = line.split()
        if len(f) == 2:
            got[f[0]] = f[1]
        else:
            got[f[0]] = (f[1], f[2])
            grids[f[0]] = (int(f[3]), int(f[4]))
    assert got == EXPECTED
    assert {k: grids[k] for k in GRIDS} == GRIDS
