"""CPU: which kernel every pio_layernorm_cast / pio_softmax_rows call goes to and which calls are refused
(perceiverio_pytorch_amd/csrc/pio_rows_route.h through the g++ driver of tests/rows_route_driver.py): every case of
tests/primitive_cases.py reaches the launcher branch it names, the thresholds sit where the kernels' register budgets
put them, and the error codes and their precedence."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import primitive_cases as PC  # noqa: E402
import rows_route_driver as RR  # noqa: E402

B, T = PC.LN_B, PC.LN_T
ROWS4 = (B * T + 3) // 4
SM_ROWS = PC.SM_B * PC.SM_H * PC.SM_TQ


def test_layernorm_cases_reach_their_branch():
    """Every LAYERNORM_CASES x LN_LAYOUTS call, both dtypes, with and without the affine: the case's branch, in every
    layout; even_rows exactly for the register float4 kernel on evenly spaced rows."""
    calls, want = [], {}
    for c in PC.LAYERNORM_CASES:
        for layout in PC.LN_LAYOUTS:
            sb, st, _ = PC.ln_strides(c, layout)
            for dt in PC.DTYPES:
                for has_ln in (True, False):
                    name = f"{c['id']}/{layout}/{dt}/{int(has_ln)}"
                    calls.append(RR.ln_case_call(name, c, layout, dt, has_ln))
                    want[name] = (c["branch"], ROWS4, int(c["branch"].startswith("reg_nv") and sb == T * st))
    assert RR.ask(calls) == want
    assert set(RR.ln_variants().values()) == set(PC.LN_BRANCHES)


def test_softmax_cases_reach_their_branch():
    calls, want = [], {}
    for c in PC.SOFTMAX_CASES:
        for form in PC.SM_FORMS:
            for dt in PC.DTYPES:
                name = f"{c['id']}/{form}/{dt}"
                calls.append(RR.sm_case_call(name, c, form, dt))
                label = c["branch"] + ("_" + ("plain" if form == "plain" else "masked") if c["branch"].startswith("reg") else "")
                want[name] = (label, SM_ROWS if c["branch"] == "gen_w4" else (SM_ROWS + 3) // 4)
    assert RR.ask(calls) == want


def test_layernorm_thresholds():
    def ln(name, C, c_pad, **kw):
        return RR.ln_call(name, "f16", B, T, C, c_pad, T * C, C, **kw)

    got = RR.ask([
        ln("c_pad_1024", 1024, 1024), ln("c_pad_1032", 1032, 1032),          # 4 -> 8 float4 per lane
        ln("c_pad_2048", 2048, 2048), ln("c_pad_2056", 2056, 2056),          # the widest register row
        ln("c2046_pad_2048", 2046, 2048), ln("c2050_pad_2056", 2050, 2056),  # ... of the float2 kernel
        ln("x_8_bytes", 1024, 1024, x=8), ln("x_4_bytes", 1024, 1024, x=4),
        ln("y_lo_4_bytes", 1024, 1024, y_lo=4), ln("y_2_bytes", 1024, 1024, y=2),
        ln("gamma_8_bytes", 1024, 1024, gamma=8), ln("gamma_8_bytes_no_ln", 1024, 1024, gamma=8, has_ln=False),
        ln("beta_4_bytes", 1024, 1024, beta=4),
        RR.ln_call("one_sample_any_stride_b", "f16", 1, T, 64, 64, 12345 * 4, 64),
        RR.ln_call("stride_b_odd", "f16", B, T, 64, 64, T * 64 + 1, 64),
        RR.ln_call("stride_t_2_mod_4", "bf16", B, T, 64, 64, T * 66, 66),
    ])
    assert got == {
        "c_pad_1024": ("reg_nv4", ROWS4, 1), "c_pad_1032": ("reg_nv8", ROWS4, 1),
        "c_pad_2048": ("reg_nv8", ROWS4, 1), "c_pad_2056": ("gen_vec", ROWS4, 0),
        "c2046_pad_2048": ("reg2", ROWS4, 0), "c2050_pad_2056": ("gen_scalar", ROWS4, 0),
        "x_8_bytes": ("reg2", ROWS4, 0), "x_4_bytes": ("gen_scalar", ROWS4, 0),
        "y_lo_4_bytes": ("reg2", ROWS4, 0), "y_2_bytes": ("gen_scalar", ROWS4, 0),
        "gamma_8_bytes": ("reg2", ROWS4, 0), "gamma_8_bytes_no_ln": ("reg_nv4", ROWS4, 1),
        "beta_4_bytes": ("gen_scalar", ROWS4, 0),
        "one_sample_any_stride_b": ("reg_nv4", (T + 3) // 4, 1),
        "stride_b_odd": ("gen_scalar", ROWS4, 0),
        "stride_t_2_mod_4": ("reg2", ROWS4, 0),
    }


def test_softmax_thresholds():
    def sm(name, Tk, ldp=None, **kw):
        return RR.sm_call(name, "f16", PC.SM_B, PC.SM_H, PC.SM_TQ, Tk, Tk, Tk if ldp is None else ldp, **kw)

    got = RR.ask([
        sm("ldp_512", 512), sm("ldp_516", 516), sm("ldp_2048", 2048), sm("ldp_2052", 2052), sm("ldp_4096", 4096),
        sm("ldp_4100", 4100),
        sm("tk_2048_generic", 2048, S=4), sm("tk_2049_generic", 2049, 2056),
        sm("tk_8_ldp_4100", 8, 4100),                                        # the pitch of P, not Tk, sizes the registers
        sm("p_4_bytes", 512, P=4), sm("p_lo_4_bytes", 512, full=True, P_lo=4), sm("bias_8_bytes", 512, full=True, bias=8),
        sm("kv_mask_2_bytes", 512, full=True, kv_mask=2), sm("full_mask_1_byte", 512, full=True, full_mask=1),
        sm("probs_8_bytes", 512, probs=8),
        RR.sm_call("lds_2_mod_4", "bf16", PC.SM_B, PC.SM_H, PC.SM_TQ, 512, 514, 512),
    ])
    r4 = (SM_ROWS + 3) // 4
    assert got == {
        "ldp_512": ("reg_nv2_plain", r4), "ldp_516": ("reg_nv8_plain", r4), "ldp_2048": ("reg_nv8_plain", r4),
        "ldp_2052": ("reg_nv16_plain", r4), "ldp_4096": ("reg_nv16_plain", r4), "ldp_4100": ("gen_w4", SM_ROWS),
        "tk_2048_generic": ("gen_w1", r4), "tk_2049_generic": ("gen_w4", SM_ROWS),
        "tk_8_ldp_4100": ("gen_w1", r4),
        "p_4_bytes": ("gen_w1", r4), "p_lo_4_bytes": ("gen_w1", r4), "bias_8_bytes": ("gen_w1", r4),
        "kv_mask_2_bytes": ("gen_w1", r4), "full_mask_1_byte": ("gen_w1", r4), "probs_8_bytes": ("gen_w1", r4),
        "lds_2_mod_4": ("gen_w1", r4),
    }


def test_refusals():
    """The error code of every refused call; where several apply: shape before alignment before the dtype."""
    def ln(name, dt="f16", Bv=B, C=64, c_pad=64):
        return RR.ln_call(name, dt, Bv, T, C, c_pad, T * C, C)

    def sm(name, dt="f16", Tk=64, lds=64, ldp=64, Tq=PC.SM_TQ):
        return RR.sm_call(name, dt, PC.SM_B, PC.SM_H, Tq, Tk, lds, ldp)

    def cat(name, dt="f16", C1=64, C2=258, c_pad=None, **kw):
        # x1, x2 as tests/test_primitives_gpu.py::test_layernorm_cast_cat_refuses builds them: column slices of arrays one wider
        cp = PC.pad8(C1 + C2) if c_pad is None else c_pad
        return RR.cat_call(name, dt, B, T, C1, 1, T, C2, C1 + C2, cp, T * (C1 + 1), C1 + 1, T * (C2 + 1), C2 + 1, **kw)

    calls = [
        ln("ln_no_samples", Bv=0), ln("ln_c_pad_below_c", c_pad=56), ln("ln_c_pad_not_8", C=60, c_pad=60),
        ln("ln_dtype", dt="bad"), ln("ln_dtype_wide", dt="bad", C=4096, c_pad=4096), ln("ln_shape_and_dtype", dt="bad", c_pad=60),
        sm("sm_no_keys", Tk=0), sm("sm_ldp_below_tk", ldp=60), sm("sm_lds_below_tk", lds=60), sm("sm_no_queries", Tq=0),
        sm("sm_dtype", dt="bad"), sm("sm_shape_and_dtype", dt="bad", ldp=60),
        RR.cat_call("cat_ok", "bf16", B, T, 64, 1, T, 258, 322, 328, T * 64, 64, T * 258, 258),
        RR.cat_call("cat_t_differs", "f16", B, T, 64, 1, T + 1, 258, 322, 328, T * 64, 64, T * 258, 258),
        RR.cat_call("cat_b2_neither_b_nor_1", "f16", B, T, 64, 2, T, 258, 322, 328, T * 64, 64, T * 258, 258),
        RR.cat_call("cat_ln_width", "f16", B, T, 64, 1, T, 258, 320, 328, T * 64, 64, T * 258, 258),
        RR.cat_call("cat_odd_stride", "f16", B, T, 64, 1, T, 258, 322, 328, T * 65, 65, T * 258, 258),
        RR.cat_call("cat_x1_4_bytes", "f16", B, T, 64, 1, T, 258, 322, 328, T * 64, 64, T * 258, 258, x1=4),
        RR.cat_call("cat_y_2_bytes", "f16", B, T, 64, 1, T, 258, 322, 328, T * 64, 64, T * 258, 258, y=2),
        RR.cat_call("cat_gamma_4_bytes", "f16", B, T, 64, 1, T, 258, 322, 328, T * 64, 64, T * 258, 258, gamma=4),
        RR.cat_call("cat_dtype", "bad", B, T, 64, 1, T, 258, 322, 328, T * 64, 64, T * 258, 258),
        RR.cat_call("cat_align_and_dtype", "bad", B, T, 64, 1, T, 258, 322, 328, T * 64, 64, T * 258, 258, x2=4),
        RR.cat_call("cat_shape_and_align", "f16", B, T, 64, 1, T, 258, 322, 2056, T * 64, 64, T * 258, 258, x2=4),
    ]
    calls += [cat("refused_" + c["id"], C1=c["C1"], C2=c["C2"], c_pad=c["c_pad"]) for c in PC.LNCAT_REFUSED]
    want = {
        "ln_no_samples": "PIO_E_SHAPE", "ln_c_pad_below_c": "PIO_E_SHAPE", "ln_c_pad_not_8": "PIO_E_SHAPE",
        "ln_dtype": "PIO_E_ARG", "ln_dtype_wide": "PIO_E_ARG", "ln_shape_and_dtype": "PIO_E_SHAPE",
        "sm_no_keys": "PIO_E_SHAPE", "sm_ldp_below_tk": "PIO_E_SHAPE", "sm_lds_below_tk": "PIO_E_SHAPE",
        "sm_no_queries": "PIO_E_SHAPE", "sm_dtype": "PIO_E_ARG", "sm_shape_and_dtype": "PIO_E_SHAPE",
        "cat_ok": "cat2", "cat_t_differs": "PIO_E_SHAPE", "cat_b2_neither_b_nor_1": "PIO_E_SHAPE", "cat_ln_width": "PIO_E_SHAPE",
        "cat_odd_stride": "PIO_E_ALIGN", "cat_x1_4_bytes": "PIO_E_ALIGN", "cat_y_2_bytes": "PIO_E_ALIGN",
        "cat_gamma_4_bytes": "PIO_E_ALIGN", "cat_dtype": "PIO_E_ARG", "cat_align_and_dtype": "PIO_E_ALIGN",
        "cat_shape_and_align": "PIO_E_SHAPE",
    }
    want.update({"refused_" + c["id"]: "PIO_E_SHAPE" for c in PC.LNCAT_REFUSED})
    assert RR.ask(calls) == want


def test_lncat_cases_take_the_float2_kernel_when_materialised():
    """tests/test_primitives_gpu.py::test_layernorm_cast_cat compares the cat kernel bit for bit with pio_layernorm_cast
    of the materialised concatenation placed two floats past a 16-byte boundary: that call is the float2 register kernel
    for every LNCAT_CASES entry, also where C1 + C2 is a multiple of four."""
    calls = [RR.ln_call(c["id"], "f16", B, T, c["C1"] + c["C2"], PC.pad8(c["C1"] + c["C2"]), T * (c["C1"] + c["C2"]),
                        c["C1"] + c["C2"], x=8) for c in PC.LNCAT_CASES]
    assert RR.ask(calls) == {c["id"]: ("reg2", ROWS4, 0) for c in PC.LNCAT_CASES}
    assert any((c["C1"] + c["C2"]) % 4 == 0 for c in PC.LNCAT_CASES)


def test_header_is_host_only():
    """No HIP include, no environment read, no state: the header compiles with a plain C++ compiler (above) and names none."""
    src = open(RR.HEADER).read()
    assert "hip_runtime" not in src and "getenv" not in src and "static " not in src
