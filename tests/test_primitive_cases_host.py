"""CPU: the float64 references of tests/primitive_cases.py against torch's float64 ops, and the coverage of the case
tables: every launcher branch of csrc/pio_elementwise.hip that tests/test_primitives_gpu.py is meant to reach has a
case for each operand dtype (the dtype is a loop of the GPU test over primitive_cases.DTYPES)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import primitive_cases as PC  # noqa: E402
import rows_route_driver as RR  # noqa: E402

TOL = 1e-12


def test_ref_softmax_rows_matches_torch():
    for name in ("tk13", "tk512"):
        case = next(c for c in PC.SOFTMAX_CASES if c["id"] == name)
        for form in PC.SM_FORMS:
            d = PC.sm_inputs(case, form)
            ref = PC.ref_softmax_rows(d["S"], d["scale"], d["kv_mask"], d["q_mask"], d["full_mask"], d["bias"])
            s = torch.from_numpy(d["S"]).double()
            if d["bias"] is not None:
                s = s + torch.from_numpy(d["bias"]).double()
            s = s * d["scale"]
            ok = torch.from_numpy(np.broadcast_to(PC.softmax_valid(d["S"].shape, d["kv_mask"], d["q_mask"], d["full_mask"]),
                                                  d["S"].shape).copy())
            want = torch.softmax(s.masked_fill(~ok, float("-inf")), dim=-1)
            want = torch.where(ok.any(-1, keepdim=True), want, torch.zeros_like(want))      # rows without a key: zeros
            assert np.abs(ref - want.numpy()).max() <= TOL
            assert (ref[~ok.numpy()] == 0).all()
            if form == "full":
                assert (ref[1] == 0).all() and (ref[0, :, PC.SM_ROW_QMASKED] == 0).all()
                assert (ref[0, :, PC.SM_ROW_FULL_EMPTY] == 0).all()
                one = ref[0, :, PC.SM_ROW_ONE_KEY]
                assert (one[:, -1] == 1).all() and (one[:, :-1] == 0).all()
            assert np.abs(d["S"][0, :, PC.SM_ROW_LARGE] * d["scale"]).max() >= 1e4 * (1 - 1e-6)


def test_softmax_mask_bytes_count_when_non_zero():
    case = next(c for c in PC.SOFTMAX_CASES if c["id"] == "tk13")
    d = PC.sm_inputs(case, "full")
    base = PC.ref_softmax_rows(d["S"], d["scale"], d["kv_mask"], d["q_mask"], d["full_mask"], d["bias"])
    for v in PC.MASK_TRUE_BYTES:
        for which in ("kv_mask", "q_mask", "full_mask"):
            e = dict(d)
            e[which] = (d[which] * v).astype(np.uint8)
            got = PC.ref_softmax_rows(e["S"], e["scale"], e["kv_mask"], e["q_mask"], e["full_mask"], e["bias"])
            assert np.array_equal(got, base)


def test_ref_layernorm_cast_matches_torch():
    for name in ("c8", "c261", "c600_pad640"):
        case = next(c for c in PC.LAYERNORM_CASES if c["id"] == name)
        x, g, b = PC.ln_inputs(case)
        ref = PC.ref_layernorm_cast(x, g, b, PC.LN_EPS, case["c_pad"])
        want = F.layer_norm(torch.from_numpy(x).double(), (case["C"],), torch.from_numpy(g).double(),
                            torch.from_numpy(b).double(), PC.LN_EPS).numpy()
        assert np.abs(ref[..., :case["C"]] - want).max() <= TOL * max(1.0, np.abs(want).max())
        assert (ref[..., case["C"]:] == 0).all() and ref.shape[-1] == case["c_pad"]
        plain = PC.ref_layernorm_cast(x, None, None, 0.0, case["c_pad"])
        assert np.array_equal(plain[..., :case["C"]], x.astype(np.float64))
        # the planted rows are what they claim to be: exact means, in fp32 and in any order
        assert np.float32(x[0, PC.LN_ROW_MEAN1E3].astype(np.float64).mean()) == 1000.0
        assert x[1, 0].astype(np.float64).mean() == 0.5
        assert np.abs(ref[0, PC.LN_ROW_CONST, :case["C"]] - b).max() <= TOL
        assert np.abs(ref[0, PC.LN_ROW_ZERO, :case["C"]] - b).max() <= TOL


def test_ref_pack_linear_matches_indexing():
    for case in PC.PACK_CASES:
        out, inn, rh, ch = case
        rows_p, cols_used, k_pad, _ldw, rows_total = PC.pack_geometry(case)
        w, bias = PC.pack_inputs(case)
        img, bimg, written = PC.ref_pack_linear(w, bias, rh, ch, k_pad, PC.PACK_ROW0, rows_total)
        dr, dc = out // rh, inn // ch
        drp, dcp = PC.pad8(dr), PC.pad8(dc)
        t = torch.zeros(rh, drp, ch, dcp, dtype=torch.float64)
        t[:, :dr, :, :dc] = torch.from_numpy(w).double().reshape(rh, dr, ch, dc)
        want = torch.zeros(rows_p, k_pad, dtype=torch.float64)
        want[:, :cols_used] = t.reshape(rows_p, cols_used)
        part = img[PC.PACK_ROW0:PC.PACK_ROW0 + rows_p]
        assert np.array_equal(part, want.numpy())
        tb = torch.zeros(rh, drp, dtype=torch.float64)
        tb[:, :dr] = torch.from_numpy(bias).double().reshape(rh, dr)
        assert np.array_equal(bimg[PC.PACK_ROW0:PC.PACK_ROW0 + rows_p], tb.reshape(-1).numpy())
        assert written.sum() == rows_p and np.isnan(img[~written]).all() and np.isnan(bimg[~written]).all()
        _, b0, _ = PC.ref_pack_linear(w, None, rh, ch, k_pad, PC.PACK_ROW0, rows_total)
        assert (b0[written] == 0).all()


def test_round_to_matches_torch():
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.standard_normal(4096).astype(np.float32) * np.float32(10.0) ** rng.integers(-9, 4, 4096),
                        np.array([0.0, 3e-8, 6e-8, 65504.0, 1.00390625, 1.01171875], dtype=np.float32)]).astype(np.float32)
    assert np.array_equal(PC.round_to("f16", a), torch.from_numpy(a).to(torch.float16).float().numpy())
    assert np.array_equal(PC.round_to("bf16", a), torch.from_numpy(a).to(torch.bfloat16).float().numpy())


@pytest.mark.parametrize("pads", PC.POOL_PADS)
def test_ref_bn_relu_maxpool_matches_torch(pads):
    pt, pl = pads
    for C, (H, W) in ((1, (1, 1)), (3, (2, 3)), (5, (7, 10)), (4, (5, 9))):
        x, scale, shift = PC.pool_inputs(C, H, W)
        ref, mag = PC.ref_bn_relu_maxpool_tokens(x, scale, shift, pt, pl)
        OH, OW = (H + 1) // 2, (W + 1) // 2
        r = torch.relu(torch.from_numpy(x).double() * torch.from_numpy(scale).double()[None, :, None, None]
                       + torch.from_numpy(shift).double()[None, :, None, None])
        pb, pr = 2 * (OH - 1) + 3 - H - pt, 2 * (OW - 1) + 3 - W - pl
        want = F.max_pool2d(F.pad(r, (pl, max(pr, 0), pt, max(pb, 0))), 3, 2)[:, :, :OH, :OW]
        want = want.permute(0, 2, 3, 1).reshape(PC.POOL_B, OH * OW, C).numpy()
        assert np.abs(ref - want).max() <= TOL
        assert (mag >= np.abs(ref) - TOL).all()
        if H >= 3 and W >= 3 and pt == 0 and pl == 0:
            assert (ref[1, 0] == 0).all()           # the planted all-negative window


def test_every_launcher_branch_has_a_case():
    seen, variant = set(), RR.softmax_variants()                    # (the launcher's routing header, through a g++ driver)
    for c in PC.SOFTMAX_CASES:
        for form in PC.SM_FORMS:
            v = variant[c["id"], form]
            assert v.startswith(c["branch"]), (c["id"], v)          # the case reaches the branch it names
            seen.add(v)
    want = {f"reg_nv{n}_{f}" for n in (2, 8, 16) for f in ("plain", "masked")} | {"gen_w1", "gen_w4"}
    assert seen == want
    for b in PC.SM_BRANCHES:                                        # ... and the generic kernels run both forms
        assert any(c["branch"] == b for c in PC.SOFTMAX_CASES)
    assert any(c["lds"] > c["Tk"] and c["branch"].startswith("reg") for c in PC.SOFTMAX_CASES)
    assert any(c["ldp"] > PC.pad8(c["Tk"]) for c in PC.SOFTMAX_CASES)
    for name in PC.SM_MASK_BYTE_CASES:
        assert any(c["id"] == name for c in PC.SOFTMAX_CASES)

    seen, variant = set(), RR.ln_variants()
    for c in PC.LAYERNORM_CASES:
        for layout in PC.LN_LAYOUTS:
            v = variant[c["id"], layout]
            assert v == c["branch"], (c["id"], layout, v)           # no layout moves a case to another kernel
            seen.add(v)
    assert seen == set(PC.LN_BRANCHES)
    assert len(PC.DTYPES) == 2
    assert any((c["C1"] + c["C2"]) % 4 for c in PC.LNCAT_CASES) and any(c["table"] for c in PC.LNCAT_CASES)
    assert any(not c["table"] for c in PC.LNCAT_CASES) and any(c["x1_gap"] for c in PC.LNCAT_CASES)
    assert any(c["c_pad"] > 2048 for c in PC.LNCAT_REFUSED)
