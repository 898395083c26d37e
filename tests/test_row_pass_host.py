"""CPU: the references, fault coverage and refusal tables of tests/row_pass_cases.py (pio_rowstats_cast, pio_transpose16).

1. the references against an independent formulation (plain loops / torch float64);
2. every fault these kernels can have, modelled as a mutation of the numpy model, is rejected by at least one case of the
   table the GPU test runs (printed: which);
3. the refusal tables against a restatement of the launchers' checks (tests/test_row_pass_gpu.py runs the same tables
   against the launchers themselves, on real buffers)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import row_pass_cases as RC  # noqa: E402


# ---- 1. references ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", RC.DTYPES)
def test_rowstats_reference_against_loops_and_torch(dt):
    tdt = torch.float16 if dt == "f16" else torch.bfloat16
    for C_, w, rows in ((256, 64, 3), (512, 128, 5)):
        x = RC.rs_input(C_, w, rows, "gauss", dt)
        y, lo, part, bound = RC.rs_reference(x, w, dt)
        xt = torch.from_numpy(x)
        yt = xt.to(tdt)
        assert np.array_equal(yt.float().numpy(), y) and np.array_equal((xt - yt.float()).to(tdt).float().numpy(), lo)
        for r in range(rows):
            for s in range(C_ // w):
                sm = sq = 0.0
                for c in range(s * w, (s + 1) * w):
                    sm += float(x[r, c])
                    sq += float(x[r, c]) * float(x[r, c])
                assert abs(part[r, s, 0] - sm) <= 1e-12 and abs(part[r, s, 1] - sq) <= 1e-12
        # the bound holds for fp32 sums in three orders (forward, reverse, pairwise) and is not slack by orders
        xs = x.reshape(rows, C_ // w, w)
        fwd = np.zeros((rows, C_ // w, 2), np.float32)
        rev = np.zeros_like(fwd)
        for i in range(w):
            fwd[..., 0] += xs[..., i]
            fwd[..., 1] += xs[..., i] * xs[..., i]
            rev[..., 0] += xs[..., w - 1 - i]
            rev[..., 1] += xs[..., w - 1 - i] * xs[..., w - 1 - i]
        s_, q_ = xs.copy(), xs * xs
        while s_.shape[-1] > 1:
            s_, q_ = s_[..., 0::2] + s_[..., 1::2], q_[..., 0::2] + q_[..., 1::2]
        pair = np.stack([s_[..., 0], q_[..., 0]], axis=-1)
        for got in (fwd, rev, pair):
            assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - part) <= bound).all()
        assert (bound[..., 1] <= 1e-5 * part[..., 1]).all()


@pytest.mark.parametrize("dt", RC.DTYPES)
def test_rowstats_probes_are_what_they_claim(dt):
    for C_, w, rows in RC.RS_SHAPES:
        x = RC.rs_input(C_, w, rows, "int", dt)
        y, lo, part, _ = RC.rs_reference(x, w, dt)
        assert np.array_equal(y, x) and not lo.any() and not np.signbit(lo).any()
        assert np.array_equal(x * 4, np.rint(x * 4)) and np.abs(x * 4).max() <= 256
        xs = np.abs(x.astype(np.float64)).reshape(rows, C_ // w, w)
        assert (16 * (xs * xs).sum(axis=2)).max() < 2.0 ** 24 and (4 * xs.sum(axis=2)).max() < 2.0 ** 24   # exact in any order
        assert np.array_equal(part.astype(np.float32).astype(np.float64), part)
        n = rows * (C_ // w)
        assert len(set(part[..., 0].reshape(-1).tolist())) == n and len(set(part[..., 1].reshape(-1).tolist())) == n
    for C_, w, rows in RC.RS_SHAPES_FEW:
        x, h, l = RC.rs_input(C_, w, rows, "residual", dt)
        y, lo, _, _ = RC.rs_reference(x, w, dt)
        assert np.array_equal(y, h) and np.array_equal(lo, l) and (l != 0).all()
        assert np.array_equal(RC.round_to(dt, h), h) and np.array_equal(RC.round_to(dt, l), l)
        x = RC.rs_input(C_, w, rows, "big", dt)
        y, lo, part, _ = RC.rs_reference(x, w, dt)
        r, c = RC.RS_BIG_AT
        assert part[r, c // w, 1] == np.inf and np.isfinite(part[r, c // w, 0])
        assert np.isfinite(np.delete(part[..., 1].reshape(-1), (rows - 1) * (C_ // w) + c // w)).all()
        if dt == "f16":
            assert y[r, c] == np.inf and lo[r, c] == -np.inf
        else:
            assert y[r, c] == 2.0 ** 70 and lo[r, c] == 0
        assert np.isfinite(np.delete(y.reshape(-1), (rows - 1) * C_ + c)).all()


def test_transpose_reference_against_loops():
    for case in RC.TR_CASES[:4] + [RC.TR_CASES[6]]:
        B, T, C_, ldx, tkv = RC.tr_shape(case)
        x, vt = RC.tr_input(case), RC.tr_reference(case)
        assert vt.shape == (B, C_, tkv)
        for b in range(B):
            for c in range(C_):
                for t in range(tkv):
                    assert vt[b, c, t] == (x[(b * T + t) * ldx + c] if t < T else 0)
        assert np.array_equal(RC.tr_model(case, x), vt)
    vals = RC.hash16(*np.ogrid[:3, :129, :328])
    spec = vals.view(np.float16)
    assert np.isnan(spec).any() and np.isinf(spec).any() and (vals == 0x8000).any(), "the hash should reach NaN, inf and -0"


def test_transpose_table_reaches_every_value():
    for axis, values in enumerate((RC.TR_T, RC.TR_C, RC.TR_LDX, RC.TR_TKV, RC.TR_B)):
        assert {c[axis] for c in RC.TR_CASES} == set(values), axis
    for t_on in (True, False):
        for c_on in (True, False):
            assert any((c[0] % 64 == 0) == t_on and (c[1] % 64 == 0) == c_on for c in RC.TR_CASES)
    assert any(RC.tr_shape(c)[4] - RC.tr_shape(c)[1] >= 128 for c in RC.TR_CASES), "whole tiles of zeros"
    assert any(c[1] == 328 and c[2] == "padc" and c[4] == 3 for c in RC.TR_CASES), "the encoder's 328 of 384, batched"


# ---- 2. faults -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", RC.RS_FAULTS)
def test_rowstats_fault_is_rejected(fault):
    caught = []
    for C_, w, rows in RC.RS_SHAPES:
        for with_lo in (True, False):
            x = RC.rs_input(C_, w, rows, "int", "f16")
            assert not RC.rs_rejects(x, w, "f16", with_lo, RC.rs_model(x, w, "f16", with_lo)), "the sound model must pass"
            if RC.rs_rejects(x, w, "f16", with_lo, RC.rs_model(x, w, "f16", with_lo, fault)):
                caught.append(f"C{C_}_w{w}_r{rows}_lo{int(with_lo)}")
    if fault == "lo_copy_of_y":      # y_lo == 0 == y only where x is 0: the int probe sees it; the residual probe by design
        x, h, l = RC.rs_input(512, 128, 3, "residual", "f16")
        assert RC.rs_rejects(x, 128, "f16", True, RC.rs_model(x, 128, "f16", True, fault))
    print(f"rowstats fault {fault}: rejected by {len(caught)} cases: {caught[:6]}{' ...' if len(caught) > 6 else ''}")
    assert caught, f"no case rejects {fault}"


@pytest.mark.parametrize("fault", RC.TR_FAULTS)
def test_transpose_fault_is_rejected(fault):
    caught = []
    for case in RC.TR_CASES:
        x, ref = RC.tr_input(case), RC.tr_reference(case)
        assert np.array_equal(RC.tr_model(case, x), ref), "the sound model must pass"
        if not np.array_equal(RC.tr_model(case, x, fault), ref):
            caught.append(RC.tr_id(case))
    print(f"transpose fault {fault}: rejected by {len(caught)} cases: {caught}")
    assert caught, f"no case rejects {fault}"
    if fault == "clip_last_c_tile":
        assert any("C328" in c for c in caught)


# ---- 3. refusals -----------------------------------------------------------------------------------------------------
BASE = dict(x=RC.PTR, y16=RC.PTR + (1 << 20), y16_lo=RC.PTR + (2 << 20), part=RC.PTR + (3 << 20), vt=RC.PTR + (1 << 20))


def test_rowstats_refusal_table():
    assert {code for _, code, _ in RC.RS_REFUSED} == {RC.E_ARG, RC.E_SHAPE, RC.E_ALIGN}
    for cid, code, change in RC.RS_REFUSED:
        args = RC.rs_call_args(change, BASE)
        assert RC.rowstats_refusal(*args) == code, cid
    for cid, change in RC.RS_ACCEPTED:
        assert RC.rowstats_refusal(*RC.rs_call_args(change, BASE)) == 0, cid


def test_transpose_refusal_table():
    assert {code for _, code, _ in RC.TR_REFUSED} == {RC.E_ARG, RC.E_SHAPE, RC.E_ALIGN}
    for cid, code, change in RC.TR_REFUSED:
        args = RC.tr_call_args(change, BASE)
        assert RC.transpose_refusal(*args) == code, cid
    for cid, change in RC.TR_ACCEPTED:
        assert RC.transpose_refusal(*RC.tr_call_args(change, BASE)) == 0, cid
    for case in RC.TR_CASES:
        B, T, C_, ldx, tkv = RC.tr_shape(case)
        assert RC.transpose_refusal(RC.PTR, ldx, B, T, C_, RC.PTR, tkv) == 0 and ldx >= C_, case
