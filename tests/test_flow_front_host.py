"""CPU: the float64 definition of the flow front end (tests/flow_front_cases.py) against the torch chain it stands for --
patches_for_flow -> movedim -> ImagePreprocessor._features (space_to_depth + the Linear of conv_after_patching) run in
float64 -- which pins the channel order; and the refusal table of pio_flow_patch_tokens (no launch: a refused call
returns before it touches a device)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_front_cases as FC  # noqa: E402


def make_prep(case, d, dtype):
    from perceiverio_pytorch_amd.io_processors import ImagePreprocessor
    from perceiverio_pytorch_amd.position_encoding import PosEncodingType
    hw = (case["H"], case["W"])
    prep = ImagePreprocessor(img_size=hw, input_channels=9 * case["C"], prep_type="patches", spatial_downsample=1,
                             temporal_downsample=2, conv_after_patching=not case["raw"], num_channels=case["out"],
                             position_encoding_type=PosEncodingType.FOURIER,
                             fourier_position_encoding_kwargs=dict(num_bands=4, max_resolution=hw, sine_only=False,
                                                                   concat_pos=True))
    if not case["raw"]:
        with torch.no_grad():
            prep._conv_after_patch_layer.weight.copy_(torch.from_numpy(d["w"]))
            prep._conv_after_patch_layer.bias.copy_(torch.from_numpy(d["bias"]))
    return prep.to(dtype).eval()


@pytest.mark.parametrize("name", ["odd", "thin_row", "thin_col", "raw"])
def test_definition_equals_the_torch_chain_in_float64(name):
    from perceiverio_pytorch_amd.io_processors import patches_for_flow
    case, d = FC.CASES[name], FC.gen(name)
    ref, _ = FC.reference(d)
    prep = make_prep(case, d, torch.float64)
    pair = torch.stack([torch.from_numpy(f) for f in d["frames"]], dim=1).double()
    with torch.no_grad():
        got = prep._features(patches_for_flow(pair).movedim(-1, -3)).numpy()
    assert got.shape == ref.shape == (case["N"], case["H"] * case["W"], case["out"])
    err = float(np.abs(got - ref).max())
    print(f"{name}: max |definition - torch chain| = {err:.3e}")
    assert err <= 1e-12


def test_case_table_covers_what_it_claims():
    c = FC.CASES
    assert (c["one_pixel"]["H"], c["one_pixel"]["W"]) == (1, 1)
    assert c["thin_row"]["H"] == 1 and c["thin_row"]["W"] > 64 and c["thin_col"]["W"] == 1 and c["thin_col"]["H"] > 64
    assert c["odd"]["H"] % 4 and c["odd"]["W"] % 64 and c["odd"]["N"] > 1
    assert (c["c1_out4"]["C"], c["c1_out4"]["out"], c["c4_out128"]["C"], c["c4_out128"]["out"]) == (1, 4, 4, 128)
    assert c["raw"]["raw"] and c["raw"]["out"] == 18 * c["raw"]["C"] and c["raw"]["ldy"] == 56
    s = c["strided"]
    assert s["ldy"] == 72 and s["full"][0] == (40, 100) and s["full"][0] != s["full"][1]
    for name, k in c.items():
        d = FC.gen(name)
        for t in range(2):
            (oy, ox), full = k["origin"][t], d["full"][t]
            assert oy >= 1 and ox >= 1 and oy + k["H"] < full.shape[2] and ox + k["W"] < full.shape[3], name
            inside = np.zeros(full.shape[2:], dtype=bool)
            inside[oy:oy + k["H"], ox:ox + k["W"]] = True
            assert np.isnan(full[:, :, ~inside]).all() and np.isfinite(full[:, :, inside]).all(), name


@pytest.mark.parametrize("what,changes,code", FC.REFUSALS, ids=[r[0] for r in FC.REFUSALS])
def test_refusal_table(what, changes, code):
    """Bad arguments are refused with the documented code before anything is launched: made-up (aligned, non-NULL)
    addresses are enough, and no device is needed."""
    from perceiverio_pytorch_amd import _lib as L
    ptrs = dict(frame0=0x10000, frame1=0x20000, w=0x30000, bias=0x40000, y=0x50000)
    assert FC.refusal_call(L.lib(), ptrs, changes) == code
