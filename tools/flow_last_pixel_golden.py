"""Build-container tool: the reference's full-size flow field at the points the 8x sub-sampled golden leaves out.

tests/golden/model_flow_full.npz (oracle/make_goldens.py) holds out[:, :, ::8, ::8]: rows 0..360, columns 0..488.  The
last decoder row -- pixel (367, 495) -- is off that grid.  This runs the same reference model on the same
generated parameters and frames (oracle/cases.py) once more, checks that it reproduces the committed sub-sampled golden
(to fp32 summation order: 3e-6 of the field's magnitude), and writes the last image row and the last image column to
tests/golden/model_flow_full_edge.npz:

    out_last_row [1, 2, 496] = out[:, :, 367, :]      out_last_col [1, 2, 368] = out[:, :, :, 495]

Fixtures hold tensors only.  Without a reference checkout this exits 0 without doing anything (like make_goldens.py).

    python tools/flow_last_pixel_golden.py REFERENCE_DIR       # a few minutes and ~10 GB on 8 cores
"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REF = sys.argv[1] if len(sys.argv) > 1 else ""
if (not REF or os.path.realpath(REF) == os.path.realpath(ROOT)          # (this repository's perceiver_io/ is a shim)
        or not os.path.isdir(os.path.join(REF, "perceiver_io"))):
    print("no reference checkout here: nothing to do")
    sys.exit(0)
sys.path[:0] = [os.path.join(ROOT, "oracle", "_standin"), REF, os.path.join(ROOT, "oracle")]

import torch  # noqa: E402
from cases import MODEL_CASES, gen_state_dict, model_inputs, model_seed, model_stats  # noqa: E402
from perceiver_io.flow_perceiver import FlowPerceiver  # noqa: E402  (the reference)

name = "model_flow_full"
torch.manual_seed(0)
model = FlowPerceiver(**MODEL_CASES[name]["kw"])
spec = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
params = gen_state_dict(spec, model_seed(name), model_stats(name))
model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
model.eval()
frames = [torch.from_numpy(a) for a in model_inputs(name)]
with torch.inference_mode():
    out = model(frames[0], frames[1]).numpy()
gold = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
dev = np.abs(out[:, :, ::8, ::8] - gold["out_sub"]).max() / float(gold["out_absmax"])
print(f"sub-sampled grid against the committed golden: max / absmax = {dev:.3e}")
assert dev <= 3e-6, "this run does not reproduce tests/golden/model_flow_full.npz"
np.savez_compressed(os.path.join(ROOT, "tests", "golden", name + "_edge.npz"),
                    out_last_row=out[:, :, -1, :], out_last_col=out[:, :, :, -1])
print("last pixel", out[0, :, -1, -1])
