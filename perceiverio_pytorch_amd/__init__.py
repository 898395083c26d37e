"""perceiverio_pytorch_amd: the PerceiverIO forward hot path as hand-written MI355X (gfx950) HIP kernels
behind a C-ABI (include/pio_hip.h), exposed through the reference's own nn.Module surface."""
from .runtime import (get_backend, get_precision_policy, invalidate_packed_weights, set_backend,  # noqa: F401
                      set_precision_policy)
from ._lib import PioError, build, lib  # noqa: F401
from .probe import (logit_probe, range_probe, recommend_operand_dtype,  # noqa: F401
                    recommend_precision_policy)
from .flow_image import flow_to_image  # noqa: F401

# flow_to_image of a CUDA fp32 tensor under the hip backend: pio_flow_to_image (two launches, nothing read back) when True;
# False sends it down the torch restatement of the same formula (flow_image.restatement), which every other input takes
fused_flow_image = True

from .image_prep import prepare_images  # noqa: E402,F401

# prepare_images of CUDA uint8 / fp32 images under the hip backend: pio_prepare_images (one launch per 32 sources) when True;
# False sends them down the torch chain (image_prep.chain), which CPU tensors and whatever the plan declines take
fused_image_prep = True

from .media import to_frames, to_pcm16, top_labels  # noqa: E402,F401

# to_frames / to_pcm16 of a CUDA fp32 tensor under the hip backend: pio_finish_media (one launch, the tensor read in place)
# when True; False sends them down the torch restatement of the same formulas (media.restatement, the same bits), which
# every other input takes
fused_media = True

__version__ = "0.1.0"
