"""The four task models of the reference, assembled from the HIP-backed PerceiverIO core and the torch I/O plumbing:
ClassificationPerceiver (classification_perceiver.py), LanguagePerceiver (language_perceiver.py), FlowPerceiver
(flow_perceiver.py), MultiModalPerceiver (multimodal_perceiver.py).  Same constructor arguments, `self.perceiver`
attribute and state_dict keys, so `load_state_dict(ckpt["model_state_dict"])` of a reference checkpoint works.  The fused
tile blend of FlowPerceiver (_blend_tiles_fused) is a hook into fused_io.py."""
from __future__ import annotations

import itertools
from enum import Enum
from typing import NamedTuple, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import fused_io as FIO
from . import image_prep
from . import io_processors
from . import media
from . import runtime as R
from .io_processors import (AudioPostprocessor, AudioPreprocessor, ClassificationPostprocessor,
                            EmbeddingPostprocessor, EmbeddingPreprocessor, FlowPostprocessor, ImagePreprocessor,
                            OneHotPreprocessor, ProjectionPostprocessor)
from .output_queries import FlowQuery, FourierQuery, TrainableQuery
from .perceiver import PerceiverIO
from .runtime import get_backend, precision, split_policy, split_policy3  # noqa: F401  (both re-exported)
from .position_encoding import PosEncodingType


# Precision policy each task model runs under unless `model.precision_policy` is changed (None = the global policy of
# perceiverio_pytorch_amd.set_precision_policy).  The defaults are the fastest policies that meet the 1e-3 parity bar
# against the reference on that architecture (tests/test_models.py).
# "A/B" = policy A for the encoder (cross-attend + latent stack), B for the decoder: the dense-output models (one
# output per pixel / sample, nothing averaged behind the decoder) owe almost all of their error to operand rounding in
# the decoder (tools/policy_mix.py, full-size flow: x2w everywhere 5.8e-4 / 1.5e-3; decoder alone at x3 1.1e-4 /
# 1.1e-4; everything at x3 5e-6 at 9x the time), so they run the encoder on the fused single-sweep kernels and only the
# decoder with split operands.
# The decoder half runs "x3f": split operands in every projection / MLP / head GEMM, the attention core itself
# single-sweep on the fused kernel with its output returned as a pair (flow: 9.5e-5 / 2.0e-4 at 9.2 ms against 9.3e-5 /
# 1.0e-4 at 12.0 ms with a fully 3-sweep decoder, and no score matrix at all: peak memory 0.7 instead of 4.6 GiB on
# the full-size multimodal model).
# Round 3: the decoders of the dense-output models run "x2af" -- split ACTIVATIONS against single weights (two sweeps)
# around the single-sweep fused core: their error is the rounding of the wide-range query / latent activations, not of
# the weights (flow 1.6e-4 / 2.7e-4 at 7.4 ms, multimodal chunk 3.9e-4 / 4.8e-4 at 49 ms instead of 55; with split weights
# and single activations -- "x2w" -- the max figure is 1.3-1.5e-3), and the flow encoder single-sweep fp16 (its error
# does not show behind the decoder's: 1.07e-4 with "fp16/fp16x3f" against 1.5e-4 with "fp16x2w/fp16x3f").
# Late round 3: the classifier's default is "fp16x3f/fp16sd/fp16x3f" -- the 48-layer stack single-sweep with
# error-feedback rounding of its shared weights ("fp16sd"), the two cross-attends (weights applied once: encoder input
# and decoder, 1.2 of 16.5 ms) with split operands around the fused single-sweep core.  Six B = 4 goldens, worst case:
# 3.2e-4 / 3.9e-4 at 17.5 ms -- "fp16x2w" (the previous default) 3.1e-4 / 3.4e-4 at 20.8 ms, "fp16sd" alone 6.6e-4 /
# 7.3e-4 at 16.5 ms, "fp16sd/fp16x3f" 4.2e-4 / 5.0e-4 at 17.1 ms (tools/sd_parity.py, bench.py --policy).
# The language model (26 distinct layers: nothing to feed back over) keeps split weights for proj_v / final in the stack
# ("fp16x2s") and takes the same split-operand cross-attends: 3.7e-4 / 3.9e-4 at 27.6 ms for B = 100 against "fp16x2w"
# 3.8e-4 / 4.8e-4 at 28.4 ms; "fp16/fp16x3f" (single-sweep stack) passes the bar at 6.4e-4 / 8.7e-4 and 22.8 ms.
# Round 4 widened what the margins are measured on (oracle/cases.py: two classifier goldens with TRAINED-LIKE parameter
# statistics -- log-normal weight-row scales over a decade, LayerNorm gains in [0.2, 5], outlier channels -- and a second
# parameter / input seed for each dense-output model at full size) and two defaults moved (tools/r4_policy_table.py):
#  * classifier: "fp16sd" alone FAILS the trained-like golden on natural-image inputs (8.3e-4 / 1.72e-3); with the decoder
#    split ("fp16sd/fp16x3f") 6.7e-4 / 1.23e-3; the heavy-tailed rows sit in the two cross-attends.  Eight goldens, worst
#    case: "fp16x3f/fp16sd/fp16x3f" 4.9e-4 / 6.6e-4 at +7.4 % time over "fp16sd"; "fp16x2w/fp16sd/fp16x3f" (the encoder's
#    cross-attend with split WEIGHTS only: two sweeps instead of three) 5.6e-4 / 5.8e-4 at +4.8 %;
#    "fp16x2w/fp16sd/fp16x2w" 6.5e-4 / 9.5e-4 at +2.3 %.  With the K / V projection fold of the DECODER (single-weight
#    policies; xattn_tall_kernel on the LayerNorm'd latents) "fp16x2w/fp16sd/fp16x2af" -- decoder activations split, its K / V
#    weights folded exactly -- holds 6.05e-4 / 5.6e-4 at +3.3 % (16.26 against 16.49 ms for the x3f decoder on one box):
#    THE DEFAULT since late round 4.
#  * multimodal: "fp16x2w/fp16x2af" holds on seed 31 (3.9e-4 / 4.8e-4) and FAILS seed 32 (1.01e-3 / 1.14e-3: there the
#    rounding of the decoder's WEIGHTS dominates, on seed 31 that of its activations -- "x2w" decoders fail seed 31 at
#    1.3e-3); with both split ("fp16x2w/fp16x3f") 0.6e-4 / 2.7e-4 on both at +17 % time.  Which weights: splitting only the
#    OUTPUT side of the decoder -- attention out projection, final_layer, the heads behind it ("fp16x2afo") -- holds
#    4.0e-4 / 5.3e-4 on both seeds at +4 % (each alone does not: post 7.5e-4 / 9.7e-4, final 7.6e-4 / 6.6e-4, final_layer
#    9.3e-4 / 1.09e-3, fc1 + fc2 8.4e-4 / 9.3e-4 at +13 %): the default now.
#  * language (round 4: LayerNorm fold + fused q|k|v now serve its 1280-channel stack, whose residual stream is then a
#    22-bit pair instead of 11-bit LayerNorm outputs): "fp16x3f/fp16x2s/fp16x3f" 3.7e-4 / 4.1e-4 at 24.0 ms (B = 100);
#    "fp16x2w/fp16x2o/fp16x3f" -- encoder cross-attend with split weights only, of the stack's weights only the out
#    projection split ("fp16x2o") -- 5.4e-4 / 5.7e-4 at 21.0 ms: the default now; a fully single-sweep stack
#    ("fp16x3f/fp16/fp16x3f") 6.1e-4 / 6.2e-4 at 20.5 ms.
#    KNOWN LIMIT (tests/golden/model_language_trained): with trained-like statistics (LayerNorm gains up to 5) the
#    attention logits of this model reach |s| ~ 10-15, and q / k rounded ONCE to fp16 in front of the fused cores put
#    delta s ~ |s| 2^-11 into the exponent: 2.6e-3 / 4.1e-3 under every policy with fused single-sweep cores in the
#    cross-attends (the latent stack's cores alone -- "fp16x3/fp16x3f/fp16x3", 50 ms -- 7.1e-4 / 8.7e-4 ... 1.03e-3 by
#    rounding realisation); only "fp16x3" (materialised fp32 scores, 1e-5, 59 ms) holds there.  Q / K as 16-bit pairs in
#    the cores' Q K^T (three MFMAs instead of one on 1/6 of a 32-wide head's flops; not built) would remove the cores'
#    share, but on that golden the stack's GEMMs alone leave 8e-4 ... 1e-3 under "x2w" / "x2s" (exact cross-attends,
#    "fp16x3/fp16x2w/fp16x3f": 1.09e-3 / 1.44e-3; "fp16x3/fp16x2s/fp16x3": 1.20e-3 / 1.34e-3): with those statistics this
#    model needs three-sweep GEMMs AND pair cores, i.e. about twice the default's time.
DEFAULT_POLICY = {"ClassificationPerceiver": "fp16x2w/fp16sd/fp16x2af", "LanguagePerceiver": "fp16x2w/fp16x2o/fp16x3f",
                  "FlowPerceiver": "fp16/fp16x2af", "MultiModalPerceiver": "fp16x2w/fp16x2afo"}


class _policy_scope:
    """Runs a block under a task model's precision policy: the ambient policy is the encoder's, the decoder's override
    is set on the PerceiverIO core for the duration."""

    def __init__(self, model):
        self._model = model
        cross, enc, dec = split_policy3(model.precision_policy)
        self._ctx = precision(enc)
        self._dec = dec if dec != enc else None
        self._cross = cross if cross != enc else None

    def __enter__(self):
        # a decoder policy the USER set on the core (model.perceiver.decoder_policy = ...) wins over the decoder half of
        # the model's "encoder/decoder" policy string; it is restored untouched afterwards either way.  Likewise the
        # cross-attend's own policy (PerceiverEncoder.cross_attend_policy).
        core = self._model.perceiver
        self._saved = core.decoder_policy
        if self._saved is None:
            core.decoder_policy = self._dec
        self._saved_cross = core._encoder.cross_attend_policy
        if self._saved_cross is None:
            core._encoder.cross_attend_policy = self._cross
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self._model.perceiver.decoder_policy = self._saved
        self._model.perceiver._encoder.cross_attend_policy = self._saved_cross
        return self._ctx.__exit__(*exc)


class PrepType(Enum):
    FOURIER_POS_CONVNET = 1
    LEARNED_POS_1X1CONV = 2
    FOURIER_POS_PIXEL = 3


class ClassificationPerceiver(nn.Module):
    """ImageNet classifier: 512 x 1024 latents, 8 blocks x 6 self-attends, 1000 learned queries (reference
    classification_perceiver.py:21-131)."""

    def __init__(self, num_classes: int = 1000, img_size: Sequence[int] = (224, 224), img_channels: int = 3,
                 prep_type: PrepType = PrepType.FOURIER_POS_CONVNET, num_self_attends_per_block: int = 6,
                 num_blocks: int = 8, num_latents: int = 512, num_latent_channels: int = 1024,
                 precision_policy: str = DEFAULT_POLICY["ClassificationPerceiver"], decode_row0_only: bool = False):
        super().__init__()
        self.precision_policy = precision_policy
        fourier = dict(concat_pos=True, num_bands=64, sine_only=False)
        if prep_type == PrepType.FOURIER_POS_CONVNET:
            prep = ImagePreprocessor(img_size=img_size, input_channels=img_channels, prep_type="conv",
                                     position_encoding_type=PosEncodingType.FOURIER,
                                     fourier_position_encoding_kwargs=dict(max_resolution=(56, 56), **fourier))
        elif prep_type == PrepType.LEARNED_POS_1X1CONV:
            prep = ImagePreprocessor(img_size=img_size, input_channels=img_channels, prep_type="conv1x1",
                                     position_encoding_type=PosEncodingType.TRAINABLE,
                                     trainable_position_encoding_kwargs=dict(init_scale=0.02, num_channels=256),
                                     project_pos_dim=256, num_channels=256, spatial_downsample=1,
                                     concat_or_add_pos="concat")
        elif prep_type == PrepType.FOURIER_POS_PIXEL:
            prep = ImagePreprocessor(img_size=img_size, input_channels=img_channels, prep_type="pixels",
                                     spatial_downsample=1, position_encoding_type=PosEncodingType.FOURIER,
                                     fourier_position_encoding_kwargs=dict(max_resolution=(224, 224), **fourier))
        else:
            raise ValueError(f"Unknown prep_type type: {prep_type}")
        self.perceiver = PerceiverIO(
            num_blocks=num_blocks, num_self_attends_per_block=num_self_attends_per_block, num_latents=num_latents,
            num_latent_channels=num_latent_channels, input_preprocessors=prep,
            perceiver_encoder_kwargs=dict(num_self_attend_heads=8, use_query_residual=True),
            output_queries=TrainableQuery(output_index_dims=num_classes, num_channels=1024, init_scale=0.02),
            perceiver_decoder_kwargs=dict(use_query_residual=prep_type != PrepType.LEARNED_POS_1X1CONV),
            final_project_out_channels=num_classes,
            output_postprocessors=ClassificationPostprocessor(num_classes=num_classes, num_input_channels=num_classes,
                                                              project=False))
        # opt-in: the postprocessor keeps query row 0 only (postprocessors.py:187), and decoder rows are independent
        self.decode_row0_only = decode_row0_only
        self.img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)

    # example_img_classify.py: the pixel statistics its Normalize is given
    MEAN_RGB = (0.485 * 255, 0.456 * 255, 0.406 * 255)
    STDDEV_RGB = (0.229 * 255, 0.224 * 255, 0.225 * 255)

    def prepare(self, images) -> torch.Tensor:
        """Photographs (a tensor or a list of differently sized ones, values 0 .. 255) as the example prepares them: centre
        square, antialiased bilinear resize to img_size, Normalize(MEAN_RGB, STDDEV_RGB): [N, 3, H, W] for forward()."""
        return image_prep.prepare_images(images, self.img_size, crop="center", antialias=True, mean=self.MEAN_RGB,
                                         std=self.STDDEV_RGB)

    @property
    def decode_row0_only(self) -> bool:
        return self.perceiver.decoder_query_rows is not None

    @decode_row0_only.setter
    def decode_row0_only(self, on: bool) -> None:
        self.perceiver.decoder_query_rows = slice(0, 1) if on else None

    # The encoder input of the LEARNED_POS_1X1CONV and FOURIER_POS_PIXEL variants from ONE HIP launch each for CUDA fp32
    # images under the hip backend (ImagePreprocessor.fused_conv1x1 -> pio_conv1x1_tokens, with the projected position table
    # built once and handed over next to the features; ImagePreprocessor.fused_pixels -> pio_assemble_tokens); False restores
    # the chain of torch ops and the concatenated hand-off.  The pixel variant gives the same bits either way.
    @property
    def fused_front_end(self) -> bool:
        prep = self.perceiver._multi_preprocessor._preprocessors["__default"]
        return prep.fused_conv1x1 and prep.fused_pixels

    @fused_front_end.setter
    def fused_front_end(self, on: bool) -> None:
        prep = self.perceiver._multi_preprocessor._preprocessors["__default"]
        prep.fused_conv1x1 = prep.fused_pixels = bool(on)

    def forward(self, img: torch.Tensor):
        """img: (batch, channels, H, W) -> logits (batch, num_classes)."""
        with _policy_scope(self):
            return self.perceiver(img)

    def classify(self, images: torch.Tensor, k: int = 5, return_logits: bool = False) -> "Labels":
        """Labels(ids int64 [B, k], probs fp32 [B, k], logits [B, num_classes] or None): the k most probable classes, most
        probable first (media.top_labels: on the device, nothing read back).  The forward of this call decodes query row 0
        alone, whatever decode_row0_only says; the setting is restored afterwards, also when the forward raises."""
        core = self.perceiver
        saved = core.decoder_query_rows
        core.decoder_query_rows = slice(0, 1)
        try:
            logits = self.forward(images)
        finally:
            core.decoder_query_rows = saved
        ids, probs = media.top_labels(logits, k)
        return Labels(ids, probs, logits if return_logits else None)


class Labels(NamedTuple):
    """classify(): ids int64 [B, k], probs fp32 [B, k] (softmax, most probable first), logits fp32 [B, num_classes] or None."""
    ids: torch.Tensor
    probs: torch.Tensor
    logits: Optional[torch.Tensor]


class Media(NamedTuple):
    """MultiModalPerceiver.reconstruct: frames uint8 [B, T, H, W, 3], pcm int16 of the audio's shape, label logits [B, classes]."""
    frames: torch.Tensor
    pcm: torch.Tensor
    label: torch.Tensor


class Prediction(NamedTuple):
    """LanguagePerceiver.predict: ids int64 [B, P, k], logprobs fp32 [B, P, k], logits fp32 [B, P, V] or None."""
    ids: torch.Tensor
    logprobs: torch.Tensor
    logits: Optional[torch.Tensor]


class LanguagePerceiver(nn.Module):
    """Byte-level masked language model: 256 x 1280 latents, 26 self-attends (reference language_perceiver.py:10-74)."""

    def __init__(self, vocab_size: int = 262, max_seq_len: int = 2048, embed_dim: int = 768,
                 num_self_attends_per_block: int = 26, num_blocks: int = 1, num_latents: int = 256,
                 num_latent_channels: int = 1280, precision_policy: str = DEFAULT_POLICY["LanguagePerceiver"]):
        super().__init__()
        self.precision_policy = precision_policy
        prep = EmbeddingPreprocessor(vocab_size=vocab_size, max_seq_len=max_seq_len, embedding_dims=embed_dim)
        prep.need_tokens = False     # (the TrainableQuery below never reads the position-free tokens)
        self.perceiver = PerceiverIO(
            final_project=False, num_self_attends_per_block=num_self_attends_per_block, num_blocks=num_blocks,
            num_latents=num_latents, num_latent_channels=num_latent_channels, input_preprocessors=prep,
            output_postprocessors=EmbeddingPostprocessor(prep.embed),
            perceiver_encoder_kwargs=dict(num_self_attend_heads=8, num_cross_attend_heads=8, qk_channels=8 * 32,
                                          v_channels=num_latent_channels, use_query_residual=True),
            perceiver_decoder_kwargs=dict(qk_channels=8 * 32, v_channels=embed_dim, num_heads=8,
                                          use_query_residual=False),
            output_queries=TrainableQuery(output_index_dims=max_seq_len, num_channels=embed_dim))

    # The encoder input -- the byte embedding gathered by id plus the learned position embedding -- comes from ONE HIP launch
    # (EmbeddingPreprocessor.fused_embedding -> pio_embed_tokens) for CUDA int32 / int64 ids of the full sequence length
    # under the hip backend; False restores nn.Embedding, the add and the one-element torch.cat.  Same bits either way.
    # An id outside [0, vocab_size) gives a NaN row and sets prep.bad_ids_flag(device) instead of ATen's device-side assert.
    @property
    def fused_front_end(self) -> bool:
        return self.perceiver._multi_preprocessor._preprocessors["__default"].fused_embedding

    @fused_front_end.setter
    def fused_front_end(self, on: bool) -> None:
        self.perceiver._multi_preprocessor._preprocessors["__default"].fused_embedding = bool(on)

    def forward(self, inputs: torch.Tensor, input_masks: torch.Tensor):
        with _policy_scope(self):
            return self.perceiver(inputs, input_mask=input_masks, query_mask=input_masks)

    # predict(): only the positions asked for are decoded (decoder rows are independent), and the rows become logits,
    # log-probabilities and top-k ids on the device (EmbeddingPostprocessor.fused_predict -> pio_vocab_topk); False restores
    # the chain behind the decoder: the tied-embedding GEMM, log_softmax and topk in torch.
    @property
    def fused_predict(self) -> bool:
        return self.perceiver._output_postprocessors["__default"].fused_predict

    @fused_predict.setter
    def fused_predict(self, on: bool) -> None:
        self.perceiver._output_postprocessors["__default"].fused_predict = bool(on)

    def _positions(self, positions, batch: int, device):
        """`positions` of predict() as a validated int64 index tensor [P] or [B, P] on `device` (None: None)."""
        t = self.perceiver._output_queries["__default"]._position_encoding.pos_embs.shape[0]
        if positions is None:
            return None
        if not isinstance(positions, torch.Tensor):
            positions = torch.as_tensor(list(positions), dtype=torch.int64)
        if positions.dtype.is_floating_point or positions.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise ValueError(f"predict: positions must be integers, got {positions.dtype}")
        if positions.dim() not in (1, 2) or (positions.dim() == 2 and positions.shape[0] != batch):
            raise ValueError(f"predict: positions must be [P] or [{batch}, P], got {tuple(positions.shape)}")
        if positions.shape[-1] < 1:
            raise ValueError("predict: no positions")
        host = positions.detach().cpu()          # (a CUDA tensor: the one read-back)
        lo, hi = int(host.min()), int(host.max())
        if lo < 0 or hi >= t:
            raise ValueError(f"predict: position {lo if lo < 0 else hi} outside [0, {t})")
        return positions.detach().to(device=device, dtype=torch.int64)

    def predict(self, inputs: torch.Tensor, input_masks: torch.Tensor, positions=None, k: int = 5,
                return_logits: bool = False) -> "Prediction":
        """Masked-token prediction: Prediction(ids int64 [B, P, k], logprobs fp32 [B, P, k], logits fp32 [B, P, V] or None) --
        the k most probable tokens of every chosen position, most probable first, with their log-probabilities.

        positions: a sequence of ints or an integer tensor [P] (the same positions for every sample) or [B, P] (each sample
        its own); None: every position.  A CPU tensor or a sequence is validated where it is; a CUDA tensor is read back to
        the host ONCE for validation (a synchronisation).  An index outside [0, max_seq_len) or an empty selection raises
        ValueError before anything reaches the device, and so does k outside [1, vocab_size]."""
        post = self.perceiver._output_postprocessors["__default"]
        if not 1 <= int(k) <= post._vocab_size:
            raise ValueError(f"predict: k = {k} outside [1, vocab_size = {post._vocab_size}]")
        index = self._positions(positions, inputs.shape[0], inputs.device)
        with _policy_scope(self):
            out = self.perceiver(inputs, input_mask=input_masks, query_mask=input_masks, query_index=index,
                                 postprocess=lambda rows: post.predict(rows, int(k), bool(return_logits)))
        return Prediction(*out)


class FlowPerceiver(nn.Module):
    """Optical flow: 3x3 patches of a frame pair in, dense per-pixel queries out (reference flow_perceiver.py:20-199)."""

    # test_mode under the hip backend, CUDA fp32: the tile groups' flows are kept as they come and blended by ONE HIP launch
    # behind the last group (pio_flow_blend_tiles) instead of a multiply, two pads and two full-image adds per tile and a
    # ramp built on the host.  Same bits.  False (and whatever _blend_tiles_fused declines): the chain.
    fused_blend = True

    def __init__(self, img_size: Sequence[int] = (368, 496), flow_scale_factor: int = 20 / 100,
                 num_latents: int = 2048, num_latent_channels=512, num_self_attends_per_block: int = 24,
                 num_blocks: int = 1, mixed_precision: bool = False, precision_policy: str = None):
        super().__init__()
        # The reference wraps the forward in torch.cuda.amp.autocast(enabled=mixed_precision) (flow_perceiver.py:14,
        # 129): fp16 matmul operands, fp32 accumulation -- that is this library's single-sweep `fp16` policy.  An
        # explicit precision_policy wins; otherwise mixed_precision=False keeps the validated class default.
        if precision_policy is None:
            precision_policy = "fp16" if mixed_precision else DEFAULT_POLICY["FlowPerceiver"]
        self.precision_policy = precision_policy
        self.mixed_precision = mixed_precision
        self._flow_scale_factor = flow_scale_factor
        self.query_shard = None      # (rank, world): decode this rank's query rows only + all-gather (dist.py)
        self.tiles_per_call = 4      # test-mode tiling: tiles batched per forward (1 = the reference's one at a time)
        # CUDA fp32 frames under the hip backend reach the preprocessor as the RAW pair: 3x3 patches, the frames side
        # by side and the 54 -> 64 projection are one HIP pass (pio_flow_patch_tokens) instead of pad / unfold / two
        # permute copies / a BLAS call.  False (and every other input): patches_for_flow here, as the reference does.
        self.fused_front_end = True
        prep = ImagePreprocessor(img_size=img_size, input_channels=3 * 3 ** 2, prep_type="patches",
                                 spatial_downsample=1, temporal_downsample=2, conv_after_patching=True,
                                 num_channels=64, n_extra_pos_mlp=0, position_encoding_type=PosEncodingType.FOURIER,
                                 fourier_position_encoding_kwargs=dict(num_bands=64, max_resolution=img_size,
                                                                       sine_only=False, concat_pos=True))
        self.perceiver = PerceiverIO(
            final_project_out_channels=2, num_blocks=num_blocks,
            num_self_attends_per_block=num_self_attends_per_block, num_latents=num_latents,
            num_latent_channels=num_latent_channels, perceiver_encoder_kwargs=dict(num_self_attend_heads=16),
            perceiver_decoder_kwargs=dict(output_w_init="zeros"),
            output_queries=FlowQuery(preprocessed_input_channels=prep.n_output_channels(), output_img_size=img_size,
                                     output_num_channels=2),
            input_preprocessors=prep,
            output_postprocessors=FlowPostprocessor(img_size=img_size, flow_scale_factor=flow_scale_factor))
        self.H, self.W = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)

    @staticmethod
    def prepare(img) -> torch.Tensor:
        """A frame (or a batch of frames) with values 0 .. 255 scaled to [-1, 1], at its own size: (x - 127.5) / 127.5, which
        is example_opt_flow.py's 2 (x / 255) - 1 up to rounding (2 ulp of 1.0 at most over the 256 byte values)."""
        return image_prep.prepare_images(img, None, mean=127.5, std=127.5)

    def compute_grid_indices(self, image_shape: tuple, min_overlap: int):
        """Top-left corners of training-size tiles covering the image with at least ``min_overlap`` overlap."""
        return itertools.product(*self._grid_axes(image_shape, min_overlap))

    def _grid_axes(self, image_shape: tuple, min_overlap: int):
        """(ys, xs): the corners are their product, ys outer."""
        if min_overlap >= self.H or min_overlap >= self.W:
            raise ValueError(f"Overlap should be less than size of patch (got {min_overlap}"
                             f"for patch size {(self.H, self.W)}).")
        ys = list(range(0, image_shape[0], self.H - min_overlap))
        xs = list(range(0, image_shape[1], self.W - min_overlap))
        ys[-1] = image_shape[0] - self.H
        xs[-1] = image_shape[1] - self.W
        if image_shape[0] == self.H:
            ys = [0]
        if image_shape[1] == self.W:
            xs = [0]
        return ys, xs

    def _predict_patch(self, patch):
        fused = self.fused_front_end and patch.is_cuda and patch.dtype == torch.float32 and get_backend() == "hip"
        with _policy_scope(self):
            x = patch if fused else io_processors.patches_for_flow(patch).movedim(-1, -3)
            return self.perceiver(x, query_shard=self.query_shard)

    def _blend_tiles_fused(self, pair, h, w, min_overlap):
        return FIO.blend_tiles(self, pair, h, w, min_overlap)

    def forward(self, image1: torch.Tensor, image2: torch.Tensor, test_mode: bool = False, min_overlap: int = 20):
        h, w = image1.shape[2], image1.shape[3]
        pair = torch.stack([image1.contiguous(), image2.contiguous()], dim=1)
        if h < self.H:
            raise ValueError(f"Height of image (shape: {image1.shape}) must be at least {self.H:}."
                             "Please pad or resize your image to the minimum dimension.")
        if w < self.W:
            raise ValueError(f"Width of image (shape: {image1.shape}) must be at least {self.W}."
                             "Please pad or resize your image to the minimum dimension.")
        if not test_mode:
            assert h == self.H and w == self.W, \
                f"In training mode images must have size equal to specified img_size {(self.H, self.W)}"
            return self._predict_patch(pair)
        fused = self._blend_tiles_fused(pair, h, w, min_overlap)
        if fused is not None:
            return fused
        # tiled inference: every tile's flow is blended with a linear ramp that peaks at the tile centre
        yy, xx = torch.meshgrid(torch.arange(self.H), torch.arange(self.W), indexing="ij")
        ramp = torch.minimum(torch.minimum(xx + 1, self.W - xx), torch.minimum(yy + 1, self.H - yy))
        ramp = (ramp / ramp.max())[None, None].to(image1.device)
        # Tiles are independent samples: `tiles_per_call` of them go through the model as ONE batch (the reference runs
        # them one at a time, flow_perceiver.py:165-190) -- same flows, blended in the same order, with the latent
        # stack's GEMMs seeing tiles_per_call x 2048 rows instead of 2048.
        total, weight = 0, 0
        corners = list(self.compute_grid_indices((h, w), min_overlap))
        b = pair.shape[0]
        step = max(1, int(self.tiles_per_call))
        for i in range(0, len(corners), step):
            group = corners[i:i + step]
            tiles = torch.cat([pair[..., y:y + self.H, x:x + self.W] for y, x in group], dim=0)
            flows = self._predict_patch(tiles)
            for j, (y, x) in enumerate(group):
                flow = flows[j * b:(j + 1) * b]
                pad = (x, w - x - self.W, y, h - y - self.H)
                total = total + F.pad(flow * ramp, pad)
                weight = weight + F.pad(ramp, pad)
        return total / weight


class MultiModalPerceiver(R.PackedOwner):
    """Video + audio + label auto-encoder (reference multimodal_perceiver.py:12-167).  The output is decoded in
    ``n_chunks`` query chunks.  The encoder input does not depend on the chunk (mask probabilities are 0 / 0 / 1), so
    by default the preprocess + encode step runs ONCE and only the decoder runs per chunk (`encode_once=False`
    restores the reference's recompute-everything loop; the results are identical)."""

    def __init__(self, img_size: Sequence[int] = (224, 224), img_channels: int = 3, num_frames: int = 16,
                 num_classes: int = 700, audio_samples_per_frame: int = 48000 // 25,
                 audio_samples_per_patch: int = 16, num_self_attends_per_block: int = 8, num_blocks: int = 1,
                 num_latents: int = 28 * 28 * 1, num_latent_channels: int = 512, encode_once: bool = True,
                 precision_policy: str = DEFAULT_POLICY["MultiModalPerceiver"], decode_chunks_per_call: int = 16):
        super().__init__()
        self.precision_policy = precision_policy
        # (encode_once only) how many of the n_chunks output chunks one decoder call handles: chunk k's query points
        # are the contiguous index range [k * size, (k + 1) * size), so g consecutive chunks are one range g times as
        # long -- same rows, same order, 1/g of the launches on g-times-taller (better filled) GEMMs.  Measured, full
        # size, one sample, 128 chunks (tools/mm_chunks_probe.py; ms per forward / peak GiB): g = 4 31.4 / 4.3, 8 29.1 /
        # 5.0, 16 27.6 / 6.5, 32 26.7 / 9.6, 128 25.3 / 26.5 -- the decoder workspace grows with batch x g, hence 16.
        self.decode_chunks_per_call = max(1, int(decode_chunks_per_call))
        self.H, self.W = img_size
        self.num_classes = num_classes
        self.audio_samples_per_frame = audio_samples_per_frame
        self.audio_samples_per_patch = audio_samples_per_patch
        self.encode_once = encode_once
        n_audio = num_frames * audio_samples_per_frame
        vid_res = (num_frames, self.H // 4, self.W // 4)
        preps = {
            "audio": AudioPreprocessor(samples_per_batch=n_audio, prep_type="patches",
                                       samples_per_patch=audio_samples_per_patch, n_extra_pos_mlp=0,
                                       position_encoding_type=PosEncodingType.FOURIER,
                                       fourier_position_encoding_kwargs=dict(num_bands=192,
                                                                             max_resolution=(n_audio,),
                                                                             sine_only=False, concat_pos=True)),
            "image": ImagePreprocessor(img_size=(self.H, self.W), input_channels=img_channels, num_frames=num_frames,
                                       prep_type="patches", spatial_downsample=4, temporal_downsample=1,
                                       n_extra_pos_mlp=0, position_encoding_type=PosEncodingType.FOURIER,
                                       fourier_position_encoding_kwargs=dict(num_bands=32, max_resolution=vid_res,
                                                                             sine_only=False, concat_pos=True)),
            "label": OneHotPreprocessor(input_channels=num_classes),
        }
        posts = {
            "audio": AudioPostprocessor(in_channels=512, samples_per_patch=audio_samples_per_patch),
            "image": ProjectionPostprocessor(num_inputs=512, num_outputs=3),
            "label": ClassificationPostprocessor(num_input_channels=512, num_classes=num_classes),
        }
        queries = {
            "audio": FourierQuery(concat_preprocessed_input=False,
                                  output_index_dims=(n_audio // audio_samples_per_patch,), num_bands=192,
                                  max_resolution=(n_audio,), sine_only=False, concat_pos=True),
            "image": FourierQuery(concat_preprocessed_input=False, output_index_dims=(num_frames, self.H, self.W),
                                  num_bands=32, max_resolution=vid_res, sine_only=False, concat_pos=True),
            "label": TrainableQuery(output_index_dims=(1,), concat_preprocessed_input=False, num_channels=1024,
                                    init_scale=0.02),
        }
        self.perceiver = PerceiverIO(
            num_self_attends_per_block=num_self_attends_per_block, num_blocks=num_blocks, num_latents=num_latents,
            num_latent_channels=num_latent_channels, input_preprocessors=preps, output_postprocessors=posts,
            output_queries=queries, input_padding_channels=4, output_query_padding_channels=2,
            input_mask_probs={"image": 0.0, "audio": 0.0, "label": 1.0})

    # The encoder input -- audio | video | label, each padded to 704 channels, the label replaced by its mask token, the
    # three concatenated -- comes from ONE HIP launch (MultimodalPreprocessor.fused_assembly -> pio_assemble_tokens) for
    # CUDA fp32 inputs under the hip backend; False restores the chain of torch.cat calls.  Same bits either way.
    @property
    def fused_front_end(self) -> bool:
        return self.perceiver._multi_preprocessor.fused_assembly

    @fused_front_end.setter
    def fused_front_end(self, on: bool) -> None:
        self.perceiver._multi_preprocessor.fused_assembly = bool(on)

    # The decoder query array of a chunk group -- Fourier features of the audio and video index points, the learned label
    # query, the three padding embeddings -- comes from ONE HIP launch as well (PerceiverIO.fused_queries ->
    # pio_build_queries) under the hip backend on a GPU; False restores the chain of torch ops.  Moves are the same bits
    # either way, sines and cosines agree to the device math library's accuracy.
    @property
    def fused_queries(self) -> bool:
        return self.perceiver.fused_queries

    @fused_queries.setter
    def fused_queries(self, on: bool) -> None:
        self.perceiver.fused_queries = bool(on)

    # The two narrow heads behind the decoder -- image 512 -> 3, audio 512 -> 16 -- are ONE HIP launch per decoder call
    # (PerceiverIO.fused_heads -> pio_project_heads) that reads the fp32 decoder output once and, with encode_once, writes
    # each group's rows straight into the final image / audio arrays: no 16-bit copy of the decoder output, no per-group
    # pieces, no torch.cat.  fp32 products of the unrounded decoder output, where the chain multiplies its 16-bit image.
    # False restores the chain (runtime.hip_linear per head, torch.cat behind the loop) exactly.  The label head is the
    # chain's either way.
    @property
    def fused_heads(self) -> bool:
        return self.perceiver.fused_heads

    @fused_heads.setter
    def fused_heads(self, on: bool) -> None:
        self.perceiver.fused_heads = bool(on)

    def forward(self, images: torch.Tensor, audio: torch.Tensor, n_chunks: int = 128):
        with _policy_scope(self):
            return self._forward(images, audio, n_chunks)

    def classify(self, images: torch.Tensor, audio: torch.Tensor, k: int = 5, return_logits: bool = False) -> "Labels":
        """Labels(ids int64 [B, k], probs fp32 [B, k], logits [B, num_classes] or None) without the reconstruction: the label
        is ONE query row and decoder rows are independent, so after the same preprocess + encode as forward the decoder runs
        once on that row (no chunk loop, no video or audio query, no narrow heads, nothing kept in the query cache), then the
        label head and media.top_labels.  forward's label is the mean of one estimate per chunk -- copies of this row."""
        b = images.shape[0]
        inputs = {"image": images, "audio": audio, "label": torch.zeros((b, self.num_classes), device=images.device)}
        P = self.perceiver
        with _policy_scope(self):
            x, sizes, without_pos = P._multi_preprocessor(inputs, pos=None)
            with precision(P.encoder_policy):
                latents = P._encoder(x, P._encoder.latents(x))
            query, _ = P.decoder_query(x, sizes, without_pos, modalities=("label",))
            with precision(P.decoder_policy):
                row = P._decoder(query, latents)
                logits = P._output_postprocessors["label"](row, pos=None, modality_sizes=None)
        ids, probs = media.top_labels(logits, k)
        return Labels(ids, probs, logits if return_logits else None)

    def reconstruct(self, images: torch.Tensor, audio: torch.Tensor, n_chunks: int = 128, bgr: bool = False) -> "Media":
        """forward, then the outputs as the example writes them, made on the device: Media(frames uint8 [B, T, H, W, 3] --
        clipped to [0, 1], times 255, truncated; bgr: in OpenCV's channel order --, pcm int16 of audio's shape -- times 2**15,
        truncated, saturated --, label logits): two pio_finish_media launches behind forward, its image view read in place."""
        out = self.forward(images, audio, n_chunks)
        return Media(media.to_frames(out["image"], bgr=bgr, channels_first=True), media.to_pcm16(out["audio"]), out["label"])

    def prepare_video(self, frames, bgr: bool = True) -> torch.Tensor:
        """Decoded frames (a [T, H, W, 3] tensor or a list of [H, W, 3] ones, values 0 .. 255; bgr: in OpenCV's channel
        order) as example_multimodal.py's load_video prepares them: crop_center_square (its own corner, x // 2 - m // 2),
        bilinear resize without antialiasing to the model's frame size, RGB order, / 255: [1, T, 3, H, W] for forward()."""
        shapes = [frames.shape[1:3]] * frames.shape[0] if isinstance(frames, torch.Tensor) else [f.shape[:2] for f in frames]
        boxes = [(h // 2 - min(h, w) // 2, w // 2 - min(h, w) // 2, min(h, w), min(h, w)) for h, w in shapes]
        x = image_prep.prepare_images(frames, (self.H, self.W), crop=boxes, antialias=False, reverse_channels=bgr, std=255.0,
                                      channels_last=True)
        return x.unsqueeze(0)

    # The decoder query array of an output chunk -- Fourier features of the chunk's index points, the learned label
    # query, the padding embeddings -- depends on no input, only on parameters and constants (every output query of
    # this model has concat_preprocessed_input=False): like the packed weight images it is built once per (parameter
    # version, chunk group, device) and kept -- as ONE batch-invariant [1, Q, C] array (412 MB per group of 16 chunks,
    # 3.3 GB for the 128 chunks of a forward, whatever the batch) that every sample reads through a stride-0 view: the
    # decoder then also normalises / projects the queries once per call instead of once per sample.  The cache is bounded
    # in BYTES (`query_cache_max_bytes`, default 8 GiB: two chunkings of a forward); `cache_queries=False` rebuilds the
    # array on every call, as the reference does (multimodal_perceiver.py:146-161 -> perceiver.py:327-367).
    cache_queries = True
    cache_projected_queries = True      # (needs cache_queries: the projection is kept beside the array it belongs to)
    query_cache_max_bytes = 8 << 30

    def _chunk_queries(self, x, sizes, without_pos, points, chunk_key):
        P = self.perceiver
        if not self.cache_queries:
            return P.decoder_query(x, sizes, without_pos, subsampled_points=points) + (None,)
        params = [p for q in P._output_queries.values() for p in q.parameters()] + list(P.padding_embeddings.parameters())
        key = (chunk_key, str(x.device), tuple(sorted(sizes.items())), R.param_key(*params)[:-1])

        def build():
            with torch.inference_mode(False), torch.no_grad():
                # (the queries read the batch size and the device from their input, nothing else: a ONE-sample stand-in of
                #  the right length keeps the cached array batch-invariant and an ordinary -- not inference-mode -- tensor)
                shape_only = torch.zeros((1, x.shape[1], 1), device=x.device)
                q, qsizes = P.decoder_query(shape_only, sizes, None, subsampled_points=points)
            nbytes = q.numel() * q.element_size()
            held = sum(v[0].numel() * v[0].element_size() for v in self._packed.values())
            if held + nbytes > self.query_cache_max_bytes:
                self._packed.clear()
            return (q, qsizes, {}), None          # ({}: the decoder's cache of the PROJECTED queries of this array)

        # (one slot per key: the arrays of every chunk group and parameter version stay side by side, up to the byte cap)
        q, qsizes, qc = self._packed.get(key, build, slot=key)
        return torch.broadcast_to(q, (x.shape[0],) + tuple(q.shape[1:])), qsizes, qc

    def _forward(self, images, audio, n_chunks):
        b, t, c, h, w = images.shape
        img_chunk = t * h * w // n_chunks
        aud_chunk = audio.shape[1] // self.audio_samples_per_patch // n_chunks
        inputs = {"image": images, "audio": audio,
                  "label": torch.zeros((b, self.num_classes), device=images.device)}
        P = self.perceiver
        rec = {"image": [], "audio": [], "label": []}
        cached = None
        bufs, tied = None, []       # (fused heads: the final image / audio arrays, made once; the group views that wrote them)
        step = self.decode_chunks_per_call if self.encode_once else 1
        for k in range(0, n_chunks, step):
            g = min(step, n_chunks - k)
            # (index ranges made ON THE DEVICE: a CPU torch.arange of more than 32 768 elements runs on the intra-op
            #  thread pool, whose spinning workers exhaust a container's CPU quota -- the process is then throttled
            #  for the rest of the scheduler period and the GPU queue starves for ~90 ms, several times per forward)
            dev = images.device
            points = {"image": torch.arange(img_chunk * k, img_chunk * (k + g), device=dev),
                      "audio": torch.arange(aud_chunk * k, aud_chunk * (k + g), device=dev), "label": None}
            if not self.encode_once:
                out = P(inputs, subsampled_output_points=points)
            else:
                if cached is None:
                    x, sizes, without_pos = P._multi_preprocessor(inputs, pos=None)
                    with precision(P.encoder_policy):
                        cached = (x, sizes, without_pos, P._encoder(x, P._encoder.latents(x)))
                x, sizes, without_pos, latents = cached
                query, qsizes, qc = self._chunk_queries(x, sizes, without_pos, points, (k, g, n_chunks))
                from .perceiver import restructure
                with precision(P.decoder_policy):
                    # (qc: LayerNorm_q + proj_q of a cached -- parameter-only -- query array run once, not per forward:
                    #  206 MB of projected queries per group of 16 chunks at the default policy)
                    decoded = P._decoder(query, latents, q_cache=qc if self.cache_projected_queries else None)
                    # (fused heads: every group writes its rows of the final arrays in place -- no per-group pieces, no
                    #  torch.cat behind the loop.  The decision does not depend on the group: taken at the first one.)
                    if k == 0 and P._heads_accept(decoded):
                        patch = self.audio_samples_per_patch
                        bufs = {"image": torch.empty((b, img_chunk * n_chunks, c), dtype=torch.float32, device=dev),
                                "audio": torch.empty((b, aud_chunk * n_chunks, patch), dtype=torch.float32, device=dev)}
                    out = None
                    if bufs is not None:
                        into = {"image": bufs["image"][:, img_chunk * k:img_chunk * (k + g)],
                                "audio": bufs["audio"][:, aud_chunk * k:aud_chunk * (k + g)]}
                        out = P._project_heads(decoded, qsizes, into=into)
                        if out is not None:
                            tied += [out["image"], out["audio"]]
                    if out is None:
                        per_mod = restructure(qsizes, decoded)
                        out = {m: post(per_mod[m], pos=None, modality_sizes=None)
                               for m, post in P._output_postprocessors.items()}
                        if bufs is not None:
                            for m in into:
                                into[m].copy_(out[m].reshape(into[m].shape))
            if bufs is None:
                rec["image"].append(out["image"])
                rec["audio"].append(out["audio"])
            rec["label"].extend([out["label"][:, None]] * g)      # (one label estimate per chunk, as the reference has)
        if bufs is not None:
            image, sound = R.forward_only(bufs["image"], *tied), R.forward_only(bufs["audio"], *tied)
        else:
            image, sound = torch.cat(rec["image"], dim=1), torch.cat(rec["audio"], dim=1)
        return {"image": image.reshape([b, t, h, w, c]).moveaxis(-1, -3),
                "audio": sound.reshape(audio.shape),
                "label": torch.cat(rec["label"], dim=1).mean(dim=1)}
