"""MI355X-native PerceiverEncoder / PerceiverDecoder (reference: perceiver_io/perceiver.py:13-180).

Same constructor arguments, sub-module names and forward signatures as the reference.  ``forward``
is ONE C call each (``pio_encoder_fwd`` / ``pio_decoder_fwd``): the whole cross-attend + num_blocks x
num_self_attends_per_block stack is enqueued on the current HIP stream without returning to Python.
The fused paths around them (_assemble, _fused_decoder_query, _project_heads) are hooks into fused_io.py.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib as L
from . import fused_io as FIO
from . import probe as LP
from . import runtime as R
from .position_encoding import TrainablePositionEncoding
from .transformer_primitives import CrossAttention, SelfAttention, lecun_normal_, make_cross_attention_mask  # noqa: F401


class PerceiverEncoder(R.PackedOwner):
    """Cross-attend inputs into the latent array, then num_blocks x (weight-shared) self-attend block."""

    def __init__(self, num_input_channels: int, num_self_attends_per_block: int = 6, num_blocks: int = 8,
                 num_latents: int = 512, num_latent_channels: int = 1024, qk_channels: int = None,
                 v_channels: int = None, num_cross_attend_heads: int = 1, num_self_attend_heads: int = 8,
                 cross_attend_widening_factor: int = 1, self_attend_widening_factor: int = 1,
                 dropout_prob: float = 0.0, latent_pos_enc_init_scale: float = 0.02,
                 cross_attention_shape_for_attn: str = "kv", use_query_residual: bool = True):
        super().__init__()
        if num_latent_channels % num_self_attend_heads != 0:
            raise ValueError(f"num_z_channels ({num_latent_channels}) must be divisible by"
                             f" num_self_attend_heads ({num_self_attend_heads}).")
        if num_latent_channels % num_cross_attend_heads != 0:
            raise ValueError(f"num_z_channels ({num_latent_channels}) must be divisible by"
                             f" num_cross_attend_heads ({num_cross_attend_heads}).")
        self._num_blocks = num_blocks
        self.latent_pos_enc = TrainablePositionEncoding(index_dim=num_latents, num_channels=num_latent_channels,
                                                        init_scale=latent_pos_enc_init_scale)
        self.cross_attend = CrossAttention(q_in_channels=num_latent_channels, kv_in_channels=num_input_channels,
                                           dropout_prob=dropout_prob, num_heads=num_cross_attend_heads,
                                           widening_factor=cross_attend_widening_factor,
                                           shape_for_attn=cross_attention_shape_for_attn, qk_channels=qk_channels,
                                           v_channels=v_channels, use_query_residual=use_query_residual)
        self.self_attends = nn.ModuleList()
        for _ in range(num_self_attends_per_block):
            self.self_attends.append(SelfAttention(in_channels=num_latent_channels, num_heads=num_self_attend_heads,
                                                   dropout_prob=dropout_prob, qk_channels=qk_channels,
                                                   v_channels=v_channels,
                                                   widening_factor=self_attend_widening_factor))

    # Optional precision policy of the cross-attend alone (None = the ambient policy).  Its weights are applied ONCE to
    # the raw input features; the stack's 48 applications of shared weights are what single-sweep speed matters for.
    # On the ImageNet goldens "fp16x3f" here and in the decoder with the stack on "fp16sd" gives 3.2e-4 / 3.9e-4 (worst
    # of six) against 6.6e-4 / 7.3e-4 with "fp16sd" everywhere, for 1.1 ms of 16.4 (tools/sd_parity.py).
    cross_attend_policy = None

    def latents(self, inputs):
        return self.latent_pos_enc(batch_size=inputs.shape[0])

    def forward(self, inputs, latents, *, input_mask=None):
        """Reference signature (perceiver.py:98).  Extension: `inputs` may be a pair (features [B,M,C1], table [M,C2] or
        [1,M,C2]) standing for their channel-wise concatenation with the table broadcast over the batch -- the
        encoder then never sees a materialised [B,M,C1+C2] array (pio_encoder_call_t.inputs_tail)."""
        if R.cpu_plumbing(inputs[0] if isinstance(inputs, (tuple, list)) else inputs, "PerceiverEncoder.forward"):
            from . import cpu_plumbing as CP
            return CP.encoder(self, inputs, latents, input_mask)
        inputs_tail = None
        if isinstance(inputs, (tuple, list)):
            inputs, inputs_tail = inputs
            inputs_tail = R.as_f32_3d(inputs_tail if inputs_tail.dim() == 3 else inputs_tail[None])
        R.require_device(inputs, "PerceiverEncoder.forward")
        if self.training and any(m.dropout.p > 0 for m in self.self_attends):
            raise NotImplementedError("the HIP path is forward/inference only")
        lib = L.lib()
        x, z0 = R.as_f32_3d(inputs), R.as_f32_3d(latents)
        B, M, _ = x.shape
        N, D = z0.shape[1], z0.shape[2]
        dev = x.device
        # (cross_attend_policy: the cross-attend's own precision policy -- its weights are applied once, unlike the
        #  stack's; None = the ambient policy.  The descriptor carries its dtype / split flags into the library.)
        with R.precision(self.cross_attend_policy):
            cross = self.cross_attend._desc()
        Lyr = len(self.self_attends)
        # policy "fp16sd": one set of packed images per block (error-feedback rounding of the shared weights over the
        # block index, SelfAttention._desc_blocks) -- layers[b * Lyr + i]; otherwise the Lyr shared descriptors
        per_block = R.policy().feedback and self._num_blocks > 1 and Lyr > 0
        nset = self._num_blocks if per_block else 1
        descs = []
        for sa in self.self_attends:
            descs.append(sa._desc_blocks(self._num_blocks) if per_block else [sa._desc()])
        im, im_ptr = R.mask_u8(input_mask, (B, M), dev)
        out = torch.empty((B, N, D), dtype=torch.float32, device=dev)
        tail3 = R.tensor3(inputs_tail) if inputs_tail is not None else None
        # fp16 range guard of the LayerNorm-folded stack (runtime.range_check): the GEMMs that produce the folded residual
        # stream report a non-finite row statistic into a device word (pio_ln_fold_t.range_flag) -- whatever policy or
        # branch the fold is taken under, and only when it IS taken
        guard = R.range_check() and Lyr > 0 and not self._range_fallback
        flag = None
        if guard:
            flag = R.range_flag(dev, self)        # this encoder's own word (two models on a device do not share one)
            flag.zero_()
        # the descriptor array handed to the library: rebuilt only when a descriptor or the guard word changes (the
        # cached descriptor objects are replaced whenever their parameters / the policy change)
        def build_layers():
            layers = (L.SelfAttention * max(Lyr * nset, 1))()
            for i, ds in enumerate(descs):
                for b, d in enumerate(ds):
                    layers[b * Lyr + i] = d
            if guard:
                for i in range(Lyr * nset):
                    layers[i].fold.range_flag = flag.data_ptr()
            return layers, descs     # (descs: keeps the ids of the key alive)

        layers = self._packed.get((tuple(id(d) for ds in descs for d in ds), flag.data_ptr() if guard else 0), build_layers)

        # one pio_encoder_fwd call on the current stream's workspace (the un-folded repeat of the range guard is a PER-CALL
        # option, opts.ln_fold = 1: no process state changes around the call)
        rec = L.EncoderCall(C.pointer(cross), C.cast(layers, C.POINTER(L.SelfAttention)), Lyr, self._num_blocks,
                            int(per_block), C.pointer(R.tensor3(x)), C.pointer(tail3) if tail3 is not None else None,
                            C.pointer(R.tensor3(z0)), im_ptr, out.data_ptr(), L.CallOpts(1 if self._range_fallback else 0, 0))
        LP.expect("cross", *["stack"] * (Lyr * self._num_blocks))    # (one attention call per block, this order)
        LP.mark_range("cross")           # (range probe: the library marks "stack" behind the cross-attend itself)
        try:
            ws = R.workspace(dev, lib.pio_encoder_workspace_bytes(*L.arguments(
                "pio_encoder_workspace_bytes", (), dict(cross=cross, layers=layers, L=Lyr, B=B, M=M, N=N))))
            R.call(dev, "pio_encoder_fwd", C.byref(rec), ws.data_ptr(), ws.numel())
        finally:
            LP.mark_range("attention")
        return self._finish(out, flag, inputs, inputs_tail, latents, input_mask)

    _range_fallback = False   # True while the call is being repeated un-folded (the guard's fallback)

    def _finish(self, out, flag, inputs, inputs_tail, latents, input_mask):
        """Range guard, host side.  Inside PerceiverIO.forward the check is deferred to the end of the forward (no
        synchronisation between encoder and decoder); called on its own the encoder resolves it here; during stream
        capture nobody reads the word (runtime.last_range_flag)."""
        if self._range_fallback:
            # the un-folded repeat: nothing reports into a word here, so look at the result itself (rare path)
            if not bool(torch.isfinite(out).all()):
                raise L.PioError("PerceiverEncoder.forward: PIO_E_RANGE -- non-finite latents with and without the "
                                 "LayerNorm fold: activations exceed the fp16 operand range (65504); use the "
                                 "precision policy 'bf16x3' for this model")
        elif flag is not None and not R.capturing(out.device):
            pend = R.range_deferred()
            if pend is not None:
                pend.append(flag)
            elif int(flag.item()) != 0:
                full = inputs if inputs_tail is None else (inputs, inputs_tail)
                return self.forward_unfolded(full, latents, input_mask=input_mask)
        return R.forward_only(out, inputs, latents, *self.parameters())

    def forward_unfolded(self, inputs, latents, *, input_mask=None):
        """The same call with the LayerNorm fold off (fp32 residual stream): the range guard's fallback.  The switch is a
        per-call option of the library (pio_call_opts_t.ln_fold = 1), not a process-wide one."""
        self._range_fallback = True
        try:
            return self.forward(inputs, latents, input_mask=input_mask)
        finally:
            self._range_fallback = False


class PerceiverDecoder(R.PackedOwner):
    """Cross-attention decoder (queries attend to latents) with an optional final nn.Linear."""

    def __init__(self, query_channels: int, final_project_out_channels: int, num_latent_channels: int = 1024,
                 qk_channels: int = None, v_channels: int = None, use_query_residual: bool = False,
                 output_w_init: str = "lecun_normal", num_heads: int = 1, final_project: bool = True):
        super().__init__()
        self._output_num_channels = final_project_out_channels
        self._output_w_init = output_w_init
        self._use_query_residual = use_query_residual
        self._qk_channels = qk_channels
        self._v_channels = v_channels
        self._final_project = final_project
        self._num_heads = num_heads
        self.query_channels = query_channels
        self.decoding_cross_attn = CrossAttention(q_in_channels=query_channels, kv_in_channels=num_latent_channels,
                                                  dropout_prob=0.0, num_heads=self._num_heads, widening_factor=1,
                                                  shape_for_attn="kv", qk_channels=self._qk_channels,
                                                  v_channels=self._v_channels,
                                                  use_query_residual=self._use_query_residual)
        if self._final_project:
            self.final_layer = nn.Linear(query_channels, self._output_num_channels)
            if self._output_w_init == "lecun_normal":
                lecun_normal_(self.final_layer.weight)
            elif self._output_w_init == "zeros":
                nn.init.constant_(self.final_layer.weight, 0)
            else:
                raise ValueError(f"{self._output_w_init} not supported as output_w_init")
            nn.init.constant_(self.final_layer.bias, 0)

    def _final_desc(self):
        fl = self.final_layer
        return self._packed.get(R.param_key(fl.weight, fl.bias), lambda: (
            R.PackedLinear(fl.weight, fl.bias, 1, 1, R.policy().dtype, R.splits("final_layer")), None))

    def forward(self, query, latents, *, query_mask=None, q_cache=None):
        """Reference signature (perceiver.py:166) plus `q_cache`: a dict the CALLER keeps per query array whose content
        depends on parameters and constants only (MultiModalPerceiver's per-chunk queries).  The decoder leaves the
        normalised + projected queries there on the first call and skips LayerNorm_q / proj_q afterwards
        (pio_decoder_call_t.q16_hi); it revalidates the entry against its own parameters and the precision policy.  Only
        without the query residual.

        Extension (as PerceiverEncoder.forward's): `query` may be a pair (features [B,Q,C1], table [Q,C2] or [1,Q,C2])
        standing for their channel-wise concatenation -- dense decoders whose queries are the network's preprocessed
        input (FlowQuery): LayerNorm_q reads the two arrays, nothing is concatenated (pio_decoder_call_t.query_tail).  Only
        without the query residual."""
        query_tail = None
        if isinstance(query, (tuple, list)):
            query, query_tail = query
            if self._use_query_residual:
                raise ValueError("a (features, table) query needs use_query_residual=False")
        if R.cpu_plumbing(query, "PerceiverDecoder.forward"):
            from . import cpu_plumbing as CP
            if query_tail is not None:
                t = query_tail if query_tail.dim() == 3 else query_tail[None]
                query = torch.cat([query, t.expand(query.shape[0], -1, -1)], dim=-1)
            return CP.decoder(self, query, latents, query_mask)
        R.require_device(query, "PerceiverDecoder.forward")
        lib = L.lib()
        q, z = R.as_f32_3d(query), R.as_f32_3d(latents)
        if query_tail is not None:
            query_tail = R.as_f32_3d(query_tail if query_tail.dim() == 3 else query_tail[None])
        B, Q, _ = q.shape
        N = z.shape[1]
        dev = q.device
        cross = self.decoding_cross_attn._desc()
        fin = self._final_desc() if self._final_project else None
        out_ch = self._output_num_channels if self._final_project else self.query_channels
        qm, qm_ptr = R.mask_u8(query_mask, (B, Q), dev)
        out = torch.empty((B, Q, out_ch), dtype=torch.float32, device=dev)
        fin_ptr = C.pointer(fin.desc) if fin is not None else None
        ws = R.workspace(dev, lib.pio_decoder_workspace_bytes(*L.arguments(
            "pio_decoder_workspace_bytes", (), dict(cross=cross, final_layer=fin_ptr, B=B, Q=Q, N=N))))
        qhi = qlo = None
        valid = 0
        if q_cache is not None and not self._use_query_residual and query_tail is None:
            ca = self.decoding_cross_attn
            Bq = 1 if (q.stride(0) == 0 and B > 1) else B
            try:
                qver = q._version
            except RuntimeError:                 # (inference tensors carry no version counter)
                qver = -1
            key = (R.param_key(ca.layer_norm_q.weight, ca.layer_norm_q.bias, ca.attention.proj_q.weight,
                               ca.attention.proj_q.bias), Bq, Q, q.data_ptr(), qver, int(cross.attn.act_split))
            fresh = q_cache.get("key") != key
            # (during stream capture a cache is only READ: nothing is allocated or validated inside a graph)
            if not (R.capturing(dev) and (fresh or not q_cache.get("valid"))):
                if fresh:
                    nb = lib.pio_decoder_qcache_bytes(cross, Bq, Q)
                    with torch.inference_mode(False):
                        q_cache["hi"] = torch.empty(nb, dtype=torch.uint8, device=dev)
                        q_cache["lo"] = torch.empty(nb, dtype=torch.uint8, device=dev) if cross.attn.act_split else None
                    q_cache["key"], q_cache["valid"] = key, False
                qhi = q_cache["hi"].data_ptr()
                qlo = q_cache["lo"].data_ptr() if q_cache["lo"] is not None else None
                valid = 1 if q_cache["valid"] else 0
        rec = L.DecoderCall(C.pointer(cross), fin_ptr, out_ch, C.pointer(R.tensor3(q)),
                            C.pointer(R.tensor3(query_tail)) if query_tail is not None else None, C.pointer(R.tensor3(z)),
                            qm_ptr, out.data_ptr(), qhi, qlo, valid)
        LP.expect("decoder")
        LP.mark_range("decoder")
        try:
            R.call(dev, "pio_decoder_fwd", C.byref(rec), ws.data_ptr(), ws.numel())
        finally:
            LP.mark_range("attention")
        if qhi is not None:
            q_cache["valid"] = True
        return R.forward_only(out, query, latents, *self.parameters())


# ==================================================================================================
# Orchestration around the hot path (reference perceiver.py:183-499): plain PyTorch plumbing that keeps the
# PerceiverIO constructor surface and state_dict layout.  Modalities are always handled in sorted-key order.
# ==================================================================================================
def restructure(modality_sizes, inputs: torch.Tensor):
    """Split a [B, N, C] array back into per-modality views, in sorted modality order (reference :370-387)."""
    out, start = {}, 0
    for name in sorted(modality_sizes.keys()):
        n = modality_sizes[name]
        out[name] = inputs[:, start:start + n]
        start += n
    return out


def _as_module_dict(x):
    if type(x) is dict:
        return nn.ModuleDict(x)
    if isinstance(x, nn.Module) and not isinstance(x, nn.ModuleDict):
        return nn.ModuleDict({"__default": x})
    return x


class MultimodalPreprocessor(nn.Module):
    """Runs each modality's preprocessor, pads all of them to a common channel count with learned padding
    embeddings, optionally replaces tokens by a learned mask token, and concatenates along the index axis
    (reference :390-499)."""

    def __init__(self, input_preprocessors=None, mask_probs=None, min_padding_size: int = 2, input_channels=None):
        super().__init__()
        self._preprocessors = input_preprocessors
        self._min_padding_size = min_padding_size
        self._mask_probs = mask_probs
        if input_preprocessors is not None:
            assert input_channels is None, "input_channels and modalities are mutually exclusive"
            input_channels = {m: p.n_output_channels() for m, p in input_preprocessors.items()}
        else:
            assert input_channels is not None, "if no preprocessors, input_channels must be specified"
        self._common_channels = max(input_channels.values()) + min_padding_size
        if mask_probs is not None:
            self.mask_tokens = nn.ModuleDict({
                m: TrainablePositionEncoding(index_dim=1, num_channels=self._common_channels, init_scale=0.02)
                for m in self._preprocessors.keys()})
        self.padding_embeddings = None
        ragged = max(input_channels.values()) != min(input_channels.values())
        if ragged or min_padding_size != 0:
            self.padding_embeddings = nn.ModuleDict({
                m: TrainablePositionEncoding(index_dim=1, num_channels=self._common_channels - p.n_output_channels(),
                                             init_scale=0.02)
                for m, p in self._preprocessors.items()})

    def n_output_channels(self):
        return self._common_channels

    # One HIP launch (pio_assemble_tokens) instead of the chain of copies below, when every modality is a pure move: see
    # _assemble.  False, and every input or configuration _assemble declines, runs the chain exactly as before.
    fused_assembly = True

    def _assemble(self, inputs, pos):
        return FIO.assemble_tokens(self, inputs, pos)

    def _single_embedding(self, inputs):
        """(x, sizes, without_pos) of forward() for ONE EmbeddingPreprocessor without padding embeddings or mask
        probabilities whose fused path (pio_embed_tokens) takes these inputs: its output IS the encoder input, so it is
        returned as it stands instead of going through the one-element torch.cat below (a plain copy of the largest
        activation).  Same values.  None -- and the chain below, unchanged -- for everything else."""
        from .io_processors import EmbeddingPreprocessor
        if (self._preprocessors is None or len(self._preprocessors) != 1 or self.padding_embeddings is not None
                or self._mask_probs is not None):
            return None
        (m, prep), = self._preprocessors.items()
        if not isinstance(prep, EmbeddingPreprocessor) or m not in inputs:
            return None
        fused = prep._fused(inputs[m])
        if fused is None:
            return None
        return fused[0], {m: fused[0].shape[1]}, {m: fused[1]}

    def forward(self, inputs, *, pos=None):
        fused = self._assemble(inputs, pos)
        if fused is not None:
            return fused
        fused = self._single_embedding(inputs)
        if fused is not None:
            return fused
        if self._preprocessors is None:
            outputs, without_pos = inputs, inputs
        else:
            outputs, without_pos = {}, {}
            for m, prep in self._preprocessors.items():
                outputs[m], without_pos[m] = prep(inputs[m], pos=pos)
        if self.padding_embeddings is not None:
            padded = {}
            for m, x in outputs.items():
                pad = torch.broadcast_to(self.padding_embeddings[m](x.shape[0]),
                                         [x.shape[0], x.shape[1], self._common_channels - x.shape[2]])
                padded[m] = torch.cat([x, pad], dim=2)
            outputs = padded
        sizes = {m: x.shape[1] for m, x in outputs.items()}
        if self._mask_probs is not None:
            masked = {}
            for m, x in outputs.items():
                token = self.mask_tokens[m](x.shape[0])
                p = self._mask_probs[m]
                if p <= 0.0:
                    masked[m] = x                              # bernoulli(0) is all zeros: (1-0)*x + 0*token
                elif p >= 1.0:
                    masked[m] = torch.broadcast_to(token, x.shape) + 0 * x
                else:
                    mask = torch.bernoulli(torch.full([x.shape[0], x.shape[1]], fill_value=float(p))).to(x.device)
                    mask = mask[:, :, None]
                    masked[m] = (1 - mask) * x + mask * token
            outputs = masked
        ordered = [outputs[m] for m in sorted(outputs.keys())]
        return torch.cat(ordered, dim=1), sizes, without_pos


class PerceiverIO(nn.Module):
    """preprocess -> PerceiverEncoder -> decoder queries -> PerceiverDecoder -> postprocess (reference :183-367).
    The encoder / decoder are the HIP-backed modules above; everything else here is batch-invariant table building
    and tensor bookkeeping in stock torch."""

    def __init__(self, num_blocks: int = 8, num_self_attends_per_block: int = 6, num_latents: int = 512,
                 num_latent_channels: int = 1024, final_project: bool = True, final_project_out_channels: int = None,
                 perceiver_encoder_kwargs=None, perceiver_decoder_kwargs=None, input_preprocessors=None,
                 output_postprocessors=None, output_queries=None, output_query_padding_channels: int = 0,
                 input_padding_channels: int = 0, input_channels=None, input_mask_probs: dict = None):
        super().__init__()
        perceiver_encoder_kwargs = perceiver_encoder_kwargs or {}
        perceiver_decoder_kwargs = perceiver_decoder_kwargs or {}
        if final_project_out_channels is None:
            final_project_out_channels = num_latent_channels
        if type(input_channels) is int:
            input_channels = {"__default": input_channels}
        self._multi_preprocessor = MultimodalPreprocessor(input_preprocessors=_as_module_dict(input_preprocessors),
                                                          mask_probs=input_mask_probs,
                                                          min_padding_size=input_padding_channels,
                                                          input_channels=input_channels)
        self._output_postprocessors = _as_module_dict(output_postprocessors)
        self._output_queries = _as_module_dict(output_queries)
        query_channels = max(q.n_query_channels() for q in self._output_queries.values()) + \
            output_query_padding_channels
        self.query_channels = query_channels
        # every query is padded to the widest one with a learned embedding (width 0 for a single modality:
        # the (1, 0) parameter still exists in the state_dict, as in the reference)
        self.padding_embeddings = nn.ModuleDict({
            m: TrainablePositionEncoding(index_dim=1, num_channels=query_channels - q.n_query_channels(),
                                         init_scale=0.02)
            for m, q in self._output_queries.items()})
        self._encoder = PerceiverEncoder(num_input_channels=self._multi_preprocessor.n_output_channels(),
                                         num_blocks=num_blocks,
                                         num_self_attends_per_block=num_self_attends_per_block,
                                         num_latents=num_latents, num_latent_channels=num_latent_channels,
                                         **perceiver_encoder_kwargs)
        self._decoder = PerceiverDecoder(query_channels=query_channels, final_project=final_project,
                                         final_project_out_channels=final_project_out_channels,
                                         num_latent_channels=num_latent_channels, **perceiver_decoder_kwargs)
        # Opt-in (None = decode every query row, as the reference does): a slice of query rows to decode.  Decoder rows
        # are independent, so a postprocessor that keeps only some rows (ClassificationPostprocessor: row 0,
        # postprocessors.py:180-187) gets the same values from the rows alone -- ClassificationPerceiver(
        # decode_row0_only=True) sets slice(0, 1) and skips 999 / 1000 of the decoder's work.
        self.decoder_query_rows = None
        # Optional precision policies of the two halves (None = the ambient policy): dense-output models are far more
        # sensitive to operand rounding in the DECODER (no averaging behind it) than in the encoder -- the full-size
        # optical-flow model meets 1e-3 with "fp16x2w" everywhere except the decoder (tools/policy_mix.py).
        self.encoder_policy = None
        self.decoder_policy = None

    # Fused preprocessing hand-off (on by default): a single image modality whose network input is [conv features |
    # batch-invariant Fourier / learned position table] reaches the encoder as those two arrays
    # (ImagePreprocessor.forward_split -> PerceiverEncoder.forward((features, table), ...)).  Applies when nothing else
    # needs the concatenated array: no channel padding, no token masking, queries that do not read the inputs.
    split_encoder_input = True

    def _split_input(self, inputs, pos):
        mp = self._multi_preprocessor
        if (pos is not None or mp._preprocessors is None or list(mp._preprocessors.keys()) != ["__default"]
                or mp.padding_embeddings is not None or mp._mask_probs is not None):
            return None
        prep = mp._preprocessors["__default"]
        if not hasattr(prep, "forward_split") or not inputs["__default"].is_cuda:
            return None
        if any(getattr(q, "_concat_preprocessed_input", False) for q in self._output_queries.values()):
            # a query that reads the preprocessed inputs needs the concatenated array -- unless the inputs themselves ARE
            # the query rows (FlowQuery: no position encoding of its own) and the decoder can take them as two arrays too
            if not self._identity_query():
                return None
        return prep.forward_split(inputs["__default"])

    def _identity_query(self):
        """True when the single output query returns the preprocessed inputs unchanged (BasicQuery with
        PosEncodingType.NONE: output_queries.py) and the decoder neither adds the query back nor pads / sub-samples it:
        the decoder then takes the encoder's (features, table) pair as its query (PerceiverDecoder.forward)."""
        qs = list(self._output_queries.values())
        if len(qs) != 1 or list(self._output_queries.keys()) != ["__default"]:
            return False
        q = qs[0]
        return (getattr(q, "_position_encoding", 0) is None and getattr(q, "_concat_preprocessed_input", False)
                and not self._decoder._use_query_residual and self.decoder_query_rows is None
                and q.n_query_channels() == self.query_channels)

    # One HIP launch (pio_build_queries) instead of the chain of torch ops in decoder_query, for a multi-modality model whose
    # queries depend on parameters and constants only: see _fused_decoder_query.  False, and every configuration it
    # declines, runs the chain exactly as before.
    fused_queries = True

    def _fused_decoder_query(self, inputs, subsampled_points):
        return FIO.build_queries(self, inputs, subsampled_points)

    # One HIP launch (pio_project_heads) instead of one runtime.hip_linear chain per narrow output head (row slice copy,
    # 16-bit cast, GEMM, result copied into place), for a multi-modality model: see _project_heads.  fp32 products of the
    # unrounded decoder output.  False, and every configuration it declines, runs the chain exactly as before.
    fused_heads = True

    def _heads_eligible(self, k: int) -> bool:
        return FIO.heads_eligible(self, k)

    def _heads_accept(self, outputs) -> bool:
        return FIO.heads_accept(self, outputs)

    def _project_heads(self, outputs, query_sizes, into=None):
        return FIO.project_heads(self, outputs, query_sizes, into)

    def decoder_query(self, inputs, modality_sizes, inputs_without_pos=None, subsampled_points=None, modalities=None):
        """`modalities` (None = all of them, which changes nothing): the names of the output queries to build -- those
        segments only, in sorted order, by the chain of torch ops (never the fused launch, which builds every segment), with
        the same bits for their rows (MultiModalPerceiver.classify: the label row alone)."""
        per_mod = restructure(modality_sizes, inputs)
        subsampled_points = subsampled_points or {}
        if modalities is not None:
            unknown = [m for m in modalities if m not in self._output_queries]
            if unknown or len(modalities) < 1:
                raise ValueError(f"decoder_query: modalities {list(modalities)!r} must name some of "
                                 f"{sorted(self._output_queries.keys())}")
        else:
            fused = self._fused_decoder_query(inputs, subsampled_points)
            if fused is not None:
                return fused
        any_input = next(iter(per_mod.values()))
        queries = {}
        for m, make_query in self._output_queries.items():
            if modalities is not None and m not in modalities:
                continue
            wo = inputs_without_pos.get(m) if inputs_without_pos is not None else None
            src = per_mod.get(m)
            if src is None:      # a query without a matching input still needs batch size / device
                src = torch.zeros((any_input.shape[0], 0), device=any_input.device)
            q = make_query(src, inputs_without_pos=wo, subsampled_points=subsampled_points.get(m))
            q = q.reshape(q.shape[0], -1, q.shape[-1])
            pad = torch.broadcast_to(self.padding_embeddings[m](q.shape[0]),
                                     [q.shape[0], q.shape[1], self.query_channels - q.shape[2]])
            queries[m] = torch.cat([q, pad], dim=2) if pad.shape[2] > 0 else q
        sizes = {m: q.shape[1] for m, q in queries.items()}
        if len(queries) == 1:
            return next(iter(queries.values())), sizes        # keeps a broadcast table a stride-0 view
        return torch.cat([queries[m] for m in sorted(queries.keys())], dim=1), sizes

    def forward(self, inputs, *, subsampled_output_points=None, pos=None, input_mask=None, query_mask=None,
                query_shard=None, query_index=None, postprocess=None):
        """Reference signature (perceiver.py:287-288) plus `query_shard=(rank, world)`: decode only this rank's slice
        of the query rows and all-gather the result along the query axis (dist.decode_query_sharded) -- the
        multi-GPU form for batches smaller than the world (optical flow).  Needs an initialised process group.

        `query_index` (None = every row): an int64 index tensor [P] (the same rows for every sample) or [B, P] (each
        sample its own) of the query rows to decode, for a single output modality -- see _gather_query_rows; the caller
        validates the indices.  `postprocess` (None = the output postprocessors): a callable that takes the decoder output
        [B, rows, C] in their place, under the decoder's precision policy (LanguagePerceiver.predict).

        The fp16 range guard of the folded latent stack (runtime.range_check) is resolved HERE, once, after everything
        has been enqueued: the encoder's kernels report into a device word, nothing synchronises between encoder and
        decoder, and the word is read where the caller is about to consume the outputs.  A set word repeats the
        forward with the fold off (PIO_E_RANGE if that does not help)."""
        kw = dict(subsampled_output_points=subsampled_output_points, pos=pos, input_mask=input_mask,
                  query_mask=query_mask, query_shard=query_shard, query_index=query_index, postprocess=postprocess)
        with R.defer_range_checks() as guard:
            outputs = self._forward(inputs, **kw)
        if guard.pending and any(int(f.item()) != 0 for f in guard.pending):
            self._encoder._range_fallback = True       # (-> pio_call_opts_t.ln_fold = 1 on the encoder's call)
            try:
                outputs = self._forward(inputs, **kw)
            finally:
                self._encoder._range_fallback = False
        return outputs

    @staticmethod
    def _gather_query_rows(query, query_mask, index):
        """(query, query_mask) restricted to the rows `index` names: int64 [P] -- the same rows of every sample; a
        batch-invariant (stride-0) query stays ONE [1, P, C] array behind a stride-0 batch axis, so the decoder still
        normalises and projects it once -- or [B, P], each sample its own rows.  Decoder rows are independent and the mask
        is gathered with them: a gathered row sees exactly what it sees in a full forward."""
        b = query.shape[0]
        if index.dim() == 1:
            if b > 1 and query.stride(0) == 0:
                query = torch.broadcast_to(query[:1].index_select(1, index), (b, index.shape[0], query.shape[2]))
            else:
                query = query.index_select(1, index)
            if query_mask is not None:
                query_mask = query_mask.index_select(1, index.to(query_mask.device))
        else:
            if tuple(index.shape[:1]) != (b,) or index.dim() != 2:
                raise ValueError(f"query_index: expected [P] or [{b}, P], got {tuple(index.shape)}")
            query = torch.gather(query, 1, index[:, :, None].expand(-1, -1, query.shape[2]))
            if query_mask is not None:
                query_mask = torch.gather(query_mask, 1, index.to(query_mask.device))
        return query, query_mask

    def _forward(self, inputs, *, subsampled_output_points=None, pos=None, input_mask=None, query_mask=None,
                 query_shard=None, query_index=None, postprocess=None):
        if type(inputs) is torch.Tensor:
            inputs = {"__default": inputs}
        split = self._split_input(inputs, pos) if self.split_encoder_input else None
        if split is not None and split[0] == "full":
            # (the preprocessor could not hand over two arrays: its ordinary output, computed once)
            x = split[1]
            sizes, without_pos = {"__default": x.shape[1]}, {"__default": split[2]}
            latents0 = self._encoder.latents(x)
            query, query_sizes = self.decoder_query(x, sizes, without_pos, subsampled_points=subsampled_output_points)
            with R.precision(self.encoder_policy):
                latents = self._encoder(x, latents0, input_mask=input_mask)
        elif split is not None:
            # the encoder input as (features, batch-invariant position table): never concatenated / replicated in HBM
            feats, table = split[1], split[2]
            sizes, without_pos = {"__default": feats.shape[1]}, {"__default": feats}
            latents0 = self._encoder.latents(feats)
            if self._identity_query() and subsampled_output_points is None and query_shard is None:
                query, query_sizes = (feats, table), dict(sizes)      # the inputs are the query rows: two arrays again
            else:
                if self._identity_query():
                    x = torch.cat([feats, torch.broadcast_to(table[None], (feats.shape[0],) + tuple(table.shape))], -1)
                    query, query_sizes = self.decoder_query(x, sizes, without_pos,
                                                            subsampled_points=subsampled_output_points)
                else:
                    query, query_sizes = self.decoder_query(feats, sizes, without_pos,
                                                            subsampled_points=subsampled_output_points)
            with R.precision(self.encoder_policy):
                latents = self._encoder((feats, table), latents0, input_mask=input_mask)
        else:
            x, sizes, without_pos = self._multi_preprocessor(inputs, pos=pos)
            latents0 = self._encoder.latents(x)
            query, query_sizes = self.decoder_query(x, sizes, without_pos, subsampled_points=subsampled_output_points)
            with R.precision(self.encoder_policy):
                latents = self._encoder(x, latents0, input_mask=input_mask)
        if self.decoder_query_rows is not None:
            query = query[:, self.decoder_query_rows]
            if query_mask is not None:
                query_mask = query_mask[:, self.decoder_query_rows]
            assert len(query_sizes) == 1, "decoder_query_rows is defined for a single output modality"
            query_sizes = {m: query.shape[1] for m in query_sizes}
        if query_index is not None:
            assert len(query_sizes) == 1 and not isinstance(query, (tuple, list)), \
                "query_index is defined for a single output modality with one query array"
            query, query_mask = self._gather_query_rows(query, query_mask, query_index)
            query_sizes = {m: query.shape[1] for m in query_sizes}
        with R.precision(self.decoder_policy):
            if query_shard is not None:
                from .dist import decode_query_sharded
                outputs = decode_query_sharded(self._decoder, query, latents, query_mask, *query_shard)
            else:
                outputs = self._decoder(query, latents, query_mask=query_mask)
        if postprocess is not None:
            with R.precision(self.decoder_policy):
                return postprocess(outputs)
        if self._output_postprocessors:
            with R.precision(self.decoder_policy):       # (the heads behind the decoder belong to its half)
                heads = self._project_heads(outputs, query_sizes)
                if heads is None:
                    per_mod = restructure(query_sizes, outputs)
                    heads = {m: post(per_mod[m], pos=None, modality_sizes=None)
                             for m, post in self._output_postprocessors.items()}
            outputs = heads
        if type(outputs) is not torch.Tensor and list(outputs.keys()) == ["__default"]:
            outputs = outputs["__default"]
        return outputs
