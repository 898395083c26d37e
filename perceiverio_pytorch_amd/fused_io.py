"""The fused input / output paths: one HIP launch each in place of a chain of torch ops of the I/O plumbing.  Every function
takes the module it serves first, decides whether the launch stands for the chain exactly, and returns None when it declines
-- its caller (a one-line hook of the module: _assemble, _fused, _project_heads, ...) then runs the chain, which stays in the
model files with the switches.  The decline rules are the specification: a wrong accept gives silently wrong tokens."""
import itertools
import math

import torch

from . import _lib as L, probe as LP, runtime as R
from . import io_processors as IO, output_queries as OQ, perceiver as PV, position_encoding as PE


def gate(on, *tensors, dtypes=(torch.float32,)) -> bool:
    """In front of every path: the switch is on, the backend is hip, `tensors` are CUDA tensors of `dtypes` (None: any)."""
    if not on or R.get_backend() != "hip":
        return False
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or not (dtypes is None or t.dtype in dtypes):
            return False
    return True


def rows(t, *, min_stride=False, stride4=False, aligned=False):
    """`t` as a kernel reads its rows: `t` itself when the last stride is 1 and what the entry point asks for beyond that
    holds (min_stride: row stride >= row length; stride4: row stride a multiple of 4 elements; aligned: 16-byte aligned
    pointer), a detached contiguous copy otherwise.  Only pointers and strides are taken from the result."""
    ok = t.stride(-1) == 1 and not ((min_stride and t.stride(-2) < t.shape[-1]) or (stride4 and t.stride(-2) % 4)
                                    or (aligned and t.data_ptr() % 16))
    return t if ok else t.detach().contiguous()


def param_row(p, width, dev):
    """A learned (1, width) fp32 parameter on `dev` (padding embedding, mask token) as a kernel reads it: `p` itself, or a
    detached contiguous copy; None for width 0 (the segment carries no pointer), False when `p` is anything else (decline)."""
    if tuple(p.shape) != (1, width) or p.dtype != torch.float32 or p.device != dev:
        return False
    return None if width < 1 else p if p.is_contiguous() else p.detach().contiguous()


def place(segs):
    """{name: segment} -> (ctypes array of the segments in sorted-name order with row0 assigned along it, total rows); the
    array is None when the total reaches 2^31 (row indices are int32): decline."""
    arr, row0 = (type(next(iter(segs.values()))) * len(segs))(), 0
    for i, m in enumerate(sorted(segs)):
        segs[m].row0 = row0
        arr[i] = segs[m]
        row0 += segs[m].M
    return (arr if row0 < 2 ** 31 else None), row0


def embed_tokens(prep, inputs):
    """(embed(inputs) + pos, embed(inputs) or None) from ONE pio_embed_tokens call, or None.  Taken under the hip
    backend for a 2-D CUDA int32 / int64 id tensor with unit stride along t whose length equals the position table's,
    fp32 embedding and position tables on that device, no padding_idx and no max_norm.  y is one fresh [B, T, C]
    allocation and equals the chain's bit for bit (one rounded fp32 add of the same operands).  Unlike ATen, which
    raises a device-side assert, an id outside [0, vocab_size) gives a NaN row in both outputs and sets the word of
    bad_ids_flag(device)."""
    w, p = prep.embed.weight, prep.input_pos_encoding.pos_embs
    if not gate(prep.fused_embedding, inputs, dtypes=(torch.int32, torch.int64)) or inputs.dim() != 2:
        return None
    dev, (b, t) = inputs.device, inputs.shape
    if (b < 1 or t < 1 or (t > 1 and inputs.stride(1) != 1) or t != p.shape[0]
            or (b > 1 and inputs.stride(0) < t)):
        return None
    if (w.dtype != torch.float32 or p.dtype != torch.float32 or w.device != dev or p.device != dev
            or p.dim() != 2 or p.shape[1] != w.shape[1] or w.shape[1] < 1
            or prep.embed.padding_idx is not None or prep.embed.max_norm is not None):
        return None
    # (min_stride: the entry point refuses tables whose rows overlap -- an expanded parameter -- instead of reading them)
    table, ptab = rows(w, min_stride=True), rows(p, min_stride=True)
    v, c = table.shape
    y = torch.empty((b, t, c), dtype=torch.float32, device=dev)
    tokens = torch.empty((b, t, c), dtype=torch.float32, device=dev) if prep.need_tokens else None
    flag = prep.bad_ids_flag(dev).zero_()
    R.call_named(dev, "pio_embed_tokens", ids=inputs.data_ptr(), id_bytes=inputs.element_size(), ids_sb=inputs.stride(0),
                 table=table.data_ptr(), ldt=table.stride(0), V=v, pos=ptab.data_ptr(), ldp=ptab.stride(0), y=y.data_ptr(),
                 y_sb=t * c, ldy=c, tokens=None if tokens is None else tokens.data_ptr(), tok_sb=t * c, ldtok=c,
                 bad_ids=flag.data_ptr(), B=b, T=t, C=c)
    y = R.forward_only(y, w, p)
    return y, (None if tokens is None else R.forward_only(tokens, w, p))


def flow_patch_tokens(prep, pair):
    """The optical-flow front end on a RAW frame pair [N, 2, C, H, W] by ONE HIP kernel (pio_flow_patch_tokens):
    patches_for_flow (3x3 zero-padded neighbourhoods), the channels-last copy, space_to_depth (the two frames side by
    side: 18 C channels) and the Linear of conv_after_patching, without any of their temporaries.  Returns the feature
    array [N, H*W, out] -- without the Linear the 18 C patch channels, as a view of rows padded to a multiple of 4
    -- or None when this configuration or input is not the covered one (the caller's ordinary path then runs: it
    expects the PATCHED frames [N, 2, 9 C, H, W])."""
    if (prep._prep_type != "patches" or prep._spatial_downsample != 1 or prep._temporal_downsample != 2
            or not gate(True, pair) or pair.dim() != 5 or pair.shape[1] != 2):
        return None
    n, _, c, h, w = pair.shape
    if not 1 <= c <= 4 or [h, w] != list(prep.index_dims):
        return None
    if prep._conv_after_patching:
        lin = prep._conv_after_patch_layer
        out = lin.out_features
        if lin.in_features != 18 * c or out % 4 or out > 128 or lin.weight.dtype != torch.float32:
            return None
        wt, bias = lin.weight.detach().contiguous(), lin.bias.detach().contiguous()    # (the entry takes no row stride)
        deps = (pair, lin.weight, lin.bias)
    else:
        out = 18 * c
        if prep._patch_channels != out:
            return None
        wt, bias, deps = None, None, (pair,)
    pair = rows(pair) if w > 1 else pair        # (one pixel per image row: its stride is never used)
    ldy = (out + 3) // 4 * 4
    y = torch.empty((n, h * w, ldy), dtype=torch.float32, device=pair.device)
    R.call_named(pair.device, "pio_flow_patch_tokens", frame0=pair[:, 0].data_ptr(), frame1=pair[:, 1].data_ptr(),
                 sn0=pair.stride(0), sc0=pair.stride(2), sy0=pair.stride(3), sn1=pair.stride(0), sc1=pair.stride(2),
                 sy1=pair.stride(3), w=None if wt is None else wt.data_ptr(), bias=None if bias is None else bias.data_ptr(),
                 y=y.data_ptr(), ldy=ldy, N=n, C=c, H=h, W=w, out=out)
    return R.forward_only(y if ldy == out else y[:, :, :out], *deps)


# No size of the two classifier front ends below is routed back to the chain: a measurement (profiles/classify_front_ends.json,
# tools/prep_bench.py --classify-front, B = 1 / 8 / 32 at 224 x 224) found no crossover -- the 1x1 hand-off 27 / 86 / 300 us
# against 100 / 3370 / 14350 us, the pixel hand-off 30 / 162 / 606 us against 30 / 221 / 940 us (equal at one sample, inside the
# repeats' range), the whole forward never slower.  Smaller images and s > 1 were not timed.
def conv1x1_tokens(prep, x):
    """The "conv1x1" image front end on an image batch [B, C, H, W] by ONE HIP kernel (pio_conv1x1_tokens): the strided 1x1
    convolution and the channels-last copy behind it, without the [B, N, OH, OW] array between them.  Returns the features
    [B, OH*OW, N] (one fresh allocation) or None: the switch off, the torch backend, anything but a 4-D CUDA fp32 tensor, a
    preprocessor that is not "conv1x1", a conv with groups, dilation, padding, a non-square stride, a kernel other than 1x1
    or a padding mode other than "zeros", a weight or bias that is not fp32 on the input's device, C outside [1, 4], a
    stride outside [1, 8] or one that does not divide H and W, N outside [4, PIO_CONV1X1_MAX_N] or no multiple of 4, an
    empty axis, 2^31 rows or more, OH*OW != prod(index_dims).  The image is read in place through its own strides."""
    if getattr(prep, "_prep_type", None) != "conv1x1" or not gate(prep.fused_conv1x1, x) or x.dim() != 4:
        return None
    conv = prep.convnet_1x1
    wt, bias = conv.weight, conv.bias
    if (conv.groups != 1 or tuple(conv.kernel_size) != (1, 1) or tuple(conv.dilation) != (1, 1)
            or isinstance(conv.padding, str) or tuple(conv.padding) != (0, 0) or conv.padding_mode != "zeros"
            or conv.stride[0] != conv.stride[1]):
        return None
    dev, (b, c, h, w), s = x.device, x.shape, int(conv.stride[0])
    if (wt.dtype != torch.float32 or wt.device != dev or tuple(wt.shape[1:]) != (c, 1, 1)
            or (bias is not None and (bias.dtype != torch.float32 or bias.device != dev))):
        return None
    n = wt.shape[0]
    if (not 1 <= c <= 4 or not 1 <= s <= 8 or min(b, h, w) < 1 or h % s or w % s or n % 4
            or not 4 <= n <= L.PIO_CONV1X1_MAX_N or x.data_ptr() % 4):
        return None
    m = (h // s) * (w // s)
    if m != int(math.prod(prep.index_dims)) or b * m >= 2 ** 31:
        return None
    w2 = rows(wt.reshape(n, c), min_stride=True)
    bias_c = None if bias is None else bias.detach().contiguous()
    y = torch.empty((b, m, n), dtype=torch.float32, device=dev)
    R.call_named(dev, "pio_conv1x1_tokens", x=x.data_ptr(), sb=x.stride(0), sc=x.stride(1), sy=x.stride(2), sx=x.stride(3),
                 w=w2.data_ptr(), ldw=w2.stride(0), bias=None if bias_c is None else bias_c.data_ptr(), y=y.data_ptr(), ldy=n,
                 sYb=m * n, B=b, C=c, H=h, W=w, s=s, N=n)
    return R.forward_only(y, x, wt, bias)


def projected_pos_table(prep, feats):
    """The position half [M, C2] of a preprocessor whose position encoding is a PositionEncodingProjector over a learned
    table or a Fourier grid table, for features `feats` [B, M, C1] -- ONE fp32 F.linear of the [M, .] base table instead of
    the chain's BLAS call over B identical copies on every forward -- or None.  It depends on parameters only: built once
    (outside inference mode, without autograd) and kept in the preprocessor's PackedCache under the parameters' key and the
    device; .to(), load_state_dict and invalidate_packed_weights drop it.  Taken under the hip backend for CUDA fp32
    features with the preprocessor's switch (fused_conv1x1) on, concatenated positions, no extra position MLPs and fp32
    base table, weight and bias on the features' device."""
    enc = prep._positional_encoding
    if (not isinstance(prep, R.PackedOwner) or not gate(getattr(prep, "fused_conv1x1", False), feats) or feats.dim() != 3
            or type(enc) is not PE.PositionEncodingProjector or prep._concat_or_add_pos != "concat"
            or prep._n_extra_pos_mlp > 0):
        return None
    base, lin, dev = enc._base_position_encoding, enc._projector, feats.device
    if type(base) is PE.TrainablePositionEncoding:
        src = base.pos_embs
    elif type(base) is PE.FourierPositionEncoding:
        src = base(None, None, device=dev)          # (the grid table, built once per device by the encoding itself)
    else:
        return None
    wt, bias = lin.weight, lin.bias
    if (src.dim() != 2 or src.shape[0] != feats.shape[1] or src.shape[1] != wt.shape[1]
            or any(t is not None and (t.dtype != torch.float32 or t.device != dev) for t in (src, wt, bias))):
        return None

    def build():
        with torch.inference_mode(False), torch.no_grad():
            table = torch.nn.functional.linear(src.detach(), wt.detach(), None if bias is None else bias.detach())
            return table.contiguous(), None
    table = prep._packed.get((R.param_key(src, wt, bias), str(dev)), build, slot="pos_table")
    return R.forward_only(table, src, wt, bias)


class _OneImage:
    """What assemble_tokens reads of a MultimodalPreprocessor, for ONE ImagePreprocessor: no padding, no masking, the
    common width the preprocessor's own."""
    padding_embeddings = mask_tokens = _mask_probs = None

    def __init__(self, prep):
        self.fused_assembly = prep.fused_pixels
        self._preprocessors = {"__default": prep}
        self._common_channels = prep.n_output_channels()


def pixel_tokens(prep, x):
    """(inputs_with_pos [B, M, C + C2], inputs_without_pos) of a "pixels" ImagePreprocessor without subsampling on an image
    batch [B, C, H, W], from ONE pio_assemble_tokens call (assemble_tokens' own plan: one space-to-depth segment with s = 1,
    the position table as C2, no padding), or None.  For the hand-off that cannot be split: C or C2 odd.  Bit-identical to
    the chain (every operation is a move); inputs_without_pos is the [:, :, :C] view of the result."""
    if (prep._prep_type != "pixels" or prep._spatial_downsample != 1 or not isinstance(x, torch.Tensor) or x.dim() != 4
            or not (x.shape[1] | prep._positional_encoding.n_output_channels()) & 1):
        return None
    got = assemble_tokens(_OneImage(prep), {"__default": x}, None)
    return None if got is None else (got[0], got[2]["__default"])


def bn_relu_pool_tokens(convnet, x):
    """The tail of Conv2DDownsample.forward_tokens: the last layer's BatchNorm (inference statistics) -> ReLU -> 3x3 stride-2
    max-pool (SAME) -> channels-last tokens [B, OH*OW, C] of its conv output `x` by ONE pio_bn_relu_maxpool_tokens call."""
    x = x.float().contiguous()
    b, c, h, w = x.shape
    if convnet.norms is not None:
        bn = convnet.norms[len(convnet.convs) - 1]
        scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).float()
        shift = (bn.bias - bn.running_mean * scale).float()
    else:
        scale, shift = torch.ones(c, device=x.device), torch.zeros(c, device=x.device)
    pads = IO.same_padding(x.shape[1:], 3, 2)          # [left, right, top, bottom]
    y = torch.empty((b, ((h + 1) // 2) * ((w + 1) // 2), c), dtype=torch.float32, device=x.device)
    R.call_named(x.device, "pio_bn_relu_maxpool_tokens", x=x.data_ptr(), scale=scale.contiguous().data_ptr(),
                 shift=shift.contiguous().data_ptr(), y=y.data_ptr(), B=b, C=c, H=h, W=w, pad_top=pads[2], pad_left=pads[0])
    return R.forward_only(y, x, *convnet.parameters())     # (x carries the network input's and the convs' autograd)


def assemble_tokens(mm, inputs, pos):
    """(x, sizes, without_pos) of forward() from ONE pio_assemble_tokens call, or None.  Taken under the hip backend
    for pos=None, CUDA fp32 inputs, mask probabilities <= 0 or >= 1 and modalities that only move values:
    ImagePreprocessor "patches" (temporal_downsample 1, no conv_after_patching; a space-to-depth segment) or "pixels"
    without subsampling, AudioPreprocessor, OneHotPreprocessor -- image / audio with a concatenated, batch-invariant
    position table and no extra position MLPs.  A masked space-to-depth modality takes the chain.  The result is
    bit-identical to the chain's; without_pos[m] is a view of x (of the modality's own features where it is masked)."""
    if not mm.fused_assembly or pos is not None or mm._preprocessors is None:
        return None
    names = list(mm._preprocessors.keys())
    if not 1 <= len(names) <= L.PIO_MAX_TOKEN_SEGMENTS or not gate(True, *[inputs.get(m) for m in names]):
        return None
    dev, batch, cc = None, None, mm._common_channels
    deps, plan, views = [], {}, {}      # (deps: what the launch reads, kept alive, and what the result is tied to)
    for m in names:
        prep, x = mm._preprocessors[m], inputs[m]
        if x.dim() < 2:
            return None
        if dev is None:
            dev, batch = x.device, x.shape[0]
        if x.device != dev or x.shape[0] != batch or batch < 1:
            return None
        p = 0.0 if mm._mask_probs is None else float(mm._mask_probs[m])
        if 0.0 < p < 1.0:
            return None
        seg = L.TokenSegment()
        if isinstance(prep, IO.OneHotPreprocessor):
            if x.dim() != 2:
                return None
            feats = x[:, None, :]
        elif isinstance(prep, IO.AudioPreprocessor):
            feats = x.reshape(batch, -1, prep._samples_per_patch)
        elif isinstance(prep, IO.ImagePreprocessor):
            s = prep._spatial_downsample
            if prep._prep_type == "patches":
                if prep._temporal_downsample != 1 or prep._conv_after_patching:
                    return None
            elif prep._prep_type != "pixels" or s != 1 or (x.dim() == 5 and prep._temporal_downsample != 1):
                return None
            if x.dim() not in (4, 5) or p >= 1.0:
                return None
            t = x.shape[1] if x.dim() == 5 else 1
            c, h, w = x.shape[-3:]
            if not (1 <= s <= 8 and 1 <= c <= 4) or h % s or w % s or min(t, h, w) < 1:
                return None
            if t * (h // s) * (w // s) != int(math.prod(prep.index_dims)):
                return None
            x = rows(x)
            feats = None
            seg.kind, seg.feature, seg.M, seg.C1 = L.PIO_TOKENS_S2D, x.data_ptr(), t * (h // s) * (w // s), s * s * c
            seg.sb, seg.st, seg.sc, seg.sy = x.stride(0), x.stride(1) if x.dim() == 5 else 0, x.stride(-3), x.stride(-2)
            seg.T, seg.C, seg.H, seg.W, seg.s = t, c, h, w, s
            deps.append(x)
        else:
            return None
        if feats is not None:
            f = rows(feats)
            seg.kind, seg.feature, seg.M, seg.C1 = L.PIO_TOKENS_ROWS, f.data_ptr(), f.shape[1], f.shape[2]
            seg.sb, seg.sm = f.stride(0), f.stride(1)
            deps.append(f)
        if seg.M < 1 or seg.C1 < 1:
            return None
        if not isinstance(prep, IO.OneHotPreprocessor):
            if prep._concat_or_add_pos != "concat" or prep._n_extra_pos_mlp > 0:
                return None
            enc = prep._positional_encoding(batch_size=batch, pos=None, device=dev).to(dev)
            if (enc.dim() != 3 or (enc.shape[0] > 1 and enc.stride(0) != 0) or enc.shape[1] != seg.M
                    or enc.dtype != torch.float32):
                return None
            if enc.shape[2] > 0:
                table = rows(enc[0])            # (any row stride: the entry point takes it as ldt)
                seg.table, seg.ldt, seg.C2 = table.data_ptr(), table.stride(0), table.shape[1]
                deps += [table, enc]
        cp = cc - seg.C1 - seg.C2
        if cp < 0 or (cp > 0 and mm.padding_embeddings is None):
            return None
        params = [(mm.padding_embeddings[m].pos_embs, cp, "pad")] if mm.padding_embeddings is not None else []
        if p >= 1.0:
            params.append((mm.mask_tokens[m].pos_embs, cc, "token"))
        for w_, width, field in params:
            w_c = param_row(w_, width, dev)
            if w_c is False:
                return None
            if w_c is not None:
                setattr(seg, field, w_c.data_ptr())
                deps += [w_c, w_]
        plan[m], views[m] = seg, feats      # (feats: the caller's own view, as the chain returns it, not the kernel's copy)
        deps.append(inputs[m])
    segs, mtot = place(plan)
    if segs is None:
        return None
    y = torch.empty((batch, mtot, cc), dtype=torch.float32, device=dev)
    R.call_named(dev, "pio_assemble_tokens", segs=segs, nseg=len(names), y=y.data_ptr(), ldy=cc, sYb=mtot * cc, B=batch,
                 Mtot=mtot, Cc=cc)
    x = R.forward_only(y, *deps)
    without_pos = {m: views[m] if s.token else x[:, s.row0:s.row0 + s.M, :s.C1] for m, s in plan.items()}
    return x, {m: s.M for m, s in plan.items()}, without_pos


def query_tables(io, name, enc, device):
    """(axis tables, bands [d, K]) of a Fourier query on `device`, built once per module and device with the chain's own
    arithmetic: axis[j][i] = -1 + 2 * i / dims[j] as BasicQuery._encode computes it (int64 -> fp32 division on that
    device), bands from the torch.linspace calls of generate_fourier_features.  Constants of the module's configuration:
    they depend on no parameter, so no write can make them stale and `io` is no runtime.PackedOwner for them."""
    store = io.__dict__.setdefault("_query_table_cache", {})
    key = (name, str(device))
    hit = store.get(key)
    if hit is None:
        with torch.no_grad():
            axes = [(-1 + 2 * torch.arange(int(n), device=device) / torch.tensor(int(n), device=device)).contiguous()
                    for n in enc._index_dims]
            bands = torch.stack([torch.linspace(1.0, res / 2, steps=enc._num_bands) for res in enc._max_resolution],
                                dim=0).to(device).contiguous()
        hit = store[key] = (axes, bands)
    return hit


def build_queries(io, inputs, subsampled_points):
    """(query, sizes) of decoder_query from ONE pio_build_queries call, or None.  Taken under the hip backend on a CUDA
    device for two to four output queries, every one a BasicQuery with concat_preprocessed_input=False over either an
    unprojected FourierPositionEncoding (d <= 3) with a 1-D int64 `subsampled_points` tensor on that device, or a
    TrainablePositionEncoding (fp32) without points; at least one Fourier; fp32 padding embeddings.  The array is
    batch-invariant: ONE [1, Q, Cq] allocation returned as a stride-0 view over the batch (the decoder projects such
    views once).  Position, table and padding channels equal the chain's bit for bit, sine / cosine to the device
    library's accuracy."""
    names = list(io._output_queries.keys())
    # (dtypes=None: the inputs only say where the queries go)
    if not gate(io.fused_queries, inputs, dtypes=None) or not 2 <= len(names) <= L.PIO_MAX_QUERY_SEGMENTS:
        return None
    dev, cq = inputs.device, io.query_channels
    plan, deps, n_fourier = {}, [], 0
    for m in names:
        q = io._output_queries[m]
        if not isinstance(q, OQ.BasicQuery) or q._concat_preprocessed_input:
            return None
        enc, points = q._position_encoding, subsampled_points.get(m)
        seg = L.QuerySegment()
        if type(enc) is PE.FourierPositionEncoding:
            dims, d, k = tuple(enc._index_dims), len(enc._index_dims), int(enc._num_bands)
            if (not 1 <= d <= 3 or len(enc._max_resolution) != d or k < 1 or min(dims) < 1
                    or math.prod(dims) >= 2 ** 31):
                return None
            if (not isinstance(points, torch.Tensor) or points.dim() != 1 or points.dtype != torch.int64
                    or points.device != dev or points.numel() < 1):
                return None
            feats = d * k * (1 if enc._sine_only else 2)
            if 4 * (288 + d * k + 32 * feats) > 65536:      # (a strip's feature rows have to fit the kernel's LDS)
                return None
            axes, bands = query_tables(io, m, enc, dev)
            points = rows(points)
            seg.kind, seg.M, seg.d, seg.K, seg.ldb = L.PIO_QUERY_FOURIER, points.numel(), d, k, bands.stride(0)
            seg.concat_pos, seg.sine_only = int(bool(enc._concat_pos)), int(bool(enc._sine_only))
            for j in range(d):
                seg.dims[j], seg.axis[j] = dims[j], axes[j].data_ptr()
            seg.bands, seg.points = bands.data_ptr(), points.data_ptr()
            width = enc.n_output_channels()
            deps.append(points)
            n_fourier += 1
        elif type(enc) is PE.TrainablePositionEncoding:
            w = enc.pos_embs
            if points is not None or w.dim() != 2 or w.dtype != torch.float32 or w.device != dev or w.shape[0] < 1:
                return None
            table = rows(w)     # (any row stride: ldt; a zero-width table is contiguous as it stands and has no pointer)
            seg.kind, seg.M, seg.C, seg.ldt = L.PIO_QUERY_TABLE, table.shape[0], table.shape[1], table.stride(0)
            seg.table = table.data_ptr() if table.shape[1] > 0 else None
            width = table.shape[1]
            deps += [table, w]
        else:
            return None
        pad = io.padding_embeddings[m].pos_embs
        pad_c = param_row(pad, cq - width, dev)
        if width != q.n_query_channels() or pad_c is False:
            return None
        if pad_c is not None:
            seg.pad = pad_c.data_ptr()
            deps += [pad_c, pad]
        plan[m] = seg
    segs, qtot = place(plan)
    if n_fourier < 1 or segs is None:
        return None
    y = torch.empty((1, qtot, cq), dtype=torch.float32, device=dev)
    R.call_named(dev, "pio_build_queries", segs=segs, nseg=len(names), y=y.data_ptr(), ldy=cq, Qtot=qtot, Cq=cq)
    y = R.forward_only(y, *deps)
    return torch.broadcast_to(y, (inputs.shape[0], qtot, cq)), {m: plan[m].M for m in names}


def head_linear(post):
    """The nn.Linear of a narrow head pio_project_heads can stand for, or None."""
    kind = type(post)
    return post.projection if kind is IO.ProjectionPostprocessor else post.linear if kind is IO.AudioPostprocessor else None


def heads_eligible(io, k: int) -> bool:
    """The part of project_heads' decision that the modules alone settle, for decoder rows of k channels: the switch, at
    least two output modalities, no active range probe (the chain then keeps its "cast" records), every postprocessor a
    ProjectionPostprocessor / AudioPostprocessor with fp32 [n_out <= 16, k] weights or a ClassificationPostprocessor,
    at least one and at most four of the former, k a multiple of 4 in [4, 1024].  Row counts, the batch and the chunk
    grouping play no part: a forward takes one path for all of its decoder calls."""
    posts = io._output_postprocessors
    if not io.fused_heads or posts is None or len(posts) < 2 or LP.range_active() or k < 4 or k > 1024 or k % 4:
        return False
    narrow = 0
    for post in posts.values():
        if type(post) is IO.ClassificationPostprocessor:
            continue
        lin = head_linear(post)
        if lin is None:
            return False
        w, b = lin.weight, lin.bias
        if (w.dtype != torch.float32 or w.dim() != 2 or w.shape[1] != k or not 1 <= w.shape[0] <= 16
                or (b is not None and (b.dtype != torch.float32 or b.device != w.device))):
            return False
        narrow += 1
    return 1 <= narrow <= L.PIO_MAX_HEAD_SEGMENTS


def heads_accept(io, outputs) -> bool:
    """True when project_heads takes this decoder output: the hip backend, a CUDA fp32 [B, Q, K] tensor with unit channel
    stride and 16-byte aligned rows, heads on its device, and heads_eligible(K)."""
    if not gate(True, outputs) or outputs.dim() != 3 or outputs.stride(2) != 1:
        return False
    if (not heads_eligible(io, outputs.shape[2]) or outputs.data_ptr() % 16 or outputs.stride(1) % 4
            or (outputs.shape[0] > 1 and outputs.stride(0) % 4)):
        return False
    return all(lin is None or lin.weight.device == outputs.device
               for lin in map(head_linear, io._output_postprocessors.values()))


def project_heads(io, outputs, query_sizes, into=None):
    """The dict of postprocessed outputs of a decoder output [B, Q, K] from ONE pio_project_heads call for the narrow
    heads (plus the ClassificationPostprocessor's own hip_linear on row 0, unchanged), or None when it declines
    (heads_accept).  `into`: optional {modality: fp32 [B, rows, n_out] view with unit last stride} -- that head's rows are
    written there, in place (MultiModalPerceiver: the group's rows of the final output array), and the view is what the
    dict holds for it; without it a ProjectionPostprocessor returns a fresh [B, rows, n_out] array and an
    AudioPostprocessor a fresh [B, rows * n_out], as the chain does."""
    posts = io._output_postprocessors
    order = sorted(query_sizes)
    if not heads_accept(io, outputs) or order != sorted(posts.keys()) or sum(query_sizes.values()) > outputs.shape[1]:
        return None
    (batch, qtot, k), dev = outputs.shape, outputs.device
    # (not place(): the rows of EVERY modality count, the label's included, and only the narrow heads become segments)
    row0 = dict(zip(order, itertools.accumulate([0] + [query_sizes[m] for m in order])))
    plan, keep, ys = [], [], {}
    for m, post in posts.items():
        lin = head_linear(post)
        if lin is None:
            continue
        w = rows(lin.weight, stride4=True, aligned=True)        # (the kernel reads weight rows as 16-byte vectors)
        b = None if lin.bias is None else lin.bias.detach().contiguous()
        nrows, n_out = query_sizes[m], w.shape[0]
        y = into.get(m) if into is not None else None
        if y is None:
            y = torch.empty((batch, nrows, n_out), dtype=torch.float32, device=dev)
        elif (tuple(y.shape) != (batch, nrows, n_out) or y.dtype != torch.float32 or y.device != dev
                or (nrows > 0 and y.stride(2) != 1)):
            raise ValueError(f"_project_heads: into[{m!r}] must be a float32 [{batch}, {nrows}, {n_out}] view on {dev} "
                             "with unit last stride")
        ys[m] = R.forward_only(y, outputs, lin.weight, lin.bias)
        if nrows < 1:
            continue
        seg = L.HeadSegment()
        seg.row0, seg.rows, seg.n_out = row0[m], nrows, n_out
        seg.w, seg.ldw, seg.bias = w.data_ptr(), w.stride(0), None if b is None else b.data_ptr()
        seg.y, seg.y_sb, seg.y_rs = y.data_ptr(), y.stride(0) if batch > 1 else 0, y.stride(1)
        plan.append(seg)
        keep += [w, b, y]
    if plan:
        R.call_named(dev, "pio_project_heads", segs=(L.HeadSegment * len(plan))(*plan), nseg=len(plan), x=outputs.data_ptr(),
                     x_sb=outputs.stride(0) if batch > 1 else 0, ldx=outputs.stride(1), B=batch, Q=qtot, K=k)
    per_mod = PV.restructure(query_sizes, outputs)
    result = {}
    for m, post in posts.items():
        if m not in ys:
            result[m] = post(per_mod[m], pos=None, modality_sizes=None)
        elif type(post) is IO.AudioPostprocessor and (into is None or m not in into):
            result[m] = ys[m].reshape(batch, -1)
        else:
            result[m] = ys[m]
    return result


# Rows (B x P) up to which pio_vocab_topk multiplies itself; above it runtime.hip_linear makes the logits and the kernel's
# second mode selects.  A measurement (profiles/language_predict.json, tools/prep_bench.py --language-predict): at 262 x 768
# the kernel's own fp32 multiply lost to cast + GEMM + selection at EVERY row count from 1 to 204 800 (55 against 48 us at one
# row, where eight waves stream the whole embedding; 5.2 against 1.6 ms at 204 800), so the shipped routing is the selection
# alone: 0.  The computing mode stays in the library and in the tests (the C-ABI, and the model with this raised).
VOCAB_FUSED_MAX_ROWS = 0


def vocab_plan(post, x, k):
    """What vocab_topk does with a decoder output x [B, P, K] and k: "fused" (the kernel multiplies), "select" (hip_linear, then
    the kernel's selection alone) or None (decline: the chain).  Declines the switch off, the torch backend, CPU tensors,
    anything but fp32 x / embedding / bias on one device, x that is not 3-D with unit channel stride and at least one row,
    V > 1024, k outside [1, min(8, V)] and an active range probe (the chain keeps its "cast" record of x)."""
    w, bias = post._embedding.weight, post.bias
    if not gate(post.fused_predict, x) or LP.range_active() or w.dtype != torch.float32 or bias.dtype != torch.float32:
        return None
    if x.dim() != 3 or w.dim() != 2 or x.shape[2] != w.shape[1] or x.shape[0] < 1 or x.shape[1] < 1 or x.stride(2) != 1:
        return None
    v, kk = w.shape
    if w.device != x.device or bias.device != x.device or tuple(bias.shape) != (v,):
        return None
    if not 1 <= v <= 1024 or not 1 <= k <= min(8, v) or x.shape[0] * x.shape[1] >= 2 ** 31:
        return None
    fused = 4 <= kk <= 1024 and kk % 4 == 0 and x.shape[0] * x.shape[1] <= VOCAB_FUSED_MAX_ROWS
    return "fused" if fused else "select"


def vocab_topk(post, x, k, return_logits=False):
    """(ids int64 [B, P, k], logprobs fp32 [B, P, k], logits fp32 [B, P, V] or None) of a decoder output x [B, P, K] behind an
    EmbeddingPostprocessor from pio_vocab_topk, or None when it declines (vocab_plan).  "fused": ONE launch multiplies the
    unrounded fp32 rows against the fp32 embedding and selects; "select": the postprocessor's own hip_linear (the chain's
    logits, bit for bit), then one launch for log-sum-exp and top-k.  Equal logits put the lower id first."""
    mode = vocab_plan(post, x, k)
    if mode is None:
        return None
    w, bias = post._embedding.weight, post.bias
    (b, p, _), v, dev = x.shape, w.shape[0], x.device
    ids = torch.empty((b, p, k), dtype=torch.int32, device=dev)
    logprob = torch.empty((b, p, k), dtype=torch.float32, device=dev)
    if mode == "fused":
        xr = rows(x, min_stride=True, stride4=True, aligned=True)
        if b > 1 and xr.stride(0) % 4:
            xr = xr.detach().contiguous()
        wr = rows(w, min_stride=True, stride4=True, aligned=True)
        br = bias.detach().contiguous()
        logits = torch.empty((b, p, v), dtype=torch.float32, device=dev) if return_logits else None
        R.call_named(dev, "pio_vocab_topk", x=xr.data_ptr(), x_sb=xr.stride(0) if b > 1 else 0,
                     ldx=xr.stride(1) if p > 1 else xr.shape[2], w=wr.data_ptr(), ldw=wr.stride(0) if v > 1 else wr.shape[1],
                     bias=br.data_ptr(), B=b, Q=p, V=v, K=xr.shape[2], k=k, ids=ids.data_ptr(), logprob=logprob.data_ptr(),
                     lse=None, logits=None if logits is None else logits.data_ptr(), ldl=v)
    else:
        logits = post(x).contiguous()
        R.call_named(dev, "pio_vocab_topk", x=None, x_sb=0, ldx=0, w=None, ldw=0, bias=None, B=b, Q=p, V=v, K=0, k=k,
                     ids=ids.data_ptr(), logprob=logprob.data_ptr(), lse=None, logits=logits.data_ptr(), ldl=v)
        if not return_logits:
            logits = None
    logprob = R.forward_only(logprob, x, w, bias)
    return ids.long(), logprob, (None if logits is None else R.forward_only(logits, x, w, bias))


def top_labels(logits, k):
    """(ids int64 [.., k], probs fp32 [.., k]) of logits [.., V] from ONE pio_vocab_topk call in its selection mode -- the k
    largest logits of every row, largest first, the lower id first among equal logits, probs = exp(logit - log-sum-exp) -- or
    None when it declines: the torch backend, anything but a CUDA fp32 tensor with at least one row, V > 1024, k outside
    [1, min(8, V)], 2^31 rows or more, an active range probe."""
    if not gate(True, logits) or LP.range_active() or logits.dim() < 1:
        return None
    v = logits.shape[-1]
    n = logits.numel() // v if v else 0
    if not 1 <= v <= 1024 or not 1 <= k <= min(8, v) or not 1 <= n < 2 ** 31:
        return None
    dev, lead = logits.device, tuple(logits.shape[:-1])
    flat = logits.detach().reshape(n, v).contiguous()
    ids = torch.empty((n, k), dtype=torch.int32, device=dev)
    logprob = torch.empty((n, k), dtype=torch.float32, device=dev)
    R.call_named(dev, "pio_vocab_topk", x=None, x_sb=0, ldx=0, w=None, ldw=0, bias=None, B=1, Q=n, V=v, K=0, k=k,
                 ids=ids.data_ptr(), logprob=logprob.data_ptr(), lse=None, logits=flat.data_ptr(), ldl=v)
    return ids.long().reshape(lead + (k,)), R.forward_only(torch.exp(logprob).reshape(lead + (k,)), logits)


def finish_media(on, x, kind, reverse=False):
    """The media samples of an fp32 [n, h, w, C] view `x` from ONE pio_finish_media call: contiguous uint8 (kind
    PIO_MEDIA_U8; reverse: channel c written to C - 1 - c) or int16 (PIO_MEDIA_S16) [n, h, w, C] on x's device, x read in
    place through its strides -- or None when it declines: the switch off, the torch backend, anything but a 4-D CUDA fp32
    tensor with 1 to 4 channels and no empty axis, h * w or the workgroup count beyond 2^31 - 1, a data pointer that is not
    4-byte aligned."""
    if not gate(on, x) or x.dim() != 4:
        return None
    n, h, w, c = x.shape
    if min(n, h, w) < 1 or not 1 <= c <= 4 or h * w >= 2 ** 31 or n * h * w >= 2 ** 41 or x.data_ptr() % 4:
        return None
    y = torch.empty((n, h, w, c), dtype=torch.uint8 if kind == L.PIO_MEDIA_U8 else torch.int16, device=x.device)
    sn, sy, sx, sc = x.stride()
    R.call_named(x.device, "pio_finish_media", x=x.data_ptr(), sn=sn, sy=sy, sx=sx, sc=sc, n=n, h=h, w=w, C=c, kind=kind,
                 reverse=int(bool(reverse)), y=y.data_ptr())
    return y


def _covers(corners, length, size):
    """True when the intervals [c, c + length) of the corners cover [0, size)."""
    pos = 0
    while pos < size:
        reach = max([c + length for c in corners if c <= pos], default=pos)
        if reach <= pos:
            return False
        pos = reach
    return True


def blend_tiles(model, pair, h, w, min_overlap):
    """Tiled inference with the blend as ONE pio_flow_blend_tiles call, or None when this call is not the covered one
    (the caller then runs the chain from the start).  The tile groups go through the model exactly as in the chain
    (torch.cat of the tiles, tiles_per_call); nothing is multiplied, padded or added, every group's flows are kept,
    and one launch behind the last group writes the [b, 2, h, w] result: no host tensor, no copy to the device.
    Taken under the hip backend for CUDA fp32 frames when the corner lists and the groups fit the entry's tables (64
    each), every pixel is covered by a tile and every group's flows are CUDA fp32 [g*b, 2, H, W] with the same
    non-negative strides in allocations that do not overlap (checked, not assumed: a model that handed out views of
    one reused buffer would have overwritten the earlier groups)."""
    if not gate(model.fused_blend, pair):
        return None
    ys, xs = model._grid_axes((h, w), min_overlap)
    corners = list(itertools.product(ys, xs))
    b, dev = pair.shape[0], pair.device
    step = max(1, int(model.tiles_per_call))
    ngroups = (len(corners) + step - 1) // step
    if (b < 1 or len(ys) > L.PIO_MAX_BLEND_AXIS or len(xs) > L.PIO_MAX_BLEND_AXIS or ngroups > L.PIO_MAX_BLEND_GROUPS
            or not _covers(ys, model.H, h) or not _covers(xs, model.W, w)):
        return None
    keep, spans = [], []
    for i in range(0, len(corners), step):
        group = corners[i:i + step]
        tiles = torch.cat([pair[..., y:y + model.H, x:x + model.W] for y, x in group], dim=0)
        flows = model._predict_patch(tiles)
        if (not isinstance(flows, torch.Tensor) or flows.device != dev or flows.dtype != torch.float32
                or tuple(flows.shape) != (len(group) * b, 2, model.H, model.W) or min(flows.stride()) < 0
                or (keep and flows.stride() != keep[0].stride()) or flows.data_ptr() % 4):
            return None
        lo = flows.data_ptr()
        hi = lo + 4 * (1 + sum((n - 1) * s for n, s in zip(flows.shape, flows.stride())))
        if any(lo < b1 and a1 < hi for a1, b1 in spans):
            return None
        keep.append(flows)
        spans.append((lo, hi))
    p = L.FlowBlend()
    for i, flows in enumerate(keep):
        p.group[i] = flows.data_ptr()
    p.sn, p.sc, p.sy, p.sx = keep[0].stride()
    p.ngroups, p.tiles_per_group, p.ny, p.nx = len(keep), step, len(ys), len(xs)
    p.ys[:len(ys)], p.xs[:len(xs)] = ys, xs
    p.N, p.H, p.W, p.h, p.w = b, model.H, model.W, h, w
    out = torch.empty((b, 2, h, w), dtype=torch.float32, device=dev)
    # (PIO_E_SHAPE / PIO_E_ALIGN: a refusal, nothing was launched -- the chain)
    if not R.call_named(dev, "pio_flow_blend_tiles", p=p, out=out.data_ptr(), on=2 * h * w, oc=h * w, oy=w,
                        declines=(L.PIO_E_SHAPE, L.PIO_E_ALIGN)):
        return None
    return R.forward_only(out, *keep)


def image_prep_decline(on, items, oh, ow):
    """Why prepare_images does not take `items` ([(view [n, C, H, W], (top, left, height, width)), ..]) to oh x ow, as a
    sentence, or None when it takes them: the switch, the backend, a tensor that is not a CUDA uint8 / fp32 tensor, sizes
    beyond the entry point's caps (source sides 16 384, output sides 1024, a reduction above PIO_IMAGE_MAX_REDUCTION per
    axis), more images than an int32 counts."""
    if not on:
        return "fused_image_prep is off"
    if R.get_backend() != "hip":
        return "the backend is not hip"
    if not 1 <= oh <= 1024 or not 1 <= ow <= 1024:
        return "an output side beyond 1024"
    total = 0
    for x, (_, _, ch, cw) in items:
        if not x.is_cuda:
            return "a tensor that is not on a GPU"
        if x.dtype not in (torch.uint8, torch.float32):
            return "a dtype other than uint8 and float32"
        if x.shape[2] > 16384 or x.shape[3] > 16384:
            return "a source side beyond 16384"
        if ch > L.PIO_IMAGE_MAX_REDUCTION * oh or cw > L.PIO_IMAGE_MAX_REDUCTION * ow:
            return f"a reduction above {L.PIO_IMAGE_MAX_REDUCTION}"
        total += x.shape[0]
    return "2^31 images or more" if total >= 2 ** 31 else None


def prepare_images(on, items, c, oh, ow, antialias, reverse, mean, std, out):
    """`out` [N, C, oh, ow] (fp32, contiguous within an image) filled by pio_prepare_images from `items` (see
    image_prep_decline; every view is read in place through its strides), in launches of at most PIO_MAX_IMAGE_SOURCES
    descriptors, or None when image_prep_decline gives a reason.  mean / std: C Python floats each."""
    if image_prep_decline(on, items, oh, ow) is not None:
        return None
    dev = out.device
    fl = (L.C.c_float * c)
    mean_c, std_c = fl(*mean), fl(*std)
    sb = out.stride(0) if out.shape[0] > 1 else c * oh * ow
    done = 0
    for i in range(0, len(items), L.PIO_MAX_IMAGE_SOURCES):
        group = items[i:i + L.PIO_MAX_IMAGE_SOURCES]
        arr = (L.ImageSource * len(group))()
        for d, (x, (y0, x0, ch, cw)) in zip(arr, group):
            d.data, d.dtype = x.data_ptr(), L.PIO_IMAGE_U8 if x.dtype == torch.uint8 else L.PIO_IMAGE_F32
            d.sb, d.sc, d.sy, d.sx = x.stride()
            d.n, d.C, d.H, d.W = x.shape
            d.y0, d.x0, d.ch, d.cw = y0, x0, ch, cw
        R.call_named(dev, "pio_prepare_images", srcs=arr, nsrc=len(group), C=c, oh=oh, ow=ow, antialias=int(bool(antialias)),
                     reverse_channels=int(bool(reverse)), mean=mean_c, std=std_c, out=out.data_ptr() + 4 * done * sb, out_sb=sb)
        done += sum(x.shape[0] for x, _ in group)
    return out
