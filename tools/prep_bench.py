"""Dev tool (GPU): the preprocessing front ends -- one HIP pass against the torch ops it replaces.

    python tools/prep_bench.py                  the Conv2DDownsample tail (pio_bn_relu_maxpool_tokens)
    python tools/prep_bench.py --flow-front     the flow front end (pio_flow_patch_tokens): 368 x 496 frame pairs, N = 1
                                                and N = 4 (a test-mode tile group); prints one JSON line
    python tools/prep_bench.py --multimodal-front   the multimodal front end (pio_assemble_tokens) at full size
                                                ([B, 52097, 704]), B = 1 and B = 4; prints one JSON line
    python tools/prep_bench.py --decoder-queries    the multimodal decoder queries (pio_build_queries) at full size: one
                                                16-chunk group [1, 100593, 1026] and the 8 groups of a 128-chunk forward,
                                                the sine / cosine error of chain and kernel over tests/query_cases.py, and
                                                the whole model with and without the query cache; prints one JSON line
    python tools/prep_bench.py --multimodal-heads   the multimodal output heads (pio_project_heads) on one 16-chunk decoder
                                                call [B, 100593, 512], B = 1 and B = 4, against the hip_linear chain;
                                                prints one JSON line
    python tools/prep_bench.py --language-front     the language front end (pio_embed_tokens) at full size ([B, 2048, 768],
                                                V = 262, int64 ids), B = 1, 8 and 100; prints one JSON line
    python tools/prep_bench.py --language-predict   masked-token prediction (LanguagePerceiver.predict, pio_vocab_topk) against
                                                the full forward plus log_softmax / topk at (B, P) = (1, 9), (8, 307),
                                                (100, 307), (100, 2048), and the vocabulary head alone in both modes over
                                                1 .. 204 800 rows (the routing threshold); prints one JSON line
    python tools/prep_bench.py --flow-blend         the tile blend of tiled flow inference (pio_flow_blend_tiles) against the
                                                torch chain at 436 x 1024 (6 tiles) and 1080 x 1920 (20 tiles), b = 1; prints
                                                one JSON line
    python tools/prep_bench.py --flow-blend-forward [--package-root DIR]   the whole test_mode forward of the full-size
                                                FlowPerceiver at 436 x 1024 with the package under DIR (default: this tree):
                                                run it alternately on two checkouts to compare them; prints one JSON line
    python tools/prep_bench.py --flow-image         flow_to_image on the device (pio_flow_to_image) against .cpu().numpy() plus
                                                the numpy function at 368 x 496, 436 x 1024 and 1080 x 1920, b = 1; prints
                                                one JSON line
    python tools/prep_bench.py --image-prep         prepare_images (pio_prepare_images) against the torch chain on four
                                                workloads, and ClassificationPerceiver.prepare + forward at B = 32; prints
                                                one JSON line
    python tools/prep_bench.py --classify-front     the encoder hand-off of the 1x1-conv and pixel classifiers
                                                (pio_conv1x1_tokens, pio_assemble_tokens) against the torch chain at B = 1, 8
                                                and 32, and the whole forward with the switch on and off; prints one JSON line
    python tools/prep_bench.py --media              to_frames / to_pcm16 (pio_finish_media) on the multimodal model's outputs
                                                ([1, 16, 3, 224, 224] and [1, 30720, 1]) against .cpu().numpy() plus the
                                                example's numpy expressions, with and without the copy of the samples to the
                                                host, and the entry alone in TB/s; prints one JSON line
    python tools/prep_bench.py --multimodal-classify   MultiModalPerceiver.classify against forward + softmax + topk at
                                                B = 1 and B = 4, full size; prints one JSON line
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if "--package-root" in sys.argv:                 # (--flow-blend-forward: time another checkout's package)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1])
sys.path[:0] = [ROOT]
import torch  # noqa: E402
from perceiverio_pytorch_amd.io_processors import Conv2DDownsample  # noqa: E402

dev = torch.device("cuda:0")


def timed(f, n=20):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def conv_tail():
    net = Conv2DDownsample(num_layers=1, num_channels=64, use_batchnorm=True).to(dev).eval()
    x = torch.randn(32, 3, 224, 224, device=dev)

    def torch_path():
        y = net(x)
        return y.movedim(1, -1).reshape(y.shape[0], -1, y.shape[1]).contiguous()
    print(f"conv + torch ops (BatchNorm, ReLU, pad + max-pool, channels-last copy): {timed(torch_path):8.1f} us")
    print(f"conv + pio_bn_relu_maxpool_tokens:                                       {timed(lambda: net.forward_tokens(x)):8.1f} us")
    import torch.nn.functional as F
    from perceiverio_pytorch_amd.io_processors import same_padding
    conv = net.convs[0]
    print(f"conv alone:                                                              {timed(lambda: conv(F.pad(x, same_padding(x.shape[1:], conv.kernel_size, conv.stride)))):8.1f} us")


def flow_front(repeats, launches):
    """Three ways to the [N, 182528, 64] features of a 368 x 496 frame pair, timed with device events around `launches`
    back-to-back calls (after 3 warm-up calls each), `repeats` times, the three alternating inside every repeat:
      chain  -- what FlowPerceiver ran before: stack, patches_for_flow (pad, unfold, permute copy), movedim, space_to_depth
                (permute copy), nn.Linear(54, 64)
      module -- ImagePreprocessor._features on the raw pair (stack + pio_flow_patch_tokens + the output allocation)
      entry  -- pio_flow_patch_tokens alone, on the two frames where they are, into a resident output
    Reported per way: median and (min, max) of the repeats in microseconds; for the entry also the rate over the bytes the
    algorithm needs (frames read once, features written once)."""
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd.io_processors import ImagePreprocessor, patches_for_flow
    from perceiverio_pytorch_amd.position_encoding import PosEncodingType
    H, W, C, out = 368, 496, 3, 64
    prep = ImagePreprocessor(img_size=(H, W), input_channels=9 * C, prep_type="patches", spatial_downsample=1,
                             temporal_downsample=2, conv_after_patching=True, num_channels=out,
                             position_encoding_type=PosEncodingType.FOURIER,
                             fourier_position_encoding_kwargs=dict(num_bands=64, max_resolution=(H, W), sine_only=False,
                                                                   concat_pos=True)).to(dev).eval()
    lin = prep._conv_after_patch_layer
    with torch.no_grad():
        lin.bias.normal_(0.0, 0.1)
    lib, stream = L.lib(), torch.cuda.current_stream().cuda_stream
    result = {"tool": "tools/prep_bench.py --flow-front", "shape": [C, H, W], "out": out, "repeats": repeats,
              "launches_per_repeat": launches, "unit": "us", "cases": {}}
    for n in (1, 4):
        im0, im1 = torch.randn(n, C, H, W, device=dev), torch.randn(n, C, H, W, device=dev)
        y = torch.empty(n, H * W, out, device=dev)

        def chain():
            return prep._features(patches_for_flow(torch.stack([im0, im1], dim=1)).movedim(-1, -3))

        def module():
            return prep._features(torch.stack([im0, im1], dim=1))

        def entry():
            L.check(lib.pio_flow_patch_tokens(im0.data_ptr(), im1.data_ptr(), C * H * W, H * W, W, C * H * W, H * W, W,
                                              lin.weight.data_ptr(), lin.bias.data_ptr(), y.data_ptr(), out, n, C, H, W,
                                              out, stream), "pio_flow_patch_tokens")
        ways = {"chain": chain, "module": module, "entry": entry}
        with torch.no_grad():
            a, b = chain(), module()
            entry()
            torch.cuda.synchronize()
            assert torch.equal(b, y), "module and raw entry disagree"
            dev_ab = float((a - b).abs().max())
            times = {k: [] for k in ways}
            for _ in range(repeats):
                for k, f in ways.items():
                    times[k].append(timed(f, launches))
        case = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        need = 4.0 * n * H * W * (2 * C + out)
        case["entry"]["algorithm_bytes"] = need
        case["entry"]["GB_per_s_at_median"] = need / (case["entry"]["median"] * 1e-6) / 1e9
        case["max_abs_chain_minus_fused"] = dev_ab
        result["cases"][f"N={n}"] = case
    print(json.dumps(result))


def multimodal_front(repeats, launches):
    """MultimodalPreprocessor of the default MultiModalPerceiver (16 x 224 x 224 video, 30 720 audio samples, label) both
    ways, timed with device events around `launches` back-to-back calls (after 3 warm-up calls each), `repeats` times, the
    two alternating inside every repeat:
      chain -- the torch ops: movedim + space_to_depth, cat with the Fourier table, cat with the padding embedding (image
               and audio), token + 0 * x for the label, cat over the modalities
      fused -- MultimodalPreprocessor._assemble: the output allocation + ONE pio_assemble_tokens launch
    Reported per way: median and (min, max) of the repeats in microseconds and torch.cuda.max_memory_allocated above what
    was allocated before the call; for the fused way also the store rate over the output's bytes."""
    from perceiverio_pytorch_amd.models import MultiModalPerceiver
    model = MultiModalPerceiver().to(dev).eval()
    mp = model.perceiver._multi_preprocessor
    with torch.no_grad():
        for p in list(mp.padding_embeddings.parameters()) + list(mp.mask_tokens.parameters()):
            p.normal_(0.0, 0.02)
    result = {"tool": "tools/prep_bench.py --multimodal-front", "library": os.path.basename(
        os.environ.get("PIO_LIB_PATH", "libpio_hip.so")), "repeats": repeats, "launches_per_repeat": launches, "unit": "us",
        "cases": {}}
    for b in (1, 4):
        ins = {"image": torch.randn(b, 16, 3, 224, 224, device=dev), "audio": torch.randn(b, 30720, 1, device=dev),
               "label": torch.zeros(b, 700, device=dev)}

        def way(on):
            def f():
                mp.fused_assembly = on
                return mp(ins, pos=None)[0]
            return f
        ways = {"chain": way(False), "fused": way(True)}
        xa, xb = ways["chain"](), ways["fused"]()
        assert mp._assemble(ins, None) is not None, "the fused path declined"
        assert torch.equal(xa, xb), "chain and fused outputs differ"
        shape = list(xa.shape)
        del xa, xb
        peak = {}
        for k, f in ways.items():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            f()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
        times = {k: [] for k in ways}
        for _ in range(repeats):
            for k, f in ways.items():
                times[k].append(timed(f, launches))
        case = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "peak_bytes_above_inputs": peak[k]}
                for k, v in times.items()}
        out_bytes = 4.0 * shape[0] * shape[1] * shape[2]
        case["fused"]["output_bytes"] = out_bytes
        case["fused"]["store_GB_per_s_at_median"] = out_bytes / (case["fused"]["median"] * 1e-6) / 1e9
        case["shape"] = shape
        result["cases"][f"B={b}"] = case
    mp.fused_assembly = True
    print(json.dumps(result))


def _query_errors():
    """Largest |value - float64 sine / cosine of the fp32 phase| over the cases of tests/query_cases.py: the torch chain
    (FourierQuery on this device) and pio_build_queries, each case's bands being torch.linspace's."""
    sys.path[:0] = [os.path.join(ROOT, "tests")]
    import numpy as np
    import query_cases as QC
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd.output_queries import FourierQuery
    from test_queries_host import build_queries
    worst = {"chain": 0.0, "kernel": 0.0}
    per_case = {}
    for name, c in QC.CASES.items():
        bands = {i: torch.stack([torch.linspace(1.0, r / 2, steps=g["K"]) for r in g["res"]]).numpy()
                 for i, g in enumerate(c["segs"]) if g["kind"] == QC.FOURIER}
        data = QC.gen(name, bands)
        ref = QC.reference(name, data)
        held = {(i, w): torch.from_numpy(d[w + "_full"]).to(dev) for i, d in enumerate(data) for w in QC.POINTER_FIELDS
                if d[w + "_full"] is not None}
        segs, args = QC.call_fields(name, data, lambda i, w: held[(i, w)].data_ptr())
        y = torch.full((c["Qtot"], c["ldy"]), float("nan"), device=dev)
        L.check(build_queries(L, segs, y.data_ptr(), args, torch.cuda.current_stream().cuda_stream), name)
        chain = np.full(ref[0].shape, np.nan, dtype=np.float32)
        for g in c["segs"]:
            rows = slice(g["row0"], g["row0"] + g["M"])
            if g["kind"] == QC.FOURIER:
                q = FourierQuery(output_index_dims=g["dims"], num_bands=g["K"], max_resolution=g["res"],
                                 sine_only=g["sine_only"], concat_pos=g["concat_pos"])
                pts = torch.from_numpy(g["points"]) if g["points"] is not None else torch.arange(g["start"], g["start"] + g["M"])
                chain[rows, :g["width"]] = q(torch.zeros(1, 1, 1, device=dev), subsampled_points=pts.to(dev))[0].cpu().numpy()
                chain[rows, g["width"]:c["Cq"]] = ref[0][rows, g["width"]:c["Cq"]]
            else:
                chain[rows, :c["Cq"]] = ref[0][rows, :c["Cq"]]
        per_case[name] = {"max_abs_phase_rad": QC.max_phase(name, data),
                          "chain": QC.compare(chain, ref, name + " chain", bound=1.0),
                          "kernel": QC.compare(y.cpu().numpy(), ref, name + " kernel", bound=1.0)}
        for k in worst:
            worst[k] = max(worst[k], per_case[name][k])
    return {"reference": "float64 sine / cosine of the fp32 phase; position, table and padding channels bit-identical",
            "chain": worst["chain"], "kernel": worst["kernel"], "bound_in_tests": 2 * worst["chain"], "per_case": per_case}


def decoder_queries(repeats, launches):
    """The decoder query array of the default MultiModalPerceiver both ways, timed like multimodal_front:
      chain -- PerceiverIO.decoder_query's torch ops (unravel_index, division, the [n, d, K] product, sin, cos, three cats)
      fused -- PerceiverIO._fused_decoder_query: the output allocation + ONE pio_build_queries launch
    for one 16-chunk group (Q = 100 593) and for the 8 groups of a 128-chunk forward; then the whole model: the first forward
    of a fresh model, and the steady step with cache_queries=False both ways beside the cached step."""
    import time
    from perceiverio_pytorch_amd.models import MultiModalPerceiver
    result = {"tool": "tools/prep_bench.py --decoder-queries", "repeats": repeats, "launches_per_repeat": launches,
              "unit": "us", "cases": {}}
    import contextlib
    with contextlib.redirect_stdout(sys.stderr):         # (the comparison prints each case's figure)
        result["sincos_error"] = _query_errors()
    model = MultiModalPerceiver().to(dev).eval()
    P = model.perceiver
    with torch.no_grad():
        for p in P.padding_embeddings.parameters():
            p.normal_(0.0, 0.02)
    n_chunks, g = 128, model.decode_chunks_per_call
    img_chunk, aud_chunk = 16 * 224 * 224 // n_chunks, 30720 // 16 // n_chunks
    x, sizes = torch.zeros((1, 6, 1), device=dev), {"audio": 2, "image": 2, "label": 2}

    def points(k):
        return {"image": torch.arange(img_chunk * k, img_chunk * (k + g), device=dev),
                "audio": torch.arange(aud_chunk * k, aud_chunk * (k + g), device=dev), "label": None}
    groups = [points(k) for k in range(0, n_chunks, g)]

    def way(on, pts):
        def f():
            P.fused_queries = on
            q = None
            for p in pts:
                q = P.decoder_query(x, sizes, None, subsampled_points=p)[0]
            return q
        return f
    for label, pts in (("one 16-chunk group", groups[:1]), ("128-chunk forward (8 groups)", groups)):
        ways = {"chain": way(False, pts), "fused": way(True, pts)}
        qa, qb = ways["chain"](), ways["fused"]()
        assert P._fused_decoder_query(x, pts[0]) is not None, "the fused path declined"
        shape = list(qa.shape)
        diff = float((qa - qb).abs().max())
        del qa, qb
        peak = {}
        for k, f in ways.items():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            f()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
        times = {k: [] for k in ways}
        for _ in range(repeats):
            for k, f in ways.items():
                times[k].append(timed(f, launches))
        case = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "peak_bytes_above_inputs": peak[k]}
                for k, v in times.items()}
        out_bytes = 4.0 * shape[1] * shape[2] * len(pts)
        for k in case:
            case[k]["store_GB_per_s_at_median"] = out_bytes / (case[k]["median"] * 1e-6) / 1e9
        case.update(shape=shape, arrays=len(pts), output_bytes=out_bytes, max_abs_chain_minus_fused=diff)
        result["cases"][label] = case
    del model, P, groups
    torch.cuda.empty_cache()

    gen = torch.Generator().manual_seed(7)
    images = torch.rand(1, 16, 3, 224, 224, generator=gen).to(dev)
    audio = (torch.rand(1, 30720, 1, generator=gen) * 2 - 1).to(dev)

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    whole = {"unit": "ms", "steps": 5}
    with torch.inference_mode():                         # (one forward of a throw-away model: the process's one-time costs --
        warm = MultiModalPerceiver().to(dev).eval()      #  code objects loaded on first use -- belong to neither way)
        warm(images, audio)
        del warm
    torch.cuda.empty_cache()
    for k, on in (("chain", False), ("fused", True)):
        torch.manual_seed(3)
        m = MultiModalPerceiver().to(dev).eval()
        m.fused_queries = on
        with torch.inference_mode():
            m.cache_queries = False
            cold = wall(lambda: m(images, audio))       # (weight packing and workspaces included, the same both ways)
            uncached = [wall(lambda: m(images, audio)) for _ in range(5)]
            m.cache_queries = True
            first_cached = wall(lambda: m(images, audio))
            cached = [wall(lambda: m(images, audio)) for _ in range(5)]
        whole[k] = {"cold_first_forward": cold, "step_cache_queries_False": statistics.median(uncached),
                    "step_cache_queries_False_min_max": [min(uncached), max(uncached)],
                    "first_forward_filling_the_cache": first_cached, "step_cached": statistics.median(cached),
                    "step_cached_min_max": [min(cached), max(cached)]}
        del m
        torch.cuda.empty_cache()
    result["whole_model_B1_128_chunks"] = whole
    print(json.dumps(result))


def _device_ops(f):
    """(kernels, copies) the device runs for one call of f, from torch.profiler's device events; None where the profiler
    gives none (not measured)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        f()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            f()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
    except Exception as exc:                             # noqa: BLE001 (a tool: report, do not guess)
        print(f"torch.profiler unavailable: {exc!r}", file=sys.stderr)
        return None
    if not names:
        return None
    copies = [n for n in names if "memcpy" in n.lower() or "memset" in n.lower() or "copy" in n.lower()]
    return {"kernels": len(names) - len(copies), "copies": len(copies), "names": sorted(set(names))}


def multimodal_heads(repeats, launches):
    """The output heads of the default MultiModalPerceiver on ONE decoder call of a 16-chunk group ([B, 100 593, 512] fp32:
    240 audio + 100 352 image + 1 label rows), B = 1 and B = 4, timed like multimodal_front, the ways alternating inside
    every repeat, under the model's decoder policy:
      chain -- fused_heads = False: restructure + the three postprocessors through runtime.hip_linear (row slice copy for
               B > 1, 16-bit cast(s), GEMM, a fresh result per head); the torch.cat behind the model's loop is NOT included
      fused -- PerceiverIO._project_heads with into= views of the final image / audio arrays (one pio_project_heads launch +
               the label head's hip_linear on row 0)
      entry -- pio_project_heads alone, into resident outputs: the kernel's read bandwidth over the bytes of the covered rows
    Reported per way: median and (min, max) of the repeats in microseconds, the peak memory above the inputs, the device
    kernels and copies of one call (torch.profiler; null where it reports nothing)."""
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd.models import MultiModalPerceiver, split_policy
    from perceiverio_pytorch_amd.perceiver import restructure
    from perceiverio_pytorch_amd.runtime import precision
    torch.manual_seed(3)
    model = MultiModalPerceiver().to(dev).eval()
    P = model.perceiver
    posts = P._output_postprocessors
    sizes = {"audio": 240, "image": 100352, "label": 1}
    q, k = sum(sizes.values()), 512
    result = {"tool": "tools/prep_bench.py --multimodal-heads", "repeats": repeats, "launches_per_repeat": launches,
              "unit": "us", "policy": model.precision_policy, "rows": sizes, "K": k, "cases": {}}
    lib, stream = L.lib(), torch.cuda.current_stream().cuda_stream
    for b in (1, 4):
        x = torch.randn(b, q, k, device=dev)
        final = {"image": torch.empty(b, 8 * sizes["image"], 3, device=dev),
                 "audio": torch.empty(b, 8 * sizes["audio"], 16, device=dev)}
        into = {m: final[m][:, 3 * sizes[m]:4 * sizes[m]] for m in final}
        segs = (L.HeadSegment * 2)()
        for i, (m, lin, row0) in enumerate((("audio", posts["audio"].linear, 0), ("image", posts["image"].projection, 240))):
            s = segs[i]
            s.row0, s.rows, s.n_out, s.w, s.ldw, s.bias = row0, sizes[m], lin.weight.shape[0], lin.weight.data_ptr(), k, lin.bias.data_ptr()
            s.y, s.y_sb, s.y_rs = into[m].data_ptr(), into[m].stride(0), into[m].stride(1)

        def chain():
            P.fused_heads = False
            per_mod = restructure(sizes, x)
            return {m: post(per_mod[m], pos=None, modality_sizes=None) for m, post in posts.items()}

        def fused():
            P.fused_heads = True
            return P._project_heads(x, sizes, into=into)

        def entry():
            L.check(lib.pio_project_heads(segs, 2, x.data_ptr(), x.stride(0), x.stride(1), b, q, k, stream), "pio_project_heads")
        ways = {"chain": chain, "fused": fused, "entry": entry}
        with precision(split_policy(model.precision_policy)[1]):
            a, f = chain(), fused()
            assert f is not None, "the fused path declined"
            diff = {m: float((a[m].reshape(f[m].shape) - f[m]).abs().max()) for m in ("image", "audio", "label")}
            del a, f
            peak, ops = {}, {}
            for name, fn in ways.items():
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                fn()
                torch.cuda.synchronize()
                peak[name] = torch.cuda.max_memory_allocated() - base
                ops[name] = _device_ops(fn)
            times = {name: [] for name in ways}
            for _ in range(repeats):
                for name, fn in ways.items():
                    times[name].append(timed(fn, launches))
        case = {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "peak_bytes_above_inputs": peak[name],
                       "device_ops_per_call": ops[name]} for name, v in times.items()}
        read = 4.0 * b * (sizes["audio"] + sizes["image"]) * k
        case["entry"]["read_bytes"] = read
        case["entry"]["read_GB_per_s_at_median"] = read / (case["entry"]["median"] * 1e-6) / 1e9
        spread = (case["chain"]["max"] - case["chain"]["min"]) + (case["fused"]["max"] - case["fused"]["min"])
        case.update(x_shape=[b, q, k], max_abs_chain_minus_fused=diff, chain_minus_fused_median=case["chain"]["median"] -
                    case["fused"]["median"], both_spreads=spread)
        result["cases"][f"B={b}"] = case
        del x, final, into
        torch.cuda.empty_cache()
    print(json.dumps(result))


def language_front(repeats, launches):
    """The encoder input of the default LanguagePerceiver (T = 2048, C = 768, V = 262, int64 ids) for B = 1, 8 and 100, timed
    like multimodal_front (device events around `launches` back-to-back calls after 3 warm-up calls, `repeats` times, the
    ways alternating inside every repeat):
      chain -- MultimodalPreprocessor with the switch off: nn.Embedding, the add of the position table, the one-element cat
      fused -- the same call with the switch on (need_tokens = False, as the model sets it): the output allocation, the
               memset of the flag word and ONE pio_embed_tokens launch
      entry -- pio_embed_tokens alone into a resident output, no flag word
    Reported per way: median and (min, max) of the repeats in microseconds, the store rate over the output's bytes and (chain,
    fused) torch.cuda.max_memory_allocated above what was allocated before the call."""
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd.io_processors import EmbeddingPreprocessor
    from perceiverio_pytorch_amd.perceiver import MultimodalPreprocessor
    T, C, V = 2048, 768, 262
    torch.manual_seed(5)
    prep = EmbeddingPreprocessor(vocab_size=V, max_seq_len=T, embedding_dims=C).to(dev).eval()
    prep.need_tokens = False
    mp = MultimodalPreprocessor(input_preprocessors=torch.nn.ModuleDict({"__default": prep}), min_padding_size=0)
    table, pos = prep.embed.weight.detach(), prep.input_pos_encoding.pos_embs.detach()
    lib, stream = L.lib(), torch.cuda.current_stream().cuda_stream
    result = {"tool": "tools/prep_bench.py --language-front", "library": os.path.basename(
        os.environ.get("PIO_LIB_PATH", "libpio_hip.so")), "T": T, "C": C, "V": V, "ids": "int64", "repeats": repeats,
        "launches_per_repeat": launches, "unit": "us", "cases": {}}
    for b in (1, 8, 100):
        ids = torch.randint(0, V, (b, T), device=dev)
        ins = {"__default": ids}
        resident = torch.empty(b, T, C, device=dev)

        def way(on):
            def f():
                prep.fused_embedding = on
                return mp(ins, pos=None)[0]
            return f

        def entry():
            L.check(lib.pio_embed_tokens(ids.data_ptr(), 8, T, table.data_ptr(), C, V, pos.data_ptr(), C, resident.data_ptr(),
                                         T * C, C, None, 0, 0, None, b, T, C, stream), "pio_embed_tokens")
        ways = {"chain": way(False), "fused": way(True), "entry": entry}
        with torch.no_grad():
            xa, xb = ways["chain"](), ways["fused"]()
            entry()
            assert prep._fused(ids) is not None, "the fused path declined"
            assert torch.equal(xa, xb) and torch.equal(xa, resident), "chain and fused outputs differ"
            del xa, xb
            peak = {}
            for k in ("chain", "fused"):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                ways[k]()
                torch.cuda.synchronize()
                peak[k] = torch.cuda.max_memory_allocated() - base
            times = {k: [] for k in ways}
            for _ in range(repeats):
                for k, f in ways.items():
                    times[k].append(timed(f, launches))
        out_bytes = 4.0 * b * T * C
        case = {k: {"median": statistics.median(v), "min": min(v), "max": max(v),
                    "store_GB_per_s_at_median": out_bytes / (statistics.median(v) * 1e-6) / 1e9} for k, v in times.items()}
        for k, v in peak.items():
            case[k]["peak_bytes_above_inputs"] = v
        case.update(shape=[b, T, C], output_bytes=out_bytes)
        result["cases"][f"B={b}"] = case
        del resident, ids, ins
        torch.cuda.empty_cache()
    prep.fused_embedding = True
    print(json.dumps(result))


def language_predict(repeats, launches):
    """Masked-token prediction of the default LanguagePerceiver (T = 2048, C = 768, V = 262, k = 5), timed like language_front
    (device events around back-to-back calls after 3 warm-up calls, `repeats` times, the ways alternating inside every
    repeat; `launches` calls per repeat, 3 at B = 100):
      parent  -- what the parent commit offers: model(ids, mask) (all 2048 positions decoded, [B, 2048, 262] logits -- forward is
                 untouched by predict, bit for bit), then log_softmax(out[b, pos]).topk(k) in torch
      predict -- model.predict(ids, mask, pos, k) with the shipped routing
      chain   -- model.predict with fused_predict = False: the chosen rows decoded, then hip_linear, log_softmax, topk
    for (B, P) = (1, 9), (8, 307), (100, 307) with per-sample positions and (100, 2048) with positions=None.
    Then the vocabulary head alone on seeded decoder rows [1, R, 768] under the decoder's policy, R from 1 to 204 800:
      fused   -- ONE pio_vocab_topk launch that multiplies and selects
      select  -- hip_linear (cast + GEMM), then pio_vocab_topk's selection alone
      chain   -- hip_linear, log_softmax, topk
    and from it the routing threshold: the largest R of the sweep up to which `fused` is the faster of the two kernel routes at
    every R measured.  Prints one JSON line."""
    from perceiverio_pytorch_amd import fused_io as FIO, runtime as R
    from perceiverio_pytorch_amd.models import LanguagePerceiver, split_policy
    T, V, K = 2048, 262, 5
    torch.manual_seed(5)
    model = LanguagePerceiver().to(dev).eval()
    post = model.perceiver._output_postprocessors["__default"]
    with torch.no_grad():
        post.bias.copy_(torch.randn(V) * 0.1)
    result = {"tool": "tools/prep_bench.py --language-predict", "policy": model.precision_policy, "T": T, "V": V, "k": K,
              "repeats": repeats, "unit": "us", "shipped_VOCAB_FUSED_MAX_ROWS": FIO.VOCAB_FUSED_MAX_ROWS, "model": {},
              "head_alone": {}}

    def stats(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}
    for b, p in ((1, 9), (8, 307), (100, 307), (100, T)):
        n = launches if b < 100 else 3
        ids = torch.randint(0, V, (b, T), device=dev)
        mask = torch.ones(b, T, device=dev)
        gen = torch.Generator().manual_seed(b * 7 + p)
        # (positions as a host tensor, as a tokenizer hands them over: a CUDA tensor costs predict a read-back per call)
        pos = None if p == T else torch.stack([torch.randperm(T, generator=gen)[:p] for _ in range(b)])
        index = torch.arange(T, device=dev).expand(b, T) if pos is None else pos.to(dev)

        def parent():
            out = model(ids, mask)
            rows = torch.gather(out, 1, index[:, :, None].expand(-1, -1, V))
            return torch.log_softmax(rows, dim=-1).topk(K, dim=-1)

        def predict(on=True):
            def f():
                model.fused_predict = on
                return model.predict(ids, mask, pos, k=K)
            return f
        ways = {"parent": parent, "predict": predict(True), "chain": predict(False)}
        a, c = ways["parent"](), ways["predict"]()
        agree = float((a[1][..., 0] == c.ids[..., 0]).float().mean())
        del a, c
        times = {w: [] for w in ways}
        for _ in range(repeats):
            for w, f in ways.items():
                times[w].append(timed(f, n))
        model.fused_predict = True
        case = {w: stats(v) for w, v in times.items()}
        case.update(rows=b * p, calls_per_repeat=n, top1_agreement_with_parent=agree,
                    route=FIO.vocab_plan(post, torch.empty(b, p, 768, device=dev), K))
        result["model"][f"B={b},P={p}"] = case
        del ids, mask
        torch.cuda.empty_cache()
    sweep = (1, 9, 64, 512, 2456, 4096, 8192, 16384, 30700, 65536, 204800)
    shipped = FIO.VOCAB_FUSED_MAX_ROWS
    with R.precision(split_policy(model.precision_policy)[1]):
        for r in sweep:
            x = torch.randn(1, r, 768, device=dev, generator=torch.Generator(device=dev).manual_seed(r))

            def head(limit):
                def f():
                    FIO.VOCAB_FUSED_MAX_ROWS = limit
                    return FIO.vocab_topk(post, x, K)
                return f

            def chain():
                return torch.log_softmax(post(x), dim=-1).topk(K, dim=-1)
            ways = {"fused": head(2 ** 31), "select": head(0), "chain": chain}
            times = {w: [] for w in ways}
            for _ in range(repeats):
                for w, f in ways.items():
                    times[w].append(timed(f, launches if r < 65536 else 5))
            result["head_alone"][f"R={r}"] = {w: stats(v) for w, v in times.items()}
            del x
            torch.cuda.empty_cache()
    FIO.VOCAB_FUSED_MAX_ROWS = shipped
    threshold = 0
    for r in sweep:
        t = result["head_alone"][f"R={r}"]
        if t["fused"]["median"] > t["select"]["median"]:
            break
        threshold = r
    result["measured_threshold_rows"] = threshold
    print(json.dumps(result))


def _kernel_launches(f):
    """Device kernels and memory copies of one call of f, counted by the profiler (None where it is not usable)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        f()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            f()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
        copies = sum(1 for e in ev if "memcpy" in e.name.lower() or "copy" in e.name.lower() and "kernel" not in e.name.lower())
        return {"device_events": len(ev), "of_them_memory_copies": copies}
    except Exception as e:      # noqa: BLE001
        return {"error": repr(e)}


def flow_blend(repeats, launches):
    """The tile blend of FlowPerceiver.forward(test_mode=True) at the default tile size 368 x 496, b = 1, tiles_per_call 4,
    for a Sintel frame (436 x 1024, min_overlap 20: 6 tiles) and a 1080p frame (1080 x 1920, min_overlap 24: 20 tiles).  _predict_patch is
    replaced by a stub that hands out resident flows in the layout FlowPostprocessor returns, so no model runs and the two
    ways differ in the blend alone; both still stack the frames and torch.cat the tiles of every group, as the model does.
      chain -- fused_blend = False: the ramp built on the host and copied over, per tile multiply, two pads, two adds, one divide
      fused -- fused_blend = True: the output allocation and ONE pio_flow_blend_tiles launch
      entry -- pio_flow_blend_tiles alone into a resident output
      stack_and_cats -- the stack and the cats alone (what chain and fused share)
    Timed like the other front ends (device events around `launches` back-to-back calls after 3 warm-up calls, `repeats`
    times, the ways alternating inside every repeat): median and (min, max) in microseconds; device events of one call from
    the profiler; torch.cuda.max_memory_allocated above what was allocated before the call."""
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd.models import FlowPerceiver
    H, W = 368, 496
    model = FlowPerceiver(num_latents=4, num_latent_channels=16, num_self_attends_per_block=1).to(dev).eval()
    lib, stream = L.lib(), torch.cuda.current_stream().cuda_stream
    result = {"tool": "tools/prep_bench.py --flow-blend", "tile": [H, W], "b": 1, "tiles_per_call": 4,
              "repeats": repeats, "launches_per_repeat": launches, "unit": "us", "cases": {}}
    # (1080 x 1920 at min_overlap 20 puts a corner at x = 1428 > 1920 - 496: that tile hangs over the edge and the model's
    #  torch.cat of tiles refuses it, chain or not; 24 is the smallest overlap whose 20 tiles all lie inside the frame)
    for h, w, overlap in ((436, 1024, 20), (1080, 1920, 24)):
        ys, xs = model._grid_axes((h, w), overlap)
        tiles = len(ys) * len(xs)
        groups = [torch.randn(min(4, tiles - i), H, W, 2, device=dev).permute(0, 3, 1, 2) for i in range(0, tiles, 4)]
        frames = torch.randn(1, 3, h, w, device=dev)
        resident = torch.empty(1, 2, h, w, device=dev)
        state = {"i": 0}

        def predict(t):
            state["i"] = (state["i"] + 1) % len(groups)
            return groups[state["i"] - 1]
        model._predict_patch = predict

        def way(on):
            def f():
                model.fused_blend = on
                state["i"] = 0
                return model(frames, frames, test_mode=True, min_overlap=overlap)
            return f

        p = L.FlowBlend()
        for i, g in enumerate(groups):
            p.group[i] = g.data_ptr()
        p.sn, p.sc, p.sy, p.sx = groups[0].stride()
        p.ngroups, p.tiles_per_group, p.ny, p.nx = len(groups), 4, len(ys), len(xs)
        p.ys[:len(ys)], p.xs[:len(xs)] = ys, xs
        p.N, p.H, p.W, p.h, p.w = 1, H, W, h, w

        def entry():
            L.check(lib.pio_flow_blend_tiles(p, resident.data_ptr(), 2 * h * w, h * w, w, stream), "pio_flow_blend_tiles")

        def tiles_only():
            pair = torch.stack([frames.contiguous(), frames.contiguous()], dim=1)
            for i in range(0, tiles, 4):
                torch.cat([pair[..., y:y + H, x:x + W] for y in ys for x in xs][i:i + 4], dim=0)
        ways = {"chain": way(False), "fused": way(True), "entry": entry, "stack_and_cats": tiles_only}
        xa, xb = ways["chain"](), ways["fused"]()
        entry()
        torch.cuda.synchronize()
        assert torch.equal(xb, resident), "module and raw entry disagree"
        equal = bool(torch.equal(xa.view(torch.int32), xb.view(torch.int32)))
        maxdiff = float((xa - xb).abs().max())
        del xa, xb
        peak, events = {}, {}
        for k in ("chain", "fused"):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ways[k]()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
        for k in ways:
            events[k] = _kernel_launches(ways[k])
        times = {k: [] for k in ways}
        for _ in range(repeats):
            for k, f in ways.items():
                times[k].append(timed(f, launches))
        case = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "one_call": events[k]}
                for k, v in times.items()}
        for k, v in peak.items():
            case[k]["peak_bytes_above_inputs"] = v
        need = 8.0 * h * w + 8.0 * tiles * H * W
        case["entry"]["algorithm_bytes"] = need
        case["entry"]["GB_per_s_at_median"] = need / (case["entry"]["median"] * 1e-6) / 1e9
        case.update(image=[h, w], min_overlap=overlap, tiles=tiles, groups=len(groups), chain_equals_fused_bit_for_bit=equal,
                    max_abs_chain_minus_fused=maxdiff)
        result["cases"][f"{h}x{w}"] = case
        del groups, frames, resident
        torch.cuda.empty_cache()
    print(json.dumps(result))


def flow_blend_forward(repeats, launches):
    """The whole test_mode forward of the full-size FlowPerceiver (default policy, tiles_per_call 4) on a 436 x 1024 frame
    pair, b = 1: 6 tile forwards in two groups and the blend.  Timed with device events around `launches` forwards after 3
    warm-up forwards, `repeats` times; prints the package it ran and whether that package has the fused blend."""
    from perceiverio_pytorch_amd.models import FlowPerceiver
    torch.manual_seed(1)
    model = FlowPerceiver().to(dev).eval()
    with torch.no_grad():
        for q in model.parameters():             # (the decoder's output weights start as zeros)
            if q.numel() and float(q.abs().max()) == 0.0:
                q.normal_(0.0, 0.02)
    a, b = torch.randn(1, 3, 436, 1024, device=dev), torch.randn(1, 3, 436, 1024, device=dev)
    with torch.inference_mode():
        f = lambda: model(a, b, test_mode=True, min_overlap=20)      # noqa: E731
        out = f()
        t = [timed(f, launches) for _ in range(repeats)]
    import hashlib
    print(json.dumps({"tool": "tools/prep_bench.py --flow-blend-forward", "package_root": ROOT,
                      "fused_blend": getattr(model, "fused_blend", None), "image": [436, 1024], "unit": "us",
                      "repeats": repeats, "launches_per_repeat": launches, "median": statistics.median(t), "min": min(t),
                      "max": max(t), "output_sha1": hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()}))


def flow_image(repeats, launches):
    """flow_to_image of one flow field (b = 1) at 368 x 496, 436 x 1024 and 1080 x 1920, the field resident on the device as
    the model leaves it ([1, 2, h, w], handed over as the permuted [h, w, 2] view):
      device -- perceiverio_pytorch_amd.flow_to_image: two allocations, the memset and the two launches; the image stays
                on the device (device events around `launches` back-to-back calls after 3 warm-up calls)
      entry  -- pio_flow_to_image alone into a resident image (timed the same way)
      host   -- today's path: .cpu().numpy() and utils.flow_utils.flow_to_image (host clock, the copy synchronises)
      copy   -- the .cpu().numpy() of that path alone
    `repeats` alternating runs each: median and (min, max) in microseconds.  The entry's bytes per second are over one read of
    the flow and one write of the image (11 bytes per pixel; the entry reads the flow twice, once per launch)."""
    import time
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L
    from utils import flow_utils as FU
    lib, stream = L.lib(), torch.cuda.current_stream().cuda_stream
    result = {"tool": "tools/prep_bench.py --flow-image", "b": 1, "repeats": repeats, "launches_per_repeat": launches,
              "unit": "us", "cases": {}}
    for h, w in ((368, 496), (436, 1024), (1080, 1920)):
        flow = torch.randn(1, 2, h, w, device=dev) * 3.0
        view = flow[0].permute(1, 2, 0)
        img = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
        rad = torch.empty(1, dtype=torch.int32, device=dev)

        def entry():
            L.check(lib.pio_flow_to_image(flow.data_ptr(), 0, w, 1, h * w, 1, h, w, 0.0, False, False, img.data_ptr(),
                                          rad.data_ptr(), stream), "pio_flow_to_image")

        def host_clock(f, n):
            f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                f()
            return (time.perf_counter() - t0) / n * 1e6
        n_host = max(2, launches // 5)
        ways = {"device": lambda: timed(lambda: P.flow_to_image(view), launches), "entry": lambda: timed(entry, launches),
                "host": lambda: host_clock(lambda: FU.flow_to_image(view.cpu().numpy()), n_host),
                "copy": lambda: host_clock(lambda: view.cpu().numpy(), n_host)}
        a, b = P.flow_to_image(view), FU.flow_to_image(view.cpu().numpy())
        entry()
        torch.cuda.synchronize()
        assert torch.equal(a, img), "public function and raw entry disagree"
        differ = int((a.cpu().numpy() != b).sum())
        times = {k: [] for k in ways}
        for _ in range(repeats):
            for k, f in ways.items():
                times[k].append(f())
        case = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        need = 11.0 * h * w
        case["entry"]["algorithm_bytes"] = need
        case["entry"]["GB_per_s_at_median"] = need / (case["entry"]["median"] * 1e-6) / 1e9
        case["device"]["one_call"] = _kernel_launches(lambda: P.flow_to_image(view))
        case.update(image=[h, w], bytes_differing_from_numpy=differ, bytes=3 * h * w)
        result["cases"][f"{h}x{w}"] = case
        del flow, view, img
        torch.cuda.empty_cache()
    print(json.dumps(result))


def image_prep(repeats, launches, forward=True):
    """prepare_images (pio_prepare_images) against the torch chain (fused_image_prep = False) on the same device, sources
    resident, `repeats` alternating runs of `launches` back-to-back calls each (device events, 3 warm-up calls):
      batch32   -- 32 uint8 channels-last photographs of 500 x 375 as ONE tensor -> 224 x 224, centre square, antialiased
      list32    -- 32 such photographs of mixed sizes between 256 and 640 as a list
      video16   -- a 16-frame 240 x 320 BGR clip through MultiModalPerceiver.prepare_video
      frame1080 -- one 1080 x 1920 frame -> 224 x 224, antialiased
    Per workload: median and (min, max) in microseconds of both paths, device kernels and copies of one call, peak memory
    above the inputs, and the kernel path's bytes per second over the bytes it must move (crop in, output out).  Then the
    whole step: ClassificationPerceiver.prepare + forward at B = 32 against chain + forward, three alternating runs."""
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd.models import ClassificationPerceiver, MultiModalPerceiver
    from perceiverio_pytorch_amd.image_prep import center_box
    g = torch.Generator().manual_seed(0)

    def photo(h, w):
        return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).to(dev)
    sizes = [(256 + (37 * i) % 385, 256 + (101 * i) % 385) for i in range(32)]
    mm = MultiModalPerceiver.__new__(MultiModalPerceiver)
    mm.H, mm.W = 224, 224
    batch, many = torch.stack([photo(500, 375) for _ in range(32)]), [photo(h, w) for h, w in sizes]
    clip, frame = torch.stack([photo(240, 320) for _ in range(16)]), photo(1080, 1920)
    cls = dict(size=(224, 224), crop="center", mean=ClassificationPerceiver.MEAN_RGB, std=ClassificationPerceiver.STDDEV_RGB)
    work = {"batch32": (lambda: P.prepare_images(batch, **cls), [(500, 375)] * 32),
            "list32": (lambda: P.prepare_images(many, **cls), sizes),
            "video16": (lambda: mm.prepare_video(clip), [(240, 320)] * 16),
            "frame1080": (lambda: P.prepare_images(frame, (224, 224)), None)}
    result = {"tool": "tools/prep_bench.py --image-prep", "repeats": repeats, "launches_per_repeat": launches, "unit": "us",
              "cases": {}}

    def switched(on, f):
        def run():
            P.fused_image_prep = on
            try:
                return f()
            finally:
                P.fused_image_prep = True
        return run

    def peak(f):
        f()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        f()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    for name, (f, shapes) in work.items():
        ways = {"kernel": switched(True, f), "chain": switched(False, f)}
        a, b = ways["kernel"](), ways["chain"]()
        times = {k: [] for k in ways}
        for _ in range(repeats):
            for k, w in ways.items():
                times[k].append(timed(w, launches))
        case = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "one_call": _kernel_launches(ways[k]),
                    "peak_bytes_above_inputs": peak(ways[k])} for k, v in times.items()}
        crops = [(1080, 1920)] if shapes is None else [center_box(h, w)[2:] for h, w in shapes]
        need = sum(3 * ch * cw for ch, cw in crops) + 4.0 * a.numel()
        case["kernel"]["algorithm_bytes"] = need
        case["kernel"]["GB_per_s_at_median"] = need / (case["kernel"]["median"] * 1e-6) / 1e9
        case["max_abs_difference_kernel_chain"] = float((a - b).abs().max())
        result["cases"][name] = case
    if forward:
        model = ClassificationPerceiver().to(dev).eval()
        steps = {"kernel": switched(True, lambda: model(model.prepare(batch))),
                 "chain": switched(False, lambda: model(model.prepare(batch)))}
        times = {k: [] for k in steps}
        for _ in range(3):
            for k, w in steps.items():
                times[k].append(timed(w, max(2, launches // 4)))
        result["classifier_step_B32"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)}
                                         for k, v in times.items()}
    print(json.dumps(result))


def classify_front(repeats, launches):
    """The encoder hand-off of the LEARNED_POS_1X1CONV and FOURIER_POS_PIXEL classifiers ([B, 3, 224, 224] images, 50 176
    tokens) for B = 1, 8 and 32, timed like language_front (device events around back-to-back calls after 3 warm-up calls,
    `repeats` times, the ways alternating inside every repeat; `launches` calls per repeat at B = 1, a quarter of them above):
      chain -- ImagePreprocessor.forward_split with the switch off: the torch ops and the concatenated array
      fused -- the same call with the switch on: ONE launch (1x1: the features, next to the cached table; pixels: the array)
      entry -- 1x1 only: pio_conv1x1_tokens alone into a resident output
    Reported per way: median and (min, max) in microseconds, device kernels and copies per call, and (chain, fused)
    torch.cuda.max_memory_allocated above what was allocated before the call; for the entry the rate of its one write.
    Then the whole forward of both classifiers at B = 1 and B = 8 with fused_front_end on and off (off runs the code the
    switch was added to), three alternating runs of `launches` / 4 forwards each."""
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd.models import ClassificationPerceiver, PrepType
    torch.manual_seed(7)
    lib, stream = L.lib(), torch.cuda.current_stream().cuda_stream
    result = {"tool": "tools/prep_bench.py --classify-front", "library": os.path.basename(
        os.environ.get("PIO_LIB_PATH", "libpio_hip.so")), "image": [3, 224, 224], "tokens": 50176, "repeats": repeats,
        "launches_per_repeat": {"B=1": launches, "B>1": max(2, launches // 4)}, "unit": "us", "handoff": {}, "forward": {}}
    models = {"conv1x1": ClassificationPerceiver(prep_type=PrepType.LEARNED_POS_1X1CONV).to(dev).eval(),
              "pixels": ClassificationPerceiver(prep_type=PrepType.FOURIER_POS_PIXEL).to(dev).eval()}
    for variant, model in models.items():
        prep = model.perceiver._multi_preprocessor._preprocessors["__default"]
        for b in (1, 8, 32):
            n = launches if b == 1 else max(2, launches // 4)
            x = torch.randn(b, 3, 224, 224, device=dev)

            def way(on, model=model, prep=prep, x=x):
                def f():
                    model.fused_front_end = on
                    return prep.forward_split(x)
                return f
            ways = {"chain": way(False), "fused": way(True)}
            if variant == "conv1x1":
                conv = prep.convnet_1x1
                resident = torch.empty(b, 50176, 256, device=dev)

                def entry(conv=conv, resident=resident, x=x, b=b):
                    L.check(lib.pio_conv1x1_tokens(x.data_ptr(), *x.stride(), conv.weight.data_ptr(), 3, conv.bias.data_ptr(),
                                                   resident.data_ptr(), 256, 50176 * 256, b, 3, 224, 224, 1, 256, stream),
                            "pio_conv1x1_tokens")
                ways["entry"] = entry
            got = {k: ways[k]() for k in ("chain", "fused")}
            # (1x1 at B = 1: the chain's projected positions are one table as they stand, so it hands over a pair as well)
            assert got["fused"][0] == ("split" if variant == "conv1x1" else "full"), "the fused path declined"
            kinds = {k: got[k][0] for k in got}
            if variant == "pixels":
                assert torch.equal(got["chain"][1], got["fused"][1]), "chain and fused arrays differ"
            else:
                err = (got["chain"][1][:, :, :256] - got["fused"][1]).abs().max().item()
                assert err <= 1e-5, f"chain and fused features differ by {err}"
            del got
            ops = {k: _device_ops(ways[k]) for k in ways}
            peak = {}
            for k in ("chain", "fused"):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                ways[k]()
                torch.cuda.synchronize()
                peak[k] = torch.cuda.max_memory_allocated() - base
            times = {k: [] for k in ways}
            for _ in range(repeats):
                for k, f in ways.items():
                    times[k].append(timed(f, n))
            case = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "device_ops": ops[k]}
                    for k, v in times.items()}
            for k, v in peak.items():
                case[k]["peak_bytes_above_inputs"] = v
                case[k]["handoff"] = kinds[k]
            if "entry" in case:
                out_bytes = 4.0 * b * 50176 * 256
                case["entry"].update(output_bytes=out_bytes,
                                     write_TB_per_s_at_median=out_bytes / (case["entry"]["median"] * 1e-6) / 1e12)
            result["handoff"].setdefault(variant, {})[f"B={b}"] = case
            del x, ways
            torch.cuda.empty_cache()
        model.fused_front_end = True
    for variant, model in models.items():
        for b in (1, 8):
            x = torch.randn(b, 3, 224, 224, device=dev)
            runs = {"on": [], "off": []}
            for _ in range(3):
                for k in ("off", "on"):
                    model.fused_front_end = k == "on"
                    runs[k].append(timed(lambda: model(x), max(2, launches // 4)))
            model.fused_front_end = True
            result["forward"].setdefault(variant, {})[f"B={b}"] = {
                k: {"runs": v, "min": min(v), "max": max(v)} for k, v in runs.items()}
    print(json.dumps(result))


def _host_clock(f, n):
    import time
    f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def media(repeats, launches):
    """to_frames on the multimodal model's image output ([1, 16, 3, 224, 224], the moveaxis view of [1, 16*224*224, 3]
    storage) and to_pcm16 on its audio output ([1, 30720, 1]), both resident on the device:
      device      -- perceiverio_pytorch_amd.to_frames / to_pcm16: one allocation and one launch; the samples stay on the
                     device (device events around `launches` back-to-back calls after 3 warm-up calls)
      entry       -- pio_finish_media alone into a resident output (timed the same way), with its TB/s over one read of the
                     fp32 array and one write of the samples
      entry_chw   -- frames only: the entry on a channels-first CONTIGUOUS copy of the image (the strided path at full size)
      device+copy -- the public function, then .cpu() of the samples (host clock)
      host        -- the example's path: .cpu().numpy(), then np.clip / * 255 / astype per frame, or (a * 2**15).astype
                     (host clock, the copy synchronises)
    `repeats` alternating runs each: median and (min, max) in microseconds."""
    import numpy as np
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L
    lib, stream = L.lib(), torch.cuda.current_stream().cuda_stream
    t, h, w = 16, 224, 224
    store = torch.rand(1, t * h * w, 3, device=dev) * 1.2 - 0.1
    image = store.reshape(1, t, h, w, 3).moveaxis(-1, -3)
    planar = image.contiguous()
    audio = torch.rand(1, 30720, 1, device=dev) * 2 - 1
    frames = torch.empty(t, h, w, 3, dtype=torch.uint8, device=dev)
    frames2 = torch.empty_like(frames)
    pcm = torch.empty(30720, dtype=torch.int16, device=dev)

    def entry_frames():
        L.check(lib.pio_finish_media(store.data_ptr(), h * w * 3, w * 3, 3, 1, t, h, w, 3, L.PIO_MEDIA_U8, 0, frames.data_ptr(),
                                     stream), "pio_finish_media")

    def entry_chw():
        L.check(lib.pio_finish_media(planar.data_ptr(), 3 * h * w, w, 1, h * w, t, h, w, 3, L.PIO_MEDIA_U8, 0,
                                     frames2.data_ptr(), stream), "pio_finish_media")

    def entry_pcm():
        L.check(lib.pio_finish_media(audio.data_ptr(), 0, 0, 1, 1, 1, 1, 30720, 1, L.PIO_MEDIA_S16, 0, pcm.data_ptr(), stream),
                "pio_finish_media")

    def host_frames():
        video = image.cpu().numpy()[0]
        return [(np.clip(np.moveaxis(f, 0, -1), 0, 1) * 255).astype(np.uint8) for f in video]

    def host_pcm():
        return (audio.cpu().numpy()[0, :, 0] * 2 ** 15).astype(np.int16)
    n_host = max(2, launches // 5)
    work = {
        "frames": {"device": lambda: timed(lambda: P.to_frames(image), launches),
                   "entry": lambda: timed(entry_frames, launches), "entry_chw": lambda: timed(entry_chw, launches),
                   "device+copy": lambda: _host_clock(lambda: P.to_frames(image).cpu(), n_host),
                   "host": lambda: _host_clock(host_frames, n_host)},
        "pcm": {"device": lambda: timed(lambda: P.to_pcm16(audio), launches), "entry": lambda: timed(entry_pcm, launches),
                "device+copy": lambda: _host_clock(lambda: P.to_pcm16(audio).cpu(), n_host),
                "host": lambda: _host_clock(host_pcm, n_host)},
    }
    entry_frames(), entry_chw(), entry_pcm()
    torch.cuda.synchronize()
    got = P.to_frames(image)
    assert torch.equal(got[0], frames) and torch.equal(frames, frames2), "public function and raw entry disagree"
    assert np.array_equal(got[0].cpu().numpy(), np.stack(host_frames())), "device frames differ from numpy's"
    assert torch.equal(P.to_pcm16(audio).reshape(-1), pcm) and np.array_equal(pcm.cpu().numpy(), host_pcm())
    result = {"tool": "tools/prep_bench.py --media", "repeats": repeats, "launches_per_repeat": launches,
              "host_calls_per_repeat": n_host, "unit": "us", "image": [1, t, 3, h, w], "audio": [1, 30720, 1], "cases": {}}
    need = {"frames": 5.0 * t * h * w * 3, "pcm": 6.0 * 30720}
    for name, ways in work.items():
        times = {k: [] for k in ways}
        for _ in range(repeats):
            for k, f in ways.items():
                times[k].append(f())
        case = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        for k in ("entry", "entry_chw"):
            if k in case:
                case[k]["algorithm_bytes"] = need[name]
                case[k]["TB_per_s_at_median"] = need[name] / (case[k]["median"] * 1e-6) / 1e12
        result["cases"][name] = case
    result["cases"]["frames"]["device"]["one_call"] = _kernel_launches(lambda: P.to_frames(image))
    result["cases"]["pcm"]["device"]["one_call"] = _kernel_launches(lambda: P.to_pcm16(audio))
    print(json.dumps(result))


def multimodal_classify(repeats, launches):
    """MultiModalPerceiver.classify (one decoder row, top-5 on the device) against what there was before it: forward (128
    chunks), then softmax + topk of its label, at B = 1 and B = 4 on the full-size model.  Whole calls, device events around
    `launches` / 4 back-to-back calls after 3 warm-up calls, three alternating runs each: the runs, min and max in
    microseconds; and whether the two agree on the labels."""
    from perceiverio_pytorch_amd.models import MultiModalPerceiver
    torch.manual_seed(3)
    model = MultiModalPerceiver().to(dev).eval()
    n = max(2, launches // 4)
    result = {"tool": "tools/prep_bench.py --multimodal-classify", "calls_per_run": n, "unit": "us", "cases": {}}
    for b in (1, 4):
        images, audio = torch.rand(b, 16, 3, 224, 224, device=dev), torch.rand(b, 30720, 1, device=dev) * 2 - 1

        def before():
            probs, ids = torch.softmax(model(images, audio)["label"], dim=-1).topk(5, dim=-1)
            return ids, probs

        def classify():
            lab = model.classify(images, audio, k=5)
            return lab.ids, lab.probs
        ways = {"forward+softmax+topk": before, "classify": classify}
        a, c = before(), classify()
        runs = {k: [] for k in ways}
        for _ in range(3):
            for k, f in ways.items():
                runs[k].append(timed(f, n))
        case = {k: {"runs": v, "min": min(v), "max": max(v)} for k, v in runs.items()}
        case["same_top5_ids"] = bool(torch.equal(a[0], c[0]))
        case["max_abs_prob_difference"] = float((a[1] - c[1]).abs().max())
        case["classify"]["one_call"] = _kernel_launches(classify)
        result["cases"][f"B={b}"] = case
        del images, audio
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--classify-front", action="store_true",
                    help="time the 1x1-conv and pixel classifier hand-offs (pio_conv1x1_tokens, pio_assemble_tokens)")
    ap.add_argument("--image-prep", action="store_true", help="time pio_prepare_images against the torch chain")
    ap.add_argument("--flow-front", action="store_true", help="time pio_flow_patch_tokens against the torch chain")
    ap.add_argument("--multimodal-front", action="store_true", help="time pio_assemble_tokens against the torch chain")
    ap.add_argument("--decoder-queries", action="store_true", help="time pio_build_queries against the torch chain")
    ap.add_argument("--multimodal-heads", action="store_true", help="time pio_project_heads against the hip_linear chain")
    ap.add_argument("--language-front", action="store_true", help="time pio_embed_tokens against the torch chain")
    ap.add_argument("--language-predict", action="store_true", help="time LanguagePerceiver.predict and pio_vocab_topk")
    ap.add_argument("--flow-blend", action="store_true", help="time pio_flow_blend_tiles against the torch chain")
    ap.add_argument("--flow-blend-forward", action="store_true", help="time the whole tiled forward of the flow model")
    ap.add_argument("--flow-image", action="store_true", help="time flow_to_image on the device against the numpy path")
    ap.add_argument("--media", action="store_true", help="time to_frames / to_pcm16 (pio_finish_media) against the numpy path")
    ap.add_argument("--multimodal-classify", action="store_true",
                    help="time MultiModalPerceiver.classify against forward + softmax + topk")
    ap.add_argument("--package-root", default=None, help="--flow-blend-forward: the checkout whose package is timed")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    with torch.no_grad():
        if args.classify_front:
            classify_front(args.repeats, args.launches)
        elif args.image_prep:
            image_prep(args.repeats, args.launches)
        elif args.flow_front:
            flow_front(args.repeats, args.launches)
        elif args.multimodal_front:
            multimodal_front(args.repeats, args.launches)
        elif args.decoder_queries:
            decoder_queries(args.repeats, args.launches)
        elif args.multimodal_heads:
            multimodal_heads(args.repeats, args.launches)
        elif args.language_front:
            language_front(args.repeats, args.launches)
        elif args.language_predict:
            language_predict(args.repeats, args.launches)
        elif args.flow_blend:
            flow_blend(args.repeats, args.launches)
        elif args.flow_blend_forward:
            flow_blend_forward(args.repeats, args.launches)
        elif args.flow_image:
            flow_image(args.repeats, args.launches)
        elif args.media:
            media(args.repeats, args.launches)
        elif args.multimodal_classify:
            multimodal_classify(args.repeats, args.launches)
        else:
            conv_tail()
