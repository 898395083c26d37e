"""Dev tool (GPU): the preprocessing front ends -- one HIP pass against the torch ops it replaces.

    python tools/prep_bench.py                  the Conv2DDownsample tail (pio_bn_relu_maxpool_tokens)
    python tools/prep_bench.py --flow-front     the flow front end (pio_flow_patch_tokens): 368 x 496 frame pairs, N = 1
                                                and N = 4 (a test-mode tile group); prints one JSON line
    python tools/prep_bench.py --multimodal-front   the multimodal front end (pio_assemble_tokens) at full size
                                                ([B, 52097, 704]), B = 1 and B = 4; prints one JSON line
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--flow-front", action="store_true", help="time pio_flow_patch_tokens against the torch chain")
    ap.add_argument("--multimodal-front", action="store_true", help="time pio_assemble_tokens against the torch chain")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    with torch.no_grad():
        if args.flow_front:
            flow_front(args.repeats, args.launches)
        elif args.multimodal_front:
            multimodal_front(args.repeats, args.launches)
        else:
            conv_tail()
