"""GPU: the tile blend of tiled flow inference -- pio_flow_blend_tiles through the raw C-ABI on every case of
tests/flow_blend_cases.py against the definition, as int32 bit patterns, twice; the same tiles with xs reversed; its refusal
table on device memory; FlowPerceiver on the small flow golden with fused_blend on and off at tiles_per_call 4 and 1 (equal
bits, both within TOL of the golden, exactly ONE kernel call on the fused path and none on the chain's); the fallbacks.

Memory safety by construction: every group sits between a NaN guard sample in front and one behind, with NaN pad rows and
columns inside (a read outside a tile turns the output NaN); the output sits in a NaN-filled allocation between 4 KiB guard
bands, with oy > w and gaps behind every plane and sample, and is compared as a whole."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_blend_cases as BC  # noqa: E402
from test_flow_front_gpu import GuardedOut  # noqa: E402
from test_flow_blend_host import blend_chain  # noqa: E402
from test_models import TOL, _close, _load_generated, build  # noqa: E402
from _golden import load  # noqa: E402
from cases import model_inputs, model_seed, model_stats  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


_REF = {}


def case_data(name):
    """(inputs, definition) of a case, computed once and shared (read-only) by the tests below."""
    if name not in _REF:
        data = BC.gen(name)
        _REF[name] = (data, BC.reference(name, data))
    return _REF[name]


def launch(dev, name, data, xs=None):
    """One call of the raw entry on the case's NaN-surrounded groups; returns the guarded output allocation."""
    from perceiverio_pytorch_amd import _lib as L
    c = BC.CASES[name]
    held = [torch.from_numpy(a).to(dev) for a in data["full"]]
    out = GuardedOut(dev, 1, BC.out_layout(c)[4])
    f = BC.case_fields(name, data, [t.data_ptr() for t in held], out.t.data_ptr(), xs=xs)
    L.check(BC.blend(L, f, torch.cuda.current_stream().cuda_stream), f"pio_flow_blend_tiles[{name}]")
    out.check(name)
    return out


def _same_bits(got, want_np, what):
    want = torch.from_numpy(want_np.view(np.int32)).to(got.device)
    assert torch.equal(got.reshape(-1).view(torch.int32), want), what


@pytest.mark.parametrize("name", sorted(BC.CASES))
def test_raw_entry_against_the_definition(dev, name):
    """Equal to the definition bit for bit, signs of zeros included; everything outside out -- the columns [w, oy), the gaps
    behind planes and samples -- still NaN; two launches identical."""
    data, ref = case_data(name)
    want = BC.expected_full(name, ref)
    a = launch(dev, name, data)
    _same_bits(a.t, want, f"{name}: kernel and definition differ, or the kernel wrote outside out")
    b = launch(dev, name, data)
    assert torch.equal(a.t.view(torch.int32), b.t.view(torch.int32)), f"{name}: two launches differ"


@pytest.mark.parametrize("name", ["odd", "dup"])
def test_tile_order_is_part_of_the_contract(dev, name):
    """The same tiles with xs reversed: not the forward-order result, and the definition evaluated in the reversed order."""
    data, ref = case_data(name)
    xs = BC.CASES[name]["xs"][::-1]
    rev = BC.reference(name, data, xs=xs)
    assert not np.array_equal(rev.view(np.int32), ref.view(np.int32))
    got = launch(dev, name, data, xs=xs)
    _same_bits(got.t, BC.expected_full(name, rev), f"{name}: reversed xs")
    assert not torch.equal(got.t.view(torch.int32), launch(dev, name, data).t.view(torch.int32))


@pytest.mark.parametrize("what,changes,code", BC.REFUSALS, ids=[r[0] for r in BC.REFUSALS])
def test_refusals_launch_nothing(dev, what, changes, code):
    from perceiverio_pytorch_amd import _lib as L
    groups = [torch.randn(BC.R_GROUP_ELEMS + 8, device=dev) for _ in range(2)]
    out = GuardedOut(dev, 1, 2 * BC.R_OUT_ELEMS)
    out.t.fill_(-7.5)
    ptrs = {"g0": groups[0].data_ptr(), "g1": groups[1].data_ptr(), "out": out.t.data_ptr()}
    assert BC.blend(L, BC.refusal_fields(ptrs, changes), torch.cuda.current_stream().cuda_stream) == code
    out.check(what)
    assert bool((out.t == -7.5).all()), f"{what}: a refused call wrote to out"


def test_the_valid_call_of_the_refusal_table_runs(dev):
    from perceiverio_pytorch_amd import _lib as L
    groups = [torch.randn(BC.R_GROUP_ELEMS, device=dev) for _ in range(2)]
    out = GuardedOut(dev, 1, BC.R_OUT_ELEMS)
    ptrs = {"g0": groups[0].data_ptr(), "g1": groups[1].data_ptr(), "out": out.t.data_ptr()}
    assert BC.blend(L, BC.base_fields(ptrs), torch.cuda.current_stream().cuda_stream) == BC.PIO_OK
    out.check("valid call")
    views = [g.view(2, 2, BC.R_H, BC.R_W).cpu() for g in groups]
    want = blend_chain(BC.R_H, BC.R_W, BC.R_h, BC.R_w, list(itertools.product([0, 2], [0, 3])), 2, 1, views)
    assert torch.equal(out.t.cpu().view(1, 2, BC.R_h, BC.R_w).view(torch.int32), want.view(torch.int32))


def _counting(monkeypatch):
    """pio_flow_blend_tiles as every module sees it (a proxy in front of _lib.lib()), counted."""
    from perceiverio_pytorch_amd import _lib as L
    calls = {"kernel": 0}
    real = L.lib()

    class _Lib:
        def __getattr__(self, k):
            return getattr(real, k)

        def pio_flow_blend_tiles(self, *a):
            calls["kernel"] += 1
            return real.pio_flow_blend_tiles(*a)
    proxy = _Lib()
    monkeypatch.setattr(L, "lib", lambda: proxy)
    return calls


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_flow_perceiver_small_golden_fused_blend_on_and_off(dev, monkeypatch):
    """model_flow_small (48 x 64 training size, 60 x 80 frames: 4 tiles) in test_mode at tiles_per_call 4 and 1: fused_blend
    True and False within TOL of the golden and equal bit for bit; one kernel call on the fused path, none on the chain's.
    Should the GPU chain (ATen's multiply, pad, add, divide) and the kernel ever differ, the CPU chain on copies of the very
    tile flows the fused run kept decides: the kernel must equal that."""
    name = "model_flow_small"
    g = load(name)
    model = _load_generated(build(name), g, dev, model_seed(name), model_stats(name))
    assert model.fused_blend is True
    ins = [torch.from_numpy(a).to(dev) for a in model_inputs(name)]
    calls = _counting(monkeypatch)
    kept = []
    real_predict = model._predict_patch

    def predict(tiles):
        kept.append(real_predict(tiles))
        return kept[-1]
    monkeypatch.setattr(model, "_predict_patch", predict)
    corners = list(model.compute_grid_indices((60, 80), 10))
    for tpc in (4, 1):
        model.tiles_per_call = tpc
        outs, flows = {}, {}
        for on in (True, False):
            model.fused_blend = on
            del kept[:]
            before = calls["kernel"]
            with torch.inference_mode():
                outs[on] = model(ins[0], ins[1], test_mode=True, min_overlap=10)
            assert calls["kernel"] - before == (1 if on else 0), (tpc, on, calls)
            assert len(kept) == (len(corners) + tpc - 1) // tpc
            flows[on] = [f.cpu() for f in kept]
            _close(outs[on], g["out_test"], f"{name} tiled, tiles_per_call={tpc}, fused_blend={on}", TOL)
        assert outs[True].shape == (1, 2, 60, 80) and outs[True].is_contiguous()
        if not torch.equal(_bits(outs[True]), _bits(outs[False])):
            diff = float((outs[True] - outs[False]).abs().max())
            print(f"{name} tiles_per_call={tpc}: GPU chain and kernel differ by {diff:.3e}; the CPU chain decides")
            want = blend_chain(48, 64, 60, 80, corners, tpc, 1, flows[True])
            assert torch.equal(_bits(outs[True].cpu()), _bits(want)), f"tiles_per_call={tpc}: kernel differs from the CPU chain"


def _stub_model(dev, H, W):
    from perceiverio_pytorch_amd.models import FlowPerceiver
    return FlowPerceiver(img_size=(H, W), num_latents=4, num_latent_channels=16, num_self_attends_per_block=1).to(dev).eval()


def test_fallbacks_take_the_chain(dev, monkeypatch):
    """fused_blend = False, more than 64 groups (65 tiles, one per call), flows that are views of one reused buffer, a flow
    dtype the entry does not take: no kernel call, and the result of the chain on the same flows.  _predict_patch is a stub
    that hands out random flows, so no model runs."""
    H, W, h, w, overlap = 4, 6, 39, 25, 1                         # ys: 13 corners, xs: 5 corners -> 65 tiles, none overhanging
    model = _stub_model(dev, H, W)
    corners = list(model.compute_grid_indices((h, w), overlap))
    assert len(corners) == 65 and all(y + H <= h and x + W <= w for y, x in corners)
    calls = _counting(monkeypatch)
    gen = torch.Generator(device="cpu").manual_seed(3)
    pool = {}

    def run(tpc, fused, mode="fresh"):
        """test_mode forward with stubbed flows: (result, the flows handed out)."""
        model.tiles_per_call, model.fused_blend = tpc, fused
        handed = []

        def predict(tiles):
            k = int(tiles[0, 0, 0, 0, 0].item()) // tpc        # (the frames number the corners: which group this is)
            v = pool.setdefault((tpc, k), torch.randn(tiles.shape[0], H, W, 2, generator=gen)).to(dev)
            if mode == "reused":                      # every group a view of ONE buffer
                buf = pool.setdefault("buf", torch.empty(tpc, H, W, 2, device=dev))
                buf[:v.shape[0]].copy_(v)
                v = buf[:v.shape[0]]
            elif mode == "double":
                v = v.double()
            handed.append(v.permute(0, 3, 1, 2))
            return handed[-1]
        monkeypatch.setattr(model, "_predict_patch", predict)
        frames = torch.zeros(1, 3, h, w, device=dev)
        for i, (y, x) in enumerate(corners):
            frames[0, 0, y, x] = i
        with torch.inference_mode():
            return model(frames, frames, test_mode=True, min_overlap=overlap), handed

    # the fused path itself on this geometry: 17 groups of 4
    out, handed = run(4, True)
    assert calls["kernel"] == 1 and len(handed) == 17
    want = blend_chain(H, W, h, w, corners, 4, 1, [f.cpu() for f in handed])
    assert torch.equal(_bits(out.cpu()), _bits(want))
    # the switch
    off, handed = run(4, False)
    assert calls["kernel"] == 1 and len(handed) == 17
    assert torch.equal(_bits(off), _bits(blend_chain(H, W, h, w, corners, 4, 1, handed)))
    # 65 groups: beyond the entry's table
    out65, handed = run(1, True)
    assert calls["kernel"] == 1 and len(handed) == 65
    ref65, _ = run(1, False)
    assert calls["kernel"] == 1 and torch.equal(_bits(out65), _bits(ref65))
    # 64 groups fit: two tiles per call make 33
    out2, handed = run(2, True)
    assert calls["kernel"] == 2 and len(handed) == 33
    assert torch.equal(_bits(out2.cpu()), _bits(blend_chain(H, W, h, w, corners, 2, 1, [f.cpu() for f in handed])))
    # views of one reused buffer are noticed (the fused attempt stops at the second group; the chain starts over)
    before = calls["kernel"]
    reused, handed = run(4, True, mode="reused")
    assert calls["kernel"] == before and len(handed) == 2 + 17
    ref, _ = run(4, False, mode="reused")
    assert torch.equal(_bits(reused), _bits(ref))
    # another dtype
    dbl, handed = run(4, True, mode="double")
    assert calls["kernel"] == before and dbl.dtype == torch.float64 and len(handed) == 1 + 17


def test_fused_blend_in_a_graph(dev, monkeypatch):
    """No host tensor, no copy to the device, no synchronisation: a test_mode forward with the fused blend (stubbed flows)
    captures into a graph, and the replay equals the eager result."""
    H, W, h, w = 8, 12, 13, 21
    model = _stub_model(dev, H, W)
    corners = list(model.compute_grid_indices((h, w), 3))
    src = torch.randn(len(corners), H, W, 2, device=dev)
    calls = _counting(monkeypatch)
    state = {"i": 0}

    def predict(tiles):
        i = state["i"]
        state["i"] += tiles.shape[0]
        return (src[i:i + tiles.shape[0]] * 0.5).permute(0, 3, 1, 2)
    monkeypatch.setattr(model, "_predict_patch", predict)
    frames = torch.zeros(1, 3, h, w, device=dev)
    model.tiles_per_call = 4
    with torch.inference_mode():
        eager = model(frames, frames, test_mode=True, min_overlap=3)
        assert calls["kernel"] == 1
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        state["i"] = 0
        with torch.cuda.graph(graph):
            captured = model(frames, frames, test_mode=True, min_overlap=3)
        assert calls["kernel"] == 2
        src.mul_(-2.0)
        graph.replay()
        torch.cuda.synchronize()
        state["i"] = 0
        again = model(frames, frames, test_mode=True, min_overlap=3)
    assert torch.equal(_bits(captured), _bits(again)) and not torch.equal(_bits(again), _bits(eager))
