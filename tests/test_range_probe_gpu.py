"""GPU: the range probe -- absmax16_kernel through pio_absmax16 against torch on the very same device buffer (exact: a
max involves no rounding) inside +inf fences, the hooks of the block entry points (pio_range_probe_begin / _mark / _end)
against the CPU plumbing backend's figures, overflow seen under fp16 and cured under bf16, recommend_operand_dtype on a
small PerceiverIO, the LayerNorm-folded route, and both probes together."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import range_probe_cases as RC

pytestmark = pytest.mark.gpu

_probe_started = False      # set by everything below that starts a range probe in this process


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import perceiverio_pytorch_amd as P
    assert P.lib().pio_arch_ok() == 1
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _ambient_policy():
    """The raw modules run under the ambient precision policy: pin it (other test modules may have left another one)."""
    from perceiverio_pytorch_amd import runtime as R
    with R.precision("fp16x3"):
        yield


def _tdt(name):
    return torch.float16 if name == "f16" else torch.bfloat16


# ---- block builders (used by the module-level baseline below) ------------------------------------------------------------
def _build_block(name):
    """(module on the CPU, inputs on the CPU, mask or None) of one RC.BLOCKS case."""
    from perceiverio_pytorch_amd.transformer_primitives import CrossAttention, SelfAttention
    c = RC.BLOCKS[name]
    torch.manual_seed(sum(map(ord, name)))
    if c["kind"] == "self":
        m = SelfAttention(c["D"], widening_factor=1, num_heads=c["H"]).eval()
        with torch.no_grad():
            m.layer_norm1.weight.uniform_(0.5, 3.0)
            m.layer_norm2.weight.uniform_(0.5, 3.0)
        return m, (torch.randn(c["B"], c["N"], c["D"]) * 2,), None
    m = CrossAttention(q_in_channels=c["Cq"], kv_in_channels=c["Ckv"], num_heads=c["H"]).eval()
    with torch.no_grad():
        m.layer_norm_kv.weight.uniform_(0.5, 3.0)
    mask = None
    if c["mask"]:
        km = torch.rand(c["B"], c["Tk"]) > 0.3
        km[:, 0] = True
        mask = km[:, None, :].expand(c["B"], c["Tq"], c["Tk"]).contiguous()
    return m, (torch.randn(c["B"], c["Tq"], c["Cq"]) * 2, torch.randn(c["B"], c["Tk"], c["Ckv"]) * 2), mask


def _run_block(dev, m_dev, ins_dev, mask_dev, policy, probe_records=0):
    """One forward of the module through its C entry point under the launch profiler; probe_records > 0: under the range
    probe as well.  Returns (output, [(part, kind, figure)], records seen, launches per profiler class)."""
    global _probe_started
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L, probe as LP, runtime as R
    lib = P.lib()
    prev = R.get_precision_policy()
    P.set_precision_policy(policy)
    try:
        kw = dict(attention_mask=mask_dev) if mask_dev is not None else {}
        m_dev(*ins_dev, **kw)                            # (packs the weights, sizes the workspace: not profiled)
        rec = torch.zeros(64, dtype=torch.float32, device=dev)
        parts, kinds = (C.c_int32 * 64)(), (C.c_int32 * 64)()
        torch.cuda.synchronize()
        L.check(lib.pio_prof_begin(256), "pio_prof_begin")
        n = 0
        if probe_records:
            _probe_started = True
            L.check(lib.pio_range_probe_begin(rec.data_ptr(), probe_records), "pio_range_probe_begin")
        try:
            out = m_dev(*ins_dev, **kw)
        finally:
            if probe_records:
                n = lib.pio_range_probe_end(parts, kinds, 64)
            launches = (C.c_int64 * 9)()
            assert lib.pio_prof_end(None, None, None, launches) >= 0
        torch.cuda.synchronize()
        vals = rec.cpu().tolist()
        records = [(LP.RANGE_PARTS[parts[i]], LP.RANGE_KINDS[kinds[i]], vals[i]) for i in range(min(n, probe_records))]
        assert vals[min(n, probe_records):] == [0.0] * (64 - min(n, probe_records)), "a record past the count was written"
        return out, records, n, list(launches)
    finally:
        P.set_precision_policy(prev)


def _cpu_records(m, ins, mask):
    """The CPU plumbing backend's records of the same forward (fp32: the true magnitudes)."""
    import perceiverio_pytorch_amd as P
    P.set_backend("torch")
    try:
        with P.range_probe() as probe:
            out = m(*ins, **(dict(attention_mask=mask) if mask is not None else {}))
    finally:
        P.set_backend("hip")
    return probe.records, out


@pytest.fixture(scope="module")
def pristine(dev):
    """Launch counts and outputs of every block case BEFORE any range probe has been started in this process (the first
    thing this module does on the device: every test below that starts a probe depends on this fixture)."""
    assert not _probe_started, "the baseline must be taken before the first pio_range_probe_begin of the process"
    base = {}
    for name in sorted(RC.BLOCKS):
        m, ins, mask = _build_block(name)
        m_dev, ins_dev = copy.deepcopy(m).to(dev), tuple(t.to(dev) for t in ins)
        mask_dev = mask.to(dev) if mask is not None else None
        for policy in RC.POLICIES:
            out, _, _, launches = _run_block(dev, m_dev, ins_dev, mask_dev, policy)
            base[name, policy] = (out.clone(), launches)
    return base


# ---- raw primitive ---------------------------------------------------------------------------------------------------
def _absmax16(dev, dtype, buf, lay, absmax):
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L
    code = P.lib().pio_absmax16(L.PIO_DT_F16 if dtype == "f16" else L.PIO_DT_BF16, buf.data_ptr() + 2 * lay["base"],
                                lay["rows"], lay["cols"], lay["ld"], lay["batch"], lay["stride_b"], absmax.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream)
    L.check(code, "pio_absmax16")


def _measure(dev, dtype, buf, lay, preset=0.0):
    out = torch.full((1,), preset, dtype=torch.float32, device=dev)
    _absmax16(dev, dtype, buf, lay, out)
    return float(out.item())


def _torch_max(buf, lay):
    """torch on the same device buffer: the strided view of exactly the elements pio_absmax16 may read."""
    v = torch.as_strided(buf, (lay["nb"], lay["rows"], lay["cols"]), (lay["stride_b"], lay["ld"], 1), lay["base"])
    return float(v.float().abs().max().item())


@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("shape", RC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_absmax16_vs_torch_inside_inf_fences(dev, shape, dtype):
    for li, name in enumerate(sorted(RC.LAYOUTS)):
        lay = RC.layout(shape, name)
        assert lay["base"] >= RC.FENCE and lay["base"] + (lay["nb"] - 1) * lay["stride_b"] + lay["rows"] * lay["ld"] \
            + RC.FENCE == lay["total"]                  # (bounds of everything handed to the kernel)
        host = torch.from_numpy(RC.fill(lay, seed=17 * li + shape[1])).to(_tdt(dtype))
        buf = host.to(dev)
        assert buf.data_ptr() % 16 == 0
        tag = f"{shape} {name} {dtype}"
        # the data alone: finite (nothing outside the extent was read) and exactly torch's figure
        ref = _torch_max(buf, lay)
        got = _measure(dev, dtype, buf, lay)
        assert np.isfinite(got) and got == ref and 0 < ref < 20, (tag, got, ref)
        # the maximum, negative, planted at each of the four positions in turn
        for pos in RC.plant_positions(lay):
            b2 = buf.clone()
            b2[RC.index(lay, *pos)] = RC.PLANT
            assert _torch_max(b2, lay) == -RC.PLANT
            assert _measure(dev, dtype, b2, lay) == -RC.PLANT, (tag, pos)
        # one NaN anywhere gives inf, and so does one -inf
        mid = RC.index(lay, lay["nb"] - 1, lay["rows"] // 2, lay["cols"] // 2)
        for bad in (float("nan"), float("-inf")):
            b2 = buf.clone()
            b2[mid] = bad
            assert _measure(dev, dtype, b2, lay) == float("inf"), (tag, bad)
        # two calls into one word max-merge, in either order
        b2 = buf.clone()
        b2[RC.index(lay, *RC.plant_positions(lay)[1])] = RC.PLANT
        word = torch.zeros(1, dtype=torch.float32, device=dev)
        _absmax16(dev, dtype, b2, lay, word)
        _absmax16(dev, dtype, buf, lay, word)
        assert float(word.item()) == -RC.PLANT, tag
        word.zero_()
        _absmax16(dev, dtype, buf, lay, word)
        assert float(word.item()) == ref
        _absmax16(dev, dtype, b2, lay, word)
        assert float(word.item()) == -RC.PLANT, tag
        # an all-zero buffer leaves a pre-set 3.0 untouched
        zero = torch.from_numpy(RC.fill(lay, seed=0, zero=True)).to(_tdt(dtype)).to(dev)
        assert _measure(dev, dtype, zero, lay, preset=3.0) == 3.0, tag


def test_argument_errors_return_the_documented_codes(dev):
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import _lib as L
    lib = P.lib()
    x = torch.full((4096,), 7.0, dtype=torch.float16, device=dev)
    o = torch.zeros(1, dtype=torch.float32, device=dev)
    p, op = x.data_ptr(), o.data_ptr()
    assert lib.pio_absmax16(L.PIO_DT_F16, None, 4, 8, 8, 1, 0, op, 0) == -6        # PIO_E_ARG: NULL
    assert lib.pio_absmax16(L.PIO_DT_F16, p, 4, 8, 8, 1, 0, None, 0) == -6
    assert lib.pio_absmax16(7, p, 4, 8, 8, 1, 0, op, 0) == -6                      # unknown dtype
    assert lib.pio_absmax16(L.PIO_DT_F16, p, 4, 9, 8, 1, 0, op, 0) == -1           # PIO_E_SHAPE: cols > ld, rows > 1
    assert lib.pio_absmax16(L.PIO_DT_F16, p, -1, 8, 8, 1, 0, op, 0) == -1          # negative extents
    assert lib.pio_absmax16(L.PIO_DT_F16, p, 4, -8, 8, 1, 0, op, 0) == -1
    assert lib.pio_absmax16(L.PIO_DT_F16, p, 4, 8, 8, -1, 0, op, 0) == -1
    assert lib.pio_absmax16(L.PIO_DT_F16, p, 0, 8, 8, 1, 0, op, 0) == 0            # empty extents: PIO_OK, nothing launched
    assert lib.pio_absmax16(L.PIO_DT_F16, p, 4, 0, 8, 1, 0, op, 0) == 0
    assert lib.pio_absmax16(L.PIO_DT_F16, p, 4, 8, 8, 0, 0, op, 0) == 0
    assert lib.pio_range_probe_begin(None, 4) == -6 and lib.pio_range_probe_begin(op, 0) == -6
    assert lib.pio_range_probe_mark(4) == -6 and lib.pio_range_probe_mark(-1) == -6
    assert lib.pio_range_probe_end(None, None, 0) == 0                             # not active
    torch.cuda.synchronize()
    assert float(o.item()) == 0.0, "an argument error must not launch"
    assert lib.pio_absmax16(L.PIO_DT_F16, p, 1, 9, 8, 1, 0, op, 0) == 0            # (one row: cols > ld is legal)
    torch.cuda.synchronize()
    assert float(o.item()) == 7.0


# ---- block level -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", RC.POLICIES)
@pytest.mark.parametrize("name", sorted(RC.BLOCKS))
def test_block_hooks_change_nothing_and_agree_with_the_cpu_backend(dev, pristine, name, policy):
    m, ins, mask = _build_block(name)
    m_dev, ins_dev = copy.deepcopy(m).to(dev), tuple(t.to(dev) for t in ins)
    mask_dev = mask.to(dev) if mask is not None else None
    out0, launches0 = pristine[name, policy]
    out_on, records, n, launches_on = _run_block(dev, m_dev, ins_dev, mask_dev, policy, probe_records=64)
    out_off, rec_off, n_off, launches_off = _run_block(dev, m_dev, ins_dev, mask_dev, policy)
    cpu, out_cpu = _cpu_records(m, ins, mask)
    print(f"{name} [{policy}]: launches {launches_on}")
    assert torch.isfinite(out0).all()
    assert torch.equal(out_on, out0) and torch.equal(out_off, out0), "the probe changed the block's output"
    assert launches_on == launches0, "the probe changed what the block launches (profiled classes)"
    assert launches_off == launches0 and n_off == 0 and rec_off == [], "something stayed behind after pio_range_probe_end"
    assert n == len(records) and {p for p, _, _ in records} == {"attention"}
    pairs = RC.align(records, cpu)
    for part, kind, got, ref in pairs:
        rel = abs(got - ref) / ref
        print(f"  {kind:7s} hip {got:.6g} cpu {ref:.6g} rel {rel:.2e}")
    for part, kind, got, ref in pairs:
        assert np.isfinite(got) and ref > 0 and abs(got - ref) <= RC.FIGURE_RTOL * ref, (name, policy, kind, got, ref)
    # records past max_records are counted, not recorded
    _, few, n_few, _ = _run_block(dev, m_dev, ins_dev, mask_dev, policy, probe_records=3)
    assert n_few == n and few == records[:3]


def _overflowing_self_attention():
    """The "self" block with ln2's gain and fc1's weights scaled so that the hidden activations leave fp16's range."""
    m, ins, _ = _build_block("self")
    with torch.no_grad():
        m.layer_norm2.weight.mul_(300.0)
        m.mlp.fc1.weight.mul_(180.0)
    return m, ins


@pytest.mark.parametrize("policy", RC.POLICIES)
def test_overflow_is_seen_under_fp16_and_cured_under_bf16(dev, pristine, policy):
    m, ins = _overflowing_self_attention()
    cpu, out_cpu = _cpu_records(m, ins, None)
    hidden_cpu = [v for _, k, v in cpu if k == "hidden"]
    lo, hi = RC.OVERFLOW_WINDOW
    print(f"CPU-backend hidden abs-max {hidden_cpu}")
    assert len(hidden_cpu) == 1 and lo < hidden_cpu[0] < hi, hidden_cpu
    assert torch.isfinite(out_cpu).all()
    m_dev, ins_dev = copy.deepcopy(m).to(dev), tuple(t.to(dev) for t in ins)
    out, records, n, _ = _run_block(dev, m_dev, ins_dev, None, policy, probe_records=64)
    hidden = [v for _, k, v in records if k == "hidden"]
    print(f"[{policy}] hidden record {hidden} output finite: {bool(torch.isfinite(out).all())}")
    assert len(hidden) == 1
    if policy == "fp16x3":
        assert hidden[0] == float("inf") and not torch.isfinite(out).all()
    else:
        assert np.isfinite(hidden[0]) and abs(hidden[0] - hidden_cpu[0]) <= RC.FIGURE_RTOL * hidden_cpu[0]
        assert torch.isfinite(out).all()
        for part, kind, got, ref in RC.align(records, cpu):
            assert abs(got - ref) <= RC.FIGURE_RTOL * ref, (kind, got, ref)


# ---- encoder + decoder -----------------------------------------------------------------------------------------------
def _small_io():
    from perceiverio_pytorch_amd.output_queries import TrainableQuery
    from perceiverio_pytorch_amd.perceiver import PerceiverIO
    torch.manual_seed(11)
    model = PerceiverIO(num_blocks=1, num_self_attends_per_block=2, num_latents=8, num_latent_channels=64,
                        input_channels=24, final_project_out_channels=5,
                        perceiver_encoder_kwargs=dict(num_self_attend_heads=2, num_cross_attend_heads=1),
                        output_queries=TrainableQuery(output_index_dims=4, num_channels=64)).eval()
    return model, torch.randn(2, 32, 24)


def test_perceiver_io_parts_in_order_and_python_api(dev, pristine):
    global _probe_started
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import probe as LP
    model, x = _small_io()
    cpu, _ = _cpu_records(model, (x,), None)
    model_dev, x_dev = copy.deepcopy(model).to(dev), x.to(dev)
    y0 = model_dev(x_dev)
    _probe_started = True
    with P.range_probe() as probe:
        y1 = model_dev(x_dev)
    parts = [p for p, _, _ in probe.records]
    assert parts == sorted(parts, key=("cross", "stack", "decoder").index) and set(parts) == {"cross", "stack", "decoder"}
    assert probe.calls == len(probe.records) == 8 + 2 * 7 + 9
    assert [k for p, k, _ in probe.records if p == "decoder"][-1] == "stream"
    assert torch.equal(y0, y1) and torch.equal(y0, model_dev(x_dev))
    for part, kind, got, ref in RC.align(probe.records, cpu):
        assert abs(got - ref) <= RC.FIGURE_RTOL * ref, (part, kind, got, ref)
    assert probe.worst() == {p: max(d.values()) for p, d in probe.by_part().items()}
    # the part is back at "attention" behind the encoder / decoder calls
    with P.range_probe() as probe:
        model_dev._encoder.self_attends[0](y1.new_zeros(1, 8, 64))
    assert {p for p, _, _ in probe.records} == {"attention"} and probe.calls == 7
    # life-cycle on the HIP backend: one at a time, nothing active after an exception, no start during stream capture
    with P.range_probe():
        with pytest.raises(P.PioError, match="already active"):
            with P.range_probe():
                pass
    with pytest.raises(ZeroDivisionError):
        with P.range_probe():
            1 / 0
    assert not LP.range_active() and P.lib().pio_range_probe_end(None, None, 0) == 0
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        model_dev(x_dev)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        with pytest.raises(P.PioError, match="stream capture"):
            with P.range_probe():
                pass
        model_dev(x_dev)
    assert not LP.range_active() and P.lib().pio_range_probe_end(None, None, 0) == 0


def test_recommendation_changes_only_the_decoder_and_the_forward_is_finite_under_it(dev, pristine):
    global _probe_started
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import runtime as R
    from perceiverio_pytorch_amd.models import split_policy3
    model, x = _small_io()
    ca = model._decoder.decoding_cross_attn
    with torch.no_grad():
        ca.layer_norm2.weight.mul_(300.0)
        ca.mlp.fc1.weight.mul_(480.0)
    cpu, _ = _cpu_records(model, (x,), None)
    hidden_cpu = [v for p, k, v in cpu if (p, k) == ("decoder", "hidden")]
    lo, hi = RC.OVERFLOW_WINDOW
    assert len(hidden_cpu) == 1 and lo < hidden_cpu[0] < hi, hidden_cpu
    model_dev, x_dev = copy.deepcopy(model).to(dev), x.to(dev)
    assert R.get_precision_policy() == "fp16x3"
    assert not torch.isfinite(model_dev(x_dev)).all()
    _probe_started = True
    policy, report = P.recommend_operand_dtype(model_dev, x_dev)
    print(f"{report['absmax']} -> {policy}")
    assert report["absmax"]["decoder"]["hidden"] == float("inf") and report["policy"] == "fp16x3"
    assert report["limit"] == 65504.0 and report["calls"] == 8 + 2 * 7 + 9
    assert policy == "fp16x3/fp16x3/bf16x3"
    assert R.get_precision_policy() == "fp16x3" and model_dev.decoder_policy is None      # (nothing is set)
    cross, stack, dec = split_policy3(policy)
    model_dev.decoder_policy = dec
    model_dev._encoder.cross_attend_policy = cross
    with R.precision(stack):
        y = model_dev(x_dev)
        again, _ = P.recommend_operand_dtype(model_dev, x_dev)
    assert torch.isfinite(y).all()
    assert again == policy                               # (finite now, still beyond fp16: the same answer)


# ---- the LayerNorm-folded route ------------------------------------------------------------------------------------------
def test_ln_folded_stack_yields_stream_records_and_identical_outputs(dev, pristine):
    """512 rows of 512 channels: the smallest stack the tile-kernel fold takes in its automatic mode."""
    global _probe_started
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import runtime as R
    from perceiverio_pytorch_amd.perceiver import PerceiverEncoder
    lib = P.lib()
    torch.manual_seed(21)
    enc = PerceiverEncoder(40, 2, 1, 512, 512, num_self_attend_heads=8).to(dev).eval()
    x = torch.randn(1, 60, 40, device=dev)
    prev_policy = R.get_precision_policy()
    prev = lib.pio_ln_fold_enable(2)
    try:
        P.set_precision_policy("fp16")
        y0 = enc(x, enc.latents(x)).clone()
        _probe_started = True
        with P.range_probe() as probe:
            y1 = enc(x, enc.latents(x)).clone()
        y2 = enc(x, enc.latents(x)).clone()
        lib.pio_ln_fold_enable(0)
        with P.range_probe() as unfolded:
            enc(x, enc.latents(x))
    finally:
        lib.pio_ln_fold_enable(prev)
        P.set_precision_policy(prev_policy)
    stack = [k for p, k, _ in probe.records if p == "stack"]
    print(f"folded stack kinds: {stack}")
    assert torch.isfinite(y0).all() and torch.equal(y1, y0) and torch.equal(y2, y0)
    assert stack == ["stream", "q", "attn", "stream", "hidden", "stream"] + ["q", "attn", "stream", "hidden", "stream"]
    assert all(np.isfinite(v) and v > 0 for _, _, v in probe.records)
    assert "stream" not in [k for p, k, _ in unfolded.records if p == "stack"], "the fold was not what made the records"
    assert [p for p, _, _ in probe.records][:1] == ["cross"] and {p for p, _, _ in probe.records} == {"cross", "stack"}


# ---- both probes ---------------------------------------------------------------------------------------------------------
def test_both_probes_together_leave_the_logit_records_unchanged(dev, pristine):
    global _probe_started
    import perceiverio_pytorch_amd as P
    model, x = _small_io()
    model, x = model.to(dev), x.to(dev)
    with P.logit_probe() as alone:
        y0 = model(x)
    _probe_started = True
    with P.logit_probe() as logits, P.range_probe() as ranges:
        y1 = model(x)
    with P.range_probe() as ranges_alone:
        model(x)
    assert logits.records == alone.records and logits.calls == alone.calls == 4
    assert ranges.records == ranges_alone.records and ranges.calls == 8 + 2 * 7 + 9
    assert torch.equal(y0, y1)
