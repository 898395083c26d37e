"""CPU: what the fused I/O planners share (fused_io.gate / rows / param_row / place) and the one launch helper
(runtime.call), each against what it promises its callers."""
import contextlib
import ctypes

import pytest
import torch


def test_rows_returns_the_tensor_or_a_copy_exactly_as_each_option_demands():
    from perceiverio_pytorch_amd import fused_io as FIO
    base = torch.arange(64 * 12, dtype=torch.float32).reshape(64, 12)
    assert base.data_ptr() % 16 == 0

    def same(t, **kw):
        r = FIO.rows(t, **kw)
        if r is t:
            return True
        assert torch.equal(r, t) and r.is_contiguous() and not r.requires_grad and r.data_ptr() != t.data_ptr()
        return False

    every = dict(min_stride=True, stride4=True, aligned=True)
    assert same(base) and same(base, **every)                              # contiguous: never copied
    assert same(torch.nn.Parameter(base), **every) and same(base[3])       # a parameter; a 1-D array (index points)
    assert not same(base[:, ::2]) and not same(base[:, ::2], **every)      # last stride 2: always copied
    assert not same(torch.nn.Parameter(base)[:, ::2])                      # ... detached from autograd
    short = base[:1].expand(5, 12)                                         # row stride 0 < 12: overlapping rows
    assert same(short) and same(short, stride4=True, aligned=True) and not same(short, min_stride=True)
    odd = torch.as_strided(base, (20, 8), (13, 1))                         # row stride 13
    assert same(odd, min_stride=True, aligned=True) and not same(odd, stride4=True)
    assert FIO.rows(odd, stride4=True).stride() == (8, 1)
    off = base[:, 1:9]                                                     # row stride 12, pointer 4 bytes past alignment
    assert off.data_ptr() % 16 == 4
    assert same(off, min_stride=True, stride4=True) and not same(off, aligned=True)
    assert FIO.rows(off, aligned=True).data_ptr() % 16 == 0


def test_param_row_declines_what_is_not_a_one_by_width_fp32_parameter_on_the_device():
    from perceiverio_pytorch_amd import fused_io as FIO
    cpu = torch.device("cpu")
    p = torch.nn.Parameter(torch.randn(1, 6))
    assert FIO.param_row(p, 6, cpu) is p                                                    # read where it is
    wide = torch.nn.Parameter(torch.randn(1, 12))
    got = FIO.param_row(wide[:, ::2], 6, cpu)                                               # channel stride 2: a copy
    assert torch.equal(got, wide[:, ::2]) and not got.requires_grad and got.is_contiguous()
    assert FIO.param_row(p, 5, cpu) is False and FIO.param_row(p[0], 6, cpu) is False       # wrong width; wrong rank
    assert FIO.param_row(torch.randn(2, 6), 6, cpu) is False                                # two rows
    assert FIO.param_row(p.double(), 6, cpu) is False                                       # wrong dtype
    assert FIO.param_row(torch.empty(1, 6, device="meta"), 6, cpu) is False                 # wrong device
    assert FIO.param_row(torch.zeros(1, 0), 0, cpu) is None                                 # zero width: no pointer
    assert FIO.param_row(torch.zeros(1, 0), -1, cpu) is False and FIO.param_row(torch.zeros(1, 0).double(), 0, cpu) is False


def test_place_assigns_row0_in_sorted_name_order_and_declines_at_2_to_the_31():
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd import fused_io as FIO

    def segs(kind, sizes):
        out = {}
        for i, (m, n) in enumerate(sizes.items()):
            out[m] = kind()
            out[m].M, out[m].kind = n, i
        return out

    for kind in (L.TokenSegment, L.QuerySegment):
        plan = segs(kind, {"video": 7, "audio": 5, "label": 1})            # given unsorted
        arr, total = FIO.place(plan)
        assert isinstance(arr, kind * 3) and total == 13
        assert [(s.kind, s.M, s.row0) for s in arr] == [(1, 5, 0), (2, 1, 5), (0, 7, 6)]       # audio, label, video
        assert {m: s.row0 for m, s in plan.items()} == {"video": 6, "audio": 0, "label": 5}    # the caller's own too
    arr, total = FIO.place(segs(L.TokenSegment, {"c": 2 ** 30, "a": 2 ** 30, "b": 0}))
    assert arr is None and total == 2 ** 31
    arr, total = FIO.place(segs(L.TokenSegment, {"c": 2 ** 30, "a": 2 ** 30 - 1, "b": 0}))
    assert total == 2 ** 31 - 1 and [s.row0 for s in arr] == [0, 2 ** 30 - 1, 2 ** 30 - 1]


def test_gate_reads_the_switch_the_backend_and_the_tensors_own_is_cuda():
    import perceiverio_pytorch_amd as P
    from perceiverio_pytorch_amd import fused_io as FIO

    class FakeCuda(torch.Tensor):
        @property
        def is_cuda(self):
            return True
    x = torch.zeros(2, 3)
    fx, ids = x.as_subclass(FakeCuda), torch.zeros(2, 3, dtype=torch.int64).as_subclass(FakeCuda)
    assert P.get_backend() == "hip"
    assert FIO.gate(True) and not FIO.gate(False) and not FIO.gate(False, fx)
    assert FIO.gate(True, fx) and FIO.gate(1, fx, fx)
    assert not FIO.gate(True, x) and not FIO.gate(True, fx, x)                       # a CPU tensor
    assert not FIO.gate(True, None) and not FIO.gate(True, [fx])                     # not a tensor
    assert not FIO.gate(True, ids) and not FIO.gate(True, fx.double().as_subclass(FakeCuda))
    assert FIO.gate(True, ids, dtypes=(torch.int32, torch.int64)) and FIO.gate(True, ids, dtypes=None)
    P.set_backend("torch")
    try:
        assert not FIO.gate(True) and not FIO.gate(True, fx)
    finally:
        P.set_backend("hip")


def test_call_appends_the_stream_labels_errors_and_honours_the_stand_ins(monkeypatch):
    from perceiverio_pytorch_amd import _lib as L
    from perceiverio_pytorch_amd import runtime as R
    seen, entered = [], []

    class _Lib:
        code = 0

        def pio_thing(self, *a):
            seen.append(a)
            return self.code
    lib = _Lib()

    @contextlib.contextmanager
    def on_device(dev):
        entered.append(("in", dev))
        try:
            yield
        finally:
            entered.append(("out", dev))
    monkeypatch.setattr(L, "lib", lambda: lib)
    monkeypatch.setattr(R, "on_device", on_device)
    monkeypatch.setattr(R, "stream_ptr", lambda dev: ("stream of", dev))
    p = ctypes.c_int(3)
    assert R.call("dev0", "pio_thing", 1, None, p) is True
    assert seen == [(1, None, p, ("stream of", "dev0"))]                     # the arguments in order, then the stream
    assert entered == [("in", "dev0"), ("out", "dev0")]                      # inside the patched on_device
    assert R.call("dev0", "pio_thing", 1, stream=77) is True and seen[-1] == (1, 77)                # a given stream
    with pytest.raises(AttributeError):
        R.call("dev0", "pio_missing")                                        # a missing entry point is an error
    lib.code = -1
    with pytest.raises(L.PioError, match=r"^pio_thing: PIO_E_SHAPE$"):
        R.call("dev0", "pio_thing")
    assert R.call("dev0", "pio_thing", 5, declines=(-1, -2)) is False and seen[-1] == (5, ("stream of", "dev0"))
    lib.code = -5
    with pytest.raises(L.PioError, match=r"^pio_thing: PIO_E_LAUNCH$"):
        R.call("dev0", "pio_thing", declines=(-1, -2))                       # only the listed codes decline
    assert entered.count(("in", "dev0")) == entered.count(("out", "dev0"))   # left again after every raise
