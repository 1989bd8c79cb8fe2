"""The guarded allocator of tests/guarded_alloc.py, checked on the CPU device."""
import os

import pytest
import torch

from tests import guarded_alloc as ga
from tests.guarded_alloc import ALIGN, FILL, RED, guarded

# torch.empty / empty_like / zeros / zeros_like / new_empty / new_zeros calls in fastvocoder_amd/**/*.py.
# A change of this number means an allocation site came or went: look at test_gpu_guarded.py's
# coverage test and its allow-list, then update it.
PROJECT_SITES = 136


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _block_of(g, t):
    (a,) = [a for a in g.allocations if a.view is t]
    return a


def test_empty_body_is_nan_and_zones_are_ff():
    with guarded("cpu") as g:
        x = torch.empty(3, 5)
        a = _block_of(g, x)
        assert x.shape == (3, 5) and x.dtype == torch.float32 and x.is_contiguous()
        assert torch.isnan(x).all()
        assert a.nbytes == 60 and a.block.numel() == RED + ALIGN + RED and a.block.dtype == torch.uint8
        assert x.data_ptr() == a.block.data_ptr() + RED
        assert (a.block[:RED] == FILL).all() and (a.block[RED + 60:] == FILL).all()
        assert g.check() == []


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float64])
def test_ff_bytes_are_nan_in_every_float_format(dtype):
    with guarded("cpu"):
        x = torch.empty(7, dtype=dtype)
        assert torch.isnan(x).all()


def test_zeros_zeroes_the_body_only():
    with guarded("cpu") as g:
        z = torch.zeros(2, 3, dtype=torch.float64)
        a = _block_of(g, z)
        assert (z == 0).all() and a.nbytes == 48
        assert (a.block[:RED] == FILL).all() and (a.block[RED + 48:] == FILL).all()
        zl = torch.zeros_like(z)
        assert (zl == 0).all() and zl.dtype == torch.float64 and zl.shape == z.shape
        assert g.check() == []


def test_call_forms():
    with guarded("cpu") as g:
        src = torch.ones(4, 2, dtype=torch.float16)
        got = [
            (torch.empty(2, 3), (2, 3), torch.float32),
            (torch.empty((2, 3)), (2, 3), torch.float32),
            (torch.empty([2, 3]), (2, 3), torch.float32),
            (torch.empty(torch.Size((2, 3))), (2, 3), torch.float32),
            (torch.empty(size=(2, 3)), (2, 3), torch.float32),
            (torch.empty(()), (), torch.float32),
            (torch.empty(0), (0,), torch.float32),
            (torch.empty(5, dtype=None, device=None), (5,), torch.float32),       # as nn modules pass them
            (torch.empty((5, 1), dtype=None, device=None), (5, 1), torch.float32),
            (torch.zeros(2, 3), (2, 3), torch.float32),
            (torch.zeros((2, 3), dtype=torch.float64, device="cpu"), (2, 3), torch.float64),
            (torch.zeros((), dtype=torch.float32, device=torch.device("cpu")), (), torch.float32),
            (torch.empty_like(src), (4, 2), torch.float16),
            (torch.empty_like(src, dtype=torch.float32), (4, 2), torch.float32),
            (torch.zeros_like(src), (4, 2), torch.float16),
            (torch.zeros_like(src, memory_format=torch.preserve_format), (4, 2), torch.float16),
            (torch.zeros_like(torch.ones(2, 3, 4)[:, :, 0]), (2, 3), torch.float32),      # a strided slice: torch's is contiguous too
            (src.new_empty((3,)), (3,), torch.float16),
            (src.new_empty(3, 2), (3, 2), torch.float16),
            (src.new_zeros((1,) + tuple(src.shape[1:])), (1, 2), torch.float16),
            (src.new_zeros(2, dtype=torch.int32), (2,), torch.int32),
        ]
        assert len(g.allocations) == len(got) and g.passed == []
        for t, shape, dtype in got:
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device.type == "cpu"
            assert t.numel() == 0 or t.data_ptr() == _block_of(g, t).block.data_ptr() + RED
        assert g.check() == []


@pytest.mark.parametrize("dtype,poisoned", [(torch.uint8, 255), (torch.int16, -1), (torch.int32, -1), (torch.int64, -1)])
def test_integer_types(dtype, poisoned):
    with guarded("cpu") as g:
        x = torch.empty(9, dtype=dtype)
        z = torch.zeros((3, 3), dtype=dtype)
        assert x.dtype == dtype and (x == poisoned).all()
        assert z.dtype == dtype and (z == 0).all()
        assert _block_of(g, x).nbytes == 9 * x.element_size()
        assert g.check() == []


def test_nn_module_and_autograd_work_through_it():
    torch.manual_seed(0)
    ref = torch.nn.Linear(5, 3)
    x = torch.randn(4, 5)
    want = ref(x).sum()
    want.backward()
    with guarded("cpu") as g:
        lin = torch.nn.Linear(5, 3)              # allocates with dtype=None, device=None
        lin.load_state_dict(ref.state_dict())
        y = lin(g.place(x)).sum()
        y.backward()
        assert len(g.allocations) >= 3
        assert g.check() == []
    assert torch.equal(y, want) and torch.equal(lin.weight.grad, ref.weight.grad)


def test_a_write_before_or_after_the_view_is_reported_with_its_site():
    with guarded("cpu") as g:
        clean = torch.empty(10)
        before = torch.empty(10)
        after = torch.zeros(10)
        clean[:] = 1.0                                            # inside the view: not reported
        clean[9] = 2.0
        assert g.check() == []
        blk = _block_of(g, before).block
        blk[RED - 1] = 0                                           # one element before the start
        found = g.check()
        assert [f.view.data_ptr() for f in found] == [before.data_ptr()]
        blk = _block_of(g, after).block
        blk.view(torch.float32)[RED // 4 + 10] = 0.0              # one float past the end
        found = g.check()
        assert sorted(f.view.data_ptr() for f in found) == sorted([before.data_ptr(), after.data_ptr()])
        for f in found:
            assert f.site.file == os.path.abspath(__file__)
            assert f.site.function == "test_a_write_before_or_after_the_view_is_reported_with_its_site"
        kinds = {f.view.data_ptr(): f.kind for f in found}
        assert kinds == {before.data_ptr(): "empty", after.data_ptr(): "zeros"}
        lines = {f.view.data_ptr(): f.site.line for f in found}
        assert lines[after.data_ptr()] == lines[before.data_ptr()] + 1
        assert str(found[0].site).startswith(os.path.join("tests", "test_guarded_alloc_host.py") + ":")


def test_a_write_into_the_alignment_pad_and_the_far_end_is_reported():
    with guarded("cpu") as g:
        x = torch.empty(3, dtype=torch.int16)                      # 6 bytes of body, 250 of pad
        blk = _block_of(g, x).block
        blk[RED + 5] = 0                                           # last body byte
        assert g.check() == []
        blk[RED + 6] = 0                                           # first pad byte
        assert len(g.check()) == 1
    with guarded("cpu") as g:
        x = torch.empty(64)
        _block_of(g, x).block[-1] = 1
        assert len(g.check()) == 1
    with guarded("cpu") as g:
        x = torch.empty(64)
        _block_of(g, x).block[0] = 1
        assert len(g.check()) == 1


def test_place_and_poison():
    src = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    with guarded("cpu") as g:
        p = g.place(src)
        a = _block_of(g, p)
        assert torch.equal(p, src) and p.data_ptr() != src.data_ptr() and a.kind == "place"
        assert a.site.function == "test_place_and_poison" and a.site.file == os.path.abspath(__file__)
        assert (a.block[:RED] == FILL).all() and (a.block[RED + 48:] == FILL).all()
        q = g.place(src.t())                                       # a strided input lands contiguous
        assert torch.equal(q, src.t()) and q.is_contiguous()
        g.poison(p)
        assert torch.isnan(p).all() and (_bytes(p) == FILL).all()
        live = torch.zeros(5, dtype=torch.int32)
        ga.poison(live)
        assert (live == -1).all()
        assert g.check() == []


def test_originals_are_restored_also_after_an_exception():
    orig = (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like)
    base_new = (torch.Tensor.new_empty, torch.Tensor.new_zeros)
    own = [n in torch.Tensor.__dict__ for n in ("new_empty", "new_zeros")]
    with guarded("cpu"):
        assert torch.empty is not orig[0] and torch.Tensor.new_zeros is not base_new[1]
    assert (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like) == orig
    with pytest.raises(RuntimeError, match="boom"):
        with guarded("cpu"):
            torch.empty(3)
            raise RuntimeError("boom")
    assert (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like) == orig
    assert (torch.Tensor.new_empty, torch.Tensor.new_zeros) == base_new
    assert [n in torch.Tensor.__dict__ for n in ("new_empty", "new_zeros")] == own
    assert not torch.isnan(torch.zeros(3)).any()


def test_pass_through_requests_are_listed():
    with guarded("cpu") as g:
        a = torch.empty(3, device="meta")                          # another device
        b = torch.empty(3, requires_grad=True)                     # a further keyword argument
        c = torch.zeros(2, 2, pin_memory=False)
        d = torch.empty_like(torch.ones(2, 3).t())                 # strides to preserve
        assert a.device.type == "meta" and b.requires_grad and (c == 0).all() and d.shape == (3, 2)
        assert g.allocations == []
        assert [p.kind for p in g.passed] == ["empty", "empty", "zeros", "empty_like"]
        assert [p.reason for p in g.passed] == ["other device", "keyword arguments requires_grad",
                                                "keyword arguments pin_memory", "keyword arguments (strides of a permuted source)"]
        assert g.passed[0].device.type == "meta" and g.passed[1].device.type == "cpu"
        for p in g.passed:
            assert p.site.function == "test_pass_through_requests_are_listed"
        # none of them came from the package, so none counts against a GPU case
        assert g.unguarded() == []
        assert len(g.unguarded(under=os.path.dirname(os.path.abspath(__file__)), device_type="cpu")) == 3


def test_a_guard_for_another_device_leaves_cpu_requests_alone():
    with guarded("cuda:0") as g:
        x = torch.zeros(4)
        assert (x == 0).all() and g.allocations == [] and len(g.passed) == 1 and g.passed[0].reason == "other device"


def test_static_scan_of_the_package():
    sites = ga.scan_sites()
    assert len(sites) == PROJECT_SITES, "\n".join(str(s) for s in sites)
    assert len(set(sites)) == len(sites)
    per_file = {}
    for s in sites:
        per_file[s.file] = per_file.get(s.file, 0) + 1
    assert len(per_file) == 15
    assert per_file[os.path.join("fastvocoder_amd", "_native.py")] == 89                # 88 lines, one with two calls
    assert per_file[os.path.join("fastvocoder_amd", "generator", "basis_grad.py")] == 1
    calls = {s.call for s in sites}
    assert calls == {"empty", "empty_like", "zeros", "zeros_like", "new_zeros"}
    # Plan.run's arena and output are two of them
    assert {s.call for s in sites if s.function == "run" and s.file.endswith("_native.py")} >= {"empty"}


def test_reached_maps_recorded_sites_onto_the_static_list(tmp_path):
    sites = ga.scan_sites()
    one = next(s for s in sites if s.file.endswith("basis_grad.py"))
    rec = [ga.Site(os.path.join(ga.ROOT, one.file), one.line, one.function),
           ga.Site(os.path.join(ga.ROOT, one.file), 1, "<module>"),
           ga.Site(str(tmp_path / "elsewhere.py"), one.line, "f")]
    assert ga.reached(sites, rec) == [one]
    assert ga.reached(sites, []) == []
