"""CPU tests of fastvocoder_amd.optim.Adam and of the oracle behind tests/test_gpu_optim.py (tests/optim_reference.py):
the float64 closed form meets float64 torch, the float32 yardsticks are printed, the state dict interchanges with
torch.optim.Adam in both directions, the constructor refuses what the kernels do not do, the table has the layout the
header declares, and the header, the library and the ABI version carry the new entries."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native, optim
from tests import optim_reference as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fv_grad_sq_norm", "fv_grad_sq_norm_workspace_bytes", "fv_adam_step")
YARDSTICK_THREADS = 4


def _params():
    return [torch.nn.Parameter(torch.from_numpy(p)) for p in oref.initial_parameters()[:4]]


@pytest.mark.parametrize("max_norm", [oref.CLIP_ON, oref.CLIP_OFF])
def test_the_closed_form_meets_float64_torch(max_norm):
    ref, _ = oref.run_reference(max_norm)
    worst = oref.errors(oref.run_torch(max_norm, dtype=torch.float64), ref, oref.initial_parameters())
    print(f"float64 torch against the closed form, max_norm {max_norm}: {worst}")
    assert max(worst.values()) <= 1e-11, worst
    assert (ref[0][0] > oref.CLIP_ON) and (ref[0][0] < oref.CLIP_OFF)     # one bound clips, the other does not
    assert ref[1][5][oref.SKIP[1]] is None                               # the skipped tensor got no update


def test_float32_torch_error_of_the_case_is_printed():
    """The yardstick the constants of tests/test_gpu_optim.py are read against."""
    n = torch.get_num_threads()
    torch.set_num_threads(YARDSTICK_THREADS)
    try:
        for max_norm in (oref.CLIP_OFF, oref.CLIP_ON):
            ref, _ = oref.run_reference(max_norm)
            worst = oref.errors(oref.run_torch(max_norm), ref, oref.initial_parameters())
            print(f"yardstick max_norm {max_norm}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
            assert 0.0 < worst["p"] < 1e-6 and 0.0 < worst["m"] < 1e-4 and 0.0 < worst["norm"] < 1e-4
    finally:
        torch.set_num_threads(n)


def _equal_state(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys()
        for name in a["state"][k]:
            x, y = a["state"][k][name], b["state"][k][name]
            assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), (k, name)


def test_the_state_dict_interchanges_with_torch_adam():
    def grads(ps, seed):
        g = torch.Generator().manual_seed(seed)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)

    # torch -> ours -> torch: the detour changes nothing, and the trajectory continues bit for bit
    a = _params()
    ta = torch.optim.Adam(a, lr=1e-3, eps=1e-6)
    for s in range(2):
        grads(a, s)
        ta.step()
    ours = optim.Adam(_params(), lr=5e-2, eps=1e-3)
    ours.load_state_dict(copy.deepcopy(ta.state_dict()))     # (a copy, as a checkpoint is: torch shares the step tensors)
    _equal_state(ours.state_dict(), ta.state_dict())
    assert ours.param_groups[0]["lr"] == 1e-3 and ours.param_groups[0]["eps"] == 1e-6
    step = ours.state[ours.param_groups[0]["params"][0]]["step"]
    assert torch.is_tensor(step) and step.device.type == "cpu" and step.dtype == torch.float32 and float(step) == 2.0
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    tb = torch.optim.Adam(b, lr=7.0)
    tb.load_state_dict(copy.deepcopy(ours.state_dict()))
    grads(a, 9)
    grads(b, 9)
    ta.step()
    tb.step()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # a fresh optimizer of ours has torch's empty state and groups
    fresh, tfresh = optim.Adam(_params(), lr=1e-4, eps=1e-6), torch.optim.Adam(_params(), lr=1e-4, eps=1e-6)
    _equal_state(fresh.state_dict(), tfresh.state_dict())
    # a reference checkpoint of an older torch stores the step count as a number
    old = copy.deepcopy(ta.state_dict())
    for s in old["state"].values():
        s["step"] = int(s["step"])
    ours.load_state_dict(old)
    step = ours.state[ours.param_groups[0]["params"][0]]["step"]
    assert torch.is_tensor(step) and float(step) == 3.0


def test_the_constructor_refuses_what_the_kernels_do_not_do():
    for kw, word in ((dict(amsgrad=True), "amsgrad"), (dict(weight_decay=0.01), "weight_decay"),
                     (dict(maximize=True), "maximize"), (dict(capturable=True), "capturable"),
                     (dict(differentiable=True), "differentiable")):
        with pytest.raises(ValueError, match=word):
            optim.Adam(_params(), lr=1e-3, **kw)
    with pytest.raises(ValueError, match="fp32"):
        optim.Adam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError, match="fp32"):
        optim.Adam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float16))])
    with pytest.raises(ValueError, match="contiguous"):
        optim.Adam([torch.zeros(4, 6).t().requires_grad_(True)])
    with pytest.raises(ValueError, match="lr as a float"):
        optim.Adam(_params(), lr=torch.tensor(1e-3))
    opt = optim.Adam(_params(), lr=1e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0, amsgrad=False)
    assert isinstance(opt, torch.optim.Adam) and opt.defaults["betas"] == (0.8, 0.99)
    with pytest.raises(ValueError, match="weight_decay"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))], "weight_decay": 0.1})
    bad = torch.optim.Adam(_params(), lr=1e-3, amsgrad=True).state_dict()
    with pytest.raises(ValueError, match="amsgrad"):
        optim.Adam(_params(), lr=1e-3).load_state_dict(bad)


def test_step_has_no_cpu_path_and_leaves_the_state_alone():
    ps = _params()
    opt = optim.Adam(ps, lr=1e-3)
    assert opt.step(max_norm=1.0) is None and len(opt.state) == 0           # no gradient anywhere: nothing to do
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(_native.NativeError, match="ROCm device"):
        opt.step(max_norm=1.0)
    assert all(torch.equal(p, b) for p, b in zip(ps, before))
    assert all(float(s["step"]) == 0.0 for s in opt.state.values())         # no step count moved
    with pytest.raises(ValueError, match="closure"):
        opt.step(lambda: 0.0)
    with pytest.raises(ValueError, match="max_norm"):
        opt.step(max_norm=-1.0)


def test_the_table_has_the_layout_of_the_header():
    C = _native.ADAM_CHUNK
    rows = [(0x1000, 0x2000, 0x3000, 0x4004, 1, 0.5, 2.0), (0x10, 0x20, 0x30, 0x40, C, 0.25, 4.0),
            (0x11, 0x21, 0x31, 0x41, 2 * C + 1, 0.125, 8.0)]
    raw, first = optim.adam_table(rows)
    assert raw.dtype == np.uint8 and list(first) == [0, 1, 2, 5]
    assert raw.size == 48 * 3 + 8 * 5 == _native.ADAM_ROW_BYTES * 3 + _native.ADAM_CHUNK_BYTES * 5
    table = raw[:48 * 3].view(optim.ROW)
    assert [tuple(r) for r in table.tolist()] == [tuple(r) for r in rows]
    assert raw[32:40].view("<i8")[0] == 1 and raw[40:44].view("<f4")[0] == 0.5 and raw[44:48].view("<f4")[0] == 2.0
    chunks = raw[48 * 3:].view("<i4").reshape(-1, 2).tolist()
    assert chunks == [[0, 0], [1, 0], [2, 0], [2, 1], [2, 2]]
    step_size, inv = optim.bias_factors(1e-3, 0.9, 0.999, 3)
    assert step_size == pytest.approx(1e-3 / (1 - 0.9 ** 3), rel=1e-15)
    assert inv == pytest.approx((1 - 0.999 ** 3) ** -0.5, rel=1e-15)


def test_the_header_declares_the_entries_and_the_abi_stays():
    with open(os.path.join(ROOT, "include", "fastvocoder_hip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert re.search(rf"\b(int|int64_t) {name}\(", header), name
        assert hasattr(lib, name), name
    assert re.search(r"#define FV_ABI_VERSION 18\b", header) and _native.ABI_VERSION == 18
    assert re.search(rf"#define FV_ADAM_CHUNK {_native.ADAM_CHUNK}\b", header)
    assert "typedef struct fv_adam_tensor" in header and "typedef struct fv_adam_chunk" in header
    assert "optim.hip" in _native.SOURCES
    assert os.path.exists(os.path.join(ROOT, "fastvocoder_amd", "csrc", "optim.hip"))


def test_the_entries_refuse_bad_arguments_before_they_touch_a_pointer():
    L = _native.lib()
    assert _native.grad_sq_norm_workspace_floats(1) == 2 and _native.grad_sq_norm_workspace_floats(1000) == 2000
    for bad in (0, -3, 1 << 31):
        with pytest.raises(_native.NativeError):
            _native.grad_sq_norm_workspace_floats(bad)
    inv = _native.ERR_INVALID_ARG
    assert L.fv_grad_sq_norm(None, None, 1, 1, 1.0, None, 0, None, None) == inv            # null table
    assert L.fv_grad_sq_norm(8, 16, 0, 1, 1.0, 8, 8, 8, None) == inv                        # no tensors
    assert L.fv_grad_sq_norm(8, 16, 1, 0, 1.0, 8, 8, 8, None) == inv                        # no chunks
    assert L.fv_grad_sq_norm(8, 16, 1, 1, -1.0, 8, 8, 8, None) == inv                       # max_norm < 0
    assert L.fv_grad_sq_norm(8, 16, 1, 1, float("nan"), 8, 8, 8, None) == inv
    assert L.fv_grad_sq_norm(12, 16, 1, 1, 1.0, 8, 8, 8, None) == inv                       # misaligned table
    assert L.fv_grad_sq_norm(8, 16, 1, 1, 1.0, None, 8, 8, None) == inv                     # no workspace
    assert L.fv_grad_sq_norm(8, 16, 1, 3, 1.0, 8, 16, 8, None) == _native.ERR_WORKSPACE     # 3 chunks need 24 bytes
    assert L.fv_adam_step(None, None, 1, 1, None, 0.9, 0.999, 1e-6, None) == inv
    assert L.fv_adam_step(8, 16, 1, 1, None, 1.0, 0.999, 1e-6, None) == inv                 # beta1 = 1
    assert L.fv_adam_step(8, 16, 1, 1, None, 0.9, -0.1, 1e-6, None) == inv
    assert L.fv_adam_step(8, 16, 1, 1, None, 0.9, 0.999, -1.0, None) == inv
    assert L.fv_adam_step(8, 16, 1, 1, 2, 0.9, 0.999, 1e-6, None) == inv                    # misaligned coef
    assert L.fv_adam_step(8, 16, 1, 1 << 31, None, 0.9, 0.999, 1e-6, None) == inv
