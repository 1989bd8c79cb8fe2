"""GPU tests of fastvocoder_amd.optim.Adam (csrc/optim.hip) against the float64 closed form of
tests/optim_reference.py on the same fp32 inputs: six tensors -- (1,), (7,), (4099,), (3, 5, 1031), (256, 128, 16) and
a view 4 bytes into its storage --, three steps with gradients over four decades, the learning rate changed between
steps, one parameter without a gradient at the second step; with clipping active (max_norm 1) and inactive.

The constants are about ten times the worst error measured on MI355X per class (DESIGN 6.21 has the table, ``-s``
prints the figures); every figure is relative to the tensor's largest magnitude.  The yardstick beside them is float32
torch.optim.Adam + clip_grad_norm_ on the CPU against the same float64
(tests/test_optim_host.py::test_float32_torch_error_of_the_case_is_printed): p 1.0e-7, update 5.0e-5, m 9.0e-8 / 2.8e-6
with clipping, v 1.4e-7 / 6.0e-6, the clipped gradient 3.0e-6, the norm 2.9e-6.  The update's figure is the rounding of
p itself (half an ulp of 0.4 against steps of 3e-4 .. 1e-3).
"""
import copy

import numpy as np
import pytest
import torch

from fastvocoder_amd import optim
from tests import optim_reference as oref

pytestmark = pytest.mark.gpu

# class -> (without clipping, with clipping)
# measured on MI355X:  p 1.04e-7 / 1.01e-7, update 4.97e-5 / 4.97e-5, m 1.48e-7 / 1.19e-7, v 1.49e-7 / 1.61e-7,
#                      grad 0 (coef is exactly 1) / 8.65e-8, norm 4.53e-8 / 4.53e-8
TOL = {"p": (1.0e-6, 1.0e-6), "update": (5e-4, 5e-4), "m": (1.5e-6, 1.5e-6), "v": (1.6e-6, 1.6e-6),
       "grad": (0.0, 9e-7), "norm": (5e-7, 5e-7)}


def _run(max_norm, device, steps=oref.STEPS, poison=False):
    """Our optimizer on the case -> (snapshots per step, the optimizer, its parameters, what the test observed about
    the skipped parameter)."""
    params = oref.torch_parameters(oref.initial_parameters(), device)
    assert params[-1].data_ptr() % 16 == 4 and params[-1].is_contiguous()
    opt = optim.Adam(params, lr=oref.LRS[0], betas=oref.BETAS, eps=oref.EPS)
    if poison:
        opt._workspace = torch.full((1 << 16,), float("nan"), dtype=torch.float32, device=device)
    out, seen = [], {}
    for s in range(steps):
        for group in opt.param_groups:
            group["lr"] = oref.LRS[s]
        oref.set_grads(params, oref.gradients(s))
        if s == oref.SKIP[0]:
            st = opt.state[params[oref.SKIP[1]]]
            seen["before"] = (params[oref.SKIP[1]].detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(),
                              float(st["step"]))
        norm = opt.step(max_norm=max_norm)
        assert norm.dim() == 0 and norm.is_cuda and norm.dtype == torch.float32
        if s == oref.SKIP[0]:
            st = opt.state[params[oref.SKIP[1]]]
            seen["after"] = (params[oref.SKIP[1]].detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(),
                             float(st["step"]))
        out.append(oref.snapshot(opt, params, float(norm)))
    return out, opt, params, seen


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def runs(device):
    """max_norm -> (our trajectory and its objects, the float64 trajectory): computed once."""
    return {mn: (_run(mn, device), oref.run_reference(mn)) for mn in (oref.CLIP_OFF, oref.CLIP_ON)}


@pytest.mark.parametrize("clipped", [False, True])
def test_three_steps_meet_float64(runs, clipped):
    (got, opt, params, _), (ref, _) = runs[oref.CLIP_ON if clipped else oref.CLIP_OFF]
    worst = oref.errors(got, ref, oref.initial_parameters())
    print(f"optim clipped={clipped}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    coef = [oref.clip_coef(r[0], oref.CLIP_ON if clipped else oref.CLIP_OFF) for r in ref]
    assert all(c < 0.2 for c in coef) if clipped else all(c == 1.0 for c in coef)
    for k, v in worst.items():
        assert v <= TOL[k][clipped], (k, v)
    # the step counts: every tensor at 3, the skipped one at 2
    steps = [float(opt.state[p]["step"]) for p in params]
    assert steps == [3.0 if k != oref.SKIP[1] else 2.0 for k in range(len(params))]
    assert all(opt.state[p]["step"].device.type == "cpu" for p in params)


def test_without_max_norm_nothing_is_clipped_or_returned(device):
    params = oref.torch_parameters(oref.initial_parameters(), device)
    opt = optim.Adam(params, lr=oref.LRS[0], betas=oref.BETAS, eps=oref.EPS)
    grads = oref.gradients(0)
    oref.set_grads(params, grads)
    assert opt.step() is None
    ref = oref.Reference(oref.initial_parameters())
    ref.step(grads, oref.LRS[0])
    for p, g, rp in zip(params, grads, ref.p):
        assert np.array_equal(p.grad.cpu().numpy(), g)                    # the gradient is left as it was
        assert oref.rel_err(p.detach().cpu().numpy(), rp) <= TOL["p"][0]


def test_a_parameter_without_gradient_keeps_its_bits(runs):
    for mn in runs:
        seen = runs[mn][0][3]
        for a, b in zip(seen["before"][:3], seen["after"][:3]):
            assert torch.equal(a, b)
        assert seen["before"][3] == seen["after"][3] == 1.0


def test_two_runs_give_identical_bits_and_the_workspace_does_not_matter(runs, device):
    got = runs[oref.CLIP_ON][0][0]
    for poison in (False, True):
        again = _run(oref.CLIP_ON, device, poison=poison)[0]
        for (n1, *a), (n2, *b) in zip(got, again):
            assert n1 == n2
            for xs, ys in zip(a, b):
                for x, y in zip(xs, ys):
                    assert (x is None and y is None) or np.array_equal(x, y)


def test_parameter_versions_move(device):
    """Whatever is cached against the parameters' versions (packed weights, plans) must see the update."""
    params = oref.torch_parameters(oref.initial_parameters(), device)
    opt = optim.Adam(params, lr=1e-3)
    oref.set_grads(params, oref.gradients(0))
    before = [p._version for p in params]
    opt.step(max_norm=1.0)
    assert all(p._version > b for p, b in zip(params, before))


def test_torch_adam_continues_the_trajectory_from_our_state_dict(runs, device):
    (_, opt, params, _), _ = runs[oref.CLIP_ON]
    _, ref = oref.run_reference(oref.CLIP_ON)
    clones = [p.detach().clone().requires_grad_(True) for p in params]
    topt = torch.optim.Adam(clones, lr=123.0)
    topt.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert topt.param_groups[0]["lr"] == oref.LRS[oref.STEPS - 1] and topt.param_groups[0]["eps"] == oref.EPS
    for group in topt.param_groups:
        group["lr"] = oref.LRS[oref.STEPS]
    grads = oref.gradients(oref.STEPS)
    oref.set_grads(clones, grads)
    torch.nn.utils.clip_grad_norm_(clones, oref.CLIP_ON)
    topt.step()
    ref.step(grads, oref.LRS[oref.STEPS], oref.CLIP_ON)
    worst = max(oref.rel_err(c.detach().cpu().numpy(), rp) for c, rp in zip(clones, ref.p))
    print(f"torch.optim.Adam continuing from our state: p {worst:.2e}")
    assert worst <= TOL["p"][1]
    assert [float(topt.state[c]["step"]) for c in clones] == \
        [4.0 if k != oref.SKIP[1] else 3.0 for k in range(len(clones))]


def test_the_pinned_table_buffers_are_not_reused_while_a_copy_may_read_them(device):
    params = oref.torch_parameters(oref.initial_parameters(), device)
    opt = optim.Adam(params, lr=1e-3)
    for s in range(8):                      # queued back to back, never synchronised
        oref.set_grads(params, oref.gradients(0))
        opt.step(max_norm=1.0)
    torch.cuda.synchronize()
    assert 1 <= len(opt._pinned) <= 8 and all(buf.is_pinned() for buf, _ in opt._pinned)
    n = len(opt._pinned)
    oref.set_grads(params, oref.gradients(0))
    opt.step(max_norm=1.0)                  # every earlier copy has completed: a buffer is reused
    assert len(opt._pinned) == n
