"""Float64 closed form of clip_grad_norm_ + Adam (csrc/optim.hip, fastvocoder_amd/optim.py) and the case the host and
the GPU tests share: six tensors, three steps, gradients over four decades, a learning rate that changes, and one
parameter without a gradient at the second step.

TEST INFRASTRUCTURE ONLY; nothing here runs on the GPU."""
import math

import numpy as np
import torch

SHAPES = [(1,), (7,), (4099,), (3, 5, 1031), (256, 128, 16)]
VIEW_ELEMENTS = 1030            # the sixth parameter: base[1:], a contiguous view 4 bytes into its storage
GRAD_SCALES = [1e-2, 1.0, 1e-1, 1e-3, 1e-2, 1e-4]      # per tensor: four decades between the (7,) and the view
LRS = [1e-3, 3e-4, 5e-4, 1e-3]                         # the fourth is the step torch.optim.Adam continues with
STEPS = 3
SKIP = (1, 2)                   # (step index, tensor index) whose gradient is None
BETAS, EPS = (0.9, 0.999), 1e-6
CLIP_ON, CLIP_OFF = 1.0, 1e3    # the total norm is about 10: clipped by the first, untouched by the second


def all_shapes():
    return SHAPES + [(VIEW_ELEMENTS,)]


def initial_parameters(seed=11):
    """fp32 ndarrays, one per tensor (the view's is its own 1030 elements)."""
    rs = np.random.RandomState(seed)
    return [(0.1 * rs.randn(*s)).astype(np.float32) for s in all_shapes()]


def gradients(step, seed=23):
    """fp32 ndarrays of step ``step`` (None for the skipped tensor)."""
    out = []
    for k, (s, scale) in enumerate(zip(all_shapes(), GRAD_SCALES)):
        rs = np.random.RandomState(seed + 97 * step + k)
        g = (scale * (1.0 + 0.5 * step) * rs.randn(*s)).astype(np.float32)
        out.append(None if (step, k) == SKIP else g)
    return out


def total_norm(grads):
    return math.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in grads if g is not None))


def clip_coef(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


class Reference:
    """The trajectory in float64 from fp32 inputs: per tensor p, m, v and its own step count."""

    def __init__(self, params, betas=BETAS, eps=EPS):
        self.p = [np.asarray(p, np.float64).copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.t = [0] * len(self.p)
        self.betas, self.eps = betas, eps

    def step(self, grads, lr, max_norm=None):
        """-> (norm or None, the clipped gradients, the updates p_after - p_before); tensors whose gradient is None
        are left alone (None in both lists)."""
        b1, b2 = self.betas
        norm = total_norm(grads) if max_norm is not None else None
        coef = clip_coef(norm, max_norm) if max_norm is not None else 1.0
        clipped, updates = [], []
        for k, g in enumerate(grads):
            if g is None:
                clipped.append(None)
                updates.append(None)
                continue
            g = coef * np.asarray(g, np.float64)
            self.t[k] += 1
            self.m[k] = b1 * self.m[k] + (1 - b1) * g
            self.v[k] = b2 * self.v[k] + (1 - b2) * g * g
            step_size = lr / (1 - b1 ** self.t[k])
            denom = np.sqrt(self.v[k]) / math.sqrt(1 - b2 ** self.t[k]) + self.eps
            upd = -step_size * self.m[k] / denom
            self.p[k] = self.p[k] + upd
            clipped.append(g)
            updates.append(upd)
        return norm, clipped, updates


def rel_err(got, want):
    """max |got - want| relative to the largest magnitude of ``want``."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def torch_parameters(params, device="cpu", dtype=torch.float32):
    """Leaf tensors of the case on ``device``; the last is a view one element into a larger storage."""
    out = []
    for k, p in enumerate(params):
        t = torch.from_numpy(np.asarray(p)).to(dtype)
        if k == len(params) - 1:
            base = torch.zeros(t.numel() + 1, dtype=dtype, device=device)
            base[1:] = t.to(device)
            t = base[1:]
        else:
            t = t.to(device).clone()
        out.append(t.requires_grad_(True))
    return out


def set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else torch.from_numpy(g).to(device=p.device, dtype=p.dtype)


def run_torch(max_norm, dtype=torch.float32, device="cpu", steps=STEPS):
    """clip_grad_norm_ + torch.optim.Adam on the case -> per step (norm, [p], [m], [v], [grad after the step]) as
    float64 ndarrays (None entries where a tensor has no state yet / no gradient)."""
    params = torch_parameters(initial_parameters(), device, dtype)
    opt = torch.optim.Adam(params, lr=LRS[0], betas=BETAS, eps=EPS)
    out = []
    for s in range(steps):
        for group in opt.param_groups:
            group["lr"] = LRS[s]
        set_grads(params, gradients(s))
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        out.append(snapshot(opt, params, float(norm)))
    return out


def snapshot(opt, params, norm):
    def arr(t):
        return None if t is None else t.detach().double().cpu().numpy().copy()
    return (norm, [arr(p) for p in params], [arr(opt.state[p].get("exp_avg")) for p in params],
            [arr(opt.state[p].get("exp_avg_sq")) for p in params], [arr(p.grad) for p in params])


def run_reference(max_norm, steps=STEPS):
    """The same trajectory in float64 -> (per step (norm, [p], [m], [v], [clipped grad], [update]), the Reference)."""
    ref = Reference(initial_parameters())
    out = []
    for s in range(steps):
        norm, clipped, updates = ref.step(gradients(s), LRS[s], max_norm)
        seen = [t > 0 for t in ref.t]
        out.append((norm, [p.copy() for p in ref.p], [m.copy() if ok else None for m, ok in zip(ref.m, seen)],
                    [v.copy() if ok else None for v, ok in zip(ref.v, seen)], clipped, updates))
    return out, ref


CLASSES = ("p", "update", "m", "v", "grad", "norm")


def errors(got_steps, ref_steps, start):
    """Worst error per class of a trajectory ``got_steps`` (snapshots) against the float64 one, each relative to the
    tensor's largest magnitude; ``start``: the fp32 initial parameters.  "update" is p_after - p_before of a step,
    each trajectory against its own p_before."""
    worst = dict.fromkeys(CLASSES, 0.0)
    before = [np.asarray(p, np.float64) for p in start]
    rbefore = [b.copy() for b in before]
    for (norm, ps, ms, vs, gs), (rnorm, rps, rms, rvs, rgs, rupd) in zip(got_steps, ref_steps):
        worst["norm"] = max(worst["norm"], abs(norm - rnorm) / rnorm)
        for k in range(len(ps)):
            worst["p"] = max(worst["p"], rel_err(ps[k], rps[k]))
            if rupd[k] is not None:
                worst["update"] = max(worst["update"], rel_err(ps[k] - before[k], rps[k] - rbefore[k]))
                worst["grad"] = max(worst["grad"], rel_err(gs[k], rgs[k]))
            if rms[k] is not None:
                worst["m"] = max(worst["m"], rel_err(ms[k], rms[k]))
                worst["v"] = max(worst["v"], rel_err(vs[k], rvs[k]))
        before, rbefore = ps, rps
    return worst
