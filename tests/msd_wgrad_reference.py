"""Float64 numpy restatement of the closed forms behind csrc/disc_wgrad.hip, written from
their definitions; tests/test_msd_wgrad_host.py pins each one to float64 torch autograd, and
tests/test_gpu_msd_wgrad.py compares the kernels with them on the same fp32 inputs.  ``param_grad`` is float64 torch
autograd of the discriminator's own loss (bin/train.py:157-169: real + fake) with respect to every entry of the state
dict, weight norm folded inside the graph; ``sgd_steps`` repeats it along a few plain SGD steps."""
import numpy as np
import torch

from tests import disc_grad_reference as gref


def _f64(a):
    return np.asarray(a, np.float64)


def pad_input(x, pad, mode):
    """x [B, C, T] padded by ``pad`` on both sides: "zero" or "reflect" (mirrored without the edge sample)."""
    x = _f64(x)
    return np.pad(x, ((0, 0), (0, 0), (pad, pad)), mode="constant" if mode == "zero" else "reflect")


def dense_weight_grad(g_pre, x, k, pad, mode="zero"):
    """dW[co, ci, j] = sum_{b, t} g_pre[b, co, t] xpad[b, ci, t + j] of a stride-1 conv."""
    g_pre, xp = _f64(g_pre), pad_input(x, pad, mode)
    tout = g_pre.shape[2]
    assert tout == xp.shape[2] - k + 1
    dw = np.zeros((g_pre.shape[1], xp.shape[1], k))
    for j in range(k):
        dw[:, :, j] = np.einsum("bot,bit->oi", g_pre, xp[:, :, j:j + tout])
    return dw


def grouped_weight_grad(g_pre, x, k, stride, pad):
    """dW[oc, ci, j] = sum_{b, t} g_pre[b, oc, t] x[b, 4 g + ci, t stride + j - pad] (0 outside the input), oc in
    group g of Cin / 4 groups."""
    g_pre, xp = _f64(g_pre), pad_input(x, pad, "zero")
    B, cout, tout = g_pre.shape
    cin = xp.shape[1]
    G = cin // 4
    opg = cout // G
    need = (tout - 1) * stride + k                       # samples of the padded input the windows reach
    if xp.shape[2] < need:
        xp = np.pad(xp, ((0, 0), (0, 0), (0, need - xp.shape[2])))
    dw = np.zeros((cout, 4, k))
    for j in range(k):
        xs = xp[:, :, j:j + (tout - 1) * stride + 1:stride]                        # [B, cin, tout]
        for g in range(G):
            dw[g * opg:(g + 1) * opg, :, j] = np.einsum("bot,bit->oi", g_pre[:, g * opg:(g + 1) * opg],
                                                        xs[:, 4 * g:4 * g + 4])
    return dw


def bias_grad(g_pre):
    return _f64(g_pre).sum(axis=(0, 2))


def weight_norm_grad(dw, v, g):
    """The adjoint of w = g v / |v| per row of dim 0: dg = <dw, v> / n, dv = (g / n)(dw - (<dw, v> / n^2) v)."""
    dw, v = _f64(dw), _f64(v)
    g = _f64(g).reshape(-1)
    flat_w, flat_v = dw.reshape(len(g), -1), v.reshape(len(g), -1)
    dot = (flat_w * flat_v).sum(axis=1)
    n = np.sqrt((flat_v * flat_v).sum(axis=1))
    dv = (g / n)[:, None] * (flat_w - (dot / n ** 2)[:, None] * flat_v)
    return dv.reshape(v.shape), dot / n


# ---- float64 torch autograd of the discriminator's own loss ----
def step_terms(est_p, p):
    """real, fake and their sum (bin/train.py:157-169) on the graph of both passes."""
    L = len(p)
    real = sum(((r[-1] - 1) ** 2).mean() for r in p) / L
    fake = sum((e[-1] ** 2).mean() for e in est_p) / L
    return {"real": real, "fake": fake, "discriminator": real + fake}


def param_grad(est, real, sd, scale=None, dtype=torch.float64, with_x=False, **kw):
    """d(real + fake)/d(every entry of ``sd``) of the MSD (``scale`` None) or of scale ``scale`` alone, by torch
    autograd in ``dtype``; weight norm is folded inside the graph (disc_grad_reference._typed_run).  ``with_x``: the
    estimate is NOT detached and its gradient is returned under the key "x".
    -> ({key: float64 ndarray}, {term: float}, est maps, real maps)."""
    params = {k: torch.as_tensor(np.asarray(v), dtype=dtype).clone().requires_grad_(True) for k, v in sd.items()}
    run = gref._typed_run(params, scale, dtype, kw)
    x = torch.as_tensor(np.asarray(est), dtype=dtype).clone().requires_grad_(bool(with_x))
    p = run(torch.as_tensor(np.asarray(real), dtype=dtype))
    est_p = run(x)
    terms = step_terms(est_p, p)
    terms["discriminator"].backward()
    grads = {k: (torch.zeros_like(q) if q.grad is None else q.grad).numpy().astype(np.float64)
             for k, q in params.items() if scale is None or k.startswith(f"discriminators.{scale}.")}
    if with_x:
        grads["x"] = x.grad.numpy().astype(np.float64)
    return grads, {k: float(v.detach()) for k, v in terms.items()}, est_p, p


def sgd_steps(est, real, sd, steps, lr, **kw):
    """``steps`` plain SGD steps on real + fake in float64 -> (the loss before each step, the state dict after the
    last, the gradient of the last step)."""
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    losses, grads = [], None
    for _ in range(steps):
        grads, terms, _, _ = param_grad(est, real, sd, **kw)
        losses.append(terms["discriminator"])
        sd = {k: v - lr * grads[k] for k, v in sd.items()}
    return losses, sd, grads


def preactivation_kink_count(lists, slope=0.2, rel=1e-4):
    """How many pre-activations of the activated maps (every map but each list's last; recovered from the stored map:
    a leaky ReLU keeps the sign) lie within ``rel`` x their map's largest magnitude of zero."""
    count = 0
    for lst in lists:
        for m in lst[:-1]:
            m = m.detach()
            pre = torch.where(m > 0, m, m / slope)
            count += int((pre.abs() <= rel * pre.abs().max()).sum())
    return count
