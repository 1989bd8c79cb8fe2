"""Float64 numpy restatement of the closed forms behind csrc/disc_grad.hip, written from
their definitions; tests/test_disc_grad_host.py pins each one to float64 torch autograd, and
tests/test_gpu_disc_grad.py compares the kernels with them on the same fp32 inputs.  ``chain_grad`` is float64 torch
autograd through tests/discriminator_reference.py, the oracle of the module tests."""
import numpy as np
import torch

from tests import discriminator_reference as ref


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def map_grad(g_up, g_map, y, slope):
    """(g_up + g_map) * (y > 0 ? 1 : slope); either addend may be None, y may be None with slope 1."""
    g_up, g_map, y = _f64(g_up), _f64(g_map), _f64(y)
    g = g_up if g_map is None else g_map if g_up is None else g_up + g_map
    return g.copy() if y is None else g * np.where(y > 0, 1.0, slope)


def grouped_input_grad(g_pre, w, cin, tin, k, stride, pad):
    """dx[b, 4g+ci, i] = sum_{oc in g} sum_{j = p, p+s, ...} w[oc, ci, j] g_pre[b, oc, (i + pad - j) / s] with
    p = (i + pad) % s, over the 0 <= t < Tout: the polyphase form, one phase at a time."""
    g_pre, w = _f64(g_pre), _f64(w)
    B, cout, tout = g_pre.shape
    G = cin // 4
    opg = cout // G
    dx = np.zeros((B, cin, tin))
    i = np.arange(tin)
    P = i + pad
    for p in range(min(stride, k)):
        sel = i[P % stride == p]
        q = P[sel] // stride
        for m, j in enumerate(range(p, k, stride)):
            t = q - m
            ok = (t >= 0) & (t < tout)
            for g in range(G):
                gy = g_pre[:, g * opg:(g + 1) * opg][:, :, t[ok]]                 # [B, opg, n]
                dx[:, 4 * g:4 * g + 4, sel[ok]] += np.einsum("oc,bon->bcn", w[g * opg:(g + 1) * opg, :, j], gy)
    return dx


def dense_input_grad(g_pre, w, pad):
    """The data gradient of a stride-1 conv1d with zero padding ``pad`` as a conv1d of the gradient:
    W'[ci, co, j] = W[co, ci, k-1-j], zero padding k - 1 - pad.  ``pad = 0`` gives the padded-length gradient."""
    g_pre, w = _f64(g_pre), _f64(w)
    k = w.shape[2]
    wt = np.ascontiguousarray(w[:, :, ::-1].transpose(1, 0, 2))
    gp = np.pad(g_pre, ((0, 0), (0, 0), (k - 1 - pad,) * 2))
    n = gp.shape[2] - k + 1
    out = np.zeros((g_pre.shape[0], wt.shape[0], n))
    for j in range(k):
        out += np.einsum("co,bon->bcn", wt[:, :, j], gp[:, :, j:j + n])
    return out


def reflect_fold(gp, P):
    """Adjoint of ReflectionPad1d(P): [..., T + 2P] -> [..., T]."""
    gp = _f64(gp)
    T = gp.shape[-1] - 2 * P
    assert T > P
    i = np.arange(T)
    dx = gp[..., i + P].copy()
    left = (i >= 1) & (i <= P)
    dx[..., left] += gp[..., P - i[left]]
    right = (i >= T - 1 - P) & (i <= T - 2)
    dx[..., right] += gp[..., P + 2 * (T - 1) - i[right]]
    return dx


def avg_pool_input_grad(g, tin, k, s, p):
    """Adjoint of AvgPool1d(k, s, p, count_include_pad=False): each sample gathers g[t] / count(t)."""
    g = _f64(g)
    tout = g.shape[-1]
    assert tout == (tin + 2 * p - k) // s + 1
    dx = np.zeros(g.shape[:-1] + (tin,))
    for i in range(tin):
        for t in range(max(0, -(-(i + p - k + 1) // s)), min(tout - 1, (i + p) // s) + 1):
            a, e = max(t * s - p, 0), min(t * s - p + k, tin)
            dx[..., i] += g[..., t] / (e - a)
    return dx


def score_grad(e, r, c_l1, c_adv, c_fake):
    e, r = _f64(e), _f64(r)
    return c_l1 * np.sign(e - r) + 2 * c_adv * (e - 1) + 2 * c_fake * e


def score_coefficients(grad_terms, counts, lengths, batch):
    """(c_l1, c_adv, c_fake) per flattened map from d/d(adversarial, feature_map, real, fake, discriminator): the
    means over B n_m elements, the divisors L and L (len(est_p[0]) - 1) of bin/train.py."""
    g_adv, g_fm, _, g_fake, g_disc = grad_terms
    L = len(lengths)
    coef, m = [], 0
    for n in lengths:
        for j in range(n):
            den = float(counts[m] * batch)
            if j < n - 1:
                coef.append((g_fm / (L * (lengths[0] - 1) * den), 0.0, 0.0))
            else:
                coef.append((0.0, g_adv / (L * den), (g_fake + g_disc) / (L * den)))
            m += 1
    return coef


# ---- float64 torch autograd through the discriminator oracle ----
def terms(est_p, p):
    """The five scores as float64 tensors on the graph of est_p (discriminator_reference.scores returns floats)."""
    L = len(est_p)
    adv = sum(((e[-1] - 1) ** 2).mean() for e in est_p) / L
    fm = sum((est_p[i][j] - p[i][j].detach()).abs().mean() for i in range(L) for j in range(len(est_p[i]) - 1))
    fm = fm / (L * (len(est_p[0]) - 1))
    real = sum(((r[-1].detach() - 1) ** 2).mean() for r in p) / L
    fake = sum((e[-1] ** 2).mean() for e in est_p) / L
    return {"adversarial": adv, "feature_map": fm, "real": real, "fake": fake, "discriminator": real + fake}


def chain_grad(est, real, sd, which=("adversarial", "feature_map"), scale=None, dtype=torch.float64, **kw):
    """d(sum of the ``which`` terms)/d est of the MSD (``scale`` None) or of scale ``scale`` alone, by torch autograd
    in ``dtype`` through discriminator_reference.  -> (gradient, est maps, real maps) as numpy / lists of tensors."""
    x = torch.as_tensor(np.asarray(est), dtype=dtype).clone().requires_grad_(True)
    y = torch.as_tensor(np.asarray(real), dtype=dtype)
    sd = {k: torch.as_tensor(np.asarray(v), dtype=dtype) for k, v in sd.items()}

    def run(v):
        if scale is None:
            return ref.msd(v, sd, **kw)
        kw1 = {k: v_ for k, v_ in kw.items() if k not in ("scales", "pool")}
        return [ref.melgan(v, sd, f"discriminators.{scale}", **kw1)]

    if dtype != torch.float64:        # discriminator_reference.folded casts to float64: fold here, in dtype
        run = _typed_run(sd, scale, dtype, kw)
    est_p = run(x)
    with torch.no_grad():
        p = run(y)
    t = terms(est_p, p)
    sum(t[k] for k in which).backward()
    return x.grad.numpy().astype(np.float64), est_p, p


def _typed_run(sd, scale, dtype, kw):
    import torch.nn.functional as F

    def folded(prefix):
        w = sd.get(f"{prefix}.weight")
        if w is None:
            v, g = sd[f"{prefix}.weight_v"], sd[f"{prefix}.weight_g"]
            w = v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))
        return w, sd.get(f"{prefix}.bias")

    ks = kw.get("kernel_sizes", (5, 3))
    channels, cap = kw.get("channels", 16), kw.get("max_downsample_channels", 1024)
    scales_, slope = kw.get("downsample_scales", (4, 4, 4, 4)), kw.get("slope", 0.2)

    def melgan(x, prefix):
        outs, pre = [], f"{prefix}.layers"
        k0 = int(np.prod(ks))
        w, b = folded(f"{pre}.0.1")
        x = F.leaky_relu(F.conv1d(F.pad(x, ((k0 - 1) // 2,) * 2, mode="reflect"), w, b), slope)
        outs.append(x)
        c = channels
        for i, s in enumerate(scales_):
            w, b = folded(f"{pre}.{i + 1}.0")
            x = F.leaky_relu(F.conv1d(x, w, b, stride=s, padding=5 * s, groups=c // 4), slope)
            outs.append(x)
            c = min(c * s, cap)
        n = len(scales_) + 1
        w, b = folded(f"{pre}.{n}.0")
        x = F.leaky_relu(F.conv1d(x, w, b, padding=(ks[0] - 1) // 2), slope)
        outs.append(x)
        w, b = folded(f"{pre}.{n + 1}")
        outs.append(F.conv1d(x, w, b, padding=(ks[1] - 1) // 2))
        return outs

    def run(v):
        if scale is not None:
            return [melgan(v, f"discriminators.{scale}")]
        outs = []
        for i in range(kw.get("scales", 3)):
            outs.append(melgan(v, f"discriminators.{i}"))
            v = F.avg_pool1d(v, *kw.get("pool", (4, 2, 1)), count_include_pad=False)
        return outs
    return run


def kink_count(est_p, p, slope=0.2, rel=1e-4):
    """How many values of the oracle sit within ``rel`` x their map's largest magnitude of a kink: the
    pre-activations of every activated map (recovered from the stored map: a leaky ReLU keeps the sign) and the
    differences e - r of every feature map (their scale: the larger peak of the two maps)."""
    count = 0
    for le, lr in zip(est_p, p):
        for j in range(len(le) - 1):
            e, r = le[j].detach(), lr[j].detach()
            pre = torch.where(e > 0, e, e / slope)
            count += int((pre.abs() <= rel * pre.abs().max()).sum())
            count += int(((e - r).abs() <= rel * max(float(e.abs().max()), float(r.abs().max()))).sum())
    return count
