"""The oracle of the multi-period discriminator's input gradient (csrc/mpd_grad.hip, DESIGN.md section 4.13;
fastvocoder_amd.loss.generator_adversarial_terms(..., period_grad=True)): float64 numpy written from the formulas.

  * conv_h_adjoint: the adjoint of mpd_reference.conv_h (k taps along h, stride s, (k - 1) / 2 zero rows), and
    mask(): the leaky-ReLU factor of a stored output;
  * view_adjoint: the adjoint of mpd_reference.view (the reflect tail folds back onto samples T - 1 - n_pad .. T - 2);
  * objective_grad: d(adversarial + feature_map)/d estimate of bin/train.py:97-120 through a DiscriminatorP, the MPD
    or Discriminator(use_mpd=True), for both forms of the loss (``real`` None: the adversarial term alone);
  * the same with every kink decision -- each leaky ReLU's side, each sign(e - r) -- taken from given maps
    (``est_maps`` / ``real_maps``), returning the decisions that differ from float64's own;
  * typed_mpd / eager_grad: the same chain as torch conv2d autograd in a chosen dtype, the yardstick of the GPU bounds.
tests/test_mpd_grad_host.py pins the pieces to each other and to the reference's own gradient
(tests/golden/mpd_grad.npz); tests/test_gpu_mpd_grad.py compares the kernels with them."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import mpd_reference as ref

SLOPE = ref.SLOPE
PERIODS = ref.PERIODS
SEEDS = {"mpd": 21, "discriminator": 22}            # the weights of tests/test_gpu_mpd.py
KINK_BAND = 1e-4
UNRESOLVED = 3e-7                                    # 5 float32 ulps (2^-24) of a map's largest magnitude
# the tiny cases: period -> T; B = 2, T % period != 0 (a reflect tail), every map from two rows down to one; the seeds
# are chosen by tests/golden/make_mpd_grad_golden.py and stored in the golden
TINY_T = {2: 13, 3: 20, 5: 33, 7: 45, 11: 64}
N2311 = (2311, 77)                                   # samples, RandomState seed; B = 2
# (Cin, Cout) of the three strided layers; the kernel tests' heights are chosen by tests/test_gpu_mpd_grad.py
PERIOD_LAYERS = ((32, 128), (128, 512), (512, 1024))
YARDSTICK_SHAPES = [(32, 128, 2, 40), (128, 512, 3, 23), (512, 1024, 5, 11), (32, 128, 7, 20), (128, 512, 11, 13)]
# The error of float32 eager autograd (torch conv2d on the CPU) against float64 per case family, as
# tests/test_mpd_grad_host.py::test_float32_eager_autograd_error_is_the_yardstick computes it on 4 threads and
# asserts within 5 %; the GPU bounds of tests/test_gpu_mpd_grad.py are 10 x these.
YARDSTICK_THREADS = 4
YARDSTICK = {"period_conv": 1.89e-6, "first": 2.95e-7, "tiny": 9.88e-7, "n2311": 8.99e-7}


def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, np.float64)


def sub_state_dict(sd, i, prefix=""):
    """The state dict of DiscriminatorP number i of an MPD's."""
    pre = f"{prefix}discriminators.{i}."
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


def signals(seed, T, B=2):
    rs = np.random.RandomState(seed)
    real = rs.uniform(-0.8, 0.8, (B, 1, T)).astype(np.float32)
    est = (real + 0.3 * rs.randn(B, 1, T)).astype(np.float32)
    return est, real


def mask(g, y, slope=SLOPE):
    """g * (y > 0 ? 1 : slope): the gradient in front of a leaky ReLU from the one behind it and the stored output."""
    return _f64(g) * np.where(_f64(y) > 0, 1.0, slope)


def conv_h_adjoint(g_pre, w, H, stride):
    """The adjoint of mpd_reference.conv_h in its input: g_pre [B, Cout, Hout, p], w [Cout, Cin, k] -> [B, Cin, H, p],
    dx[b, ci, r, c] = sum_co sum_{j : (r + pad - j) % stride == 0} w[co, ci, j] g_pre[b, co, (r + pad - j) / stride, c]."""
    g_pre, w = _f64(g_pre), _f64(w)
    k = w.shape[2]
    pad = k // 2
    B, _, Hout, p = g_pre.shape
    assert Hout == (H + 2 * pad - k) // stride + 1
    dxp = np.zeros((B, w.shape[1], H + 2 * pad, p))
    for j in range(k):
        dxp[:, :, j:j + stride * (Hout - 1) + 1:stride, :] += np.einsum("oc,bohp->bchp", w[:, :, j], g_pre,
                                                                        optimize=True)
    return dxp[:, :, pad:pad + H, :]


def view_adjoint(gv, T):
    """The adjoint of mpd_reference.view: gv [B, 1, H, p] -> [B, 1, T]; padded sample T + i folds onto T - 2 - i."""
    gv = _f64(gv)
    flat = gv.reshape(gv.shape[0], 1, -1)
    dx = flat[..., :T].copy()
    for i in range(flat.shape[-1] - T):
        dx[..., T - 2 - i] += flat[..., T + i]
    return dx


def first_input_grad(g_pre, w, T, period):
    """fv_mpd_first_input_grad's formula: g_pre [B, 32, H1, p] (already masked), w [32, 5] -> dx [B, 1, T]."""
    H = (T + ref.reflect_tail(T, period)) // period
    return view_adjoint(conv_h_adjoint(g_pre, _f64(w).reshape(32, 1, 5), H, 3), T)


def _lists(x, sd, prefix, periods):
    return [ref.discriminator_p(x, sd, f"{prefix}discriminators.{i}", p)[:6] for i, p in periods]


def mpd_part(est, real, sd, prefix, periods, L, fm_len, est_maps=None, real_maps=None, first_list=0):
    """The MPD's share of the objective sum_i MSE(score_i, 1) / L + sum_ij L1(e_ij, r_ij) / (L fm_len) and its
    gradient.  periods: [(index of the sub-discriminator, period)]; est_maps / real_maps: per period the six maps
    whose signs decide every kink (None: float64's own).
    -> (gradient [B, 1, T], {"adversarial", "feature_map"} contributions, differing decisions)."""
    est = _f64(est)
    T = est.shape[-1]
    e_all = _lists(est, sd, prefix, periods)
    r_all = None if real is None else _lists(_f64(real), sd, prefix, periods)
    grad = np.zeros_like(est)
    terms = {"adversarial": 0.0, "feature_map": 0.0}
    differ = []
    for q, (i, p) in enumerate(periods):
        e, r = e_all[q], None if r_all is None else r_all[q]
        dec = e if est_maps is None else [_f64(m).reshape(o.shape) for m, o in zip(est_maps[q][:6], e)]
        rdec = r if (real_maps is None or r is None) else [_f64(m).reshape(o.shape)
                                                           for m, o in zip(real_maps[q][:6], r)]
        terms["adversarial"] += ((e[5] - 1) ** 2).mean() / L
        g_map = [None] * 6
        g_map[5] = 2 * (e[5] - 1) / (L * e[5].size)
        if r is not None:
            for j in range(6):
                sgn = np.sign(dec[j] - rdec[j])
                terms["feature_map"] += (sgn * (e[j] - r[j])).mean() / (L * fm_len)
                g = sgn / (L * fm_len * e[j].size)
                g_map[j] = g if g_map[j] is None else g_map[j] + g
                d = e[j] - r[j]
                bad = np.sign(d) != sgn
                if bad.any():
                    pk = max(np.abs(e[j]).max(), np.abs(r[j]).max())
                    differ.append((first_list + q, j, int(bad.sum()), float(np.abs(d[bad]).max() / pk), "sign(e - r)"))
        for j in range(5):
            bad = (e[j] > 0) != (dec[j] > 0)
            if bad.any():
                differ.append((first_list + q, j, int(bad.sum()),
                               float(np.abs(e[j][bad]).max() / np.abs(e[j]).max()), "mask"))
        hs = [(T + ref.reflect_tail(T, p)) // p] + [m.shape[2] for m in e]
        g_up = None
        for j in range(5, -1, -1):
            g = g_map[j] if g_up is None else (g_up if g_map[j] is None else g_up + g_map[j])
            if g is None:
                continue
            if j < 5:
                g = mask(g, dec[j])
            name = f"{prefix}discriminators.{i}.convs.{j}" if j < 5 else f"{prefix}discriminators.{i}.conv_post"
            g_up = conv_h_adjoint(g, ref.folded(sd, name)[0], hs[j], ref.LAYERS[j][3])
        grad += view_adjoint(g_up, T)
    return grad, terms, differ


def objective_grad(kind, est, real, sd, est_maps=None, real_maps=None, period=None):
    """d(adversarial + feature_map)/d est in float64 (``real`` None: adversarial alone) of ``kind``: "p" (one
    DiscriminatorP(period), sd keys without prefix as DiscriminatorP's own), "mpd" or "discriminator"
    (Discriminator(use_mpd=True)).  est_maps / real_maps: nested lists as the module returns them (for "p": one
    list); every kink decision is then taken from them.
    -> (gradient float64 [B, 1, T], terms, differing decisions [(list, map, count, largest |value| / peak, kind)])."""
    if kind == "p":
        sd = {f"discriminators.0.{k}": v for k, v in sd.items()}
        return mpd_part(est, real, sd, "", [(0, period)], 1, 6, est_maps, real_maps)
    if kind == "mpd":
        return mpd_part(est, real, sd, "", list(enumerate(PERIODS)), 5, 6, est_maps, real_maps)
    if kind != "discriminator":
        raise ValueError(kind)
    L = 11
    g, t, differ = mpd_part(est, real, sd, "mpd.", list(enumerate(PERIODS)), L, 6,
                            None if est_maps is None else est_maps[:5], None if real_maps is None else real_maps[:5])
    g2, t2, d2 = _msd_mfd_part(est, real, sd, L, 6, None if est_maps is None else est_maps[5:],
                               None if real_maps is None else real_maps[5:])
    return g + g2, {k: t[k] + t2[k] for k in t}, differ + d2


def _msd_mfd_part(est, real, sd, L, fm_len, est_maps, real_maps):
    """The MSD's and the MFD's share, by float64 torch autograd through tests/mfd_grad_reference.py's conv stacks."""
    from tests import discriminator_reference as dref
    from tests import mfd_grad_reference as mref
    x = torch.as_tensor(_f64(est)).clone().requires_grad_(True)
    y = None if real is None else torch.as_tensor(_f64(real))

    def run(v, decisions=None):
        outs, cur = [], v
        for i in range(dref.MSD_DEFAULT["scales"]):
            outs.append(mref.typed_conv_stack(cur, sd, f"msd.discriminators.{i}", lambda s: 10 * s + 1, torch.float64,
                                              channels=16, downsample_scales=(4, 4, 4, 4),
                                              decisions=None if decisions is None else decisions[i]))
            cur = dref.avg_pool(cur, *dref.MSD_DEFAULT["pool"])
        for i, (nf, hop, wl) in enumerate(dref.MFD_RESOLUTIONS):
            outs.append(mref.stft_disc(v[:, 0], sd, f"mfd.stft_discriminator.{i}", fft_size=nf, shift_size=hop,
                                       win_length=wl, decisions=None if decisions is None else decisions[3 + i]))
        return outs

    dec = None if est_maps is None else [[torch.as_tensor(_f64(m)) for m in lst] for lst in est_maps]
    e = run(x, dec)
    with torch.no_grad():
        own = run(x.detach())
        r = None if y is None else run(y)
    rdec = r if (real_maps is None or r is None) else [[torch.as_tensor(_f64(m)) for m in lst] for lst in real_maps]
    adv, fm, differ = 0.0, 0.0, []
    for i, lst in enumerate(e):
        adv = adv + ((lst[-1] - 1) ** 2).mean() / L
        for j in range(len(lst) - 1):
            d_own = dec[i][j] if dec is not None else own[i][j]
            bad = (own[i][j] > 0) != (d_own > 0)
            if bad.any():
                differ.append((5 + i, j, int(bad.sum()), float(own[i][j][bad].abs().max() / own[i][j].abs().max()),
                               "mask"))
            if r is None:
                continue
            sgn = torch.sign(d_own - rdec[i][j])
            fm = fm + (sgn * (lst[j] - r[i][j])).mean() / (L * fm_len)
            d = own[i][j] - r[i][j]
            bad = torch.sign(d) != sgn
            if bad.any():
                pk = max(float(own[i][j].abs().max()), float(r[i][j].abs().max()))
                differ.append((5 + i, j, int(bad.sum()), float(d[bad].abs().max()) / pk, "sign(e - r)"))
    (adv + fm).backward()
    return x.grad.numpy().astype(np.float64), {"adversarial": float(adv.detach()), "feature_map": float(fm.detach()) if torch.is_tensor(fm) else fm}, differ


def kink_count(kind, est, real, sd, period=None, rel=KINK_BAND):
    """How many float64 values of the MPD part sit within ``rel`` x their map's largest magnitude of a kink: the
    pre-activations of the five activated maps (a leaky ReLU keeps the sign) and e - r of all six."""
    if kind == "p":
        sd = {f"discriminators.0.{k}": v for k, v in sd.items()}
        periods = [(0, period)]
    else:
        periods = list(enumerate(PERIODS))
    pre = "mpd." if kind == "discriminator" else ""
    e_all, r_all = _lists(_f64(est), sd, pre, periods), _lists(_f64(real), sd, pre, periods)
    count = 0
    for e, r in zip(e_all, r_all):
        for j in range(6):
            if j < 5:
                v = np.where(e[j] > 0, e[j], e[j] / SLOPE)
                count += int((np.abs(v) <= rel * np.abs(v).max()).sum())
            count += int((np.abs(e[j] - r[j]) <= rel * max(np.abs(e[j]).max(), np.abs(r[j]).max())).sum())
    return count


# ---- the same chain as torch conv2d in a chosen dtype (float32: the yardstick) ----
def _folded_t(sd, prefix, dtype):
    v = torch.as_tensor(np.asarray(sd[f"{prefix}.weight_v"])).to(dtype)
    g = torch.as_tensor(np.asarray(sd[f"{prefix}.weight_g"])).to(dtype)
    return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1)), torch.as_tensor(np.asarray(sd[f"{prefix}.bias"])).to(dtype)


def typed_disc_p(x, sd, prefix, period, dtype):
    """x [B, 1, T] tensor -> the six maps and the score [B, 1, H p] on x's graph."""
    T = x.shape[-1]
    n_pad = ref.reflect_tail(T, period)
    if n_pad:
        x = F.pad(x, (0, n_pad), "reflect")
    x = x.view(x.shape[0], 1, -1, period)
    outs = []
    for j, (_, _, k, s) in enumerate(ref.LAYERS):
        w, b = _folded_t(sd, f"{prefix}.convs.{j}" if j < 5 else f"{prefix}.conv_post", dtype)
        x = F.conv2d(x, w, b, stride=(s, 1), padding=(k // 2, 0))
        if j < 5:
            x = F.leaky_relu(x, SLOPE)
        outs.append(x)
    return outs + [x.flatten(1).unsqueeze(1)]


def eager_grad(kind, est, real, sd, dtype=torch.float32, period=None):
    """objective_grad by torch autograd in ``dtype`` ("p" or "mpd") -> (gradient float64 numpy, est maps, real maps)."""
    if kind == "p":
        sd = {f"discriminators.0.{k}": v for k, v in sd.items()}
        periods = [(0, period)]
    else:
        periods = list(enumerate(PERIODS))
    x = torch.as_tensor(np.asarray(est)).to(dtype).clone().requires_grad_(True)
    e = [typed_disc_p(x, sd, f"discriminators.{i}", p, dtype) for i, p in periods]
    L = len(e)
    loss = sum(((lst[-1] - 1) ** 2).mean() for lst in e) / L
    r = None
    if real is not None:
        with torch.no_grad():
            y = torch.as_tensor(np.asarray(real)).to(dtype)
            r = [typed_disc_p(y, sd, f"discriminators.{i}", p, dtype) for i, p in periods]
        loss = loss + sum((a - b).abs().mean() for le, lr in zip(e, r) for a, b in zip(le[:-1], lr[:-1])) / (L * 6)
    loss.backward()
    maps = lambda lists: None if lists is None else [[m.detach().numpy() for m in lst] for lst in lists]  # noqa: E731
    return x.grad.numpy().astype(np.float64), maps(e), maps(r)


def period_conv_inputs(cin, cout, p, H, B=2, seed=None):
    """Seeded float32 inputs of one strided layer's data gradient: w [cout, cin, 5], g_up, g_map, y [B, cout, H', p]."""
    rs = np.random.RandomState(cin + cout + 31 * p + H if seed is None else seed)
    hout = (H - 1) // 3 + 1
    w = (rs.randn(cout, cin, 5) / np.sqrt(5 * cin)).astype(np.float32)
    g_up, g_map, y = (rs.randn(B, cout, hout, p).astype(np.float32) for _ in range(3))
    return w, g_up, g_map, y


def period_conv_input_grad(g_up, g_map, y, w, H, slope=SLOPE):
    """fv_period_conv_input_grad's formula in float64 (g_up or g_map may be None; y None: no mask)."""
    g = _f64(g_up if g_up is not None else g_map)
    if g_up is not None and g_map is not None:
        g = g + _f64(g_map)
    if y is not None:
        g = mask(g, y, slope)
    return conv_h_adjoint(g, w, H, 3)
