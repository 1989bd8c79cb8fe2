"""The oracle of the STFT and period discriminators' parameter gradient (csrc/mpd_wgrad.hip, DESIGN.md section 4.15;
fastvocoder_amd.loss.discriminator_step_terms(..., stft_grad=True, period_grad=True)).

  * period_conv_weight_grad / first_weight_grad: the float64 numpy closed forms of the two new kernels, written from
    their definitions;
  * run / param_grad: the discriminators in torch with the state dict's entries as leaves of the graph (weight norm
    folded inside it), float64 for the oracle, float32 for the yardstick; d(real + fake)/d(every entry) of
    bin/train.py:157-169 for "stft", "mfd", "p", "mpd", "discriminator" (MSD + MFD) and "discriminator_mpd".  With
    ``est_maps`` / ``real_maps`` every leaky ReLU takes its side of zero from the sign of the given maps;
  * unresolved_count: the pre-activations of either signal inside the float32-unresolvable band of a kink;
  * YARDSTICK: the float32 eager-autograd error against float64 per case family.
tests/test_mpd_wgrad_host.py pins the pieces to each other and to the reference's own gradient
(tests/golden/mpd_mfd_param_grad.npz); tests/test_gpu_mpd_wgrad.py compares the kernels with them."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import discriminator_reference as dref
from tests import mfd_grad_reference as mfr
from tests import mpd_grad_reference as mgr
from tests import mpd_reference as ref
from tests import msd_wgrad_reference as mw

PERIODS = ref.PERIODS
UNRESOLVED = mgr.UNRESOLVED                       # 3e-7 of a map's peak: the band of tests/test_mpd_grad_host.py
# (Cin, Cout, k, stride) of the layers fv_period_conv_weight_grad serves
KERNEL_LAYERS = ((32, 128, 5, 3), (128, 512, 5, 3), (512, 1024, 5, 3), (1024, 1024, 5, 1), (1024, 1, 3, 1))
SMALL_STFT = dict(fft_size=512, shift_size=50, win_length=240, channels=8, max_downsample_channels=32,
                  downsample_scales=[2, 2])
WEIGHT_SEEDS = {"p": 31, "stft": 32, "mfd": 33, "mpd": 34, "discriminator": 35, "discriminator_mpd": 36}
TINY_T = {2: 301, 3: 400, 5: 523, 7: 611, 11: 700}           # one DiscriminatorP per period, B = 2
SMALL_STFT_T = 700
FULL_T = 1703                                     # just above Discriminator().min_length() = 1680; T % p != 0 for every period
# the signal seeds of the chain cases, found by tests/test_mpd_wgrad_host.py's search (no pre-activation of either
# signal inside the UNRESOLVED band): {case: seed}
SIGNAL_SEEDS = {"p2": 0, "p3": 0, "p5": 0, "p7": 1, "p11": 1, "stft": 0}
FULL_SIGNAL_SEEDS = {"mfd": 5, "mpd": 37, "discriminator": 10, "discriminator_mpd": 18}
SAMPLE = 160                                      # golden: tensors above this many entries keep a strided sample
# The error of float32 eager autograd (torch on the CPU) against float64 per case family, relative to the peak of each
# tensor, the worst tensor of the family; tests/test_mpd_wgrad_host.py computes it on YARDSTICK_THREADS threads and
# asserts these figures within 5 %; the GPU bounds of tests/test_gpu_mpd_wgrad.py are 10 x these.
YARDSTICK_THREADS = 4
YARDSTICK = {"period_conv": 6.03e-7, "conv_post": 5.38e-5, "first": 1.20e-6, "mfd_first": 1.99e-7, "p": 1.263e-6, "stft": 8.295e-7,
             "full": 2.241e-6}


def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, np.float64)


# ---- the closed forms of the kernels ----
def period_conv_weight_grad(g_pre, x, k, stride):
    """dW[co, ci, j] = sum_{b, h', c} g_pre[b, co, h', c] x[b, ci, stride h' + j - (k - 1) / 2, c] (0 outside the
    rows), db[co] = sum g_pre[b, co]: g_pre [B, Cout, H', p], x [B, Cin, H, p] -> (dw [Cout, Cin, k], db [Cout])."""
    g_pre, x = _f64(g_pre), _f64(x)
    pad = (k - 1) // 2
    hout = g_pre.shape[2]
    assert hout == (x.shape[2] - 1) // stride + 1
    need = stride * (hout - 1) + k
    xp = np.pad(x, ((0, 0), (0, 0), (pad, max(pad, need - pad - x.shape[2])), (0, 0)))
    dw = np.zeros((g_pre.shape[1], x.shape[1], k))
    for j in range(k):
        dw[:, :, j] = np.einsum("bohp,bihp->oi", g_pre, xp[:, :, j:j + stride * (hout - 1) + 1:stride, :],
                                optimize=True)
    return dw, g_pre.sum(axis=(0, 2, 3))


def first_weight_grad(g_pre, x, period):
    """The same for the first layer, straight from the waveform x [B, 1, T]: the reflect tail and the [H, p] view of
    mpd_reference.view, then 5 taps at stride 3 -> (dw [32, 5], db [32])."""
    dw, db = period_conv_weight_grad(g_pre, ref.view(x, period), 5, 3)
    return dw[:, 0, :], db


def kernel_inputs(cin, cout, k, stride, p, H, B):
    """Seeded float32 (g_pre [B, cout, H', p], x [B, cin, H, p])."""
    rs = np.random.RandomState(cin + 3 * cout + 31 * p + 7 * H + B)
    hout = (H - 1) // stride + 1
    return rs.randn(B, cout, hout, p).astype(np.float32), rs.randn(B, cin, H, p).astype(np.float32)


def first_inputs(p, T, B):
    rs = np.random.RandomState(1000 + 31 * p + T + B)
    H = (T + ref.reflect_tail(T, p)) // p
    return rs.randn(B, 32, (H - 1) // 3 + 1, p).astype(np.float32), rs.uniform(-0.8, 0.8, (B, 1, T)).astype(np.float32)


def eager_weight_grad(g_pre, x, k, stride, dtype=torch.float32):
    """period_conv_weight_grad by torch autograd of conv2d in ``dtype`` -> (dw, db) float64 numpy."""
    g, xx = torch.as_tensor(np.asarray(g_pre)).to(dtype), torch.as_tensor(np.asarray(x)).to(dtype)
    w = torch.zeros((g.shape[1], xx.shape[1], k, 1), dtype=dtype, requires_grad=True)
    b = torch.zeros((g.shape[1],), dtype=dtype, requires_grad=True)
    (F.conv2d(xx, w, b, stride=(stride, 1), padding=((k - 1) // 2, 0)) * g).sum().backward()
    return w.grad[..., 0].numpy().astype(np.float64), b.grad.numpy().astype(np.float64)


def eager_first_weight_grad(g_pre, x, period, dtype=torch.float32):
    xx = torch.as_tensor(np.asarray(x)).to(dtype)
    n_pad = ref.reflect_tail(xx.shape[-1], period)
    if n_pad:
        xx = F.pad(xx, (0, n_pad), "reflect")
    dw, db = eager_weight_grad(g_pre, xx.view(xx.shape[0], 1, -1, period).numpy(), 5, 3, dtype)
    return dw[:, 0, :], db


def eager_dense_weight_grad(g_pre, x, k, pad, dtype=torch.float32):
    """The reflect-padded stride-1 conv1d's weight and bias gradient by torch autograd in ``dtype``."""
    g, xx = torch.as_tensor(np.asarray(g_pre)).to(dtype), torch.as_tensor(np.asarray(x)).to(dtype)
    w = torch.zeros((g.shape[1], xx.shape[1], k), dtype=dtype, requires_grad=True)
    b = torch.zeros((g.shape[1],), dtype=dtype, requires_grad=True)
    (F.conv1d(F.pad(xx, (pad, pad), mode="reflect"), w, b) * g).sum().backward()
    return w.grad.numpy().astype(np.float64), b.grad.numpy().astype(np.float64)


def kernel_yardsticks():
    """The float32 eager-autograd error of the kernel families at the kernel tests' largest shapes (B = 3; the height
    one row past a unit boundary; the first layer at T = 6 p + 1 and at several units; the MFD's first layer at 8 and
    33 frames): {"period_conv", "conv_post", "first", "mfd_first"}."""
    out = {"period_conv": 0.0, "conv_post": 0.0, "first": 0.0, "mfd_first": 0.0}
    for cin, cout, k, s in KERNEL_LAYERS:
        for p in PERIODS:
            H = s * ((32 if k == 5 else 1024) // p) + 1
            g, x = kernel_inputs(cin, cout, k, s, p, H, 3)
            want, got = period_conv_weight_grad(g, x, k, s), eager_weight_grad(g, x, k, s)
            fam = "period_conv" if k == 5 else "conv_post"
            out[fam] = max(out[fam], rel_err(got[0], want[0]), rel_err(got[1], want[1]))
    for p in PERIODS:
        for T in (6 * p + 1, 3 * (1024 // p) * p + 2 * p + 1):
            g, x = first_inputs(p, T, 3)
            want, got = first_weight_grad(g, x, p), eager_first_weight_grad(g, x, p)
            out["first"] = max(out["first"], rel_err(got[0], want[0]), rel_err(got[1], want[1]))
    for cin in (257, 1025):
        for frames in (8, 33):
            g, x = mfd_first_inputs(cin, frames, 3)
            got = eager_dense_weight_grad(g, x, 15, 7)
            out["mfd_first"] = max(out["mfd_first"], rel_err(got[0], mw.dense_weight_grad(g, x, 15, 7, "reflect")),
                                   rel_err(got[1], mw.bias_grad(g)))
    return out


def mfd_first_inputs(cin, frames, B):
    rs = np.random.RandomState(cin + frames + B)
    return rs.randn(B, 64, frames).astype(np.float32), rs.randn(B, cin, frames).astype(np.float32)


def signals(seed, T, B=2):
    return mgr.signals(seed, T, B)


def case_kind(name):
    """(the ``kind`` of run / param_grad, its kwargs) of a chain case: "p<period>", "stft", "mfd", "mpd",
    "discriminator" or "discriminator_mpd"."""
    if name[0] == "p":
        return "p", {"period": int(name[1:])}
    return name, (dict(SMALL_STFT) if name == "stft" else {})


def case_state_dict(name):
    """The seeded weights of a chain case ({key: float32 ndarray}, fastvocoder_amd.synthetic)."""
    from fastvocoder_amd.synthetic import seeded_discriminator_state_dict as seeded
    if name[0] == "p":
        return mgr.sub_state_dict(seeded("mpd", WEIGHT_SEEDS["p"]), PERIODS.index(int(name[1:])))
    if name == "stft":
        return seeded("stft", WEIGHT_SEEDS["stft"], **SMALL_STFT)
    if name in ("mfd", "mpd"):
        return seeded(name, WEIGHT_SEEDS[name])
    return seeded("discriminator", WEIGHT_SEEDS[name], use_mpd=name == "discriminator_mpd")


def case_signals(name, seed=None):
    """(est, real) float32 of a chain case, B = 2: (2, 1, T), for "stft" (2, T)."""
    if name in FULL_SIGNAL_SEEDS:
        return signals(FULL_SIGNAL_SEEDS[name] if seed is None else seed, FULL_T)
    seed = SIGNAL_SEEDS[name] if seed is None else seed
    if name == "stft":
        est, real = signals(seed, SMALL_STFT_T)
        return est[:, 0], real[:, 0]
    return signals(seed, TINY_T[int(name[1:])])


def case_unresolved(name, seed=None):
    """unresolved_count of both signals' float64 forwards of a chain case."""
    kind, kw = case_kind(name)
    est, real = case_signals(name, seed)
    P = {k: _leaf(v, torch.float64) for k, v in case_state_dict(name).items()}
    with torch.no_grad():
        return sum(unresolved_count(run(kind, torch.as_tensor(np.asarray(x), dtype=torch.float64), P, **kw),
                                    slopes_of(kind)) for x in (est, real))


# ---- the discriminators with the state dict's entries as leaves ----
def _fold(P, prefix):
    w = P.get(f"{prefix}.weight")
    if w is None:
        v, g = P[f"{prefix}.weight_v"], P[f"{prefix}.weight_g"]
        w = v * (g / v.flatten(1).norm(dim=1).view(-1, *([1] * (v.dim() - 1))))
    return w, P.get(f"{prefix}.bias")


def _act(v, slope, dec):
    if dec is None:
        return F.leaky_relu(v, slope)
    return v * torch.where(torch.as_tensor(_f64(dec)).reshape(v.shape) > 0, 1.0, slope).to(v.dtype)


def disc_p(x, P, prefix, period, dec=None):
    """x [B, 1, T] -> the six maps and the score [B, 1, H p] (mpd.py:131-164)."""
    pre = f"{prefix}." if prefix else ""
    n_pad = ref.reflect_tail(x.shape[-1], period)
    if n_pad:
        x = F.pad(x, (0, n_pad), "reflect")
    x = x.view(x.shape[0], 1, -1, period)
    outs = []
    for j, (_, _, k, s) in enumerate(ref.LAYERS):
        w, b = _fold(P, f"{pre}convs.{j}" if j < 5 else f"{pre}conv_post")
        x = F.conv2d(x, w, b, stride=(s, 1), padding=(k // 2, 0))
        if j < 5:
            x = _act(x, ref.SLOPE, None if dec is None else dec[j])
        outs.append(x)
    return outs + [x.flatten(1).unsqueeze(1)]


def conv_stack(x, P, prefix, tap, kernel_sizes=(5, 3), channels=64, max_downsample_channels=1024,
               downsample_scales=(4, 4), slope=0.2, dec=None, **_):
    """The layer list of MelGANDiscriminator / STFTDiscriminator (msd.py:54-103, mfd.py:76-121) on x [B, C, T]."""
    d = (lambda i: None) if dec is None else (lambda i: dec[i])
    outs, pre = [], f"{prefix}.layers" if prefix else "layers"
    k0 = int(np.prod(kernel_sizes))
    w, b = _fold(P, f"{pre}.0.1")
    x = _act(F.conv1d(F.pad(x, ((k0 - 1) // 2,) * 2, mode="reflect"), w, b), slope, d(0))
    outs.append(x)
    c = channels
    for i, s in enumerate(downsample_scales):
        k = tap(s)
        w, b = _fold(P, f"{pre}.{i + 1}.0")
        x = _act(F.conv1d(x, w, b, stride=s, padding=(k - 1) // 2, groups=c // 4), slope, d(i + 1))
        outs.append(x)
        c = min(c * s, max_downsample_channels)
    n = len(downsample_scales) + 1
    w, b = _fold(P, f"{pre}.{n}.0")
    x = _act(F.conv1d(x, w, b, padding=(kernel_sizes[0] - 1) // 2), slope, d(n))
    outs.append(x)
    w, b = _fold(P, f"{pre}.{n + 1}")
    outs.append(F.conv1d(x, w, b, padding=(kernel_sizes[1] - 1) // 2))
    return outs


def stft_disc(x, P, prefix="", fft_size=1024, shift_size=120, win_length=600, dec=None, **kw):
    """x (B, n) -> the STFTDiscriminator's maps; the clamped magnitude (mfd_grad_reference.magnitude_bins) is a
    constant of the parameters, the window the state dict's buffer."""
    win = P.get(f"{prefix}.window" if prefix else "window")
    with torch.no_grad():
        mag = mfr.magnitude_bins(x, fft_size, shift_size, win_length, None if win is None else win.detach().numpy())
    kw["downsample_scales"] = tuple(kw.get("downsample_scales", (4, 4)))
    return conv_stack(mag, P, prefix, lambda s: 6 * s + 1, dec=dec, **kw)


def _mfd(x, P, pre, dec):
    return [stft_disc(x[:, 0], P, f"{pre}stft_discriminator.{i}", nf, hop, wl, None if dec is None else dec[i])
            for i, (nf, hop, wl) in enumerate(dref.MFD_RESOLUTIONS)]


def _msd(x, P, pre, dec):
    outs = []
    for i in range(dref.MSD_DEFAULT["scales"]):
        outs.append(conv_stack(x, P, f"{pre}discriminators.{i}", lambda s: 10 * s + 1, channels=16,
                               downsample_scales=(4, 4, 4, 4), dec=None if dec is None else dec[i]))
        x = dref.avg_pool(x, *dref.MSD_DEFAULT["pool"])
    return outs


def _mpd(x, P, pre, dec):
    return [disc_p(x, P, f"{pre}discriminators.{i}", p, None if dec is None else dec[i])
            for i, p in enumerate(PERIODS)]


def run(kind, x, P, dec=None, **kw):
    """The nested map lists (the score last in each) of ``kind`` on the graph of the tensors of P: "stft" (x (B, n),
    the constructor's kwargs), "p" (period=), "mfd", "mpd", "discriminator" or "discriminator_mpd" (x (B, 1, n))."""
    if kind == "stft":
        return [stft_disc(x, P, "", dec=None if dec is None else dec[0], **kw)]
    if kind == "p":
        return [disc_p(x, P, "", kw["period"], None if dec is None else dec[0])]
    if kind == "mfd":
        return _mfd(x, P, "", dec)
    if kind == "mpd":
        return _mpd(x, P, "", dec)
    if kind == "discriminator":
        return _msd(x, P, "msd.", None if dec is None else dec[:3]) + _mfd(x, P, "mfd.", None if dec is None else dec[3:])
    if kind == "discriminator_mpd":
        return _mpd(x, P, "mpd.", None if dec is None else dec[:5]) + \
            _msd(x, P, "msd.", None if dec is None else dec[5:8]) + _mfd(x, P, "mfd.", None if dec is None else dec[8:])
    raise ValueError(kind)


def _leaf(v, dtype):
    t = torch.as_tensor(np.asarray(v))
    return (t.to(dtype) if t.is_floating_point() else t).clone()


def is_param(key):
    return key.rsplit(".", 1)[-1] in ("weight", "weight_g", "weight_v", "bias")


def param_grad(kind, est, real, sd, dtype=torch.float64, est_maps=None, real_maps=None, **kw):
    """d(real + fake)/d(every parameter of ``sd``) (bin/train.py:157-169; the estimate is a constant) by torch
    autograd in ``dtype``.  est_maps / real_maps: nested lists as ``run`` returns them, whose signs decide every leaky
    ReLU (None: the arithmetic's own).  -> ({key: float64 ndarray}, {term: float}, est maps, real maps)."""
    P = {k: _leaf(v, dtype) for k, v in sd.items()}
    for k, q in P.items():
        if is_param(k):
            q.requires_grad_(True)
    p = run(kind, torch.as_tensor(np.asarray(real), dtype=dtype), P, real_maps, **kw)
    est_p = run(kind, torch.as_tensor(np.asarray(est), dtype=dtype), P, est_maps, **kw)
    terms = mw.step_terms(est_p, p)
    terms["discriminator"].backward()
    grads = {k: (torch.zeros_like(q) if q.grad is None else q.grad).numpy().astype(np.float64)
             for k, q in P.items() if is_param(k)}
    maps = lambda lists: [[m.detach().numpy() for m in lst] for lst in lists]  # noqa: E731
    return grads, {k: float(v.detach()) for k, v in terms.items()}, maps(est_p), maps(p)


def worst_error(got, want):
    """(key, error) of the worst tensor of ``got`` against ``want``, each relative to the peak of the wanted tensor."""
    errs = {k: rel_err(got[k], want[k]) for k in want}
    k = max(errs, key=errs.get)
    return k, errs[k]


def chain_yardstick(family):
    """The float32 eager-autograd error of a chain family against float64, the worst parameter tensor of its cases:
    "p" (the five tiny DiscriminatorP cases), "stft" (the small STFTDiscriminator) or "full" (the default MFD and
    Discriminator(use_mpd=True) at FULL_T, float64 taking float32's leaky-ReLU sides)."""
    names = {"p": [f"p{p}" for p in PERIODS], "stft": ["stft"], "full": ["mfd", "discriminator_mpd"]}[family]
    worst = 0.0
    for name in names:
        kind, kw = case_kind(name)
        est, real = case_signals(name)
        sd = case_state_dict(name)
        g32, _, e32, r32 = param_grad(kind, est, real, sd, torch.float32, **kw)
        adopt = dict(est_maps=e32, real_maps=r32) if family == "full" else {}
        g64 = param_grad(kind, est, real, sd, **adopt, **kw)[0]
        worst = max(worst, worst_error(g32, g64)[1])
    return worst


def sgd_steps(kind, est, real, sd, steps, lr, **kw):
    """``steps`` plain SGD steps on real + fake in float64 -> (the loss before each step, the state dict after the
    last)."""
    sd = {k: np.asarray(v, np.float64) if is_param(k) else np.asarray(v) for k, v in sd.items()}
    losses = []
    for _ in range(steps):
        grads, terms, _, _ = param_grad(kind, est, real, sd, **kw)
        losses.append(terms["discriminator"])
        sd = {k: v - lr * grads[k] if is_param(k) else v for k, v in sd.items()}
    return losses, sd


def unresolved_count(lists, slopes, rel=UNRESOLVED):
    """How many pre-activations of the activated maps (every map of a list but its last two entries for an MPD list,
    whose score repeats conv_post, and its last for a conv stack; recovered from the stored map: a leaky ReLU keeps
    the sign) lie within ``rel`` x their map's largest magnitude of zero.  slopes: one per list."""
    count = 0
    for lst, slope in zip(lists, slopes):
        for m in (lst[:5] if slope == ref.SLOPE else lst[:-1]):
            m = _f64(m)
            pre = np.where(m > 0, m, m / slope)
            count += int((np.abs(pre) <= rel * np.abs(pre).max()).sum())
    return count


def differing_sides(own, adopted, slopes):
    """Where the activated maps ``adopted`` (another forward's) take another side of zero than float64's ``own``:
    (count, the largest float64 |value| among them relative to its map's peak)."""
    count, worst = 0, 0.0
    for lo, la, slope in zip(own, adopted, slopes):
        n = 5 if slope == ref.SLOPE else len(lo) - 1
        for o, a in zip(lo[:n], la[:n]):
            o = _f64(o)
            bad = (o > 0) != (_f64(a).reshape(o.shape) > 0)
            if bad.any():
                count += int(bad.sum())
                worst = max(worst, float(np.abs(o[bad]).max() / np.abs(o).max()))
    return count, worst


def slopes_of(kind):
    return {"stft": [0.2], "p": [0.1], "mfd": [0.2] * 3, "mpd": [0.1] * 5, "discriminator": [0.2] * 6,
            "discriminator_mpd": [0.1] * 5 + [0.2] * 6}[kind]


def sample(a):
    """The golden's view of a gradient tensor: (the whole flat tensor, or SAMPLE entries at a fixed stride; its L2
    norm)."""
    a = _f64(a).reshape(-1)
    step = max(1, a.size // SAMPLE)
    return (a if a.size <= SAMPLE else a[::step][:SAMPLE]), float(np.sqrt((a * a).sum()))


def rel_err(got, want):
    """max |got - want| relative to the peak of ``want``."""
    got, want = _f64(got), _f64(want)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
