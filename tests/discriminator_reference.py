"""Float64 torch-CPU restatement of the reference's discriminators (model/discriminator/msd.py, mfd.py,
discriminator.py) and of the scores of bin/train.py:97-117, 157-169, written from their semantics (DESIGN.md
section 4.6); the oracle of tests/test_gpu_discriminator.py.

Weights are plain dicts ``prefix -> (w [Cout, Cin/groups, k] folded, bias or None)`` keyed like the modules'
``state_dict`` (``<prefix>.weight`` / ``.weight_g`` / ``.weight_v`` / ``.bias``)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import stft_loss_reference as sref

MSD_DEFAULT = dict(scales=3, pool=(4, 2, 1), kernel_sizes=(5, 3), channels=16, max_downsample_channels=1024,
                   downsample_scales=(4, 4, 4, 4), slope=0.2)
MFD_RESOLUTIONS = ((2048, 240, 1200), (1024, 120, 600), (512, 50, 240))
STFT_DEFAULT = dict(kernel_sizes=(5, 3), channels=64, max_downsample_channels=1024, downsample_scales=(4, 4), slope=0.2)


def folded(sd, prefix):
    """(weight, bias) float64 of the conv at ``prefix`` in a state dict of numpy arrays or tensors."""
    def get(k):
        v = sd.get(f"{prefix}.{k}" if prefix else k)
        return None if v is None else torch.as_tensor(np.asarray(v), dtype=torch.float64)
    w = get("weight")
    if w is None:
        v, g = get("weight_v"), get("weight_g")
        w = v * (g / v.flatten(1).norm(dim=1).view(-1, *([1] * (v.dim() - 1))))
    return w, get("bias")


def conv_stack(x, sd, prefix, kernel_sizes, channels, max_downsample_channels, downsample_scales, slope, tap):
    """The shared layer list of MelGANDiscriminator / STFTDiscriminator on x [B, C, T] float64 -> list of outputs."""
    outs = []
    prefix = f"{prefix}.layers" if prefix else "layers"
    k0 = int(np.prod(kernel_sizes))
    w, b = folded(sd, f"{prefix}.0.1")
    x = F.leaky_relu(F.conv1d(F.pad(x, ((k0 - 1) // 2,) * 2, mode="reflect"), w, b), slope)
    outs.append(x)
    in_chs = channels
    for i, s in enumerate(downsample_scales):
        k = tap(s)
        w, b = folded(sd, f"{prefix}.{i + 1}.0")
        x = F.leaky_relu(F.conv1d(x, w, b, stride=s, padding=(k - 1) // 2, groups=in_chs // 4), slope)
        outs.append(x)
        in_chs = min(in_chs * s, max_downsample_channels)
    n = len(downsample_scales) + 1
    w, b = folded(sd, f"{prefix}.{n}.0")
    x = F.leaky_relu(F.conv1d(x, w, b, padding=(kernel_sizes[0] - 1) // 2), slope)
    outs.append(x)
    w, b = folded(sd, f"{prefix}.{n + 1}")
    outs.append(F.conv1d(x, w, b, padding=(kernel_sizes[1] - 1) // 2))
    return outs


def avg_pool(x, k, s, p):
    """AvgPool1d(k, s, p, count_include_pad=False) on [..., T]: each window's real samples, averaged."""
    xp = F.pad(x, (p, p))
    real = F.pad(torch.ones_like(x), (p, p))
    return xp.unfold(-1, k, s).sum(-1) / real.unfold(-1, k, s).sum(-1)


def melgan(x, sd, prefix, kernel_sizes=(5, 3), channels=16, max_downsample_channels=1024,
           downsample_scales=(4, 4, 4, 4), slope=0.2, **_):
    return conv_stack(x, sd, prefix, kernel_sizes, channels, max_downsample_channels, downsample_scales, slope,
                      lambda s: 10 * s + 1)


def msd(x, sd, prefix="", scales=3, pool=(4, 2, 1), **kw):
    """x [B, 1, T] -> list of each scale's outputs."""
    pre = f"{prefix}." if prefix else ""
    outs = []
    for i in range(scales):
        outs.append(melgan(x, sd, f"{pre}discriminators.{i}", **kw))
        x = avg_pool(x, *pool)
    return outs


def stft_magnitude_bins(x, n_fft, hop, win_length, window=None):
    """(B, bins, frames) float64: mfd.py's stft, which does not transpose."""
    return torch.from_numpy(sref.stft_magnitude(np.asarray(x, np.float64), n_fft, hop, win_length,
                                                window=window)).transpose(1, 2)


def stft_disc(x, sd, prefix, fft_size=1024, shift_size=120, win_length=600, kernel_sizes=(5, 3), channels=64,
              max_downsample_channels=1024, downsample_scales=(4, 4), slope=0.2, **_):
    """x [B, T] -> list of outputs; the window is the state dict's ``<prefix>.window`` buffer when it holds one."""
    win = sd.get(f"{prefix}.window" if prefix else "window")
    win = None if win is None else np.asarray(win, np.float64)
    mag = stft_magnitude_bins(x.numpy() if torch.is_tensor(x) else x, fft_size, shift_size, win_length, win)
    return conv_stack(mag, sd, prefix, kernel_sizes, channels, max_downsample_channels, downsample_scales, slope,
                      lambda s: 6 * s + 1)


def mfd(x, sd, prefix="", resolutions=MFD_RESOLUTIONS):
    """x [B, 1, T] -> list of each resolution's outputs."""
    pre = f"{prefix}." if prefix else ""
    return [stft_disc(x[:, 0], sd, f"{pre}stft_discriminator.{i}", nf, hop, wl)
            for i, (nf, hop, wl) in enumerate(resolutions)]


def discriminator(x, sd):
    """Discriminator(): msd(x) + mfd(x) on x [B, 1, T] float64."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    return msd(x, sd, "msd") + mfd(x, sd, "mfd")


def scores(est_p, p):
    """The five scores of bin/train.py, as float: the reference's formulas, term by term."""
    L = len(est_p)
    adv = sum(float(((e[-1] - 1) ** 2).mean()) for e in est_p) / L
    fm = 0.0
    for i in range(L):
        for j in range(len(est_p[i]) - 1):
            fm += float((est_p[i][j] - p[i][j]).abs().mean())
    fm /= L * (len(est_p[0]) - 1)
    real = sum(float(((r[-1] - 1) ** 2).mean()) for r in p) / L
    fake = sum(float((e[-1] ** 2).mean()) for e in est_p) / L
    return {"adversarial": adv, "feature_map": fm, "real": real, "fake": fake, "discriminator": real + fake}
