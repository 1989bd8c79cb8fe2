"""Float64 numpy restatement of the reference's multi-period discriminator (model/discriminator/mpd.py:131-164
DiscriminatorP, :288-304 MultiPeriodDiscriminator), written from its formulas; the oracle of tests/test_gpu_mpd.py.

DiscriminatorP(p) on x [B, 1, T]:
  1. n_pad = p - T % p samples of reflect padding on the right when T % p != 0 (index T + i reads x[T - 2 - i]);
     n_pad >= T is refused, as torch's pad refuses it;
  2. the padded signal viewed as [B, 1, H, p], H = (T + n_pad) / p: flat sample n is (h, c) = (n // p, n % p);
  3. four convs along h with 5 taps, stride 3 and 2 zero rows on either side (1 -> 32 -> 128 -> 512 -> 1024), one
     with 5 taps and stride 1 (1024 -> 1024), each followed by leaky_relu(0.1), then one with 3 taps, stride 1 and 1
     zero row (1024 -> 1) without activation; every output is a feature map; H' = (H + 2 pad - k) // stride + 1;
  4. every conv is weight-normed: w = v * g / ||v|| with the norm over all dims but the first.
The score is the last map flattened, [B, 1, H_6 p]."""
import numpy as np

PERIODS = (2, 3, 5, 7, 11)
SLOPE = 0.1
# (Cout, Cin, taps, stride) of convs.0 .. convs.4 and conv_post
LAYERS = ((32, 1, 5, 3), (128, 32, 5, 3), (512, 128, 5, 3), (1024, 512, 5, 3), (1024, 1024, 5, 1), (1, 1024, 3, 1))


def folded(sd, prefix):
    """(w [Cout, Cin, k], bias [Cout]) float64 of the weight-normed Conv2d at ``prefix`` (weights [Cout, Cin, k, 1])."""
    v = np.asarray(sd[f"{prefix}.weight_v"], np.float64)
    g = np.asarray(sd[f"{prefix}.weight_g"], np.float64)
    norm = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(1))
    w = v * (g.reshape(-1) / norm).reshape(-1, 1, 1, 1)
    return w[..., 0], np.asarray(sd[f"{prefix}.bias"], np.float64)


def reflect_tail(T, period):
    """Samples appended to T."""
    return period - T % period if T % period else 0


def min_length(periods=PERIODS):
    """Shortest T from which on every period's tail is shorter than the signal (so that every T' >= T is accepted)."""
    t = max(periods)
    while t > 1 and all(reflect_tail(t - 1, p) < t - 1 for p in periods):
        t -= 1
    return t


def heights(T, period):
    """[H, H_1, ..., H_6]: the height of the view and of the six maps."""
    hs = [(T + reflect_tail(T, period)) // period]
    for _, _, k, s in LAYERS:
        hs.append((hs[-1] + 2 * (k // 2) - k) // s + 1)
    return hs


def view(x, period):
    """x [B, 1, T] -> [B, 1, H, period] after the reflect tail."""
    x = np.asarray(x, np.float64)
    T = x.shape[-1]
    n_pad = reflect_tail(T, period)
    if n_pad >= T:
        raise ValueError(f"reflect padding of {n_pad} samples on a signal of {T}")
    if n_pad:
        x = np.concatenate([x, x[..., T - 2 - np.arange(n_pad)]], axis=-1)
    return x.reshape(x.shape[0], 1, -1, period)


def conv_h(x, w, b, stride, slope=None):
    """x [B, Cin, H, p], w [Cout, Cin, k] -> [B, Cout, H', p]: k taps along h, (k - 1) / 2 zero rows on either side."""
    k = w.shape[2]
    pad = k // 2
    H = x.shape[2]
    Hout = (H + 2 * pad - k) // stride + 1
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (0, 0)))
    y = np.zeros((x.shape[0], w.shape[0], Hout, x.shape[3]))
    for j in range(k):
        rows = xp[:, :, j:j + stride * (Hout - 1) + 1:stride, :]
        y += np.einsum("oc,bchp->bohp", w[:, :, j], rows, optimize=True)
    y += b.reshape(1, -1, 1, 1)
    return y if slope is None else np.where(y >= 0, y, y * slope)


def discriminator_p(x, sd, prefix, period, layers=6):
    """x [B, 1, T] -> the first ``layers`` feature maps, and with all six also the score [B, 1, H_6 p]."""
    x = view(x, period)
    outs = []
    for j, (_, _, _, stride) in enumerate(LAYERS[:layers]):
        name = f"{prefix}.convs.{j}" if j < 5 else f"{prefix}.conv_post"
        w, b = folded(sd, name)
        x = conv_h(x, w, b, stride, SLOPE if j < 5 else None)
        outs.append(x)
    if layers == 6:
        outs.append(x.reshape(x.shape[0], 1, -1))
    return outs


def mpd(x, sd, prefix=""):
    """MultiPeriodDiscriminator on x [B, 1, T]: five lists of six maps and the score."""
    pre = f"{prefix}." if prefix else ""
    return [discriminator_p(x, sd, f"{pre}discriminators.{i}", p) for i, p in enumerate(PERIODS)]


def discriminator_with_mpd(x, sd):
    """Discriminator(use_mpd=True): mpd(x) + msd(x) + mfd(x), every map a float64 torch tensor."""
    import torch

    from tests import discriminator_reference as dref
    outs = [[torch.from_numpy(np.ascontiguousarray(m)) for m in lst] for lst in mpd(x, sd, "mpd")]
    return outs + dref.discriminator(x, sd)
