"""Seeded synthetic checkpoints and mels for the four generators.

There is no trained checkpoint in the reference tree (only a URL,
/root/reference/README.md:18) and no network, so benchmarks and parity tests run
on random-init weights of the right architecture.  This module derives the
reference's ``state_dict`` key/shape list from the yaml kwargs alone
(``*.weight_g / *.weight_v / *.bias`` with weight norm
attached, the wire format of bin/train.py:235-247) and fills it from a frozen
``numpy.random.RandomState`` stream, so the same bytes are regenerated on any
box.  Weights are gain-calibrated so the networks stay input-sensitive (with
the default init MelGAN's output moves ~1e-5 when the mel changes, which would
make a 1e-4 parity check vacuous).
"""
import numpy as np

from .generator.pqmf import design_pqmf_filters

# per-model multiplicative gain on the uniform init bound (calibrated so the
# output has std ~0.1-0.5 and depends on the mel; see tests/golden/make_golden.py)
DEFAULT_GAIN = {"hifigan": 1.9, "multiband-hifigan": 1.6, "melgan": 1.7, "basis-melgan": 1.9}


def _conv(spec, prefix, cout, cin, k, bias, wn):
    """torch.nn.Conv1d(cin, cout, k) keys; weight norm g is per OUTPUT channel."""
    if not wn:
        spec.append((prefix + ".weight", (cout, cin, k), ("v", cin * k)))
    if bias:
        spec.append((prefix + ".bias", (cout,), ("b", cin * k)))
    if wn:  # weight norm re-registers g and v after the bias
        spec.append((prefix + ".weight_g", (cout, 1, 1), ("g", prefix)))
        spec.append((prefix + ".weight_v", (cout, cin, k), ("v", cin * k)))


def _batchnorm(spec, prefix, c):
    """torch.nn.BatchNorm1d(c) keys, with non-trivial statistics so the fold is exercised."""
    spec.append((prefix + ".weight", (c,), ("u", 0.7, 1.3)))
    spec.append((prefix + ".bias", (c,), ("u", -0.2, 0.2)))
    spec.append((prefix + ".running_mean", (c,), ("u", -0.3, 0.3)))
    spec.append((prefix + ".running_var", (c,), ("u", 0.5, 1.5)))
    spec.append((prefix + ".num_batches_tracked", (), ("count",)))


def _convT(spec, prefix, cin, cout, k, stride, bias, wn):
    """torch.nn.ConvTranspose1d(cin, cout, k) keys; weight [cin,cout,k], g per INPUT channel."""
    fan = max(1, cin * k // stride)
    if not wn:
        spec.append((prefix + ".weight", (cin, cout, k), ("v", fan)))
    if bias:
        spec.append((prefix + ".bias", (cout,), ("b", fan)))
    if wn:
        spec.append((prefix + ".weight_g", (cin, 1, 1), ("g", prefix)))
        spec.append((prefix + ".weight_v", (cin, cout, k), ("v", fan)))


def state_dict_spec(model_name, cfg, weight_norm=True):
    """[(key, shape, kind)] in the reference's registration order."""
    spec = []
    if model_name in ("hifigan", "multiband-hifigan"):
        bias = cfg.get("bias", True)
        c0 = cfg["upsample_initial_channel"]
        ks, ds = cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]
        _conv(spec, "conv_pre", c0, 80, 7, bias, weight_norm)
        for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
            cin, cout = c0 // 2 ** i, c0 // 2 ** (i + 1)
            if cfg.get("transposedconv", True):
                _convT(spec, f"ups.{i}", cin, cout, k, u, bias, weight_norm)
            else:
                _conv(spec, f"ups.{i}.conv", cout, cin, k, bias, weight_norm)
        ch = c0
        for i in range(len(cfg["upsample_rates"])):
            ch = c0 // 2 ** (i + 1)
            for j, (k, d) in enumerate(zip(ks, ds)):
                p = f"resblocks.{i * len(ks) + j}"
                if str(cfg.get("resblock_type", "1")) == "1":
                    for m in range(3):
                        _conv(spec, f"{p}.convs1.{m}", ch, ch, k, bias, weight_norm)
                    for m in range(3):
                        _conv(spec, f"{p}.convs2.{m}", ch, ch, k, bias, weight_norm)
                else:
                    for m in range(2):
                        _conv(spec, f"{p}.convs.{m}", ch, ch, k, bias, weight_norm)
        _conv(spec, "conv_post", 4 if model_name == "multiband-hifigan" else 1, ch, 7, bias, weight_norm)
        if model_name == "multiband-hifigan":
            spec.append(("pqmf.analysis_filter", (4, 1, 63), ("pqmf", "analysis")))
            spec.append(("pqmf.synthesis_filter", (1, 4, 63), ("pqmf", "synthesis")))
            spec.append(("pqmf.updown_filter", (4, 4, 4), ("pqmf", "updown")))
        return spec
    if model_name in ("melgan", "basis-melgan"):
        causal = cfg.get("use_causal_conv", False)
        bias = cfg.get("bias", True)
        wn = weight_norm and cfg.get("use_weight_norm", True)
        K = cfg.get("kernel_size", 7)
        ch = cfg["channels"]
        sk, stacks = cfg.get("stack_kernel_size", 3), cfg.get("stacks", 3)
        idx = 1
        _conv(spec, f"melgan.{idx}", ch[0], cfg.get("in_channels", 80), K, bias, wn)
        idx += 1
        for i, s in enumerate(cfg["upsample_scales"]):
            idx += 1
            if cfg.get("transposedconv", True):
                _convT(spec, f"melgan.{idx}", ch[i], ch[i + 1], 2 * s, s, bias, wn)
            else:
                _conv(spec, f"melgan.{idx}.conv", ch[i + 1], ch[i], 2 * s + 1, bias, wn)
            idx += 1
            for _ in range(stacks):
                c = ch[i + 1]
                if causal:      # CausalConv1d at stack.1 (owns .conv), 1x1 at stack.3
                    _conv(spec, f"melgan.{idx}.stack.1.conv", c, c, sk, bias, wn)
                    _conv(spec, f"melgan.{idx}.stack.3", c, c, 1, bias, wn)
                else:
                    _conv(spec, f"melgan.{idx}.stack.2", c, c, sk, bias, wn)
                    _conv(spec, f"melgan.{idx}.stack.4", c, c, 1, bias, wn)
                _conv(spec, f"melgan.{idx}.skip_layer", c, c, 1, bias, wn)
                idx += 1
        if model_name == "melgan":
            _conv(spec, f"melgan.{idx}.conv", cfg.get("out_channels", 1), ch[-1], K, bias, wn)
        else:
            if cfg.get("lastlinear", False):     # LastLinear head (modules.py:116-132)
                h, o = ch[-1], cfg.get("out_channels", 256)
                for n, cout in (("1", h), ("2", o)):
                    _batchnorm(spec, f"melgan.{idx}.bn_{n}", h)
                    _conv(spec, f"melgan.{idx}.linear_{n}", cout, h, 1, bias, wn)
            spec.append(("basis_signal.layer.weight", (cfg.get("L", 30), cfg.get("out_channels", 256)),
                         ("basis", cfg.get("out_channels", 256))))
        return spec
    raise Exception("no model find!")


def seeded_state_dict(model_name, cfg, seed=0, gain=None, weight_norm=True):
    """{key: float32 ndarray}; bit-identical for a given (model, cfg, seed, gain)."""
    gain = DEFAULT_GAIN[model_name] if gain is None else gain
    return _fill(state_dict_spec(model_name, cfg, weight_norm), np.random.RandomState(seed), gain)


def _fill(spec, rng, gain):
    """Draw the values of a [(key, shape, kind)] spec from rng, in the fixed order of seeded_state_dict."""
    sd, vs = {}, {}
    # v / plain weights / biases first, in key order, then g from ||v||
    for key, shape, kind in sorted(spec, key=lambda e: e[0]):
        tag = kind[0]
        if tag in ("v", "b"):
            bound = gain / np.sqrt(kind[1])
            if tag == "b":
                bound *= 0.5
            sd[key] = rng.uniform(-bound, bound, size=shape).astype(np.float32)
            if key.endswith(".weight_v"):
                vs[key[: -len(".weight_v")]] = sd[key]
        elif tag == "u":
            sd[key] = rng.uniform(kind[1], kind[2], size=shape).astype(np.float32)
        elif tag == "count":
            sd[key] = np.array(1000, dtype=np.int64)
        elif tag == "basis":
            bound = 0.35 / np.sqrt(kind[1])
            sd[key] = rng.uniform(-bound, bound, size=shape).astype(np.float32)
    for key, shape, kind in sorted(spec, key=lambda e: e[0]):
        if kind[0] == "g":
            v = vs[kind[1]].astype(np.float64)
            nrm = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(1))
            jitter = rng.uniform(0.85, 1.15, size=nrm.shape)
            sd[key] = (nrm * jitter).astype(np.float32).reshape(shape)
        elif kind[0] == "pqmf":
            ha, hs = design_pqmf_filters()
            if kind[1] == "analysis":
                sd[key] = ha.astype(np.float32)[:, None, :]
            elif kind[1] == "synthesis":
                sd[key] = hs.astype(np.float32)[None, :, :]
            else:
                u = np.zeros((4, 4, 4), np.float32)
                for k in range(4):
                    u[k, k, 0] = 1.0
                sd[key] = u
        elif kind[0] == "window":
            n = kind[1]
            sd[key] = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)   # torch.hann_window(n)
    return {k: sd[k] for k, _, _ in spec}


# Discriminators (model/discriminator/).  The reference draws conv weights from N(0, 0.02) (msd.py:240), which leaves
# the late feature maps of a random network near-constant -- a parity check on them would be vacuous (the same lesson
# as SURVEY.md section 8c).  The uniform fan-in gain below keeps every map input-dependent (std of the last map's
# response to the input ~0.1-1 at the default configuration; tests/golden/make_discriminator_golden.py prints it).
DISCRIMINATOR_GAIN = 2.4
MSD_KW = dict(scales=3, kernel_sizes=[5, 3], channels=16, max_downsample_channels=1024, bias=True,
              downsample_scales=[4, 4, 4, 4])
STFT_KW = dict(fft_size=1024, shift_size=120, win_length=600, kernel_sizes=[5, 3], channels=64,
               max_downsample_channels=1024, bias=True, downsample_scales=[4, 4])
MFD_RESOLUTIONS = ([2048, 1024, 512], [240, 120, 50], [1200, 600, 240])


# The MPD (mpd.py:131-164).  Per-layer factors on DISCRIMINATOR_GAIN, so that every map's standard deviation stays
# near the input's: with w ~ U(-g / sqrt(fan), g / sqrt(fan)) a layer multiplies the second moment by g^2 / 3, and a
# leaky ReLU(0.1) about halves it.  The first layer sees the zero rows of the padding and the raw (zero-mean) signal,
# the last has no activation (tests/golden/make_mpd_golden.py prints every map's std; test_mpd_host.py checks them).
MPD_PERIODS = (2, 3, 5, 7, 11)
MPD_LAYER_GAIN = (1.0, 1.0, 1.0, 1.0, 1.0, 0.7)


def _conv2d(spec, prefix, cout, cin, k, factor):
    """weight-normed torch.nn.Conv2d(cin, cout, (k, 1)) keys; ``factor`` scales the gain of this layer."""
    fan = cin * k / factor ** 2
    spec.append((prefix + ".bias", (cout,), ("b", fan)))
    spec.append((prefix + ".weight_g", (cout, 1, 1, 1), ("g", prefix)))
    spec.append((prefix + ".weight_v", (cout, cin, k, 1), ("v", fan)))


def _conv_stack_spec(spec, prefix, cin, kernel_sizes, channels, max_downsample_channels, bias, downsample_scales,
                     tap, wn):
    k0 = int(np.prod(kernel_sizes))
    _conv(spec, f"{prefix}layers.0.1", channels, cin, k0, bias, wn)
    in_chs = channels
    for i, s in enumerate(downsample_scales):
        out_chs = min(in_chs * s, max_downsample_channels)
        _conv(spec, f"{prefix}layers.{i + 1}.0", out_chs, 4, tap(s), bias, wn)
        in_chs = out_chs
    n = len(downsample_scales) + 1
    out_chs = min(in_chs * 2, max_downsample_channels)
    _conv(spec, f"{prefix}layers.{n}.0", out_chs, in_chs, kernel_sizes[0], bias, wn)
    _conv(spec, f"{prefix}layers.{n + 1}", 1, out_chs, kernel_sizes[1], bias, wn)


def discriminator_spec(kind="discriminator", weight_norm=True, prefix="", **kw):
    """[(key, shape, kind)] of fastvocoder_amd.discriminator's (and the reference's) modules: kind "melgan"
    (MelGANDiscriminator), "msd" (MelGANMultiScaleDiscriminator), "stft" (STFTDiscriminator), "mfd"
    (MultiResolutionSTFTDiscriminator), "mpd" (MultiPeriodDiscriminator, no kwargs) or "discriminator"
    (Discriminator(); ``use_mpd=True`` is its only kwarg), with the shape kwargs of the constructor.  ``weight_norm``: g / v pairs (every module but a bare MelGANDiscriminator has them)."""
    spec = []
    if kind == "melgan":
        c = dict(MSD_KW, **kw)
        _conv_stack_spec(spec, prefix, 1, c["kernel_sizes"], c["channels"], c["max_downsample_channels"], c["bias"],
                         c["downsample_scales"], lambda s: 10 * s + 1, weight_norm)
    elif kind == "msd":
        c = dict(MSD_KW, **kw)
        for i in range(c.pop("scales")):
            spec += discriminator_spec("melgan", weight_norm, f"{prefix}discriminators.{i}.", **c)
    elif kind == "stft":
        c = dict(STFT_KW, **kw)
        spec.append((f"{prefix}window", (c["win_length"],), ("window", c["win_length"])))
        _conv_stack_spec(spec, prefix, c["fft_size"] // 2 + 1, c["kernel_sizes"], c["channels"],
                         c["max_downsample_channels"], c["bias"], c["downsample_scales"], lambda s: 6 * s + 1,
                         weight_norm)
    elif kind == "mfd":
        ffts, hops, wins = kw.get("fft_sizes", MFD_RESOLUTIONS[0]), kw.get("hop_sizes", MFD_RESOLUTIONS[1]), \
            kw.get("win_lengths", MFD_RESOLUTIONS[2])
        for i, (nf, hop, wl) in enumerate(zip(ffts, hops, wins)):
            spec += discriminator_spec("stft", weight_norm, f"{prefix}stft_discriminator.{i}.", fft_size=nf,
                                       shift_size=hop, win_length=wl)
    elif kind == "mpd":
        if not weight_norm or kw:
            raise ValueError("the MPD has no constructor arguments and always carries weight norm")
        for i in range(len(MPD_PERIODS)):
            chans = [(32, 1), (128, 32), (512, 128), (1024, 512), (1024, 1024)]
            for j, (cout, cin) in enumerate(chans):
                _conv2d(spec, f"{prefix}discriminators.{i}.convs.{j}", cout, cin, 5, MPD_LAYER_GAIN[j])
            _conv2d(spec, f"{prefix}discriminators.{i}.conv_post", 1, 1024, 3, MPD_LAYER_GAIN[5])
    elif kind == "discriminator":
        if kw.pop("use_mpd", False):
            spec += discriminator_spec("mpd", weight_norm, f"{prefix}mpd.")
        spec += discriminator_spec("msd", weight_norm, f"{prefix}msd.")
        spec += discriminator_spec("mfd", weight_norm, f"{prefix}mfd.")
    else:
        raise ValueError(f"unknown discriminator kind {kind!r}")
    return spec


def seeded_discriminator_state_dict(kind="discriminator", seed=0, gain=DISCRIMINATOR_GAIN, weight_norm=True, **kw):
    """{key: float32 ndarray} for discriminator_spec(kind, weight_norm, **kw); bit-identical for given arguments."""
    return _fill(discriminator_spec(kind, weight_norm, **kw), np.random.RandomState(seed), gain)


def seeded_mel(T, seed=0, batch=None):
    """U[0,1) fp32 mel, [T,80] (inference layout) or [B,80,T] (forward layout);
    the reference's normalised mel range is [0,1] (data/audio.py:159-160)."""
    rng = np.random.RandomState(1000 + seed)
    if batch is None:
        return rng.rand(T, 80).astype(np.float32)
    return rng.rand(batch, 80, T).astype(np.float32)
