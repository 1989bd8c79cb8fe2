"""The float64 error budget (tests/accuracy_budget.py) has teeth: subtle faults of the kind a kernel or a plan can
make -- injected into the fp32 ATen port, which then plays the part of a faulty GPU output -- fail it by at least 2x,
while the older bounds (1e-4 max-abs from the fp32 port; 1e-5 of the whole run for chunking) let some through.  CPU only."""
import torch
import torch.nn.functional as F

from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict
from oracle import torch_port
from tests import accuracy_budget as ab
from tests import cases

T = 64                 # frames: 15 360 samples, long enough for every layer to reach its steady state
OLD_TOL = 1e-4         # tests/test_gpu_parity.py TOL
OLD_CHUNK_TOL = 1e-5   # stitched chunks vs the whole run


def _setup(name, path):
    cfg = cases.load_conf(path)
    sd = seeded_state_dict(name, cfg, seed=0)
    mel = seeded_mel(T, seed=41)
    p32 = torch_port.inference(name, mel, torch_port.fold_state_dict(sd), cfg)
    r64 = torch_port.inference(name, mel, torch_port.fold_state_dict(sd, torch.float64), cfg, dtype=torch.float64)
    return cfg, sd, mel, p32, r64


def _nth(fn, pick, alter):
    """A wrapper of ``fn`` that hands its call number ``pick(args, kwargs)`` selects -- once -- to ``alter``."""
    count = [0, 0]

    def wrapped(*args, **kwargs):
        if pick(*args, **kwargs):
            count[0] += 1
            if count[0] == count[1]:
                return alter(*args, **kwargs)
        return fn(*args, **kwargs)

    return wrapped, count


def _faulty(monkeypatch, fn_name, pick, alter, nth):
    orig = getattr(F, fn_name)
    wrapped, count = _nth(orig, pick, lambda *a, **k: alter(orig, *a, **k))
    count[1] = nth
    monkeypatch.setattr(F, fn_name, wrapped)
    return count


def _report(what, g, p32, r64, old_ok):
    m = ab.measure(g, p32, r64)
    print(f"fault {what}: {ab.fmt(m)}; old bound {'LETS IT THROUGH' if old_ok else 'catches it'}")
    assert m["excess"] >= 2.0, (what, ab.fmt(m))
    return m


def test_budget_accepts_the_fp32_port_itself():
    """The yardstick of the yardstick: the fp32 port meets the budget by definition (1x) and the float64 port is 0."""
    _, _, _, p32, r64 = _setup("hifigan", "conf/hifigan/light.yaml")
    m = ab.check(p32, p32, r64, "fp32 port")
    assert m["max_ratio"] == 1.0 and m["rms_ratio"] == 1.0
    assert ab.check(r64, p32, r64, "float64 port")["max_err"] == 0.0


def test_f16_operands_in_one_64_channel_resblock_conv(monkeypatch):
    """The split without its low halves: one 64-channel ResBlock conv of HiFi-GAN light with x and w rounded to f16."""
    cfg, sd, mel, p32, r64 = _setup("hifigan", "conf/hifigan/light.yaml")
    folded = torch_port.fold_state_dict(sd)

    def f16(orig, x, w, b=None, *a, **k):
        return orig(x.half().float(), w.half().float(), b, *a, **k)

    count = _faulty(monkeypatch, "conv1d", lambda x, w, *a, **k: x.shape[1] == 64 and w.shape[2] > 1, f16, 5)
    g = torch_port.inference("hifigan", mel, folded, cfg)
    assert count[0] >= 5
    _report("f16 operands, one 64-ch conv", g, p32, r64, float((g - p32).abs().max()) <= OLD_TOL)


def test_bias_lost_on_the_last_37_columns_of_one_conv(monkeypatch):
    """A ragged-tile epilogue fault: one 32-channel ResBlock conv's bias missing on its last 37 output columns."""
    cfg, sd, mel, p32, r64 = _setup("hifigan", "conf/hifigan/light.yaml")
    folded = torch_port.fold_state_dict(sd)

    def no_bias_tail(orig, x, w, b=None, *a, **k):
        y = orig(x, w, b, *a, **k)
        y[..., -37:] -= b[None, :, None]
        return y

    count = _faulty(monkeypatch, "conv1d", lambda x, w, *a, **k: x.shape[1] == 32 and w.shape[0] == 32, no_bias_tail, 7)
    g = torch_port.inference("hifigan", mel, folded, cfg)
    assert count[0] >= 7
    _report("bias lost on 37 columns", g, p32, r64, float((g - p32).abs().max()) <= OLD_TOL)


def test_residual_stack_reflection_off_by_one_at_the_right_end(monkeypatch):
    """MelGAN: one ResidualStack's right-end reflection includes the edge sample ([.., c, d | d, c] for [.., c, d | c, b])."""
    cfg, sd, mel, p32, r64 = _setup("melgan", "conf/melgan/original.yaml")
    folded = torch_port.fold_state_dict(sd)

    def edge_included(orig, x, pad, mode="constant", *a, **k):
        y = orig(x, pad, mode, *a, **k)
        p = pad[1]
        y[..., -p:] = x[..., -p:].flip(-1)
        return y

    # reflect pads in call order: the first conv, 3 stacks per upsampler (dilations 1, 3, 9), the last layer;
    # call 11 is the 4th upsampler's d = 3 stack, at full rate
    count = _faulty(monkeypatch, "pad", lambda x, pad, mode="constant", *a, **k: mode == "reflect", edge_included, 11)
    g = torch_port.inference("melgan", mel, folded, cfg)
    assert count[0] == 14
    _report("reflection off by one", g, p32, r64, float((g - p32).abs().max()) <= OLD_TOL)


def _receptive_halo(cfg, sd, hop):
    """Frames of context per side that one frame's output samples depend on (HiFi-GAN trunk), by autograd."""
    folded = torch_port.fold_state_dict(sd, torch.float64)
    n, f = 96, 48
    x = torch.from_numpy(seeded_mel(n, seed=2).T[None].copy()).double().requires_grad_(True)
    y = torch_port.hifigan_trunk(x, folded, cfg)
    y[0, 0, f * hop:(f + 1) * hop].sum().backward()
    frames = torch.nonzero(x.grad[0].abs().sum(0)).flatten()
    lo, hi = int(frames.min()), int(frames.max())
    assert 0 < lo and hi < n - 1, (lo, hi)
    return max(f - lo, hi - f)


def _chunked(name, mel, sd, cfg, chunk, halo, hop, dtype=torch.float32):
    """The port over chunks with ``halo`` frames of context, stitched the way NativeModule._run_chunked does."""
    Tm = mel.shape[0]
    pieces = []
    for a in range(0, Tm, chunk):
        b = min(Tm, a + chunk)
        lo, hi = max(0, a - halo), min(Tm, b + halo)
        y = torch_port.inference(name, mel[lo:hi], sd, cfg, dtype=dtype)
        pieces.append(y[(a - lo) * hop:(b - lo) * hop])
    return torch.cat(pieces)


def test_chunk_halo_one_frame_short():
    """Time-chunked evaluation (chunks of 16 frames) whose halo is one frame short of the context that matters.  The
    structural receptive field of HiFi-GAN light is 14 frames per side, but its outermost two frames reach the output
    through edge taps only, below fp32 resolution: with 13 or 12 frames the stitched output is still inside the budget
    (no bound could tell it from the whole run).  12 is the halo that matters; with 11 the budget fails."""
    cfg, sd, mel, p32, r64 = _setup("hifigan", "conf/hifigan/light.yaml")
    folded = torch_port.fold_state_dict(sd)
    hop = 240
    halo = _receptive_halo(cfg, sd, hop)
    assert halo == 14
    for h in (halo, halo - 1, halo - 2):
        ok = _chunked("hifigan", mel, folded, cfg, 16, h, hop)
        assert ok.shape == p32.shape
        ab.check(ok, p32, r64, f"chunks of 16 with a halo of {h}")
    g = _chunked("hifigan", mel, folded, cfg, 16, halo - 3, hop)
    print(f"receptive halo {halo} frames, {halo - 2} of them above fp32 resolution; chunks of 16 with {halo - 3}")
    _report(f"chunk halo one frame short ({halo - 3} for {halo - 2}), vs 1e-5 of the whole run", g, p32, r64,
            float((g - p32).abs().max()) <= OLD_CHUNK_TOL)
    _report(f"chunk halo one frame short ({halo - 3} for {halo - 2}), vs 1e-4 of the port", g, p32, r64,
            float((g - p32).abs().max()) <= OLD_TOL)
