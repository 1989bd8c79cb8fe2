"""Sustained ms per call of audio.melspectrogram (one fv_melspectrogram launch) against the same mel computed on
the device by the eager torch chain (preemphasis, torch.stft center=True / reflect with the centred periodic Hann,
abs, matmul by the Slaney filters, log10, clip), at B = 1 and B = 64 utterances of n = 240 000 samples (1001 frames).
Prints one JSON line.  Timing: every shape warmed up first, then device events around a run of back-to-back calls
(at least ~0.5 s of device work per figure), best of three such runs.

    python tools/mel_bench.py [--n 240000] [--batches 1,64]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastvocoder_amd import audio  # noqa: E402


def eager_chain(basis, window):
    def run(x):
        p = torch.cat([x[:, :1], x[:, 1:] - 0.97 * x[:, :-1]], dim=1)
        S = torch.stft(p, 2048, hop_length=240, win_length=1200, window=window, center=True, pad_mode="reflect",
                       return_complex=True).abs()
        mel = torch.matmul(basis, S)
        return ((20 * torch.log10(torch.clamp(mel, min=1e-5)) - 20 + 100) / 100).clamp(0, 1)
    return run


def ms_per_call(fn, x, target_s=0.5):
    for _ in range(3):
        fn(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(x)
    e1.record()
    e1.synchronize()
    reps = max(5, min(2000, int(target_s * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    best = float("inf")
    for _ in range(3):
        e0.record()
        for _ in range(reps):
            fn(x)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=240000)
    ap.add_argument("--batches", default="1,64")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mel_bench measures on the ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    basis = torch.from_numpy(audio._build_mel_basis()).float().to(dev)
    window = torch.hann_window(1200, periodic=True, dtype=torch.float32, device=dev)
    eager = eager_chain(basis, window)
    T = 1 + args.n // 240
    out = {"tool": "mel_bench", "n": args.n, "frames_per_utterance": T, "device": torch.cuda.get_device_name(dev)}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            x = torch.from_numpy(np.random.RandomState(B).uniform(-1, 1, (B, args.n)).astype(np.float32)).to(dev)
            fused = ms_per_call(audio.melspectrogram, x)
            row = {"fused_ms": round(fused, 4), "fused_frames_per_s": round(B * T / fused * 1e3)}
            try:
                diff = float((eager(x) - audio.melspectrogram(x)).abs().max())
                ms = ms_per_call(eager, x)
                row.update(torch_ms=round(ms, 4), torch_frames_per_s=round(B * T / ms * 1e3),
                           speedup=round(ms / fused, 2), max_abs_diff_vs_torch=diff)
            except RuntimeError as e:       # torch.stft not available on the device
                row.update(torch_ms=None, torch_frames_per_s=None, speedup=None, torch_error=str(e)[:200])
            out[f"B{B}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
