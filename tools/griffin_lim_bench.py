"""Sustained ms per call of the GPU Griffin-Lim (fv_griffin_lim: two launches per iteration, the projection with the
frame resident in LDS and the overlap-add gather) against the same iteration written as the eager torch chain on the
same device (torch.istft / torch.stft with the centred periodic Hann, the phase normalised as X / |X| with 1 for a zero
bin, in a Python loop), at B = 1 and B = 16 spectrograms of T = 1001 frames, 60 iterations.  Both start from the same
S and initial phase, so the eager chain doubles as a third opinion on correctness (max |difference| relative to the
peak, after 2 iterations -- before the float32 drift of the iteration separates any two implementations -- and after
all of them).  Also times the whole audio.inv_mel_spectrogram on device mels (mel -> S, Griffin-Lim, inverse
preemphasis; the host draw and upload of the initial phase excluded: angles are given as a device-resident phase).
Prints one JSON line.  Timing: every shape warmed up first, then device events around a run of back-to-back calls
(at least ~0.5 s of device work per figure), best of three such runs.

    python tools/griffin_lim_bench.py [--frames 1001] [--batches 1,16] [--iters 60]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastvocoder_amd import _native, audio, hparams  # noqa: E402


def eager_chain(window, iters):
    kw = dict(n_fft=2048, hop_length=240, win_length=1200, window=window, center=True)

    def run(S, phase0):
        """S [B, 1025, T] fp32, phase0 [B, 1025, T] complex64 -> y [B, 240 (T - 1)]"""
        y = torch.istft(S * phase0, **kw)
        for _ in range(iters):
            X = torch.stft(y, pad_mode="reflect", return_complex=True, **kw)
            mag = X.abs()
            ph = torch.where(mag > 0, X / mag.clamp_min(1e-30), torch.ones_like(X))
            y = torch.istft(S * ph, **kw)
        return y
    return run


def ms_per_call(fn, target_s=0.5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    reps = max(3, min(2000, int(target_s * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    best = float("inf")
    for _ in range(3):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1001)
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--iters", type=int, default=hparams.griffin_lim_iters)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "griffin_lim_bench measures on the ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    window = torch.hann_window(1200, periodic=True, dtype=torch.float32, device=dev)
    tab = audio.griffin_lim_tables(dev)
    T = args.frames
    out = {"tool": "griffin_lim_bench", "frames": T, "iters": args.iters, "device": torch.cuda.get_device_name(dev)}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            rs = np.random.RandomState(B)
            mel = torch.from_numpy(rs.rand(B, 80, T).astype(np.float32)).to(dev)
            S = audio._mel_to_linear_device(mel, hparams.power)                       # [B, T, 1025]
            ph = audio._initial_phase(None, B, B, T, dev)                             # [B, T, 1025] complex64
            St, pht = S.transpose(1, 2).contiguous(), ph.transpose(1, 2).contiguous()  # torch's [B, 1025, T]

            def fused(iters=args.iters):
                return _native.griffin_lim(S, ph, tab, iters)

            def whole():
                return _native.inv_preemphasis(_native.griffin_lim(audio._mel_to_linear_device(mel, hparams.power),
                                                                   ph, tab, args.iters), hparams.preemphasis)
            ms = ms_per_call(fused)
            row = {"fused_ms": round(ms, 4), "fused_us_per_iteration": round(ms / max(args.iters, 1) * 1e3, 2),
                   "fused_frame_iterations_per_s": round(B * T * args.iters / ms * 1e3),
                   "inv_mel_spectrogram_ms": round(ms_per_call(whole), 4)}
            try:
                def rel(a, b):
                    return float((a - b).abs().max() / b.abs().max())
                row["max_rel_diff_vs_torch_2_iterations"] = rel(fused(2), eager_chain(window, 2)(St, pht))
                eager = eager_chain(window, args.iters)
                row["max_rel_diff_vs_torch"] = rel(fused(), eager(St, pht))
                tms = ms_per_call(lambda: eager(St, pht))
                row.update(torch_ms=round(tms, 4), speedup=round(tms / ms, 2))
            except RuntimeError as e:       # torch.stft / torch.istft not available on the device
                row.update(torch_ms=None, speedup=None, torch_error=str(e)[:200])
            out[f"B{B}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
