"""Sustained ms per call of the GPU resampler (audio.resample, one fv_resample launch) for 48000 -> 24000 and
44100 -> 24000 at 64 waveforms of 10 s, float32 and int16 input, beside

- scipy.signal.resample_poly with the SAME FIR on the host (one waveform, times 64): what a user without this kernel
  would run in place of resampy; its result doubles as a second opinion (max |difference|);
- the HBM bytes the launch must move (the input once, the output once, the table once), as the time those bytes take
  at the device's peak bandwidth and as the bandwidth the kernel achieved on them; and the FMAs it executes (taps per
  output) as achieved GFLOP/s.  The kernel is an fp32 FIR of 140-550 taps per output: compute, not HBM, bounds it.
Prints one JSON line.  Timing: every shape warmed up first, then device events around a run of back-to-back calls (at
least ~0.5 s of device work per figure), best of three such runs; the host figure is the best of three calls.

    python tools/resample_bench.py [--batch 64] [--seconds 10] [--pairs 48000:24000,44100:24000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.signal
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastvocoder_amd import audio  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12       # MI355X HBM3E


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


def host_fir(orig_sr, target_sr):
    """(L, M, hf): the table's filter as the FIR resample_poly(x, L, M, window=hf) / L applies."""
    L, M, scale, _ = audio._resample_geometry(orig_sr, target_sr)
    reach = int(np.ceil(audio.RESAMPLE_NUM_ZEROS * L / scale))
    u = scale * np.arange(-reach, reach + 1) / L
    inside = np.abs(u) < audio.RESAMPLE_NUM_ZEROS
    arg = np.sqrt(np.where(inside, 1.0 - (u / audio.RESAMPLE_NUM_ZEROS) ** 2, 0.0))
    return L, M, scale * np.where(inside, np.sinc(u) * np.i0(audio.RESAMPLE_BETA * arg) / np.i0(audio.RESAMPLE_BETA), 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--pairs", default="48000:24000,44100:24000")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resample_bench measures on the ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"tool": "resample_bench", "batch": args.batch, "seconds": args.seconds,
           "device": torch.cuda.get_device_name(dev)}
    for pair in args.pairs.split(","):
        orig_sr, target_sr = (int(v) for v in pair.split(":"))
        L, M, _, half = audio._resample_geometry(orig_sr, target_sr)
        taps, n_in = 2 * half + 2, int(args.seconds * orig_sr)
        pcm = np.random.RandomState(orig_sr % 1000).randint(-32768, 32768, (args.batch, n_in)).astype(np.int16)
        x16 = torch.from_numpy(pcm).to(dev)
        x32 = x16.to(torch.float32) / 32768.0
        y = audio.resample(x32, orig_sr, target_sr)
        n_out = y.shape[1]
        assert torch.equal(audio.resample(x16, orig_sr, target_sr), y)
        row = {"L": L, "M": M, "taps": taps, "table_KB": round(taps * L * 4 / 1024, 1), "n_in": n_in, "n_out": n_out}
        for name, x, width in (("f32", x32, 4), ("s16", x16, 2)):
            ms = ms_per_call(lambda: audio.resample(x, orig_sr, target_sr))
            hbm = args.batch * (n_in * width + n_out * 4) + taps * L * 4
            row[name] = {"ms": round(ms, 4), "x_realtime": round(args.batch * args.seconds / ms * 1e3),
                         "hbm_MB": round(hbm / 1e6, 2), "hbm_ms_at_peak": round(hbm / HBM_PEAK_BYTES_PER_S * 1e3, 4),
                         "achieved_GB_per_s": round(hbm / ms / 1e6, 1),
                         "achieved_GFLOP_per_s": round(2.0 * taps * n_out * args.batch / ms / 1e6, 1)}
        Lh, Mh, hf = host_fir(orig_sr, target_sr)
        x0 = pcm[0].astype(np.float64) / 32768.0
        best = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            ref = scipy.signal.resample_poly(x0, Lh, Mh, window=hf) / Lh
            best = min(best, time.perf_counter() - t0)
        row["scipy_resample_poly_ms_per_waveform"] = round(best * 1e3, 3)
        row["scipy_resample_poly_ms_batch"] = round(best * 1e3 * args.batch, 1)
        row["speedup_vs_scipy_f32"] = round(best * 1e3 * args.batch / row["f32"]["ms"], 1)
        row["max_abs_diff_vs_scipy"] = float(np.abs(y[0].cpu().numpy().astype(np.float64) - ref).max())
        out[f"{orig_sr}->{target_sr}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
