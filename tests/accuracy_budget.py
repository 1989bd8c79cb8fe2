"""Whole-generator error budget against a float64 evaluation of the same graph.

A GPU output ``g`` is judged by its distance from the exact answer ``r64`` (oracle/torch_port.py with
``dtype=torch.float64``), compared with the distance of a plain fp32 evaluation ``p32`` (the same port in fp32)
from it -- the "x times fp32" bound tests/test_split_precision.py proves per layer (3x max, 1.6x rms), here for
the whole model:

    max|g - r64| <= A * max|p32 - r64| + F * s
    rms(g - r64) <= R * rms(p32 - r64) + F * s / 4

``s = max(1, max|r64|)`` scales the floor for outputs not bounded by tanh (Basis-MelGAN's ``weight``); ``F`` is
2 ulp at 1.0, so that tiny outputs (one frame: 240 samples) whose fp32 error happens to be near zero do not fail
on chance.  A and R are the per-layer claims plus a margin for compounding through a deep graph; they were set
before any GPU run and are not fitted to one.
"""
import numpy as np

A_MAX = 4.0                   # per-layer max-error claim 3x, plus compounding margin
R_RMS = 2.0                   # per-layer rms claim 1.6x, plus compounding margin
FLOOR = 2.0 * 2.0 ** -23      # 2 ulp at 1.0 = 2.4e-7


def _f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def measure(g, p32, r64, A=A_MAX, R=R_RMS):
    """The budget's numbers for one output: absolute errors of ``g`` and ``p32`` against ``r64``, their ratios,
    and ``excess`` -- the larger of (max error / max bound) and (rms error / rms bound); <= 1 is inside."""
    g, p32, r64 = _f64(g), _f64(p32), _f64(r64)
    assert g.shape == p32.shape == r64.shape, (g.shape, p32.shape, r64.shape)
    s = max(1.0, float(np.abs(r64).max())) if r64.size else 1.0
    dg, dp = g - r64, p32 - r64
    gmax, pmax = float(np.abs(dg).max()), float(np.abs(dp).max())
    grms, prms = float(np.sqrt(np.mean(dg * dg))), float(np.sqrt(np.mean(dp * dp)))
    max_bound, rms_bound = A * pmax + FLOOR * s, R * prms + FLOOR * s / 4
    return dict(max_err=gmax, rms_err=grms, fp32_max=pmax, fp32_rms=prms,
                max_ratio=gmax / pmax if pmax > 0 else float("inf") if gmax > 0 else 0.0,
                rms_ratio=grms / prms if prms > 0 else float("inf") if grms > 0 else 0.0,
                excess=max(gmax / max_bound, grms / rms_bound), scale=s, A=A, R=R)


def fmt(m):
    return (f"max {m['max_ratio']:.2f}x fp32 (A={m['A']:g}), rms {m['rms_ratio']:.2f}x fp32 (R={m['R']:g}), "
            f"|g - f64| max {m['max_err']:.2e} rms {m['rms_err']:.2e}, fp32 max {m['fp32_max']:.2e}, "
            f"budget used {m['excess']:.2f}")


def check(g, p32, r64, what="", A=A_MAX, R=R_RMS):
    """Assert ``g`` meets the budget; print and return the measured numbers (see :func:`measure`)."""
    m = measure(g, p32, r64, A, R)
    print(f"budget {what}: {fmt(m)}")
    assert m["excess"] <= 1.0, f"{what}: outside the float64 error budget: {fmt(m)}"
    return m
