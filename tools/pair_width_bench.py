"""Time the fused 128-channel pair launches of HiFi-GAN light with the 11-tap member on 64- and on 80-column tiles
(csrc/convq2_kernels.hpp kPair128Col80; Tuning::convq_nm11), and what ONE tile of each width costs: the 11-tap member alone on
a grid that gives every block one tile, then two (the difference is a tile without the launch's fixed part) -- the ratio
the launcher's model assumes is 49 : 60 (csrc/convh_launch.hip pair_width_plan, Tuning::convq_cost80).
usage: python tools/pair_width_bench.py [T [B]]"""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from fastvocoder_amd import _native  # noqa: E402
from tools.stage_bench import timed  # noqa: E402

SPLIT = _native.PAIR_SPLIT_F16
DILS = (1, 3, 5)
KS = (11, 7, 3)
C = 128


def main():
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 8000
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    P1 = {k: _native.pack_pair(torch.from_numpy((rng.randn(C, C, k) / np.sqrt(C * k)).astype(np.float32)).to(dev), SPLIT) for k in KS}
    P2 = {k: _native.pack_pair(torch.from_numpy((rng.randn(C, C, k) / np.sqrt(C * k)).astype(np.float32)).to(dev), SPLIT) for k in KS}
    b1 = {k: torch.from_numpy(rng.randn(C).astype(np.float32) * 0.1).to(dev) for k in KS}
    b2 = {k: torch.from_numpy(rng.randn(C).astype(np.float32) * 0.1).to(dev) for k in KS}
    xs = [torch.from_numpy(rng.randn(B, C, T).astype(np.float32)).to(dev) for _ in KS]
    outs = [torch.empty_like(x) for x in xs]
    mids = [torch.empty_like(x) for x in xs]

    def launch(ks, dil):
        n = len(ks)
        return lambda: _native.resblock1_fused(xs[:n], [P1[k] for k in ks], [P2[k] for k in ks], [b1[k] for k in ks],
                                               [b2[k] for k in ks], list(ks), dil, 0.1, prec=SPLIT, outs=outs[:n], mids=mids[:n])

    _native.tuning_set("convq_wide", 1 << 20)        # narrow tiles, as the batch-1 launches run
    print(f"C={C} B={B} T={T}  (us per launch: min / median of 5 interleaved rounds)")
    for dil in DILS:
        # name -> (convq_nm11, convh_blocks, members)
        variants = {}
        for nm in (64, 80):
            tiles = B * -(-T // (nm - 10))
            variants[f"11 + 7 + 3 taps, {nm} columns"] = (nm, 0, KS)
            variants[f"11 + 7 taps, {nm} columns"] = (nm, 0, KS[:2])
            variants[f"11 taps alone, {nm} columns, 1 tile a block"] = (nm, 0, KS[:1])
            variants[f"11 taps alone, {nm} columns, 2 tiles a block"] = (nm, -(-tiles // 2), KS[:1])
        variants["7 taps alone, 1 tile a block"] = (64, 0, (7,))
        variants["3 taps alone, 1 tile a block"] = (64, 0, (3,))
        best = {k: [] for k in variants}
        for rnd in range(5):
            for name, (nm, blocks, ks) in variants.items():
                _native.tuning_set("convq_nm11", nm)
                _native.tuning_set("convh_blocks", blocks)
                best[name].append(timed(launch(ks, dil), reps=40, warm=5))
        _native.tuning_set("convq_nm11", -1)
        _native.tuning_set("convh_blocks", 0)
        print(f" dilation {dil}")
        for name, ts in best.items():
            print(f"  {name:48s} {min(ts):8.1f} {sorted(ts)[2]:8.1f}")
        one = {nm: min(best[f"11 taps alone, {nm} columns, 1 tile a block"]) for nm in (64, 80)}
        two = {nm: min(best[f"11 taps alone, {nm} columns, 2 tiles a block"]) for nm in (64, 80)}
        t64, t80 = two[64] - one[64], two[80] - one[80]
        print(f"  a second (warm) 11-tap tile: {t64:.1f} us at 64 columns, {t80:.1f} at 80 -- ratio {t80 / t64:.3f} (model: 55 / 44 = 1.250 "
              f"of the K steps, 60 / 49 = 1.224 with the per-tile constant); whole first tile {one[80] / one[64]:.3f}")
        pl = _native.debug_pair_widths(C, B, T, dil, KS, 256)
        print(f"  the launcher's choice for 11 + 7 + 3 taps: {pl['widths']} items {pl['items']} costs {pl['costs']} makespan {pl['makespan']}")


if __name__ == "__main__":
    main()
