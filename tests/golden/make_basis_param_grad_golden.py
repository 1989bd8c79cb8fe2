"""Writes tests/golden/basis_param_grad.npz: the reference's own autograd gradient of

    L = <c, est> + Loss().l1_loss(est_weight, target),      (est, est_weight) = BasisMelGANGenerator(mel),

with respect to every parameter of model/generator/basis_melgan.py's BasisMelGANGenerator -- its two-pass forward, the
zero pass on the graph --, torch on the CPU with the module and the mel in float64, on the seeded weights of
fastvocoder_amd.synthetic (seeded_state_dict("basis-melgan", GOLDEN_CFG, GOLDEN_WEIGHT_SEED), regenerated on any box,
not stored).  The weight term is model/loss/loss.py's own ``l1_loss`` member, as Loss.forward applies it (loss.py:39-40);
the estimate of this case is 108 samples long, too short for the reflect pad of Loss's STFT resolutions, so the
waveform's side of the loss is the linear functional the other parameter-gradient fixtures use.  Run once against a
checkout of the reference, with the SciPy >= 1.13 shim make_golden.py uses:

    python tests/golden/make_basis_param_grad_golden.py /path/to/FastVocoder

The inputs come from one RandomState seed (tests/basis_grad_reference.golden_inputs).  The maker searches the seeds
0..199 for the first one at which no pre-activation of the float64 forward lies within 1e-5 of its map's peak of a
kink -- every F.leaky_relu input, the input of the final ReLU of BOTH passes (read off the ReLU module with a forward
hook) and est_weight - target of the L1 term --, asserts that for the seed it uses, and records the seed and the
smallest margin; were there none, it keeps the seed with the largest margin and says so when it runs.

Contents:
  mel            [2, 80, 6] float32
  c              [2, 108] float32      the cotangent of est
  target         [2, 36, 8] float32    the target weights
  est            [2, 108] float64,  weight [2, 36, 8] float64
  grad/<state key>     float64         dL / d parameter, one entry per state-dict key (the basis' too: the reference
                                       gives it one and never applies it; the tests read the trunk's), rounded to
                                       32 bits of mantissa so that the file stays under 100 KB
  input_seed, weight_seed, margin
The fixture is data only; no test reads the reference tree."""
import os
import sys
import warnings

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True

import numpy as np
import scipy.signal
import scipy.signal.windows
import torch

scipy.signal.kaiser = scipy.signal.windows.kaiser

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from fastvocoder_amd.synthetic import seeded_state_dict  # noqa: E402
from tests import basis_grad_reference as bref           # noqa: E402

SEEDS = 200


def _short(a):
    """float64 rounded to 32 bits of mantissa (2.3e-10 relative, four orders below any tolerance the fixture is used
    with): the low 20 bits are zero and compress away, which keeps the file under 100 KB."""
    bits = np.ascontiguousarray(a, np.float64).view(np.uint64)
    return ((bits + np.uint64(1 << 19)) & ~np.uint64((1 << 20) - 1)).view(np.float64).copy()


def main(reference):
    sys.path.insert(0, reference)
    from model.generator.basis_melgan import BasisMelGANGenerator
    from model.loss.loss import Loss

    cfg = bref.GOLDEN_CFG
    sd = seeded_state_dict("basis-melgan", cfg, bref.GOLDEN_WEIGHT_SEED)
    gen = BasisMelGANGenerator(basis_signal_weight=torch.from_numpy(sd[bref.BASIS_KEY]), **cfg)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    gen = gen.double().train()
    l1 = Loss().l1_loss
    margins = []
    relu = [m for m in gen.melgan if isinstance(m, torch.nn.ReLU)]
    assert len(relu) == 1
    relu[0].register_forward_hook(lambda m, inp, out: bref._margin(inp[0], margins))

    def run(seed):
        mel, c, target = bref.golden_inputs(seed)
        gen.zero_grad()
        del margins[:]
        with bref.recorded_margins(margins):
            est, weight = gen(torch.from_numpy(mel).double())
        bref._margin(weight.detach() - torch.from_numpy(target).double(), margins)
        return mel, c, target, est, weight, min(margins), len(margins)

    best, chosen = (-1.0, None), None
    for seed in range(SEEDS):
        with torch.no_grad():
            margin = run(seed)[5]
        if margin > best[0]:
            best = (margin, seed)
        if margin > bref.KINK:
            chosen = seed
            break
    if chosen is None:
        chosen = best[1]
        print(f"none of the first {SEEDS} seeds is clear of the kinks: keeping seed {chosen}, margin {best[0]:.3e}")
    mel, c, target, est, weight, margin, count = run(chosen)
    stacks = len(cfg["upsample_scales"]) * cfg["stacks"]
    # every LeakyReLU of both passes, the final ReLU of both, the L1 difference
    assert count == 2 * (len(cfg["upsample_scales"]) + 2 * stacks) + 2 + 1, count
    assert margin > bref.KINK or best[0] <= bref.KINK, (chosen, margin)
    ((est * torch.from_numpy(c).double()).sum() + l1(weight, torch.from_numpy(target).double())).backward()
    named = dict(gen.named_parameters())
    assert sorted(named) == sorted(sd), "every state-dict entry is a parameter"
    out = {"mel": mel, "c": c, "target": target, "est": est.detach().numpy().copy(),
           "weight": weight.detach().numpy().copy(), "input_seed": np.int64(chosen),
           "weight_seed": np.int64(bref.GOLDEN_WEIGHT_SEED), "margin": np.float64(margin)}
    for k in sd:
        out[f"grad/{k}"] = _short(named[k].grad.numpy())
    path = os.path.join(HERE, "basis_param_grad.npz")
    np.savez_compressed(path, **out)
    norm = np.sqrt(sum(np.sum(v ** 2) for k, v in out.items() if k.startswith("grad/")))
    print(f"wrote {path}: {os.path.getsize(path)} bytes; seed {chosen}, margin {margin:.3e}, |grad| {norm:.6e}")


if __name__ == "__main__":
    main(sys.argv[1])
