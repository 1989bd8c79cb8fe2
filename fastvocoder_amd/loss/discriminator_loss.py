"""The discriminator scores of the reference's training loop (bin/train.py:97-117, 157-169), forward only.

With est_p = D(estimate) and p = D(real), lists of L lists of feature maps (the last map of each list its score):

    adversarial   = sum_i MSE(est_p[i][-1], 1) / L
    feature_map   = sum_i sum_{j < len(est_p[i]) - 1} L1(est_p[i][j], p[i][j]) / (L * (len(est_p[0]) - 1))
    real          = sum_i MSE(p[i][-1], 1) / L
    fake          = sum_i MSE(est_p[i][-1], 0) / L
    discriminator = real + fake

MSE and L1 are means over the whole batch tensor.  The feature-map divisor uses the length of the FIRST list for
every list, as the reference does (6 x 6 = 36 for Discriminator(), whose MFD lists add only 4 terms each).  All the
sums come from one fv_disc_score_sums call (two launches) in float64.
"""
import torch

from .. import _native

TERMS = ("adversarial", "feature_map", "real", "fake", "discriminator")


def compose_terms(sums, counts, lengths, per_utterance=False):
    """The five terms from the sums of fv_disc_score_sums.  sums: float64 [M, B, 4] (sum|e-r|, sum(e-1)^2, sum e^2,
    sum(r-1)^2) over the maps of the flattened lists; counts: elements per row of each map [M]; lengths: the number
    of maps in each list.  -> dict of float64 tensors, 0-d, or [B] with ``per_utterance`` (each row as a batch of one)."""
    sums = torch.as_tensor(sums, dtype=torch.float64)
    counts = torch.as_tensor(counts, dtype=torch.float64, device=sums.device)
    if per_utterance:
        means = sums / counts[:, None, None]                          # [M, B, 4]
    else:
        means = sums.sum(dim=1) / (counts[:, None] * sums.shape[1])   # [M, 4]
    L = len(lengths)
    last, fm_idx, m = [], [], 0
    for n in lengths:
        fm_idx += range(m, m + n - 1)
        last.append(m + n - 1)
        m += n
    fm_den = float(L * (lengths[0] - 1))
    fm = means[fm_idx, ..., 0].sum(dim=0) / fm_den
    adv = means[last, ..., 1].sum(dim=0) / L
    fake = means[last, ..., 2].sum(dim=0) / L
    real = means[last, ..., 3].sum(dim=0) / L
    return {"adversarial": adv, "feature_map": fm, "real": real, "fake": fake, "discriminator": real + fake}


def discriminator_terms(est_p, p, per_utterance=False):
    """The reference's adversarial, feature-map, real, fake and discriminator scores (module docstring) of the
    discriminator outputs est_p = D(estimate) and p = D(real), nested lists of device maps of matching shapes.
    -> dict of fp32 device tensors: 0-d (batch-level, as train.py logs them), or [B] with ``per_utterance``."""
    if len(est_p) != len(p) or not est_p or any(len(a) != len(b) for a, b in zip(est_p, p)):
        raise ValueError("est_p and p must be lists of the same number of lists of the same lengths")
    if any(len(a) < 1 for a in est_p) or len(est_p[0]) < 2:
        raise ValueError("every list needs its score map, and the first at least one feature map before it")
    es = [m for lst in est_p for m in lst]
    rs = [m for lst in p for m in lst]
    for e, r in zip(es, rs):
        for t, name in ((e, "est_p"), (r, "p")):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise _native.NativeError(f"{name} maps must be ROCm device tensors (there is no CPU path in "
                                          "fastvocoder_amd)")
            if t.requires_grad and torch.is_grad_enabled():
                raise RuntimeError(f"{name} requires grad: discriminator_terms is inference-only; call it under "
                                   "torch.no_grad()")
        if e.shape != r.shape:
            raise ValueError(f"map shapes differ: {tuple(e.shape)} and {tuple(r.shape)}")
    es = [e.to(torch.float32).contiguous() for e in es]
    rs = [r.to(torch.float32).contiguous() for r in rs]
    sums = _native.disc_score_sums(es, rs)
    terms = compose_terms(sums, [e[0].numel() for e in es], [len(lst) for lst in est_p], per_utterance)
    return {k: v.float() for k, v in terms.items()}
