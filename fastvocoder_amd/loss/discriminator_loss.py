"""The discriminator scores of the reference's training loop (bin/train.py:97-117, 157-169); with
``differentiable=True`` they carry the gradient with respect to the estimate's maps, and discriminator_step_terms
carries the gradient of the discriminator's own update with respect to its parameters (the MSD as it is, the STFT and
period discriminators and Discriminator() with its keywords stft_grad / period_grad).

With est_p = D(estimate) and p = D(real), lists of L lists of feature maps (the last map of each list its score):

    adversarial   = sum_i MSE(est_p[i][-1], 1) / L
    feature_map   = sum_i sum_{j < len(est_p[i]) - 1} L1(est_p[i][j], p[i][j]) / (L * (len(est_p[0]) - 1))
    real          = sum_i MSE(p[i][-1], 1) / L
    fake          = sum_i MSE(est_p[i][-1], 0) / L
    discriminator = real + fake

MSE and L1 are means over the whole batch tensor.  The feature-map divisor uses the length of the FIRST list for
every list, as the reference does (6 x 6 = 36 for Discriminator(), whose MFD lists add only 4 terms each).  All the
sums come from one fv_disc_score_sums call (two launches) in float64.

The gradient (one fv_disc_score_grad launch) reaches est_p only: p is detached in the reference
(``p[ii][jj].detach()``), so ``real`` is a constant of the estimate, and ``fake`` and ``discriminator`` differentiate
through sum e^2.
"""
import torch

from .. import _native

TERMS = ("adversarial", "feature_map", "real", "fake", "discriminator")


def _map_index(lengths):
    """(indices of the feature maps, indices of the score maps) in the flattened lists."""
    last, fm_idx, m = [], [], 0
    for n in lengths:
        fm_idx += range(m, m + n - 1)
        last.append(m + n - 1)
        m += n
    return fm_idx, last


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
    fm_idx, last = _map_index(lengths)
    fm_den = float(L * (lengths[0] - 1))
    fm = means[fm_idx, ..., 0].sum(dim=0) / fm_den
    adv = means[last, ..., 1].sum(dim=0) / L
    fake = means[last, ..., 2].sum(dim=0) / L
    real = means[last, ..., 3].sum(dim=0) / L
    return {"adversarial": adv, "feature_map": fm, "real": real, "fake": fake, "discriminator": real + fake}


def grad_coefficients(grad_terms, counts, lengths, batch):
    """Per map the (c_l1, c_adv, c_fake) of fv_disc_score_grad from the gradients of the five TERMS: a feature map m
    carries c_l1 = g_fm / (L (len(est_p[0]) - 1) n_m B), a score map c_adv = g_adv / (L n_m B) and
    c_fake = (g_fake + g_discriminator) / (L n_m B); ``real`` does not depend on the estimate."""
    g = dict(zip(TERMS, (float(v) for v in grad_terms)))
    L = len(lengths)
    fm_idx, last = _map_index(lengths)
    fm_den = float(L * (lengths[0] - 1))
    coef = [[0.0, 0.0, 0.0] for _ in counts]
    for m in fm_idx:
        coef[m][0] = g["feature_map"] / (fm_den * counts[m] * batch)
    for m in last:
        coef[m][1] = g["adversarial"] / (L * counts[m] * batch)
        coef[m][2] = (g["fake"] + g["discriminator"]) / (L * counts[m] * batch)
    return coef


class _Terms(torch.autograd.Function):
    """The five TERMS as one float64 [5] tensor: the forward of discriminator_terms, the backward one
    fv_disc_score_grad launch for every estimate map that requires grad."""

    @staticmethod
    def forward(ctx, lengths, *maps):
        M = len(maps) // 2
        es, rs = list(maps[:M]), list(maps[M:])
        sums = _native.disc_score_sums(es, rs)
        terms = compose_terms(sums, [e[0].numel() for e in es], lengths)
        ctx.lengths = lengths
        ctx.save_for_backward(*maps)
        return torch.stack([terms[k] for k in TERMS])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_terms):
        maps = ctx.saved_tensors
        M = len(maps) // 2
        es, rs = list(maps[:M]), list(maps[M:])
        coef = grad_coefficients(grad_terms.detach().cpu().tolist(), [e[0].numel() for e in es], ctx.lengths,
                                 es[0].shape[0])
        skip = [not need for need in ctx.needs_input_grad[1:M + 1]]
        return (None,) + tuple(_native.disc_score_grad(es, rs, coef, skip)) + (None,) * M


def _adversarial(es):
    """sum_i MSE(es[i], 1) / L as a float64 0-d tensor (fv_disc_score_sums on the score maps against themselves)."""
    sums = torch.as_tensor(_native.disc_score_sums(es, es), dtype=torch.float64)
    counts = torch.as_tensor([e[0].numel() for e in es], dtype=torch.float64, device=sums.device)
    return (sums[..., 1].sum(dim=1) / (counts * sums.shape[1])).sum() / len(es)


class _Adversarial(torch.autograd.Function):
    """The adversarial term of the score maps alone (generator_adversarial_terms with real=None): no feature map is
    reduced in the forward or given a gradient in the backward."""

    @staticmethod
    def forward(ctx, *es):
        ctx.save_for_backward(*es)
        return _adversarial(list(es))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        es = list(ctx.saved_tensors)
        g, L, B = float(g), len(es), es[0].shape[0]
        coef = [(0.0, g / (L * e[0].numel() * B), 0.0) for e in es]
        return tuple(_native.disc_score_grad(es, es, coef, [not n for n in ctx.needs_input_grad]))


def _as_lists(discriminator, out):
    """A module's output as a list of lists of maps, the score last in each: DiscriminatorP's (score, maps) and the
    bare list of a single stack become one list."""
    from ..discriminator import DiscriminatorP
    if isinstance(discriminator, DiscriminatorP):
        return [out[1] + [out[0].unsqueeze(1)]]
    return [out] if torch.is_tensor(out[0]) else out


def generator_adversarial_terms(discriminator, estimate, real=None, *, period_grad=False):
    """The generator's adversarial and feature-map terms (bin/train.py:97-120) as one call, attached to the graph of
    ``estimate``: {"adversarial", "feature_map"} as 0-d fp32 device tensors with the reference's divisors
    (len(est_p[0]) - 1 for every list).  ``estimate`` and ``real`` are (B, 1, T) fp32 device tensors ((B, T) for an
    STFTDiscriminator, as its forward takes them); ``estimate`` may require grad.  The discriminator's graph-mode
    forward runs on ``estimate`` (the launches and bits of its plain forward, the input gradient from
    csrc/disc_grad.hip, csrc/stft_mag_grad.hip and csrc/mpd_grad.hip), its plain forward on ``real`` under
    torch.no_grad().  With
    ``real=None`` (the reference's use_feature_map_loss = False) only "adversarial" is returned and D(real) is not
    run.  The module's ``differentiable`` attribute is not consulted; its parameters are constants (``.grad`` stays
    None).  Under torch.no_grad(), or when ``estimate`` does not require grad, the same values come back with no
    graph.  Accepted: MelGANDiscriminator, MelGANMultiScaleDiscriminator, STFTDiscriminator,
    MultiResolutionSTFTDiscriminator and Discriminator().  The modules that hold the period convs of the MPD
    (DiscriminatorP, MultiPeriodDiscriminator, Discriminator(use_mpd=True)) are refused unless ``period_grad=True``
    is passed: their gradient is opt-in, and for every other module the keyword changes nothing."""
    from ..discriminator import Discriminator, DiscriminatorP, MultiPeriodDiscriminator
    if isinstance(discriminator, (DiscriminatorP, MultiPeriodDiscriminator)) or \
            (isinstance(discriminator, Discriminator) and discriminator.use_mpd):
        if not period_grad:
            raise NotImplementedError(f"generator_adversarial_terms: {type(discriminator).__name__} holds the period "
                                      "convs of the MPD, whose input gradient is opt-in: pass period_grad=True")
    graph = getattr(discriminator, "_graph_forward", None)
    if graph is None:
        raise TypeError(f"generator_adversarial_terms: {type(discriminator).__name__} is not a fastvocoder_amd "
                        "discriminator with an input gradient")
    est_p = _as_lists(discriminator, graph(estimate))
    if real is None:      # the score maps alone: adversarial = sum_i MSE(score_i, 1) / L reads nothing else
        es = [lst[-1].to(torch.float32).contiguous() for lst in est_p]
        if torch.is_grad_enabled() and any(e.requires_grad for e in es):
            return {"adversarial": _Adversarial.apply(*es).float()}
        return {"adversarial": _adversarial(es).float()}
    with torch.no_grad():
        p = _as_lists(discriminator, discriminator(real))
    terms = discriminator_terms(est_p, p, differentiable=True)
    return {"adversarial": terms["adversarial"], "feature_map": terms["feature_map"]}


def _step_terms(es, rs):
    """(real, fake, discriminator) as one float64 [3] tensor from the score maps alone (es the estimate's, rs the real
    signal's): the sums, means and divisors of compose_terms, hence its bits."""
    sums = torch.as_tensor(_native.disc_score_sums(es, rs), dtype=torch.float64)
    counts = torch.as_tensor([e[0].numel() for e in es], dtype=torch.float64, device=sums.device)
    means = sums.sum(dim=1) / (counts[:, None] * sums.shape[1])
    L, last = len(es), list(range(len(es)))
    fake = means[last, ..., 2].sum(dim=0) / L
    real = means[last, ..., 3].sum(dim=0) / L
    return torch.stack([real, fake, real + fake])


class _StepTerms(torch.autograd.Function):
    """_step_terms on the graph of the score maps of both passes: the backward is one fv_disc_score_grad launch per
    pass, the (e - 1)^2 coefficient on the real signal's score maps and the e^2 coefficient on the estimate's."""

    @staticmethod
    def forward(ctx, *maps):
        L = len(maps) // 2
        ctx.save_for_backward(*maps)
        return _step_terms(list(maps[:L]), list(maps[L:]))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        maps = ctx.saved_tensors
        L = len(maps) // 2
        es, rs = list(maps[:L]), list(maps[L:])
        g_real, g_fake, g_disc = (float(v) for v in g.detach().cpu().tolist())
        B = es[0].shape[0]
        need = ctx.needs_input_grad
        ge, gr = [None] * L, [None] * L
        if any(need[:L]):
            coef = [(0.0, 0.0, (g_fake + g_disc) / (L * e[0].numel() * B)) for e in es]
            ge = _native.disc_score_grad(es, es, coef, [not n for n in need[:L]])
        if any(need[L:]):
            coef = [(0.0, (g_real + g_disc) / (L * r[0].numel() * B), 0.0) for r in rs]
            gr = _native.disc_score_grad(rs, rs, coef, [not n for n in need[L:]])
        return tuple(ge) + tuple(gr)


def discriminator_step_terms(discriminator, estimate, real, *, stft_grad=False, period_grad=False):
    """The terms of the discriminator's own update (bin/train.py:157-169) as one call, attached to the graph of the
    discriminator's PARAMETERS: {"real", "fake", "discriminator"} as 0-d fp32 device tensors with the reference's
    divisors, real = sum_i MSE(D(real)[i][-1], 1) / L and fake = sum_i MSE(D(estimate.detach())[i][-1], 0) / L
    (L = 3 for the MSD and the MFD, 5 for the MPD, 6 for Discriminator(), 11 with use_mpd).  ``estimate`` and
    ``real`` are (B, 1, T) fp32 device tensors ((B, T) for a single STFTDiscriminator, as its forward takes them);
    ``estimate`` is detached, as train.py:159 does, and neither may require grad.  The module's parameter-gradient
    forward runs on both signals whatever its ``parameter_grad`` attribute says (the launches and bits of its plain
    forward); ``terms["discriminator"].backward()`` accumulates into the ``.grad`` of every conv parameter that
    requires grad (csrc/disc_wgrad.hip, csrc/mpd_wgrad.hip).  The feature maps get no gradient.  Under
    torch.no_grad(), or with every parameter frozen, the same values come back with no graph; a frozen parameter gets
    no gradient and costs no launch.  Accepted as they are: MelGANDiscriminator and MelGANMultiScaleDiscriminator.
    The other families are opt-in: ``stft_grad=True`` admits STFTDiscriminator and MultiResolutionSTFTDiscriminator,
    ``period_grad=True`` admits DiscriminatorP and MultiPeriodDiscriminator, Discriminator() needs ``stft_grad=True``
    and Discriminator(use_mpd=True) both; without the keyword it needs a module is refused.  For the MSD modules the
    keywords change nothing."""
    from ..discriminator import (Discriminator, DiscriminatorP, MelGANDiscriminator, MelGANMultiScaleDiscriminator,
                                 MultiPeriodDiscriminator, MultiResolutionSTFTDiscriminator, STFTDiscriminator)
    missing = []
    if isinstance(discriminator, (STFTDiscriminator, MultiResolutionSTFTDiscriminator, Discriminator)) \
            and not stft_grad:
        missing.append("stft_grad=True")
    if (isinstance(discriminator, (DiscriminatorP, MultiPeriodDiscriminator))
            or (isinstance(discriminator, Discriminator) and discriminator.use_mpd)) and not period_grad:
        missing.append("period_grad=True")
    known = (MelGANDiscriminator, MelGANMultiScaleDiscriminator, STFTDiscriminator, MultiResolutionSTFTDiscriminator,
             DiscriminatorP, MultiPeriodDiscriminator, Discriminator)
    if missing or not isinstance(discriminator, known):
        hint = f"; the gradient of this module is opt-in: pass {' and '.join(missing)}" if missing else ""
        raise NotImplementedError(f"discriminator_step_terms: {type(discriminator).__name__} has no parameter gradient "
                                  f"yet; supported: MelGANDiscriminator, MelGANMultiScaleDiscriminator{hint}")
    if not torch.is_tensor(estimate):
        raise TypeError(f"estimate must be a tensor, got {type(estimate).__name__}")
    p = _as_lists(discriminator, discriminator._param_forward(real))
    est_p = _as_lists(discriminator, discriminator._param_forward(estimate.detach()))
    es = [lst[-1].to(torch.float32).contiguous() for lst in est_p]
    rs = [lst[-1].to(torch.float32).contiguous() for lst in p]
    if torch.is_grad_enabled() and any(m.requires_grad for m in es + rs):
        terms = _StepTerms.apply(*es, *rs)
    else:
        terms = _step_terms(es, rs)
    return {k: terms[i].float() for i, k in enumerate(("real", "fake", "discriminator"))}


def discriminator_terms(est_p, p, per_utterance=False, differentiable=False):
    """The reference's adversarial, feature-map, real, fake and discriminator scores (module docstring) of the
    discriminator outputs est_p = D(estimate) and p = D(real), nested lists of device maps of matching shapes.
    -> dict of fp32 device tensors: 0-d (batch-level, as train.py logs them), or [B] with ``per_utterance``.
    ``differentiable``: the (batch-level) terms are attached to the graph of the est_p maps that require grad; p
    never gets a gradient."""
    if len(est_p) != len(p) or not est_p or any(len(a) != len(b) for a, b in zip(est_p, p)):
        raise ValueError("est_p and p must be lists of the same number of lists of the same lengths")
    if any(len(a) < 1 for a in est_p) or len(est_p[0]) < 2:
        raise ValueError("every list needs its score map, and the first at least one feature map before it")
    if differentiable and per_utterance:
        raise NotImplementedError("discriminator_terms(differentiable=True) gives the batch-level terms only: "
                                  "per_utterance terms are not differentiable")
    es = [m for lst in est_p for m in lst]
    rs = [m for lst in p for m in lst]
    for e, r in zip(es, rs):
        for t, name in ((e, "est_p"), (r, "p")):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise _native.NativeError(f"{name} maps must be ROCm device tensors (there is no CPU path in "
                                          "fastvocoder_amd)")
            if t.requires_grad and torch.is_grad_enabled() and not differentiable:
                raise RuntimeError(f"{name} requires grad: discriminator_terms is inference-only; call it under "
                                   "torch.no_grad()")
        if e.shape != r.shape:
            raise ValueError(f"map shapes differ: {tuple(e.shape)} and {tuple(r.shape)}")
    es = [e.to(torch.float32).contiguous() for e in es]
    rs = [r.detach().to(torch.float32).contiguous() if differentiable else r.to(torch.float32).contiguous()
          for r in rs]
    lengths = [len(lst) for lst in est_p]
    if differentiable and torch.is_grad_enabled() and any(e.requires_grad for e in es):
        terms = dict(zip(TERMS, _Terms.apply(lengths, *es, *rs)))
    else:
        sums = _native.disc_score_sums(es, rs)
        terms = compose_terms(sums, [e[0].numel() for e in es], lengths, per_utterance)
    return {k: v.float() for k, v in terms.items()}
