"""The reference's composed generator loss (model/loss/loss.py): the multi-resolution STFT loss of a full-band
estimate, or of the sub-bands and their PQMF synthesis for the multiband generators, plus the Basis-MelGAN weight L1
term.  Forward only by default; ``Loss.differentiable = True`` switches the gradient with respect to the estimate on
(stft_loss.py), through the PQMF synthesis too on the multiband path, and routes the weight term of an ``est_weight``
that is on a graph through csrc/basis_grad.hip (``BasisWeightL1``)."""
import torch

from .. import _native
from .stft_loss import MultiResolutionSTFTLoss, _signal


class PqmfSynthesis(torch.autograd.Function):
    """pqmf.synthesis with its adjoint.  synthesis is y[m] = S sum_k sum_t g_k[S t + taps/2 - m] x[k, t] (zero
    stuffing by S, then the zero-padded FIR g_k), so dL/dx[k, t] = sum_m (S g_k[taps - j]) dL/dy[m] at
    j = m - S t + taps/2: the analysis kernel (a zero-padded FIR decimated by S) with the filter S * flip(g_k).
    ``pqmf_synthesis(x, pqmf)`` is the call: the training loop puts the multiband generator's waveform on the graph
    with it before the discriminator sees it (bin/train.py:96)."""

    @staticmethod
    def forward(ctx, x, pqmf):
        ctx.save_for_backward(pqmf.synthesis_filter)
        ctx.subbands = pqmf.subbands
        return pqmf.synthesis(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        (g,) = ctx.saved_tensors
        S = ctx.subbands
        adjoint = (S * torch.flip(g[0], dims=(-1,))).reshape(S, 1, -1)
        return _native.pqmf_analysis(gy.contiguous().float(), adjoint), None


def pqmf_synthesis(x, pqmf):
    """pqmf.synthesis(x) [B, 1, S T] of the sub-bands x [B, S, T], on the graph of x when x requires grad."""
    x = x.contiguous().float()
    if x.requires_grad and torch.is_grad_enabled():
        return PqmfSynthesis.apply(x, pqmf)
    return pqmf.synthesis(x)


class BasisWeightL1(torch.autograd.Function):
    """L1Loss(est_weight, weight) of Basis-MelGAN's estimated weights [B, F, C] against the targets [B, F, C], with its
    gradient: -> (mean |est_weight - weight|, mean est_weight), two device scalars from fv_basis_weight_l1; the second
    is the reference's ``weight_average_value`` and carries no gradient.  ``est_weight`` is the transposed view of the
    generator's D [B, C, F]; the target keeps the data layout and is transposed on chip.  The backward writes
    coef sign(est_weight - weight) / (B F C) in D's storage (fv_basis_weight_l1_grad) and returns its transposed view,
    which the generator's head adjoint reads without a copy."""

    @staticmethod
    def forward(ctx, est_weight, weight):
        D = est_weight.transpose(1, 2).contiguous()              # no copy for the generator's own view
        out = _native.basis_weight_l1(D, weight)
        ctx.save_for_backward(D, weight)
        loss, average = out[0], out[1]
        ctx.mark_non_differentiable(average)
        return loss, average

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _):
        D, weight = ctx.saved_tensors
        if g is None:
            return None, None
        return _native.basis_weight_l1_grad(D, weight, g.to(torch.float32).reshape(1).contiguous()).transpose(1, 2), None


class Loss(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.stft_loss = MultiResolutionSTFTLoss()
        self.l1_loss = torch.nn.L1Loss()

    @property
    def differentiable(self):
        return self.stft_loss.differentiable

    @differentiable.setter
    def differentiable(self, value):
        self.stft_loss.differentiable = value

    def weight_term(self, est_weight, weight):
        """Basis-MelGAN's weight term -> (L1(est_weight, weight), mean(est_weight) or None).  ``torch.nn.L1Loss`` and
        None as they stand; when ``differentiable`` and est_weight is a device tensor (B, F, C) on a graph,
        ``BasisWeightL1``, whose reduction also gives the mean (the reference's ``weight_average_value``)."""
        if (self.differentiable and est_weight.requires_grad and torch.is_grad_enabled() and est_weight.dim() == 3
                and est_weight.shape == weight.shape and est_weight.is_cuda):
            return BasisWeightL1.apply(est_weight, weight.contiguous().float())
        return self.l1_loss(est_weight, weight), None

    def forward(self, est_source, wav, est_weight=None, weight=None, pqmf=None):
        """-> (stft_loss, weight_loss).  Single band: est_source, wav (B, T); stft_loss = sc + mag.
        ``pqmf`` given: est_source (B, subbands, T / subbands) sub-band estimate, wav (B, T) full band;
        stft_loss = ((sc + mag) of the sub-band rows against pqmf.analysis(wav) + (sc + mag) of
        pqmf.synthesis(est_source) against wav) / 2, and weight_loss is None.  Otherwise weight_loss is
        ``weight_term(est_weight, weight)[0]`` when both are given (Basis-MelGAN), else None."""
        weight_loss = None
        if pqmf is not None:
            if est_source.dim() != 3:
                raise ValueError(f"est_source must be (B, subbands, T/subbands) with pqmf, got {tuple(est_source.shape)}")
            wav_full_band = _signal(wav, "wav")
            est_source_sub_band = est_source.contiguous().float()
            wav_sub_band = pqmf.analysis(wav_full_band.unsqueeze(1))
            if self.differentiable and est_source_sub_band.requires_grad and torch.is_grad_enabled():
                est_source_full_band = PqmfSynthesis.apply(est_source_sub_band, pqmf)[:, 0, :]
            else:
                est_source_full_band = pqmf.synthesis(est_source_sub_band)[:, 0, :]
            est_source_sub_band = est_source_sub_band.view(-1, est_source_sub_band.size(2))
            wav_sub_band = wav_sub_band.reshape(-1, wav_sub_band.size(2))
            if est_source_sub_band.shape != wav_sub_band.shape:
                raise ValueError(f"sub-band estimate {tuple(est_source_sub_band.shape)} and pqmf.analysis(wav) "
                                 f"{tuple(wav_sub_band.shape)} differ")
            sc_sub, mag_sub = self.stft_loss(est_source_sub_band, wav_sub_band)
            sc_full, mag_full = self.stft_loss(est_source_full_band, wav_full_band)
            return ((sc_sub + mag_sub) + (sc_full + mag_full)) / 2., weight_loss

        if est_source.dim() != 2 or wav.dim() != 2 or est_source.size(1) != wav.size(1):
            raise ValueError(f"est_source and wav must both be (B, T) of one length, got {tuple(est_source.shape)} "
                             f"and {tuple(wav.shape)}")
        sc_loss, mag_loss = self.stft_loss(est_source, wav)
        stft_loss = sc_loss + mag_loss

        if est_weight is not None and weight is not None:
            weight_loss = self.weight_term(est_weight, weight)[0]

        return stft_loss, weight_loss
