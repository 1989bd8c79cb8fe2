"""The reference's composed generator loss (model/loss/loss.py), forward only: the multi-resolution STFT loss of
a full-band estimate, or of the sub-bands and their PQMF synthesis for the multiband generators, plus the
Basis-MelGAN weight L1 term."""
import torch

from .stft_loss import MultiResolutionSTFTLoss, _signal


class Loss(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.stft_loss = MultiResolutionSTFTLoss()
        self.l1_loss = torch.nn.L1Loss()

    def forward(self, est_source, wav, est_weight=None, weight=None, pqmf=None):
        """-> (stft_loss, weight_loss).  Single band: est_source, wav (B, T); stft_loss = sc + mag.
        ``pqmf`` given: est_source (B, subbands, T / subbands) sub-band estimate, wav (B, T) full band;
        stft_loss = ((sc + mag) of the sub-band rows against pqmf.analysis(wav) + (sc + mag) of
        pqmf.synthesis(est_source) against wav) / 2, and weight_loss is None.  Otherwise weight_loss is
        L1(est_weight, weight) when both are given (Basis-MelGAN), else None."""
        weight_loss = None
        if pqmf is not None:
            if est_source.dim() != 3:
                raise ValueError(f"est_source must be (B, subbands, T/subbands) with pqmf, got {tuple(est_source.shape)}")
            wav_full_band = _signal(wav, "wav")
            est_source_sub_band = est_source.contiguous().float()
            wav_sub_band = pqmf.analysis(wav_full_band.unsqueeze(1))
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
            weight_loss = self.l1_loss(est_weight, weight)

        return stft_loss, weight_loss
