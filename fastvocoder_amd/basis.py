"""Learning Basis-MelGAN's basis and target weights: ``BasisAutoencoder`` (csrc/basis_learn.hip).

The reference takes ``Basis-MelGAN-dataset/`` (``basis_signal_weight.npy`` [L, C] and one ``weight/<name>.npy`` [C, F]
per utterance) from a separate project, ConvTasNet4BasisMelGAN.  What that project does is public: Conv-TasNet's encoder
/ decoder pair with no separator in between.  Its code, loss and hyper-parameters are not restated here; this module's
contract is the file formats ``MODE=train`` reads, framing that matches the generator's own decoder, and gradients that
meet float64.

With hop = L / 2 and F = ceil(n / hop):

    encode   W[b, c, f] = relu(sum_{j < L} E[c, j] wav[b, f hop + j])      samples at or beyond n read as 0
    decode   est[b, t]  = sum_{f hop + j == t} sum_c basis[j, c] W[b, c, f]   for t < F hop

The encoder is a ``Conv1d(1, C, L, stride=hop, bias=False)`` on the right-padded waveform followed by ReLU
(fv_basis_encode); the decoder is ``BasisSignalLayer`` (fv_pack_basis + fv_basis_ola) cut to F hop samples, the cut of
the generator's forward.  No bias, no weight norm.  There is no CPU path.
"""
import os

import numpy as np
import torch

from . import _native
from .generator.engine import NativeModule, cached
from .generator.modules import BasisSignalLayer


class _Autoencode(torch.autograd.Function):
    """(enc [C, L], basis [L, C]) -> (est [B, F hop], W [B, C, F]); the waveform is a constant.  The backward is one
    fv_basis_learn_grad call from the cotangent of est; W is returned detached (the target weights are data)."""

    @staticmethod
    def forward(ctx, model, wav, enc, basis):
        W = _native.basis_encode(wav, enc)
        est = model._decode(W)
        ctx.save_for_backward(wav, W, basis)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(W)
        return est, W

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_est, _g_w):
        wav, W, basis = ctx.saved_tensors
        want_enc, want_basis = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if g_est is None or not (want_enc or want_basis):
            return None, None, None, None
        g_est = g_est.to(torch.float32).contiguous()
        d_enc, d_basis = _native.basis_learn_grad(wav, g_est, W, basis.contiguous(), want_enc, want_basis)
        return None, None, d_enc, d_basis


class BasisAutoencoder(NativeModule):
    """``encoder.weight`` [C, 1, L] (a ``Conv1d(1, C, L, stride=L // 2, bias=False)``) and
    ``basis_signal.layer.weight`` [L, C], the generator's own key: a learnt checkpoint's basis drops into
    ``BasisMelGANGenerator``."""

    def __init__(self, L=30, channels=256):
        super().__init__()
        if L < 2 or L % 2:
            raise ValueError(f"BasisAutoencoder: L must be even and at least 2, got {L}")
        if channels < 1:
            raise ValueError(f"BasisAutoencoder: channels must be at least 1, got {channels}")
        self.L, self.channels = int(L), int(channels)
        self.encoder = torch.nn.Conv1d(1, self.channels, self.L, stride=self.L // 2, bias=False)
        self.basis_signal = BasisSignalLayer(torch.nn.Linear(self.channels, self.L, bias=False).weight.detach().clone(),
                                             self.L)

    @property
    def hop(self):
        return self.L // 2

    def _wav(self, wav):
        if torch.is_tensor(wav) and wav.requires_grad:
            raise RuntimeError("the waveform requires grad: the autoencoder's gradient treats its input as a constant "
                               "(there is no gradient with respect to the waveform); pass a detached tensor")
        x = self._prepare(wav)
        if x.dim() != 2 or x.shape[1] < 1:
            raise ValueError(f"wav must be (B, n) with n >= 1, got {tuple(x.shape)}")
        return x

    def _enc(self):
        return self.encoder.weight.view(self.channels, self.L)

    def _decode(self, W):
        """W [B, C, F] contiguous -> est [B, F hop]; the packed basis is rebuilt when the parameter moved."""
        basis = self.basis_signal.layer.weight
        packed = cached(self, "basis_packed", lambda: _native.pack_basis(basis.detach().contiguous().float()))
        return _native.basis_ola(W, packed, self.L)[:, 0, : W.shape[2] * self.hop]

    def encode(self, wav):
        """wav [B, n] -> weight [B, F, C]: the transposed view of the [B, C, F] storage, the generator's convention."""
        with torch.no_grad():
            return _native.basis_encode(self._wav(wav), self._enc().detach().contiguous()).transpose(1, 2)

    def decode(self, weight):
        """weight [B, F, C] -> est [B, F hop]."""
        w = self._prepare(weight)
        if w.dim() != 3 or w.shape[2] != self.channels:
            raise ValueError(f"weight must be (B, F, {self.channels}), got {tuple(w.shape)}")
        with torch.no_grad():
            return self._decode(w.transpose(1, 2).contiguous())

    def forward(self, wav):
        """wav [B, n] -> (est [B, F hop], weight [B, F, C]).  With grad enabled and a parameter requiring grad, est is
        on the graph of (encoder.weight, basis_signal.layer.weight); a frozen parameter gets no gradient."""
        x = self._wav(wav)
        enc, basis = self._enc(), self.basis_signal.layer.weight
        if torch.is_grad_enabled() and (enc.requires_grad or basis.requires_grad):
            est, W = _Autoencode.apply(self, x, enc, basis)
        else:
            with torch.no_grad():
                W = _native.basis_encode(x, enc.detach().contiguous())
                est = self._decode(W)
        return est, W.transpose(1, 2)


def export_dataset(directory, basis, encoder, weights):
    """Write the directory ``MODE=train --model_name basis-melgan`` reads: ``basis_signal_weight.npy`` float32 [L, C],
    ``encoder_weight.npy`` [C, L] and ``weight/<name>`` float32 [C, F] for every (name, array) of ``weights`` (an
    iterable; ``name`` is the basename of the utterance's audio path, as data.load_data_to_buffer looks it up)."""
    basis = np.ascontiguousarray(basis, dtype=np.float32)
    encoder = np.ascontiguousarray(encoder, dtype=np.float32)
    if basis.ndim != 2 or encoder.shape != basis.shape[::-1]:
        raise ValueError(f"export_dataset: basis [L, C] and encoder [C, L] expected, got {basis.shape} and {encoder.shape}")
    os.makedirs(os.path.join(directory, "weight"), exist_ok=True)
    np.save(os.path.join(directory, "basis_signal_weight.npy"), basis)
    np.save(os.path.join(directory, "encoder_weight.npy"), encoder)
    count = 0
    for name, w in weights:
        w = np.ascontiguousarray(w, dtype=np.float32)
        if w.ndim != 2 or w.shape[0] != basis.shape[1]:
            raise ValueError(f"export_dataset: weight {name} must be [{basis.shape[1]}, F], got {w.shape}")
        path = os.path.join(directory, "weight", name)
        with open(path, "wb") as f:                # np.save(path) would append ".npy" to a name without it
            np.save(f, w)
        count += 1
    return count
