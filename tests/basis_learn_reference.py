"""Torch restatement (float64 by default) of the basis autoencoder of fastvocoder_amd/basis.py, written from its two
formulas alone: with hop = L / 2 and F = ceil(n / hop),

    W[b, c, f] = relu(sum_{j < L} E[c, j] wav[b, f hop + j])                    samples at or beyond n read as 0
    est[b, t]  = sum_{f hop + j == t} sum_c basis[j, c] W[b, c, f]              t < F hop

as ``conv1d(stride=hop)`` on the right-padded waveform, ``relu``, ``einsum`` and ``fold`` cut to F hop; and of the loss
``MODE=basis`` trains on, sc + mag of the multi-resolution STFT loss (torch.stft).  Everything stays on the arguments'
graph and in their dtype, so the same text is the float64 reference and the float32 eager yardstick."""
import numpy as np
import torch
import torch.nn.functional as F

RESOLUTIONS = ((2048, 240, 1200), (1024, 120, 600), (512, 50, 240))
# the seeded cases of the chain and flip checks: (L, C, B, n)
CHAIN_CASES = ((6, 8, 2, 2520), (30, 256, 2, 2520))
FLIP_CASES = CHAIN_CASES + ((6, 8, 3, 2520), (30, 32, 1, 3000))
LEARN_CASE = (30, 256, 4, 140 * 240)


def frames(n, L):
    hop = L // 2
    return (n + hop - 1) // hop


def pre_activation(wav, enc):
    """wav [B, n], enc [C, L] -> the encoder's conv output [B, C, F] before the ReLU."""
    L = enc.shape[1]
    hop, n = L // 2, wav.shape[1]
    x = F.pad(wav, (0, (frames(n, L) - 1) * hop + L - n))
    return F.conv1d(x[:, None, :], enc[:, None, :], stride=hop)


def encode(wav, enc):
    return torch.relu(pre_activation(wav, enc))


def decode(W, basis):
    """W [B, C, F], basis [L, C] -> est [B, F hop]: the overlap-add of basis W, cut."""
    L, Fr = basis.shape[0], W.shape[2]
    hop = L // 2
    fr = torch.einsum("jc,bcf->bjf", basis, W)
    out = F.fold(fr, output_size=(1, (Fr - 1) * hop + L), kernel_size=(1, L), stride=(1, hop))
    return out[:, 0, 0, : Fr * hop]


def forward(wav, enc, basis):
    W = encode(wav, enc)
    return decode(W, basis), W


def stft_loss(x, y):
    """sc + mag of the multi-resolution STFT loss, x predicted and y ground truth (B, n), on x's graph."""
    total = 0.0
    for nf, hop, wl in RESOLUTIONS:
        w = torch.hann_window(wl, dtype=x.dtype)

        def mag(v):
            S = torch.stft(v, nf, hop, wl, w, return_complex=True)
            return torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=1e-7))
        X, Y = mag(x), mag(y)
        total = total + torch.norm(Y - X, p="fro") / torch.norm(Y, p="fro") + F.l1_loss(torch.log(Y), torch.log(X))
    return total / len(RESOLUTIONS)


def rel_err(got, want):
    """max |got - want| relative to the largest magnitude of want (1 when want is all zero)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    peak = float(np.abs(want).max()) if want.size else 0.0
    return float(np.abs(got - want).max()) / (peak if peak > 0.0 else 1.0) if want.size else 0.0


def sine_noise(B, n, seed):
    """B sine-plus-noise rows of n samples, float32."""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 24000.0
    rows = [0.3 * np.sin(2 * np.pi * (150.0 + 40 * i) * t + rs.uniform(0, 6.28)) + 0.02 * rs.randn(n) for i in range(B)]
    return np.stack(rows).astype(np.float32)


def seeded_case(L, C, B, n, seed=0, sines=True):
    """float32 (wav [B, n], enc [C, L], basis [L, C], g_est [B, F hop]) of a seed."""
    rs = np.random.RandomState(1000 * seed + 7 * L + 3 * C + B)
    wav = sine_noise(B, n, seed + L + C) if sines else rs.uniform(-1, 1, (B, n)).astype(np.float32)
    enc = (rs.uniform(-1, 1, (C, L)) / np.sqrt(L)).astype(np.float32)
    basis = (rs.uniform(-1, 1, (L, C)) / np.sqrt(C)).astype(np.float32)
    g_est = rs.uniform(-1, 1, (B, frames(n, L) * (L // 2))).astype(np.float32)
    return wav, enc, basis, g_est


def kernel_reference(wav, enc, basis, g_est, dtype=torch.float64):
    """(W, est, d_enc, d_basis) as numpy arrays in ``dtype``, for the cotangent g_est of est; d_enc flows through the
    mask of W > 0 as autograd gives it."""
    t = [torch.from_numpy(np.asarray(a)).to(dtype) for a in (wav, enc, basis, g_est)]
    e, b = t[1].requires_grad_(True), t[2].requires_grad_(True)
    est, W = forward(t[0], e, b)
    (est * t[3]).sum().backward()
    return W.detach().numpy(), est.detach().numpy(), e.grad.numpy(), b.grad.numpy()


def grad_from_weights(wav, W, basis, g_est):
    """float64 (d_enc, d_basis) of the backward alone, with W [B, C, F] given (its mask is W > 0): what
    fv_basis_learn_grad computes from its inputs."""
    wav, W, basis, g_est = (torch.from_numpy(np.asarray(a)).double() for a in (wav, W, basis, g_est))
    L, C = basis.shape
    hop, Fr, n = L // 2, W.shape[2], wav.shape[1]
    G = F.pad(g_est, (0, hop)).unfold(1, L, hop)                   # [B, F, L]: 0 behind the crop
    X = F.pad(wav, (0, (Fr - 1) * hop + L - n)).unfold(1, L, hop)   # [B, F, L]
    gW = torch.einsum("jc,bfj->bcf", basis, G) * (W > 0)
    return torch.einsum("bcf,bfj->cj", gW, X).numpy(), torch.einsum("bfj,bcf->jc", G, W).numpy()


def chain_reference(wav, enc, basis, dtype=torch.float64):
    """(loss, est, d_enc, d_basis) of stft_loss(forward(wav)[0], wav) in ``dtype``."""
    w, e, b = (torch.from_numpy(np.asarray(a)).to(dtype) for a in (wav, enc, basis))
    e.requires_grad_(True), b.requires_grad_(True)
    est, _ = forward(w, e, b)
    loss = stft_loss(est, w)
    loss.backward()
    return float(loss.detach()), est.detach().numpy(), e.grad.numpy(), b.grad.numpy()


def relu_flips(wav, enc):
    """Elements whose pre-activation lies on different sides of 0 in float32 and float64 on the CPU."""
    w, e = torch.from_numpy(np.asarray(wav)), torch.from_numpy(np.asarray(enc))
    return int(((pre_activation(w.float(), e.float()) > 0) != (pre_activation(w.double(), e.double()) > 0)).sum())


def eager_learning(wav, enc, basis, steps, lr, clip, dtype=torch.float32):
    """``steps`` Adam steps (eps 1e-6, clip_grad_norm_) on one batch with eager torch -> the loss before each step."""
    w = torch.from_numpy(np.asarray(wav)).to(dtype)
    e = torch.nn.Parameter(torch.from_numpy(np.array(enc)).to(dtype))
    b = torch.nn.Parameter(torch.from_numpy(np.array(basis)).to(dtype))
    opt = torch.optim.Adam([e, b], lr=lr, eps=1e-6)
    losses = []
    for _ in range(steps):
        loss = stft_loss(forward(w, e, b)[0], w)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_([e, b], clip)
        opt.step()
        losses.append(float(loss.detach()))
    return losses
