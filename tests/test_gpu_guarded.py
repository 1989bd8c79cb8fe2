"""Every kernel family on NaN-poisoned, red-zoned device allocations (tests/guarded_alloc.py).

Each case runs the same code twice on the same seeded inputs: once inside ``guarded()`` -- every ``torch.empty`` /
``zeros`` of the library served from a block filled with 0xFF bytes, the inputs and the parameters copied into guarded
blocks of their own -- and once plain.  The library states that its results are deterministic (no atomics, equal bits
on a second call), so the check needs no tolerance and no CPU reference: every returned tensor, gradient, parameter and
optimizer moment has the bits of the plain run and is finite wherever that is, no byte next to any allocation was
touched, and no device allocation of the library went past the guard.  An output element, a pad row of a packed image
or a column of a plan arena that a kernel never writes reads as NaN here; a store or a load that feeds a result up to
4096 bytes outside a tensor lands in a zone of 0xFF.

The closing test compares the allocation sites the cases reached with the static list of
tests/test_guarded_alloc_host.py; the sites it exempts are named in ALLOW, one reason each.  DESIGN.md section 5.4
says what the harness cannot see.

Shapes: the rows the families' own GPU grids mark as edges (named at each case), else the shortest row plus one whose
channel counts are no tile multiples."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native, audio, optim
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.discriminator import (Discriminator, DiscriminatorP, MelGANMultiScaleDiscriminator,
                                           STFTDiscriminator)
from fastvocoder_amd.discriminator.common import ConvStack
from fastvocoder_amd.generator import PQMF
from fastvocoder_amd.loss import (MultiResolutionSTFTLoss, discriminator_step_terms, generator_adversarial_terms)
from fastvocoder_amd.loss.loss import BasisWeightL1
from fastvocoder_amd.loss.stft_loss import _stft_table_host
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict, seeded_mel, seeded_state_dict
from fastvocoder_amd.train import KEYS, Trainer, samples_per_frame
from tests import basis_grad_reference as bref
from tests import cases
from tests import generator_grad_reference as gref
from tests import guarded_alloc as ga
from tests import melgan_grad_reference as mref
from tests import mpd_wgrad_reference as wref
from tests import optim_reference as oref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, SPLIT = _native.PAIR_F32, _native.PAIR_SPLIT_F16
ZERO, REFLECT = _native.PAD_ZERO, _native.PAD_REFLECT

_REACHED = set()          # guarded_alloc.Site of every allocation and pass-through seen under guarded()
_RAN = set()              # ids of the cases that ran
ALL_CASES = []            # ids of the cases this file declares (filled as the tests are defined)


# ---- the harness ----------------------------------------------------------------------------------------------------
class _Put:
    """How a case gets its tensors onto the device: plain copies, or guarded blocks of their own."""

    def __init__(self, guard):
        self.g = guard

    def __call__(self, a):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if t.dtype == torch.float64:
            t = t.float()
        return self.g.place(t) if self.g is not None else t.to(DEV).clone()

    def module(self, m):
        """``m`` on the device; under the guard every parameter and buffer in a guarded block."""
        m = m.to(DEV)
        if self.g is not None:
            with torch.no_grad():
                for t in list(m.parameters()) + list(m.buffers()):
                    t.data = self.g.place(t.data)
        return m

    @staticmethod
    def ws(n, dtype=torch.float32):
        """A workspace for a ``workspace=`` argument: under the guard it is full of NaN between its zones."""
        return torch.empty(max(int(n), 1), dtype=dtype, device=DEV)


def _flat(o, path="out"):
    if o is None:
        return []
    if torch.is_tensor(o) or isinstance(o, (bool, int, float, str)):
        return [(path, o)]
    if isinstance(o, dict):
        return [x for k, v in o.items() for x in _flat(v, f"{path}[{k!r}]")]
    if isinstance(o, (list, tuple)):
        return [x for i, v in enumerate(o) for x in _flat(v, f"{path}[{i}]")]
    raise TypeError(f"{path}: {type(o).__name__}")


def _compare(case_id, got, plain):
    got, plain = _flat(got), _flat(plain)
    assert [p for p, _ in got] == [p for p, _ in plain], case_id
    assert got, f"{case_id}: the case returned nothing to compare"
    for (path, a), (_, b) in zip(got, plain):
        if not torch.is_tensor(a):
            assert a == b or (a != a and b != b), (case_id, path, a, b)
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, (case_id, path, a.shape, b.shape)
        if not torch.equal(a, b):
            differ = (a != b) | (torch.isnan(a) != torch.isnan(b)) if a.is_floating_point() else a != b
            where = differ.reshape(-1).nonzero().reshape(-1)
            raise AssertionError(f"{case_id}: {path} {tuple(a.shape)} differs from the plain run in {where.numel()} elements, "
                                 f"the first at flat index {where[:8].tolist()}: guarded "
                                 f"{a.reshape(-1)[where[:4]].tolist()}, plain {b.reshape(-1)[where[:4]].tolist()}")
        if a.is_floating_point() or a.is_complex():
            assert bool((torch.isfinite(a) | ~torch.isfinite(b)).all()), (case_id, path)


def _twice(case_id, fn, compare=True):
    """``fn(put)`` under the guard and plain -> what the guarded run returned."""
    _RAN.add(case_id)
    with ga.guarded(DEV) as g:
        try:
            got = fn(_Put(g))
            torch.cuda.synchronize()
            touched = [repr(a) for a in g.check()]
            loose = [repr(p) for p in g.unguarded()]
            # as aligned as a plain allocation: no launcher takes another path under the guard
            assert all(a.view.data_ptr() % ga.ALIGN == 0 for a in g.allocations if a.nbytes), case_id
        finally:
            _REACHED.update(a.site for a in g.allocations)
            _REACHED.update(p.site for p in g.passed)
    plain = fn(_Put(None))
    torch.cuda.synchronize()
    assert not touched, f"{case_id}: bytes next to these allocations were written: {touched}"
    assert not loose, f"{case_id}: device allocations of the library went past the guard: {loose}"
    if compare:
        _compare(case_id, got, plain)
    return got


def _declare(ids):
    ALL_CASES.extend(ids)
    return ids


def _rs(seed):
    return np.random.RandomState(seed)


def _randn(rs, *shape, scale=1.0):
    return (scale * rs.randn(*shape)).astype(np.float32)


def _conv_w(rs, cout, cin, k):
    return _randn(rs, cout, cin, k, scale=1.0 / np.sqrt(cin * k))


# ---- a. direct entries -----------------------------------------------------------------------------------------------
DIRECT = {}


def direct(name):
    def deco(fn):
        assert name not in DIRECT
        DIRECT[name] = fn
        return fn
    return deco


@direct("pack/fold_weight_norm")
def _(put):
    rs = _rs(1)
    out = [_native.fold_weight_norm(put(_randn(rs, co, ci, k)), put(_randn(rs, co, 1, 1))) for co, ci, k in ((20, 12, 7), (1, 16, 7))]
    bn = torch.nn.BatchNorm1d(32).eval()
    with torch.no_grad():
        for t in (bn.weight, bn.bias, bn.running_mean):
            t.copy_(torch.from_numpy(_randn(rs, 32)))
        bn.running_var.copy_(torch.from_numpy(rs.uniform(0.5, 2.0, 32).astype(np.float32)))
    bn = put.module(bn)
    return out, _native.fold_batchnorm_conv(put(_conv_w(rs, 24, 32, 1)), put(_randn(rs, 24)), bn)


@direct("pack/conv_images")
def _(put):
    rs = _rs(2)
    return dict(
        conv1d=[_native.pack_conv1d(put(_conv_w(rs, co, ci, k))) for co, ci, k in ((12, 20, 7), (64, 80, 7), (1, 16, 7))],
        convt=[_native.pack_conv_transpose1d(put(_conv_w(rs, ci, co, k)), s, p)
               for ci, co, k, s, p in ((64, 32, 7, 3, 2), (32, 16, 4, 2, 1), (20, 12, 10, 5, 3))],
        upsample=[_native.pack_upsample_conv1d(put(_conv_w(rs, co, ci, k)), r, p) for co, ci, k, r, p in ((32, 64, 7, 3, 3), (12, 20, 16, 8, 7))],
        basis=_native.pack_basis(put(_randn(rs, 30, 32))),
        period=_native.pack_period_conv(put(_conv_w(rs, 128, 32, 5))),
        period_grad=_native.pack_period_conv_grad(put(_conv_w(rs, 128, 32, 5))))


@direct("pack/split_images")
def _(put):
    rs = _rs(3)
    out = dict(
        convt=[_native.pack_conv_transpose1d_split(put(_conv_w(rs, ci, co, 2 * s)), s) for ci, co, s in ((64, 32, 3), (128, 64, 8))],
        two_src=_native.pack_conv1x1_2src_split(put(_conv_w(rs, 128, 128, 1)), put(_conv_w(rs, 128, 128, 1))),
        stack=_native.pack_residual_stack_split(put(_conv_w(rs, 32, 32, 3)), put(_conv_w(rs, 32, 32, 1)), put(_conv_w(rs, 32, 32, 1))),
        pair=[_native.pack_pair(put(_conv_w(rs, c, c, k)), prec) for c, k, prec in ((16, 3, F32), (32, 11, F32), (16, 7, SPLIT),
                                                                                 (32, 11, SPLIT), (64, 3, SPLIT), (128, 7, SPLIT))])
    for c in (16, 32):
        out[f"stage{c}"] = _stage_image(put, rs, c, (3, 7, 11))[0]
    return out


def _stage_image(put, rs, c, ks, bias=True):
    w1 = [_conv_w(rs, c, c, ks[j]) for j in range(3) for _ in range(3)]
    w2 = [_conv_w(rs, c, c, ks[j]) for j in range(3) for _ in range(3)]
    b1 = [_randn(rs, c, scale=0.1) if bias else None for _ in range(9)]
    b2 = [_randn(rs, c, scale=0.1) if bias else None for _ in range(9)]
    dev = lambda lst: [None if a is None else put(a) for a in lst]          # noqa: E731
    return _native.pack_mrf_stage(dev(w1), dev(w2), dev(b1), dev(b2), ks), (w1, w2, b1, b2)


@direct("conv/fp32")
def _(put):
    rs = _rs(4)
    out = {}
    # (Cin, Cout, k, dil, pad, mode, T, B): channel counts that are no tile multiples; T = pad + 1 under reflection at
    # dilation 9 (both mirrors on one column); one output column
    for n, (ci, co, k, dil, pad, mode, T, B) in enumerate([(20, 12, 7, 3, 9, ZERO, 50, 2), (16, 16, 3, 9, 9, REFLECT, 10, 3),
                                                           (80, 64, 7, 1, 0, ZERO, 7, 1)]):
        x, w, b = put(_randn(rs, B, ci, T)), put(_conv_w(rs, co, ci, k)), put(_randn(rs, co))
        tout = T + 2 * pad - dil * (k - 1)
        act = torch.empty((B, co, tout), dtype=torch.float32, device=DEV)
        y = _native.conv1d_fused(x, _native.pack_conv1d(w), b, co, k, dil=dil, pad=pad, pad_mode=mode, pre_slope=0.1, out_act=act,
                                 act_slope=0.2)
        out[f"conv{n}"] = (y, act)
    x, x2 = put(_randn(rs, 2, 16, 33)), put(_randn(rs, 2, 8, 33))
    w = put(np.concatenate([_conv_w(rs, 12, 16, 1), _conv_w(rs, 12, 8, 1)], axis=1))
    out["two_src"] = _native.conv1d_2src_fused(x, x2, _native.pack_conv1d(w), put(_randn(rs, 12)), 12, res=put(_randn(rs, 2, 12, 33)))
    # tests/test_gpu_generator_grad.py CONVT_GRID: k % s != 0 with k > 2 s; one input sample
    for n, (ci, co, k, s, p, op, T, B) in enumerate([(64, 32, 7, 3, 2, 1, 6, 2), (32, 16, 4, 2, 1, 0, 1, 1)]):
        x, w = put(_randn(rs, B, ci, T)), put(_conv_w(rs, ci, co, k))
        out[f"convt{n}"] = _native.conv_transpose1d_fused(x, _native.pack_conv_transpose1d(w, s, p), put(_randn(rs, co)), co, k, s, p, op,
                                                          pre_slope=0.1)
    for n, (ci, co, k, r, p, T, B) in enumerate([(64, 32, 7, 3, 3, 11, 2), (20, 12, 16, 8, 7, 3, 1)]):
        x, w = put(_randn(rs, B, ci, T)), put(_conv_w(rs, co, ci, k))
        out[f"upsample{n}"] = _native.upsample_conv1d_fused(x, _native.pack_upsample_conv1d(w, r, p), put(_randn(rs, co)), co, k, r, p,
                                                            pre_slope=0.1)
    return out


@direct("conv/split_f16")
def _(put):
    rs = _rs(5)
    out = {}
    # (C, k, dil, mode, T, B): MelGAN's dilation 9 at T = pad + 1 under reflection; a length that is no tile multiple
    for n, (c, k, dil, mode, T, B) in enumerate([(64, 3, 9, REFLECT, 10, 3), (64, 11, 5, ZERO, 37, 2), (128, 7, 3, ZERO, 131, 1)]):
        xs = [put(_randn(rs, B, c, T)) for _ in range(2)]
        packed = [_native.pack_pair(put(_conv_w(rs, c, c, k)), SPLIT) for _ in range(2)]
        out[f"conv{n}"] = _native.conv1d_split_f16(xs, packed, [put(_randn(rs, c, scale=0.1)) for _ in range(2)], [k, k], dil, pre_slope=0.1,
                                                   res=[put(_randn(rs, B, c, T)) for _ in range(2)], pad_mode=mode)
    x, x2 = put(_randn(rs, 2, 128, 37)), put(_randn(rs, 2, 128, 37))
    packed = _native.pack_conv1x1_2src_split(put(_conv_w(rs, 128, 128, 1)), put(_conv_w(rs, 128, 128, 1)))
    out["two_src"] = _native.conv1x1_2src_split_f16(x, x2, packed, put(_randn(rs, 128, scale=0.1)), pre_slope=0.2)
    for n, (ci, co, s, p, op, T, B) in enumerate([(64, 32, 3, 2, 1, 11, 2), (128, 64, 8, 4, 0, 1, 1)]):
        x, w = put(_randn(rs, B, ci, T)), put(_conv_w(rs, ci, co, 2 * s))
        out[f"convt{n}"] = _native.conv_transpose1d_split_f16(x, _native.pack_conv_transpose1d_split(w, s), put(_randn(rs, co, scale=0.1)),
                                                              co, 2 * s, s, p, op, pre_slope=0.1)
    # the one-launch ResidualStack: T = pad + 1 at dilation 9, and more than one tile
    for n, (c, dil, T, B) in enumerate([(32, 9, 10, 3), (64, 3, 70, 2)]):
        packed = _native.pack_residual_stack_split(put(_conv_w(rs, c, c, 3)), put(_conv_w(rs, c, c, 1)), put(_conv_w(rs, c, c, 1)))
        out[f"stack{n}"] = _native.residual_stack_split_f16(put(_randn(rs, B, c, T)), packed, put(_randn(rs, c, scale=0.1)),
                                                            put(_randn(rs, c, scale=0.1)), 3, dil, 0.2, pad_mode=REFLECT)
    return out


@direct("pair/fused")
def _(put):
    rs = _rs(6)
    out = {}
    ks = (3, 7, 11)
    # (C, arithmetic, dil, T, B): 16 / 32 channels in fp32 and split-f16; 64 channels (two conv launches through `mids`);
    # the pair kernels take rows of whole 16 bytes: T = 4 is the shortest
    for n, (c, prec, dil, T, B) in enumerate([(16, F32, 3, 68, 2), (32, F32, 5, 4, 1), (32, SPLIT, 1, 68, 3), (64, SPLIT, 5, 36, 2)]):
        xs = [put(_randn(rs, B, c, T)) for _ in ks]
        w1 = [_native.pack_pair(put(_conv_w(rs, c, c, k)), prec) for k in ks]
        w2 = [_native.pack_pair(put(_conv_w(rs, c, c, k)), prec) for k in ks]
        b1, b2 = ([put(_randn(rs, c, scale=0.1)) for _ in ks] for _ in range(2))
        out[f"pair{n}"] = _native.resblock1_fused(xs, w1, w2, b1, b2, list(ks), dil, 0.1, prec=prec)
        if c == 16 and prec == F32:
            out["mrf_stage"] = _native.mrf_stage(xs, w1, w2, b1, b2, list(ks), dil, 0.1)
    return out


@direct("stage/one_launch")
def _(put):
    rs = _rs(7)
    out = {}
    ks = (3, 7, 11)
    for c, T, B in ((16, 67, 2), (32, 67, 2), (32, 1, 1), (32, 300, 3)):
        packed, _ = _stage_image(put, rs, c, ks)
        x = put(_randn(rs, B, c, T))
        act = torch.empty_like(x)
        out[f"stage{c}_{T}"] = (_native.mrf_stage_split_f16(x, packed, ks, out_act=act, act_slope=0.1), act)
        fold = (put(_randn(rs, c, 7, scale=0.1)), put(_randn(rs, 1)))
        out[f"fold{c}_{T}"] = _native.mrf_stage_split_f16(x, packed, ks, fold=fold, act_slope=0.01, post=_native.POST_TANH)
    # two block classes need two blocks per utterance: tests/test_gpu_stage_classes.py's one window per class (two blocks
    # forced) and its two utterances of 1800 columns under the launcher's own choice
    try:
        for T, B, blocks in ((252, 1, 2), (1800, 2, 0)):
            _native.tuning_set("mrf_blocks", blocks)
            packed, _ = _stage_image(put, rs, 32, ks)
            x = put(_randn(rs, B, 32, T))
            out[f"classes_{T}"] = _native.mrf_stage_classes_f16(x, packed, ks, work=_native.mrf_stage_workspace(32, DEV))
            out[f"classes_own_work_{T}"] = _native.mrf_stage_classes_f16(x, packed, ks)
            out[f"class_a_{T}"] = _native.mrf_stage_one_class_f16(x, packed, ks, "a")
            out[f"class_b_{T}"] = _native.mrf_stage_one_class_f16(x, packed, ks, "b", work=_native.mrf_stage_workspace(32, DEV))
    finally:
        _native.tuning_set("mrf_blocks", 0)
    return out


@direct("pqmf_basis_wav")
def _(put):
    rs = _rs(8)
    pqmf = put.module(PQMF())
    out = {}
    for n, (B, T) in enumerate([(2, 4 * 61 + 3), (1, 4), (3, 1001)]):
        sub = _native.pqmf_analysis(put(_randn(rs, B, 1, T)), pqmf.analysis_filter)
        out[f"pqmf{n}"] = (sub, pqmf.synthesis(sub))
    w = put(_conv_w(rs, 4, 16, 7))
    out["conv_post_pqmf"] = [_native.conv_post_pqmf(put(_randn(rs, B, 16, T)), _native.pack_conv1d(w), put(_randn(rs, 4, scale=0.1)),
                                                    pqmf.synthesis_filter, 7, 3, pre_slope=0.01) for B, T in ((2, 37), (1, 1))]
    packed = _native.pack_basis(put(_randn(rs, 30, 32)))
    out["ola"] = [_native.basis_ola(put(_randn(rs, B, 32, F)), packed, 30) for B, F in ((2, 9), (1, 1), (3, 130))]
    out["wav"] = [_native.encode_16bits(put(_randn(rs, *shape)), 0.9) for shape in ((3, 1001), (1,), (2, 4099))]
    return out


@direct("audio")
def _(put):
    rs = _rs(9)
    n_fft, hop, win = audio._stft_parameters()
    hp = audio.hparams
    mel_tab, gl_tab, inv = put(audio._mel_table_host()), put(audio._gl_table_host()), put(audio._inv_mel_basis_host())
    out = {}
    # n = n_fft / 2 + 1 is the shortest the reflect padding takes; 1680 = 7 hops
    out["mel"] = [_native.melspectrogram(put(_randn(rs, B, n, scale=0.3)), mel_tab, hp.sample_rate, n_fft, hop, win, hp.num_mels, float(hp.fmin)) for B, n in ((1, 1025), (3, 1680), (2, 2401))]
    y = put(_randn(rs, 2, 1680, scale=0.3))
    spec = _native.stft_complex(y, gl_tab, n_fft, hop, win)
    out["stft"] = torch.view_as_real(spec)
    out["istft"] = _native.istft(spec, gl_tab, n_fft, hop, win)
    S = _native.mel_to_linear(put(rs.rand(2, 80, 8).astype(np.float32)), inv, 1.5)
    out["mel_to_linear"] = S
    phase = torch.view_as_complex(put(np.stack([np.cos(a := 2 * np.pi * rs.rand(2, 8, n_fft // 2 + 1)), np.sin(a)], -1).astype(np.float32)))
    out["griffin_lim"] = _native.griffin_lim(S, phase, gl_tab, 3, None, n_fft, hop, win)
    out["griffin_lim_from_y"] = _native.griffin_lim(S, None, gl_tab, 2, out["griffin_lim"], n_fft, hop, win)
    out["inv_preemphasis"] = [_native.inv_preemphasis(put(_randn(rs, B, n)), 0.97) for B, n in ((2, 1680), (1, 1), (3, 4099))]
    # the module's own entries (their tables are the device's cached copies)
    out["inv_mel_spectrogram"] = audio.inv_mel_spectrogram(put(rs.rand(2, 80, 8).astype(np.float32)), seed=3, iters=2)
    out["melspectrogram"] = audio.melspectrogram(put(_randn(rs, 2, 1300, scale=0.3)))
    return out


@direct("resample")
def _(put):
    rs = _rs(10)
    out = {}
    # tests/test_gpu_resample.py: down, up by a ratio of large terms, int16 PCM; one sample; lengths that are no block multiples
    for n, (orig, target, B, n_in, pcm) in enumerate([(24000, 16000, 2, 1001, False), (22050, 24000, 1, 777, True),
                                                      (48000, 24000, 3, 1, False), (16000, 24000, 1, 4099, False)]):
        L, M, _, half = audio._resample_geometry(orig, target)
        table = put(audio._resample_table_host(orig, target).reshape(-1))
        x = put((rs.randint(-30000, 30000, (B, n_in)).astype(np.int16)) if pcm else _randn(rs, B, n_in, scale=0.3))
        out[f"resample{n}"] = _native.resample(x, table, L, M, half)
    out["module"] = audio.resample(put(_randn(rs, 2, 1001, scale=0.3)), 24000, 16000)
    return out


RESOLUTIONS = [(2048, 240, 1200), (1024, 120, 600), (512, 50, 240)]


@direct("stft_loss")
def _(put):
    rs = _rs(11)
    tables = [put(_stft_table_host(nf, wl)) for nf, _, wl in RESOLUTIONS]
    geometry = ([r[0] for r in RESOLUTIONS], [r[1] for r in RESOLUTIONS], [r[2] for r in RESOLUTIONS])
    out = {}
    for B, n in ((1, 1025), (3, 1301)):          # the shortest the 2048-point reflect padding takes; no hop multiple
        x, y = put(_randn(rs, B, n, scale=0.3)), put(_randn(rs, B, n, scale=0.3))
        out[f"distance{n}"] = _native.stft_distance(x, y, tables, *geometry)
        out[f"distance_grad{n}"] = _native.stft_distance_grad(x, y, tables, *geometry, put(_randn(rs, 3, B, 2)))
        for (nf, hop, wl), tab in zip(RESOLUTIONS, tables):
            mag = _native.stft_magnitude(x, tab, nf, hop, wl)
            bins = _native.stft_magnitude_bins(x, tab, nf, hop, wl)
            grad = _native.stft_magnitude_bins_grad(x, put(_randn(rs, *bins.shape)), tab, nf, hop, wl)
            out[f"magnitude{n}_{nf}"] = (mag, bins, grad)
    return out


@direct("disc/forward")
def _(put):
    rs = _rs(12)
    out = {}
    # tests/test_gpu_disc_grad.py: the "positions beyond the last window" shape (1030 - 41 = 4 * 247 + 1), and T = 3
    for n, (ci, co, k, s, pad, T, B) in enumerate([(16, 64, 41, 4, 0, 1030, 1), (8, 32, 13, 2, 6, 3, 3), (4, 1, 11, 1, 5, 999, 2)]):
        out[f"grouped{n}"] = _native.grouped_conv1d(put(_randn(rs, B, ci, T)), put(_conv_w(rs, co, 4, k)), put(_randn(rs, co)), k, s, pad, 0.2)
    out["pool"] = [_native.avg_pool1d(put(_randn(rs, 3, 1, T)), k, s, p) for T, k, s, p in ((2, 4, 2, 1), (5, 4, 2, 2), (1001, 4, 2, 1))]
    # period convs at periods 2 and 11, batch 3, H = 4 rows: the smallest height with two output rows
    for p in (2, 11):
        T = 4 * p - 1                                             # a reflect tail of one sample
        out[f"first{p}"] = _native.mpd_conv_first(put(_randn(rs, 3, 1, T, scale=0.5)), put(_conv_w(rs, 32, 1, 5).reshape(32, 5)),
                                                  put(_randn(rs, 32, scale=0.1)), p)
        for ci, co in ((32, 128), (128, 512)):
            packed = _native.pack_period_conv(put(_conv_w(rs, co, ci, 5)))
            out[f"period{p}_{ci}"] = _native.period_conv(put(_randn(rs, 3, ci, 4, p)), packed, put(_randn(rs, co, scale=0.1)), co)
    es = [put(_randn(rs, 2, c, t)) for c, t in ((1, 1), (3, 2049), (16, 700))]
    rr = [put(_randn(rs, *e.shape)) for e in es]
    out["score_sums"] = _native.disc_score_sums(es, rr)
    return out


@direct("disc/input_grad")
def _(put):
    rs = _rs(13)
    out = {}
    for n, (ci, co, k, s, pad, T, B) in enumerate([(16, 64, 41, 4, 0, 1030, 1), (8, 32, 13, 2, 6, 3, 3), (4, 4, 3, 5, 0, 40, 1)]):
        tout = (T + 2 * pad - k) // s + 1
        g_up, g_map, y = (put(_randn(rs, B, co, tout)) for _ in range(3))
        w = put(_conv_w(rs, co, 4, k))
        out[f"grouped{n}"] = (_native.grouped_conv1d_input_grad(g_up, g_map, y, w, ci, T, k, s, pad, 0.2),
                              _native.grouped_conv1d_input_grad(g_up, None, None, w, ci, T, k, s, pad, 1.0))
    out["map"] = [_native.disc_map_grad(put(_randn(rs, 2, 3, n)), put(_randn(rs, 2, 3, n)), put(_randn(rs, 2, 3, n)), 0.2)
                  for n in (1, 257, 4099)]
    out["fold"] = [_native.reflect_pad_fold(put(_randn(rs, 3, 2, T + 2 * P)), P) for T, P in ((8, 7), (9, 7), (5, 0), (1027, 7))]
    out["pool"] = [_native.avg_pool1d_input_grad(put(_randn(rs, 3, 1, (T + 2 * p - k) // s + 1)), T, k, s, p)
                   for T, k, s, p in ((2, 4, 2, 1), (5, 4, 2, 2), (1001, 4, 2, 1), (8, 5, 3, 0))]
    es = [put(_randn(rs, 2, c, t)) for c, t in ((1, 1), (3, 2049), (16, 700))]
    rr = [put(_randn(rs, *e.shape)) for e in es]
    out["score"] = _native.disc_score_grad(es, rr, [(0.3, 0.0, 0.0), (0.0, 0.25, 0.5), (0.7, -0.2, 0.1)], skip=[False, True, False])
    for p in (2, 11):
        T = 4 * p - 1
        g_up, g_map, y0 = (put(_randn(rs, 3, 32, 2, p)) for _ in range(3))
        out[f"first{p}"] = _native.mpd_first_input_grad(g_up, g_map, y0, put(_conv_w(rs, 32, 1, 5).reshape(32, 5)), T)
        packed = _native.pack_period_conv_grad(put(_conv_w(rs, 128, 32, 5)))
        g_up, g_map, y = (put(_randn(rs, 3, 128, 2, p)) for _ in range(3))
        out[f"period{p}"] = _native.period_conv_input_grad(g_up, g_map, y, packed, 32, 4)
    return out


@direct("disc/weight_grad")
def _(put):
    rs = _rs(14)
    out = {}
    for n, (ci, co, k, s, pad, T, B) in enumerate([(16, 64, 41, 4, 0, 1030, 1), (8, 32, 13, 2, 6, 3, 3)]):
        tout = (T + 2 * pad - k) // s + 1
        g, x = put(_randn(rs, B, co, tout)), put(_randn(rs, B, ci, T))
        ws = put.ws(_native.conv_weight_grad_workspace_floats(True, B, ci, co, T, k, s, pad))
        out[f"grouped{n}"] = (_native.grouped_conv1d_weight_grad(g, x, k, s, pad, True, True),
                              _native.grouped_conv1d_weight_grad(g, x, k, s, pad, True, True, workspace=ws))
    # the MFD's first layer (tests/test_gpu_mpd_wgrad.py): 257 bins under reflection, 8 frames
    g, x = (put(a) for a in wref.mfd_first_inputs(257, 8, 3))
    ws = put.ws(_native.conv_weight_grad_workspace_floats(False, 3, 257, 64, 8, 15, 1, 7, REFLECT))
    out["dense"] = (_native.conv1d_weight_grad(g, x, 15, 7, REFLECT, True, True),
                    _native.conv1d_weight_grad(g, x, 15, 7, REFLECT, True, True, workspace=ws))
    g, x = put(_randn(rs, 2, 12, 50)), put(_randn(rs, 2, 20, 50))
    out["dense_zero"] = _native.conv1d_weight_grad(g, x, 5, 2, ZERO, True, True)
    # strides 3 and 1 (tests/mpd_wgrad_reference.py KERNEL_LAYERS) at periods 2 and 11, batch 3, two output rows
    for p in (2, 11):
        for ci, co, k, s in ((32, 128, 5, 3), (1024, 1024, 5, 1), (1024, 1, 3, 1)):
            H = 4 if s == 3 else 2
            g, x = (put(a) for a in wref.kernel_inputs(ci, co, k, s, p, H, 3))
            for prec in ("f32", "bf16"):
                ws = put.ws(_native.period_conv_weight_grad_workspace_floats(3, ci, co, H, p, k, s, prec))
                out[f"period{p}_{ci}_{co}_{prec}"] = (_native.period_conv_weight_grad(g, x, k, s, True, True, precision=prec),
                                                      _native.period_conv_weight_grad(g, x, k, s, True, True, workspace=ws, precision=prec))
        T = 4 * p - 1
        g, x = (put(a) for a in wref.first_inputs(p, T, 3))
        out[f"first{p}"] = (_native.mpd_first_weight_grad(g, x, True, True),
                            _native.mpd_first_weight_grad(g, x, True, True, workspace=put.ws(1 << 14)))
    dw, v, gg = put(_randn(rs, 20, 12, 7)), put(_randn(rs, 20, 12, 7)), put(_randn(rs, 20, 1, 1))
    out["weight_norm"] = (_native.weight_norm_grad(dw, v, gg), _native.weight_norm_grad(put(_randn(rs, 1, 16, 7)), put(_randn(rs, 1, 16, 7)),
                                                                                         put(_randn(rs, 1, 1, 1))))
    return out


@direct("gen/weight_grad")
def _(put):
    out = {}
    # tests/test_gpu_generator_grad.py DILATED_GRID: channel counts that are no tile multiples; only the centre tap alive;
    # and a reduction of three blocks with a ragged end
    for ci, co, k, dil, T, B in ((20, 12, 7, 3, 50, 2), (16, 16, 11, 5, 1, 1), (8, 8, 3, 1, 65, 3)):
        pad = dil * (k - 1) // 2
        g, x = (put(a) for a in gref.kernel_inputs((B, co, T), (B, ci, T), ci + co + k + T))
        for prec in ("f32", "bf16"):
            ws = put.ws(_native.conv1d_weight_grad_dilated_workspace_floats(B, ci, co, T, k, dil, pad, precision=prec))
            out[f"dilated_{ci}_{k}_{T}_{prec}"] = (_native.conv1d_weight_grad_dilated(g, x, k, dil, pad, True, True, precision=prec),
                                                   _native.conv1d_weight_grad_dilated(g, x, k, dil, pad, True, True, workspace=ws, precision=prec))
    # tests/test_gpu_melgan_grad.py: T = pad + 1 at dilation 9 under reflection, a ragged and a one-row channel pair
    for ci, co, B in ((48, 48, 3), (32, 1, 1), (80, 64, 1)):
        k, dil, pad, T = 3, 9, 9, 10
        g, x = (put(a) for a in gref.kernel_inputs((B, co, T), (B, ci, T), ci + co + T))
        for prec in ("f32", "bf16"):
            ws = put.ws(_native.conv1d_weight_grad_dilated_workspace_floats(B, ci, co, T, k, dil, pad, REFLECT, prec))
            out[f"reflect_{ci}_{co}_{prec}"] = (
                _native.conv1d_weight_grad_dilated(g, x, k, dil, pad, True, True, pad_mode=REFLECT, precision=prec),
                _native.conv1d_weight_grad_dilated(g, x, k, dil, pad, True, True, workspace=ws, pad_mode=REFLECT, precision=prec))
        wt = put(_conv_w(_rs(ci), ci, co, k))
        out[f"reflect_input_{ci}_{co}"] = _native.conv1d_input_grad_reflect(g, wt, T, dil, pad)
    # CONVT_GRID: k % s != 0 with k > 2 s; one input sample
    for ci, co, k, s, p, op, T, B in ((64, 32, 7, 3, 2, 1, 6, 2), (32, 16, 4, 2, 1, 0, 1, 1)):
        tout = gref.convt_out_len(T, k, s, p, op)
        g, x = (put(a) for a in gref.kernel_inputs((B, co, tout), (B, ci, T), ci + co + k + s + T))
        out[f"convt_input_{ci}"] = _native.conv_transpose1d_input_grad(g, put(_conv_w(_rs(k + s), ci, co, k)), T, s, p, op)
        for prec in ("f32", "bf16"):
            ws = put.ws(_native.conv_transpose1d_weight_grad_workspace_floats(B, ci, co, T, k, s, p, op, prec))
            out[f"convt_{ci}_{prec}"] = (_native.conv_transpose1d_weight_grad(g, x, k, s, p, op, True, True, precision=prec),
                                         _native.conv_transpose1d_weight_grad(g, x, k, s, p, op, True, True, workspace=ws, precision=prec))
    return out


@direct("gen/elementwise")
def _(put):
    rs = _rs(16)
    out = {}
    for shape in ((3, 7, 1031), (1, 1, 1)):
        g, d, x, acc = (put(_randn(rs, *shape)) for _ in range(4))
        out[str(shape)] = (_native.tanh_grad(g, put(np.tanh(_randn(rs, *shape)))), _native.residual_merge_grad(g, d, x, 0.1),
                           _native.residual_merge_grad(g, d, x, 0.1, acc=acc), _native.grad_div(g, 3.0))
    return out


@direct("basis")
def _(put):
    rs = _rs(17)
    out = {}
    for B, c, F, L_ in ((2, 32, 17, 30), (1, 24, 1, 30), (3, 32, 70, 30)):        # rows of tests/test_gpu_basis_grad.py's axes
        Y, basis = put(_randn(rs, B + 1, c, F)), put(_randn(rs, L_, c, scale=0.2))
        D = _native.basis_head_forward(Y)
        g_est, g_w = put(_randn(rs, B, F * (L_ // 2))), put(_randn(rs, B, c, F))
        target = put(_randn(rs, B, F, c))
        out[f"head{F}"] = (D, _native.basis_head_grad(g_est, g_w, Y, basis), _native.basis_head_grad(g_est, None, Y, basis),
                           _native.basis_head_grad(None, g_w, Y, basis))
        out[f"l1_{F}"] = (_native.basis_weight_l1(D, target), _native.basis_weight_l1_grad(D, target, put(_randn(rs, 1))),
                          _native.basis_weight_l1_grad(D, target))
        n = F * (L_ // 2) - 4                                      # the last frame reaches past the waveform
        wav, enc = put(_randn(rs, B, n, scale=0.3)), put(_randn(rs, c, L_, scale=0.2))
        W = _native.basis_encode(wav, enc)
        nbytes = _native.lib().fv_basis_learn_grad_workspace_bytes(B, n, c, L_)
        out[f"learn{F}"] = (W, _native.basis_learn_grad(wav, g_est, W, basis),
                            _native.basis_learn_grad(wav, g_est, W, basis, workspace=put.ws((nbytes + 3) // 4)))
    return out


@pytest.mark.parametrize("name", _declare([f"direct/{k}" for k in DIRECT]))
def test_direct_entries(name):
    _twice(name, DIRECT[name[len("direct/"):]])


def _adam_case(put, bucket):
    """tests/optim_reference.py: six tensors (one a view 4 bytes into its storage), three steps, a skipped gradient."""
    params = []
    for k, p in enumerate(oref.initial_parameters()):
        if k == len(oref.all_shapes()) - 1:
            base = put(np.concatenate([np.zeros(1, np.float32), p]))
            t = base[1:]
        else:
            t = put(p)
        params.append(t.requires_grad_(True))
    opt = optim.Adam(params, lr=oref.LRS[0], betas=oref.BETAS, eps=oref.EPS)
    norms = []
    for s in range(oref.STEPS):
        for group in opt.param_groups:
            group["lr"] = oref.LRS[s]
        for p, g in zip(params, oref.gradients(s)):
            p.grad = None if g is None else put(g)
        if bucket and s == 0:
            # the data-parallel step's own launch without a process group: every gradient into its span of the bucket
            rows, touched, spans, device, src, flat, views = opt._rows_bucket()
            host, first = optim.adam_table(rows, src)
            table = opt._upload(host, device)
            _native.grad_bucket_pack(table, len(rows), int(first[-1]), 0.5)
            norms.append(flat.clone())
            for p in params:                                      # _rows_bucket advanced the step counts: as before
                opt.state[p]["step"] -= 1
        norms.append(opt.step(max_norm=oref.CLIP_ON))
    state = [(opt.state[p].get("exp_avg"), opt.state[p].get("exp_avg_sq"), float(opt.state[p]["step"])) for p in params]
    return norms, [p.detach() for p in params], [p.grad for p in params], state


@pytest.mark.parametrize("name", _declare(["adam/clip_and_step", "adam/bucket_pack"]))
def test_adam_step_with_clipping(name):
    _twice(name, functools.partial(_adam_case, bucket=name.endswith("bucket_pack")))


def test_the_timing_hook_stays_inside_its_scratch():
    _twice("hook/mfma_rate", lambda put: _native.profile_mfma_f16_rate(launches=2, iters=8) > 0)


_declare(["hook/mfma_rate"])


# ---- b. whole generators ---------------------------------------------------------------------------------------------
def _generator(put, name, cfg, seed=0, train=False):
    m = build_generator(name, cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in seeded_state_dict(name, cfg, seed=seed).items()})
    return put.module(m.train() if train else m.eval())


def _arenas(m):
    plans = [v[1] for v in m._fv_plans.values() if isinstance(v, tuple) and len(v) == 2]
    return [plan._ws for plan in plans if getattr(plan, "_ws", None) is not None]


def _forward(name, cfg, B, T, **policy):
    def fn(put):
        m = _generator(put, name, cfg)
        for k, v in policy.items():
            setattr(m, k, v)
        with torch.no_grad():
            out = m(put(seeded_mel(T, seed=21000 + T, batch=B)))
        assert not m.check_range()
        return out
    return fn


@pytest.mark.parametrize("tag", _declare([f"small/{c[0]}" for c in cases.SMALL]))
def test_small_generators(tag):
    _, name, cfg = next(c for c in cases.SMALL if c[0] == tag[len("small/"):])
    _twice(tag, _forward(name, cfg, cases.SMALL_B, cases.SMALL_T))


@pytest.mark.parametrize("B,T", [(1, 37), (3, 24)])
@pytest.mark.parametrize("tag", [c[0] for c in cases.SHIPPED])
def test_shipped_generators(tag, B, T):
    _, name, path = next(c for c in cases.SHIPPED if c[0] == tag)
    _twice(f"shipped/{tag}/{B}x{T}", _forward(name, cases.load_conf(path), B, T))


_declare([f"shipped/{c[0]}/{B}x{T}" for c in cases.SHIPPED for B, T in ((1, 37), (3, 24))])

# the (B, T) rows of tests/test_gpu_parity.py test_saturated_kernel_forms_vs_aten_port
SATURATED = [("hifigan", "conf/hifigan/light.yaml", 12, 500), ("hifigan", "conf/hifigan/large.yaml", 6, 250),
             ("multiband-hifigan", "conf/multiband-hifigan/light.yaml", 12, 500), ("basis-melgan", "conf/basis-melgan/light.yaml", 12, 500),
             ("melgan", "conf/melgan/original.yaml", 8, 300)]


@pytest.mark.parametrize("name,path,B,T", SATURATED, ids=[f"{p.split('/', 1)[1][:-5]}_B{B}" for _, p, B, _ in SATURATED])
def test_saturated_kernel_forms(name, path, B, T):
    _twice(f"saturated/{path}", _forward(name, cases.load_conf(path), B, T))


_declare([f"saturated/{p}" for _, p, _, _ in SATURATED])

POLICIES = [("precision", "f32"), ("fuse_pairs", False), ("fuse_stage", False), ("fold_post", False), ("range_guard", "off")]


@pytest.mark.parametrize("attr,value", POLICIES)
def test_hifigan_light_under_each_policy(attr, value):
    fn = _forward("hifigan", cases.load_conf("conf/hifigan/light.yaml"), 2, 120, **{attr: value})
    _twice(f"policy/{attr}", fn)


_declare([f"policy/{a}" for a, _ in POLICIES])


def test_a_long_a_shorter_and_the_long_input_again_on_one_module_with_the_arena_poisoned():
    cfg = cases.load_conf("conf/hifigan/light.yaml")

    def fn(put):
        m = _generator(put, "hifigan", cfg)
        long, short = put(seeded_mel(120, seed=61, batch=2)), put(seeded_mel(37, seed=62, batch=2))
        out = []
        with torch.no_grad():
            for n, x in enumerate((long, short, long)):
                if n and put.g is not None:
                    arenas = _arenas(m)
                    assert arenas, "no plan arena was found to poison"
                    for ws in arenas:
                        ga.poison(ws)
                out.append(m(x).clone())
        assert torch.equal(out[0], out[2])
        return out
    _twice("arena/long_short_long", fn)


_declare(["arena/long_short_long"])


@pytest.mark.parametrize("what", _declare(["flows/inference_minus", "flows/chunked", "flows/chunked_basis"]))
def test_inference_minus_and_chunked_inference(what):
    name, path = ("basis-melgan", "conf/basis-melgan/light.yaml") if what.endswith("basis") else \
        ("multiband-hifigan", "conf/multiband-hifigan/light.yaml")
    cfg = cases.load_conf(path)

    def fn(put):
        m = _generator(put, name, cfg)
        mel = seeded_mel(48, seed=5)
        with torch.no_grad():
            if what.endswith("minus"):
                bias = m.inference(np.zeros_like(mel)).clone()
                return bias, m.inference_minus(mel, bias)
            # (the chunked run meets the whole run within 1e-5, tests/test_gpu_parity.py: other tile shapes; each of the
            # two is compared with its own plain run here)
            whole = m(put(mel.T[None].copy()))
            m.max_frames_per_run = 11
            return whole, m(put(mel.T[None].copy()))
    _twice(what, fn)


# ---- c. discriminators and losses -------------------------------------------------------------------------------------
SMALL_MSD = dict(channels=4, max_downsample_channels=16, downsample_scales=[4, 2])      # tests/test_gpu_disc_grad.py


def _disc(put, kind):
    """(module, estimate, real, keywords of the two term functions) of a small discriminator case."""
    if kind == "msd":
        module = MelGANMultiScaleDiscriminator(**SMALL_MSD)
        sd = seeded_discriminator_state_dict("msd", 3, **SMALL_MSD)
        est, real = wref.signals(3, 2001)
        kw_g, kw_d = {}, {}
    else:
        name = kind.split("_")[0]
        _, kw = wref.case_kind(name)
        module = STFTDiscriminator(**wref.SMALL_STFT) if name == "stft" else DiscriminatorP(kw["period"])
        sd = wref.case_state_dict(name)
        est, real = wref.case_signals(name)
        kw_g, kw_d = (({}, dict(stft_grad=True)) if name == "stft" else (dict(period_grad=True), dict(period_grad=True)))
    module.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()})
    module = put.module(module.eval())
    if kind.endswith("_bf16"):
        module.grad_precision = "bf16"
    return module, put(est), put(real), kw_g, kw_d


DISCS = ["msd", "p2", "p11", "p3_bf16", "stft"]


@pytest.mark.parametrize("kind", DISCS)
def test_discriminator_forward_input_gradient_and_parameter_gradient(kind):
    def fn(put):
        module, est, real, kw_g, kw_d = _disc(put, kind)
        with torch.no_grad():
            maps = module(est)
        est_g = put(est.detach()).requires_grad_(True)
        terms = generator_adversarial_terms(module, est_g, real, **kw_g)
        (terms["adversarial"] + terms["feature_map"]).backward()
        assert all(q.grad is None for q in module.parameters())
        step = discriminator_step_terms(module, est, real, **kw_d)
        step["discriminator"].backward()
        grads = {k: q.grad for k, q in module.named_parameters()}
        assert all(v is not None for v in grads.values())
        return maps, {k: v.detach() for k, v in terms.items()}, est_g.grad, {k: v.detach() for k, v in step.items()}, grads
    _twice(f"disc/{kind}", fn)


_declare([f"disc/{k}" for k in DISCS])


def test_the_zero_gradient_of_an_input_no_map_reaches():
    """The walks' answer when no map carries a gradient (the backward's None inputs): zeros, from no launch."""
    def fn(put):
        msd, est, _, _, _ = _disc(put, "msd")
        stack = next(m for m in msd.modules() if isinstance(m, ConvStack))
        n = len(stack._native_grad_layers())
        params = [q for ps in stack._conv_params() for q in ps]
        gx, gparams = stack._param_grad(est, [None] * n, params, [None] * n, True, [False] * len(params))
        assert all(g is None for g in gparams)
        period, est_p, _, _, _ = _disc(put, "p3")
        with torch.no_grad():
            outs = period._run_layers(est_p)
        return stack._input_grad(est, [None] * n, [None] * n), gx, period._input_grad(est_p, outs, [None] * len(outs))
    got = _twice("disc/zero_gradient", fn)
    assert all(not t.any() for t in got)


_declare(["disc/zero_gradient"])


def test_differentiable_multi_resolution_stft_loss():
    def fn(put):
        mr = put.module(MultiResolutionSTFTLoss())
        mr.differentiable = True
        rs = _rs(21)
        x, y = put(_randn(rs, 3, 1301, scale=0.3)).requires_grad_(True), put(_randn(rs, 3, 1301, scale=0.3))
        sc, mag = mr(x, y)
        (sc + mag).backward()
        with torch.no_grad():
            plain = mr(x.detach(), y)
        return sc.detach(), mag.detach(), x.grad, plain
    _twice("loss/mr_stft", fn)


_declare(["loss/mr_stft"])


# ---- d. generators in training ----------------------------------------------------------------------------------------
def _training_case(tag):
    """(model name, cfg, state dict, mel, the cotangents of the outputs, the attributes that turn the gradient on)."""
    if tag in ("hifigan_s", "mb_s"):
        name, cfg, sd, mel, c = gref.chain_case(tag)
        return name, cfg, sd, mel, [c], ("parameter_grad",)
    if tag == "melgan_s":
        cfg, sd, mel, c = mref.chain_case(tag)
        return "melgan", cfg, sd, mel, [c], ("stack_grad", "parameter_grad")
    cfg, sd, mel, c_est, c_w, _ = bref.chain_case(tag)
    return "basis-melgan", cfg, sd, mel, [c_est, c_w], ("basis_grad", "parameter_grad")


TRAINING = ["hifigan_s", "mb_s", "melgan_s", "basis_s"]


@pytest.mark.parametrize("tag", TRAINING)
def test_generators_in_training(tag):
    name, cfg, sd, mel, cots, attrs = _training_case(tag)

    def fn(put):
        gen = build_generator(name, cfg)
        gen.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()})
        gen = put.module(gen)
        for a in attrs:
            setattr(gen, a, True)
        out = gen(put(mel))
        outs = list(out) if isinstance(out, (tuple, list)) else [out]
        assert len(outs) == len(cots) and all(o.requires_grad for o in outs)
        torch.autograd.backward(outs, [put(c) for c in cots])
        grads = {k: q.grad for k, q in gen.named_parameters()}
        assert any(v is not None for v in grads.values())
        return [o.detach() for o in outs], grads
    _twice(f"training/{tag}", fn)


_declare([f"training/{t}" for t in TRAINING])


def test_basis_weight_l1_term():
    cfg, sd, mel, c_est, c_w, target = bref.chain_case("basis_s")

    def fn(put):
        gen = build_generator("basis-melgan", cfg)
        gen.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()})
        gen = put.module(gen)
        gen.basis_grad = gen.parameter_grad = True
        est, weight = gen(put(mel))
        l1, average = BasisWeightL1.apply(weight, put(target))
        ((est * put(c_est)).sum() + l1).backward()
        return est.detach(), weight.detach(), l1.detach(), average.detach(), {k: q.grad for k, q in gen.named_parameters()}
    _twice("training/basis_l1", fn)


_declare(["training/basis_l1"])


# ---- e. one whole step -------------------------------------------------------------------------------------------------
FRAMES, BATCH = 140, 2                               # tests/test_gpu_train.py: the shortest the 2048-point STFT takes


@functools.lru_cache(maxsize=None)
def _discriminator_state():
    torch.manual_seed(5)
    return copy.deepcopy(Discriminator().state_dict())


def _batch(spf, seed):
    rs = _rs(seed)
    mel = rs.uniform(-4.0, 1.0, (BATCH, 80, FRAMES)).astype(np.float32)
    t = np.arange(FRAMES * spf) / 24000.0
    wav = np.stack([0.4 * np.sin(2 * np.pi * (180.0 + 70 * b) * t) + 0.2 * np.sin(2 * np.pi * (1900.0 + 300 * b) * t + 1.0)
                    for b in range(BATCH)]) + 0.02 * rs.randn(BATCH, FRAMES * spf)
    return mel, wav.astype(np.float32)


@pytest.mark.parametrize("phase", ["stft_only", "adversarial"])
def test_one_trainer_step(phase):
    state = _discriminator_state()

    def fn(put):
        g = _generator(put, "hifigan", gref.GOLDEN_CFG, seed=3, train=True)
        d = Discriminator()
        d.load_state_dict(state)
        d = put.module(d)
        opt_g, opt_d = optim.Adam(g.parameters(), lr=1e-4, eps=1e-6), optim.Adam(d.parameters(), lr=5e-5, eps=1e-6)
        trainer = Trainer(g, d, opt_g, opt_d, pqmf=None, lambda_stft=5.0, use_feature_map_loss=True,
                          discriminator_train_start_steps=1 if phase == "stft_only" else 0, grad_clip_thresh=1.0)
        mel, wav = _batch(samples_per_frame(g, None), seed=1)
        out = trainer.step(put(mel), put(wav), 1)
        assert tuple(out) == KEYS
        moments = [{k: [(o.state[p].get("exp_avg"), o.state[p].get("exp_avg_sq")) for p in m.parameters() if p in o.state]}
                   for k, m, o in (("g", g, opt_g), ("d", d, opt_d))]
        return dict(out), [p.detach() for p in g.parameters()], [p.detach() for p in d.parameters()], moments
    _twice(f"trainer/{phase}", fn)


_declare(["trainer/stft_only", "trainer/adversarial"])


# ---- f. coverage ---------------------------------------------------------------------------------------------------------
# (file under fastvocoder_amd/, enclosing function or "*") -> why no guarded case reaches the site
ALLOW = {
    ("parallel.py", "*"): "multi-process wire buffers and buckets: they exist only inside a process group, which the ddp and "
                          "multi-GPU tests start in worker processes of their own",
    ("bin/test.py", "*"): "CLI front end (host-side zeros for the bias pass); tests/test_gpu_cli.py runs it as a process",
    ("bin/synthesize.py", "*"): "CLI front end (host-side zeros for the bias pass; build_generator's basis placeholder is "
                                "reached); tests/test_gpu_cli.py runs it as a process",
}


def _allowed(site):
    rel = os.path.relpath(os.path.join(ga.ROOT, site.file), ga.PACKAGE)
    return (rel, "*") in ALLOW or (rel, site.function) in ALLOW


def test_every_allocation_site_of_the_package_was_reached():
    missing = sorted(set(ALL_CASES) - _RAN)
    if missing:
        pytest.skip(f"{len(missing)} guarded cases did not run in this session (deselected?), e.g. {missing[:3]}: "
                    "the coverage of allocation sites is checked by a run of the whole file")
    assert len(set(ALL_CASES)) == len(ALL_CASES)
    static = ga.scan_sites()
    hit = set(ga.reached(static, _REACHED))
    assert hit, "no site was recorded"
    unreached = [s for s in static if s not in hit and not _allowed(s)]
    stale = [k for k in ALLOW if not any((os.path.relpath(os.path.join(ga.ROOT, s.file), ga.PACKAGE), "*") == k
                                         or (os.path.relpath(os.path.join(ga.ROOT, s.file), ga.PACKAGE), s.function) == k for s in static)]
    print(f"guarded allocation sites: {len(hit)} of {len(static)} reached, {sum(_allowed(s) for s in static if s not in hit)} on the allow-list")
    assert not stale, f"allow-list entries that name no site: {stale}"
    assert not unreached, "allocation sites no guarded case reached:\n" + "\n".join(str(s) for s in unreached)
