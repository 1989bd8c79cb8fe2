"""Kernel instantiations the rest of the suite never launched (tests/kernel_census.json): each case forces
one instantiation through the public operator, proves with the launch log that exactly that kernel ran, and compares it
with the reference and at the tolerance its family already uses (the C oracle; 2e-5 of the tensor's scale for the fp32
operators, 4e-6 for split-f16).

conv_mfma_kernel: the launcher picks one of six tile shapes by per-utterance size (csrc/conv_mfma.hip prepare_conv) and
one of 23 tap / dilation / ACT / SLOW variants by the layer (csrc/conv_kernels.hpp launch_geom).  Small test shapes land
on the narrow tile shapes; `shape16` / `shape32` / `shape64` force every shape here.  Rows: 16 for the 16-row shapes, 32
for the 32-row ones, 64 for the 64-row one; 16 input channels, two utterances; two tiles of the forced shape plus a
ragged third.  The plain variants need 16-byte aligned rows (`Tin % 4 == 0`, the launcher's own condition), so their
ragged tile has 4 columns; the SLOW and ACT cases take 5 (unaligned rows) or reflection padding on aligned rows.
"""
import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from oracle import ops as oo

pytestmark = pytest.mark.gpu

# id -> (MF, WM, WN, WK, NR), rows, columns of a tile (csrc/conv_mfma.hip kShapes)
SHAPES = {0: ((16, 1, 4, 1, 2), 16, 128), 1: ((16, 1, 2, 2, 2), 16, 64), 2: ((32, 1, 4, 1, 1), 32, 128),
          3: ((32, 1, 2, 2, 1), 32, 64), 4: ((32, 1, 1, 4, 1), 32, 32), 5: ((32, 2, 2, 1, 1), 64, 64)}
CIN, BATCH = 16, 2


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _t(a):
    return None if a is None else torch.from_numpy(a).to(_dev())


def _rel(a, b):
    a = a.detach().cpu().numpy().astype(np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all()
    return float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))


class forced_shape:
    """shape16 / shape32 / shape64 = id for the block (the launcher consults the one that matches the padded row count)."""

    def __init__(self, shape):
        self.shape = shape

    def __enter__(self):
        for key in ("shape16", "shape32", "shape64"):
            _native.tuning_set(key, self.shape)

    def __exit__(self, *exc):
        for key in ("shape16", "shape32", "shape64"):
            _native.tuning_set(key, -1)
        return False


def _mfma_name(shape, kt, dil, act, slow):
    geom = ", ".join(str(v) for v in SHAPES[shape][0])
    return f"conv_mfma_kernel<{geom}, {kt}, {dil}, {'true' if act else 'false'}, {'true' if slow else 'false'}>"


def _variant(k, dil, reflect, aligned, slope):
    """The (KT, DIL, ACT, SLOW) launch_geom picks (csrc/conv_kernels.hpp)."""
    if slope != 1.0:
        return 0, 0, True, True
    if reflect or not aligned:
        if k == 3:
            return 3, dil if dil in (1, 3, 9) else 0, False, True
        if k == 7:
            return 7, 1 if dil == 1 else 0, False, True
        return 0, 0, False, True
    if k == 1:
        return 1, 1, False, False
    if k == 2:
        return (2, 1, False, False) if dil == 1 else (0, 0, False, False)
    if k in (3, 7, 11):
        return k, dil if dil in (1, 3, 5) else 0, False, False
    return 0, 0, False, False


# (k, dil, reflect, aligned, pre_slope): every variant of launch_geom.  Either trigger of the SLOW path alone: each 3- and 7-tap
# SLOW variant once with reflection padding on aligned rows and once with zero padding on unaligned rows (T % 4 != 0)
LAYERS = [(1, 1, False, True, 1.0), (2, 1, False, True, 1.0), (5, 1, False, True, 1.0), (2, 3, False, True, 1.0)] + \
         [(k, d, False, True, 1.0) for k in (3, 7, 11) for d in (1, 3, 5, 2)] + \
         [(3, d, r, r, 1.0) for d in (1, 3, 9, 2) for r in (True, False)] + \
         [(7, d, r, r, 1.0) for d in (1, 3) for r in (True, False)] + \
         [(11, 1, True, True, 1.0), (5, 2, False, False, 1.0)] + \
         [(3, 1, False, False, 0.1), (7, 3, True, True, 0.2), (1, 1, False, True, 0.0)]
assert len(set(LAYERS)) == len(LAYERS)
CONV_CASES = [(s,) + layer for s in SHAPES for layer in LAYERS]


def _case_id(c):
    s, k, d, reflect, aligned, slope = c
    return f"shape{s}-k{k}d{d}-{'reflect' if reflect else 'zero'}-{'aligned' if aligned else 'ragged'}-slope{slope}"


@pytest.mark.parametrize("case", CONV_CASES, ids=_case_id)
def test_conv_mfma_instantiation_vs_oracle(case):
    shape, k, dil, reflect, aligned, slope = case
    _, rows, cols = SHAPES[shape]
    T = 2 * cols + (4 if aligned else 5)
    pad = (k - 1) * dil // 2 if k % 2 else 1          # 'same'; the 2-tap conv grows by one column
    mode = _native.PAD_REFLECT if reflect else _native.PAD_ZERO
    rng = np.random.RandomState(1000 * shape + 100 * k + 10 * dil + 2 * reflect + aligned)
    x = rng.randn(BATCH, CIN, T).astype(np.float32)
    w = (rng.randn(rows, CIN, k) / np.sqrt(CIN * k)).astype(np.float32)
    b = rng.randn(rows).astype(np.float32)
    ref = oo.conv1d(x, w, b, dil=dil, pad=pad, pad_mode=mode, pre_slope=slope)
    res = rng.randn(*ref.shape).astype(np.float32)
    X, P, Bi, R = _t(x), _native.pack_conv1d(_t(w)), _t(b), _t(res)
    want = _mfma_name(shape, *_variant(k, dil, reflect, aligned, slope))
    with forced_shape(shape):
        with _native.launch_log() as log:
            y = _native.conv1d_fused(X, P, Bi, rows, k, dil=dil, pad=pad, pad_mode=mode, pre_slope=slope)
            twin = torch.empty_like(y)
            y2 = _native.conv1d_fused(X, P, Bi, rows, k, dil=dil, pad=pad, pad_mode=mode, pre_slope=slope, res=R,
                                      out_div=2.0, out_act=twin, act_slope=0.1)
    assert log.kernels == {want: 2}, log.kernels
    assert ref.shape[2] > 2 * cols                     # a full tile, a tile boundary and a ragged last tile
    assert _rel(y, ref) <= 2e-5
    ref2 = (ref + res) / np.float32(2.0)
    assert _rel(y2, ref2) <= 2e-5 and _rel(twin, oo.lrelu(ref2, 0.1)) <= 2e-5


@pytest.mark.parametrize("shape", [2, 3, 4, 5])
def test_conv_mfma_phase_major_transposed_conv_vs_oracle(shape):
    """The 2-tap variant as the generators use it: ConvTranspose1d(k = 2 stride) in phase-major form (a row tile holds
    one phase, so the output channels are a multiple of the tile's rows: no 16-row shape can take it)."""
    _, rows, cols = SHAPES[shape]
    s, T = 2, 2 * cols + 4
    k, pad = 2 * s, 1
    rng = np.random.RandomState(50 + shape)
    x = rng.randn(BATCH, CIN, T).astype(np.float32)
    w = (rng.randn(CIN, rows, k) / np.sqrt(CIN * 2)).astype(np.float32)
    b = rng.randn(rows).astype(np.float32)
    ref = oo.conv_transpose1d(x, w, b, s, pad, 0, pre_slope=1.0)
    X, P, Bi = _t(x), _native.pack_conv_transpose1d(_t(w), s, pad), _t(b)
    with forced_shape(shape):
        with _native.launch_log() as log:
            y = _native.conv_transpose1d_fused(X, P, Bi, rows, k, s, pad, 0)
    assert log.kernels == {_mfma_name(shape, 2, 1, False, False): 1}, log.kernels
    assert tuple(y.shape) == ref.shape and _rel(y, ref) <= 2e-5


@pytest.mark.parametrize("dil", [1, 3, 5])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_conv_group3_instantiation_vs_oracle(shape, dil):
    """The grouped launch of an MRF position (csrc/conv_mfma.hip launch_conv_group: the 11-, 7- and 3-tap convs of the three
    ResBlocks, one dilation) through a plan group, at 16 / 32 / 64 channels; a 1-tap identity conv sums the three outputs
    into the plan's output (exact copies: selection weights)."""
    geom, C, cols = SHAPES[shape]
    T = 2 * cols + 4
    ks = (11, 7, 3)
    rng = np.random.RandomState(300 + 10 * shape + dil)
    x = rng.randn(BATCH, C, T).astype(np.float32)
    ws = [(rng.randn(C, C, k) / np.sqrt(C * k)).astype(np.float32) for k in ks]
    bs = [rng.randn(C).astype(np.float32) for _ in ks]
    c11, c7, c3 = [oo.conv1d(x, w, b, dil=dil, pad=(k - 1) * dil // 2) for w, b, k in zip(ws, bs, ks)]
    plan = _native.Plan(C)
    plan.set_group(1)
    for j, k in enumerate(ks):
        plan.add_conv1d(_native.SLOT_IN, 2 + j, _native.pack_conv1d(_t(ws[j])), _t(bs[j]), C, C, k, dil=dil,
                        pad=(k - 1) * dil // 2)
    plan.set_group(0)
    eye = torch.eye(C, device=_dev()).reshape(C, C, 1).contiguous()
    plan.add_conv1d(2, _native.SLOT_OUT, _native.pack_conv1d(eye), None, C, C, 1, acc=3, acc2=4)
    X = _t(x)
    with forced_shape(shape):
        with _native.launch_log() as log:
            y = plan.run(X)
    group = f"conv_group3_kernel<{', '.join(str(v) for v in geom)}, {dil}>"
    assert log.kernels == {group: 1, _mfma_name(shape, 1, 1, False, False): 1}, log.kernels
    assert _rel(y, (c7 + c3) + c11) <= 2e-5


@pytest.mark.parametrize("dil", [1, 3, 5])
def test_fp32_mrf_stage_end_at_32_channels_is_refused(dil):
    """pair_sum_kernel<2, 1, 8, dil> -- the fp32 MRF stage end at 32 channels -- is compiled but can never be selected:
    launch_pairs (csrc/pair_launch.hip), the one place that launches it, refuses the sum form unless C = 16 (three weight
    sets must fit in LDS); fv_mrf_stage is the entry exercised here.  This is the reason behind the three excuses of tests/kernel_census.json: nothing
    is launched, and the 32-channel stage ends in three pair launches and a merge instead."""
    B, C, T, ks = 2, 32, 300, (3, 11, 7)
    rng = np.random.RandomState(3200 + dil)
    xs = [_t(rng.randn(B, C, T).astype(np.float32)) for _ in ks]
    w1s = [_native.pack_pair(_t((rng.randn(C, C, k) / np.sqrt(C * k)).astype(np.float32))) for k in ks]
    w2s = [_native.pack_pair(_t((rng.randn(C, C, k) / np.sqrt(C * k)).astype(np.float32))) for k in ks]
    bs = [_t(rng.randn(C).astype(np.float32)) for _ in ks]
    with _native.launch_log() as log:
        with pytest.raises(_native.NativeError, match="mrf sum: C = 32"):
            _native.mrf_stage(xs, w1s, w2s, bs, bs, list(ks), dil, 0.1, out_div=3.0)
    assert log.kernels == {}, log.kernels


@pytest.mark.parametrize("cin,cout,k,stride,p,H,B", [(16, 64, 5, 3, 5, 37, 2), (16, 64, 5, 3, 11, 16, 2)])
def test_period_weight_grad_bf16_on_64_row_tiles(cin, cout, k, stride, p, H, B):
    """The strided bf16 weight gradient of a period conv with 64 output channels at periods 5 and 11 (the suite ran the
    64-row tile at periods 2, 3 and 7): against the float64 closed form on bf16-rounded operands, at the kernels' floor."""
    from tests import mpd_wgrad_bf16_reference as pb
    from tests import mpd_wgrad_reference as wref
    from tests.test_gpu_generator_grad import KERNEL_RTOL
    from tests.test_gpu_mpd_wgrad import _rel as rel              # the family's measure: of the reference's largest element
    g, x = wref.kernel_inputs(cin, cout, k, stride, p, H, B)
    rounded, exact_db = pb.period_conv_weight_grad(g, x, k, stride)
    with _native.launch_log() as log:
        dw, db = _native.period_conv_weight_grad(_t(g), _t(x), k, stride, True, True, precision="bf16")
    assert f"gen_wgrad_bf16_kernel<64, false, {p}>" in log.kernels, log.kernels
    assert {n for n in log.kernels if n.startswith("gen_wgrad")} == {f"gen_wgrad_bf16_kernel<64, false, {p}>"}, log.kernels
    assert dw.shape == (cout, cin, k)
    assert rel(dw, rounded) <= KERNEL_RTOL and rel(db, exact_db) <= KERNEL_RTOL
