"""The two doors of every forward operator give the same launch: one direct call (fv_conv1d_fused, ...) and one run of
a one-launch plan (fv_plan_add_conv1d, ...) on the same input return the same bits and log the same kernels.

Both doors describe the op through one builder (csrc/api_internal.h build_*) and launch through the same launch
records; this is the test that they do.  A plan has one input, so every operand a twin case reads (x, x2, each member's
x, res, add1, add2) is that one tensor on both sides.  Shapes: tests/test_gpu_guarded.py's direct cases -- the smallest
at which these kernels still meet a ragged tile, a mirrored column or a single sample.  No range guard on either side.

Left to the families' own tests, because a plan cannot be given them this way: operands of another shape than the input
(the residual of a conv that changes the channel count or the length, fp32 running sums), the folded output conv of a
stage, the merged input of the transposed conv, and the one-class debug entry, which has no plan twin."""
import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.generator.pqmf import PQMF

pytestmark = pytest.mark.gpu
F32, SPLIT = _native.PAIR_F32, _native.PAIR_SPLIT_F16
ZERO, REFLECT = _native.PAD_ZERO, _native.PAD_REFLECT
IN, OUT, OUT2, TMP = _native.SLOT_IN, _native.SLOT_OUT, _native.SLOT_OUT2, _native.SLOT_TMP0
KS = (3, 7, 11)


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _randn(rs, *shape, scale=1.0):
    return _t((scale * rs.randn(*shape)).astype(np.float32))


def _conv_w(rs, cout, cin, k):
    return _randn(rs, cout, cin, k, scale=1.0 / np.sqrt(cin * k))


def _twins(direct, build, x, outputs=1):
    """direct() -> the direct call's output tensors; build(plan) adds the one-launch plan whose outputs are SLOT_OUT (and
    SLOT_OUT2).  Equal bits, equal kernel names and counts, one launch each."""
    with _native.launch_log() as dlog:
        want = direct()
    want = list(want) if isinstance(want, (tuple, list)) else [want]
    plan = _native.Plan(x.shape[1])
    build(plan)
    with _native.launch_log() as plog:
        got = plan.run(x, out2=outputs == 2)
    got = list(got) if outputs == 2 else [got]
    torch.cuda.synchronize()
    assert len(want) == len(got) == outputs
    for n, (w, g) in enumerate(zip(want, got)):
        assert w.shape == g.shape and torch.equal(w, g), f"output {n}: {(w - g).abs().max().item():.3e}"
        assert torch.isfinite(w).all()
    assert dlog.kernels == plog.kernels and sum(dlog.kernels.values()) == 1, (dlog.kernels, plog.kernels)
    return plog.kernels


@pytest.mark.parametrize("ci,co,k,dil,pad,mode,T,B", [(20, 12, 7, 3, 9, ZERO, 50, 2), (16, 16, 3, 9, 9, REFLECT, 10, 3)])
def test_fp32_conv(ci, co, k, dil, pad, mode, T, B):
    rs = np.random.RandomState(4)
    x, P, b = _randn(rs, B, ci, T), _native.pack_conv1d(_conv_w(rs, co, ci, k)), _randn(rs, co)
    same = ci == co and 2 * pad == dil * (k - 1)          # the input has the output's shape: it is the residual too
    tout = T + 2 * pad - dil * (k - 1)

    def direct():
        act = torch.empty((B, co, tout), dtype=torch.float32, device=x.device)
        return _native.conv1d_fused(x, P, b, co, k, dil=dil, pad=pad, pad_mode=mode, pre_slope=0.1, res=x if same else None,
                                    out_act=act, act_slope=0.2), act

    _twins(direct, lambda p: p.add_conv1d(IN, OUT, P, b, ci, co, k, dil=dil, pad=pad, pad_mode=mode, pre_slope=0.1,
                                          res=IN if same else _native.SLOT_NONE, y_act=OUT2, act_slope=0.2), x, 2)


def test_transposed_conv():
    rs = np.random.RandomState(5)
    ci, co, k, s, p, op, T, B = 64, 32, 7, 3, 2, 1, 6, 2
    x, P, b = _randn(rs, B, ci, T), _native.pack_conv_transpose1d(_conv_w(rs, ci, co, k), s, p), _randn(rs, co)
    _twins(lambda: _native.conv_transpose1d_fused(x, P, b, co, k, s, p, op, pre_slope=0.1),
           lambda pl: pl.add_conv_transpose1d(IN, OUT, P, b, ci, co, k, s, p, op, pre_slope=0.1), x)


def test_upsample_conv():
    rs = np.random.RandomState(6)
    ci, co, k, r, p, T, B = 20, 12, 16, 8, 7, 3, 1
    x, P, b = _randn(rs, B, ci, T), _native.pack_upsample_conv1d(_conv_w(rs, co, ci, k), r, p), _randn(rs, co)
    _twins(lambda: _native.upsample_conv1d_fused(x, P, b, co, k, r, p, pre_slope=0.1),
           lambda pl: pl.add_upsample_conv1d(IN, OUT, P, b, ci, co, k, r, p, pre_slope=0.1), x)


def test_two_source_conv():
    rs = np.random.RandomState(7)
    x, P, b = _randn(rs, 2, 16, 33), _native.pack_conv1d(_conv_w(rs, 12, 32, 1)), _randn(rs, 12)
    _twins(lambda: _native.conv1d_2src_fused(x, x, P, b, 12), lambda pl: pl.add_conv1d_2src(IN, IN, OUT, P, b, 16, 16, 12), x)


def test_split_f16_two_source_conv():
    rs = np.random.RandomState(8)
    x, b = _randn(rs, 2, 128, 37), _randn(rs, 128, scale=0.1)
    P = _native.pack_conv1x1_2src_split(_conv_w(rs, 128, 128, 1), _conv_w(rs, 128, 128, 1))
    _twins(lambda: _native.conv1x1_2src_split_f16(x, x, P, b, pre_slope=0.2, res=x),
           lambda pl: pl.add_conv1x1_2src_split_f16(IN, IN, OUT, P, b, 128, pre_slope=0.2, res=IN), x)


def test_split_f16_transposed_conv():
    rs = np.random.RandomState(9)
    ci, co, s, p, op, T, B = 64, 32, 3, 2, 1, 11, 2
    x, b = _randn(rs, B, ci, T), _randn(rs, co, scale=0.1)
    P = _native.pack_conv_transpose1d_split(_conv_w(rs, ci, co, 2 * s), s)
    _twins(lambda: _native.conv_transpose1d_split_f16(x, P, b, co, 2 * s, s, p, op, pre_slope=0.1),
           lambda pl: pl.add_conv_transpose1d_split_f16(IN, OUT, P, b, ci, co, 2 * s, s, p, op, pre_slope=0.1), x)


@pytest.mark.parametrize("c,dil,mode,T,B", [(32, 9, REFLECT, 10, 3), (64, 3, ZERO, 70, 2)])
def test_residual_stack(c, dil, mode, T, B):
    rs = np.random.RandomState(10)
    x, bd, bo = _randn(rs, B, c, T), _randn(rs, c, scale=0.1), _randn(rs, c, scale=0.1)
    P = _native.pack_residual_stack_split(_conv_w(rs, c, c, 3), _conv_w(rs, c, c, 1), _conv_w(rs, c, c, 1))
    _twins(lambda: _native.residual_stack_split_f16(x, P, bd, bo, 3, dil, 0.2, pad_mode=mode),
           lambda pl: pl.add_residual_stack_split_f16(IN, OUT, P, bd, bo, c, 3, dil, 0.2, pad_mode=mode), x)


@pytest.mark.parametrize("T,B", [(37, 2), (1, 1)])
def test_conv_post_pqmf(T, B):
    rs = np.random.RandomState(11)
    pqmf = PQMF().to(_dev())
    x, P, b = _randn(rs, B, 16, T), _native.pack_conv1d(_conv_w(rs, 4, 16, 7)), _randn(rs, 4, scale=0.1)
    h = pqmf.synthesis_filter.reshape(4, -1).contiguous().float()
    _twins(lambda: _native.conv_post_pqmf(x, P, b, pqmf.synthesis_filter, 7, 3, pre_slope=0.01),
           lambda pl: pl.add_conv_post_pqmf(IN, OUT, P, b, 16, 7, 3, h, pre_slope=0.01), x)


def test_pqmf_synthesis():
    rs = np.random.RandomState(12)
    pqmf = PQMF().to(_dev())
    x = _randn(rs, 2, 4, 61)
    h = pqmf.synthesis_filter.reshape(4, -1).contiguous().float()
    _twins(lambda: _native.pqmf_synthesis(x, pqmf.synthesis_filter, torch.empty((2, 1, 4 * 61), dtype=torch.float32, device=x.device)),
           lambda pl: pl.add_pqmf_synthesis(IN, OUT, h), x)


@pytest.mark.parametrize("c,prec,dil,T,B", [(16, F32, 3, 68, 2), (32, SPLIT, 1, 68, 3), (64, SPLIT, 5, 36, 2)])
def test_fused_pairs_of_three_members(c, prec, dil, T, B):
    """Three members, one launch.  A plan hands back two tensors: the plan runs twice with the members' outputs in
    other slots, so that every member's is seen (the launch is the same one)."""
    rs = np.random.RandomState(13)
    x = _randn(rs, B, c, T)
    w1 = [_native.pack_pair(_conv_w(rs, c, c, k), prec) for k in KS]
    w2 = [_native.pack_pair(_conv_w(rs, c, c, k), prec) for k in KS]
    b1, b2 = ([_randn(rs, c, scale=0.1) for _ in KS] for _ in range(2))
    adds = dict(add1=[x] * 3, add2=[x] * 3, out_div=3.0) if prec == SPLIT else {}          # (fp32 pairs take no addends)
    plan_adds = dict(add1=IN, add2=IN, out_div=3.0) if prec == SPLIT else {}
    want = []

    def direct():
        want[:] = _native.resblock1_fused([x] * 3, w1, w2, b1, b2, list(KS), dil, 0.1, prec=prec, **adds)
        return want[:2]

    def build(slots):
        def add(pl):
            pl.set_group(1)
            for j, k in enumerate(KS):
                pl.add_resblock_pair(IN, slots[j], w1[j], w2[j], b1[j], b2[j], c, k, dil, 0.1, prec=prec,
                                     mid=TMP + 1 + j if c >= 64 else _native.SLOT_NONE, **plan_adds)
        return add

    _twins(direct, build((OUT, OUT2, TMP)), x, 2)
    plan = _native.Plan(c)
    build((TMP, OUT, OUT2))(plan)
    with _native.launch_log() as log:
        got = plan.run(x, out2=True)
    assert torch.equal(got[0], want[1]) and torch.equal(got[1], want[2]) and sum(log.kernels.values()) == 1


def test_mrf_sum():
    rs = np.random.RandomState(14)
    c, dil, T, B = 16, 3, 68, 2
    x = _randn(rs, B, c, T)
    w1 = [_native.pack_pair(_conv_w(rs, c, c, k)) for k in KS]
    w2 = [_native.pack_pair(_conv_w(rs, c, c, k)) for k in KS]
    b1, b2 = ([_randn(rs, c, scale=0.1) for _ in KS] for _ in range(2))

    def direct():
        act = torch.empty_like(x)
        return _native.mrf_stage([x] * 3, w1, w2, b1, b2, list(KS), dil, 0.1, out_act=act, act_slope=0.1), act

    _twins(direct, lambda pl: pl.add_mrf_sum([IN] * 3, OUT, w1, w2, b1, b2, c, list(KS), dil, 0.1, y_act=OUT2, act_slope=0.1), x, 2)


def _stage_image(rs, c):
    w1 = [_conv_w(rs, c, c, KS[j]) for j in range(3) for _ in range(3)]
    w2 = [_conv_w(rs, c, c, KS[j]) for j in range(3) for _ in range(3)]
    b1, b2 = ([_randn(rs, c, scale=0.1) for _ in range(9)] for _ in range(2))
    return _native.pack_mrf_stage(w1, w2, b1, b2, KS)


@pytest.mark.parametrize("c,T,B", [(16, 67, 2), (32, 67, 2)])
def test_one_launch_stage_with_its_activated_twin(c, T, B):
    rs = np.random.RandomState(15)
    P, x = _stage_image(rs, c), _randn(rs, B, c, T)

    def direct():
        act = torch.empty_like(x)
        return _native.mrf_stage_split_f16(x, P, KS, out_act=act, act_slope=0.1), act

    _twins(direct, lambda pl: pl.add_mrf_stage(IN, OUT, P, c, KS, _native.MRF_STAGE_DILATIONS, 0.1, y_act=OUT2, act_slope=0.1), x, 2)


def test_stage_in_two_block_classes():
    rs = np.random.RandomState(16)
    P, x = _stage_image(rs, 32), _randn(rs, 1, 32, 252)
    try:
        _native.tuning_set("mrf_blocks", 2)          # two blocks: one window per class
        _twins(lambda: _native.mrf_stage_classes_f16(x, P, KS),
               lambda pl: pl.add_mrf_stage_classes(IN, OUT, OUT2, P, 32, KS, _native.MRF_STAGE_DILATIONS, 0.1), x, 2)
    finally:
        _native.tuning_set("mrf_blocks", 0)


@pytest.mark.parametrize("c,k,dil,mode,T,B", [(64, 3, 9, REFLECT, 10, 3), (128, 7, 3, ZERO, 131, 1)])
def test_wide_split_f16_convs_of_two_members(c, k, dil, mode, T, B):
    rs = np.random.RandomState(17)
    x = _randn(rs, B, c, T)
    P = [_native.pack_pair(_conv_w(rs, c, c, k), SPLIT) for _ in range(2)]
    b = [_randn(rs, c, scale=0.1) for _ in range(2)]

    def build(pl):
        pl.set_group(1)
        for j, y in enumerate((OUT, OUT2)):
            pl.add_conv1d_split_f16(IN, y, P[j], b[j], c, k, dil, pre_slope=0.1, res=IN, pad_mode=mode)

    _twins(lambda: _native.conv1d_split_f16([x] * 2, P, b, [k, k], dil, pre_slope=0.1, res=[x] * 2, pad_mode=mode), build, x, 2)
