"""The 32-channel MRF stage as ONE launch of two block classes (fv_mrf_stage_classes_f16, csrc/mrfw_kernels.hpp SPLIT):
class A blocks run the 11-tap ResBlock and store r_2, class B blocks the 3- and 7-tap ones and store r_0 + r_1.  Bit for
bit against the three pair launches; block counts forced through fv_tuning_set as tests/test_gpu_stage.py does."""
import ctypes

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native

pytestmark = pytest.mark.gpu

SPLIT = _native.PAIR_SPLIT_F16
DILS = (1, 3, 5)
KS = (3, 7, 11)


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@pytest.fixture
def tuning():
    yield _native.tuning_set
    _native.tuning_set("mrf_blocks", 0)


def _stage_weights(rng, bias=True, C=32):
    """Nine pairs: index 3 j + p = pair p of ResBlock j (taps KS[j], dilation DILS[p])."""
    w1, w2, b1, b2 = [], [], [], []
    for j in range(3):
        for _ in range(3):
            k = KS[j]
            w1.append((rng.randn(C, C, k) / np.sqrt(C * k)).astype(np.float32))
            w2.append((rng.randn(C, C, k) / np.sqrt(C * k)).astype(np.float32))
            b1.append(rng.randn(C).astype(np.float32) * 0.3 if bias else None)
            b2.append(rng.randn(C).astype(np.float32) * 0.3 if bias else None)
    return w1, w2, b1, b2


def _pack(ws):
    w1, w2, b1, b2 = ws
    return _native.pack_mrf_stage([_t(w) for w in w1], [_t(w) for w in w2], [_t(b) for b in b1], [_t(b) for b in b2], list(KS))


def _pairs(x, ws, slope=0.1):
    """r_0, r_1, r_2 from three launches of fused pairs (one per pair position, three members each)."""
    w1, w2, b1, b2 = ws
    cur = [x, x, x]
    for p in range(3):
        idx = [3 * j + p for j in range(3)]
        cur = _native.resblock1_fused(cur, [_native.pack_pair(_t(w1[i]), SPLIT) for i in idx],
                                      [_native.pack_pair(_t(w2[i]), SPLIT) for i in idx], [_t(b1[i]) for i in idx],
                                      [_t(b2[i]) for i in idx], list(KS), DILS[p], slope, prec=SPLIT)
    return cur


def _check(X, P, ws, **kw):
    with _native.launch_log() as log_pairs:
        r = _pairs(X, ws)
    with _native.launch_log() as log:
        y_s, y_r2 = _native.mrf_stage_classes_f16(X, P, KS, **kw)
    # the two-class instantiation of mrfw_kernel on one side, the pair launches on the other
    assert log.kernels == {"mrfw_kernel<3, 8, 1, 3, 5, false, true>": 1}, log.kernels
    assert log_pairs.families() == {"pairh_kernel"}, log_pairs.kernels
    assert torch.equal(y_r2, r[2]), "r_2 differs from the pair launches"
    assert torch.equal(y_s, r[0] + r[1]), "r_0 + r_1 differs from the pair launches"
    return y_s, y_r2


# T, windows of the class-A / class-B block (384-column windows: a run's first gives 264 / 312 columns, further ones 324 / 348)
@pytest.mark.parametrize("T", [252, 600, 1300], ids=["1x1windows", "3x2windows", "5x4windows"])
def test_one_block_per_class(T, tuning):
    rng = np.random.RandomState(T)
    x = rng.randn(1, 32, T).astype(np.float32)
    ws = _stage_weights(rng)
    tuning("mrf_blocks", 2)
    plan = _native.mrf_class_schedule(1, T, 2, force=True)
    assert plan["split"] and (plan["n_a"], plan["n_b"]) == (1, 1)
    guard = torch.zeros(1, dtype=torch.int32, device=_dev())
    _check(_t(x), _pack(ws), ws, guard=guard)
    assert int(guard.item()) == 0


def test_runs_on_both_sides_of_an_utterance_end(tuning):
    rng = np.random.RandomState(21)
    x = rng.randn(2, 32, 1800).astype(np.float32)
    ws = _stage_weights(rng, bias=False)
    tuning("mrf_blocks", 5)
    plan = _native.mrf_class_schedule(2, 1800, 5, force=True)
    assert plan["split"] and plan["n_a"] >= 2 and plan["n_b"] >= 2
    X, P = _t(x), _pack(ws)
    y_s, y_r2 = _check(X, P, ws)
    # ... and neither the block count nor the batch changes a bit
    for blocks in (4, 16, 0):
        tuning("mrf_blocks", blocks)
        a, b = _native.mrf_stage_classes_f16(X, P, KS)
        assert torch.equal(a, y_s) and torch.equal(b, y_r2), blocks
    a, b = _native.mrf_stage_classes_f16(X[1:].contiguous(), P, KS)
    assert torch.equal(a[0], y_s[1]) and torch.equal(b[0], y_r2[1])


def test_one_block_is_refused(tuning):
    """A block's columns lie inside one utterance and a block has one class: fewer than two blocks per utterance is
    FV_ERR_UNSUPPORTED (nothing is launched; the all-in-one kernel is the form for one block)."""
    rng = np.random.RandomState(22)
    X = _t(rng.randn(1, 32, 700).astype(np.float32))
    P = _pack(_stage_weights(rng))
    tuning("mrf_blocks", 1)
    with pytest.raises(_native.NativeError):
        _native.mrf_stage_classes_f16(X, P, KS)
    tuning("mrf_blocks", 3)
    with pytest.raises(_native.NativeError):
        _native.mrf_stage_classes_f16(torch.cat([X, X]), P, KS)
    # taps in another order: r_0 + r_1 would not be the reference's first sum
    with pytest.raises(_native.NativeError):
        _native.mrf_stage_classes_f16(X, P, (11, 7, 3))


def test_history_survives_a_dirty_workspace(tuning):
    rng = np.random.RandomState(23)
    x = rng.randn(2, 32, 1800).astype(np.float32)
    ws = _stage_weights(rng)
    X, P = _t(x), _pack(ws)
    tuning("mrf_blocks", 5)
    n = _native.lib().fv_mrf_stage_workspace_bytes(32)
    work = torch.full((n // 4,), float("nan"), device=_dev())
    _check(X, P, ws, work=work)
    # a workspace that is too small: refused
    y = torch.empty_like(X)
    karr, darr = (ctypes.c_int * 3)(*KS), (ctypes.c_int * 3)(*DILS)
    rc = _native.lib().fv_mrf_stage_classes_f16(X.data_ptr(), P.data_ptr(), y.data_ptr(), torch.empty_like(X).data_ptr(), 2, 32, 1800,
                                                karr, darr, 0.1, work.data_ptr(), 1000, None, None)
    assert rc == _native.ERR_WORKSPACE


def test_guards(tuning):
    rng = np.random.RandomState(24)
    ws = _stage_weights(rng)
    P = _pack(ws)
    tuning("mrf_blocks", 5)
    guard = torch.zeros(1, dtype=torch.int32, device=_dev())
    x = rng.randn(2, 32, 900).astype(np.float32)
    big = x.copy()
    big[1, 19, 450] = 1.0e6
    y_s, y_r2 = _native.mrf_stage_classes_f16(_t(big), P, KS, guard=guard)
    assert int(guard.item()) == 1 and not bool(torch.isfinite(y_s).all() and torch.isfinite(y_r2).all())
    guard.zero_()
    nob = _stage_weights(rng, bias=False)
    _native.mrf_stage_classes_f16(_t(x * np.float32(2.0 ** -14)), _pack(nob), KS, guard=guard)
    assert int(guard.item()) == _native.GUARD_LOW
    guard.zero_()
    y_s, y_r2 = _native.mrf_stage_classes_f16(_t(np.zeros_like(x)), _pack(nob), KS, guard=guard)
    assert int(guard.item()) == 0 and float(y_s.abs().max()) == 0.0 and float(y_r2.abs().max()) == 0.0


def test_plan_op(tuning):
    rng = np.random.RandomState(25)
    x = rng.randn(2, 32, 1000).astype(np.float32)
    ws = _stage_weights(rng)
    X, P = _t(x), _pack(ws)
    plan = _native.Plan(32)
    s = _native.SLOT_TMP0
    plan.add_mrf_stage_classes(_native.SLOT_IN, _native.SLOT_OUT, s, P, 32, KS, DILS, 0.1)
    y_s, y_r2 = _native.mrf_stage_classes_f16(X, P, KS)
    assert torch.equal(plan.run(X), y_s)
    # ... and the r_2 slot: the same op with the plan's output as ITS second slot
    swapped = _native.Plan(32)
    swapped.add_mrf_stage_classes(_native.SLOT_IN, s, _native.SLOT_OUT, P, 32, KS, DILS, 0.1)
    assert torch.equal(swapped.run(X), y_r2)
    # both slots downstream, as the generators use them: the upsampler's two-tensor merge against the three pair launches' sum
    r = _pairs(X, ws)
    rng2 = np.random.RandomState(26)
    wt = _t((rng2.randn(32, 16, 4) / 8.0).astype(np.float32))
    packed = _native.pack_conv_transpose1d_split(wt, 2)
    both = _native.Plan(32)
    both.add_mrf_stage_classes(_native.SLOT_IN, s, s + 1, P, 32, KS, DILS, 0.1)
    both.add_conv_transpose1d_split_f16(s, _native.SLOT_OUT, packed, None, 32, 16, 4, 2, 1, 0, pre_slope=0.1,
                                        merge=(s + 1, _native.SLOT_NONE, 3.0))
    # (the mean on the host: numpy's float32 division is correctly rounded, as the kernels' div_exact is)
    mean = _t(((r[0] + r[1]) + r[2]).cpu().numpy() / np.float32(3.0))
    assert torch.equal(both.run(X), _native.conv_transpose1d_split_f16(mean, packed, None, 16, 4, 2, 1, 0, pre_slope=0.1))
    # two outputs in one slot: refused
    with pytest.raises(_native.NativeError):
        _native.Plan(32).add_mrf_stage_classes(_native.SLOT_IN, s, s, P, 32, KS, DILS, 0.1)


def test_one_class_alone(tuning):
    """The timing hook (fv_debug_mrf_stage_class_f16): either class's blocks of the same table alone give that class's sum."""
    rng = np.random.RandomState(27)
    X = _t(rng.randn(2, 32, 1800).astype(np.float32))
    P = _pack(_stage_weights(rng))
    tuning("mrf_blocks", 7)
    y_s, y_r2 = _native.mrf_stage_classes_f16(X, P, KS)
    assert torch.equal(_native.mrf_stage_one_class_f16(X, P, KS, "a"), y_r2)
    assert torch.equal(_native.mrf_stage_one_class_f16(X, P, KS, "b"), y_s)
