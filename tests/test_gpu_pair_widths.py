"""The fused 128-channel pair with its 11-tap member on 80-column tiles (csrc/convq2_kernels.hpp kPair128Col80, chosen by
csrc/convh_launch.hip pair_width_plan) against the same launch on 64-column tiles and against the two conv launches a
fused pair replaces: the same MFMA order per output, so every bit.  The width is forced through fv_tuning_set."""
import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict
from tests import cases

pytestmark = pytest.mark.gpu

SPLIT = _native.PAIR_SPLIT_F16
C, B = 128, 2
KS = (11, 7, 3)
# below the halo; one cold 80-column tile exactly (70 outputs) and one column either side of it; the first warm tile's end
# (70 + 80) and one column past it; many tiles
LENGTHS = (5, 69, 70, 71, 150, 151, 520)


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@pytest.fixture
def tuning():
    yield _native.tuning_set
    for key, value in (("convq_nm11", -1), ("convh_blocks", 0), ("convq_wide", 20)):
        _native.tuning_set(key, value)


_WEIGHTS = {}


def _weights():
    """Per tap count: packed conv1 / conv2 images and biases (the dilation is the launch's, not the image's)."""
    if not _WEIGHTS:
        rng = np.random.RandomState(808)
        for k in KS:
            w1 = (rng.randn(C, C, k) / np.sqrt(C * k)).astype(np.float32)
            w2 = (rng.randn(C, C, k) / np.sqrt(C * k)).astype(np.float32)
            _WEIGHTS[k] = (_native.pack_pair(_t(w1), SPLIT), _native.pack_pair(_t(w2), SPLIT),
                           _t(rng.randn(C).astype(np.float32)), _t(rng.randn(C).astype(np.float32)))
    return _WEIGHTS


_INPUTS = {}


def _inputs(T):
    """One input per member and two addends for the merged output."""
    if T not in _INPUTS:
        rng = np.random.RandomState(T)
        _INPUTS[T] = [_t(rng.randn(B, C, T).astype(np.float32)) for _ in range(5)]
    return _INPUTS[T]


def _launch(ks, T, dil, merged):
    ws, xs = _weights(), _inputs(T)
    n = len(ks)
    kw = dict(add1=[xs[3]] * n, add2=[xs[4]] + [None] * (n - 1), out_div=3.0, act_slope=0.1) if merged else {}
    return _native.resblock1_fused(xs[:n], [ws[k][0] for k in ks], [ws[k][1] for k in ks], [ws[k][2] for k in ks],
                                   [ws[k][3] for k in ks], list(ks), dil, 0.1, prec=SPLIT, **kw)


@pytest.mark.parametrize("dil", [1, 3, 5])
@pytest.mark.parametrize("ks", [(11, 7, 3), (11, 7), (11,)], ids=["three", "two", "one"])
def test_80_column_tiles_give_the_bits_of_64_column_tiles(ks, dil, tuning):
    """Every length, a full grid and three blocks (long runs of warm tiles across the utterance end), with and without the
    merged output ((x' + add1) + add2) / 3 -- add2 on the 11-tap member only, so both forms of the merge run."""
    tuning("convq_wide", 1 << 20)                    # narrow tiles only: the wide form has no 11-tap width to choose
    ws = _weights()
    for T in LENGTHS:
        xs = _inputs(T)
        outs = {}
        for nm in (64, 80):
            tuning("convq_nm11", nm)
            assert _native.debug_pair_widths(C, B, T, dil, ks, 256)["widths"][0] == nm
            for blocks in (0, 3):
                tuning("convh_blocks", blocks)
                with _native.launch_log() as log:
                    outs[nm, blocks] = _launch(ks, T, dil, False) + _launch(ks, T, dil, True)
                # the two sides are different instantiations of convq2_kernel<dilation, form>: 128 -- every member on 64 columns,
                # 130 -- the 11-tap member on 80 (csrc/convh_launch.hip launch_fused_pair)
                assert log.kernels == {f"convq2_kernel<{dil}, {128 if nm == 64 else 130}>": 2}, (T, nm, blocks, log.kernels)
        tuning("convh_blocks", 0)
        base = outs[64, 0]
        for key, ys in outs.items():
            for j, (y, yb) in enumerate(zip(ys, base)):
                assert torch.equal(y, yb), (T, key, j)
        # ... and the bits of the two conv launches (convh_kernel) the fused pair replaces
        n = len(ks)
        with _native.launch_log() as log:
            mids = _native.conv1d_split_f16(xs[:n], [ws[k][0] for k in ks], [ws[k][2] for k in ks], list(ks), dil, pre_slope=0.1)
            two = _native.conv1d_split_f16(mids, [ws[k][1] for k in ks], [ws[k][3] for k in ks], list(ks), 1, pre_slope=0.1, res=xs[:n])
        assert log.families() <= {"convh_kernel", "convs_kernel"} and sum(log.kernels.values()) == 2, log.kernels
        for j in range(n):
            assert torch.equal(outs[80, 0][j], two[j]), (T, j)
            assert bool(torch.isfinite(two[j]).all()) and float(two[j].abs().max()) > 0.5


def test_both_range_guards_fire_on_80_column_tiles(tuning):
    """An operand beyond the f16 range and a tensor below its low side, each raised by the 80-column form as by the other."""
    tuning("convq_wide", 1 << 20)
    ws = _weights()[11]
    x = _inputs(520)[0]
    xn = x / x.abs().max()
    loud = xn.clone()
    loud[1, 5, 300] = 7e4
    for nm in (64, 80):
        tuning("convq_nm11", nm)
        guard = torch.zeros(1, dtype=torch.int32, device=_dev())
        args = ([ws[0]], [ws[1]], [ws[2]], [ws[3]], [11], 3, 0.1)
        _native.resblock1_fused([xn], *args, prec=SPLIT, guard=guard)
        assert int(guard.item()) == 0
        _native.resblock1_fused([loud], *args, prec=SPLIT, guard=guard)
        assert int(guard.item()) == _native.GUARD_HIGH
        _native.resblock1_fused([xn * 2.0 ** -11], *args, prec=SPLIT, guard=guard)
        assert int(guard.item()) == _native.GUARD_HIGH | _native.GUARD_LOW


def test_hifigan_light_with_80_column_tiles_forced(tuning):
    """The whole generator through its plan: the waveform does not depend on the width, nor does the graph."""
    cfg = cases.load_conf("conf/hifigan/light.yaml")
    m = build_generator("hifigan", cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict("hifigan", cfg, seed=3).items()})
    m = m.to(_dev()).eval()
    frames = 40
    x = torch.from_numpy(seeded_mel(frames, seed=31, batch=3)).to(_dev())
    got = {}
    with torch.no_grad():
        for nm in (64, 80):
            tuning("convq_nm11", nm)
            assert _native.debug_pair_widths(C, 3, 8 * frames, 1, KS, 256)["widths"] == [nm, 64, 64]
            got[nm] = (m(x).clone(), m._plan_tag(frames), m._trunk_plan(frames).num_ops())
    assert not m.check_range()
    assert torch.equal(got[80][0], got[64][0]) and float(got[64][0].abs().max()) > 1e-3
    assert got[80][1:] == got[64][1:]
