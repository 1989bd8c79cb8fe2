"""Tile widths of the fused 128-channel pair launches (csrc/convh_launch.hip pair_width_plan, through the host-only hook
fv_debug_pair_widths): the 11-tap member runs on 64 or 80 intermediate columns, whichever the block schedule's model
finishes earlier.  No GPU: the hook touches no device."""
import pytest

from fastvocoder_amd import _native

TAPS = (11, 7, 3)
SWITCH = 4           # Tuning::sched_switch


@pytest.fixture
def tuning():
    yield _native.tuning_set
    for key, value in (("convq_nm11", -1), ("convq_cost80", -1), ("sched", 1), ("sched_switch", SWITCH)):
        _native.tuning_set(key, value)


def _tiles(T, nm, k):
    nout = nm - (k - 1)
    return (T + nout - 1) // nout


def _makespan(shares, cost):
    return max(sum(cnt * c for (lo, cnt), c in zip(sh, cost)) + SWITCH * max(0, sum(1 for lo, cnt in sh if cnt) - 1) for sh in shares)


def test_headline_launch_takes_80_columns_for_the_11_tap_member(tuning):
    """HiFi-GAN light at 1000 frames, batch 1: 8000 columns at 128 channels on 256 blocks."""
    for dil in (1, 3, 5):
        pl = _native.debug_pair_widths(128, 1, 8000, dil, TAPS, 256)
        assert pl["widths"] == [80, 64, 64]
        assert pl["items"] == [115, 138, 130] and pl["costs"] == [60, 33, 17]
        assert pl["makespan"] == 60 and pl["nblk"] == 256
    # the schedule those items and costs get: every item handed out exactly once, consecutive ranges in block order
    on, shares = _native.debug_pair_schedule(pl["items"], pl["costs"], 256, mode=0, three_members=True)
    assert on == 1 and len(shares) == 256
    for m, n in enumerate(pl["items"]):
        at = 0
        for sh in shares:
            lo, cnt = sh[m]
            if cnt:
                assert lo == at
            at += cnt
        assert at == n
    assert _makespan(shares, pl["costs"]) == 60


@pytest.mark.parametrize("T", [2000, 4000, 5600])
def test_one_tile_per_block_keeps_64_columns(T, tuning):
    """Up to one 11-tap tile per block the shorter tile finishes earlier: 49 against 60."""
    pl = _native.debug_pair_widths(128, 1, T, 3, TAPS, 256)
    assert pl["widths"] == [64, 64, 64]
    assert pl["items"] == [_tiles(T, 64, k) for k in TAPS] and pl["costs"] == [49, 33, 17]
    assert pl["makespan"] == 49


def test_forcing_64_reproduces_the_table_of_equal_widths(tuning):
    tuning("convq_nm11", 64)
    pl = _native.debug_pair_widths(128, 1, 8000, 5, TAPS, 256)
    assert pl["widths"] == [64, 64, 64] and pl["items"] == [149, 138, 130] and pl["costs"] == [49, 33, 17]
    assert pl["makespan"] == 70
    on, shares = _native.debug_pair_schedule([149, 138, 130], [49, 33, 17], 256, mode=0, three_members=True)
    assert on == 1 and _makespan(shares, [49, 33, 17]) == 70
    # two members, as the last launch of a stage has them
    pl = _native.debug_pair_widths(128, 1, 8000, 1, (11, 7), 256)
    assert pl["widths"] == [64, 64] and pl["items"] == [149, 138]


def test_forced_and_chosen_widths_do_not_share_a_cache_entry(tuning):
    """The plan is kept per shape: the key holds the forced width, so asking in any order gives each its own answer."""
    auto = _native.debug_pair_widths(128, 1, 8000, 3, TAPS, 256)
    tuning("convq_nm11", 64)
    f64 = _native.debug_pair_widths(128, 1, 8000, 3, TAPS, 256)
    tuning("convq_nm11", 80)
    f80 = _native.debug_pair_widths(128, 1, 5600, 3, TAPS, 256)
    tuning("convq_nm11", -1)
    again = _native.debug_pair_widths(128, 1, 8000, 3, TAPS, 256)
    a5600 = _native.debug_pair_widths(128, 1, 5600, 3, TAPS, 256)
    assert auto == again and auto["widths"][0] == 80
    assert f64["widths"][0] == 64 and f64["makespan"] == 70
    assert f80["widths"] == [80, 64, 64] and f80["items"][0] == _tiles(5600, 80, 11) and f80["makespan"] == 60
    assert a5600["widths"][0] == 64 and a5600["makespan"] == 49
    tuning("convq_nm11", 64)
    assert _native.debug_pair_widths(128, 1, 8000, 3, TAPS, 256) == f64


def test_width_80_needs_an_11_tap_member_and_a_block_schedule(tuning):
    assert _native.debug_pair_widths(128, 1, 8000, 1, (7, 3), 256)["widths"] == [64, 64]
    tuning("convq_nm11", 80)
    assert _native.debug_pair_widths(128, 1, 8000, 1, (7, 3), 256)["widths"] == [64, 64]
    tuning("convq_nm11", -1)
    # many items per block: pair_schedule leaves the launch to the contiguous cut, nothing to compare -- 64
    pl = _native.debug_pair_widths(128, 16, 64000, 1, TAPS, 256)
    assert pl["widths"] == [64, 64, 64] and pl["makespan"] == -1
    # a calibrated cost at which 80 columns stop paying at the headline
    tuning("convq_cost80", 71)
    assert _native.debug_pair_widths(128, 1, 8000, 1, TAPS, 256)["widths"] == [64, 64, 64]


def test_width_hook_refuses_what_the_launcher_has_no_plan_for():
    for args in ((64, 1, 8000, 1, TAPS, 256), (128, 1, 8000, 2, TAPS, 256), (128, 0, 8000, 1, TAPS, 256),
                 (128, 1, 8000, 1, (3, 7, 11), 256), (128, 1, 8000, 1, (11, 5), 256), (128, 1, 8000, 1, TAPS, 0)):
        with pytest.raises(_native.NativeError):
            _native.debug_pair_widths(*args)
