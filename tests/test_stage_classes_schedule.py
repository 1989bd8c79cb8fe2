"""The block table of the 32-channel MRF stage in two block classes (csrc/mrfh_launch.hip mrf_class_plan), through the
host-only hook fv_debug_mrf_class_schedule: no GPU."""
import pytest

from fastvocoder_amd import _native

# (utterances, columns per utterance, blocks): the headline stage (batch 1, 1000 frames), the 560-frame mel whose share is one
# window, two short utterances on a few blocks, one block, three blocks
SHAPES = [(1, 120000, 256), (1, 61440, 256), (2, 1800, 7), (1, 700, 1), (1, 5000, 3)]


def _windows(cols, window, reach):
    """Whole windows the kernel runs for a run of ``cols`` columns: the first is final for window - 2 reach columns (it
    starts `reach` early and its last `reach` columns wait for the next), the rest for window - reach."""
    first, rest = window - 2 * reach, window - reach
    return 1 if cols <= first else 1 + -(-(cols - first) // rest)


def _check_plan(plan, B, T, nblk):
    W = plan["window"]
    assert plan["n_a"] + plan["n_b"] <= nblk
    assert len(plan["ranges"]) == plan["n_a"] + plan["n_b"]
    classes = [("A", plan["reach_a"], plan["cost_a"], plan["ranges"][:plan["n_a"]]),
               ("B", plan["reach_b"], plan["cost_b"], plan["ranges"][plan["n_a"]:])]
    if not plan["split"]:
        # the all-in-one form: every block runs all three ResBlocks on an equal share, which may cross utterance ends
        assert plan["n_a"] == 0 and plan["n_b"] == nblk
        classes = [("all", plan["reach_b"], plan["cost_one"], plan["ranges"])]
    worst = 0
    for name, reach, cost, ranges in classes:
        covered = [0] * (B * T)
        for lo, hi in ranges:
            assert 0 <= lo < hi <= B * T, (name, lo, hi)
            if plan["split"]:
                assert lo // T == (hi - 1) // T, f"class {name}: [{lo}, {hi}) crosses an utterance end"
            windows, a = 0, lo
            while a < hi:                       # (the all-in-one form starts a new run at an utterance end)
                end = min(hi, (a // T + 1) * T)
                windows += _windows(end - a, W, reach)
                # the whole windows cover the run: W - 2 reach, then W - reach each
                assert (W - 2 * reach) + (_windows(end - a, W, reach) - 1) * (W - reach) >= end - a
                a = end
            worst = max(worst, windows * cost)
            for c in range(lo, hi):
                covered[c] += 1
        assert all(v == 1 for v in covered), f"class {name}: a column belongs to {set(covered)} blocks"
    assert worst == plan["makespan"]
    return worst


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_every_column_once_and_no_slower_than_all_in_one(shape):
    B, T, nblk = shape
    plan = _native.mrf_class_schedule(B, T, nblk)
    _check_plan(plan, B, T, nblk)
    # the all-in-one form's makespan from the hook's own constants: equal shares of the concatenated columns
    one = 0
    for i in range(nblk):
        lo, hi = B * T * i // nblk, B * T * (i + 1) // nblk
        windows, a = 0, lo
        while a < hi:
            end = min(hi, (a // T + 1) * T)
            windows += _windows(end - a, plan["window"], 60)
            a = end
        one = max(one, windows * plan["cost_one"])
    assert one == plan["makespan_one"]
    assert plan["makespan"] <= one
    assert plan["split"] == (plan["makespan"] < one)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_forced_split(shape):
    """What fv_mrf_stage_classes_f16 launches: the split wherever each class can have a block per utterance."""
    B, T, nblk = shape
    plan = _native.mrf_class_schedule(B, T, nblk, force=True)
    assert plan["split"] == (nblk >= 2 * B)       # one block: the all-in-one form (the entry itself refuses)
    _check_plan(plan, B, T, nblk)
    if plan["split"]:
        assert plan["n_a"] >= B and plan["n_b"] >= B and (plan["reach_a"], plan["reach_b"]) == (60, 36)


def test_headline_split_is_the_issue_s():
    plan = _native.mrf_class_schedule(1, 120000, 256)
    # 3 windows per block in either class: 264 + 2 x 324 = 912 columns (class A), 312 + 2 x 348 = 1008 (class B)
    assert plan["split"] and (plan["n_a"], plan["n_b"]) == (132, 120)
    assert plan["ranges"][0] == (0, 912) and plan["ranges"][132] == (0, 1008)


def test_refusals():
    for args in [(0, 100, 4), (1, 0, 4), (1, 100, 0), (1, 100, 257), (1 << 16, 1 << 16, 4)]:
        with pytest.raises(_native.NativeError):
            _native.mrf_class_schedule(*args)
