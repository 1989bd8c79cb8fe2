"""hifigan.stage32_form: which of its three forms the 32-channel MRF stage takes, from the launcher's own window arithmetic
(the host-only hook fv_debug_mrf_class_schedule).  No GPU."""
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.generator import hifigan
from fastvocoder_amd.generator.engine import PlanBuilder
from fastvocoder_amd.generator.hifigan import stage32_form, stage32_windows_fit
from tests import cases


def test_forms_at_the_measured_shapes():
    # HiFi-GAN light, 120 samples per frame at 32 channels, 256 CUs (tools/stage_policy_bench.py)
    assert stage32_form(1, 120 * 1000, 256) == "c"        # the headline: 132 + 120 blocks of three windows
    assert stage32_form(1, 120 * 560, 256) == "s"         # one window per block covers the share: nothing to split
    assert stage32_form(1, 120 * 700, 256) == "c"
    for frames in (500, 560, 700, 1000):
        assert stage32_form(4, 120 * frames, 256) == "c"
    # short inputs: a launch of pairs costs less than one window
    for frames in (9, 16, 40, 125):
        assert stage32_form(1, 120 * frames, 256) == "pairs"
        assert stage32_form(3, 120 * frames, 256) in ("pairs", "s")


def test_the_classes_only_replace_a_slower_form():
    for batch in (1, 2, 4, 7):
        for t in range(120 * 8, 120 * 1300, 120 * 37):
            form = stage32_form(batch, t, 256)
            base = "s" if stage32_windows_fit(batch * t, 256) else "pairs"
            assert form in (base, "c")
            if form == "c":
                plan = _native.mrf_class_schedule(batch, t, min(256, -(-batch * t // 128)))
                assert plan["split"] and plan["makespan"] < plan["makespan_one"]
    assert stage32_form(1, 0, 256) == "pairs" and stage32_form(300, 128, 256) in ("pairs", "s")


def _host_model(conf, monkeypatch):
    """The generator on the host, its device questions answered for a 256-CU GPU: the policy is host arithmetic."""
    m = build_generator("hifigan", cases.load_conf(conf)).eval()
    dev = torch.device("cuda:0")
    monkeypatch.setattr(m, "_device", lambda: dev)
    monkeypatch.setitem(hifigan._CU_COUNT, dev, 256)
    return m


@pytest.mark.parametrize("batch", [4, 16, 64])
@pytest.mark.parametrize("frames", [250, 1000])
def test_a_last_32_channel_stage_keeps_the_all_in_one_kernel(batch, frames, monkeypatch):
    """HiFi-GAN large ends in its 32-channel stage (240 samples per frame): no upsampler behind it merges two tensors, so the
    two classes do not exist there -- the stage stays ONE all-in-one launch with conv_post folded into it wherever the
    window rule picks that, whatever the classes' estimate says."""
    m = _host_model("conf/hifigan/large.yaml", monkeypatch)
    last = m.num_upsamples - 1
    assert m.resblocks[last * m.num_kernels].channels == 32
    assert not m._stage_classes_possible(last, "split")
    flags = m._fused_flags(frames, batch)
    assert "c" not in flags
    assert flags[-1] == ("s" if stage32_windows_fit(batch * 240 * frames, 256) else True)
    # (the case the estimate alone would have moved to the classes: all-in-one by the window rule, classes estimated lower)
    if (batch, frames) in ((4, 1000), (16, 1000), (64, 1000), (16, 250)):
        assert flags[-1] == "s" and stage32_form(batch, 240 * frames, 256) == "c"
        assert m._fold_post(PlanBuilder(80), flags)
    assert m._flag_tag(frames, batch) == m._plan_tag(frames, batch)


def test_light_s_32_channel_stage_can_run_in_two_classes(monkeypatch):
    m = _host_model("conf/hifigan/light.yaml", monkeypatch)
    assert m._stage_classes_possible(2, "split") and not m._stage_classes_possible(3, "split")
    assert not m._stage_classes_possible(2, "f32")
    assert m._plan_tag(1000, 1) == "ffcs" and m._plan_tag(560, 1) == "ffss" and m._plan_tag(125, 1) == "fffs"
    m.merge_in_upsampler = False                      # nothing behind the stage merges: the window rule alone
    assert m._plan_tag(1000, 1) == "fffs" and m._plan_tag(560, 1) == "ffss"
    m.merge_in_upsampler = True
    m.fuse_stage = (16, "32c")
    assert m._plan_tag(40, 1) == "ffcs" and m._flag_tag(40, 1) == "fffs"
    m.merge_in_upsampler = False
    assert m._plan_tag(40, 1) == "fffs"
    for bad in ((16, "16c"), ("64c",), (16, 32, "c")):
        m.fuse_stage = bad
        with pytest.raises(_native.NativeError):
            m._fused_flags(40, 1)


def test_the_batch_is_an_argument_of_the_policy(monkeypatch):
    """HiFi-GAN light without the merging upsampler (the window rule alone), 140 frames: the 32-channel stage has 16 800
    columns per utterance, and of the batches 1 .. 5 only batch 4 gives every block a share -- 263 columns -- above
    0.65 x 384 = 249.6 (stage32_windows_fit, worked by hand).  140 frames is the smallest round length at which the batch
    flips the form.  The batch is an argument: the answers do not depend on the order of the questions."""
    m = _host_model("conf/hifigan/light.yaml", monkeypatch)
    m.merge_in_upsampler = False
    want = dict(zip((1, 2, 3, 4, 5), ["fffs", "fffs", "fffs", "ffss", "fffs"]))
    assert [m._plan_tag(140, b) for b in (1, 2, 3, 4, 5)] == list(want.values())
    for order in ((5, 4, 3, 2, 1), (4, 1, 4, 5, 2, 3), (1, 4, 4, 1)):
        assert [m._plan_tag(140, b) for b in order] == [want[b] for b in order]
    assert [str(m._fused_flags(140, b)) for b in (4, 1)] == ["ffss", "fffs"]
    assert m._plan_tag(140) == "fffs"                  # without a batch: the most recent call's, 1 before any call
