"""Behind the 32-channel MRF stage in two block classes (tests/test_gpu_stage_classes.py): the upsamplers' merge of TWO
tensors -- ((r_0 + r_1) + r_2) / 3 from s = r_0 + r_1 and r_2 -- and HiFi-GAN light with that form of the stage forced,
bit for bit against the three-tensor merge and the pair launches."""
import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict
from tests import cases

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def tuning():
    yield _native.tuning_set
    for k, v in {"convt_lean": 50, "convt_rows64": -1}.items():
        _native.tuning_set(k, v)


_MERGE_INPUTS = {}      # (cin, T) -> (x, 1-tap conv images): shared by the cases of one shape


def _merge_inputs(cin, T):
    if (cin, T) not in _MERGE_INPUTS:
        rng = np.random.RandomState(1000 * cin + T)
        x = torch.from_numpy(rng.randn(2, cin, T).astype(np.float32)).to(_dev())
        ws = [_native.pack_conv1d(torch.from_numpy((rng.randn(cin, cin, 1) / np.sqrt(cin)).astype(np.float32)).to(_dev()))
              for _ in range(2)]
        _MERGE_INPUTS[cin, T] = (x, ws)
    return _MERGE_INPUTS[cin, T]


# the kernels behind fv_plan_set_input_merge: the 32 -> 16 x 2 kernel of its own (convtn), the lean kernel (convtl) and, with
# convt_lean = 0, the general 64-row one (convh_kernels.hpp convt_kernel)
@pytest.mark.parametrize("lean", [50, 0], ids=["lean", "general"])
@pytest.mark.parametrize("T", [96, 1000])
@pytest.mark.parametrize("cin,cout,stride", [(32, 16, 2), (32, 16, 3), (64, 32, 2), (64, 32, 3)],
                         ids=["32to16x2", "32to16x3", "64to32x2", "64to32x3"])
def test_two_tensor_merge_equals_three_tensor_merge(cin, cout, stride, T, lean, tuning):
    """r_0 = x, r_1 = W1 x, r_2 = W2 x (1-tap convs inside the plan); s = W1 x + x is the same conv with x as its residual,
    which is fl(r_1 + r_0) -- checked first.  Then convT(((r_0 + r_1) + r_2) / 3) == convT((s + r_2) / 3), every bit."""
    tuning("convt_lean", lean)
    x, (w1, w2) = _merge_inputs(cin, T)
    IN, OUT, A, B, S = _native.SLOT_IN, _native.SLOT_OUT, _native.SLOT_TMP0, _native.SLOT_TMP0 + 1, _native.SLOT_TMP0 + 2
    p1 = _native.Plan(cin)
    p1.add_conv1d(IN, OUT, w1, None, cin, cin, 1)
    ps = _native.Plan(cin)
    ps.add_conv1d(IN, OUT, w1, None, cin, cin, 1, res=IN)
    assert torch.equal(ps.run(x), p1.run(x) + x), "the test's premise: a conv's residual is added to its rounded result"
    rng = np.random.RandomState(stride)
    k = 2 * stride
    wt = torch.from_numpy((rng.randn(cin, cout, k) / np.sqrt(cin * 2)).astype(np.float32)).to(_dev())
    bias = torch.from_numpy(rng.randn(cout).astype(np.float32) * 0.2).to(_dev())
    packed = _native.pack_conv_transpose1d_split(wt, stride)
    three = _native.Plan(cin)
    three.add_conv1d(IN, A, w1, None, cin, cin, 1)
    three.add_conv1d(IN, B, w2, None, cin, cin, 1)
    three.add_conv_transpose1d_split_f16(IN, OUT, packed, bias, cin, cout, k, stride, 1, 0, pre_slope=0.1, merge=(A, B, 3.0))
    two = _native.Plan(cin)
    two.add_conv1d(IN, S, w1, None, cin, cin, 1, res=IN)
    two.add_conv1d(IN, B, w2, None, cin, cin, 1)
    two.add_conv_transpose1d_split_f16(S, OUT, packed, bias, cin, cout, k, stride, 1, 0, pre_slope=0.1,
                                       merge=(B, _native.SLOT_NONE, 3.0))
    want, got = three.run(x), two.run(x)
    assert want.shape == (2, cout, (T - 1) * stride - 2 + k)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0.1
    assert torch.equal(got, want)


def _model(fuse_stage):
    cfg = cases.load_conf("conf/hifigan/light.yaml")
    m = build_generator("hifigan", cfg)
    sd = seeded_state_dict("hifigan", cfg, seed=3)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(_dev()).eval()
    m.fuse_stage = fuse_stage
    return m


@pytest.fixture(scope="module")
def models():
    return _model((16, "32c")), _model((16,))


@pytest.mark.parametrize("frames", [16, 40])
def test_hifigan_light_with_the_two_class_stage_forced(frames, models):
    """The 32-channel stage as one launch of two block classes + the two-tensor merge in the last upsampler, against the
    three pair launches + the three-tensor merge: the plan op (a batch and a single utterance) and the chunked runner."""
    split, pairs = models
    assert split._plan_tag(frames) == "ffcs" and pairs._plan_tag(frames) == "fffs"      # (what the plan cache keys on)
    x = torch.from_numpy(seeded_mel(frames, seed=31, batch=3)).to(_dev())

    def launches(m, v):
        torch.cuda.synchronize()
        _native.profile_collect(-1)
        _native.profile_enable(True)
        y = m(v).clone()
        torch.cuda.synchronize()
        _native.profile_enable(False)
        return y, int(_native.profile_collect(-1)["launches"])

    with torch.no_grad():
        split(x), pairs(x)
        with _native.launch_log() as log_split:
            a, n_split = launches(split, x)
        with _native.launch_log() as log_pairs:
            b, n_pairs = launches(pairs, x)
        assert torch.equal(a, b)
        # the two sides differ by the kernel the test is about: the two-class instantiation of mrfw_kernel against the
        # 32-channel pair launches, and no all-in-one stage kernel on either side
        assert "mrfw_kernel<3, 8, 1, 3, 5, false, true>" in log_split.kernels and "mrfw_kernel" not in log_pairs.families()
        assert {k for k in log_split.kernels if k.startswith("mrfw_kernel")} == {"mrfw_kernel<3, 8, 1, 3, 5, false, true>"}
        assert any(k.startswith("pairh_kernel<2,") for k in log_pairs.kernels) and \
            not any(k.startswith("pairh_kernel<2,") for k in log_split.kernels), (log_split.kernels, log_pairs.kernels)
        assert n_split == n_pairs - 2, (n_split, n_pairs)         # three launches of fused pairs -> one
        one = x[1:2].contiguous()
        assert torch.equal(split(one), pairs(one)) and torch.equal(split(one)[0], a[1])
        mel = seeded_mel(frames, seed=32)
        whole = pairs.inference(mel)
        assert torch.equal(split.inference(mel), whole)
        for m in (split, pairs):
            m.max_frames_per_run = 11
        try:
            got, want = split.inference(mel), pairs.inference(mel)
        finally:
            for m in (split, pairs):
                m.max_frames_per_run = type(m).max_frames_per_run
        assert torch.equal(got, want)
    assert not split.check_range() and not pairs.check_range()
