"""How a call reaches its plan (engine.NativeModule._resolve / _plan): the batch is an argument of the policy, a call never
sees an earlier call's batch, and the shape-dependent choice is evaluated once per plan build.  HiFi-GAN light, seeded
weights, 140 frames -- the smallest round length at which the batch flips the 32-channel stage's form
(tests/test_stage_form_policy.py works the arithmetic by hand) -- and one seeded mel of batch 5."""
import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.generator.engine import PlanBuilder
from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict
from oracle import torch_port
from tests import accuracy_budget as ab
from tests import cases

pytestmark = pytest.mark.gpu

FRAMES = 140
CFG = cases.load_conf("conf/hifigan/light.yaml")


def _model():
    m = build_generator("hifigan", CFG)
    sd = seeded_state_dict("hifigan", CFG, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(torch.device("cuda:0")).eval(), sd


@pytest.fixture(scope="module")
def mel():
    return seeded_mel(FRAMES, seed=71, batch=5)


@pytest.fixture(scope="module")
def ports(mel):
    """(fp32 ATen port, float64 port) of the whole batch, computed once; rows of a batch never mix."""
    sd = seeded_state_dict("hifigan", CFG, seed=0)
    return (torch_port.forward("hifigan", mel, sd, CFG).numpy(), torch_port.forward("hifigan", mel, sd, CFG, dtype=torch.float64))


def _counted(fn):
    """(fn(), launches it issued)."""
    torch.cuda.synchronize()
    _native.profile_collect(-1)
    _native.profile_enable(True)
    with torch.no_grad():
        out = fn()
    torch.cuda.synchronize()
    _native.profile_enable(False)
    return out, int(_native.profile_collect(-1)["launches"])


def _names(m, kind):
    return sorted(name for name, _ in m._fv_plans if name.startswith(kind))


def test_the_batch_picks_the_variant_on_one_module(mel, ports):
    m, _ = _model()
    m.merge_in_upsampler = False
    x = torch.from_numpy(mel).to("cuda:0")
    assert [m._plan_tag(FRAMES, b) for b in (1, 2, 3, 4, 5)] == ["fffs", "fffs", "fffs", "ffss", "fffs"]
    outs, ns = [], []
    for rows in (4, 1, 4, 5):
        out, n = _counted(lambda: m(x[:rows].contiguous()).clone())
        assert m._plan_tag(FRAMES) == m._plan_tag(FRAMES, rows)          # (without a batch: this call's)
        ab.check(out, ports[0][:rows], ports[1][:rows], f"batch {rows}: {n} launches")
        outs.append(out)
        ns.append(n)
    assert ns[0] < ns[1] and ns[2] < ns[1], ns                           # one launch for the 32-channel stage, not three
    assert ns[0] == ns[2] and torch.equal(outs[0], outs[2])
    assert all(torch.equal(o[0], outs[0][0]) for o in outs)
    assert _names(m, "trunk") == ["trunkfffs", "trunkffss"]
    assert not m.check_range()


def test_no_stale_batch(mel):
    m, _ = _model()
    m.merge_in_upsampler = False
    fresh, _ = _model()
    fresh.merge_in_upsampler = False
    x = torch.from_numpy(mel).to("cuda:0")
    one = np.ascontiguousarray(mel[0].T)                                  # [T, 80]
    with torch.no_grad():
        want_est, want_rem = fresh.inference_minus(one, torch.zeros(FRAMES * 240))
        m(x[:4].contiguous())
        est, rem = m.inference_minus(one, torch.zeros(FRAMES * 240))
    assert _names(m, "minus") == ["minusfffs"] == _names(fresh, "minus")   # batch 1's; batch 4's would be "minusffss"
    assert _names(m, "trunk") == ["trunkffss"]
    assert torch.equal(est, want_est) and torch.equal(rem, want_rem) and torch.equal(est, rem)
    assert not m.check_range()


def test_one_evaluation_per_plan_build(mel, monkeypatch):
    m, _ = _model()
    x = torch.from_numpy(mel[:2]).to("cuda:0")
    count = {"flags": 0, "builds": 0}
    flags, finalize = m._fused_flags, PlanBuilder.finalize

    def counting_flags(T, B):
        count["flags"] += 1
        return flags(T, B)

    def counting_finalize(self):
        count["builds"] += 1
        return finalize(self)
    monkeypatch.setattr(m, "_fused_flags", counting_flags)
    monkeypatch.setattr(PlanBuilder, "finalize", counting_finalize)

    def forward():
        before = dict(count)
        with torch.no_grad():
            out = m(x).clone()
        return out, count["flags"] - before["flags"], count["builds"] - before["builds"]
    cold, nf, nb = forward()
    assert nb >= 1 and nf == nb, (nf, nb)           # (a weight beyond the f16 range would make it two attempts: two and two)
    assert m._fv_policy()[0] == "split" and nb == 1
    warm, nf, nb = forward()
    assert (nf, nb) == (0, 0) and torch.equal(warm, cold)
    m.fuse_stage = False
    plain, nf, nb = forward()
    assert nb == 1 and nf == 1 and torch.equal(plain, cold)
    m.fuse_stage = True
    back, nf, nb = forward()
    assert nb == 0 and torch.equal(back, cold)
    assert not m.check_range()
