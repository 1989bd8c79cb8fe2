"""The child processes of tests/test_gpu_ddp.py and the case they share with it.

``python tests/ddp_worker.py adam | trainer`` runs as ONE rank with an RCCL group of its own (MASTER_ADDR / MASTER_PORT
from the environment); ``python -m torch.distributed.run --nproc-per-node 2 tests/ddp_worker.py two_ranks`` runs as two
ranks that share cuda:0 over gloo.  A mode prints ``DDP_OK <mode>`` when every assertion held; the figures it prints
before asserting are for the log."""
import copy
import datetime
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"
GROUP_TIMEOUT = datetime.timedelta(seconds=120)

# ---- the tensors of the pack and optimizer tests -----------------------------------------------------------------------
SHAPES = [(1,), (7,), (4096,), (4097,), (3, 5, 1031), (256, 128, 16)]
VIEW_ELEMENTS = 1030             # a tensor 4 bytes into its storage (parameter and gradient alike)
NO_GRAD_SHAPE = (5,)             # the last parameter: requires grad, never gets one
LR, BETAS, EPS, MAX_NORM = 1e-3, (0.9, 0.999), 1e-6, 1.0


def _offset_view(values, device):
    base = torch.zeros(values.size + 1, dtype=torch.float32, device=device)
    base[1:] = torch.from_numpy(values).to(device)
    view = base[1:]
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def case_parameters(device=DEV, seed=11):
    rs = np.random.RandomState(seed)
    out = [torch.from_numpy((0.1 * rs.randn(*s)).astype(np.float32)).to(device) for s in SHAPES]
    out.append(_offset_view((0.1 * rs.randn(VIEW_ELEMENTS)).astype(np.float32), device))
    out.append(torch.from_numpy((0.1 * rs.randn(*NO_GRAD_SHAPE)).astype(np.float32)).to(device))
    return [t.requires_grad_(True) for t in out]


def case_gradients(step, device=DEV, seed=23):
    """One gradient per parameter of ``case_parameters``: the view's 4 bytes into its storage, the last one None."""
    rs = np.random.RandomState(seed + 97 * step)
    out = [torch.from_numpy(((1.0 + step) * rs.randn(*s)).astype(np.float32)).to(device) for s in SHAPES]
    out.append(_offset_view(rs.randn(VIEW_ELEMENTS).astype(np.float32), device))
    out.append(None)
    return out


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


# ---- the models of the trainer tests -----------------------------------------------------------------------------------
FRAMES = 140
T_LR, T_LR_D, CLIP, LAMBDA_STFT = 1e-4, 5e-5, 1.0, 5.0


def _models():
    from fastvocoder_amd.bin.synthesize import build_generator
    from fastvocoder_amd.discriminator import Discriminator
    from fastvocoder_amd.synthetic import seeded_state_dict
    from tests import generator_grad_reference as gref
    g = build_generator("hifigan", gref.GOLDEN_CFG)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict("hifigan", gref.GOLDEN_CFG, seed=3).items()})
    torch.manual_seed(5)
    return g.to(DEV).train(), Discriminator().to(DEV)


def _batch(rows, spf, seed):
    """mel uniform in [-4, 1]; the target two sinusoids per row plus 0.02 noise (tests/test_gpu_train.py's)."""
    rs = np.random.RandomState(seed)
    mel = rs.uniform(-4.0, 1.0, (rows, 80, FRAMES)).astype(np.float32)
    t = np.arange(FRAMES * spf) / 24000.0
    wav = np.stack([0.4 * np.sin(2 * np.pi * (180.0 + 70 * b) * t) + 0.2 * np.sin(2 * np.pi * (1900.0 + 300 * b) * t + 1.0)
                    for b in range(rows)]) + 0.02 * rs.randn(rows, FRAMES * spf)
    return torch.from_numpy(mel).to(DEV), torch.from_numpy(wav.astype(np.float32)).to(DEV)


def _trainer(g, d, start, group):
    from fastvocoder_amd import optim
    from fastvocoder_amd.train import Trainer
    return Trainer(g, d, optim.Adam(g.parameters(), lr=T_LR, eps=1e-6), optim.Adam(d.parameters(), lr=T_LR_D, eps=1e-6),
                   lambda_stft=LAMBDA_STFT, use_feature_map_loss=True, discriminator_train_start_steps=start,
                   grad_clip_thresh=CLIP, process_group=group)


def _one_rank_group():
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, timeout=GROUP_TIMEOUT, device_id=torch.device(DEV))
    return dist.group.WORLD


# ---- mode adam: Adam.step over the bucket against Adam.step without a group ----------------------------------------------

def mode_adam():
    from fastvocoder_amd import optim
    group = _one_rank_group()
    a, b = case_parameters(), case_parameters()
    opt_a = optim.Adam(a, lr=LR, betas=BETAS, eps=EPS)
    opt_b = optim.Adam(b, lr=LR, betas=BETAS, eps=EPS)
    for step in range(3):
        for params in (a, b):
            for p, g in zip(params, case_gradients(step)):
                p.grad = g
        norm_a = opt_a.step(max_norm=MAX_NORM, process_group=group)
        norm_b = opt_b.step(max_norm=MAX_NORM)
        print(f"adam step {step}: norm {float(norm_a):.9e} / {float(norm_b):.9e}", flush=True)
        assert float(norm_a) > MAX_NORM, "the case must clip"
        assert same_bits(norm_a, norm_b), (step, float(norm_a), float(norm_b))
        flat = opt_a._bucket[1]
        offsets, total = optim.bucket_layout(a)
        assert flat.numel() == total
        for k, (p, q, off) in enumerate(zip(a, b, offsets)):
            assert same_bits(p, q), (step, k)
            # p.grad is the parameter's span of the bucket, and holds the clipped gradient
            assert p.grad.data_ptr() == flat.data_ptr() + 4 * off and p.grad.shape == p.shape, (step, k)
            assert p.grad.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr(), (step, k)
            sa = opt_a.state[p]
            assert float(sa["step"]) == step + 1
            if q.grad is None:                 # without a group the parameter is skipped; with one it sees zeros
                assert k == len(a) - 1 and len(opt_b.state[q]) == 0
                assert not bool(p.grad.any()) and not bool(sa["exp_avg"].any()) and not bool(sa["exp_avg_sq"].any())
                continue
            sb = opt_b.state[q]
            assert same_bits(p.grad, q.grad), (step, k)
            assert same_bits(sa["exp_avg"], sb["exp_avg"]) and same_bits(sa["exp_avg_sq"], sb["exp_avg_sq"]), (step, k)
    torch.cuda.synchronize()


# ---- mode trainer: two Trainer steps with a one-rank group against two without --------------------------------------------

def mode_trainer():
    from fastvocoder_amd.train import KEYS, samples_per_frame
    group = _one_rank_group()
    outs = []
    for grp in (group, None):
        g, d = _models()
        trainer = _trainer(g, d, 1, grp)                      # step 1 STFT only, step 2 adversarial
        mel, wav = _batch(2, samples_per_frame(g), seed=1)
        scalars = [trainer.step(mel, wav, s) for s in (1, 2)]
        assert all(tuple(o) == KEYS for o in scalars)
        outs.append((g, d, scalars))
    (g1, d1, s1), (g2, d2, s2) = outs
    print("trainer scalars with a group   ", s1, flush=True)
    print("trainer scalars without a group", s2, flush=True)
    assert s1 == s2
    assert s1[1]["discriminator"] > 0.0 and s1[1]["discriminator_grad_norm"] > 0.0
    for (k, p), (_, q) in zip(list(g1.named_parameters()) + list(d1.named_parameters()),
                              list(g2.named_parameters()) + list(d2.named_parameters())):
        assert same_bits(p, q), k
    fresh_g, fresh_d = _models()
    assert any(not torch.equal(p, q) for p, q in zip(g1.parameters(), fresh_g.parameters()))
    assert any(not torch.equal(p, q) for p, q in zip(d1.parameters(), fresh_d.parameters()))
    torch.cuda.synchronize()


# ---- mode two_ranks: two shards, two ranks on one GPU, against the average composed by hand -------------------------------

def _mean(a, b):
    """The mean of two device scalars as the trainer forms it: an fp32 sum, halved."""
    return float((a.detach().float() + b.detach().float()) / 2)


def _first_mismatch(named_a, named_b):
    for (k, p), (_, q) in zip(named_a, named_b):
        if not same_bits(p, q):
            return k, float((p.detach() - q.detach()).abs().max())
    return None


def _mean_grads(params, per_shard):
    for p, g0, g1 in zip(params, *per_shard):
        assert g0 is not None and g1 is not None, "every parameter gets a gradient from every shard"
        p.grad = 0.5 * g0 + 0.5 * g1


def mode_two_ranks():
    import torch.distributed as dist
    from fastvocoder_amd import optim
    from fastvocoder_amd.loss import Loss, discriminator_step_terms, generator_adversarial_terms
    from fastvocoder_amd.train import fit_estimate, samples_per_frame
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert world == 2
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=GROUP_TIMEOUT)
    group = dist.group.WORLD
    per = 2
    for phase in ("stft_only", "adversarial"):
        start = 1 if phase == "stft_only" else 0              # current_step = 1 on both sides
        g, d = _models()
        d_before = copy.deepcopy(d.state_dict())
        spf = samples_per_frame(g)
        mel, wav = _batch(per * world, spf, seed=1)           # the whole global batch, on every rank
        lo = rank * per
        trainer = _trainer(g, d, start, group)
        out = trainer.step(mel[lo:lo + per].contiguous(), wav[lo:lo + per].contiguous(), 1)

        # ---- the oracle: both shards by hand in this process, the gradients averaged with torch
        g2, d2 = _models()
        g2.parameter_grad = True
        loss = Loss().to(DEV)
        loss.differentiable = True
        gp, dp = list(g2.parameters()), list(d2.parameters())
        grads, seen = [], []
        for shard in range(world):
            m, w = mel[shard * per:(shard + 1) * per].contiguous(), wav[shard * per:(shard + 1) * per].contiguous()
            for p in gp + dp:
                p.grad = None
            est = fit_estimate(g2(m), w.shape[1])
            stft, _ = loss(est, w)
            total = LAMBDA_STFT * stft
            adv = fm = torch.zeros((), device=DEV)
            if phase == "adversarial":
                t = generator_adversarial_terms(d2, est.unsqueeze(1), w.unsqueeze(1))
                adv, fm = t["adversarial"], t["feature_map"]
                total = total + 1.0 * adv + 1.0 * fm
            total.backward()
            assert all(p.grad is None for p in dp)
            grads.append([p.grad for p in gp])
            seen.append(dict(stft=stft, total=total, adversarial=adv, feature_map=fm))
        _mean_grads(gp, grads)
        hand = [p.grad.clone() for p in gp]
        norm2 = optim.Adam(gp, lr=T_LR, eps=1e-6).step(max_norm=CLIP)
        want = {k: _mean(seen[0][k], seen[1][k]) for k in seen[0]}
        want["grad_norm"] = float(norm2)
        print(f"rank {rank} {phase}: generator " + ", ".join(f"{k} {out[k]!r} / {want[k]!r}" for k in want), flush=True)
        bad = _first_mismatch(g.named_parameters(), g2.named_parameters())
        if bad is not None:                    # which stage differs: the bucket after the collective, or the update
            coef = min(1.0, CLIP / (out["grad_norm"] + 1e-6))
            stage = _first_mismatch([(k, p.grad) for k, p in g.named_parameters()],
                                    [(k, h * coef) for (k, _), h in zip(g2.named_parameters(), hand)])
            print(f"rank {rank} {phase}: generator parameters differ first at {bad}; averaged clipped gradient vs hand "
                  f"average times the factor: {stage}", flush=True)
        assert bad is None, bad
        for k in want:
            assert out[k] == want[k], (phase, k, out[k], want[k])

        if phase == "stft_only":
            assert out["adversarial"] == out["feature_map"] == out["discriminator"] == 0.0
            assert out["discriminator_grad_norm"] == 0.0
            for k, v in d.state_dict().items():
                assert torch.equal(v, d_before[k]), k
        else:
            # ---- the discriminator's half, on the generator both sides left (g2 has g's bits)
            dgrads, dlosses = [], []
            for shard in range(world):
                m, w = mel[shard * per:(shard + 1) * per].contiguous(), wav[shard * per:(shard + 1) * per].contiguous()
                for p in dp:
                    p.grad = None
                with torch.no_grad():
                    est_d = fit_estimate(g2(m), w.shape[1])
                d_loss = discriminator_step_terms(d2, est_d.unsqueeze(1), w.unsqueeze(1), stft_grad=True)["discriminator"]
                d_loss.backward()
                dgrads.append([p.grad for p in dp])
                dlosses.append(d_loss)
            _mean_grads(dp, dgrads)
            dnorm2 = optim.Adam(dp, lr=T_LR_D, eps=1e-6).step(max_norm=CLIP)
            want_d = _mean(dlosses[0], dlosses[1])
            print(f"rank {rank} {phase}: discriminator loss {out['discriminator']!r} / {want_d!r}, norm "
                  f"{out['discriminator_grad_norm']!r} / {float(dnorm2)!r}", flush=True)
            bad = _first_mismatch(d.named_parameters(), d2.named_parameters())
            assert bad is None, bad
            assert out["discriminator"] == want_d and out["discriminator_grad_norm"] == float(dnorm2)
            assert out["adversarial"] > 0.0 and out["feature_map"] > 0.0 and out["discriminator"] > 0.0
            assert any(not torch.equal(v, d_before[k]) for k, v in d.state_dict().items())

        # ---- the two ranks hold the same bits: a float64 checksum per tensor, rank 1's to rank 0
        sums = torch.stack([p.detach().double().sum() for p in list(g.parameters()) + list(d.parameters())]).cpu()
        got = [torch.empty_like(sums) for _ in range(world)] if rank == 0 else None
        dist.gather(sums, gather_list=got, dst=0, group=group)
        if rank == 0:
            assert torch.equal(got[0], got[1]), int((got[0] != got[1]).sum())
        dist.barrier()
    torch.cuda.synchronize()


if __name__ == "__main__":
    mode = sys.argv[1]
    try:
        {"adam": mode_adam, "trainer": mode_trainer, "two_ranks": mode_two_ranks}[mode]()
        print(f"DDP_OK {mode}", flush=True)
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
