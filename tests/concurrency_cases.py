"""The small workloads the stream tests (tests/test_gpu_streams.py) and the thread tests (tests/test_gpu_threads.py,
tests/threads_worker.py) share.  ``make(put)`` builds a FRESH module and fresh inputs through ``put`` (test_gpu_guarded._Put
or stream_tools.Staged) and returns a Case: ``forward()`` builds the graph and returns the outputs, ``backward(outs)`` runs
autograd and returns everything to compare; ``step()`` is one after the other, with the gradients cleared first, so that a
loop of steps gives the same bits every time.  Cotangents are the outputs themselves (detached): no kernel of torch's
own stands between the library's forward and its backward.

An ordinary module that tests import; it is no pytest plugin."""
import hashlib

import numpy as np
import torch

from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.discriminator import MelGANMultiScaleDiscriminator
from fastvocoder_amd.loss import MultiResolutionSTFTLoss
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict, seeded_mel, seeded_state_dict
from tests import cases
from tests import mpd_wgrad_reference as wref
from tests import test_gpu_guarded as G


class Case:
    def __init__(self, forward, backward=None, clear=()):
        self.forward, self._backward, self._clear = forward, backward, clear

    def backward(self, outs):
        return outs if self._backward is None else self._backward(outs)

    def step(self):
        for t in self._clear:
            t.grad = None
        return self.backward(self.forward())


def _tensors(o):
    return [t for _, t in G._flat(o) if torch.is_tensor(t)]


def hifigan_s(put, range_guard="lazy"):
    """``hifigan_s`` forward at 3 x 24 frames (cases.SMALL)."""
    _, name, cfg = next(c for c in cases.SMALL if c[0] == "hifigan_s")
    m = build_generator(name, cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in seeded_state_dict(name, cfg, seed=0).items()})
    m = put.module(m.eval())
    m.range_guard = range_guard
    x = put(seeded_mel(cases.SMALL_T, seed=21000 + cases.SMALL_T, batch=cases.SMALL_B))

    def forward():
        with torch.no_grad():
            return m(x)
    case = Case(forward)
    case.module = m
    return case


def hifigan_s_training(put):
    """test_gpu_guarded's ``training/hifigan_s``: forward on the parameters' graph, backward from its seeded cotangent."""
    name, cfg, sd, mel, cots, attrs = G._training_case("hifigan_s")
    gen = build_generator(name, cfg)
    gen.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()})
    gen = put.module(gen)
    for a in attrs:
        setattr(gen, a, True)
    x, cots = put(mel), [put(c) for c in cots]

    def forward():
        out = gen(x)
        return list(out) if isinstance(out, (tuple, list)) else [out]

    def backward(outs):
        torch.autograd.backward(outs, cots)
        return [o.detach() for o in outs], {k: q.grad for k, q in gen.named_parameters()}
    return Case(forward, backward, list(gen.parameters()))


def small_msd(put, T=100):
    """The small MSD (test_gpu_disc_grad.SMALL_MSD), forward plus BOTH gradients: of the input and of the parameters."""
    msd = MelGANMultiScaleDiscriminator(**G.SMALL_MSD)
    sd = seeded_discriminator_state_dict("msd", 3, **G.SMALL_MSD)
    msd.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()})
    msd = put.module(msd.eval())
    msd.differentiable = msd.parameter_grad = True
    x = put(wref.signals(3, T)[0]).requires_grad_(True)

    def forward():
        return _tensors(msd(x))

    def backward(maps):
        torch.autograd.backward(maps, [m.detach() for m in maps])
        grads = {k: q.grad for k, q in msd.named_parameters()}
        assert x.grad is not None and all(g is not None for g in grads.values())
        return [m.detach() for m in maps], x.grad, grads
    return Case(forward, backward, [x] + list(msd.parameters()))


def stft_loss(put, B=2, n=1680):
    """The differentiable multi-resolution STFT loss and its gradient (1680 samples = 7 hops of the 2048-point resolution)."""
    mr = put.module(MultiResolutionSTFTLoss())
    mr.differentiable = True
    rs = np.random.RandomState(21)
    x = put((0.3 * rs.randn(B, n)).astype(np.float32)).requires_grad_(True)
    y = put((0.3 * rs.randn(B, n)).astype(np.float32))

    def forward():
        return list(mr(x, y))

    def backward(outs):
        torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
        return [o.detach() for o in outs], x.grad
    return Case(forward, backward, [x])


def hifigan_then_split_conv(put):
    """``hifigan_s`` forward, then every launch of ``direct/conv/split_f16``: with the same shapes in every thread the schedule
    and width caches of csrc/convh_launch.hip and the LDS grants are asked for one key at once."""
    gen = hifigan_s(put)

    def forward():
        return gen.forward(), G.DIRECT["conv/split_f16"](put)
    return Case(forward)


def clone(o):
    """A copy of every tensor of a result (on the current stream): a module's next call may reuse its buffers."""
    if torch.is_tensor(o):
        return o.detach().clone()
    if isinstance(o, dict):
        return {k: clone(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [clone(v) for v in o]
    return o


def digest(o):
    """sha256 over the bytes of every tensor of a result, in order (what a child process reports instead of tensors)."""
    h = hashlib.sha256()
    for path, t in G._flat(o):
        h.update(path.encode())
        h.update(t.detach().cpu().numpy().tobytes() if torch.is_tensor(t) else repr(t).encode())
    return h.hexdigest()
