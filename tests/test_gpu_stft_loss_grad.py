"""GPU tests of the gradient of the multi-resolution STFT loss (csrc/stft_loss_grad.hip, fv_stft_distance_grad;
fastvocoder_amd.loss with ``differentiable`` set) against the float64 oracle tests/stft_loss_grad_reference.py and
the reference's own float64 autograd values (tests/golden/stft_loss_grad.npz)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fastvocoder_amd.generator.pqmf import PQMF
from fastvocoder_amd.loss import Loss, MultiResolutionSTFTLoss, STFTLoss, stft
from tests import cases
from tests import stft_loss_grad_reference as gref
from tests import stft_loss_reference as ref
from tests import stft_reference
from tests import stream_tools
from tests.test_gpu_stft_loss import _pairs

pytestmark = pytest.mark.gpu

# Per row, against the float64 oracle: relative L2 error, and max error over the row's peak, of the gradients of sc,
# of mag and of Loss: (sc L2, sc peak, mag L2, mag peak, Loss L2, Loss peak).  Each figure is 10 x the smaller of the
# error measured on MI355X for the device path and for the float32 eager torch.stft chain on the same inputs
# (DESIGN.md section 6.12 lists both): the project's margin of about 10, capped so that no bound exceeds 10 x the
# eager chain's own error.  The mag gradient is discontinuous where X crosses Y or the 1e-7 clamp: the frames in which
# the device puts a bin on the other side than float64 are excluded from every comparison (flipped_frames, at most
# MAX_EXCLUDED_FRAMES of them, for the device path and the eager chain alike).  What remains still depends on how
# close the signal's bins sit to those jumps, which is why the bounds are per case.
PAIR_BOUNDS = {
    "noise": (1.5e-06, 2.3e-06, 7.0e-03, 7.3e-03, 6.9e-03, 7.2e-03),
    "demo": (2.7e-06, 4.3e-06, 1.5e-03, 1.5e-03, 1.5e-03, 1.5e-03),
    # the clamp-sensitive pairs
    "sine": (6.3e-07, 2.0e-06, 2.9e-03, 5.1e-03, 2.9e-03, 5.1e-03),
    "silent_target": (6.3e-07, 9.6e-07, 1.4e-03, 1.3e-03, 8.3e-07, 1.9e-06),
    "quiet": (7.1e-06, 5.0e-06, 2.0e-06, 2.3e-06, 4.8e-06, 3.6e-06),
}
LENGTH_BOUNDS = {
    "B1_n1025": (1.3e-06, 1.3e-06, 5.6e-04, 3.8e-04, 5.6e-04, 3.8e-04),
    "B3_n1025": (1.3e-06, 1.5e-06, 4.9e-03, 4.0e-03, 4.9e-03, 4.0e-03),
    "B1_n5003": (1.7e-06, 1.8e-06, 2.9e-03, 1.8e-03, 2.8e-03, 1.8e-03),
    "B2_n24119": (1.6e-06, 1.9e-06, 3.2e-04, 3.2e-04, 2.8e-04, 3.2e-04),
    "B3_n1026": (1.3e-06, 1.7e-06, 6.0e-03, 3.7e-03, 6.0e-03, 3.7e-03),
}
# single resolutions and odd geometries: the tightest of the length cases; the reference's golden values (broadband
# signals, as "noise" and "demo"): the looser of those two pairs
SINGLE_BOUNDS = LENGTH_BOUNDS["B1_n1025"]
GOLDEN_BOUNDS = tuple(max(a, b) for a, b in zip(PAIR_BOUNDS["noise"], PAIR_BOUNDS["demo"]))


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def _mr():
    mr = MultiResolutionSTFTLoss().to(_dev())
    mr.differentiable = True
    return mr


def _loss():
    m = Loss().to(_dev())
    m.differentiable = True
    return m


def _grad(fn, x32):
    """d fn(x) / dx as float64 numpy, x a fresh leaf on the device"""
    x = _t(x32).requires_grad_(True)
    out = fn(x)
    assert out.grad_fn is not None
    out.backward()
    assert x.grad is not None and x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    return x.grad.cpu().numpy().astype(np.float64)


def _errors(got, want, keep=None):
    """worst over the rows: (relative L2 error, max error over the row's peak); keep: the samples [rows, n] compared"""
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    keep = np.ones(want.shape, bool) if keep is None else keep.reshape(want.shape)
    diff, want = np.where(keep, got - want, 0.0), np.where(keep, want, 0.0)
    l2 = np.linalg.norm(diff, axis=1) / np.linalg.norm(want, axis=1)
    peak = np.abs(diff).max(axis=1) / np.abs(want).max(axis=1)
    return float(l2.max()), float(peak.max())


MAX_EXCLUDED_FRAMES = 0.01


def flipped_frames(x32, y32):
    """(keep [B, n], share): the mag gradient jumps where a bin of x crosses the 1e-7 clamp or X crosses Y, so a bin
    that the device's float32 spectrum puts on the other side than float64 is not a matter of accuracy.  The device's
    decisions are read from its own magnitudes (``stft``: the gradient kernel forms every bin with the same
    arithmetic); the frames that hold such a bin are excluded from the comparison, i.e. the samples under their
    windows, and ``share`` is their part of all frames."""
    B, n = x32.shape
    keep = np.ones((B, n), bool)
    clamp = np.sqrt(np.float32(1e-7))
    flagged = total = 0
    for nf, hop, wl in ref.RESOLUTIONS:
        Xd = stft(_t(x32), nf, hop, wl, "hann_window").cpu().numpy()
        Yd = stft(_t(y32), nf, hop, wl, "hann_window").cpu().numpy()
        sx = stft_reference.stft(x32.astype(np.float64), nf, hop, wl)
        sy = stft_reference.stft(y32.astype(np.float64), nf, hop, wl)
        px, py = sx.real ** 2 + sx.imag ** 2, sy.real ** 2 + sy.imag ** 2
        X, Y = np.sqrt(np.maximum(px, 1e-7)), np.sqrt(np.maximum(py, 1e-7))
        # sqrtf may round a power just above the clamp onto the clamp's root: such a bin counts as flipped too
        flip = ((Xd > clamp) != (px > 1e-7)) | ((Xd == clamp) & (px > 0.9999e-7)) | (np.sign(Yd - Xd) != np.sign(Y - X))
        frames = flip.any(axis=2)                                 # [B, T]
        flagged, total = flagged + int(frames.sum()), total + frames.size
        src = gref._reflect_source(n, nf // 2)
        lpad = (nf - wl) // 2
        for b, t in zip(*np.nonzero(frames)):
            keep[b, src[t * hop + lpad:t * hop + lpad + wl]] = False
    return keep, flagged / total


def measure_pair(x, y):
    """{term: (l2, peak)} of the device gradients of sc, mag and Loss against the oracle for one pair, the frames of
    ``flipped_frames`` excluded, and their share"""
    x32, y32 = x.astype(np.float32), y.astype(np.float32)
    yt = _t(y32)
    want_sc, want_mag = gref.multi_resolution_stft_loss(x32.astype(np.float64), y32.astype(np.float64))
    keep, share = flipped_frames(x32, y32)
    mr, loss = _mr(), _loss()
    return {"sc": _errors(_grad(lambda v: mr(v, yt)[0], x32), want_sc, keep),
            "mag": _errors(_grad(lambda v: mr(v, yt)[1], x32), want_mag, keep),
            "loss": _errors(_grad(lambda v: loss(v, yt)[0], x32), want_sc + want_mag, keep)}, share


def _check(name, errs, share_or_bounds, bounds=None):
    share, bounds = (share_or_bounds, bounds) if bounds is not None else (0.0, share_or_bounds)
    print(f"{name}: " + ", ".join(f"{k} L2 {v[0]:.2e} peak {v[1]:.2e}" for k, v in errs.items())
          + f"; {100 * share:.3f} % of the frames excluded")
    assert share <= MAX_EXCLUDED_FRAMES, (name, share)
    for i, term in enumerate(("sc", "mag", "loss", "multiband")):
        if term in errs:
            bound = bounds[2 * min(i, 2):2 * min(i, 2) + 2]      # the multiband Loss shares the Loss bound
            assert errs[term][0] <= bound[0] and errs[term][1] <= bound[1], (name, term, errs[term], bound)


@pytest.mark.parametrize("name", sorted(PAIR_BOUNDS))
def test_gradient_against_the_oracle(golden_dir, name):
    """Measured on MI355X, device path / eager float32 chain (L2, peak): noise sc 1.5e-7, 2.5e-7 / 2.0e-7, 2.3e-7,
    mag 7.0e-4, 7.3e-4 / 2.5e-3, 2.6e-3; demo sc 2.6e-7, 4.3e-7 / 3.1e-7, 7.2e-7, mag 1.5e-4, 1.5e-4 / 1.2e-3, 3.3e-3;
    sine mag 2.8e-4, 5.0e-4 / 1.7e-3, 6.6e-3 with 8 of its 7803 frames excluded (0.10 %).  With every frame compared,
    sine's mag error is 1.5e-2, 6.9e-2: two bins of the estimate's noise floor, one at a power of 0.9998e-7 beside the
    1e-7 clamp and one where X = Y to four digits, fall on the other side in float32 and carry all of it."""
    x, y, _ = _pairs(golden_dir)[name]
    _check(name, *measure_pair(x, y), PAIR_BOUNDS[name])


def length_cases():
    """name -> (x, y): lengths that are not multiples of the hops, the shortest signal, B = 1 and B > 1"""
    rs = np.random.RandomState(41)
    out = {}
    for B, n in ((1, 1025), (3, 1025), (1, 5003), (2, 24119), (3, 1026)):
        env = np.sin(np.arange(n) / 300.0)
        out[f"B{B}_n{n}"] = (rs.uniform(-1, 1, (B, n)) * env, rs.uniform(-1, 1, (B, n)) * env)
    return out


def test_gradient_on_odd_lengths_and_batches():
    for name, (x, y) in length_cases().items():
        _check(name, *measure_pair(x, y), LENGTH_BOUNDS[name])


def single_resolution_cases():
    """(n_fft, hop, win_length, n): the shortest n = n_fft/2 + 1 of every size, win_length < n_fft (odd left pad),
    win_length = n_fft, a hop of one sample"""
    return ((2048, 240, 1200, 1025), (1024, 120, 600, 513), (512, 50, 240, 257), (1024, 77, 1024, 5003),
            (2048, 333, 601, 7001), (512, 1, 7, 700))


def measure_single(nf, hop, wl, n, B=2):
    rs = np.random.RandomState(nf + hop + n)
    x32, y32 = rs.uniform(-1, 1, (B, n)).astype(np.float32), rs.uniform(-1, 1, (B, n)).astype(np.float32)
    x64, y64 = x32.astype(np.float64), y32.astype(np.float64)
    f = STFTLoss(nf, hop, wl).to(_dev())
    f.differentiable = True
    yt = _t(y32)
    sums = ref.partial_sums(x64, y64, nf, hop, wl).sum(axis=0)
    gd, gl = gref.grad_sums(x64, y64, nf, hop, wl)
    want_sc = 0.5 / (np.sqrt(sums[0]) * np.sqrt(sums[1])) * gd
    want_mag = gl / (B * (1 + n // hop) * (nf // 2 + 1))
    return {"sc": _errors(_grad(lambda v: f(v, yt)[0], x32), want_sc),
            "mag": _errors(_grad(lambda v: f(v, yt)[1], x32), want_mag)}


def test_single_resolutions_against_the_oracle():
    for nf, hop, wl, n in single_resolution_cases():
        _check(f"STFTLoss({nf}, {hop}, {wl}) n={n}", measure_single(nf, hop, wl, n), SINGLE_BOUNDS)


def measure_golden(golden_dir):
    d = np.load(os.path.join(golden_dir, "stft_loss_grad.npz"))
    yt = _t(d["y"])
    mr, loss, pqmf = _mr(), _loss(), PQMF().to(_dev())
    return {"sc": _errors(_grad(lambda v: mr(v, yt)[0], d["x"]), d["g_sc"]),
            "mag": _errors(_grad(lambda v: mr(v, yt)[1], d["x"]), d["g_mag"]),
            "loss": _errors(_grad(lambda v: loss(v, yt)[0], d["x"]), d["g_single"]),
            "multiband": _errors(_grad(lambda v: loss(v, yt, pqmf=pqmf)[0], d["est_sub"]), d["g_multi"])}


def test_gradient_meets_the_reference_golden(golden_dir):
    _check("golden", measure_golden(golden_dir), GOLDEN_BOUNDS)


def test_identical_signals_give_a_zero_gradient():
    x32 = np.random.RandomState(2).uniform(-1, 1, (3, 20011)).astype(np.float32)
    yt = _t(x32)
    mr = _mr()
    for term in (0, 1):
        g = _grad(lambda v: mr(v, yt)[term], x32)
        assert np.isfinite(g).all() and not g.any(), term
        g = _grad(lambda v: mr.per_utterance(v, yt)[:, term].sum(), x32)
        assert np.isfinite(g).all() and not g.any(), term
    g = _grad(lambda v: _loss()(v, yt)[0], x32)
    assert np.isfinite(g).all() and not g.any()


def test_forward_values_are_the_default_path_bits():
    rs = np.random.RandomState(3)
    x, y = _t(rs.randn(4, 9000)), _t(rs.randn(4, 9000))
    plain, mr = MultiResolutionSTFTLoss(), _mr()
    with torch.no_grad():
        want, want_per, want_sums = plain(x, y), plain.per_utterance(x, y), plain.partial_sums(x, y)
        got_ng = mr(x, y)
    xg = x.clone().requires_grad_(True)
    got, got_per, got_sums = mr(xg, y), mr.per_utterance(xg, y), mr.partial_sums(xg, y)
    assert all(v.grad_fn is not None for v in (*got, got_per, got_sums))
    assert all(v.grad_fn is None for v in got_ng)
    for a, b in zip((*got, got_per, got_sums, *got_ng), (*want, want_per, want_sums, *want)):
        assert torch.equal(a.detach(), b)
    f, fd = STFTLoss(1024, 120, 600), STFTLoss(1024, 120, 600)
    fd.differentiable = True
    with torch.no_grad():
        want = f(x, y)
    for a, b in zip(fd(xg, y), want):
        assert a.grad_fn is not None and torch.equal(a.detach(), b)
    with torch.no_grad():
        want = Loss()(x, y)[0]
    assert torch.equal(_loss()(xg, y)[0].detach(), want)


def test_two_backward_calls_are_bit_identical():
    rs = np.random.RandomState(4)
    x32, yt = rs.randn(8, 50000).astype(np.float32), _t(rs.randn(8, 50000))
    mr = _mr()
    a = _grad(lambda v: sum(mr(v, yt)), x32)
    b = _grad(lambda v: sum(mr(v, yt)), x32)
    assert np.array_equal(a, b) and a.any()


def test_a_row_alone_gives_its_batch_bits():
    rs = np.random.RandomState(5)
    x32, y32 = rs.randn(4, 9000).astype(np.float32), rs.randn(4, 9000).astype(np.float32)
    x32[2] *= 1e-2
    mr = _mr()
    for b in range(4):
        batch = _grad(lambda v: mr.per_utterance(v, _t(y32))[b].sum(), x32)
        alone = _grad(lambda v: mr.per_utterance(v, _t(y32[b:b + 1]))[0].sum(), x32[b:b + 1])
        assert np.array_equal(batch[b:b + 1], alone), b
        assert not np.delete(batch, b, axis=0).any()              # the other rows: exactly zero


def test_non_default_stream_and_non_contiguous_input():
    rs = np.random.RandomState(6)
    x32, y32 = rs.randn(3, 30000).astype(np.float32), rs.randn(3, 30000).astype(np.float32)
    yt = _t(y32)
    mr = _mr()
    want, wall = stream_tools.timed(_grad, lambda v: sum(mr(v, yt)), x32)
    torch.cuda.synchronize()
    # on a side stream that is still busy (tests/stream_tools.py): the inputs arrive behind a delay and hold NaN until then,
    # so a forward or backward launch on any other stream than the caller's reads NaN  (_grad's own .cpu() would wait)
    s = stream_tools.side_stream()
    with stream_tools.delayed(s, stream_tools.delay_ms(wall)) as put:
        x = put(x32).requires_grad_(True)
        out = sum(mr(x, put(y32)))
        assert out.grad_fn is not None
        out.backward()
        stream_tools.assert_busy(put, "the STFT loss and its gradient")
    s.synchronize()
    assert x.grad is not None and x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    assert np.array_equal(x.grad.cpu().numpy().astype(np.float64), want)
    base = torch.empty((30000, 3), device=_dev()).copy_(_t(x32).t()).requires_grad_(True)
    xt = base.t()                                                 # a transposed view of a leaf
    assert not xt.is_contiguous()
    sum(mr(xt, yt)).backward()
    assert np.array_equal(base.grad.t().cpu().numpy().astype(np.float64), want)
    wide = torch.zeros((3, 60000), device=_dev())
    wide[:, ::2] = _t(x32)
    wide.requires_grad_(True)
    sum(mr(wide[:, ::2], yt)).backward()
    assert np.array_equal(wide.grad[:, ::2].cpu().numpy().astype(np.float64), want)
    assert not wide.grad[:, 1::2].any()


def test_what_stays_refused():
    x = torch.zeros((2, 5000), device=_dev())
    g = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only"):
        MultiResolutionSTFTLoss()(g, x)                           # the default path
    with pytest.raises(RuntimeError, match="inference-only"):
        Loss()(g, x)
    with pytest.raises(RuntimeError, match="target"):
        _mr()(x, g)                                               # the target has no gradient
    with pytest.raises(RuntimeError, match="target"):
        _mr()(g, x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="inference-only"):
        _loss()(x, g)
    with torch.no_grad():
        sc, mag = _mr()(g, x)                                     # no grad mode: nothing changes
    assert sc.grad_fn is None and mag.grad_fn is None
    sc, mag = _mr()(x, x)                                         # nothing requires grad: the plain call
    assert sc.grad_fn is None


def test_gradient_descent_lowers_the_loss_at_every_step(golden_dir):
    """Thirty steps of plain gradient descent on a leaf waveform, from noise towards a piece of the demo clip; the
    step size 0.1 was tuned on the float64 oracle, where every step lowers sc + mag by 0.3 % or more (0.3 works
    there too)."""
    demo = np.load(os.path.join(golden_dir, "mel_demo.npz"))["wav"] / 32768.0
    yt = _t(demo[20000:28000][None])
    x = _t(0.05 * np.random.RandomState(31).randn(1, 8000)).requires_grad_(True)
    mr = _mr()
    values = []
    for _ in range(31):
        loss = sum(mr(x, yt))
        values.append(float(loss.detach()))
        x.grad = None
        loss.backward()
        with torch.no_grad():
            x -= 0.1 * x.grad
    print(f"descent: {values[0]:.4f} -> {values[-1]:.4f}")
    assert all(b < a for a, b in zip(values, values[1:])), values
    assert values[-1] < 0.95 * values[0]


def test_a_torch_generator_trains_through_the_loss():
    torch.manual_seed(0)
    gen = torch.nn.Sequential(torch.nn.Conv1d(1, 4, 9, padding=4), torch.nn.Tanh(),
                              torch.nn.Conv1d(4, 1, 9, padding=4)).to(_dev())
    z = torch.randn(2, 1, 6000, device=_dev())
    y = _t(np.random.RandomState(8).uniform(-0.5, 0.5, (2, 6000)))
    loss = _loss()
    opt = torch.optim.SGD(gen.parameters(), lr=1e-2)
    before = float(loss(gen(z)[:, 0, :], y)[0].detach())
    opt.zero_grad()
    value, _ = loss(gen(z)[:, 0, :], y)
    value.backward()
    for p in gen.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
    opt.step()
    assert np.isfinite(before) and np.isfinite(float(loss(gen(z)[:, 0, :], y)[0].detach()))


def test_multiband_gradient_reaches_the_sub_bands():
    rs = np.random.RandomState(9)
    sub = _t(0.1 * rs.randn(2, 4, 1500)).requires_grad_(True)
    y = _t(rs.uniform(-0.5, 0.5, (2, 6000)))
    ew = torch.randn(3, 5, device=_dev(), requires_grad=True)
    value, _ = _loss()(sub, y, pqmf=PQMF().to(_dev()))
    value.backward()
    assert torch.isfinite(sub.grad).all() and sub.grad.abs().max() > 0
    full = _t(rs.randn(2, 6000)).requires_grad_(True)
    value, wl = _loss()(full, y, est_weight=ew, weight=torch.zeros(3, 5, device=_dev()))
    (value + wl).backward()
    assert torch.isfinite(full.grad).all() and torch.isfinite(ew.grad).all() and ew.grad.abs().max() > 0


def test_grad_bench_tool_prints_one_json_line():
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "tools", "stft_loss_grad_bench.py"), "--batches", "1",
                        "--samples", "24000", "--target-s", "0.05"], cwd=cases.ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    row = json.loads(lines[0])["rows"][0]
    assert row["B"] == 1 and row["n"] == 24000
    for k in ("fused_ms", "eager_ms", "fused_peak_mb", "eager_peak_mb"):
        assert row[k] > 0, row
