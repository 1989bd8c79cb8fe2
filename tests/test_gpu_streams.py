"""The stream half of the library's contract: every launch of a call goes to the caller's stream.

a. Attribution (exact, no timing).  Every case of tests/test_gpu_guarded.py -- its functions ``fn(put)``, run through
   that file's own test functions with its runner ``_twice`` replaced -- runs once plain on the default stream and once
   more inside ``with torch.cuda.stream(side)`` under ``_native.launch_log``, on a fresh module and fresh inputs: equal
   bits, and the log's stream table holds ``side`` alone, with as many entries as kernels were launched and memsets and
   copies enqueued.  Two kinds of case are left out: ``saturated/*`` (five; their point is the kernel form, and
   ``policy/*`` and ``shipped/*`` launch the same sites) and ``hook/mfma_rate`` (takes no tensor).  Three cases also run
   with the graph built on ``side`` and ``.backward()`` called outside the block, on the default stream: autograd
   restores the forward's stream on its worker thread, so the library's backward launches belong on ``side`` too.
   (What torch's own kernels do is not the log's business: it sees the library's launches only.)

b. Ordering (end to end).  tests/stream_tools.py ``delayed(side)``: the side stream is busy with a delay, every input
   arrives behind it and every buffer holds NaN until then.  A launch on any other stream reads NaN and equality with
   the reference (the same case on the default stream, its own module, computed and synchronised beforehand) fails.
   A case counts only if the delay was still running when the call returned (``Staged.still_delayed``); otherwise it FAILS as
   inconclusive.  Delay: three times the host wall time of the reference run, 20 ms at least, 1 s at most.  The side stream
   is one that a probe has shown to run beside the null stream (stream_tools.side_stream: on a shared hardware queue a
   launch on the null stream would wait for the delay too, and show nothing).
   Substitutions for calls that synchronise inside:
   * ``small/hifigan_s`` with ``range_guard = "lazy"``: a fresh module's first call waits for the pack kernels' verdict
     on the weights (fastvocoder_amd/generator/engine.py, NativeModule._plan: ``current_stream(...).synchronize()``).
     Under the delay runs the module's SECOND call, on a new input; the fresh-module build (pack kernels and plan
     behind the delay) runs with ``range_guard = "off"``, which has no verdict to wait for.
   * ``audio.melspectrogram`` with its table first built under ``side``: the table's upload is a copy from pageable
     memory, which waits for the stream (fastvocoder_amd/_stft_tables.py, device_cached: ``.to(device)``).  Under the
     delay runs the call on the table the reference run cached: a cached-table consumer.
   DESIGN.md section 5.6 has the calibration and the delay of every case."""
import pytest
import torch

from fastvocoder_amd import _native, audio
from tests import concurrency_cases as cc
from tests import stream_tools as st
from tests import test_gpu_guarded as G

pytestmark = pytest.mark.gpu

LEFT_OUT = {c for c in G.ALL_CASES if c.startswith("saturated/")} | {"hook/mfma_rate"}
_ATTRIBUTED = set()


def _side():
    return torch.cuda.Stream(device=G.DEV)


def _library_launches(log):
    return sum(log.kernels.values()) + log.copies


def _assert_all_on(log, side, what):
    n = _library_launches(log)
    assert n > 0, f"{what}: the library launched nothing"
    assert log.streams == {side.cuda_stream: n}, (what, f"side stream {side.cuda_stream:#x}", log.streams, log.kernels)


# ---- a. attribution ----------------------------------------------------------------------------------------------------
def _attributed(case_id, fn, compare=True):
    """Stands in for test_gpu_guarded._twice: ``fn(put)`` plain on the default stream, then on a side stream under the log."""
    assert case_id in G.ALL_CASES and case_id not in LEFT_OUT, case_id
    plain = fn(G._Put(None))
    torch.cuda.synchronize()
    side = _side()
    with torch.cuda.stream(side):
        with _native.launch_log() as log:
            got = fn(G._Put(None))
        side.synchronize()
    torch.cuda.synchronize()
    _ATTRIBUTED.add(case_id)
    print(f"{case_id}: {sum(log.kernels.values())} kernel launches, {log.copies} async memsets / copies")
    _assert_all_on(log, side, case_id)
    if compare:
        G._compare(case_id, got, plain)
    return got


# (the test function of test_gpu_guarded.py that runs the case, its arguments) per case id
_RUNNERS = {}
_RUNNERS.update({f"direct/{k}": (G.test_direct_entries, (f"direct/{k}",)) for k in G.DIRECT})
_RUNNERS.update({name: (G.test_adam_step_with_clipping, (name,)) for name in ("adam/clip_and_step", "adam/bucket_pack")})
_RUNNERS.update({f"small/{c[0]}": (G.test_small_generators, (f"small/{c[0]}",)) for c in G.cases.SMALL})
_RUNNERS.update({f"shipped/{c[0]}/{B}x{T}": (G.test_shipped_generators, (c[0], B, T)) for c in G.cases.SHIPPED
                 for B, T in ((1, 37), (3, 24))})
_RUNNERS.update({f"policy/{a}": (G.test_hifigan_light_under_each_policy, (a, v)) for a, v in G.POLICIES})
_RUNNERS["arena/long_short_long"] = (G.test_a_long_a_shorter_and_the_long_input_again_on_one_module_with_the_arena_poisoned, ())
_RUNNERS.update({w: (G.test_inference_minus_and_chunked_inference, (w,))
                 for w in ("flows/inference_minus", "flows/chunked", "flows/chunked_basis")})
_RUNNERS.update({f"disc/{k}": (G.test_discriminator_forward_input_gradient_and_parameter_gradient, (k,)) for k in G.DISCS})
_RUNNERS["disc/zero_gradient"] = (G.test_the_zero_gradient_of_an_input_no_map_reaches, ())
_RUNNERS["loss/mr_stft"] = (G.test_differentiable_multi_resolution_stft_loss, ())
_RUNNERS.update({f"training/{t}": (G.test_generators_in_training, (t,)) for t in G.TRAINING})
_RUNNERS["training/basis_l1"] = (G.test_basis_weight_l1_term, ())
_RUNNERS.update({f"trainer/{p}": (G.test_one_trainer_step, (p,)) for p in ("stft_only", "adversarial")})


def test_the_case_table_is_the_guarded_file_s_minus_the_two_exclusions():
    assert set(_RUNNERS) == set(G.ALL_CASES) - LEFT_OUT and len(LEFT_OUT) == 6 and len(_RUNNERS) == len(G.ALL_CASES) - 6


@pytest.mark.parametrize("case_id", sorted(_RUNNERS))
def test_every_launch_of_a_case_goes_to_the_callers_stream(case_id, monkeypatch):
    monkeypatch.setattr(G, "_twice", _attributed)
    test, args = _RUNNERS[case_id]
    _ATTRIBUTED.discard(case_id)
    test(*args)
    assert case_id in _ATTRIBUTED, f"{case_id}: the guarded file's test did not run the case through its runner"


BACKWARD_OUTSIDE = {"msd_both_gradients": lambda put: cc.small_msd(put, 2001), "training/hifigan_s": cc.hifigan_s_training,
                    "loss/mr_stft": lambda put: cc.stft_loss(put, 3, 1301)}


@pytest.mark.parametrize("name", sorted(BACKWARD_OUTSIDE))
def test_a_backward_called_on_the_default_stream_launches_on_the_forwards_stream(name):
    make = BACKWARD_OUTSIDE[name]
    plain = make(G._Put(None)).step()
    torch.cuda.synchronize()
    side = _side()
    with torch.cuda.stream(side):
        case = make(G._Put(None))
        with _native.launch_log() as forward_log:
            outs = case.forward()
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
    with _native.launch_log() as backward_log:
        got = case.backward(outs)
    torch.cuda.synchronize()
    print(f"{name}: forward {_library_launches(forward_log)} launches, backward {_library_launches(backward_log)}")
    _assert_all_on(forward_log, side, f"{name} forward")
    _assert_all_on(backward_log, side, f"{name} backward")
    G._compare(name, got, plain)


# ---- b. ordering ---------------------------------------------------------------------------------------------------------
def _direct(key):
    return G.DIRECT[key]


def _adam(put):
    return G._adam_case(put, bucket=False)


def _hifigan_off(put):
    return cc.hifigan_s(put, range_guard="off").step()


def _msd(put):
    return cc.small_msd(put, 2001).step()


ORDERED = {
    "direct/conv/fp32": _direct("conv/fp32"),                       # an exact-fp32 kernel
    "direct/conv/split_f16": _direct("conv/split_f16"),             # a split-f16 kernel
    "direct/pair/fused": _direct("pair/fused"),
    "direct/stage/one_launch": _direct("stage/one_launch"),
    "direct/pqmf_basis_wav": _direct("pqmf_basis_wav"),             # the wav sink's memset
    "direct/pack/split_images": _direct("pack/split_images"),       # the pack memset and copies
    "direct/resample": _direct("resample"),
    "direct/disc/input_grad": _direct("disc/input_grad"),
    "direct/gen/weight_grad": _direct("gen/weight_grad"),           # a weight-gradient tile
    "adam/clip_and_step": _adam,                                    # the optimizer: the pinned-table upload and its event
    "small/hifigan_s/off/fresh": _hifigan_off,                      # a plan run: pack kernels and plan build behind the delay
    "msd_both_gradients": _msd,                                     # an autograd backward
}


def _ordered(name, reference, under_delay, after=None):
    """``reference(put)`` on the default stream (timed: the delay's length), ``under_delay(put)`` behind the delay."""
    want, wall = st.timed(reference, G._Put(None))
    torch.cuda.synchronize()
    ms = st.delay_ms(wall)
    side = st.side_stream()
    with st.delayed(side, ms) as put:
        got, under = st.timed(under_delay, put)
        busy = put.still_delayed()
        side.synchronize()
    torch.cuda.synchronize()
    print(f"{name}: reference run {1e3 * wall:.1f} ms of host time, delay {ms:.0f} ms, the call behind it returned after "
          f"{1e3 * under:.1f} ms, {'conclusive' if busy else 'INCONCLUSIVE'}")
    assert busy, (f"{name}: inconclusive -- the delay on the side stream had ended when the call returned (the call synchronised, "
                  "or the delay was too short): a launch on another stream could not have shown")
    if after is not None:
        after()
    G._compare(name, got, want)


@pytest.mark.parametrize("name", sorted(ORDERED))
def test_a_case_behind_a_busy_side_stream_equals_the_default_stream_run(name):
    _ordered(name, ORDERED[name], ORDERED[name])


def test_hifigan_s_lazy_second_call_behind_a_busy_side_stream():
    """``small/hifigan_s`` with ``range_guard = "lazy"`` (the module docstring says why it is the second call), then
    ``check_range()`` once the conclusiveness is settled."""
    from fastvocoder_amd.synthetic import seeded_mel
    mel2 = seeded_mel(G.cases.SMALL_T, seed=77, batch=G.cases.SMALL_B)
    held = {}

    def reference(put):
        case = cc.hifigan_s(put)
        case.step()
        with torch.no_grad():
            return case.module(put(mel2)).clone()

    def under_delay(put):
        with torch.no_grad():
            return held["case"].module(put(mel2))

    held["case"] = cc.hifigan_s(G._Put(None))            # its own module; the first call builds the plan and waits for the verdict
    held["case"].step()
    torch.cuda.synchronize()
    _ordered("small/hifigan_s/lazy/second_call", reference, under_delay, after=lambda: _no_range_error(held["case"].module))


def _no_range_error(module):
    assert not module.check_range()


def test_melspectrogram_on_its_cached_table_behind_a_busy_side_stream():
    import numpy as np
    x = (0.3 * np.random.RandomState(9).randn(2, 1300)).astype(np.float32)
    _ordered("audio.melspectrogram", lambda put: audio.melspectrogram(put(x)), lambda put: audio.melspectrogram(put(x)))
