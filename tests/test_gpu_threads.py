"""The thread half of the library's contract: one module instance per worker thread, each on a stream of its own, needs
no lock (include/fastvocoder_hip.h).

Three Python threads (tests/threads_worker.py), each with its own ``torch.cuda.Stream``, its own modules and its own
seeded inputs, start from a barrier and run 20 iterations each; every iteration's result is cloned on the thread's
stream and compared after the join, bit for bit, with a serial run of the same steps made beforehand on the default
stream.  The library has no atomics: equal bits is the bar.  What the threads share is host state: the schedule and
width caches of csrc/convh_launch.hip and the LDS grants (mutexes), the tuning table (call_once), the device's CU count
(an atomic), the thread-local error text, and in Python the per-device tables of _stft_tables.py.

One instance driven from two threads is refused by documentation and not tested.  A fault or a hang here is a finding
to diagnose from the code; the test is not to be repeated to provoke it."""
import ctypes
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from tests import concurrency_cases as cc
from tests import test_gpu_guarded as G
from tests import threads_worker as tw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROUND_1 = [cc.hifigan_s, lambda put: cc.small_msd(put, 100), lambda put: cc.stft_loss(put, 2, 1680)]
ROUND_2 = [cc.hifigan_then_split_conv] * 3


def _serial(make, iterations=tw.ITERATIONS):
    """The same steps on the default stream, one after the other: (every iteration's result, the launch log of the run)."""
    with _native.launch_log() as log:
        case = make(G._Put(None))
        results = [cc.clone(case.step()) for _ in range(iterations)]
    torch.cuda.synchronize()
    return results, log


def _compare_with_serial(workers, serial, what):
    for w, want in zip(workers, serial):
        assert len(w.results) == len(want) == tw.ITERATIONS, (what, w.index, len(w.results))
        for i, (got, ref) in enumerate(zip(w.results, want)):
            G._compare(f"{what}, thread {w.index}, iteration {i}", got, ref)


@pytest.mark.parametrize("name,makes", [("different families", ROUND_1), ("one family and shape", ROUND_2)],
                         ids=["round_1", "round_2"])
def test_three_threads_give_the_bits_of_a_serial_run(name, makes):
    serial = [_serial(make)[0] for make in (makes if makes is ROUND_1 else makes[:1])]
    if makes is ROUND_2:
        serial = serial * 3
    for want in serial:                                     # the serial run itself repeats its bits
        for i, ref in enumerate(want[1:]):
            G._compare(f"{name}, serial iteration {i + 1}", ref, want[0])
    workers = tw.run_threads(makes)
    _compare_with_serial(workers, serial, name)


def test_cold_start_in_a_fresh_process():
    """Round 2 in a child whose first library calls race (tests/threads_worker.py cold); the digests are compared with a
    serial run made here."""
    want = [cc.digest(r) for r in _serial(cc.hifigan_then_split_conv)[0]]
    assert len(set(want)) == 1
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "threads_worker.py"), "cold"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    digests = json.loads(r.stdout.strip().splitlines()[-1])["digests"]
    assert len(digests) == 3 and all(len(d) == tw.ITERATIONS for d in digests)
    for k, d in enumerate(digests):
        assert d == want, (k, [i for i, (a, b) in enumerate(zip(d, want)) if a != b])


def test_the_launch_log_under_threads_sums_the_serial_logs_and_names_three_streams():
    """The only test here that turns the log on: ``kernels`` is the three serial logs summed, ``streams`` holds exactly the
    three threads' streams, each with its thread's count."""
    serial = [_serial(make) for make in ROUND_1]
    want_kernels = {}
    for _, log in serial:
        assert set(log.streams) == {0}, log.streams                      # the serial runs: the null stream alone
        for name, n in log.kernels.items():
            want_kernels[name] = want_kernels.get(name, 0) + n
    with _native.launch_log() as log:
        workers = tw.run_threads(ROUND_1)
    _compare_with_serial(workers, [s[0] for s in serial], "logged round")
    assert log.kernels == want_kernels, {k: (log.kernels.get(k), want_kernels.get(k))
                                         for k in set(log.kernels) | set(want_kernels) if log.kernels.get(k) != want_kernels.get(k)}
    assert log.streams == {w.stream.cuda_stream: sum(s[1].streams.values()) for w, s in zip(workers, serial)}
    assert len(log.streams) == 3 and log.copies == sum(s[1].copies for s in serial)


def test_errors_stay_with_their_thread():
    """Two threads loop over two different host-side refusals (no launch), a third makes valid calls: every NativeError
    carries its own thread's message and the third thread's error text stays empty."""
    L = _native.lib()
    z = torch.zeros(4096, dtype=torch.float32, device=G.DEV)
    p = z.data_ptr()

    def refused(cin, cout, k, pad):
        return L.fv_grouped_conv1d_input_grad(p, None, None, p + 4, p + 8, 1, cin, cout, 100, k, 1, pad, ctypes.c_float(1.0), None)

    calls = [lambda: refused(6, 3, 5, 2),                   # not 4 channels per group: unsupported
             lambda: refused(8, 4, 5, -1)]                  # negative padding: invalid argument
    expected = []
    for call in calls:
        with pytest.raises(_native.NativeError) as e:
            _native.check(call())
        expected.append(str(e.value))
    assert expected[0] != expected[1] and "-2" in expected[0] and "-1" in expected[1], expected
    x = torch.from_numpy(np.random.RandomState(3).randn(3, 1, 1001).astype(np.float32)).to(G.DEV)
    want = _native.avg_pool1d(x, 4, 2, 1)
    torch.cuda.synchronize()
    barrier, rounds = threading.Barrier(3), 200
    seen, problems = [[], [], []], []

    def refuser(k):
        barrier.wait(timeout=60)
        for _ in range(rounds):
            try:
                _native.check(calls[k]())
                seen[k].append("no error")
            except _native.NativeError as e:
                seen[k].append(str(e))

    def valid():
        try:
            stream = torch.cuda.Stream(device=G.DEV)
            with torch.cuda.stream(stream):
                barrier.wait(timeout=60)
                for _ in range(rounds):
                    got = _native.avg_pool1d(x, 4, 2, 1)
                    seen[2].append(L.fv_last_error().decode())
                stream.synchronize()
                if not torch.equal(got, want):
                    problems.append("the valid thread's result differs")
        except BaseException as e:                          # noqa: BLE001
            problems.append(repr(e))

    threads = [threading.Thread(target=refuser, args=(0,), daemon=True), threading.Thread(target=refuser, args=(1,), daemon=True),
               threading.Thread(target=valid, daemon=True)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(tw.JOIN_TIMEOUT_S)
    assert not any(t.is_alive() for t in threads), [len(s) for s in seen]
    assert not problems, problems
    assert seen[0] == [expected[0]] * rounds and seen[1] == [expected[1]] * rounds, (set(seen[0]), set(seen[1]))
    assert seen[2] == [""] * rounds, set(seen[2])
