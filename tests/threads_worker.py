"""Worker threads of tests/test_gpu_threads.py, and the child process of its cold-start test.

``run_threads(makes, iterations)`` starts one daemon thread per entry of ``makes``; each thread gets a
``torch.cuda.Stream`` of its own, waits at a barrier, builds its own module and inputs (``make(put)`` of
tests/concurrency_cases.py) and runs ``iterations`` steps on its stream, keeping a clone of every step's result.

``python tests/threads_worker.py cold`` is the cold-start child: a fresh process in which the three threads' FIRST
library calls race -- the tuning table, the device's CU count, the LDS grants, the schedule and width caches of
csrc/convh_launch.hip, the tables cached per device.  It prints one JSON line: per thread, the digest of every
iteration's result (concurrency_cases.digest)."""
import json
import os
import sys
import threading
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEV = "cuda:0"
ITERATIONS = 20
JOIN_TIMEOUT_S = 120


class Worker:
    def __init__(self, index, make, barrier, iterations, put):
        self.index, self.make, self.barrier, self.iterations, self.put = index, make, barrier, iterations, put
        self.stream = torch.cuda.Stream(device=DEV)
        self.results, self.reached, self.error = [], "the barrier", None
        self.thread = threading.Thread(target=self._run, name=f"fv-worker-{index}", daemon=True)

    def _run(self):
        from tests import concurrency_cases as cc
        try:
            torch.cuda.set_device(DEV)
            with torch.cuda.stream(self.stream):
                self.barrier.wait(timeout=JOIN_TIMEOUT_S)
                self.reached = "the build of its module"
                case = self.make(self.put)
                for i in range(self.iterations):
                    self.reached = f"iteration {i}"
                    self.results.append(cc.clone(case.step()))
                self.reached = "its last synchronize"
                self.stream.synchronize()
                self.reached = "the end"
        except BaseException:                              # noqa: BLE001 -- reported by the test, with the thread's name
            self.error = traceback.format_exc()


def run_threads(makes, iterations=ITERATIONS, put=None):
    """-> the Workers, joined.  A thread that has not ended after JOIN_TIMEOUT_S, or that raised, is an AssertionError."""
    from tests import test_gpu_guarded as G
    put = G._Put(None) if put is None else put
    barrier = threading.Barrier(len(makes))
    workers = [Worker(k, make, barrier, iterations, put) for k, make in enumerate(makes)]
    for w in workers:
        w.thread.start()
    for w in workers:
        w.thread.join(JOIN_TIMEOUT_S)
    stuck = [f"thread {w.index} had reached {w.reached}" for w in workers if w.thread.is_alive()]
    assert not stuck, f"not joined after {JOIN_TIMEOUT_S} s: {stuck}"
    failed = [f"thread {w.index} at {w.reached}:\n{w.error}" for w in workers if w.error]
    assert not failed, "\n".join(failed)
    torch.cuda.synchronize()
    return workers


def main(argv):
    from tests import concurrency_cases as cc
    if argv[1:] != ["cold"]:
        raise SystemExit("usage: python tests/threads_worker.py cold")
    workers = run_threads([cc.hifigan_then_split_conv] * 3)
    print(json.dumps({"digests": [[cc.digest(r) for r in w.results] for w in workers]}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
