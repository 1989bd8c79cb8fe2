#!/usr/bin/env python
"""Kernel census: which compiled kernel instantiation has a test ever launched?

Every `__global__` instantiation of libfastvocoder_hip.so has a host stub among the library's dynamic symbols
(`__device_stub__<kernel>`).  This tool lists them from the built .so (a small .dynsym reader, names through the
library's own fv_debug_kernel_name: no external program), runs the GPU suite in ONE process with every test wrapped in
the launch log (`_native.launch_log`; see Recorder) and writes tests/kernel_census.json: for every instantiation up to
three witnesses -- node ids of tests whose own body launched it -- or, where no test can, an `excuse`.

    python tools/kernel_census.py                 # run the GPU suite, rewrite tests/kernel_census.json
    python tools/kernel_census.py --check         # run it again: fail if a committed witness no longer launches its kernel
    python tools/kernel_census.py --list          # the built instantiations (no GPU needed)
    python tools/kernel_census.py --out F --per-test G [pytest args]   # other targets / a test -> kernels dump
    python tools/kernel_census.py --from-per-test G [G2 ...]            # the census from recorded dumps (no GPU; a later
                                                                        #  dump replaces an earlier one's files)

It is a tool: it changes no conftest.py and no pytest setting and registers no plugin or hook: the recorder stands between
the Python binding and the library, and learns the running test from pytest's PYTEST_CURRENT_TEST.
What it cannot see: launches of child processes (the CLI tests, bench.py, the data-parallel workers) and which block or
path inside a kernel ran.  tests/test_kernel_census_host.py checks the committed file against the built library.
"""
import argparse
import json
import os
import struct
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CENSUS_PATH = os.path.join(ROOT, "tests", "kernel_census.json")
STUB = "__device_stub__"
MAX_WITNESSES = 3

HEADER = {
    "about": "tools/kernel_census.py: every kernel instantiation of libfastvocoder_hip.so (the __device_stub__ dynamic "
             "symbols) with up to three tests whose body launched it under _native.launch_log, or an excuse",
    "not_seen": "launches of child processes (tests of the command-line tools, bench.py and the data-parallel workers) "
                "and which block or path inside a kernel ran",
}

# Kernels no generator, discriminator, loss, gradient, optimizer or audio entry point can launch with valid arguments.
# tests/test_kernel_census_host.py pins this set by name.
EXCUSES = {
    "profile_null_kernel": "measurement: the empty kernel of fv_profile_bracket_cost (bench.py's per-launch cost)",
    "profile_mfma_f16_kernel": "measurement: the register-only MFMA loop of fv_profile_mfma_f16_rate (bench.py's roofline)",
    "div_probe_kernel": "probe: fv_div_probe's self-check of div_exact against the device's division",
}
# Instantiations a dispatcher can never select (dead code; listed so that they are not mistaken for a gap in the tests).
EXCUSES.update({f"pair_sum_kernel<2, 1, 8, {dil}>":
                "dead: launch_pairs (csrc/pair_launch.hip) refuses the fp32 MRF sum form unless C = 16, so the 32-channel "
                "instantiation is never selected (tests/test_gpu_kernel_reach.py pins the refusal)" for dil in (1, 3, 5)})


def dynamic_symbols(path):
    """Names of the DEFINED symbols of an ELF64 little-endian file's .dynsym (bytes, mangled)."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:6] != b"\x7fELF\x02\x01":
        raise ValueError(f"{path}: not a little-endian ELF64 file")
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = []
    for _, sh_type, _, _, off, size, link, _, _, entsize in sections:
        if sh_type != 11:                                  # SHT_DYNSYM
            continue
        str_off, str_size = sections[link][4], sections[link][5]
        strtab = data[str_off:str_off + str_size]
        for at in range(off, off + size, entsize or 24):
            st_name, _, _, st_shndx, _, _ = struct.unpack_from("<IBBHQQ", data, at)
            if st_shndx == 0 or st_name == 0:              # undefined / nameless
                continue
            names.append(strtab[st_name:strtab.index(b"\0", st_name)])
    return names


def built_kernels(path=None):
    """Sorted names of every kernel instantiation the built library holds, as the launch log prints them."""
    from fastvocoder_amd import _native
    path = path or _native.LIB_PATH
    stubs = [s for s in dynamic_symbols(path) if STUB.encode() in s]
    names = sorted({_native.kernel_name(s) for s in stubs})
    if len(names) != len(stubs):
        raise RuntimeError(f"{len(stubs)} stubs but {len(names)} distinct names: the normalisation merges kernels")
    return names


READERS = ("fv_debug_launch_log_read", "fv_debug_launch_log_streams")    # they read the table: no launch, no restart


class Recorder:
    """Attributes the library's launches to the test that made them, without any hook into the test runner.  The launch
    log stays on for the whole run; the binding's library handle (`_native._lib`) is replaced by a proxy that, after every
    call into the library, reads what the log gained and books it to the test pytest names in PYTEST_CURRENT_TEST (its
    documented environment variable: "<node id> (call)" while a test's body runs).  A test that opens
    `_native.launch_log` itself goes through the same proxy: what the log holds is booked before its `(1)` clears the
    table and again at its `(0)`, and recording resumes with the next call."""

    def __init__(self, native=None):
        if native is None:
            from fastvocoder_amd import _native as native
        self.native = native          # (tests/test_kernel_census_host.py hands in a stand-in with a scripted library)
        self.real = native.lib()
        self.seen = {}           # node id -> {kernel name: launches}
        self.last = {}           # the table as it was read last
        self.node = None         # the node whose launches the table holds
        self.off = False         # a test's own launch_log has stopped the log

    def read(self):
        need = self.real.fv_debug_launch_log_read(None, 0)
        buf = self.native.ctypes.create_string_buffer(max(int(need), 1))
        self.real.fv_debug_launch_log_read(buf, need)
        table = {}
        for line in buf.raw[:need].decode().splitlines():
            count, name = line.split("\t", 1)
            table[name] = table.get(name, 0) + int(count)
        return table

    @staticmethod
    def current():
        """The node id of the test whose body is running, or None (set-up, tear-down, collection)."""
        cur = os.environ.get("PYTEST_CURRENT_TEST", "")
        return cur[:-len(" (call)")] if cur.endswith(" (call)") else None

    def book(self):
        """Books the launches since the last reading to the node they were made under."""
        table = self.read()
        if self.node is not None:
            rec = self.seen.setdefault(self.node, {})
            for name, count in table.items():
                gained = count - self.last.get(name, 0)
                if gained > 0:
                    rec[name] = rec.get(name, 0) + gained
        self.last = table

    def restart(self):
        self.real.fv_debug_launch_log(1)
        self.last, self.off = {}, False

    def before(self, name):
        node = self.current()
        if name in READERS:
            return
        if name == "fv_debug_launch_log":          # a test's own log: book what the table holds before it is cleared / stopped
            if not self.off:
                self.book()
            return
        if self.off or node != self.node:          # a new test (a short table again), or a test's own log has ended
            if not self.off:
                self.book()
            self.node = node
            self.restart()

    def after(self, name, args):
        if name == "fv_debug_launch_log":
            self.node = self.current()
            self.last, self.off = {}, not args[0]
        elif name not in READERS and not self.off:
            if self.node is not None:
                self.seen.setdefault(self.node, {})
            self.book()

    def install(self):
        rec = self

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(rec.real, name)
                if not name.startswith("fv_") or name in ("fv_last_error", "fv_version", "fv_build_id"):
                    return fn

                def call(*args):
                    rec.before(name)
                    out = fn(*args)
                    rec.after(name, args)
                    return out
                setattr(self, name, call)
                return call

        self.native._lib = Proxy()
        self.restart()

    def remove(self):
        if not self.off:
            self.book()
        self.real.fv_debug_launch_log(0)
        self.native._lib = self.real


def run_suite(extra):
    rec = Recorder()
    # (--rootdir: node ids relative to the repository root, whatever directory the tool was started from)
    args = ["-q", "-p", "no:cacheprovider", "--rootdir", ROOT, "-m", "gpu"] + (extra or [os.path.join(ROOT, "tests")])
    rec.install()
    try:
        rc = pytest.main(args)
    finally:
        rec.remove()
    return int(rc), rec.seen


def make_census(kernels, seen, previous=None):
    """kernels: built names; seen: node id -> {kernel: count} in collection order; previous: the committed entries, whose
    witnesses are kept where they still hold (a stable file)."""
    by_kernel = {}
    for node, ks in seen.items():
        for name in ks:
            by_kernel.setdefault(name, []).append(node)
    unknown = sorted(set(by_kernel) - set(kernels))
    if unknown:
        raise RuntimeError(f"the launch log names kernels the library does not list: {unknown[:5]}")
    entries = {}
    for name in kernels:
        nodes = by_kernel.get(name, [])
        keep = [w for w in (previous or {}).get(name, {}).get("witnesses", []) if w in nodes]
        witnesses = (keep + [n for n in nodes if n not in keep])[:MAX_WITNESSES]
        entry = {"witnesses": witnesses}
        family = name.split("<", 1)[0]
        if not witnesses:
            entry["excuse"] = EXCUSES.get(name) or EXCUSES.get(family) or ""
        entries[name] = entry
    return entries


def load(path=CENSUS_PATH):
    with open(path) as f:
        return json.load(f)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--check", action="store_true", help="fail if a committed witness no longer launches its kernel")
    ap.add_argument("--list", action="store_true", help="print the built instantiations and exit")
    ap.add_argument("--out", default=CENSUS_PATH, help="where to write the census (default: tests/kernel_census.json)")
    ap.add_argument("--per-test", default=None, help="also write {node id: {kernel: launches}} to this file")
    ap.add_argument("--from-per-test", nargs="+", default=None, metavar="DUMP",
                    help="build the census from --per-test dumps instead of running the suite; the tests of a file that a "
                         "later dump holds replace that file's tests of the earlier ones")
    ap.add_argument("pytest_args", nargs="*", help="test files / node ids instead of the whole GPU suite")
    a = ap.parse_args(argv)

    kernels = built_kernels()
    if a.list:
        print("\n".join(kernels))
        print(f"{len(kernels)} instantiations", file=sys.stderr)
        return 0
    if a.from_per_test:
        rc, seen = 0, {}
        for path in a.from_per_test:
            with open(path) as f:
                dump = json.load(f)
            files = {node.split("::", 1)[0] for node in dump}
            seen = {node: ks for node, ks in seen.items() if node.split("::", 1)[0] not in files}
            seen.update(dump)
    else:
        rc, seen = run_suite(a.pytest_args)
    if a.per_test:
        with open(a.per_test, "w") as f:
            json.dump(seen, f, indent=0)
    if rc != 0:
        print(f"kernel_census: the suite failed (pytest exit code {rc}); no census written", file=sys.stderr)
        return rc
    previous = load()["kernels"] if os.path.exists(CENSUS_PATH) else {}
    if a.check:
        launched = {n: set(ks) for n, ks in seen.items()}
        stale = [(name, w) for name, e in previous.items() for w in e.get("witnesses", [])
                 if name not in launched.get(w, ())]
        missing = sorted(set(kernels) ^ set(previous))
        for name, w in stale:
            print(f"kernel_census: {w} no longer launches {name}", file=sys.stderr)
        if missing:
            print(f"kernel_census: the file and the library disagree on {missing[:5]} ...", file=sys.stderr)
        print(f"kernel_census --check: {len(previous)} entries, {len(stale)} stale witnesses")
        return 1 if stale or missing else 0
    entries = make_census(kernels, seen, previous)
    witnessed = sum(1 for e in entries.values() if e["witnesses"])
    excused = sum(1 for e in entries.values() if not e["witnesses"] and e.get("excuse"))
    header = dict(HEADER, total=len(entries), witnessed=witnessed, excused=excused)
    with open(a.out, "w") as f:
        json.dump({"header": header, "kernels": entries}, f, indent=1, sort_keys=False)
        f.write("\n")
    bare = [n for n, e in entries.items() if not e["witnesses"] and not e.get("excuse")]
    print(f"kernel_census: {len(entries)} instantiations, {witnessed} witnessed, {excused} excused, {len(bare)} with neither")
    for n in bare:
        print("  unreached:", n)
    return 0


if __name__ == "__main__":
    sys.exit(main())
