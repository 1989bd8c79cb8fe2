"""tests/kernel_census.json against the built library, and the host side of the launch log (no GPU): every kernel
instantiation of libfastvocoder_hip.so has an entry, every entry names a test that launched it (tools/kernel_census.py
recorded that on the MI355X; `--check` repeats it) or is excused, and the excused set is pinned here by name."""
import importlib.util
import os
import re

import pytest

from fastvocoder_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Only a kernel that no generator, discriminator, loss, gradient, optimizer or audio entry point can launch with valid
# arguments may stand here.  profile_null_kernel is fv_profile_bracket_cost's empty kernel: a measurement aid of bench.py,
# whose only caller in the suite is a child process (tests/test_gpu_bench.py), which the launch log does not see.
# pair_sum_kernel<2, 1, 8, dil> is the fp32 MRF stage end at 32 channels: compiled, but launch_pairs refuses the sum form unless
# C = 16, so no dispatcher can select it (tests/test_gpu_kernel_reach.py pins the refusal).
EXCUSED = {"profile_null_kernel", "pair_sum_kernel<2, 1, 8, 1>", "pair_sum_kernel<2, 1, 8, 3>", "pair_sum_kernel<2, 1, 8, 5>"}


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_census", os.path.join(ROOT, "tools", "kernel_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return _tool()


@pytest.fixture(scope="module")
def census(tool):
    return tool.load()


def test_every_built_instantiation_has_an_entry_and_no_entry_is_stale(tool, census):
    built = tool.built_kernels()
    assert len(built) == len(set(built)) and len(built) > 300
    listed = set(census["kernels"])
    assert listed == set(built), {"missing from the file": sorted(set(built) - listed)[:10],
                                  "no longer built": sorted(listed - set(built))[:10]}
    assert census["header"]["total"] == len(built)


def test_every_entry_has_a_witness_or_an_excuse(census):
    bare = [name for name, e in census["kernels"].items() if not e["witnesses"] and not e.get("excuse")]
    assert not bare, bare
    for name, e in census["kernels"].items():
        assert len(e["witnesses"]) <= 3 and len(set(e["witnesses"])) == len(e["witnesses"]), name
        assert not (e["witnesses"] and e.get("excuse")), name      # an excuse stands only where no test launches the kernel


def test_the_excused_set_is_pinned(tool, census):
    excused = {name for name, e in census["kernels"].items() if not e["witnesses"]}
    assert excused == EXCUSED
    for name in excused:
        reason = census["kernels"][name]["excuse"]
        assert reason == tool.EXCUSES[name] and len(reason) > 20, name
    # measurement and probe kernels and the dead instantiations are all the tool may excuse
    assert set(tool.EXCUSES) == EXCUSED | {"profile_mfma_f16_kernel", "div_probe_kernel"}


def test_every_witness_names_a_test_that_exists(census):
    sources = {}
    for name, e in census["kernels"].items():
        for w in e["witnesses"]:
            path, _, rest = w.partition("::")
            func = rest.split("[", 1)[0]
            assert path.startswith("tests/test_gpu_") and path.endswith(".py") and func.startswith("test_"), (name, w)
            if path not in sources:
                full = os.path.join(ROOT, path)
                assert os.path.isfile(full), (name, w)
                with open(full) as f:
                    sources[path] = f.read()
            assert re.search(rf"^def {re.escape(func)}\(", sources[path], flags=re.M), (name, w)


def test_the_header_says_what_the_log_cannot_see(census):
    assert "child process" in census["header"]["not_seen"] and "inside a kernel" in census["header"]["not_seen"]


def test_dynamic_symbol_reader_finds_the_c_abi(tool):
    names = set(tool.dynamic_symbols(_native.LIB_PATH))
    assert {b"fv_version", b"fv_debug_launch_log", b"fv_debug_launch_log_read", b"fv_debug_kernel_name"} <= names
    stubs = [n for n in names if b"__device_stub__" in n]
    handles = {n.replace(b"__device_stub__", b"") for n in stubs}
    assert len(stubs) == len(tool.built_kernels()) and len(handles) == len(stubs)


@pytest.mark.parametrize("symbol,name", [
    ("_ZN2fv12convh_kernelILi2ELi2ELi1EEEvNS_10PairParamsE", "convh_kernel<2, 2, 1>"),
    ("_ZN2fv27__device_stub__convh_kernelILi2ELi2ELi1EEEvNS_10PairParamsE", "convh_kernel<2, 2, 1>"),
    ("_ZN2fv12convr_kernelENS_10PairParamsE", "convr_kernel"),
    ("_ZN2fv15resample_kernelIsEEvPKT_PKfPflliii", "resample_kernel<short>"),
    # a parameter type the demangler may not know (_Float16*): the name is still the kernel's
    ("_ZN2fv33__device_stub__pack_convtn_kernelEPKfPDF16_S1_Pi", "pack_convtn_kernel"),
    ("fv_version", "fv_version"),
])
def test_kernel_names(symbol, name):
    assert _native.kernel_name(symbol) == name


def test_launch_log_is_off_by_default_and_does_not_nest():
    L = _native.lib()
    assert L.fv_debug_launch_log(2) == _native.ERR_INVALID_ARG
    with _native.launch_log() as log:
        assert log.kernels == {}
        with pytest.raises(_native.NativeError, match="already active"):
            with _native.launch_log():
                pass
    assert log.kernels == {} and log.families() == set()      # nothing was launched: an empty table reads as empty
    assert L.fv_debug_launch_log_read(None, 0) == 0
    with _native.launch_log() as again:                           # usable again after the refused nesting
        pass
    assert again.kernels == {}


def test_the_stream_table_reads_as_empty_when_nothing_was_launched():
    import ctypes
    L = _native.lib()
    with _native.launch_log() as log:
        pass
    assert log.streams == {} and log.copies == 0
    copies = ctypes.c_int64(-1)
    assert L.fv_debug_launch_log_streams(None, None, 0, ctypes.byref(copies)) == 0 and copies.value == 0
    assert b"fv_debug_launch_log_streams" in set(_tool().dynamic_symbols(_native.LIB_PATH))


def test_every_enqueueing_call_is_written_in_the_two_helpers_alone():
    """Kernel launches and asynchronous memsets / copies appear in csrc/fv_internal.h only (FV_KERNEL_LAUNCH, memset_async,
    memcpy_async): what the launch log's stream table counts is everything the library enqueues."""
    csrc = os.path.join(ROOT, "fastvocoder_amd", "csrc")
    forbidden = re.compile(r"hipLaunchKernelGGL|hipLaunchKernel\b|hipModuleLaunchKernel|hipExtLaunchKernel|hipLaunchCooperativeKernel|<<<|"
                           r"hipMemsetAsync|hipMemcpyAsync|hipMemset\w*Async|hipMemcpy\w*Async|hipMemcpy\w*\(|hipMemset\w*\(|hipGraphLaunch")
    sites, helper_uses = [], 0
    for name in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, name)) as f:
            for n, line in enumerate(f, 1):
                if forbidden.search(line) and name != "fv_internal.h":
                    sites.append(f"{name}:{n}: {line.strip()}")
                helper_uses += len(re.findall(r"\bFV_KERNEL_LAUNCH\(|\bmemset_async\(|\bmemcpy_async\(", line)) if name != "fv_internal.h" else 0
    assert not sites, sites
    assert helper_uses >= 128 + 4, helper_uses
    with open(os.path.join(csrc, "fv_internal.h")) as f:
        own = f.read()
    code = "\n".join(line.split("//", 1)[0] for line in own.splitlines())
    assert len(re.findall(r"hipLaunchKernelGGL\(", code)) == 1 and len(re.findall(r"hipMemsetAsync\(", code)) == 1
    assert len(re.findall(r"hipMemcpyAsync\(", code)) == 1


class _ScriptedLibrary:
    """The three log entries and two operators that 'launch', as the recorder's proxy sees a library."""

    def __init__(self):
        self.on, self.table = 0, {}

    def fv_debug_launch_log(self, on):
        if on:
            self.table = {}
        self.on = on
        return 0

    def fv_debug_launch_log_read(self, buf, cap):
        text = "".join(f"{n}\t{name}\n" for name, n in self.table.items()).encode()
        if buf is not None:
            buf[:min(len(text), cap)] = text[:cap]
        return len(text)

    def fv_debug_launch_log_streams(self, handles, counts, cap, copies):
        return 1 if self.table else 0

    def _launch(self, name):
        if self.on:
            self.table[name] = self.table.get(name, 0) + 1
        return 0

    def fv_op_a(self):
        return self._launch("a_kernel<1>")

    def fv_op_b(self):
        return self._launch("b_kernel")


def test_recorder_books_launches_to_the_running_test(tool, monkeypatch):
    """tools/kernel_census.py's Recorder on a scripted library: launches go to the test named in PYTEST_CURRENT_TEST while its
    body runs, not to set-up or tear-down; a test's own launch log (clear, stop, read) loses nothing and recording resumes."""
    import ctypes
    import types
    real = _ScriptedLibrary()
    native = types.SimpleNamespace(ctypes=ctypes, _lib=real, lib=lambda: real)
    rec = tool.Recorder(native)
    rec.install()
    lib = native._lib
    assert lib is not real and real.on == 1
    monkeypatch.setenv("PYTEST_CURRENT_TEST", "tests/test_gpu_x.py::test_one (setup)")
    lib.fv_op_a()                                                   # a fixture's launch: nobody's
    monkeypatch.setenv("PYTEST_CURRENT_TEST", "tests/test_gpu_x.py::test_one (call)")
    lib.fv_op_a()
    lib.fv_op_a()
    lib.fv_debug_launch_log(1)                                      # the test opens its own log ...
    lib.fv_op_b()
    lib.fv_debug_launch_log(0)
    buf = ctypes.create_string_buffer(64)
    n = lib.fv_debug_launch_log_read(buf, 64)
    assert buf.raw[:n] == b"1\tb_kernel\n"                         # ... and reads what it launched, no more
    assert lib.fv_debug_launch_log_streams(None, None, 0, None) == 1     # ... its stream table too: reading restarts nothing
    lib.fv_op_a()                                                   # recording resumes with the next call
    monkeypatch.setenv("PYTEST_CURRENT_TEST", "tests/test_gpu_x.py::test_one (teardown)")
    lib.fv_op_b()
    monkeypatch.setenv("PYTEST_CURRENT_TEST", "tests/test_gpu_x.py::test_two[p] (call)")
    lib.fv_op_b()
    rec.remove()
    assert native._lib is real and real.on == 0
    assert rec.seen == {"tests/test_gpu_x.py::test_one": {"a_kernel<1>": 3, "b_kernel": 1},
                        "tests/test_gpu_x.py::test_two[p]": {"b_kernel": 1}}


def test_census_from_dumps_replaces_a_files_tests(tool, tmp_path):
    import json
    one, two = tmp_path / "one.json", tmp_path / "two.json"
    one.write_text(json.dumps({"tests/test_gpu_a.py::t": {"profile_null_kernel": 1}, "tests/test_gpu_b.py::t_0": {"mel_kernel": 1}}))
    two.write_text(json.dumps({"tests/test_gpu_b.py::t": {"mel_kernel": 2}}))
    out = tmp_path / "census.json"
    assert tool.main(["--from-per-test", str(one), str(two), "--out", str(out)]) == 0
    got = json.loads(out.read_text())["kernels"]
    assert got["mel_kernel"]["witnesses"] == ["tests/test_gpu_b.py::t"]
    assert got["profile_null_kernel"]["witnesses"] == ["tests/test_gpu_a.py::t"]
