"""ctypes binding of libfastvocoder_hip.so (include/fastvocoder_hip.h; every entry's signature and every FV_*
constant below are read from that header by _abi.py, none is restated here).

PyTorch-ROCm is plumbing here: it owns device memory (tensors) and the stream;
every function below passes raw device pointers and the current HIP stream to
the C ABI.  There is NO fallback: if the shared library is missing or a tensor
is not a contiguous fp32 tensor on a ROCm device, these raise.
"""
import ctypes
import os
import subprocess

import torch

from . import _abi
from ._abi import NativeError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfastvocoder_hip.so")
_CSRC = os.path.join(_HERE, "csrc")
# conv_inst_s*.hip instantiate the conv kernel templates (conv_kernels.hpp) one tile shape each,
# so that the ~170 kernel variants compile in parallel
SOURCES = ["conv_mfma.hip", "api.hip", "plan.hip", "pack.hip", "pqmf.hip", "wav_sink.hip", "mel.hip", "resample.hip", "griffin_lim.hip", "stft_loss.hip", "stft_loss_grad.hip", "stft_mag_grad.hip", "disc.hip", "disc_grad.hip", "disc_wgrad.hip", "mpd.hip", "mpd_grad.hip", "mpd_wgrad.hip", "gen_grad.hip", "gen_grad_bf16.hip", "basis_grad.hip", "basis_learn.hip", "optim.hip", "conv_inst_narrow.hip",
           "pair_launch.hip", "pair_inst_c16.hip", "pair_inst_c32.hip", "pairh_inst_c16.hip", "pairh_inst_c32.hip",
           "convh_launch.hip", "convh_inst_c64.hip", "convh_inst_c128.hip", "convt_inst.hip",
           "convg_inst.hip", "convr_inst.hip", "convtn_inst.hip", "convk_inst.hip", "convq2_inst.hip",
           "mrfh_launch.hip", "mrfh_inst_a.hip", "mrfh_inst_b.hip", "mrfw_inst.hip", "convtl_inst.hip", "convs2_inst.hip", "convu2_inst.hip"] + \
          [f"conv_inst_s{i}.hip" for i in range(6)]
HEADERS = ["fv_internal.h", "launch_host.hpp", "conv_kernels.hpp", "pair_kernels.hpp", "pair_inst.hpp", "pairh_kernels.hpp",
           "pairh_inst.hpp", "convh_kernels.hpp", "convh_inst.hpp", "convr_kernels.hpp",
           "convtn_kernels.hpp", "convk_kernels.hpp", "convq2_kernels.hpp", "mrfh_kernels.hpp", "mrfh_inst.hpp", "mrfw_kernels.hpp", "convtl_kernels.hpp", "convs2_kernels.hpp", "convu2_kernels.hpp", "api_internal.h", "stft_core.hpp", "basis_grad_host.hpp", "wgrad_tile.hpp", "gen_grad_host.hpp"]

_C = _abi.constants()        # every FV_X below is include/fastvocoder_hip.h's `#define FV_X <integer>`
PAD_ZERO, PAD_REFLECT = _C["FV_PAD_ZERO"], _C["FV_PAD_REFLECT"]
PAD_CAUSAL = _C["FV_PAD_CAUSAL"]      # flag: pad (k-1)*dil on both sides, keep the first Tin outputs (CausalConv1d)
POST_NONE, POST_TANH, POST_RELU = _C["FV_POST_NONE"], _C["FV_POST_TANH"], _C["FV_POST_RELU"]
SLOT_NONE, SLOT_IN, SLOT_OUT, SLOT_TMP0 = _C["FV_SLOT_NONE"], _C["FV_SLOT_IN"], _C["FV_SLOT_OUT"], _C["FV_SLOT_TMP0"]
MAX_SLOTS = _C["FV_MAX_SLOTS"]
# caller-provided tensors of Plan.run(aux=..., out2=...)
SLOT_AUX_IN0, SLOT_AUX_IN1, SLOT_OUT2 = _C["FV_SLOT_AUX_IN0"], _C["FV_SLOT_AUX_IN1"], _C["FV_SLOT_OUT2"]
ABI_VERSION = _C["FV_ABI_VERSION"]
PAIR_F32, PAIR_SPLIT_F16 = _C["FV_PAIR_F32"], _C["FV_PAIR_SPLIT_F16"]   # arithmetic of the fused ResBlock-pair kernels


ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = _C["FV_ERR_INVALID_ARG"], _C["FV_ERR_UNSUPPORTED"], _C["FV_ERR_WORKSPACE"]
ERR_RANGE = _C["FV_ERR_RANGE"]    # fv_plan_check_range: a split-f16 kernel met an operand beyond the f16 range
GUARD_HIGH, GUARD_LOW = _C["FV_GUARD_HIGH"], _C["FV_GUARD_LOW"]   # the two sides of a guard word (separate bytes)
ERR_RANGE_LOW = _C["FV_ERR_RANGE_LOW"]   # ... only the low-side guard fired (a block's share of a tensor was small as a whole)


class RangeError(NativeError):
    """A weight or an activation lies outside the domain of the split-f16 kernels (|v| < 65520, the f16 range;
    include/fastvocoder_hip.h FV_PAIR_SPLIT_F16): the computation has to be repeated with PAIR_F32 arithmetic.
    engine.NativeModule does that by itself; the exception reaches a caller only from the single-operator
    functions of this module."""


BASE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
              "-Wno-unused-value", "-Wno-comment", "-Wno-pass-failed",
              # MFMA results straight in VGPRs (unified register file on gfx950): no
              # v_accvgpr_read/write pairs around every stage -- VALU work costs MFMA time
              "-mllvm", "-amdgpu-mfma-vgpr-form=1",
              # the device code objects compressed inside the fat binary (zstd; the HIP runtime inflates them when the library
              # is loaded): the .so is 2.4 MB instead of 10.9
              "--offload-compress"]


def source_hash():
    """sha256 (first 16 hex digits) over every source of the library and the extra compiler flags: the
    build id the .so carries (fv_build_id), so that a binary can be proven to be built from this tree."""
    import hashlib
    h = hashlib.sha256()
    paths = [os.path.join(_CSRC, s) for s in SOURCES] + [os.path.join(_CSRC, x) for x in HEADERS] + \
        [os.path.join(_HERE, "..", "include", "fastvocoder_hip.h")]
    for path in paths:
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as f:
            h.update(f.read())
    h.update(" ".join(BASE_FLAGS[4:]).encode())      # (the flags that were added after round 4: older ids stay comparable)
    h.update(os.environ.get("FV_HIPCC_FLAGS", "").encode())
    return h.hexdigest()[:16]


def built_id():
    """Build id of the .so on disk, or None when it is missing / predates build ids.  Read from the file's bytes
    (the "fv-build-id:" tag in front of the string fv_build_id() returns), not through dlopen: a library this
    process has already loaded would answer for the OLD image after a rebuild."""
    if not os.path.exists(LIB_PATH):
        return None
    with open(LIB_PATH, "rb") as f:
        data = f.read()
    at = data.find(b"fv-build-id:")
    if at < 0:
        return None
    end = data.find(b"\0", at)
    return data[at + 12:end].decode(errors="replace") if 0 < end - at - 12 <= 64 else None


def _local_includes(path, seen=None):
    """Transitive closure of the `#include "..."` files of a source (paths relative to the including file)."""
    import re
    seen = set() if seen is None else seen
    with open(path) as f:
        text = f.read()
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, flags=re.M):
        dep = os.path.normpath(os.path.join(os.path.dirname(path), inc))
        if dep not in seen and os.path.exists(dep):
            seen.add(dep)
            _local_includes(dep, seen)
    return seen


def _object_stamp(src, flags):
    """Hash of everything an object file depends on: its source, the headers it includes (transitively), the flags."""
    import hashlib
    h = hashlib.sha256()
    for path in [src] + sorted(_local_includes(src)):
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as f:
            h.update(f.read())
    h.update(" ".join(flags).encode())
    return h.hexdigest()


def build(force=False, verbose=False):
    """hipcc the kernels for gfx950 into fastvocoder_amd/libfastvocoder_hip.so
    (cross-compiles without a GPU): one object per source, compiled in parallel, then linked.
    Up to date <=> the library's embedded build id equals the hash of the sources.  Objects are rebuilt only when their
    own source, a header they include or the flags changed (a stamp file next to each object); the build id is compiled
    into api.hip alone."""
    srcs = [os.path.join(_CSRC, s) for s in SOURCES]
    want = source_hash()
    if not force and built_id() == want:
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = BASE_FLAGS + os.environ.get("FV_HIPCC_FLAGS", "").split()
    objdir = os.path.join(_HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    jobs, objs = [], []
    for src in srcs:
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        own = flags + ([f'-DFV_BUILD_ID="{want}"'] if os.path.basename(src) == "api.hip" else [])
        stamp, stamp_path = _object_stamp(src, own), obj + ".stamp"
        if not force and os.path.exists(obj) and os.path.exists(stamp_path):
            with open(stamp_path) as f:
                if f.read() == stamp:
                    continue
        cmd = [hipcc] + own + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        if os.path.exists(stamp_path):
            os.remove(stamp_path)
        jobs.append((cmd, stamp_path, stamp, subprocess.Popen(cmd)))
    for cmd, stamp_path, stamp, proc in jobs:
        if proc.wait() != 0:
            for _, _, _, other in jobs:
                if other.poll() is None:
                    other.kill()
            raise subprocess.CalledProcessError(proc.returncode, cmd)
        with open(stamp_path, "w") as f:
            f.write(stamp)
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB_PATH]
    if verbose:
        print(" ".join(link))
    subprocess.check_call(link)
    return LIB_PATH


_lib = None


def lib():
    """Load the library (never builds implicitly: a GPU box gets the prebuilt .so)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). fastvocoder_amd has no CPU or eager fallback.")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _abi.prototypes().items():      # (a declared entry the library lacks raises here)
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.fv_version() != ABI_VERSION:
        raise NativeError(f"ABI mismatch: library reports {L.fv_version()}, binding expects {ABI_VERSION}")
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise NativeError(f"libfastvocoder_hip error {rc}: {lib().fv_last_error().decode()}")


def _ptr(t, name="tensor", allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise NativeError(f"{name} is None")
    if not t.is_cuda:
        raise NativeError(f"{name} lives on {t.device}; the HIP kernels need a ROCm device "
                          "tensor (there is no CPU path in fastvocoder_amd)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise NativeError(f"{name} must be contiguous float32, got {t.dtype} "
                          f"contiguous={t.is_contiguous()}")
    return t.data_ptr()


class _on:
    """Context for one native call: makes the operands' device current (the kernels launch on the
    CURRENT device; after ``model.to('cuda:1')`` that need not be the tensors') and yields that
    device's current stream.  All tensor operands must live on one device."""

    def __init__(self, *tensors):
        devs = {t.device for t in tensors if t is not None}
        if len(devs) != 1:
            raise NativeError(f"operands of a native call must share one ROCm device, got {sorted(map(str, devs))}")
        self.dev = devs.pop()
        if self.dev.type != "cuda":
            raise NativeError(f"operands live on {self.dev}; the HIP kernels need a ROCm device tensor "
                              "(there is no CPU path in fastvocoder_amd)")
        self._guard = torch.cuda.device(self.dev)

    def __enter__(self):
        self._guard.__enter__()
        return torch.cuda.current_stream(self.dev).cuda_stream

    def __exit__(self, *exc):
        return self._guard.__exit__(*exc)


class GuardWord:
    """Two int32 words in pinned, device-mapped host memory: [0] raised by the split-f16 kernels of a run when an
    activation left the f16 range (fv_plan_set_guard), [1] by the pack kernels when a weight does.  The kernels write
    them through the host pointer; the host reads them after the stream has drained (or, lazily, whenever)."""

    def __init__(self):
        self.t = torch.zeros(2, dtype=torch.int32).pin_memory()

    def ptr(self, i=0):
        return self.t.data_ptr() + 4 * i

    def peek(self, i=0):
        """The word as it is now (no synchronisation)."""
        return int(self.t[i])

    def clear(self, i=0):
        self.t[i] = 0


def tuning_set(key, value):
    """Test / tuning hook (fv_tuning_set): one of the launchers' switches, process-wide."""
    check(lib().fv_tuning_set(key.encode(), int(value)))


class launch_log:
    """Test hook (fv_debug_launch_log, host only): `with launch_log() as log:` records every kernel the library launches
    inside the block; afterwards `log.kernels` is a dict of instantiation name ("convh_kernel<2, 2, 1>") to launch count,
    in first-launch order; `log.streams` is a dict of stream handle (`torch.cuda.Stream.cuda_stream`; 0: the null stream)
    to the kernels launched plus the asynchronous memsets and copies enqueued on it, and `log.copies` is how many of those
    were memsets and copies: sum(streams.values()) == sum(kernels.values()) + copies.  Process-wide and not nestable:
    entering while one is active raises.  Launches of child processes are not seen, nor which block or path inside a
    kernel ran, nor anything torch itself enqueues."""
    _active = False

    def __init__(self):
        self.kernels, self.streams, self.copies = {}, {}, 0

    def __enter__(self):
        if launch_log._active:
            raise NativeError("launch_log is already active (the log is process-wide and does not nest)")
        check(lib().fv_debug_launch_log(1))
        launch_log._active = True
        return self

    def __exit__(self, *exc):
        L = lib()
        launch_log._active = False
        check(L.fv_debug_launch_log(0))
        need = L.fv_debug_launch_log_read(None, 0)
        buf = ctypes.create_string_buffer(max(int(need), 1))
        L.fv_debug_launch_log_read(buf, need)
        self.kernels = {}
        for line in buf.raw[:need].decode().splitlines():
            count, name = line.split("\t", 1)
            self.kernels[name] = self.kernels.get(name, 0) + int(count)
        n = int(L.fv_debug_launch_log_streams(None, None, 0, None))
        handles, counts, copies = (ctypes.c_uint64 * max(n, 1))(), (ctypes.c_int64 * max(n, 1))(), ctypes.c_int64(0)
        L.fv_debug_launch_log_streams(handles, counts, n, ctypes.byref(copies))
        self.streams = {int(handles[k]): int(counts[k]) for k in range(n)}
        self.copies = int(copies.value)
        return False

    def operators(self):
        """`kernels` without the weight-preparation kernels (pack_*, row_scale_kernel, fold_*): a module packs its weights
        inside its first call, which is not the operator a test asks about."""
        return {name: n for name, n in self.kernels.items()
                if not name.startswith(("pack_", "fold_")) and name not in ("row_scale_kernel", "transpose_basis_kernel")}

    def families(self):
        """The operators' names without template arguments: {"convh_kernel", ...}."""
        return {name.split("<", 1)[0] for name in self.operators()}


def kernel_name(symbol):
    """fv_debug_kernel_name: the launch log's name for a dynamic symbol of the library (a kernel handle or its host stub)."""
    L = lib()
    sym = symbol.encode() if isinstance(symbol, str) else symbol
    need = L.fv_debug_kernel_name(sym, None, 0)
    buf = ctypes.create_string_buffer(max(int(need), 1))
    L.fv_debug_kernel_name(sym, buf, need)
    return buf.raw[:need].decode()


def debug_pair_schedule(n_items, cost, nblk, mode=0, three_members=False):
    """Test hook (fv_debug_pair_schedule, host only): the block schedule of a fused-pair launch.  Returns
    ``(sched_on, shares)``: sched_on 1 -- ``shares[b][m] = (lo, count)``, member m's items of block b (pair_schedule);
    2 -- ``shares[i]`` = first item of share i in the members' concatenated item sequence (pair_cut_schedule); 0 -- no
    table for this shape (``shares`` is None)."""
    n = len(n_items)
    arr = ctypes.c_int * n
    table = (ctypes.c_uint * 512)()
    rc = lib().fv_debug_pair_schedule(n, arr(*[int(v) for v in n_items]), arr(*[int(v) for v in cost]), int(nblk), int(mode),
                                      1 if three_members else 0, table)
    check(rc if rc < 0 else 0)
    if rc == 1:
        out = []
        for b in range(nblk):
            w0, w1 = table[2 * b], table[2 * b + 1]
            e = [w0 & 0xFFFF, w0 >> 16, w1 & 0xFFFF]
            out.append([(v & 2047, v >> 11) for v in e[:n]])
        return 1, out
    if rc == 2:
        return 2, [int(table[i]) for i in range(nblk)]
    return 0, None


def debug_pair_widths(channels, batch, t, dil, taps, blocks):
    """Test and policy hook (fv_debug_pair_widths, host only): the tile widths the fused 128-channel pair launcher picks for
    ``batch`` utterances of ``t`` columns, members of ``taps`` taps (largest first), at most ``blocks`` persistent blocks.
    Returns a dict: ``widths`` / ``items`` / ``costs`` per member, ``makespan`` (the block schedule's model, -1: no block
    schedule for this shape) and ``nblk``.  ``tuning_set("convq_nm11", 64 | 80)`` forces the 11-tap member's width."""
    n = len(taps)
    info = (ctypes.c_int64 * 12)()
    check(lib().fv_debug_pair_widths(int(channels), int(batch), int(t), int(dil), n, (ctypes.c_int * n)(*[int(k) for k in taps]),
                                     int(blocks), info))
    return {"widths": [int(info[m]) for m in range(n)], "items": [int(info[3 + m]) for m in range(n)],
            "costs": [int(info[6 + m]) for m in range(n)], "makespan": int(info[9]), "nblk": int(info[10])}


def mrf_class_schedule(batch, t, nblk, force=False):
    """Test and policy hook (fv_debug_mrf_class_schedule, host only): what the 32-channel MRF stage's launchers do with
    ``batch`` utterances of ``t`` columns on at most ``nblk`` blocks.  Returns a dict: ``split`` (two block classes, or the
    all-in-one form where that is not slower by the window arithmetic -- ``force``: the split whenever nblk >= 2 batch),
    ``n_a`` / ``n_b`` blocks per class, ``makespan`` / ``makespan_one`` (hundreds of cycles), ``reach_a`` / ``reach_b``,
    ``window``, ``cost_a`` / ``cost_b`` / ``cost_one`` and ``ranges``: block i (class A first) owns the global columns
    [lo, hi) of the utterances concatenated."""
    info = (ctypes.c_int64 * 12)()
    table = (ctypes.c_uint * 512)()
    check(lib().fv_debug_mrf_class_schedule(int(batch), int(t), int(nblk), 1 if force else 0, info, table))
    keys = ("split", "n_a", "n_b", "makespan", "makespan_one", "reach_a", "reach_b", "window", "cost_a", "cost_b", "cost_one")
    out = {k: int(info[i]) for i, k in enumerate(keys)}
    out["split"] = bool(out["split"])
    out["ranges"] = [(int(table[2 * i]), int(table[2 * i + 1])) for i in range(out["n_a"] + out["n_b"])]
    return out


def _flag_ptr(flag):
    """Address of a range-flag word: None, a GuardWord (weights: word 1), an int address or an int32 tensor."""
    if flag is None:
        return None
    if isinstance(flag, GuardWord):
        return flag.ptr(1)
    if isinstance(flag, int):
        return flag
    return flag.data_ptr()


def _guard_ptr(guard):
    if guard is None:
        return None
    if isinstance(guard, GuardWord):
        return guard.ptr(0)
    return guard.data_ptr()


# ---------------------------------------------------------------------------
# weight preparation
# ---------------------------------------------------------------------------

def fold_weight_norm(v, g):
    """w = v * g/||v|| over all dims but 0 (torch.nn.utils.weight_norm semantics)."""
    v = v.detach().contiguous().float()
    g = g.detach().contiguous().float()
    w = torch.empty_like(v)
    with _on(v, g) as stream:
        check(lib().fv_fold_weight_norm(_ptr(v, "v"), _ptr(g, "g"), _ptr(w), v.shape[0], v[0].numel(), stream))
    return w


def pack_conv1d(w):
    """Conv1d weight [Cout,Cin,k] -> packed K-major image (flat tensor)."""
    w = w.detach().contiguous().float()
    cout, cin, k = w.shape
    out = torch.empty(lib().fv_packed_conv1d_floats(cout, cin, k), dtype=torch.float32, device=w.device)
    with _on(w) as stream:
        check(lib().fv_pack_conv1d_weight(_ptr(w, "w"), _ptr(out), cout, cin, k, stream))
    return out


def pack_conv_transpose1d(w, stride, pad):
    """ConvTranspose1d weight [Cin,Cout,k] -> packed polyphase image (flat tensor)."""
    w = w.detach().contiguous().float()
    cin, cout, k = w.shape
    n = lib().fv_packed_conv_transpose1d_floats(cin, cout, k, stride, pad)
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    with _on(w) as stream:
        check(lib().fv_pack_conv_transpose1d_weight(_ptr(w, "w"), _ptr(out), cin, cout, k, stride, pad, stream))
    return out


def conv_transpose_split_supported(cin, cout, k, stride, pad, out_pad):
    """Shapes of the split-f16 transposed conv (csrc/convh_launch.hip launch_convt)."""
    if conv_transpose_small(cin, cout, k, stride):
        return pad == 1 and out_pad == 0
    return (cin in (32, 64, 128, 256, 512) and 2 <= stride <= 16 and k == 2 * stride and cout * stride >= 32
            and 0 <= pad <= stride and -stride <= out_pad < stride)


def conv_transpose_small(cin, cout, k, stride):
    """The shape with a kernel of its own (csrc/convtn_kernels.hpp): HiFi-GAN light's last upsampler, 32 -> 16 channels x 2."""
    return (cin, cout, k, stride) == (32, 16, 4, 2)


def pack_conv_transpose1d_split(w, stride, flag=None):
    """ConvTranspose1d weight [Cin,Cout,2*stride] -> split-f16 stage image of convt_kernel (flat fp32-typed tensor).
    ``flag`` (GuardWord / int32 tensor): raised by the kernel when a weight is outside the f16 range."""
    w = w.detach().contiguous().float()
    cin, cout, k = w.shape
    n = lib().fv_packed_conv_transpose1d_split_floats(cin, cout, k, stride)
    if n <= 0:
        raise NativeError(f"pack_conv_transpose1d_split: Cin={cin} Cout={cout} k={k} stride={stride} is not built")
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    with _on(w) as stream:
        check(lib().fv_pack_conv_transpose1d_split_f16(_ptr(w, "w"), _ptr(out), cin, cout, k, stride, _flag_ptr(flag),
                                                       stream))
    return out


def conv1x1_2src_split_supported(channels):
    """Channel counts of the split-f16 two-source 1x1 conv (csrc/convh_launch.hip launch_convg)."""
    return channels in (128, 256, 512)


def pack_conv1x1_2src_split(w1, w2, flag=None):
    """Two 1x1 Conv1d weights [C,C,1] -> split-f16 stage image of convg_kernel for y = W1 act(x) + W2 x2 (flat tensor)."""
    w1, w2 = w1.detach().contiguous().float(), w2.detach().contiguous().float()
    c = w1.shape[0]
    if tuple(w1.shape) != (c, c, 1) or tuple(w2.shape) != (c, c, 1):
        raise NativeError(f"pack_conv1x1_2src_split: two [C,C,1] weights expected, got {tuple(w1.shape)}, {tuple(w2.shape)}")
    n = lib().fv_packed_conv1x1_2src_split_floats(c)
    if n <= 0:
        raise NativeError(f"pack_conv1x1_2src_split: C={c} is not built (128, 256, 512)")
    out = torch.empty(n, dtype=torch.float32, device=w1.device)
    with _on(w1, w2) as stream:
        check(lib().fv_pack_conv1x1_2src_split_f16(_ptr(w1, "w1"), _ptr(w2, "w2"), _ptr(out), c, _flag_ptr(flag), stream))
    return out


def residual_stack_split_supported(channels, k, dil):
    """Shapes of the one-launch MelGAN ResidualStack (csrc/convk_kernels.hpp)."""
    return channels in (32, 64, 128, 256) and k == 3 and dil in (1, 3, 9)


def pack_residual_stack_split(w_dilated, w_pointwise, w_skip, flag=None):
    """The three Conv1d weights of a ResidualStack ([C,C,3] dilated, [C,C,1] stack[4], [C,C,1] skip_layer) -> the
    split-f16 stage image of convk_kernel (flat tensor)."""
    ws = [w.detach().contiguous().float() for w in (w_dilated, w_pointwise, w_skip)]
    c, k = ws[0].shape[0], ws[0].shape[2]
    if tuple(ws[0].shape) != (c, c, k) or tuple(ws[1].shape) != (c, c, 1) or tuple(ws[2].shape) != (c, c, 1):
        raise NativeError(f"pack_residual_stack_split: [C,C,k], [C,C,1], [C,C,1] expected, got {[tuple(w.shape) for w in ws]}")
    n = lib().fv_packed_residual_stack_floats(c, k)
    if n <= 0:
        raise NativeError(f"pack_residual_stack_split: C={c}, k={k} is not built (32 / 64 / 128 / 256 channels, 3 taps)")
    out = torch.empty(n, dtype=torch.float32, device=ws[0].device)
    with _on(*ws) as stream:
        check(lib().fv_pack_residual_stack_split_f16(_ptr(ws[0], "w_dilated"), _ptr(ws[1], "w_pointwise"), _ptr(ws[2], "w_skip"),
                                                     _ptr(out), c, k, _flag_ptr(flag), stream))
    return out


def residual_stack_split_f16(x, packed, bias_dilated, bias_out, k, dil, slope, pad_mode=PAD_REFLECT, out=None, out_act=None,
                             act_slope=1.0, guard=None, post=POST_NONE):
    """MelGAN ResidualStack as one launch (fv_residual_stack_split_f16); packed = pack_residual_stack_split(...),
    bias_out = stack[4].bias + skip_layer.bias."""
    B, c, T = x.shape
    if out is None:
        out = torch.empty_like(x)
    with _on(x, packed, bias_dilated, bias_out, out, out_act) as stream:
        check(lib().fv_residual_stack_split_f16(_ptr(x, "x"), _ptr(packed, "packed"), _ptr(bias_dilated, "bias_dilated", True),
                                                _ptr(bias_out, "bias_out", True), _ptr(out, "out"), _ptr(out_act, "out_act", True),
                                                B, c, T, k, dil, float(slope), pad_mode, post, float(act_slope), _guard_ptr(guard), stream))
    return out


def fold_batchnorm_conv(w, b, bn):
    """Fold an eval-mode ``torch.nn.BatchNorm1d`` into the conv weight/bias that follow it;
    returns (w', b') on w's device."""
    w = w.detach().contiguous().float()
    cout, cin, k = w.shape
    w_out = torch.empty_like(w)
    b_out = torch.empty(cout, dtype=torch.float32, device=w.device)
    t = lambda a: None if a is None else a.detach().contiguous().float()  # noqa: E731
    b, gamma, beta, mean, var = t(b), t(bn.weight), t(bn.bias), t(bn.running_mean), t(bn.running_var)
    with _on(w, b, gamma, beta, mean, var) as stream:
        check(lib().fv_fold_batchnorm_conv(_ptr(w, "w"), _ptr(b, "b", True), _ptr(gamma, "gamma", True),
                                           _ptr(beta, "beta", True), _ptr(mean, "running_mean"),
                                           _ptr(var, "running_var"), float(bn.eps), _ptr(w_out), _ptr(b_out),
                                           cout, cin, k, stream))
    return w_out, b_out


def pack_upsample_conv1d(w, rate, pad):
    """UpsampleLayer conv weight [Cout,Cin,k] -> packed phase image (flat tensor)."""
    w = w.detach().contiguous().float()
    cout, cin, k = w.shape
    n = lib().fv_packed_upsample_conv1d_floats(cout, cin, k, rate, pad)
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    with _on(w) as stream:
        check(lib().fv_pack_upsample_conv1d_weight(_ptr(w, "w"), _ptr(out), cout, cin, k, rate, pad, stream))
    return out


def pack_pair(w, prec=PAIR_F32, flag=None):
    """ResBlock Conv1d weight [C,C,k] -> A-operand image of the fused pair kernels (flat tensor); ``prec``
    selects the fp32 (pair_kernels.hpp) or the split-f16 layout (pairh_kernels.hpp).  ``flag`` (GuardWord / int32
    tensor, split-f16 only): raised by the kernel when a weight is outside the f16 range."""
    w = w.detach().contiguous().float()
    c, c2, k = w.shape
    if c != c2:
        raise NativeError(f"pack_pair: square [C,C,k] weight expected, got {tuple(w.shape)}")
    n = lib().fv_packed_pair_floats_ex(c, k, prec)
    if n <= 0:
        raise NativeError(f"pack_pair: no packed layout for C={c} k={k} arithmetic {prec}")
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    with _on(w) as stream:
        check(lib().fv_pack_pair_weight_ex(_ptr(w, "w"), _ptr(out), c, k, prec, _flag_ptr(flag), stream))
    return out


def pair_supported(channels, k, dil, prec=PAIR_F32):
    """Shapes the fused ResBlock-pair kernels are built for (csrc/pair_launch.hip)."""
    chans = (16, 32) if prec == PAIR_F32 else (16, 32, 64, 128, 256, 512)
    return channels in chans and k in (3, 7, 11) and dil in (1, 3, 5) and prec in (PAIR_F32, PAIR_SPLIT_F16)


def conv_split_supported(channels, k, dil):
    """Shapes of the conv-level split-f16 op (csrc/convh_launch.hip): the ResBlock shapes plus MelGAN's dilation 9."""
    return channels in (64, 128, 256, 512) and ((k in (3, 7, 11) and dil in (1, 3, 5)) or (k == 3 and dil == 9))


def _vp_array(tensors, name, allow_none=False):
    return (ctypes.c_void_p * len(tensors))(*[_ptr(t, name, allow_none) for t in tensors])


# ---------------------------------------------------------------------------
# single fused operators (used by tests and by modules outside a plan)
# ---------------------------------------------------------------------------

def resblock1_fused(xs, w1s, w2s, b1s, b2s, ks, dil, slope, act_slope=1.0, outs=None, outs_act=None,
                    prec=PAIR_F32, add1=None, add2=None, out_div=1.0, post=POST_NONE, mids=None, guard=None):
    """n = len(xs) independent fused ResBlock pairs in one launch (fv_resblock1_fused_ex):
    y_j = x_j + conv2_j(lrelu(conv1_j(lrelu(x_j)) + b1_j)) + b2_j; w1s / w2s from pack_pair(w, prec).
    With add1 / add2 (split-f16 arithmetic): y_j = post(((y_j + add1_j) + add2_j) / out_div)."""
    n = len(xs)
    B, C, T = xs[0].shape
    if outs is None:
        outs = [torch.empty_like(x) for x in xs]
    acts = list(outs_act) if outs_act is not None else [None] * n
    a1 = list(add1) if add1 is not None else [None] * n
    a2 = list(add2) if add2 is not None else [None] * n
    # C >= 64 (split-f16): the pair runs as two conv launches through a scratch tensor per member
    mids = [torch.empty_like(x) if C >= 64 else None for x in xs] if mids is None else list(mids)
    with _on(*xs, *w1s, *w2s, *b1s, *b2s, *outs, *acts, *a1, *a2, *mids) as stream:
        check(lib().fv_resblock1_fused_ex(n, _vp_array(xs, "x"), _vp_array(w1s, "w1"), _vp_array(w2s, "w2"),
                                          _vp_array(b1s, "b1", True), _vp_array(b2s, "b2", True),
                                          _vp_array(outs, "y"), _vp_array(acts, "y_act", True),
                                          _vp_array(mids, "mid", True),
                                          _vp_array(a1, "add1", True), _vp_array(a2, "add2", True),
                                          (ctypes.c_int * n)(*ks), B, C, T, dil, float(slope), float(out_div), post,
                                          float(act_slope), prec, _guard_ptr(guard), stream))
    return outs


def conv1d_split_f16(xs, packed, biases, ks, dil, pre_slope=1.0, res=None, add1=None, add2=None, out_div=1.0,
                     post=POST_NONE, act_slope=1.0, outs=None, outs_act=None, pad_mode=PAD_ZERO, guard=None):
    """n = len(xs) independent 'same' convs with split-f16 operands in one launch (fv_conv1d_split_f16), C = 64 ... 512:
    y_j = post((conv(pad(lrelu(x_j, pre_slope))) + bias_j + res_j + add1_j + add2_j) / out_div), zero or reflection
    padding; packed from pack_pair(w, PAIR_SPLIT_F16)."""
    n = len(xs)
    B, C, T = xs[0].shape
    if outs is None:
        outs = [torch.empty_like(x) for x in xs]
    none = [None] * n
    acts = list(outs_act) if outs_act is not None else none
    rs, a1, a2 = (list(v) if v is not None else none for v in (res, add1, add2))
    with _on(*xs, *packed, *biases, *rs, *a1, *a2, *outs, *acts) as stream:
        check(lib().fv_conv1d_split_f16(n, _vp_array(xs, "x"), _vp_array(packed, "packed"),
                                        _vp_array(biases, "bias", True), _vp_array(rs, "res", True),
                                        _vp_array(a1, "add1", True), _vp_array(a2, "add2", True), _vp_array(outs, "y"),
                                        _vp_array(acts, "y_act", True), (ctypes.c_int * n)(*ks), B, C, T, dil,
                                        pad_mode, float(pre_slope), float(out_div), post, float(act_slope),
                                        _guard_ptr(guard), stream))
    return outs


MRF_STAGE_DILATIONS = (1, 3, 5)


def mrf_stage_supported(channels, ks, dils):
    """Shapes the one-launch MRF stage kernels are built for (csrc/mrfh_launch.hip): 16 or 32 channels, three ResBlocks
    with 3 / 7 / 11 taps (any order), pair dilations (1, 3, 5)."""
    return (channels in (16, 32) and len(ks) == 3 and all(k in (3, 7, 11) for k in ks)
            and tuple(dils) == MRF_STAGE_DILATIONS)


def mrf_stage_workspace(channels, device):
    """The scratch a one-launch MRF stage needs next to its tensors (fv_mrf_stage_workspace_bytes: the 32-channel
    kernel's columns of history; nothing at 16 channels -> None).  One per launch in flight; contents don't matter."""
    n = lib().fv_mrf_stage_workspace_bytes(int(channels))
    return torch.empty((n + 3) // 4, dtype=torch.float32, device=device) if n > 0 else None


def _work_args(work):
    return (_ptr(work, "workspace", True), 0 if work is None else work.numel() * 4)


def pack_mrf_stage(w1s, w2s, b1s, b2s, ks, flag=None):
    """The 18 convs of a 16-channel MRF stage -> the packed stage of fv_mrf_stage_split_f16 (flat tensor).  w1s / w2s:
    nine [16, 16, k_j] weights in the order pair p of ResBlock j at index 3 j + p; b1s / b2s: nine [16] biases or None;
    ks: the three ResBlocks' taps.  ``flag``: raised for a non-finite weight (as pack_pair)."""
    w1s = [w.detach().contiguous().float() for w in w1s]
    w2s = [w.detach().contiguous().float() for w in w2s]
    b1s = [None if b is None else b.detach().contiguous().float() for b in b1s]
    b2s = [None if b is None else b.detach().contiguous().float() for b in b2s]
    if not (len(w1s) == len(w2s) == len(b1s) == len(b2s) == 9 and len(ks) == 3):
        raise NativeError("pack_mrf_stage: nine pairs (three ResBlocks x three positions) expected")
    c = w1s[0].shape[0]
    for i, w in enumerate(w1s + w2s):
        if tuple(w.shape) != (c, c, ks[(i % 9) // 3]):
            raise NativeError(f"pack_mrf_stage: weight {i} has shape {tuple(w.shape)}, expected {(c, c, ks[(i % 9) // 3])}")
    karr = (ctypes.c_int * 3)(*ks)
    nfl = lib().fv_packed_mrf_stage_floats(c, karr)
    if nfl <= 0:
        raise NativeError(f"pack_mrf_stage: no packed layout for C={c} taps={list(ks)}")
    out = torch.empty(nfl, dtype=torch.float32, device=w1s[0].device)
    with _on(*w1s, *w2s, *b1s, *b2s, out) as stream:
        check(lib().fv_pack_mrf_stage_split_f16(_vp_array(w1s, "w1"), _vp_array(w2s, "w2"), _vp_array(b1s, "b1", True),
                                                _vp_array(b2s, "b2", True), _ptr(out), c, karr, _flag_ptr(flag), stream))
    return out


def mrf_stage_split_f16(x, packed, ks, dils=MRF_STAGE_DILATIONS, slope=0.1, out_div=3.0, post=POST_NONE, act_slope=1.0,
                        out=None, out_act=None, fold=None, guard=None):
    """A whole 16- or 32-channel MRF stage in one launch (fv_mrf_stage_split_f16): y = post(((r0 + r1) + r2) / out_div)
    with r_j = ResBlock1_j(x); ``packed`` from pack_mrf_stage.  ``fold`` = (w [C, 7], bias [1] or None):
    returns post(conv1d(lrelu(y, act_slope); w, padding 3) + bias), [B, 1, T], instead of y.  The 32-channel kernel's
    scratch is allocated here, per call (stream-ordered by the caching allocator)."""
    B, C, T = x.shape
    karr, darr = (ctypes.c_int * 3)(*ks), (ctypes.c_int * 3)(*dils)
    work = mrf_stage_workspace(C, x.device)
    if fold is not None:
        fw, fb = fold
        fw = fw.detach().contiguous().float()
        fb = None if fb is None else fb.detach().contiguous().float()
        res = torch.empty((B, 1, T), dtype=torch.float32, device=x.device)
        with _on(x, packed, fw, fb, res) as stream:
            check(lib().fv_mrf_stage_split_f16(_ptr(x, "x"), _ptr(packed, "packed"), None, None, B, C, T, karr, darr,
                                               float(slope), float(out_div), post, float(act_slope), _ptr(fw, "fold_w"),
                                               _ptr(fb, "fold_b", True), _ptr(res), *_work_args(work), _guard_ptr(guard), stream))
        return res
    if out is None:
        out = torch.empty_like(x)
    with _on(x, packed, out, out_act, work) as stream:
        check(lib().fv_mrf_stage_split_f16(_ptr(x, "x"), _ptr(packed, "packed"), _ptr(out, "y"), _ptr(out_act, "y_act", True),
                                           B, C, T, karr, darr, float(slope), float(out_div), post, float(act_slope), None,
                                           None, None, *_work_args(work), _guard_ptr(guard), stream))
    return out


def mrf_stage_classes_f16(x, packed, ks, dils=MRF_STAGE_DILATIONS, slope=0.1, guard=None, work=None):
    """The 32-channel MRF stage as one launch of two block classes (fv_mrf_stage_classes_f16): returns
    (r_0 + r_1, r_2), un-divided, r_j = ResBlock1_j(x); taps (3, 7, 11) in this order.  ``work``: the scratch
    (mrf_stage_workspace; allocated here when None)."""
    B, C, T = x.shape
    karr, darr = (ctypes.c_int * 3)(*ks), (ctypes.c_int * 3)(*dils)
    if work is None:
        work = mrf_stage_workspace(C, x.device)
    y_s, y_r2 = torch.empty_like(x), torch.empty_like(x)
    with _on(x, packed, y_s, y_r2, work) as stream:
        check(lib().fv_mrf_stage_classes_f16(_ptr(x, "x"), _ptr(packed, "packed"), _ptr(y_s, "y_s"), _ptr(y_r2, "y_r2"), B, C, T,
                                             karr, darr, float(slope), *_work_args(work), _guard_ptr(guard), stream))
    return y_s, y_r2


def mrf_stage_one_class_f16(x, packed, ks, cls, dils=MRF_STAGE_DILATIONS, slope=0.1, work=None):
    """Timing hook (fv_debug_mrf_stage_class_f16): mrf_stage_classes_f16's launch with the blocks of one class alone --
    ``cls`` "a": returns r_2, "b": r_0 + r_1."""
    B, C, T = x.shape
    karr, darr = (ctypes.c_int * 3)(*ks), (ctypes.c_int * 3)(*dils)
    if work is None:
        work = mrf_stage_workspace(C, x.device)
    y = torch.empty_like(x)
    with _on(x, packed, y, work) as stream:
        check(lib().fv_debug_mrf_stage_class_f16(_ptr(x, "x"), _ptr(packed, "packed"), _ptr(y, "y"), {"a": 1, "b": 2}[cls], B, C, T,
                                                 karr, darr, float(slope), *_work_args(work), stream))
    return y


def mrf_stage(xs, w1s, w2s, b1s, b2s, ks, dil, slope, out_div=3.0, post=POST_NONE, act_slope=1.0, out=None,
              out_act=None):
    """y = post(sum_j pair_j(x_j) / out_div): the last pairs of three ResBlocks + the MRF mean (fv_mrf_stage)."""
    B, C, T = xs[0].shape
    if out is None:
        out = torch.empty_like(xs[0])
    with _on(*xs, *w1s, *w2s, *b1s, *b2s, out, out_act) as stream:
        check(lib().fv_mrf_stage(_vp_array(xs, "x"), _vp_array(w1s, "w1"), _vp_array(w2s, "w2"),
                                 _vp_array(b1s, "b1", True), _vp_array(b2s, "b2", True), _ptr(out, "y"),
                                 _ptr(out_act, "y_act", True), (ctypes.c_int * 3)(*ks), B, C, T, dil, float(slope),
                                 float(out_div), post, float(act_slope), stream))
    return out


def conv1d_fused(x, packed, bias, cout, k, dil=1, pad=0, pad_mode=PAD_ZERO, pre_slope=1.0,
                 res=None, acc_in=None, out_div=1.0, post=POST_NONE, out=None, out_act=None,
                 act_slope=1.0, acc_in2=None):
    """One fused conv launch; ``out_act`` (optional) receives lrelu(out, act_slope)."""
    B, cin, T = x.shape
    tout = T if pad_mode & PAD_CAUSAL else T + 2 * pad - dil * (k - 1)
    if out is None:
        out = torch.empty((B, cout, tout), dtype=torch.float32, device=x.device)
    with _on(x, packed, bias, res, acc_in, acc_in2, out, out_act) as stream:
        check(lib().fv_conv1d_fused(_ptr(x, "x"), _ptr(packed, "packed"), _ptr(bias, "bias", True),
                                    _ptr(res, "res", True), _ptr(acc_in, "acc_in", True),
                                    _ptr(acc_in2, "acc_in2", True), _ptr(out, "out"),
                                    _ptr(out_act, "out_act", True), B, cin, cout, T, k, dil, pad, pad_mode,
                                    float(pre_slope), float(out_div), post, float(act_slope), stream))
    return out


def conv1d_2src_fused(x, x2, packed, bias, cout, res=None, post=POST_NONE, out=None, out_act=None,
                      act_slope=1.0):
    """y = post(W1 x + W2 x2 + bias + res) with packed = pack_conv1d(cat([W1, W2], 1)); 1-tap convs."""
    B, c1, T = x.shape
    c2 = x2.shape[1]
    if out is None:
        out = torch.empty((B, cout, T), dtype=torch.float32, device=x.device)
    with _on(x, x2, packed, bias, res, out, out_act) as stream:
        check(lib().fv_conv1d_2src_fused(_ptr(x, "x"), _ptr(x2, "x2"), _ptr(packed, "packed"),
                                         _ptr(bias, "bias", True), _ptr(res, "res", True), _ptr(out, "out"),
                                         _ptr(out_act, "out_act", True), B, c1, c2, cout, T, post,
                                         float(act_slope), stream))
    return out


def conv1x1_2src_split_f16(x, x2, packed, bias, pre_slope=1.0, res=None, post=POST_NONE, out=None, out_act=None,
                           act_slope=1.0, guard=None):
    """y = post(W1 lrelu(x, pre_slope) + W2 x2 + bias + res), split-f16 operands (fv_conv1x1_2src_split_f16);
    packed = pack_conv1x1_2src_split(W1, W2)."""
    B, c, T = x.shape
    if out is None:
        out = torch.empty_like(x)
    with _on(x, x2, packed, bias, res, out, out_act) as stream:
        check(lib().fv_conv1x1_2src_split_f16(_ptr(x, "x"), _ptr(x2, "x2"), _ptr(packed, "packed"), _ptr(bias, "bias", True),
                                              _ptr(res, "res", True), _ptr(out, "out"), _ptr(out_act, "out_act", True), B, c,
                                              T, float(pre_slope), post, float(act_slope), _guard_ptr(guard), stream))
    return out


def conv_transpose1d_fused(x, packed, bias, cout, k, stride, pad, out_pad, pre_slope=1.0,
                           post=POST_NONE, out=None, out_act=None, act_slope=1.0):
    B, cin, T = x.shape
    tout = (T - 1) * stride - 2 * pad + k + out_pad
    if out is None:
        out = torch.empty((B, cout, tout), dtype=torch.float32, device=x.device)
    with _on(x, packed, bias, out, out_act) as stream:
        check(lib().fv_conv_transpose1d_fused(_ptr(x, "x"), _ptr(packed, "packed"),
                                              _ptr(bias, "bias", True), _ptr(out, "out"),
                                              _ptr(out_act, "out_act", True), B, cin, cout, T, k, stride,
                                              pad, out_pad, float(pre_slope), post, float(act_slope),
                                              stream))
    return out


def pack_basis(W):
    """BasisSignalLayer weight W [L, C] (nn.Linear.weight) -> fv_pack_basis image (flat tensor)."""
    L_, c = W.shape
    n = lib().fv_packed_basis_floats(L_, c)
    if n <= 0:
        raise NativeError(f"pack_basis: L={L_} (even, >= 2) C={c}")
    out = torch.empty(n, dtype=torch.float32, device=W.device)
    with _on(W, out) as stream:
        check(lib().fv_pack_basis(_ptr(W, "W"), _ptr(out), L_, c, stream))
    return out


def basis_ola(weight, packed_basis, L_):
    """fv_basis_ola: weight [B, C, F] (channel-major trunk output) -> [B, 1, (F - 1) L/2 + L]."""
    B, c, F = weight.shape
    out = torch.empty((B, 1, (F - 1) * (L_ // 2) + L_), dtype=torch.float32, device=weight.device)
    with _on(weight, packed_basis, out) as stream:
        check(lib().fv_basis_ola(_ptr(weight, "weight"), _ptr(packed_basis, "packed_basis"), _ptr(out), B, c, F, L_, stream))
    return out


def conv_transpose1d_split_f16(x, packed, bias, cout, k, stride, pad, out_pad, pre_slope=1.0, out=None, out_act=None,
                               act_slope=1.0, guard=None):
    """ConvTranspose1d (kernel = 2 stride) with split-f16 operands (fv_conv_transpose1d_split_f16)."""
    B, cin, T = x.shape
    tout = (T - 1) * stride - 2 * pad + k + out_pad
    if out is None:
        out = torch.empty((B, cout, tout), dtype=torch.float32, device=x.device)
    with _on(x, packed, bias, out, out_act) as stream:
        check(lib().fv_conv_transpose1d_split_f16(_ptr(x, "x"), _ptr(packed, "packed"), _ptr(bias, "bias", True),
                                                  _ptr(out, "out"), _ptr(out_act, "out_act", True), B, cin, cout, T, k,
                                                  stride, pad, out_pad, float(pre_slope), float(act_slope),
                                                  _guard_ptr(guard), stream))
    return out


def upsample_conv1d_fused(x, packed, bias, cout, k, rate, pad, pre_slope=1.0, post=POST_NONE,
                          out=None, out_act=None, act_slope=1.0):
    B, cin, T = x.shape
    tout = T * rate + 2 * pad - (k - 1)
    if out is None:
        out = torch.empty((B, cout, tout), dtype=torch.float32, device=x.device)
    with _on(x, packed, bias, out, out_act) as stream:
        check(lib().fv_upsample_conv1d_fused(_ptr(x, "x"), _ptr(packed, "packed"), _ptr(bias, "bias", True),
                                             _ptr(out, "out"), _ptr(out_act, "out_act", True), B, cin, cout,
                                             T, k, rate, pad, float(pre_slope), post, float(act_slope),
                                             stream))
    return out


def encode_16bits(x, rescale_out=1.0, scale_in_place=True):
    """x [n] or [B,n] float32 device tensor -> (int16 tensor of the same shape, peaks [B]).
    Row-wise ``encode_16bits`` of the reference; with ``scale_in_place`` x is scaled like
    the reference scales its argument."""
    flat = x if x.dim() == 2 else x.reshape(1, -1)
    B, n = flat.shape
    out = torch.empty((B, n), dtype=torch.int16, device=x.device)
    peak = torch.empty(B, dtype=torch.float32, device=x.device)
    with _on(flat, out, peak) as stream:
        check(lib().fv_encode_16bits(_ptr(flat, "x"), out.data_ptr(), _ptr(peak), B, n, float(rescale_out),
                                     1 if scale_in_place else 0, stream))
    return out.reshape(x.shape), peak


def pqmf_analysis(x, analysis_filter):
    """x [B,1,T] or [B,T] full band, analysis_filter [S,1,ntaps] -> [B,S,(T-S)//S+1]."""
    S, ntaps = analysis_filter.shape[0], analysis_filter.shape[-1]
    x = x.reshape(x.shape[0], -1)
    B, T = x.shape
    h = analysis_filter.detach().reshape(S, ntaps).contiguous().float()
    y = torch.empty((B, S, (T - S) // S + 1), dtype=torch.float32, device=x.device)
    with _on(x, h, y) as stream:
        check(lib().fv_pqmf_analysis(_ptr(x, "x"), _ptr(h, "analysis_filter"), _ptr(y), B, S, ntaps, T, stream))
    return y


def mel_table_floats():
    """Length of the fp32 table fv_melspectrogram reads (FV_MEL_TABLE_FLOATS)."""
    return lib().fv_mel_table_floats()


def melspectrogram(x, tables, sample_rate=24000, n_fft=2048, hop=240, win_length=1200, n_mels=80, fmin=40.0):
    """x [B,n] fp32 device waveforms -> [B,n_mels,1+n//hop] normalised mel (fv_melspectrogram, one launch on the
    current stream); tables: the fp32 device table of audio.mel_tables (include/fastvocoder_hip.h layout)."""
    if x.dim() != 2:
        raise NativeError(f"melspectrogram: x must be [B, n], got {tuple(x.shape)}")
    B, n = x.shape
    mel = torch.empty((B, n_mels, 1 + n // hop if hop > 0 else 0), dtype=torch.float32, device=x.device)
    if tables.numel() != mel_table_floats():
        raise NativeError(f"melspectrogram: tables hold {tables.numel()} floats, the library reads {mel_table_floats()}")
    with _on(x, tables, mel) as stream:
        check(lib().fv_melspectrogram(_ptr(x, "x"), _ptr(mel), _ptr(tables, "tables"), B, n, int(sample_rate),
                                      int(n_fft), int(hop), int(win_length), int(n_mels), float(fmin), stream))
    return mel


PCM_F32, PCM_S16 = _C["FV_PCM_F32"], _C["FV_PCM_S16"]          # fv_resample's x_format
# fv_resample's limits (FV_RESAMPLE_MAX_*): L and M, floats of the table, floats of a block's input window
RESAMPLE_MAX_FACTOR, RESAMPLE_MAX_TABLE_FLOATS = 1 << 20, 1 << 20      # (expressions in the header: mirrored by hand)
RESAMPLE_MAX_WINDOW = _C["FV_RESAMPLE_MAX_WINDOW"]


def resample(x, table, L, M, half):
    """x [B, n_in] float32 or int16 (PCM, read as s / 32768) device waveforms -> float32 [B, ceil(n_in L / M)]
    (fv_resample, one launch on the current stream); table: the fp32 device table of audio.resample_tables for L / M,
    (2 half + 2) L floats, tap-major."""
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.int16):
        raise NativeError(f"resample: x must be a float32 or int16 [B, n] tensor, got {x.dtype} {tuple(x.shape)}")
    if not x.is_cuda or not x.is_contiguous():
        raise NativeError(f"resample: x must be a contiguous ROCm device tensor (on {x.device}, "
                          f"contiguous={x.is_contiguous()}; there is no CPU path in fastvocoder_amd)")
    if table.numel() != (2 * half + 2) * L:
        raise NativeError(f"resample: the table holds {table.numel()} floats, L={L} half={half} reads {(2 * half + 2) * L}")
    B, n_in = x.shape
    n_out = lib().fv_resample_out_len(n_in, int(L), int(M))
    if n_out < 0:
        check(int(n_out))
    y = torch.empty((B, n_out), dtype=torch.float32, device=x.device)
    with _on(x, table, y) as stream:
        check(lib().fv_resample(x.data_ptr(), PCM_S16 if x.dtype == torch.int16 else PCM_F32, _ptr(y), _ptr(table, "table"),
                                B, n_in, n_out, int(L), int(M), int(half), stream))
    return y


def gl_table_floats():
    """Length of the fp32 table the Griffin-Lim entry points read (FV_GL_TABLE_FLOATS)."""
    return lib().fv_gl_table_floats()


def _gl_tables(tables, who):
    if tables.numel() != gl_table_floats():
        raise NativeError(f"{who}: tables hold {tables.numel()} floats, the library reads {gl_table_floats()}")


def _gl_workspace(B, T, device):
    need = lib().fv_griffin_lim_workspace_bytes(B, T)
    if need < 0:
        check(int(need))
    return torch.empty((need + 3) // 4, dtype=torch.float32, device=device)


def stft_complex(y, tables, n_fft=2048, hop=240, win_length=1200):
    """y [B,n] fp32 device -> complex64 [B, 1+n//hop, n_fft//2+1] (fv_stft, one launch; frames-major)."""
    if y.dim() != 2:
        raise NativeError(f"stft: y must be [B, n], got {tuple(y.shape)}")
    _gl_tables(tables, "stft")
    B, n = y.shape
    spec = torch.empty((B, 1 + n // hop if hop > 0 else 0, n_fft // 2 + 1, 2), dtype=torch.float32, device=y.device)
    with _on(y, tables, spec) as stream:
        check(lib().fv_stft(_ptr(y, "y"), _ptr(spec), _ptr(tables, "tables"), B, n, int(n_fft), int(hop),
                            int(win_length), stream))
    return torch.view_as_complex(spec)


def _complex_floats(z, shape_tail, who):
    """A complex64 (or [..., 2] float32) device tensor as contiguous float32 [..., 2]."""
    if z.is_complex():
        if z.dtype != torch.complex64:
            raise NativeError(f"{who}: expected complex64, got {z.dtype}")
        z = torch.view_as_real(z.contiguous())
    if z.dim() != 4 or z.shape[-1] != 2 or z.shape[2] != shape_tail:
        raise NativeError(f"{who}: expected [B, T, {shape_tail}] complex, got {tuple(z.shape)}")
    return z.contiguous()


def istft(spec, tables, n_fft=2048, hop=240, win_length=1200):
    """spec complex64 [B, T, n_fft//2+1] device (frames-major) -> y [B, hop (T-1)] (fv_istft, two launches)."""
    _gl_tables(tables, "istft")
    spec = _complex_floats(spec, n_fft // 2 + 1, "istft")
    B, T = spec.shape[:2]
    y = torch.empty((B, max(hop * (T - 1), 0)), dtype=torch.float32, device=spec.device)
    ws = _gl_workspace(B, T, spec.device)
    with _on(spec, tables, y, ws) as stream:
        check(lib().fv_istft(_ptr(spec, "spec"), _ptr(y), _ptr(tables, "tables"), B, T, int(n_fft), int(hop),
                             int(win_length), ws.data_ptr(), ws.numel() * 4, stream))
    return y


def griffin_lim(S, phase0, tables, iters, y=None, n_fft=2048, hop=240, win_length=1200):
    """S [B, T, n_fft//2+1] fp32 device magnitudes (frames-major), phase0 complex64 [B, T, n_fft//2+1] initial phases
    -> y [B, hop (T-1)] after ``iters`` projections (fv_griffin_lim: two launches per iteration on the current stream,
    no host synchronisation).  phase0=None: the iterations start from ``y`` (which is not modified)."""
    _gl_tables(tables, "griffin_lim")
    if S.dim() != 3 or S.shape[2] != n_fft // 2 + 1:
        raise NativeError(f"griffin_lim: S must be [B, T, {n_fft // 2 + 1}], got {tuple(S.shape)}")
    B, T = S.shape[:2]
    if phase0 is not None:
        phase0 = _complex_floats(phase0, n_fft // 2 + 1, "griffin_lim")
        if tuple(phase0.shape[:2]) != (B, T):
            raise NativeError(f"griffin_lim: phase0 is {tuple(phase0.shape[:3])}, S is {tuple(S.shape)}")
        y = torch.empty((B, max(hop * (T - 1), 0)), dtype=torch.float32, device=S.device)
    else:
        if y is None or tuple(y.shape) != (B, hop * (T - 1)):
            raise NativeError(f"griffin_lim: without phase0 a starting y [B, {hop * (T - 1)}] is needed")
        y = y.clone().contiguous()
    ws = _gl_workspace(B, T, S.device)
    with _on(S, tables, y, ws, *([] if phase0 is None else [phase0])) as stream:
        check(lib().fv_griffin_lim(_ptr(S, "S"), _ptr(phase0, "phase0", True), _ptr(y, "y"), _ptr(tables, "tables"),
                                   B, T, int(iters), int(n_fft), int(hop), int(win_length), ws.data_ptr(),
                                   ws.numel() * 4, stream))
    return y


def mel_to_linear(mel, inv_basis, power):
    """mel [B,80,T] fp32 device (normalised), inv_basis [80,1025] fp32 device -> S [B,T,1025] (fv_mel_to_linear)."""
    if mel.dim() != 3 or inv_basis.dim() != 2 or mel.shape[1] != inv_basis.shape[0]:
        raise NativeError(f"mel_to_linear: mel [B, n_mels, T] and inv_basis [n_mels, n_freq], got {tuple(mel.shape)} "
                          f"and {tuple(inv_basis.shape)}")
    B, n_mels, T = mel.shape
    n_freq = inv_basis.shape[1]
    S = torch.empty((B, T, n_freq), dtype=torch.float32, device=mel.device)
    with _on(mel, inv_basis, S) as stream:
        check(lib().fv_mel_to_linear(_ptr(mel, "mel"), _ptr(inv_basis, "inv_basis"), _ptr(S), B, T, n_mels, n_freq,
                                     float(power), stream))
    return S


def inv_preemphasis(y, coef):
    """y [B,n] fp32 device -> out[b,i] = y[b,i] + coef out[b,i-1] (fv_inv_preemphasis, one launch)."""
    if y.dim() != 2:
        raise NativeError(f"inv_preemphasis: y must be [B, n], got {tuple(y.shape)}")
    out = torch.empty_like(y)
    with _on(y, out) as stream:
        check(lib().fv_inv_preemphasis(_ptr(y, "y"), _ptr(out), y.shape[0], y.shape[1], float(coef), stream))
    return out


def stft_table_floats(n_fft, win_length):
    """Length of the fp32 table fv_stft_magnitude / fv_stft_distance read for one resolution."""
    rc = lib().fv_stft_table_floats(int(n_fft), int(win_length))
    if rc < 0:
        check(rc)
    return rc


def stft_magnitude(x, table, n_fft, hop, win_length):
    """x [B,n] fp32 device -> |STFT| [B, 1+n//hop, n_fft//2+1] (fv_stft_magnitude, one launch on the current
    stream); table: the fp32 device table of loss.stft_tables (include/fastvocoder_hip.h layout)."""
    if x.dim() != 2:
        raise NativeError(f"stft_magnitude: x must be [B, n], got {tuple(x.shape)}")
    B, n = x.shape
    if table.numel() != stft_table_floats(n_fft, win_length):
        raise NativeError(f"stft_magnitude: table holds {table.numel()} floats, the library reads "
                          f"{stft_table_floats(n_fft, win_length)}")
    mag = torch.empty((B, 1 + n // hop if hop > 0 else 0, n_fft // 2 + 1), dtype=torch.float32, device=x.device)
    with _on(x, table, mag) as stream:
        check(lib().fv_stft_magnitude(_ptr(x, "x"), _ptr(mag), _ptr(table, "table"), B, n, int(n_fft), int(hop),
                                      int(win_length), stream))
    return mag


def stft_distance(x, y, tables, n_ffts, hops, win_lengths):
    """x, y [B,n] fp32 device -> float64 [R,B,3] partial sums (S_diff, S_ref, S_log) per resolution and row
    (fv_stft_distance: two launches on the current stream, the workspace from torch's allocator)."""
    if x.dim() != 2 or x.shape != y.shape:
        raise NativeError(f"stft_distance: x and y must both be [B, n], got {tuple(x.shape)} and {tuple(y.shape)}")
    B, n = x.shape
    R = len(tables)
    if not (len(n_ffts) == len(hops) == len(win_lengths) == R):
        raise NativeError("stft_distance: one table, n_fft, hop and win_length per resolution")
    for t, nf, wl in zip(tables, n_ffts, win_lengths):
        if t.numel() != stft_table_floats(nf, wl):
            raise NativeError(f"stft_distance: a table holds {t.numel()} floats, the library reads "
                              f"{stft_table_floats(nf, wl)}")
    ia = ctypes.c_int * R
    nf_a, hop_a, wl_a = ia(*map(int, n_ffts)), ia(*map(int, hops)), ia(*map(int, win_lengths))
    need = lib().fv_stft_distance_workspace_bytes(B, n, R, nf_a, hop_a)
    if need < 0:
        check(int(need))
    out = torch.empty((R, B, 3), dtype=torch.float64, device=x.device)
    ws = torch.empty((max(need, 8) + 7) // 8, dtype=torch.float64, device=x.device)
    with _on(x, y, out, ws, *tables) as stream:
        tab_a = (ctypes.c_void_p * R)(*[_ptr(t, "table") for t in tables])
        check(lib().fv_stft_distance(_ptr(x, "x"), _ptr(y, "y"), tab_a, B, n, R, nf_a, hop_a, wl_a, out.data_ptr(),
                                     ws.data_ptr(), ws.numel() * 8, stream))
    return out


def stft_distance_grad(x, y, tables, n_ffts, hops, win_lengths, coef):
    """x, y [B,n] fp32 device, coef [R,B,2] fp32 (dL/dS_diff, dL/dS_log per resolution and row) -> dL/dx [B,n] fp32
    (fv_stft_distance_grad: two launches on the current stream, the frames workspace from torch's allocator)."""
    if x.dim() != 2 or x.shape != y.shape:
        raise NativeError(f"stft_distance_grad: x and y must both be [B, n], got {tuple(x.shape)} and "
                          f"{tuple(y.shape)}")
    B, n = x.shape
    R = len(tables)
    if not (len(n_ffts) == len(hops) == len(win_lengths) == R):
        raise NativeError("stft_distance_grad: one table, n_fft, hop and win_length per resolution")
    if tuple(coef.shape) != (R, B, 2):
        raise NativeError(f"stft_distance_grad: coef must be [R, B, 2] = {(R, B, 2)}, got {tuple(coef.shape)}")
    for t, nf, wl in zip(tables, n_ffts, win_lengths):
        if t.numel() != stft_table_floats(nf, wl):
            raise NativeError(f"stft_distance_grad: a table holds {t.numel()} floats, the library reads "
                              f"{stft_table_floats(nf, wl)}")
    ia = ctypes.c_int * R
    nf_a, hop_a, wl_a = ia(*map(int, n_ffts)), ia(*map(int, hops)), ia(*map(int, win_lengths))
    need = lib().fv_stft_distance_grad_workspace_bytes(B, n, R, nf_a, hop_a, wl_a)
    if need < 0:
        check(int(need))
    gx = torch.empty((B, n), dtype=torch.float32, device=x.device)
    ws = torch.empty((max(need, 4) + 3) // 4, dtype=torch.float32, device=x.device)
    with _on(x, y, coef, gx, ws, *tables) as stream:
        tab_a = (ctypes.c_void_p * R)(*[_ptr(t, "table") for t in tables])
        check(lib().fv_stft_distance_grad(_ptr(x, "x"), _ptr(y, "y"), tab_a, B, n, R, nf_a, hop_a, wl_a,
                                          _ptr(coef, "coef"), _ptr(gx), ws.data_ptr(), ws.numel() * 4, stream))
    return gx


def stft_magnitude_bins(x, table, n_fft, hop, win_length):
    """x [B,n] fp32 device -> |STFT| [B, n_fft//2+1, 1+n//hop], bins-major (fv_stft_magnitude_bins, one launch): the
    transpose of stft_magnitude's result, bit for bit."""
    if x.dim() != 2:
        raise NativeError(f"stft_magnitude_bins: x must be [B, n], got {tuple(x.shape)}")
    B, n = x.shape
    if table.numel() != stft_table_floats(n_fft, win_length):
        raise NativeError(f"stft_magnitude_bins: table holds {table.numel()} floats, the library reads "
                          f"{stft_table_floats(n_fft, win_length)}")
    mag = torch.empty((B, n_fft // 2 + 1, 1 + n // hop if hop > 0 else 0), dtype=torch.float32, device=x.device)
    with _on(x, table, mag) as stream:
        check(lib().fv_stft_magnitude_bins(_ptr(x, "x"), _ptr(mag), _ptr(table, "table"), B, n, int(n_fft), int(hop),
                                           int(win_length), stream))
    return mag


def stft_magnitude_bins_grad(x, gmag, table, n_fft, hop, win_length):
    """x [B,n], gmag = dL/dmag [B, n_fft//2+1, 1+n//hop] fp32 device -> dL/dx [B,n] fp32, the adjoint of
    stft_magnitude_bins (fv_stft_magnitude_bins_grad: two launches on the current stream, the frames workspace from
    torch's allocator)."""
    if x.dim() != 2:
        raise NativeError(f"stft_magnitude_bins_grad: x must be [B, n], got {tuple(x.shape)}")
    B, n = x.shape
    want = (B, n_fft // 2 + 1, 1 + n // hop if hop > 0 else 0)
    if tuple(gmag.shape) != want:
        raise NativeError(f"stft_magnitude_bins_grad: gmag must be [B, bins, frames] = {want}, got "
                          f"{tuple(gmag.shape)}")
    if table.numel() != stft_table_floats(n_fft, win_length):
        raise NativeError(f"stft_magnitude_bins_grad: table holds {table.numel()} floats, the library reads "
                          f"{stft_table_floats(n_fft, win_length)}")
    need = lib().fv_stft_magnitude_bins_grad_workspace_bytes(B, n, int(n_fft), int(hop), int(win_length))
    if need < 0:
        check(int(need))
    gx = torch.empty((B, n), dtype=torch.float32, device=x.device)
    ws = torch.empty((max(need, 4) + 3) // 4, dtype=torch.float32, device=x.device)
    with _on(x, gmag, table, gx, ws) as stream:
        check(lib().fv_stft_magnitude_bins_grad(_ptr(x, "x"), _ptr(gmag, "gmag"), _ptr(table, "table"), B, n,
                                                int(n_fft), int(hop), int(win_length), _ptr(gx), ws.data_ptr(),
                                                ws.numel() * 4, stream))
    return gx


def grouped_conv1d(x, w, bias, k, stride, pad, slope=1.0, out=None):
    """x [B,Cin,Tin], w [Cout,4,k] folded weight (groups = Cin/4), bias [Cout] or None -> lrelu(conv, slope)
    [B,Cout,(Tin+2pad-k)//stride+1] (fv_grouped_conv1d, one launch)."""
    if x.dim() != 3 or w.dim() != 3:
        raise NativeError(f"grouped_conv1d: x [B,Cin,T] and w [Cout,4,k], got {tuple(x.shape)} and {tuple(w.shape)}")
    B, cin, T = x.shape
    cout = w.shape[0]
    if w.shape[1:] != (4, k):
        raise NativeError(f"grouped_conv1d: w must be [Cout, 4, {k}], got {tuple(w.shape)}")
    tout = (T + 2 * pad - k) // stride + 1 if stride > 0 else 0
    if out is None:
        out = torch.empty((B, cout, max(tout, 0)), dtype=torch.float32, device=x.device)
    with _on(x, w, bias, out) as stream:
        check(lib().fv_grouped_conv1d(_ptr(x, "x"), _ptr(w, "w"), _ptr(bias, "bias", True), _ptr(out, "out"), B, cin,
                                      cout, T, int(k), int(stride), int(pad), float(slope), stream))
    return out


def avg_pool1d(x, k, stride, pad):
    """x [..., Tin] fp32 device -> AvgPool1d(k, stride, pad, count_include_pad=False) [..., Tout] (fv_avg_pool1d)."""
    tin = x.shape[-1]
    rows = x.numel() // tin if tin else 0
    tout = (tin + 2 * pad - k) // stride + 1 if stride > 0 else 0
    out = torch.empty(tuple(x.shape[:-1]) + (max(tout, 0),), dtype=torch.float32, device=x.device)
    with _on(x, out) as stream:
        check(lib().fv_avg_pool1d(_ptr(x, "x"), _ptr(out), rows, tin, int(k), int(stride), int(pad), stream))
    return out


def mpd_reflect_tail(T, period):
    """Samples DiscriminatorP's reflect pad appends to T (mpd.py:150-153)."""
    return period - T % period if T % period else 0


def mpd_conv_first(x, w, bias, period, slope=0.1):
    """x [B,1,T] waveform, w [32,5] folded weight, bias [32] or None -> lrelu(conv, slope) [B,32,H',period]: the
    reflect tail pad, the [H, period] view and DiscriminatorP's first conv (fv_mpd_conv_first, one launch)."""
    if x.dim() != 3 or x.shape[1] != 1 or tuple(w.shape) != (32, 5):
        raise NativeError(f"mpd_conv_first: x [B,1,T] and w [32,5], got {tuple(x.shape)} and {tuple(w.shape)}")
    B, _, T = x.shape
    H = (T + mpd_reflect_tail(T, period)) // period if period > 0 else 0
    out = torch.empty((B, 32, max((H - 1) // 3 + 1, 0), max(period, 0)), dtype=torch.float32, device=x.device)
    with _on(x, w, bias, out) as stream:
        check(lib().fv_mpd_conv_first(_ptr(x, "x"), _ptr(w, "w"), _ptr(bias, "bias", True), _ptr(out, "out"), B, T,
                                      int(period), float(slope), stream))
    return out


def pack_period_conv(w):
    """Folded weight [Cout,Cin,5] of a strided period conv -> the image fv_period_conv reads (flat tensor)."""
    w = w.detach().contiguous().float()
    if w.dim() != 3 or w.shape[2] != 5:
        raise NativeError(f"pack_period_conv: w must be [Cout, Cin, 5], got {tuple(w.shape)}")
    cout, cin, _ = w.shape
    out = torch.empty(max(lib().fv_packed_period_conv_floats(cout, cin), 1), dtype=torch.float32, device=w.device)
    with _on(w) as stream:
        check(lib().fv_pack_period_conv(_ptr(w, "w"), _ptr(out), cout, cin, stream))
    return out


def period_conv(x, packed, bias, cout, slope=0.1):
    """x [B,Cin,H,p] -> lrelu(Conv2d(Cin, cout, (5,1), (3,1), padding (2,0)), slope) [B,cout,(H-1)//3+1,p]
    (fv_period_conv, one launch on the fp32 matrix cores); packed = pack_period_conv(w)."""
    if x.dim() != 4:
        raise NativeError(f"period_conv: x must be [B,Cin,H,p], got {tuple(x.shape)}")
    B, cin, H, p = x.shape
    out = torch.empty((B, cout, (H - 1) // 3 + 1 if H > 0 else 0, p), dtype=torch.float32, device=x.device)
    with _on(x, packed, bias, out) as stream:
        check(lib().fv_period_conv(_ptr(x, "x"), _ptr(packed, "packed"), _ptr(bias, "bias", True), _ptr(out, "out"),
                                   B, cin, int(cout), H, p, float(slope), stream))
    return out


def pack_period_conv_grad(w):
    """Folded weight [Cout,Cin,5] of a strided period conv -> the image fv_period_conv_input_grad reads (flat
    tensor)."""
    w = w.detach().contiguous().float()
    if w.dim() != 3 or w.shape[2] != 5:
        raise NativeError(f"pack_period_conv_grad: w must be [Cout, Cin, 5], got {tuple(w.shape)}")
    cout, cin, _ = w.shape
    out = torch.empty(max(lib().fv_packed_period_conv_grad_floats(cout, cin), 1), dtype=torch.float32,
                      device=w.device)
    with _on(w) as stream:
        check(lib().fv_pack_period_conv_grad(_ptr(w, "w"), _ptr(out), cout, cin, stream))
    return out


def _grad_like(name, g_up, g_map, y, dims=None):
    """The first of g_up / g_map that is given, after the check every input-gradient wrapper makes: at least one of
    the two is given (with ``dims`` dimensions where the wrapper names a rank), and g_up / g_map / y have one shape."""
    like = g_up if g_up is not None else g_map
    if like is None:
        raise NativeError(f"{name}: g_up and g_map are both None")
    if dims is not None and like.dim() != dims:
        raise NativeError(f"{name}: a gradient of {dims} dimensions expected, got {tuple(like.shape)}")
    for t in (g_up, g_map, y):
        if t is not None and t.shape != like.shape:
            raise NativeError(f"{name}: shapes {tuple(t.shape)} and {tuple(like.shape)} differ")
    return like


def period_conv_input_grad(g_up, g_map, y, packed, cin, H, slope=0.1):
    """The gradient of period_conv with respect to its input x [B,cin,H,p] (fv_period_conv_input_grad, one launch on
    the fp32 matrix cores): g_up / g_map / y [B,Cout,(H-1)//3+1,p] as disc_map_grad takes them (the mask is applied
    while the gradient is staged), packed = pack_period_conv_grad(w) -> dx [B,cin,H,p]."""
    like = _grad_like("period_conv_input_grad", g_up, g_map, y, 4)
    B, cout, hout, p = like.shape
    if H < 1 or hout != (H - 1) // 3 + 1:
        raise NativeError(f"period_conv_input_grad: {hout} output rows do not belong to an input of {H} rows")
    dx = torch.empty((B, int(cin), int(H), p), dtype=torch.float32, device=like.device)
    with _on(g_up, g_map, y, packed, dx) as stream:
        check(lib().fv_period_conv_input_grad(_ptr(g_up, "g_up", True), _ptr(g_map, "g_map", True),
                                              _ptr(y, "y", True), _ptr(packed, "packed"), _ptr(dx), B, int(cin), cout,
                                              int(H), p, float(slope), stream))
    return dx


def mpd_first_input_grad(g_up, g_map, y0, w, T, slope=0.1):
    """The gradient of mpd_conv_first with respect to the waveform x [B,1,T] (fv_mpd_first_input_grad, one launch):
    g_up / g_map / y0 [B,32,H1,p] as disc_map_grad takes them, w [32,5] the folded weight -> dx [B,1,T], the adjoint
    of the reflect tail folded in."""
    like = _grad_like("mpd_first_input_grad", g_up, g_map, y0, 4)
    B, c, h1, p = like.shape
    H = (T + mpd_reflect_tail(T, p)) // p if p > 0 else 0
    if c != 32 or tuple(w.shape) != (32, 5) or T < 1 or h1 != (H - 1) // 3 + 1:
        raise NativeError(f"mpd_first_input_grad: a gradient [B,32,H1,p] of a waveform of {T} samples and w [32,5] "
                          f"expected, got {tuple(like.shape)} and {tuple(w.shape)}")
    dx = torch.empty((B, 1, int(T)), dtype=torch.float32, device=like.device)
    with _on(g_up, g_map, y0, w, dx) as stream:
        check(lib().fv_mpd_first_input_grad(_ptr(g_up, "g_up", True), _ptr(g_map, "g_map", True),
                                            _ptr(y0, "y0", True), _ptr(w, "w"), _ptr(dx), B, int(T), p, float(slope),
                                            stream))
    return dx


DISC_MAX_MAPS = _C["FV_DISC_MAX_MAPS"]      # maps per fv_disc_score_sums call


def disc_score_sums(es, rs):
    """Lists of M map pairs, each e_m and r_m fp32 device [B, ...] of one shape -> float64 [M, B, 4]:
    sum|e-r|, sum(e-1)^2, sum e^2, sum(r-1)^2 per map and row (fv_disc_score_sums: two launches per DISC_MAX_MAPS
    maps; a map's sums do not depend on which other maps share its call)."""
    if len(es) == len(rs) and len(es) > DISC_MAX_MAPS:
        return torch.cat([disc_score_sums(es[i:i + DISC_MAX_MAPS], rs[i:i + DISC_MAX_MAPS])
                          for i in range(0, len(es), DISC_MAX_MAPS)])
    M = len(es)
    if M != len(rs) or M == 0:
        raise NativeError(f"disc_score_sums: {len(es)} estimate maps and {len(rs)} real maps")
    B = es[0].shape[0]
    for e, r in zip(es, rs):
        if e.shape != r.shape or e.shape[0] != B:
            raise NativeError(f"disc_score_sums: map shapes {tuple(e.shape)} and {tuple(r.shape)} (batch {B})")
    n = (ctypes.c_int64 * M)(*[e[0].numel() for e in es])
    need = lib().fv_disc_score_workspace_bytes(B, M, n)
    if need < 0:
        check(int(need))
    dev = es[0].device
    out = torch.empty((M, B, 4), dtype=torch.float64, device=dev)
    ws = torch.empty((max(need, 8) + 7) // 8, dtype=torch.float64, device=dev)
    with _on(out, ws, *es, *rs) as stream:
        e_a = (ctypes.c_void_p * M)(*[_ptr(e, "e") for e in es])
        r_a = (ctypes.c_void_p * M)(*[_ptr(r, "r") for r in rs])
        check(lib().fv_disc_score_sums(e_a, r_a, n, M, B, out.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream))
    return out


def disc_map_grad(g_up, g_map, y, slope=1.0):
    """(g_up + g_map) * (y > 0 ? 1 : slope), elementwise (fv_disc_map_grad, one launch): the gradient in front of a
    layer's LeakyReLU.  g_up or g_map may be None; y (the layer's output) may be None when slope is 1."""
    like = _grad_like("disc_map_grad", g_up, g_map, y)
    out = torch.empty_like(like)
    with _on(g_up, g_map, y, out) as stream:
        check(lib().fv_disc_map_grad(_ptr(g_up, "g_up", True), _ptr(g_map, "g_map", True), _ptr(y, "y", True),
                                     _ptr(out), like.numel(), float(slope), stream))
    return out


def grouped_conv1d_input_grad(g_up, g_map, y, w, cin, tin, k, stride, pad, slope=1.0):
    """The gradient of grouped_conv1d with respect to its input x [B, cin, tin] (fv_grouped_conv1d_input_grad, one
    launch): g_up / g_map / y [B,Cout,Tout] as disc_map_grad takes them (the mask is applied while the gradient is
    staged), w [Cout,4,k] the forward's weight -> dx [B, cin, tin]."""
    like = _grad_like("grouped_conv1d_input_grad", g_up, g_map, y, 3)
    if w.dim() != 3 or w.shape[1:] != (4, k) or w.shape[0] != like.shape[1]:
        raise NativeError(f"grouped_conv1d_input_grad: a gradient [B,Cout,Tout] and w [Cout,4,{k}] expected, got "
                          f"{tuple(like.shape)} and {tuple(w.shape)}")
    B, cout, tout = like.shape
    if stride > 0 and tin + 2 * pad >= k and tout != (tin + 2 * pad - k) // stride + 1:
        raise NativeError(f"grouped_conv1d_input_grad: {tout} output times do not belong to an input of {tin} samples")
    dx = torch.empty((B, int(cin), max(int(tin), 0)), dtype=torch.float32, device=like.device)
    with _on(g_up, g_map, y, w, dx) as stream:
        check(lib().fv_grouped_conv1d_input_grad(_ptr(g_up, "g_up", True), _ptr(g_map, "g_map", True),
                                                 _ptr(y, "y", True), _ptr(w, "w"), _ptr(dx), B, int(cin), cout,
                                                 int(tin), int(k), int(stride), int(pad), float(slope), stream))
    return dx


def _workspace_floats(need):
    """fp32 words of a workspace of ``need`` bytes as a *_workspace_bytes entry returns them (negative: its refusal)."""
    if need < 0:
        check(int(need))
    return (need + 3) // 4


def _weight_grad_call(name, entry, inputs, want_dw, want_db, dw_shape, db_shape, args, workspace, floats):
    """What the weight-gradient wrappers share once their shapes are checked: ``inputs`` the (name, tensor) of the
    gradient and of the layer's input, ``floats()`` the size of the fresh workspace when none is given, and the call
    ``entry(g, x, dw, db, *args, workspace, bytes, stream)`` -> (dw or None, db or None)."""
    if not (want_dw or want_db):
        raise NativeError(f"{name}: neither the weight nor the bias gradient is asked for")
    dev = inputs[0][1].device
    if workspace is None:
        workspace = torch.empty(floats(), dtype=torch.float32, device=dev)
    dw = torch.empty(dw_shape, dtype=torch.float32, device=dev) if want_dw else None
    db = torch.empty(db_shape, dtype=torch.float32, device=dev) if want_db else None
    with _on(*(t for _, t in inputs), workspace, dw, db) as stream:
        check(getattr(lib(), entry)(*(_ptr(t, n) for n, t in inputs), _ptr(dw, "dw", True), _ptr(db, "db", True), *args,
                                    _ptr(workspace, "workspace"), workspace.numel() * 4, stream))
    return dw, db


def conv_weight_grad_workspace_floats(grouped, B, cin, cout, tin, k, stride=1, pad=0, pad_mode=PAD_ZERO):
    """fp32 words of workspace conv1d_weight_grad (``grouped`` False) or grouped_conv1d_weight_grad needs for these
    shapes (fv_conv_weight_grad_workspace_bytes); raises for shapes the entries refuse."""
    return _workspace_floats(lib().fv_conv_weight_grad_workspace_bytes(
        int(bool(grouped)), int(B), int(cin), int(cout), int(tin), int(k), int(stride), int(pad), int(pad_mode)))


def _weight_grad(name, grouped, g_pre, x, k, stride, pad, pad_mode, want_dw, want_db, workspace):
    """What conv1d_weight_grad and grouped_conv1d_weight_grad share: the shape checks, the workspace and the call."""
    if g_pre.dim() != 3 or x.dim() != 3 or g_pre.shape[0] != x.shape[0]:
        raise NativeError(f"{name}: g_pre [B,Cout,Tout] and x [B,Cin,Tin] expected, got {tuple(g_pre.shape)} and "
                          f"{tuple(x.shape)}")
    B, cout, tout = g_pre.shape
    cin, tin = x.shape[1], x.shape[2]
    k, stride, pad = int(k), int(stride), int(pad)
    if stride > 0 and tin + 2 * pad >= k and tout != (tin + 2 * pad - k) // stride + 1:
        raise NativeError(f"{name}: {tout} output times do not belong to an input of {tin} samples")
    return _weight_grad_call(
        name, "fv_grouped_conv1d_weight_grad" if grouped else "fv_conv1d_weight_grad", (("g_pre", g_pre), ("x", x)),
        want_dw, want_db, (cout, 4 if grouped else cin, k), (cout,),
        (B, cin, cout, tin, k, stride, pad) if grouped else (B, cin, cout, tin, k, pad, int(pad_mode)), workspace,
        lambda: conv_weight_grad_workspace_floats(grouped, B, cin, cout, tin, k, stride, pad, pad_mode))


def conv1d_weight_grad(g_pre, x, k, pad=0, pad_mode=PAD_ZERO, want_dw=True, want_db=False, workspace=None):
    """The weight (and bias) gradient of a dense stride-1 conv (fv_conv1d_weight_grad, two launches): g_pre
    [B,Cout,Tout] the gradient in front of the LeakyReLU (disc_map_grad), x [B,Cin,Tin] the layer's input, padded by
    indexing -> (dw [Cout,Cin,k] or None, db [Cout] or None).  ``workspace``: an fp32 device tensor to use instead
    of a fresh one (its contents do not matter)."""
    return _weight_grad("conv1d_weight_grad", False, g_pre, x, k, 1, pad, pad_mode, want_dw, want_db, workspace)


def grouped_conv1d_weight_grad(g_pre, x, k, stride, pad, want_dw=True, want_db=False, workspace=None):
    """The weight (and bias) gradient of grouped_conv1d (fv_grouped_conv1d_weight_grad, two launches): g_pre
    [B,Cout,Tout], x [B,Cin,Tin] -> (dw [Cout,4,k] or None, db [Cout] or None)."""
    return _weight_grad("grouped_conv1d_weight_grad", True, g_pre, x, k, stride, pad, PAD_ZERO, want_dw, want_db,
                        workspace)


PERIOD_WGRAD_UNIT = 32       # flat positions h' p + c per unit of period_wgrad_mfma_kernel (csrc/mpd_wgrad.hip kPwTK)
PERIOD_WGRAD_CHUNK = 1024    # ... of its plain path and of the first layer's kernel (kPwChunk)


def period_conv_weight_grad_workspace_floats(B, cin, cout, H, period, k, stride, precision="f32"):
    """fp32 words of workspace period_conv_weight_grad needs for these shapes
    (fv_period_conv_weight_grad_workspace_bytes; with ``precision="bf16"``
    fv_period_conv_weight_grad_bf16_workspace_bytes); raises for shapes the entry refuses."""
    bf16 = _grad_precision("period_conv_weight_grad_workspace_floats", precision) == "bf16"
    entry = "fv_period_conv_weight_grad_bf16_workspace_bytes" if bf16 else "fv_period_conv_weight_grad_workspace_bytes"
    return _workspace_floats(getattr(lib(), entry)(
        int(B), int(cin), int(cout), int(H), int(period), int(k), int(stride)))


def period_conv_weight_grad(g_pre, x, k, stride, want_dw=True, want_db=False, workspace=None, precision="f32"):
    """The weight (and bias) gradient of a (k, 1) conv along H with zero padding (k - 1) // 2
    (fv_period_conv_weight_grad, two launches): g_pre [B,Cout,(H-1)//stride+1,p] the gradient in front of the
    LeakyReLU, x [B,Cin,H,p] the layer's input -> (dw [Cout,Cin,k] or None, db [Cout] or None).  ``workspace``: an
    fp32 device tensor to use instead of a fresh one (its contents do not matter).  ``precision="bf16"``
    (fv_period_conv_weight_grad_bf16): dw from the operands rounded to bf16 (nearest even) with fp32 accumulation, db
    from the un-rounded g_pre; stride 1 for every shape, stride 2 and 3 for Cout >= 64 with Cin k >= 64."""
    _grad_precision("period_conv_weight_grad", precision)
    if g_pre.dim() != 4 or x.dim() != 4 or g_pre.shape[0] != x.shape[0] or g_pre.shape[3] != x.shape[3]:
        raise NativeError(f"period_conv_weight_grad: g_pre [B,Cout,H',p] and x [B,Cin,H,p] expected, got "
                          f"{tuple(g_pre.shape)} and {tuple(x.shape)}")
    B, cout, hout, p = g_pre.shape
    cin, H = x.shape[1], x.shape[2]
    k, stride = int(k), int(stride)
    if stride > 0 and H > 0 and hout != (H - 1) // stride + 1:
        raise NativeError(f"period_conv_weight_grad: {hout} output rows do not belong to an input of {H} rows")
    return _weight_grad_call(
        "period_conv_weight_grad",
        "fv_period_conv_weight_grad_bf16" if precision == "bf16" else "fv_period_conv_weight_grad",
        (("g_pre", g_pre), ("x", x)), want_dw, want_db, (cout, cin, k), (cout,), (B, cin, cout, H, p, k, stride),
        workspace, lambda: period_conv_weight_grad_workspace_floats(B, cin, cout, H, p, k, stride, precision))


def mpd_first_weight_grad(g_pre, x, want_dw=True, want_db=False, workspace=None):
    """The weight (and bias) gradient of mpd_conv_first (fv_mpd_first_weight_grad, two launches): g_pre [B,32,H1,p],
    x [B,1,T] the waveform -> (dw [32,5] or None, db [32] or None)."""
    if g_pre.dim() != 4 or g_pre.shape[1] != 32 or x.dim() != 3 or x.shape[1] != 1 or x.shape[0] != g_pre.shape[0]:
        raise NativeError(f"mpd_first_weight_grad: g_pre [B,32,H1,p] and x [B,1,T] expected, got "
                          f"{tuple(g_pre.shape)} and {tuple(x.shape)}")
    B, _, h1, p = g_pre.shape
    T = x.shape[2]
    H = (T + mpd_reflect_tail(T, p)) // p if p > 0 else 0
    if T < 1 or h1 != (H - 1) // 3 + 1:
        raise NativeError(f"mpd_first_weight_grad: {h1} output rows do not belong to a waveform of {T} samples")
    return _weight_grad_call(
        "mpd_first_weight_grad", "fv_mpd_first_weight_grad", (("g_pre", g_pre), ("x", x)), want_dw, want_db, (32, 5),
        (32,), (B, T, p), workspace, lambda: _workspace_floats(lib().fv_mpd_first_weight_grad_workspace_bytes(B, T, p)))


def weight_norm_grad(dw, v, g, want_dv=True, want_dg=True):
    """The adjoint of fold_weight_norm (fv_weight_norm_grad, one launch): dw and v of one shape [dim0, ...], g with
    dim0 elements -> (dv like v or None, dg like g or None)."""
    if dw.shape != v.shape or v.dim() < 1 or g.numel() != v.shape[0] or not (want_dv or want_dg):
        raise NativeError(f"weight_norm_grad: dw {tuple(dw.shape)}, v {tuple(v.shape)}, g {tuple(g.shape)}")
    dv = torch.empty_like(v) if want_dv else None
    dg = torch.empty_like(g) if want_dg else None
    with _on(dw, v, g, dv, dg) as stream:
        check(lib().fv_weight_norm_grad(_ptr(dw, "dw"), _ptr(v, "v"), _ptr(g, "g"), _ptr(dv, "dv", True),
                                        _ptr(dg, "dg", True), v.shape[0], v[0].numel(), stream))
    return dv, dg


# ---------------------------------------------------------------------------
# the generators' parameter gradient (csrc/gen_grad.hip)
# ---------------------------------------------------------------------------

GRAD_PRECISIONS = ("f32", "bf16")   # arithmetic of the generators' and the MPD's weight gradients (csrc/gen_grad_bf16.hip)


def _grad_precision(name, precision):
    if precision not in GRAD_PRECISIONS:
        raise NativeError(f"{name}: precision {precision!r} ('f32' or 'bf16')")
    return precision


def conv1d_weight_grad_dilated_workspace_floats(B, cin, cout, tin, k, dil=1, pad=0, pad_mode=None, precision="f32"):
    """fp32 words of workspace conv1d_weight_grad_dilated needs for these shapes
    (fv_conv1d_weight_grad_dilated_workspace_bytes; with a ``pad_mode`` fv_conv1d_weight_grad_dilated_mode_workspace_bytes;
    with ``precision="bf16"`` fv_conv1d_weight_grad_dilated_bf16_workspace_bytes); raises for shapes the entry refuses."""
    args = (int(B), int(cin), int(cout), int(tin), int(k), int(dil), int(pad))
    if _grad_precision("conv1d_weight_grad_dilated_workspace_floats", precision) == "bf16":
        return _workspace_floats(lib().fv_conv1d_weight_grad_dilated_bf16_workspace_bytes(
            *args, PAD_ZERO if pad_mode is None else int(pad_mode)))
    if pad_mode is None:
        return _workspace_floats(lib().fv_conv1d_weight_grad_dilated_workspace_bytes(*args))
    return _workspace_floats(lib().fv_conv1d_weight_grad_dilated_mode_workspace_bytes(*args, int(pad_mode)))


def conv1d_weight_grad_dilated(g_pre, xa, k, dil=1, pad=0, want_dw=True, want_db=False, workspace=None, pad_mode=None,
                               precision="f32"):
    """The weight (and bias) gradient of a dense stride-1 dilated conv with zero padding
    (fv_conv1d_weight_grad_dilated, two launches): g_pre [B,Cout,Tout], xa [B,Cin,Tin] the conv's input as it saw it
    -> (dw [Cout,Cin,k] or None, db [Cout] or None).  ``workspace``: an fp32 device tensor to use instead of a fresh
    one (its contents do not matter).  ``pad_mode`` PAD_ZERO or PAD_REFLECT goes through
    fv_conv1d_weight_grad_dilated_mode: PAD_REFLECT reads xa through ReflectionPad1d(pad) without building it.
    ``precision="bf16"`` (fv_conv1d_weight_grad_dilated_bf16): dw from the operands rounded to bf16 (nearest even) with
    fp32 accumulation, db from the un-rounded g_pre."""
    name = "conv1d_weight_grad_dilated"
    _grad_precision(name, precision)
    if g_pre.dim() != 3 or xa.dim() != 3 or g_pre.shape[0] != xa.shape[0]:
        raise NativeError(f"{name}: g_pre [B,Cout,Tout] and xa [B,Cin,Tin] expected, got {tuple(g_pre.shape)} and "
                          f"{tuple(xa.shape)}")
    B, cout, tout = g_pre.shape
    cin, tin = xa.shape[1], xa.shape[2]
    k, dil, pad = int(k), int(dil), int(pad)
    if k > 0 and dil > 0 and tin + 2 * pad - dil * (k - 1) >= 1 and tout != tin + 2 * pad - dil * (k - 1):
        raise NativeError(f"{name}: {tout} output times do not belong to an input of {tin} samples")
    args = (B, cin, cout, tin, k, dil, pad)
    if precision == "bf16":
        entry, call_args = "fv_conv1d_weight_grad_dilated_bf16", args + (PAD_ZERO if pad_mode is None else int(pad_mode),)
    elif pad_mode is None:
        entry, call_args = "fv_conv1d_weight_grad_dilated", args
    else:
        entry, call_args = "fv_conv1d_weight_grad_dilated_mode", args + (int(pad_mode),)
    return _weight_grad_call(
        name, entry, (("g_pre", g_pre), ("xa", xa)), want_dw, want_db, (cout, cin, k), (cout,), call_args, workspace,
        lambda: conv1d_weight_grad_dilated_workspace_floats(*args, pad_mode, precision))


def conv1d_input_grad_reflect(g, wt, tin, dil=1, pad=0):
    """The data gradient of conv(ReflectionPad1d(pad)(xa), W, dilation=dil) (fv_conv1d_input_grad_reflect, one launch,
    no padded tensor): g [B,Cout,Tout], wt [Cin,Cout,k] = W.transpose(0, 1) contiguous -> dxa [B,Cin,tin]."""
    name = "conv1d_input_grad_reflect"
    if g.dim() != 3 or wt.dim() != 3 or wt.shape[1] != g.shape[1]:
        raise NativeError(f"{name}: g [B,Cout,Tout] and wt [Cin,Cout,k] expected, got {tuple(g.shape)} and "
                          f"{tuple(wt.shape)}")
    tin, dil, pad = int(tin), int(dil), int(pad)
    cin, cout, k = wt.shape
    if dil > 0 and tin + 2 * pad - dil * (k - 1) >= 1 and g.shape[2] != tin + 2 * pad - dil * (k - 1):
        raise NativeError(f"{name}: {g.shape[2]} output times do not belong to an input of {tin} samples")
    B = g.shape[0]
    dxa = torch.empty((B, cin, max(tin, 0)), dtype=torch.float32, device=g.device)
    with _on(g, wt, dxa) as stream:
        check(lib().fv_conv1d_input_grad_reflect(_ptr(g, "g"), _ptr(wt, "wt"), _ptr(dxa), B, cin, cout, tin, k, dil, pad,
                                                 stream))
    return dxa


def _convt_grad_shapes(name, g, cin_tin, w_shape, k, stride, pad, out_pad):
    if g.dim() != 3:
        raise NativeError(f"{name}: g [B,Cout,Tout] expected, got {tuple(g.shape)}")
    tin = int(cin_tin)
    if stride > 0 and tin >= 1 and g.shape[2] != (tin - 1) * stride - 2 * pad + k + out_pad:
        raise NativeError(f"{name}: {g.shape[2]} output times do not belong to an input of {tin} samples")
    if w_shape is not None and (len(w_shape) != 3 or w_shape[1] != g.shape[1] or w_shape[2] != k):
        raise NativeError(f"{name}: w [Cin,{g.shape[1]},{k}] expected, got {tuple(w_shape)}")


def conv_transpose1d_input_grad(g, w, tin, stride, pad, out_pad=0):
    """The data gradient of ConvTranspose1d (fv_conv_transpose1d_input_grad, one launch): g [B,Cout,Tout], w
    [Cin,Cout,k] the forward's (folded) weight -> dxa [B,Cin,tin]."""
    stride, pad, out_pad = int(stride), int(pad), int(out_pad)
    k = int(w.shape[2]) if w.dim() == 3 else 0
    _convt_grad_shapes("conv_transpose1d_input_grad", g, tin, tuple(w.shape), k, stride, pad, out_pad)
    B, cout, _ = g.shape
    cin = w.shape[0]
    dxa = torch.empty((B, cin, max(int(tin), 0)), dtype=torch.float32, device=g.device)
    with _on(g, w, dxa) as stream:
        check(lib().fv_conv_transpose1d_input_grad(_ptr(g, "g"), _ptr(w, "w"), _ptr(dxa), B, cin, cout, int(tin), k,
                                                   stride, pad, out_pad, stream))
    return dxa


def conv_transpose1d_weight_grad_workspace_floats(B, cin, cout, tin, k, stride, pad, out_pad=0, precision="f32"):
    """fp32 words of workspace conv_transpose1d_weight_grad needs for these shapes
    (fv_conv_transpose1d_weight_grad_workspace_bytes; with ``precision="bf16"``
    fv_conv_transpose1d_weight_grad_bf16_workspace_bytes); raises for shapes the entry refuses."""
    bf16 = _grad_precision("conv_transpose1d_weight_grad_workspace_floats", precision) == "bf16"
    entry = "fv_conv_transpose1d_weight_grad_bf16_workspace_bytes" if bf16 else "fv_conv_transpose1d_weight_grad_workspace_bytes"
    return _workspace_floats(getattr(lib(), entry)(
        int(B), int(cin), int(cout), int(tin), int(k), int(stride), int(pad), int(out_pad)))


def conv_transpose1d_weight_grad(g, xa, k, stride, pad, out_pad=0, want_dw=True, want_db=False, workspace=None,
                                 precision="f32"):
    """The weight (and bias) gradient of ConvTranspose1d (fv_conv_transpose1d_weight_grad, two launches): g
    [B,Cout,Tout], xa [B,Cin,Tin] the layer's input as it saw it -> (dw [Cin,Cout,k] or None, db [Cout] or None).
    ``precision="bf16"`` (fv_conv_transpose1d_weight_grad_bf16): dw from the operands rounded to bf16 (nearest even)
    with fp32 accumulation, db from the un-rounded g."""
    name = "conv_transpose1d_weight_grad"
    _grad_precision(name, precision)
    k, stride, pad, out_pad = int(k), int(stride), int(pad), int(out_pad)
    if xa.dim() != 3 or g.dim() != 3 or g.shape[0] != xa.shape[0]:
        raise NativeError(f"{name}: g [B,Cout,Tout] and xa [B,Cin,Tin] expected, got {tuple(g.shape)} and "
                          f"{tuple(xa.shape)}")
    B, cin, tin = xa.shape
    _convt_grad_shapes(name, g, tin, None, k, stride, pad, out_pad)
    cout = g.shape[1]
    args = (B, cin, cout, tin, k, stride, pad, out_pad)
    return _weight_grad_call(
        name, "fv_conv_transpose1d_weight_grad_bf16" if precision == "bf16" else "fv_conv_transpose1d_weight_grad",
        (("g", g), ("xa", xa)), want_dw, want_db, (cin, cout, k), (cout,), args, workspace,
        lambda: conv_transpose1d_weight_grad_workspace_floats(*args, precision=precision))


def _same_shape(name, *tensors):
    like = tensors[0]
    for t in tensors[1:]:
        if t is not None and t.shape != like.shape:
            raise NativeError(f"{name}: operands of one shape expected, got {[tuple(t.shape) for t in tensors if t is not None]}")
    return like


def tanh_grad(g, y):
    """g * (1 - y * y), elementwise (fv_tanh_grad, one launch): the gradient in front of y = tanh(z)."""
    like = _same_shape("tanh_grad", g, y)
    out = torch.empty_like(like)
    with _on(g, y, out) as stream:
        check(lib().fv_tanh_grad(_ptr(g, "g"), _ptr(y, "y"), _ptr(out), like.numel(), stream))
    return out


def residual_merge_grad(g_y, d, x, slope, acc=None):
    """[acc +] (g_y + (x > 0 ? 1 : slope) * d), elementwise (fv_residual_merge_grad, one launch): the gradient of x in
    x_next = x + conv(lrelu(x, slope)) from g_y = dL/dx_next and the conv's data gradient d."""
    like = _same_shape("residual_merge_grad", g_y, d, x, acc)
    out = torch.empty_like(like)
    with _on(g_y, d, x, acc, out) as stream:
        check(lib().fv_residual_merge_grad(_ptr(g_y, "g_y"), _ptr(d, "d"), _ptr(x, "x"), _ptr(acc, "acc", True),
                                           _ptr(out), like.numel(), float(slope), stream))
    return out


def grad_div(g, div):
    """g / div, elementwise (fv_grad_div, one launch): the adjoint of the MRF mean."""
    out = torch.empty_like(g)
    with _on(g, out) as stream:
        check(lib().fv_grad_div(_ptr(g, "g"), _ptr(out), g.numel(), float(div), stream))
    return out


# ---------------------------------------------------------------------------
# the head of Basis-MelGAN for training (csrc/basis_grad.hip)
# ---------------------------------------------------------------------------

def _basis_rows(name, Y):
    if Y.dim() != 3 or Y.shape[0] < 2:
        raise NativeError(f"{name}: Y [B+1,C,F] with the zero-mel row last expected, got {tuple(Y.shape)}")
    return Y.shape[0] - 1, Y.shape[1], Y.shape[2]


def basis_head_forward(Y):
    """Y [B+1,C,F], the trunk's raw output with the zero-mel row last -> D [B,C,F] = relu(Y[b]) - relu(Y[B])
    (fv_basis_head_forward, one launch)."""
    B, c, F = _basis_rows("basis_head_forward", Y)
    D = torch.empty((B, c, F), dtype=torch.float32, device=Y.device)
    with _on(Y, D) as stream:
        check(lib().fv_basis_head_forward(_ptr(Y, "Y"), _ptr(D), B, c, F, stream))
    return D


def basis_head_grad(g_est, g_w, Y, basis):
    """The adjoint of the head in one launch (fv_basis_head_grad): g_est [B, F L/2] or None, g_w [B,C,F] (the cotangent
    of weight in D's storage) or None, Y [B+1,C,F], basis [L,C] -> g_Y [B+1,C,F]."""
    B, c, F = _basis_rows("basis_head_grad", Y)
    if basis.dim() != 2 or basis.shape[1] != c:
        raise NativeError(f"basis_head_grad: basis [L,{c}] expected, got {tuple(basis.shape)}")
    L_ = basis.shape[0]
    if g_est is not None and tuple(g_est.shape) != (B, F * (L_ // 2)):
        raise NativeError(f"basis_head_grad: g_est {(B, F * (L_ // 2))} expected, got {tuple(g_est.shape)}")
    if g_w is not None and tuple(g_w.shape) != (B, c, F):
        raise NativeError(f"basis_head_grad: g_w {(B, c, F)} expected, got {tuple(g_w.shape)}")
    g_Y = torch.empty_like(Y)
    with _on(g_est, g_w, Y, basis, g_Y) as stream:
        check(lib().fv_basis_head_grad(_ptr(g_est, "g_est", True), _ptr(g_w, "g_w", True), _ptr(Y, "Y"),
                                       _ptr(basis, "basis"), _ptr(g_Y), B, c, F, L_, stream))
    return g_Y


def _basis_l1_shapes(name, D, target):
    if D.dim() != 3 or target.dim() != 3 or tuple(target.shape) != (D.shape[0], D.shape[2], D.shape[1]):
        raise NativeError(f"{name}: D [B,C,F] and target [B,F,C] expected, got {tuple(D.shape)} and {tuple(target.shape)}")
    return D.shape


def basis_weight_l1(D, target):
    """D [B,C,F] against target [B,F,C] -> two device floats, (mean |D^T - target|, mean D) (fv_basis_weight_l1, two
    launches)."""
    B, c, F = _basis_l1_shapes("basis_weight_l1", D, target)
    nbytes = lib().fv_basis_weight_l1_workspace_bytes(B, c, F)
    if nbytes < 0:
        check(int(nbytes))
    workspace = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=D.device)
    out = torch.empty(2, dtype=torch.float32, device=D.device)
    with _on(D, target, workspace, out) as stream:
        check(lib().fv_basis_weight_l1(_ptr(D, "D"), _ptr(target, "target"), _ptr(out), B, c, F, workspace.data_ptr(),
                                       workspace.numel() * 8, stream))
    return out


def basis_weight_l1_grad(D, target, coef=None):
    """coef * sign(D^T - target) / (B F C) in D's [B,C,F] storage (fv_basis_weight_l1_grad, one launch); coef: a
    one-element device tensor, or None for 1."""
    B, c, F = _basis_l1_shapes("basis_weight_l1_grad", D, target)
    if coef is not None and coef.numel() != 1:
        raise NativeError(f"basis_weight_l1_grad: coef of one element expected, got {tuple(coef.shape)}")
    g = torch.empty_like(D)
    with _on(D, target, coef, g) as stream:
        check(lib().fv_basis_weight_l1_grad(_ptr(D, "D"), _ptr(target, "target"), _ptr(coef, "coef", True), _ptr(g), B, c,
                                            F, stream))
    return g


# ---------------------------------------------------------------------------
# learning the basis: the encoder and the whole backward of (encode, decode) (csrc/basis_learn.hip)
# ---------------------------------------------------------------------------

def _basis_learn_shapes(name, wav, enc):
    if wav.dim() != 2 or enc.dim() != 2:
        raise NativeError(f"{name}: wav [B,n] and enc [C,L] expected, got {tuple(wav.shape)} and {tuple(enc.shape)}")
    return wav.shape[0], wav.shape[1], enc.shape[0], enc.shape[1]


def basis_frames(n, L_):
    """F = ceil(n / hop), hop = L / 2: the weight frames of n samples."""
    hop = L_ // 2
    return (n + hop - 1) // hop


def basis_encode(wav, enc):
    """wav [B,n], enc [C,L] -> W [B,C,F] = relu(conv1d(wav, enc, stride=L/2)) over the zero-extended waveform
    (fv_basis_encode, one launch)."""
    B, n, c, L_ = _basis_learn_shapes("basis_encode", wav, enc)
    W = torch.empty((B, c, basis_frames(n, L_) if L_ >= 2 else 0), dtype=torch.float32, device=wav.device)
    with _on(wav, enc, W) as stream:
        check(lib().fv_basis_encode(_ptr(wav, "wav"), _ptr(enc, "enc"), _ptr(W), B, n, c, L_, stream))
    return W


def basis_learn_grad(wav, g_est, W, basis, want_enc=True, want_basis=True, workspace=None):
    """The backward of est = crop(overlap_add(basis W)), W = basis_encode(wav, enc), in one launch and a combine
    (fv_basis_learn_grad): wav [B,n], g_est [B, F L/2], W [B,C,F], basis [L,C] -> (d_enc [C,L] or None,
    d_basis [L,C] or None).  ``workspace``: a float32 device tensor of at least the entry's size, for a test."""
    if W.dim() != 3 or basis.dim() != 2 or wav.dim() != 2 or basis.shape[1] != W.shape[1] or wav.shape[0] != W.shape[0]:
        raise NativeError(f"basis_learn_grad: wav [B,n], W [B,C,F] and basis [L,C] expected, got {tuple(wav.shape)}, "
                          f"{tuple(W.shape)} and {tuple(basis.shape)}")
    (B, n), c, L_ = wav.shape, W.shape[1], basis.shape[0]
    F = basis_frames(n, L_) if L_ >= 2 else 0
    if W.shape[2] != F or tuple(g_est.shape) != (B, F * (L_ // 2)):
        raise NativeError(f"basis_learn_grad: W {(B, c, F)} and g_est {(B, F * (L_ // 2))} expected, got "
                          f"{tuple(W.shape)} and {tuple(g_est.shape)}")
    if not (want_enc or want_basis):
        return None, None
    nbytes = lib().fv_basis_learn_grad_workspace_bytes(B, n, c, L_)
    if nbytes < 0:
        check(int(nbytes))
    if workspace is None:
        workspace = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=W.device)
    d_enc = torch.empty((c, L_), dtype=torch.float32, device=W.device) if want_enc else None
    d_basis = torch.empty((L_, c), dtype=torch.float32, device=W.device) if want_basis else None
    with _on(wav, g_est, W, basis, d_enc, d_basis, workspace) as stream:
        check(lib().fv_basis_learn_grad(_ptr(wav, "wav"), _ptr(g_est, "g_est"), _ptr(W, "W"), _ptr(basis, "basis"),
                                        _ptr(d_enc, "d_enc", True), _ptr(d_basis, "d_basis", True), B, n, c, L_,
                                        workspace.data_ptr(), workspace.numel() * 4, stream))
    return d_enc, d_basis


# ---------------------------------------------------------------------------
# gradient clipping + Adam over a table of tensors (csrc/optim.hip)
# ---------------------------------------------------------------------------

ADAM_CHUNK = _C["FV_ADAM_CHUNK"]               # elements per table chunk, one workgroup each
ADAM_ROW_BYTES, ADAM_CHUNK_BYTES = 48, 8      # sizeof(fv_adam_tensor), sizeof(fv_adam_chunk)


def _adam_table(table, n_tensors, n_chunks, name):
    """(rows pointer, chunks pointer) of a device table laid out as optim.adam_table does: n_tensors fv_adam_tensor
    rows, then n_chunks fv_adam_chunk entries, in one uint8 device tensor."""
    n_tensors, n_chunks = int(n_tensors), int(n_chunks)
    need = ADAM_ROW_BYTES * n_tensors + ADAM_CHUNK_BYTES * n_chunks
    if not torch.is_tensor(table) or not table.is_cuda or table.dtype != torch.uint8 or not table.is_contiguous():
        raise NativeError(f"{name}: the table must be a contiguous uint8 ROCm device tensor")
    if n_tensors < 1 or n_chunks < 1 or table.numel() < need:
        raise NativeError(f"{name}: a table of {n_tensors} rows and {n_chunks} chunks needs {need} bytes, got "
                          f"{table.numel()}")
    return table.data_ptr(), table.data_ptr() + ADAM_ROW_BYTES * n_tensors


def grad_sq_norm_workspace_floats(n_chunks):
    """fp32 words of workspace grad_sq_norm needs for a table of n_chunks chunks (fv_grad_sq_norm_workspace_bytes)."""
    need = lib().fv_grad_sq_norm_workspace_bytes(int(n_chunks))
    if need < 0:
        check(int(need))
    return (need + 3) // 4


def grad_sq_norm(table, n_tensors, n_chunks, max_norm, workspace, out):
    """The 2-norm of all the gradients of a table and clip_grad_norm_'s factor (fv_grad_sq_norm, two launches): writes
    out[0] = norm, out[1] = min(1, max_norm / (norm + 1e-6)); ``out``: two fp32 device words, ``workspace``: an fp32
    device tensor of grad_sq_norm_workspace_floats(n_chunks) words whose contents do not matter."""
    rows, chunks = _adam_table(table, n_tensors, n_chunks, "grad_sq_norm")
    if out.numel() < 2:
        raise NativeError("grad_sq_norm: out must hold two floats")
    with _on(table, workspace, out) as stream:
        check(lib().fv_grad_sq_norm(rows, chunks, int(n_tensors), int(n_chunks), float(max_norm),
                                    _ptr(workspace, "workspace"), workspace.numel() * 4, _ptr(out, "out"), stream))


def adam_step(table, n_tensors, n_chunks, coef, beta1, beta2, eps, first_chunk=0, chunk_count=None):
    """The Adam update of the chunks [first_chunk, first_chunk + chunk_count) of a table (fv_adam_step, one launch);
    ``coef``: a one-element fp32 device tensor that scales every gradient first (and is written back to it), or None."""
    rows, chunks = _adam_table(table, n_tensors, n_chunks, "adam_step")
    first_chunk = int(first_chunk)
    chunk_count = int(n_chunks) - first_chunk if chunk_count is None else int(chunk_count)
    if first_chunk < 0 or chunk_count < 1 or first_chunk + chunk_count > int(n_chunks):
        raise NativeError(f"adam_step: chunks [{first_chunk}, {first_chunk + chunk_count}) of {n_chunks}")
    with _on(table, coef) as stream:
        check(lib().fv_adam_step(rows, chunks + ADAM_CHUNK_BYTES * first_chunk, int(n_tensors), chunk_count,
                                 _ptr(coef, "coef", True), float(beta1), float(beta2), float(eps), stream))


def grad_bucket_pack(table, n_tensors, n_chunks, scale):
    """Every gradient into its span of the flat bucket, times ``scale`` (fv_grad_bucket_pack, one launch).  ``table``:
    the rows and chunks of optim.adam_table, the rows' ``g`` pointing INTO the bucket, followed by the n_tensors source
    pointers (the parameters' own gradients, 0 for a span of zeros) as uint64 -- one upload carries all three."""
    rows, chunks = _adam_table(table, n_tensors, n_chunks, "grad_bucket_pack")
    src = chunks - table.data_ptr() + ADAM_CHUNK_BYTES * int(n_chunks)
    if table.numel() < src + 8 * int(n_tensors):
        raise NativeError(f"grad_bucket_pack: a table of {int(n_tensors)} rows and {int(n_chunks)} chunks with its source "
                          f"pointers needs {src + 8 * int(n_tensors)} bytes, got {table.numel()}")
    with _on(table) as stream:
        check(lib().fv_grad_bucket_pack(rows, chunks, int(n_tensors), int(n_chunks), table.data_ptr() + src,
                                        float(scale), stream))


def reflect_pad_fold(gp, pad):
    """The adjoint of ReflectionPad1d(pad): gp [..., T + 2 pad] -> [..., T] (fv_reflect_pad_fold, one launch)."""
    T = gp.shape[-1] - 2 * int(pad)
    rows = gp.numel() // gp.shape[-1] if gp.shape[-1] else 0
    dx = torch.empty(tuple(gp.shape[:-1]) + (max(T, 0),), dtype=torch.float32, device=gp.device)
    with _on(gp, dx) as stream:
        check(lib().fv_reflect_pad_fold(_ptr(gp, "gp"), _ptr(dx), rows, T, int(pad), stream))
    return dx


def avg_pool1d_input_grad(g, tin, k, stride, pad):
    """The adjoint of avg_pool1d: g [..., Tout] -> dx [..., tin] (fv_avg_pool1d_input_grad, one launch)."""
    tout = g.shape[-1]
    rows = g.numel() // tout if tout else 0
    if stride > 0 and tin + 2 * pad >= k and tout != (tin + 2 * pad - k) // stride + 1:
        raise NativeError(f"avg_pool1d_input_grad: {tout} windows do not belong to an input of {tin} samples")
    dx = torch.empty(tuple(g.shape[:-1]) + (max(int(tin), 0),), dtype=torch.float32, device=g.device)
    with _on(g, dx) as stream:
        check(lib().fv_avg_pool1d_input_grad(_ptr(g, "g"), _ptr(dx), rows, int(tin), int(k), int(stride), int(pad),
                                             stream))
    return dx


def disc_score_grad(es, rs, coef, skip=None):
    """Lists of M map pairs as disc_score_sums takes them and M host triples (c_l1, c_adv, c_fake) -> the list of
    g_m = c_l1 sign(e_m - r_m) + 2 c_adv (e_m - 1) + 2 c_fake e_m (fv_disc_score_grad: one launch per DISC_MAX_MAPS
    maps).  ``skip``: M flags; a flagged map gets no gradient (None)."""
    M = len(es)
    if M != len(rs) or M == 0 or len(coef) != M:
        raise NativeError(f"disc_score_grad: {len(es)} estimate maps, {len(rs)} real maps, {len(coef)} coefficients")
    skip = [False] * M if skip is None else list(skip)
    if M > DISC_MAX_MAPS:
        out = []
        for i in range(0, M, DISC_MAX_MAPS):
            j = i + DISC_MAX_MAPS
            out += disc_score_grad(es[i:j], rs[i:j], coef[i:j], skip[i:j])
        return out
    B = es[0].shape[0]
    for e, r in zip(es, rs):
        if e.shape != r.shape or e.shape[0] != B:
            raise NativeError(f"disc_score_grad: map shapes {tuple(e.shape)} and {tuple(r.shape)} (batch {B})")
    gs = [None if s else torch.empty_like(e) for e, s in zip(es, skip)]
    n = (ctypes.c_int64 * M)(*[e[0].numel() for e in es])
    c = (ctypes.c_float * (3 * M))(*[float(v) for t in coef for v in t])
    with _on(*es, *rs, *gs) as stream:
        e_a = (ctypes.c_void_p * M)(*[_ptr(e, "e") for e in es])
        r_a = (ctypes.c_void_p * M)(*[_ptr(r, "r") for r in rs])
        g_a = (ctypes.c_void_p * M)(*[_ptr(g, "g", True) for g in gs])
        check(lib().fv_disc_score_grad(e_a, r_a, g_a, n, c, M, B, stream))
    return gs


def pqmf_synthesis(x, synthesis_filter, y):
    """x [B,S,Tsub], synthesis_filter [1,S,ntaps] -> y [B,1,S*Tsub] (filled in place)."""
    B, S, Tsub = x.shape
    h = synthesis_filter.reshape(S, -1).contiguous().float()
    with _on(x, h, y) as stream:
        check(lib().fv_pqmf_synthesis(_ptr(x, "x"), _ptr(h, "h"), _ptr(y, "y"), B, S, h.shape[1], Tsub,
                                      stream))
    return y


def conv_post_pqmf(x, packed, bias, synthesis_filter, k, pad, pre_slope=1.0, post=POST_TANH):
    """pqmf_synthesis(post(conv1d(lrelu(x, pre_slope)) + bias)) in one launch (fv_conv_post_pqmf): x [B,Cin,T],
    packed = pack_conv1d(w [S,Cin,k]), synthesis_filter [1,S,ntaps] -> [B,1,S*T]."""
    B, cin, T = x.shape
    S = synthesis_filter.shape[1]
    h = synthesis_filter.reshape(S, -1).contiguous().float()
    y = torch.empty((B, 1, S * T), dtype=torch.float32, device=x.device)
    with _on(x, packed, bias, h, y) as stream:
        check(lib().fv_conv_post_pqmf(_ptr(x, "x"), _ptr(packed, "packed"), _ptr(bias, "bias", True), _ptr(h, "h"),
                                      _ptr(y, "y"), B, cin, S, T, k, pad, float(pre_slope), post, h.shape[1], stream))
    return y


# ---------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------

class Plan:
    """Owner of a native op list (fv_plan_t) plus the tensors its ops point at."""

    def __init__(self, in_channels):
        self._h = lib().fv_plan_create(in_channels)
        self.in_channels = in_channels
        self._keep = []        # packed weights / biases the native plan references
        self._ws = None
        self._calls = {}       # (B, T, device) -> (output channels, output length, workspace bytes)
        self._guard = None     # GuardWord of the owning module (set_guard)
        self._dev = None       # device of the last run
        self.guarded = False   # the plan holds split-f16 launches (PlanBuilder.finalize)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.fv_plan_destroy(h)

    def keep(self, t):
        self._keep.append(t)
        return t

    # a plan is a raw native handle + device pointers into its owner's tensors: never copied or pickled
    def __deepcopy__(self, memo):
        raise NativeError("a native plan cannot be copied; the owning module rebuilds its plans on demand")

    def __reduce__(self):
        raise NativeError("a native plan cannot be pickled; the owning module rebuilds its plans on demand")

    def add_conv1d(self, x, y, packed, bias, cin, cout, k, dil=1, pad=0, pad_mode=PAD_ZERO,
                   pre_slope=1.0, res=SLOT_NONE, acc=SLOT_NONE, out_div=1.0, post=POST_NONE,
                   y_act=SLOT_NONE, act_slope=1.0, acc2=SLOT_NONE):
        self.keep(packed)
        if bias is not None:
            self.keep(bias)
        check(lib().fv_plan_add_conv1d(self._h, x, y, y_act, res, acc, acc2, _ptr(packed, "packed"),
                                       _ptr(bias, "bias", True), cin, cout, k, dil, pad, pad_mode,
                                       float(pre_slope), float(out_div), post, float(act_slope)))

    def add_conv_transpose1d(self, x, y, packed, bias, cin, cout, k, stride, pad, out_pad,
                             pre_slope=1.0, post=POST_NONE, y_act=SLOT_NONE, act_slope=1.0):
        self.keep(packed)
        if bias is not None:
            self.keep(bias)
        check(lib().fv_plan_add_conv_transpose1d(self._h, x, y, y_act, _ptr(packed, "packed"),
                                                 _ptr(bias, "bias", True), cin, cout, k, stride,
                                                 pad, out_pad, float(pre_slope), post,
                                                 float(act_slope)))

    def add_conv_transpose1d_split_f16(self, x, y, packed, bias, cin, cout, k, stride, pad, out_pad, pre_slope=1.0,
                                       y_act=SLOT_NONE, act_slope=1.0, merge=None):
        """``merge = (add1_slot, add2_slot, div)``: the input is ((x + add1) + add2) / div, formed in the kernel's window
        loader (fv_plan_set_input_merge: the MRF merge of hifigan.py:99-103 inside the upsampler behind the stage)."""
        self.keep(packed)
        if bias is not None:
            self.keep(bias)
        check(lib().fv_plan_add_conv_transpose1d_split_f16(self._h, x, y, y_act, _ptr(packed, "packed"),
                                                           _ptr(bias, "bias", True), cin, cout, k, stride, pad, out_pad,
                                                           float(pre_slope), float(act_slope)))
        if merge is not None:
            check(lib().fv_plan_set_input_merge(self._h, int(merge[0]), int(merge[1]), float(merge[2])))

    def add_conv1d_2src(self, x, x2, y, packed, bias, cin1, cin2, cout, res=SLOT_NONE, post=POST_NONE,
                        y_act=SLOT_NONE, act_slope=1.0):
        self.keep(packed)
        if bias is not None:
            self.keep(bias)
        check(lib().fv_plan_add_conv1d_2src(self._h, x, x2, y, y_act, res, _ptr(packed, "packed"),
                                            _ptr(bias, "bias", True), cin1, cin2, cout, post,
                                            float(act_slope)))

    def add_conv1x1_2src_split_f16(self, x, x2, y, packed, bias, channels, pre_slope=1.0, res=SLOT_NONE, post=POST_NONE,
                                   y_act=SLOT_NONE, act_slope=1.0):
        self.keep(packed)
        if bias is not None:
            self.keep(bias)
        check(lib().fv_plan_add_conv1x1_2src_split_f16(self._h, x, x2, y, y_act, res, _ptr(packed, "packed"),
                                                       _ptr(bias, "bias", True), channels, float(pre_slope), post,
                                                       float(act_slope)))

    def add_residual_stack_split_f16(self, x, y, packed, bias_dilated, bias_out, channels, k, dil, slope, pad_mode=PAD_REFLECT,
                                     y_act=SLOT_NONE, act_slope=1.0, two_launch=None, post=POST_NONE):
        """``two_launch`` = (hidden slot, pack_pair image of the dilated conv, pack_conv1x1_2src_split image of the 1x1 pair):
        the form a run with many tiles takes instead (fv_plan_set_stack_two_launch; 256 channels)."""
        self.keep(packed)
        for b in (bias_dilated, bias_out):
            if b is not None:
                self.keep(b)
        check(lib().fv_plan_add_residual_stack_split_f16(self._h, x, y, y_act, _ptr(packed, "packed"),
                                                         _ptr(bias_dilated, "bias_dilated", True), _ptr(bias_out, "bias_out", True),
                                                         channels, k, dil, float(slope), pad_mode, post, float(act_slope)))
        if two_launch is not None:
            hidden, pd, pp = two_launch
            self.keep(pd)
            self.keep(pp)
            check(lib().fv_plan_set_stack_two_launch(self._h, hidden, _ptr(pd, "packed_dilated"), _ptr(pp, "packed_pair")))

    def add_upsample_conv1d(self, x, y, packed, bias, cin, cout, k, rate, pad, pre_slope=1.0,
                            post=POST_NONE, y_act=SLOT_NONE, act_slope=1.0):
        self.keep(packed)
        if bias is not None:
            self.keep(bias)
        check(lib().fv_plan_add_upsample_conv1d(self._h, x, y, y_act, _ptr(packed, "packed"),
                                                _ptr(bias, "bias", True), cin, cout, k, rate, pad,
                                                float(pre_slope), post, float(act_slope)))

    def add_conv1d_sum3(self, xs, ress, tmps, y, packed, bias_sum, channels, ks, out_div=1.0, post=POST_NONE,
                        y_act=SLOT_NONE, act_slope=1.0):
        """The three last convs of an MRF stage into one output (fv_plan_add_conv1d_sum3)."""
        for t in packed:
            self.keep(t)
        if bias_sum is not None:
            self.keep(bias_sum)
        i3 = ctypes.c_int * 3
        wp = (ctypes.c_void_p * 3)(*[_ptr(t, "packed") for t in packed])
        check(lib().fv_plan_add_conv1d_sum3(self._h, i3(*xs), i3(*ress), (ctypes.c_int * 2)(*tmps), y, y_act, wp,
                                            _ptr(bias_sum, "bias_sum", True), channels, i3(*ks),
                                            float(out_div), post, float(act_slope)))

    def add_resblock_pair(self, x, y, packed1, packed2, bias1, bias2, channels, k, dil, slope,
                          y_act=SLOT_NONE, act_slope=1.0, prec=PAIR_F32, add1=SLOT_NONE, add2=SLOT_NONE,
                          out_div=1.0, post=POST_NONE, mid=SLOT_NONE):
        """One fused ResBlock pair (fv_plan_add_resblock_pair_ex); group members share a launch."""
        for t in (packed1, packed2, bias1, bias2):
            if t is not None:
                self.keep(t)
        check(lib().fv_plan_add_resblock_pair_ex(self._h, x, y, y_act, mid, add1, add2, _ptr(packed1, "packed1"),
                                                 _ptr(packed2, "packed2"), _ptr(bias1, "bias1", True),
                                                 _ptr(bias2, "bias2", True), channels, k, dil, float(slope),
                                                 float(out_div), post, float(act_slope), prec))

    def add_mrf_stage(self, x, y, packed, channels, ks, dils, slope, out_div=3.0, post=POST_NONE, y_act=SLOT_NONE,
                      act_slope=1.0):
        """A whole 16- / 32-channel MRF stage as one op / one launch (fv_plan_add_mrf_stage_split_f16); the 32-channel
        kernel's scratch belongs to the op (a plan runs its ops in order on one stream)."""
        self.keep(packed)
        work = mrf_stage_workspace(channels, packed.device)
        if work is not None:
            self.keep(work)
        check(lib().fv_plan_add_mrf_stage_split_f16(self._h, x, y, y_act, _ptr(packed, "packed"), channels,
                                                    (ctypes.c_int * 3)(*ks), (ctypes.c_int * 3)(*dils), float(slope),
                                                    float(out_div), post, float(act_slope), *_work_args(work)))

    def add_mrf_stage_classes(self, x, y_s, y_r2, packed, channels, ks, dils, slope):
        """The 32-channel MRF stage as one launch of two block classes (fv_plan_add_mrf_stage_classes_f16): slot ``y_s``
        receives r_0 + r_1, ``y_r2`` r_2; the op owns its scratch."""
        self.keep(packed)
        work = mrf_stage_workspace(channels, packed.device)
        if work is not None:
            self.keep(work)
        check(lib().fv_plan_add_mrf_stage_classes_f16(self._h, x, y_s, y_r2, _ptr(packed, "packed"), channels,
                                                      (ctypes.c_int * 3)(*ks), (ctypes.c_int * 3)(*dils), float(slope),
                                                      *_work_args(work)))

    def set_pair_output_conv(self, w, bias, y, act_slope, post=POST_NONE):
        """Fold a 16 -> 1 channel, 7-tap conv into the resblock pair appended last (fv_plan_set_pair_output_conv):
        ``y`` becomes post(conv(lrelu(pair result, act_slope)) + bias), [B, 1, T]."""
        self.keep(w)
        if bias is not None:
            self.keep(bias)
        check(lib().fv_plan_set_pair_output_conv(self._h, _ptr(w, "w"), _ptr(bias, "bias", True), y, float(act_slope), post))

    def add_conv1d_split_f16(self, x, y, packed, bias, channels, k, dil, pre_slope=1.0, res=SLOT_NONE, add1=SLOT_NONE,
                             add2=SLOT_NONE, out_div=1.0, post=POST_NONE, y_act=SLOT_NONE, act_slope=1.0,
                             pad_mode=PAD_ZERO):
        """One 'same' conv with split-f16 operands (fv_plan_add_conv1d_split_f16); group members share a launch."""
        for t in (packed, bias):
            if t is not None:
                self.keep(t)
        check(lib().fv_plan_add_conv1d_split_f16(self._h, x, y, y_act, res, add1, add2, _ptr(packed, "packed"),
                                                 _ptr(bias, "bias", True), channels, k, dil, pad_mode,
                                                 float(pre_slope), float(out_div), post, float(act_slope)))

    def add_mrf_sum(self, xs, y, packed1, packed2, bias1, bias2, channels, ks, dil, slope, out_div=3.0,
                    post=POST_NONE, y_act=SLOT_NONE, act_slope=1.0):
        """Last pairs of the three ResBlocks + the MRF mean in one launch (fv_plan_add_mrf_sum)."""
        for t in list(packed1) + list(packed2) + list(bias1) + list(bias2):
            if t is not None:
                self.keep(t)
        i3 = ctypes.c_int * 3
        check(lib().fv_plan_add_mrf_sum(self._h, i3(*xs), y, y_act, _vp_array(packed1, "packed1"),
                                        _vp_array(packed2, "packed2"), _vp_array(bias1, "bias1", True),
                                        _vp_array(bias2, "bias2", True), channels, i3(*ks), dil, float(slope),
                                        float(out_div), post, float(act_slope)))

    def set_sum_order(self, own_first):
        check(lib().fv_plan_set_sum_order(self._h, 1 if own_first else 0))

    def set_guard(self, guard):
        """Range guard of the plan's split-f16 launches (fv_plan_set_guard): a GuardWord, or None."""
        self._guard = self.keep(guard) if guard is not None else None
        check(lib().fv_plan_set_guard(self._h, guard.ptr(0) if guard is not None else None))

    def check_range(self):
        """Drain the current stream, then: did a split-f16 kernel of the runs since the last check meet an operand
        beyond the f16 range?  (fv_plan_check_range; clears the word.)"""
        if self._guard is None:
            return False
        rc = lib().fv_plan_check_range(self._h, torch.cuda.current_stream(self._dev).cuda_stream)
        if rc == ERR_RANGE:
            return True
        if rc == ERR_RANGE_LOW:
            return "low"             # (truthy: the run has to be repeated; the caller may treat it as a property of the input)
        check(rc)
        return False

    def set_group(self, group):
        check(lib().fv_plan_set_group(self._h, group))

    def add_pqmf_synthesis(self, x, y, h):
        """h [S, ntaps] contiguous fp32 device tensor."""
        self.keep(h)
        check(lib().fv_plan_add_pqmf_synthesis(self._h, x, y, _ptr(h, "h"), h.shape[0], h.shape[1]))

    def add_conv_post_pqmf(self, x, y, packed, bias, cin, k, pad, h, pre_slope=1.0, post=POST_TANH):
        """conv_post (cin -> S sub-bands) + post + PQMF synthesis as one op (fv_plan_add_conv_post_pqmf); h [S, ntaps]."""
        for t in (packed, bias, h):
            if t is not None:
                self.keep(t)
        check(lib().fv_plan_add_conv_post_pqmf(self._h, x, y, _ptr(packed, "packed"), _ptr(bias, "bias", True), cin,
                                               h.shape[0], k, pad, float(pre_slope), post, _ptr(h, "h"), h.shape[1]))

    def set_output_offset(self, aux_slot, y2_slot=SLOT_NONE, y_slot=SLOT_OUT):
        """The op added last (output slot ``y_slot``) subtracts auxiliary input ``aux_slot`` in its epilogue
        (fv_plan_set_output_offset)."""
        check(lib().fv_plan_set_output_offset(self._h, aux_slot, y2_slot))
        self.__dict__.setdefault("_aux_of", {})[aux_slot] = y_slot

    def _aux_elems(self, T, aux_slot):
        """Elements per utterance of the tensor auxiliary input ``aux_slot`` is subtracted from (None: unused)."""
        y = self.__dict__.get("_aux_of", {}).get(aux_slot)
        if y is None:
            return None
        c, n = self.slot_shape(T, y)
        return c * n

    def slot_shape(self, T, slot):
        c, n = ctypes.c_int(), ctypes.c_int64()
        check(lib().fv_plan_slot_shape(self._h, T, slot, ctypes.byref(c), ctypes.byref(n)))
        return c.value, n.value

    def output_shape(self, T):
        return self.slot_shape(T, SLOT_OUT)

    def num_ops(self):
        return lib().fv_plan_num_ops(self._h)

    def run(self, x, out=None, aux=(), out2=False):
        """x [B,Cin,T] contiguous fp32 on a ROCm device -> [B,Cout,Tout].  ``aux``: up to two tensors for the
        plan's auxiliary inputs (output offsets: [C,T'], [1,C,T'] or, per utterance, [B,C,T']); ``out2``: also
        return the plan's second output (SLOT_OUT2) -> (out, out2)."""
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise NativeError(f"plan input must be [B, {self.in_channels}, T], got {tuple(x.shape)}")
        B, _, T = x.shape
        if B == 0 or T == 0:
            raise NativeError(f"plan input is empty: {tuple(x.shape)}")
        dev = x.device
        key = (B, T, dev)
        ent = self._calls.get(key)
        if ent is None:
            # once per (batch, frames, device): output shape and workspace size (two native queries), and that the plan's
            # packed weights live where the input does
            _on(x, *self._keep[:1])
            c, n = self.output_shape(T)
            nbytes = lib().fv_plan_workspace_bytes(self._h, B, T)
            if nbytes < 0:
                check(int(nbytes))
            if len(self._calls) >= 256:
                self._calls.clear()
            ent = self._calls[key] = (c, n, max(int(nbytes), 256))
        c, n, nbytes = ent
        if out is None:
            out = torch.empty((B, c, n), dtype=torch.float32, device=dev)
        self._dev = dev
        if self._ws is None or self._ws.device != dev or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)      # (grows, never shrinks: one arena per plan)
        if not aux and not out2:
            # the common call (no auxiliary inputs, one output): one pointer check per operand, no marshalling of empties
            if not (x.is_cuda and x.dtype is torch.float32 and x.is_contiguous()):
                _ptr(x, "input")
            if not (out.is_cuda and out.dtype is torch.float32 and out.is_contiguous() and out.device == dev):
                _ptr(out, "out")
                raise NativeError(f"out lives on {out.device}, the input on {dev}")
            if torch.cuda.current_device() == dev.index:
                check(lib().fv_plan_run_aux(self._h, B, T, x.data_ptr(), out.data_ptr(), None, None, None,
                                            self._ws.data_ptr(), self._ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
            else:
                with torch.cuda.device(dev):
                    check(lib().fv_plan_run_aux(self._h, B, T, x.data_ptr(), out.data_ptr(), None, None, None,
                                                self._ws.data_ptr(), self._ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
            return out
        second = None
        if out2:
            c2, n2 = self.slot_shape(T, SLOT_OUT2)
            second = torch.empty((B, c2, n2), dtype=torch.float32, device=x.device)
        aux = list(aux) + [None] * (2 - len(aux))
        ptrs = (ctypes.c_void_p * 2)(*[_ptr(a, "aux", True) for a in aux])
        # an auxiliary input is an output offset: exactly the element count of the tensor it is subtracted from
        # (per utterance, or one row per utterance) -- the kernels index it without bounds
        batched = []
        for j, a in enumerate(aux):
            if a is None:
                batched.append(0)
                continue
            per = self._aux_elems(T, SLOT_AUX_IN0 + j)
            if per is None:
                raise NativeError(f"auxiliary input {j} was given, but no op of the plan subtracts it")
            if a.numel() == per:
                batched.append(0)
            elif a.numel() == B * per:
                batched.append(1)
            else:
                raise NativeError(f"auxiliary input {j} has {a.numel()} elements; the tensor it is subtracted from has "
                                  f"{per} per utterance (batch {B})")
        batched = (ctypes.c_int * 2)(*batched)
        with _on(x, out, self._ws, second, *aux, *self._keep[:1]) as stream:
            check(lib().fv_plan_run_aux(self._h, B, T, _ptr(x, "input"), _ptr(out, "out"), _ptr(second, "out2", True),
                                        ptrs, batched, self._ws.data_ptr(), self._ws.numel(), stream))
        return (out, second) if out2 else out


# ---------------------------------------------------------------------------
# measurement hook
# ---------------------------------------------------------------------------

def profile_enable(on):
    check(lib().fv_profile_enable(1 if on else 0))


KERNEL_CONV_MFMA32, KERNEL_CONV_MFMA16 = _C["FV_KERNEL_CONV_MFMA32"], _C["FV_KERNEL_CONV_MFMA16"]
KERNEL_CONV_NARROW, KERNEL_PAIR16, KERNEL_PAIR32 = _C["FV_KERNEL_CONV_NARROW"], _C["FV_KERNEL_PAIR16"], _C["FV_KERNEL_PAIR32"]
KERNEL_PAIRH16, KERNEL_PAIRH32 = _C["FV_KERNEL_PAIRH16"], _C["FV_KERNEL_PAIRH32"]
KERNEL_CONVH64, KERNEL_CONVH128 = _C["FV_KERNEL_CONVH64"], _C["FV_KERNEL_CONVH128"]
KERNEL_CONVT, KERNEL_CONVG, KERNEL_STACK = _C["FV_KERNEL_CONVT"], _C["FV_KERNEL_CONVG"], _C["FV_KERNEL_STACK"]
KERNEL_MRF16 = _C["FV_KERNEL_MRF16"]     # a whole 16-channel MRF stage as one launch (mrfh_kernel)
KERNEL_MRF32 = _C["FV_KERNEL_MRF32"]     # ... 32-channel (mrfw_kernel)


def profile_bracket_cost(n=200):
    """Milliseconds the (begin, end) event pair of the measurement hook adds per launch."""
    ms = ctypes.c_double()
    check(lib().fv_profile_bracket_cost(torch.cuda.current_stream().cuda_stream, n, ctypes.byref(ms)))
    return ms.value


def profile_mfma_f16_rate(launches=40, iters=20000):
    """The device's achievable dense f16 matrix rate in TFLOP/s (fv_profile_mfma_f16_rate: nothing but v_mfma_f32_16x16x32_f16 on
    registers, timed over the last half of ``launches`` back-to-back launches on the current stream)."""
    props = torch.cuda.get_device_properties(torch.cuda.current_device())
    scratch = torch.empty(512 * 2 * props.multi_processor_count, dtype=torch.float32, device="cuda")
    tf = ctypes.c_double()
    check(lib().fv_profile_mfma_f16_rate(scratch.data_ptr(), scratch.numel(), int(launches), int(iters),
                                         torch.cuda.current_stream().cuda_stream, ctypes.byref(tf)))
    return tf.value


def profile_collect(kind=-1):
    """Drain the per-launch HIP-event records of one kernel family (-1: all)."""
    n, ms = ctypes.c_int64(), ctypes.c_double()
    fl, by = ctypes.c_double(), ctypes.c_double()
    check(lib().fv_profile_collect(kind, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl),
                                   ctypes.byref(by)))
    return {"launches": n.value, "ms": ms.value, "flops": fl.value, "bytes": by.value}
