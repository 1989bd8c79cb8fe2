"""CPU tests of fastvocoder_amd/_abi.py: the binding's signatures and constants are read from include/fastvocoder_hip.h.
The parser on small headers written here, then the project's header: every declared entry is bound with as many
parameters as it declares, every entry the Python sources name is declared, and four signatures checked by hand."""
import ctypes
import glob
import os
import re

import pytest

from fastvocoder_amd import _abi, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i, f, d, i64, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_int64, ctypes.c_char_p

SMALL = """
#ifndef SMALL_H
#define SMALL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define FV_NEG (-3)
#define FV_HEX 0x1F0
#define FV_PLAIN 18   /* 18: fv_commented(int a); a comment after the value */
#define FV_ZERO 0 // and this form
#define FV_SHIFT (1 << 20)
#define FV_SUM (FV_NEG + FV_HEX)
#define FV_CAST ((int64_t)1 << 40)
#define FV_AT(n_fft) (2 * (n_fft))
#define FV_AT0(n_fft) 0
#define FV_LINES 1 + \\
                 2
typedef struct fv_row {
    float* p;        /* fv_in_struct(1); */
    int64_t n;
} fv_row;
typedef struct fv_plan fv_plan_t;

int fv_three(const float* x,
             int64_t n,
             float slope);
/* between two prototypes: ( ) ; int fv_ghost(int a); */
int64_t fv_after(const float* const* x, unsigned long long* q, size_t n, const fv_row* rows, double eps, unsigned bits,
                 unsigned int more, long long big);
// int fv_line_comment(void);
const char* fv_text(void);
int fv_none();
void fv_free(fv_plan_t* plan);
fv_plan_t* fv_make(const char* key, char* buf, int k[3], const int taps[], const void* any);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_prototypes_of_a_small_header():
    protos, _ = _abi.parse(SMALL)
    assert protos == {
        "fv_three": (i, [vp, i64, f]),                                                  # over three lines
        "fv_after": (i64, [vp, vp, ctypes.c_size_t, vp, d, ctypes.c_uint, ctypes.c_uint, ctypes.c_longlong]),
        "fv_text": (cp, []),                                                            # (void)
        "fv_none": (i, []),
        "fv_free": (None, [vp]),
        "fv_make": (vp, [cp, vp, vp, vp, vp]),                                          # int k[3] is a pointer
    }


def test_constants_of_a_small_header():
    _, consts = _abi.parse(SMALL)
    # expressions and function-like macros are absent, not mis-read
    assert consts == {"FV_NEG": -3, "FV_HEX": 0x1F0, "FV_PLAIN": 18, "FV_ZERO": 0}


@pytest.mark.parametrize("decl", ["int fv_bad(const float* x, long n);", "int fv_bad(short n);", "uint64_t fv_bad(int n);",
                                  "int fv_bad(fv_row row);", "int fv_bad(int);", "long fv_bad(void);"])
def test_an_unknown_scalar_type_raises_and_names_the_function(decl):
    with pytest.raises(_abi.NativeError, match="fv_bad"):
        _abi.parse("int fv_good(int a);\n" + decl)


def test_a_declaration_the_parser_cannot_read_raises():
    with pytest.raises(_abi.NativeError, match="fv_callback"):
        _abi.parse("int fv_callback(void (*fn)(int), int n);")


def test_a_missing_header_raises_naming_the_path(monkeypatch):
    monkeypatch.setattr(_abi, "_parsed", None)
    monkeypatch.setattr(_abi, "HEADER", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(_native.NativeError, match="no_such_header.h"):
        _abi.prototypes()


def test_the_header_is_parsed_once_per_process(monkeypatch):
    assert _abi.prototypes() is _abi.prototypes() and _abi.constants() is _abi.constants()
    monkeypatch.setattr(_abi, "parse", None)            # a second parse would raise
    assert len(_abi.prototypes()) > 100 and _abi.constants()["FV_ABI_VERSION"] == _native.ABI_VERSION


# ---- the project's header ---------------------------------------------------------------------------------------------

def _header():
    with open(os.path.join(ROOT, "include", "fastvocoder_hip.h")) as fh:
        return fh.read()


def test_every_name_of_the_header_is_parsed():
    names = set(re.findall(r"\b(fv_[a-z0-9_]+)\s*\(", _header()))        # test_c_abi_library_exports_every_declared_symbol's
    assert set(_abi.prototypes()) == names


def test_every_entry_is_bound_with_as_many_parameters_as_it_declares():
    header = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    lib = _native.lib()
    for name, (restype, argtypes) in _abi.prototypes().items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, header)
        assert decl, name
        params = decl.group(1).strip()
        count = 0 if params in ("", "void") else params.count(",") + 1
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count == len(argtypes), name
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name


def test_every_entry_the_python_sources_name_is_declared():
    used = set()
    for path in glob.glob(os.path.join(ROOT, "fastvocoder_amd", "**", "*.py"), recursive=True):
        with open(path) as fh:
            text = fh.read()
        used |= set(re.findall(r"\.(fv_[a-z0-9_]+)\b", text))             # lib().fv_x, L.fv_x
        used |= set(re.findall(r"[\"'](fv_[a-z0-9_]+)[\"']", text))       # getattr(lib(), entry) of the weight-gradient wrappers
    assert {"fv_conv1d_fused", "fv_plan_run_aux","fv_period_conv_weight_grad_bf16", "fv_mpd_first_weight_grad",
            "fv_conv_transpose1d_weight_grad_bf16_workspace_bytes"} <= used and len(used) > 100
    assert used <= set(_abi.prototypes()), sorted(used - set(_abi.prototypes()))


def test_four_signatures_checked_by_hand():
    lib = _native.lib()
    assert list(lib.fv_adam_step.argtypes) == [vp, vp, i, i64, vp, d, d, d, vp] and lib.fv_adam_step.restype is i
    assert list(lib.fv_stft_distance.argtypes) == [vp, vp, vp, i, i64, i, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    assert list(lib.fv_plan_slot_shape.argtypes) == [vp, i, i, vp, vp]
    assert list(lib.fv_conv1d_fused.argtypes) == [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, f, f, i, f, vp]
    assert len(lib.fv_conv1d_fused.argtypes) == 21
    assert lib.fv_plan_workspace_bytes.restype is i64 and lib.fv_plan_create.restype is vp
    assert lib.fv_plan_destroy.restype is None and lib.fv_last_error.restype is cp and lib.fv_build_id.restype is cp
    assert list(lib.fv_tuning_set.argtypes) == [cp, i]


def test_c_void_p_takes_what_the_wrappers_pass():
    """None, an address, a ctypes array of any element type and byref(...): what the call sites give a pointer parameter."""
    conv = ctypes.c_void_p.from_param
    for value in (None, 4096, (ctypes.c_int * 3)(1, 2, 3), (ctypes.c_void_p * 2)(), (ctypes.c_double * 1)(),
                  ctypes.byref(ctypes.c_int64(0)), ctypes.create_string_buffer(8), ctypes.c_void_p(4096)):
        conv(value)


def test_the_python_constants_are_the_headers():
    consts = _abi.constants()
    mirrored = [n[3:] for n in consts if hasattr(_native, n[3:])]
    assert len(mirrored) >= 40 and {"ABI_VERSION", "ERR_RANGE_LOW", "GUARD_LOW", "SLOT_OUT2", "KERNEL_MRF32", "ADAM_CHUNK",
                                    "DISC_MAX_MAPS", "PCM_S16", "RESAMPLE_MAX_WINDOW"} <= set(mirrored)
    for name in mirrored:
        assert getattr(_native, name) == consts["FV_" + name], name
    assert (_native.ERR_INVALID_ARG, _native.SLOT_NONE, _native.GUARD_LOW, _native.MAX_SLOTS) == (-1, -1, 0x100, 32)
