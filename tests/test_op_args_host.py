"""CPU-only tests of the argument contract of the forward operators, through their plan entries.

A plan entry (fv_plan_add_*) never launches anything and never dereferences a tensor pointer, so a dummy non-null address
serves as weights and the whole contract runs without a GPU.  The plan entry and its direct twin describe the op through
one builder (csrc/api_internal.h build_*), so what is pinned here is the direct entries' shape contract too; where the
two differ on purpose the plan side is pinned as it is.

For every plan entry: one minimal valid call returns 0 and adds one op; each call of a list, wrong in exactly one
argument, returns the code named next to it and adds no op."""
import ctypes

import pytest

from fastvocoder_amd import _native

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, _native.ERR_INVALID_ARG, _native.ERR_UNSUPPORTED, _native.ERR_WORKSPACE
NONE, IN, OUT = _native.SLOT_NONE, _native.SLOT_IN, _native.SLOT_OUT
F32, SPLIT = _native.PAIR_F32, _native.PAIR_SPLIT_F16
ZERO, REFLECT, CAUSAL = _native.PAD_ZERO, _native.PAD_REFLECT, _native.PAD_CAUSAL
W = ctypes.c_void_p(16)          # "weights": never dereferenced by a plan entry


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def ptrs(*v):
    return (ctypes.c_void_p * len(v))(*[p.value if isinstance(p, ctypes.c_void_p) else p for p in v])


K3, D3 = ints(3, 7, 11), ints(1, 3, 5)


def stage_bytes():
    return _native.lib().fv_mrf_stage_workspace_bytes(32)


# entry -> (its arguments behind the plan, in order, with the values of the minimal valid call,
#           [(what is wrong, {argument: value}, code)])
ENTRIES = {
    "fv_plan_add_conv1d": (
        dict(x=IN, y=2, y_act=NONE, res=NONE, acc=NONE, acc2=NONE, packed=W, bias=None, Cin=20, Cout=12, k=7, dil=3, pad=9,
             pad_mode=ZERO, pre_slope=0.1, out_div=1.0, post=0, act_slope=1.0),
        [("no input channels", dict(Cin=0), INVALID), ("no output channels", dict(Cout=0), INVALID),
         ("no taps", dict(k=0), INVALID), ("no dilation", dict(dil=0), INVALID),
         ("pad mode out of range", dict(pad_mode=4), INVALID), ("negative pad mode", dict(pad_mode=-1), INVALID),
         ("causal pad too small", dict(pad_mode=CAUSAL, pad=8), INVALID), ("null weights", dict(packed=None), INVALID),
         ("writes the input slot", dict(y=IN), INVALID), ("slot out of range", dict(x=_native.MAX_SLOTS), INVALID),
         ("causal pad that is large enough", dict(pad_mode=CAUSAL, pad=9), OK),
         ("reflection padding", dict(Cin=16, Cout=16, k=3, dil=9, pad=9, pad_mode=REFLECT), OK)]),
    "fv_plan_add_conv_transpose1d": (
        dict(x=IN, y=2, y_act=NONE, packed=W, bias=None, Cin=64, Cout=32, k=7, stride=3, pad=2, out_pad=1, pre_slope=0.1, post=0,
             act_slope=1.0),
        [("no output channels", dict(Cout=0), INVALID), ("no taps", dict(k=0), INVALID), ("no stride", dict(stride=0), INVALID),
         ("negative pad", dict(pad=-1), INVALID), ("out_pad below -stride", dict(out_pad=-4), INVALID),
         ("null weights", dict(packed=None), INVALID),
         # the direct entry refuses out_pad >= stride, this one takes it
         ("out_pad == stride", dict(out_pad=3), OK), ("out_pad above the stride", dict(out_pad=5), OK),
         ("out_pad == -stride", dict(out_pad=-3), OK)]),
    "fv_plan_add_upsample_conv1d": (
        dict(x=IN, y=2, y_act=NONE, packed=W, bias=None, Cin=20, Cout=12, k=16, rate=8, pad=7, pre_slope=0.1, post=0, act_slope=1.0),
        [("no rate", dict(rate=0), INVALID), ("negative pad", dict(pad=-1), INVALID), ("no taps", dict(k=0), INVALID),
         ("no input channels", dict(Cin=0), INVALID)]),
    "fv_plan_add_conv1d_2src": (
        dict(x=IN, x2=2, y=3, y_act=NONE, res=NONE, packed=W, bias=None, Cin1=16, Cin2=16, Cout=12, post=0, act_slope=1.0),
        [("first source without channels", dict(Cin1=0), INVALID), ("second source without channels", dict(Cin2=0), INVALID),
         ("no output channels", dict(Cout=0), INVALID), ("no second source", dict(x2=NONE), INVALID),
         ("null weights", dict(packed=None), INVALID)]),
    "fv_plan_add_conv1x1_2src_split_f16": (
        dict(x=IN, x2=2, y=3, y_act=NONE, res=NONE, packed=W, bias=None, C=128, pre_slope=0.2, post=0, act_slope=1.0),
        # C is checked here when the op is added (the direct entry leaves it to the launcher)
        [("unsupported channel count", dict(C=64), UNSUPPORTED), ("no channels", dict(C=0), UNSUPPORTED),
         ("no second source", dict(x2=NONE), INVALID), ("256 channels", dict(C=256), OK), ("512 channels", dict(C=512), OK)]),
    "fv_plan_add_conv_transpose1d_split_f16": (
        dict(x=IN, y=2, y_act=NONE, packed=W, bias=None, Cin=64, Cout=32, k=6, stride=3, pad=2, out_pad=1, pre_slope=0.1, act_slope=1.0),
        [("unsupported channel count", dict(Cin=48), UNSUPPORTED), ("k != 2 * stride", dict(k=7), UNSUPPORTED),
         ("stride out of range", dict(k=2, stride=1), UNSUPPORTED), ("Cout * stride < 32", dict(Cout=8), UNSUPPORTED),
         ("pad above the stride", dict(pad=4), INVALID), ("out_pad == stride", dict(out_pad=3), INVALID),
         ("32 -> 16 channels with pad != 1", dict(Cin=32, Cout=16, k=4, stride=2, pad=0, out_pad=0), UNSUPPORTED),
         ("32 -> 16 channels with out_pad != 0", dict(Cin=32, Cout=16, k=4, stride=2, pad=1, out_pad=1), UNSUPPORTED),
         ("32 -> 16 channels, pad 1", dict(Cin=32, Cout=16, k=4, stride=2, pad=1, out_pad=0), OK)]),
    "fv_plan_add_residual_stack_split_f16": (
        dict(x=IN, y=2, y_act=NONE, packed=W, bias_dilated=None, bias_out=None, C=64, k=3, dil=3, slope=0.2, pad_mode=REFLECT, post=0,
             act_slope=1.0),
        [("unsupported channel count", dict(C=16), UNSUPPORTED), ("512 channels", dict(C=512), UNSUPPORTED),
         ("unsupported taps", dict(k=5), UNSUPPORTED), ("even taps", dict(k=4), UNSUPPORTED),
         ("unsupported dilation", dict(dil=5), UNSUPPORTED), ("causal padding", dict(pad_mode=CAUSAL), UNSUPPORTED),
         ("pad mode out of range", dict(pad_mode=4), UNSUPPORTED), ("slope above 1", dict(slope=1.5), INVALID),
         ("negative activation slope", dict(act_slope=-0.1), INVALID), ("unknown post op", dict(post=3), INVALID),
         ("dilation 9, 32 channels", dict(C=32, dil=9), OK), ("256 channels, ReLU behind", dict(C=256, post=_native.POST_RELU), OK)]),
    "fv_plan_add_conv_post_pqmf": (
        dict(x=IN, y=OUT, packed=W, bias=None, Cin=16, S=4, k=7, pad=3, pre_slope=0.01, post=1, h=W, ntaps=63),
        [("S != 4", dict(S=2), UNSUPPORTED), ("ntaps != 63", dict(ntaps=31), UNSUPPORTED),
         # FV_ERR_INVALID_ARG from the direct entry
         ("null filter", dict(h=None), UNSUPPORTED),
         ("even taps", dict(k=6, pad=2), INVALID), ("not a 'same' conv", dict(pad=4), INVALID),
         ("no input channels", dict(Cin=0), INVALID), ("null weights", dict(packed=None), INVALID)]),
    "fv_plan_add_pqmf_synthesis": (
        dict(x=IN, y=OUT, h=W, S=4, ntaps=63),
        [("even tap count", dict(ntaps=62), INVALID), ("no taps", dict(ntaps=0), INVALID), ("no sub-bands", dict(S=0), INVALID),
         ("null filter", dict(h=None), INVALID), ("slot out of range", dict(y=_native.MAX_SLOTS), INVALID)]),
    "fv_plan_add_resblock_pair": (
        dict(x=IN, y=2, y_act=NONE, packed1=W, packed2=W, bias1=None, bias2=None, C=16, k=3, dil=3, slope=0.1, act_slope=1.0),
        [("unsupported channel count", dict(C=48), UNSUPPORTED), ("64 channels in fp32", dict(C=64), UNSUPPORTED),
         ("unsupported taps", dict(k=5), UNSUPPORTED), ("even taps", dict(k=4), UNSUPPORTED),
         ("unsupported dilation", dict(dil=2), UNSUPPORTED), ("null weights", dict(packed2=None), INVALID)]),
    "fv_plan_add_resblock_pair_ex": (
        dict(x=IN, y=2, y_act=NONE, mid=NONE, add1=NONE, add2=NONE, packed1=W, packed2=W, bias1=None, bias2=None, C=16, k=3, dil=3,
             slope=0.1, out_div=1.0, post=0, act_slope=1.0, prec=F32),
        [("unsupported channel count", dict(C=48), UNSUPPORTED), ("64 channels in fp32", dict(C=64, mid=4), UNSUPPORTED),
         ("unsupported taps", dict(k=5), UNSUPPORTED), ("unsupported dilation", dict(dil=9), UNSUPPORTED),
         # the next four are refused here; the direct entry leaves them to the launchers
         ("unknown arithmetic", dict(prec=7), INVALID), ("FV_PAIR_F32 with an addend", dict(add1=3), UNSUPPORTED),
         ("FV_PAIR_F32 with out_div", dict(out_div=3.0), UNSUPPORTED), ("FV_PAIR_F32 with a post op", dict(post=1), UNSUPPORTED),
         ("a scratch slot at C = 16", dict(prec=SPLIT, mid=4), INVALID), ("no scratch slot at C = 64", dict(prec=SPLIT, C=64), INVALID),
         ("add2 without add1", dict(prec=SPLIT, add2=3), INVALID), ("writes the input slot", dict(y=IN), INVALID),
         ("64 channels, split-f16, both addends", dict(prec=SPLIT, C=64, mid=4, add1=IN, add2=3, out_div=3.0, post=1), OK),
         ("512 channels, split-f16", dict(prec=SPLIT, C=512, mid=4), OK)]),
    "fv_plan_add_conv1d_split_f16": (
        dict(x=IN, y=2, y_act=NONE, res=NONE, add1=NONE, add2=NONE, packed=W, bias=None, C=64, k=3, dil=9, pad_mode=REFLECT,
             pre_slope=0.2, out_div=1.0, post=0, act_slope=1.0),
        [("unsupported channel count", dict(C=32), UNSUPPORTED), ("unsupported taps", dict(k=5), UNSUPPORTED),
         ("even taps", dict(k=4), UNSUPPORTED), ("unsupported dilation", dict(dil=2), UNSUPPORTED),
         ("dilation 9 with 7 taps", dict(k=7), UNSUPPORTED), ("causal padding", dict(pad_mode=CAUSAL), UNSUPPORTED),
         ("add2 without add1", dict(add2=3), INVALID), ("the output aliases the residual", dict(res=2), INVALID),
         ("the output aliases an addend", dict(add1=2), INVALID), ("null weights", dict(packed=None), INVALID),
         ("128 channels, 7 taps, dilation 3", dict(C=128, k=7, dil=3, pad_mode=ZERO), OK)]),
    "fv_plan_add_mrf_sum": (
        dict(xs=ints(IN, 2, 3), y=4, y_act=NONE, packed1=ptrs(W, W, W), packed2=ptrs(W, W, W), bias1=None, bias2=None, C=16, k=K3,
             dil=1, slope=0.1, out_div=3.0, post=0, act_slope=1.0),
        # 32 channels are refused here when the op is added (the direct entry leaves them to the launcher)
        [("32 channels", dict(C=32), UNSUPPORTED), ("unsupported channel count", dict(C=48), UNSUPPORTED),
         ("unsupported taps", dict(k=ints(3, 5, 11)), UNSUPPORTED), ("unsupported dilation", dict(dil=2), UNSUPPORTED),
         ("a member without weights", dict(packed1=ptrs(W, None, W)), INVALID),
         ("member slot out of range", dict(xs=ints(IN, 40, 3)), INVALID), ("null taps", dict(k=None), INVALID)]),
    "fv_plan_add_mrf_stage_split_f16": (
        dict(x=IN, y=2, y_act=NONE, packed=W, C=16, k=K3, dil=D3, slope=0.1, out_div=3.0, post=0, act_slope=1.0, workspace=None,
             workspace_bytes=0),
        [("unsupported channel count", dict(C=64), UNSUPPORTED), ("unsupported taps", dict(k=ints(3, 7, 9)), UNSUPPORTED),
         ("unsupported dilations", dict(dil=ints(1, 3, 9)), UNSUPPORTED), ("slope above 1", dict(slope=1.5), INVALID),
         ("activation slope above 1", dict(act_slope=2.0), INVALID), ("unknown post op", dict(post=5), INVALID),
         ("null taps", dict(k=None), INVALID), ("null weights", dict(packed=None), INVALID),
         # the workspace is checked here when the op is added (the direct entry leaves it to the launcher)
         ("32 channels without a workspace", dict(C=32), WORKSPACE),
         ("a workspace that is too small", lambda: dict(C=32, workspace=W, workspace_bytes=stage_bytes() - 1), WORKSPACE),
         ("a null workspace of the right size", lambda: dict(C=32, workspace_bytes=stage_bytes()), WORKSPACE),
         ("32 channels with their workspace", lambda: dict(C=32, workspace=W, workspace_bytes=stage_bytes()), OK),
         ("taps in another order", dict(k=ints(11, 3, 7)), OK)]),
    "fv_plan_add_mrf_stage_classes_f16": (
        dict(x=IN, ys=OUT, yr2=2, packed=W, C=32, k=K3, dil=D3, slope=0.1, workspace=W, workspace_bytes=None),
        [("16 channels", dict(C=16), UNSUPPORTED), ("no second output", dict(yr2=NONE), UNSUPPORTED),
         ("one slot for both outputs", dict(yr2=OUT), UNSUPPORTED), ("taps out of order", dict(k=ints(7, 3, 11)), UNSUPPORTED),
         ("unsupported dilations", dict(dil=ints(1, 3, 9)), UNSUPPORTED), ("slope above 1", dict(slope=1.5), INVALID),
         ("a workspace that is too small", lambda: dict(workspace_bytes=stage_bytes() - 1), WORKSPACE),
         ("a null workspace", dict(workspace=None), WORKSPACE)]),
}


def _call(L, plan, entry, changed):
    args = dict(ENTRIES[entry][0])
    if "workspace_bytes" in args and args["workspace_bytes"] is None:
        args["workspace_bytes"] = stage_bytes()
    args.update(changed() if callable(changed) else changed)
    return getattr(L, entry)(plan, *args.values())


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_minimal_valid_call_adds_one_op(entry):
    L = _native.lib()
    plan = L.fv_plan_create(20)
    try:
        assert _call(L, plan, entry, {}) == OK, L.fv_last_error()
        assert L.fv_plan_num_ops(plan) == 1
    finally:
        L.fv_plan_destroy(plan)


@pytest.mark.parametrize("entry,what,changed,code",
                         [(e, what, changed, code) for e in sorted(ENTRIES) for what, changed, code in ENTRIES[e][1]],
                         ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_call_wrong_in_one_argument(entry, what, changed, code):
    L = _native.lib()
    plan = L.fv_plan_create(20)
    try:
        assert _call(L, plan, entry, {}) == OK
        assert _call(L, plan, entry, changed) == code, (what, L.fv_last_error())
        assert L.fv_plan_num_ops(plan) == (2 if code == OK else 1), what      # a rejected call leaves the plan as it was
    finally:
        L.fv_plan_destroy(plan)


def test_null_plan_is_refused_by_every_entry():
    L = _native.lib()
    for entry in sorted(ENTRIES):
        assert _call(L, None, entry, {}) == INVALID, entry


def test_error_text_names_what_is_wrong():
    """The fragments other tests and callers match, from the plan side."""
    L = _native.lib()
    plan = L.fv_plan_create(20)
    try:
        for entry, changed, text in [
                ("fv_plan_add_conv_post_pqmf", dict(pad=4), b"pad = (k - 1) / 2"),
                ("fv_plan_add_conv1d", dict(pad_mode=4), b"pad_mode"),
                ("fv_plan_add_conv1d", dict(pad_mode=CAUSAL, pad=8), b"causal conv"),
                ("fv_plan_add_conv1d_split_f16", dict(C=32), b"64, 128, 256 or 512"),
                ("fv_plan_add_conv1d_split_f16", dict(k=7), b"dilation 9"),
                ("fv_plan_add_conv1d_split_f16", dict(pad_mode=CAUSAL), b"pad_mode"),
                ("fv_plan_add_conv_transpose1d_split_f16", dict(Cin=48), b"Cin = 48"),
                ("fv_plan_add_conv_transpose1d_split_f16", dict(pad=4), b"pad="),
                ("fv_plan_add_residual_stack_split_f16", dict(dil=5), b"dilation 5"),
                ("fv_plan_add_residual_stack_split_f16", dict(pad_mode=CAUSAL), b"pad_mode"),
                ("fv_plan_add_resblock_pair_ex", dict(k=5), b"resblock pair: 5 taps (3, 7 or 11)"),
                ("fv_plan_add_resblock_pair_ex", dict(dil=2), b"resblock pair: dilation 2 (1, 3 or 5)"),
                ("fv_plan_add_resblock_pair_ex", dict(C=64, mid=4), b"C = 64"),
                ("fv_plan_add_resblock_pair_ex", dict(prec=SPLIT, C=64), b"scratch"),
                ("fv_plan_add_resblock_pair_ex", dict(add1=3), b"SPLIT_F16 only"),
                ("fv_plan_add_resblock_pair_ex", dict(prec=SPLIT, add2=3), b"add2 without add1"),
                ("fv_plan_add_mrf_stage_split_f16", dict(dil=ints(1, 3, 9)), b"dilations"),
                ("fv_plan_add_mrf_stage_split_f16", dict(slope=1.5), b"slope outside [0, 1]"),
                ("fv_plan_add_mrf_stage_split_f16", dict(C=32), b"fv_mrf_stage_workspace_bytes")]:
            assert _call(L, plan, entry, changed) != OK
            assert text in L.fv_last_error(), (entry, changed, L.fv_last_error())
        assert L.fv_plan_num_ops(plan) == 0
    finally:
        L.fv_plan_destroy(plan)


def test_slots_an_entry_does_not_take_are_none():
    """An op reads only the slots its entry was given: a plan of one transposed conv infers its shape with nothing but
    the input set, and an entry without an activated twin has none."""
    L = _native.lib()
    plan = L.fv_plan_create(64)
    try:
        assert _call(L, plan, "fv_plan_add_conv_transpose1d", dict(y=OUT)) == OK
        c, n = ctypes.c_int(), ctypes.c_int64()
        assert L.fv_plan_output_shape(plan, 6, ctypes.byref(c), ctypes.byref(n)) == OK, L.fv_last_error()
        assert (c.value, n.value) == (32, (6 - 1) * 3 - 2 * 2 + 7 + 1)
        assert L.fv_plan_slot_shape(plan, 6, 2, ctypes.byref(c), ctypes.byref(n)) != OK      # never written
    finally:
        L.fv_plan_destroy(plan)
