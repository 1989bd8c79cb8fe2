// The plan executor of libfastvocoder_hip.so (include/fastvocoder_hip.h, fv_plan_*): a recorded sequence of ops over numbered
// slots; one shape rule (set_shapes) for inference and run, one workspace arena (arena) for fv_plan_workspace_bytes and the
// run; and the run itself: fv_plan_run_aux dispatches to one function per kind of launch (run_*), groups of ops included.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "api_internal.h"
#include "launch_host.hpp"

using namespace fv;

namespace fv {

// Channels of an op's result: its residual / running-sum inputs and the activated twin have them, and so has y unless an
// output conv is folded in (set_shapes).  The PQMF ops write the one full-band channel.
static int out_channels(const Op& o) { return (o.type == OP_PQMF || o.pq_h) ? 1 : o.Cout; }

static void put_shape(Shape* sh, int64_t* slot_elems, int B, int slot, int C, int64_t T) {
    sh[slot] = {C, T, true};
    const int64_t e = (int64_t)B * C * T;
    if (slot_elems && e > slot_elems[slot]) slot_elems[slot] = e;
}

// The one shape rule: everything op `o` writes, from its input's shape in sh[] -- the scratch tensors of the two-launch
// forms (sum3: tmpb / tmpc; a wide pair's intermediate tmpb; a residual stack's hidden tensor alt_mid; each [Cout, Tin]),
// y and the activated twin y2.  infer() passes slot_elems (the slots' largest uses over B utterances); the run, which
// walks the ops again because a reused slot changes shape, does not.
static void set_shapes(const Op& o, Shape* sh, int64_t* slot_elems = nullptr, int B = 0) {
    const int64_t Tin = sh[o.x].T, Tout = conv_out_len(o, Tin);
    const int scratch[3] = {o.sum3 || o.type == OP_PAIR ? o.tmpb : FV_SLOT_NONE, o.sum3 ? o.tmpc : FV_SLOT_NONE,
                            o.type == OP_STACK ? o.alt_mid : FV_SLOT_NONE};
    for (int t : scratch)
        if (t != FV_SLOT_NONE) put_shape(sh, slot_elems, B, t, o.Cout, Tin);
    put_shape(sh, slot_elems, B, o.y, o.fold_w ? 1 : out_channels(o), Tout);
    if (o.y2 != FV_SLOT_NONE) put_shape(sh, slot_elems, B, o.y2, out_channels(o), Tout);
}

static void reset_shapes(const fv_plan* plan, int T, Shape* sh) {
    for (int i = 0; i < FV_MAX_SLOTS; ++i) sh[i].set = false;
    sh[FV_SLOT_IN] = {plan->in_channels, T, true};
}

// Propagate shapes through the op list: every op's checks, then set_shapes; fills per-slot max element counts.
static int infer(const fv_plan* plan, int B, int T, Shape* sh, int64_t* slot_elems) {
    for (int i = 0; i < FV_MAX_SLOTS; ++i) slot_elems[i] = 0;
    reset_shapes(plan, T, sh);
    for (size_t n = 0; n < plan->ops.size(); ++n) {
        const Op& o = plan->ops[n];
        if (o.x == FV_SLOT_AUX_IN0 || o.x == FV_SLOT_AUX_IN1 || o.y == FV_SLOT_AUX_IN0 || o.y == FV_SLOT_AUX_IN1 ||
            o.y2 == FV_SLOT_AUX_IN0 || o.y2 == FV_SLOT_AUX_IN1)
            return fail(FV_ERR_INVALID_ARG, "op %zu: the auxiliary input slots can only be output offsets", n);
        if (!sh[o.x].set) return fail(FV_ERR_INVALID_ARG, "op %zu reads unset slot %d", n, o.x);
        const int cin_x = o.x2 == FV_SLOT_NONE ? o.Cin : o.Cin1;
        if (sh[o.x].C != cin_x)
            return fail(FV_ERR_INVALID_ARG, "op %zu: slot %d has %d channels, op expects %d", n,
                        o.x, sh[o.x].C, cin_x);
        if (o.x2 != FV_SLOT_NONE &&
            (!sh[o.x2].set || sh[o.x2].C != o.Cin - o.Cin1 || sh[o.x2].T != sh[o.x].T))
            return fail(FV_ERR_INVALID_ARG, "op %zu: second input slot %d must be [%d, T] like the first", n,
                        o.x2, o.Cin - o.Cin1);
        const int64_t Tout = conv_out_len(o, sh[o.x].T);
        if (Tout <= 0) return fail(FV_ERR_INVALID_ARG, "op %zu: empty output (T=%lld)", n, (long long)sh[o.x].T);
        const int aux[3] = {o.res, o.acc, o.acc2};
        for (int a = 0; a < 3; ++a) {
            if (aux[a] == FV_SLOT_NONE) continue;
            if (!sh[aux[a]].set || sh[aux[a]].C != out_channels(o) || sh[aux[a]].T != Tout)
                return fail(FV_ERR_INVALID_ARG, "op %zu: residual/accumulator slot %d shape mismatch", n, aux[a]);
        }
        if (o.in_merge) {
            const int extra[2] = {o.xb, o.xc};
            for (int e = 0; e < 2; ++e)
                if (extra[e] != FV_SLOT_NONE && (!sh[extra[e]].set || sh[extra[e]].C != o.Cin || sh[extra[e]].T != sh[o.x].T ||
                                                 extra[e] == o.y || extra[e] == o.y2))
                    return fail(FV_ERR_INVALID_ARG, "op %zu: merged input slot %d must be [%d, T] like the first and not the output",
                                n, extra[e], o.Cin);
        }
        if (o.type == OP_MRFSUM) {
            const int extra[2] = {o.xb, o.xc};
            for (int e = 0; e < 2; ++e)
                if (!sh[extra[e]].set || sh[extra[e]].C != o.Cin || sh[extra[e]].T != sh[o.x].T || extra[e] == o.y ||
                    extra[e] == o.y2)
                    return fail(FV_ERR_INVALID_ARG, "op %zu: mrf member slot %d must be [%d, T] and not the output", n,
                                extra[e], o.Cin);
        }
        if (o.sum3) {
            const int extra[4] = {o.xb, o.xc, o.resb, o.resc};
            for (int e = 0; e < 4; ++e)
                if (!sh[extra[e]].set || sh[extra[e]].C != o.Cin || sh[extra[e]].T != sh[o.x].T || extra[e] == o.y ||
                    extra[e] == o.y2)
                    return fail(FV_ERR_INVALID_ARG, "op %zu: sum3 member slot %d must be [%d, T] and not the output",
                                n, extra[e], o.Cin);
        }
        if (o.sum3) {   // the scratch tensors of the two-launch form
            const int t2[2] = {o.tmpb, o.tmpc};
            for (int e = 0; e < 2; ++e)
                if (t2[e] == o.x || t2[e] == o.xb || t2[e] == o.xc || t2[e] == o.res || t2[e] == o.resb ||
                    t2[e] == o.resc || t2[e] == o.y || t2[e] == o.y2 || t2[e] == FV_SLOT_IN)
                    return fail(FV_ERR_INVALID_ARG, "op %zu: sum3 scratch slot %d aliases an operand", n, t2[e]);
        }
        if (o.type == OP_STACK && o.alt_mid != FV_SLOT_NONE &&   // hidden tensor of the two-launch form
            (o.alt_mid == o.x || o.alt_mid == o.y || o.alt_mid == o.y2 || o.alt_mid == FV_SLOT_IN))
            return fail(FV_ERR_INVALID_ARG, "op %zu: stack scratch slot %d aliases an operand", n, o.alt_mid);
        if (o.type == OP_PAIR && o.tmpb != FV_SLOT_NONE &&       // intermediate of a two-launch (C >= 64) pair
            (o.tmpb == o.x || o.tmpb == o.y || o.tmpb == o.y2 || o.tmpb == o.acc || o.tmpb == o.acc2 || o.tmpb == FV_SLOT_IN))
            return fail(FV_ERR_INVALID_ARG, "op %zu: pair scratch slot %d aliases an operand", n, o.tmpb);
        if (o.y == o.x || o.y == o.x2) return fail(FV_ERR_INVALID_ARG, "op %zu: output aliases input", n);
        if (o.y2 != FV_SLOT_NONE && (o.y2 == o.x || o.y2 == o.y || o.y2 == o.x2))
            return fail(FV_ERR_INVALID_ARG, "op %zu: activated twin aliases another tensor of the op", n);
        set_shapes(o, sh, slot_elems, B);
    }
    return 0;
}

// The workspace arena: the temporary slots one after the other, each sized by its largest use and 256-byte aligned.
// Returns the bytes needed; with `base`, also writes the slots' addresses inside `workspace`.
static int64_t arena(const int64_t* slot_elems, void* workspace = nullptr, float** base = nullptr) {
    int64_t off = 0;
    for (int i = FV_SLOT_TMP0; i < FV_SLOT_AUX_IN0; ++i) {
        if (base) base[i] = reinterpret_cast<float*>(static_cast<char*>(workspace) + off);
        off += (slot_elems[i] * 4 + 255) / 256 * 256;
    }
    return off;
}

}  // namespace fv

extern "C" {

int fv_plan_add_upsample_conv1d(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot,
                                const float* packed, const float* bias, int Cin, int Cout, int k,
                                int rate, int pad, float pre_slope, int post, float act_slope) {
    if (int rc = fv_plan_add_conv_transpose1d(plan, x_slot, y_slot, y_act_slot, packed, bias, Cin, Cout, k,
                                              rate, pad, 0, pre_slope, post, act_slope))
        return rc;
    plan->ops.back().type = OP_UPCONV;
    return 0;
}

fv_plan_t* fv_plan_create(int in_channels) {
    fv_plan* p = new fv_plan();
    p->in_channels = in_channels;
    return p;
}

void fv_plan_destroy(fv_plan_t* plan) {
    delete plan;
}

static int check_slot(int s, bool allow_none) {
    if (s == FV_SLOT_NONE && allow_none) return 0;
    if (s < 0 || s >= FV_MAX_SLOTS) return fail(FV_ERR_INVALID_ARG, "slot %d out of range", s);
    return 0;
}

// What every fv_plan_add_* function ends with: the slot checks they share (x and y are slots, y_act and the optional ones
// slots or FV_SLOT_NONE, and no op writes the plan's input), the op's slots, the push
static int push(fv_plan* plan, Op& o, int x, int y, int y_act, int res = FV_SLOT_NONE, int acc = FV_SLOT_NONE,
                int acc2 = FV_SLOT_NONE) {
    if (int rc = check_slot(x, false)) return rc;
    if (int rc = check_slot(y, false)) return rc;
    for (int s : {y_act, res, acc, acc2})
        if (int rc = check_slot(s, true)) return rc;
    if (y == FV_SLOT_IN || y_act == FV_SLOT_IN) return fail(FV_ERR_INVALID_ARG, "plan: the input slot is read-only");
    o.x = x;
    o.y = y;
    o.y2 = y_act;
    o.res = res;
    o.acc = acc;
    o.acc2 = acc2;
    plan->ops.push_back(o);
    return 0;
}

int fv_plan_add_conv1d(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot, int res_slot,
                       int acc_slot, int acc2_slot, const float* packed, const float* bias, int Cin,
                       int Cout, int k, int dil, int pad, int pad_mode, float pre_slope, float out_div,
                       int post, float act_slope) {
    if (!plan || !packed) return fail(FV_ERR_INVALID_ARG, "plan_add_conv1d: null");
    Op o = {};
    if (int rc = build_conv(o, packed, bias, Cin, Cout, k, dil, pad, pad_mode, pre_slope, out_div, post, act_slope)) return rc;
    o.group = plan->cur_group;
    o.own_first = plan->cur_own_first;
    return push(plan, o, x_slot, y_slot, y_act_slot, res_slot, acc_slot, acc2_slot);
}

int fv_plan_add_conv1d_sum3(fv_plan_t* plan, const int* x_slots, const int* res_slots, const int* tmp_slots,
                            int y_slot, int y_act_slot, const float* const* packed, const float* bias_sum,
                            int C, const int* k, float out_div, int post, float act_slope) {
    if (!plan || !x_slots || !res_slots || !tmp_slots || !packed || !k)
        return fail(FV_ERR_INVALID_ARG, "plan_add_conv1d_sum3: null");
    for (int j = 0; j < 2; ++j)
        if (int rc = check_slot(tmp_slots[j], false)) return rc;
    for (int j = 0; j < 3; ++j) {
        if (!packed[j] || k[j] < 1 || k[j] % 2 == 0)
            return fail(FV_ERR_INVALID_ARG, "plan_add_conv1d_sum3: member %d needs packed weights and an odd tap count", j);
        if (int rc = check_slot(x_slots[j], false)) return rc;
        if (int rc = check_slot(res_slots[j], false)) return rc;
    }
    if (int rc = fv_plan_add_conv1d(plan, x_slots[0], y_slot, y_act_slot, res_slots[0], FV_SLOT_NONE, FV_SLOT_NONE,
                                    packed[0], bias_sum, C, C, k[0], 1, (k[0] - 1) / 2, FV_PAD_ZERO, 1.f, out_div,
                                    post, act_slope))
        return rc;
    Op& o = plan->ops.back();
    o.sum3 = true;
    o.group = 0;
    o.xb = x_slots[1];
    o.xc = x_slots[2];
    o.resb = res_slots[1];
    o.resc = res_slots[2];
    o.wpb = packed[1];
    o.wpc = packed[2];
    o.kb = k[1];
    o.kc = k[2];
    o.tmpb = tmp_slots[0];
    o.tmpc = tmp_slots[1];
    return 0;
}

int fv_plan_add_conv1d_2src(fv_plan_t* plan, int x_slot, int x2_slot, int y_slot, int y_act_slot,
                            int res_slot, const float* packed, const float* bias, int Cin1, int Cin2,
                            int Cout, int post, float act_slope) {
    if (!plan || !packed) return fail(FV_ERR_INVALID_ARG, "plan_add_conv1d_2src: null");
    Op o = {};
    if (int rc = build_conv_2src(o, packed, bias, Cin1, Cin2, Cout, post, act_slope)) return rc;
    if (int rc = check_slot(x2_slot, false)) return rc;
    o.x2 = x2_slot;
    o.own_first = plan->cur_own_first;
    return push(plan, o, x_slot, y_slot, y_act_slot, res_slot);
}

int fv_plan_add_conv1x1_2src_split_f16(fv_plan_t* plan, int x_slot, int x2_slot, int y_slot, int y_act_slot, int res_slot,
                                       const float* packed, const float* bias, int C, float pre_slope, int post,
                                       float act_slope) {
    if (!plan || !packed) return fail(FV_ERR_INVALID_ARG, "plan_add_conv1x1_2src_split_f16: null");
    if (fv_packed_conv1x1_2src_split_floats(C) <= 0)     // this entry alone: fv_conv1x1_2src_split_f16 leaves C to launch_convg
        return fail(FV_ERR_UNSUPPORTED, "plan_add_conv1x1_2src_split_f16: C = %d (128, 256 or 512)", C);
    Op o = {};
    if (int rc = build_convg(o, packed, bias, C, pre_slope, post, act_slope)) return rc;
    if (int rc = check_slot(x2_slot, false)) return rc;
    o.x2 = x2_slot;
    o.own_first = plan->cur_own_first;
    return push(plan, o, x_slot, y_slot, y_act_slot, res_slot);
}

int fv_plan_add_residual_stack_split_f16(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot, const float* packed,
                                         const float* bias_dilated, const float* bias_out, int C, int k, int dil, float slope,
                                         int pad_mode, int post, float act_slope) {
    if (!plan || !packed) return fail(FV_ERR_INVALID_ARG, "plan_add_residual_stack_split_f16: null");
    Op o = {};
    if (int rc = build_stack(o, packed, bias_dilated, bias_out, C, k, dil, slope, pad_mode, post, act_slope)) return rc;
    return push(plan, o, x_slot, y_slot, y_act_slot);
}

int fv_plan_set_stack_two_launch(fv_plan_t* plan, int hidden_slot, const float* packed_dilated, const float* packed_pair) {
    if (!plan || plan->ops.empty() || !packed_dilated || !packed_pair)
        return fail(FV_ERR_INVALID_ARG, "plan_set_stack_two_launch: no op / null weights");
    if (int rc = check_slot(hidden_slot, false)) return rc;
    Op& o = plan->ops.back();
    if (o.type != OP_STACK || fv_packed_conv1x1_2src_split_floats(o.Cout) <= 0 || o.Cout < 128)
        return fail(FV_ERR_UNSUPPORTED, "plan_set_stack_two_launch: the last op must be a residual stack of 128 or 256 channels");
    if (hidden_slot == FV_SLOT_IN || hidden_slot == o.x || hidden_slot == o.y || hidden_slot == o.y2)
        return fail(FV_ERR_INVALID_ARG, "plan_set_stack_two_launch: the scratch slot aliases an operand");
    o.alt_w1 = packed_dilated;
    o.alt_w2 = packed_pair;
    o.alt_mid = hidden_slot;
    return 0;
}

// (any out_pad >= -stride here; fv_conv_transpose1d_fused refuses one of the stride or more)
int fv_plan_add_conv_transpose1d(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot,
                                 const float* packed, const float* bias, int Cin, int Cout, int k,
                                 int stride, int pad, int out_pad, float pre_slope, int post,
                                 float act_slope) {
    if (!plan || !packed) return fail(FV_ERR_INVALID_ARG, "plan_add_conv_transpose1d: null");
    Op o = {};
    if (int rc = build_convt(o, packed, bias, Cin, Cout, k, stride, pad, out_pad, pre_slope, post, act_slope)) return rc;
    return push(plan, o, x_slot, y_slot, y_act_slot);
}

int fv_plan_add_conv_transpose1d_split_f16(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot, const float* packed,
                                           const float* bias, int Cin, int Cout, int k, int stride, int pad,
                                           int out_pad, float pre_slope, float act_slope) {
    if (!plan || !packed) return fail(FV_ERR_INVALID_ARG, "plan_add_conv_transpose1d_split_f16: null");
    Op o = {};
    if (int rc = build_convt_split(o, packed, bias, Cin, Cout, k, stride, pad, out_pad, pre_slope, act_slope)) return rc;
    return push(plan, o, x_slot, y_slot, y_act_slot);
}

int fv_plan_set_input_merge(fv_plan_t* plan, int add1_slot, int add2_slot, float div) {
    if (!plan || plan->ops.empty()) return fail(FV_ERR_INVALID_ARG, "plan_set_input_merge: no op to attach to");
    Op& o = plan->ops.back();
    if (o.type != OP_CONVT || o.prec != FV_PAIR_SPLIT_F16)
        return fail(FV_ERR_UNSUPPORTED, "plan_set_input_merge: the last op is not a split-f16 transposed conv");
    if (add1_slot == FV_SLOT_NONE || add1_slot < 0 || add1_slot >= FV_MAX_SLOTS ||
        (add2_slot != FV_SLOT_NONE && (add2_slot < 0 || add2_slot >= FV_MAX_SLOTS)))
        return fail(FV_ERR_INVALID_ARG, "plan_set_input_merge: slots %d, %d", add1_slot, add2_slot);
    if (!(div > 0.f)) return fail(FV_ERR_INVALID_ARG, "plan_set_input_merge: divisor %g", (double)div);
    o.in_merge = true;
    o.xb = add1_slot;
    o.xc = add2_slot;
    o.out_div = div;
    return 0;
}

int fv_plan_add_conv_post_pqmf(fv_plan_t* plan, int x_slot, int y_slot, const float* packed, const float* bias, int Cin,
                               int S, int k, int pad, float pre_slope, int post, const float* h, int ntaps) {
    if (!plan || !packed) return fail(FV_ERR_INVALID_ARG, "plan_add_conv_post_pqmf: null");
    // this entry alone: a null filter is FV_ERR_INVALID_ARG from fv_conv_post_pqmf
    if (!h) return fail(FV_ERR_UNSUPPORTED, "plan_add_conv_post_pqmf: null filter");
    Op o = {};
    if (int rc = build_conv_post_pqmf(o, packed, bias, h, Cin, S, k, pad, pre_slope, post, ntaps)) return rc;
    o.own_first = plan->cur_own_first;
    return push(plan, o, x_slot, y_slot, FV_SLOT_NONE);
}

// (its two slots may be any, the plan's input included: no push())
int fv_plan_add_pqmf_synthesis(fv_plan_t* plan, int x_slot, int y_slot, const float* h, int S,
                               int ntaps) {
    if (!plan || !h) return fail(FV_ERR_INVALID_ARG, "plan_add_pqmf: null");
    Op o = {};
    if (int rc = build_pqmf(o, h, S, ntaps)) return rc;
    if (int rc = check_slot(x_slot, false)) return rc;
    if (int rc = check_slot(y_slot, false)) return rc;
    o.x = x_slot;
    o.y = y_slot;
    plan->ops.push_back(o);
    return 0;
}

int fv_plan_add_mrf_stage_split_f16(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot, const float* packed, int C,
                                    const int* k, const int* dil, float slope, float out_div, int post, float act_slope,
                                    void* workspace, int64_t workspace_bytes) {
    if (!plan || !packed) return fail(FV_ERR_INVALID_ARG, "plan_add_mrf_stage: null");
    Op o = {};
    if (int rc = build_stage(o, packed, C, k, dil, slope, out_div, post, act_slope, workspace, workspace_bytes)) return rc;
    // this entry alone: fv_mrf_stage_split_f16 leaves the workspace to launch_mrfh
    if (workspace_bytes < mrf_workspace_bytes(C) || (mrf_workspace_bytes(C) > 0 && !workspace))
        return fail(FV_ERR_WORKSPACE, "plan_add_mrf_stage: C = %d needs a workspace of %lld bytes (fv_mrf_stage_workspace_bytes)", C,
                    (long long)mrf_workspace_bytes(C));
    return push(plan, o, x_slot, y_slot, y_act_slot);
}

int fv_plan_add_mrf_stage_classes_f16(fv_plan_t* plan, int x_slot, int ys_slot, int yr2_slot, const float* packed, int C,
                                      const int* k, const int* dil, float slope, void* workspace, int64_t workspace_bytes) {
    if (C != 32 || yr2_slot == FV_SLOT_NONE || yr2_slot == ys_slot)
        return fail(FV_ERR_UNSUPPORTED, "plan_add_mrf_stage_classes: 32 channels and two distinct output slots");
    // the op is an OP_STAGE whose second output slot (Op::y2: elsewhere the activated twin) holds r_2 -- the all-in-one entry's
    // checks of slots, shape and workspace apply as they are, with yr2_slot in its y_act_slot argument; Op::classes tells run_stage
    if (int rc = fv_plan_add_mrf_stage_split_f16(plan, x_slot, ys_slot, yr2_slot, packed, C, k, dil, slope, 1.f, FV_POST_NONE, 1.f,
                                                 workspace, workspace_bytes))
        return rc;
    if (k[0] != 3 || k[1] != 7 || k[2] != 11) {
        plan->ops.pop_back();
        return fail(FV_ERR_UNSUPPORTED, "plan_add_mrf_stage_classes: taps (3, 7, 11) in this order");
    }
    plan->ops.back().classes = true;
    return 0;
}

int fv_plan_add_resblock_pair(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot, const float* packed1,
                              const float* packed2, const float* bias1, const float* bias2, int C, int k, int dil,
                              float slope, float act_slope) {
    return fv_plan_add_resblock_pair_ex(plan, x_slot, y_slot, y_act_slot, FV_SLOT_NONE, FV_SLOT_NONE, FV_SLOT_NONE,
                                        packed1, packed2, bias1, bias2, C, k, dil, slope, 1.f, FV_POST_NONE, act_slope,
                                        FV_PAIR_F32);
}

int fv_plan_add_resblock_pair_ex(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot, int mid_slot, int add1_slot,
                                 int add2_slot, const float* packed1, const float* packed2, const float* bias1,
                                 const float* bias2, int C, int k, int dil, float slope, float out_div, int post,
                                 float act_slope, int prec) {
    if (!plan || !packed1 || !packed2) return fail(FV_ERR_INVALID_ARG, "plan_add_resblock_pair: null");
    Op o = {};
    if (int rc = build_pair(o, 0, &packed1, &packed2, &bias1, &bias2, &k, C, dil, slope, out_div, post, act_slope, prec)) return rc;
    if ((C >= 64) != (mid_slot != FV_SLOT_NONE))
        return fail(FV_ERR_INVALID_ARG, "plan_add_resblock_pair: a scratch slot is needed at C >= 64 and only there");
    if (int rc = check_slot(mid_slot, true)) return rc;
    // the next two are this entry's alone: fv_resblock1_fused_ex leaves them to the launchers
    if (prec != FV_PAIR_F32 && prec != FV_PAIR_SPLIT_F16)
        return fail(FV_ERR_INVALID_ARG, "plan_add_resblock_pair: unknown arithmetic %d", prec);
    if (prec == FV_PAIR_F32 && (add1_slot != FV_SLOT_NONE || add2_slot != FV_SLOT_NONE || out_div != 1.f || post != FV_POST_NONE))
        return fail(FV_ERR_UNSUPPORTED, "plan_add_resblock_pair: add1 / add2 / out_div / post exist with FV_PAIR_SPLIT_F16 only");
    if (int rc = check_adds("plan_add_resblock_pair", add1_slot != FV_SLOT_NONE, add2_slot != FV_SLOT_NONE)) return rc;
    o.tmpb = mid_slot;
    o.group = plan->cur_group;
    return push(plan, o, x_slot, y_slot, y_act_slot, FV_SLOT_NONE, add1_slot, add2_slot);   // (the MRF addends travel as running sums)
}

int fv_plan_add_conv1d_split_f16(fv_plan_t* plan, int x_slot, int y_slot, int y_act_slot, int res_slot, int add1_slot,
                                 int add2_slot, const float* packed, const float* bias, int C, int k, int dil,
                                 int pad_mode, float pre_slope, float out_div, int post, float act_slope) {
    if (!plan || !packed) return fail(FV_ERR_INVALID_ARG, "plan_add_conv1d_split_f16: null");
    Op o = {};
    if (int rc = build_convh(o, 0, &packed, &bias, &k, C, dil, pad_mode, pre_slope, out_div, post, act_slope)) return rc;
    if (int rc = check_adds("plan_add_conv1d_split_f16", add1_slot != FV_SLOT_NONE, add2_slot != FV_SLOT_NONE)) return rc;
    if (y_slot == res_slot || y_slot == add1_slot || y_slot == add2_slot)
        return fail(FV_ERR_INVALID_ARG, "plan_add_conv1d_split_f16: the output aliases an addend");
    o.group = plan->cur_group;
    return push(plan, o, x_slot, y_slot, y_act_slot, res_slot, add1_slot, add2_slot);
}

int fv_plan_add_mrf_sum(fv_plan_t* plan, const int* x_slots, int y_slot, int y_act_slot,
                        const float* const* packed1, const float* const* packed2, const float* const* bias1,
                        const float* const* bias2, int C, const int* k, int dil, float slope, float out_div,
                        int post, float act_slope) {
    if (!plan || !x_slots || !packed1 || !packed2 || !k) return fail(FV_ERR_INVALID_ARG, "plan_add_mrf_sum: null");
    Op o = {};
    if (int rc = build_mrfsum(o, packed1, packed2, bias1, bias2, k, C, dil, slope, out_div, post, act_slope)) return rc;
    if (C != 16) return fail(FV_ERR_UNSUPPORTED, "plan_add_mrf_sum: C = %d (16)", C);     // here when the op is added: fv_mrf_stage leaves 32 channels to launch_pairs
    for (int j = 0; j < 3; ++j) {
        if (!packed1[j] || !packed2[j]) return fail(FV_ERR_INVALID_ARG, "plan_add_mrf_sum: member %d has no weights", j);
        if (int rc = check_slot(x_slots[j], false)) return rc;
    }
    o.xb = x_slots[1];
    o.xc = x_slots[2];
    return push(plan, o, x_slots[0], y_slot, y_act_slot);
}

int fv_plan_set_output_offset(fv_plan_t* plan, int aux_slot, int y2_slot) {
    if (!plan || plan->ops.empty()) return fail(FV_ERR_INVALID_ARG, "plan_set_output_offset: no op to attach to");
    if (aux_slot != FV_SLOT_AUX_IN0 && aux_slot != FV_SLOT_AUX_IN1)
        return fail(FV_ERR_INVALID_ARG, "plan_set_output_offset: slot %d is not an auxiliary input", aux_slot);
    if (int rc = check_slot(y2_slot, true)) return rc;
    Op& o = plan->ops.back();
    if (o.type == OP_PAIR || o.type == OP_MRFSUM || o.type == OP_CONVH || o.sum3 || o.group != 0 ||
        (o.type == OP_CONVT && o.prec == FV_PAIR_SPLIT_F16))   // (a pair with a folded output conv included)
        return fail(FV_ERR_UNSUPPORTED, "plan_set_output_offset: only plain conv / transposed conv / two-source 1x1 / residual stack / pqmf ops carry an offset");
    if (y2_slot != FV_SLOT_NONE) {
        if (o.y2 != FV_SLOT_NONE) return fail(FV_ERR_INVALID_ARG, "plan_set_output_offset: the op already has a second output");
        if (y2_slot == o.y || y2_slot == o.x || y2_slot == FV_SLOT_IN) return fail(FV_ERR_INVALID_ARG, "plan_set_output_offset: y2 aliases");
        o.y2 = y2_slot;
        if (o.type != OP_PQMF) o.act_slope = 1.f;
    }
    o.sub = aux_slot;
    return 0;
}

int fv_plan_set_pair_output_conv(fv_plan_t* plan, const float* w, const float* bias, int y_slot, float act_slope, int post) {
    if (!plan || plan->ops.empty() || !w) return fail(FV_ERR_INVALID_ARG, "plan_set_pair_output_conv: no op / null weights");
    if (int rc = check_slot(y_slot, false)) return rc;
    Op& o = plan->ops.back();
    if ((o.type != OP_PAIR && o.type != OP_STAGE) || o.prec != FV_PAIR_SPLIT_F16 || !(o.Cin == 16 || (o.Cin == 32 && o.type == OP_STAGE)) ||
        o.group != 0 || o.y2 != FV_SLOT_NONE || o.post != FV_POST_NONE || o.fold_w)
        return fail(FV_ERR_UNSUPPORTED, "plan_set_pair_output_conv: the last op must be an ungrouped 16-channel split-f16 "
                    "resblock pair (or a one-launch MRF stage of 16 or 32 channels) without an activated twin or a post op of its own");
    if (y_slot == FV_SLOT_IN || y_slot == o.x || y_slot == o.acc || y_slot == o.acc2 || y_slot == o.tmpb)
        return fail(FV_ERR_INVALID_ARG, "plan_set_pair_output_conv: the output slot aliases an operand");
    if (act_slope < 0.f || act_slope > 1.f) return fail(FV_ERR_INVALID_ARG, "plan_set_pair_output_conv: slope outside [0, 1]");
    o.fold_w = w;
    o.fold_b = bias;
    o.y = y_slot;
    o.act_slope = act_slope;
    o.post = post;
    return 0;
}

int fv_plan_set_group(fv_plan_t* plan, int group) {
    if (!plan || group < 0) return fail(FV_ERR_INVALID_ARG, "plan_set_group: group %d", group);
    plan->cur_group = group;
    return 0;
}

int fv_plan_set_sum_order(fv_plan_t* plan, int own_first) {
    if (!plan) return fail(FV_ERR_INVALID_ARG, "plan_set_sum_order: null plan");
    plan->cur_own_first = own_first ? 1 : 0;
    return 0;
}

int fv_plan_slot_shape(fv_plan_t* plan, int T, int slot, int* channels, int64_t* len) {
    if (!plan) return fail(FV_ERR_INVALID_ARG, "null plan");
    if (int rc = check_slot(slot, false)) return rc;
    Shape sh[FV_MAX_SLOTS];
    int64_t elems[FV_MAX_SLOTS];
    if (int rc = infer(plan, 1, T, sh, elems)) return rc;
    if (!sh[slot].set) return fail(FV_ERR_INVALID_ARG, "plan never writes slot %d", slot);
    if (channels) *channels = sh[slot].C;
    if (len) *len = sh[slot].T;
    return 0;
}

int fv_plan_output_shape(fv_plan_t* plan, int T, int* out_channels, int64_t* out_len) {
    return fv_plan_slot_shape(plan, T, FV_SLOT_OUT, out_channels, out_len);
}

int64_t fv_plan_workspace_bytes(fv_plan_t* plan, int B, int T) {
    if (!plan) return fail(FV_ERR_INVALID_ARG, "null plan");
    Shape sh[FV_MAX_SLOTS];
    int64_t elems[FV_MAX_SLOTS];
    if (int rc = infer(plan, B, T, sh, elems)) return rc < 0 ? rc : -rc;
    return arena(elems);
}

}  // extern "C"

namespace fv {

// ---------------------------------------------------------------------------
// the run: one function per kind of launch; fv_plan_run_aux checks, lays the arena out and dispatches
// ---------------------------------------------------------------------------
// What the branches share.  sh[] holds the shapes in front of the op (or group of ops) being launched.
struct Run {
    const fv_plan* plan;
    int B;
    float* const* base;      // slot -> tensor
    const Shape* sh;
    const int* aux_b;        // auxiliary input 0 / 1 has a batch dimension
    hipStream_t s;
    const Op& op(size_t n) const { return plan->ops[n]; }
    float* at(int slot) const { return ptr(base, slot); }
    int64_t T(const Op& o) const { return sh[o.x].T; }
    int* guard() const { return plan->guard_dev; }
    const float* sub(const Op& o) const { return ptr(base, o.sub); }
    int sub_batched(const Op& o) const { return o.sub == FV_SLOT_NONE ? 0 : aux_b[o.sub - FV_SLOT_AUX_IN0]; }
};

// "Same launch": may op b join the group that op a starts?  One predicate per kernel family -- each lists what ITS launch
// record holds once for all members (the fp32 conv group takes any three convs: every member has a ConvParams of its own).
static bool same_convh(const Op& a, const Op& b) {
    return b.type == OP_CONVH && b.group == a.group && b.Cin == a.Cin && b.dil == a.dil && b.pad_mode == a.pad_mode &&
           b.pre_slope == a.pre_slope && b.act_slope == a.act_slope && b.out_div == a.out_div && b.post == a.post;
}
static bool same_pair(const Op& a, const Op& b) {      // (a pair with a folded output conv runs alone)
    return b.type == OP_PAIR && b.group == a.group && b.Cin == a.Cin && b.dil == a.dil && b.pre_slope == a.pre_slope &&
           b.act_slope == a.act_slope && !a.fold_w && !b.fold_w && b.prec == a.prec && b.out_div == a.out_div && b.post == a.post;
}
static bool same_conv(const Op& a, const Op& b) { return b.type == OP_CONV && b.group == a.group; }

// End of the group that op n starts: up to three consecutive ops with its (non-zero) group id that `same` lets share a launch
static size_t group_end(const fv_plan* plan, size_t n, bool (*same)(const Op&, const Op&)) {
    size_t m = n + 1;
    if (plan->ops[n].group != 0)
        while (m < plan->ops.size() && m - n < 3 && same(plan->ops[n], plan->ops[m])) ++m;
    return m;
}

// split-f16 convs of the wide stages: the members [n, m) of a group in one launch
static int run_convh_group(const Run& r, size_t n, size_t m) {
    const Op& o = r.op(n);
    PairParams pp = pair_params(o, (int)(m - n), r.B, r.T(o), r.guard());
    for (size_t q = n; q < m; ++q) {
        const Op& qo = r.op(q);
        pp.m[q - n] = op_member(qo, 0, r.base[qo.x], r.base[qo.y], r.at(qo.y2), r.at(qo.res), r.at(qo.acc), r.at(qo.acc2));
    }
    return launch_convh(pp, o.Cin, o.dil, r.s);
}

// a whole 16- / 32-channel MRF stage: one launch (with a folded output conv, y is THAT conv's output)
static int run_stage(const Run& r, const Op& o) {
    float* const y = r.base[o.y];
    if (o.classes)
        return launch_mrfw_split(mrf_split_params(o, r.base[o.x], y, r.at(o.y2), r.B, r.T(o), r.guard()), o.sdil, r.s);
    return launch_mrfh(mrf_params(o, r.base[o.x], o.fold_w ? nullptr : y, o.fold_w ? nullptr : r.at(o.y2), o.fold_w ? y : nullptr,
                                  r.B, r.T(o), r.guard()),
                       o.Cin, o.sdil, r.s);
}

// fused ResBlock pairs: the members [n, m) of a group (the three ResBlocks of an MRF stage) in one launch, or an
// OP_MRFSUM, which holds its three members itself
static int run_pair_group(const Run& r, size_t n, size_t m) {
    const Op& o = r.op(n);
    const bool sum = o.type == OP_MRFSUM;
    PairParams pp = pair_params(o, sum ? 3 : (int)(m - n), r.B, r.T(o), r.guard());
    float* mids[3] = {nullptr, nullptr, nullptr};
    if (sum) {
        const int xs3[3] = {o.x, o.xb, o.xc};
        pp.sum = 1;
        for (int j = 0; j < 3; ++j) pp.m[j] = op_member(o, j, r.base[xs3[j]], r.base[o.y], r.at(o.y2));
    } else {
        for (size_t q = n; q < m; ++q) {
            const Op& qo = r.op(q);
            pp.m[q - n] = op_member(qo, 0, r.base[qo.x], qo.fold_w ? nullptr : r.base[qo.y], r.at(qo.y2), nullptr, r.at(qo.acc),
                                    r.at(qo.acc2));
            mids[q - n] = r.at(qo.tmpb);
            if (qo.fold_w) {            // (never grouped: one member)
                pp.fold_w = qo.fold_w;
                pp.fold_b = qo.fold_b;
                pp.fold_y = r.base[qo.y];
            }
        }
    }
    return launch_pair_family(pp, mids, o.Cin, o.dil, o.prec, r.s);
}

// a group of mutually independent fp32 convs: one launch when possible
static int run_conv_group(const Run& r, size_t n, size_t m) {
    ConvParams gp[3];
    for (size_t q = n; q < m; ++q) {
        const Op& qo = r.op(q);
        gp[q - n] = make_params(qo, r.base[qo.x], r.base[qo.y], r.at(qo.y2), r.at(qo.res), r.at(qo.acc), r.at(qo.acc2), r.B,
                                r.T(qo), r.at(qo.x2));
    }
    return launch_conv_group(gp, (int)(m - n), r.s);
}

// the last convs of the three ResBlocks of an fp32 MRF stage, summed (fv_plan_add_conv1d_sum3)
static int run_sum3(const Run& r, const Op& o) {
    float* const* base = r.base;
    Op mb = o, mc = o;           // members 1, 2: same layer geometry, their own taps / weights
    mb.k = o.kb; mb.pad = (o.kb - 1) / 2; mb.wp = o.wpb; mb.bias = nullptr;
    mc.k = o.kc; mc.pad = (o.kc - 1) / 2; mc.wp = o.wpc; mc.bias = nullptr;
    float* y2s = r.at(o.y2);
    // One launch pays when the three K loops in a row still leave enough blocks to fill the
    // GPU (tiles of 32 x 128, or 16 x 128); otherwise the two-launch form: members 1, 2 as a
    // grouped launch into scratch, then member 0 with both as running-sum inputs.
    const int64_t T3 = r.T(o);
    const int Mp = pad_rows(o.Cout);
    const int64_t blocks = (int64_t)(Mp == 16 ? 1 : Mp / 32) * ((T3 + 127) / 128);
    const int min_blocks = tuning().sum3_min;   // 800 -- measured: HiFi-GAN light, B = 1
    if (blocks >= min_blocks && Mp == o.Cout) {   // (whole row tiles only: the kernel's epilogue is the affine one)
        ConvParams ps[3] = {
            make_params(o, base[o.x], base[o.y], y2s, base[o.res], nullptr, nullptr, r.B, T3),
            make_params(mb, base[o.xb], base[o.y], y2s, base[o.resb], nullptr, nullptr, r.B, T3),
            make_params(mc, base[o.xc], base[o.y], y2s, base[o.resc], nullptr, nullptr, r.B, T3)};
        return launch_conv_sum3(ps, r.s);
    }
    Op duo_b = mb, duo_c = mc;                 // r_b, r_c: conv + residual, raw, no mean / activation
    duo_b.out_div = duo_c.out_div = 1.f;
    duo_b.act_slope = duo_c.act_slope = 1.f;
    duo_b.post = duo_c.post = FV_POST_NONE;
    ConvParams duo[2] = {
        make_params(duo_b, base[o.xb], base[o.tmpb], nullptr, base[o.resb], nullptr, nullptr, r.B, T3),
        make_params(duo_c, base[o.xc], base[o.tmpc], nullptr, base[o.resc], nullptr, nullptr, r.B, T3)};
    if (int rc = launch_conv_group(duo, 2, r.s)) return rc;
    Op car = o;                                // ((own + r_b) + r_c) / out_div, summed bias on this one
    car.own_first = 1;
    return launch_conv(make_params(car, base[o.x], base[o.y], y2s, base[o.res], base[o.tmpb], base[o.tmpc], r.B, T3), r.s);
}

// A residual stack that carries its two-launch form (256 channels): one launch up to Tuning::stack_items tiles per CU (in
// tenths), else two launches on 128-row x 128-column tiles.  [measured, Basis-MelGAN light, 1000 frames, batch 1 / 4 / 16 /
// 64, tools/bench_configs.py --only 3 --batch B --tuning stack_items=0 against the default] 0.385 -> 0.304, 1.03 -> 0.94,
// 3.55 -> 3.35, 13.0 -> 12.45 ms: the one-launch kernel wins at every size, so the default limit is "none"; the switch
// stays for A/B runs and the bit-identity tests
static bool stack_two_launch(int C, int B, int64_t T) {
    const int nm = convk_tile_columns(C);
    const int64_t items = (int64_t)B * ((T + nm - 1) / nm);
    return items * 10 > (int64_t)tuning().stack_items * device_cu_count();
}

// ... its two launches: the dilated conv into the scratch slot, raw (convs_kernel), then the K-concatenated 1x1 pair over
// the hidden tensor and x (convr_kernel), which carries the op's activation, post op and output offset
static int run_stack_two_launch(const Run& r, const Op& o) {
    PairParams pp = pair_params(o, 1, r.B, r.T(o), r.guard());
    pp.act_slope = 1.f;
    pp.post = FV_POST_NONE;
    pp.m[0] = pair_member(r.base[o.x], o.alt_w1, nullptr, o.bias, nullptr, o.k, r.base[o.alt_mid], nullptr);
    if (int rc = launch_convh(pp, o.Cin, o.dil, r.s)) return rc;
    PairParams pg = pair_params(o, 1, r.B, r.T(o), r.guard(), r.sub(o), r.sub_batched(o));
    pg.m[0] = pair_member(r.base[o.alt_mid], o.alt_w2, nullptr, o.bias2, nullptr, 1, r.base[o.y], r.at(o.y2), nullptr, nullptr,
                          nullptr, r.base[o.x]);
    return launch_convg(pg, o.Cout, r.s);
}

// every other op: one launch of its own
static int run_single(const Run& r, const Op& o) {
    const bool merge = o.type == OP_CONVT && o.in_merge;   // merged INPUT (fv_plan_set_input_merge): xb, xc travel as acc, acc2
    return run_op(o, r.base[o.x], r.base[o.y], r.at(o.y2), r.at(o.res), r.at(merge ? o.xb : o.acc), r.at(merge ? o.xc : o.acc2),
                  r.B, r.T(o), r.s, r.at(o.x2), r.sub(o), r.sub_batched(o), r.guard());
}

}  // namespace fv

extern "C" {

int fv_plan_run(fv_plan_t* plan, int B, int T, const float* in, float* out, void* workspace,
                int64_t workspace_bytes, void* stream) {
    return fv_plan_run_aux(plan, B, T, in, out, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream);
}

int fv_plan_run_aux(fv_plan_t* plan, int B, int T, const float* in, float* out, float* out2,
                    const float* const* aux_in, const int* aux_batched, void* workspace,
                    int64_t workspace_bytes, void* stream) {
    if (!plan || !in || !out) return fail(FV_ERR_INVALID_ARG, "plan_run: null argument");
    if (B <= 0 || T <= 0) return fail(FV_ERR_INVALID_ARG, "plan_run: B=%d T=%d", B, T);
    Shape sh[FV_MAX_SLOTS];
    int64_t elems[FV_MAX_SLOTS];
    if (int rc = infer(plan, B, T, sh, elems)) return rc;
    float* base[FV_MAX_SLOTS] = {};
    const int64_t need = arena(elems, workspace, base);
    base[FV_SLOT_AUX_IN0] = aux_in ? const_cast<float*>(aux_in[0]) : nullptr;
    base[FV_SLOT_AUX_IN1] = aux_in ? const_cast<float*>(aux_in[1]) : nullptr;
    base[FV_SLOT_OUT2] = out2;
    const int aux_b[2] = {aux_batched ? aux_batched[0] : 0, aux_batched ? aux_batched[1] : 0};
    for (const Op& o : plan->ops) {
        if (o.sub != FV_SLOT_NONE && !base[o.sub]) return fail(FV_ERR_INVALID_ARG, "plan_run: the plan subtracts auxiliary input %d, which was not given", o.sub - FV_SLOT_AUX_IN0);
        if ((o.y == FV_SLOT_OUT2 || o.y2 == FV_SLOT_OUT2) && !out2) return fail(FV_ERR_INVALID_ARG, "plan_run: the plan writes a second output, which was not given");
    }
    if (need > workspace_bytes || (need > 0 && !workspace))
        return fail(FV_ERR_WORKSPACE, "plan needs %lld workspace bytes, got %lld", (long long)need,
                    (long long)workspace_bytes);
    base[FV_SLOT_IN] = const_cast<float*>(in);
    base[FV_SLOT_OUT] = out;
    const Run r = {plan, B, base, sh, aux_b, (hipStream_t)stream};
    reset_shapes(plan, T, sh);      // shapes again, launch by launch (a slot may change shape when it is reused)
    for (size_t n = 0; n < plan->ops.size();) {
        const Op& o = plan->ops[n];
        size_t m = n + 1;           // the launch runs the ops [n, m)
        int rc;
        if (o.type == OP_CONVH) {
            m = group_end(plan, n, same_convh);
            rc = run_convh_group(r, n, m);
        } else if (o.type == OP_STAGE) {
            rc = run_stage(r, o);
        } else if (o.type == OP_PAIR || o.type == OP_MRFSUM) {
            m = group_end(plan, n, same_pair);
            rc = run_pair_group(r, n, m);
        } else if (o.type == OP_CONV && o.group != 0) {
            m = group_end(plan, n, same_conv);
            rc = run_conv_group(r, n, m);
        } else if (o.sum3) {
            rc = run_sum3(r, o);
        } else if (o.type == OP_STACK && o.alt_w1 && stack_two_launch(o.Cout, B, r.T(o))) {
            rc = run_stack_two_launch(r, o);
        } else {
            rc = run_single(r, o);
        }
        if (rc) return rc;
        for (; n < m; ++n) set_shapes(plan->ops[n], sh);
    }
    return 0;
}

int fv_plan_num_ops(fv_plan_t* plan) { return plan ? (int)plan->ops.size() : 0; }

int fv_plan_set_guard(fv_plan_t* plan, int* word) {
    if (!plan) return fail(FV_ERR_INVALID_ARG, "plan_set_guard: null plan");
    plan->guard_host = plan->guard_dev = nullptr;
    if (!word) return 0;
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, word, 0) != hipSuccess || !dev) {
        (void)hipGetLastError();
        return fail(FV_ERR_INVALID_ARG, "plan_set_guard: the guard word must live in pinned, device-mapped host memory "
                                        "(hipHostMalloc / torch pin_memory)");
    }
    plan->guard_host = word;
    plan->guard_dev = static_cast<int*>(dev);
    return 0;
}

int fv_plan_check_range(fv_plan_t* plan, void* stream) {
    if (!plan) return fail(FV_ERR_INVALID_ARG, "plan_check_range: null plan");
    if (!plan->guard_host) return 0;
    FV_HIP(hipStreamSynchronize((hipStream_t)stream));
    volatile int* w = plan->guard_host;
    const int seen = *w;
    if (seen == 0) return 0;
    *w = 0;
    if ((seen & ~FV_GUARD_LOW) == 0)   // only the low side's byte: whatever order the blocks stored in (the sides are separate bytes)
        return fail(FV_ERR_RANGE_LOW, "a split-f16 kernel met operands that were smaller than 2^-10 throughout a block's share of a "
                                      "tensor (not all zero): the last run may carry fewer than 22 bits; repeat it on an fp32-precision plan");
    return fail(FV_ERR_RANGE, "a split-f16 kernel met an operand outside its domain (|v| >= 65520 or a non-finite value; "
                              "or operands that were smaller than 2^-10 throughout a block's share of a tensor): the "
                              "results of the last run are not valid; repeat it on an fp32-precision plan");
}

}  // extern "C"
