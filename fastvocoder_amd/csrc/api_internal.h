// What api.hip (operators, measurement hook, tuning) and plan.hip (the plan executor) share: the op record, the plan, the
// op builders (argument checks + the record, one per family), and what both the direct entry points and their plan ops launch
// through: run_op, the builders of the launch records (PairParams / PairMember / MrfParams from an Op and resolved pointers)
// and the pair dispatch.
#pragma once
#include <stdint.h>

#include <vector>

#include "fv_internal.h"

namespace fv {

// ---------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------
enum OpType { OP_CONV = 0, OP_CONVT = 1, OP_PQMF = 2, OP_UPCONV = 3, OP_PAIR = 4, OP_MRFSUM = 5, OP_CONVH = 6, OP_CONVG = 7, OP_STACK = 8, OP_STAGE = 9 };

struct Op {
    int type;
    int x = FV_SLOT_NONE, y = FV_SLOT_NONE, res = FV_SLOT_NONE, acc = FV_SLOT_NONE, y2 = FV_SLOT_NONE, acc2 = FV_SLOT_NONE;
    int group;     // ops with the same non-zero id are mutually independent: one grouped launch
    const float* wp;
    const float* bias;
    const float* bias2 = nullptr;   // OP_STACK: bias of the 1x1 pair (stack[4] + skip_layer); `bias` is the dilated conv's
    // OP_STACK at 256 channels (fv_plan_set_stack_two_launch): the two-launch form for runs with many tiles -- the dilated
    // conv's fv_pack_pair_weight_ex image, the 1x1 pair's fv_pack_conv1x1_2src_split_f16 image, the hidden tensor's slot
    const float* alt_w1 = nullptr;
    const float* alt_w2 = nullptr;
    int alt_mid = FV_SLOT_NONE;
    int Cin, Cout, k, dil, pad, pad_mode, stride, out_pad;
    float pre_slope, out_div, act_slope;
    int post;
    // two-source conv (1 tap): GEMM rows ci >= Cin1 are read from slot x2 (Cin - Cin1 channels)
    int x2 = FV_SLOT_NONE;
    int Cin1 = 0;
    int own_first = 0;   // association of the MRF sum in the epilogue (ConvParams::own_first)
    // sum3 (fv_plan_add_conv1d_sum3): two more (input, residual, weight, taps) members; this op's own
    // x / res / wp / k / bias (summed) / y are member 0
    bool sum3 = false;
    int xb = FV_SLOT_NONE, xc = FV_SLOT_NONE, resb = FV_SLOT_NONE, resc = FV_SLOT_NONE;
    int tmpb = FV_SLOT_NONE, tmpc = FV_SLOT_NONE;   // [B,C,T] scratch for the two-launch form (few tiles)
    const float* wpb = nullptr;
    const float* wpc = nullptr;
    int kb = 0, kc = 0;
    // fused ResBlock pairs (OP_PAIR: member 0 only; OP_MRFSUM: the three members, inputs x / xb / xc)
    const float* pw1[3] = {nullptr, nullptr, nullptr};
    const float* pw2[3] = {nullptr, nullptr, nullptr};
    const float* pb1[3] = {nullptr, nullptr, nullptr};
    const float* pb2[3] = {nullptr, nullptr, nullptr};
    int pk[3] = {0, 0, 0};
    int sdil[3] = {0, 0, 0};  // OP_STAGE: dilations of the three pair positions (pk: taps of the three ResBlocks; wp: the packed stage)
    void* work = nullptr;     // OP_STAGE, 32 channels: the launch's history slots (caller-owned)
    bool classes = false;     // OP_STAGE: fv_plan_add_mrf_stage_classes_f16 (y: r_0 + r_1, y2: r_2)
    int64_t work_bytes = 0;
    int prec = 0;             // FV_PAIR_F32 / FV_PAIR_SPLIT_F16
    bool in_merge = false;    // fv_plan_set_input_merge (split-f16 transposed conv): the input is ((x + xb) + xc) / out_div
    // fv_plan_set_pair_output_conv: a 16 -> 1 channel, 7-tap conv folded into the pair; y is ITS output [B, 1, T]
    const float* fold_w = nullptr;
    const float* fold_b = nullptr;
    int sub = FV_SLOT_NONE;   // fv_plan_set_output_offset: auxiliary input subtracted in this op's epilogue
    // fv_plan_add_conv_post_pqmf: an OP_CONV (Cout = S sub-bands) whose launch also runs the PQMF synthesis: y is the
    // FULL-BAND output [B, 1, S * T']
    const float* pq_h = nullptr;
    int pq_taps = 0;
};

struct Shape {
    int C;
    int64_t T;
    bool set;
};

}  // namespace fv

struct fv_plan {
    int in_channels;
    std::vector<fv::Op> ops;
    int cur_group = 0;
    int cur_own_first = 0;
    // range guard of the split-f16 launches (fv_plan_set_guard): a caller-owned word in pinned, device-mapped host
    // memory -- the host's and the device's view of it
    int* guard_host = nullptr;
    int* guard_dev = nullptr;
};

namespace fv {

int64_t conv_out_len(const Op& o, int64_t Tin);
ConvParams make_params(const Op& o, const float* x, float* y, float* y2, const float* res,
                              const float* acc, const float* acc2, int B, int64_t Tin,
                              const float* x2 = nullptr, const float* sub = nullptr, int sub_batched = 0);
int run_op(const Op& o, const float* x, float* y, float* y2, const float* res, const float* acc,
                  const float* acc2, int B, int64_t Tin, hipStream_t s, const float* x2 = nullptr,
                  const float* sub = nullptr, int sub_batched = 0, int* guard = nullptr);

// ---------------------------------------------------------------------------
// op builders: one per operator family, called by the family's direct entry (api.hip) and by its plan entry (plan.hip).
// Each checks every argument that is neither a tensor nor a slot and fills every field of `o` (an `Op o = {}`) that is no
// slot; 0, or fail()'s code.  What one of the two entries checks and its twin does not stands in that entry.
// ---------------------------------------------------------------------------
int build_conv(Op& o, const float* packed, const float* bias, int Cin, int Cout, int k, int dil, int pad, int pad_mode,
               float pre_slope, float out_div, int post, float act_slope);
int build_conv_2src(Op& o, const float* packed, const float* bias, int Cin1, int Cin2, int Cout, int post, float act_slope);
int build_convt(Op& o, const float* packed, const float* bias, int Cin, int Cout, int k, int stride, int pad, int out_pad,
                float pre_slope, int post, float act_slope);
int build_convt_split(Op& o, const float* packed, const float* bias, int Cin, int Cout, int k, int stride, int pad, int out_pad,
                      float pre_slope, float act_slope);
int build_convg(Op& o, const float* packed, const float* bias, int C, float pre_slope, int post, float act_slope);
int build_stack(Op& o, const float* packed, const float* bias_dilated, const float* bias_out, int C, int k, int dil, float slope,
                int pad_mode, int post, float act_slope);
int build_conv_post_pqmf(Op& o, const float* packed, const float* bias, const float* h, int Cin, int S, int k, int pad,
                         float pre_slope, int post, int ntaps);
int build_pqmf(Op& o, const float* h, int S, int ntaps);
// (the grouped families: one member per op, its weights, biases and taps in pw1[0] and its siblings; member j of the arrays)
int build_pair(Op& o, int j, const float* const* w1, const float* const* w2, const float* const* b1, const float* const* b2,
               const int* k, int C, int dil, float slope, float out_div, int post, float act_slope, int prec);
int build_convh(Op& o, int j, const float* const* packed, const float* const* bias, const int* k, int C, int dil, int pad_mode,
                float pre_slope, float out_div, int post, float act_slope);
int build_mrfsum(Op& o, const float* const* w1, const float* const* w2, const float* const* b1, const float* const* b2,
                 const int* k, int C, int dil, float slope, float out_div, int post, float act_slope);
int build_stage(Op& o, const float* packed, int C, const int* k, const int* dil, float slope, float out_div, int post,
                float act_slope, void* workspace, int64_t workspace_bytes);

// ---------------------------------------------------------------------------
// launch records: every PairParams / PairMember / MrfParams of the direct entries and of the plan is built here
// ---------------------------------------------------------------------------
// a plan's slot as a pointer
inline float* ptr(float* const* base, int slot) { return slot == FV_SLOT_NONE ? nullptr : base[slot]; }
// What a launch takes from its op: B, T, the slopes, out_div, post, the arithmetic, reflection padding; the range guard and the
// output offset as resolved by the caller.  The members, `sum` and `fold_*` are the caller's.
PairParams pair_params(const Op& o, int n_members, int B, int64_t T, int* guard, const float* sub = nullptr, int sub_batched = 0);
PairMember pair_member(const float* x, const float* w1, const float* w2, const float* b1, const float* b2, int k, float* y,
                       float* y_act, const float* res = nullptr, const float* add1 = nullptr, const float* add2 = nullptr,
                       const float* x2 = nullptr);
// member j of a grouped family's op (OP_PAIR, OP_CONVH: j = 0; OP_MRFSUM: 0..2) on resolved pointers
inline PairMember op_member(const Op& o, int j, const float* x, float* y, float* y_act, const float* res = nullptr,
                            const float* add1 = nullptr, const float* add2 = nullptr) {
    return pair_member(x, o.pw1[j], o.pw2[j], o.pb1[j], o.pb2[j], o.pk[j], y, y_act, res, add1, add2);
}
// an OP_STAGE's launch: blob, taps, slopes, out_div, post, fold_w / fold_b and the history slots from the op
MrfParams mrf_params(const Op& o, const float* x, float* y, float* y_act, float* fold_y, int B, int64_t T, int* guard);
// ... in two block classes (Op::classes): y_s = r_0 + r_1, y_r2 = r_2
MrfSplitParams mrf_split_params(const Op& o, const float* x, float* y_s, float* y_r2, int B, int64_t T, int* guard);
// a launch of fused ResBlock pairs, by the kernel family of its channel count (mid: the members' scratch tensors, C >= 64)
int launch_pair_family(const PairParams& pp, float* const* mid, int C, int dil, int prec, hipStream_t s);

}  // namespace fv
