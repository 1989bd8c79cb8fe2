// C-ABI entry points of libfastvocoder_hip.so (include/fastvocoder_hip.h): the fused operators as direct calls, the op core they
// share with the plan executor (plan.hip) -- the op builders (build_*: the one description of each family), run_op, the builders
// of every launch record (pair_params, pair_member, mrf_params) and the one pair dispatch (launch_pair_family) --, error text,
// tuning switches and the measurement hook.  (Weight preparation: pack.hip.)
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <mutex>
#include <utility>
#include <vector>

#include <ctype.h>
#include <string.h>
#include <unistd.h>

#include <cxxabi.h>
#include <dlfcn.h>

#include "api_internal.h"
#include "launch_host.hpp"

namespace fv {

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code ? code : FV_ERR_INVALID_ARG;
}


// ---------------------------------------------------------------------------
// launch log (fv_debug_launch_log; FV_KERNEL_LAUNCH of fv_internal.h): which kernels ran, host side only
// ---------------------------------------------------------------------------
std::atomic<int> g_launch_log_on{0};
static std::mutex g_launch_log_mutex;
static std::vector<std::pair<const void*, long long>> g_launch_log;   // (kernel handle, launches) in first-seen order
static std::vector<std::pair<hipStream_t, long long>> g_launch_log_streams;   // (stream handle, launches + async copies)
static long long g_launch_log_copies = 0;                              // async memsets / copies (memset_async, memcpy_async)

template <class K>
static void launch_log_count(std::vector<std::pair<K, long long>>& table, K key) {
    for (auto& e : table)
        if (e.first == key) {
            ++e.second;
            return;
        }
    table.emplace_back(key, 1);
}

// handle: the kernel's, or null for an asynchronous memset / copy
void launch_log_note(const void* handle, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g_launch_log_mutex);
    if (handle) launch_log_count(g_launch_log, handle);
    else ++g_launch_log_copies;
    launch_log_count(g_launch_log_streams, stream);
}

// "void fv::convh_kernel<2, 2, 1>(fv::PairParams)" -> "convh_kernel<2, 2, 1>": the return type, every "fv::", the host
// stub's "__device_stub__" and the argument list go.  Parentheses inside template arguments (enumerators print as casts)
// are not the argument list: that one opens outside every <>.
// Limit: where __cxa_demangle gives up (a parameter type it does not know), only a NON-TEMPLATE kernel "_ZN2fv<length><name>E..."
// is named right; a templated kernel with such a parameter would lose its template arguments, and two of them would share a
// name -- tools/kernel_census.py built_kernels() refuses a library in which two stubs get one name.
static std::string kernel_display_name(const char* mangled) {
    int status = 0;
    char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
    std::string s = (status == 0 && dem) ? dem : mangled;
    free(dem);
    if (!(status == 0) && s.compare(0, 3, "_ZN") == 0) {
        // a demangler that does not know a parameter type (_Float16 pointers: "PDF16_") gives up on the whole symbol.  Those
        // kernels are plain functions "_ZN2fv<length><name>E<parameters>": the last <length><name> of the nested name is theirs
        size_t at = 3, name_at = 0, name_len = 0;
        while (at < s.size() && isdigit((unsigned char)s[at])) {
            size_t len = 0;
            while (at < s.size() && isdigit((unsigned char)s[at])) len = len * 10 + (size_t)(s[at++] - '0');
            if (at + len > s.size()) break;
            name_at = at;
            name_len = len;
            at += len;
        }
        if (name_len) s = s.substr(name_at, name_len);
    }
    for (const char* drop : {"__device_stub__", "fv::"})
        for (size_t at; (at = s.find(drop)) != std::string::npos;) s.erase(at, strlen(drop));
    size_t begin = 0, end = s.size();
    int depth = 0;
    for (size_t i = 0; i < s.size(); ++i) {
        const char c = s[i];
        if (c == '<') ++depth;
        else if (c == '>') --depth;
        else if (depth == 0 && c == ' ') begin = i + 1;
        else if (depth == 0 && c == '(') { end = i; break; }
    }
    return s.substr(begin, end - begin);
}

// ---------------------------------------------------------------------------
// measurement hook
// ---------------------------------------------------------------------------
// A launch's duration is completion-to-completion on its stream: from the end of the launch before it (or, for the
// first one, from an event recorded in front of it) to its own end -- its dispatch latency is part of it, as it is in
// rocprofv3's dispatch durations, and the durations of a run add up to the run.  One event per launch.
struct ProfRec {
    hipEvent_t a, b;        // a: only where there is no previous launch to measure from
    hipStream_t s;
    double ms;              // < 0: not read back yet
    double flops, bytes;
    int kind;
};
static bool g_prof_on = false;
static bool g_prof_need_start = true;
static std::vector<ProfRec> g_prof;
static hipEvent_t g_prof_start;

void profile_begin(hipStream_t s) {
    if (!g_prof_on) return;
    g_prof_start = nullptr;
    if (g_prof_need_start || g_prof.empty() || g_prof.back().s != s || !g_prof.back().b) {
        (void)hipEventCreate(&g_prof_start);
        (void)hipEventRecord(g_prof_start, s);
        g_prof_need_start = false;
    }
}

void profile_end(hipStream_t s, int kind, double flops, double bytes) {
    if (!g_prof_on) return;
    ProfRec r;
    r.a = g_prof_start;
    g_prof_start = nullptr;
    (void)hipEventCreate(&r.b);
    (void)hipEventRecord(r.b, s);
    r.s = s;
    r.ms = -1.0;
    r.flops = flops;
    r.bytes = bytes;
    r.kind = kind;
    g_prof.push_back(r);
}

// read every pending record back (in order: a record without its own start event is measured from its predecessor's
// end), then drop the events
static int profile_resolve() {
    for (size_t i = 0; i < g_prof.size(); ++i) {
        ProfRec& r = g_prof[i];
        if (r.ms >= 0) continue;
        FV_HIP(hipEventSynchronize(r.b));
        float e = 0.f;
        FV_HIP(hipEventElapsedTime(&e, r.a ? r.a : g_prof[i - 1].b, r.b));
        r.ms = e;
    }
    for (ProfRec& r : g_prof) {
        if (r.a) (void)hipEventDestroy(r.a);
        if (r.b) (void)hipEventDestroy(r.b);
        r.a = r.b = nullptr;
    }
    g_prof_need_start = true;
    return 0;
}

// the events of one measurement call: destroyed on every way out of it
struct ScopedEvents {
    std::vector<hipEvent_t> ev;
    explicit ScopedEvents(size_t n) : ev(n, nullptr) {}
    ScopedEvents(const ScopedEvents&) = delete;
    ScopedEvents& operator=(const ScopedEvents&) = delete;
    ~ScopedEvents() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int create() {
        for (hipEvent_t& e : ev) FV_HIP(hipEventCreate(&e));
        return 0;
    }
};

}  // namespace fv

namespace fv {

int64_t conv_out_len(const Op& o, int64_t Tin) {
    if (o.type == OP_PAIR || o.type == OP_MRFSUM || o.type == OP_CONVH || o.type == OP_CONVG || o.type == OP_STACK ||
        o.type == OP_STAGE)
        return Tin;
    if (o.type == OP_CONV) {
        const int64_t t = (o.pad_mode & FV_PAD_CAUSAL) ? Tin : Tin + 2LL * o.pad - (int64_t)o.dil * (o.k - 1);
        return o.pq_h ? t * o.Cout : t;      // (conv_post + pqmf: the S sub-bands interleave into S * T' samples)
    }
    if (o.type == OP_CONVT) return (Tin - 1) * o.stride - 2LL * o.pad + o.k + o.out_pad;
    if (o.type == OP_UPCONV) return Tin * o.stride + 2LL * o.pad - (o.k - 1);
    return Tin * o.Cin;  // PQMF: S sub-bands interleave into S*Tsub samples
}


ConvParams make_params(const Op& o, const float* x, float* y, float* y2, const float* res,
                              const float* acc, const float* acc2, int B, int64_t Tin,
                              const float* x2, const float* sub, int sub_batched) {
    ConvParams p = {};
    p.sub = sub;
    p.sub_batched = sub_batched;
    p.x = x;
    p.x2 = x2;
    p.Cin1 = x2 ? o.Cin1 : o.Cin;
    p.wp = o.wp;
    p.bias = o.bias;
    p.res = res;
    p.acc_in = acc;
    p.acc_in2 = acc2;
    p.y = y;
    p.y_act = y2;
    p.act_slope = o.act_slope;
    p.B = B;
    p.Cin = o.Cin;
    p.Cout = o.Cout;
    p.Tin = (int)Tin;
    p.pad_mode = o.pad_mode & ~FV_PAD_CAUSAL;
    p.pre_slope = o.pre_slope;
    p.out_div = o.out_div;
    p.post = o.post;
    p.own_first = o.own_first;
    p.Tout = (int)conv_out_len(o, Tin);
    if (o.type == OP_CONV) {
        p.M = o.Cout;
        p.k = o.k;
        p.dil = o.dil;
        p.pad = o.pad;
        p.ups = 1;
        p.Tq = p.Tout;
    } else {
        const Polyphase ph = o.type == OP_UPCONV ? upsample_phases(o.k, o.stride, o.pad)
                                                 : polyphase(o.k, o.stride, o.pad);
        p.M = o.Cout * o.stride;
        p.k = ph.taps;
        p.dil = 1;
        p.pad = -ph.dmin;
        if (o.type == OP_CONVT && convt_phase_major(o.Cout, o.k, o.stride, o.pad)) {
            p.phase_major = 1;
            p.pad_orig = o.pad;
            p.k = o.k / o.stride;          // taps of every phase
            p.pad = p.k - 1;               // the widest window shift (phases with (r+p)/s == 0)
        }
        p.pad_mode = FV_PAD_ZERO;
        p.ups = o.stride;
        p.Tq = (p.Tout + o.stride - 1) / o.stride;
        // MACs of a ConvTranspose1d = Tin * Cin * Cout * k, whatever the polyphase image pads
        if (o.type == OP_CONVT) p.alg_flops = 2.0 * B * (double)Tin * o.Cin * o.Cout * o.k;
    }
    p.Mpad = pad_rows(p.M);
    return p;
}

int run_op(const Op& o, const float* x, float* y, float* y2, const float* res, const float* acc,
                  const float* acc2, int B, int64_t Tin, hipStream_t s, const float* x2,
                  const float* sub, int sub_batched, int* guard) {
    if (o.type == OP_PQMF) return launch_pqmf(x, o.wp, y, y2, sub, sub_batched, B, o.Cin, o.k, (int)Tin, s);
    if (o.pq_h) {
        Op c = o;                              // the conv in front: [B, S, T'] sub-bands that never leave the CU
        c.pq_h = nullptr;
        return launch_conv_post_pqmf(make_params(c, x, y, nullptr, nullptr, nullptr, nullptr, B, Tin), o.pq_h, o.pq_taps, y, y2,
                                     sub, sub_batched, s);
    }
    if (o.type == OP_CONVG) {
        PairParams pp = pair_params(o, 1, B, Tin, guard, sub, sub_batched);
        pp.m[0] = pair_member(x, o.wp, nullptr, o.bias, nullptr, o.k, y, y2, res, nullptr, nullptr, x2);
        return launch_convg(pp, o.Cout, s);
    }
    if (o.type == OP_STACK) {
        PairParams pp = pair_params(o, 1, B, Tin, guard, sub, sub_batched);
        pp.m[0] = pair_member(x, o.wp, nullptr, o.bias, o.bias2, o.k, y, y2);
        return launch_convk(pp, o.Cout, o.dil, s);
    }
    if (o.type == OP_CONVT && o.prec == FV_PAIR_SPLIT_F16) {
        // fv_plan_set_input_merge: the input is ((x + acc) + acc2) / out_div, formed in the kernel's window loader (the
        // launchers take out_div as 1 without acc)
        PairParams pp = pair_params(o, 1, B, Tin, guard);
        pp.m[0] = pair_member(x, o.wp, nullptr, o.bias, nullptr, o.k, y, y2, nullptr, acc, acc2);
        if (convtn_shape(o.Cin, o.Cout, o.k, o.stride)) return launch_convtn(pp, (int)conv_out_len(o, Tin), s);
        return launch_convt(pp, o.Cin, o.Cout, o.stride, o.pad, (int)conv_out_len(o, Tin), s);
    }
    return launch_conv(make_params(o, x, y, y2, res, acc, acc2, B, Tin, x2, sub, sub_batched), s);
}

PairParams pair_params(const Op& o, int n_members, int B, int64_t T, int* guard, const float* sub, int sub_batched) {
    PairParams pp = {};
    pp.n_members = n_members;
    pp.B = B;
    pp.T = (int)T;
    pp.slope = o.pre_slope;
    pp.act_slope = o.act_slope;
    pp.out_div = o.out_div;
    pp.post = o.post;
    pp.prec = o.prec;
    pp.guard = guard;
    pp.reflect = (o.pad_mode & FV_PAD_REFLECT) ? 1 : 0;
    pp.sub = sub;
    pp.sub_batched = sub_batched;
    return pp;
}

PairMember pair_member(const float* x, const float* w1, const float* w2, const float* b1, const float* b2, int k, float* y,
                       float* y_act, const float* res, const float* add1, const float* add2, const float* x2) {
    PairMember mb = {};
    mb.x = x;
    mb.x2 = x2;
    mb.w1 = w1;
    mb.w2 = w2;
    mb.b1 = b1;
    mb.b2 = b2;
    mb.k = k;
    mb.y = y;
    mb.y_act = y_act;
    mb.res = res;
    mb.add1 = add1;
    mb.add2 = add2;
    return mb;
}

MrfParams mrf_params(const Op& o, const float* x, float* y, float* y_act, float* fold_y, int B, int64_t T, int* guard) {
    MrfParams mp = {};
    mp.x = x;
    mp.y = y;
    mp.y_act = y_act;
    mp.blob = o.wp;
    for (int j = 0; j < 3; ++j) mp.k[j] = o.pk[j];
    mp.B = B;
    mp.T = (int)T;
    mp.slope = o.pre_slope;
    mp.out_div = o.out_div;
    mp.act_slope = o.act_slope;
    mp.post = o.post;
    mp.fold_w = o.fold_w;
    mp.fold_b = o.fold_b;
    mp.fold_y = fold_y;
    mp.guard = guard;
    mp.hist = static_cast<float*>(o.work);
    mp.hist_bytes = o.work_bytes;
    return mp;
}

MrfSplitParams mrf_split_params(const Op& o, const float* x, float* y_s, float* y_r2, int B, int64_t T, int* guard) {
    MrfSplitParams sp = {};
    static_cast<MrfParams&>(sp) = mrf_params(o, x, y_s, nullptr, nullptr, B, T, guard);
    sp.y2 = y_r2;
    return sp;
}

// CausalConv1d keeps the first Tin outputs of a conv padded on both sides: only a pad of
// at least (k-1)*dil - which makes that many outputs exist - is meaningful.
int check_pad_mode(int pad_mode, int pad, int k, int dil) {
    if (pad_mode < 0 || pad_mode > (FV_PAD_REFLECT | FV_PAD_CAUSAL))
        return fail(FV_ERR_INVALID_ARG, "unknown pad_mode %d", pad_mode);
    if ((pad_mode & FV_PAD_CAUSAL) && 2LL * pad < (int64_t)dil * (k - 1))
        return fail(FV_ERR_INVALID_ARG, "causal conv: pad=%d leaves fewer than Tin outputs (k=%d dil=%d)",
                    pad, k, dil);
    return 0;
}

int check_conv_args(int Cin, int Cout, int k, int dil) {
    if (Cin <= 0 || Cout <= 0 || k <= 0 || dil <= 0)
        return fail(FV_ERR_INVALID_ARG, "bad conv shape Cin=%d Cout=%d k=%d dil=%d", Cin, Cout, k, dil);
    return 0;
}

// ---- ConvTranspose1d with split-f16 operands (convt_kernel) ----
int check_convt_split_args(int Cin, int Cout, int k, int stride, int pad, int out_pad) {
    if (Cin != 32 && Cin != 64 && Cin != 128 && Cin != 256 && Cin != 512)
        return fail(FV_ERR_UNSUPPORTED, "conv_transpose1d_split_f16: Cin = %d (32, 64, 128, 256 or 512)", Cin);
    if (stride < 2 || stride > 16 || k != 2 * stride)
        return fail(FV_ERR_UNSUPPORTED, "conv_transpose1d_split_f16: kernel %d, stride %d (kernel = 2 x stride, stride 2..16)", k, stride);
    if (Cout <= 0 || Cout * stride < 32)
        return fail(FV_ERR_UNSUPPORTED, "conv_transpose1d_split_f16: Cout * stride = %d (32 or more)", Cout * stride);
    if (pad < 0 || pad > stride || out_pad < -stride || out_pad >= stride)
        return fail(FV_ERR_INVALID_ARG, "conv_transpose1d_split_f16: pad=%d (0..stride) out_pad=%d", pad, out_pad);
    if (convtn_shape(Cin, Cout, k, stride) && (pad != 1 || out_pad != 0))
        return fail(FV_ERR_UNSUPPORTED, "conv_transpose1d_split_f16: 32 -> 16 channels, kernel 4, stride 2 exists with pad=1, "
                    "out_pad=0 only (got %d, %d)", pad, out_pad);
    return 0;
}

// ---------------------------------------------------------------------------
// op builders (api_internal.h): the one description of each operator family, for its direct entry and its plan entry
// ---------------------------------------------------------------------------
// the fields that every family but the PQMF has
static void fill(Op& o, int prec, const float* wp, const float* bias, int Cin, int Cout, int k, int dil, float pre_slope,
                 float out_div, int post, float act_slope) {
    o.prec = prec;
    o.wp = wp;
    o.bias = bias;
    o.Cin = Cin;
    o.Cout = Cout;
    o.k = k;
    o.dil = dil;
    o.pre_slope = pre_slope;
    o.out_div = out_div;
    o.post = post;
    o.act_slope = act_slope;
}

int build_conv(Op& o, const float* packed, const float* bias, int Cin, int Cout, int k, int dil, int pad, int pad_mode,
               float pre_slope, float out_div, int post, float act_slope) {
    if (int rc = check_conv_args(Cin, Cout, k, dil)) return rc;
    if (int rc = check_pad_mode(pad_mode, pad, k, dil)) return rc;
    o.type = OP_CONV;
    fill(o, FV_PAIR_F32, packed, bias, Cin, Cout, k, dil, pre_slope, out_div, post, act_slope);
    o.pad = pad;
    o.pad_mode = pad_mode;
    return 0;
}

int build_conv_2src(Op& o, const float* packed, const float* bias, int Cin1, int Cin2, int Cout, int post, float act_slope) {
    if (Cin1 <= 0 || Cin2 <= 0) return fail(FV_ERR_INVALID_ARG, "conv1d_2src: Cin1=%d Cin2=%d", Cin1, Cin2);
    o.Cin1 = Cin1;
    return build_conv(o, packed, bias, Cin1 + Cin2, Cout, 1, 1, 0, FV_PAD_ZERO, 1.f, 1.f, post, act_slope);
}

// (the conv taps are not dilated: Op::dil stays 0, as OP_CONVT and OP_UPCONV never read it)
int build_convt(Op& o, const float* packed, const float* bias, int Cin, int Cout, int k, int stride, int pad, int out_pad,
                float pre_slope, int post, float act_slope) {
    if (int rc = check_conv_args(Cin, Cout, k, 1)) return rc;
    // negative out_pad trims the tail (CausalConvTranspose1d, modules.py:297-317: -stride)
    if (stride <= 0 || pad < 0 || out_pad < -stride)
        return fail(FV_ERR_INVALID_ARG, "conv_transpose1d: stride=%d pad=%d out_pad=%d", stride, pad, out_pad);
    o.type = OP_CONVT;
    fill(o, FV_PAIR_F32, packed, bias, Cin, Cout, k, 0, pre_slope, 1.f, post, act_slope);
    o.stride = stride;
    o.pad = pad;
    o.out_pad = out_pad;
    return 0;
}

int build_convt_split(Op& o, const float* packed, const float* bias, int Cin, int Cout, int k, int stride, int pad, int out_pad,
                      float pre_slope, float act_slope) {
    if (int rc = check_convt_split_args(Cin, Cout, k, stride, pad, out_pad)) return rc;
    if (int rc = build_convt(o, packed, bias, Cin, Cout, k, stride, pad, out_pad, pre_slope, FV_POST_NONE, act_slope)) return rc;
    o.prec = FV_PAIR_SPLIT_F16;
    return 0;
}

// (no check of C: the plan entry makes one, the direct entry leaves it to launch_convg)
int build_convg(Op& o, const float* packed, const float* bias, int C, float pre_slope, int post, float act_slope) {
    o.type = OP_CONVG;
    fill(o, FV_PAIR_SPLIT_F16, packed, bias, 2 * C, C, 1, 1, pre_slope, 1.f, post, act_slope);
    o.Cin1 = C;
    return 0;
}

int build_stack(Op& o, const float* packed, const float* bias_dilated, const float* bias_out, int C, int k, int dil, float slope,
                int pad_mode, int post, float act_slope) {
    if (post != FV_POST_NONE && post != FV_POST_TANH && post != FV_POST_RELU)
        return fail(FV_ERR_INVALID_ARG, "residual_stack_split_f16: post op %d", post);
    if (!convk_shape(C, k, dil))
        return fail(FV_ERR_UNSUPPORTED, "residual_stack_split_f16: C = %d, k = %d, dilation %d (32 / 64 / 128 / 256 channels, 3 taps, "
                    "dilation 1, 3 or 9)", C, k, dil);
    if (pad_mode != FV_PAD_ZERO && pad_mode != FV_PAD_REFLECT)
        return fail(FV_ERR_UNSUPPORTED, "residual_stack_split_f16: pad_mode %d (zero or reflection padding of the 'same' conv)", pad_mode);
    if (int rc = check_slopes("residual_stack_split_f16", slope, act_slope)) return rc;
    o.type = OP_STACK;
    fill(o, FV_PAIR_SPLIT_F16, packed, bias_dilated, C, C, k, dil, slope, 1.f, post, act_slope);
    o.bias2 = bias_out;
    o.pad = dil * (k - 1) / 2;
    o.pad_mode = pad_mode;
    o.stride = 1;
    return 0;
}

int build_conv_post_pqmf(Op& o, const float* packed, const float* bias, const float* h, int Cin, int S, int k, int pad,
                         float pre_slope, int post, int ntaps) {
    if (S != 4 || ntaps != 63) return fail(FV_ERR_UNSUPPORTED, "conv_post_pqmf: S=%d ntaps=%d (4 sub-bands, 63 taps)", S, ntaps);
    // a 'same' conv: y holds S * T samples per utterance (a larger pad would make the kernel store past it)
    if (k % 2 != 1 || pad != (k - 1) / 2)
        return fail(FV_ERR_INVALID_ARG, "conv_post_pqmf: k=%d pad=%d (odd kernel, pad = (k - 1) / 2)", k, pad);
    o.pq_h = h;
    o.pq_taps = ntaps;
    return build_conv(o, packed, bias, Cin, S, k, 1, pad, FV_PAD_ZERO, pre_slope, 1.f, post, 1.f);
}

int build_pqmf(Op& o, const float* h, int S, int ntaps) {
    if (S <= 0 || ntaps <= 0 || ntaps % 2 == 0) return fail(FV_ERR_INVALID_ARG, "pqmf: S=%d ntaps=%d", S, ntaps);
    o.type = OP_PQMF;
    o.wp = h;
    o.Cin = S;
    o.Cout = 1;
    o.k = ntaps;
    return 0;
}

static int check_pair_args(int n, int C, const int* k, int dil, int prec) {
    if (n < 1 || n > 3) return fail(FV_ERR_INVALID_ARG, "resblock pair: %d members (1..3)", n);
    if (C != 16 && C != 32 && !(prec == FV_PAIR_SPLIT_F16 && (C == 64 || C == 128 || C == 256 || C == 512)))
        return fail(FV_ERR_UNSUPPORTED, "resblock pair: C = %d (16 or 32; 64 ... 512 with split-f16 operands); use the conv1d ops", C);
    if (dil != 1 && dil != 3 && dil != 5) return fail(FV_ERR_UNSUPPORTED, "resblock pair: dilation %d (1, 3 or 5)", dil);
    for (int j = 0; j < n; ++j)
        if (int rc = check_taps("resblock pair", k[j])) return rc;
    return 0;
}

template <class P>
static P at(P const* a, int j) { return a ? a[j] : nullptr; }      // member j of an optional array argument

// member j of the arrays as member `slot` of the op
static void fill_member(Op& o, int slot, int j, const float* const* w1, const float* const* w2, const float* const* b1,
                        const float* const* b2, const int* k) {
    o.pw1[slot] = w1[j];
    o.pw2[slot] = at(w2, j);
    o.pb1[slot] = at(b1, j);
    o.pb2[slot] = at(b2, j);
    o.pk[slot] = k[j];
}

int build_pair(Op& o, int j, const float* const* w1, const float* const* w2, const float* const* b1, const float* const* b2,
               const int* k, int C, int dil, float slope, float out_div, int post, float act_slope, int prec) {
    if (int rc = check_pair_args(1, C, k + j, dil, prec)) return rc;
    o.type = OP_PAIR;
    fill(o, prec, nullptr, nullptr, C, C, k[j], dil, slope, out_div, post, act_slope);
    fill_member(o, 0, j, w1, w2, b1, b2, k);
    return 0;
}

int build_mrfsum(Op& o, const float* const* w1, const float* const* w2, const float* const* b1, const float* const* b2,
                 const int* k, int C, int dil, float slope, float out_div, int post, float act_slope) {
    if (int rc = check_pair_args(3, C, k, dil, FV_PAIR_F32)) return rc;
    o.type = OP_MRFSUM;
    fill(o, FV_PAIR_F32, nullptr, nullptr, C, C, k[0], dil, slope, out_div, post, act_slope);
    for (int j = 0; j < 3; ++j) fill_member(o, j, j, w1, w2, b1, b2, k);
    return 0;
}

int build_convh(Op& o, int j, const float* const* packed, const float* const* bias, const int* k, int C, int dil, int pad_mode,
                float pre_slope, float out_div, int post, float act_slope) {
    if (pad_mode != FV_PAD_ZERO && pad_mode != FV_PAD_REFLECT)
        return fail(FV_ERR_UNSUPPORTED, "conv1d_split_f16: pad_mode %d (FV_PAD_ZERO or FV_PAD_REFLECT)", pad_mode);
    if (C != 64 && C != 128 && C != 256 && C != 512)
        return fail(FV_ERR_UNSUPPORTED, "conv1d_split_f16: C = %d (64, 128, 256 or 512)", C);
    if (dil != 1 && dil != 3 && dil != 5 && dil != 9)
        return fail(FV_ERR_UNSUPPORTED, "conv1d_split_f16: dilation %d (1, 3, 5; 9 with 3 taps)", dil);
    if ((k[j] != 3 && k[j] != 7 && k[j] != 11) || (dil == 9 && k[j] != 3))
        return fail(FV_ERR_UNSUPPORTED, "conv1d_split_f16: %d taps at dilation %d (3, 7 or 11; 3 at dilation 9)", k[j], dil);
    o.type = OP_CONVH;
    fill(o, FV_PAIR_SPLIT_F16, nullptr, nullptr, C, C, k[j], dil, pre_slope, out_div, post, act_slope);
    o.pad_mode = pad_mode;
    fill_member(o, 0, j, packed, nullptr, bias, nullptr, k);
    return 0;
}

// (the workspace is the entries' to check: the plan entry does when the op is added, the direct entries leave it to the launchers)
int build_stage(Op& o, const float* packed, int C, const int* k, const int* dil, float slope, float out_div, int post,
                float act_slope, void* workspace, int64_t workspace_bytes) {
    if (!k || !dil) return fail(FV_ERR_INVALID_ARG, "mrf stage: null taps / dilations");
    if (!mrf_stage_shape(C, k, dil))
        return fail(FV_ERR_UNSUPPORTED, "mrf stage: C = %d, taps (%d, %d, %d), dilations (%d, %d, %d): built for 16 / 32 channels, "
                    "taps 3 / 7 / 11, dilations (1, 3, 5)", C, k[0], k[1], k[2], dil[0], dil[1], dil[2]);
    if (int rc = check_slopes("mrf stage", slope, act_slope)) return rc;
    if (post != FV_POST_NONE && post != FV_POST_TANH && post != FV_POST_RELU) return fail(FV_ERR_INVALID_ARG, "mrf stage: post %d", post);
    o.type = OP_STAGE;
    fill(o, FV_PAIR_SPLIT_F16, packed, nullptr, C, C, k[0], dil[0], slope, out_div, post, act_slope);
    for (int j = 0; j < 3; ++j) {
        o.pk[j] = k[j];
        o.sdil[j] = dil[j];
    }
    o.work = workspace;
    o.work_bytes = workspace_bytes;
    return 0;
}

}  // namespace fv

using namespace fv;

namespace fv {
int allow_dynamic_lds(const void* kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return 0;
    struct Grant { const void* kernel; int device; size_t bytes; };
    static std::mutex mu;
    static std::vector<Grant> granted;                               // a few dozen kernels per device at most
    int dev = 0;
    FV_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    for (Grant& g : granted)
        if (g.kernel == kernel && g.device == dev) {
            if (g.bytes >= bytes) return 0;
            FV_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
            g.bytes = bytes;
            return 0;
        }
    FV_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    granted.push_back({kernel, dev, bytes});
    return 0;
}

// Tuning switches (fv_internal.h struct Tuning).  Defaults unless the process was started with FV_TUNING=1, in which
// case the FV_* variables of the table below are read ONCE, here; after that the launch path never touches the
// environment.  fv_tuning_set changes an entry at run time (tests: different block counts / schedules must give the
// same bits).
static Tuning g_tuning;
static std::once_flag g_tuning_once;
struct TuningEntry {
    const char* key;      // fv_tuning_set key; the environment variable is "FV_" + upper case
    int Tuning::*field;
};
static const TuningEntry kTuningTable[] = {
    {"pair_dbg", &Tuning::pair_dbg},       {"dbg", &Tuning::conv_dbg},           {"sched", &Tuning::sched},
    {"sched_switch", &Tuning::sched_switch}, {"convh_skel", &Tuning::convh_skel}, {"convp_skel", &Tuning::convp_skel},
    {"convq_skel", &Tuning::convq_skel},   {"pair128_unfused", &Tuning::pair128_unfused},
    {"convg_rows64", &Tuning::convg_rows64}, {"stack_items", &Tuning::stack_items}, {"stack_wide", &Tuning::stack_wide},
    {"convp_wide", &Tuning::convp_wide},   {"convq_wide", &Tuning::convq_wide},
    {"convq_nm11", &Tuning::convq_nm11},   {"convq_cost80", &Tuning::convq_cost80},
    {"convh_rows64", &Tuning::convh_rows64},  {"convt_rows64", &Tuning::convt_rows64},
    {"pairh_skel", &Tuning::pairh_skel},   {"pair_skel", &Tuning::pair_skel},    {"convh_blocks", &Tuning::convh_blocks},
    {"pair_blocks", &Tuning::pair_blocks}, {"sum3_min", &Tuning::sum3_min},      {"lds_budget", &Tuning::lds_budget},
    {"units", &Tuning::units},             {"shape16", &Tuning::shape16},        {"shape32", &Tuning::shape32},
    {"shape64", &Tuning::shape64},         {"krows", &Tuning::krows},            {"grid_cap", &Tuning::grid_cap},
    {"no_group", &Tuning::no_group},       {"mrf_blocks", &Tuning::mrf_blocks},  {"mrf_shape", &Tuning::mrf_shape},
    {"mrf_prio", &Tuning::mrf_prio},       {"convt_lean", &Tuning::convt_lean},
    {"mrf_cost_a", &Tuning::mrf_cost_a},   {"mrf_cost_b", &Tuning::mrf_cost_b},  {"mrf_cost_one", &Tuning::mrf_cost_one},
    {"convs_ringfree", &Tuning::convs_ringfree}, {"convu_resident", &Tuning::convu_resident},
};
static void tuning_from_env() {
    const char* on = getenv("FV_TUNING");
    if (!on || atoi(on) != 1) return;
    for (const TuningEntry& e : kTuningTable) {
        char name[64] = "FV_";
        size_t n = 3;
        for (const char* c = e.key; *c && n + 1 < sizeof(name); ++c) name[n++] = (char)toupper((unsigned char)*c);
        name[n] = 0;
        const char* v = getenv(name);
        if (v && *v) g_tuning.*(e.field) = atoi(v);
    }
    const char* tp = getenv("FV_PAIR_TRACE_PTR");
    if (tp && *tp) g_tuning.trace_ptr = strtoull(tp, nullptr, 0);
}
const Tuning& tuning() {
    std::call_once(g_tuning_once, tuning_from_env);
    return g_tuning;
}

int device_cu_count() {
    // one device model per process (the boxes hold eight identical GPUs).  Threads that come first together each ask the
    // runtime and store the same number: an atomic, so that the first uses of two threads are no data race.
    static std::atomic<int> cus{0};
    int v = cus.load(std::memory_order_relaxed);
    if (!v) {
        int dev = 0;
        v = hipGetDevice(&dev) == hipSuccess &&
                    hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0
                ? v : 256;
        cus.store(v, std::memory_order_relaxed);
    }
    return v;
}
}  // namespace fv

extern "C" {

int fv_version(void) { return FV_ABI_VERSION; }


#ifndef FV_BUILD_ID
#define FV_BUILD_ID "unknown"
#endif
// (the "fv-build-id:" tag lets the id be read from the file without loading it: _native.built_id)
const char* fv_build_id(void) { return "fv-build-id:" FV_BUILD_ID + 12; }

const char* fv_last_error(void) { return g_err.c_str(); }

int fv_upsample_conv1d_fused(const float* x, const float* packed, const float* bias, float* y,
                             float* y_act, int B, int Cin, int Cout, int Tin, int k, int rate, int pad,
                             float pre_slope, int post, float act_slope, void* stream) {
    if (!x || !packed || !y) return fail(FV_ERR_INVALID_ARG, "upsample_conv1d: null tensor");
    if (x == y || x == y_act || (y_act && y_act == y))
        return fail(FV_ERR_INVALID_ARG, "upsample_conv1d: y / y_act must not alias x or each other");
    Op o = {};
    if (int rc = build_convt(o, packed, bias, Cin, Cout, k, rate, pad, 0, pre_slope, post, act_slope)) return rc;
    o.type = OP_UPCONV;          // the transposed conv's record, as fv_plan_add_upsample_conv1d retypes it
    if (conv_out_len(o, Tin) <= 0) return fail(FV_ERR_INVALID_ARG, "upsample_conv1d: empty output");
    return run_op(o, x, y, y_act, nullptr, nullptr, nullptr, B, Tin, (hipStream_t)stream);
}

int fv_conv1d_fused(const float* x, const float* packed, const float* bias, const float* res,
                    const float* acc_in, const float* acc_in2, float* y, float* y_act, int B, int Cin,
                    int Cout, int Tin, int k, int dil, int pad, int pad_mode, float pre_slope,
                    float out_div, int post, float act_slope, void* stream) {
    if (!x || !packed || !y) return fail(FV_ERR_INVALID_ARG, "conv1d: null tensor");
    if (x == y || x == y_act || (y_act && y_act == y))
        return fail(FV_ERR_INVALID_ARG, "conv1d: y / y_act must not alias x or each other");
    Op o = {};
    if (int rc = build_conv(o, packed, bias, Cin, Cout, k, dil, pad, pad_mode, pre_slope, out_div, post, act_slope)) return rc;
    if (conv_out_len(o, Tin) <= 0) return fail(FV_ERR_INVALID_ARG, "conv1d: empty output");
    return run_op(o, x, y, y_act, res, acc_in, acc_in2, B, Tin, (hipStream_t)stream);
}

int fv_conv_transpose1d_fused(const float* x, const float* packed, const float* bias, float* y,
                              float* y_act, int B, int Cin, int Cout, int Tin, int k, int stride,
                              int pad, int out_pad, float pre_slope, int post, float act_slope,
                              void* stream) {
    if (!x || !packed || !y) return fail(FV_ERR_INVALID_ARG, "conv_transpose1d: null tensor");
    if (x == y || x == y_act || (y_act && y_act == y))
        return fail(FV_ERR_INVALID_ARG, "conv_transpose1d: y / y_act must not alias x or each other");
    Op o = {};
    if (int rc = build_convt(o, packed, bias, Cin, Cout, k, stride, pad, out_pad, pre_slope, post, act_slope)) return rc;
    if (out_pad >= stride + (stride == 1))      // this entry alone: fv_plan_add_conv_transpose1d takes any out_pad >= -stride
        return fail(FV_ERR_INVALID_ARG, "conv_transpose1d: out_pad=%d at stride=%d (below the stride)", out_pad, stride);
    if (conv_out_len(o, Tin) <= 0) return fail(FV_ERR_INVALID_ARG, "conv_transpose1d: empty output");
    return run_op(o, x, y, y_act, nullptr, nullptr, nullptr, B, Tin, (hipStream_t)stream);
}

int fv_basis_ola(const float* weight, const float* packed_basis, float* out, int B, int C, int F, int L, void* stream) {
    if (L < 2 || L % 2 != 0) return fail(FV_ERR_INVALID_ARG, "basis_ola: L=%d (even, >= 2)", L);
    return fv_conv_transpose1d_fused(weight, packed_basis, nullptr, out, nullptr, B, C, 1, F, L, L / 2, 0, 0, 1.f, FV_POST_NONE,
                                     1.f, stream);
}

int fv_generator_run(fv_plan_t* plan, int B, int T, const float* mel, float* out, void* workspace, int64_t workspace_bytes,
                     void* stream) {
    return fv_plan_run(plan, B, T, mel, out, workspace, workspace_bytes, stream);
}

int fv_conv_transpose1d_split_f16(const float* x, const float* packed, const float* bias, float* y, float* y_act, int B,
                                  int Cin, int Cout, int Tin, int k, int stride, int pad, int out_pad, float pre_slope,
                                  float act_slope, int* guard, void* stream) {
    if (!x || !packed || !y) return fail(FV_ERR_INVALID_ARG, "conv_transpose1d_split_f16: null tensor");
    if (x == y || x == y_act || (y_act && y_act == y))
        return fail(FV_ERR_INVALID_ARG, "conv_transpose1d_split_f16: y / y_act must not alias x or each other");
    Op o = {};
    if (int rc = build_convt_split(o, packed, bias, Cin, Cout, k, stride, pad, out_pad, pre_slope, act_slope)) return rc;
    if (B < 0 || Tin < 0) return fail(FV_ERR_INVALID_ARG, "conv_transpose1d_split_f16: B=%d Tin=%d", B, Tin);
    if (B == 0 || Tin == 0) return 0;
    if (conv_out_len(o, Tin) <= 0) return fail(FV_ERR_INVALID_ARG, "conv_transpose1d_split_f16: empty output");
    return run_op(o, x, y, y_act, nullptr, nullptr, nullptr, B, Tin, (hipStream_t)stream, nullptr, nullptr, 0, guard);
}

int fv_pqmf_synthesis(const float* x, const float* h, float* y, int B, int S, int ntaps, int Tsub,
                      void* stream) {
    if (!x || !h || !y || B < 0 || Tsub < 0) return fail(FV_ERR_INVALID_ARG, "pqmf: null tensor or B=%d Tsub=%d", B, Tsub);
    Op o = {};
    if (int rc = build_pqmf(o, h, S, ntaps)) return rc;
    return run_op(o, x, y, nullptr, nullptr, nullptr, nullptr, B, Tsub, (hipStream_t)stream);
}

int fv_pqmf_analysis(const float* x, const float* h, float* y, int B, int S, int ntaps, int64_t T,
                     void* stream) {
    if (!x || !h || !y || B < 0 || S <= 0 || ntaps <= 0 || ntaps % 2 == 0 || T < S)
        return fail(FV_ERR_INVALID_ARG, "pqmf analysis: B=%d S=%d ntaps=%d T=%lld", B, S, ntaps, (long long)T);
    return launch_pqmf_analysis(x, h, y, B, S, ntaps, T, (hipStream_t)stream);
}

int fv_encode_16bits(float* x, int16_t* out, float* peak, int B, int64_t n, float rescale_out,
                     int scale_in_place, void* stream) {
    if (!x || !out || !peak || B < 0 || n < 0)
        return fail(FV_ERR_INVALID_ARG, "encode_16bits: null tensor or B=%d n=%lld", B, (long long)n);
    return launch_encode16(x, B, n, rescale_out, reinterpret_cast<short*>(out),
                           reinterpret_cast<unsigned*>(peak), scale_in_place, (hipStream_t)stream);
}

int fv_mel_table_floats(void) { return FV_MEL_TABLE_FLOATS; }

int fv_melspectrogram(const float* x, float* mel, const float* tables, int B, int64_t n, int sample_rate, int n_fft,
                      int hop, int win_length, int n_mels, float fmin, void* stream) {
    if (sample_rate != 24000 || n_fft != 2048 || hop != 240 || win_length != 1200 || n_mels != 80 || fmin != 40.f)
        return fail(FV_ERR_UNSUPPORTED,
                    "melspectrogram: only sr=24000 n_fft=2048 hop=240 win_length=1200 n_mels=80 fmin=40 "
                    "(got sr=%d n_fft=%d hop=%d win_length=%d n_mels=%d fmin=%g)",
                    sample_rate, n_fft, hop, win_length, n_mels, (double)fmin);
    if (!x || !mel || !tables || B <= 0 || B > 65535)
        return fail(FV_ERR_INVALID_ARG, "melspectrogram: null tensor or B=%d", B);
    if (n < n_fft / 2 + 1 || n / hop >= (int64_t)1 << 32)
        return fail(FV_ERR_INVALID_ARG, "melspectrogram: n=%lld samples (reflect padding by %d needs n >= %d)",
                    (long long)n, n_fft / 2, n_fft / 2 + 1);
    return launch_melspectrogram(x, mel, tables, B, n, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// resampling (resample.hip)
// ---------------------------------------------------------------------------
int64_t fv_resample_out_len(int64_t n_in, int L, int M) {
    if (n_in < 0 || n_in > FV_RESAMPLE_MAX_SAMPLES || L < 1 || L > FV_RESAMPLE_MAX_FACTOR || M < 1 ||
        M > FV_RESAMPLE_MAX_FACTOR)
        return fail(FV_ERR_INVALID_ARG, "resample: n_in=%lld L=%d M=%d", (long long)n_in, L, M);
    return (n_in * L + M - 1) / M;
}

int fv_resample(const void* x, int x_format, float* y, const float* table, int B, int64_t n_in, int64_t n_out, int L,
                int M, int half, void* stream) {
    if (x_format != FV_PCM_F32 && x_format != FV_PCM_S16)
        return fail(FV_ERR_INVALID_ARG, "resample: x_format=%d (FV_PCM_F32 or FV_PCM_S16)", x_format);
    if (!x || !y || !table || B <= 0 || B > 65535) return fail(FV_ERR_INVALID_ARG, "resample: null tensor or B=%d", B);
    if (n_in < 1) return fail(FV_ERR_INVALID_ARG, "resample: n_in=%lld", (long long)n_in);
    const int64_t want = fv_resample_out_len(n_in, L, M);
    if (want < 0) return (int)want;
    if (n_out != want)
        return fail(FV_ERR_INVALID_ARG, "resample: n_out=%lld, %lld samples at L/M = %d/%d give %lld", (long long)n_out,
                    (long long)n_in, L, M, (long long)want);
    if (half < 1 || half > FV_RESAMPLE_MAX_WINDOW || (2 * (int64_t)half + 2) * L > FV_RESAMPLE_MAX_TABLE_FLOATS ||
        resample_window(L, M, half) > FV_RESAMPLE_MAX_WINDOW)
        return fail(FV_ERR_UNSUPPORTED,
                    "resample: L/M = %d/%d with half=%d needs a table of %lld floats (at most %d) and a window of %lld "
                    "(at most %d)", L, M, half, (long long)((2 * (int64_t)half + 2) * L), FV_RESAMPLE_MAX_TABLE_FLOATS,
                    (long long)resample_window(L, M, half), FV_RESAMPLE_MAX_WINDOW);
    if ((n_out + 255) / 256 > 0x7fffffffLL) return fail(FV_ERR_INVALID_ARG, "resample: n_out=%lld", (long long)n_out);
    return launch_resample(x, x_format, y, table, B, n_in, n_out, L, M, half, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// Griffin-Lim (griffin_lim.hip)
// ---------------------------------------------------------------------------
static int gl_check_geometry(const char* who, int n_fft, int hop, int win_length) {
    if (n_fft != 2048 || hop != 240 || win_length != 1200)
        return fail(FV_ERR_UNSUPPORTED, "%s: only n_fft=2048 hop=240 win_length=1200 (got n_fft=%d hop=%d win_length=%d)",
                    who, n_fft, hop, win_length);
    return 0;
}

static int gl_check_frames(const char* who, int B, int T, int min_T) {
    if (B <= 0 || B > 65535) return fail(FV_ERR_INVALID_ARG, "%s: B=%d (1..65535)", who, B);
    if (T < min_T || T > FV_GL_MAX_FRAMES)
        return fail(FV_ERR_INVALID_ARG, "%s: T=%d frames (%d..%d)", who, T, min_T, FV_GL_MAX_FRAMES);
    return 0;
}

static int gl_check_workspace(const char* who, int B, int T, const void* workspace, size_t workspace_bytes) {
    const int64_t need = fv_istft_workspace_bytes(B, T);
    if (!workspace || (uint64_t)workspace_bytes < (uint64_t)need || ((uintptr_t)workspace & 15))
        return fail(FV_ERR_WORKSPACE, "%s: workspace of %zu bytes, needs %lld (16-byte aligned)", who, workspace_bytes,
                    (long long)need);
    return 0;
}

int fv_gl_table_floats(void) { return FV_GL_TABLE_FLOATS; }

int64_t fv_istft_workspace_bytes(int B, int T) {
    if (B <= 0 || B > 65535 || T < 1 || T > FV_GL_MAX_FRAMES) return fail(FV_ERR_INVALID_ARG, "istft workspace: B=%d T=%d", B, T);
    return (int64_t)B * T * 1200 * (int64_t)sizeof(float);
}

int64_t fv_griffin_lim_workspace_bytes(int B, int T) { return fv_istft_workspace_bytes(B, T); }

int fv_stft(const float* y, float* spec, const float* tables, int B, int64_t n, int n_fft, int hop, int win_length,
            void* stream) {
    if (int rc = gl_check_geometry("stft", n_fft, hop, win_length)) return rc;
    if (!y || !spec || !tables || ((uintptr_t)spec & 7) || ((uintptr_t)tables & 15))
        return fail(FV_ERR_INVALID_ARG, "stft: null or misaligned pointer");
    if (n < n_fft / 2 + 1 || n / hop >= FV_GL_MAX_FRAMES)
        return fail(FV_ERR_INVALID_ARG, "stft: n=%lld samples (reflect padding by %d needs n >= %d)", (long long)n,
                    n_fft / 2, n_fft / 2 + 1);
    if (int rc = gl_check_frames("stft", B, (int)(1 + n / hop), 1)) return rc;
    return launch_stft_complex(y, spec, tables, B, n, (hipStream_t)stream);
}

int fv_istft(const float* spec, float* y, const float* tables, int B, int T, int n_fft, int hop, int win_length,
             void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = gl_check_geometry("istft", n_fft, hop, win_length)) return rc;
    if (int rc = gl_check_frames("istft", B, T, 2)) return rc;
    if (!spec || !y || !tables || ((uintptr_t)spec & 7) || ((uintptr_t)y & 15) || ((uintptr_t)tables & 15))
        return fail(FV_ERR_INVALID_ARG, "istft: null or misaligned pointer");
    if (int rc = gl_check_workspace("istft", B, T, workspace, workspace_bytes)) return rc;
    return launch_istft(spec, y, tables, B, T, static_cast<float*>(workspace), (hipStream_t)stream);
}

int fv_griffin_lim(const float* S, const float* phase0, float* y, const float* tables, int B, int T, int iters,
                   int n_fft, int hop, int win_length, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = gl_check_geometry("griffin_lim", n_fft, hop, win_length)) return rc;
    // the iterate of 240 (T - 1) samples is reflect-padded by 1024: T >= 6
    if (int rc = gl_check_frames("griffin_lim", B, T, 6)) return rc;
    if (iters < 0) return fail(FV_ERR_INVALID_ARG, "griffin_lim: iters=%d", iters);
    if (!S || !y || !tables || ((uintptr_t)phase0 & 7) || ((uintptr_t)y & 15) || ((uintptr_t)tables & 15))
        return fail(FV_ERR_INVALID_ARG, "griffin_lim: null or misaligned pointer");
    if (int rc = gl_check_workspace("griffin_lim", B, T, workspace, workspace_bytes)) return rc;
    return launch_griffin_lim(S, phase0, y, tables, B, T, iters, static_cast<float*>(workspace), (hipStream_t)stream);
}

int fv_mel_to_linear(const float* mel, const float* inv_basis, float* S, int B, int T, int n_mels, int n_freq,
                     float power, void* stream) {
    if (n_mels != 80 || n_freq != 1025)
        return fail(FV_ERR_UNSUPPORTED, "mel_to_linear: only n_mels=80 n_freq=1025 (got %d, %d)", n_mels, n_freq);
    if (int rc = gl_check_frames("mel_to_linear", B, T, 1)) return rc;
    if (!mel || !inv_basis || !S || !(power > 0.f))
        return fail(FV_ERR_INVALID_ARG, "mel_to_linear: null tensor or power=%g", (double)power);
    return launch_mel_to_linear(mel, inv_basis, S, B, T, power, (hipStream_t)stream);
}

int fv_inv_preemphasis(const float* y, float* out, int B, int64_t n, float coef, void* stream) {
    if (!y || !out || B <= 0 || B > 65535 || n < 1 || !(fabsf(coef) < 1.f))
        return fail(FV_ERR_INVALID_ARG, "inv_preemphasis: null tensor, B=%d, n=%lld or |coef|=%g >= 1", B, (long long)n,
                    (double)fabsf(coef));
    return launch_inv_preemphasis(y, out, B, n, coef, (hipStream_t)stream);
}

static int stft_check_res(const char* who, int64_t n, int n_fft, int hop, int win_length) {
    if ((n_fft != 512 && n_fft != 1024 && n_fft != 2048) || hop < 1 || win_length < 1 || win_length > n_fft)
        return fail(FV_ERR_UNSUPPORTED,
                    "%s: n_fft must be 512, 1024 or 2048, hop >= 1 and 1 <= win_length <= n_fft "
                    "(got n_fft=%d hop=%d win_length=%d)", who, n_fft, hop, win_length);
    if (n < n_fft / 2 + 1 || n / hop >= (int64_t)1 << 31)
        return fail(FV_ERR_INVALID_ARG, "%s: n=%lld samples (reflect padding by %d needs n >= %d)", who,
                    (long long)n, n_fft / 2, n_fft / 2 + 1);
    return 0;
}

int fv_stft_table_floats(int n_fft, int win_length) {
    if ((n_fft != 512 && n_fft != 1024 && n_fft != 2048) || win_length < 1 || win_length > n_fft)
        return fail(FV_ERR_UNSUPPORTED, "stft table: n_fft=%d win_length=%d", n_fft, win_length);
    return FV_STFT_TAB_WINDOW(n_fft) + win_length;
}

int fv_stft_magnitude(const float* x, float* mag, const float* table, int B, int64_t n, int n_fft, int hop,
                      int win_length, void* stream) {
    if (int rc = stft_check_res("stft_magnitude", n, n_fft, hop, win_length)) return rc;
    if (!x || !mag || !table || B <= 0 || B > 65535)
        return fail(FV_ERR_INVALID_ARG, "stft_magnitude: null tensor or B=%d", B);
    return launch_stft_magnitude(x, mag, table, B, n, n_fft, hop, win_length, (hipStream_t)stream);
}

static int64_t stft_distance_check(int B, int64_t n, int R, const int* n_fft, const int* hop, const int* win) {
    if (R < 1 || R > FV_STFT_MAX_RES || !n_fft || !hop)
        return fail(FV_ERR_INVALID_ARG, "stft_distance: R=%d resolutions (1..%d)", R, FV_STFT_MAX_RES);
    if (B <= 0 || B > 65535) return fail(FV_ERR_INVALID_ARG, "stft_distance: B=%d", B);
    int64_t chunks = 0;
    for (int r = 0; r < R; ++r) {
        if (int rc = stft_check_res("stft_distance", n, n_fft[r], hop[r], win ? win[r] : n_fft[r])) return rc;
        chunks += stft_chunks(n, hop[r]);
    }
    if (chunks >= (int64_t)1 << 31) return fail(FV_ERR_INVALID_ARG, "stft_distance: n=%lld too long", (long long)n);
    return (int64_t)B * chunks * 3 * (int64_t)sizeof(double);
}

int64_t fv_stft_distance_workspace_bytes(int B, int64_t n, int R, const int* n_fft, const int* hop) {
    return stft_distance_check(B, n, R, n_fft, hop, nullptr);
}

int fv_stft_distance(const float* x, const float* y, const float* const* tables, int B, int64_t n, int R,
                     const int* n_fft, const int* hop, const int* win_length, double* out, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (!win_length) return fail(FV_ERR_INVALID_ARG, "stft_distance: win_length is null");
    const int64_t need = stft_distance_check(B, n, R, n_fft, hop, win_length);
    if (need < 0) return (int)need;
    if (!x || !y || !tables || !out || !workspace)
        return fail(FV_ERR_INVALID_ARG, "stft_distance: null pointer");
    for (int r = 0; r < R; ++r)
        if (!tables[r]) return fail(FV_ERR_INVALID_ARG, "stft_distance: table %d is null", r);
    if ((uint64_t)workspace_bytes < (uint64_t)need || ((uintptr_t)workspace & 7))
        return fail(FV_ERR_INVALID_ARG, "stft_distance: workspace of %zu bytes, needs %lld (8-byte aligned)",
                    workspace_bytes, (long long)need);
    return launch_stft_distance(x, y, tables, B, n, R, n_fft, hop, win_length, out,
                                static_cast<double*>(workspace), (hipStream_t)stream);
}

static int64_t stft_grad_check(int B, int64_t n, int R, const int* n_fft, const int* hop, const int* win) {
    if (R < 1 || R > FV_STFT_MAX_RES || !n_fft || !hop || !win)
        return fail(FV_ERR_INVALID_ARG, "stft_distance_grad: R=%d resolutions (1..%d) or a null parameter array", R,
                    FV_STFT_MAX_RES);
    if (B <= 0 || B > 65535) return fail(FV_ERR_INVALID_ARG, "stft_distance_grad: B=%d", B);
    int64_t chunks = 0, floats = 0;
    for (int r = 0; r < R; ++r) {
        if (int rc = stft_check_res("stft_distance_grad", n, n_fft[r], hop[r], win[r])) return rc;
        chunks += stft_grad_chunks(n, hop[r]);
        floats += (int64_t)B * (1 + n / hop[r]) * win[r];
    }
    if (chunks >= (int64_t)1 << 31 || (n + 255) / 256 >= (int64_t)1 << 31 || floats >= (int64_t)1 << 40)
        return fail(FV_ERR_INVALID_ARG, "stft_distance_grad: n=%lld too long", (long long)n);
    return floats * (int64_t)sizeof(float);
}

int64_t fv_stft_distance_grad_workspace_bytes(int B, int64_t n, int R, const int* n_fft, const int* hop,
                                              const int* win_length) {
    return stft_grad_check(B, n, R, n_fft, hop, win_length);
}

int fv_stft_distance_grad(const float* x, const float* y, const float* const* tables, int B, int64_t n, int R,
                          const int* n_fft, const int* hop, const int* win_length, const float* coef, float* gx,
                          void* workspace, size_t workspace_bytes, void* stream) {
    const int64_t need = stft_grad_check(B, n, R, n_fft, hop, win_length);
    if (need < 0) return (int)need;
    if (!x || !y || !tables || !coef || !gx || !workspace)
        return fail(FV_ERR_INVALID_ARG, "stft_distance_grad: null pointer");
    for (int r = 0; r < R; ++r)
        if (!tables[r]) return fail(FV_ERR_INVALID_ARG, "stft_distance_grad: table %d is null", r);
    if ((uint64_t)workspace_bytes < (uint64_t)need || ((uintptr_t)workspace & 3))
        return fail(FV_ERR_INVALID_ARG, "stft_distance_grad: workspace of %zu bytes, needs %lld (4-byte aligned)",
                    workspace_bytes, (long long)need);
    return launch_stft_distance_grad(x, y, tables, B, n, R, n_fft, hop, win_length, coef, gx,
                                     static_cast<float*>(workspace), (hipStream_t)stream);
}

int fv_stft_magnitude_bins(const float* x, float* mag, const float* table, int B, int64_t n, int n_fft, int hop,
                           int win_length, void* stream) {
    if (int rc = stft_check_res("stft_magnitude_bins", n, n_fft, hop, win_length)) return rc;
    if (!x || !mag || !table || B <= 0 || B > 65535)
        return fail(FV_ERR_INVALID_ARG, "stft_magnitude_bins: null tensor or B=%d", B);
    return launch_stft_magnitude(x, mag, table, B, n, n_fft, hop, win_length, (hipStream_t)stream, true);
}

static int64_t stft_mag_grad_check(int B, int64_t n, int n_fft, int hop, int win) {
    if (int rc = stft_check_res("stft_magnitude_bins_grad", n, n_fft, hop, win)) return rc;
    if (B <= 0 || B > 65535) return fail(FV_ERR_INVALID_ARG, "stft_magnitude_bins_grad: B=%d", B);
    const int64_t floats = (int64_t)B * (1 + n / hop) * win;
    if (stft_mag_grad_chunks(n, hop) >= (int64_t)1 << 31 || (n + 255) / 256 >= (int64_t)1 << 31 ||
        floats >= (int64_t)1 << 40)
        return fail(FV_ERR_INVALID_ARG, "stft_magnitude_bins_grad: n=%lld too long", (long long)n);
    return floats * (int64_t)sizeof(float);
}

int64_t fv_stft_magnitude_bins_grad_workspace_bytes(int B, int64_t n, int n_fft, int hop, int win_length) {
    return stft_mag_grad_check(B, n, n_fft, hop, win_length);
}

int fv_stft_magnitude_bins_grad(const float* x, const float* gmag, const float* table, int B, int64_t n, int n_fft,
                                int hop, int win_length, float* gx, void* workspace, size_t workspace_bytes,
                                void* stream) {
    const int64_t need = stft_mag_grad_check(B, n, n_fft, hop, win_length);
    if (need < 0) return (int)need;
    if (!x || !gmag || !table || !gx || !workspace)
        return fail(FV_ERR_INVALID_ARG, "stft_magnitude_bins_grad: null pointer");
    if ((uint64_t)workspace_bytes < (uint64_t)need || ((uintptr_t)workspace & 3))
        return fail(FV_ERR_INVALID_ARG, "stft_magnitude_bins_grad: workspace of %zu bytes, needs %lld (4-byte "
                    "aligned)", workspace_bytes, (long long)need);
    const auto overlaps = [&](const void* p, int64_t bytes) {
        const uintptr_t a = (uintptr_t)gx, ae = a + (uintptr_t)B * n * sizeof(float), c = (uintptr_t)p;
        return a < c + (uintptr_t)bytes && c < ae;
    };
    const int64_t gbytes = (int64_t)B * (n_fft / 2 + 1) * (1 + n / hop) * (int64_t)sizeof(float);
    if (overlaps(x, (int64_t)B * n * (int64_t)sizeof(float)) || overlaps(gmag, gbytes) || overlaps(workspace, need))
        return fail(FV_ERR_INVALID_ARG, "stft_magnitude_bins_grad: gx aliases x, gmag or the workspace");
    return launch_stft_magnitude_bins_grad(x, gmag, table, B, n, n_fft, hop, win_length, gx,
                                           static_cast<float*>(workspace), (hipStream_t)stream);
}

int fv_grouped_conv1d(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int Tin,
                      int k, int stride, int pad, float slope, void* stream) {
    if (Cin < 4 || Cin % 4 || Cout < 1 || Cout % (Cin / 4) || k < 1 || stride < 1)
        return fail(FV_ERR_UNSUPPORTED, "grouped_conv1d: Cin=%d Cout=%d k=%d stride=%d (Cin %% 4 == 0, groups = Cin/4 "
                    "dividing Cout, k >= 1, stride >= 1)", Cin, Cout, k, stride);
    const int opg = Cout / (Cin / 4);
    if (grouped_conv_lds_bytes(k, stride, opg % 16 == 0 ? 16 : 4) > 65536)
        return fail(FV_ERR_UNSUPPORTED, "grouped_conv1d: k=%d stride=%d exceed a block's shared memory", k, stride);
    if (!x || !w || !y || B <= 0 || B > 65535 || Tin < 1 || pad < 0)
        return fail(FV_ERR_INVALID_ARG, "grouped_conv1d: null tensor, B=%d, Tin=%d or pad=%d", B, Tin, pad);
    if (y == x || y == w) return fail(FV_ERR_INVALID_ARG, "grouped_conv1d: y must not alias x or w");
    const int64_t span = (int64_t)Tin + 2 * (int64_t)pad - k;
    if (span < 0) return fail(FV_ERR_INVALID_ARG, "grouped_conv1d: empty output (Tin=%d pad=%d k=%d)", Tin, pad, k);
    return launch_grouped_conv1d(x, w, bias, y, B, Cin, Cout, Tin, (int)(span / stride + 1), k, stride, pad, slope,
                                 (hipStream_t)stream);
}

int fv_avg_pool1d(const float* x, float* y, int rows, int64_t Tin, int k, int stride, int pad, void* stream) {
    if (!x || !y || x == y || rows < 1 || rows > 65535 || k < 1 || stride < 1 || pad < 0 || 2 * pad > k)
        return fail(FV_ERR_INVALID_ARG, "avg_pool1d: rows=%d k=%d stride=%d pad=%d", rows, k, stride, pad);
    const int64_t span = Tin + 2 * (int64_t)pad - k;
    if (Tin < 1 || span < 0)
        return fail(FV_ERR_INVALID_ARG, "avg_pool1d: empty output (Tin=%lld k=%d pad=%d)", (long long)Tin, k, pad);
    return launch_avg_pool1d(x, y, rows, Tin, span / stride + 1, k, stride, pad, (hipStream_t)stream);
}

int64_t fv_disc_score_workspace_bytes(int B, int M, const int64_t* n) {
    if (M < 1 || M > FV_DISC_MAX_MAPS || !n)
        return fail(FV_ERR_INVALID_ARG, "disc_score_sums: M=%d maps (1..%d)", M, FV_DISC_MAX_MAPS);
    if (B <= 0 || B > 65535) return fail(FV_ERR_INVALID_ARG, "disc_score_sums: B=%d", B);
    for (int m = 0; m < M; ++m)
        if (n[m] < 1) return fail(FV_ERR_INVALID_ARG, "disc_score_sums: map %d has %lld elements", m, (long long)n[m]);
    const int64_t chunks = score_chunks(M, n);
    if (chunks >= (int64_t)1 << 31) return fail(FV_ERR_INVALID_ARG, "disc_score_sums: maps too large");
    return (int64_t)B * chunks * 4 * (int64_t)sizeof(double);
}

int fv_disc_score_sums(const float* const* e, const float* const* r, const int64_t* n, int M, int B, double* out,
                       void* workspace, size_t workspace_bytes, void* stream) {
    const int64_t need = fv_disc_score_workspace_bytes(B, M, n);
    if (need < 0) return (int)need;
    if (!e || !r || !out || !workspace) return fail(FV_ERR_INVALID_ARG, "disc_score_sums: null pointer");
    for (int m = 0; m < M; ++m)
        if (!e[m] || !r[m]) return fail(FV_ERR_INVALID_ARG, "disc_score_sums: map %d is null", m);
    if ((uint64_t)workspace_bytes < (uint64_t)need || ((uintptr_t)workspace & 7))
        return fail(FV_ERR_INVALID_ARG, "disc_score_sums: workspace of %zu bytes, needs %lld (8-byte aligned)",
                    workspace_bytes, (long long)need);
    return launch_disc_score_sums(e, r, n, M, B, out, static_cast<double*>(workspace), (hipStream_t)stream);
}

int fv_grouped_conv1d_input_grad(const float* g_up, const float* g_map, const float* y, const float* w, float* dx,
                                 int B, int Cin, int Cout, int Tin, int k, int stride, int pad, float slope,
                                 void* stream) {
    if (Cin < 4 || Cin % 4 || Cout < 1 || Cout % (Cin / 4) || k < 1 || stride < 1)
        return fail(FV_ERR_UNSUPPORTED, "grouped_conv1d_input_grad: Cin=%d Cout=%d k=%d stride=%d (Cin %% 4 == 0, "
                    "groups = Cin/4 dividing Cout, k >= 1, stride >= 1)", Cin, Cout, k, stride);
    const int opg = Cout / (Cin / 4);
    if (grouped_conv_lds_bytes(k, stride, opg % 16 == 0 ? 16 : 4) > 65536)     // the forward's own bound
        return fail(FV_ERR_UNSUPPORTED, "grouped_conv1d_input_grad: k=%d stride=%d exceed a block's shared memory", k,
                    stride);
    if ((!g_up && !g_map) || !w || !dx || B <= 0 || B > 65535 || Tin < 1 || pad < 0)
        return fail(FV_ERR_INVALID_ARG, "grouped_conv1d_input_grad: null tensor, B=%d, Tin=%d or pad=%d", B, Tin, pad);
    if (!y && slope != 1.f)
        return fail(FV_ERR_INVALID_ARG, "grouped_conv1d_input_grad: slope=%g needs the layer's output y", slope);
    if (dx == g_up || dx == g_map || dx == y || dx == w)
        return fail(FV_ERR_INVALID_ARG, "grouped_conv1d_input_grad: dx must not alias an input");
    const int64_t span = (int64_t)Tin + 2 * (int64_t)pad - k;
    if (span < 0)
        return fail(FV_ERR_INVALID_ARG, "grouped_conv1d_input_grad: empty output (Tin=%d pad=%d k=%d)", Tin, pad, k);
    return launch_grouped_conv1d_input_grad(g_up, g_map, y, w, dx, B, Cin, Cout, Tin, (int)(span / stride + 1), k,
                                            stride, pad, slope, (hipStream_t)stream);
}

int fv_disc_map_grad(const float* g_up, const float* g_map, const float* y, float* g_pre, int64_t n, float slope,
                     void* stream) {
    if ((!g_up && !g_map) || !g_pre || n < 1 || (n + 255) / 256 >= (int64_t)1 << 31)
        return fail(FV_ERR_INVALID_ARG, "disc_map_grad: null tensor or n=%lld", (long long)n);
    if (!y && slope != 1.f) return fail(FV_ERR_INVALID_ARG, "disc_map_grad: slope=%g needs the layer's output y", slope);
    return launch_disc_map_grad(g_up, g_map, y, g_pre, n, slope, (hipStream_t)stream);
}

int fv_reflect_pad_fold(const float* gp, float* dx, int rows, int64_t T, int P, void* stream) {
    if (!gp || !dx || gp == dx || rows < 1 || rows > 65535 || P < 0)
        return fail(FV_ERR_INVALID_ARG, "reflect_pad_fold: null tensor, rows=%d or P=%d", rows, P);
    if (T <= P || (T + 255) / 256 >= (int64_t)1 << 31)
        return fail(FV_ERR_INVALID_ARG, "reflect_pad_fold: T=%lld must exceed the pad %d", (long long)T, P);
    return launch_reflect_pad_fold(gp, dx, rows, T, P, (hipStream_t)stream);
}

int fv_avg_pool1d_input_grad(const float* g, float* dx, int rows, int64_t Tin, int k, int stride, int pad,
                             void* stream) {
    if (!g || !dx || g == dx || rows < 1 || rows > 65535 || k < 1 || stride < 1 || pad < 0 || 2 * pad > k)
        return fail(FV_ERR_INVALID_ARG, "avg_pool1d_input_grad: rows=%d k=%d stride=%d pad=%d", rows, k, stride, pad);
    const int64_t span = Tin + 2 * (int64_t)pad - k;
    if (Tin < 1 || span < 0 || (Tin + 255) / 256 >= (int64_t)1 << 31)
        return fail(FV_ERR_INVALID_ARG, "avg_pool1d_input_grad: empty output (Tin=%lld k=%d pad=%d)", (long long)Tin, k,
                    pad);
    return launch_avg_pool1d_input_grad(g, dx, rows, Tin, span / stride + 1, k, stride, pad, (hipStream_t)stream);
}

int fv_disc_score_grad(const float* const* e, const float* const* r, float* const* g, const int64_t* n,
                       const float* coef, int M, int B, void* stream) {
    if (M < 1 || M > FV_DISC_MAX_MAPS || !n)
        return fail(FV_ERR_INVALID_ARG, "disc_score_grad: M=%d maps (1..%d)", M, FV_DISC_MAX_MAPS);
    if (B <= 0 || B > 65535) return fail(FV_ERR_INVALID_ARG, "disc_score_grad: B=%d", B);
    if (!e || !r || !g || !coef) return fail(FV_ERR_INVALID_ARG, "disc_score_grad: null pointer");
    for (int m = 0; m < M; ++m) {
        if (n[m] < 1) return fail(FV_ERR_INVALID_ARG, "disc_score_grad: map %d has %lld elements", m, (long long)n[m]);
        if (!e[m] || !r[m] || g[m] == e[m] || g[m] == r[m])
            return fail(FV_ERR_INVALID_ARG, "disc_score_grad: map %d is null or its gradient aliases it", m);
    }
    if (score_grad_chunks(M, n) >= (int64_t)1 << 31) return fail(FV_ERR_INVALID_ARG, "disc_score_grad: maps too large");
    return launch_disc_score_grad(e, r, g, n, coef, M, B, (hipStream_t)stream);
}

int fv_conv1d_2src_fused(const float* x, const float* x2, const float* packed, const float* bias,
                         const float* res, float* y, float* y_act, int B, int Cin1, int Cin2, int Cout,
                         int T, int post, float act_slope, void* stream) {
    if (!x || !x2 || !packed || !y) return fail(FV_ERR_INVALID_ARG, "conv1d_2src: null tensor");
    if (x == y || x2 == y || x == y_act || x2 == y_act || (y_act && y_act == y))
        return fail(FV_ERR_INVALID_ARG, "conv1d_2src: y / y_act must not alias an input or each other");
    Op o = {};
    if (int rc = build_conv_2src(o, packed, bias, Cin1, Cin2, Cout, post, act_slope)) return rc;
    if (T <= 0) return fail(FV_ERR_INVALID_ARG, "conv1d_2src: empty output");
    return run_op(o, x, y, y_act, res, nullptr, nullptr, B, T, (hipStream_t)stream, x2);
}

int fv_conv1x1_2src_split_f16(const float* x, const float* x2, const float* packed, const float* bias, const float* res,
                              float* y, float* y_act, int B, int C, int T, float pre_slope, int post, float act_slope,
                              int* guard, void* stream) {
    if (!x || !x2 || !packed || !y) return fail(FV_ERR_INVALID_ARG, "conv1x1_2src_split_f16: null tensor");
    if (x == y || x2 == y || x == y_act || x2 == y_act || (y_act && y_act == y) || (res && (res == y || res == y_act)))
        return fail(FV_ERR_INVALID_ARG, "conv1x1_2src_split_f16: y / y_act must not alias an input or each other");
    Op o = {};
    if (int rc = build_convg(o, packed, bias, C, pre_slope, post, act_slope)) return rc;   // C: launch_convg's to refuse
    if (B < 0 || T < 0) return fail(FV_ERR_INVALID_ARG, "conv1x1_2src_split_f16: B=%d T=%d", B, T);
    return run_op(o, x, y, y_act, res, nullptr, nullptr, B, T, (hipStream_t)stream, x2, nullptr, 0, guard);
}

int fv_residual_stack_split_f16(const float* x, const float* packed, const float* bias_dilated, const float* bias_out, float* y,
                                float* y_act, int B, int C, int T, int k, int dil, float slope, int pad_mode, int post,
                                float act_slope, int* guard, void* stream) {
    if (!x || !packed || !y) return fail(FV_ERR_INVALID_ARG, "residual_stack_split_f16: null tensor");
    if (x == y || x == y_act || (y_act && y_act == y))
        return fail(FV_ERR_INVALID_ARG, "residual_stack_split_f16: y / y_act must not alias x or each other");
    Op o = {};
    if (int rc = build_stack(o, packed, bias_dilated, bias_out, C, k, dil, slope, pad_mode, post, act_slope)) return rc;
    if (B < 0 || T < 0) return fail(FV_ERR_INVALID_ARG, "residual_stack_split_f16: B=%d T=%d", B, T);
    return run_op(o, x, y, y_act, nullptr, nullptr, nullptr, B, T, (hipStream_t)stream, nullptr, nullptr, 0, guard);
}

int fv_conv_post_pqmf(const float* x, const float* packed, const float* bias, const float* h, float* y, int B, int Cin,
                      int S, int T, int k, int pad, float pre_slope, int post, int ntaps, void* stream) {
    // (a null filter is FV_ERR_INVALID_ARG here and FV_ERR_UNSUPPORTED from fv_plan_add_conv_post_pqmf)
    if (!x || !packed || !h || !y) return fail(FV_ERR_INVALID_ARG, "conv_post_pqmf: null tensor");
    Op o = {};
    if (int rc = build_conv_post_pqmf(o, packed, bias, h, Cin, S, k, pad, pre_slope, post, ntaps)) return rc;
    if (B <= 0 || T <= 0) return 0;
    if (conv_out_len(o, T) <= 0) return fail(FV_ERR_INVALID_ARG, "conv_post_pqmf: empty output");
    return run_op(o, x, y, nullptr, nullptr, nullptr, nullptr, B, T, (hipStream_t)stream);
}

}  // extern "C"

namespace fv {
// A pair at C >= 64 (split-f16 arithmetic only): conv1 of every member in one launch, then conv2 + residual
// (+ the MRF addends); the members' intermediates go through mid[j]
static int launch_wide_pairs(const PairParams& pp, float* const* mid, int C, int dil, hipStream_t s) {
    PairParams c1 = pp, c2 = pp;
    c1.act_slope = 1.f;
    c1.out_div = 1.f;
    c1.post = FV_POST_NONE;
    for (int j = 0; j < pp.n_members; ++j) {
        if (!mid || !mid[j]) return fail(FV_ERR_INVALID_ARG, "resblock pair: C = %d needs a scratch tensor per member (mid)", C);
        if (mid[j] == pp.m[j].x || mid[j] == pp.m[j].y || mid[j] == pp.m[j].y_act || mid[j] == pp.m[j].add1 ||
            mid[j] == pp.m[j].add2)
            return fail(FV_ERR_INVALID_ARG, "resblock pair: mid aliases another tensor of member %d", j);
        PairMember& a = c1.m[j];
        a.y = mid[j];
        a.y_act = nullptr;
        a.res = a.add1 = a.add2 = nullptr;
        PairMember& b = c2.m[j];
        b.x = mid[j];
        b.w1 = pp.m[j].w2;
        b.b1 = pp.m[j].b2;
        b.res = pp.m[j].x;
    }
    if (int rc = launch_convh(c1, C, dil, s)) return rc;
    return launch_convh(c2, C, 1, s);
}

// The kernel family of a launch of fused pairs.  The fused 64- / 128-channel kernels exist in split-f16 arithmetic only;
// so do pairs of that width at all (check_pair_args, which the direct entry and fv_plan_add_resblock_pair_ex both pass,
// refuses C >= 64 with FV_PAIR_F32), which is why testing `prec` here accepts exactly what testing C alone did.
int launch_pair_family(const PairParams& pp, float* const* mid, int C, int dil, int prec, hipStream_t s) {
    if (C == 64 && prec == FV_PAIR_SPLIT_F16) return launch_convp(pp, dil, s);
    if (C == 128 && prec == FV_PAIR_SPLIT_F16 && !tuning().pair128_unfused) return launch_convq(pp, dil, s);
    if (C >= 64) return launch_wide_pairs(pp, mid, C, dil, s);
    return launch_pairs(pp, C, dil, s);
}

}  // namespace fv

extern "C" {

int fv_resblock1_fused(int n, const float* const* x, const float* const* w1, const float* const* w2,
                       const float* const* b1, const float* const* b2, float* const* y, float* const* y_act,
                       const int* k, int B, int C, int T, int dil, float slope, float act_slope, void* stream) {
    return fv_resblock1_fused_ex(n, x, w1, w2, b1, b2, y, y_act, nullptr, nullptr, nullptr, k, B, C, T, dil, slope,
                                 1.f, FV_POST_NONE, act_slope, FV_PAIR_F32, nullptr, stream);
}

// (an unknown `prec`, and add1 / add2 / out_div / post with FV_PAIR_F32, are the launchers' to refuse here;
// fv_plan_add_resblock_pair_ex refuses them itself)
int fv_resblock1_fused_ex(int n, const float* const* x, const float* const* w1, const float* const* w2,
                          const float* const* b1, const float* const* b2, float* const* y, float* const* y_act,
                          float* const* mid, const float* const* add1, const float* const* add2, const int* k, int B,
                          int C, int T, int dil, float slope, float out_div, int post, float act_slope, int prec,
                          int* guard, void* stream) {
    if (!x || !w1 || !w2 || !y || !k) return fail(FV_ERR_INVALID_ARG, "resblock1_fused: null argument");
    if (n < 1 || n > 3) return fail(FV_ERR_INVALID_ARG, "resblock pair: %d members (1..3)", n);
    PairParams pp = {};
    for (int j = 0; j < n; ++j) {
        Op o = {};
        if (int rc = build_pair(o, j, w1, w2, b1, b2, k, C, dil, slope, out_div, post, act_slope, prec)) return rc;
        if (j == 0) pp = pair_params(o, n, B, T, prec == FV_PAIR_SPLIT_F16 ? guard : nullptr);
        if (!x[j] || !y[j] || x[j] == y[j] || (y_act && y_act[j] && (y_act[j] == y[j] || y_act[j] == x[j])))
            return fail(FV_ERR_INVALID_ARG, "resblock1_fused: member %d: null tensor, or y / y_act aliases x or each other", j);
        const PairMember mb = op_member(o, 0, x[j], y[j], at(y_act, j), nullptr, at(add1, j), at(add2, j));
        if ((mb.add1 && (mb.add1 == mb.y || mb.add1 == mb.y_act)) || (mb.add2 && (mb.add2 == mb.y || mb.add2 == mb.y_act)))
            return fail(FV_ERR_INVALID_ARG, "resblock1_fused: member %d: add1 / add2 alias an output", j);
        pp.m[j] = mb;
    }
    return launch_pair_family(pp, mid, C, dil, prec, (hipStream_t)stream);
}

// (32 channels pass the builder and are launch_pairs's to refuse; fv_plan_add_mrf_sum refuses them when the op is added)
int fv_mrf_stage(const float* const* x, const float* const* w1, const float* const* w2, const float* const* b1,
                 const float* const* b2, float* y, float* y_act, const int* k, int B, int C, int T, int dil,
                 float slope, float out_div, int post, float act_slope, void* stream) {
    if (!x || !w1 || !w2 || !y || !k) return fail(FV_ERR_INVALID_ARG, "mrf_stage: null argument");
    Op o = {};
    if (int rc = build_mrfsum(o, w1, w2, b1, b2, k, C, dil, slope, out_div, post, act_slope)) return rc;
    PairParams pp = pair_params(o, 3, B, T, nullptr);
    pp.sum = 1;
    for (int j = 0; j < 3; ++j) {
        if (!x[j] || x[j] == y || x[j] == y_act || (y_act && y_act == y))
            return fail(FV_ERR_INVALID_ARG, "mrf_stage: member %d: null input, or y / y_act aliases an input or each other", j);
        pp.m[j] = op_member(o, j, x[j], y, y_act);
    }
    return launch_pairs(pp, C, dil, (hipStream_t)stream);
}

int64_t fv_mrf_stage_workspace_bytes(int C) { return mrf_workspace_bytes(C); }

// (the workspace is launch_mrfh's to check here; fv_plan_add_mrf_stage_split_f16 checks it when the op is added)
int fv_mrf_stage_split_f16(const float* x, const float* packed, float* y, float* y_act, int B, int C, int T, const int* k,
                           const int* dil, float slope, float out_div, int post, float act_slope, const float* fold_w,
                           const float* fold_b, float* fold_y, void* workspace, int64_t workspace_bytes, int* guard,
                           void* stream) {
    Op o = {};
    if (int rc = build_stage(o, packed, C, k, dil, slope, out_div, post, act_slope, workspace, workspace_bytes)) return rc;
    if (B < 0 || T < 0) return fail(FV_ERR_INVALID_ARG, "mrf stage: B=%d T=%d", B, T);
    o.fold_w = fold_w;
    o.fold_b = fold_b;
    return launch_mrfh(mrf_params(o, x, y, y_act, fold_y, B, T, guard), C, o.sdil, (hipStream_t)stream);
}

// the stage in two block classes, or (cls 1 / 2) one class alone: y_r2 null.  (The order of the taps is launch_mrfw_split's to
// check here; fv_plan_add_mrf_stage_classes_f16 checks it itself.)
static int run_stage_classes(const float* x, const float* packed, float* y_s, float* y_r2, int cls, int B, int C, int T, const int* k,
                             const int* dil, float slope, void* workspace, int64_t workspace_bytes, int* guard, void* stream) {
    Op o = {};
    if (int rc = build_stage(o, packed, C, k, dil, slope, 1.f, FV_POST_NONE, 1.f, workspace, workspace_bytes)) return rc;
    if (C != 32) return fail(FV_ERR_UNSUPPORTED, "mrf stage (two classes): C = %d (32)", C);
    if (B < 0 || T < 0) return fail(FV_ERR_INVALID_ARG, "mrf stage (two classes): B=%d T=%d", B, T);
    return launch_mrfw_split(mrf_split_params(o, x, y_s, y_r2, B, T, guard), o.sdil, (hipStream_t)stream, cls);
}

int fv_mrf_stage_classes_f16(const float* x, const float* packed, float* y_s, float* y_r2, int B, int C, int T, const int* k,
                             const int* dil, float slope, void* workspace, int64_t workspace_bytes, int* guard, void* stream) {
    return run_stage_classes(x, packed, y_s, y_r2, 0, B, C, T, k, dil, slope, workspace, workspace_bytes, guard, stream);
}

int fv_debug_mrf_stage_class_f16(const float* x, const float* packed, float* y, int cls, int B, int C, int T, const int* k,
                                 const int* dil, float slope, void* workspace, int64_t workspace_bytes, void* stream) {
    if (cls != 1 && cls != 2) return fail(FV_ERR_INVALID_ARG, "debug_mrf_stage_class: class %d (1: A, 2: B)", cls);
    return run_stage_classes(x, packed, y, nullptr, cls, B, C, T, k, dil, slope, workspace, workspace_bytes, nullptr, stream);
}

int fv_debug_mrf_class_schedule(int B, int T, int nblk, int force, int64_t* info, unsigned* table) {
    if (!info || !table) return fail(FV_ERR_INVALID_ARG, "debug_mrf_class_schedule: null argument");
    fv::MrfClassPlan pl;
    if (!fv::mrf_class_plan(B, T, nblk, force != 0, pl))
        return fail(FV_ERR_INVALID_ARG, "debug_mrf_class_schedule: B=%d T=%d on %d blocks (1 .. %d blocks, B x T < 2^31)", B, T, nblk, fv::kSchedBlocks);
    const fv::Tuning& tn = fv::tuning();
    const int64_t v[12] = {pl.split, pl.n_a, pl.n_b, pl.makespan, pl.makespan_one, pl.reach_a, pl.reach_b, 384,
                           tn.mrf_cost_a, tn.mrf_cost_b, tn.mrf_cost_one, 0};
    memcpy(info, v, sizeof(v));
    memcpy(table, pl.range, sizeof(pl.range));
    return 0;
}

int fv_conv1d_split_f16(int n, const float* const* x, const float* const* packed, const float* const* bias,
                        const float* const* res, const float* const* add1, const float* const* add2, float* const* y,
                        float* const* y_act, const int* k, int B, int C, int T, int dil, int pad_mode, float pre_slope,
                        float out_div, int post, float act_slope, int* guard, void* stream) {
    if (!x || !packed || !y || !k) return fail(FV_ERR_INVALID_ARG, "conv1d_split_f16: null argument");
    if (n < 1 || n > 3) return fail(FV_ERR_INVALID_ARG, "conv1d_split_f16: %d members (1..3)", n);
    PairParams pp = {};
    for (int j = 0; j < n; ++j) {
        Op o = {};
        if (int rc = build_convh(o, j, packed, bias, k, C, dil, pad_mode, pre_slope, out_div, post, act_slope)) return rc;
        if (j == 0) pp = pair_params(o, n, B, T, guard);
        const PairMember& mb = pp.m[j] = op_member(o, 0, x[j], y[j], at(y_act, j), at(res, j), at(add1, j), at(add2, j));
        if (!mb.x || !mb.y || mb.x == mb.y || mb.y == mb.res || mb.y == mb.add1 || mb.y == mb.add2 ||
            (mb.y_act && (mb.y_act == mb.y || mb.y_act == mb.x || mb.y_act == mb.res)))
            return fail(FV_ERR_INVALID_ARG, "conv1d_split_f16: member %d: null tensor or an output aliases an input", j);
    }
    return launch_convh(pp, C, dil, (hipStream_t)stream);
}

int fv_div_probe(unsigned first_bits, int64_t n, float d, unsigned long long* mismatches, void* stream) {
    if (!mismatches || n <= 0) return fail(FV_ERR_INVALID_ARG, "div_probe: null counter / empty range");
    return fv::launch_div_probe(first_bits, (long long)n, d, mismatches, (hipStream_t)stream);
}

int fv_tuning_set(const char* key, int value) {
    if (!key) return fail(FV_ERR_INVALID_ARG, "tuning_set: null key");
    (void)tuning();                         // the environment (FV_TUNING=1) is read first, once
    for (const TuningEntry& e : kTuningTable)
        if (strcmp(e.key, key) == 0) {
            g_tuning.*(e.field) = value;
            return 0;
        }
    // Switches of removed experiments (convp_pp: the two-wave-group pair kernels): "off" is the one state they have left,
    // so a caller that puts every switch it knows back to its default keeps working; switching one on is an unknown key.
    static const char* const kRetiredKeys[] = {"convp_pp"};
    for (const char* retired : kRetiredKeys)
        if (value == 0 && strcmp(retired, key) == 0) return 0;
    return fail(FV_ERR_INVALID_ARG, "tuning_set: unknown key '%s'", key);
}

int fv_debug_launch_log(int on) {
    if (on != 0 && on != 1) return fail(FV_ERR_INVALID_ARG, "debug_launch_log: on = %d (0 or 1)", on);
    std::lock_guard<std::mutex> lock(fv::g_launch_log_mutex);
    if (on) {
        fv::g_launch_log.clear();
        fv::g_launch_log_streams.clear();
        fv::g_launch_log_copies = 0;
    }
    fv::g_launch_log_on.store(on, std::memory_order_relaxed);
    return 0;
}

int64_t fv_debug_launch_log_streams(uint64_t* handles, int64_t* counts, int64_t cap, int64_t* copies) {
    std::lock_guard<std::mutex> lock(fv::g_launch_log_mutex);
    const int64_t n = (int64_t)fv::g_launch_log_streams.size();
    for (int64_t i = 0; i < n && i < cap; ++i) {
        if (handles) handles[i] = (uint64_t)(uintptr_t)fv::g_launch_log_streams[i].first;
        if (counts) counts[i] = fv::g_launch_log_streams[i].second;
    }
    if (copies) *copies = fv::g_launch_log_copies;
    return n;
}

int64_t fv_debug_launch_log_read(char* buf, int64_t cap) {
    std::string text;
    {
        std::lock_guard<std::mutex> lock(fv::g_launch_log_mutex);
        for (const auto& e : fv::g_launch_log) {
            Dl_info info;
            std::string name;
            if (dladdr(e.first, &info) && info.dli_sname && info.dli_saddr == e.first) name = fv::kernel_display_name(info.dli_sname);
            else {                                  // a handle without an exported symbol: still one line, never a merged count
                char raw[32];
                snprintf(raw, sizeof(raw), "?%p", e.first);
                name = raw;
            }
            text += std::to_string(e.second) + "\t" + name + "\n";
        }
    }
    if (buf && cap > 0) {
        const size_t n = text.size() < (size_t)cap ? text.size() : (size_t)cap;
        memcpy(buf, text.data(), n);
    }
    return (int64_t)text.size();
}

int64_t fv_debug_kernel_name(const char* symbol, char* buf, int64_t cap) {
    if (!symbol) return fail(FV_ERR_INVALID_ARG, "debug_kernel_name: null symbol");
    const std::string name = fv::kernel_display_name(symbol);
    if (buf && cap > 0) {
        const size_t n = name.size() < (size_t)cap ? name.size() : (size_t)cap;
        memcpy(buf, name.data(), n);
    }
    return (int64_t)name.size();
}

int fv_debug_pair_schedule(int n_members, const int* n_items, const int* cost, int nblk, int mode, int three_members,
                           unsigned* table) {
    if (!n_items || !cost || !table) return fail(FV_ERR_INVALID_ARG, "debug_pair_schedule: null argument");
    if (n_members < 1 || n_members > 3) return fail(FV_ERR_INVALID_ARG, "debug_pair_schedule: %d members", n_members);
    if (mode != 0 && mode != 1) return fail(FV_ERR_INVALID_ARG, "debug_pair_schedule: mode %d", mode);
    if (nblk < 1 || nblk > (mode == 0 ? fv::kSchedBlocks : 2 * fv::kSchedBlocks))
        return fail(FV_ERR_INVALID_ARG, "debug_pair_schedule: %d blocks", nblk);
    fv::PairParams p = {};
    p.n_members = n_members;
    long long n[3] = {0, 0, 0};
    for (int m = 0; m < n_members; ++m) {
        // (the schedulers form block x n_items x cost sums in signed 64 bits: below 3 x 2^31 x 2^16 within these bounds)
        if (n_items[m] < 0 || n_items[m] >= (1LL << 31) / nblk || cost[m] < 1 || cost[m] > 65535)
            return fail(FV_ERR_INVALID_ARG, "debug_pair_schedule: member %d", m);
        p.m[m].n_items = n_items[m];
        p.m[m].cost = cost[m];
        n[m] = n_items[m];
    }
    if (mode == 0) fv::pair_schedule(p, nblk, three_members != 0);
    else fv::pair_cut_schedule(p, nblk, n);
    memcpy(table, p.sched, sizeof(p.sched));
    return p.sched_on;
}

int fv_debug_pair_widths(int C, int B, int T, int dil, int n_members, const int* taps, int blocks, int64_t* info) {
    if (!taps || !info) return fail(FV_ERR_INVALID_ARG, "debug_pair_widths: null argument");
    if (C != 128) return fail(FV_ERR_UNSUPPORTED, "debug_pair_widths: C = %d (128: the other launchers have one width)", C);
    if (dil != 1 && dil != 3 && dil != 5) return fail(FV_ERR_UNSUPPORTED, "debug_pair_widths: dilation %d (1, 3 or 5)", dil);
    if (n_members < 1 || n_members > 3) return fail(FV_ERR_INVALID_ARG, "debug_pair_widths: %d members", n_members);
    if (B < 1 || T < 1 || blocks < 1 || (double)B * T >= 2147483647.0)
        return fail(FV_ERR_INVALID_ARG, "debug_pair_widths: B=%d T=%d on %d blocks (B x T < 2^31)", B, T, blocks);
    for (int m = 0; m < n_members; ++m)
        if ((taps[m] != 3 && taps[m] != 7 && taps[m] != 11) || (m > 0 && taps[m] > taps[m - 1]))
            return fail(FV_ERR_INVALID_ARG, "debug_pair_widths: member %d: %d taps (3, 7 or 11, largest first)", m, taps[m]);
    const fv::PairWidthPlan pl = fv::pair_width_plan(B, T, n_members, taps, blocks);
    for (int m = 0; m < 3; ++m) {
        info[m] = m < n_members ? pl.nm[m] : 0;
        info[3 + m] = m < n_members ? pl.n_items[m] : 0;
        info[6 + m] = m < n_members ? pl.cost[m] : 0;
    }
    info[9] = pl.makespan;
    info[10] = pl.nblk;
    info[11] = 0;
    return 0;
}

int fv_profile_enable(int on) {
    g_prof_on = on != 0;
    g_prof_need_start = true;
    return 0;
}

// What the measurement adds to a launch: the end-of-launch event record is one more packet on the stream.  A chain
// of n (null kernel, event record) pairs against a chain of n null kernels, per launch.
__global__ void profile_null_kernel() {}

int fv_profile_bracket_cost(void* stream, int n, double* ms_per_bracket) {
    if (n <= 0 || !ms_per_bracket) return fail(FV_ERR_INVALID_ARG, "profile_bracket_cost: n=%d", n);
    hipStream_t s = (hipStream_t)stream;
    ScopedEvents events((size_t)n + 4);
    if (int rc = events.create()) return rc;
    const std::vector<hipEvent_t>& ev = events.ev;
    for (int i = 0; i < 8; ++i) FV_KERNEL_LAUNCH(profile_null_kernel, dim3(1), dim3(64), 0, s);
    FV_HIP(hipEventRecord(ev[n], s));
    for (int i = 0; i < n; ++i) {
        FV_KERNEL_LAUNCH(profile_null_kernel, dim3(1), dim3(64), 0, s);
        FV_HIP(hipEventRecord(ev[i], s));
    }
    FV_HIP(hipEventRecord(ev[n + 1], s));
    for (int i = 0; i < n; ++i) FV_KERNEL_LAUNCH(profile_null_kernel, dim3(1), dim3(64), 0, s);
    FV_HIP(hipEventRecord(ev[n + 2], s));
    FV_HIP(hipEventSynchronize(ev[n + 2]));
    float with = 0.f, without = 0.f;
    FV_HIP(hipEventElapsedTime(&with, ev[n], ev[n - 1]));
    FV_HIP(hipEventElapsedTime(&without, ev[n + 1], ev[n + 2]));
    const double cost = ((double)with - (double)without) / n;
    *ms_per_bracket = cost > 0 ? cost : 0;
    return 0;
}

// A dense stream of v_mfma_f32_16x16x32_f16 from registers: the matrix rate the device sustains when nothing else is asked of it.
typedef _Float16 peak_f16x8 __attribute__((ext_vector_type(8)));
typedef float peak_f32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(512) void profile_mfma_f16_kernel(float* out, int iters) {
    const int lane = threadIdx.x & 63;
    // eight operand pairs, one per accumulator, all different per lane and element and of both signs (products of order 1e-3):
    // consecutive MFMAs see different operands, as in a GEMM (the same pair every time would leave the multipliers' inputs
    // unchanged from one instruction to the next -- and the device's clock higher than any real kernel sees)
    peak_f16x8 a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            a[j][i] = (_Float16)(0.03125f * (float)(((lane * 7 + i * 13 + j * 17) % 29) - 14) + 0.001f * (float)j);
            b[j][i] = (_Float16)(0.0078125f * (float)(((lane * 11 + i * 5 + j * 23) % 31) - 15) - 0.0007f * (float)j);
        }
    peak_f32x4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = peak_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < iters; it += 8) {          // (iters: rounded up to a multiple of 8 by the host)
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[j], b[(j + r) & 7], acc[j], 0, 0, 0);
    }
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) t += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = t;
}

int fv_profile_mfma_f16_rate(float* scratch, long long scratch_floats, int launches, int iters, void* stream, double* tflops) {
    if (!scratch || !tflops || launches < 2 || iters < 1)
        return fail(FV_ERR_INVALID_ARG, "profile_mfma_f16_rate: launches=%d iters=%d", launches, iters);
    iters = (iters + 7) / 8 * 8;
    const int blocks = 2 * fv::device_cu_count();
    if (scratch_floats < 512LL * blocks)
        return fail(FV_ERR_INVALID_ARG, "profile_mfma_f16_rate: scratch of %lld floats, %lld needed", scratch_floats, 512LL * blocks);
    hipStream_t s = (hipStream_t)stream;
    ScopedEvents events(2);
    if (int rc = events.create()) return rc;
    const hipEvent_t e0 = events.ev[0], e1 = events.ev[1];
    const int first = launches / 2;
    for (int i = 0; i < launches; ++i) {
        if (i == first) FV_HIP(hipEventRecord(e0, s));
        FV_KERNEL_LAUNCH(profile_mfma_f16_kernel, dim3(blocks), dim3(512), 0, s, scratch, iters);
    }
    FV_HIP(hipEventRecord(e1, s));
    FV_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    FV_HIP(hipEventElapsedTime(&ms, e0, e1));
    const double flop = (double)(launches - first) * blocks * 8.0 * iters * 8.0 * 16384.0;
    *tflops = ms > 0.f ? flop / ((double)ms * 1e-3) / 1e12 : 0.0;
    return 0;
}

int fv_profile_collect(int kind, int64_t* launches, double* ms, double* flops, double* bytes) {
    if (int rc = profile_resolve()) return rc;
    double tms = 0, tf = 0, tb = 0;
    int64_t n = 0;
    std::vector<ProfRec> rest;
    for (ProfRec& r : g_prof) {
        if (kind >= 0 && r.kind != kind) {
            rest.push_back(r);
            continue;
        }
        tms += r.ms;
        tf += r.flops;
        tb += r.bytes;
        ++n;
    }
    if (launches) *launches = n;
    if (ms) *ms = tms;
    if (flops) *flops = tf;
    if (bytes) *bytes = tb;
    g_prof.swap(rest);
    return 0;
}

}  // extern "C"
