// What the generators' weight-gradient entries share between their two arithmetics (gen_grad.hip: exact fp32;
// gen_grad_bf16.hip: operands rounded to bf16, fp32 accumulation): the kernel arguments, the bias column of the
// launch, the plan, the argument checks and the launch + combine.  The unit length (reduction steps per staged tile)
// is the one thing that differs between them, so the plan and the bias column take it as a parameter.
#pragma once
#include "wgrad_tile.hpp"

namespace fv {

constexpr int kGgBRows = kWgNT / 8;   // rows of the B tile a thread stages (16)
constexpr int kGgDead = -(1 << 30);   // position of a column / row beyond the problem: below every source row

struct GgWArgs {
    const float* a;         // A source [B, M, TR]: row m, step t
    const float* b;         // B source [B, Cb, TB]: column n = cb k + j reads b[., cb, t sB + j dB - pad]
    const float* bias_src;  // [B, Cbias, Tbias], or null
    float* ws;              // [S][R], R = M N + Cbias
    WgSplit sp;
    int M, TR, Cb, TB, k, sB, dB, pad;
    int Cbias, Tbias, bias_scale;   // a unit's bias positions: [t0 bias_scale, (t0 + TK) bias_scale), the row's last unit to Tbias
    int x_tiles;            // column tiles of the GEMM (0: the bias alone); the blocks beyond them sum the bias
};

// the bias columns of a weight-gradient launch (the gridDim.x - x_tiles blocks with blockIdx.x >= x_tiles): the bias
// rows of the split's units [u0, u1) of TK steps each.  A channel is summed by ONE wave, its lanes striding the unit's
// positions, units ascending: a chain of dependent loads as long as the split.  The channels are dealt over the waves
// of all the bias blocks (wave w of bias block j owns channels 4 j + w, + 4 (blocks), ...); which wave sums a channel
// does not change the sum's bits.  The fp32 kernels launch one bias block (their matrix time covers its chain, and
// more blocks take CU slots from the tiles: 208 -> 305 us measured at 64 -> 64, k 3); the bf16 kernels, whose tiles
// finish first otherwise, up to 32.
template <int TK>
__device__ __forceinline__ void gg_bias_column(const GgWArgs& a, float* rec, int64_t u0, int64_t u1, int N) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves = 4 * ((int)gridDim.x - a.x_tiles);
    for (int c = 4 * ((int)blockIdx.x - a.x_tiles) + wave; c < a.Cbias; c += waves) {
        float v = 0.f;
        for (int64_t u = u0; u < u1; ++u) {
            const int b = (int)(u / a.sp.nch), ch = (int)(u % a.sp.nch);
            const int64_t p0 = (int64_t)ch * TK * a.bias_scale;
            int64_t p1 = ch == a.sp.nch - 1 ? a.Tbias : p0 + (int64_t)TK * a.bias_scale;
            if (p1 > a.Tbias) p1 = a.Tbias;
            const float* row = a.bias_src + ((size_t)b * a.Cbias + c) * a.Tbias;
            for (int64_t p = p0 + lane; p < p1; p += 64) v += row[p];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) rec[(size_t)a.M * N + c] = v;
    }
}

static inline int gg_rows(int M) { return M > 64 ? 128 : M > 32 ? 64 : M > 16 ? 32 : 16; }

// LAUNCH(MT) at the tile height rows = gg_rows(.): 128, 64, 32 or 16
#define GG_BY_ROWS(rows, LAUNCH)    \
    switch (rows) {                 \
    case 128: LAUNCH(128); break;   \
    case 64: LAUNCH(64); break;     \
    case 32: LAUNCH(32); break;     \
    default: LAUNCH(16); break;     \
    }

struct GgWPlan : WgSplit {
    int MT, bx, by;
};

// the plan of a weight-gradient GEMM of M rows x N columns over B rows of TR steps in units of `unit` steps, with
// Cbias bias words per record
static inline void gg_wgrad_plan(int B, int M, int64_t N, int TR, int Cbias, GgWPlan* p, int unit = kWgTK) {
    p->MT = gg_rows(M);
    p->bx = (int)((N + kWgNT - 1) / kWgNT);
    p->by = (M + p->MT - 1) / p->MT;
    p->nch = (TR + unit - 1) / unit;
    p->U = (int64_t)B * p->nch;
    p->R = (int64_t)M * N + Cbias;
    p->S = wg_splits((int64_t)p->bx * p->by, p->U, p->MT >= 64 ? 512 : 1024);
}

// the checks, the launch (`launch(MT, grid, args)`: the arithmetic's kernel at that tile height) and the combine
// `bias_blocks`: the most bias blocks per split (gg_bias_column)
template <class Launch>
static inline int gg_wgrad_run(const GgWPlan& p, GgWArgs a, float* dw, float* db, void* workspace,
                               size_t workspace_bytes, const char* who, hipStream_t st, int bias_blocks, Launch launch) {
    if (int rc = wg_tensor_check(who, a.a, a.b, dw, db)) return rc;
    if (int rc = wg_workspace_check(who, workspace, workspace_bytes, p.bytes())) return rc;
    a.sp = p;
    a.ws = static_cast<float*>(workspace);
    a.x_tiles = dw ? p.bx : 0;
    if (!db) a.bias_src = nullptr;
    if (!db) bias_blocks = 0;
    else if (bias_blocks > (a.Cbias + 3) / 4) bias_blocks = (a.Cbias + 3) / 4;
    const dim3 grid((unsigned)(a.x_tiles + bias_blocks), (unsigned)(dw ? p.by : 1), (unsigned)p.S);
    launch(p.MT, grid, a);
    FV_HIP(hipGetLastError());
    return launch_wgrad_combine(a.ws, dw, db, p.R - a.Cbias, a.Cbias, p.R, p.S, st);
}

static inline int dilated_wgrad_plan(int B, int Cin, int Cout, int Tin, int k, int dil, int pad, GgWPlan* p,
                                     int unit = kWgTK) {
    if (Cin < 1 || Cout < 1 || k < 1 || dil < 1 || (int64_t)Cin * Cout * k >= (int64_t)1 << 31 ||
        (int64_t)Cin * k >= (int64_t)1 << 30 || (Cout + 15) / 16 > 65535)
        return fail(FV_ERR_UNSUPPORTED, "conv1d_weight_grad_dilated: Cin=%d Cout=%d k=%d dil=%d", Cin, Cout, k, dil);
    if (B <= 0 || B > 65535 || Tin < 1 || pad < 0)
        return fail(FV_ERR_INVALID_ARG, "conv1d_weight_grad_dilated: B=%d, Tin=%d or pad=%d", B, Tin, pad);
    const int64_t Tout = (int64_t)Tin + 2 * (int64_t)pad - (int64_t)dil * (k - 1);
    if (Tout < 1)
        return fail(FV_ERR_INVALID_ARG, "conv1d_weight_grad_dilated: empty output (Tin=%d pad=%d k=%d dil=%d)", Tin, pad,
                    k, dil);
    const int64_t big = Cin > Cout ? Cin : Cout;
    if (big * ((int64_t)Tin + 2 * (int64_t)pad) >= (int64_t)1 << 30)
        return fail(FV_ERR_INVALID_ARG, "conv1d_weight_grad_dilated: a map of %lld x %d samples is too long",
                    (long long)big, Tin);
    gg_wgrad_plan(B, Cout, (int64_t)Cin * k, (int)Tout, Cout, p, unit);
    return 0;
}

static inline int dilated_mode_check(const char* who, int Tin, int pad, int pad_mode) {
    if (pad_mode != FV_PAD_ZERO && pad_mode != FV_PAD_REFLECT)
        return fail(FV_ERR_INVALID_ARG, "%s: pad_mode=%d (FV_PAD_ZERO or FV_PAD_REFLECT)", who, pad_mode);
    if (pad_mode == FV_PAD_REFLECT && pad >= Tin)
        return fail(FV_ERR_INVALID_ARG, "%s: a reflection pad of %d needs more than %d samples", who, pad, Tin);
    return 0;
}

// Tout, or an error code
static inline int64_t convt_grad_check(const char* who, int B, int Cin, int Cout, int Tin, int k, int stride, int pad,
                                       int out_pad) {
    if (Cin < 1 || Cout < 1 || k < 1 || stride < 1 || (int64_t)Cin * Cout * k >= (int64_t)1 << 31 ||
        (int64_t)Cout * k >= (int64_t)1 << 30 || (Cin + 15) / 16 > 65535)
        return fail(FV_ERR_UNSUPPORTED, "%s: Cin=%d Cout=%d k=%d stride=%d", who, Cin, Cout, k, stride);
    if (B <= 0 || B > 65535 || Tin < 1 || pad < 0)
        return fail(FV_ERR_INVALID_ARG, "%s: B=%d, Tin=%d or pad=%d", who, B, Tin, pad);
    const int64_t Tout = ((int64_t)Tin - 1) * stride - 2 * (int64_t)pad + k + out_pad;
    if (Tout < 1)
        return fail(FV_ERR_INVALID_ARG, "%s: empty output (Tin=%d k=%d stride=%d pad=%d out_pad=%d)", who, Tin, k, stride,
                    pad, out_pad);
    const int64_t span = (int64_t)Tin * stride + k + pad;
    if ((int64_t)Cout * (Tout > span ? Tout : span) >= (int64_t)1 << 30 || (int64_t)Cin * Tin >= (int64_t)1 << 30)
        return fail(FV_ERR_INVALID_ARG, "%s: a map of %d x %lld samples is too long", who, Cout, (long long)Tout);
    return Tout;
}

// the arguments of the dilated conv's weight gradient: [Cout] x [Cin k] over B Tout, columns read xa at t + j dil - pad
static inline GgWArgs gg_dilated_args(const float* g_pre, const float* xa, int Cin, int Cout, int Tin, int k, int dil,
                                      int pad) {
    const int Tout = Tin + 2 * pad - dil * (k - 1);
    GgWArgs a{};
    a.a = g_pre;
    a.b = xa;
    a.bias_src = g_pre;
    a.M = Cout;
    a.TR = Tout;
    a.Cb = Cin;
    a.TB = Tin;
    a.k = k;
    a.sB = 1;
    a.dB = dil;
    a.pad = pad;
    a.Cbias = Cout;
    a.Tbias = Tout;
    a.bias_scale = 1;
    return a;
}

// of the transposed conv's: [Cin] x [Cout k] over B Tin, columns gather g at t stride + j - pad
static inline GgWArgs gg_convt_args(const float* g, const float* xa, int Cin, int Cout, int Tin, int Tout, int k,
                                    int stride, int pad) {
    GgWArgs a{};
    a.a = xa;
    a.b = g;
    a.bias_src = g;
    a.M = Cin;
    a.TR = Tin;
    a.Cb = Cout;
    a.TB = Tout;
    a.k = k;
    a.sB = stride;
    a.dB = 1;
    a.pad = pad;
    a.Cbias = Cout;
    a.Tbias = Tout;
    a.bias_scale = stride;
    return a;
}

}  // namespace fv
