// Parameter gradient of the HiFi-GAN generators (reference: model/generator/hifigan.py:92-106, the generator's half of
// bin/train.py:67-136; include/fastvocoder_hip.h fv_conv1d_weight_grad_dilated, fv_conv_transpose1d_input_grad,
// fv_conv_transpose1d_weight_grad, fv_tanh_grad, fv_residual_merge_grad, fv_grad_div).  Exact fp32, no atomics, no
// waiting between workgroups.
//
// All three GEMMs run on the tile of wgrad_tile.hpp (WgTile<MT>, MT = 128, 64, 32 or 16 rows by the channel count):
// both operands K-contiguous in LDS -- as[row][step], bs[column][step]; the staging writes put the 32 lanes of a group
// on 32 consecutive words of one row.  Each result is one step-ordered fmaf chain.
//
// The B operand is an im2col column resolved WHILE STAGING: bs[n][t] with
// n = (channel, tap) reads source[channel][t sB + j dB - pad] (zero outside the row) from per-thread offsets computed
// before the unit loop -- (sB, dB) = (1, dil) for the dilated conv's weight gradient, (stride, 1) for the transposed
// conv's.  The MFMA loop's B read is therefore the same conflict-free pattern for every dilation and stride; a staged
// span xs[ci][tile + dil (k - 1)] would be read at lane stride (row stride + dil-dependent tap offset) and collide for
// dil 3 and 5 at the tap counts 7 and 11.  The price: a source element is loaded once per tap that touches it, from L2
// after the first (a unit's span is a few KB), not once.
//
// gen_wgrad_kernel<MT>: dW[m][n] over (b, t) in the split / record / combine scheme of wgrad_tile.hpp (units of 32
// steps).  One extra block column sums the bias rows of the split's units (gen_grad_host.hpp gg_bias_column: wave w
// owns channels w, w + 4, ...; lanes stride the unit's positions; one shuffle tree at the end), so every record word the
// combine reads is written by this launch.
//
// gen_dgrad_kernel<MT>: the transposed conv's data gradient as the GEMM [Cin] x [B Tin] over Cout k: the columns are
// the flat positions q = b Tin + i, A = the forward's weight [Cin][Cout k] as it lies in memory, B the stride-s gather
// g[b, co, i s + j - p].  One launch; every element one (co, j)-ordered chain, whatever the batch or the grid.
//
// The ReflectionPad1d convs of MelGAN (fv_conv1d_weight_grad_dilated_mode, fv_conv1d_input_grad_reflect): the pad is
// never built.  gen_wgrad_kernel<MT, true> mirrors the staged position (i < 0 -> -i, i >= T -> 2 (T - 1) - i) where
// the dilated read is resolved anyway; the <MT, false> instantiations are the zero-padding kernels, unchanged.
// gen_dgrad_reflect_kernel<MT> is the GEMM [Cin] x [B T] over Cout k whose staged B operand of column i is the sum of
// its one to three gathers g[b, co, p - j dil] over the padded positions p that the pad maps onto i: the straight one
// p = i + pad, the left mirror p = pad - i (1 <= i <= pad) and the right mirror p = pad + 2 (T - 1) - i
// (T - 1 - pad <= i <= T - 2), added in that order before the MFMA sees them.  One launch, no [B, C, T + 2 pad] tensor.
#include <math.h>

#include "gen_grad_host.hpp"

namespace fv {

// grid (x_tiles + (bias ? 1 : 0), ceil(M / MT), S); REFLECT: the B source is read through a reflection pad (pad < TB)
template <int MT, bool REFLECT = false>
__global__ __launch_bounds__(kWgThreads) void gen_wgrad_kernel(GgWArgs a) {
    using T = WgTile<MT>;
    __shared__ float as[MT * T::STR];
    __shared__ float bs[kWgNT * T::STR];
    const int s = blockIdx.z, tid = threadIdx.x;
    const int64_t u0 = (int64_t)s * a.sp.U / a.sp.S, u1 = (int64_t)(s + 1) * a.sp.U / a.sp.S;
    const int N = a.Cb * a.k;
    float* rec = a.ws + (size_t)s * a.sp.R;
    if ((int)blockIdx.x >= a.x_tiles) {                   // the bias column
        if (blockIdx.y == 0) gg_bias_column<kWgTK>(a, rec, u0, u1, N);
        return;
    }
    const int n0 = blockIdx.x * kWgNT, m0 = blockIdx.y * MT;
    const int sc = tid & 31, sr = tid >> 5;
    int b_off[kGgBRows], b_pos[kGgBRows];                 // cb TB, and j dB - pad
#pragma unroll
    for (int i = 0; i < kGgBRows; ++i) {
        const int n = n0 + sr + 8 * i, cb = n / a.k;
        b_off[i] = n < N ? cb * a.TB : 0;
        b_pos[i] = n < N ? (n - cb * a.k) * a.dB - a.pad : kGgDead;
    }
    T tile;
    tile.init();
    for (int64_t u = u0; u < u1; ++u) {
        const int b = (int)(u / a.sp.nch), t = (int)(u % a.sp.nch) * kWgTK + sc;
        const bool live = t < a.TR;
        const float* ab = a.a + (size_t)b * a.M * a.TR + t;
        const float* bb = a.b + (size_t)b * a.Cb * a.TB;
        const int64_t tb = (int64_t)t * a.sB;
        __syncthreads();                                  // the previous unit's reads are done
#pragma unroll
        for (int i = 0; i < T::ARows; ++i) {
            const int row = sr + 8 * i, m = m0 + row;
            as[row * T::STR + sc] = (live && m < a.M) ? ab[(size_t)m * a.TR] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kGgBRows; ++i) {
            int64_t pos = tb + b_pos[i];
            if constexpr (REFLECT) {                      // one mirror is enough: pad < TB; a dead column stays outside
                if (pos < 0) pos = -pos;
                else if (pos >= a.TB) pos = 2 * ((int64_t)a.TB - 1) - pos;
            }
            bs[(sr + 8 * i) * T::STR + sc] = (live && pos >= 0 && pos < a.TB) ? bb[(size_t)b_off[i] + pos] : 0.f;
        }
        __syncthreads();
        tile.mma(as, bs);
    }
    tile.store(rec, m0, n0, a.M, N);
}

struct GgDArgs {
    const float* w;     // [Cin, Cout k]
    const float* g;     // [B, Cout, Tout]
    float* dx;          // [B, Cin, Tin]
    int64_t Q;          // B Tin
    int Cin, Cout, Tin, Tout, k, stride, pad;
};

// grid (ceil(B Tin / 128), ceil(Cin / MT))
template <int MT>
__global__ __launch_bounds__(kWgThreads) void gen_dgrad_kernel(GgDArgs a) {
    using T = WgTile<MT>;
    __shared__ float as[MT * T::STR];
    __shared__ float bs[kWgNT * T::STR];
    const int tid = threadIdx.x, sc = tid & 31, sr = tid >> 5;
    const int K = a.Cout * a.k, m0 = blockIdx.y * MT;
    const int64_t q0 = (int64_t)blockIdx.x * kWgNT;
    int64_t c_base[kGgBRows];                             // b Cout Tout
    int c_pos[kGgBRows];                                  // i stride - pad
#pragma unroll
    for (int i = 0; i < kGgBRows; ++i) {
        const int64_t q = q0 + sr + 8 * i;
        const int64_t b = q / a.Tin;
        c_base[i] = q < a.Q ? b * a.Cout * a.Tout : 0;
        c_pos[i] = q < a.Q ? (int)(q - b * a.Tin) * a.stride - a.pad : kGgDead;
    }
    T tile;
    tile.init();
    for (int kc = 0; kc < K; kc += kWgTK) {
        const int kk = kc + sc;
        const bool live = kk < K;
        const int co = kk / a.k, j = kk - co * a.k;
        __syncthreads();                                  // the previous tile's reads are done
#pragma unroll
        for (int i = 0; i < T::ARows; ++i) {
            const int row = sr + 8 * i, m = m0 + row;
            as[row * T::STR + sc] = (live && m < a.Cin) ? a.w[(size_t)m * K + kk] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kGgBRows; ++i) {
            const int pos = c_pos[i] + j;
            bs[(sr + 8 * i) * T::STR + sc] =
                (live && pos >= 0 && pos < a.Tout) ? a.g[(size_t)c_base[i] + (size_t)co * a.Tout + pos] : 0.f;
        }
        __syncthreads();
        tile.mma(as, bs);
    }
#pragma unroll
    for (int h = 0; h < T::FN; ++h) {
        const int64_t q = q0 + tile.col(h);
        if (q >= a.Q) continue;
        const int64_t b = q / a.Tin;
        float* out = a.dx + (size_t)b * a.Cin * a.Tin + (q - b * a.Tin);
#pragma unroll
        for (int f = 0; f < T::FM; ++f)
#pragma unroll
            for (int e = 0; e < T::NE; ++e) {
                const int m = m0 + tile.row(f, e);
                if (m < a.Cin) out[(size_t)m * a.Tin] = tile.acc[f][h][e];
            }
    }
}

struct GgRArgs {
    const float* w;     // [Cin, Cout k]: the forward's weight [Cout, Cin, k] with its first two axes swapped
    const float* g;     // [B, Cout, Tout]
    float* dx;          // [B, Cin, T]
    int64_t Q;          // B T
    int Cin, Cout, T, Tout, k, dil, pad;
};

// grid (ceil(B T / 128), ceil(Cin / MT))
template <int MT>
__global__ __launch_bounds__(kWgThreads) void gen_dgrad_reflect_kernel(GgRArgs a) {
    using T = WgTile<MT>;
    __shared__ float as[MT * T::STR];
    __shared__ float bs[kWgNT * T::STR];
    const int tid = threadIdx.x, sc = tid & 31, sr = tid >> 5;
    const int K = a.Cout * a.k, m0 = blockIdx.y * MT;
    const int64_t q0 = (int64_t)blockIdx.x * kWgNT;
    int64_t c_base[kGgBRows];                             // b Cout Tout
    int c_pos[kGgBRows];                                  // x + pad: the padded position of the straight gather
    int c_left[kGgBRows], c_right[kGgBRows];              // the mirrors' padded positions, kGgDead where there is none
#pragma unroll
    for (int i = 0; i < kGgBRows; ++i) {
        const int64_t q = q0 + sr + 8 * i;
        const int64_t b = q / a.T;
        const bool in = q < a.Q;
        const int x = (int)(q - b * a.T);
        c_base[i] = in ? b * a.Cout * a.Tout : 0;
        c_pos[i] = in ? x + a.pad : kGgDead;
        c_left[i] = (in && x >= 1 && x <= a.pad) ? a.pad - x : kGgDead;
        c_right[i] = (in && x >= a.T - 1 - a.pad && x <= a.T - 2) ? a.pad + 2 * (a.T - 1) - x : kGgDead;
    }
    T tile;
    tile.init();
    for (int kc = 0; kc < K; kc += kWgTK) {
        const int kk = kc + sc;
        const bool live = kk < K;
        const int co = kk / a.k, jd = (kk - co * a.k) * a.dil;
        const float* gr = a.g + (size_t)co * a.Tout;
        __syncthreads();                                  // the previous tile's reads are done
#pragma unroll
        for (int i = 0; i < T::ARows; ++i) {
            const int row = sr + 8 * i, m = m0 + row;
            as[row * T::STR + sc] = (live && m < a.Cin) ? a.w[(size_t)m * K + kk] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kGgBRows; ++i) {
            const float* gb = gr + (size_t)c_base[i];
            const int ps = c_pos[i] - jd, pl = c_left[i] - jd, pr = c_right[i] - jd;
            float v = (live && ps >= 0 && ps < a.Tout) ? gb[ps] : 0.f;       // straight, left mirror, right mirror
            if (live && pl >= 0 && pl < a.Tout) v += gb[pl];
            if (live && pr >= 0 && pr < a.Tout) v += gb[pr];
            bs[(sr + 8 * i) * T::STR + sc] = v;
        }
        __syncthreads();
        tile.mma(as, bs);
    }
#pragma unroll
    for (int h = 0; h < T::FN; ++h) {
        const int64_t q = q0 + tile.col(h);
        if (q >= a.Q) continue;
        const int64_t b = q / a.T;
        float* out = a.dx + (size_t)b * a.Cin * a.T + (q - b * a.T);
#pragma unroll
        for (int f = 0; f < T::FM; ++f)
#pragma unroll
            for (int e = 0; e < T::NE; ++e) {
                const int m = m0 + tile.row(f, e);
                if (m < a.Cin) out[(size_t)m * a.T] = tile.acc[f][h][e];
            }
    }
}

// ---- the elementwise steps of the walk ----
// the adjoint of y = tanh(z): g (1 - y y)
__global__ __launch_bounds__(256) void tanh_grad_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                        float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = g[i] * (1.f - y[i] * y[i]);
}

// the gradient in front of x_next = x + conv(lrelu(x)): g_y + (x > 0 ? 1 : slope) d, plus a running sum
// (no __restrict__: out may alias g_y, d or acc -- every thread reads its element before it writes it)
__global__ __launch_bounds__(256) void residual_merge_grad_kernel(const float* g_y, const float* d, const float* x,
                                                                  const float* acc, float* out, int64_t n, float slope) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = fmaf(x[i] > 0.f ? 1.f : slope, d[i], g_y[i]);
    out[i] = acc ? acc[i] + v : v;
}

// the adjoint of the MRF mean: g / div, a true division
__global__ __launch_bounds__(256) void grad_div_kernel(const float* __restrict__ g, float* __restrict__ out, int64_t n,
                                                       float div) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = g[i] / div;
}

// ---- host side ----
// the exact-fp32 kernel at the plan's tile height
static int gg_wgrad_f32(const GgWPlan& p, const GgWArgs& a, float* dw, float* db, void* workspace, size_t workspace_bytes,
                        const char* who, hipStream_t st, bool reflect = false) {
    return gg_wgrad_run(p, a, dw, db, workspace, workspace_bytes, who, st, 1, [&](int rows, dim3 grid, const GgWArgs& ka) {
#define GG_WGRAD(MT)                                                                                          \
    if (reflect) FV_KERNEL_LAUNCH((gen_wgrad_kernel<MT, true>), grid, dim3(kWgThreads), 0, st, ka);           \
    else FV_KERNEL_LAUNCH((gen_wgrad_kernel<MT, false>), grid, dim3(kWgThreads), 0, st, ka)
        GG_BY_ROWS(rows, GG_WGRAD)
#undef GG_WGRAD
    });
}

static int gg_elementwise_check(const char* who, const void* a, const void* b, const void* out, int64_t n) {
    if (!a || !b || !out || n < 1 || (n + 255) / 256 > 0x7fffffff)
        return fail(FV_ERR_INVALID_ARG, "%s: null tensor or n=%lld", who, (long long)n);
    return 0;
}

}  // namespace fv

using namespace fv;

extern "C" {

int64_t fv_conv1d_weight_grad_dilated_workspace_bytes(int B, int Cin, int Cout, int Tin, int k, int dil, int pad) {
    GgWPlan p;
    if (int rc = dilated_wgrad_plan(B, Cin, Cout, Tin, k, dil, pad, &p)) return rc;
    return (int64_t)p.bytes();
}

int64_t fv_conv1d_weight_grad_dilated_mode_workspace_bytes(int B, int Cin, int Cout, int Tin, int k, int dil, int pad,
                                                           int pad_mode) {
    GgWPlan p;
    if (int rc = dilated_wgrad_plan(B, Cin, Cout, Tin, k, dil, pad, &p)) return rc;
    if (int rc = dilated_mode_check("conv1d_weight_grad_dilated_mode", Tin, pad, pad_mode)) return rc;
    return (int64_t)p.bytes();
}

int fv_conv1d_weight_grad_dilated(const float* g_pre, const float* xa, float* dw, float* db, int B, int Cin, int Cout,
                                  int Tin, int k, int dil, int pad, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    return fv_conv1d_weight_grad_dilated_mode(g_pre, xa, dw, db, B, Cin, Cout, Tin, k, dil, pad, FV_PAD_ZERO, workspace,
                                              workspace_bytes, stream);
}

int fv_conv1d_weight_grad_dilated_mode(const float* g_pre, const float* xa, float* dw, float* db, int B, int Cin,
                                       int Cout, int Tin, int k, int dil, int pad, int pad_mode, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    GgWPlan p;
    if (int rc = dilated_wgrad_plan(B, Cin, Cout, Tin, k, dil, pad, &p)) return rc;
    if (int rc = dilated_mode_check("conv1d_weight_grad_dilated_mode", Tin, pad, pad_mode)) return rc;
    return gg_wgrad_f32(p, gg_dilated_args(g_pre, xa, Cin, Cout, Tin, k, dil, pad), dw, db, workspace, workspace_bytes,
                        "conv1d_weight_grad_dilated", (hipStream_t)stream, pad_mode == FV_PAD_REFLECT);
}

int fv_conv1d_input_grad_reflect(const float* g, const float* wt, float* dxa, int B, int Cin, int Cout, int Tin, int k,
                                 int dil, int pad, void* stream) {
    const char* who = "conv1d_input_grad_reflect";
    if (Cin < 1 || Cout < 1 || k < 1 || dil < 1 || (int64_t)Cin * Cout * k >= (int64_t)1 << 31 ||
        (int64_t)Cout * k >= (int64_t)1 << 30 || (Cin + 15) / 16 > 65535)
        return fail(FV_ERR_UNSUPPORTED, "%s: Cin=%d Cout=%d k=%d dil=%d", who, Cin, Cout, k, dil);
    if (B <= 0 || B > 65535 || Tin < 1 || pad < 0)
        return fail(FV_ERR_INVALID_ARG, "%s: B=%d, Tin=%d or pad=%d", who, B, Tin, pad);
    if (pad >= Tin) return fail(FV_ERR_INVALID_ARG, "%s: a reflection pad of %d needs more than %d samples", who, pad, Tin);
    const int64_t Tout = (int64_t)Tin + 2 * (int64_t)pad - (int64_t)dil * (k - 1);
    if (Tout < 1)
        return fail(FV_ERR_INVALID_ARG, "%s: empty output (Tin=%d pad=%d k=%d dil=%d)", who, Tin, pad, k, dil);
    const int64_t big = Cin > Cout ? Cin : Cout;
    if (big * ((int64_t)Tin + 2 * (int64_t)pad) >= (int64_t)1 << 30 || (int64_t)dil * (k - 1) >= (int64_t)1 << 30)
        return fail(FV_ERR_INVALID_ARG, "%s: a map of %lld x %d samples is too long", who, (long long)big, Tin);
    if (!g || !wt || !dxa || dxa == g || dxa == wt)
        return fail(FV_ERR_INVALID_ARG, "%s: null tensor, or the result aliases an input", who);
    GgRArgs a{};
    a.w = wt;
    a.g = g;
    a.dx = dxa;
    a.Q = (int64_t)B * Tin;
    a.Cin = Cin;
    a.Cout = Cout;
    a.T = Tin;
    a.Tout = (int)Tout;
    a.k = k;
    a.dil = dil;
    a.pad = pad;
    const int MT = gg_rows(Cin);
    const int64_t gx = (a.Q + kWgNT - 1) / kWgNT;
    if (gx > 0x7fffffff) return fail(FV_ERR_INVALID_ARG, "%s: B Tin = %lld", who, (long long)a.Q);
    const dim3 grid((unsigned)gx, (unsigned)((Cin + MT - 1) / MT));
    const hipStream_t st = (hipStream_t)stream;
#define GG_DGRAD(MT) FV_KERNEL_LAUNCH(gen_dgrad_reflect_kernel<MT>, grid, dim3(kWgThreads), 0, st, a)
    GG_BY_ROWS(MT, GG_DGRAD)
#undef GG_DGRAD
    FV_HIP(hipGetLastError());
    return 0;
}

int fv_conv_transpose1d_input_grad(const float* g, const float* w, float* dxa, int B, int Cin, int Cout, int Tin, int k,
                                   int stride, int pad, int out_pad, void* stream) {
    const int64_t Tout = convt_grad_check("conv_transpose1d_input_grad", B, Cin, Cout, Tin, k, stride, pad, out_pad);
    if (Tout < 0) return (int)Tout;
    if (!g || !w || !dxa || dxa == g || dxa == w)
        return fail(FV_ERR_INVALID_ARG, "conv_transpose1d_input_grad: null tensor, or the result aliases an input");
    GgDArgs a{};
    a.w = w;
    a.g = g;
    a.dx = dxa;
    a.Q = (int64_t)B * Tin;
    a.Cin = Cin;
    a.Cout = Cout;
    a.Tin = Tin;
    a.Tout = (int)Tout;
    a.k = k;
    a.stride = stride;
    a.pad = pad;
    const int MT = gg_rows(Cin);
    const int64_t gx = (a.Q + kWgNT - 1) / kWgNT;
    if (gx > 0x7fffffff) return fail(FV_ERR_INVALID_ARG, "conv_transpose1d_input_grad: B Tin = %lld", (long long)a.Q);
    const dim3 grid((unsigned)gx, (unsigned)((Cin + MT - 1) / MT));
    const hipStream_t st = (hipStream_t)stream;
#define GG_DGRAD(MT) FV_KERNEL_LAUNCH(gen_dgrad_kernel<MT>, grid, dim3(kWgThreads), 0, st, a)
    GG_BY_ROWS(MT, GG_DGRAD)
#undef GG_DGRAD
    FV_HIP(hipGetLastError());
    return 0;
}

int64_t fv_conv_transpose1d_weight_grad_workspace_bytes(int B, int Cin, int Cout, int Tin, int k, int stride, int pad,
                                                        int out_pad) {
    const int64_t Tout = convt_grad_check("conv_transpose1d_weight_grad", B, Cin, Cout, Tin, k, stride, pad, out_pad);
    if (Tout < 0) return Tout;
    GgWPlan p;
    gg_wgrad_plan(B, Cin, (int64_t)Cout * k, Tin, Cout, &p);
    return (int64_t)p.bytes();
}

int fv_conv_transpose1d_weight_grad(const float* g, const float* xa, float* dw, float* db, int B, int Cin, int Cout,
                                    int Tin, int k, int stride, int pad, int out_pad, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const int64_t Tout = convt_grad_check("conv_transpose1d_weight_grad", B, Cin, Cout, Tin, k, stride, pad, out_pad);
    if (Tout < 0) return (int)Tout;
    GgWPlan p;
    gg_wgrad_plan(B, Cin, (int64_t)Cout * k, Tin, Cout, &p);
    return gg_wgrad_f32(p, gg_convt_args(g, xa, Cin, Cout, Tin, (int)Tout, k, stride, pad), dw, db, workspace,
                        workspace_bytes, "conv_transpose1d_weight_grad", (hipStream_t)stream);
}

int fv_tanh_grad(const float* g, const float* y, float* out, int64_t n, void* stream) {
    if (int rc = gg_elementwise_check("tanh_grad", g, y, out, n)) return rc;
    FV_KERNEL_LAUNCH(tanh_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, y, out,
                       n);
    FV_HIP(hipGetLastError());
    return 0;
}

int fv_residual_merge_grad(const float* g_y, const float* d, const float* x, const float* acc, float* out, int64_t n,
                           float slope, void* stream) {
    if (int rc = gg_elementwise_check("residual_merge_grad", g_y, d, out, n)) return rc;
    if (!x) return fail(FV_ERR_INVALID_ARG, "residual_merge_grad: null tensor");
    FV_KERNEL_LAUNCH(residual_merge_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       g_y, d, x, acc, out, n, slope);
    FV_HIP(hipGetLastError());
    return 0;
}

int fv_grad_div(const float* g, float* out, int64_t n, float div, void* stream) {
    if (int rc = gg_elementwise_check("grad_div", g, g, out, n)) return rc;
    if (!(div != 0.f)) return fail(FV_ERR_INVALID_ARG, "grad_div: div = %g", (double)div);
    FV_KERNEL_LAUNCH(grad_div_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, out, n,
                       div);
    FV_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
