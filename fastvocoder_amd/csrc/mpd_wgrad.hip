// Parameter gradient of the multi-period discriminator (reference: model/discriminator/mpd.py:131-164 DiscriminatorP;
// bin/train.py:143-188 the discriminator's update; include/fastvocoder_hip.h fv_period_conv_weight_grad,
// fv_mpd_first_weight_grad).  Exact fp32 in the split / record / combine scheme of wgrad_tile.hpp: a UNIT is one row b
// and one run of flat output positions q = h' p + c, and the record of a split is
//     ws[s][0 .. Cout N)  the weight gradient,   ws[s][Cout N .. Cout N + Cout)  the bias gradient.
// Every word of a record that the second launch (wgrad_combine_kernel, disc_wgrad.hip) reads is written by the first.
//
// period_wgrad_mfma_kernel<P> (Cout >= 64 and Cin k >= 64: the three strided layers and the 1024 -> 1024 layer): dW as
// the GEMM [Cout] x [Cin k] over B H' p on WgTile<128> (wgrad_tile.hpp): a block owns 128 output channels x 128 columns
// n = ci k + j.  A unit is 32 consecutive flat positions q of one b.  Both operands are staged as the tile wants them,
// K-contiguous: gs[co][q] (a coalesced flat copy) and
// bs[n][q] = x[b, ci, stride h' + j - pad, c], the im2col column of (ci, j) -- the strided (or, at stride 1, dilated)
// read is resolved once, while staging, from per-thread offsets computed before the unit loop; rows outside [0, H)
// stage 0, so the padding is never materialised.  A unit therefore need not be a run of whole rows, one kernel serves
// both strides, and the MFMA loop reads A = gs[co][kk + (l >> 5)], B = bs[n][kk + (l >> 5)] with the same row stride
// of 33 words for both: the 32 lanes of a lane group read rows lm = 0..31 at 33 lm + const, 32 different banks, for
// every period and stride (a staged span xs[ci][(stride t + j) p + c] would make the B read depend on p and collide for
// p = 3, 5, 7, 11 as the forward's header notes).  The price is that x is loaded k / stride times per unit from L2
// instead of once; the stride-1 layer's alternative, de-interleaving to [B p, C, H] for fv_conv1d_weight_grad, costs
// two more passes over the 1024-channel maps and was not taken.  Each result is one q-ordered fmaf chain over its
// units.
//
// period_wgrad_plain_kernel (every other shape: conv_post, 1024 -> 1): a block owns one (co, ci) and all k <= 5 taps;
// its 256 threads stride over the positions of the block's units (1024 positions each), then a wave-shuffle + LDS tree
// adds them.
//
// mpd_first_wgrad_kernel (1 -> 32, k 5, stride 3, straight from the waveform): a block owns one output channel, its
// 5 taps and its bias; the reflect tail and the [H, p] view are the address arithmetic of mpd_first_kernel.
#include "wgrad_tile.hpp"

namespace fv {

constexpr int kPwThreads = kWgThreads;
constexpr int kPwTile = kWgNT;      // mfma kernel: output channels and columns per block
constexpr int kPwTK = kWgTK;        // mfma kernel: flat output positions per unit
constexpr int kPwStr = WgTile<kPwTile>::STR;            // row stride of gs and bs
constexpr int kPwRows = kPwTile * kPwTK / kPwThreads;   // rows of a tile a thread stages (16)
constexpr int kPwChunk = 1024;      // plain and first-layer kernels: flat output positions per unit
constexpr int kPwMaxK = 5;          // taps
constexpr int kPwFirstC = 32;       // channels of the first layer
constexpr int kPwBlocks = 1024;     // blocks a launch aims at (512 for the mfma kernel)

struct PwArgs {
    const float* g;       // [B, Cout, Hout, p]
    const float* x;       // [B, Cin, H, p]
    float* ws;            // [S][R]
    WgSplit sp;
    int Cin, Cout, H, Hout, k, stride, pad, p;
    int with_bias;
};

// grid (ceil(Cin k / 128), ceil(Cout / 128), S)
template <int P>
__global__ __launch_bounds__(kPwThreads) void period_wgrad_mfma_kernel(PwArgs a) {
    __shared__ float gs[kPwTile * kPwStr];
    __shared__ float bs[kPwTile * kPwStr];
    const int k = a.k, N = a.Cin * k, Nin = a.H * P, Nout = a.Hout * P;
    const int n0 = blockIdx.x * kPwTile, co0 = blockIdx.y * kPwTile, s = blockIdx.z;
    const int tid = threadIdx.x;
    // staging: this thread owns position sc of the unit and the rows sr + 8 i of both tiles
    const int sc = tid & 31, sr = tid >> 5;
    int x_off[kPwRows], x_row[kPwRows];                   // ci Nin, and j - pad (far below any row for n >= N)
#pragma unroll
    for (int i = 0; i < kPwRows; ++i) {
        const int n = n0 + sr + 8 * i;
        const int ci = n / k;
        x_off[i] = n < N ? ci * Nin : 0;
        x_row[i] = n < N ? n - ci * k - a.pad : -(1 << 29);
    }
    WgTile<kPwTile> tile;
    tile.init();
    float bsum = 0.f;
    const bool bias = a.with_bias && blockIdx.x == 0 && tid < kPwTile;
    const int64_t u0 = (int64_t)s * a.sp.U / a.sp.S, u1 = (int64_t)(s + 1) * a.sp.U / a.sp.S;
    for (int64_t u = u0; u < u1; ++u) {
        const int b = (int)(u / a.sp.nch), q = (int)(u % a.sp.nch) * kPwTK + sc;
        const bool live = q < Nout;
        const int t = q / P, c = q - t * P;
        const int r0 = a.stride * t;
        const float* gb = a.g + (size_t)b * a.Cout * Nout + q;
        const float* xb = a.x + (size_t)b * a.Cin * Nin + c;
        __syncthreads();                                  // the previous unit's reads are done
#pragma unroll
        for (int i = 0; i < kPwRows; ++i) {
            const int row = sr + 8 * i, co = co0 + row;
            gs[row * kPwStr + sc] = (live && co < a.Cout) ? gb[(size_t)co * Nout] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kPwRows; ++i) {
            const int row = sr + 8 * i, r = r0 + x_row[i];
            bs[row * kPwStr + sc] = (live && r >= 0 && r < a.H) ? xb[(size_t)x_off[i] + (size_t)r * P] : 0.f;
        }
        __syncthreads();
        tile.mma(gs, bs);
        if (bias)
#pragma unroll
            for (int cc = 0; cc < kPwTK; ++cc) bsum += gs[tid * kPwStr + cc];
    }
    float* rec = a.ws + (size_t)s * a.sp.R;
    tile.store(rec, co0, n0, a.Cout, N);
    if (bias && co0 + tid < a.Cout) rec[(size_t)a.Cout * N + co0 + tid] = bsum;
}

// grid (Cout Cin, 1, S)
__global__ __launch_bounds__(kPwThreads) void period_wgrad_plain_kernel(PwArgs a) {
    __shared__ float part[4];
    const int co = blockIdx.x / a.Cin, ci = blockIdx.x % a.Cin, s = blockIdx.z;
    const int p = a.p, Nin = a.H * p, Nout = a.Hout * p;
    const int64_t u0 = (int64_t)s * a.sp.U / a.sp.S, u1 = (int64_t)(s + 1) * a.sp.U / a.sp.S;
    float* rec = a.ws + (size_t)s * a.sp.R;
    float acc[kPwMaxK];
#pragma unroll
    for (int j = 0; j < kPwMaxK; ++j) acc[j] = 0.f;
    float bsum = 0.f;
    for (int64_t u = u0; u < u1; ++u) {
        const int b = (int)(u / a.sp.nch), ch = (int)(u % a.sp.nch);
        const float* gr = a.g + ((size_t)b * a.Cout + co) * Nout;
        const float* xr = a.x + ((size_t)b * a.Cin + ci) * Nin;
        const int q1 = Nout - ch * kPwChunk < kPwChunk ? Nout : (ch + 1) * kPwChunk;
        for (int q = ch * kPwChunk + threadIdx.x; q < q1; q += kPwThreads) {
            const float gv = gr[q];
            bsum += gv;
            const int t = q / p, c = q - t * p;
#pragma unroll
            for (int j = 0; j < kPwMaxK; ++j) {
                const int r = a.stride * t + j - a.pad;
                if (j < a.k && r >= 0 && r < a.H) acc[j] = fmaf(gv, xr[(size_t)r * p + c], acc[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kPwMaxK; ++j) {
        if (j >= a.k) break;
        const float v = wg_block_sum(acc[j], part);
        if (threadIdx.x == 0) rec[((size_t)co * a.Cin + ci) * a.k + j] = v;
    }
    if (a.with_bias && ci == 0) {
        const float v = wg_block_sum(bsum, part);
        if (threadIdx.x == 0) rec[(size_t)a.Cout * a.Cin * a.k + co] = v;
    }
}

// grid (32, 1, S); g [B, 32, H1, p], x [B, T]; record: dw [32][5], then db [32]
__global__ __launch_bounds__(kPwThreads) void mpd_first_wgrad_kernel(const float* __restrict__ g,
                                                                     const float* __restrict__ x, float* __restrict__ ws,
                                                                     int64_t T, int H, int H1, int p, int64_t U, int S,
                                                                     int nch, int with_bias) {
    __shared__ float part[4];
    const int co = blockIdx.x, s = blockIdx.z;
    const int N1 = H1 * p;
    const int64_t u0 = (int64_t)s * U / S, u1 = (int64_t)(s + 1) * U / S;
    float* rec = ws + (size_t)s * (kPwFirstC * kPwMaxK + kPwFirstC);
    float acc[kPwMaxK];
#pragma unroll
    for (int j = 0; j < kPwMaxK; ++j) acc[j] = 0.f;
    float bsum = 0.f;
    for (int64_t u = u0; u < u1; ++u) {
        const int b = (int)(u / nch), ch = (int)(u % nch);
        const float* gr = g + ((size_t)b * kPwFirstC + co) * N1;
        const float* xr = x + (size_t)b * T;
        const int n1 = N1 - ch * kPwChunk < kPwChunk ? N1 : (ch + 1) * kPwChunk;
        for (int n = ch * kPwChunk + threadIdx.x; n < n1; n += kPwThreads) {
            const float gv = gr[n];
            bsum += gv;
            const int h = n / p, c = n - h * p;
#pragma unroll
            for (int j = 0; j < kPwMaxK; ++j) {
                const int r = 3 * h + j - 2;
                if (r >= 0 && r < H) {
                    int64_t i = (int64_t)r * p + c;
                    if (i >= T) i = 2 * (T - 1) - i;      // the reflect tail (n_pad < T is checked by the caller)
                    acc[j] = fmaf(gv, xr[i], acc[j]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kPwMaxK; ++j) {
        const float v = wg_block_sum(acc[j], part);
        if (threadIdx.x == 0) rec[co * kPwMaxK + j] = v;
    }
    if (with_bias) {
        const float v = wg_block_sum(bsum, part);
        if (threadIdx.x == 0) rec[kPwFirstC * kPwMaxK + co] = v;
    }
}

// ---- host side: which kernel, how many splits ----
struct PwPlan : WgSplit {
    bool mfma;
    int Hout;
    dim3 grid;
};

// what fv_period_conv_weight_grad and its bf16 twin (gen_grad_bf16.hip) refuse alike (fv_internal.h)
int period_wgrad_check(int B, int Cin, int Cout, int H, int period, int k, int stride) {
    if (!mpd_period_ok(period))
        return fail(FV_ERR_UNSUPPORTED, "period_conv_weight_grad: period %d (2, 3, 5, 7 or 11)", period);
    if (Cin < 1 || Cout < 1 || k < 1 || k > kPwMaxK || k % 2 == 0 || stride < 1 || stride > 3 ||
        (int64_t)Cin * Cout * k >= (int64_t)1 << 31 || (int64_t)Cin * Cout > 0x7fffffff)
        return fail(FV_ERR_UNSUPPORTED, "period_conv_weight_grad: Cin=%d Cout=%d k=%d stride=%d (k 1, 3 or 5; stride "
                    "1..3)", Cin, Cout, k, stride);
    if (B <= 0 || B > 65535 || H < 1)
        return fail(FV_ERR_INVALID_ARG, "period_conv_weight_grad: B=%d or H=%d", B, H);
    const int64_t big = Cin > Cout ? Cin : Cout;
    if (big * ((int64_t)H + kPwMaxK) * period >= (int64_t)1 << 31)
        return fail(FV_ERR_INVALID_ARG, "period_conv_weight_grad: a map of %lld x %d x %d words is too long",
                    (long long)big, H, period);
    return 0;
}

static int period_wgrad_plan(int B, int Cin, int Cout, int H, int period, int k, int stride, PwPlan* p) {
    if (int rc = period_wgrad_check(B, Cin, Cout, H, period, k, stride)) return rc;
    const int Hout = (H - 1) / stride + 1;                // padding (k - 1) / 2
    const int64_t N = (int64_t)Cin * k, Nout = (int64_t)Hout * period;
    p->Hout = Hout;
    p->R = (int64_t)Cout * N + Cout;
    p->mfma = period_wgrad_gemm_shape(Cin, Cout, k);
    if (p->mfma) {
        p->nch = (int)((Nout + kPwTK - 1) / kPwTK);
        p->U = (int64_t)B * p->nch;
        const int64_t bx = (N + kPwTile - 1) / kPwTile, by = (Cout + kPwTile - 1) / kPwTile;
        p->S = wg_splits(bx * by, p->U, kPwBlocks / 2);
        p->grid = dim3((unsigned)bx, (unsigned)by, (unsigned)p->S);
    } else {
        p->nch = (int)((Nout + kPwChunk - 1) / kPwChunk);
        p->U = (int64_t)B * p->nch;
        p->S = wg_splits((int64_t)Cin * Cout, p->U, kPwBlocks);
        p->grid = dim3((unsigned)(Cin * Cout), 1, (unsigned)p->S);
    }
    return 0;
}

struct PwFirstPlan : WgSplit {
    MpdView v;
};

static int first_wgrad_plan(int B, int64_t T, int period, PwFirstPlan* p) {
    if (!mpd_period_ok(period))
        return fail(FV_ERR_UNSUPPORTED, "mpd_first_weight_grad: period %d (2, 3, 5, 7 or 11)", period);
    if (B <= 0 || B > 65535 || T < 1)
        return fail(FV_ERR_INVALID_ARG, "mpd_first_weight_grad: B=%d or T=%lld", B, (long long)T);
    p->v = mpd_view(T, period);
    if (p->v.n_pad >= T)
        return fail(FV_ERR_INVALID_ARG, "mpd_first_weight_grad: T=%lld is not longer than the reflect tail of %lld "
                    "samples", (long long)T, (long long)p->v.n_pad);
    if (T + p->v.n_pad >= (int64_t)1 << 30)
        return fail(FV_ERR_INVALID_ARG, "mpd_first_weight_grad: T=%lld too long", (long long)T);
    p->nch = (int)((p->v.H1 * period + kPwChunk - 1) / kPwChunk);
    p->U = (int64_t)B * p->nch;
    p->R = kPwFirstC * kPwMaxK + kPwFirstC;
    p->S = wg_splits(kPwFirstC, p->U, kPwBlocks);
    return 0;
}

}  // namespace fv

using namespace fv;

extern "C" {

int64_t fv_period_conv_weight_grad_workspace_bytes(int B, int Cin, int Cout, int H, int period, int k, int stride) {
    PwPlan p;
    if (int rc = period_wgrad_plan(B, Cin, Cout, H, period, k, stride, &p)) return rc;
    return (int64_t)p.bytes();
}

int fv_period_conv_weight_grad(const float* g_pre, const float* x, float* dw, float* db, int B, int Cin, int Cout, int H,
                               int period, int k, int stride, void* workspace, size_t workspace_bytes, void* stream) {
    PwPlan p;
    if (int rc = period_wgrad_plan(B, Cin, Cout, H, period, k, stride, &p)) return rc;
    if (int rc = wg_tensor_check("period_conv_weight_grad", g_pre, x, dw, db)) return rc;
    if (int rc = wg_workspace_check("period_conv_weight_grad", workspace, workspace_bytes, p.bytes())) return rc;
    const hipStream_t st = (hipStream_t)stream;
    PwArgs a{};
    a.sp = p;
    a.g = g_pre;
    a.x = x;
    a.ws = static_cast<float*>(workspace);
    a.Cin = Cin;
    a.Cout = Cout;
    a.H = H;
    a.Hout = p.Hout;
    a.k = k;
    a.stride = stride;
    a.pad = (k - 1) / 2;
    a.p = period;
    a.with_bias = db != nullptr;
    if (!p.mfma) {
        FV_KERNEL_LAUNCH(period_wgrad_plain_kernel, p.grid, dim3(kPwThreads), 0, st, a);
    } else {
#define FV_PERIOD(P)                                                                                  \
    case P:                                                                                           \
        FV_KERNEL_LAUNCH((period_wgrad_mfma_kernel<P>), p.grid, dim3(kPwThreads), 0, st, a);          \
        break;
        switch (period) {
            FV_PERIOD(2) FV_PERIOD(3) FV_PERIOD(5) FV_PERIOD(7) FV_PERIOD(11)
        }
#undef FV_PERIOD
    }
    FV_HIP(hipGetLastError());
    return launch_wgrad_combine(a.ws, dw, db, p.R - Cout, Cout, p.R, p.S, st);
}

int64_t fv_mpd_first_weight_grad_workspace_bytes(int B, int64_t T, int period) {
    PwFirstPlan p;
    if (int rc = first_wgrad_plan(B, T, period, &p)) return rc;
    return (int64_t)p.bytes();
}

int fv_mpd_first_weight_grad(const float* g_pre, const float* x, float* dw, float* db, int B, int64_t T, int period,
                             void* workspace, size_t workspace_bytes, void* stream) {
    PwFirstPlan p;
    if (int rc = first_wgrad_plan(B, T, period, &p)) return rc;
    if (int rc = wg_tensor_check("mpd_first_weight_grad", g_pre, x, dw, db)) return rc;
    if (int rc = wg_workspace_check("mpd_first_weight_grad", workspace, workspace_bytes, p.bytes())) return rc;
    const hipStream_t st = (hipStream_t)stream;
    float* ws = static_cast<float*>(workspace);
    FV_KERNEL_LAUNCH(mpd_first_wgrad_kernel, dim3(kPwFirstC, 1, (unsigned)p.S), dim3(kPwThreads), 0, st, g_pre, x, ws,
                       T, (int)p.v.H, (int)p.v.H1, period, p.U, p.S, p.nch, db != nullptr ? 1 : 0);
    FV_HIP(hipGetLastError());
    return launch_wgrad_combine(ws, dw, db, kPwFirstC * kPwMaxK, kPwFirstC, p.R, p.S, st);
}

}  // extern "C"
