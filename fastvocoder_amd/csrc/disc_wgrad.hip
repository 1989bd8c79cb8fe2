// Parameter gradient of the multi-scale discriminator (reference: model/discriminator/msd.py; bin/train.py:143-188 the
// discriminator's update; include/fastvocoder_hip.h fv_conv1d_weight_grad, fv_grouped_conv1d_weight_grad,
// fv_weight_norm_grad).  Exact fp32 in the split / record / combine scheme of wgrad_tile.hpp: a UNIT is one row b and
// one run of output times, and the record of a split is
//     ws[s][0 .. Cout N)  the weight gradient,   ws[s][Cout N .. Cout N + Cout)  the bias gradient.
// Every word of a record that the second launch (wgrad_combine_kernel, here) reads is written by the first.
//
// dense_wgrad_mfma_kernel (Cout >= 64 and Cin k >= 64): dW as the GEMM [Cout] x [Cin k] over B Tout on WgTile<128>
// (wgrad_tile.hpp): a block owns 128 output channels x 128 columns n = ci k + j.  Per unit (32 output times) the
// gradient tile gs[128][32 (+1)] and the input rows xs[ci][32 + k - 1 (+1)] of the at most 127 / k + 2 channels the
// columns touch are staged in LDS -- padding by indexing, never materialised -- and lane l feeds
// A = gs[co][t + (l >> 5)], B = xs[ci][t + j + (l >> 5)]: the B operand is a span read once, not a [column][step]
// tile, so the kernel sets the tile's off_b itself.  The row strides 33 and 32 + k (congruent to k modulo 32) keep both
// operand reads free of bank conflicts.  Each result is one k-ordered fmaf chain over its units' times.
//
// dense_wgrad_plain_kernel (every other dense shape: the 1-channel first layer, the 1-channel score layer, channel
// counts below a tile): a block owns one (co, ci) and 8 taps at a time; its 256 threads stride over the times of the
// block's units, then a wave-shuffle + LDS tree adds them.
//
// grouped_wgrad_kernel<OC>: the strided grouped conv on the VALU.  Per group the GEMM is only (outputs per group) x 4 k
// with the input read at stride s, so a matrix-core tile would be mostly empty (4 outputs per group in the
// 1024 -> 1024 layer) and its B operand a gather; instead a thread owns one (ci, j) of the group and OC accumulators
// (OC = 16, or 4 for groups of at most 4 outputs), the group's gradient tile sits in LDS as gs[t][oc] (one float4
// broadcast per 4 outputs) and the 4 input rows as xs[ci][(TT - 1) s + k] (lanes read consecutive words).
#include <math.h>

#include "wgrad_tile.hpp"

namespace fv {

constexpr int kWgTaps = 8;          // plain kernel: taps per pass
constexpr int kWgChunk = 1024;      // plain kernel: output times per unit
constexpr int kWmGS = WgTile<kWgNT>::STR;   // mfma kernel (128 output channels x 128 columns, units of 32 times): row stride of gs
constexpr int kWgTT = 64;           // grouped kernel: output times per unit (halved until the tile fits LDS)
constexpr int kWgBlocks = 1024;     // blocks a launch aims at (512 for the mfma kernel: its blocks are large)

// xpad[q] of a row of Tin samples padded by `pad` on both sides (zeros, or mirrored without the edge sample)
struct WgArgs {
    const float* g;       // [B, Cout, Tout]
    const float* x;       // [B, Cin, Tin]
    float* ws;            // [S][R], R = Cout N + Cout
    WgSplit sp;
    int Cin, Cout, Tin, Tout, k, pad, reflect, stride;
    int with_bias;
};

__device__ __forceinline__ float wg_xpad(const float* __restrict__ row, int q, int Tin, int pad, int reflect) {
    if (q < 0 || q >= Tin + 2 * pad) return 0.f;
    int p = q - pad;
    if (p < 0) {
        if (!reflect) return 0.f;
        p = -p;
    } else if (p >= Tin) {
        if (!reflect) return 0.f;
        p = 2 * (Tin - 1) - p;
    }
    return row[p];
}

// grid (Cout Cin, 1, S)
__global__ __launch_bounds__(kWgThreads) void dense_wgrad_plain_kernel(WgArgs a) {
    __shared__ float part[4];
    const int co = blockIdx.x / a.Cin, ci = blockIdx.x % a.Cin, s = blockIdx.z;
    const int64_t u0 = (int64_t)s * a.sp.U / a.sp.S, u1 = (int64_t)(s + 1) * a.sp.U / a.sp.S;
    float* rec = a.ws + (size_t)s * a.sp.R;
    const bool bias = a.with_bias && ci == 0;
    for (int j0 = 0; j0 < a.k; j0 += kWgTaps) {
        float acc[kWgTaps];
#pragma unroll
        for (int jj = 0; jj < kWgTaps; ++jj) acc[jj] = 0.f;
        float bsum = 0.f;
        for (int64_t u = u0; u < u1; ++u) {
            const int b = (int)(u / a.sp.nch), c = (int)(u % a.sp.nch);
            const float* gr = a.g + ((size_t)b * a.Cout + co) * a.Tout;
            const float* xr = a.x + ((size_t)b * a.Cin + ci) * a.Tin;
            const int t1 = a.Tout - c * kWgChunk < kWgChunk ? a.Tout : (c + 1) * kWgChunk;
            for (int t = c * kWgChunk + threadIdx.x; t < t1; t += kWgThreads) {
                const float gv = gr[t];
                bsum += gv;
#pragma unroll
                for (int jj = 0; jj < kWgTaps; ++jj)
                    if (j0 + jj < a.k) acc[jj] = fmaf(gv, wg_xpad(xr, t + j0 + jj, a.Tin, a.pad, a.reflect), acc[jj]);
            }
        }
#pragma unroll
        for (int jj = 0; jj < kWgTaps; ++jj) {
            if (j0 + jj >= a.k) break;
            const float v = wg_block_sum(acc[jj], part);
            if (threadIdx.x == 0) rec[((size_t)co * a.Cin + ci) * a.k + j0 + jj] = v;
        }
        if (bias && j0 == 0) {
            const float v = wg_block_sum(bsum, part);
            if (threadIdx.x == 0) rec[(size_t)a.Cout * a.Cin * a.k + co] = v;
        }
    }
}

// grid (ceil(Cin k / 128), ceil(Cout / 128), S); dynamic LDS: gs[128][33] + xs[127 / k + 2][32 + k]
__global__ __launch_bounds__(kWgThreads) void dense_wgrad_mfma_kernel(WgArgs a) {
    extern __shared__ float lds[];
    float* gs = lds;
    float* xs = lds + kWgNT * kWmGS;
    const int k = a.k, W = kWgTK + k, N = a.Cin * k;
    const int n0 = blockIdx.x * kWgNT, co0 = blockIdx.y * kWgNT, s = blockIdx.z;
    const int n_last = n0 + kWgNT - 1 < N - 1 ? n0 + kWgNT - 1 : N - 1;
    const int ci_lo = n0 / k, nci = n_last / k - ci_lo + 1;
    const int tid = threadIdx.x;
    WgTile<kWgNT> tile;
    tile.init();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int n = n0 + tile.col(h);
        if (n > n_last) n = n_last;                       // (a column beyond N: any staged word; never stored)
        tile.off_b[h] = (n / k - ci_lo) * W + n % k + tile.kq;
    }
    float bsum = 0.f;
    const bool bias = a.with_bias && blockIdx.x == 0 && tid < kWgNT;
    const int64_t u0 = (int64_t)s * a.sp.U / a.sp.S, u1 = (int64_t)(s + 1) * a.sp.U / a.sp.S;
    for (int64_t u = u0; u < u1; ++u) {
        const int b = (int)(u / a.sp.nch), t0 = (int)(u % a.sp.nch) * kWgTK;
        __syncthreads();                                  // the previous unit's reads are done
        for (int i = tid; i < kWgNT * kWgTK; i += kWgThreads) {
            const int row = i >> 5, c = i & 31, co = co0 + row, t = t0 + c;
            gs[row * kWmGS + c] = (co < a.Cout && t < a.Tout) ? a.g[((size_t)b * a.Cout + co) * a.Tout + t] : 0.f;
        }
        for (int i = tid; i < nci * (W - 1); i += kWgThreads) {
            const int row = i / (W - 1), c = i - row * (W - 1);
            xs[row * W + c] = wg_xpad(a.x + ((size_t)b * a.Cin + ci_lo + row) * a.Tin, t0 + c, a.Tin, a.pad, a.reflect);
        }
        __syncthreads();
        tile.mma(gs, xs);
        if (bias)
#pragma unroll
            for (int c = 0; c < kWgTK; ++c) bsum += gs[tid * kWmGS + c];
    }
    float* rec = a.ws + (size_t)s * a.sp.R;
    tile.store(rec, co0, n0, a.Cout, N);
    if (bias && co0 + tid < a.Cout) rec[(size_t)a.Cout * N + co0 + tid] = bsum;
}

// grid (ceil(4 k / blockDim), G ceil(opg / OC), S); dynamic LDS: gs[TT][OC + 4] + xs[4][(TT - 1) s + k]
template <int OC>
__global__ __launch_bounds__(kWgThreads) void grouped_wgrad_kernel(WgArgs a, int TT) {
    extern __shared__ float lds[];
    constexpr int GW = OC + 4;                            // row stride of gs (16-byte aligned rows)
    const int NT = blockDim.x, tid = threadIdx.x;
    const int k = a.k, st = a.stride, XW = (TT - 1) * st + k;
    float* gs = lds;
    float* xs = lds + TT * GW;
    const int G = a.Cin / 4, opg = a.Cout / G, ocg = (opg + OC - 1) / OC;
    const int grp = blockIdx.y / ocg, oc0 = (blockIdx.y % ocg) * OC, s = blockIdx.z;
    const int pair = blockIdx.x * NT + tid;
    const bool valid = pair < 4 * k;
    const int ci = valid ? pair / k : 0, j = valid ? pair % k : 0;
    const int xoff = ci * XW + j;
    float acc[OC];
#pragma unroll
    for (int o = 0; o < OC; ++o) acc[o] = 0.f;
    float bsum = 0.f;
    const bool bias = a.with_bias && blockIdx.x == 0 && tid < OC;
    const int64_t u0 = (int64_t)s * a.sp.U / a.sp.S, u1 = (int64_t)(s + 1) * a.sp.U / a.sp.S;
    for (int64_t u = u0; u < u1; ++u) {
        const int b = (int)(u / a.sp.nch), t0 = (int)(u % a.sp.nch) * TT;
        const int nt = a.Tout - t0 < TT ? a.Tout - t0 : TT;
        __syncthreads();                                  // the previous unit's reads are done
        for (int i = tid; i < TT * OC; i += NT) {
            const int oc = i / TT, t = i - oc * TT;
            gs[t * GW + oc] = (t < nt && oc0 + oc < opg)
                                  ? a.g[((size_t)b * a.Cout + grp * opg + oc0 + oc) * a.Tout + t0 + t] : 0.f;
        }
        const int64_t p0 = (int64_t)t0 * st - a.pad;      // input position of xs[.][0]
        for (int i = tid; i < 4 * XW; i += NT) {
            const int c = i / XW, p = i - c * XW;
            const int64_t pos = p0 + p;
            xs[i] = (pos >= 0 && pos < a.Tin) ? a.x[((size_t)b * a.Cin + 4 * grp + c) * a.Tin + pos] : 0.f;
        }
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            const float xv = xs[xoff + t * st];
            const float4* gp = reinterpret_cast<const float4*>(gs + t * GW);
#pragma unroll
            for (int q = 0; q < OC / 4; ++q) {
                const float4 gv = gp[q];
                acc[4 * q + 0] = fmaf(gv.x, xv, acc[4 * q + 0]);
                acc[4 * q + 1] = fmaf(gv.y, xv, acc[4 * q + 1]);
                acc[4 * q + 2] = fmaf(gv.z, xv, acc[4 * q + 2]);
                acc[4 * q + 3] = fmaf(gv.w, xv, acc[4 * q + 3]);
            }
        }
        if (bias)
            for (int t = 0; t < nt; ++t) bsum += gs[t * GW + tid];
    }
    float* rec = a.ws + (size_t)s * a.sp.R;
    if (valid)
#pragma unroll
        for (int o = 0; o < OC; ++o)
            if (oc0 + o < opg) rec[((size_t)(grp * opg + oc0 + o) * 4 + ci) * k + j] = acc[o];
    if (bias && oc0 + tid < opg) rec[(size_t)a.Cout * 4 * k + grp * opg + oc0 + tid] = bsum;
}

// grid ceil((MN + Cout) / 256): dw[i] = sum_s ws[s][i], db[c] = sum_s ws[s][MN + c], s ascending
__global__ __launch_bounds__(256) void wgrad_combine_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                            float* __restrict__ db, int64_t MN, int Cout, int64_t R,
                                                            int S) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= MN + Cout) return;
    float* dst = i < MN ? (dw ? dw + i : nullptr) : (db ? db + (i - MN) : nullptr);
    if (!dst) return;
    float v = ws[i];
    int s = 1;
    for (; s + 8 <= S; s += 8) {                          // 8 loads in flight, added in the same ascending order:
        float t[8];                                       // the bits of the one-by-one loop, without its latency chain
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = ws[(size_t)(s + j) * R + i];
#pragma unroll
        for (int j = 0; j < 8; ++j) v += t[j];
    }
    for (; s < S; ++s) v += ws[(size_t)s * R + i];
    *dst = v;
}

// one block per row: dot = <dw_r, v_r>, n = |v_r|; dg_r = dot / n, dv_r = (g_r / n)(dw_r - (dot / n^2) v_r)
__global__ __launch_bounds__(256) void weight_norm_grad_kernel(const float* __restrict__ dw, const float* __restrict__ v,
                                                               const float* __restrict__ g, float* __restrict__ dv,
                                                               float* __restrict__ dg, int64_t inner) {
    __shared__ float part[4];
    const int r = blockIdx.x;
    const float* wr = dw + (size_t)r * inner;
    const float* vr = v + (size_t)r * inner;
    float dot = 0.f, ss = 0.f;
    for (int64_t i = threadIdx.x; i < inner; i += 256) {
        dot = fmaf(wr[i], vr[i], dot);
        ss = fmaf(vr[i], vr[i], ss);
    }
    dot = wg_block_sum(dot, part);
    ss = wg_block_sum(ss, part);
    const float nrm = sqrtf(ss);
    if (dg && threadIdx.x == 0) dg[r] = dot / nrm;
    if (!dv) return;
    const float scale = g[r] / nrm, c = dot / ss;
    for (int64_t i = threadIdx.x; i < inner; i += 256) dv[(size_t)r * inner + i] = scale * (wr[i] - c * vr[i]);
}

// ---- host side: which kernel, how many splits ----
enum { kWgPlain = 0, kWgMfma = 1, kWgGrouped16 = 2, kWgGrouped4 = 3 };

struct WgPlan : WgSplit {
    int path, TT, threads;
    size_t lds;
    dim3 grid;
};

static size_t wg_mfma_lds(int k) { return sizeof(float) * ((size_t)kWgNT * kWmGS + (size_t)(127 / k + 2) * (kWgTK + k)); }

static int dense_wgrad_plan(int B, int Cin, int Cout, int Tin, int k, int pad, int pad_mode, WgPlan* p) {
    if (Cin < 1 || Cout < 1 || k < 1 || (pad_mode != FV_PAD_ZERO && pad_mode != FV_PAD_REFLECT) ||
        (int64_t)Cin * Cout * k >= (int64_t)1 << 31 || (int64_t)Cin * Cout > 0x7fffffff)
        return fail(FV_ERR_UNSUPPORTED, "conv1d_weight_grad: Cin=%d Cout=%d k=%d pad_mode=%d", Cin, Cout, k, pad_mode);
    if (B <= 0 || B > 65535 || Tin < 1 || pad < 0 || (int64_t)Tin + 2 * (int64_t)pad >= (int64_t)1 << 30)
        return fail(FV_ERR_INVALID_ARG, "conv1d_weight_grad: B=%d, Tin=%d or pad=%d", B, Tin, pad);
    if (pad_mode == FV_PAD_REFLECT && pad >= Tin)
        return fail(FV_ERR_INVALID_ARG, "conv1d_weight_grad: a reflection pad of %d needs more than %d samples", pad, Tin);
    const int64_t Tout = (int64_t)Tin + 2 * (int64_t)pad - k + 1;
    if (Tout < 1) return fail(FV_ERR_INVALID_ARG, "conv1d_weight_grad: empty output (Tin=%d pad=%d k=%d)", Tin, pad, k);
    const int64_t N = (int64_t)Cin * k;
    p->R = (int64_t)Cout * N + Cout;
    p->TT = 0;
    p->threads = kWgThreads;
    if (Cout >= 64 && N >= 64 && wg_mfma_lds(k) <= 65536 && (Cout + kWgNT - 1) / kWgNT <= 65535) {
        p->path = kWgMfma;
        p->nch = (int)((Tout + kWgTK - 1) / kWgTK);
        p->U = (int64_t)B * p->nch;
        p->lds = wg_mfma_lds(k);
        const int64_t bx = (N + kWgNT - 1) / kWgNT, by = (Cout + kWgNT - 1) / kWgNT;
        p->S = wg_splits(bx * by, p->U, kWgBlocks / 2);
        p->grid = dim3((unsigned)bx, (unsigned)by, (unsigned)p->S);
    } else {
        p->path = kWgPlain;
        p->nch = (int)((Tout + kWgChunk - 1) / kWgChunk);
        p->U = (int64_t)B * p->nch;
        p->lds = 0;
        p->S = wg_splits((int64_t)Cin * Cout, p->U, kWgBlocks);
        p->grid = dim3((unsigned)(Cin * Cout), 1, (unsigned)p->S);
    }
    return 0;
}

static int grouped_wgrad_plan(int B, int Cin, int Cout, int Tin, int k, int stride, int pad, WgPlan* p) {
    if (Cin < 4 || Cin % 4 || Cout < 1 || Cout % (Cin / 4) || k < 1 || stride < 1)
        return fail(FV_ERR_UNSUPPORTED, "grouped_conv1d_weight_grad: Cin=%d Cout=%d k=%d stride=%d (Cin %% 4 == 0, "
                    "groups = Cin/4 dividing Cout, k >= 1, stride >= 1)", Cin, Cout, k, stride);
    const int G = Cin / 4, opg = Cout / G;
    if (grouped_conv_lds_bytes(k, stride, opg % 16 == 0 ? 16 : 4) > 65536)     // the forward's own bound
        return fail(FV_ERR_UNSUPPORTED, "grouped_conv1d_weight_grad: k=%d stride=%d exceed a block's shared memory", k,
                    stride);
    const int OC = opg > 4 ? 16 : 4;
    int TT = kWgTT;
    const auto lds = [&](int tt) { return sizeof(float) * ((size_t)tt * (OC + 4) + 4 * ((size_t)(tt - 1) * stride + k)); };
    while (TT > 1 && lds(TT) > 65536) TT /= 2;
    const int64_t by = (int64_t)G * ((opg + OC - 1) / OC);
    if (lds(TT) > 65536 || by > 65535 || (int64_t)Cout * 4 * k >= (int64_t)1 << 31)
        return fail(FV_ERR_UNSUPPORTED, "grouped_conv1d_weight_grad: k=%d stride=%d or %d groups exceed a launch", k,
                    stride, G);
    if (B <= 0 || B > 65535 || Tin < 1 || pad < 0)
        return fail(FV_ERR_INVALID_ARG, "grouped_conv1d_weight_grad: B=%d, Tin=%d or pad=%d", B, Tin, pad);
    const int64_t span = (int64_t)Tin + 2 * (int64_t)pad - k;
    if (span < 0)
        return fail(FV_ERR_INVALID_ARG, "grouped_conv1d_weight_grad: empty output (Tin=%d pad=%d k=%d)", Tin, pad, k);
    const int64_t Tout = span / stride + 1;
    p->path = OC == 16 ? kWgGrouped16 : kWgGrouped4;
    p->TT = TT;
    p->lds = lds(TT);
    p->threads = 4 * k >= kWgThreads ? kWgThreads : round_up(4 * k, 64);
    p->nch = (int)((Tout + TT - 1) / TT);
    p->U = (int64_t)B * p->nch;
    p->R = (int64_t)Cout * 4 * k + Cout;
    const int64_t bx = (4 * (int64_t)k + p->threads - 1) / p->threads;
    p->S = wg_splits(bx * by, p->U, kWgBlocks);
    p->grid = dim3((unsigned)bx, (unsigned)by, (unsigned)p->S);
    return 0;
}

int launch_wgrad_combine(const float* ws, float* dw, float* db, int64_t MN, int Cout, int64_t R, int S, hipStream_t st) {
    FV_KERNEL_LAUNCH(wgrad_combine_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, ws, dw, db, MN, Cout, R,
                       S);
    FV_HIP(hipGetLastError());
    return 0;
}

// the two launches: the kernel p.path names, then the combine
static int wgrad_run(const WgPlan& p, WgArgs a, float* dw, float* db, void* workspace, size_t workspace_bytes,
                     const char* who, hipStream_t st) {
    if (int rc = wg_tensor_check(who, a.g, a.x, dw, db)) return rc;
    if (int rc = wg_workspace_check(who, workspace, workspace_bytes, p.bytes())) return rc;
    a.sp = p;
    a.ws = static_cast<float*>(workspace);
    a.with_bias = db != nullptr;
    switch (p.path) {
    case kWgMfma:
        FV_KERNEL_LAUNCH(dense_wgrad_mfma_kernel, p.grid, dim3(kWgThreads), p.lds, st, a);
        break;
    case kWgPlain:
        FV_KERNEL_LAUNCH(dense_wgrad_plain_kernel, p.grid, dim3(kWgThreads), 0, st, a);
        break;
    case kWgGrouped16:
        FV_KERNEL_LAUNCH(grouped_wgrad_kernel<16>, p.grid, dim3(p.threads), p.lds, st, a, p.TT);
        break;
    default:
        FV_KERNEL_LAUNCH(grouped_wgrad_kernel<4>, p.grid, dim3(p.threads), p.lds, st, a, p.TT);
        break;
    }
    FV_HIP(hipGetLastError());
    return launch_wgrad_combine(a.ws, dw, db, p.R - a.Cout, a.Cout, p.R, p.S, st);
}

}  // namespace fv

using namespace fv;

extern "C" {

int64_t fv_conv_weight_grad_workspace_bytes(int grouped, int B, int Cin, int Cout, int Tin, int k, int stride, int pad,
                                            int pad_mode) {
    WgPlan p;
    const int rc = grouped ? grouped_wgrad_plan(B, Cin, Cout, Tin, k, stride, pad, &p)
                           : dense_wgrad_plan(B, Cin, Cout, Tin, k, pad, pad_mode, &p);
    if (rc) return rc;
    return (int64_t)p.bytes();
}

int fv_conv1d_weight_grad(const float* g_pre, const float* x, float* dw, float* db, int B, int Cin, int Cout, int Tin,
                          int k, int pad, int pad_mode, void* workspace, size_t workspace_bytes, void* stream) {
    WgPlan p;
    if (int rc = dense_wgrad_plan(B, Cin, Cout, Tin, k, pad, pad_mode, &p)) return rc;
    WgArgs a{};
    a.g = g_pre;
    a.x = x;
    a.Cin = Cin;
    a.Cout = Cout;
    a.Tin = Tin;
    a.Tout = Tin + 2 * pad - k + 1;
    a.k = k;
    a.pad = pad;
    a.reflect = pad_mode == FV_PAD_REFLECT;
    a.stride = 1;
    return wgrad_run(p, a, dw, db, workspace, workspace_bytes, "conv1d_weight_grad", (hipStream_t)stream);
}

int fv_grouped_conv1d_weight_grad(const float* g_pre, const float* x, float* dw, float* db, int B, int Cin, int Cout,
                                  int Tin, int k, int stride, int pad, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    WgPlan p;
    if (int rc = grouped_wgrad_plan(B, Cin, Cout, Tin, k, stride, pad, &p)) return rc;
    WgArgs a{};
    a.g = g_pre;
    a.x = x;
    a.Cin = Cin;
    a.Cout = Cout;
    a.Tin = Tin;
    a.Tout = (int)(((int64_t)Tin + 2 * (int64_t)pad - k) / stride + 1);
    a.k = k;
    a.pad = pad;
    a.reflect = 0;
    a.stride = stride;
    return wgrad_run(p, a, dw, db, workspace, workspace_bytes, "grouped_conv1d_weight_grad", (hipStream_t)stream);
}

int fv_weight_norm_grad(const float* dw, const float* v, const float* g, float* dv, float* dg, int dim0, int64_t inner,
                        void* stream) {
    if (!dw || !v || !g || (!dv && !dg) || dv == dw || dv == v || dim0 <= 0 || inner <= 0)
        return fail(FV_ERR_INVALID_ARG, "weight_norm_grad: null tensor, aliasing, dim0=%d or inner=%lld", dim0,
                    (long long)inner);
    FV_KERNEL_LAUNCH(weight_norm_grad_kernel, dim3(dim0), dim3(256), 0, (hipStream_t)stream, dw, v, g, dv, dg, inner);
    FV_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
