// The head of Basis-MelGAN for training (reference: basis_melgan.py:140-162 under bin/train.py:64-95 and loss.py:39-40;
// include/fastvocoder_hip.h fv_basis_head_forward, fv_basis_head_grad, fv_basis_weight_l1, fv_basis_weight_l1_grad).
// Exact fp32, no atomics, no waiting between workgroups: identical calls return identical bits.
//
// The trunk runs once over B + 1 rows, the last one the all-zero mel (generator/basis_grad.py), and ends in the raw
// Y [B+1, C, F].  With D[b] = relu(Y[b]) - relu(Y[B]) the module's two outputs are weight = D^T and
// est = crop(overlap_add(basis D)), the second by linearity of the overlap-add (fv_basis_ola on D).
//
// basis_head_grad_kernel: the whole head adjoint in one launch.  A block owns kBhTC channels x kBhTF frames and walks
//     the batch in ascending order.  Per row it stages the (kBhTF + 1) hop samples of g_est its frames touch (read as
//     0 from F hop on: the crop) next to the basis tile [L][kBhTC], which is staged once.  Lane = frame, so Y, g_w and
//     g_Y move in 256-byte runs; a wave owns four contiguous channels, whose basis taps are one 16-byte LDS broadcast
//     per tap.  A lane's sample reads are hop words apart: conflict-free for an odd hop (the shipped 15).  Each
//     element is one j-ordered fmaf chain plus g_w; the block keeps the running batch sum in registers and writes
//     row B = -[Y[B] > 0] sum last.
// basis_l1_kernel / basis_l1_finish_kernel: mean |D^T - target| and mean D.  D [B,C,F] is read with lane = frame into
//     a 64 x 65 LDS tile, target [B,F,C] with lane = channel against the tile's columns (bank = lane + frame:
//     conflict-free), so both sides move in 256-byte runs.  Per block two doubles (a fixed xor tree inside a wave, the
//     four waves in ascending order); the one-block finish adds them as optim.hip's does.
// basis_l1_grad_kernel: coef sign(D^T - target) / (B F C) in D's storage, target through the same tile.
#include <math.h>

#include "basis_grad_host.hpp"
#include "fv_internal.h"

namespace fv {

typedef float bh_f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void basis_head_forward_kernel(const float* __restrict__ Y, float* __restrict__ D,
                                                                 int B, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float z = fmaxf(Y[(int64_t)B * n + i], 0.f);
    for (int b = 0; b < B; ++b) D[(int64_t)b * n + i] = fmaxf(Y[(int64_t)b * n + i], 0.f) - z;
}

struct BhArgs {
    const float* g_est;
    const float* g_w;
    const float* Y;
    const float* basis;
    float* g_Y;
    int B, C, F, L, hop, span;
    int64_t n;
};

__global__ __launch_bounds__(kBhThreads) void basis_head_grad_kernel(BhArgs a) {
    extern __shared__ __attribute__((aligned(16))) float bh_smem[];
    float* sb = bh_smem;                       // [L][kBhTC]
    float* sg = bh_smem + a.L * kBhTC;         // [span]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t f0 = (int64_t)blockIdx.x * kBhTF;
    const int c0 = blockIdx.y * kBhTC;
    if (a.g_est)
        for (int i = tid; i < a.L * kBhTC; i += kBhThreads) {
            const int c = c0 + i % kBhTC;
            sb[i] = c < a.C ? a.basis[(int64_t)(i / kBhTC) * a.C + c] : 0.f;
        }
    const int64_t f = f0 + lane, s0 = f0 * a.hop;
    const int cw = c0 + kBhPer * w;
    const bool live = f < a.F;
    float sum[kBhPer] = {};
    for (int b = 0; b < a.B; ++b) {
        float v[kBhPer] = {};
        if (a.g_est) {
            __syncthreads();                   // the row before is read; the basis tile is written
            const float* src = a.g_est + (int64_t)b * a.n;
            for (int i = tid; i < a.span; i += kBhThreads) sg[i] = s0 + i < a.n ? src[s0 + i] : 0.f;
            __syncthreads();
            for (int j = 0; j < a.L; ++j) {
                const bh_f32x4 bw = *(const bh_f32x4*)(sb + j * kBhTC + kBhPer * w);
                const float s = sg[basis_head_tap(lane, a.hop, j)];
#pragma unroll
                for (int i = 0; i < kBhPer; ++i) v[i] = fmaf(bw[i], s, v[i]);
            }
        }
        if (!live) continue;
#pragma unroll
        for (int i = 0; i < kBhPer; ++i) {
            if (cw + i >= a.C) break;
            const int64_t at = ((int64_t)b * a.C + cw + i) * a.F + f;
            const float gp = a.g_w ? v[i] + a.g_w[at] : v[i];
            sum[i] += gp;
            a.g_Y[at] = a.Y[at] > 0.f ? gp : 0.f;
        }
    }
    if (!live) return;
#pragma unroll
    for (int i = 0; i < kBhPer; ++i) {
        if (cw + i >= a.C) break;
        const int64_t at = ((int64_t)a.B * a.C + cw + i) * a.F + f;
        a.g_Y[at] = a.Y[at] > 0.f ? -sum[i] : 0.f;
    }
}
static_assert(kBhPer == 4, "a wave's basis taps are one 16-byte LDS read");

// the sum of a block's 256 doubles, in a fixed order, valid in thread 0
static __device__ __forceinline__ double bl_block_sum(double d, double* wave_sum) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) d += __shfl_xor(d, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = d;
    __syncthreads();
    double t = wave_sum[0];
#pragma unroll
    for (int w = 1; w < kBhThreads / 64; ++w) t += wave_sum[w];
    return t;
}

__global__ __launch_bounds__(kBhThreads) void basis_l1_kernel(const float* __restrict__ D, const float* __restrict__ tgt,
                                                              double* __restrict__ part, int C, int F) {
    __shared__ float tile[kBlT][kBlT + 1];     // [channel][frame]
    __shared__ double wave_abs[kBhThreads / 64], wave_d[kBhThreads / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t b = blockIdx.z, f0 = (int64_t)blockIdx.x * kBlT;
    const int c0 = blockIdx.y * kBlT;
    float sd = 0.f;
#pragma unroll
    for (int i = 0; i < kBlPer; ++i) {
        const int cl = w + 4 * i;
        const float v = (c0 + cl < C && f0 + lane < F) ? D[(b * C + c0 + cl) * F + f0 + lane] : 0.f;
        tile[cl][lane] = v;
        sd += v;
    }
    __syncthreads();
    float sa = 0.f;
#pragma unroll
    for (int i = 0; i < kBlPer; ++i) {
        const int fl = w + 4 * i;
        if (f0 + fl < F && c0 + lane < C) sa += fabsf(tile[lane][fl] - tgt[(b * F + f0 + fl) * C + c0 + lane]);
    }
    const double ta = bl_block_sum((double)sa, wave_abs), td = bl_block_sum((double)sd, wave_d);
    if (threadIdx.x == 0) {
        const int64_t at = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part[2 * at] = ta;
        part[2 * at + 1] = td;
    }
}

__global__ __launch_bounds__(kBhThreads) void basis_l1_finish_kernel(const double* __restrict__ part, int64_t blocks,
                                                                     double count, float* __restrict__ out) {
    __shared__ double range_abs[kBhThreads], range_d[kBhThreads];
    int64_t lo, hi;
    basis_l1_range(blocks, (int)threadIdx.x, &lo, &hi);
    double ta = 0.0, td = 0.0;
    for (int64_t i = lo; i < hi; ++i) {
        ta += part[2 * i];
        td += part[2 * i + 1];
    }
    range_abs[threadIdx.x] = ta;
    range_d[threadIdx.x] = td;
    __syncthreads();
    if (threadIdx.x != 0) return;
    ta = td = 0.0;
    for (int i = 0; i < kBhThreads; ++i) {
        ta += range_abs[i];
        td += range_d[i];
    }
    out[0] = (float)(ta / count);
    out[1] = (float)(td / count);
}

__global__ __launch_bounds__(kBhThreads) void basis_l1_grad_kernel(const float* __restrict__ D,
                                                                   const float* __restrict__ tgt,
                                                                   const float* __restrict__ coef,
                                                                   float* __restrict__ g, int C, int F, float count) {
    __shared__ float tile[kBlT][kBlT + 1];     // [frame][channel]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t b = blockIdx.z, f0 = (int64_t)blockIdx.x * kBlT;
    const int c0 = blockIdx.y * kBlT;
#pragma unroll
    for (int i = 0; i < kBlPer; ++i) {
        const int fl = w + 4 * i;
        tile[fl][lane] = (f0 + fl < F && c0 + lane < C) ? tgt[(b * F + f0 + fl) * C + c0 + lane] : 0.f;
    }
    __syncthreads();
    const float s = (coef ? coef[0] : 1.f) / count;
#pragma unroll
    for (int i = 0; i < kBlPer; ++i) {
        const int cl = w + 4 * i;
        if (c0 + cl >= C || f0 + lane >= F) continue;
        const int64_t at = (b * C + c0 + cl) * F + f0 + lane;
        const float d = D[at] - tile[lane][cl];
        g[at] = d > 0.f ? s : d < 0.f ? -s : 0.f;
    }
}

static int bg_check(const char* who, int B, int C, int F) {
    const int rc = basis_shape_check(B, C, F);
    if (rc == 1) return fail(FV_ERR_INVALID_ARG, "%s: B=%d C=%d F=%d (each 1 or more)", who, B, C, F);
    if (rc == 2) return fail(FV_ERR_UNSUPPORTED, "%s: B=%d C=%d F=%d exceed a launch", who, B, C, F);
    return 0;
}

}  // namespace fv

using namespace fv;

extern "C" {

int fv_basis_head_forward(const float* Y, float* D, int B, int C, int F, void* stream) {
    if (int rc = bg_check("basis_head_forward", B, C, F)) return rc;
    if (!Y || !D || Y == D) return fail(FV_ERR_INVALID_ARG, "basis_head_forward: null tensor, or D aliases Y");
    const int64_t n = (int64_t)C * F;
    FV_KERNEL_LAUNCH(basis_head_forward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Y,
                       D, B, n);
    FV_HIP(hipGetLastError());
    return 0;
}

int fv_basis_head_grad(const float* g_est, const float* g_w, const float* Y, const float* basis, float* g_Y, int B, int C,
                       int F, int L, void* stream) {
    const int lrc = basis_L_check(L);
    if (lrc == 1) return fail(FV_ERR_INVALID_ARG, "basis_head_grad: L=%d (even, >= 2)", L);
    if (int rc = bg_check("basis_head_grad", B, C, F)) return rc;
    if (lrc == 2) return fail(FV_ERR_UNSUPPORTED, "basis_head_grad: L=%d (%d at most)", L, kBhMaxL);
    if (!Y || !g_Y || (!g_est && !g_w) || (g_est && !basis))
        return fail(FV_ERR_INVALID_ARG, "basis_head_grad: null tensor (one of g_est and g_w may be null)");
    if (g_Y == Y || g_Y == g_w || g_Y == g_est)
        return fail(FV_ERR_INVALID_ARG, "basis_head_grad: g_Y aliases an input");
    const BasisHeadGeom g = basis_head_geom(C, F, L);
    BhArgs a = {g_est, g_w, Y, basis, g_Y, B, C, F, L, g.hop, g.span, g.n};
    FV_KERNEL_LAUNCH(basis_head_grad_kernel, dim3(g.gx, g.gy), dim3(kBhThreads), g.lds_bytes, (hipStream_t)stream, a);
    FV_HIP(hipGetLastError());
    return 0;
}

int64_t fv_basis_weight_l1_workspace_bytes(int B, int C, int F) {
    if (int rc = bg_check("basis_weight_l1", B, C, F)) return rc;
    return 2 * (int64_t)sizeof(double) * basis_l1_geom(B, C, F).blocks;
}

int fv_basis_weight_l1(const float* D, const float* target, float* out, int B, int C, int F, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (int rc = bg_check("basis_weight_l1", B, C, F)) return rc;
    if (!D || !target || !out) return fail(FV_ERR_INVALID_ARG, "basis_weight_l1: null tensor");
    const BasisL1Geom g = basis_l1_geom(B, C, F);
    const size_t need = 2 * sizeof(double) * (size_t)g.blocks;
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7))
        return fail(FV_ERR_INVALID_ARG, "basis_weight_l1: workspace of %zu bytes, needs %zu (8-byte aligned)",
                    workspace_bytes, need);
    double* part = static_cast<double*>(workspace);
    FV_KERNEL_LAUNCH(basis_l1_kernel, dim3(g.gx, g.gy, g.gz), dim3(kBhThreads), 0, (hipStream_t)stream, D, target, part,
                       C, F);
    FV_HIP(hipGetLastError());
    FV_KERNEL_LAUNCH(basis_l1_finish_kernel, dim3(1), dim3(kBhThreads), 0, (hipStream_t)stream, part, g.blocks, g.count,
                       out);
    FV_HIP(hipGetLastError());
    return 0;
}

int fv_basis_weight_l1_grad(const float* D, const float* target, const float* coef, float* g, int B, int C, int F,
                            void* stream) {
    if (int rc = bg_check("basis_weight_l1_grad", B, C, F)) return rc;
    if (!D || !target || !g || g == D || g == target)
        return fail(FV_ERR_INVALID_ARG, "basis_weight_l1_grad: null tensor, or g aliases an input");
    const BasisL1Geom geo = basis_l1_geom(B, C, F);
    FV_KERNEL_LAUNCH(basis_l1_grad_kernel, dim3(geo.gx, geo.gy, geo.gz), dim3(kBhThreads), 0, (hipStream_t)stream, D,
                       target, coef, g, C, F, (float)geo.count);
    FV_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
