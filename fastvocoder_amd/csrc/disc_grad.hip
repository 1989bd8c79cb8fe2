// Input gradient of the multi-scale discriminator (reference: model/discriminator/msd.py; bin/train.py:97-117 the
// adversarial and feature-map terms; include/fastvocoder_hip.h fv_grouped_conv1d_input_grad, fv_disc_map_grad,
// fv_reflect_pad_fold, fv_avg_pool1d_input_grad, fv_disc_score_grad).  Exact fp32, no atomics: every result element is
// summed by one thread in one fixed order, so identical calls give identical bits and a row never depends on B.
//
// grouped_input_grad_kernel: the data gradient of grouped_conv_kernel (disc.hip), evaluated POLYPHASE.  With the padded
// position P = i + pad = q s + p, input sample i meets only the taps j = p + m s and the output times t = q - m, so a
// phase costs ceil((k - p) / s) taps instead of k.  A block owns one (row, group) and QT = blockDim.x * kGradU values
// of q; for each phase p in turn a thread keeps 4 (input channels) x kGradU accumulators.  The group's incoming
// gradient over the block's range of t sits in LDS as gs[oc][t] -- the 64 lanes of a wave own consecutive q and read
// consecutive words for every tap -- and the weights as ws[oc][j][ci], one float4 that every lane reads (a broadcast).
// The sum runs oc ascending, then j ascending (m ascending), one fmaf each.  Groups with more output channels than the
// LDS holds at once are staged in chunks of `occ` channels, in the same order.  The staging applies the leaky-ReLU
// mask of the layer that produced the gradient (map_grad of fv_internal.h), so the masked [B, Cout, Tout] gradient never exists
// in memory.  Times outside [0, Tout) are staged as 0: input positions past the last window come out as exactly 0.
//
// map_grad_kernel: g_pre = (g_up + g_map) * (y > 0 ? 1 : slope), elementwise.
// reflect_fold_kernel: the adjoint of ReflectionPad1d(P); avg_pool_grad_kernel: the adjoint of avg_pool_kernel, a
// gather over the at most ceil(k / s) windows that hold a sample; score_grad_kernel: d(score sums)/d(estimate maps)
// for every map in one launch (blockIdx.x walks the maps' chunks as in score_sums_kernel).
#include "fv_internal.h"

namespace fv {

constexpr int kGradU = 2;                            // values of q per thread (strided by the block)

__global__ __launch_bounds__(256) void grouped_input_grad_kernel(const float* __restrict__ g_up,
                                                                 const float* __restrict__ g_map,
                                                                 const float* __restrict__ y,
                                                                 const float* __restrict__ w, float* __restrict__ dx,
                                                                 int Cin, int Cout, int Tin, int Tout, int k, int s,
                                                                 int pad, float slope, int occ) {
    extern __shared__ float lds[];
    const int NT = blockDim.x, QT = NT * kGradU;
    const int G = Cin / 4, opg = Cout / G;
    const int g = blockIdx.y, b = blockIdx.z;
    const int q0 = blockIdx.x * QT;
    const int mmax = (k - 1) / s, ncols = QT + mmax; // column c of gs holds t = q0 - mmax + c
    float* ws = lds;                                 // [occ][k][4]
    float* gs = lds + (size_t)occ * k * 4;           // [occ][ncols]
    const bool resident = occ >= opg;                // the whole group is staged once, for every phase
    for (int p = 0; p < s; ++p) {
        float acc[4][kGradU];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci)
#pragma unroll
            for (int u = 0; u < kGradU; ++u) acc[ci][u] = 0.f;
        const int nm = p < k ? (k - p + s - 1) / s : 0;          // taps of this phase
        for (int c0 = 0; c0 < opg; c0 += occ) {
            const int no = opg - c0 < occ ? opg - c0 : occ;
            if (!resident || p == 0) {
                __syncthreads();                                 // (the previous chunk's readers are done)
                for (int i = threadIdx.x; i < no * k * 4; i += NT) {
                    const int ci = i & 3, oj = i >> 2, oc = oj / k, j = oj % k;
                    ws[i] = w[((size_t)(g * opg + c0 + oc) * 4 + ci) * k + j];
                }
                for (int i = threadIdx.x; i < no * ncols; i += NT) {
                    const int oc = i / ncols, c = i % ncols;
                    const int t = q0 - mmax + c;
                    gs[i] = (t >= 0 && t < Tout)
                                ? map_grad(g_up, g_map, y, ((size_t)b * Cout + g * opg + c0 + oc) * Tout + t, slope)
                                : 0.f;
                }
                __syncthreads();
            }
            for (int oc = 0; oc < no; ++oc) {
                const float* gr = gs + (size_t)oc * ncols + mmax + threadIdx.x;
                const float4* wr = reinterpret_cast<const float4*>(ws) + oc * k + p;
                for (int m = 0; m < nm; ++m) {
                    const float4 wv = wr[m * s];
#pragma unroll
                    for (int u = 0; u < kGradU; ++u) {
                        const float gv = gr[u * NT - m];
                        acc[0][u] = fmaf(wv.x, gv, acc[0][u]);
                        acc[1][u] = fmaf(wv.y, gv, acc[1][u]);
                        acc[2][u] = fmaf(wv.z, gv, acc[2][u]);
                        acc[3][u] = fmaf(wv.w, gv, acc[3][u]);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kGradU; ++u) {
            const int64_t i = (int64_t)(q0 + (int)threadIdx.x + u * NT) * s + p - pad;
            if (i < 0 || i >= Tin) continue;
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) dx[((size_t)b * Cin + 4 * g + ci) * Tin + i] = acc[ci][u];
        }
    }
}

// threads per block for nq values of q: short maps (the deep layers) get small blocks
static int grouped_input_grad_threads(int64_t nq) { return nq > 256 ? 256 : nq > 64 ? 128 : 64; }

// channels of a group staged at once: the largest of 16, 8, 4, 2, 1 that covers the group or fits 64 KiB
static int grouped_input_grad_occ(int opg, int k, int s, int threads) {
    const int ncols = threads * kGradU + (k - 1) / s;
    int occ = 16;
    while (occ > 1 && (occ / 2 >= opg || sizeof(float) * (size_t)occ * (4 * k + ncols) > 65536)) occ /= 2;
    return occ;
}

int launch_grouped_conv1d_input_grad(const float* g_up, const float* g_map, const float* y, const float* w, float* dx,
                                     int B, int Cin, int Cout, int Tin, int Tout, int k, int s, int pad, float slope,
                                     hipStream_t st) {
    const int G = Cin / 4, opg = Cout / G;
    const int64_t nq = ((int64_t)Tin - 1 + pad) / s + 1;                     // q of the last input sample, + 1
    const int threads = grouped_input_grad_threads(nq);
    const int occ = grouped_input_grad_occ(opg, k, s, threads);
    const int QT = threads * kGradU;
    const size_t lds = sizeof(float) * (size_t)occ * (4 * k + QT + (k - 1) / s);
    if (lds > 65536) return fail(FV_ERR_UNSUPPORTED, "grouped_conv1d_input_grad: k=%d exceeds a block's shared memory", k);
    const dim3 grid((unsigned)((nq + QT - 1) / QT), (unsigned)G, (unsigned)B);
    if (G > 65535) return fail(FV_ERR_UNSUPPORTED, "grouped_conv1d_input_grad: %d groups (65535 at most)", G);
    FV_KERNEL_LAUNCH(grouped_input_grad_kernel, grid, dim3(threads), lds, st, g_up, g_map, y, w, dx, Cin, Cout, Tin,
                       Tout, k, s, pad, slope, occ);
    FV_HIP(hipGetLastError());
    return 0;
}

// grid ceil(n / 256): g_pre[i] = (g_up[i] + g_map[i]) * (y[i] > 0 ? 1 : slope)
__global__ __launch_bounds__(256) void map_grad_kernel(const float* __restrict__ g_up, const float* __restrict__ g_map,
                                                       const float* __restrict__ y, float* __restrict__ g_pre,
                                                       int64_t n, float slope) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) g_pre[i] = map_grad(g_up, g_map, y, (size_t)i, slope);
}

int launch_disc_map_grad(const float* g_up, const float* g_map, const float* y, float* g_pre, int64_t n, float slope,
                         hipStream_t st) {
    FV_KERNEL_LAUNCH(map_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g_up, g_map, y, g_pre, n,
                       slope);
    FV_HIP(hipGetLastError());
    return 0;
}

// grid (ceil(T / 256), rows): dx[row, i] = gp[i + P] + the left mirror image (1 <= i <= P) + the right one
// (T - 1 - P <= i <= T - 2), in that order
__global__ __launch_bounds__(256) void reflect_fold_kernel(const float* __restrict__ gp, float* __restrict__ dx,
                                                           int64_t T, int P) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const float* r = gp + (size_t)blockIdx.y * (T + 2 * (int64_t)P);
    float v = r[i + P];
    if (i >= 1 && i <= P) v += r[P - i];
    if (i >= T - 1 - P && i <= T - 2) v += r[P + 2 * (T - 1) - i];
    dx[(size_t)blockIdx.y * T + i] = v;
}

int launch_reflect_pad_fold(const float* gp, float* dx, int rows, int64_t T, int P, hipStream_t st) {
    FV_KERNEL_LAUNCH(reflect_fold_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)rows), dim3(256), 0, st, gp, dx,
                       T, P);
    FV_HIP(hipGetLastError());
    return 0;
}

// grid (ceil(Tin / 256), rows): dx[row, i] = sum over the windows t that hold i, ascending, of g[row, t] / count(t)
__global__ __launch_bounds__(256) void avg_pool_grad_kernel(const float* __restrict__ g, float* __restrict__ dx,
                                                            int64_t Tin, int64_t Tout, int k, int s, int p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Tin) return;
    const float* gr = g + (size_t)blockIdx.y * Tout;
    int64_t lo = i + p - k + 1;                      // t s - p + k > i
    lo = lo <= 0 ? 0 : (lo + s - 1) / s;
    int64_t hi = (i + p) / s;                        // t s - p <= i
    if (hi > Tout - 1) hi = Tout - 1;
    float sum = 0.f;
    for (int64_t t = lo; t <= hi; ++t) {
        int64_t a = t * s - p, e = a + k;
        if (a < 0) a = 0;
        if (e > Tin) e = Tin;
        sum += gr[t] / (float)(e - a);
    }
    dx[(size_t)blockIdx.y * Tin + i] = sum;
}

int launch_avg_pool1d_input_grad(const float* g, float* dx, int rows, int64_t Tin, int64_t Tout, int k, int s, int p,
                                 hipStream_t st) {
    FV_KERNEL_LAUNCH(avg_pool_grad_kernel, dim3((unsigned)((Tin + 255) / 256), (unsigned)rows), dim3(256), 0, st, g,
                       dx, Tin, Tout, k, s, p);
    FV_HIP(hipGetLastError());
    return 0;
}

// ---- gradient of the score sums ----
constexpr int kScoreGradThreads = 256;
constexpr int kScoreGradLoop = 8;                     // elements per thread
constexpr int64_t kScoreGradChunk = (int64_t)kScoreGradThreads * kScoreGradLoop;

struct ScoreGradMap {
    const float* e;
    const float* r;
    float* g;             // NULL: the map is skipped
    int64_t n;            // elements per row
    int64_t chunk0;       // first block (blockIdx.x) of this map
    float c_l1, c_adv2, c_fake2;   // c_l1, 2 c_adv, 2 c_fake
};
struct ScoreGradArgs {
    ScoreGradMap map[FV_DISC_MAX_MAPS];
    int M;
};

// grid (chunks over all maps, B): g[b, i] = c_l1 sign(e - r) + 2 c_adv (e - 1) + 2 c_fake e
__global__ __launch_bounds__(kScoreGradThreads) void score_grad_kernel(ScoreGradArgs a) {
    const int64_t blk = blockIdx.x;
    int m = 0;
    while (m + 1 < a.M && blk >= a.map[m + 1].chunk0) ++m;
    const ScoreGradMap& mp = a.map[m];
    if (!mp.g) return;
    const size_t row = (size_t)blockIdx.y * mp.n;
    const int64_t i0 = (blk - mp.chunk0) * kScoreGradChunk + threadIdx.x;
#pragma unroll
    for (int u = 0; u < kScoreGradLoop; ++u) {
        const int64_t i = i0 + (int64_t)u * kScoreGradThreads;
        if (i < mp.n) {
            const float e = mp.e[row + i], d = e - mp.r[row + i];
            float v = mp.c_l1 * (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f);
            v = fmaf(mp.c_adv2, e - 1.f, v);
            v = fmaf(mp.c_fake2, e, v);
            mp.g[row + i] = v;
        }
    }
}

int64_t score_grad_chunks(int M, const int64_t* n) {
    int64_t c = 0;
    for (int m = 0; m < M; ++m) c += (n[m] + kScoreGradChunk - 1) / kScoreGradChunk;
    return c;
}

int launch_disc_score_grad(const float* const* e, const float* const* r, float* const* g, const int64_t* n,
                           const float* coef, int M, int B, hipStream_t st) {
    ScoreGradArgs a{};
    a.M = M;
    int64_t c = 0;
    for (int m = 0; m < M; ++m) {
        a.map[m] = ScoreGradMap{e[m], r[m], g[m], n[m], c, coef[3 * m], 2.f * coef[3 * m + 1], 2.f * coef[3 * m + 2]};
        c += (n[m] + kScoreGradChunk - 1) / kScoreGradChunk;
    }
    FV_KERNEL_LAUNCH(score_grad_kernel, dim3((unsigned)c, (unsigned)B), dim3(kScoreGradThreads), 0, st, a);
    FV_HIP(hipGetLastError());
    return 0;
}

}  // namespace fv
