// Discriminator kernels (reference: model/discriminator/msd.py, mfd.py; bin/train.py:97-117, 157-169 the scores;
// include/fastvocoder_hip.h fv_grouped_conv1d, fv_avg_pool1d, fv_disc_score_sums).
//
// grouped_conv_kernel: Conv1d(Cin, Cout, k, stride s, zero pad, groups = Cin / 4) + bias + leaky ReLU, exact fp32 on
// the VALU.  On gfx950 an fp32 MFMA runs at the fp32 VALU rate (MI355X_MICROARCH.md), and a group's GEMM is tiny
// (K = 4 k, M = Cout / groups <= 16 here), so the kernel is a register-blocked VALU loop: a block owns one (row,
// group, chunk of OCB output channels) and kDiscTT output times; the group's 4 input channels over the block's
// receptive field are staged in LDS once, PHASE-MAJOR (position P = m s + p at xs[ci][p][m]), so that the 64 lanes
// of a wave, which own consecutive output times, read consecutive words for every tap (no bank conflicts at any
// stride); the weights sit in LDS as [ci][j][oc] and every lane reads the same word (a broadcast).  Each thread keeps
// kDiscTPT x OCB accumulators, summed in the fixed order ci = 0..3, j = 0..k-1 (one fmaf each), then + bias, then
// the activation: a row's result never depends on B or on the other rows.
//
// avg_pool_kernel: AvgPool1d(k, s, p, count_include_pad=False, ceil_mode=False): the fp32 sum of the window's real
// samples in order, divided by their count.
//
// score_sums_kernel / score_combine_kernel: for M (estimate e, real r) map pairs, per map and row, the float64 sums
// sum |e - r|, sum (e - 1)^2, sum e^2, sum (r - 1)^2.  One launch covers every map (blockIdx.x walks the maps' chunks
// one after another); each block writes four float64 partials, and the combine launch adds a (map, row)'s partials
// in a fixed order.  No atomics: identical calls give identical bits.
#include "fv_internal.h"

namespace fv {

constexpr int kDiscThreads = 256;
constexpr int kDiscTPT = 2;                          // output times per thread (strided by the block)
constexpr int kDiscTT = kDiscThreads * kDiscTPT;     // output times per block

template <int OCB>
__global__ __launch_bounds__(kDiscThreads) void grouped_conv_kernel(const float* __restrict__ x,
                                                                    const float* __restrict__ w,
                                                                    const float* __restrict__ bias,
                                                                    float* __restrict__ y, int Cin, int Cout, int Tin,
                                                                    int Tout, int k, int s, int pad, float slope) {
    extern __shared__ float lds[];
    const int G = Cin / 4, opg = Cout / G, chunks = (opg + OCB - 1) / OCB;
    const int g = blockIdx.y / chunks, oc0 = (blockIdx.y % chunks) * OCB;
    const int b = blockIdx.z;
    const int t0 = blockIdx.x * kDiscTT;
    const int M = kDiscTT + (k - 1) / s + 1;         // phase columns a block reads
    float* xs = lds;                                 // [4][s][M]
    float* ws = lds + 4 * s * M;                     // [4][k][OCB]
    const float* xr = x + ((size_t)b * Cin + 4 * g) * Tin;
    const int64_t P0 = (int64_t)t0 * s - pad;
    for (int i = threadIdx.x; i < 4 * s * M; i += kDiscThreads) {
        const int ci = i / (s * M), rem = i % (s * M), m = rem / s, p = rem % s;   // (consecutive i: consecutive P)
        const int64_t P = P0 + (int64_t)m * s + p;
        xs[(ci * s + p) * M + m] = (P >= 0 && P < Tin) ? xr[(size_t)ci * Tin + P] : 0.f;
    }
    for (int i = threadIdx.x; i < 4 * k * OCB; i += kDiscThreads) {
        const int oc = i % OCB, cj = i / OCB, ci = cj / k, j = cj % k;
        const int co = oc0 + oc;
        ws[i] = co < opg ? w[((size_t)(g * opg + co) * 4 + ci) * k + j] : 0.f;
    }
    __syncthreads();
    float acc[kDiscTPT][OCB];
#pragma unroll
    for (int u = 0; u < kDiscTPT; ++u)
#pragma unroll
        for (int o = 0; o < OCB; ++o) acc[u][o] = 0.f;
    for (int ci = 0; ci < 4; ++ci) {
        int p = 0, q = 0;                            // j = q s + p
        for (int j = 0; j < k; ++j) {
            const float* xc = xs + (ci * s + p) * M + q + threadIdx.x;
            const float4* wc = reinterpret_cast<const float4*>(ws + (ci * k + j) * OCB);
            float xv[kDiscTPT];
#pragma unroll
            for (int u = 0; u < kDiscTPT; ++u) xv[u] = xc[u * kDiscThreads];
#pragma unroll
            for (int o4 = 0; o4 < OCB / 4; ++o4) {
                const float4 wv = wc[o4];
#pragma unroll
                for (int u = 0; u < kDiscTPT; ++u) {
                    acc[u][4 * o4 + 0] = fmaf(wv.x, xv[u], acc[u][4 * o4 + 0]);
                    acc[u][4 * o4 + 1] = fmaf(wv.y, xv[u], acc[u][4 * o4 + 1]);
                    acc[u][4 * o4 + 2] = fmaf(wv.z, xv[u], acc[u][4 * o4 + 2]);
                    acc[u][4 * o4 + 3] = fmaf(wv.w, xv[u], acc[u][4 * o4 + 3]);
                }
            }
            if (++p == s) { p = 0; ++q; }
        }
    }
#pragma unroll
    for (int u = 0; u < kDiscTPT; ++u) {
        const int t = t0 + threadIdx.x + u * kDiscThreads;
        if (t >= Tout) continue;
#pragma unroll
        for (int o = 0; o < OCB; ++o) {
            const int co = oc0 + o;
            if (co >= opg) break;
            const int c = g * opg + co;
            float v = acc[u][o];
            if (bias) v += bias[c];
            v = v >= 0.f ? v : v * slope;
            y[((size_t)b * Cout + c) * Tout + t] = v;
        }
    }
}

size_t grouped_conv_lds_bytes(int k, int s, int ocb) {
    const int M = kDiscTT + (k - 1) / s + 1;
    return sizeof(float) * ((size_t)4 * s * M + (size_t)4 * k * ocb);
}

int launch_grouped_conv1d(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout,
                          int Tin, int Tout, int k, int s, int pad, float slope, hipStream_t st) {
    const int G = Cin / 4, opg = Cout / G;
    const int ocb = opg % 16 == 0 ? 16 : 4;
    const int chunks = (opg + ocb - 1) / ocb;
    const dim3 grid((unsigned)((Tout + kDiscTT - 1) / kDiscTT), (unsigned)(G * chunks), (unsigned)B);
    const size_t lds = grouped_conv_lds_bytes(k, s, ocb);
    if (ocb == 16)
        FV_KERNEL_LAUNCH(grouped_conv_kernel<16>, grid, dim3(kDiscThreads), lds, st, x, w, bias, y, Cin, Cout, Tin,
                           Tout, k, s, pad, slope);
    else
        FV_KERNEL_LAUNCH(grouped_conv_kernel<4>, grid, dim3(kDiscThreads), lds, st, x, w, bias, y, Cin, Cout, Tin,
                           Tout, k, s, pad, slope);
    FV_HIP(hipGetLastError());
    return 0;
}

// grid (ceil(Tout / 256), rows): y[row, t] = mean of x[row, t s - p .. t s - p + k) over the samples inside [0, Tin)
__global__ __launch_bounds__(256) void avg_pool_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t Tin,
                                                       int64_t Tout, int k, int s, int p) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= Tout) return;
    const float* xr = x + (size_t)blockIdx.y * Tin;
    int64_t a = t * s - p, e = a + k;
    if (a < 0) a = 0;
    if (e > Tin) e = Tin;
    float sum = 0.f;
    for (int64_t i = a; i < e; ++i) sum += xr[i];
    y[(size_t)blockIdx.y * Tout + t] = sum / (float)(e - a);
}

int launch_avg_pool1d(const float* x, float* y, int rows, int64_t Tin, int64_t Tout, int k, int s, int p,
                      hipStream_t st) {
    FV_KERNEL_LAUNCH(avg_pool_kernel, dim3((unsigned)((Tout + 255) / 256), (unsigned)rows), dim3(256), 0, st, x, y,
                       Tin, Tout, k, s, p);
    FV_HIP(hipGetLastError());
    return 0;
}

// ---- score sums ----
constexpr int kScoreThreads = 256;
constexpr int kScoreLoop = 16;                        // elements per thread per block
constexpr int64_t kScoreChunk = (int64_t)kScoreThreads * kScoreLoop;

struct ScoreMap {
    const float* e;
    const float* r;
    int64_t n;            // elements per row (C * T)
    int64_t chunk0;       // first block (blockIdx.x) of this map
};
struct ScoreArgs {
    ScoreMap map[FV_DISC_MAX_MAPS];
    int M;
    int64_t chunks;       // blocks per row over all maps
};

__device__ __forceinline__ double score_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (chunks over all maps, B): block (chunk, b) -> workspace[b][chunk][4] float64 partials
__global__ __launch_bounds__(kScoreThreads) void score_sums_kernel(ScoreArgs a, double* __restrict__ ws) {
    __shared__ double red[4 * kScoreThreads / 64];
    const int64_t g = blockIdx.x;
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int m = 0;
    while (m + 1 < a.M && g >= a.map[m + 1].chunk0) ++m;
    const ScoreMap& mp = a.map[m];
    const float* er = mp.e + (size_t)b * mp.n;
    const float* rr = mp.r + (size_t)b * mp.n;
    const int64_t i0 = (g - mp.chunk0) * kScoreChunk + threadIdx.x;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < kScoreLoop; ++u) {
        const int64_t i = i0 + (int64_t)u * kScoreThreads;
        if (i < mp.n) {
            const float e = er[i], r = rr[i];
            const float em = e - 1.f, rm = r - 1.f;
            s[0] += fabsf(e - r);
            s[1] = fmaf(em, em, s[1]);
            s[2] = fmaf(e, e, s[2]);
            s[3] = fmaf(rm, rm, s[3]);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double v = score_wave_sum((double)s[c]);
        if (lane == 0) red[4 * wv + c] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double acc = 0.0;
        for (int w = 0; w < kScoreThreads / 64; ++w) acc += red[4 * w + threadIdx.x];
        ws[((size_t)b * a.chunks + g) * 4 + threadIdx.x] = acc;
    }
}

// grid (M, B), one wave: out[m][b][c] = sum over the chunks of map m of workspace[b][chunk][c], in a fixed order
__global__ __launch_bounds__(64) void score_combine_kernel(const double* __restrict__ ws, ScoreArgs a, int B,
                                                           double* __restrict__ out) {
    const int m = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int64_t c0 = a.map[m].chunk0, c1 = m + 1 < a.M ? a.map[m + 1].chunk0 : a.chunks;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t c = c0 + lane; c < c1; c += 64) {
        const double* p = ws + ((size_t)b * a.chunks + c) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] += p[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double v = score_wave_sum(s[i]);
        if (lane == 0) out[((size_t)m * B + b) * 4 + i] = v;
    }
}

int64_t score_chunks(int M, const int64_t* n) {
    int64_t c = 0;
    for (int m = 0; m < M; ++m) c += (n[m] + kScoreChunk - 1) / kScoreChunk;
    return c;
}

int launch_disc_score_sums(const float* const* e, const float* const* r, const int64_t* n, int M, int B, double* out,
                           double* ws, hipStream_t st) {
    ScoreArgs a{};
    a.M = M;
    int64_t c = 0;
    for (int m = 0; m < M; ++m) {
        a.map[m] = ScoreMap{e[m], r[m], n[m], c};
        c += (n[m] + kScoreChunk - 1) / kScoreChunk;
    }
    a.chunks = c;
    FV_KERNEL_LAUNCH(score_sums_kernel, dim3((unsigned)c, (unsigned)B), dim3(kScoreThreads), 0, st, a, ws);
    FV_HIP(hipGetLastError());
    FV_KERNEL_LAUNCH(score_combine_kernel, dim3((unsigned)M, (unsigned)B), dim3(64), 0, st, ws, a, B, out);
    FV_HIP(hipGetLastError());
    return 0;
}

}  // namespace fv
