// Input gradient of the multi-period discriminator's strided convs (reference: model/discriminator/mpd.py:131-164
// DiscriminatorP; bin/train.py:97-117 the adversarial and feature-map terms; include/fastvocoder_hip.h
// fv_period_conv_input_grad, fv_pack_period_conv_grad, fv_mpd_first_input_grad).  Exact fp32, no atomics: every
// result element is summed by one lane in one fixed order, so identical calls give identical bits and a row never
// depends on B or on the grid.
//
// period_grad_kernel: the data gradient of period_conv_kernel (mpd.hip), a strided transposed conv, evaluated POLYPHASE
// as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32, an fmaf chain).  Write the input row r as
// r + 2 = 3 m + ph.  Row r meets only the taps j = ph (output row m) and j = ph + 3 (output row m - 1): phase 0 has
// taps 0 and 3, phase 1 taps 1 and 4, phase 2 tap 2.  On the flattened axis n = m p + c of the gradient map
// [Hout, p] the two reads are n and n - p for every phase and every period.
//   * GEMM.  M = Cin (a block owns MT = min(Cin, 128) input channels), N = NT consecutive n (m-space positions; each
//     stands for the three input rows 3 m - 2 .. 3 m), K = Cout x the taps of a phase, walked in chunks of 8 output
//     channels.  A block has 4 waves.  Cin >= 128: 2 (M) x 2 (N) waves, each 64 x 32, NT = 64; Cin = 32: 1 x 4 waves,
//     each 32 x 32, NT = 128 (M is not padded).  A wave keeps one accumulator fragment per phase and M fragment
//     (3 x 2 x 16 or 3 x 16 registers); a channel pair costs 5 MFMAs per M fragment from 5 A words and 2 B words.
//   * Gradient tile.  gs[co][i] holds g_pre at n = n0 - p + i, i < NT + p (a p-word halo in front), staged flat and
//     coalesced; the staging applies (g_up + g_map) * (y > 0 ? 1 : slope) (map_grad of fv_internal.h), so the masked
//     gradient never exists in memory.  n < 0 and n >= Hout p are staged as 0: row m = -1 and rows past the last
//     output contribute nothing.  A lane group reads 32 consecutive words for either tap.
//   * Weights.  Packed once as [Cin / MT][Cout][5][MT] (fv_pack_period_conv_grad): a chunk is 8 x 5 x MT contiguous
//     floats, copied as float4; a lane group reads 32 consecutive words.
//   * Order.  acc[ph] = 0; for the pair (co, co + 1) ascending: tap ph, then tap ph + 3 (phases 0 and 1), one MFMA
//     each (co before co + 1 inside it).  Nothing depends on B, on the grid or on a switch.
//   * Stores.  Input row 3 m + ph - 2 of column c is flat word (3 (m - m0) + ph) p + c behind row 3 m0 - 2
//     (m0 = n0 / p): the three phases of a tile interleave into one contiguous span.  Per accumulator register the
//     block writes its rows into an LDS line at that word and reads the line back in order, so global stores are
//     consecutive.  Words of rows outside [0, H) and of positions that belong to the neighbouring tile are skipped;
//     every (r, c) with 0 <= r < H belongs to exactly one tile, so all of dx is written.
//
// mpd_first_grad_kernel: the gradient of mpd_first_kernel down to the waveform, VALU.  A thread owns one sample i and
// computes P(i), the gradient of the padded flat sample i, and, where the reflect tail mirrors onto i
// (T - 1 - n_pad <= i <= T - 2), P(2 (T - 1) - i), added in that order.  P(n) is summed co ascending, then the taps of
// n's phase ascending (one fmaf each).
#include "fv_internal.h"

namespace fv {

namespace {

typedef float mpdg_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kGFirstC = 32;               // channels of the first layer
constexpr int kGT = 5;                     // taps
constexpr int kGCK = 8;                    // output channels (K) per chunk
constexpr int kGThreads = 256;
constexpr int kGHalo = 11;                 // the largest period

}  // namespace

// w [Cout, Cin, 5] -> packed [Cin / MT][Cout][5][MT], MT = min(Cin, 128)
__global__ __launch_bounds__(256) void pack_period_conv_grad_kernel(const float* __restrict__ w,
                                                                    float* __restrict__ packed, int Cout, int Cin,
                                                                    int MT) {
    const int64_t total = (int64_t)Cout * Cin * kGT;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int m = (int)(i % MT);
        const int64_t r = i / MT;
        const int j = (int)(r % kGT);
        const int64_t r2 = r / kGT;
        const int co = (int)(r2 % Cout), mt = (int)(r2 / Cout);
        packed[i] = w[((size_t)co * Cin + mt * MT + m) * kGT + j];
    }
}

// grid (ceil(Mrows P / NT), Cin / MT, B), Mrows = (H + 1) / 3 + 1; WM waves along M with MF fragments each
template <int P, int WM, int MF>
__global__ __launch_bounds__(kGThreads) void period_grad_kernel(const float* __restrict__ g_up,
                                                                const float* __restrict__ g_map,
                                                                const float* __restrict__ y,
                                                                const float* __restrict__ wp, float* __restrict__ dx,
                                                                int Cin, int Cout, int H, int Hout, float slope) {
    constexpr int WN = 4 / WM;
    constexpr int MT = WM * MF * 32;                     // input channels of a block
    constexpr int NT = WN * 32;                          // m-space positions of a block
    constexpr int W = NT + P;                            // staged words of one gradient channel
    constexpr int kStr = NT + 16;                        // its line in LDS (>= NT + kGHalo)
    constexpr int kGIters = (kGCK * W + kGThreads - 1) / kGThreads;
    constexpr int kOutRows = WM * 2;                     // rows in flight per accumulator register
    constexpr int kOutW = 3 * (NT + 2 * P);              // words of an output line: 3 (m1 - m0 + 1) P at most
    constexpr int kOIters = (kOutW + kGThreads - 1) / kGThreads;
    static_assert(kStr >= NT + kGHalo, "a gradient line holds the tile and its halo");
    static_assert(kGCK * kGT * MT >= kOutRows * kOutW, "the output lines reuse the weight buffer");
    __shared__ __attribute__((aligned(16))) float gs[kGCK * kStr];
    __shared__ __attribute__((aligned(16))) float ws[kGCK * kGT * MT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lm = lane & 31, kq = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int b = blockIdx.z, mt = blockIdx.y;
    const int Nout = Hout * P;
    const int n0 = blockIdx.x * NT;
    const int m0 = n0 / P;

    // what this thread stages of every chunk: element e = tid + 256 u -> (channel, word)
    int s_lds[kGIters], s_cl[kGIters], s_n[kGIters];
#pragma unroll
    for (int u = 0; u < kGIters; ++u) {
        const int e = tid + u * kGThreads;
        const int cl = e / W, i = e - cl * W;
        const int n = n0 - P + i;
        s_lds[u] = e < kGCK * W ? cl * kStr + i : -1;
        s_cl[u] = cl;
        s_n[u] = (n >= 0 && n < Nout) ? n : -1;
    }

    mpdg_f32x16 acc[3][MF];
#pragma unroll
    for (int ph = 0; ph < 3; ++ph)
#pragma unroll
        for (int f = 0; f < MF; ++f)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ph][f][e] = 0.f;

    const size_t gb = (size_t)b * Cout * Nout;
    const float* a_base = ws + kq * (kGT * MT) + wm * (MF * 32) + lm;
    const float* b_base = gs + kq * kStr + P + wn * 32 + lm;

    for (int co0 = 0; co0 < Cout; co0 += kGCK) {
        __syncthreads();                                   // the previous chunk's reads are done
        const size_t cb = gb + (size_t)co0 * Nout;
#pragma unroll
        for (int u = 0; u < kGIters; ++u)
            if (s_lds[u] >= 0)
                gs[s_lds[u]] = s_n[u] >= 0 ? map_grad(g_up, g_map, y, cb + (size_t)s_cl[u] * Nout + s_n[u], slope)
                                           : 0.f;
        const float4* wsrc = reinterpret_cast<const float4*>(wp + ((size_t)mt * Cout + co0) * (kGT * MT));
        float4* wdst = reinterpret_cast<float4*>(ws);
#pragma unroll
        for (int u = 0; u < (kGCK * kGT * MT / 4 + kGThreads - 1) / kGThreads; ++u) {
            const int i = tid + u * kGThreads;
            if (i < kGCK * kGT * MT / 4) wdst[i] = wsrc[i];
        }
        __syncthreads();
#pragma unroll
        for (int cp = 0; cp < kGCK / 2; ++cp) {
            const float* pb = b_base + 2 * cp * kStr;
            const float g0 = pb[0], g1 = pb[-P];           // output rows m and m - 1
#pragma unroll
            for (int f = 0; f < MF; ++f) {
                const float* pa = a_base + 2 * cp * (kGT * MT) + f * 32;
                const float a0 = pa[0], a1 = pa[MT], a2 = pa[2 * MT], a3 = pa[3 * MT], a4 = pa[4 * MT];
                acc[0][f] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, g0, acc[0][f], 0, 0, 0);
                acc[1][f] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, g0, acc[1][f], 0, 0, 0);
                acc[2][f] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, g0, acc[2][f], 0, 0, 0);
                acc[0][f] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, g1, acc[0][f], 0, 0, 0);
                acc[1][f] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4, g1, acc[1][f], 0, 0, 0);
            }
        }
    }

    // ---- stores, through LDS lines os[row][word] (the weight buffer) ----
    float* os = ws;
    // this lane's column n: word of its phase-0 value in the line
    const int n = n0 + wn * 32 + lm;
    const int m = n / P, c = n - m * P;
    const int word0 = 3 * (m - m0) * P + c;
    // the words this thread reads back: word -> (row, phase, column) -> the position it came from
    const int64_t Nin = (int64_t)H * P;
    const int64_t base = ((int64_t)3 * m0 - 2) * P;        // flat input position of word 0
    bool o_ok[kOIters];
#pragma unroll
    for (int u = 0; u < kOIters; ++u) {
        const int word = tid + u * kGThreads;
        const int rr = word / P, cc = word - rr * P;
        const int nn = (m0 + rr / 3) * P + cc;             // the m-space position that owns the word
        const int64_t at = base + word;
        o_ok[u] = word < kOutW && nn >= n0 && nn < n0 + NT && at >= 0 && at < Nin;
    }
    float* dxb = dx + ((size_t)b * Cin + (size_t)mt * MT) * Nin;
#pragma unroll
    for (int f = 0; f < MF; ++f) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            __syncthreads();                               // the lines (or, first, the weights) are read
            float* line = os + (wm * 2 + kq) * kOutW + word0;
#pragma unroll
            for (int ph = 0; ph < 3; ++ph) line[ph * P] = acc[ph][f][e];
            __syncthreads();
#pragma unroll
            for (int row = 0; row < kOutRows; ++row) {
                const int ci = (row >> 1) * (MF * 32) + f * 32 + (e & 3) + 8 * (e >> 2) + 4 * (row & 1);
#pragma unroll
                for (int u = 0; u < kOIters; ++u)
                    if (o_ok[u]) dxb[(size_t)ci * Nin + base + tid + u * kGThreads] = os[row * kOutW + tid + u * kGThreads];
            }
        }
    }
}

// grid (ceil(T / 256), B): one thread per waveform sample
__global__ __launch_bounds__(256) void mpd_first_grad_kernel(const float* __restrict__ g_up,
                                                             const float* __restrict__ g_map,
                                                             const float* __restrict__ y, const float* __restrict__ w,
                                                             float* __restrict__ dx, int64_t T, int n_pad, int H1,
                                                             int p, float slope) {
    __shared__ float wsh[kGFirstC * kGT];
    if (threadIdx.x < kGFirstC * kGT) wsh[threadIdx.x] = w[threadIdx.x];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const int64_t N1 = (int64_t)H1 * p;
    const size_t gb = (size_t)blockIdx.y * kGFirstC * N1;
    const bool mirrored = i >= T - 1 - n_pad && i <= T - 2;
    float v = 0.f;
    for (int pass = 0; pass < (mirrored ? 2 : 1); ++pass) {
        const int64_t n = pass ? 2 * (T - 1) - i : i;
        const int r = (int)(n / p), c = (int)(n - (int64_t)r * p);
        const int m = (r + 2) / 3, ph = (r + 2) - 3 * m;
        const bool t0 = m < H1;                            // tap ph, output row m
        const bool t1 = ph < 2 && m >= 1 && m - 1 < H1;    // tap ph + 3, output row m - 1
        const size_t at0 = gb + (size_t)m * p + c, at1 = at0 - p;
        float acc = 0.f;
        for (int co = 0; co < kGFirstC; ++co) {
            if (t0) acc = fmaf(wsh[co * kGT + ph], map_grad(g_up, g_map, y, at0 + (size_t)co * N1, slope), acc);
            if (t1) acc = fmaf(wsh[co * kGT + ph + 3], map_grad(g_up, g_map, y, at1 + (size_t)co * N1, slope), acc);
        }
        v = pass ? v + acc : acc;
    }
    dx[(size_t)blockIdx.y * T + i] = v;
}

}  // namespace fv

using namespace fv;

extern "C" {

static int period_grad_shape(const char* what, int Cin, int Cout) {
    if (!((Cin == 32 && Cout == 128) || (Cin == 128 && Cout == 512) || (Cin == 512 && Cout == 1024)))
        return fail(FV_ERR_UNSUPPORTED, "%s: Cin=%d Cout=%d ((32, 128), (128, 512) or (512, 1024))", what, Cin, Cout);
    return 0;
}

int64_t fv_packed_period_conv_grad_floats(int Cout, int Cin) {
    if (period_grad_shape("packed_period_conv_grad_floats", Cin, Cout)) return 0;
    return (int64_t)Cout * Cin * kGT;
}

int fv_pack_period_conv_grad(const float* w, float* packed, int Cout, int Cin, void* stream) {
    if (int rc = period_grad_shape("pack_period_conv_grad", Cin, Cout)) return rc;
    if (!w || !packed || w == packed) return fail(FV_ERR_INVALID_ARG, "pack_period_conv_grad: null tensor or aliasing");
    const int64_t total = (int64_t)Cout * Cin * kGT;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    FV_KERNEL_LAUNCH(pack_period_conv_grad_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, packed, Cout,
                       Cin, Cin < 128 ? Cin : 128);
    FV_HIP(hipGetLastError());
    return 0;
}

int fv_period_conv_input_grad(const float* g_up, const float* g_map, const float* y, const float* packed, float* dx,
                              int B, int Cin, int Cout, int H, int period, float slope, void* stream) {
    if (!mpd_period_ok(period))
        return fail(FV_ERR_UNSUPPORTED, "period_conv_input_grad: period %d (2, 3, 5, 7 or 11)", period);
    if (int rc = period_grad_shape("period_conv_input_grad", Cin, Cout)) return rc;
    if ((!g_up && !g_map) || !packed || !dx || B <= 0 || B > 65535 || H < 1)
        return fail(FV_ERR_INVALID_ARG, "period_conv_input_grad: null tensor, B=%d or H=%d", B, H);
    if (!y && slope != 1.f)
        return fail(FV_ERR_INVALID_ARG, "period_conv_input_grad: slope=%g needs the layer's output y", slope);
    if (dx == g_up || dx == g_map || dx == y || dx == packed)
        return fail(FV_ERR_INVALID_ARG, "period_conv_input_grad: dx must not alias an input");
    if (((int64_t)H + 5) * period >= (int64_t)1 << 31)
        return fail(FV_ERR_INVALID_ARG, "period_conv_input_grad: H=%d x period %d too long", H, period);
    const int Hout = (int)period_conv_rows(H);
    const int64_t nm = ((int64_t)(H + 1) / 3 + 1) * period;      // m-space positions: r + 2 = 3 m + ph, r < H
    const hipStream_t st = (hipStream_t)stream;
    const bool narrow = Cin == 32;
    const int NT = narrow ? 128 : 64;
    const dim3 grid((unsigned)((nm + NT - 1) / NT), (unsigned)(narrow ? 1 : Cin / 128), (unsigned)B);
#define FV_PERIOD(P)                                                                                                \
    case P:                                                                                                         \
        if (narrow)                                                                                                 \
            FV_KERNEL_LAUNCH((period_grad_kernel<P, 1, 1>), grid, dim3(kGThreads), 0, st, g_up, g_map, y, packed,   \
                               dx, Cin, Cout, H, Hout, slope);                                                      \
        else                                                                                                        \
            FV_KERNEL_LAUNCH((period_grad_kernel<P, 2, 2>), grid, dim3(kGThreads), 0, st, g_up, g_map, y, packed,   \
                               dx, Cin, Cout, H, Hout, slope);                                                      \
        break;
    switch (period) {
        FV_PERIOD(2) FV_PERIOD(3) FV_PERIOD(5) FV_PERIOD(7) FV_PERIOD(11)
    }
#undef FV_PERIOD
    FV_HIP(hipGetLastError());
    return 0;
}

int fv_mpd_first_input_grad(const float* g_up, const float* g_map, const float* y0, const float* w, float* dx, int B,
                            int64_t T, int period, float slope, void* stream) {
    if (!mpd_period_ok(period))
        return fail(FV_ERR_UNSUPPORTED, "mpd_first_input_grad: period %d (2, 3, 5, 7 or 11)", period);
    if ((!g_up && !g_map) || !w || !dx || B <= 0 || B > 65535 || T < 1)
        return fail(FV_ERR_INVALID_ARG, "mpd_first_input_grad: null tensor, B=%d or T=%lld", B, (long long)T);
    if (!y0 && slope != 1.f)
        return fail(FV_ERR_INVALID_ARG, "mpd_first_input_grad: slope=%g needs the layer's output y0", slope);
    if (dx == g_up || dx == g_map || dx == y0 || dx == w)
        return fail(FV_ERR_INVALID_ARG, "mpd_first_input_grad: dx must not alias an input");
    const MpdView v = mpd_view(T, period);
    if (v.n_pad >= T)
        return fail(FV_ERR_INVALID_ARG, "mpd_first_input_grad: T=%lld is not longer than the reflect tail of %lld "
                    "samples", (long long)T, (long long)v.n_pad);
    if (T + v.n_pad >= (int64_t)1 << 31)
        return fail(FV_ERR_INVALID_ARG, "mpd_first_input_grad: T=%lld too long", (long long)T);
    FV_KERNEL_LAUNCH(mpd_first_grad_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, g_up, g_map, y0, w, dx, T, (int)v.n_pad, (int)v.H1, period, slope);
    FV_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
