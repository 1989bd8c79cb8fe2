// Multi-period discriminator kernels (reference: model/discriminator/mpd.py:131-164 DiscriminatorP;
// include/fastvocoder_hip.h fv_mpd_conv_first, fv_pack_period_conv, fv_period_conv).
//
// A map [B, C, H, p] is contiguous, as the reference keeps it: the flattened axis n = h p + c is the time axis, and
// Conv2d((5, 1), stride (3, 1), padding (2, 0)) reads, for the output (h', c), the input rows 3 h' + j - 2 of column c.
//
// mpd_first_kernel (1 -> 32 channels): VALU, straight from the raw waveform.  The reflect tail pad (flat index
// n >= T reads x[2 (T - 1) - n]) and the [H, p] view are address arithmetic; a thread owns one (h', c) and all 32
// channels, each summed j = 0..4 (one fmaf each), then + bias, then the activation.
//
// period_conv_kernel (32 -> 128, 128 -> 512, 512 -> 1024): implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32, an
// fmaf chain).  M = 128 output channels, N = 128 consecutive flattened outputs (h', c), K = Cin x 5 walked in chunks
// of 8 channels.  A block has 4 waves as 2 (M) x 2 (N), each with a 64 x 64 tile (2 x 2 fragments, 64 accumulators):
// one K step reads 2 A and 2 B words per lane for 4 MFMAs.
//   * Input.  The rows a tile needs, 3 h0 - 3 .. 3 h1 + 2 (h0, h1 the first and last output row of the tile), are one
//     contiguous span of the flattened input.  It is read coalesced and stored PHASE-MAJOR: row 3 h0 - 3 + 3 m + ph of
//     channel ci goes to xs[ci][ph][m p + c].  Tap j of output (h', c) is row 3 (h' - h0 + q) + ph with
//     j + 1 = 3 q + ph, so lane n reads xs[ci][ph][(n0 - h0 p) + n + q p]: the 32 lanes of a lane group read 32
//     consecutive words for every tap and every period (the flat layout 3 p h' + c collides for p = 3, 5, 7, 11:
//     e.g. p = 3 puts h' = 0, c = 0 and h' = 7, c = 1 in one bank).  Lanes 32..63 read the next channel, which is a
//     lane group of its own for ds_read_b32.
//   * Weights.  Packed once as [Cout / 128][Cin][5][128]: a chunk is 5120 contiguous floats, copied as float4; a lane
//     group reads 32 consecutive words.
//   * Order.  acc = 0; for ci pair (ci, ci + 1), for j = 0..4: one MFMA; then + bias, then the activation.  Nothing in
//     it depends on B, on the grid or on a switch.
#include "fv_internal.h"

namespace fv {

namespace {

typedef float mpd_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kFirstC = 32;                // channels of the first layer
constexpr int kPM = 128, kPN = 128;        // block tile: output channels x flattened outputs
constexpr int kPCK = 8;                    // input channels per K chunk
constexpr int kPT = 5;                     // taps
constexpr int kPThreads = 256;
constexpr int kPStr = 160;                 // words of one (channel, phase) line: (h1 - h0 + 2) p <= 128 + 3 * 11 - 2
constexpr int kPSpan = 3 * kPStr;          // flattened inputs staged per channel (an upper bound)
constexpr int kPIters = (kPSpan + kPThreads - 1) / kPThreads;

}  // namespace

// grid (ceil(Hout p / 256), B)
__global__ __launch_bounds__(256) void mpd_first_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y,
                                                        int64_t T, int H, int Hout, int p, float slope) {
    const int64_t Nout = (int64_t)Hout * p;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= Nout) return;
    const int b = blockIdx.y;
    const int h = (int)(n / p), c = (int)(n - (int64_t)h * p);
    const float* xr = x + (size_t)b * T;
    float xv[kPT];
#pragma unroll
    for (int j = 0; j < kPT; ++j) {
        const int r = 3 * h + j - 2;
        float v = 0.f;
        if (r >= 0 && r < H) {
            int64_t i = (int64_t)r * p + c;
            if (i >= T) i = 2 * (T - 1) - i;          // the reflect tail (n_pad < T is checked by the caller)
            v = xr[i];
        }
        xv[j] = v;
    }
    float* yr = y + (size_t)b * kFirstC * Nout + n;
#pragma unroll 4
    for (int co = 0; co < kFirstC; ++co) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < kPT; ++j) acc = fmaf(w[co * kPT + j], xv[j], acc);
        if (bias) acc += bias[co];
        yr[(size_t)co * Nout] = acc >= 0.f ? acc : acc * slope;
    }
}

// w [Cout, Cin, 5] -> packed [Cout / 128][Cin][5][128]
__global__ __launch_bounds__(256) void pack_period_conv_kernel(const float* __restrict__ w, float* __restrict__ packed,
                                                               int Cout, int Cin) {
    const int64_t total = (int64_t)Cout * Cin * kPT;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int m = (int)(i % kPM);
        const int64_t r = i / kPM;
        const int j = (int)(r % kPT);
        const int64_t r2 = r / kPT;
        const int ci = (int)(r2 % Cin), mt = (int)(r2 / Cin);
        packed[i] = w[((size_t)(mt * kPM + m) * Cin + ci) * kPT + j];
    }
}

// grid (ceil(Hout P / 128), Cout / 128, B)
template <int P>
__global__ __launch_bounds__(kPThreads) void period_conv_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ wp,
                                                                const float* __restrict__ bias, float* __restrict__ y,
                                                                int Cin, int Cout, int H, int Hout, float slope) {
    __shared__ __attribute__((aligned(16))) float xs[kPCK * 3 * kPStr];
    __shared__ __attribute__((aligned(16))) float ws[kPCK * kPT * kPM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lm = lane & 31, kq = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int b = blockIdx.z, mt = blockIdx.y;
    const int Nin = H * P, Nout = Hout * P;
    const int n0 = blockIdx.x * kPN;
    const int h0 = n0 / P;
    const int R0 = 3 * h0 - 3;                             // first staged input row

    // what this thread stages of every channel: flattened span element i = tid + 256 u -> (row, c) -> phase-major word
    int s_lds[kPIters], s_glb[kPIters];
#pragma unroll
    for (int u = 0; u < kPIters; ++u) {
        const int i = tid + u * kPThreads;
        const int rr = i / P, c = i - rr * P;
        const int m = rr / 3, ph = rr - 3 * m;
        const int word = m * P + c;
        const int r = R0 + rr;
        s_lds[u] = (i < kPSpan && word < kPStr) ? ph * kPStr + word : -1;
        s_glb[u] = (r >= 0 && r < H) ? r * P + c : -1;
    }

    mpd_f32x16 acc[2][2];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[f][g][e] = 0.f;

    const float* xb = x + (size_t)b * Cin * Nin;
    const float* a_base = ws + kq * (kPT * kPM) + wm * 64 + lm;
    const float* b_base = xs + kq * (3 * kPStr) + (n0 - h0 * P) + wn * 64 + lm;

    for (int ci0 = 0; ci0 < Cin; ci0 += kPCK) {
        __syncthreads();                                   // the previous chunk's reads are done
#pragma unroll
        for (int cl = 0; cl < kPCK; ++cl) {
            const float* xc = xb + (size_t)(ci0 + cl) * Nin;
#pragma unroll
            for (int u = 0; u < kPIters; ++u)
                if (s_lds[u] >= 0) xs[cl * 3 * kPStr + s_lds[u]] = s_glb[u] >= 0 ? xc[s_glb[u]] : 0.f;
        }
        const float4* wsrc = reinterpret_cast<const float4*>(wp + ((size_t)mt * Cin + ci0) * (kPT * kPM));
        float4* wdst = reinterpret_cast<float4*>(ws);
#pragma unroll
        for (int u = 0; u < kPCK * kPT * kPM / 4 / kPThreads; ++u) wdst[tid + u * kPThreads] = wsrc[tid + u * kPThreads];
        __syncthreads();
#pragma unroll
        for (int cp = 0; cp < kPCK / 2; ++cp) {
#pragma unroll
            for (int j = 0; j < kPT; ++j) {
                const int q = (j + 1) / 3, ph = (j + 1) % 3;
                const float* pa = a_base + (2 * cp * kPT + j) * kPM;
                const float* pb = b_base + (2 * cp * 3 + ph) * kPStr + q * P;
                const float a0 = pa[0], a1 = pa[32];
                const float b0 = pb[0], b1 = pb[32];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }

    // C/D map of the 32x32 fragment: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int f = 0; f < 2; ++f) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = mt * kPM + wm * 64 + f * 32 + (e & 3) + 8 * (e >> 2) + 4 * kq;
            const float bv = bias ? bias[co] : 0.f;
            float* yr = y + ((size_t)b * Cout + co) * Nout;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const int n = n0 + wn * 64 + g * 32 + lm;
                if (n < Nout) {
                    const float v = acc[f][g][e] + bv;
                    yr[n] = v >= 0.f ? v : v * slope;
                }
            }
        }
    }
}

}  // namespace fv

using namespace fv;

extern "C" {

int fv_mpd_conv_first(const float* x, const float* w, const float* bias, float* y, int B, int64_t T, int period,
                      float slope, void* stream) {
    if (!mpd_period_ok(period))
        return fail(FV_ERR_UNSUPPORTED, "mpd_conv_first: period %d (2, 3, 5, 7 or 11)", period);
    if (!x || !w || !y || y == x || B <= 0 || B > 65535 || T < 1)
        return fail(FV_ERR_INVALID_ARG, "mpd_conv_first: null tensor, aliasing, B=%d or T=%lld", B, (long long)T);
    const MpdView v = mpd_view(T, period);
    if (v.n_pad >= T)
        return fail(FV_ERR_INVALID_ARG, "mpd_conv_first: T=%lld is not longer than the reflect tail of %lld samples",
                    (long long)T, (long long)v.n_pad);
    if (T + v.n_pad >= (int64_t)1 << 31)
        return fail(FV_ERR_INVALID_ARG, "mpd_conv_first: T=%lld too long", (long long)T);
    const int64_t blocks = (v.H1 * period + 255) / 256;
    FV_KERNEL_LAUNCH(mpd_first_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, w,
                       bias, y, T, (int)v.H, (int)v.H1, period, slope);
    FV_HIP(hipGetLastError());
    return 0;
}

static int period_conv_shape(const char* what, int Cin, int Cout) {
    if ((Cin != 32 && Cin != 128 && Cin != 512) || (Cout != 128 && Cout != 512 && Cout != 1024))
        return fail(FV_ERR_UNSUPPORTED, "%s: Cin=%d Cout=%d (Cin 32, 128 or 512; Cout 128, 512 or 1024)", what, Cin,
                    Cout);
    return 0;
}

int64_t fv_packed_period_conv_floats(int Cout, int Cin) {
    if (period_conv_shape("packed_period_conv_floats", Cin, Cout)) return 0;
    return (int64_t)Cout * Cin * kPT;
}

int fv_pack_period_conv(const float* w, float* packed, int Cout, int Cin, void* stream) {
    if (int rc = period_conv_shape("pack_period_conv", Cin, Cout)) return rc;
    if (!w || !packed || w == packed) return fail(FV_ERR_INVALID_ARG, "pack_period_conv: null tensor or aliasing");
    const int64_t total = (int64_t)Cout * Cin * kPT;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    FV_KERNEL_LAUNCH(pack_period_conv_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, packed, Cout, Cin);
    FV_HIP(hipGetLastError());
    return 0;
}

int fv_period_conv(const float* x, const float* packed, const float* bias, float* y, int B, int Cin, int Cout, int H,
                   int period, float slope, void* stream) {
    if (!mpd_period_ok(period)) return fail(FV_ERR_UNSUPPORTED, "period_conv: period %d (2, 3, 5, 7 or 11)", period);
    if (int rc = period_conv_shape("period_conv", Cin, Cout)) return rc;
    if (!x || !packed || !y || y == x || y == packed || B <= 0 || B > 65535 || H < 1)
        return fail(FV_ERR_INVALID_ARG, "period_conv: null tensor, aliasing, B=%d or H=%d", B, H);
    if ((int64_t)H * period >= (int64_t)1 << 31)
        return fail(FV_ERR_INVALID_ARG, "period_conv: H=%d x period %d too long", H, period);
    const int Hout = (int)period_conv_rows(H);
    const dim3 grid((unsigned)(((int64_t)Hout * period + kPN - 1) / kPN), (unsigned)(Cout / kPM), (unsigned)B);
    const hipStream_t st = (hipStream_t)stream;
#define FV_PERIOD(P)                                                                                              \
    case P:                                                                                                       \
        FV_KERNEL_LAUNCH(period_conv_kernel<P>, grid, dim3(kPThreads), 0, st, x, packed, bias, y, Cin, Cout, H,   \
                           Hout, slope);                                                                          \
        break;
    switch (period) {
        FV_PERIOD(2) FV_PERIOD(3) FV_PERIOD(5) FV_PERIOD(7) FV_PERIOD(11)
    }
#undef FV_PERIOD
    FV_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
