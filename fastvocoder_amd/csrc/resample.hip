// Rational-ratio resampling by band-limited interpolation (include/fastvocoder_hip.h fv_resample): the Kaiser-windowed
// sinc of resampy's kaiser_best, what librosa < 0.10's load(sr=...) runs in the reference's load_wav, as a polyphase FIR.
//
// With L = sr_out / g, M = sr_in / g, output j sits at input position j M / L = c + p / L (c, p = divmod(j M, L)) and is
//   y[j] = sum_{t < taps} tab[t][j mod L] * x[c - half + t],      taps = 2 half + 2,   x = 0 outside [0, n_in).
// The phase p depends on j mod L alone, so the host hands over L rows of taps coefficients (audio.py resample_tables),
// TAP-MAJOR: tab[t * L + r].  Consecutive lanes are consecutive outputs, hence consecutive r (mod L): a wave's read of
// tap t is one or two contiguous runs.  The table (up to 4 MB; two of the common rate pairs exceed the 160 KB of LDS)
// stays in global memory and is read through L1 / L2 -- a block of 256 outputs touches min(L, 256) of its rows.
//
// A block owns 256 consecutive outputs of one row.  Their input window, x[c0 - half .. c0 - half + win), c0 the block's
// first c, is staged in LDS once (zeros outside the row: those loads are predicated off), int16 PCM converted on the way
// (s / 32768, exact).  Then each thread runs ONE sequential fp32 FMA chain over its taps, t ascending: no atomics, no
// cross-lane reduction, so an output's bits depend on its input neighbourhood and its phase only -- not on the batch
// row, the block it fell in or the grid.
//
// Index width: j M passes 2^31 after 6.7 million outputs at M = 320 (five minutes at 22.05 kHz); the block's base
// (j0 M, c0, row offsets) is 64-bit, what a thread adds to it (threadIdx M + p0 < 2^28 + 2^20) fits 32 bits.
#include "fv_internal.h"

namespace fv {

constexpr int kRsBlock = 256;

__device__ inline float rs_sample(const float* p) { return *p; }
__device__ inline float rs_sample(const short* p) { return (float)*p * (1.f / 32768.f); }

template <typename T>
__global__ __launch_bounds__(kRsBlock) void resample_kernel(const T* __restrict__ x, const float* __restrict__ tab,
                                                            float* __restrict__ y, int64_t n_in, int64_t n_out, int L,
                                                            int M, int half, int win) {
    extern __shared__ float xs[];   // [win] the block's input window
    const int64_t j0 = (int64_t)blockIdx.x * kRsBlock;
    const int64_t a0 = j0 * M;
    const int64_t c0 = a0 / L;
    const unsigned p0 = (unsigned)(a0 - c0 * L);
    const unsigned r0 = (unsigned)(j0 % L);
    x += (size_t)blockIdx.y * (size_t)n_in;
    y += (size_t)blockIdx.y * (size_t)n_out;
    const int64_t w0 = c0 - half;
    for (int i = threadIdx.x; i < win; i += kRsBlock) {
        const int64_t g = w0 + i;
        xs[i] = (g >= 0 && g < n_in) ? rs_sample(x + g) : 0.f;
    }
    __syncthreads();
    const int64_t j = j0 + threadIdx.x;
    if (j >= n_out) return;
    // c - c0 <= (L - 1 + 255 M) / L, so the last tap read is xs[win - 1] at most (resample_window)
    const unsigned dc = (p0 + threadIdx.x * (unsigned)M) / (unsigned)L;
    const unsigned r = (r0 + threadIdx.x) % (unsigned)L;
    const float* xr = xs + dc;
    const float* hr = tab + r;
    const int taps = 2 * half + 2;
    float acc = 0.f;
    for (int t = 0; t < taps; ++t) acc = fmaf(hr[(size_t)t * L], xr[t], acc);
    y[j] = acc;
}

int launch_resample(const void* x, int format, float* y, const float* tab, int B, int64_t n_in, int64_t n_out, int L,
                    int M, int half, hipStream_t s) {
    const int win = (int)resample_window(L, M, half);   // <= FV_RESAMPLE_MAX_WINDOW (fv_resample)
    const dim3 grid((unsigned)((n_out + kRsBlock - 1) / kRsBlock), B);
    const size_t lds = (size_t)win * sizeof(float);
    if (format == FV_PCM_S16)
        FV_KERNEL_LAUNCH(resample_kernel<short>, grid, dim3(kRsBlock), lds, s, static_cast<const short*>(x), tab, y,
                           n_in, n_out, L, M, half, win);
    else
        FV_KERNEL_LAUNCH(resample_kernel<float>, grid, dim3(kRsBlock), lds, s, static_cast<const float*>(x), tab, y,
                           n_in, n_out, L, M, half, win);
    FV_HIP(hipGetLastError());
    return 0;
}

}  // namespace fv
