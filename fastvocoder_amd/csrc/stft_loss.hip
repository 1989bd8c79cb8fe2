// Multi-resolution STFT distance (reference: model/loss/stft_loss.py:16-39 stft, :42-80 the spectral convergence and
// log-magnitude terms, :124-155 MultiResolutionSTFTLoss; include/fastvocoder_hip.h fv_stft_distance) and the
// magnitude helper alone (fv_stft_magnitude).
//
// torch.stft defaults: center=True with numpy 'reflect' padding by n_fft/2, the win_length window centred in n_fft,
// 1 + n / hop frames, bins 0..n_fft/2; mag = sqrt(max(re^2 + im^2, 1e-7)).
//
// One wave per frame, the windowed real FFT of stft_core.hpp with Nc = n_fft/2 = 256, 512 or 1024.
// In the distance kernel a wave transforms the same frame of x and of y side by side (two Nc-point buffers, the same
// instructions for both), so x == y gives |X| == |Y| bit for bit and both terms exactly 0.  The magnitudes stay in
// registers: each block reduces (|Y| - |X|)^2, |Y|^2 and |ln|Y| - ln|X|| over its frames and bins and writes the three
// float64 partials to the workspace; stft_sum_kernel then adds a (resolution, utterance)'s partials in a fixed order.
// No atomics: two identical calls give identical bits.  All resolutions of a call run in the one launch: blockIdx.x
// walks the resolutions' frame chunks one after another.
// Every table (FFT twiddles, split twiddles, window) comes from the host in float64 rounded once to fp32.
#include "stft_core.hpp"

namespace fv {

constexpr int kStftWaves = 4;                    // waves (= frames in flight) per block
constexpr int kStftThreads = 64 * kStftWaves;
constexpr int kStftLoop = 4;                     // frames per wave per block in the distance kernel
constexpr int kStftNcMax = 1024;                 // complex FFT size for n_fft = 2048

struct StftRes {
    const float* tab;     // FV_STFT_TAB_* layout
    int nfft, hop, win;
    int64_t T;            // frames = 1 + n / hop
    int64_t chunk0;       // first block (blockIdx.x) of this resolution
};
struct StftArgs {
    StftRes res[FV_STFT_MAX_RES];
    int R;
    int64_t chunks;       // blocks per utterance over all resolutions
};

// split step for bin k < Nc of one buffer (sp = W^k), then the clamped magnitude of the reference
__device__ __forceinline__ float stft_bin_mag(const float2* __restrict__ zb, int k, int Nc, float2 sp) {
    const float2 X = split_bin(zb, k, Nc, sp).k;
    const float re = X.x, im = X.y;
    return sqrtf(fmaxf(re * re + im * im, 1e-7f));
}

// bin Nc (Nyquist): Re Z[0] - Im Z[0]
__device__ __forceinline__ float stft_nyq_mag(const float2* __restrict__ zb) {
    const float re = zb[0].x - zb[0].y;
    return sqrtf(fmaxf(re * re, 1e-7f));
}

__device__ __forceinline__ double stft_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int Nc>
__device__ void stft_distance_block(const float* __restrict__ x, const float* __restrict__ y, const StftRes& rs,
                                    int64_t chunk, int64_t n, float2* zs, float2* tw, double* red, double* part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float2* __restrict__ twg = reinterpret_cast<const float2*>(rs.tab + FV_STFT_TAB_TWIDDLE(rs.nfft));
    const float2* __restrict__ spg = reinterpret_cast<const float2*>(rs.tab + FV_STFT_TAB_SPLIT(rs.nfft));
    const float* __restrict__ win = rs.tab + FV_STFT_TAB_WINDOW(rs.nfft);
    const int lpad = (rs.nfft - rs.win) / 2;
    for (int i = threadIdx.x; i < Nc; i += kStftThreads) tw[i] = twg[i];
    float2* z = zs + (size_t)wv * 2 * Nc;
    const float* src[2] = {x, y};
    const auto fetch = [&](int s, int64_t P) { return src[s][reflect_index(n, Nc, P)]; };   // half = n_fft / 2 = Nc
    double dsum = 0.0, rsum = 0.0, lsum = 0.0;
    __syncthreads();
    for (int f = 0; f < kStftLoop; ++f) {
        const int64_t tf = (chunk * kStftLoop + f) * kStftWaves + wv;
        const bool live = tf < rs.T;
        const int64_t t[2] = {live ? tf : -1, live ? tf : -1};
        gather_pass<Nc, 2>(z, fetch, t, win, rs.hop, rs.win, lpad, lane);
        fft_rest<Nc, 2>(z, tw, lane);
        if (live) {
            float sd = 0.f, sr = 0.f, sl = 0.f;
#pragma unroll
            for (int i = 0; i < Nc / 64; ++i) {
                const int k = lane + 64 * i;
                const float2 sp = spg[k];
                const float mx = stft_bin_mag(z, k, Nc, sp), my = stft_bin_mag(z + Nc, k, Nc, sp);
                const float d = my - mx;
                sd = fmaf(d, d, sd);
                sr = fmaf(my, my, sr);
                sl += fabsf(logf(my) - logf(mx));
            }
            if (lane == 0) {
                const float mx = stft_nyq_mag(z), my = stft_nyq_mag(z + Nc);
                const float d = my - mx;
                sd = fmaf(d, d, sd);
                sr = fmaf(my, my, sr);
                sl += fabsf(logf(my) - logf(mx));
            }
            dsum += sd;
            rsum += sr;
            lsum += sl;
        }
        __syncthreads();   // the next frame's gather overwrites z
    }
    dsum = stft_wave_sum(dsum);
    rsum = stft_wave_sum(rsum);
    lsum = stft_wave_sum(lsum);
    if (lane == 0) {
        red[3 * wv + 0] = dsum;
        red[3 * wv + 1] = rsum;
        red[3 * wv + 2] = lsum;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double acc = 0.0;
        for (int w = 0; w < kStftWaves; ++w) acc += red[3 * w + threadIdx.x];
        part[threadIdx.x] = acc;
    }
}

// grid (chunks over all resolutions, B): block (chunk, b) -> workspace[b][chunk][3] float64 partials
__global__ __launch_bounds__(kStftThreads) void stft_distance_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ y, StftArgs a,
                                                                     int64_t n, double* __restrict__ ws) {
    __shared__ float2 zs[kStftWaves * 2 * kStftNcMax];   // two Nc-point buffers per wave
    __shared__ float2 tw[kStftNcMax];
    __shared__ double red[3 * kStftWaves];
    const int64_t g = blockIdx.x;
    const int b = blockIdx.y;
    int r = 0;
    while (r + 1 < a.R && g >= a.res[r + 1].chunk0) ++r;
    const StftRes& rs = a.res[r];
    const int64_t chunk = g - rs.chunk0;
    double* part = ws + ((size_t)b * a.chunks + g) * 3;
    const float* xr = x + (size_t)b * n;
    const float* yr = y + (size_t)b * n;
    switch (rs.nfft) {
        case 512: stft_distance_block<256>(xr, yr, rs, chunk, n, zs, tw, red, part); break;
        case 1024: stft_distance_block<512>(xr, yr, rs, chunk, n, zs, tw, red, part); break;
        default: stft_distance_block<1024>(xr, yr, rs, chunk, n, zs, tw, red, part); break;
    }
}

// grid (R, B), one wave: out[r][b][c] = sum over the chunks of resolution r of workspace[b][chunk][c], in float64 and
// in a fixed order (lane-strided sums, then a fixed butterfly)
__global__ __launch_bounds__(64) void stft_sum_kernel(const double* __restrict__ ws, StftArgs a, int B,
                                                      double* __restrict__ out) {
    const int r = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int64_t c0 = a.res[r].chunk0, c1 = r + 1 < a.R ? a.res[r + 1].chunk0 : a.chunks;
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t c = c0 + lane; c < c1; c += 64) {
        const double* p = ws + ((size_t)b * a.chunks + c) * 3;
        s[0] += p[0];
        s[1] += p[1];
        s[2] += p[2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double v = stft_wave_sum(s[i]);
        if (lane == 0) out[((size_t)r * B + b) * 3 + i] = v;
    }
}

// magnitude mode: the two buffers of a wave hold frames t0 + 2 wv and t0 + 2 wv + 1 of one row;
// grid (ceil(T / 2 kStftWaves), B) -> mag [B, T, Nc + 1], or [B, Nc + 1, T] with BinsMajor (the discriminator's
// layout, mfd.py: the same arithmetic, only the store address differs)
template <int Nc, bool BinsMajor>
__device__ void stft_magnitude_block(const float* __restrict__ xr, float* __restrict__ mag, const float* tab,
                                     int64_t n, int hop, int wlen, int64_t T, float2* zs, float2* tw) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float2* __restrict__ twg = reinterpret_cast<const float2*>(tab + FV_STFT_TAB_TWIDDLE(2 * Nc));
    const float2* __restrict__ spg = reinterpret_cast<const float2*>(tab + FV_STFT_TAB_SPLIT(2 * Nc));
    const float* __restrict__ win = tab + FV_STFT_TAB_WINDOW(2 * Nc);
    const int lpad = (2 * Nc - wlen) / 2;
    for (int i = threadIdx.x; i < Nc; i += kStftThreads) tw[i] = twg[i];
    __syncthreads();
    float2* z = zs + (size_t)wv * 2 * Nc;
    const int64_t t0 = (int64_t)blockIdx.x * 2 * kStftWaves + 2 * wv;
    const float* src[2] = {xr, xr};
    const int64_t t[2] = {t0 < T ? t0 : -1, t0 + 1 < T ? t0 + 1 : -1};
    gather_pass<Nc, 2>(z, [&](int s, int64_t P) { return src[s][reflect_index(n, Nc, P)]; }, t, win, hop, wlen, lpad,
                       lane);
    fft_rest<Nc, 2>(z, tw, lane);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (t[s] < 0) continue;
        // element of bin k: row[k * kstride]
        float* row = BinsMajor ? mag + t[s] : mag + (size_t)t[s] * (Nc + 1);
        const size_t kstride = BinsMajor ? (size_t)T : 1;
#pragma unroll
        for (int i = 0; i < Nc / 64; ++i) {
            const int k = lane + 64 * i;
            row[k * kstride] = stft_bin_mag(z + s * Nc, k, Nc, spg[k]);
        }
        if (lane == 0) row[Nc * kstride] = stft_nyq_mag(z + s * Nc);
    }
}

template <bool BinsMajor>
__global__ __launch_bounds__(kStftThreads) void stft_magnitude_kernel(const float* __restrict__ x,
                                                                      float* __restrict__ mag,
                                                                      const float* __restrict__ tab, int64_t n,
                                                                      int nfft, int hop, int wlen, int64_t T) {
    __shared__ float2 zs[kStftWaves * 2 * kStftNcMax];
    __shared__ float2 tw[kStftNcMax];
    const int b = blockIdx.y;
    const float* xr = x + (size_t)b * n;
    float* mr = mag + (size_t)b * T * (nfft / 2 + 1);
    switch (nfft) {
        case 512: stft_magnitude_block<256, BinsMajor>(xr, mr, tab, n, hop, wlen, T, zs, tw); break;
        case 1024: stft_magnitude_block<512, BinsMajor>(xr, mr, tab, n, hop, wlen, T, zs, tw); break;
        default: stft_magnitude_block<1024, BinsMajor>(xr, mr, tab, n, hop, wlen, T, zs, tw); break;
    }
}

int64_t stft_chunks(int64_t n, int hop) {
    const int64_t T = 1 + n / hop;
    const int64_t per = (int64_t)kStftLoop * kStftWaves;
    return (T + per - 1) / per;
}

int launch_stft_distance(const float* x, const float* y, const float* const* tables, int B, int64_t n, int R,
                         const int* nfft, const int* hop, const int* win, double* out, double* ws, hipStream_t s) {
    StftArgs a{};
    a.R = R;
    int64_t c = 0;
    for (int r = 0; r < R; ++r) {
        a.res[r] = StftRes{tables[r], nfft[r], hop[r], win[r], 1 + n / hop[r], c};
        c += stft_chunks(n, hop[r]);
    }
    a.chunks = c;
    FV_KERNEL_LAUNCH(stft_distance_kernel, dim3((unsigned)c, (unsigned)B), dim3(kStftThreads), 0, s, x, y, a, n,
                       ws);
    FV_HIP(hipGetLastError());
    FV_KERNEL_LAUNCH(stft_sum_kernel, dim3((unsigned)R, (unsigned)B), dim3(64), 0, s, ws, a, B, out);
    FV_HIP(hipGetLastError());
    return 0;
}

int launch_stft_magnitude(const float* x, float* mag, const float* tab, int B, int64_t n, int nfft, int hop, int win,
                          hipStream_t s, bool bins_major) {
    const int64_t T = 1 + n / hop;
    const int64_t blocks = (T + 2 * kStftWaves - 1) / (2 * kStftWaves);
    if (bins_major)
        FV_KERNEL_LAUNCH(stft_magnitude_kernel<true>, dim3((unsigned)blocks, (unsigned)B), dim3(kStftThreads), 0, s,
                           x, mag, tab, n, nfft, hop, win, T);
    else
        FV_KERNEL_LAUNCH(stft_magnitude_kernel<false>, dim3((unsigned)blocks, (unsigned)B), dim3(kStftThreads), 0, s,
                           x, mag, tab, n, nfft, hop, win, T);
    FV_HIP(hipGetLastError());
    return 0;
}

}  // namespace fv
