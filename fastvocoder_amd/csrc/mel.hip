// Mel-spectrogram front end (reference: data/audio.py:58-61 melspectrogram with hparams.py:4-15,
// librosa < 0.10 semantics; include/fastvocoder_hip.h fv_melspectrogram) in one launch:
// wav -> preemphasis -> reflect-padded, Hann-windowed frames -> |rFFT| -> Slaney mel filters -> dB, clip.
//
// One wave per frame, kMelFrames frames per block.  The 2048-point real FFT is stft_core.hpp's: a 1024-point complex
// FFT of the sample pairs in the frame's own 8 KB of LDS, whose first pass reads its inputs straight from x (frame
// gather, preemphasis and the reflect index mapping on the fly; only the 600 pairs under the window are non-zero), and
// the split step into bins 0..1024.  The magnitudes then overwrite the frame's LDS, and the block's 80 x kMelFrames
// (filter, frame) dot products run over the sparse filters; lanes that share a filter write kMelFrames consecutive
// frames of one [B, 80, T] row.
// Every table (window, twiddles, filters) comes from the host in float64 rounded once to fp32.
#include "stft_core.hpp"

namespace fv {

constexpr int kMelHop = 240, kMelWin = 1200, kMelLpad = 424, kMelHalf = 1024, kMelMels = 80;
constexpr int kMelFrames = 4;              // frames (= waves) per block
constexpr int kMelThreads = 64 * kMelFrames;

// preemphasised sample at padded position P (p = lfilter([1, -0.97], [1], x), then numpy 'reflect' by 1024)
__device__ __forceinline__ float mel_sample(const float* __restrict__ xr, int64_t n, int64_t P) {
    const int64_t q = reflect_index(n, kMelHalf, P);
    const float v = xr[q];
    return q > 0 ? fmaf(-0.97f, xr[q - 1], v) : v;
}

__global__ __launch_bounds__(kMelThreads) void mel_kernel(const float* __restrict__ x, float* __restrict__ mel,
                                                          const float* __restrict__ tab, int64_t n, int64_t T) {
    __shared__ float2 zs[kMelFrames][kMelNc];   // one frame per wave: complex FFT, then its magnitudes
    __shared__ float2 tw[kMelNc];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * kMelFrames;
    const int64_t t = t0 + wv;
    const float* __restrict__ xr = x + (size_t)b * n;
    const float* __restrict__ win = tab + FV_MEL_TAB_WINDOW;
    const float2* __restrict__ twg = reinterpret_cast<const float2*>(tab + FV_MEL_TAB_TWIDDLE);
    for (int i = threadIdx.x; i < kMelNc; i += kMelThreads) tw[i] = twg[i];
    float2* z = zs[wv];

    // pass 1 (Ns = 1, no twiddles) on the gathered frame: z[m] = (w f)[2m] + i (w f)[2m+1].  stft_core.hpp's
    // gather_pass<kMelNc, 1> with this geometry fixed at compile time: window and left pad are even, so one range test
    // covers a pair (the same values; the general per-tap form measured 0.8 % slower at B = 64, DESIGN.md "STFT core")
    {
        float2 v[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = lane + 64 * q + 256 * r;
                const int i0 = 2 * m - kMelLpad;   // window tap of sample 2m (even; the window length is even)
                float2 s = make_float2(0.f, 0.f);
                if (t < T && i0 >= 0 && i0 < kMelWin) {
                    const int64_t P = t * kMelHop + 2 * m;
                    s.x = win[i0] * mel_sample(xr, n, P);
                    s.y = win[i0 + 1] * mel_sample(xr, n, P + 1);
                }
                v[q][r] = s;
            }
            const int j = lane + 64 * q;
            radix4(v[q]);
#pragma unroll
            for (int r = 0; r < 4; ++r) z[4 * j + r] = v[q][r];
        }
        __syncthreads();
    }
    fft_rest<kMelNc, 1>(z, tw, lane);

    // split step: |X[k]| for k = lane + 64 i; X[1024] = Re Z[0] - Im Z[0]
    {
        const float2* __restrict__ sp = reinterpret_cast<const float2*>(tab + FV_MEL_TAB_SPLIT);
        float mag[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int k = lane + 64 * i;
            const float2 X = split_bin(z, k, kMelNc, sp[k]).k;
            const float re = X.x, im = X.y;
            mag[i] = sqrtf(fmaf(re, re, im * im));
        }
        const float nyq = fabsf(z[0].x - z[0].y);
        __syncthreads();
        float* mz = reinterpret_cast<float*>(z);
#pragma unroll
        for (int i = 0; i < 16; ++i) mz[lane + 64 * i] = mag[i];
        if (lane == 0) mz[kMelNc] = nyq;
        __syncthreads();
    }

    // mel filters, dB, normalise: task = (filter m, frame f), frames fastest so that a filter's lanes store
    // kMelFrames consecutive outputs of its row
    const float* __restrict__ heads = tab + FV_MEL_TAB_FILTERS;
    const float* __restrict__ wts = tab + FV_MEL_TAB_WEIGHTS;
    for (int task = threadIdx.x; task < kMelMels * kMelFrames; task += kMelThreads) {
        const int m = task / kMelFrames, f = task % kMelFrames;
        const int64_t tf = t0 + f;
        if (tf >= T) continue;
        const int start = (int)heads[3 * m], len = (int)heads[3 * m + 1], off = (int)heads[3 * m + 2];
        const float* mz = reinterpret_cast<const float*>(zs[f]) + start;
        const float* w = wts + off;
        float acc = 0.f;
        for (int i = 0; i < len; ++i) acc = fmaf(w[i], mz[i], acc);
        const float db = 20.f * log10f(fmaxf(1e-5f, acc)) - 20.f;           // _amp_to_db - ref_level_db
        const float v = fminf(fmaxf((db + 100.f) * 0.01f, 0.f), 1.f);        // _normalize
        mel[((size_t)b * kMelMels + m) * (size_t)T + tf] = v;
    }
}

int launch_melspectrogram(const float* x, float* mel, const float* tab, int B, int64_t n, hipStream_t s) {
    const int64_t T = 1 + n / kMelHop;
    const int64_t blocks = (T + kMelFrames - 1) / kMelFrames;
    FV_KERNEL_LAUNCH(mel_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(kMelThreads), 0, s, x, mel, tab, n, T);
    FV_HIP(hipGetLastError());
    return 0;
}

}  // namespace fv
