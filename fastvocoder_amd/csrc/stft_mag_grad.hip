// Adjoint of the bins-major clamped STFT magnitude (include/fastvocoder_hip.h fv_stft_magnitude_bins_grad; forward:
// stft_loss.hip stft_magnitude_kernel<true>), the link between the STFT discriminators' conv stack and the signal.
// Given g = dL/dmag [B, Nc + 1, T] and x [B, n], per bin of frame t with (re, im) the spectrum of x:
//   C[k] = g[b, k, t] (re + i im) / sqrt(max(re^2 + im^2, 1e-7))  where re^2 + im^2 > 1e-7, else 0
// and then the adjoint stft_loss_grad.hip documents: f[i] = w[i] Re sum_k C[k] exp(+2 pi i k i / n_fft) through the
// merge step and the packed inverse FFT (interior bins as they are, DC and Nyquist doubled and real), the frame's
// win_length taps to the workspace, and stft_loss_grad.hip's overlap-add gather with R = 1.
//
// stft_mag_grad_frame_kernel<Nc>: one wave per frame, ONE Nc-point buffer per wave (the distance's gradient needs
// two: x and y), so a block of 8 waves holds what a block of 4 held there and still owns 16 consecutive frames,
// two per wave.  The spectrum comes from the same stft_core.hpp calls as the forward, so the clamp decisions are the
// forward's.  LDS is sized by Nc (one instantiation per n_fft), not by the largest.
//
// The g read is the one new access pattern: a wave needs g[b, k, t] for all k at ONE t, a stride of 4 T bytes between
// lanes.  The block's 16 frames are, per k, 64 contiguous bytes, so the block stages the tile [Nc + 1 bins][16
// frames] once, ahead of the frame loop, with lanes mapped (k, t) = (idx / 16, idx % 16): every wave instruction
// reads four 64-byte runs, and each byte of g is requested once per call.  The tile is kept transposed, gt[t][k]
// with a row stride of Nc + 2 floats: (Nc + 2) % 32 == 2 spreads the 32 lanes of a half-wave store (16 t x 2 k) over
// 32 banks, and the frame loop's reads (lanes over k at one t, and the partner bins Nc - k) are contiguous.
#include "stft_core.hpp"

namespace fv {

constexpr int kMgWaves = 8;                      // waves (= frames in flight) per block
constexpr int kMgThreads = 64 * kMgWaves;
constexpr int kMgLoop = 2;                       // frames per wave per block
constexpr int kMgFrames = kMgWaves * kMgLoop;    // 16 consecutive frames per block: 64-byte runs of g per bin

// C = dL/d(re, im) of one bin from the bin X of x and g = dL/dmag; dc: DC or Nyquist (real, doubled for the merge)
__device__ __forceinline__ float2 stft_mag_grad_bin(float2 X, float g, bool dc) {
    const float re = X.x, im = X.y;
    const float p = re * re + im * im;
    const float s = p > 1e-7f ? (dc ? 2.f : 1.f) * g / sqrtf(fmaxf(p, 1e-7f)) : 0.f;
    return make_float2(s * re, dc ? 0.f : s * im);
}

// grid (ceil(T / 16), B): block (chunk, b) -> frames chunk * 16 .. + 15 of row b, taps to ws[b][t][wlen]
template <int Nc>
__global__ __launch_bounds__(kMgThreads) void stft_mag_grad_frame_kernel(
    const float* __restrict__ x, const float* __restrict__ gmag, const float* __restrict__ tab, int64_t n, int hop,
    int wlen, int64_t T, float* __restrict__ ws) {
    constexpr int GS = Nc + 2;                   // row stride of the staged tile
    __shared__ float2 zs[kMgWaves * Nc];         // one Nc-point buffer per wave
    __shared__ float2 tw[Nc];
    __shared__ float gt[kMgFrames * GS];         // gt[t - t0][k], k = 0..Nc
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * kMgFrames;
    const float* __restrict__ xr = x + (size_t)b * n;
    const float* __restrict__ gb = gmag + (size_t)b * (Nc + 1) * T;
    float* __restrict__ frames = ws + (size_t)b * T * wlen;
    const float2* __restrict__ twg = reinterpret_cast<const float2*>(tab + FV_STFT_TAB_TWIDDLE(2 * Nc));
    const float2* __restrict__ spg = reinterpret_cast<const float2*>(tab + FV_STFT_TAB_SPLIT(2 * Nc));
    const float* __restrict__ win = tab + FV_STFT_TAB_WINDOW(2 * Nc);
    const int lpad = (2 * Nc - wlen) / 2;
    for (int i = threadIdx.x; i < Nc; i += kMgThreads) tw[i] = twg[i];
    for (int idx = threadIdx.x; idx < (Nc + 1) * kMgFrames; idx += kMgThreads) {
        const int k = idx / kMgFrames, tl = idx % kMgFrames;
        const int64_t t = t0 + tl;
        gt[tl * GS + k] = t < T ? gb[(size_t)k * T + t] : 0.f;
    }
    float2* z = zs + (size_t)wv * Nc;
    const auto fetch = [&](int, int64_t P) { return xr[reflect_index(n, Nc, P)]; };   // half = n_fft / 2 = Nc
    __syncthreads();
    for (int f = 0; f < kMgLoop; ++f) {
        const int tl = f * kMgWaves + wv;
        const int64_t tf = t0 + tl;
        const bool live = tf < T;                // a dead wave runs the passes (block-wide barriers) on zeros
        const int64_t t[1] = {live ? tf : -1};
        gather_pass<Nc, 1>(z, fetch, t, win, hop, wlen, lpad, lane);
        fft_rest<Nc, 1>(z, tw, lane);
        const float* __restrict__ g = gt + tl * GS;
        // bin pairs (k, Nc - k), k = 0..Nc/2: k = lane + 64 i, and k = Nc/2 on lane 0.  In place: the pair reads and
        // writes z[k] and z[Nc - k] only (stft_loss_grad.hip stft_grad_block, with one buffer).
#pragma unroll 1
        for (int i = 0; i <= Nc / 128; ++i) {
            const int k = i < Nc / 128 ? lane + 64 * i : Nc / 2;
            if (i == Nc / 128 && lane != 0) break;
            const int kz = (Nc - k) & (Nc - 1);  // the partner bin's place in z (bin Nc, Nyquist, shares z[0])
            const float2 w = spg[k];
            const BinPair X = split_bin(z, k, Nc, w);
            const float2 ck = stft_mag_grad_bin(X.k, g[k], k == 0);
            // the partner bin as the forward forms it (split_bin(Nc - k).k), so that the clamp decision is the
            // forward's bit for bit; Nyquist (k = 0) is Re Z[0] - Im Z[0] either way; k = Nc/2 pairs with itself
            float2 xm = X.m;
            if (k != 0 && 2 * k != Nc) xm = split_bin(z, Nc - k, Nc, spg[Nc - k]).k;
            const float2 cm = 2 * k == Nc ? ck : stft_mag_grad_bin(xm, g[Nc - k], k == 0);
            // merge (griffin_lim.hip): E = (S[k] + conj S[Nc-k]) / 2, O = conj(W^k) (S[k] - conj S[Nc-k]) / 2,
            // Z[k] = E + i O, Z[Nc-k] = conj E + i conj O; stored conjugated for the inverse transform
            const float2 e = make_float2(0.5f * (ck.x + cm.x), 0.5f * (ck.y - cm.y));
            const float2 d = make_float2(0.5f * (ck.x - cm.x), 0.5f * (ck.y + cm.y));
            const float2 o = cmul(make_float2(w.x, -w.y), d);
            z[k] = make_float2(e.x - o.y, -(e.y + o.x));
            z[kz] = make_float2(e.x + o.y, e.y - o.x);
        }
        __syncthreads();
        fft_pass4<Nc, 1, 1>(z, tw, lane);
        fft_rest<Nc, 1>(z, tw, lane);
        // g[2m] = Re conj(z[m]), g[2m+1] = Im conj(z[m]); tap i of the window sits at position i + lpad
        if (live) {
            float* __restrict__ fr = frames + (size_t)tf * wlen;
            for (int i = lane; i < wlen; i += 64) {
                const int j = i + lpad;
                const float2 v = z[j >> 1];
                fr[i] = win[i] * ((j & 1) ? -v.y : v.x);
            }
        }
        __syncthreads();   // the next frame's gather overwrites z
    }
}

int64_t stft_mag_grad_chunks(int64_t n, int hop) {
    const int64_t T = 1 + n / hop;
    return (T + kMgFrames - 1) / kMgFrames;
}

int launch_stft_magnitude_bins_grad(const float* x, const float* gmag, const float* tab, int B, int64_t n, int nfft,
                                    int hop, int win, float* gx, float* ws, hipStream_t s) {
    const int64_t T = 1 + n / hop;
    const dim3 grid((unsigned)stft_mag_grad_chunks(n, hop), (unsigned)B), block(kMgThreads);
    switch (nfft) {
        case 512: FV_KERNEL_LAUNCH(stft_mag_grad_frame_kernel<256>, grid, block, 0, s, x, gmag, tab, n, hop, win, T,
                                     ws); break;
        case 1024: FV_KERNEL_LAUNCH(stft_mag_grad_frame_kernel<512>, grid, block, 0, s, x, gmag, tab, n, hop, win,
                                      T, ws); break;
        default: FV_KERNEL_LAUNCH(stft_mag_grad_frame_kernel<1024>, grid, block, 0, s, x, gmag, tab, n, hop, win, T,
                                    ws); break;
    }
    FV_HIP(hipGetLastError());
    return launch_stft_grad_ola(ws, tab, B, n, nfft, hop, win, gx, s);
}

}  // namespace fv
