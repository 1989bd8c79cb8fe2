// Gradient of the multi-resolution STFT distance with respect to the estimate x (include/fastvocoder_hip.h
// fv_stft_distance_grad; forward: stft_loss.hip).  With X, Y the clamped magnitudes of x and y and the caller's
// coefficients c_diff = dL/dS_diff, c_log = dL/dS_log per (resolution, row):
//   G = c_diff * -2 (Y - X) + c_log * -sign(Y - X) / X            (sign(ln Y - ln X) = sign(Y - X), sign(0) = 0)
//   C[k] = G (re + i im) / X  where re^2 + im^2 > 1e-7, else 0     (the clamp passes no gradient)
//   frame gradient f[i] = w[i] Re sum_{k=0..n_fft/2} C[k] exp(+2 pi i k i / n_fft)
// That sum is the adjoint of the one-sided real FFT: n_fft * irfft of the bins with the interior bins halved, i.e.
// the Hermitian spectrum H with H[k] = C[k] / 2 inside and H[0] = Re C[0], H[n_fft/2] = Re C[n_fft/2].  The merge
// step and packed inverse FFT of griffin_lim.hip compute conj(fft(conj Z(S))) = (1/2) sum_{k<n_fft} S[k] exp(+...),
// so they are fed S = 2 H: the interior bins as they are, DC and Nyquist doubled and real; no scale afterwards.
//
// stft_grad_frame_kernel: one wave per frame, the forward kernel's shape (stft_distance_kernel: two Nc-point buffers
// per wave, frame t of x and of y transformed side by side by the same instructions, so x == y gives X == Y bit for
// bit, G = 0 and a gradient of exactly 0).  The bin pair (k, Nc - k) is formed in registers from Z[k] and Z[Nc - k] of
// both buffers and merged back in place into the x buffer, which the inverse passes then transform alone; the
// frame's win_length windowed taps go to its slab frames[r][b][t][win_length] in the workspace.  Spectra and
// magnitudes never reach HBM.
// stft_grad_ola_kernel: overlap-add as a gather.  Sample i of row b sums, resolution after resolution, the taps of
// every frame that covers padded position i + n_fft/2 and then those of the (at most two) reflected positions that
// read sample i in the forward padding, frames in increasing order, and writes gx once.  No atomics: identical calls
// give identical bits, and a row's gradient does not depend on B or on the other rows.
#include "stft_core.hpp"

namespace fv {

constexpr int kSgWaves = 4;                      // waves (= frames in flight) per block
constexpr int kSgThreads = 64 * kSgWaves;
constexpr int kSgLoop = 4;                       // frames per wave per block
constexpr int kSgNcMax = 1024;                   // complex FFT size for n_fft = 2048

struct StftGradRes {
    const float* tab;     // FV_STFT_TAB_* layout
    int nfft, hop, win;
    int64_t T;            // frames = 1 + n / hop
    int64_t chunk0;       // first block (blockIdx.x) of this resolution
    int64_t slab;         // first float of this resolution's frames [B][T][win] in the workspace
};
struct StftGradArgs {
    StftGradRes res[FV_STFT_MAX_RES];
    int R;
};

// C = dL/d(re, im) of one bin from the bin of x and of y; dc: DC or Nyquist (real, counted once in the Hermitian sum)
__device__ __forceinline__ float2 stft_grad_bin(float2 X, float2 Y, float cd, float cl, bool dc) {
    const float px = X.x * X.x + X.y * X.y, py = Y.x * Y.x + Y.y * Y.y;
    const float mx = sqrtf(fmaxf(px, 1e-7f)), my = sqrtf(fmaxf(py, 1e-7f));
    const float d = my - mx;
    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    const float inv = 1.f / mx;
    const float G = -2.f * cd * d - cl * sg * inv;
    const float s = px > 1e-7f ? (dc ? 2.f : 1.f) * G * inv : 0.f;
    return make_float2(s * X.x, dc ? 0.f : s * X.y);
}

template <int Nc>
__device__ void stft_grad_block(const float* __restrict__ x, const float* __restrict__ y, const StftGradRes& rs,
                                int64_t chunk, int64_t n, float cd, float cl, float* __restrict__ frames,
                                float2* zs, float2* tw) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float2* __restrict__ twg = reinterpret_cast<const float2*>(rs.tab + FV_STFT_TAB_TWIDDLE(rs.nfft));
    const float2* __restrict__ spg = reinterpret_cast<const float2*>(rs.tab + FV_STFT_TAB_SPLIT(rs.nfft));
    const float* __restrict__ win = rs.tab + FV_STFT_TAB_WINDOW(rs.nfft);
    const int lpad = (rs.nfft - rs.win) / 2;
    for (int i = threadIdx.x; i < Nc; i += kSgThreads) tw[i] = twg[i];
    float2* z = zs + (size_t)wv * 2 * Nc;        // buffer 0: x, buffer 1: y
    const float* src[2] = {x, y};
    const auto fetch = [&](int s, int64_t P) { return src[s][reflect_index(n, Nc, P)]; };   // half = n_fft / 2 = Nc
    __syncthreads();
    for (int f = 0; f < kSgLoop; ++f) {
        const int64_t tf = (chunk * kSgLoop + f) * kSgWaves + wv;
        const bool live = tf < rs.T;             // a dead wave runs the passes (block-wide barriers) on zeros
        const int64_t t[2] = {live ? tf : -1, live ? tf : -1};
        gather_pass<Nc, 2>(z, fetch, t, win, rs.hop, rs.win, lpad, lane);
        fft_rest<Nc, 2>(z, tw, lane);
        // bin pairs (k, Nc - k), k = 0..Nc/2: k = lane + 64 i, and k = Nc/2 on lane 0.  In place: the pair reads
        // z[k] and z[Nc - k] of both buffers and writes those of the x buffer only.
#pragma unroll 1   // rolled: the pairs are independent, and unrolling costs registers past two blocks per CU
        for (int i = 0; i <= Nc / 128; ++i) {
            const int k = i < Nc / 128 ? lane + 64 * i : Nc / 2;
            if (i == Nc / 128 && lane != 0) break;
            const int kz = (Nc - k) & (Nc - 1);  // the partner bin's place in z (bin Nc, Nyquist, shares z[0])
            const float2 w = spg[k];
            const BinPair X = split_bin(z, k, Nc, w), Y = split_bin(z + Nc, k, Nc, w);
            const float2 ck = stft_grad_bin(X.k, Y.k, cd, cl, k == 0);
            // The partner bin as the forward kernels form it (split_bin(Nc - k).k, not this pair's .m, which rounds
            // differently), so that the clamp and sign decisions are those of fv_stft_magnitude's values bit for bit.
            // Nyquist (k = 0) is Re Z[0] - Im Z[0] either way; k = Nc/2 pairs with itself.
            float2 xm = X.m, ym = Y.m;
            if (k != 0 && 2 * k != Nc) {
                const float2 wm = spg[Nc - k];
                xm = split_bin(z, Nc - k, Nc, wm).k;
                ym = split_bin(z + Nc, Nc - k, Nc, wm).k;
            }
            const float2 cm = 2 * k == Nc ? ck : stft_grad_bin(xm, ym, cd, cl, k == 0);
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
        // g[2m] = Re conj(z[m]), g[2m+1] = Im conj(z[m]); tap i of the window sits at g[i + lpad]
        if (live) {
            float* __restrict__ fr = frames + (size_t)tf * rs.win;
            for (int i = lane; i < rs.win; i += 64) {
                const int j = i + lpad;
                const float2 v = z[j >> 1];
                fr[i] = win[i] * ((j & 1) ? -v.y : v.x);
            }
        }
        __syncthreads();   // the next frame's gather overwrites z
    }
}

// grid (chunks over all resolutions, B): block (chunk, b) -> kSgLoop * kSgWaves frames of one resolution of row b
__global__ __launch_bounds__(kSgThreads) void stft_grad_frame_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ y, StftGradArgs a,
                                                                     int64_t n, int B, const float* __restrict__ coef,
                                                                     float* __restrict__ ws) {
    __shared__ float2 zs[kSgWaves * 2 * kSgNcMax];   // two Nc-point buffers per wave
    __shared__ float2 tw[kSgNcMax];
    const int64_t g = blockIdx.x;
    const int b = blockIdx.y;
    int r = 0;
    while (r + 1 < a.R && g >= a.res[r + 1].chunk0) ++r;
    const StftGradRes& rs = a.res[r];
    const int64_t chunk = g - rs.chunk0;
    const float cd = coef[((size_t)r * B + b) * 2], cl = coef[((size_t)r * B + b) * 2 + 1];
    float* frames = ws + rs.slab + (size_t)b * rs.T * rs.win;
    const float* xr = x + (size_t)b * n;
    const float* yr = y + (size_t)b * n;
    switch (rs.nfft) {
        case 512: stft_grad_block<256>(xr, yr, rs, chunk, n, cd, cl, frames, zs, tw); break;
        case 1024: stft_grad_block<512>(xr, yr, rs, chunk, n, cd, cl, frames, zs, tw); break;
        default: stft_grad_block<1024>(xr, yr, rs, chunk, n, cd, cl, frames, zs, tw); break;
    }
}

// the taps that the frames of one row and resolution hold for padded position P, frames in increasing order
__device__ __forceinline__ float stft_grad_position(const float* __restrict__ fb, int64_t P, int lpad, int hop,
                                                    int win, int64_t T) {
    const int64_t j = P - lpad;                  // relative to frame 0's first window tap
    if (j < 0) return 0.f;
    const int64_t thi = min(T - 1, j / hop);
    const int64_t tlo = j >= win ? (j - win) / hop + 1 : 0;
    float acc = 0.f;
    for (int64_t t = tlo; t <= thi; ++t) acc += fb[(size_t)t * win + (j - t * hop)];
    return acc;
}

// grid (ceil(n / 256), B): gx[b][i], one sample per thread
__global__ __launch_bounds__(256) void stft_grad_ola_kernel(const float* __restrict__ ws, StftGradArgs a, int64_t n,
                                                             float* __restrict__ gx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = blockIdx.y;
    float acc = 0.f;
    for (int r = 0; r < a.R; ++r) {
        const StftGradRes& rs = a.res[r];
        const int half = rs.nfft / 2, lpad = (rs.nfft - rs.win) / 2;
        const float* __restrict__ fb = ws + rs.slab + (size_t)b * rs.T * rs.win;
        acc += stft_grad_position(fb, i + half, lpad, rs.hop, rs.win, rs.T);
        // reflect_index(n, half, P) == i: on the left P = half - i (i = 1..half), on the right
        // P = half + 2 (n - 1) - i (i = n - 1 - half .. n - 2)
        if (i >= 1 && i <= half) acc += stft_grad_position(fb, half - i, lpad, rs.hop, rs.win, rs.T);
        if (i <= n - 2 && i >= n - 1 - half)
            acc += stft_grad_position(fb, half + 2 * (n - 1) - i, lpad, rs.hop, rs.win, rs.T);
    }
    gx[(size_t)b * n + i] = acc;
}

int64_t stft_grad_chunks(int64_t n, int hop) {
    const int64_t T = 1 + n / hop;
    const int64_t per = (int64_t)kSgLoop * kSgWaves;
    return (T + per - 1) / per;
}

int launch_stft_distance_grad(const float* x, const float* y, const float* const* tables, int B, int64_t n, int R,
                              const int* nfft, const int* hop, const int* win, const float* coef, float* gx,
                              float* ws, hipStream_t s) {
    StftGradArgs a{};
    a.R = R;
    int64_t c = 0, slab = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t T = 1 + n / hop[r];
        a.res[r] = StftGradRes{tables[r], nfft[r], hop[r], win[r], T, c, slab};
        c += stft_grad_chunks(n, hop[r]);
        slab += (int64_t)B * T * win[r];
    }
    FV_KERNEL_LAUNCH(stft_grad_frame_kernel, dim3((unsigned)c, (unsigned)B), dim3(kSgThreads), 0, s, x, y, a, n, B,
                       coef, ws);
    FV_HIP(hipGetLastError());
    FV_KERNEL_LAUNCH(stft_grad_ola_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, s,
                       (const float*)ws, a, n, gx);
    FV_HIP(hipGetLastError());
    return 0;
}

// the gather alone over one resolution's frames ws[B][T][win] (stft_mag_grad.hip): R = 1, slab 0
int launch_stft_grad_ola(const float* ws, const float* tab, int B, int64_t n, int nfft, int hop, int win, float* gx,
                         hipStream_t s) {
    StftGradArgs a{};
    a.R = 1;
    a.res[0] = StftGradRes{tab, nfft, hop, win, 1 + n / hop, 0, 0};
    FV_KERNEL_LAUNCH(stft_grad_ola_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, s, ws, a, n,
                       gx);
    FV_HIP(hipGetLastError());
    return 0;
}

}  // namespace fv
