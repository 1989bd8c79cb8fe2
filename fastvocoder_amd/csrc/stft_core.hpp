// The windowed real FFT shared by mel.hip (the mel front end), griffin_lim.hip (the STFT / inverse STFT pair of
// Griffin-Lim) and stft_loss.hip (the STFT distance and magnitudes).  One wave per frame: an n_fft-point real FFT is an
// Nc = n_fft/2-point complex FFT of the even/odd sample pairs (z[m] = f[2m] + i f[2m+1]) plus the split step
//   X[k] = E + W^k O,  E = (Z[k] + conj Z[Nc-k]) / 2,  O = (Z[k] - conj Z[Nc-k]) / 2i,  W = exp(-2 pi i / n_fft).
// The complex FFT is Stockham radix-4 (256 = 4^4, 1024 = 4^5; one radix-2 pass last for 512), natural order out, each
// lane its butterflies in registers, the wave's NB buffers of Nc points exchanged in place through LDS between the
// passes.  Twiddles exp(-2 pi i t / Nc) and W^k come from the host in float64 rounded once.
// Every wave of the block must run the same passes: the passes synchronise with __syncthreads().
#pragma once
#include "fv_internal.h"

namespace fv {

constexpr int kMelNc = 1024;               // complex FFT size of mel and Griffin-Lim = n_fft / 2

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// forward radix-4 DFT of v[0..3] (exp(-2 pi i rk / 4)), Stockham output order
__device__ __forceinline__ void radix4(float2* v) {
    const float2 a0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y);
    const float2 a1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
    const float2 a2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y);
    const float2 a3 = make_float2(v[1].y - v[3].y, v[3].x - v[1].x);   // -i (v1 - v3)
    v[0] = make_float2(a0.x + a2.x, a0.y + a2.y);
    v[1] = make_float2(a1.x + a3.x, a1.y + a3.y);
    v[2] = make_float2(a0.x - a2.x, a0.y - a2.y);
    v[3] = make_float2(a1.x - a3.x, a1.y - a3.y);
}

// source index of padded position P in a row of n samples (numpy 'reflect' by half = n_fft/2; n >= half + 1 keeps one
// reflection in range on either side)
__device__ __forceinline__ int64_t reflect_index(int64_t n, int half, int64_t P) {
    int64_t q = P - half;
    if (q < 0) q = -q;
    if (q >= n) q = 2 * (n - 1) - q;
    return q;
}

// One wave's NB buffers z[s Nc .. (s+1) Nc): buffer s takes frame t[s] (t[s] < 0: zeros) of the wlen-tap window win,
// lpad taps from the frame's start, at hop.  Pass 1 (Ns = 1, no twiddles) gathers its inputs on the fly:
// z[m] = (w f)[2m] + i (w f)[2m+1], f[i] = fetch(s, t[s] hop + i) the sample at that padded position.
// Butterfly J = lane + 64 q of the wave is butterfly j of buffer s (one buffer: s = 0).
template <int Nc, int NB, typename Fetch>
__device__ __forceinline__ void gather_pass(float2* __restrict__ z, Fetch fetch, const int64_t* t,
                                            const float* __restrict__ win, int hop, int wlen, int lpad, int lane) {
    constexpr int Nq = Nc / 4, Q = NB * Nc / 256;   // butterflies per buffer; per lane over the wave's buffers
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int J = lane + 64 * q, s = NB == 1 ? 0 : J / Nq, j = NB == 1 ? J : J % Nq;
        float2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = j + Nq * r;
            const int i0 = 2 * m - lpad, i1 = i0 + 1;   // window taps of samples 2m, 2m + 1
            float2 e = make_float2(0.f, 0.f);
            if (t[s] >= 0) {
                const int64_t P = t[s] * hop + 2 * m;
                if (i0 >= 0 && i0 < wlen) e.x = win[i0] * fetch(s, P);
                if (i1 >= 0 && i1 < wlen) e.y = win[i1] * fetch(s, P + 1);
            }
            v[r] = e;
        }
        radix4(v);
#pragma unroll
        for (int r = 0; r < 4; ++r) z[s * Nc + 4 * j + r] = v[r];
    }
    __syncthreads();
}

// Stockham radix-4 pass with sub-transform size Ns: butterfly j reads z[j + Nc/4 r], writes
// z[(j/Ns)*4Ns + j%Ns + Ns r]; in place (every read of the pass before any write).  Ns = 1 has no twiddles.
template <int Nc, int NB, int Ns>
__device__ __forceinline__ void fft_pass4(float2* __restrict__ z, const float2* __restrict__ tw, int lane) {
    constexpr int Nq = Nc / 4, Q = NB * Nc / 256;
    float2 v[Q][4];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int J = lane + 64 * q, s = NB == 1 ? 0 : J / Nq, j = NB == 1 ? J : J % Nq;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[q][r] = z[s * Nc + j + Nq * r];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int J = lane + 64 * q, s = NB == 1 ? 0 : J / Nq, j = NB == 1 ? J : J % Nq;
        if (Ns > 1) {
            const int ti = (j % Ns) * (Nc / (4 * Ns));   // r * ti < Nc
#pragma unroll
            for (int r = 1; r < 4; ++r) v[q][r] = cmul(v[q][r], tw[r * ti]);
        }
        radix4(v[q]);
        const int d = (j / Ns) * Ns * 4 + (j % Ns);
#pragma unroll
        for (int r = 0; r < 4; ++r) z[s * Nc + d + Ns * r] = v[q][r];
    }
    __syncthreads();
}

// Stockham radix-2 pass (the last pass of Nc = 512 = 2 * 4^4)
template <int Nc, int NB, int Ns>
__device__ __forceinline__ void fft_pass2(float2* __restrict__ z, const float2* __restrict__ tw, int lane) {
    constexpr int Nh = Nc / 2, Q = NB * Nc / 128;
    float2 v[Q][2];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int J = lane + 64 * q, s = NB == 1 ? 0 : J / Nh, j = NB == 1 ? J : J % Nh;
        v[q][0] = z[s * Nc + j];
        v[q][1] = z[s * Nc + j + Nh];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int J = lane + 64 * q, s = NB == 1 ? 0 : J / Nh, j = NB == 1 ? J : J % Nh;
        const float2 b = cmul(v[q][1], tw[(j % Ns) * (Nc / (2 * Ns))]);
        const int d = (j / Ns) * Ns * 2 + (j % Ns);
        z[s * Nc + d] = make_float2(v[q][0].x + b.x, v[q][0].y + b.y);
        z[s * Nc + d + Ns] = make_float2(v[q][0].x - b.x, v[q][0].y - b.y);
    }
    __syncthreads();
}

// the passes after pass 1 (gather_pass, or fft_pass4<Nc, NB, 1> on a buffer already in LDS), natural order out
template <int Nc, int NB>
__device__ __forceinline__ void fft_rest(float2* __restrict__ z, const float2* __restrict__ tw, int lane) {
    fft_pass4<Nc, NB, 4>(z, tw, lane);
    fft_pass4<Nc, NB, 16>(z, tw, lane);
    fft_pass4<Nc, NB, 64>(z, tw, lane);
    if constexpr (Nc == 512) fft_pass2<Nc, NB, 256>(z, tw, lane);
    if constexpr (Nc == 1024) fft_pass4<Nc, NB, 256>(z, tw, lane);
}

struct BinPair {
    float2 k, m;   // X[k], X[Nc - k]
};

// split step for bin k < Nc of one buffer (sp = W^k): X[k] = E + W^k O and, from the same terms,
// X[Nc-k] = conj(E - W^k O).  The magnitudes, and bin Nc (Nyquist: Re Z[0] - Im Z[0]), are the callers'.
__device__ __forceinline__ BinPair split_bin(const float2* __restrict__ zb, int k, int Nc, float2 sp) {
    const float2 a = zb[k], c = zb[(Nc - k) & (Nc - 1)];
    const float2 e = make_float2(0.5f * (a.x + c.x), 0.5f * (a.y - c.y));    // (Z[k] + conj Z[N-k]) / 2
    const float2 o = make_float2(0.5f * (a.y + c.y), -0.5f * (a.x - c.x));   // (Z[k] - conj Z[N-k]) / 2i
    const float2 wo = cmul(sp, o);
    return BinPair{make_float2(e.x + wo.x, e.y + wo.y), make_float2(e.x - wo.x, -(e.y - wo.y))};
}

}  // namespace fv
