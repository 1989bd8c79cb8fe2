// The 1024-point complex FFT the 2048-point real transforms are built on (mel.hip: the mel front end;
// griffin_lim.hip: the STFT / inverse STFT pair of Griffin-Lim).  One wave per transform: Stockham radix-4
// (1024 = 4^5, five passes, natural order out), each lane four radix-4 butterflies in registers, the frame
// exchanged through its own 8 KB of LDS in place between the passes.  Twiddles exp(-2 pi i t / 1024) come from
// the host in float64 rounded once (FV_MEL_TAB_TWIDDLE).
// Every wave of the block must run the same passes: the passes synchronise with __syncthreads().
#pragma once
#include "fv_internal.h"

namespace fv {

constexpr int kMelNc = 1024;               // complex FFT size = n_fft / 2

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

// Stockham pass with sub-transform size Ns: butterfly j reads z[j + 256 r], writes z[(j/Ns)*4Ns + j%Ns + Ns r]
template <int Ns>
__device__ __forceinline__ void fft1024_pass(float2* __restrict__ z, const float2* __restrict__ tw, int lane) {
    float2 v[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = lane + 64 * q;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[q][r] = z[j + 256 * r];
    }
    __syncthreads();   // every read of the pass before any write (in place)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = lane + 64 * q;
        if (Ns > 1) {
            const int ti = (j % Ns) * (kMelNc / (4 * Ns));   // r * ti < 1024
#pragma unroll
            for (int r = 1; r < 4; ++r) v[q][r] = cmul(v[q][r], tw[r * ti]);
        }
        radix4(v[q]);
        const int d = (j / Ns) * Ns * 4 + (j % Ns);
#pragma unroll
        for (int r = 0; r < 4; ++r) z[d + Ns * r] = v[q][r];
    }
    __syncthreads();
}

}  // namespace fv
