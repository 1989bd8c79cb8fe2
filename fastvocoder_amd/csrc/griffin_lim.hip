// Griffin-Lim (reference: data/audio.py:66-95,179-190 inv_mel_spectrogram with hparams.py as shipped, librosa < 0.10
// semantics; include/fastvocoder_hip.h fv_griffin_lim and friends): mel -> linear magnitude S -> 60 projections
// y = istft(S * exp(i angle(stft(y)))) -> inverse preemphasis.
//
// gl_frame_kernel: one wave per frame, kGlFrames frames per block, the frame resident in its own 8 KB of LDS from the
// gather to the windowed output.  A projection is ONE launch of it:
//   gather 1200 samples of y under the window (numpy 'reflect' index mapping) -> window -> 1024-point complex FFT of
//   the sample pairs (stft_core.hpp) -> split step to bins 0..1024 -> phase normalisation, times S[t, k] -> merge step
//   (the split step's inverse) -> inverse complex FFT -> window -> the frame's 1200 samples to frames[B, T, 1200].
// Split and merge work on the bin pair (k, 1024 - k), which depends on Z[k] and Z[1024 - k] alone, so the spectrum
// never leaves the lane's registers.  The inverse FFT is the forward one between two conjugations
// (ifft(Z) = conj(fft(conj Z)) / N: the same passes with the twiddles' conjugates), so both directions share one code path.
// The other modes are that kernel's halves: INIT / ISTFT start from a given spectrum, STFT stops after the split step.
//
// gl_ola_kernel: the overlap-add as a gather, deterministic by construction: sample n is the sum, in increasing frame
// order, of the at most five frames whose window covers it, divided by the same sum of the squared window taps
// (where that exceeds tiny(float32)).  No atomics; 1024 samples trimmed from each end are never formed.
//
// mel_to_linear_kernel: S = max(1e-10, pinv(mel_basis) @ 10^((clip(mel) 100 - 80) / 20))^power, frames-major; it runs
// once per call, so it accumulates the 80-term dot products (mixed signs, heavy cancellation near the floor) in
// float64.  inv_preemph_kernel: o[n] = y[n] + a o[n-1] as a blocked scan, the carry exact (never truncated).
#include <float.h>

#include "stft_core.hpp"

namespace fv {

constexpr int kGlHop = 240, kGlWin = 1200, kGlLpad = 424, kGlHalf = 1024, kGlBins = 1025;
constexpr int kGlFrames = 4;               // frames (= waves) per block
constexpr int kGlThreads = 64 * kGlFrames;

enum { GL_ISTFT = 0, GL_INIT = 1, GL_ITER = 2, GL_STFT = 3 };

// exp(i angle(v)), angle(0) = 0.  The components are scaled by a power of two first, so that neither the squares
// nor their sum leave the fp32 range.
__device__ __forceinline__ float2 gl_phasor(float2 v) {
    const float m = fmaxf(fabsf(v.x), fabsf(v.y));
    int e;
    (void)frexpf(m, &e);
    const float a = ldexpf(v.x, -e), b = ldexpf(v.y, -e);
    const float mag = sqrtf(fmaf(a, a, b * b));
    if (!(mag > 0.f) || !(mag < FLT_MAX)) return make_float2(1.f, 0.f);   // zero (or non-finite) bin: phase 1
    const float inv = 1.f / mag;
    return make_float2(a * inv, b * inv);
}

template <int MODE>
__global__ __launch_bounds__(kGlThreads) void gl_frame_kernel(const float* __restrict__ y, const float2* __restrict__ spec,
                                                              const float* __restrict__ S, float* __restrict__ frames,
                                                              float2* __restrict__ spec_out,
                                                              const float* __restrict__ tab, int64_t n, int T) {
    __shared__ float2 zs[kGlFrames][kMelNc];   // one frame per wave
    __shared__ float2 tw[kMelNc];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int t = blockIdx.x * kGlFrames + wv;
    const bool live = t < T;                   // a dead wave runs the passes (block-wide barriers) on zeros
    const size_t ft = (size_t)b * T + (live ? t : 0);
    const float* __restrict__ win = tab + FV_GL_TAB_WINDOW;
    const float2* __restrict__ twg = reinterpret_cast<const float2*>(tab + FV_GL_TAB_TWIDDLE);
    const float2* __restrict__ sp = reinterpret_cast<const float2*>(tab + FV_GL_TAB_SPLIT);
    for (int i = threadIdx.x; i < kMelNc; i += kGlThreads) tw[i] = twg[i];
    float2* z = zs[wv];

    if (MODE == GL_ITER || MODE == GL_STFT) {
        // z[m] = (w f)[2m] + i (w f)[2m+1]; only the 600 pairs under the window are non-zero
        const float* __restrict__ yr = y + (size_t)b * n;
        const int64_t tt[1] = {live ? t : -1};
        gather_pass<kMelNc, 1>(z, [&](int, int64_t P) { return yr[reflect_index(n, kGlHalf, P)]; }, tt, win, kGlHop,
                               kGlWin, kGlLpad, lane);
        fft_rest<kMelNc, 1>(z, tw, lane);
    }

    // bin pairs (k, 1024 - k), k = 0..512: k = lane + 64 i, and k = 512 on lane 0.  In place: the pair reads and
    // writes z[k] and z[1024 - k] only.
    const float* __restrict__ Sf = S + ft * kGlBins;
    const float2* __restrict__ specf = spec + ft * kGlBins;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int k = i < 8 ? lane + 64 * i : 512;
        if (i == 8 && lane != 0) break;
        const int kc = kMelNc - k;                 // the partner bin, 1024 for k = 0
        const int kz = kc & (kMelNc - 1);          // its place in z
        const float2 w = sp[k];
        float2 xk, xm;                             // X[k], X[1024 - k]
        if (MODE == GL_ITER || MODE == GL_STFT) {
            const BinPair X = split_bin(z, k, kMelNc, w);
            xk = X.k;
            xm = X.m;
        }
        if (MODE == GL_STFT) {
            if (live) {
                spec_out[ft * kGlBins + k] = xk;
                spec_out[ft * kGlBins + kc] = xm;
            }
            continue;
        }
        if (MODE == GL_ISTFT) {
            xk = live ? specf[k] : make_float2(0.f, 0.f);
            xm = live ? specf[kc] : make_float2(0.f, 0.f);
        } else {
            const float sk = live ? Sf[k] : 0.f, sm = live ? Sf[kc] : 0.f;
            const float2 pk = MODE == GL_INIT ? (live ? specf[k] : make_float2(1.f, 0.f)) : gl_phasor(xk);
            const float2 pm = MODE == GL_INIT ? (live ? specf[kc] : make_float2(1.f, 0.f)) : gl_phasor(xm);
            xk = make_float2(sk * pk.x, sk * pk.y);
            xm = make_float2(sm * pm.x, sm * pm.y);
        }
        if (k == 0) xk.y = xm.y = 0.f;             // the inverse real transform ignores Im of DC and Nyquist
        // merge: E = (X[k] + conj X[1024-k]) / 2,  O = conj(W^k) (X[k] - conj X[1024-k]) / 2,  Z[k] = E + i O,
        // Z[1024-k] = conj E + i conj O; stored conjugated for the inverse transform
        const float2 e = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y));
        const float2 d = make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y));
        const float2 o = cmul(make_float2(w.x, -w.y), d);
        z[k] = make_float2(e.x - o.y, -(e.y + o.x));
        z[kz] = make_float2(e.x + o.y, e.y - o.x);
    }
    if (MODE == GL_STFT) return;
    __syncthreads();
    fft_pass4<kMelNc, 1, 1>(z, tw, lane);
    fft_rest<kMelNc, 1>(z, tw, lane);

    // f[2m] = Re conj(z[m]) / 1024, f[2m+1] = Im conj(z[m]) / 1024; the 600 pairs under the window
    if (!live) return;
    float2* __restrict__ fr = reinterpret_cast<float2*>(frames + ft * kGlWin);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const int p = lane + 64 * i;               // pair under the window
        if (p >= kGlWin / 2) break;
        const float2 v = z[p + kGlLpad / 2];
        const float s = 1.f / kMelNc;
        fr[p] = make_float2(win[2 * p] * v.x * s, -(win[2 * p + 1] * v.y) * s);
    }
}

// four consecutive output samples per thread: hop, left pad and trim are multiples of four, so the four share their
// frames, and the float4 loads are aligned
__global__ __launch_bounds__(256) void gl_ola_kernel(const float* __restrict__ frames, float* __restrict__ y,
                                                      const float* __restrict__ tab, int T) {
    const int64_t N = (int64_t)kGlHop * (T - 1);
    const int64_t n0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (n0 >= N) return;
    const int b = blockIdx.y;
    const int64_t j = n0 + (kGlHalf - kGlLpad);    // position of the sample relative to frame 0's first window tap
    const int64_t thi = min((int64_t)T - 1, j / kGlHop);
    const int64_t tlo = j >= kGlWin ? (j - kGlWin) / kGlHop + 1 : 0;
    const float* __restrict__ w2 = tab + FV_GL_TAB_WIN2;
    const float* __restrict__ fb = frames + (size_t)b * T * kGlWin;
    float4 num = make_float4(0.f, 0.f, 0.f, 0.f), den = num;
    for (int64_t t = tlo; t <= thi; ++t) {
        const int i = (int)(j - t * kGlHop);
        const float4 f = *reinterpret_cast<const float4*>(fb + (size_t)t * kGlWin + i);
        const float4 w = *reinterpret_cast<const float4*>(w2 + i);
        num.x += f.x; num.y += f.y; num.z += f.z; num.w += f.w;
        den.x += w.x; den.y += w.y; den.z += w.z; den.w += w.w;
    }
    float4 o;
    o.x = den.x > FLT_MIN ? num.x / den.x : num.x;
    o.y = den.y > FLT_MIN ? num.y / den.y : num.y;
    o.z = den.z > FLT_MIN ? num.z / den.z : num.z;
    o.w = den.w > FLT_MIN ? num.w / den.w : num.w;
    *reinterpret_cast<float4*>(y + (size_t)b * N + n0) = o;
}

constexpr int kMlFrames = 8, kMlMels = 80;

// inv_basis: [80][1025] (the pseudo-inverse transposed: a wave reads consecutive bins)
__global__ __launch_bounds__(256) void mel_to_linear_kernel(const float* __restrict__ mel, const float* __restrict__ invb,
                                                             float* __restrict__ S, int T, float power) {
    __shared__ double A[kMlMels][kMlFrames];
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * kMlFrames;
    for (int i = threadIdx.x; i < kMlMels * kMlFrames; i += 256) {
        const int m = i / kMlFrames, f = i % kMlFrames;
        double a = 0.0;
        if (t0 + f < T) {
            const float v = fminf(fmaxf(mel[((size_t)b * kMlMels + m) * T + t0 + f], 0.f), 1.f);   // _denormalize clips
            a = pow(10.0, ((double)v * 100.0 - 100.0 + 20.0) * 0.05);                               // _db_to_amp(D + ref_level_db)
        }
        A[m][f] = a;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kGlBins; k += 256) {
        double acc[kMlFrames];
#pragma unroll
        for (int f = 0; f < kMlFrames; ++f) acc[f] = 0.0;
        for (int m = 0; m < kMlMels; ++m) {
            const double w = (double)invb[m * kGlBins + k];
#pragma unroll
            for (int f = 0; f < kMlFrames; ++f) acc[f] = fma(w, A[m][f], acc[f]);
        }
#pragma unroll
        for (int f = 0; f < kMlFrames; ++f) {
            if (t0 + f >= T) break;
            const double v = fmax(1e-10, acc[f]);
            S[((size_t)b * T + t0 + f) * kGlBins + k] = (float)(power == 1.5f ? v * sqrt(v) : pow(v, (double)power));
        }
    }
}

constexpr int kIpThreads = 1024, kIpSeg = 16, kIpWaves = kIpThreads / 64;

// One block per row walks the row in tiles of 1024 x 16 samples.  A thread owns 16 consecutive samples: their recurrence
// from a zero input gives the segment's end value e; a segment maps its incoming value c to a^16 c + e, and those maps are
// composed across the lanes (shuffles) and waves (LDS) in order, so every thread learns its exact incoming value and
// runs the recurrence once more from it.
__global__ __launch_bounds__(kIpThreads) void inv_preemph_kernel(const float* __restrict__ y, float* __restrict__ out,
                                                                 int64_t n, float a, float aseg) {
    __shared__ float wA[kIpWaves], wE[kIpWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float* __restrict__ yr = y + (size_t)blockIdx.x * n;
    float* __restrict__ orow = out + (size_t)blockIdx.x * n;
    float carry = 0.f;                             // o[-1] = 0 (lfilter's zero initial state)
    for (int64_t tile = 0; tile < n; tile += (int64_t)kIpThreads * kIpSeg) {
        const int64_t base = tile + (int64_t)threadIdx.x * kIpSeg;
        float v[kIpSeg];
#pragma unroll
        for (int k = 0; k < kIpSeg; ++k) v[k] = base + k < n ? yr[base + k] : 0.f;
        float e = 0.f;
#pragma unroll
        for (int k = 0; k < kIpSeg; ++k) e = fmaf(a, e, v[k]);
        float A = aseg;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {         // inclusive scan of the maps over the wave's lanes
            const float Ap = __shfl_up(A, d), ep = __shfl_up(e, d);
            if (lane >= d) {
                e = fmaf(A, ep, e);
                A *= Ap;
            }
        }
        if (lane == 63) {
            wA[wv] = A;
            wE[wv] = e;
        }
        __syncthreads();
        float c = carry;                           // value entering this wave ...
        for (int w = 0; w < wv; ++w) c = fmaf(wA[w], c, wE[w]);
        float cn = c;                              // ... and leaving the tile (the same sequence in every thread)
        for (int w = wv; w < kIpWaves; ++w) cn = fmaf(wA[w], cn, wE[w]);
        const float Ap = __shfl_up(A, 1), ep = __shfl_up(e, 1);
        float o = lane ? fmaf(Ap, c, ep) : c;      // value entering this thread's segment
#pragma unroll
        for (int k = 0; k < kIpSeg; ++k) {
            o = fmaf(a, o, v[k]);
            if (base + k < n) orow[base + k] = o;
        }
        carry = cn;
        __syncthreads();                           // wA / wE are rewritten by the next tile
    }
}

static dim3 gl_frame_grid(int B, int T) { return dim3((unsigned)((T + kGlFrames - 1) / kGlFrames), (unsigned)B); }

static int gl_ola(const float* frames, float* y, const float* tab, int B, int T, hipStream_t s) {
    const int64_t quads = (int64_t)kGlHop * (T - 1) / 4;
    FV_KERNEL_LAUNCH(gl_ola_kernel, dim3((unsigned)((quads + 255) / 256), (unsigned)B), dim3(256), 0, s, frames, y, tab, T);
    FV_HIP(hipGetLastError());
    return 0;
}

int launch_stft_complex(const float* y, float* spec, const float* tab, int B, int64_t n, hipStream_t s) {
    const int T = (int)(1 + n / kGlHop);
    FV_KERNEL_LAUNCH(gl_frame_kernel<GL_STFT>, gl_frame_grid(B, T), dim3(kGlThreads), 0, s, y, (const float2*)nullptr,
                       (const float*)nullptr, (float*)nullptr, reinterpret_cast<float2*>(spec), tab, n, T);
    FV_HIP(hipGetLastError());
    return 0;
}

int launch_istft(const float* spec, float* y, const float* tab, int B, int T, float* frames, hipStream_t s) {
    FV_KERNEL_LAUNCH(gl_frame_kernel<GL_ISTFT>, gl_frame_grid(B, T), dim3(kGlThreads), 0, s, (const float*)nullptr,
                       reinterpret_cast<const float2*>(spec), (const float*)nullptr, frames, (float2*)nullptr, tab,
                       (int64_t)0, T);
    FV_HIP(hipGetLastError());
    return gl_ola(frames, y, tab, B, T, s);
}

int launch_griffin_lim(const float* S, const float* phase0, float* y, const float* tab, int B, int T, int iters,
                       float* frames, hipStream_t s) {
    const int64_t n = (int64_t)kGlHop * (T - 1);
    if (phase0) {
        FV_KERNEL_LAUNCH(gl_frame_kernel<GL_INIT>, gl_frame_grid(B, T), dim3(kGlThreads), 0, s, (const float*)nullptr,
                           reinterpret_cast<const float2*>(phase0), S, frames, (float2*)nullptr, tab, n, T);
        FV_HIP(hipGetLastError());
        if (int rc = gl_ola(frames, y, tab, B, T, s)) return rc;
    }
    for (int i = 0; i < iters; ++i) {
        FV_KERNEL_LAUNCH(gl_frame_kernel<GL_ITER>, gl_frame_grid(B, T), dim3(kGlThreads), 0, s, (const float*)y,
                           (const float2*)nullptr, S, frames, (float2*)nullptr, tab, n, T);
        FV_HIP(hipGetLastError());
        if (int rc = gl_ola(frames, y, tab, B, T, s)) return rc;
    }
    return 0;
}

int launch_mel_to_linear(const float* mel, const float* invb, float* S, int B, int T, float power, hipStream_t s) {
    FV_KERNEL_LAUNCH(mel_to_linear_kernel, dim3((unsigned)((T + kMlFrames - 1) / kMlFrames), (unsigned)B), dim3(256), 0, s,
                       mel, invb, S, T, power);
    FV_HIP(hipGetLastError());
    return 0;
}

int launch_inv_preemphasis(const float* y, float* out, int B, int64_t n, float coef, hipStream_t s) {
    double p = 1.0;
    for (int k = 0; k < kIpSeg; ++k) p *= (double)coef;
    FV_KERNEL_LAUNCH(inv_preemph_kernel, dim3((unsigned)B), dim3(kIpThreads), 0, s, y, out, n, coef, (float)p);
    FV_HIP(hipGetLastError());
    return 0;
}

}  // namespace fv
