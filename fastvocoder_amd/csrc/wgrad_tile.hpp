// What the training-side weight gradients share (disc_wgrad.hip, mpd_wgrad.hip, gen_grad.hip; basis_learn.hip takes the
// host part; gen_grad_bf16.hip the wave / fragment split, the accumulators and the epilogue under bf16 operands): the
// exact-fp32 matrix-core tile, and the split / record / combine scheme with its host checks.
//
// WgTile<MT>: a block of 4 waves owns MT rows x 128 columns and consumes staged tiles of 32 reduction steps, both
// operands K-contiguous in LDS -- as[row][step], bs[column][step].
//     MT = 128: 2 x 2 waves of 2 x 2 fragments of v_mfma_f32_32x32x2_f32        MT = 64: 2 x 2 waves of 1 x 2
//     MT =  32: 1 x 4 waves of 1 x 1 fragments (32 rows, every one a channel)    MT = 16: 1 x 4 waves of 1 x 2 fragments
//                                                                                 of v_mfma_f32_16x16x4_f32
// so 16 and 32 channels fill their fragments.  Row stride 33 words for the 32-wide fragments (a lane group of 32 reads
// rows 0..31 at one step: banks 33 r + c = 32 different ones), 34 words for the 16-wide ones (a group of 32 lanes reads
// rows 0..15 at two consecutive steps: banks 2 r + {0, 1}, 32 different ones).  Each result is one step-ordered fmaf
// chain.  A kernel whose B operand is not a [column][step] tile of that stride sets off_b itself after init()
// (dense_wgrad_mfma_kernel: a staged span per input channel).
//
// Split / record / combine: the reduction is cut into U units, the units are dealt to S splits in contiguous ranges,
// every block sums its units in ascending order and writes its partial sums to the workspace record ws[s][0 .. R) of
// its split, and a second launch (wgrad_combine_kernel, disc_wgrad.hip) adds the S records, s ascending.  S is a
// function of the shape alone, so identical calls give identical bits; no atomics, no waiting between workgroups.
#pragma once
#include <type_traits>

#include "fv_internal.h"

namespace fv {

typedef float wg_f32x16 __attribute__((ext_vector_type(16)));
typedef float wg_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWgThreads = 256;
constexpr int kWgNT = 128;            // columns per block
constexpr int kWgTK = 32;             // reduction steps per staged tile (the units of a weight gradient)

template <int MT>
struct WgTile {
    static constexpr int F = MT >= 32 ? 32 : 16;            // fragment edge
    static constexpr int WM = MT >= 64 ? 2 : 1, WN = 4 / WM;
    static constexpr int FM = MT / (WM * F), FN = kWgNT / (WN * F);
    static constexpr int STR = F == 32 ? 33 : 34;
    static constexpr int NE = F == 32 ? 16 : 4;
    static constexpr int ARows = MT / 8;                    // rows of the A tile a thread stages
    typedef typename std::conditional<F == 32, wg_f32x16, wg_f32x4>::type acc_t;

    acc_t acc[FM][FN];
    int off_a[FM], off_b[FN];
    int row0, col0, lr, kq;

    __device__ __forceinline__ void init() {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave / WN, wn = wave % WN;
        lr = lane & (F - 1);
        kq = lane / F;
        row0 = wm * FM * F;
        col0 = wn * FN * F;
#pragma unroll
        for (int f = 0; f < FM; ++f) off_a[f] = (row0 + f * F + lr) * STR + kq;
#pragma unroll
        for (int h = 0; h < FN; ++h) off_b[h] = (col0 + h * F + lr) * STR + kq;
#pragma unroll
        for (int f = 0; f < FM; ++f)
#pragma unroll
            for (int h = 0; h < FN; ++h)
#pragma unroll
                for (int e = 0; e < NE; ++e) acc[f][h][e] = 0.f;
    }

    // one staged tile of kWgTK steps
    __device__ __forceinline__ void mma(const float* as, const float* bs) {
        constexpr int KS = F == 32 ? 2 : 4;
#pragma unroll
        for (int kk = 0; kk < kWgTK; kk += KS) {
            float av[FM], bv[FN];
#pragma unroll
            for (int f = 0; f < FM; ++f) av[f] = as[off_a[f] + kk];
#pragma unroll
            for (int h = 0; h < FN; ++h) bv[h] = bs[off_b[h] + kk];
#pragma unroll
            for (int f = 0; f < FM; ++f)
#pragma unroll
                for (int h = 0; h < FN; ++h) {
                    if constexpr (F == 32)
                        acc[f][h] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[f], bv[h], acc[f][h], 0, 0, 0);
                    else
                        acc[f][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[f], bv[h], acc[f][h], 0, 0, 0);
                }
        }
    }

    // C/D maps: 32 x 32: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5);
    //           16 x 16: col = lane & 15, row = 4 (lane >> 4) + reg
    __device__ __forceinline__ int row(int f, int e) const {
        return row0 + f * F + (F == 32 ? (e & 3) + 8 * (e >> 2) + 4 * kq : 4 * kq + e);
    }
    __device__ __forceinline__ int col(int h) const { return col0 + h * F + lr; }

    // the weight gradients' epilogue: the block's tile at (m0, n0) of the record's [M][N] matrix
    __device__ __forceinline__ void store(float* rec, int m0, int n0, int M, int N) const {
#pragma unroll
        for (int f = 0; f < FM; ++f)
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int m = m0 + row(f, e);
                if (m >= M) continue;
#pragma unroll
                for (int h = 0; h < FN; ++h) {
                    const int n = n0 + col(h);
                    if (n < N) rec[(size_t)m * N + n] = acc[f][h][e];
                }
            }
    }
};

// sum over the block's 256 threads in a fixed order: the shuffle tree of each wave, then the 4 waves ascending
__device__ __forceinline__ float wg_block_sum(float v, float* part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();                                  // (the previous sum's readers are done)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// the plan of the scheme: a host plan derives from it, a kernel's arguments hold it (`sp`)
struct WgSplit {
    int64_t R, U;         // floats per record; units
    int S, nch;           // splits; units per row b
    size_t bytes() const { return sizeof(float) * (size_t)S * (size_t)R; }   // the workspace [S][R]
};

// splits of a launch of `base` blocks per split that aims at `aim` blocks: a function of the shape alone
static inline int wg_splits(int64_t base, int64_t U, int aim) {
    int64_t S = (aim + base - 1) / base;
    if (S > U) S = U;
    if (S > 4096) S = 4096;
    return S < 1 ? 1 : (int)S;
}

static inline int wg_workspace_check(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 3))
        return fail(FV_ERR_INVALID_ARG, "%s: workspace of %zu bytes, needs %zu (4-byte aligned)", who, workspace_bytes,
                    need);
    return 0;
}

// two inputs, one or both of two results
static inline int wg_tensor_check(const char* who, const float* g, const float* x, const float* dw, const float* db) {
    if (!g || !x || (!dw && !db) || dw == g || dw == x || db == g || db == x)
        return fail(FV_ERR_INVALID_ARG, "%s: null tensor, or a result aliases an input", who);
    return 0;
}

// dw[i] = sum_s ws[s][i] (i < MN), db[c] = sum_s ws[s][MN + c] (c < Cout), s ascending; dw or db may be null
int launch_wgrad_combine(const float* ws, float* dw, float* db, int64_t MN, int Cout, int64_t R, int S, hipStream_t st);

}  // namespace fv
