// Gradient clipping and the Adam update of a whole parameter set in three launches (reference: bin/train.py:126-136,
// 176-186 -- nn.utils.clip_grad_norm_ followed by Adam.step(); include/fastvocoder_hip.h fv_grad_sq_norm,
// fv_adam_step).  Exact fp32 per element, no atomics, no waiting between workgroups.
//
// Both entries walk one device table: fv_adam_tensor rows (the four pointers of a parameter, its element count and
// the two step-dependent factors) and a list of chunks, (row, chunk within the row), kFvAdamChunk = 4096 elements
// each.  One block of 256 threads owns one chunk; thread t owns the elements 4 (256 r + t) + {0..3}, r = 0..3, of
// it -- with 16-byte loads where the row's pointers allow it, with scalar loads of the SAME elements otherwise, so
// a thread's arithmetic (and with it every bit of the result) does not depend on how a tensor happens to be aligned.
//
// grad_sq_partial_kernel: a thread adds its 16 squares in element order (one fmaf chain, fp32), the block adds the
//     256 thread sums as doubles in a fixed tree (xor shuffles inside a wave, the four waves in ascending order) and
//     writes ONE double per chunk: every word the second launch reads is written by the first.
// grad_norm_finish_kernel: one block.  Thread t adds the partials of the t-th of 256 equal ranges in ascending order,
//     thread 0 adds the 256 range sums in ascending order; norm = sqrt(sum), coef = max_norm / (norm + 1e-6) clamped
//     to at most 1 (a NaN passes, as torch.clamp lets it).
// adam_step_kernel: g' = coef g (written back to the gradient when there is a coef), m = b1 m + (1 - b1) g',
//     v = b2 v + (1 - b2) g'^2, p -= step_size * (m / (sqrt(v) * inv_sqrt_bc2 + eps)).
// grad_bucket_pack_kernel (fv_grad_bucket_pack, data-parallel training): row r's span of a flat bucket, row.g, becomes
//     scale * src[r] -- one rounding per element -- over the same table and the same thread-to-element map; the span is
//     row.n rounded up to a whole 16-byte group, the words past row.n are written as zeros, a NULL src[r] gives a span of
//     zeros: every word the collective sends is written by this launch.
#include <math.h>

#include "fv_internal.h"

namespace fv {

typedef float oa_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kFvAdamChunk = FV_ADAM_CHUNK;
constexpr int kOaThreads = 256;
constexpr int kOaRounds = kFvAdamChunk / (4 * kOaThreads);      // 16-byte groups per thread and chunk (4)
static_assert(kOaRounds * 4 * kOaThreads == kFvAdamChunk, "a chunk is a whole number of rounds");
static_assert(sizeof(fv_adam_tensor) == 48, "the table row is part of the ABI");

// the table's pointers are loaded from memory, so the compiler cannot know that they are global addresses: say so
// (global_load / global_store in place of the flat forms, which also wait on the LDS counter)
typedef __attribute__((address_space(1))) float oa_gf32;
typedef __attribute__((address_space(1))) oa_f32x4 oa_gf32x4;

static __device__ __forceinline__ bool oa_aligned(const void* a) { return ((uintptr_t)a & 15) == 0; }

// the elements [at, at + 4) of a row of n, as far as they exist (the others read as 0)
static __device__ __forceinline__ oa_f32x4 oa_load(const float* base, int64_t at, int64_t n, bool vec) {
    const oa_gf32* src = (const oa_gf32*)base + at;
    if (vec && at + 4 <= n) return *(const oa_gf32x4*)src;
    oa_f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (at + j < n) r[j] = src[j];
    return r;
}

static __device__ __forceinline__ void oa_store(float* base, int64_t at, int64_t n, bool vec, oa_f32x4 val) {
    oa_gf32* dst = (oa_gf32*)base + at;
    if (vec && at + 4 <= n) {
        *(oa_gf32x4*)dst = val;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (at + j < n) dst[j] = val[j];
}

__global__ __launch_bounds__(kOaThreads) void grad_sq_partial_kernel(const fv_adam_tensor* __restrict__ rows,
                                                                     const fv_adam_chunk* __restrict__ chunks,
                                                                     int n_tensors, double* __restrict__ partial) {
    __shared__ double wave_sum[kOaThreads / 64];
    const fv_adam_chunk c = chunks[blockIdx.x];
    if (c.tensor < 0 || c.tensor >= n_tensors || c.index < 0) {      // a table this library did not lay out
        if (threadIdx.x == 0) partial[blockIdx.x] = 0.0;
        return;
    }
    const fv_adam_tensor row = rows[c.tensor];
    const float* g = row.g;
    const int64_t base = (int64_t)c.index * kFvAdamChunk;
    const bool vec = oa_aligned(g);
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < kOaRounds; ++r) {
        const int64_t at = base + 4 * ((int64_t)r * kOaThreads + threadIdx.x);
        if (at >= row.n) break;
        const oa_f32x4 x = oa_load(g, at, row.n, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fmaf(x[j], x[j], s);
    }
    double d = (double)s;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) d += __shfl_xor(d, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = wave_sum[0];
#pragma unroll
        for (int w = 1; w < kOaThreads / 64; ++w) t += wave_sum[w];
        partial[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kOaThreads) void grad_norm_finish_kernel(const double* __restrict__ partial, int n_chunks,
                                                                      float max_norm, float* __restrict__ out) {
    __shared__ double range_sum[kOaThreads];
    const int per = (n_chunks + kOaThreads - 1) / kOaThreads;
    const int lo = min(n_chunks, (int)threadIdx.x * per), hi = min(n_chunks, lo + per);
    double t = 0.0;
    for (int i = lo; i < hi; ++i) t += partial[i];
    range_sum[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int i = 0; i < kOaThreads; ++i) total += range_sum[i];
    const float norm = (float)sqrt(total);
    const float c = max_norm / (norm + 1e-6f);
    out[0] = norm;
    out[1] = c > 1.f ? 1.f : c;           // a NaN stays a NaN
}

__global__ __launch_bounds__(kOaThreads) void adam_step_kernel(const fv_adam_tensor* __restrict__ rows,
                                                               const fv_adam_chunk* __restrict__ chunks,
                                                               int n_tensors, const float* __restrict__ coef_ptr,
                                                               float b1, float omb1, float b2, float omb2, float eps) {
    const fv_adam_chunk c = chunks[blockIdx.x];
    if (c.tensor < 0 || c.tensor >= n_tensors || c.index < 0) return;
    const fv_adam_tensor row = rows[c.tensor];
    const int64_t base = (int64_t)c.index * kFvAdamChunk;
    const bool vec = oa_aligned(row.p) && oa_aligned(row.g) && oa_aligned(row.m) && oa_aligned(row.v);
    const bool clip = coef_ptr != nullptr;
    const float coef = clip ? *coef_ptr : 1.f;
#pragma unroll
    for (int r = 0; r < kOaRounds; ++r) {
        const int64_t at = base + 4 * ((int64_t)r * kOaThreads + threadIdx.x);
        if (at >= row.n) break;
        oa_f32x4 g = oa_load(row.g, at, row.n, vec);
        oa_f32x4 m = oa_load(row.m, at, row.n, vec);
        oa_f32x4 v = oa_load(row.v, at, row.n, vec);
        oa_f32x4 p = oa_load(row.p, at, row.n, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (clip) g[j] = coef * g[j];
            m[j] = fmaf(b1, m[j], omb1 * g[j]);
            v[j] = fmaf(b2, v[j], omb2 * (g[j] * g[j]));
            const float denom = fmaf(sqrtf(v[j]), row.inv_sqrt_bc2, eps);
            p[j] = fmaf(-row.step_size, m[j] / denom, p[j]);
        }
        if (clip) oa_store(row.g, at, row.n, vec, g);
        oa_store(row.m, at, row.n, vec, m);
        oa_store(row.v, at, row.n, vec, v);
        oa_store(row.p, at, row.n, vec, p);
    }
}

__global__ __launch_bounds__(kOaThreads) void grad_bucket_pack_kernel(const fv_adam_tensor* __restrict__ rows,
                                                                      const fv_adam_chunk* __restrict__ chunks,
                                                                      int n_tensors, const float* const* __restrict__ srcs,
                                                                      float scale) {
    const fv_adam_chunk c = chunks[blockIdx.x];
    if (c.tensor < 0 || c.tensor >= n_tensors || c.index < 0) return;
    const fv_adam_tensor row = rows[c.tensor];
    const float* src = srcs[c.tensor];
    const int64_t base = (int64_t)c.index * kFvAdamChunk;
    const int64_t padded = (row.n + 3) & ~(int64_t)3;        // the span: whole 16-byte groups
    const bool vec_src = src != nullptr && oa_aligned(src);
    const bool vec_dst = oa_aligned(row.g);
#pragma unroll
    for (int r = 0; r < kOaRounds; ++r) {
        const int64_t at = base + 4 * ((int64_t)r * kOaThreads + threadIdx.x);
        if (at >= row.n) break;
        oa_f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (src != nullptr) {
            g = oa_load(src, at, row.n, vec_src);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (at + j < row.n) g[j] = scale * g[j];      // the pad words stay +0 whatever the scale
        }
        oa_store(row.g, at, padded, vec_dst, g);
    }
}

static int oa_table_check(const char* who, const void* rows, const void* chunks, int n_tensors, int64_t n_chunks) {
    if (!rows || !chunks) return fail(FV_ERR_INVALID_ARG, "%s: null table", who);
    if (n_tensors < 1 || n_chunks < 1 || n_chunks > 0x7fffffff)
        return fail(FV_ERR_INVALID_ARG, "%s: %d tensors in %lld chunks", who, n_tensors, (long long)n_chunks);
    if (((uintptr_t)rows & 7) || ((uintptr_t)chunks & 7))
        return fail(FV_ERR_INVALID_ARG, "%s: the table must be 8-byte aligned", who);
    return 0;
}

}  // namespace fv

using namespace fv;

extern "C" {

int64_t fv_grad_sq_norm_workspace_bytes(int64_t n_chunks) {
    if (n_chunks < 1 || n_chunks > 0x7fffffff)
        return fail(FV_ERR_INVALID_ARG, "grad_sq_norm: %lld chunks", (long long)n_chunks);
    return (int64_t)sizeof(double) * n_chunks;
}

int fv_grad_sq_norm(const fv_adam_tensor* tensors, const fv_adam_chunk* chunks, int n_tensors, int64_t n_chunks,
                    float max_norm, void* workspace, size_t workspace_bytes, float* out, void* stream) {
    if (int rc = oa_table_check("grad_sq_norm", tensors, chunks, n_tensors, n_chunks)) return rc;
    if (!(max_norm >= 0.f)) return fail(FV_ERR_INVALID_ARG, "grad_sq_norm: max_norm = %g", (double)max_norm);
    if (!out || !workspace || ((uintptr_t)workspace & 7) || ((uintptr_t)out & 3))
        return fail(FV_ERR_INVALID_ARG, "grad_sq_norm: null or misaligned workspace / result");
    if (workspace_bytes < sizeof(double) * (size_t)n_chunks)
        return fail(FV_ERR_WORKSPACE, "grad_sq_norm: workspace of %zu bytes, %zu needed", workspace_bytes,
                    sizeof(double) * (size_t)n_chunks);
    const hipStream_t st = (hipStream_t)stream;
    FV_KERNEL_LAUNCH(grad_sq_partial_kernel, dim3((unsigned)n_chunks), dim3(kOaThreads), 0, st, tensors, chunks,
                       n_tensors, (double*)workspace);
    FV_HIP(hipGetLastError());
    FV_KERNEL_LAUNCH(grad_norm_finish_kernel, dim3(1), dim3(kOaThreads), 0, st, (const double*)workspace,
                       (int)n_chunks, max_norm, out);
    FV_HIP(hipGetLastError());
    return 0;
}

int fv_adam_step(const fv_adam_tensor* tensors, const fv_adam_chunk* chunks, int n_tensors, int64_t n_chunks,
                 const float* coef, double beta1, double beta2, double eps, void* stream) {
    if (int rc = oa_table_check("adam_step", tensors, chunks, n_tensors, n_chunks)) return rc;
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0))
        return fail(FV_ERR_INVALID_ARG, "adam_step: betas (%g, %g), eps %g", beta1, beta2, eps);
    if ((uintptr_t)coef & 3) return fail(FV_ERR_INVALID_ARG, "adam_step: misaligned coef");
    FV_KERNEL_LAUNCH(adam_step_kernel, dim3((unsigned)n_chunks), dim3(kOaThreads), 0, (hipStream_t)stream, tensors,
                       chunks, n_tensors, coef, (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps);
    FV_HIP(hipGetLastError());
    return 0;
}

int fv_grad_bucket_pack(const fv_adam_tensor* tensors, const fv_adam_chunk* chunks, int n_tensors, int64_t n_chunks,
                        const float* const* src, float scale, void* stream) {
    if (int rc = oa_table_check("grad_bucket_pack", tensors, chunks, n_tensors, n_chunks)) return rc;
    if (!src || ((uintptr_t)src & 7)) return fail(FV_ERR_INVALID_ARG, "grad_bucket_pack: null or misaligned src array");
    FV_KERNEL_LAUNCH(grad_bucket_pack_kernel, dim3((unsigned)n_chunks), dim3(kOaThreads), 0, (hipStream_t)stream,
                       tensors, chunks, n_tensors, src, scale);
    FV_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
