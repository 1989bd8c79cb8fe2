// Learning Basis-MelGAN's basis: the encoder / decoder pair of Conv-TasNet with no separator in between
// (include/fastvocoder_hip.h fv_basis_encode, fv_basis_learn_grad).  The decoder is fv_pack_basis + fv_basis_ola.
// Exact fp32 on v_mfma_f32_32x32x2_f32 (16x16x4 for C <= 16), no atomics, no waiting between workgroups: identical
// calls return identical bits.  hop = L / 2, F = ceil(n / hop); K is padded from L to the instruction's depth by
// operands that read as 0 from tap L on.
//
// basis_encode_kernel<FR>: W[b, c, f] = relu(sum_j enc[c, j] wav[b, f hop + j]) as the GEMM [C x L] x [L x F] of one
//     row.  A block owns 64 frames and stages the (64 + 1) hop samples they touch once (0 from n on); the frame
//     operand of column f, tap j is sx[f hop + j], read at lane stride hop: 32 different banks for an odd hop (the
//     shipped 15), and the encoder operand comes from global memory (L words per lane, every block the same 30 KB).
//     FR = 32: 4 waves x 32 channels, two 32-frame fragments each; FR = 16: one 16-channel row of four 16-frame
//     fragments, one per wave.  A fragment's row of W is written as one 128-byte (64-byte) run.
//
// basis_learn_grad_kernel: the whole backward of (encode, decode) for one split of the units (b, 32 frames), one tile
//     of 128 channels (a wave owns 32) and one tile of 32 taps.  Per unit the block stages the 33 hop samples of
//     g_est (0 from F hop on: the crop) and of wav (0 from n on) and its W tile sw[128][33], then every wave runs
//         gW[c, f]      = sum_j basis[j, c] G[j, f]            A = basis from global, B = sg[f hop + j]
//         d_basis[j, c] += sum_f G[j, f] W[c, f]                A = sg[f hop + j0 + lane], B = sw[c][f]
//         sw[c][f]      = W[c, f] > 0 ? gW[c, f] : 0            in place, from the accumulator's own layout
//         d_enc[c, j]   += sum_f gW[c, f] X[j, f]               A = sw[c][f], B = sx[f hop + j0 + lane]
//     so gW lives in registers and LDS only.  Banks (ds_read_b32: two groups of 32 lanes, bank = word mod 32): the
//     sw reads are row stride 33, the sg / sx reads of the two reductions are consecutive words, the accumulator-layout
//     accesses of sw put a group's 32 lanes on 32 consecutive words of one row: all conflict-free; the gW step reads
//     sg at lane stride hop as the encoder does.  L > 32 recomputes gW once per tap tile.  The two sums stay in the
//     accumulators over the split's units and leave as one record [d_enc | d_basis]; wgrad_combine_kernel adds the
//     records in ascending order (wgrad_tile.hpp).  Every record word the combine reads is written by this launch.
#include <math.h>

#include <type_traits>

#include "basis_grad_host.hpp"
#include "wgrad_tile.hpp"

namespace fv {

typedef float le_f32x16 __attribute__((ext_vector_type(16)));
typedef float le_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kLeThreads = 256;
constexpr int kLeTF = 64;         // frames of an encode tile
constexpr int kLgTF = 32;         // frames of a gradient unit: the reduction depth of one staged tile
constexpr int kLgTC = 128;        // channels of a gradient block, 32 per wave
constexpr int kLgTJ = 32;         // taps of a gradient block
constexpr int kLgStr = 33;        // row stride of the W / gW tile
constexpr int kLgAim = 256;       // blocks a gradient launch aims at

struct LeArgs {
    const float* wav;
    const float* enc;
    float* W;
    int64_t n;
    int C, F, L, hop;
};

// grid (ceil(F / 64), ceil(C / (FR == 32 ? 128 : 16)), B); dynamic LDS: (64 + 1) hop floats
template <int FR>
__global__ __launch_bounds__(kLeThreads) void basis_encode_kernel(LeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float le_sx[];
    constexpr int KS = FR == 32 ? 2 : 4, NE = FR == 32 ? 16 : 4;
    constexpr int WM = FR == 32 ? 4 : 1, WN = 4 / WM, FN = kLeTF / (WN * FR);
    typedef typename std::conditional<FR == 32, le_f32x16, le_f32x4>::type acc_t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / WN, wn = wave % WN;
    const int lr = lane & (FR - 1), kq = lane / FR;
    const int64_t f0 = (int64_t)blockIdx.x * kLeTF, s0 = f0 * a.hop, b = blockIdx.z;
    const int cw = (int)blockIdx.y * (WM * FR) + wm * FR, span = (kLeTF + 1) * a.hop;
    const float* src = a.wav + b * a.n;
    for (int i = tid; i < span; i += kLeThreads) le_sx[i] = s0 + i < a.n ? src[s0 + i] : 0.f;
    __syncthreads();
    acc_t acc[FN];
#pragma unroll
    for (int h = 0; h < FN; ++h)
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[h][e] = 0.f;
    const int c = cw + lr;
    const float* er = a.enc + (int64_t)(c < a.C ? c : 0) * a.L;
    for (int kk = 0; kk < a.L; kk += KS) {
        const int j = kk + kq;
        const bool tap = j < a.L;
        const float av = (tap && c < a.C) ? er[j] : 0.f;
#pragma unroll
        for (int h = 0; h < FN; ++h) {
            const float bv = tap ? le_sx[(wn * FN * FR + h * FR + lr) * a.hop + j] : 0.f;
            if constexpr (FR == 32)
                acc[h] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[h], 0, 0, 0);
            else
                acc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[h], 0, 0, 0);
        }
    }
    // C/D maps: 32 x 32: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5); 16 x 16: row = 4 (lane >> 4) + reg
#pragma unroll
    for (int h = 0; h < FN; ++h) {
        const int64_t f = f0 + wn * FN * FR + h * FR + lr;
        if (f >= a.F) continue;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int row = cw + (FR == 32 ? (e & 3) + 8 * (e >> 2) + 4 * kq : 4 * kq + e);
            if (row < a.C) a.W[(b * a.C + row) * a.F + f] = fmaxf(acc[h][e], 0.f);
        }
    }
}

struct LgArgs {
    const float* wav;
    const float* g_est;
    const float* W;
    const float* basis;
    float* ws;              // [S][R]: d_enc [C][L], then d_basis [L][C]
    int64_t n, ng, U, R;    // samples of a row of wav and of g_est (F hop); units; floats per record
    int C, F, L, hop, S, nft;
    int want_enc, want_basis;
};

// grid (ceil(C / 128), ceil(L / 32), S); dynamic LDS: sg [33 hop], sx [33 hop], sw [128][33]
__global__ __launch_bounds__(kLeThreads) void basis_learn_grad_kernel(LgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lg_smem[];
    const int span = (kLgTF + 1) * a.hop;
    float* sg = lg_smem;
    float* sx = sg + span;
    float* sw = sx + span;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, kq = lane >> 5;
    const int c0 = (int)blockIdx.x * kLgTC, cw = c0 + wave * 32, j0 = (int)blockIdx.y * kLgTJ, s = blockIdx.z;
    const int64_t u0 = (int64_t)s * a.U / a.S, u1 = (int64_t)(s + 1) * a.U / a.S;
    float* swv = sw + wave * 32 * kLgStr;
    const bool my_tap = j0 + lr < a.L, my_ch = cw + lr < a.C;
    le_f32x16 acc_e, acc_b;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc_e[e] = acc_b[e] = 0.f;
    for (int64_t u = u0; u < u1; ++u) {
        const int64_t b = u / a.nft, f0 = (u % a.nft) * kLgTF, s0 = f0 * a.hop;
        const float* gsrc = a.g_est + b * a.ng;
        const float* xsrc = a.wav + b * a.n;
        __syncthreads();                                  // the unit before is read
        for (int i = tid; i < span; i += kLeThreads) {
            sg[i] = s0 + i < a.ng ? gsrc[s0 + i] : 0.f;
            sx[i] = s0 + i < a.n ? xsrc[s0 + i] : 0.f;
        }
        {
            const int fl = tid & 31;
            const bool live = f0 + fl < a.F;
#pragma unroll
            for (int i = 0; i < kLgTC / 8; ++i) {
                const int row = (tid >> 5) + 8 * i;
                sw[row * kLgStr + fl] = (live && c0 + row < a.C) ? a.W[(b * a.C + c0 + row) * a.F + f0 + fl] : 0.f;
            }
        }
        __syncthreads();
        le_f32x16 gw;
#pragma unroll
        for (int e = 0; e < 16; ++e) gw[e] = 0.f;
        if (a.want_enc)
            for (int kk = 0; kk < a.L; kk += 2) {
                const int j = kk + kq;
                const bool tap = j < a.L;
                const float av = (tap && my_ch) ? a.basis[(int64_t)j * a.C + cw + lr] : 0.f;
                const float bv = tap ? sg[lr * a.hop + j] : 0.f;
                gw = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, gw, 0, 0, 0);
            }
        if (a.want_basis)
#pragma unroll
            for (int kk = 0; kk < kLgTF; kk += 2) {
                const int f = kk + kq;
                const float av = my_tap ? sg[f * a.hop + j0 + lr] : 0.f;
                acc_b = __builtin_amdgcn_mfma_f32_32x32x2f32(av, swv[lr * kLgStr + f], acc_b, 0, 0, 0);
            }
        if (!a.want_enc) continue;
        __syncthreads();                                  // W is read as an operand; gW takes its place
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int at = ((e & 3) + 8 * (e >> 2) + 4 * kq) * kLgStr + lr;
            swv[at] = swv[at] > 0.f ? gw[e] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kLgTF; kk += 2) {
            const int f = kk + kq;
            const float bv = my_tap ? sx[f * a.hop + j0 + lr] : 0.f;
            acc_e = __builtin_amdgcn_mfma_f32_32x32x2f32(swv[lr * kLgStr + f], bv, acc_e, 0, 0, 0);
        }
    }
    float* rec = a.ws + (int64_t)s * a.R;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int row = (e & 3) + 8 * (e >> 2) + 4 * kq;
        if (a.want_enc && cw + row < a.C && my_tap) rec[(int64_t)(cw + row) * a.L + j0 + lr] = acc_e[e];
        if (a.want_basis && j0 + row < a.L && my_ch)
            rec[(int64_t)a.C * a.L + (int64_t)(j0 + row) * a.C + cw + lr] = acc_b[e];
    }
}

struct LgPlan {
    int F, hop, S, nft;
    unsigned gx, gy;
    int64_t U, R;
    size_t lds_bytes;
};

// 0, or the code of the refusal (already recorded)
static int learn_check(const char* who, int B, int64_t n, int C, int L, int* F) {
    const int lrc = basis_L_check(L);
    if (lrc == 1) return fail(FV_ERR_INVALID_ARG, "%s: L=%d (even, >= 2)", who, L);
    if (B < 1 || C < 1 || n < 1) return fail(FV_ERR_INVALID_ARG, "%s: B=%d n=%lld C=%d (each 1 or more)", who, B, (long long)n, C);
    if (lrc == 2) return fail(FV_ERR_UNSUPPORTED, "%s: L=%d (%d at most)", who, L, kBhMaxL);
    const int64_t frames = (n + L / 2 - 1) / (L / 2);
    if (frames > 0x7fffffffLL || basis_shape_check(B, C, (int)frames) || (int64_t)C * L > ((int64_t)1 << 30))
        return fail(FV_ERR_UNSUPPORTED, "%s: B=%d n=%lld C=%d exceed a launch", who, B, (long long)n, C);
    *F = (int)frames;
    return 0;
}

static void learn_grad_plan(int B, int C, int F, int L, LgPlan* p) {
    p->F = F;
    p->hop = L / 2;
    p->nft = (int)(((int64_t)F + kLgTF - 1) / kLgTF);
    p->U = (int64_t)B * p->nft;
    p->gx = (unsigned)((C + kLgTC - 1) / kLgTC);
    p->gy = (unsigned)((L + kLgTJ - 1) / kLgTJ);
    p->R = 2 * (int64_t)C * L;
    p->S = wg_splits((int64_t)p->gx * p->gy, p->U, kLgAim);
    p->lds_bytes = sizeof(float) * (2 * (size_t)(kLgTF + 1) * p->hop + (size_t)kLgTC * kLgStr);
}

}  // namespace fv

using namespace fv;

extern "C" {

int fv_basis_encode(const float* wav, const float* enc, float* W, int B, int64_t n, int C, int L, void* stream) {
    int F = 0;
    if (int rc = learn_check("basis_encode", B, n, C, L, &F)) return rc;
    if (!wav || !enc || !W || W == wav || W == enc)
        return fail(FV_ERR_INVALID_ARG, "basis_encode: null tensor, or W aliases an input");
    LeArgs a = {wav, enc, W, n, C, F, L, L / 2};
    const size_t lds = sizeof(float) * (size_t)(kLeTF + 1) * (L / 2);
    const unsigned gx = (unsigned)(((int64_t)F + kLeTF - 1) / kLeTF);
    if (C <= 16)
        FV_KERNEL_LAUNCH(basis_encode_kernel<16>, dim3(gx, 1, (unsigned)B), dim3(kLeThreads), lds, (hipStream_t)stream, a);
    else
        FV_KERNEL_LAUNCH(basis_encode_kernel<32>, dim3(gx, (unsigned)((C + 127) / 128), (unsigned)B), dim3(kLeThreads),
                           lds, (hipStream_t)stream, a);
    FV_HIP(hipGetLastError());
    return 0;
}

int64_t fv_basis_learn_grad_workspace_bytes(int B, int64_t n, int C, int L) {
    int F = 0;
    if (int rc = learn_check("basis_learn_grad", B, n, C, L, &F)) return rc;
    LgPlan p;
    learn_grad_plan(B, C, F, L, &p);
    return (int64_t)sizeof(float) * p.S * p.R;
}

int fv_basis_learn_grad(const float* wav, const float* g_est, const float* W, const float* basis, float* d_enc,
                        float* d_basis, int B, int64_t n, int C, int L, void* workspace, size_t workspace_bytes,
                        void* stream) {
    int F = 0;
    if (int rc = learn_check("basis_learn_grad", B, n, C, L, &F)) return rc;
    if (!wav || !g_est || !W || !basis || (!d_enc && !d_basis))
        return fail(FV_ERR_INVALID_ARG, "basis_learn_grad: null tensor (one of d_enc and d_basis may be null)");
    const float* in[4] = {wav, g_est, W, basis};
    for (const float* p : in)
        if (p == d_enc || p == d_basis) return fail(FV_ERR_INVALID_ARG, "basis_learn_grad: a result aliases an input");
    if (d_enc == d_basis) return fail(FV_ERR_INVALID_ARG, "basis_learn_grad: d_enc aliases d_basis");
    LgPlan p;
    learn_grad_plan(B, C, F, L, &p);
    if (int rc = wg_workspace_check("basis_learn_grad", workspace, workspace_bytes,
                                    sizeof(float) * (size_t)p.S * (size_t)p.R))
        return rc;
    LgArgs a = {wav, g_est, W, basis, static_cast<float*>(workspace), n, (int64_t)F * p.hop, p.U, p.R,
                C, F, L, p.hop, p.S, p.nft, d_enc != nullptr, d_basis != nullptr};
    FV_KERNEL_LAUNCH(basis_learn_grad_kernel, dim3(p.gx, p.gy, (unsigned)p.S), dim3(kLeThreads), p.lds_bytes,
                       (hipStream_t)stream, a);
    FV_HIP(hipGetLastError());
    return launch_wgrad_combine(a.ws, d_enc, d_basis, (int64_t)C * L, C * L, p.R, p.S, (hipStream_t)stream);
}

}  // extern "C"
