// The generators' weight gradients with bf16 operands (include/fastvocoder_hip.h fv_conv1d_weight_grad_dilated_bf16,
// fv_conv_transpose1d_weight_grad_bf16; the Python side's grad_precision = "bf16"):
//     dw = sum over (b, t) of bf16(g) bf16(xa), fp32 accumulation        db = sum of the un-rounded g
// bf16(.) is round-to-nearest-even of the fp32 value, applied to the value the kernel stages: a padded zero stays zero,
// a reflected sample is the rounded sample.  The product of two bf16 values is exact in fp32, so the result differs
// from the fp32 sum of the rounded products by the order of the additions alone.  The GEMMs, the index arithmetic, the
// arguments (GgWArgs), the checks and the split / record / combine scheme are those of gen_grad.hip; no atomics, no
// waiting between workgroups, the split count a function of the shape alone.
//
// The multi-period discriminator's (k, 1) convs take the same kernel (fv_period_conv_weight_grad_bf16): on the flat axis
// q = h' p + c of a [B, C, H, p] map a period conv is a 1-D conv whose column (ci, j) reads
//     x_flat[b, ci, pos],   pos = stride (q - q mod p) + q mod p + (j - pad) p,   zero unless 0 <= pos < H p
// (pos = (stride h' + j - pad) p + c: inside the map exactly when the row is).  At stride 1 that is the dilated conv
// with dil = p and zero padding pad p, as it stands; at stride 2 and 3 it is GgWArgs' pos = t sB + j dB - pad with
// dB = p, pad = pad p and one more term, -(sB - 1)(t mod p), which the template period P > 0 adds (P = 0: none, the
// generators' code unchanged).
//
// gen_wgrad_bf16_kernel<MT, REFLECT, P>: 4 waves own MT rows x 128 columns (the wave / fragment split of WgTile<MT>) and
// consume units of 64 reduction steps on v_mfma_f32_32x32x16_bf16 (MT >= 32) or v_mfma_f32_16x16x32_bf16 (MT = 16).
//
// LDS image: as[row][32 words], bs[column][32 words], a word = two bf16.  Which step of the unit sits at which k of
// the image is free as long as A and B agree; word c of a row holds steps (c, c + 32) of the unit, so the thread that
// stages word c loads positions t0 + c and t0 + c + 32: both loads of a 32-lane group run over 32 consecutive floats,
// as in the fp32 kernel, and a row end inside a pair is two independent bounds checks.  A lane's fragment of 8 k is
// one 16-byte read (ds_read_b128) at word 4 kq + 8 ks (32-wide: kq = lane >> 5, ks < 4) or 4 kq + 16 ks (16-wide:
// kq = lane >> 4, ks < 2).
//
// Banks.  ds_read_b128 is served in the 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32 for the upper
// half), banks = word address mod 64, i.e. 16 slots of 4 words; a group is conflict-free when its 16 slots differ.
//     32-wide, row stride 36 words: a group's lanes share kq and read rows {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31},
//     each set one residue of every class mod 16; slot = (9 r + kq + 2 ks) mod 16, and 9 is odd: 16 different slots.
//     16-wide, row stride 40 words: a group reads rows {0-3, 12-15} at kq and rows {4-11} at kq + 1 (or the other way
//     round); slot = (10 r + kq + 4 ks) mod 16; 10 r mod 16 runs over the 8 even slots on either row set (r mod 8 takes
//     every value once, 5 is odd), so one set fills the even slots and the other the odd ones: 16 different slots.
//     (An odd multiple of 4 words, as for the 32-wide fragments, would collide here: 9 r = 9 r' + 1 has solutions
//     between the two row sets.)
// The staging store is ds_write_b32, banks mod 32 per 32-lane group: a group writes words 0..31 of one row.
//
// Overlap: the loads of unit u + 1 are issued into registers before the MFMAs of unit u, and are converted and stored
// into the other of two LDS images after them: one barrier per unit (between a unit's staging and its MFMAs; an image
// is overwritten two units after it was read).  One unit of prefetch covers the unit's matrix time and fragment reads,
// not the whole round trip of its loads: at 16 and 32 channels the launch is bound by that latency.
#include "gen_grad_host.hpp"

namespace fv {

constexpr int kBfTK = 64;             // reduction steps per unit
constexpr int kBfW = kBfTK / 2;       // words per row of the LDS image
constexpr int kBfBiasBlocks = 32;     // bias blocks per split at most: one channel per wave up to 128 channels

typedef __bf16 bf_x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf_x2 __attribute__((ext_vector_type(2)));

// (lo, hi) -> one word of two bf16, round-to-nearest-even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t bf_pack(float lo, float hi) {
    bf_x2 v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return __builtin_bit_cast(uint32_t, v);
}

// WgTile<MT>'s wave / fragment split, accumulators and epilogue over the bf16 image
template <int MT>
struct BfTile : WgTile<MT> {
    using W = WgTile<MT>;
    static constexpr int STRW = W::F == 32 ? 36 : 40;     // words per row
    static constexpr int KW = W::F == 32 ? 8 : 16;        // words per MFMA: 16 or 32 k

    __device__ __forceinline__ void init() {
        W::init();
#pragma unroll
        for (int f = 0; f < W::FM; ++f) this->off_a[f] = (this->row0 + f * W::F + this->lr) * STRW + 4 * this->kq;
#pragma unroll
        for (int h = 0; h < W::FN; ++h) this->off_b[h] = (this->col0 + h * W::F + this->lr) * STRW + 4 * this->kq;
    }

    // one staged unit of kBfTK steps
    __device__ __forceinline__ void mma(const uint32_t* as, const uint32_t* bs) {
#pragma unroll
        for (int kk = 0; kk < kBfW; kk += KW) {
            bf_x8 av[W::FM], bv[W::FN];
#pragma unroll
            for (int f = 0; f < W::FM; ++f) av[f] = *reinterpret_cast<const bf_x8*>(as + this->off_a[f] + kk);
#pragma unroll
            for (int h = 0; h < W::FN; ++h) bv[h] = *reinterpret_cast<const bf_x8*>(bs + this->off_b[h] + kk);
#pragma unroll
            for (int f = 0; f < W::FM; ++f)
#pragma unroll
                for (int h = 0; h < W::FN; ++h) {
                    if constexpr (W::F == 32)
                        this->acc[f][h] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[f], bv[h], this->acc[f][h], 0, 0, 0);
                    else
                        this->acc[f][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[f], bv[h], this->acc[f][h], 0, 0, 0);
                }
        }
    }
};

// grid (x_tiles + bias blocks, ceil(M / MT), S); REFLECT: the B source is read through a reflection pad (pad < TB);
// P > 0: step t reads from t sB - (sB - 1)(t mod P), the flat axis of a period-P map under a row stride of sB
template <int MT, bool REFLECT, int P = 0>
__global__ __launch_bounds__(kWgThreads) void gen_wgrad_bf16_kernel(GgWArgs a) {
    using T = BfTile<MT>;
    constexpr int ARows = MT / 8;
    __shared__ __attribute__((aligned(16))) uint32_t as[2][MT * T::STRW];
    __shared__ __attribute__((aligned(16))) uint32_t bs[2][kWgNT * T::STRW];
    const int s = blockIdx.z, tid = threadIdx.x;
    const int64_t u0 = (int64_t)s * a.sp.U / a.sp.S, u1 = (int64_t)(s + 1) * a.sp.U / a.sp.S;
    const int N = a.Cb * a.k;
    float* rec = a.ws + (size_t)s * a.sp.R;
    if ((int)blockIdx.x >= a.x_tiles) {                   // the bias column: the un-rounded g
        if (blockIdx.y == 0) gg_bias_column<kBfTK>(a, rec, u0, u1, N);
        return;
    }
    const int n0 = blockIdx.x * kWgNT, m0 = blockIdx.y * MT;
    const int sc = tid & 31, sr = tid >> 5;
    int b_off[kGgBRows], b_pos[kGgBRows];                 // cb TB, and j dB - pad
#pragma unroll
    for (int i = 0; i < kGgBRows; ++i) {
        const int n = n0 + sr + 8 * i, cb = n / a.k;
        b_off[i] = n < N ? cb * a.TB : 0;
        b_pos[i] = n < N ? (n - cb * a.k) * a.dB - a.pad : kGgDead;
    }
    float va[ARows][2], vb[kGgBRows][2];                  // the unit in flight: steps (sc, sc + 32) of each staged row
    uint32_t ok_a[2], ok_b[2];                            // bit i: the value of staged row i counts (else: zero)

    // Every load is unconditional, from an address clamped into its row, and what lies outside the problem is zeroed
    // by its bit when the unit is staged: no branch around a load, nothing waits before the MFMAs.
    auto load = [&](int b, int ch) {                      // unit ch of row b
        const int t0 = ch * kBfTK + sc;
        const float* ab = a.a + (size_t)b * a.M * a.TR;
        const float* bb = a.b + (size_t)b * a.Cb * a.TB;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int t = t0 + e * kBfW;
            const bool live = t < a.TR;
            const int tc = live ? t : a.TR - 1;           // (tc sB stays inside the source row: no overflow)
            int tb = tc * a.sB;
            if constexpr (P > 0) tb -= (a.sB - 1) * (tc % P);
            ok_a[e] = ok_b[e] = 0;
#pragma unroll
            for (int i = 0; i < ARows; ++i) {
                const int m = m0 + sr + 8 * i;
                const bool ok = live && m < a.M;
                va[i][e] = ab[(size_t)(m < a.M ? m : a.M - 1) * a.TR + tc];
                ok_a[e] |= (uint32_t)ok << i;
            }
#pragma unroll
            for (int i = 0; i < kGgBRows; ++i) {
                int pos = tb + b_pos[i];
                if constexpr (REFLECT) {                  // one mirror is enough: pad < TB; a dead column stays outside
                    if (pos < 0) pos = -pos;
                    else if (pos >= a.TB) pos = 2 * (a.TB - 1) - pos;
                }
                const bool ok = live && (unsigned)pos < (unsigned)a.TB;
                vb[i][e] = bb[(size_t)b_off[i] + (ok ? pos : 0)];
                ok_b[e] |= (uint32_t)ok << i;
            }
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < ARows; ++i)
            as[buf][(sr + 8 * i) * T::STRW + sc] =
                bf_pack((ok_a[0] >> i & 1) ? va[i][0] : 0.f, (ok_a[1] >> i & 1) ? va[i][1] : 0.f);
#pragma unroll
        for (int i = 0; i < kGgBRows; ++i)
            bs[buf][(sr + 8 * i) * T::STRW + sc] =
                bf_pack((ok_b[0] >> i & 1) ? vb[i][0] : 0.f, (ok_b[1] >> i & 1) ? vb[i][1] : 0.f);
    };

    T tile;
    tile.init();
    int cur = 0, nb = (int)(u0 / a.sp.nch), nc = (int)(u0 % a.sp.nch);     // the unit to load next
    load(nb, nc);                                         // (a split holds at least one unit: S <= U)
    for (int64_t u = u0; u < u1; ++u) {
        stage(cur);                                       // its last readers, two units back, passed a barrier since
        __syncthreads();
        if (++nc == a.sp.nch) nc = 0, ++nb;
        if (u + 1 < u1) load(nb, nc);                     // in flight under this unit's MFMAs
        tile.mma(as[cur], bs[cur]);
        cur ^= 1;
    }
    tile.store(rec, m0, n0, a.M, N);
}

// the bf16 kernel at the plan's tile height
static int gg_wgrad_bf16(const GgWPlan& p, const GgWArgs& a, float* dw, float* db, void* workspace,
                         size_t workspace_bytes, const char* who, hipStream_t st, bool reflect) {
    return gg_wgrad_run(p, a, dw, db, workspace, workspace_bytes, who, st, kBfBiasBlocks,
                        [&](int rows, dim3 grid, const GgWArgs& ka) {
#define GG_WGRAD(MT)                                                                                               \
    if (reflect) FV_KERNEL_LAUNCH((gen_wgrad_bf16_kernel<MT, true>), grid, dim3(kWgThreads), 0, st, ka);           \
    else FV_KERNEL_LAUNCH((gen_wgrad_bf16_kernel<MT, false>), grid, dim3(kWgThreads), 0, st, ka)
        GG_BY_ROWS(rows, GG_WGRAD)
#undef GG_WGRAD
    });
}

// the periodic variant: the strided layers of DiscriminatorP, 64 output channels and more (gg_rows: 64 or 128)
static int gg_wgrad_bf16_period(const GgWPlan& p, const GgWArgs& a, float* dw, float* db, void* workspace,
                                size_t workspace_bytes, const char* who, hipStream_t st, int period) {
    return gg_wgrad_run(p, a, dw, db, workspace, workspace_bytes, who, st, kBfBiasBlocks,
                        [&](int rows, dim3 grid, const GgWArgs& ka) {
#define GG_PERIOD(P)                                                                                               \
    case P:                                                                                                        \
        if (rows == 128) FV_KERNEL_LAUNCH((gen_wgrad_bf16_kernel<128, false, P>), grid, dim3(kWgThreads), 0, st, ka);   \
        else FV_KERNEL_LAUNCH((gen_wgrad_bf16_kernel<64, false, P>), grid, dim3(kWgThreads), 0, st, ka);           \
        break;
        switch (period) {
            GG_PERIOD(2) GG_PERIOD(3) GG_PERIOD(5) GG_PERIOD(7) GG_PERIOD(11)
        }
#undef GG_PERIOD
    });
}

// the plan and the arguments of a period conv's weight gradient on the flat axis; `strided`: the periodic variant
struct PbPlan : GgWPlan {
    bool strided;
    GgWArgs a;
};

static int period_wgrad_bf16_plan(int B, int Cin, int Cout, int H, int period, int k, int stride, PbPlan* p) {
    const char* who = "period_conv_weight_grad_bf16";
    if (int rc = period_wgrad_check(B, Cin, Cout, H, period, k, stride)) return rc;
    const int pad = (k - 1) / 2 * period;
    p->strided = stride > 1;
    if (!p->strided) {                                    // a dilated conv1d on [B, C, H p]
        if (int rc = dilated_wgrad_plan(B, Cin, Cout, H * period, k, period, pad, p, kBfTK)) return rc;
        p->a = gg_dilated_args(nullptr, nullptr, Cin, Cout, H * period, k, period, pad);
        return 0;
    }
    if (!period_wgrad_gemm_shape(Cin, Cout, k))
        return fail(FV_ERR_UNSUPPORTED, "%s: stride %d needs Cout >= 64 and Cin k >= 64 (Cin=%d Cout=%d k=%d); the fp32 "
                    "entry takes every shape", who, stride, Cin, Cout, k);
    const int64_t big = Cin > Cout ? Cin : Cout;
    if (big * ((int64_t)H + k) * period >= (int64_t)1 << 30)
        return fail(FV_ERR_INVALID_ARG, "%s: a map of %lld x %d x %d words is too long", who, (long long)big, H, period);
    const int Hout = (H - 1) / stride + 1;
    gg_wgrad_plan(B, Cout, (int64_t)Cin * k, Hout * period, Cout, p, kBfTK);
    GgWArgs a{};
    a.M = Cout;
    a.TR = Hout * period;
    a.Cb = Cin;
    a.TB = H * period;
    a.k = k;
    a.sB = stride;
    a.dB = period;
    a.pad = pad;
    a.Cbias = Cout;
    a.Tbias = a.TR;
    a.bias_scale = 1;
    p->a = a;
    return 0;
}

}  // namespace fv

using namespace fv;

extern "C" {

int64_t fv_conv1d_weight_grad_dilated_bf16_workspace_bytes(int B, int Cin, int Cout, int Tin, int k, int dil, int pad,
                                                           int pad_mode) {
    GgWPlan p;
    if (int rc = dilated_wgrad_plan(B, Cin, Cout, Tin, k, dil, pad, &p, kBfTK)) return rc;
    if (int rc = dilated_mode_check("conv1d_weight_grad_dilated_bf16", Tin, pad, pad_mode)) return rc;
    return (int64_t)p.bytes();
}

int fv_conv1d_weight_grad_dilated_bf16(const float* g_pre, const float* xa, float* dw, float* db, int B, int Cin,
                                       int Cout, int Tin, int k, int dil, int pad, int pad_mode, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    GgWPlan p;
    if (int rc = dilated_wgrad_plan(B, Cin, Cout, Tin, k, dil, pad, &p, kBfTK)) return rc;
    if (int rc = dilated_mode_check("conv1d_weight_grad_dilated_bf16", Tin, pad, pad_mode)) return rc;
    return gg_wgrad_bf16(p, gg_dilated_args(g_pre, xa, Cin, Cout, Tin, k, dil, pad), dw, db, workspace, workspace_bytes,
                         "conv1d_weight_grad_dilated_bf16", (hipStream_t)stream, pad_mode == FV_PAD_REFLECT);
}

int64_t fv_conv_transpose1d_weight_grad_bf16_workspace_bytes(int B, int Cin, int Cout, int Tin, int k, int stride,
                                                             int pad, int out_pad) {
    const int64_t Tout = convt_grad_check("conv_transpose1d_weight_grad_bf16", B, Cin, Cout, Tin, k, stride, pad, out_pad);
    if (Tout < 0) return Tout;
    GgWPlan p;
    gg_wgrad_plan(B, Cin, (int64_t)Cout * k, Tin, Cout, &p, kBfTK);
    return (int64_t)p.bytes();
}

int fv_conv_transpose1d_weight_grad_bf16(const float* g, const float* xa, float* dw, float* db, int B, int Cin, int Cout,
                                         int Tin, int k, int stride, int pad, int out_pad, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    const int64_t Tout = convt_grad_check("conv_transpose1d_weight_grad_bf16", B, Cin, Cout, Tin, k, stride, pad, out_pad);
    if (Tout < 0) return (int)Tout;
    GgWPlan p;
    gg_wgrad_plan(B, Cin, (int64_t)Cout * k, Tin, Cout, &p, kBfTK);
    return gg_wgrad_bf16(p, gg_convt_args(g, xa, Cin, Cout, Tin, (int)Tout, k, stride, pad), dw, db, workspace,
                         workspace_bytes, "conv_transpose1d_weight_grad_bf16", (hipStream_t)stream, false);
}

int64_t fv_period_conv_weight_grad_bf16_workspace_bytes(int B, int Cin, int Cout, int H, int period, int k, int stride) {
    PbPlan p;
    if (int rc = period_wgrad_bf16_plan(B, Cin, Cout, H, period, k, stride, &p)) return rc;
    return (int64_t)p.bytes();
}

int fv_period_conv_weight_grad_bf16(const float* g_pre, const float* x, float* dw, float* db, int B, int Cin, int Cout,
                                    int H, int period, int k, int stride, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    const char* who = "period_conv_weight_grad_bf16";
    PbPlan p;
    if (int rc = period_wgrad_bf16_plan(B, Cin, Cout, H, period, k, stride, &p)) return rc;
    p.a.a = p.a.bias_src = g_pre;
    p.a.b = x;
    if (p.strided) return gg_wgrad_bf16_period(p, p.a, dw, db, workspace, workspace_bytes, who, (hipStream_t)stream, period);
    return gg_wgrad_bf16(p, p.a, dw, db, workspace, workspace_bytes, who, (hipStream_t)stream, false);
}

}  // extern "C"
