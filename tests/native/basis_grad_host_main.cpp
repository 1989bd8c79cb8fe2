// Stand-alone check of the index arithmetic of the Basis-MelGAN head launchers (fastvocoder_amd/csrc/basis_grad_host.hpp):
// the tile walks of basis_head_grad_kernel and of the two L1 kernels, restated on the host over buffers of exactly the
// tensors' sizes, so that a host sanitizer (-fsanitize=address,undefined) sees every index the kernels form.  The
// results are compared with the defining sums.  Build and run: tests/test_basis_grad_host.py.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../fastvocoder_amd/csrc/basis_grad_host.hpp"

using namespace fv;

static unsigned rng_state = 12345u;
static float rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((int)(rng_state >> 9) % 2001 - 1000) / 500.f;
}

static int fails = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);             \
            ++fails;                                                              \
        }                                                                         \
    } while (0)

static void head_case(int B, int C, int F, int L) {
    EXPECT(basis_shape_check(B, C, F) == 0 && basis_L_check(L) == 0);
    const BasisHeadGeom g = basis_head_geom(C, F, L);
    EXPECT(g.lds_bytes <= 64 * 1024 && g.n == (int64_t)F * g.hop);
    std::vector<float> ge((size_t)B * g.n), gw((size_t)B * C * F), Y((size_t)(B + 1) * C * F), basis((size_t)L * C);
    std::vector<float> gY(Y.size(), NAN);
    for (float& v : ge) v = rnd();
    for (float& v : gw) v = rnd();
    for (float& v : Y) v = rnd();
    for (float& v : basis) v = rnd();
    for (unsigned by = 0; by < g.gy; ++by)
        for (unsigned bx = 0; bx < g.gx; ++bx) {
            std::vector<float> sb((size_t)L * kBhTC), sg((size_t)g.span);       // the block's LDS, exact sizes
            const int64_t f0 = (int64_t)bx * kBhTF, s0 = f0 * g.hop;
            const int c0 = (int)by * kBhTC;
            for (int i = 0; i < L * kBhTC; ++i) {
                const int c = c0 + i % kBhTC;
                sb[(size_t)i] = c < C ? basis[(size_t)(i / kBhTC) * C + c] : 0.f;
            }
            std::vector<float> sum((size_t)kBhThreads * kBhPer, 0.f);
            for (int b = 0; b <= B; ++b) {
                if (b < B)
                    for (int i = 0; i < g.span; ++i) sg[(size_t)i] = s0 + i < g.n ? ge[(size_t)b * g.n + s0 + i] : 0.f;
                for (int tid = 0; tid < kBhThreads; ++tid) {
                    const int lane = tid & 63, w = tid >> 6;
                    const int64_t f = f0 + lane;
                    float v[kBhPer] = {};
                    if (b < B)
                        for (int j = 0; j < L; ++j) {
                            const float s = sg[(size_t)basis_head_tap(lane, g.hop, j)];    // dead lanes read too
                            for (int i = 0; i < kBhPer; ++i) v[i] = fmaf(sb[(size_t)j * kBhTC + kBhPer * w + i], s, v[i]);
                        }
                    if (f >= F) continue;
                    for (int i = 0; i < kBhPer; ++i) {
                        const int c = c0 + kBhPer * w + i;
                        if (c >= C) break;
                        const size_t at = ((size_t)b * C + c) * F + f;
                        float& acc = sum[(size_t)tid * kBhPer + i];
                        if (b < B) {
                            const float gp = v[i] + gw[at];
                            acc += gp;
                            EXPECT(isnan(gY[at]));                                       // written exactly once
                            gY[at] = Y[at] > 0.f ? gp : 0.f;
                        } else {
                            EXPECT(isnan(gY[at]));
                            gY[at] = Y[at] > 0.f ? -acc : 0.f;
                        }
                    }
                }
            }
        }
    double worst = 0.0;
    for (int c = 0; c < C; ++c)
        for (int f = 0; f < F; ++f) {
            double total = 0.0;
            for (int b = 0; b < B; ++b) {
                double post = gw[((size_t)b * C + c) * F + f];
                for (int j = 0; j < L; ++j)
                    if ((int64_t)f * g.hop + j < g.n) post += (double)basis[(size_t)j * C + c] * ge[(size_t)b * g.n + (size_t)f * g.hop + j];
                total += post;
                const size_t at = ((size_t)b * C + c) * F + f;
                worst = fmax(worst, fabs((Y[at] > 0.f ? post : 0.0) - gY[at]));
            }
            const size_t at = ((size_t)B * C + c) * F + f;
            worst = fmax(worst, fabs((Y[at] > 0.f ? -total : 0.0) - gY[at]));
        }
    for (float v : gY) EXPECT(!isnan(v));
    EXPECT(worst <= 1e-3);
    printf("head B=%d C=%d F=%d L=%d: grid %u x %u, span %d, %zu bytes of LDS, worst %.2e\n", B, C, F, L, g.gx, g.gy, g.span,
           g.lds_bytes, worst);
}

static void l1_case(int B, int C, int F) {
    EXPECT(basis_shape_check(B, C, F) == 0);
    const BasisL1Geom g = basis_l1_geom(B, C, F);
    std::vector<float> D((size_t)B * C * F), tgt(D.size()), grad(D.size(), NAN);
    for (float& v : D) v = rnd();
    for (float& v : tgt) v = rnd();
    tgt[0] = D[0];                                                                  // one sign(0)
    std::vector<double> part((size_t)(2 * g.blocks), NAN);
    for (unsigned bz = 0; bz < g.gz; ++bz)
        for (unsigned by = 0; by < g.gy; ++by)
            for (unsigned bx = 0; bx < g.gx; ++bx) {
                std::vector<float> tile((size_t)kBlT * (kBlT + 1), 0.f), tile_t(tile.size(), 0.f);
                const int64_t b = bz, f0 = (int64_t)bx * kBlT;
                const int c0 = (int)by * kBlT;
                double sa = 0.0, sd = 0.0;
                for (int tid = 0; tid < kBhThreads; ++tid)
                    for (int i = 0; i < kBlPer; ++i) {
                        const int lane = tid & 63, r = (tid >> 6) + 4 * i;
                        const float v = (c0 + r < C && f0 + lane < F) ? D[(size_t)((b * C + c0 + r) * F + f0 + lane)] : 0.f;
                        tile[(size_t)r * (kBlT + 1) + lane] = v;                    // [channel][frame]
                        sd += v;
                        tile_t[(size_t)r * (kBlT + 1) + lane] =                     // [frame][channel]
                            (f0 + r < F && c0 + lane < C) ? tgt[(size_t)((b * F + f0 + r) * C + c0 + lane)] : 0.f;
                    }
                for (int tid = 0; tid < kBhThreads; ++tid)
                    for (int i = 0; i < kBlPer; ++i) {
                        const int lane = tid & 63, r = (tid >> 6) + 4 * i;
                        if (f0 + r < F && c0 + lane < C)
                            sa += fabsf(tile[(size_t)lane * (kBlT + 1) + r] - tgt[(size_t)((b * F + f0 + r) * C + c0 + lane)]);
                        if (c0 + r < C && f0 + lane < F) {
                            const size_t at = (size_t)((b * C + c0 + r) * F + f0 + lane);
                            const float d = D[at] - tile_t[(size_t)lane * (kBlT + 1) + r];
                            EXPECT(isnan(grad[at]));
                            grad[at] = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
                        }
                    }
                const int64_t at = ((int64_t)bz * g.gy + by) * g.gx + bx;
                EXPECT(at < g.blocks && isnan(part[(size_t)(2 * at)]));
                part[(size_t)(2 * at)] = sa;
                part[(size_t)(2 * at + 1)] = sd;
            }
    double ta = 0.0, td = 0.0;
    int64_t seen = 0;
    for (int t = 0; t < kBhThreads; ++t) {
        int64_t lo, hi;
        basis_l1_range(g.blocks, t, &lo, &hi);
        EXPECT(lo == seen || lo == g.blocks);
        for (int64_t i = lo; i < hi; ++i, ++seen) {
            ta += part[(size_t)(2 * i)];
            td += part[(size_t)(2 * i + 1)];
        }
    }
    EXPECT(seen == g.blocks);
    double wa = 0.0, wd = 0.0;
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c)
            for (int f = 0; f < F; ++f) {
                const float d = D[((size_t)b * C + c) * F + f] - tgt[((size_t)b * F + f) * C + c];
                wa += fabsf(d);
                wd += D[((size_t)b * C + c) * F + f];
                EXPECT(grad[((size_t)b * C + c) * F + f] == (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f));
            }
    EXPECT(grad[0] == 0.f);
    EXPECT(fabs(ta - wa) <= 1e-9 * g.count + 1e-12 && fabs(td - wd) <= 1e-9 * g.count + 1e-12);
    printf("l1 B=%d C=%d F=%d: grid %u x %u x %u, %lld records\n", B, C, F, g.gx, g.gy, g.gz, (long long)g.blocks);
}

int main() {
    EXPECT(basis_L_check(1) == 1 && basis_L_check(3) == 1 && basis_L_check(0) == 1 && basis_L_check(-2) == 1);
    EXPECT(basis_L_check(2) == 0 && basis_L_check(kBhMaxL) == 0 && basis_L_check(kBhMaxL + 2) == 2);
    EXPECT(basis_shape_check(0, 1, 1) == 1 && basis_shape_check(1, 0, 1) == 1 && basis_shape_check(1, 1, 0) == 1);
    EXPECT(basis_shape_check(65536, 1, 1) == 2 && basis_shape_check(1, 1, 1) == 0);
    EXPECT(basis_head_geom(256, 2240, kBhMaxL).lds_bytes <= 64 * 1024);
    const int shapes[][4] = {{1, 1, 1, 2},  {3, 1, 2, 2},   {1, 24, 17, 8}, {3, 32, 70, 30}, {1, 80, 2, 30},
                             {3, 17, 65, 8}, {1, 256, 1, 30}, {2, 33, 129, 30}};
    for (const auto& s : shapes) {
        head_case(s[0], s[1], s[2], s[3]);
        l1_case(s[0], s[1], s[2]);
    }
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("basis_grad_host ok\n");
    return 0;
}
