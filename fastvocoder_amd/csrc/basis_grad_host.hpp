// The index arithmetic of the Basis-MelGAN head launchers and kernels (basis_grad.hip), in plain C++: no HIP header, so
// a stand-alone program can compile this file with a host sanitizer (tests/native/basis_grad_host_main.cpp).  Shared
// with the device code, which calls these very functions: the shape checks, the two geometries, the staged sample a
// lane's tap reads (basis_head_tap) and the finish launch's ranges (basis_l1_range).  The tile loops around them
// (which thread owns which element) are restated by that program, not shared.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FV_BG_HD __host__ __device__
#else
#define FV_BG_HD
#endif

namespace fv {

constexpr int kBhThreads = 256;
constexpr int kBhTF = 64;        // frames of a head tile: one per lane of a wave
constexpr int kBhTC = 16;        // channels of a head tile: four per wave, contiguous
constexpr int kBhPer = kBhTC / (kBhThreads / 64);
constexpr int kBhMaxL = 256;     // (kBhTF + 1) L/2 + kBhTC L floats of LDS stay below 64 KiB
constexpr int kBlT = 64;         // the L1 kernels' square tile (frames x channels)
constexpr int kBlPer = kBlT / (kBhThreads / 64);

// 0: fine; 1: an argument no call may pass (FV_ERR_INVALID_ARG); 2: a shape these kernels are not built for
// (FV_ERR_UNSUPPORTED)
inline int basis_shape_check(int B, int C, int F) {
    if (B < 1 || C < 1 || F < 1) return 1;
    if (B > 65535 || ((int64_t)C + kBhTC - 1) / kBhTC > 65535) return 2;
    if (((int64_t)B + 1) * C * F >= (int64_t)1 << 40) return 2;
    return 0;
}

inline int basis_L_check(int L) {
    if (L < 2 || (L & 1)) return 1;
    return L > kBhMaxL ? 2 : 0;
}

struct BasisHeadGeom {
    unsigned gx, gy;     // frame tiles, channel tiles
    int hop, span;       // L/2; the staged samples of one tile and one batch row: (kBhTF + 1) hop
    int64_t n;           // samples of a row of g_est: F hop (the crop)
    size_t lds_bytes;    // the basis tile [L][kBhTC], then the samples [span]
};

inline BasisHeadGeom basis_head_geom(int C, int F, int L) {
    BasisHeadGeom g;
    g.gx = (unsigned)(((int64_t)F + kBhTF - 1) / kBhTF);             // F may be close to 2^31: no int additions
    g.gy = (unsigned)(((int64_t)C + kBhTC - 1) / kBhTC);
    g.hop = L / 2;
    g.span = (kBhTF + 1) * g.hop;
    g.n = (int64_t)F * g.hop;
    g.lds_bytes = sizeof(float) * ((size_t)L * kBhTC + (size_t)g.span);
    return g;
}

// the staged sample a lane's tap reads: frame `lane` of the tile, tap j < L -- always below span
FV_BG_HD inline int basis_head_tap(int lane, int hop, int j) { return lane * hop + j; }

struct BasisL1Geom {
    unsigned gx, gy, gz;     // frame tiles, channel tiles, batch rows
    int64_t blocks;          // partial records (two doubles each)
    double count;            // B C F: the mean's divisor
};

inline BasisL1Geom basis_l1_geom(int B, int C, int F) {
    BasisL1Geom g;
    g.gx = (unsigned)(((int64_t)F + kBlT - 1) / kBlT);
    g.gy = (unsigned)(((int64_t)C + kBlT - 1) / kBlT);
    g.gz = (unsigned)B;
    g.blocks = (int64_t)g.gx * g.gy * g.gz;
    g.count = (double)B * (double)C * (double)F;
    return g;
}

// the finalise launch: thread t of kBhThreads adds the records [lo, hi) in ascending order
FV_BG_HD inline void basis_l1_range(int64_t blocks, int t, int64_t* lo, int64_t* hi) {
    const int64_t per = (blocks + kBhThreads - 1) / kBhThreads;
    *lo = (int64_t)t * per < blocks ? (int64_t)t * per : blocks;
    *hi = *lo + per < blocks ? *lo + per : blocks;
}

}  // namespace fv
