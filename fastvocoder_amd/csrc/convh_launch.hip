// Host side of the split-f16 wide-channel conv kernels (convh_kernels.hpp): validation, tile geometry, LDS layout,
// persistent grid, launch.  Device code: convh_inst_c64.hip / convh_inst_c128.hip.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <mutex>
#include <vector>

#include "launch_host.hpp"

namespace fv {

extern template int launch_convh_geom<4, 2>(const PairParams&, int, size_t, hipStream_t);
extern template int launch_convh_geom<2, 2>(const PairParams&, int, size_t, hipStream_t);


// ---- block schedule for launches with few items per block ----------------------------------------------------
// The kernels' own partition cuts the cost-weighted item sequence into nblk contiguous shares: with 1-3 items per
// block and items of three different costs, a share ends up anywhere between one cheap item and two expensive ones
// (HiFi-GAN light at batch 1, 128 channels: 126 items each of cost 24 / 16 / 8 on 256 blocks -- makespan 32 against a
// mean of 23.6).  Items of one member are interchangeable, so a greedy longest-processing-time-first assignment
// (most expensive member first, every item to the block that finishes it earliest; taking up a second member costs
// a pipeline refill) is computed once per shape on the host and handed to the kernel as per-block item ranges.
// [measured, MI355X, B = 1] the two-member launches at the end of a stage (11 + 7 taps: every block ends up with ONE
// member) 56.7 -> 47.7 us at 128 channels, 49.7 -> 47.0 at 64; three-member launches gain nothing (128 channels:
// a 7-tap + 3-tap block pays a member switch, a pipeline drain and refill, for what it saves) or lose (64 channels,
// 58 vs 55 us: more switches than the contiguous cut has), so they keep the contiguous cut (FV_SCHED=2: all).
// (three_members: the kernel wants its three-member launches scheduled too -- the fused 128-channel pairs, whose tiles
// are long enough for the balance to show: 191 -> 170 us over the four launches of a stage; Tuning::sched = 2: all)
void pair_schedule(PairParams& p, int nblk, bool three_members) {
    typedef std::array<unsigned, 2 * kSchedBlocks> Table;
    static std::mutex mu;
    static std::map<std::array<int, 9>, Table> cache;           // host memory only; a process sees a handful of shapes
    p.sched_on = 0;
    const Tuning& tn = tuning();
    if (tn.sched == 0) return;
    long long items = 0;
    for (int m = 0; m < p.n_members; ++m) items += p.m[m].n_items;
    if (p.n_members < 2 || nblk < 2 || nblk > kSchedBlocks || items > 6LL * nblk) return;
    if (p.n_members != 2 && tn.sched != 2 && !three_members) return;
    for (int m = 0; m < p.n_members; ++m)
        if (p.m[m].n_items > 2047) return;                       // 11-bit item numbers
    const int sw = tn.sched_switch;
    std::array<int, 9> key = {nblk, p.n_members, sw, 0, 0, 0, 0, 0, 0};
    for (int m = 0; m < p.n_members; ++m) {
        key[3 + 2 * m] = p.m[m].n_items;
        key[4 + 2 * m] = p.m[m].cost;
    }
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it == cache.end()) {
        if (cache.size() >= 256) return;
        int order[3] = {0, 1, 2};
        for (int i = 0; i < p.n_members; ++i)
            for (int j = i + 1; j < p.n_members; ++j)
                if (p.m[order[j]].cost > p.m[order[i]].cost) std::swap(order[i], order[j]);
        std::vector<long long> load(nblk, 0);
        std::vector<int> cnt((size_t)nblk * 3, 0);
        for (int oi = 0; oi < p.n_members; ++oi) {
            const int m = order[oi], c = p.m[m].cost;
            for (int i = 0; i < p.m[m].n_items; ++i) {
                int best = 0;
                long long best_end = -1;
                for (int b = 0; b < nblk; ++b) {
                    const long long end = load[b] + c + (cnt[(size_t)b * 3 + m] == 0 && load[b] > 0 ? sw : 0);
                    if (best_end < 0 || end < best_end) {
                        best_end = end;
                        best = b;
                    }
                }
                load[best] = best_end;
                ++cnt[(size_t)best * 3 + m];
            }
        }
        Table t = {};
        bool fits = true;
        int at[3] = {0, 0, 0};
        for (int b = 0; b < nblk; ++b) {
            unsigned e[3] = {0, 0, 0};
            for (int m = 0; m < p.n_members; ++m) {
                const int c = cnt[(size_t)b * 3 + m];
                if (c > 31) fits = false;                        // 5-bit counts
                e[m] = (unsigned)at[m] | ((unsigned)c << 11);
                at[m] += c;
            }
            t[2 * b] = e[0] | (e[1] << 16);
            t[2 * b + 1] = e[2];
        }
        if (!fits) return;
        it = cache.emplace(key, t).first;
    }
    memcpy(p.sched, it->second.data(), sizeof(unsigned) * 2 * (size_t)nblk);
    p.sched_on = 1;
}

// pair_kernels.hpp pair_share on the host (the same integers)
static long long host_share(long long blk, long long total, long long base, int cost, long long n, int nblk) {
    const long long num = blk * total - base * nblk;
    if (num <= 0) return 0;
    const long long den = (long long)cost * nblk;
    const long long j = (num + den - 1) / den;
    return j > n ? n : j;
}

void pair_cut_schedule(PairParams& p, int nblk, const long long* n) {
    if (nblk < 1 || nblk > 2 * kSchedBlocks) return;
    long long total = 0, items = 0;
    for (int m = 0; m < p.n_members; ++m) {
        total += n[m] * p.m[m].cost;
        items += n[m];
    }
    if (items >= (1LL << 31)) return;
    // The table depends on (shares, item counts, costs) only: a forward asks for the same handful of tables call after call
    // (nblk x members divisions each, ~5 us of host time per launch) -- kept per shape, as pair_schedule's are.
    typedef std::array<long long, 8> Key;
    typedef std::array<unsigned, 2 * kSchedBlocks> Table;
    static std::mutex mu;
    static std::map<Key, Table> cache;
    Key key = {nblk, p.n_members, 0, 0, 0, 0, 0, 0};
    for (int m = 0; m < p.n_members; ++m) {
        key[2 + 2 * m] = n[m];
        key[3 + 2 * m] = p.m[m].cost;
    }
    {
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find(key);
        if (it == cache.end()) {
            Table t = {};
            for (int i = 0; i < nblk; ++i) {
                long long g = 0, base = 0;
                for (int m = 0; m < p.n_members; ++m) {
                    g += host_share(i, total, base, p.m[m].cost, n[m], nblk);
                    base += n[m] * p.m[m].cost;
                }
                t[i] = (unsigned)g;
            }
            if (cache.size() >= 512) cache.clear();
            it = cache.emplace(key, t).first;
        }
        memcpy(p.sched, it->second.data(), sizeof(unsigned) * (size_t)nblk);
    }
    p.sched_on = 2;
}

// run-time mirror of ConvHGeom<>
ConvHShape convh_shape(int C, int k, int dil) {
    ConvHShape g = {};
    g.NCH = C > 128 ? C / 128 : 1;     // the image holds at most 128 input channels at a time
    g.NMT = C / 64;
    C = C > 128 ? 128 : C;             // ... everything below is per chunk
    g.CG = C / 32;
    g.NFW = 2;
    g.NTC = 16 * g.NFW * 4;
    g.NSTEP = k * g.CG;
    g.NST = g.NSTEP / 2;
    g.XROWS = (g.NTC + (k - 1) * dil + 3) / 4 * 4;
    g.XIMG = 4 * C * ((g.XROWS + 15) / 16 * 16);
    return g;
}

int launch_convh(PairParams p, int C, int dil, hipStream_t s) {
    const char* const fam = "split-f16 conv";
    if (p.B <= 0 || p.T <= 0) return 0;
    if (C != 64 && C != 128 && C != 256 && C != 512)
        return fail(FV_ERR_UNSUPPORTED, "split-f16 conv: C = %d (64, 128, 256 or 512)", C);
    if (dil != 1 && dil != 3 && dil != 5 && dil != 9)
        return fail(FV_ERR_UNSUPPORTED, "split-f16 conv: dilation %d (1, 3, 5; 9 with 3 taps)", dil);
    if (int rc = check_launch(fam, p, C)) return rc;
    int img_bytes = 0;
    Work work = {0, 0};
    long long items = 0;
    const int cus = device_cu_count();
    // 128 channels and more: 128-row tiles (convs_kernel, convr_kernels.hpp -- a chunk's window is converted once for
    // both 64-row tiles) when the launch has items enough for the chip that way (as launch_convg); Tuning::convh_rows64
    const long long w128 = C >= 128 ? (long long)p.n_members * ((p.T + 127) / 128) * p.B * (C / 128) : 0;     // such items
    const bool wide = C >= 128 && (tuning().convh_rows64 < 0 ? w128 * 10 >= 7LL * cus : !tuning().convh_rows64);
    // 256 / 512 channels with items enough: the ring-free form (convs2_kernels.hpp: 128 rows x 64 columns, every wave loads the A
    // operands of its own sixteen rows L2 -> registers; no reflection padding, dilations 1 / 3 / 5) -- Tuning::convs_ringfree
    const bool ringfree = wide && C >= 256 && !p.reflect && dil <= 5 && tuning().convs_ringfree != 0;
    int rf_nh = 1;                     // 128-column tiles (32 x 64 wave tiles) when they still give every CU four items
    if (ringfree) {
        rf_nh = tuning().convs_ringfree > 0 ? tuning().convs_ringfree : (w128 >= 4LL * cus ? 2 : 1);
        if (rf_nh != 1 && rf_nh != 2) rf_nh = 1;
    }
    const int rf_cols = 64 * rf_nh;
    for (int i = 0; i < p.n_members; ++i) {
        PairMember& mb = p.m[i];
        if (int rc = check_taps(fam, mb.k)) return rc;
        if (dil == 9 && mb.k != 3) return fail(FV_ERR_UNSUPPORTED, "split-f16 conv: dilation 9 with %d taps (3 only)", mb.k);
        if (p.reflect)
            if (int rc = check_reflect(fam, (mb.k - 1) / 2 * dil, p.T)) return rc;
        if (int rc = check_member(fam, mb, i, kNeedY)) return rc;
        const ConvHShape g = convh_shape(C, mb.k, dil);
        mb.n_tiles = ringfree ? (p.T + rf_cols - 1) / rf_cols : (p.T + g.NTC - 1) / g.NTC;
        mb.n_items = mb.n_tiles * p.B * (wide ? g.NMT / 2 : g.NMT);
        p.ctot = C;
        p.nch = g.NCH;
        p.nmt = g.NMT;
        // a tile costs its stages (LDS / matrix time) plus loads, conversion, epilogue
        mb.cost = g.NST * g.NCH + (tuning().convh_skel >= 0 ? tuning().convh_skel : (C == 64 ? 5 : 2));
        if (ringfree) {
            const int xrows = (rf_cols + (mb.k - 1) * dil + 3) / 4 * 4;
            const int ximg = 4 * 128 * ((xrows + 15) / 16 * 16);
            if (ximg > img_bytes) img_bytes = ximg;
        } else if (g.XIMG > img_bytes) img_bytes = g.XIMG;
        items += mb.n_items;
        work.flops += 2.0 * p.B * (double)C * C * mb.k * p.T;
        work.bytes += 4.0 * ((double)C * C * mb.k + (double)p.B * C * p.T *
                             (2 + (mb.res ? 1 : 0) + (mb.add1 ? 1 : 0) + (mb.add2 ? 1 : 0) + (mb.y_act ? 1 : 0)));
    }
    LdsLayout lds;
    p.x_off = 0;
    if (!ringfree) lds.add(4 * 16384 / 4);          // ring of 4 weight stages
    p.img_off = lds.add((size_t)img_bytes / 4);
    p.bias_off = 0;                                 // (biases are read from global memory in the epilogue)
    if (ringfree) lds.add(64);                      // the low-side guard's scratch
    if (int rc = check_lds(fam, lds.bytes())) return rc;
    p.nblk = (int)persistent_blocks(items, 1, tuning().convh_blocks);       // one 8-wave block per CU
    if (ringfree) p.sched_on = 0;
    else pair_schedule(p, p.nblk);
    if (!p.sched_on) cut_table(p, p.nblk);          // no per-block schedule: the kernels' contiguous cut, as a table instead of arithmetic
    set_debug(p);
    ProfileScope prof(s, C == 64 ? FV_KERNEL_CONVH64 : FV_KERNEL_CONVH128, work);
    return ringfree ? launch_convs2_geom(p, dil, rf_nh, lds.bytes(), s) : wide ? launch_convs_geom(p, dil, lds.bytes(), s)
         : C >= 128 ? launch_convh_geom<4, 2>(p, dil, lds.bytes(), s) : launch_convh_geom<2, 2>(p, dil, lds.bytes(), s);
}

// ---- ConvTranspose1d, kernel = 2 x stride (convt_kernel) -----------------------------------------------------------
int launch_convt(PairParams p, int Cin, int Cout, int stride, int pad, int Tout, hipStream_t s) {
    const char* const fam = "split-f16 transposed conv";
    if (p.B <= 0 || p.T <= 0 || Tout <= 0) return 0;
    if (Cin != 32 && Cin != 64 && Cin != 128 && Cin != 256 && Cin != 512)
        return fail(FV_ERR_UNSUPPORTED, "split-f16 transposed conv: Cin = %d (32, 64, 128, 256 or 512)", Cin);
    if (stride < 2 || stride > 16 || Cout <= 0 || Cout * stride < 32)
        return fail(FV_ERR_UNSUPPORTED, "split-f16 transposed conv: stride %d (2..16), Cout * stride = %d (32 or more)",
                    stride, Cout * stride);
    if (pad < 0 || pad > stride) return fail(FV_ERR_UNSUPPORTED, "split-f16 transposed conv: padding %d (0..stride)", pad);
    if (int rc = check_desc_range(fam, Cin, p.T, false)) return rc;
    if (int rc = check_desc_range(fam, Cout, Tout, false)) return rc;
    if (int rc = check_slopes(fam, p.slope, p.act_slope)) return rc;
    PairMember& mb = p.m[0];
    if (int rc = check_tensors(fam, mb, -1, kNeedY)) return rc;
    if (int rc = check_aligned(fam, mb, 0)) return rc;
    p.n_members = 1;
    p.ctot = Cin;
    const int cc = Cin <= 64 ? 64 : 128;      // input channels per chunk (64 input channels: one chunk of 64, two K steps per tap;
                                              // 32: half of that chunk -- the missing channels read as zeros)
    p.nch = (Cin + cc - 1) / cc;
    p.nmt = (Cout * stride + 63) / 64;        // rows beyond Cout * stride: zero weights, stores dropped
    p.cout = Cout;
    p.ups = stride;
    p.pad_t = pad;
    p.Tout = Tout;
    p.reflect = 0;
    const int ncols = (Tout + pad + stride - 1) / stride;          // u = (n + pad) / stride of the last sample, + 1
    mb.k = 2;
    // The form: which kernel, its tiles and items (and, for the ring pipeline, its LDS); one tail launches it.
    enum { kLean, kResident, kRing } form;
    const int cus = device_cu_count();
    const int NTC = 128;
    const int ring_tiles = (ncols + NTC - 1) / NTC;
    const long long lean_items = (long long)((ncols + 63) / 64) * p.B * p.nmt, column_items = (long long)ring_tiles * p.B;
    const int resident = tuning().convu_resident;
    long long items;
    bool wide = false;
    LdsLayout lds;
    if (tuning().convt_lean > 0 && lean_items * p.nch * 10 <= (long long)tuning().convt_lean * cus) {
        // Few items: the lean kernel (convtl_kernels.hpp: 64-column tiles, A operands L2 -> registers, no ring) -- a launch of a
        // handful of tiles per CU is all prologue on the ring pipeline below.  Tuning::convt_lean: (64 x 64 item, chunk) units per CU
        // (in tenths) up to which it runs; 0: never (A/B, bit-identity tests).  [measured, tools/convt_lean_bench.py, hot loop]
        // 256 -> 128 x 8 at 1000 frames (2 units per CU): 10.6 against 15.6 us; 512 -> 256 x 8 at 200 frames (2): 15.2 / 23.6;
        // 64 -> 32 x 3 at 40 000 (4.9): 17.5 / 19.6; 128 -> 64 x 5 at 8000 (2.5): 15.9 / 17.0; at 3.3 units the two are equal, from
        // ~8 up the ring pipeline wins (batch 16: 74 against 107 us) -- its weights reach all eight waves through LDS once.
        form = kLean;
        mb.n_tiles = (ncols + 63) / 64;
        items = lean_items;
    } else if (cc == 128 && p.nch <= 2 && p.nmt * 64 <= 1024 && !mb.add1 && resident != 0 && (resident == 2 || column_items >= 2LL * cus)) {
        // Many items, 128 / 256 input channels, no merged input: an item is a column tile with ALL its rows on resident images
        // (convu2_kernels.hpp) -- convu_kernel below converts every window once per PAIR of 64-row tiles.  Tuning::convu_resident
        form = kResident;
        mb.n_tiles = ring_tiles;
        items = column_items;
    } else {
        // The ring pipeline.  128 and more input channels: 128-row tiles (convu_kernel, convr_kernels.hpp) when that still gives
        // the chip items enough, as launch_convg / launch_convh; Tuning::convt_rows64
        // (a merged input -- mb.add1: the upsampler behind an MRF stage forms ((x + add1) + add2) / out_div in its window loader --
        // exists on the 64-row kernel only: the 128-row one has no registers left for the second window)
        form = kRing;
        mb.n_tiles = ring_tiles;
        const long long wide_items = (long long)mb.n_tiles * p.B * ((p.nmt + 1) / 2);
        wide = cc == 128 && !mb.add1 && (tuning().convt_rows64 < 0 ? wide_items * 10 >= 7LL * cus : !tuning().convt_rows64);
        items = wide ? wide_items : mb.n_tiles * p.B * p.nmt;
        const int xrows = (NTC + 1 + 3) / 4 * 4;
        p.x_off = lds.add(4 * 16384 / 4);          // ring of 4 weight stages
        p.img_off = lds.add((size_t)(4 * cc * ((xrows + 15) / 16 * 16)) / 4);
    }
    if (!mb.add1) p.out_div = 1.f;
    if (form != kResident)             // (the resident kernel has no merged input and reads neither)
        if (int rc = check_adds(fam, mb.add1, mb.add2)) return rc;
    mb.n_items = (int)items;
    mb.cost = 1;
    p.nblk = (int)persistent_blocks(items, 1, tuning().convh_blocks);
    p.sched_on = 0;
    set_debug(p, form == kRing, form != kResident);
    ProfileScope prof(s, FV_KERNEL_CONVT, convt_work(p.B, p.T, Tout, Cin, Cout, 2 * stride, 1, mb.y_act != nullptr));
    return form == kLean ? launch_convtl_geom(p, cc / 32, s) : form == kResident ? launch_convu2_geom(p, p.nch, s)
         : wide ? launch_convu_geom(p, lds.bytes(), s) : launch_convt_geom(p, cc / 32, lds.bytes(), s);
}

// ---- two-source 1x1 conv (convg_kernel) -----------------------------------------------------------------------------
int launch_convg(PairParams p, int C, hipStream_t s) {
    const char* const fam = "split-f16 two-source 1x1 conv";
    if (p.B <= 0 || p.T <= 0) return 0;
    if (C != 128 && C != 256 && C != 512)
        return fail(FV_ERR_UNSUPPORTED, "split-f16 two-source 1x1 conv: C = %d (128, 256 or 512)", C);
    if (int rc = check_desc_range(fam, C, p.T)) return rc;
    if (int rc = check_slopes(fam, p.slope, p.act_slope)) return rc;
    PairMember& mb = p.m[0];
    if (int rc = check_tensors(fam, mb, -1, kNeedX2 | kNeedY)) return rc;
    if (int rc = check_aligned(fam, mb, 0)) return rc;
    p.n_members = 1;
    p.ctot = C;                                // channels of each input and of the output
    p.nch = 2 * C / 128;                       // chunks of 128 input channels: x's, then x2's
    p.nmt = C / 64;
    p.reflect = 0;
    p.out_div = 1.f;
    const int NTC = 128;
    mb.k = 1;
    mb.n_tiles = (p.T + NTC - 1) / NTC;
    // 128 output rows per item (convr_kernels.hpp: a converted chunk of the inputs feeds two 64-row tiles), or 64
    // (convg_kernel; Tuning::convg_rows64, A/B and bit-identity tests)
    // [measured, MI355X] Basis-MelGAN light, 64 utterances: 16.3 -> 14.0 ms per step on 128-row tiles; MelGAN, one
    // utterance of 200 frames (13 - 100 column tiles per launch): 0.44 -> 0.47 ms -- with fewer items than CUs the
    // 64-row tiles keep more of the chip busy.  -1: by the item count.
    const bool wide = tuning().convg_rows64 < 0 ? (long long)mb.n_tiles * p.B * (p.nmt / 2) * 10 >= 7LL * device_cu_count()
                                                : !tuning().convg_rows64;
    mb.n_items = mb.n_tiles * p.B * (wide ? p.nmt / 2 : p.nmt);
    mb.cost = 1;
    LdsLayout lds;
    p.x_off = lds.add(4 * 16384 / 4);          // ring of 4 weight stages
    p.img_off = lds.add(4 * 128 * 128 / 4);    // image: 128 channels x 128 rows x (2 + 2) bytes
    p.nblk = (int)persistent_blocks(mb.n_items, 1, tuning().convh_blocks);
    p.sched_on = 0;
    set_debug(p);
    ProfileScope prof(s, FV_KERNEL_CONVG, Work{2.0 * p.B * (double)C * 2 * C * p.T,
                                               4.0 * (2.0 * C * C + (double)p.B * C * p.T * (3 + (mb.res ? 1 : 0) + (mb.y_act ? 1 : 0)))});
    return wide ? launch_convr_geom(p, lds.bytes(), s) : launch_convg_geom(p, lds.bytes(), s);
}

// ---- fused pairs at C = 64 and C = 128 (convq2_kernels.hpp) ----------------------------------------------------------
constexpr int kPair64Wide = 65, kPair128Wide = 129;     // (convq2_kernels.hpp: the wide forms of the ring-free pair kernel)
constexpr int kPair128Col80 = 130;                      // (... the 11-tap member on 80-column tiles)
template <int DIL, int C>
int launch_convq2_dil(const PairParams& p, size_t lds, hipStream_t s);      // convq2_inst.hip: the pairs without the weight ring
extern template int launch_convq2_dil<1, 128>(const PairParams&, size_t, hipStream_t);
extern template int launch_convq2_dil<3, 128>(const PairParams&, size_t, hipStream_t);
extern template int launch_convq2_dil<5, 128>(const PairParams&, size_t, hipStream_t);
extern template int launch_convq2_dil<1, 64>(const PairParams&, size_t, hipStream_t);
extern template int launch_convq2_dil<3, 64>(const PairParams&, size_t, hipStream_t);
extern template int launch_convq2_dil<5, 64>(const PairParams&, size_t, hipStream_t);
extern template int launch_convq2_dil<1, kPair64Wide>(const PairParams&, size_t, hipStream_t);
extern template int launch_convq2_dil<3, kPair64Wide>(const PairParams&, size_t, hipStream_t);
extern template int launch_convq2_dil<5, kPair64Wide>(const PairParams&, size_t, hipStream_t);
extern template int launch_convq2_dil<1, kPair128Wide>(const PairParams&, size_t, hipStream_t);
extern template int launch_convq2_dil<3, kPair128Wide>(const PairParams&, size_t, hipStream_t);
extern template int launch_convq2_dil<1, kPair128Col80>(const PairParams&, size_t, hipStream_t);
extern template int launch_convq2_dil<3, kPair128Col80>(const PairParams&, size_t, hipStream_t);
extern template int launch_convq2_dil<5, kPair128Col80>(const PairParams&, size_t, hipStream_t);

// Long runs of the fused 64- / 128-channel pairs (many tiles per block) are mostly WARM tiles -- NM outputs
// for the work a cold tile spends on NM - (k - 1) (convq2_kernels.hpp) -- so an ITEM (NM - (k - 1) columns) of an 11-tap
// member costs 84 % of a tile there, one of a 3-tap member 97 %: the members' partition weights follow, or the blocks that
// walk the 3-tap member finish last [measured, 128 channels, 16 x 64 000 columns, three members: 4.76 ms with equal
// tile costs whatever the tiling, against 3.50 vs 3.87 ms for the two-member launch]
#ifndef FV_WARM_TILES
#define FV_WARM_TILES 1
#endif
// (mixed: the members' tiles differ in width -- an item's share of a warm tile is nout / nm of it: in 1 / 320, 64 and 80 both
// divide it)
static void warm_run_costs(PairParams& p, long long items, const int* nm, bool mixed) {
    if (!FV_WARM_TILES || items < 8LL * p.nblk) return;
    for (int i = 0; i < p.n_members; ++i) p.m[i].cost *= (nm[i] - (p.m[i].k - 1)) * (mixed ? 320 / nm[i] : 1);
}

// What differs between the two channel counts of the fused pair.  Both run convq2_kernel (A operands from L2 into registers) on
// narrow tiles, and on wide ones (32 x 64 wave tiles) from Tuning::*wide_from tenths of a wide tile per CU up -- at 128 channels
// only where both images fit without the ring: dilation 1 and 3.
struct FusedPair {
    int C;
    int narrow, wide;              // intermediate columns per tile of the two forms
    int Tuning::*wide_from;
    int wide_dil;                  // the largest dilation the wide form exists for
    int Tuning::*skel;             // the per-tile constant of a tile's cost, in K steps of one conv ...
    int skel_auto;                 // ... its value when the key is negative (0: the key as it is)
    bool three_members;            // pair_schedule: three-member launches get the block schedule too
    int kind;
};
static const FusedPair kFusedPair64 = {64, 128, 256, &Tuning::convp_wide, 5, &Tuning::convp_skel, 0, false, FV_KERNEL_CONVH64};
static const FusedPair kFusedPair128 = {128, 64, 128, &Tuning::convq_wide, 3, &Tuning::convq_skel, 5, true, FV_KERNEL_CONVH128};

static int fused_pair_skel(const FusedPair& f) { return f.skel_auto && tuning().*f.skel < 0 ? f.skel_auto : tuning().*f.skel; }

// items, costs and pair_schedule's makespan of a 128-channel launch whose 11-tap member runs on nm11 columns
static PairWidthPlan pair_width_candidate(int B, int T, int n_members, const int* taps, int blocks, int nm11) {
    const Tuning& tn = tuning();
    PairWidthPlan pl = {};
    PairParams p = {};
    p.n_members = n_members;
    long long items = 0;
    for (int m = 0; m < n_members; ++m) {
        const int nm = taps[m] == 11 ? nm11 : 64, nout = nm - (taps[m] - 1);
        pl.nm[m] = nm;
        pl.n_tiles[m] = (T + nout - 1) / nout;
        pl.n_items[m] = pl.n_tiles[m] * B;
        pl.cost[m] = nm == 80 && tn.convq_cost80 > 0 ? tn.convq_cost80 : 128 / 32 * taps[m] * nm / 64 + fused_pair_skel(kFusedPair128);
        p.m[m].n_items = pl.n_items[m];
        p.m[m].cost = pl.cost[m];
        items += pl.n_items[m];
    }
    pl.nblk = (int)std::min<long long>(blocks, items);
    pl.makespan = -1;
    pair_schedule(p, pl.nblk, kFusedPair128.three_members);
    if (p.sched_on != 1) return pl;
    for (int b = 0; b < pl.nblk; ++b) {
        const int cnt[3] = {(int)((p.sched[2 * b] >> 11) & 31u), (int)(p.sched[2 * b] >> 27), (int)((p.sched[2 * b + 1] >> 11) & 31u)};
        long long load = 0;
        for (int m = 0; m < n_members; ++m)
            if (cnt[m]) load += (long long)cnt[m] * pl.cost[m] + (load > 0 ? tn.sched_switch : 0);
        pl.makespan = std::max(pl.makespan, load);
    }
    return pl;
}

PairWidthPlan pair_width_plan(int B, int T, int n_members, const int* taps, int blocks) {
    const Tuning& tn = tuning();
    typedef std::array<int, 13> Key;
    static std::mutex mu;
    static std::map<Key, PairWidthPlan> cache;
    Key key = {B, T, n_members, 0, 0, 0, blocks, tn.convq_nm11, tn.convq_cost80, fused_pair_skel(kFusedPair128), tn.sched, tn.sched_switch, 0};
    bool has11 = false;
    for (int m = 0; m < n_members; ++m) {
        key[3 + m] = taps[m];
        has11 = has11 || taps[m] == 11;
    }
    {
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find(key);
        if (it != cache.end()) return it->second;
    }
    PairWidthPlan pl = pair_width_candidate(B, T, n_members, taps, blocks, has11 && tn.convq_nm11 == 80 ? 80 : 64);
    if (has11 && tn.convq_nm11 != 64 && tn.convq_nm11 != 80 && pl.makespan >= 0) {
        const PairWidthPlan w = pair_width_candidate(B, T, n_members, taps, blocks, 80);
        if (w.makespan >= 0 && w.makespan < pl.makespan) pl = w;
    }
    std::lock_guard<std::mutex> lock(mu);
    if (cache.size() >= 512) cache.clear();
    cache.emplace(key, pl);
    return pl;
}

static int launch_fused_pair(const FusedPair& f, PairParams& p, int dil, hipStream_t s) {
    const char* const fam = "resblock pair";
    const int C = f.C;
    if (p.B <= 0 || p.T <= 0) return 0;
    if (dil != 1 && dil != 3 && dil != 5) return fail(FV_ERR_UNSUPPORTED, "resblock pair: dilation %d (1, 3 or 5)", dil);
    if (int rc = check_launch(fam, p, C)) return rc;
    sort_members_by_taps(p);
    long long wide_items = 0;          // (a wide tile advances by wide - (k - 1) columns)
    for (int i = 0; i < p.n_members; ++i) wide_items += (long long)p.B * ((p.T + f.wide - p.m[i].k) / (f.wide + 1 - p.m[i].k));
    const bool wide = dil <= f.wide_dil && wide_items * 10 >= (long long)(tuning().*f.wide_from) * device_cu_count();
    const int skel = fused_pair_skel(f);
    for (int i = 0; i < p.n_members; ++i)
        if (int rc = check_taps(fam, p.m[i].k)) return rc;
    // columns per tile and cost of a tile, per member: one width for all, but for the 11-tap member of a 128-channel launch on
    // narrow tiles (pair_width_plan)
    int nm[3], cost[3];
    for (int i = 0; i < p.n_members; ++i) {
        nm[i] = wide ? f.wide : f.narrow;
        cost[i] = C / 32 * p.m[i].k + skel;        // K steps of one conv + per-tile work
    }
    if (C == 128 && !wide) {
        int taps[3] = {0, 0, 0};
        for (int i = 0; i < p.n_members; ++i) taps[i] = p.m[i].k;
        const PairWidthPlan pl = pair_width_plan(p.B, p.T, p.n_members, taps, (int)persistent_blocks(1LL << 40, 1, tuning().convh_blocks));
        for (int i = 0; i < p.n_members; ++i) {
            nm[i] = pl.nm[i];
            cost[i] = pl.cost[i];
        }
    }
    const bool col80 = nm[0] == 80;
    int img_bytes = 0, nm_max = 0;
    long long items = 0;
    for (int i = 0; i < p.n_members; ++i) {
        PairMember& mb = p.m[i];
        if (int rc = check_member(fam, mb, i, kNeedW2 | kNeedY)) return rc;
        const int nout = nm[i] - (mb.k - 1);
        mb.n_tiles = (p.T + nout - 1) / nout;
        mb.n_items = mb.n_tiles * p.B;
        mb.cost = cost[i];
        const int xrows = (nm[i] + (mb.k - 1) * dil + 3) / 4 * 4;
        const int img = 4 * C * ((xrows + 15) / 16 * 16);
        if (img > img_bytes) img_bytes = img;      // both images: sized for the largest member
        if (nm[i] > nm_max) nm_max = nm[i];
        items += mb.n_items;
    }
    LdsLayout lds;
    p.x_off = 0;
    p.img_off = lds.add((size_t)img_bytes / 4);
    p.mid_off = lds.add((size_t)4 * C * (nm_max + 16) / 4);
    p.bias_off = lds.add(4 * (size_t)C + 16);      // [b1 | b2 | inverse row prescales of conv1 | conv2 | scratch of the low-range guard]
    if (int rc = check_lds(fam, lds.bytes())) return rc;
    p.nblk = (int)persistent_blocks(items, 1, tuning().convh_blocks);
    pair_schedule(p, p.nblk, f.three_members);
    if (!p.sched_on) {                 // no per-block schedule: the kernels' contiguous cut, as a table instead of arithmetic
        warm_run_costs(p, items, nm, col80);
        cut_table(p, p.nblk);
    }
    set_debug(p);
    ProfileScope prof(s, f.kind, pair_work(p, C));
    const size_t bytes = lds.bytes();
    if (C == 64)
        return wide ? by_dilation<1, 3, 5>(dil, [&](auto d) { return launch_convq2_dil<decltype(d)::value, kPair64Wide>(p, bytes, s); })
                    : by_dilation<1, 3, 5>(dil, [&](auto d) { return launch_convq2_dil<decltype(d)::value, 64>(p, bytes, s); });
    if (col80) return by_dilation<1, 3, 5>(dil, [&](auto d) { return launch_convq2_dil<decltype(d)::value, kPair128Col80>(p, bytes, s); });
    return wide ? by_dilation<1, 3, 3>(dil, [&](auto d) { return launch_convq2_dil<decltype(d)::value, kPair128Wide>(p, bytes, s); })
                : by_dilation<1, 3, 5>(dil, [&](auto d) { return launch_convq2_dil<decltype(d)::value, 128>(p, bytes, s); });
}

int launch_convp(PairParams p, int dil, hipStream_t s) { return launch_fused_pair(kFusedPair64, p, dil, s); }
int launch_convq(PairParams p, int dil, hipStream_t s) { return launch_fused_pair(kFusedPair128, p, dil, s); }

}  // namespace fv
