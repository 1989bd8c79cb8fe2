// Host side of the one-launch MRF stage (mrfh_kernels.hpp): validation, blob offsets, window geometry, grid; the 32-channel
// stage in two block classes (mrfw_kernels.hpp SPLIT): the classes' block counts and the per-block column table.
#include <string.h>
#include <array>
#include <map>
#include <mutex>
#include "launch_host.hpp"

namespace fv {

extern template int launch_mrfh_geom<3, 12>(const MrfParams&, hipStream_t);
extern template int launch_mrfh_geom<2, 16>(const MrfParams&, hipStream_t);

// history of the 32-channel kernel: one slot set per block; a launch has at most max(CUs, Tuning::mrf_blocks) blocks
static long long mrfw_max_blocks() {
    const long long cus = device_cu_count(), asked = tuning().mrf_blocks;
    return asked > cus ? asked : cus;
}
long long mrf_workspace_bytes(int C) { return C == 32 ? mrfw_max_blocks() * kMrfwHistBytes : 0; }

int launch_mrfh(MrfParams p, int C, const int* dil, hipStream_t s) {
    const char* const fam = "mrf stage";
    if (p.B <= 0 || p.T <= 0) return 0;
    if (!mrf_stage_shape(C, p.k, dil))
        return fail(FV_ERR_UNSUPPORTED, "mrf stage: C = %d, taps (%d, %d, %d), dilations (%d, %d, %d): built for 16 / 32 channels, taps "
                    "3 / 7 / 11, dilations (1, 3, 5)", C, p.k[0], p.k[1], p.k[2], dil ? dil[0] : 0, dil ? dil[1] : 0, dil ? dil[2] : 0);
    const bool fold = p.fold_w != nullptr;
    if (!p.x || !p.blob || (!fold && !p.y) || (fold && (!p.fold_y || p.y || p.y_act)))
        return fail(FV_ERR_INVALID_ARG, "mrf stage: null tensor (or both an output tensor and a folded output conv)");
    // every block reads x columns (a run's first tile starts `halo` early, plus the right-hand recompute margin) that its
    // neighbours write as y: an output that is the input would be read half-updated (the pair entries refuse it too)
    if (p.y == p.x || p.y_act == p.x || (p.y_act && p.y_act == p.y) || p.fold_y == p.x)
        return fail(FV_ERR_INVALID_ARG, "mrf stage: an output tensor aliases the input (or y_act aliases y)");
    if ((reinterpret_cast<uintptr_t>(p.blob) & 15) != 0) return fail(FV_ERR_UNSUPPORTED, "mrf stage: the packed stage must be 16-byte aligned");
    if (int rc = check_desc_range(fam, C, p.T)) return rc;
    if ((double)p.B * p.T >= 2147483647.0) return fail(FV_ERR_UNSUPPORTED, "mrf stage: B x T = %d x %d columns exceed 2^31", p.B, p.T);
    if (int rc = check_slopes(fam, p.slope, p.act_slope)) return rc;
    unsigned off = 0;
    double flops = 0;
    for (int j = 0; j < 3; ++j)
        for (int q = 0; q < 3; ++q) {
            p.blk_off[3 * j + q] = off;
            off += (unsigned)mrf_block_bytes(C, p.k[j]);
            flops += 2.0 * 2.0 * p.B * (double)C * C * p.k[j] * p.T;
        }
    p.blob_bytes = off;
    p.halo = mrf_halo(p.k, dil);
    p.ol = fold ? 3 : 0;
    p.total = (long long)p.B * p.T;
    const int shape = tuning().mrf_shape;
    const int W = C == 32 ? 384 : shape == 1 ? 512 : 576;
    const int vcols = W - p.halo, adv = vcols - 2 * p.ol;
    if (adv < 64) return fail(FV_ERR_UNSUPPORTED, "mrf stage: a %d-column window leaves %d final columns", W, adv);
    // One block per CU (the weight slots, two images and the history are 147 KB of LDS); a share below ~a quarter window
    // is all run-in (a run's first tile starts `halo` columns early).
    long long nblk = persistent_blocks((p.total + 127) / 128, 1, tuning().mrf_blocks);
    if (nblk < 1) nblk = 1;
    p.nblk = (int)nblk;
    if (C == 32) {
        if (!p.hist || p.hist_bytes < nblk * kMrfwHistBytes || (reinterpret_cast<uintptr_t>(p.hist) & 15) != 0)
            return fail(FV_ERR_WORKSPACE, "mrf stage: 32 channels need a 16-byte aligned workspace of fv_mrf_stage_workspace_bytes "
                        "(%lld bytes for %lld blocks; given %lld)", nblk * kMrfwHistBytes, nblk, p.hist ? p.hist_bytes : 0LL);
    } else {
        p.hist = nullptr;
    }
    p.prio = tuning().mrf_prio;
    p.trace = trace_buffer();
    double bytes = 4.0 * ((double)p.B * C * p.T * (fold ? 1.0 : (p.y_act ? 3.0 : 2.0)) + (fold ? (double)p.B * p.T : 0.0)) + off;
    if (fold) flops += 2.0 * p.B * (double)C * 7 * p.T;   // (the folded output conv: C -> 1 channels, 7 taps)
    ProfileScope prof(s, C == 32 ? FV_KERNEL_MRF32 : FV_KERNEL_MRF16, Work{flops, bytes});
    return C == 32 ? launch_mrfw_geom(p, s) : shape == 1 ? launch_mrfh_geom<2, 16>(p, s) : launch_mrfh_geom<3, 12>(p, s);
}

// ---- the 32-channel stage in two block classes ---------------------------------------------------------------------------
// Window arithmetic of mrfw_kernel: a run's first window gives W - 2 reach final columns, every further one W - reach.
constexpr int kMrfwW = 384, kMrfwReachA = 60, kMrfwReachB = 36;     // reaches: the 11-tap ResBlock; the 7-tap one (the 3-tap: 12)
static long long mrfw_windows(long long cols, int reach) {
    const long long first = kMrfwW - 2 * reach, next = kMrfwW - reach;
    return cols <= first ? 1 : 1 + (cols - first + next - 1) / next;
}
static long long mrfw_window_cols(long long windows, int reach) { return (kMrfwW - 2 * reach) + (windows - 1) * (long long)(kMrfwW - reach); }
// n blocks of one class on B utterances of T columns (n >= B): utterance u gets n / B blocks, the first n % B one more; its
// blocks take whole windows -- as many as the utterance's worst block needs -- from its start until it is covered.  Returns
// the windows of the launch's worst block; with `range`, appends the blocks' [first, last) global columns and counts them.
static long long mrfw_class_cut(int B, int T, int n, int reach, unsigned* range, int* used) {
    long long worst = 0;
    for (int u = 0; u < B; ++u) {
        const int m = n / B + (u < n % B ? 1 : 0);
        const long long w = mrfw_windows((T + m - 1) / m, reach), cols = mrfw_window_cols(w, reach);
        if (w > worst) worst = w;
        if (!range) continue;
        for (long long a = 0; a < T; a += cols) {
            range[2 * *used] = (unsigned)((long long)u * T + a);
            range[2 * *used + 1] = (unsigned)((long long)u * T + (a + cols < T ? a + cols : T));
            ++*used;
        }
    }
    return worst;
}

bool mrf_class_plan(int B, int T, int nblk, bool force, MrfClassPlan& out) {
    if (B < 1 || T < 1 || nblk < 1 || nblk > kSchedBlocks || (double)B * T >= 2147483647.0) return false;
    const Tuning& tn = tuning();
    typedef std::array<long long, 7> Key;
    static std::mutex mu;
    static std::map<Key, MrfClassPlan> cache;            // a forward asks for the same one or two plans call after call
    const Key key = {B, T, nblk, force, tn.mrf_cost_a, tn.mrf_cost_b, tn.mrf_cost_one};
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it == cache.end()) {
        MrfClassPlan pl = {};
        const long long total = (long long)B * T;
        // the all-in-one form: equal shares of the concatenated columns (mrfw_kernel); a share that crosses an utterance end
        // starts a new run there
        long long worst_one = 0;
        for (int i = 0; i < nblk; ++i) {
            const long long lo = total * i / nblk, hi = total * (i + 1) / nblk;
            long long w = 0;
            for (long long a = lo; a < hi;) {
                const long long end = (a / T + 1) * T < hi ? (a / T + 1) * T : hi;
                w += mrfw_windows(end - a, kMrfwReachA);
                a = end;
            }
            if (w > worst_one) worst_one = w;
        }
        pl.makespan_one = worst_one * tn.mrf_cost_one;
        // the split: the block count of class A that makes the slower class fastest (ties: the fewest windows in flight)
        int best = 0;
        long long best_span = 0, best_sum = 0;
        for (int na = B; nblk - na >= B; ++na) {
            const long long ta = mrfw_class_cut(B, T, na, kMrfwReachA, nullptr, nullptr) * tn.mrf_cost_a;
            const long long tb = mrfw_class_cut(B, T, nblk - na, kMrfwReachB, nullptr, nullptr) * tn.mrf_cost_b;
            const long long span = ta > tb ? ta : tb;
            if (!best || span < best_span || (span == best_span && ta + tb < best_sum)) {
                best = na;
                best_span = span;
                best_sum = ta + tb;
            }
        }
        if (best && (force || best_span < pl.makespan_one)) {
            pl.split = 1;
            pl.makespan = best_span;
            pl.reach_a = kMrfwReachA;
            pl.reach_b = kMrfwReachB;
            int used = 0;
            mrfw_class_cut(B, T, best, kMrfwReachA, pl.range, &used);
            pl.n_a = used;
            mrfw_class_cut(B, T, nblk - best, kMrfwReachB, pl.range, &used);
            pl.n_b = used - pl.n_a;
        } else {
            pl.makespan = pl.makespan_one;
            pl.n_b = nblk;
            pl.reach_b = kMrfwReachA;
            for (int i = 0; i < nblk; ++i) {
                pl.range[2 * i] = (unsigned)(total * i / nblk);
                pl.range[2 * i + 1] = (unsigned)(total * (i + 1) / nblk);
            }
        }
        if (cache.size() >= 64) cache.clear();
        it = cache.emplace(key, pl).first;
    }
    out = it->second;
    return true;
}

int launch_mrfw_split(MrfSplitParams p, const int* dil, hipStream_t s, int one_class) {
    const char* const fam = "mrf stage (two classes)";
    if (p.B <= 0 || p.T <= 0) return 0;
    if (!dil || dil[0] != 1 || dil[1] != 3 || dil[2] != 5 || p.k[0] != 3 || p.k[1] != 7 || p.k[2] != 11)
        return fail(FV_ERR_UNSUPPORTED, "%s: 32 channels, taps (3, 7, 11) in this order -- the sum r_0 + r_1 is the reference's first "
                    "-- and dilations (1, 3, 5)", fam);
    if (one_class) p.y2 = p.y;                           // (the class launched stores through whichever of the two is its own)
    if (!p.x || !p.blob || !p.y || !p.y2) return fail(FV_ERR_INVALID_ARG, "%s: null tensor", fam);
    if (p.y == p.x || p.y2 == p.x || (p.y == p.y2 && !one_class)) return fail(FV_ERR_INVALID_ARG, "%s: an output tensor aliases the input or the other output", fam);
    if ((reinterpret_cast<uintptr_t>(p.blob) & 15) != 0) return fail(FV_ERR_UNSUPPORTED, "%s: the packed stage must be 16-byte aligned", fam);
    if (int rc = check_desc_range(fam, 32, p.T)) return rc;
    if ((double)p.B * p.T >= 2147483647.0) return fail(FV_ERR_UNSUPPORTED, "%s: B x T = %d x %d columns exceed 2^31", fam, p.B, p.T);
    if (int rc = check_slopes(fam, p.slope, 1.f)) return rc;
    unsigned off = 0;
    double flops = 0;
    for (int j = 0; j < 3; ++j)
        for (int q = 0; q < 3; ++q) {
            p.blk_off[3 * j + q] = off;
            off += (unsigned)mrf_block_bytes(32, p.k[j]);
            flops += 2.0 * 2.0 * p.B * 32.0 * 32.0 * p.k[j] * p.T;
        }
    p.blob_bytes = off;
    p.halo = kMrfwReachA;
    p.halo_b = kMrfwReachB;
    if (p.halo != mrf_halo(p.k, dil)) return fail(FV_ERR_UNSUPPORTED, "%s: reach", fam);
    p.ol = 0;
    p.total = (long long)p.B * p.T;
    long long nblk = persistent_blocks((p.total + 127) / 128, 1, tuning().mrf_blocks);
    if (nblk > kSchedBlocks) nblk = kSchedBlocks;
    // a block's range lies inside one utterance: each class needs a block per utterance
    if (nblk < 2LL * p.B) return fail(FV_ERR_UNSUPPORTED, "%s: %lld blocks for %d utterances (two per utterance at least)", fam, nblk, p.B);
    MrfClassPlan pl;
    if (!mrf_class_plan(p.B, p.T, (int)nblk, true, pl) || !pl.split) return fail(FV_ERR_UNSUPPORTED, "%s: no plan", fam);
    p.n_a = pl.n_a;
    p.nblk = pl.n_a + pl.n_b;
    memcpy(p.range, pl.range, sizeof(p.range));
    if (one_class == 1) {                                // (the debug entry: one class's blocks of the same table alone)
        p.nblk = pl.n_a;
    } else if (one_class == 2) {
        p.n_a = 0;
        p.nblk = pl.n_b;
        memcpy(p.range, pl.range + 2 * pl.n_a, sizeof(unsigned) * 2 * (size_t)pl.n_b);
    }
    if (!p.hist || p.hist_bytes < (long long)p.nblk * kMrfwHistBytes || (reinterpret_cast<uintptr_t>(p.hist) & 15) != 0)
        return fail(FV_ERR_WORKSPACE, "%s: a 16-byte aligned workspace of fv_mrf_stage_workspace_bytes (%lld bytes for %d blocks; given %lld)",
                    fam, (long long)p.nblk * kMrfwHistBytes, p.nblk, p.hist ? p.hist_bytes : 0LL);
    p.prio = tuning().mrf_prio;
    p.trace = trace_buffer();
    ProfileScope prof(s, FV_KERNEL_MRF32, Work{flops, 4.0 * 3.0 * p.B * 32.0 * p.T + off});
    return launch_mrfw_split_geom(p, s);
}

}  // namespace fv
