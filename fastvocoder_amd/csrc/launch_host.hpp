// Host-side pieces the launchers of the persistent kernels share (convh_launch.hip, pair_launch.hip, mrfh_launch.hip,
// launch_convk, launch_convtn): argument checks, persistent grid, contiguous cut, LDS layout, work counts, the profile
// bracket.  Plain functions and PODs; nothing here allocates.  `fam` is the family's name as its messages begin.
#pragma once
#include <stdio.h>

#include <type_traits>

#include "fv_internal.h"

namespace fv {

// ---- argument checks: 0, or fail()'s code --------------------------------------------------------------------------
// the kernels address a tensor of one utterance through a buffer descriptor (dims: the message names the tensor's size)
inline int check_desc_range(const char* fam, int C, int T, bool dims = true) {
    if ((double)C * T * 4.0 < 1073741824.0) return 0;
    char size[48] = "";
    if (dims) snprintf(size, sizeof(size), " (%d x %d floats)", C, T);
    return fail(FV_ERR_UNSUPPORTED, "%s: one utterance's tensor%s exceeds the 1 GiB buffer-descriptor range; split the utterance", fam, size);
}
inline int check_slopes(const char* fam, float slope, float act_slope) {
    if (slope < 0.f || slope > 1.f || act_slope < 0.f || act_slope > 1.f)
        return fail(FV_ERR_INVALID_ARG, "%s: activation slope outside [0, 1]", fam);
    return 0;
}
// what every multi-member family checks behind its own shape checks: member count, descriptor range, slopes
inline int check_launch(const char* fam, const PairCore& p, int C) {
    if (p.n_members < 1 || p.n_members > 3) return fail(FV_ERR_INVALID_ARG, "%s: %d members", fam, p.n_members);
    if (int rc = check_desc_range(fam, C, p.T)) return rc;
    return check_slopes(fam, p.slope, p.act_slope);
}
inline int check_taps(const char* fam, int k) {
    if (k != 11 && k != 7 && k != 3) return fail(FV_ERR_UNSUPPORTED, "%s: %d taps (3, 7 or 11)", fam, k);
    return 0;
}
inline int check_reflect(const char* fam, int pad, int T) {
    if (pad >= T) return fail(FV_ERR_INVALID_ARG, "%s: reflection padding %d needs more than %d samples", fam, pad, T);
    return 0;
}
// One member's tensors.  i: the member's number as the messages name it (< 0: a family of one member, no number).
enum : unsigned { kNeedX2 = 1, kNeedW2 = 2, kNeedY = 4, kAlignX = 8 };      // x and w1 are always needed, w1 always aligned
struct MemberNote {
    char text[24];
    explicit MemberNote(int i) {
        text[0] = 0;
        if (i >= 0) snprintf(text, sizeof(text), " (member %d)", i);
    }
};
inline int check_tensors(const char* fam, const PairMember& mb, int i, unsigned rules) {
    if (!mb.x || !mb.w1 || ((rules & kNeedX2) && !mb.x2) || ((rules & kNeedW2) && !mb.w2) || ((rules & kNeedY) && !mb.y))
        return fail(FV_ERR_INVALID_ARG, "%s: null tensor%s", fam, MemberNote(i).text);
    return 0;
}
inline int check_adds(const char* fam, bool add1, bool add2, int i = -1) {
    if (add2 && !add1) return fail(FV_ERR_INVALID_ARG, "%s: add2 without add1%s", fam, MemberNote(i).text);
    return 0;
}
inline int check_aligned(const char* fam, const PairMember& mb, unsigned rules) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(mb.w1) | ((rules & kNeedW2) ? reinterpret_cast<uintptr_t>(mb.w2) : 0) |
                           ((rules & kAlignX) ? reinterpret_cast<uintptr_t>(mb.x) : 0);
    if (bits & 15) return fail(FV_ERR_UNSUPPORTED, "%s: %spacked weights must be 16-byte aligned", fam, (rules & kAlignX) ? "x / " : "");
    return 0;
}
inline int check_member(const char* fam, const PairMember& mb, int i, unsigned rules) {
    if (int rc = check_tensors(fam, mb, i, rules)) return rc;
    if (int rc = check_adds(fam, mb.add1, mb.add2, i)) return rc;
    return check_aligned(fam, mb, rules);
}

// largest taps first: the kernels' member order (the cost order of the contiguous partition)
inline void sort_members_by_taps(PairCore& p) {
    for (int i = 0; i < p.n_members; ++i)
        for (int j = i + 1; j < p.n_members; ++j)
            if (p.m[j].k > p.m[i].k) { PairMember t = p.m[i]; p.m[i] = p.m[j]; p.m[j] = t; }
}

// ---- grid, cut, debug fields ---------------------------------------------------------------------------------------
// blocks of a persistent launch: `asked` (the family's Tuning::*_blocks) when positive, else per_cu on every CU; never
// more than there are items
inline long long persistent_blocks(long long items, int per_cu, int asked) {
    long long nblk = asked > 0 ? asked : (long long)per_cu * device_cu_count();
    if (nblk > items) nblk = items;
    return nblk;
}
// the kernels' contiguous, cost-balanced cut of the members' items into `shares`, as a table (pair_cut_schedule)
inline void cut_table(PairParams& p, int shares) {
    long long n[3] = {0, 0, 0};
    for (int i = 0; i < p.n_members; ++i) n[i] = p.m[i].n_items;
    pair_cut_schedule(p, shares, n);
}
inline unsigned long long* trace_buffer() { return reinterpret_cast<unsigned long long*>(tuning().trace_ptr); }
inline void set_debug(PairCore& p, bool dbg = true, bool trace = true) {
    p.dbg = dbg ? tuning().pair_dbg : 0;
    p.trace = trace ? trace_buffer() : nullptr;
}

// ---- dynamic LDS: regions appended in floats -------------------------------------------------------------------------
struct LdsLayout {
    size_t floats = 0;
    int add(size_t n) {                // -> the float offset of the region
        const size_t at = floats;
        floats += n;
        return (int)at;
    }
    size_t bytes() const { return floats * 4; }
};
inline int check_lds(const char* fam, size_t bytes, size_t limit = 160 * 1024) {
    if (bytes > limit) return fail(FV_ERR_UNSUPPORTED, "%s: %zu bytes of LDS", fam, bytes);
    return 0;
}

// ---- work counts of the measurement hook, and its bracket ------------------------------------------------------------
struct Work {
    double flops, bytes;
};
// resblock pairs: two convs per member; x in, y (and its twin) out, the addends, both weights once
inline Work pair_work(const PairCore& p, int C) {
    Work w = {0, 0};
    for (int i = 0; i < p.n_members; ++i) {
        const PairMember& mb = p.m[i];
        w.flops += 2.0 * 2.0 * p.B * (double)C * C * mb.k * p.T;
        w.bytes += 4.0 * (2.0 * C * C * mb.k + (double)p.B * C * p.T *
                          ((p.sum ? 1 : (mb.y_act ? 3 : 2)) + (mb.add1 ? 1 : 0) + (mb.add2 ? 1 : 0)));
    }
    return w;
}
// MACs of a ConvTranspose1d = Tin * Cin * Cout * k; x_reads: x and the inputs merged into it
inline Work convt_work(int B, int T, int Tout, int Cin, int Cout, int k, int x_reads, bool twin) {
    return Work{2.0 * B * (double)T * Cin * Cout * k,
                4.0 * ((double)Cin * Cout * k + (double)B * ((double)Cin * T * x_reads + (double)Cout * Tout * (twin ? 2 : 1)))};
}
// profile_begin now, profile_end when the scope ends -- behind the launch, whatever it returned
struct ProfileScope {
    hipStream_t s;
    int kind;
    Work w;
    ProfileScope(hipStream_t stream, int kind_, Work work) : s(stream), kind(kind_), w(work) { profile_begin(s); }
    ~ProfileScope() { profile_end(s, kind, w.flops, w.bytes); }
    ProfileScope(const ProfileScope&) = delete;
    ProfileScope& operator=(const ProfileScope&) = delete;
};

// f(std::integral_constant<int, D>) for the D among the three that equals dil (the last one when none does: the callers
// have checked dil): picks a template instance by dilation
template <int D0, int D1, int D2, class F>
inline int by_dilation(int dil, F f) {
    return dil == D0 ? f(std::integral_constant<int, D0>()) : dil == D1 ? f(std::integral_constant<int, D1>())
                                                                       : f(std::integral_constant<int, D2>());
}

}  // namespace fv
