// Host races of libfastvocoder_hip.so under ThreadSanitizer: a stand-alone program (no GPU, no Python) that calls the
// host-only entries of the library from eight threads at once, on shared keys and on distinct keys, and checks that every
// thread got the answers a single thread gets.  Built against a copy of the library whose HOST code is compiled with
// -fsanitize=thread (tools/README.md has the recipe); the sanitizer's report is the result, the program's own checks are
// the second line.  It touches no device: the schedule and width caches of csrc/convh_launch.hip, the class plans of
// csrc/mrfh_launch.hip, the kernel-name hook, the launch log with its two readers, the error text, the tuning table.
//
//     host_race_check            every phase but the last
//     host_race_check tuning     also fv_tuning_set on one thread against readers on the others.  The tuning table is
//                                plain data and the header says the hook is not for concurrent use: this phase shows what
//                                the sanitizer makes of a caller that ignores that.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../include/fastvocoder_hip.h"

static const int kThreads = 8, kRounds = 200;
static std::atomic<int> g_failures{0};

#define EXPECT(cond)                                                           \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "host_race_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_failures.fetch_add(1);                                           \
        }                                                                      \
    } while (0)

struct Schedule {
    int on;
    unsigned table[512];
};

// 378 items of three costs on 256 blocks (HiFi-GAN light, batch 1), or a key of the thread's own
static Schedule pair_schedule(int key) {
    const int n_items[3] = {126 + key, 126, 126}, cost[3] = {16, 12, 8};
    Schedule s = {};
    s.on = fv_debug_pair_schedule(3, n_items, cost, 256, 0, 1, s.table);
    return s;
}

struct Widths {
    int rc;
    int64_t info[12];
};

static Widths pair_widths(int key) {
    const int taps[3] = {11, 7, 3};
    Widths w = {};
    w.rc = fv_debug_pair_widths(128, 1, 8000 + 64 * key, 1, 3, taps, 256, w.info);
    return w;
}

struct Classes {
    int rc;
    int64_t info[12];
    unsigned table[512];
};

static Classes class_schedule(int key) {
    Classes c = {};
    c.rc = fv_debug_mrf_class_schedule(1 + key % 3, 4000 + 100 * key, 256, 0, c.info, c.table);
    return c;
}

static std::string kernel_name(const char* symbol) {
    char buf[256];
    const int64_t n = fv_debug_kernel_name(symbol, buf, sizeof(buf));
    return std::string(buf, (size_t)(n < (int64_t)sizeof(buf) ? n : (int64_t)sizeof(buf)));
}

static void run(const char* what, void (*body)(int)) {
    std::vector<std::thread> threads;
    for (int t = 0; t < kThreads; ++t) threads.emplace_back(body, t);
    for (auto& t : threads) t.join();
    printf("host_race_check: %-28s %s\n", what, g_failures.load() ? "FAILED" : "ok");
}

// every thread asks for the SAME key first (the caches are filled under contention), then for keys of its own
static void schedules(int t) {
    for (int r = 0; r < kRounds; ++r) {
        const int key = r < kRounds / 2 ? r % 4 : 8 * (r % 16) + t;
        const Schedule a = pair_schedule(key), b = pair_schedule(key);
        EXPECT(a.on >= 0 && a.on == b.on && memcmp(a.table, b.table, sizeof(a.table)) == 0);
        const Widths wa = pair_widths(key), wb = pair_widths(key);
        EXPECT(wa.rc == 0 && wb.rc == 0 && memcmp(wa.info, wb.info, sizeof(wa.info)) == 0);
        const Classes ca = class_schedule(key), cb = class_schedule(key);
        EXPECT(ca.rc == 0 && cb.rc == 0 && memcmp(ca.info, cb.info, sizeof(ca.info)) == 0 &&
               memcmp(ca.table, cb.table, sizeof(ca.table)) == 0);
    }
}

static void names(int t) {
    for (int r = 0; r < kRounds; ++r) {
        EXPECT(kernel_name("_ZN2fv12convh_kernelILi2ELi2ELi1EEEvNS_10PairParamsE") == "convh_kernel<2, 2, 1>");
        EXPECT(kernel_name(t % 2 ? "_ZN2fv12convr_kernelENS_10PairParamsE" : "fv_version") == (t % 2 ? "convr_kernel" : "fv_version"));
    }
}

// refusals: every thread provokes an error text of its own and must read back exactly that
static void errors(int t) {
    unsigned table[512];
    const int n_items[3] = {1, 1, 1}, cost[3] = {1, 1, 1};
    for (int r = 0; r < kRounds; ++r) {
        char want[64];
        if (t % 2) {
            EXPECT(fv_debug_pair_schedule(4 + t, n_items, cost, 256, 0, 0, table) == FV_ERR_INVALID_ARG);
            snprintf(want, sizeof(want), "debug_pair_schedule: %d members", 4 + t);
        } else {
            const int taps[1] = {3};
            int64_t info[12];
            EXPECT(fv_debug_pair_widths(100 + t, 1, 100, 1, 1, taps, 256, info) == FV_ERR_UNSUPPORTED);
            snprintf(want, sizeof(want), "debug_pair_widths: C = %d", 100 + t);
        }
        EXPECT(strncmp(fv_last_error(), want, strlen(want)) == 0);
    }
}

// the launch log: thread 0 switches it, the others read both tables (nothing launches: the tables stay empty)
static void log_hooks(int t) {
    for (int r = 0; r < kRounds; ++r) {
        if (t == 0) {
            EXPECT(fv_debug_launch_log(r % 2) == 0);
        } else {
            char buf[64];
            uint64_t handles[4];
            int64_t counts[4], copies = -1;
            EXPECT(fv_debug_launch_log_read(buf, sizeof(buf)) == 0);
            EXPECT(fv_debug_launch_log_streams(handles, counts, 4, &copies) == 0 && copies == 0);
        }
    }
    if (t == 0) EXPECT(fv_debug_launch_log(0) == 0);
}

// fv_tuning_set against readers (pair_widths reads convq_nm11 and the schedule's costs): "tuning" mode only
static void tuning(int t) {
    for (int r = 0; r < kRounds; ++r) {
        if (t == 0) EXPECT(fv_tuning_set("convq_nm11", r % 2 ? 64 : -1) == 0);
        else EXPECT(pair_widths(1000 + 8 * r + t).rc == 0);
    }
    if (t == 0) EXPECT(fv_tuning_set("convq_nm11", -1) == 0);
}

int main(int argc, char** argv) {
    const bool with_tuning = argc > 1 && strcmp(argv[1], "tuning") == 0;
    printf("host_race_check: ABI %d, build %s, %d threads x %d rounds\n", fv_version(), fv_build_id(), kThreads, kRounds);
    run("schedules, widths, classes", schedules);
    run("kernel names", names);
    run("error text", errors);
    run("launch log and its readers", log_hooks);
    if (with_tuning) run("tuning_set against readers", tuning);
    if (g_failures.load()) {
        fprintf(stderr, "host_race_check: %d checks failed\n", g_failures.load());
        return 1;
    }
    printf("host_race_check: all answers equal the single-threaded ones\n");
    return 0;
}
