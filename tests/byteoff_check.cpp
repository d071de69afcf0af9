// The pure arithmetic that csrc/span.h adds for the token byte offsets, built by a host compiler: the 64-bit scan over
// the spans as its 1,024 threads run it (per-thread slice sums, the serial fold, per-thread offsets, in place), against
// a plain running sum -- with counts and totals that cross 2^32 -- and the lower bound that finds a span's first patch.
#include "span.h"

#include <cstdio>
#include <vector>

using namespace mbpe;

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static int failures = 0, cases = 0;

// span_scan_sum64 without the device: every "thread" in turn, the barriers between the three steps
static unsigned long long host_scan(std::vector<unsigned long long> &cnt) {
    const uint64_t n = cnt.size();
    std::vector<unsigned long long> sh(kScanThreads);
    for (uint32_t t = 0; t < (uint32_t)kScanThreads; ++t) {
        uint64_t lo, hi;
        span_scan_slice(n, t, &lo, &hi);
        if (lo > hi || hi > n) { ++failures; return 0; }
        sh[t] = span_sum_slice64(cnt.data(), lo, hi);
    }
    unsigned long long total = 0;
    for (int t = 0; t < kScanThreads; ++t) { const unsigned long long v = sh[t]; sh[t] = total; total += v; }
    for (uint32_t t = 0; t < (uint32_t)kScanThreads; ++t) {
        uint64_t lo, hi;
        span_scan_slice(n, t, &lo, &hi);
        span_offsets_slice64(cnt.data(), cnt.data(), lo, hi, sh[t]);
    }
    return total;
}

static void check_scan(uint64_t n, int kind) {
    std::vector<unsigned long long> cnt(n), want(n);
    unsigned long long run = 0;
    for (uint64_t i = 0; i < n; ++i) {
        unsigned long long v;
        switch (kind) {
            case 0: v = rnd() % 4096; break;                       // a span of short tokens
            case 1: v = 0xFFFFFFFFull; break;                      // every span just below 2^32: the sum crosses at once
            case 2: v = (1ull << 32) + rnd() % 1024; break;        // a single count beyond 2^32 (a long one-token chunk)
            default: v = rnd() % (1ull << 40); break;
        }
        cnt[i] = v;
        want[i] = run;
        run += v;
    }
    const unsigned long long total = host_scan(cnt);
    ++cases;
    bool ok = total == run;
    for (uint64_t i = 0; i < n && ok; ++i) ok = cnt[i] == want[i];
    if (!ok) { ++failures; printf("scan n=%llu kind=%d differs\n", (unsigned long long)n, kind); }
}

static void check_lower_bound() {
    const uint64_t sizes[] = {0, 1, 2, 3, 64, 1000};
    for (uint64_t n : sizes) {
        std::vector<unsigned long long> idx(n);
        unsigned long long v = 0;
        for (uint64_t i = 0; i < n; ++i) { v += 1 + rnd() % 3000; idx[i] = v + (i == n - 1 ? (1ull << 33) : 0); }
        for (int q = 0; q < 2000; ++q) {
            unsigned long long x = q < 1000 || n == 0 ? rnd() % (v + 2) : idx[rnd() % n] + (rnd() % 3) - 1;
            uint64_t want = 0;
            while (want < n && idx[want] < x) ++want;
            ++cases;
            if (lower_bound64(idx.data(), n, x) != want) { ++failures; printf("lower_bound n=%llu differs\n", (unsigned long long)n); }
        }
    }
}

int main() {
    const uint64_t sizes[] = {0, 1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 5000};
    for (uint64_t n : sizes)
        for (int kind = 0; kind < 4; ++kind) check_scan(n, kind);
    check_lower_bound();
    printf("ok: %d cases, %d failures\n", cases, failures);
    return failures != 0;
}
