// Stand-alone check of the pure arithmetic of csrc/span.h, built by the host compiler (tests/test_span_cpu.py).
//   part 1: span_fold is associative (all 64 triples), which is what licenses the slice-per-thread parity scan
//   part 2: group masks -> span summaries -> sliced scan -> run parity of every position, against a sequential count
// span_scan_parity itself is device code: of its three sweeps the first (span_fold_slice) is the shared function, the
// serial fold across the slices and the restart from {0, parity} are written out again below from span_fold.  Those
// two loops of the kernel, its slicing and its barriers are guarded by the GPU span tests only.
#include "span.h"

#include <cstdio>
#include <vector>

using namespace mbpe;

static int check_associative() {
    int bad = 0;
    for (uint32_t x = 0; x < 4; ++x)
        for (uint32_t y = 0; y < 4; ++y)
            for (uint32_t z = 0; z < 4; ++z) {
                const SpanSum a = span_unpack(x), b = span_unpack(y), c = span_unpack(z);
                const uint32_t l = span_pack(span_fold(span_fold(a, b), c)), r = span_pack(span_fold(a, span_fold(b, c)));
                if (l != r) { printf("fold not associative at (%u, %u, %u): %u != %u\n", x, y, z, l, r); ++bad; }
            }
    return bad;
}

// candidate mask of the 64 positions from `at`; positions at or beyond the end are no candidates (as in the kernels)
static unsigned long long group_mask(const std::vector<uint8_t> &c, uint64_t at) {
    unsigned long long M = 0;
    for (uint64_t l = 0; l < (uint64_t)kWave && at + l < c.size(); ++l) M |= (unsigned long long)c[at + l] << l;
    return M;
}

// the run parity of every position of c through span.h, the spans cut into `slices` slices as span_scan_parity
// cuts them into kScanThreads (its three sweeps, one "thread" after the other); compared with the sequential count.
// Returns the number of wrong positions.
static std::vector<uint32_t> span_sum, in_par, sh;      // (kept between the calls)
static uint64_t check_string(const std::vector<uint8_t> &c, uint64_t slices, const char *what) {
    const uint64_t n = c.size(), n_spans = span_count(n);
    span_sum.resize(n_spans);
    in_par.resize(n_spans);
    sh.resize(slices);
    for (uint64_t s = 0; s < n_spans; ++s) {
        SpanSum sum = span_empty();
        for (int it = 0; it < kSpanIters; ++it) sum = span_add_group(sum, group_mask(c, s * kSpan + (uint64_t)it * kWave));
        span_sum[s] = span_pack(sum);
    }
    const uint64_t per = (n_spans + slices - 1) / slices;
    auto lo_of = [&](uint64_t t) { return per * t < n_spans ? per * t : n_spans; };
    auto hi_of = [&](uint64_t t) { return lo_of(t) + per < n_spans ? lo_of(t) + per : n_spans; };
    for (uint64_t t = 0; t < slices; ++t) sh[t] = span_pack(span_fold_slice(span_sum.data(), lo_of(t), hi_of(t)));
    SpanSum acc = span_empty();
    for (uint64_t t = 0; t < slices; ++t) {
        const SpanSum v = span_unpack(sh[t]);
        sh[t] = acc.par;
        acc = span_fold(acc, v);
    }
    for (uint64_t t = 0; t < slices; ++t) {
        SpanSum a = {0u, sh[t]};
        for (uint64_t s = lo_of(t); s < hi_of(t); ++s) {
            in_par[s] = a.par;
            a = span_fold(a, span_unpack(span_sum[s]));
        }
    }
    uint64_t bad = 0, run = 0;                 // run = consecutive candidates immediately before position i
    for (uint64_t s = 0; s < n_spans; ++s) {
        uint32_t carry = in_par[s];
        for (int it = 0; it < kSpanIters; ++it) {
            const uint64_t at = s * kSpan + (uint64_t)it * kWave;
            const unsigned long long M = group_mask(c, at);
            for (uint32_t lane = 0; lane < (uint32_t)kWave && at + lane < n; ++lane) {
                const uint64_t i = at + lane;
                if ((run_below(M, lanes_below(lane), lane, carry) & 1u) != (run & 1u)) {
                    if (!bad) printf("%s, n = %llu, %llu slices: position %llu follows %llu candidates, span.h says %s\n", what,
                                     (unsigned long long)n, (unsigned long long)slices, (unsigned long long)i,
                                     (unsigned long long)run, run & 1u ? "even" : "odd");
                    ++bad;
                }
                run = c[i] ? run + 1 : 0;
            }
            carry = run_carry(M, carry);
        }
    }
    return bad;
}

static uint64_t splitmix(uint64_t *s) {
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    int failed = check_associative();
    const uint64_t lengths[] = {1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 5 * 1024 + 17};
    const uint64_t slicings[] = {1, 2, 3, (uint64_t)kScanThreads};
    uint64_t n_strings = 0, seed = 20240607;
    auto check = [&](const std::vector<uint8_t> &c, const char *what) {
        ++n_strings;
        for (uint64_t slices : slicings) failed += check_string(c, slices, what) != 0;
    };
    for (uint64_t n : lengths) {
        std::vector<uint8_t> c(n, 1);
        check(c, "all ones");
        // one zero at every position of the first group: the run after it crosses every later group and span
        for (uint64_t z = 0; z < (uint64_t)kWave && z < n; ++z) { c[z] = 0; check(c, "ones with one zero"); c[z] = 1; }
        c.assign(n, 0);
        check(c, "all zeros");
        for (uint64_t i = 0; i < n; ++i) c[i] = i & 1;
        check(c, "alternating 0 1");
        for (uint64_t i = 0; i < n; ++i) c[i] = ~i & 1;
        check(c, "alternating 1 0");
        // densities 1 - 2^-k, k = 1 .. 14: from short runs to runs of several spans
        for (int k = 0; k < 28; ++k) {
            const uint64_t zero_below = 1ull << (63 - k % 14);      // P(zero) = 2^-(k % 14 + 1)
            for (uint64_t i = 0; i < n; ++i) c[i] = splitmix(&seed) >= zero_below;
            check(c, "random");
        }
    }
    printf("%s: %llu strings, %d failures\n", failed ? "FAILED" : "ok", (unsigned long long)n_strings, failed);
    return failed ? 1 : 0;
}
