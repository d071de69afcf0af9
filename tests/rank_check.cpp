// Stand-alone check of the pure arithmetic of csrc/rank.h, built by the host compiler (tests/test_rank_cpu.py).
//   part 1: rank_fold is associative and rank_empty is its identity (all triples over a small set of summaries)
//   part 2: cand values and end flags -> the segmented minimum of every position, the way the kernels of encode.hip
//           take it -- in a group by rank_scan_step (the shuffles are array reads here), a span's summary by
//           rank_head_part / rank_tail_part, the spans by the sliced scan (rank_fold_slice, then rank_carry in both
//           directions), the groups of a span by rank_carry again -- against a brute-force minimum per segment.
//           The span summaries are also compared with the fold of the groups' summaries.
// span_scan_min and the kernels are device code: their slicing, barriers and shuffles are guarded by the GPU tests.
#include "rank.h"

#include <cstdio>
#include <vector>

using namespace mbpe;

static bool same(RankSum a, RankSum b) { return a.has_end == b.has_end && a.head == b.head && a.tail == b.tail; }

static int check_fold() {
    std::vector<RankSum> v;
    const uint32_t vals[] = {kTokNone, 256u, 300u, 0x7FFFFFFDu};
    for (uint32_t h : vals) {
        v.push_back({0u, h, h});                       // (without an end flag head and tail are the same minimum)
        for (uint32_t t : vals) v.push_back({1u, h, t});
    }
    int bad = 0;
    for (const RankSum &a : v) {
        if (!same(rank_fold(rank_empty(), a), a) || !same(rank_fold(a, rank_empty()), a)) { printf("identity fails\n"); ++bad; }
        for (const RankSum &b : v)
            for (const RankSum &c : v)
                if (!same(rank_fold(rank_fold(a, b), c), rank_fold(a, rank_fold(b, c)))) {
                    if (!bad) printf("fold not associative\n");
                    ++bad;
                }
    }
    return bad;
}

struct Str { std::vector<uint32_t> c; std::vector<uint8_t> e; };

static unsigned long long end_mask(const Str &s, uint64_t at) {
    unsigned long long E = 0;
    for (uint64_t l = 0; l < (uint64_t)kWave && at + l < s.e.size(); ++l) E |= (unsigned long long)s.e[at + l] << l;
    return E;
}

// group_seg_min of encode.hip for the 64 positions from `at`; positions at or beyond the end hold kTokNone
static void group_min(const Str &s, uint64_t at, unsigned long long E, uint32_t *m) {
    uint32_t v[kWave], nxt[kWave];
    for (uint32_t l = 0; l < (uint32_t)kWave; ++l) v[l] = at + l < s.c.size() ? s.c[at + l] : kTokNone;
    for (uint32_t d = 1; d < (uint32_t)kWave; d <<= 1) {
        for (uint32_t l = 0; l < (uint32_t)kWave; ++l)
            nxt[l] = rank_scan_step(v[l], l >= d ? v[l - d] : v[l], l, d, rank_seg_lo(E, lanes_below(l)));
        for (uint32_t l = 0; l < (uint32_t)kWave; ++l) v[l] = nxt[l];
    }
    for (uint32_t l = 0; l < (uint32_t)kWave; ++l) m[l] = v[rank_seg_hi(E, lanes_below(l))];
}

static std::vector<RankSum> sum, sh;
static std::vector<uint32_t> in_left, in_right, sh_l, sh_r, got, want;

static uint64_t check_string(const Str &s, uint64_t slices, const char *what) {
    const uint64_t n = s.c.size(), n_spans = span_count(n);
    sum.resize(n_spans); in_left.resize(n_spans); in_right.resize(n_spans);
    sh.resize(slices); sh_l.resize(slices); sh_r.resize(slices);
    got.assign(n, 0); want.assign(n, 0);
    uint64_t bad = 0;
    // k_enc_rank_sum
    for (uint64_t sp = 0; sp < n_spans; ++sp) {
        uint32_t h[kWave], t[kWave];
        for (int l = 0; l < kWave; ++l) h[l] = t[l] = kTokNone;
        bool seen = false;
        RankSum by_groups = rank_empty();
        for (int it = 0; it < kSpanIters; ++it) {
            const uint64_t at = sp * kSpan + (uint64_t)it * kWave;
            const unsigned long long E = end_mask(s, at);
            for (uint32_t l = 0; l < (uint32_t)kWave; ++l) {
                const uint32_t c = at + l < n ? s.c[at + l] : kTokNone;
                h[l] = rank_head_part(h[l], seen, E, l, c);
                t[l] = rank_tail_part(t[l], E, l, c);
            }
            seen = seen || E != 0ull;
            uint32_t m[kWave];
            group_min(s, at, E, m);
            by_groups = rank_fold(by_groups, {E != 0ull ? 1u : 0u, m[0], E >> 63 ? kTokNone : m[kWave - 1]});
        }
        RankSum r = {seen ? 1u : 0u, kTokNone, kTokNone};
        for (int l = 0; l < kWave; ++l) { r.head = rank_min(r.head, h[l]); r.tail = rank_min(r.tail, t[l]); }
        if (!same(r, by_groups)) {
            if (!bad) printf("%s, n = %llu: the summary of span %llu differs from the fold of its groups\n", what,
                             (unsigned long long)n, (unsigned long long)sp);
            ++bad;
        }
        sum[sp] = r;
    }
    // span_scan_min, one "thread" after the other
    const uint64_t per = (n_spans + slices - 1) / slices;
    auto lo_of = [&](uint64_t t) { return per * t < n_spans ? per * t : n_spans; };
    auto hi_of = [&](uint64_t t) { return lo_of(t) + per < n_spans ? lo_of(t) + per : n_spans; };
    for (uint64_t t = 0; t < slices; ++t) sh[t] = rank_fold_slice(sum.data(), lo_of(t), hi_of(t));
    uint32_t run = kTokNone;
    for (uint64_t t = 0; t < slices; ++t) { sh_l[t] = run; run = rank_carry(run, sh[t].has_end, sh[t].tail); }
    run = kTokNone;
    for (uint64_t t = slices; t > 0; --t) { sh_r[t - 1] = run; run = rank_carry(run, sh[t - 1].has_end, sh[t - 1].head); }
    for (uint64_t t = 0; t < slices; ++t) {
        run = sh_l[t];
        for (uint64_t sp = lo_of(t); sp < hi_of(t); ++sp) { in_left[sp] = run; run = rank_carry(run, sum[sp].has_end, sum[sp].tail); }
        run = sh_r[t];
        for (uint64_t sp = hi_of(t); sp > lo_of(t); --sp) {
            in_right[sp - 1] = run;
            run = rank_carry(run, sum[sp - 1].has_end, sum[sp - 1].head);
        }
    }
    // k_enc_rank_filter
    for (uint64_t sp = 0; sp < n_spans; ++sp) {
        uint32_t m[kSpanIters][kWave], head[kSpanIters], tail[kSpanIters], left[kSpanIters], right[kSpanIters];
        unsigned long long E[kSpanIters];
        for (int it = 0; it < kSpanIters; ++it) {
            const uint64_t at = sp * kSpan + (uint64_t)it * kWave;
            E[it] = end_mask(s, at);
            group_min(s, at, E[it], m[it]);
            head[it] = m[it][0];
            tail[it] = E[it] >> 63 ? kTokNone : m[it][kWave - 1];
        }
        run = in_left[sp];
        for (int it = 0; it < kSpanIters; ++it) { left[it] = run; run = rank_carry(run, E[it] != 0ull, tail[it]); }
        run = in_right[sp];
        for (int it = kSpanIters - 1; it >= 0; --it) { right[it] = run; run = rank_carry(run, E[it] != 0ull, head[it]); }
        for (int it = 0; it < kSpanIters; ++it)
            for (uint32_t l = 0; l < (uint32_t)kWave; ++l) {
                const uint64_t i = sp * kSpan + (uint64_t)it * kWave + l;
                if (i >= n) continue;
                const unsigned long long lt = lanes_below(l);
                uint32_t v = m[it][l];
                if (rank_open_left(E[it], lt)) v = rank_min(v, left[it]);
                if (rank_open_right(E[it], lt)) v = rank_min(v, right[it]);
                got[i] = v;
            }
    }
    // brute force: a segment ends at (and includes) a flagged position, or at the end of the string
    for (uint64_t a = 0; a < n;) {
        uint64_t b = a;
        while (b < n && !s.e[b]) ++b;
        if (b < n) ++b;
        uint32_t mn = kTokNone;
        for (uint64_t i = a; i < b; ++i) mn = rank_min(mn, s.c[i]);
        for (uint64_t i = a; i < b; ++i) want[i] = mn;
        a = b;
    }
    for (uint64_t i = 0; i < n; ++i)
        if (got[i] != want[i]) {
            if (!bad) printf("%s, n = %llu, %llu slices: position %llu has minimum %u, rank.h says %u\n", what,
                             (unsigned long long)n, (unsigned long long)slices, (unsigned long long)i, want[i], got[i]);
            ++bad;
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
    int failed = check_fold();
    const uint64_t lengths[] = {1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 5 * 1024 + 17};
    const uint64_t slicings[] = {1, 2, 3, (uint64_t)kScanThreads};
    uint64_t n_strings = 0, seed = 20250314;
    auto check = [&](const Str &s, const char *what) {
        ++n_strings;
        for (uint64_t slices : slicings) failed += check_string(s, slices, what) != 0;
    };
    for (uint64_t n : lengths) {
        Str s;
        auto descending = [&]() { for (uint64_t i = 0; i < n; ++i) s.c[i] = 256u + (uint32_t)(n - i); };
        // one segment over everything, the minimum in the first / a middle / the last group (or nowhere)
        s.c.assign(n, kTokNone); s.e.assign(n, 0);
        check(s, "no candidate, no end");
        const uint64_t spots[] = {0, n / 2, n - 1};
        for (uint64_t at : spots) {
            for (uint64_t i = 0; i < n; ++i) s.c[i] = 1000u + (uint32_t)(i % 7);
            s.c[at] = 256u;
            check(s, "one segment, one minimum");
            s.e[n - 1] = 1;
            check(s, "one segment that ends at the last position");
            s.e[n - 1] = 0;
        }
        // one end flag at every lane of the first group, and of the last group of the first span
        const uint64_t firsts[] = {0, (uint64_t)(kSpan - kWave)};
        for (uint64_t first : firsts)
            for (uint64_t l = 0; l < (uint64_t)kWave && first + l < n; ++l) {
                s.c.assign(n, kTokNone); s.e.assign(n, 0);
                descending();
                s.e[first + l] = 1;
                check(s, "one end flag, descending ids");
                for (uint64_t i = 0; i < n; ++i) s.c[i] = 256u + (uint32_t)i;
                check(s, "one end flag, ascending ids");
            }
        // every position ends a segment; segments of 2 and of 64 that end at lanes 63 and 62
        s.e.assign(n, 1);
        descending();
        check(s, "every position an end");
        for (uint64_t i = 0; i < n; ++i) s.e[i] = i & 1;
        check(s, "segments of two");
        for (uint64_t i = 0; i < n; ++i) s.e[i] = i % kWave == (uint64_t)kWave - 1;
        check(s, "segments end at lane 63");
        for (uint64_t i = 0; i < n; ++i) s.e[i] = i % kWave == (uint64_t)kWave - 2;
        check(s, "segments end at lane 62");
        for (uint64_t i = 0; i < n; ++i) s.e[i] = i % kWave == 0;
        check(s, "segments end at lane 0");
        // groups without a candidate between groups with some
        for (uint64_t i = 0; i < n; ++i) { s.c[i] = (i / kWave) % 3 == 1 ? 256u + (uint32_t)(i % 50) : kTokNone; s.e[i] = i % 777 == 776; }
        check(s, "all-none groups");
        // random: end flags with probability 2^-k (segments from a few positions to several spans), few or many ids
        for (int k = 0; k < 28; ++k) {
            const uint64_t end_below = 1ull << (63 - k % 14);
            const uint32_t ids = k < 14 ? 5u : 2000u;
            for (uint64_t i = 0; i < n; ++i) {
                s.e[i] = splitmix(&seed) < end_below;
                s.c[i] = splitmix(&seed) % 3 == 0 ? kTokNone : 256u + (uint32_t)(splitmix(&seed) % ids);
            }
            check(s, "random");
        }
    }
    printf("%s: %llu strings, %d failures\n", failed ? "FAILED" : "ok", (unsigned long long)n_strings, failed);
    return failed ? 1 : 0;
}
