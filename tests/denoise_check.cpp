// A stand-alone check of csrc/denoise.h, the one statement of the span-corruption rule that the host's plan, the length
// kernel and the gather kernels share (tests/test_denoise_cpu.py builds it plain and with -fsanitize=address,undefined):
//   - for every unit length 0 .. 80, 511, 512, 568, 1025 and 5000 over a grid of densities, means and sentinel limits:
//     the counts obey their clamps, both boundary lists ascend strictly from 0 to their total, and BOTH position -> source
//     maps -- position by position, and as a walk begun at any position -- equal a direct construction of the two streams
//     from the boundary lists;
//   - the three anchors: T5's 568 -> 511 / 113 and 512 -> 461 / 103, the 20-token unit, the six units of four documents;
//   - the host's plan against sums of the counts, its caps, the unit of 2^32 - 1 tokens (named; none with density 0 or
//     with segments), and the longest unit there is, 2^32 - 2: no product wraps;
//   - the spec's own rules.
#include "denoise.h"

#include <cstdio>
#include <vector>

using namespace mbpe;

static unsigned long long g_checks = 0, g_failures = 0;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond)) {                                                               \
            ++g_failures;                                                            \
            if (g_failures <= 20) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
        }                                                                            \
    } while (0)

typedef unsigned long long ull;

static mbpe_denoise_spec make_spec(uint64_t density, uint32_t mean_q8, uint32_t n_sent, uint64_t seed, uint64_t base) {
    mbpe_denoise_spec s = {};
    s.density = density;
    s.seed = seed;
    s.doc_base = base;
    s.mean_span_q8 = mean_q8;
    s.sentinel_id = 32099;
    s.sentinel_down = 1;
    s.n_sentinels = n_sent;
    return s;
}

// boundary j as the rule writes it, with the strata by plain 64-bit division (denoise.h gets by with one 32-bit one)
static ull literal(ull su, ull T, ull S, uint32_t c, ull j) {
    const ull E = T - S, q0 = ((j - 1) * E) / S, q1 = (j * E) / S;
    return j + q0 + (((ull)drop_hash(su, j, c) * (q1 - q0 + 1)) >> 32);
}

// the two streams of a unit over the tokens 0 .. L - 1, built part by part from the boundary lists; sentinel j as
// kDnSent | j
static void construct(const DnUnit &u, std::vector<ull> *in, std::vector<ull> *tg) {
    in->clear();
    tg->clear();
    if (u.S == 0) {
        for (ull i = 0; i < u.L; ++i) in->push_back(i);
        return;
    }
    ull p = 0;
    for (ull j = 0; j < u.S; ++j) {
        const ull m = dn_bm(u, j + 1) - dn_bm(u, j), n = dn_bn(u, j + 1) - dn_bn(u, j);
        for (ull i = 0; i < m; ++i) in->push_back(p++);
        in->push_back(kDnSent | j);
        tg->push_back(kDnSent | j);
        for (ull i = 0; i < n; ++i) tg->push_back(p++);
    }
}

static void check_unit(const mbpe_denoise_spec &s, ull d, ull L, bool walks) {
    const DnUnit u = dn_unit(s, d, L, 3);
    const DnCounts c = dn_counts(s, L);
    CHECK(u.N == c.N && u.S == c.S && u.L == L);
    if (s.density == 0 || L < 2) CHECK(c.S == 0 && c.N == 0);
    if (c.S) {
        CHECK(c.N >= 1 && c.N <= L - 1 && c.S >= 1 && c.S <= c.N && c.S <= L - c.N && c.S <= s.n_sentinels);
        CHECK(dn_bn(u, 0) == 0 && dn_bn(u, c.S) == c.N && dn_bm(u, 0) == 0 && dn_bm(u, c.S) == L - c.N);
        for (ull j = 0; j < c.S; ++j) CHECK(dn_bn(u, j) < dn_bn(u, j + 1) && dn_bm(u, j) < dn_bm(u, j + 1));
        for (ull j = 1; j < c.S; ++j) CHECK(dn_bn(u, j) == literal(u.su, c.N, c.S, 0, j) &&
                                            dn_bm(u, j) == literal(u.su, L - c.N, c.S, 1, j));
    }
    std::vector<ull> in, tg;
    construct(u, &in, &tg);
    CHECK(in.size() == dn_in_len(c, L) && tg.size() == (c.S ? dn_tg_len(c) : 0));
    std::vector<char> seen(L, 0);
    for (ull v : in) if (!(v & kDnSent)) { CHECK(v < L && !seen[v]); if (v < L) seen[v] = 1; }
    for (ull v : tg) if (!(v & kDnSent)) { CHECK(v < L && !seen[v]); if (v < L) seen[v] = 1; }
    for (ull i = 0; i < L; ++i) CHECK(seen[i]);
    for (ull p = 0; p < in.size(); ++p) CHECK(dn_in_source(u, p) == in[p]);
    for (ull p = 0; p < tg.size(); ++p) CHECK(dn_tg_source(u, p) == tg[p]);
    if (!walks) return;
    for (ull p0 = 0; p0 < in.size(); p0 += (in.size() > 200 ? 37 : 1)) {
        DnCur cur;
        dn_in_seek(u, p0, &cur);
        for (ull p = p0; p < in.size(); ++p) CHECK(dn_in_step(u, p, &cur) == in[p]);
    }
    for (ull p0 = 0; p0 < tg.size(); p0 += (tg.size() > 200 ? 37 : 1)) {
        DnTgCur cur;
        dn_tg_seek(u, p0, &cur);
        for (ull p = p0; p < tg.size(); ++p) CHECK(dn_tg_step(u, p, &cur) == tg[p]);
    }
    {                                                            // a walk from the start needs no seek
        DnCur ci;
        dn_in_enter(u, 0, &ci);
        for (ull p = 0; p < in.size(); ++p) CHECK(dn_in_step(u, p, &ci) == in[p]);
        if (c.S) {
            DnTgCur ct;
            dn_tg_enter(u, 0, 0, &ct);
            for (ull p = 0; p < tg.size(); ++p) CHECK(dn_tg_step(u, p, &ct) == tg[p]);
        }
    }
}

int main() {
    const uint64_t dens[] = {0, (uint64_t)(0.15 * 4294967296.0), 1ull << 31, 1ull << 32, 1};
    const uint32_t shapes[][2] = {{768, 100}, {256, 100}, {768, 2}, {1280, 1}, {256, 3}, {300, 65000}};
    std::vector<ull> lens;
    for (ull L = 0; L <= 80; ++L) lens.push_back(L);
    for (ull L : {511ull, 512ull, 568ull, 1025ull, 5000ull}) lens.push_back(L);
    for (uint64_t de : dens)
        for (const auto &sh : shapes)
            for (ull L : lens)
                for (ull d = 0; d < (L <= 80 ? 3u : 1u); ++d)
                    check_unit(make_spec(de, sh[0], sh[1], 11 + d, d * 0x100000000ull), d, L, true);
    check_unit(make_spec(1ull << 31, 256, 65000, 5, 0), 0, 70000, false);    // 35,000 parts of one token each

    // the anchors
    const mbpe_denoise_spec t5 = make_spec((uint64_t)(0.15 * 4294967296.0), 768, 100, 0, 0);
    DnCounts c = dn_counts(t5, 568);
    CHECK(c.N == 85 && c.S == 28 && dn_in_len(c, 568) == 511 && dn_tg_len(c) == 113);
    c = dn_counts(t5, 512);
    CHECK(c.N == 77 && c.S == 26 && dn_in_len(c, 512) == 461 && dn_tg_len(c) == 103);
    {
        const DnUnit u = dn_unit(t5, 0, 20, 0);
        CHECK(u.N == 3 && u.S == 1);
        for (ull p = 0; p < 17; ++p) CHECK(dn_in_source(u, p) == p);
        CHECK(dn_in_source(u, 17) == kDnSent && dn_sentinel(t5, 0) == 32099);
        CHECK(dn_tg_source(u, 0) == kDnSent);
        for (ull p = 1; p < 4; ++p) CHECK(dn_tg_source(u, p) == 16 + p);
    }
    {
        mbpe_denoise_spec s = t5;
        s.segment_tokens = 568;
        const uint64_t off[5] = {0, 0, 1, 569, 2000};
        uint64_t n = 0, bad = 0, in_off[7], tg_off[7], doc[6];
        CHECK(denoise_plan_host(off, 4, s, &n, in_off, tg_off, doc, 6, &bad) == MBPE_OK && n == 6);
        const uint64_t want_doc[6] = {0, 1, 2, 3, 3, 3};
        for (int k = 0; k < 6; ++k) CHECK(doc[k] == want_doc[k]);
        CHECK(in_off[1] == 0 && in_off[2] == 1 && in_off[3] == 512 && in_off[4] == 1023 && in_off[5] == 1534);
        CHECK(tg_off[2] == 0 && tg_off[3] == 113 && tg_off[5] == 339);
        c = dn_counts(s, 1431 - 2 * 568);
        CHECK(in_off[6] - in_off[5] == dn_in_len(c, 295) && tg_off[6] - tg_off[5] == dn_tg_len(c));
        CHECK(dn_units(s, 0) == 1 && dn_units(s, 568) == 1 && dn_units(s, 569) == 2 && dn_units(s, 1431) == 3);
        CHECK(dn_unit_len(s, 1431, 2) == 295 && dn_unit_len(s, 569, 1) == 1 && dn_unit_len(s, 0, 0) == 0);
        // a cap too small reports the count and writes nothing
        uint64_t guard[2] = {77, 77};
        CHECK(denoise_plan_host(off, 4, s, &n, guard, guard, guard, 5, &bad) == MBPE_OK && n == 6);
        CHECK(guard[0] == 77 && guard[1] == 77);
    }

    // the limits: a unit of 2^32 - 1 tokens is the call's error while density > 0, the longest one is 2^32 - 2
    {
        const uint64_t off[4] = {0, 4, 4 + 0xFFFFFFFFull, 7 + 0x100000000ull};
        uint64_t n = 0, bad = 0;
        mbpe_denoise_spec s = make_spec(1, 768, 100, 0, 0);
        CHECK(denoise_plan_host(off, 3, s, &n, nullptr, nullptr, nullptr, 0, &bad) == MBPE_ERR_ARG && bad == 1);
        s.density = 0;
        CHECK(denoise_plan_host(off, 3, s, &n, nullptr, nullptr, nullptr, 0, &bad) == MBPE_OK && n == 3);
        s.density = 1ull << 32;
        s.segment_tokens = 1000;
        CHECK(denoise_plan_host(off, 3, s, &n, nullptr, nullptr, nullptr, 0, &bad) == MBPE_OK && n == 2 + 4294968);
        s.segment_tokens = 0xFFFFFFFFu;
        CHECK(denoise_plan_host(off, 3, s, &n, nullptr, nullptr, nullptr, 0, &bad) == MBPE_ERR_ARG && bad == 1);
        s.segment_tokens = 0;
        const ull L = kDnMaxLen;
        for (uint64_t de : {1ull, 1ull << 31, 1ull << 32}) {
            s = make_spec(de, 768, 0xFFFFFFFFu, 3, ~0ull);
            s.sentinel_down = 0;
            s.sentinel_id = 0;
            c = dn_counts(s, L);
            CHECK(c.N >= 1 && c.N <= L - 1 && c.S >= 1 && c.S <= c.N && c.S <= L - c.N);
            if (de == 1ull << 31) CHECK(c.N == (L + 1) / 2 && c.S == (c.N * 256 + 384) / 768);
            const DnUnit u = dn_unit(s, 5, L, 0);
            ull prev_n = 0, prev_m = 0;
            for (ull j : {1ull, 2ull, c.S / 2, c.S - 1, c.S}) {
                if (j == 0 || j > c.S) continue;
                const ull bn = dn_bn(u, j), bm = dn_bm(u, j);
                if (j < c.S) CHECK(bn == literal(u.su, c.N, c.S, 0, j) && bm == literal(u.su, L - c.N, c.S, 1, j));
                CHECK(bn >= j && bn <= c.N && bm >= j && bm <= L - c.N && bn >= prev_n && bm >= prev_m);
                prev_n = bn;
                prev_m = bm;
            }
            CHECK(dn_in_source(u, dn_in_len(c, L) - 1) == (kDnSent | (c.S - 1)));
            CHECK(dn_tg_source(u, 0) == kDnSent);
            CHECK(dn_tg_source(u, dn_tg_len(c) - 1) == L - 1);           // a unit ends with noise
            CHECK(dn_in_source(u, 0) == 0);                              // and begins with kept text
        }
        CHECK(dn_counts(make_spec(1ull << 32, 768, 100, 0, 0), L + 1).S == 0);
    }

    // min_tokens
    {
        mbpe_denoise_spec s = make_spec(1ull << 31, 768, 100, 0, 0);
        s.min_tokens = 10;
        CHECK(dn_counts(s, 9).S == 0 && dn_counts(s, 10).S >= 1);
        s.min_tokens = 0;
        CHECK(dn_counts(s, 1).S == 0 && dn_counts(s, 2).S == 1 && dn_counts(s, 2).N == 1);
    }

    // the spec's rules
    {
        const char *msg = nullptr;
        mbpe_denoise_spec s = make_spec(1ull << 31, 768, 100, 0, 0);
        CHECK(denoise_check_spec(&s, 32, &msg) == MBPE_OK && denoise_check_spec(&s, 16, &msg) == MBPE_OK);
        CHECK(denoise_check_spec(nullptr, 32, &msg) == MBPE_ERR_ARG && msg[0]);
        s.density = (1ull << 32) + 1;
        CHECK(denoise_check_spec(&s, 32, &msg) == MBPE_ERR_ARG);
        s = make_spec(1, 255, 100, 0, 0);
        CHECK(denoise_check_spec(&s, 32, &msg) == MBPE_ERR_ARG);
        s = make_spec(1, 256, 0, 0, 0);
        CHECK(denoise_check_spec(&s, 32, &msg) == MBPE_ERR_ARG);
        s = make_spec(1, 256, 100, 0, 0);
        s.sentinel_down = 2;
        CHECK(denoise_check_spec(&s, 32, &msg) == MBPE_ERR_ARG);
        s.sentinel_down = 1;
        s.sentinel_id = 98;                                      // 98 - 99 < 0
        CHECK(denoise_check_spec(&s, 32, &msg) == MBPE_ERR_ARG);
        s.sentinel_id = 99;
        CHECK(denoise_check_spec(&s, 32, &msg) == MBPE_OK);
        s.sentinel_id = 0x7FFFFFFEu;
        CHECK(denoise_check_spec(&s, 32, &msg) == MBPE_ERR_ARG);
        s.sentinel_id = 0x7FFFFFFDu;
        CHECK(denoise_check_spec(&s, 32, &msg) == MBPE_OK && denoise_check_spec(&s, 16, &msg) == MBPE_ERR_VOCAB);
        s.sentinel_down = 0;
        CHECK(denoise_check_spec(&s, 32, &msg) == MBPE_ERR_ARG);  // + 99 leaves the range
        s.sentinel_id = 0x7FFFFFFEu - 100;
        CHECK(denoise_check_spec(&s, 32, &msg) == MBPE_OK);
        s.sentinel_id = 65436;                                   // .. 65,535
        CHECK(denoise_check_spec(&s, 16, &msg) == MBPE_OK);
        s.sentinel_id = 65437;
        CHECK(denoise_check_spec(&s, 16, &msg) == MBPE_ERR_VOCAB && denoise_check_spec(&s, 32, &msg) == MBPE_OK);
        s.sentinel_down = 1;
        s.sentinel_id = 65536;
        CHECK(denoise_check_spec(&s, 16, &msg) == MBPE_ERR_VOCAB);
        s.sentinel_id = 65535;
        CHECK(denoise_check_spec(&s, 16, &msg) == MBPE_OK);
        s.n_sentinels = 0xFFFFFFFFu;
        CHECK(denoise_check_spec(&s, 32, &msg) == MBPE_ERR_ARG);
    }

    if (g_failures) {
        std::printf("FAILED: %llu of %llu checks\n", g_failures, g_checks);
        return 1;
    }
    std::printf("ok: %llu checks, 0 failures\n", g_checks);
    return 0;
}
