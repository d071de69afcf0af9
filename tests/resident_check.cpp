// csrc/resident.h against a loop over the mask's bits: boundaries, open and closed flags, the partition and the bound on
// a tile's length, over edge masks (an end bit at every position around t B and t B + L) and random ones.
// tests/test_resident_cpu.py builds and runs it, plain and under ASan + UBSan.
#include "resident.h"

#include <cstdio>
#include <random>
#include <vector>

using namespace mbpe;

static long checks = 0, failures = 0;
#define CHECK(cond) do { ++checks; if (!(cond) && ++failures <= 20) std::printf("FAILED line %d: %s\n", __LINE__, #cond); } while (0)

// the definition, bit by bit: the mask as bytes, bit i & 7 of byte i >> 3
static ResBound brute_bound(const std::vector<uint8_t> &bits, uint64_t n, uint64_t t) {
    const uint64_t n_tiles = (n + kResB - 1) / kResB;
    if (t == 0) return {0, true};
    if (t >= n_tiles) return {n, true};
    for (uint64_t p = t * kResB - 1; p < t * kResB - 1 + kResL && p < n; ++p)
        if ((bits[p >> 3] >> (p & 7)) & 1) return {p + 1, true};
    return {t * kResB, false};
}

// ends: the positions of the end bits (those at or beyond n are set too: bits past the piece must not count)
static void check_mask(uint64_t n, const std::vector<uint64_t> &ends) {
    const uint64_t n_words = (n + 31) / 32 + 1;                       // exactly what the kernel may read, and a word
    std::vector<uint32_t> words(n_words, 0);
    std::vector<uint8_t> bits(n_words * 4, 0);
    for (uint64_t p : ends) {
        if (p >= n_words * 32) continue;
        words[p >> 5] |= 1u << (p & 31);
        bits[p >> 3] |= (uint8_t)(1u << (p & 7));
    }
    const uint64_t n_tiles = res_tile_count(n);
    uint64_t at = 0;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        const ResBound a = res_bound(words.data(), n, t), want = brute_bound(bits, n, t), b = brute_bound(bits, n, t + 1);
        CHECK(a.lo == want.lo && a.closed == want.closed);
        const ResTile g = res_tile(words.data(), n, t);
        CHECK(g.lo == at);                                            // the tiles partition the piece, in order
        CHECK(g.lo == want.lo && g.lo + g.len == b.lo && g.len <= kResMax);
        CHECK(g.resident == (want.closed && b.closed));
        if (t > 0 && want.closed) CHECK((bits[(g.lo - 1) >> 3] >> ((g.lo - 1) & 7)) & 1);   // a chunk ends right before
        at = g.lo + g.len;
    }
    CHECK(at == n);
    CHECK(res_bound(words.data(), n, n_tiles).lo == n && res_bound(words.data(), n, n_tiles).closed);
}

int main() {
    // one end bit at every position around the first and last byte the search of tiles 1 and 2 sees
    for (uint64_t t = 1; t <= 2; ++t)
        for (int64_t d = -3; d <= (int64_t)kResL + 2; ++d) {
            const uint64_t p = t * kResB + d;
            for (uint64_t n : {(uint64_t)3000, p + 1, p + 2, t * kResB + 1, t * kResB + kResL})
                if (n > 0) check_mask(n, {p, n - 1});
        }
    // sizes around one tile; no end bit at all; bits beyond the piece only
    for (uint64_t n : {1, 2, 31, 32, 33, 767, 768, 769, 1023, 1024, 1025, 1536, 1537, 5000}) {
        check_mask(n, {});
        check_mask(n, {n, n + 1, n + 5});
        std::vector<uint64_t> all;
        for (uint64_t p = 0; p < n; ++p) all.push_back(p);
        check_mask(n, all);                                           // chunks of one byte
    }
    std::mt19937_64 rng(7);
    for (int round = 0; round < 400; ++round) {
        const uint64_t n = 1 + rng() % 12000;
        const uint64_t mean = 1 + rng() % (round % 4 == 0 ? 2000 : 40);
        std::vector<uint64_t> ends;
        for (uint64_t p = rng() % mean; p < n; p += 1 + rng() % (2 * mean)) ends.push_back(p);
        ends.push_back(n - 1);
        if (round % 3 == 0) ends.push_back(n + rng() % 31);
        check_mask(n, ends);
    }
    std::printf("ok: %ld checks, %ld failures\n", checks, failures);
    return failures ? 1 : 0;
}
