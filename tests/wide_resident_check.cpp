// Stand-alone check of the region cutter of csrc/wide_resident.h (resident_cut): on streams of random chunks the 17
// offsets start at 0, end at n, ascend, fall on chunk ends only, and report a region beyond the capacity.
#include "wide_resident.h"

#include <cstdio>
#include <vector>

using namespace mbpe;

static int checks = 0, failures = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { ++failures; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); } } while (0)

static uint64_t rng_state = 42;
static uint32_t rnd(uint32_t n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % n);
}

static void one(uint32_t n, uint32_t max_chunk, uint32_t cap) {
    std::vector<uint32_t> tok(n ? n : 1, 7u);
    uint32_t longest = 0;
    for (uint32_t i = 0; i < n;) {
        const uint32_t len = 1 + rnd(max_chunk);
        const uint32_t end = i + len < n ? i + len : n;
        tok[end - 1] |= kTokEnd;
        longest = end - i > longest ? end - i : longest;
        i = end;
    }
    uint32_t off[kResRegions + 1];
    const bool ok = resident_cut(tok.data(), n, cap, off);
    CHECK(off[0] == 0 && off[kResRegions] == n);
    bool fits = true;
    for (uint32_t r = 0; r < kResRegions; ++r) {
        CHECK(off[r] <= off[r + 1]);
        CHECK(off[r + 1] == 0 || (tok[off[r + 1] - 1] & kTokEnd));
        // balanced: a region overshoots its share of ceil(n / 16) tokens by less than one chunk
        CHECK(off[r + 1] < (uint64_t)(r + 1) * ((n + kResRegions - 1) / kResRegions) + longest || off[r + 1] == n);
        fits = fits && off[r + 1] - off[r] <= cap;
    }
    CHECK(ok == fits);
}

int main() {
    for (uint32_t n : {0u, 1u, 2u, 5u, 15u, 16u, 17u, 31u, 100u, 1000u, 4099u})
        for (uint32_t max_chunk : {1u, 2u, 3u, 12u, 300u, 5000u})
            for (uint32_t cap : {4u, 64u, kResRegionCap}) one(n, max_chunk, cap);
    std::printf("ok: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
