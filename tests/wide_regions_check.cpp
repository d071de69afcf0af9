// Stand-alone check of the general region cutter (region_plan and region_cut of csrc/wide_regions.h, over
// region_boundary of csrc/wide_resident.h): on streams of random chunks the regions cover the whole stream, ascend,
// are cut behind chunk ends only and report a region beyond the capacity; with 16 regions they are resident_cut's.
#include "wide_regions.h"

#include <cstdio>
#include <vector>

using namespace mbpe;

static int checks = 0, failures = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { ++failures; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); } } while (0)

static uint64_t rng_state = 43;
static uint32_t rnd(uint32_t n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % n);
}

static std::vector<uint32_t> stream(uint32_t n, uint32_t max_chunk, uint32_t *longest) {
    std::vector<uint32_t> tok(n ? n : 1, 7u);
    *longest = 0;
    for (uint32_t i = 0; i < n;) {
        const uint32_t len = 1 + rnd(max_chunk);
        const uint32_t end = i + len < n ? i + len : n;
        tok[end - 1] |= kTokEnd;
        *longest = end - i > *longest ? end - i : *longest;
        i = end;
    }
    return tok;
}

static void one(uint32_t n, uint32_t max_chunk, uint32_t region_tokens, uint32_t cap) {
    uint32_t longest;
    const std::vector<uint32_t> tok = stream(n, max_chunk, &longest);
    const RegionPlan p = region_plan(n, region_tokens);
    CHECK(p.count >= 1 && p.count <= kRegMaxRegions && (uint64_t)p.per * p.count >= n && p.per >= region_tokens);
    uint32_t at = 0;
    bool all_ok = true;
    for (uint32_t r = 0; r < p.count; ++r) {
        const RegionCut c = region_cut(tok.data(), n, p, r, cap);
        all_ok = all_ok && c.ok;
        if (!c.ok) continue;
        CHECK(c.off >= at && c.len <= cap && c.off + c.len <= n);
        // a region starts where the one before ended, behind a chunk end
        CHECK(c.off == 0 || (tok[c.off - 1] & kTokEnd));
        if (all_ok) CHECK(c.off == at);
        at = c.off + c.len;
    }
    if (all_ok) CHECK(at == n);
    // refused exactly when the uncapped cut holds a region beyond the capacity
    bool fits = true;
    for (uint32_t r = 0; r < p.count; ++r) {
        const uint32_t lo = region_boundary(tok.data(), n, p.per, p.count, r, n);
        const uint32_t hi = region_boundary(tok.data(), n, p.per, p.count, r + 1, n);
        CHECK(lo <= hi && hi <= n);
        fits = fits && hi - lo <= cap;
    }
    CHECK(all_ok == fits);
    if (longest > cap) CHECK(!all_ok);
}

static void as_resident(uint32_t n, uint32_t max_chunk) {
    uint32_t longest;
    const std::vector<uint32_t> tok = stream(n, max_chunk, &longest);
    uint32_t off[kResRegions + 1];
    resident_cut(tok.data(), n, kResRegionCap, off);
    const uint32_t per = (n + kResRegions - 1) / kResRegions;
    for (uint32_t r = 0; r <= kResRegions; ++r) CHECK(region_boundary(tok.data(), n, per, kResRegions, r, n) == off[r]);
}

int main() {
    for (uint32_t n : {0u, 1u, 2u, 63u, 64u, 65u, 129u, 1000u, 4099u})
        for (uint32_t max_chunk : {1u, 2u, 12u, 300u, 5000u})
            for (uint32_t region_tokens : {kRegTokensMin, 512u, kRegTokensMax})
                for (uint32_t cap : {64u, 4096u, kResRegionCap}) one(n, max_chunk, region_tokens, cap);
    // a chunk beyond the real capacity: the capped scan gives up, the cut is refused
    one(70003, 70000, 512, kResRegionCap);
    one(140001, 70000, 2048, kResRegionCap);
    // more tokens than kRegMaxRegions regions of "region_tokens" hold: the regions grow
    one(kRegMaxRegions * 64u + 5u, 12, kRegTokensMin, kResRegionCap);
    for (uint32_t n : {0u, 1u, 15u, 16u, 17u, 100u, 4099u})
        for (uint32_t max_chunk : {1u, 3u, 300u}) as_resident(n, max_chunk);
    std::printf("ok: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
