// One merge over one REGION of the 32-bit stream, by one wave, in place: the walk that k_wide_resident
// (wide_resident.hip, regions of one workgroup, table updates that keep LDS bounds) and k_wide_regions_walk
// (wide_regions.hip, regions over the whole chip, plain table updates) share.  A region is a stretch of whole chunks,
// so no pair crosses its ends and no other wave touches its tokens.  The walk is k_wide_cand + k_wide_match +
// k_wide_scatter of wide.hip at once; what differs between its users -- how a table update is made, where the region's
// length lives -- is a functor and the caller's business.
#ifndef MBPE_WIDE_WALK_H
#define MBPE_WIDE_WALK_H

#include "wide_dev.h"

namespace mbpe {

// tokens of one 64-lane step of a region, and the neighbours two to the left and two to the right of every lane:
// from the registers of the previous step (prv) and of the next (nxt), never from a second load
struct ResStep { uint32_t pp, p, nx, y; };
__device__ __forceinline__ ResStep res_neighbours(uint32_t prv, uint32_t cur, uint32_t nxt, uint32_t lane) {
    ResStep r;
    const uint32_t n0 = __shfl(nxt, 0, kWave), n1 = __shfl(nxt, 1, kWave);
    const uint32_t p63 = __shfl(prv, kWave - 1, kWave), p62 = __shfl(prv, kWave - 2, kWave);
    r.nx = __shfl_down(cur, 1, kWave);
    r.y = __shfl_down(cur, 2, kWave);
    r.p = __shfl_up(cur, 1, kWave);
    r.pp = __shfl_up(cur, 2, kWave);
    if (lane == kWave - 1) { r.nx = n0; r.y = n1; }
    if (lane == kWave - 2) r.y = n0;
    if (lane == 0) { r.p = p63; r.pp = p62; }
    if (lane == 1) r.pp = p63;
    return r;
}

// what a walk leaves, the same in every lane: the region's new length, its matches, and the sum of their weights
struct WalkOut { uint32_t len, n_match, w_match; };

// The merge (a, b) -> X over the n tokens at tok[base ..] (W: and their weights at wt[base ..]).  add(key, delta) makes
// the four neighbour updates of a match; the fifth, (a, b) - w_match, is the caller's, once per region.
// Positions beyond the region read as kTokNone, which carries the end flag: no candidate starts there, no neighbour
// is taken from there (the token before a region ends a chunk, so that is what k_wide_match sees too).  The step that
// follows is loaded before this step's tokens are stored, and a store goes to an index at or below the step's first:
// no store reaches a token that is still to be read.  Nothing is stored before the first candidate.
template <bool W, class Add>
__device__ __forceinline__ WalkOut wide_walk_region(uint32_t *tok, uint32_t *wt, uint32_t base, uint32_t n, uint32_t a,
                                                    uint32_t b, uint32_t X, uint32_t lane, const Add &add) {
    const unsigned long long lt = lanes_below(lane);
    uint32_t wpos = 0, carry = 0, n_match = 0, w_match = 0;
    bool dirty = false;                                    // a candidate was seen: from here on the region is rewritten
    uint32_t prv = kTokNone, cur = lane < n ? tok[base + lane] : kTokNone;
    uint32_t wcur = W && lane < n ? wt[base + lane] : 1u;
    for (uint32_t rpos = 0; rpos < n; rpos += kWave) {
        const uint32_t j = rpos + lane, jn = j + kWave;
        const uint32_t nxt = jn < n ? tok[base + jn] : kTokNone;
        const uint32_t wnxt = W && jn < n ? wt[base + jn] : 1u;
        const ResStep nb = res_neighbours(prv, cur, nxt, lane);
        const bool c = is_cand(cur, nb.nx, a, b);
        const unsigned long long M = __ballot(c);
        const bool odd = run_below(M, lt, lane, carry) & 1u;
        const bool match = c && !odd;
        uint32_t v = kTokNone;
        if (j < n && !odd) v = match ? (X | (nb.nx & kTokEnd)) : cur;
        const WaveKeep keep = wave_keep(v != kTokNone, lt);
        dirty = dirty || M != 0ull;
        if (dirty && v != kTokNone) {
            tok[base + wpos + keep.rank] = v;
            if (W) wt[base + wpos + keep.rank] = wcur;
        }
        n_match += wave_count(match);
        if (match) {
            const int32_t w = W ? (int32_t)wcur : 1;
            if (W) w_match += (uint32_t)w;
            // the left neighbour as it stands AFTER the walk has passed it (k_wide_match has the reasoning)
            if (!(nb.p & kTokEnd)) {
                const bool swallowed = a == b ? nb.p == a : (nb.p == b && nb.pp == a);
                const uint32_t x = swallowed ? X : nb.p;
                add(((unsigned long long)x << 32) | a, -w);
                add(((unsigned long long)x << 32) | X, w);
            }
            // the right neighbour as it still is
            if (!(nb.nx & kTokEnd)) {
                const uint32_t y = nb.y & kTokIdMask;
                add(((unsigned long long)b << 32) | y, -w);
                add(((unsigned long long)X << 32) | y, w);
            }
        }
        wpos += keep.count;
        carry = run_carry(M, carry);
        prv = cur; cur = nxt; wcur = wnxt;
    }
    if (W) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) w_match += __shfl_xor(w_match, d, kWave);
    }
    return {wpos, n_match, w_match};
}

}  // namespace mbpe

#endif
