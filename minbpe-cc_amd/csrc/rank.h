// The segmented minimum of the rank-ordered encode (encode.hip, option "rank_order"), beside the run parity of span.h.
//
// A rank pass replaces, in every chunk at once, the candidates whose id is the smallest candidate id of their chunk.
// A SEGMENT is the positions of one chunk: it ends at (and includes) a token with the end flag.  The minimum of cand
// over every segment is taken on three levels: inside a group of 64 lanes (a segmented scan by shuffles, steered by the
// ballot E of the end flags), across the 16 groups of a span (a forward and a backward sweep over values every lane of
// the wave shares), and across the spans (one single-workgroup scan in both directions).  kTokNone, all ones, is "no
// candidate" and the identity of the unsigned minimum.
//
// What a stretch of positions is to its neighbours: does it hold an end flag, the minimum over its positions up to and
// including its first end flag (HEAD: the part of the chunk that enters from the left), and the minimum over the
// positions after its last end flag (TAIL: the part of the chunk that goes on to the right).  Without an end flag both
// are the minimum over the whole stretch.  Everything here is arithmetic on integers and 64-bit masks that a host
// compiler builds too (tests/test_rank_cpu.py runs it).
#ifndef MBPE_RANK_H
#define MBPE_RANK_H

#include "span.h"

namespace mbpe {

MBPE_HD uint32_t rank_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

struct RankSum { uint32_t has_end, head, tail; };
MBPE_HD RankSum rank_empty() { return {0u, kTokNone, kTokNone}; }

// L then R; associative, which is what lets the scan cut the spans into slices
MBPE_HD RankSum rank_fold(RankSum L, RankSum R) {
    return {L.has_end | R.has_end, L.has_end ? L.head : rank_min(L.head, R.head),
            R.has_end ? R.tail : rank_min(L.tail, R.tail)};
}

// the fold of sum[lo .. hi): the first sweep of the scan
MBPE_HD RankSum rank_fold_slice(const RankSum *sum, uint64_t lo, uint64_t hi) {
    RankSum acc = rank_empty();
    for (uint64_t s = lo; s < hi; ++s) acc = rank_fold(acc, sum[s]);
    return acc;
}

// `run` = minimum over the open part of the chunk that reaches a stretch from one side; the same after the stretch:
// v is the stretch's tail when walking to the right, its head when walking to the left
MBPE_HD uint32_t rank_carry(uint32_t run, uint32_t has_end, uint32_t v) { return has_end ? v : rank_min(run, v); }

// ---- inside a group: E = ballot of the end flags, lt = lanes_below(lane) ------------------------------------------
// the lanes up to and including the first end flag / the lanes after the last one (all lanes when there is none)
MBPE_HD unsigned long long rank_head_lanes(unsigned long long E) { return E ? E ^ (E - 1ull) : ~0ull; }
MBPE_HD unsigned long long rank_tail_lanes(unsigned long long E) {
    if (!E) return ~0ull;
    const uint32_t top = 63u - (uint32_t)__builtin_clzll(E);
    return top == 63u ? 0ull : ~0ull << (top + 1u);
}

// the first and the last lane of the part of `lane`'s segment that lies in this group
MBPE_HD uint32_t rank_seg_lo(unsigned long long E, unsigned long long lt) {
    const unsigned long long below = E & lt;
    return below ? 64u - (uint32_t)__builtin_clzll(below) : 0u;
}
MBPE_HD uint32_t rank_seg_hi(unsigned long long E, unsigned long long lt) {
    const unsigned long long at = E & ~lt;
    return at ? (uint32_t)__builtin_ctzll(at) : 63u;
}
// does the segment of `lane` go on beyond the group to the left / to the right
MBPE_HD bool rank_open_left(unsigned long long E, unsigned long long lt) { return (E & lt) == 0ull; }
MBPE_HD bool rank_open_right(unsigned long long E, unsigned long long lt) { return (E & ~lt) == 0ull; }

// one step of the segmented inclusive scan: `up` is the value of lane - d (anything where there is no such lane).
// After the steps d = 1, 2, 4 .. 32 a lane holds the minimum over [lo, lane]; lane hi then holds the segment's.
MBPE_HD uint32_t rank_scan_step(uint32_t v, uint32_t up, uint32_t lane, uint32_t d, uint32_t lo) {
    return lane >= lo + d ? rank_min(v, up) : v;
}

// ---- a span's summary, lane by lane: h and t are per-lane partial minima that a wave minimum finishes ------------
// seen = an earlier group of the span held an end flag
MBPE_HD uint32_t rank_head_part(uint32_t h, bool seen, unsigned long long E, uint32_t lane, uint32_t c) {
    return !seen && ((rank_head_lanes(E) >> lane) & 1ull) ? rank_min(h, c) : h;
}
MBPE_HD uint32_t rank_tail_part(uint32_t t, unsigned long long E, uint32_t lane, uint32_t c) {
    const uint32_t mine = (rank_tail_lanes(E) >> lane) & 1ull ? c : kTokNone;
    return E ? mine : rank_min(t, mine);
}

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    for (int d = kWave / 2; d > 0; d >>= 1) v = rank_min(v, (uint32_t)__shfl_xor((int)v, d, kWave));
    return v;
}

// the minimum of c over the part of this lane's segment that lies in the group
__device__ __forceinline__ uint32_t group_seg_min(uint32_t c, unsigned long long E, unsigned long long lt,
                                                  uint32_t lane) {
    const uint32_t lo = rank_seg_lo(E, lt), hi = rank_seg_hi(E, lt);
    uint32_t v = c;
    for (uint32_t d = 1; d < (uint32_t)kWave; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)v, d, kWave);
        v = rank_scan_step(v, up, lane, d, lo);
    }
    return (uint32_t)__shfl((int)v, (int)hi, kWave);
}

// ---- the scan over the spans: one workgroup of kScanThreads, slices as in span_scan_parity ------------------------
// in_left[s] = minimum over the part of the chunk that reaches span s from the left, in_right[s] = from the right.
// sh_sum, sh_l, sh_r: kScanThreads elements of LDS each.  Every thread of the workgroup has to call it (two barriers).
__device__ __forceinline__ void span_scan_min(const RankSum *__restrict__ sum, uint64_t n_spans,
                                              uint32_t *__restrict__ in_left, uint32_t *__restrict__ in_right,
                                              RankSum *sh_sum, uint32_t *sh_l, uint32_t *sh_r) {
    const uint64_t per = (n_spans + kScanThreads - 1) / kScanThreads;
    const uint64_t lo = per * threadIdx.x < n_spans ? per * threadIdx.x : n_spans;
    const uint64_t hi = lo + per < n_spans ? lo + per : n_spans;
    sh_sum[threadIdx.x] = rank_fold_slice(sum, lo, hi);
    __syncthreads();
    if (threadIdx.x == 0) {                    // to the right ...
        uint32_t run = kTokNone;               // nothing before the text
        for (int t = 0; t < kScanThreads; ++t) {
            sh_l[t] = run;
            run = rank_carry(run, sh_sum[t].has_end, sh_sum[t].tail);
        }
    }
    if (threadIdx.x == kWave) {                // ... and, in another wave, to the left
        uint32_t run = kTokNone;
        for (int t = kScanThreads - 1; t >= 0; --t) {
            sh_r[t] = run;
            run = rank_carry(run, sh_sum[t].has_end, sh_sum[t].head);
        }
    }
    __syncthreads();
    uint32_t run = sh_l[threadIdx.x];
    for (uint64_t s = lo; s < hi; ++s) {
        in_left[s] = run;
        run = rank_carry(run, sum[s].has_end, sum[s].tail);
    }
    run = sh_r[threadIdx.x];
    for (uint64_t s = hi; s > lo; --s) {
        in_right[s - 1] = run;
        run = rank_carry(run, sum[s - 1].has_end, sum[s - 1].head);
    }
}
#endif  // __HIPCC__

}  // namespace mbpe

#endif
