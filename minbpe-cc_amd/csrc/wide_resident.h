// The 32-bit training loop on a SHORT stream in one workgroup (the context option "resident", mbpe.h; DESIGN.md "The
// resident training loop").  wide.h's loop launches seven to ten kernels per merge; over a stream of some hundred
// kilobytes those launches are all it costs.  k_wide_resident runs a whole group of merges ctl->k .. ctl->k_limit in
// one launch of ONE workgroup of 1,024 threads: argmax, `first` tie-break, merge and table update, with a
// __syncthreads() wherever the loop of wide_run.cpp has a kernel boundary.  Same WideTable, WideCtl, WideBest, token
// layout and weights; after any launch the kernels of wide.hip carry on from what it leaves, and the other way round.
//
//   regions   pairs never cross a chunk, so the stream is cut at chunk ends into kResRegions = 16 regions of whole
//             chunks, one per wave, balanced by tokens (resident_cut below: plain arithmetic, the set-up kernel and
//             the host check run the same function).  A wave owns its region for the launch, walks it in 64-lane
//             steps (neighbours from the registers of the previous and the next step), carries the run parity of
//             `a a a` from step to step, and rewrites it IN PLACE: the write index never passes the read index, a
//             merged token keeps its left half's weight, a region without a candidate writes nothing.  The regions'
//             lengths live in LDS; after the last merge they are closed up into the other token buffer.
//   argmax    LDS holds, per slice of the table's slots, an upper bound of its counts, an "exact" bit and (when
//             exact) the best key.  Every add of the kernel raises its slice's bound on an increment and clears the
//             exact bit where the slice's best may have changed; a merge's argmax rescans only the slices that are
//             not exact and whose bound reaches the best exact count, one wave per slice.
//   first     the tied pairs' hashed keys go into the 64-Kibit bitmap in LDS; the waves walk their regions in stream
//             order and stop once a region before their own has reported a position.
//
// No stopping rules in the kernel (wide_run.cpp falls back to the launches of wide.h), no grid-wide barrier, and
// every loop bounded: probes by the table's capacity, merges by k_limit, the argmax's rescan by the slices.
#ifndef MBPE_WIDE_RESIDENT_H
#define MBPE_WIDE_RESIDENT_H

#include "span.h"
#ifdef __HIPCC__
#include "wide.h"
#endif

#include <stdint.h>

namespace mbpe {

constexpr uint32_t kResThreads = 1024;
constexpr uint32_t kResRegions = kResThreads / kWave;            // one region per wave
constexpr uint32_t kResRegionCap = 1u << 16;                     // tokens a region takes: a wave walks them serially
constexpr uint32_t kResMaxTokens = kResRegions * kResRegionCap;  // the largest "resident_max_tokens"
// the default of "resident_max_tokens": the longest stream at which the workgroup beat the launches of wide.h by more
// than their run-to-run spread (profiles/r32_train_resident.md); 0 until that has been measured
constexpr uint32_t kResidentMaxDefault = 0;
constexpr uint32_t kResSlices = 2048;                           // slices of the pair table's slots, at most
constexpr uint32_t kResSliceMin = 64;                            // slots of a slice, at least (one wave step)
// The largest pair table a launch takes on.  Every launch begins with a scan of the whole table by the one workgroup,
// and the table is never erased: a short stream can come with a table of tens of millions of slots.  At 2^21 slots a
// slice is 1,024 slots (16 steps of the wave that rescans it) and the scan reads 24 MiB; beyond, the launches of wide.h.
constexpr uint64_t kResMaxSlots = (uint64_t)kResSlices * 1024;

// what a launch leaves for the host beside WideCtl
struct WideResident {
    uint32_t off[kResRegions + 1];     // the regions of the launch: region r = tokens off[r] .. off[r + 1]
    uint32_t ok;                       // 0: a region is longer than kResRegionCap, the kernel did nothing
    unsigned long long n_rescanned;    // slices the argmax rescanned, summed over the launches
    unsigned long long t_argmax, t_first, t_walk;      // wall-clock ticks (100 MHz) of the three phases, likewise
};

// ---- the region cutter: plain arithmetic, host and device --------------------------------------------------------
// Boundary r of n_regions + 1 over the n flagged tokens of tok, for regions of `per` tokens (per * n_regions >= n):
// the target r * per, moved forward to just behind the next chunk end (bit 31) at or after the token before it; 0
// for r = 0, n for the last and where no chunk end follows.  Ascending in r, because the targets are.  The one
// statement of the rule: the cutters of wide_resident.hip and wide_regions.hip and the host checks all call it.
// reach: how far forward the scan looks (n: to the end).  A scan that gives up returns kRegionNoBoundary; the chunk
// it stood in is longer than `reach` tokens, and so is the region that holds it.
constexpr uint32_t kRegionNoBoundary = 0xFFFFFFFFu;
MBPE_HD uint32_t region_boundary(const uint32_t *tok, uint32_t n, uint32_t per, uint32_t n_regions, uint32_t r,
                                 uint32_t reach) {
    if (r == 0) return 0;
    if (r >= n_regions) return n;
    uint64_t i = (uint64_t)per * r;
    if (i == 0 || i >= n) return n;
    const uint64_t stop = i + reach < n ? i + reach : n;
    for (--i; i < stop; ++i)
        if (tok[i] & kTokEnd) return (uint32_t)i + 1;
    return stop < n ? kRegionNoBoundary : n;
}

// ... of the kResRegions + 1 of a resident launch: balanced by tokens, per = ceil(n / kResRegions)
MBPE_HD uint32_t resident_boundary(const uint32_t *tok, uint32_t n, uint32_t r) {
    return region_boundary(tok, n, (n + kResRegions - 1) / kResRegions, kResRegions, r, n);
}

// All of them; false when a region would hold more than `cap` tokens (a chunk longer than a region takes).
inline bool resident_cut(const uint32_t *tok, uint32_t n, uint32_t cap, uint32_t off[kResRegions + 1]) {
    bool ok = true;
    for (uint32_t r = 0; r <= kResRegions; ++r) off[r] = resident_boundary(tok, n, r);
    for (uint32_t r = 0; r < kResRegions; ++r) ok = ok && off[r + 1] - off[r] <= cap;
    return ok;
}

#ifdef __HIPCC__
// The merges ctl->k .. ctl->k_limit of the loop on the stream src (ctl->n tokens, at most kResMaxTokens; wsrc: NULL or
// its weights), either tie-break by ctl->first.  Two launches: the cutter, then the workgroup.  The closed-up stream
// goes to dst / wdst when at least one merge ran (the caller flips its buffers then); res->ok = 0: nothing ran.
void launch_wide_resident(hipStream_t s, uint32_t *src, uint32_t *dst, uint32_t *wsrc, uint32_t *wdst, WideTable t,
                          WideCtl *ctl, WideBest *best, uint32_t new_id_base, bool first, WideResident *res);
#endif

}  // namespace mbpe

#endif
