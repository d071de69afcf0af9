// The 32-bit training loop in TWO launches per merge, on regions that waves own (the context option "regions",
// mbpe.h; DESIGN.md "Merges on wave-owned regions").  wide.h's loop launches seven kernels per merge (ten with the
// `first` tie-break), and over a stream of some hundred kilobytes those launches are what it costs; the one workgroup
// of wide_resident.h is outnumbered beyond some 45,000 tokens.  This keeps that kernel's two ideas and spreads them
// over the chip, without a cooperative launch and without a grid-wide barrier:
//
//   regions   pairs never cross a chunk, so the stream is cut at chunk ends into regions of whole chunks of about
//             "region_tokens" tokens (k_wide_regions_cut: region_boundary of wide_resident.h, one thread per boundary).
//             For a GROUP of merges a wave owns a region and rewrites it in place with the walk of wide_walk.h; no
//             candidate scan, parity scan, sum scan or scatter over the stream.  off[] and len[] live in device memory;
//             after the group's last merge one scan of len[] and one copy close the regions up into the other buffer,
//             and the state is again what wide.hip, the resident kernel and the host's readers expect.
//   tickets   what is left of a merge is a reduction with one consumer, and the workgroup that arrives last does it:
//             every workgroup publishes its part, fences, and draws a ticket with atomicAdd; the one that draws the
//             last ticket fences and reads the parts.  Nobody spins, nobody waits for another workgroup.
//               k_wide_regions_argmax     k_wide_argmax_partial, its last workgroup k_wide_argmax_final
//               k_wide_regions_walk       the merge; its last workgroup takes the matches off ctl->n and advances ctl->k
//               k_wide_regions_first_pos  (`first`, after k_wide_first_gather) the earliest tied position, as the global
//                                         token index off[r] + j; its last workgroup does k_wide_first_pick's work
//
// Two launches per merge in lexical mode, four with `first`; three more per group (cut, scan, copy).  No stopping rules
// in these kernels (wide_run.cpp keeps the launches of wide.h for such trainings).  Every loop is bounded: the walk by
// the region's length, the cutter by kResRegionCap tokens per boundary, probes by the table's capacity.
#ifndef MBPE_WIDE_REGIONS_H
#define MBPE_WIDE_REGIONS_H

#include "wide_resident.h"

namespace mbpe {

constexpr uint32_t kRegMaxRegions = 1u << 16;      // one scan workgroup closes them: 1,024 threads x 64 lengths
// The longest stream a group takes on: kRegMaxRegions regions of 1,024 tokens.  This bound is arithmetic (the scan's
// reach times a region size well inside kResRegionCap), not a measurement.
constexpr uint64_t kRegMaxTokens = (uint64_t)kRegMaxRegions * 1024;
constexpr uint32_t kRegTokensMin = 64, kRegTokensMax = kResRegionCap;
// the default of "region_tokens": the best of 128 .. 2,048 on the 110,918 tokens of 1.14 GB of shakespeare, or within
// 1.3 us of it, in both tie-breaks at vocab 512 and 10,000 (profiles/r35_train_regions.md)
constexpr uint32_t kRegTokensDefault = 256;

// the regions of a group over n tokens: `per` tokens each (before the boundaries move to chunk ends), `count` of them
struct RegionPlan { uint32_t per, count; };
MBPE_HD RegionPlan region_plan(uint64_t n, uint32_t region_tokens) {
    const uint64_t least = (n + kRegMaxRegions - 1) / kRegMaxRegions;
    const uint64_t per = least > region_tokens ? least : region_tokens;
    const uint64_t count = (n + per - 1) / per;
    return {(uint32_t)per, (uint32_t)(count ? count : 1)};
}

// What the cutter's thread r computes, for the host check too: region r = tokens off .. off + len, and whether it
// fits `cap` (a boundary the scan gave up on lies beyond any cap).
struct RegionCut { uint32_t off, len; bool ok; };
MBPE_HD RegionCut region_cut(const uint32_t *tok, uint32_t n, RegionPlan p, uint32_t r, uint32_t cap) {
    const uint32_t lo = region_boundary(tok, n, p.per, p.count, r, cap);
    const uint32_t hi = region_boundary(tok, n, p.per, p.count, r + 1, cap);
    const bool ok = lo != kRegionNoBoundary && hi != kRegionNoBoundary && hi - lo <= cap;
    return {lo, ok ? hi - lo : 0u, ok};
}

// header of the regions' device state; off[count + 1], len[count] and to[count] are arrays of their own
struct WideRegions {
    uint32_t bad;                      // a region beyond kResRegionCap, or a stream that is not the host's plan: no launch
                                       //   of the group does anything, the host goes back to the launches of wide.h
    uint32_t t_argmax, t_walk, t_pos;  // the tickets; 0 between two launches
};
struct RegionBufs {
    WideRegions *hdr;
    uint32_t *off, *len;               // region r = tokens off[r] .. off[r] + len[r]
    unsigned long long *to;            // where region r goes when the group closes
};

#ifdef __HIPCC__
// the group's regions over the stream src (ctl->n tokens, which must be what `plan` was made for)
void launch_wide_regions_cut(hipStream_t s, const uint32_t *src, const WideCtl *ctl, RegionPlan plan, RegionBufs rb);
// One merge of the group: argmax (scratch: that of launch_wide_argmax), with `fs` the `first` tie-break, the walk in
// place over tok / wt (NULL: unweighted).  Advances ctl->k and takes the matches off ctl->n; nothing when ctl->k >=
// ctl->k_limit, the table is empty or rb.hdr->bad.
void launch_wide_regions_merge(hipStream_t s, uint32_t *tok, uint32_t *wt, RegionPlan plan, RegionBufs rb, WideTable t,
                               WideCtl *ctl, WideBest *best, unsigned long long *scratch, WideFirst *fs,
                               uint32_t new_id_base);
// the regions closed up into dst / wdst; ctl->n = their total length
void launch_wide_regions_close(hipStream_t s, const uint32_t *tok, uint32_t *dst, const uint32_t *wt, uint32_t *wdst,
                               RegionPlan plan, RegionBufs rb, WideCtl *ctl);
#endif

}  // namespace mbpe

#endif
