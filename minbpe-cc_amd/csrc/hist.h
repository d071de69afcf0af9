// Token frequency tables (hist.hip): how often every id occurs in a stream of tokens, in 64 bits and exact.
//
//   hist_tokens   n elements of 32 bits (bit 31 cleared on read: flagged device tokens, plain ids, a unique_of map) or
//                 of 16 bits -> counts[id] += 1 for id < n_ids, *other += 1 for the rest.  An id at or beyond n_ids
//                 never forms an address.
//   hist_runs     a table of token runs (table, ends: as expand.h describes them) with a 64-bit weight per run ->
//                 counts[table[p]] += w[run(p)].  Element-centric: a lane takes table elements and finds their run by
//                 search in ends, so a run of a million tokens is a million elements like any others.
//   hist_fold     kept[i] += repeat * call[i], in 64 bits.
//
// The partition of hist_tokens.  The elements are read in PIECES of 16 aligned bytes (kHistPiece), 4 or 8 elements a
// lane: POSITION p = skip + element index, where skip is the number of elements between the 16-byte boundary at or
// below the first element and that element, so piece q holds the positions [q * per, (q + 1) * per) and the positions
// outside [skip, skip + n) are read (the same aligned 16 bytes hold a valid element, so the load cannot leave the
// buffer's pages) and ignored.  A TILE is kHistTile = 4,096 positions, four spans of 1,024, one workgroup of 256 lanes
// at a time; workgroup g of G takes the tiles g, g + G, g + 2G, ...  Ids below kHistLocalIds are counted in a
// workgroup-private 32-bit LDS table that is flushed with 64-bit global atomics, the rest with 64-bit global atomics
// directly.  A private counter cannot wrap: a workgroup flushes after at most kHistFlushTiles tiles, and
// kHistFlushTiles * kHistTile < 2^32 (the static_assert below).
//
// This header is shared by the device code and by host programs: the index arithmetic, and hist_host / hist_runs_host /
// hist_fold_host, plain restatements through that arithmetic that tests/hist_check.cpp runs against a std::map count.
#ifndef MBPE_HIST_H
#define MBPE_HIST_H

#include "span.h"

#include <stdint.h>

#ifndef __HIP_DEVICE_COMPILE__
#include <algorithm>
#include <vector>
#endif

namespace mbpe {

// ids counted in LDS, a power of two: 2^13 = 32 KiB of 32-bit counters.  (MBPE_HIST_LOCAL_BITS: tools/token_counts_time.py
// builds hist.hip with 13, 14 and 15 for its sweep; the library is built without it.)
#ifndef MBPE_HIST_LOCAL_BITS
#define MBPE_HIST_LOCAL_BITS 13
#endif
constexpr uint32_t kHistLocalIds = 1u << MBPE_HIST_LOCAL_BITS;
constexpr int kHistThreads = 256;
constexpr uint32_t kHistPiece = 16;             // bytes of an aligned load
constexpr uint32_t kHistTile = 4096;            // positions a workgroup takes at a time: four spans of 1,024
constexpr uint64_t kHistFlushTiles = 1ull << 19;   // tiles between two flushes of the LDS table
constexpr uint32_t kHistMinTiles = 8;           // a workgroup is worth its flush from this many tiles on
constexpr uint32_t kHistMaxGroups = 1024;

static_assert((kHistLocalIds & (kHistLocalIds - 1)) == 0, "kHistLocalIds is a power of two");
static_assert(kHistFlushTiles * kHistTile < (1ull << 32),
              "what one workgroup adds to a 32-bit LDS counter between two flushes stays below 2^32");
static_assert(kHistTile % (kHistThreads * (kHistPiece / 2)) == 0, "a tile is whole rounds of the workgroup's pieces");

// the positions before the first element: the elements between the 16-byte boundary below addr and addr
MBPE_HD uint64_t hist_skip(uint64_t addr, uint32_t elem_bytes) { return (addr & (kHistPiece - 1)) / elem_bytes; }
MBPE_HD uint64_t hist_tile_count(uint64_t skip, uint64_t n) { return n ? (skip + n + kHistTile - 1) / kHistTile : 0; }
MBPE_HD uint32_t hist_group_count(uint64_t n_tiles) {
    const uint64_t g = (n_tiles + kHistMinTiles - 1) / kHistMinTiles;
    return (uint32_t)(g < 1 ? 1 : g > kHistMaxGroups ? kHistMaxGroups : g);
}
// the id of an element as it was read: 32-bit elements lose bit 31, 16-bit elements are ids as they are
MBPE_HD uint32_t hist_id(uint32_t raw, uint32_t elem_bytes) { return elem_bytes == 4 ? raw & kTokIdMask : raw; }

// run(p) of hist_runs: the first j with ends[j] > p, n_entries when there is none (ends ascend; empty runs are skipped)
MBPE_HD uint64_t hist_run_of(const unsigned long long *ends, uint64_t n_entries, unsigned long long p) {
    uint64_t lo = 0, hi = n_entries;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (ends[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

#ifndef __HIP_DEVICE_COMPILE__
// hist_tokens on the host, workgroup by workgroup and tile by tile as the device walks it; base_addr: the byte address
// the elements are taken to start at (only its low 4 bits matter).  counts has n_ids entries and is added to.
// *max_local: the largest value a private counter reached (the no-wrap bound, checked by the test).
template <typename T>
inline void hist_host(const T *elems, uint64_t n, uint64_t base_addr, unsigned long long *counts, uint64_t n_ids,
                      unsigned long long *other, uint64_t *max_local) {
    const uint32_t per = kHistPiece / sizeof(T);
    const uint64_t skip = hist_skip(base_addr, sizeof(T)), n_tiles = hist_tile_count(skip, n);
    const uint32_t G = hist_group_count(n_tiles);
    std::vector<uint32_t> local(kHistLocalIds);
    for (uint32_t g = 0; g < G; ++g) {
        for (uint64_t k0 = 0; g + k0 * G < n_tiles; k0 += kHistFlushTiles) {
            std::fill(local.begin(), local.end(), 0u);
            for (uint64_t k = k0; k < k0 + kHistFlushTiles && g + k * G < n_tiles; ++k) {
                const uint64_t tile = g + k * G;
                for (uint64_t q = tile * (kHistTile / per); q < (tile + 1) * (kHistTile / per); ++q)
                    for (uint32_t e = 0; e < per; ++e) {
                        const uint64_t pos = q * per + e;
                        if (pos < skip || pos >= skip + n) continue;
                        const uint32_t id = hist_id(elems[pos - skip], sizeof(T));
                        if (id >= n_ids) ++*other;
                        else if (id < kHistLocalIds) ++local[id];
                        else ++counts[id];
                    }
            }
            for (uint32_t i = 0; i < kHistLocalIds && i < n_ids; ++i) {
                if (max_local && local[i] > *max_local) *max_local = local[i];
                counts[i] += local[i];
            }
        }
    }
}

// hist_runs on the host, element by element; *total gets the weighted number of elements
template <typename T>
inline void hist_runs_host(const T *table, uint64_t n_table, const unsigned long long *ends, uint64_t n_entries,
                           const unsigned long long *w, unsigned long long *counts, uint64_t n_ids,
                           unsigned long long *other, unsigned long long *total) {
    for (uint64_t p = 0; p < n_table; ++p) {
        const uint64_t j = hist_run_of(ends, n_entries, p);
        if (j >= n_entries) continue;               // behind the last run: nobody copies it
        const uint32_t id = hist_id(table[p], sizeof(T));
        if (id < n_ids) counts[id] += w[j]; else *other += w[j];
        *total += w[j];
    }
}

inline void hist_fold_host(unsigned long long *kept, const unsigned long long *call, uint64_t n, unsigned long long repeat) {
    for (uint64_t i = 0; i < n; ++i) kept[i] += repeat * call[i];
}
#endif  // !__HIP_DEVICE_COMPILE__

#ifdef __HIPCC__
// ---- the launchers (hist.hip); everything named is device memory, nothing is waited for ------------------------------
// elems: n elements of elem_bits (16 or 32) bits, aligned to its elements; counts[0 .. n_ids) and *other are added to
void hist_tokens_launch(hipStream_t stream, const void *elems, uint64_t n, uint32_t elem_bits, unsigned long long *counts,
                        uint64_t n_ids, unsigned long long *other);

// table: n_table elements of elem_bits bits; run j is [ends[j - 1], ends[j]) and weighs w[j]; *total += the weights of
// all elements
void hist_runs_launch(hipStream_t stream, const void *table, uint64_t n_table, uint32_t elem_bits,
                      const unsigned long long *ends, uint64_t n_entries, const unsigned long long *w,
                      unsigned long long *counts, uint64_t n_ids, unsigned long long *other, unsigned long long *total);

// kept[i] += repeat * call[i] for i < n
void hist_fold_launch(hipStream_t stream, unsigned long long *kept, const unsigned long long *call, uint64_t n,
                      unsigned long long repeat);
#endif  // __HIPCC__

}  // namespace mbpe

#endif
