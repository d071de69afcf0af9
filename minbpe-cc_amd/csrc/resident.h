// Tiles of whole chunks: the geometry of the encoder's option "resident" (encode.hip, k_enc_resident).
//
// Chunks never interact, so a stretch of the piece that begins after one chunk end and stops at another can run every
// merge round to its fixed point without a word from its neighbours.  A TILE is such a stretch, cut near every multiple
// of kResB bytes: boundary t, for 0 < t < n_tiles, is the position after the first end bit of the piece's byte mask
// among the kResL bytes [t kResB - 1, t kResB - 1 + kResL) (CLOSED), or t kResB when there is none (OPEN: a chunk longer
// than the search bound lies across it).  Boundary 0 = 0 and boundary n_tiles = the piece's end are closed.  Boundary t
// lies in [t kResB, t kResB + kResL - 1], so the boundaries ascend, the tiles [lo_t, lo_t+1) partition the piece (one may
// be empty), and a tile holds at most kResB + kResL - 1 = 1,023 bytes: a wave's span of tokens, less one.  A tile with
// two closed boundaries holds whole chunks (RESIDENT); any other is left as it is (RAW).
//
// The boundaries come from the byte mask, not from the token flags: a chunk that is one token by rule carries its flag
// on its first token, and its bytes stay together all the same.  Everything here is arithmetic on the mask's words
// that a host compiler builds too (tests/test_resident_cpu.py runs it against a loop over the bits).
#ifndef MBPE_RESIDENT_H
#define MBPE_RESIDENT_H

#include "span.h"

namespace mbpe {

constexpr uint32_t kResB = 768;                 // a tile's window of chunk starts, in bytes
constexpr uint32_t kResL = 256;                 // the search bound: bytes looked at for a chunk end
constexpr uint32_t kResMax = kResB + kResL - 1; // the most bytes of a tile
static_assert(kResMax < (uint32_t)kSpan, "a tile fits one wave's span with a position to spare");

MBPE_HD uint64_t res_tile_count(uint64_t n_bytes) { return (n_bytes + kResB - 1) / kResB; }
inline uint32_t res_grid(uint64_t n_bytes) { return (uint32_t)((res_tile_count(n_bytes) + kSpanWaves - 1) / kSpanWaves); }

// the first end bit of the mask at or after bit `from` and below bit `to` (to <= the mask's bytes; `to` when there is
// none).  words = the mask as 32-bit words, bit i of the piece = bit i & 31 of word i >> 5; reads words [from / 32,
// (to - 1) / 32] only
MBPE_HD uint64_t res_first_end(const uint32_t *words, uint64_t from, uint64_t to) {
    if (from >= to) return to;
    const uint64_t w1 = (to - 1) >> 5;
    for (uint64_t w = from >> 5; w <= w1; ++w) {
        uint32_t v = words[w];
        if (w == from >> 5) v &= ~0u << (from & 31u);
        if (v) {
            const uint64_t at = (w << 5) + (uint32_t)__builtin_ctz(v);
            return at < to ? at : to;
        }
    }
    return to;
}

struct ResBound { uint64_t lo; bool closed; };

// boundary t of a piece of n_bytes > 0 bytes, 0 <= t <= res_tile_count(n_bytes)
MBPE_HD ResBound res_bound(const uint32_t *words, uint64_t n_bytes, uint64_t t) {
    if (t == 0) return {0, true};
    if (t >= res_tile_count(n_bytes)) return {n_bytes, true};
    const uint64_t from = t * kResB - 1;                               // (< n_bytes: tile t exists)
    const uint64_t to = from + kResL < n_bytes ? from + kResL : n_bytes;
    const uint64_t at = res_first_end(words, from, to);
    if (at < to) return {at + 1, true};
    return {t * kResB, false};
}

struct ResTile { uint64_t lo; uint32_t len; bool resident; };

// tile t of the piece: [lo, lo + len), len <= kResMax
MBPE_HD ResTile res_tile(const uint32_t *words, uint64_t n_bytes, uint64_t t) {
    const ResBound a = res_bound(words, n_bytes, t), b = res_bound(words, n_bytes, t + 1);
    return {a.lo, (uint32_t)(b.lo - a.lo), a.closed && b.closed};
}

}  // namespace mbpe

#endif
