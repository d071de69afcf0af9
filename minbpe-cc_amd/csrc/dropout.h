// BPE-dropout of the rank-ordered encode (encode.hip with the option "rank_order", Tokenizer::encode_rank_ordered).
//
// A rank pass replaces, in every chunk, the candidates whose id is the smallest candidate id of their chunk.  With
// dropout a candidate INSTANCE may be dropped first: it is then no candidate in any pass.  An instance is (pos, id):
// pos = the offset of the first byte of the pair's left token in the buffer the encoder read (64 bits, over the whole
// call, not over a piece or a chunk), id = the token the pair merges to.  The decision is a pure function of
// (seed, pos, id) -- one round of splitmix64's finisher over a linear mix of the three -- so it does not depend on how
// a text is cut into pieces or spans, on the pass in which the instance turns up, or on what other chunks do, and an
// instance that is dropped stays dropped.  Everything here is integer arithmetic that a host compiler builds too
// (tests/dropout_check.cpp runs it).
#ifndef MBPE_DROPOUT_H
#define MBPE_DROPOUT_H

#include "span.h"

namespace mbpe {

constexpr unsigned long long kDropoutOne = 1ull << 32;      // the threshold of p = 1: every instance is dropped

MBPE_HD uint32_t drop_hash(unsigned long long seed, unsigned long long pos, uint32_t id) {
    unsigned long long x = seed + pos * 0x9E3779B97F4A7C15ull + (unsigned long long)id * 0xD1B54A32D192ED03ull;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (uint32_t)(x >> 32);
}

// threshold in [0, 2^32]: 0 drops nothing, 2^32 everything
MBPE_HD bool dropout_dropped(unsigned long long seed, unsigned long long pos, uint32_t id, unsigned long long threshold) {
    return (unsigned long long)drop_hash(seed, pos, id) < threshold;
}

// floor(p * 2^32) -> *threshold; exact for p = 0 and p = 1 (p * 2^32 is a scaling by a power of two: no rounding).
// false for NaN and for p outside [0, 1]
inline bool dropout_threshold(double p, unsigned long long *threshold) {
    if (!(p >= 0.0 && p <= 1.0)) return false;
    *threshold = (unsigned long long)(p * 4294967296.0);
    return true;
}

}  // namespace mbpe

#endif
