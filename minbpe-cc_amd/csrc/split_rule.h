// The gpt2 / gpt4 split of ASCII text as a rule on bytes (split.hip), written once for the device and
// for the host compiler (tests/split_check.cpp walks texts with it, one loop iteration per device thread).
//
// Byte classes: L = A-Z a-z, N = 0-9, S = 9 10 11 12 13 32 (what \s matches below 0x80 under PCRE2_UCP), O = every
// other byte below 0x80, X = 0x80 and above (never walked here).  Position p is a SYNC POINT when 0 < p < n, t[p - 1] is
// L or N and t[p] is S: no alternative of either pattern matches a letter or digit followed by whitespace and both
// patterns cover every character, so every sync point is a chunk boundary whatever surrounds it.  The sync points
// with 0 and n cut the text into spans [a, b).  A span without an X byte and of at most max_span bytes is CLEAN and is
// walked with split_step; every other span is a HOST span and goes to PCRE2.  Neither pattern looks behind, so the
// walk from a is the true walk; no match that starts before b crosses b, and nothing reads past t[b].
//
// Several texts in one buffer (mbpe_splitter_split_docs): a CUT is a position where one text ends and the next begins
// -- a document boundary, the start or the end of a range that is not split (a special token's name, a NUL-led part).
// The boundary bitmap the walk searches is sync | cut.  A span that ends at a cut b is walked with b in place of n: then
// split_at answers "beyond the text" at b and the whitespace rule sees r == n, which is what PCRE2 sees at the end of
// a subject.  A position that is both a sync point and a cut is a cut; before a sync point the last match ends on a
// letter or digit either way.  Spans that start inside a range (its RAW bitmap bit is set) are nobody's: the host
// adds the one end bit of every range.
//
// Bitmaps: one bit per text byte, bit i & 63 of 64-bit word i >> 6 (little endian: the byte layout of the trainer's
// end mask).  Thread T of the walk owns the span starts in word T of the sync bitmap.
#ifndef MBPE_SPLIT_RULE_H
#define MBPE_SPLIT_RULE_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MBPE_SPLIT_HD __host__ __device__ inline
#else
#define MBPE_SPLIT_HD inline
#endif

namespace mbpe {

constexpr int kSplitBlock = 64;            // text bytes whose span starts one walk thread takes (MBPE_SPLIT_BLOCK)
constexpr int kSplitVec = 16;              // text bytes one lane of the sync pass loads
enum SplitClass : uint32_t { kClsL = 0, kClsN = 1, kClsS = 2, kClsO = 3, kClsX = 4 };
enum SplitPattern : int { kSplitGpt2 = 0, kSplitGpt4 = 1 };

MBPE_SPLIT_HD uint32_t split_class(uint32_t c) {
    if (c >= 0x80u) return kClsX;
    if ((c | 0x20u) - 'a' < 26u) return kClsL;
    if (c - '0' < 10u) return kClsN;
    if (c == 32u || c - 9u < 5u) return kClsS;
    return kClsO;
}

MBPE_SPLIT_HD bool split_is_sync(uint32_t prev, uint32_t cur) {
    return split_class(prev) <= kClsN && split_class(cur) == kClsS;
}

// the sync and non-ASCII bits of 16 text bytes given as four little-endian words (bytes beyond the end of the text
// are 0: an O byte, which neither is nor makes a sync point); prev = the byte before them, or an S byte at the start
// of the text (position 0 is no sync point)
MBPE_SPLIT_HD void split_vec_bits(const uint32_t w[4], uint32_t prev, uint32_t *sync_out, uint32_t *hi_out) {
    uint32_t sync = 0, hi = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (uint32_t k = 0; k < (uint32_t)kSplitVec; ++k) {
        const uint32_t c = (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu;
        sync |= (uint32_t)split_is_sync(prev, c) << k;
        hi |= (c >> 7) << k;
        prev = c;
    }
    *sync_out = sync;
    *hi_out = hi;
}

// the first set bit of bm at a position in [from, limit), or `limit` when there is none; limit <= 64 * n_words
MBPE_SPLIT_HD uint64_t split_next_bit(const unsigned long long *bm, uint64_t from, uint64_t limit) {
    if (from >= limit) return limit;
    uint64_t w = from >> 6;
    unsigned long long m = bm[w] & (~0ull << (from & 63));
    const uint64_t w_last = (limit - 1) >> 6;
    while (m == 0ull) {
        if (w == w_last) return limit;
        m = bm[++w];
    }
    const uint64_t p = (w << 6) + (uint64_t)__builtin_ctzll(m);
    return p < limit ? p : limit;
}

MBPE_SPLIT_HD bool split_any_bit(const unsigned long long *bm, uint64_t from, uint64_t to) {
    return split_next_bit(bm, from, to) < to;
}

// t[j], or an X byte at and beyond the end of the text: it belongs to no run and completes no contraction
MBPE_SPLIT_HD uint32_t split_at(const uint8_t *t, uint64_t j, uint64_t n) { return j < n ? t[j] : 0xFFu; }

// the end of the run of class `cls` that starts at i; runs stop at b (they never reach it unless b == n: t[b - 1] is
// L or N and t[b] is S)
MBPE_SPLIT_HD uint64_t split_run(const uint8_t *t, uint64_t i, uint64_t b, uint32_t cls) {
    while (i < b && split_class(t[i]) == cls) ++i;
    return i;
}

MBPE_SPLIT_HD bool split_is_crlf(uint32_t c) { return c == 10u || c == 13u; }

// The match that starts at i (a <= i < b) in the clean span that ends at b: its end e, i < e <= b.
MBPE_SPLIT_HD uint64_t split_step(const uint8_t *t, uint64_t i, uint64_t b, uint64_t n, int pattern) {
    const uint32_t c = t[i], x = split_at(t, i + 1, n);
    const uint32_t cc = split_class(c), cx = split_class(x);
    if (c == '\'') {                                            // '(?:[sdmt]|ll|ve|re), caseless for gpt4
        const uint32_t fold = pattern == kSplitGpt4 ? 0x20u : 0u;
        const uint32_t x0 = cx == kClsL ? x | fold : x;
        if (x0 == 's' || x0 == 'd' || x0 == 'm' || x0 == 't') return i + 2;
        const uint32_t y = split_at(t, i + 2, n);
        const uint32_t y0 = split_class(y) == kClsL ? y | fold : y;
        if ((x0 == 'l' && y0 == 'l') || (x0 == 'v' && y0 == 'e') || (x0 == 'r' && y0 == 'e')) return i + 3;
    }
    if (pattern == kSplitGpt2) {
        //  ?\p{L}+ |  ?\p{N}+ |  ?[^\s\p{L}\p{N}]+
        if (cc != kClsS) return split_run(t, i + 1, b, cc);
        if (c == ' ' && cx <= kClsO && cx != kClsS) return split_run(t, i + 2, b, cx);
    } else {
        if (cc == kClsL) return split_run(t, i + 1, b, kClsL);                    // [^\r\n\p{L}\p{N}]?+\p{L}+
        if (cc != kClsN && !split_is_crlf(c) && cx == kClsL) return split_run(t, i + 2, b, kClsL);
        if (cc == kClsN) {                                                         // \p{N}{1,3}
            uint64_t e = i + 1;
            while (e < b && e < i + 3 && split_class(t[e]) == kClsN) ++e;
            return e;
        }
        if (cc == kClsO || (c == ' ' && cx == kClsO)) {                            //  ?[^\s\p{L}\p{N}]++[\r\n]*
            uint64_t e = split_run(t, cc == kClsO ? i + 1 : i + 2, b, kClsO);
            while (e < b && split_is_crlf(t[e])) ++e;
            return e;
        }
    }
    // c is S, and no alternative that begins with an optional space applies
    const uint64_t r = split_run(t, i + 1, b, kClsS);
    if (pattern == kSplitGpt4) {                                                   // \s*[\r\n]
        for (uint64_t j = r; j > i; --j)
            if (split_is_crlf(t[j - 1])) return j;
    }
    // \s+(?!\S) | \s+ : the run, less its last byte when something follows it and the run is longer than one byte
    return (r == n || r == i + 1) ? r : r - 1;
}

// The walk of walk thread T over its part of the text: every span whose start lies in [64 T, 64 T + 64).
//   bnd, hi      the boundary (sync | cut) and non-ASCII bitmaps of the text (bits at and beyond n are 0),
//                n_words = ceil(n / 64) words each
//   cut, raw     the cut bitmap and the bitmap of the bytes inside ranges, or NULL when the text has none
//   end(p)       called for the last byte p of every chunk of a clean span, ascending
// Returns the starts of the host spans as a mask of the thread's 64 positions.
template <typename End>
MBPE_SPLIT_HD unsigned long long split_walk_block(const uint8_t *t, uint64_t n, const unsigned long long *bnd,
                                                  const unsigned long long *hi, const unsigned long long *cut,
                                                  const unsigned long long *raw, uint64_t T, uint64_t max_span,
                                                  int pattern, End &end) {
    unsigned long long starts = bnd[T] | (T == 0 ? 1ull : 0ull);       // position 0 starts a span (n > 0: T < n_words)
    if (raw) starts &= ~raw[T];
    unsigned long long host = 0;
    while (starts) {
        const uint32_t k = (uint32_t)__builtin_ctzll(starts);
        starts &= starts - 1;
        const uint64_t a = (T << 6) + k;
        // the span's end: the next boundary, looked for no further than a clean span may reach
        const uint64_t limit = n - a > max_span + 1 ? a + max_span + 1 : n;
        const uint64_t b = split_next_bit(bnd, a + 1, limit);
        if ((b == limit && limit != n) || b - a > max_span || split_any_bit(hi, a, b)) {
            host |= 1ull << k;
            continue;
        }
        const uint64_t n_eff = (cut && b < n && ((cut[b >> 6] >> (b & 63)) & 1ull)) ? b : n;   // a cut ends the text
        for (uint64_t i = a; i < b;) {
            uint64_t e = split_step(t, i, b, n_eff, pattern);
            if (e > b) e = b;
            end(e - 1);
            i = e;
        }
    }
    return host;
}

// one text without cuts or ranges
template <typename End>
MBPE_SPLIT_HD unsigned long long split_walk_block(const uint8_t *t, uint64_t n, const unsigned long long *sync,
                                                  const unsigned long long *hi, uint64_t T, uint64_t max_span,
                                                  int pattern, End &end) {
    return split_walk_block(t, n, sync, hi, nullptr, nullptr, T, max_span, pattern, end);
}

// ---- names (special tokens) in the text ------------------------------------------------------------------------------

constexpr uint32_t kSplitMaxNames = 256;         // mbpe.h: at most so many names ...
constexpr uint32_t kSplitMaxNameBytes = 16384;   // ... and bytes in them
constexpr int kSplitNameBits = 8;                // a hit is (position << 8) | name

struct SplitNames {
    const uint8_t *bytes;        // the names one after the other
    const uint32_t *off;         // n + 1 offsets into bytes
    const uint32_t *first;       // 8 words: bit c is set when a non-empty name starts with byte c
    uint32_t n;
};

// Every occurrence of a non-empty name that starts in the 16 text bytes at `at` (given as two little-endian words,
// bytes beyond the text 0) and ends inside the text: hit(position, name).  Only a byte of the first-byte set costs
// more than one look-up; the rest of a name is compared against the text itself.
template <typename Hit>
MBPE_SPLIT_HD void split_find_vec(const uint8_t *t, uint64_t n, uint64_t at, uint64_t lo, uint64_t up,
                                  const SplitNames &nm, Hit &hit) {
    for (uint32_t k = 0; k < (uint32_t)kSplitVec; ++k) {
        const uint64_t p = at + k;
        if (p >= n) break;
        const uint32_t c = (uint32_t)((k < 8u ? lo >> (8u * k) : up >> (8u * (k - 8u))) & 0xFFu);
        if (!((nm.first[c >> 5] >> (c & 31u)) & 1u)) continue;
        for (uint32_t j = 0; j < nm.n; ++j) {
            const uint32_t o = nm.off[j], len = nm.off[j + 1] - o;
            if (len == 0 || nm.bytes[o] != c || n - p < len) continue;
            uint32_t m = 1;
            while (m < len && t[p + m] == nm.bytes[o + m]) ++m;
            if (m == len) hit(p, j);
        }
    }
}

inline void split_first_set(const uint8_t *names, const uint32_t *off, uint32_t n_names, uint32_t first[8]) {
    for (int i = 0; i < 8; ++i) first[i] = 0;
    for (uint32_t j = 0; j < n_names; ++j)
        if (off[j + 1] > off[j]) first[names[off[j]] >> 5] |= 1u << (names[off[j]] & 31u);
}

// ---- the plan of a call: which occurrences are taken, the parts between them, the cuts (host) -------------------------

constexpr uint32_t kSplitRaw = 0xFFFFFFFFu;      // MBPE_SPLIT_RAW
struct SplitRange { uint64_t start, len; uint32_t name, pad; };   // mbpe_split_range

// hits: (position << 8) | name, ascending, i.e. ordered by (position, name).  An occurrence is taken when it lies
// inside one document and starts at or after the end of the previous one taken in that document (Tokenizer::
// split_on_special).  taken: those; parts: the maximal non-empty stretches of the documents between them.
inline void split_plan_parts(const uint64_t *hits, uint64_t n_hits, const uint64_t *doc_off, uint64_t n_docs,
                             const uint32_t *name_off, std::vector<SplitRange> *taken,
                             std::vector<SplitRange> *parts) {
    taken->clear();
    parts->clear();
    uint64_t h = 0;
    for (uint64_t d = 0; d < n_docs; ++d) {
        const uint64_t s = doc_off[d], e = doc_off[d + 1];
        uint64_t cursor = s;
        for (; h < n_hits && (hits[h] >> kSplitNameBits) < e; ++h) {
            const uint64_t pos = hits[h] >> kSplitNameBits;
            const uint32_t name = (uint32_t)(hits[h] & ((1u << kSplitNameBits) - 1u));
            const uint64_t len = name_off[name + 1] - name_off[name];
            if (pos < cursor || e - pos < len) continue;       // inside one already taken, or straddling two documents
            if (pos > cursor) parts->push_back({cursor, pos - cursor, kSplitRaw, 0});
            taken->push_back({pos, len, name, 0});
            cursor = pos + len;
        }
        if (cursor < e) parts->push_back({cursor, e - cursor, kSplitRaw, 0});
    }
}

// first[k] = the first byte of parts[k] (NULL: no part is NUL-led).  ranges: the taken occurrences and the NUL-led
// parts, ascending; cuts: the start of every part and every taken occurrence but position 0, ascending -- parts and
// occurrences tile the non-empty documents, so these are the document boundaries, the range starts and the range ends.
inline void split_plan_finish(const std::vector<SplitRange> &taken, const std::vector<SplitRange> &parts,
                              const uint8_t *first, std::vector<SplitRange> *ranges, std::vector<uint64_t> *cuts) {
    ranges->clear();
    cuts->clear();
    size_t i = 0, j = 0;
    while (i < taken.size() || j < parts.size()) {
        const bool take = j == parts.size() || (i < taken.size() && taken[i].start < parts[j].start);
        const SplitRange &r = take ? taken[i] : parts[j];
        if (r.start) cuts->push_back(r.start);
        if (take || (first && first[j] == 0)) ranges->push_back(r);
        if (take) ++i; else ++j;
    }
}

}  // namespace mbpe

#endif
