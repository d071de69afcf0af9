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
//   step         the rule: step(t, i, b, n_eff) = the end of the match that starts at i; step.whole(t, a, b, n) = false
//                when the span's edges rule the walk out
template <typename Step, typename End>
MBPE_SPLIT_HD unsigned long long split_walk_block_with(const uint8_t *t, uint64_t n, const unsigned long long *bnd,
                                                       const unsigned long long *hi, const unsigned long long *cut,
                                                       const unsigned long long *raw, uint64_t T, uint64_t max_span,
                                                       const Step &step, End &end) {
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
        if ((b == limit && limit != n) || b - a > max_span || split_any_bit(hi, a, b) || !step.whole(t, a, b, n)) {
            host |= 1ull << k;
            continue;
        }
        const uint64_t n_eff = (cut && b < n && ((cut[b >> 6] >> (b & 63)) & 1ull)) ? b : n;   // a cut ends the text
        for (uint64_t i = a; i < b;) {
            uint64_t e = step(t, i, b, n_eff);
            if (e > b) e = b;
            end(e - 1);
            i = e;
        }
    }
    return host;
}

struct SplitByteStep {
    int pattern;
    MBPE_SPLIT_HD bool whole(const uint8_t *, uint64_t, uint64_t, uint64_t) const { return true; }
    MBPE_SPLIT_HD uint64_t operator()(const uint8_t *t, uint64_t i, uint64_t b, uint64_t n) const {
        return split_step(t, i, b, n, pattern);
    }
};

template <typename End>
MBPE_SPLIT_HD unsigned long long split_walk_block(const uint8_t *t, uint64_t n, const unsigned long long *bnd,
                                                  const unsigned long long *hi, const unsigned long long *cut,
                                                  const unsigned long long *raw, uint64_t T, uint64_t max_span,
                                                  int pattern, End &end) {
    const SplitByteStep step = {pattern};
    return split_walk_block_with(t, n, bnd, hi, cut, raw, T, max_span, step, end);
}

// one text without cuts or ranges
template <typename End>
MBPE_SPLIT_HD unsigned long long split_walk_block(const uint8_t *t, uint64_t n, const unsigned long long *sync,
                                                  const unsigned long long *hi, uint64_t T, uint64_t max_span,
                                                  int pattern, End &end) {
    return split_walk_block(t, n, sync, hi, nullptr, nullptr, T, max_span, pattern, end);
}

// ---- the same rule on code points ("unicode" mode) -----------------------------------------------------
//
// "Byte" reads "well-formed UTF-8 sequence" and the class of a scalar value comes from a table that PCRE2 itself filled
// (host/presplit.cpp: split_unicode_table), 2 bits per value.  The fold set holds the values >= 0x80 that PCRE2 matches
// caselessly against one of s d m t l v e r (gpt4 contractions).  The second bitmap of the sync pass is here the
// ILL-FORMED bitmap: a bit for every byte >= 0x80 that is not part of a well-formed sequence (Unicode Table 3-7) of the
// text; a span with such a bit, or whose first byte or the byte behind it is a continuation byte (a cut inside a
// sequence), is a host span as before.  Sync points, all of them on the first byte of a well-formed sequence that
// follows a well-formed sequence:
//   (A) both patterns: the previous scalar value is L or N, the next is S;
//   (B) gpt4: the previous is CR or LF, the next is not S;  gpt2: the previous is S but not U+0020, the next is not S.
// So the walk decodes only bytes the sync pass has checked: those of its span, and the sequence at b when b is a sync
// point (at a cut and at the end of the text nothing is read at b).

constexpr uint32_t kSplitTableWords = 0x110000u / 16u;     // 2 bits per scalar value: 278,528 bytes
constexpr uint32_t kSplitMaxFold = 8;
constexpr uint32_t kSplitNoChar = 0xFFFFFFFFu;             // "beyond the text": class X, completes nothing

struct SplitFold { uint32_t n; uint32_t cp[kSplitMaxFold]; uint8_t to[kSplitMaxFold]; };
struct SplitChar { uint32_t cp, len; };

MBPE_SPLIT_HD uint32_t split_class_u(const uint32_t *tab, uint32_t cp) {
    if (cp < 0x80u) return split_class(cp);                 // (the table says the same: checked where it is built)
    if (cp >= 0x110000u) return kClsX;
    return (tab[cp >> 4] >> (2u * (cp & 15u))) & 3u;
}

MBPE_SPLIT_HD bool split_is_cont(uint32_t c) { return (c & 0xC0u) == 0x80u; }

// the sequence that starts at j < n when it is well-formed and ends inside the text, else {kSplitNoChar, 0}; reads
// t[j .. j + 3] at most, and nothing at or beyond n
MBPE_SPLIT_HD SplitChar split_decode_checked(const uint8_t *t, uint64_t j, uint64_t n) {
    const SplitChar none = {kSplitNoChar, 0u};
    const uint32_t c0 = t[j];
    if (c0 < 0x80u) return {c0, 1u};
    if (c0 < 0xC2u || c0 > 0xF4u) return none;               // a continuation byte, C0, C1, F5 .. FF
    const uint32_t len = c0 < 0xE0u ? 2u : c0 < 0xF0u ? 3u : 4u;
    if (n - j < len) return none;
    const uint32_t c1 = t[j + 1];
    uint32_t lo = 0x80u, up = 0xBFu;                          // Table 3-7: the second byte's range depends on the first
    if (c0 == 0xE0u) lo = 0xA0u;
    else if (c0 == 0xEDu) up = 0x9Fu;
    else if (c0 == 0xF0u) lo = 0x90u;
    else if (c0 == 0xF4u) up = 0x8Fu;
    if (c1 < lo || c1 > up) return none;
    if (len == 2u) return {((c0 & 0x1Fu) << 6) | (c1 & 0x3Fu), 2u};
    const uint32_t c2 = t[j + 2];
    if (!split_is_cont(c2)) return none;
    if (len == 3u) return {((c0 & 0x0Fu) << 12) | ((c1 & 0x3Fu) << 6) | (c2 & 0x3Fu), 3u};
    const uint32_t c3 = t[j + 3];
    if (!split_is_cont(c3)) return none;
    return {((c0 & 0x07u) << 18) | ((c1 & 0x3Fu) << 12) | ((c2 & 0x3Fu) << 6) | (c3 & 0x3Fu), 4u};
}

// the walk's decode: the sequence at j is known to be well-formed when j < n; {kSplitNoChar, 0} at and beyond n.  It is
// the checked decode all the same -- what it costs over an unchecked one is compares on bytes already loaded -- so
// that no byte is ever trusted: an ill-formed sequence here would read as "beyond the text".
MBPE_SPLIT_HD SplitChar split_char(const uint8_t *t, uint64_t j, uint64_t n) {
    if (j >= n) return {kSplitNoChar, 0u};
    return split_decode_checked(t, j, n);
}

MBPE_SPLIT_HD bool split_is_sync_u(uint32_t prev_cp, uint32_t prev_cls, uint32_t cur_cls, int pattern) {
    if (prev_cls <= kClsN) return cur_cls == kClsS;                                             // (A)
    if (cur_cls == kClsS) return false;
    return pattern == kSplitGpt4 ? split_is_crlf(prev_cp) : (prev_cls == kClsS && prev_cp != 32u);    // (B)
}

// The sync and ill-formed bits of the text bytes [at, at + 16) clipped to n (at < n, at a multiple of 16; bits at and
// beyond n are 0): one lane of the sync pass.  w = those bytes as four little-endian words, bytes beyond the text 0.
// A lane whose bytes and the byte before them are ASCII decides on w alone; any other lane reads the text as plain
// bytes, from t[at - 4] (the longest sequence that can end at at - 1) to t[at + 18] (... that can start at at + 15).
// Every bit is a function of the text around its position alone, so lanes agree on sequences they share.
MBPE_SPLIT_HD void split_vec_bits_u(const uint8_t *t, uint64_t n, uint64_t at, const uint32_t w[4], int pattern,
                                    const uint32_t *tab, uint32_t *sync_out, uint32_t *bad_out) {
    const uint32_t valid = n - at < (uint64_t)kSplitVec ? (uint32_t)(n - at) : (uint32_t)kSplitVec;
    const uint32_t before = at ? t[at - 1] : (uint32_t)' ';
    uint32_t sync = 0, bad = 0;
    if ((((w[0] | w[1] | w[2] | w[3]) & 0x80808080u) | (before & 0x80u)) == 0u) {
        uint32_t prev = before, prev_cls = at ? split_class(before) : (uint32_t)kClsX;      // position 0 is no sync point
#ifdef __HIPCC__
#pragma unroll
#endif
        for (uint32_t k = 0; k < (uint32_t)kSplitVec; ++k) {
            const uint32_t c = (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu, cls = split_class(c);
            sync |= (uint32_t)(prev_cls != kClsX && split_is_sync_u(prev, prev_cls, cls, pattern)) << k;
            prev = c;
            prev_cls = cls;
        }
        *sync_out = sync & ((1u << valid) - 1u);
        *bad_out = 0u;
        return;
    }
    // the sequence that ends at at - 1 or reaches into the lane: it starts at the nearest byte before `at`, at most 4
    // back, that is no continuation byte
    const uint64_t end = at + valid;
    uint64_t q = at;
    uint32_t prev = 0, prev_cls = kClsX;                     // X: no well-formed sequence ends right before q
    for (uint32_t d = 1; d <= 4u && d <= at; ++d) {
        if (split_is_cont(t[at - d])) continue;
        const SplitChar p = split_decode_checked(t, at - d, n);
        if (p.len >= d) {                                    // (len 0: ill-formed, and what follows it is on its own)
            q = at - d + p.len;
            prev = p.cp;
            prev_cls = split_class_u(tab, p.cp);
        }
        break;
    }
    while (q < end) {
        const SplitChar c = split_decode_checked(t, q, n);
        if (c.len == 0u) {                                   // ill-formed, or a continuation byte that belongs to nothing
            bad |= 1u << (uint32_t)(q - at);
            prev_cls = kClsX;
            ++q;
            continue;
        }
        const uint32_t cls = split_class_u(tab, c.cp);
        if (prev_cls != kClsX && split_is_sync_u(prev, prev_cls, cls, pattern)) sync |= 1u << (uint32_t)(q - at);
        prev = c.cp;
        prev_cls = cls;
        q += c.len;
    }
    *sync_out = sync;
    *bad_out = bad;
}

// x as the contraction letters see it: gpt4 folds case, through the ASCII fold and the fold set
MBPE_SPLIT_HD uint32_t split_fold_u(uint32_t cp, int pattern, const SplitFold &fold) {
    if (pattern != kSplitGpt4) return cp;
    if (cp < 0x80u) return split_class(cp) == kClsL ? cp | 0x20u : cp;
    uint32_t to = cp;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (uint32_t k = 0; k < kSplitMaxFold; ++k)             // (unrolled: the set stays in scalar registers)
        if (k < fold.n && fold.cp[k] == cp) to = fold.to[k];
    return to;
}

MBPE_SPLIT_HD uint64_t split_run_u(const uint8_t *t, uint64_t i, uint64_t b, uint64_t n, uint32_t cls,
                                   const uint32_t *tab) {
    while (i < b) {
        const SplitChar c = split_char(t, i, n);
        if (c.len == 0u || split_class_u(tab, c.cp) != cls) break;
        i += c.len;
    }
    return i;
}

// split_step on scalar values: the match that starts at i (a <= i < b, the first byte of a sequence) in the span that
// ends at b, all of whose sequences are well-formed: its end e, i < e.  n = the end of the text, or b when b is a cut.
MBPE_SPLIT_HD uint64_t split_step_u(const uint8_t *t, uint64_t i, uint64_t b, uint64_t n, int pattern,
                                    const uint32_t *tab, const SplitFold &fold) {
    const SplitChar c = split_char(t, i, n);
    if (c.len == 0u) return b;                               // (not reached: the span was checked)
    const uint64_t i1 = i + c.len;
    const SplitChar x = split_char(t, i1, n);
    const uint32_t cc = split_class_u(tab, c.cp), cx = split_class_u(tab, x.cp);
    if (c.cp == '\'') {                                        // '(?:[sdmt]|ll|ve|re), caseless for gpt4
        const uint32_t x0 = split_fold_u(x.cp, pattern, fold);
        if (x0 == 's' || x0 == 'd' || x0 == 'm' || x0 == 't') return i1 + x.len;
        const SplitChar y = split_char(t, i1 + x.len, n);
        const uint32_t y0 = split_fold_u(y.cp, pattern, fold);
        if ((x0 == 'l' && y0 == 'l') || (x0 == 'v' && y0 == 'e') || (x0 == 'r' && y0 == 'e')) return i1 + x.len + y.len;
    }
    if (pattern == kSplitGpt2) {
        //  ?\p{L}+ |  ?\p{N}+ |  ?[^\s\p{L}\p{N}]+ : the lead is U+0020 only
        if (cc != kClsS) return split_run_u(t, i1, b, n, cc, tab);
        if (c.cp == ' ' && cx <= kClsO && cx != kClsS) return split_run_u(t, i1 + x.len, b, n, cx, tab);
    } else {
        if (cc == kClsL) return split_run_u(t, i1, b, n, kClsL, tab);            // [^\r\n\p{L}\p{N}]?+\p{L}+
        if (cc != kClsN && !split_is_crlf(c.cp) && cx == kClsL) return split_run_u(t, i1 + x.len, b, n, kClsL, tab);
        if (cc == kClsN) {                                                         // \p{N}{1,3}: scalar values
            uint64_t e = i1;
            for (int k = 1; k < 3 && e < b; ++k) {
                const SplitChar d = split_char(t, e, n);
                if (d.len == 0u || split_class_u(tab, d.cp) != kClsN) break;
                e += d.len;
            }
            return e;
        }
        if (cc == kClsO || (c.cp == ' ' && cx == kClsO)) {                         //  ?[^\s\p{L}\p{N}]++[\r\n]*
            uint64_t e = split_run_u(t, cc == kClsO ? i1 : i1 + x.len, b, n, kClsO, tab);
            while (e < b && split_is_crlf(t[e])) ++e;
            return e;
        }
    }
    // c is S, and no alternative that begins with an optional lead applies
    const uint64_t r = split_run_u(t, i1, b, n, kClsS, tab);
    if (pattern == kSplitGpt4) {                                                   // \s*[\r\n] (CR, LF are bytes of no other sequence)
        for (uint64_t j = r; j > i; --j)
            if (split_is_crlf(t[j - 1])) return j;
    }
    // \s+(?!\S) | \s+ : the run, less its last scalar value when something follows it and the run is longer than one
    if (r == n || r == i1) return r;
    uint64_t j = r - 1;
    while (j > i1 && split_is_cont(t[j])) --j;
    return j;
}

// the walk in unicode mode: hi = the ill-formed bitmap.  A span whose first byte, or the byte behind it, is a
// continuation byte lies at a cut inside a sequence: the host's, like every span that is not well-formed.
struct SplitCharStep {
    int pattern;
    const uint32_t *tab;
    SplitFold fold;
    MBPE_SPLIT_HD bool whole(const uint8_t *t, uint64_t a, uint64_t b, uint64_t n) const {
        return !split_is_cont(t[a]) && !(b < n && split_is_cont(t[b]));
    }
    MBPE_SPLIT_HD uint64_t operator()(const uint8_t *t, uint64_t i, uint64_t b, uint64_t n) const {
        const uint64_t e = split_step_u(t, i, b, n, pattern, tab, fold);
        return e > i ? e : b;
    }
};

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
