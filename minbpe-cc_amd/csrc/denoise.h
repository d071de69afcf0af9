// Span corruption of token documents for encoder-decoder models (denoise.hip; mbpe_denoise_plan, mbpe_denoise_tokens,
// mbpe_encoder_encode_batch_denoise).  "Span" already means 1,024 scan elements here (span.h), so the objective is
// called denoise throughout.
//
// A document of L_d tokens is cut into units of segment_tokens tokens (one unit where that is 0; the last one shorter;
// an empty document keeps one empty unit).  In a unit of L tokens N of them are noise, in S runs ("noise parts") that
// alternate with S kept parts, kept first (Raffel et al., 2020):
//   inputs    kept_0 s_0 kept_1 s_1 .. kept_{S-1} s_{S-1}        L - N + S ids
//   targets   s_0 noise_0 s_1 noise_1 .. s_{S-1} noise_{S-1}     N + S ids
// N and S are closed forms of (spec, L).  The part boundaries are stratified draws of the dropout hash over the unit's
// seed: boundary j of a cut of T into S parts lies in its own stratum and costs ONE hash, so any lane can compute any
// boundary and no per-unit table is ever stored.  Everything here is integer arithmetic that a host compiler builds too
// (tests/denoise_check.cpp runs it); the host's plan, the length kernel and the gather kernels share this one
// statement of the rule.
#ifndef MBPE_DENOISE_H
#define MBPE_DENOISE_H

#include "mbpe.h"

#include "dropout.h"

namespace mbpe {

constexpr unsigned long long kDnMaxLen = 0xFFFFFFFEull;          // the longest unit the counts are formed for: 2^32 - 2
constexpr uint32_t kDnMaxId = 0x7FFFFFFEu;                       // sentinel ids lie below it
constexpr unsigned long long kDnSent = 1ull << 63;               // a source that is sentinel j: kDnSent | j

// units of a document of L tokens
MBPE_HD unsigned long long dn_units(const mbpe_denoise_spec &s, unsigned long long L) {
    if (s.segment_tokens == 0 || L <= s.segment_tokens) return 1ull;
    return (L + s.segment_tokens - 1) / s.segment_tokens;
}

// tokens of unit u (< dn_units) of such a document; they begin at u * segment_tokens
MBPE_HD unsigned long long dn_unit_len(const mbpe_denoise_spec &s, unsigned long long L, unsigned long long u) {
    if (s.segment_tokens == 0) return L;
    const unsigned long long a = u * s.segment_tokens;
    return L - a < s.segment_tokens ? L - a : s.segment_tokens;
}

// with density > 0 a unit this long is an error of the call: only without segments
MBPE_HD bool dn_too_long(const mbpe_denoise_spec &s, unsigned long long L) {
    return s.density != 0 && dn_unit_len(s, L, 0) > kDnMaxLen;
}

// noise tokens N and noise parts S of a unit of L <= kDnMaxLen tokens; 0, 0: the unit stays as it is
struct DnCounts { unsigned long long N, S; };
MBPE_HD DnCounts dn_counts(const mbpe_denoise_spec &s, unsigned long long L) {
    const unsigned long long lo = s.min_tokens > 2u ? s.min_tokens : 2u;
    DnCounts c = {0ull, 0ull};
    if (s.density == 0 || L < lo || L > kDnMaxLen) return c;
    unsigned long long N = (L * s.density + (1ull << 31)) >> 32;          // (L < 2^32 - 1, density <= 2^32: no wrap)
    N = N < 1 ? 1 : N > L - 1 ? L - 1 : N;
    // (a 64-bit division is a long routine on the device; almost every unit is short enough for a 32-bit one)
    unsigned long long S = (N >> 23) == 0 ? (unsigned long long)((uint32_t)(N * 256 + s.mean_span_q8 / 2) / s.mean_span_q8)
                                          : (N * 256 + s.mean_span_q8 / 2) / s.mean_span_q8;
    if (S > N) S = N;
    if (S > L - N) S = L - N;
    if (S > s.n_sentinels) S = s.n_sentinels;
    c.N = N;
    c.S = S < 1 ? 1 : S;
    return c;
}
MBPE_HD unsigned long long dn_in_len(DnCounts c, unsigned long long L) { return L - c.N + c.S; }
MBPE_HD unsigned long long dn_tg_len(DnCounts c) { return c.N + c.S; }

// the seed of document d of the call, and of its unit u
MBPE_HD unsigned long long dn_doc_seed(const mbpe_denoise_spec &s, unsigned long long d) {
    const unsigned long long g = s.doc_base + d;
    return ((unsigned long long)drop_hash(s.seed, g, 0x44454E00u) << 32) | drop_hash(s.seed, g, 0x44454E01u);
}
MBPE_HD unsigned long long dn_unit_seed(unsigned long long sg, unsigned long long u) {
    return ((unsigned long long)drop_hash(sg, u, 2u) << 32) | drop_hash(sg, u, 3u);
}

// A cut of T into S >= 1 parts of at least one: E = T - S excess tokens over strata q(j) = floor(j * E / S).  With
// E = a * S + b, q(j) = j * a + floor(j * b / S), and q(j) - q(j - 1) is a or a + 1: one division per boundary, a 32-bit
// one whenever (j - 1) * b fits 32 bits -- every unit of up to 65,536 parts (the 64-bit routine is some hundred
// instructions on the device, and a lane draws a dozen boundaries per 16-byte piece)
struct DnCut {
    unsigned long long T, S, a, b;
};
MBPE_HD DnCut dn_cut(unsigned long long T, unsigned long long S) {       // T, S < 2^32
    DnCut c = {T, S, 0ull, 0ull};
    if (S) {
        c.a = (uint32_t)(T - S) / (uint32_t)S;
        c.b = (uint32_t)(T - S) - (uint32_t)c.a * (uint32_t)S;
    }
    return c;
}

// boundary j in [0, S] of the cut, with draw c: strictly ascending in j, 0 at j == 0 and T at j == S;
// B_j = j + q(j - 1) + ((h(su, j, c) * (q(j) - q(j - 1) + 1)) >> 32).  j, a, b < 2^32 and j * a <= E, so no product wraps
MBPE_HD unsigned long long dn_bound(unsigned long long su, const DnCut &k, uint32_t c, unsigned long long j) {
    if (j == 0) return 0ull;
    if (j >= k.S) return k.T;
    const unsigned long long x = (j - 1) * k.b;
    unsigned long long f, r;
    if ((x >> 32) == 0) {
        f = (uint32_t)x / (uint32_t)k.S;
        r = (uint32_t)x - (uint32_t)f * (uint32_t)k.S;
    } else {
        f = x / k.S;
        r = x - f * k.S;
    }
    const unsigned long long q0 = (j - 1) * k.a + f, w = k.a + (r + k.b >= k.S ? 1ull : 0ull);   // w = q(j) - q(j - 1)
    return j + q0 + (((unsigned long long)drop_hash(su, j, c) * (w + 1)) >> 32);
}

// one unit, as the maps below need it
struct DnUnit {
    unsigned long long su, L, N, S;
    DnCut noise, kept;
};
MBPE_HD unsigned long long dn_bn(const DnUnit &u, unsigned long long j) { return dn_bound(u.su, u.noise, 0u, j); }
MBPE_HD unsigned long long dn_bm(const DnUnit &u, unsigned long long j) { return dn_bound(u.su, u.kept, 1u, j); }

// the id of sentinel j (< n_sentinels)
MBPE_HD uint32_t dn_sentinel(const mbpe_denoise_spec &s, unsigned long long j) {
    return s.sentinel_down ? s.sentinel_id - (uint32_t)j : s.sentinel_id + (uint32_t)j;
}

// A place in one side of a unit: part j, `mark` the position of the sentinel the walk meets next (inputs: s_j, behind
// kept part j; targets: s_{j+1}, behind noise part j; beyond the side's end where there is none), and `add`: a
// position p of part j that is no sentinel holds the unit's token p + add.  A unit that stays as it is has S == 0:
// its inputs are its tokens, mark lies beyond them
struct DnCur {
    unsigned long long j, mark, add;
};

MBPE_HD void dn_in_enter(const DnUnit &u, unsigned long long j, DnCur *c) {
    c->j = j;
    if (u.S == 0) { c->mark = ~0ull; c->add = 0; return; }
    c->mark = dn_bm(u, j + 1) + j;
    c->add = dn_bn(u, j) - j;
}
// the part of input position p < L - N + S: the smallest j with Bm[j + 1] + j >= p
MBPE_HD void dn_in_seek(const DnUnit &u, unsigned long long p, DnCur *c) {
    unsigned long long lo = 0, hi = u.S ? u.S - 1 : 0;
    while (lo < hi) {
        const unsigned long long m = lo + (hi - lo) / 2;
        if (dn_bm(u, m + 1) + m >= p) hi = m; else lo = m + 1;
    }
    dn_in_enter(u, lo, c);
}
// what stands at input position p, the cursor on p's part: a token's index in the unit, or kDnSent | j; then the
// cursor is on the part of p + 1 (if there is one)
MBPE_HD unsigned long long dn_in_step(const DnUnit &u, unsigned long long p, DnCur *c) {
    if (p != c->mark) return p + c->add;
    const unsigned long long j = c->j;
    if (j + 1 < u.S) dn_in_enter(u, j + 1, c);
    return kDnSent | j;
}

// targets: the cursor also keeps where its own sentinel stands
struct DnTgCur {
    unsigned long long j, at, mark, add;
};
MBPE_HD void dn_tg_enter(const DnUnit &u, unsigned long long j, unsigned long long at, DnTgCur *c) {
    c->j = j;
    c->at = at;                                                  // Bn[j] + j
    c->mark = dn_bn(u, j + 1) + j + 1;
    c->add = dn_bm(u, j + 1) - j - 1;
}
// the part of target position p < N + S (S >= 1): the largest j with Bn[j] + j <= p
MBPE_HD void dn_tg_seek(const DnUnit &u, unsigned long long p, DnTgCur *c) {
    unsigned long long lo = 0, hi = u.S - 1;
    while (lo < hi) {
        const unsigned long long m = lo + (hi - lo + 1) / 2;
        if (dn_bn(u, m) + m <= p) lo = m; else hi = m - 1;
    }
    dn_tg_enter(u, lo, dn_bn(u, lo) + lo, c);
}
MBPE_HD unsigned long long dn_tg_step(const DnUnit &u, unsigned long long p, DnTgCur *c) {
    const unsigned long long r = p == c->at ? (kDnSent | c->j) : p + c->add;
    if (p + 1 == c->mark && c->j + 1 < u.S) dn_tg_enter(u, c->j + 1, c->mark, c);
    return r;
}

// both maps for a single position
MBPE_HD unsigned long long dn_in_source(const DnUnit &u, unsigned long long p) {
    DnCur c;
    dn_in_seek(u, p, &c);
    return dn_in_step(u, p, &c);
}
MBPE_HD unsigned long long dn_tg_source(const DnUnit &u, unsigned long long p) {
    DnTgCur c;
    dn_tg_seek(u, p, &c);
    return dn_tg_step(u, p, &c);
}

// unit u of document d of the call, which has L_d tokens
MBPE_HD DnUnit dn_unit(const mbpe_denoise_spec &s, unsigned long long d, unsigned long long L_d, unsigned long long u) {
    DnUnit r;
    r.L = dn_unit_len(s, L_d, u);
    const DnCounts c = dn_counts(s, r.L);
    r.N = c.N;
    r.S = c.S;
    r.su = c.S ? dn_unit_seed(dn_doc_seed(s, d), u) : 0ull;
    r.noise = dn_cut(c.N, c.S);
    r.kept = dn_cut(r.L - c.N, c.S);
    return r;
}

// the rules of a spec for tokens of token_bits bits, without a word: MBPE_OK, MBPE_ERR_ARG or MBPE_ERR_VOCAB, *msg says why
inline int denoise_check_spec(const mbpe_denoise_spec *s, uint32_t token_bits, const char **msg) {
    *msg = "";
    if (!s) { *msg = "NULL denoise spec"; return MBPE_ERR_ARG; }
    if (s->density > kDropoutOne) { *msg = "a denoise density above 2^32"; return MBPE_ERR_ARG; }
    if (s->mean_span_q8 < 256u) { *msg = "a denoise mean_span_q8 below 256 (one token)"; return MBPE_ERR_ARG; }
    if (s->n_sentinels == 0) { *msg = "denoise n_sentinels is 0"; return MBPE_ERR_ARG; }
    if (s->sentinel_down > 1u) { *msg = "denoise sentinel_down must be 0 or 1"; return MBPE_ERR_ARG; }
    const unsigned long long span = s->n_sentinels - 1ull;
    if (s->sentinel_id >= kDnMaxId || (s->sentinel_down ? span > s->sentinel_id : s->sentinel_id + span >= kDnMaxId)) {
        *msg = "the denoise sentinel ids leave [0, 2^31 - 2)";
        return MBPE_ERR_ARG;
    }
    if (token_bits == 16 && (s->sentinel_down ? s->sentinel_id : s->sentinel_id + span) >= 65536ull) {
        *msg = "a denoise sentinel id that does not fit 16-bit tokens";
        return MBPE_ERR_VOCAB;
    }
    return MBPE_OK;
}

// the host's plan of n_docs documents with token offsets off[0 .. n_docs].  *n_units always; where cap_units holds them
// and the pointers are given, in_off and tg_off (n_units + 1 each) and unit_doc (n_units).  MBPE_OK, or MBPE_ERR_ARG
// with *bad_doc the first document that is dn_too_long (then nothing is written), or with *bad_doc ~0 for more than
// 2^40 units
inline int denoise_plan_host(const uint64_t *off, uint64_t n_docs, const mbpe_denoise_spec &s, uint64_t *n_units,
                             uint64_t *in_off, uint64_t *tg_off, uint64_t *unit_doc, uint64_t cap_units, uint64_t *bad_doc) {
    uint64_t n = 0;
    *n_units = 0;
    *bad_doc = ~0ull;
    for (uint64_t d = 0; d < n_docs; ++d) {
        const uint64_t L = off[d + 1] - off[d];
        if (dn_too_long(s, L)) { *bad_doc = d; return MBPE_ERR_ARG; }
        n += dn_units(s, L);
        if (n >> 40) return MBPE_ERR_ARG;
    }
    *n_units = n;
    if (cap_units < n) return MBPE_OK;
    uint64_t k = 0, oi = 0, ot = 0;
    for (uint64_t d = 0; d < n_docs; ++d) {
        const uint64_t L = off[d + 1] - off[d], U = dn_units(s, L);
        for (uint64_t u = 0; u < U; ++u, ++k) {
            const uint64_t Lu = dn_unit_len(s, L, u);
            const DnCounts c = dn_counts(s, Lu);
            if (in_off) in_off[k] = oi;
            if (tg_off) tg_off[k] = ot;
            if (unit_doc) unit_doc[k] = d;
            oi += dn_in_len(c, Lu);
            ot += c.S ? dn_tg_len(c) : 0;
        }
    }
    if (in_off) in_off[n] = oi;
    if (tg_off) tg_off[n] = ot;
    return MBPE_OK;
}

#ifdef __HIPCC__
// ---- the device stage (denoise.hip) -----------------------------------------------------------------------------------
// What it leaves on the device for n_docs > 0 documents and room for cap_units >= the units they make:
//   uoff      n_docs + 1: the documents' unit offsets; uoff[n_docs] the unit count
//   unit_doc  cap_units; in_off, tg_off  cap_units + 1 each: the units' offsets into the two new streams
//   res       4 words: units, input ids, target ids, the first document that is dn_too_long or ~0
//   scratch   dn_scratch_bytes(n_docs, cap_units): the scans' span sums
//   row_doc   NULL, or cap_units uint32: unit_doc again, as a matrix row's document
// in and tg: the new flat streams, plain ids of `bits`; no more than cap_in / cap_tg ids are written (cap 0: that side
// is not gathered, a pointer may be NULL).
uint64_t dn_scratch_bytes(uint64_t n_docs, uint64_t cap_units);
struct DnDst {
    void *in, *tg;
    uint64_t cap_in, cap_tg;
    unsigned long long *uoff, *unit_doc, *in_off, *tg_off, *res, *scratch;
    uint32_t *row_doc;
    uint64_t cap_units;
};

// every kernel of the stage on `stream` over tok (`bits` bits: 16 plain ids, 32 with bit 31 ignored) and doc_off
// (n_docs + 1, device).  n_docs > 0.  The unit count stays on the device: the kernels behind the first scan read it
// there.  Nothing is waited for and nothing comes back: the totals and the flag are the 32 bytes at dst.res
void dn_launch(hipStream_t stream, const void *tok, uint32_t bits, const unsigned long long *doc_off, uint64_t n_docs,
               const mbpe_denoise_spec &spec, const DnDst &dst);
#endif

}  // namespace mbpe

#endif
