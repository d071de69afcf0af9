// The fill-in-the-middle transform of token documents (fim.hip; mbpe_fim_plan, mbpe_fim_tokens, mbpe_encoder_set_fim).
//
// A document of L tokens t[0 .. L) is cut at two points a <= b into prefix t[0:a], middle t[a:b] and suffix t[b:L] and
// rewritten with three sentinel ids around the parts (Bavarian et al., 2022):
//   PSM   pre P suf S mid M            SPM   pre suf S mid P M            either way L + 3 ids
// Whether a document is transformed, where it is cut and which order it gets are pure functions of (spec, g, L), g = the
// document's number in the caller's corpus: four draws u_i = drop_hash(seed, g, i) -- dropout.h's hash, the document
// number where the byte offset stood and the draw's index where the merged id stood.  Everything here is integer
// arithmetic that a host compiler builds too (tests/fim_check.cpp runs it); the host's plan, the plan kernel and the
// gather kernel share this one statement of the rule.
#ifndef MBPE_FIM_H
#define MBPE_FIM_H

#include "mbpe.h"

#include "dropout.h"

namespace mbpe {

constexpr uint32_t kFimNone = 0, kFimPsm = 1, kFimSpm = 2;       // a plan's mode
constexpr unsigned long long kFimMaxLen = 0xFFFFFFFEull;         // the longest document the cuts are drawn for: 2^32 - 2
constexpr uint32_t kFimMaxId = 0x7FFFFFFEu;                      // sentinel ids lie below it

// what becomes of one document: mode, and the cuts a <= b (0 where mode is kFimNone)
struct FimPlan {
    uint32_t mode;
    unsigned long long a, b;
};

// with rate > 0 a document this long is an error of the call, not a document left as it is
MBPE_HD bool fim_too_long(const mbpe_fim_spec &s, unsigned long long L) { return s.rate != 0 && L > kFimMaxLen; }

// floor(u * (L + 1) / 2^32) in [0, L]; L <= kFimMaxLen, so the product stays below 2^64
MBPE_HD unsigned long long fim_cut(uint32_t u, unsigned long long L) { return ((unsigned long long)u * (L + 1)) >> 32; }

// the plan of document d of the call, L tokens long (a document fim_too_long refuses is left as it is)
MBPE_HD FimPlan fim_plan_doc(const mbpe_fim_spec &s, unsigned long long d, unsigned long long L) {
    const unsigned long long g = s.doc_base + d;
    const unsigned long long lo = s.min_tokens > 1u ? s.min_tokens : 1u;
    FimPlan p = {kFimNone, 0ull, 0ull};
    if (L < lo || (s.max_tokens != 0 && L > s.max_tokens) || L > kFimMaxLen) return p;
    if ((unsigned long long)drop_hash(s.seed, g, 0u) >= s.rate) return p;
    const unsigned long long c1 = fim_cut(drop_hash(s.seed, g, 1u), L), c2 = fim_cut(drop_hash(s.seed, g, 2u), L);
    p.a = c1 < c2 ? c1 : c2;
    p.b = c1 < c2 ? c2 : c1;
    p.mode = (unsigned long long)drop_hash(s.seed, g, 3u) < s.spm ? kFimSpm : kFimPsm;
    return p;
}

// ids of the document afterwards
MBPE_HD unsigned long long fim_len(uint32_t mode, unsigned long long L) { return mode == kFimNone ? L : L + 3; }

// what stands at position k < fim_len of the new document: a token of the old one (its index, < L) or a sentinel
constexpr unsigned long long kFimSrcPre = ~0ull, kFimSrcSuf = ~0ull - 1, kFimSrcMid = ~0ull - 2;

MBPE_HD unsigned long long fim_source(const FimPlan &p, unsigned long long L, unsigned long long k) {
    if (p.mode == kFimNone) return k;
    if (k == 0) return kFimSrcPre;
    const unsigned long long ns = L - p.b;                       // the suffix
    if (p.mode == kFimPsm) {                                     // pre P suf S mid M
        if (k <= p.a) return k - 1;
        if (k == p.a + 1) return kFimSrcSuf;
        if (k < p.a + 2 + ns) return p.b + (k - (p.a + 2));
        if (k == p.a + 2 + ns) return kFimSrcMid;
        return p.a + (k - (p.a + 3 + ns));
    }
    if (k == 1) return kFimSrcSuf;                               // pre suf S mid P M
    if (k < 2 + ns) return p.b + (k - 2);
    if (k == 2 + ns) return kFimSrcMid;
    return k - (3 + ns);                                         // (P and M follow each other as they did)
}

// the rules of a spec for tokens of token_bits bits, without a word: MBPE_OK, MBPE_ERR_ARG or MBPE_ERR_VOCAB, *msg says why
inline int fim_check_spec(const mbpe_fim_spec *s, uint32_t token_bits, const char **msg) {
    *msg = "";
    if (!s) { *msg = "NULL fim spec"; return MBPE_ERR_ARG; }
    if (s->rate > kDropoutOne || s->spm > kDropoutOne) { *msg = "a fim threshold above 2^32"; return MBPE_ERR_ARG; }
    if (s->max_tokens != 0 && s->min_tokens > s->max_tokens) { *msg = "fim min_tokens exceeds max_tokens"; return MBPE_ERR_ARG; }
    if (s->pre_id >= kFimMaxId || s->suf_id >= kFimMaxId || s->mid_id >= kFimMaxId) {
        *msg = "a fim sentinel id of 2^31 - 2 or more";
        return MBPE_ERR_ARG;
    }
    if (token_bits == 16 && (s->pre_id >= 65536u || s->suf_id >= 65536u || s->mid_id >= 65536u)) {
        *msg = "a fim sentinel id that does not fit 16-bit tokens";
        return MBPE_ERR_VOCAB;
    }
    return MBPE_OK;
}

// the host's plan of n_docs documents with token offsets off[0 .. n_docs]: off_out (n_docs + 1), and where given
// mode_out (n_docs) and cut_out (2 per document).  MBPE_OK, or MBPE_ERR_ARG with *bad_doc the first document that is
// fim_too_long (nothing is to be trusted then)
inline int fim_plan_host(const uint64_t *off, uint64_t n_docs, const mbpe_fim_spec &s, uint64_t *off_out, uint8_t *mode_out,
                         uint64_t *cut_out, uint64_t *bad_doc) {
    uint64_t o = 0;
    for (uint64_t d = 0; d < n_docs; ++d) {
        const uint64_t L = off[d + 1] - off[d];
        if (fim_too_long(s, L)) { *bad_doc = d; return MBPE_ERR_ARG; }
        const FimPlan p = fim_plan_doc(s, d, L);
        off_out[d] = o;
        o += fim_len(p.mode, L);
        if (mode_out) mode_out[d] = (uint8_t)p.mode;
        if (cut_out) { cut_out[2 * d] = p.a; cut_out[2 * d + 1] = p.b; }
    }
    off_out[n_docs] = o;
    return MBPE_OK;
}

#ifdef __HIPCC__
// ---- the device stage (fim.hip) ---------------------------------------------------------------------------------------
// What it leaves on the device for n_docs > 0 documents: off = the new token offsets (n_docs + 1; off[n_docs] the new
// token count), behind them one word that holds the number of the first fim_too_long document or ~0, then the scan's
// scratch; cut = a, b per document; mode = one byte per document; tok = the new flat stream, plain ids of `bits`.
uint64_t fim_off_bytes(uint64_t n_docs);
struct FimDst {
    void *tok;
    uint64_t cap;                            // ids tok holds; the kernel writes no more than these
    unsigned long long *off;                 // fim_off_bytes(n_docs)
    unsigned long long *cut;                 // 2 * n_docs
    uint8_t *mode;                           // n_docs
};

// k_fim_plan, the scan, k_fim_offsets and k_fim_gather on `stream` over tok (n_tokens of `bits` bits: 16 plain ids, 32
// with bit 31 ignored) and doc_off (n_docs + 1, device).  n_docs > 0.  Nothing is waited for and nothing comes back:
// the new token count and the flag are the 16 bytes at dst.off + n_docs
void fim_launch(hipStream_t stream, const void *tok, uint64_t n_tokens, uint32_t bits, const unsigned long long *doc_off,
                uint64_t n_docs, const mbpe_fim_spec &spec, const FimDst &dst);
#endif

}  // namespace mbpe

#endif
