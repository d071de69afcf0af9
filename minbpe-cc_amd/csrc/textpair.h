// Text pairs joined into one document each (textpair.hip; mbpe_textpair_plan, mbpe_textpair_tokens,
// mbpe_encoder_set_textpair): prompt + response, query + passage, sentence pairs.
//
// A call has 2 n documents; documents 2i and 2i + 1 are A and B of pair i, la and lb tokens long.  Both are truncated to
// a and b tokens so that the joined document fits spec.max_tokens, and written as
//   A' sep.. B' [end]            a + n_sep + b + (end) ids
// with a target stream beside it: target[k] = the id at k + 1 where position k predicts it, MBPE_NO_TOKEN elsewhere.
// Everything here is integer arithmetic that a host compiler builds too; the host's plan, the plan kernel and the gather
// kernel share this one statement of the rule.
#ifndef MBPE_TEXTPAIR_H
#define MBPE_TEXTPAIR_H

#include "mbpe.h"

#include "span.h"

namespace mbpe {

constexpr uint32_t kTpLongestFirst = 0, kTpOnlyFirst = 1, kTpOnlySecond = 2;     // spec.truncation
constexpr uint32_t kTpLabelAll = 0, kTpLabelSecond = 1;                          // spec.label_mode
constexpr uint32_t kTpMaxId = 0x7FFFFFFEu;                                       // sep and end ids lie below it

// the tokens kept of A and of B
struct TpKeep {
    unsigned long long a, b;
};

// ids a joined pair has beside its text: the separators and the end id
MBPE_HD uint32_t textpair_extra(const mbpe_textpair_spec &s) { return s.n_sep + (s.end_id != MBPE_NO_TOKEN ? 1u : 0u); }

// min(x, y) and the truncation of one side given what the other keeps
MBPE_HD unsigned long long tp_min(unsigned long long x, unsigned long long y) { return x < y ? x : y; }

// what is kept of a pair of la and lb tokens (both below 2^40; max_tokens >= textpair_extra or 0: textpair_check_spec)
MBPE_HD TpKeep textpair_keep(const mbpe_textpair_spec &s, unsigned long long la, unsigned long long lb) {
    if (s.max_tokens == 0) return {la, lb};
    const unsigned long long K = s.max_tokens - textpair_extra(s);
    if (s.truncation == kTpOnlyFirst) {
        const unsigned long long b = tp_min(lb, K);
        return {tp_min(la, K - b), b};
    }
    if (s.truncation == kTpOnlySecond) {
        const unsigned long long a = tp_min(la, K);
        return {a, tp_min(lb, K - a)};
    }
    // LONGEST_FIRST: "while a + b > K drop one token from the longer side, on a tie from B", in closed form
    if (la + lb <= K) return {la, lb};
    if (la <= lb && 2 * la <= K) return {la, K - la};
    if (la > lb && 2 * lb <= K) return {K - lb, lb};
    return {(K + 1) / 2, K / 2};
}

MBPE_HD unsigned long long textpair_len(const mbpe_textpair_spec &s, const TpKeep &k) { return k.a + k.b + textpair_extra(s); }

// does position k of a joined pair (n ids, a of them A') carry a target, i.e. the id at k + 1?
MBPE_HD bool textpair_predicts(const mbpe_textpair_spec &s, unsigned long long a, unsigned long long n, unsigned long long k) {
    return k + 1 < n && (s.label_mode == kTpLabelAll || k + 1 >= a + s.n_sep);
}

// the rules of a spec for tokens of token_bits bits, without a word: MBPE_OK, MBPE_ERR_ARG or MBPE_ERR_VOCAB, *msg says why
inline int textpair_check_spec(const mbpe_textpair_spec *s, uint32_t token_bits, const char **msg) {
    *msg = "";
    if (!s) { *msg = "NULL textpair spec"; return MBPE_ERR_ARG; }
    if (s->truncation > kTpOnlySecond || s->label_mode > kTpLabelSecond || s->keep_tail_a > 1 || s->keep_tail_b > 1) {
        *msg = "a textpair enum out of range";
        return MBPE_ERR_ARG;
    }
    if (s->n_sep > 2) { *msg = "textpair n_sep above 2"; return MBPE_ERR_ARG; }
    if (s->max_tokens != 0 && s->max_tokens < textpair_extra(*s)) {
        *msg = "textpair max_tokens has no room for the separators and the end id";
        return MBPE_ERR_ARG;
    }
    const bool end = s->end_id != MBPE_NO_TOKEN;
    uint32_t top = end ? s->end_id : 0u;
    for (uint32_t i = 0; i < s->n_sep; ++i) top = s->sep_id[i] > top ? s->sep_id[i] : top;
    if (top >= kTpMaxId) { *msg = "a textpair sep or end id of 2^31 - 2 or more"; return MBPE_ERR_ARG; }
    if (token_bits == 16 && top >= 65536u) { *msg = "a textpair sep or end id that does not fit 16-bit tokens"; return MBPE_ERR_VOCAB; }
    return MBPE_OK;
}

// the host's plan of n_docs = 2 n documents with token offsets off[0 .. n_docs]: off_out (n + 1) and, where given,
// kept_out (a, b per pair)
inline void textpair_plan_host(const uint64_t *off, uint64_t n_docs, const mbpe_textpair_spec &s, uint64_t *off_out,
                               uint64_t *kept_out) {
    uint64_t o = 0;
    for (uint64_t i = 0; i < n_docs / 2; ++i) {
        const TpKeep k = textpair_keep(s, off[2 * i + 1] - off[2 * i], off[2 * i + 2] - off[2 * i + 1]);
        off_out[i] = o;
        o += textpair_len(s, k);
        if (kept_out) { kept_out[2 * i] = k.a; kept_out[2 * i + 1] = k.b; }
    }
    off_out[n_docs / 2] = o;
}

#ifdef __HIPCC__
// ---- the device stage (textpair.hip) ----------------------------------------------------------------------------------
// What it leaves on the device for n > 0 pairs: off = the joined documents' token offsets (n + 1; off[n] the joined
// token count), behind them the scan's scratch; kept = a, b per pair; tok = the joined stream, plain ids of `bits`;
// tgt = its targets (NULL: none are written).
uint64_t textpair_off_bytes(uint64_t n_pairs);
struct TextpairDst {
    void *tok;
    uint32_t *tgt;
    uint64_t cap;                            // ids tok (and tgt) holds; the kernel writes no more than these
    unsigned long long *off;                 // textpair_off_bytes(n_pairs)
    unsigned long long *kept;                // 2 * n_pairs
};

// k_textpair_plan, the scan, k_textpair_offsets and k_textpair_gather on `stream` over tok (`bits` bits: 16 plain ids,
// 32 with bit 31 ignored) and doc_off (2 n_pairs + 1, device).  n_pairs > 0.  Nothing is waited for and nothing comes
// back: the joined token count is the word at dst.off + n_pairs
void textpair_launch(hipStream_t stream, const void *tok, uint32_t bits, const unsigned long long *doc_off, uint64_t n_pairs,
                     const mbpe_textpair_spec &spec, const TextpairDst &dst);
#endif

}  // namespace mbpe

#endif
