// Masked-LM corruption of token documents (mlm.hip; mbpe_mlm_plan, mbpe_mlm_tokens, mbpe_encoder_set_mlm).
//
// Between encode and pack every token of a document is either left alone or SELECTED; a selected token becomes a
// target (its old id goes to a second, uint32 stream) and is replaced by mask_id, by a random id below vocab_n, or
// kept (Devlin et al., 2019).  With whole_word the selection is drawn per word -- the tokens of one chunk of the
// encoder's split, whose last token carries bit 31 in a 32-bit stream -- so a word is masked as a whole.  Every draw
// is dropout.h's hash over (s_g, index in the document, draw number), s_g a 64-bit seed of the document made of two
// draws over (seed, g), g = the document's number in the caller's corpus.  The mask so belongs to the token in its
// document, not to a cell of a matrix: one seed gives one masked corpus however it is packed or cut into batches.
// Everything here is integer arithmetic that a host compiler builds too (tests/mlm_check.cpp runs it); the host's
// plan and the apply kernel share this one statement of the rule.
#ifndef MBPE_MLM_H
#define MBPE_MLM_H

#include "mbpe.h"

#include "dropout.h"

namespace mbpe {

constexpr uint32_t kMlmDrawHi = 0x4D4C4D00u, kMlmDrawLo = 0x4D4C4D01u;   // the two draws of s_g ("MLM", 0 and 1)
constexpr uint32_t kMlmMaxId = 0x7FFFFFFEu;                              // mask_id and vocab_n lie below it
constexpr uint32_t kMlmMaxProtect = 8;

// s_g of document d of the call
MBPE_HD unsigned long long mlm_doc_seed(const mbpe_mlm_spec &s, unsigned long long d) {
    const unsigned long long g = s.doc_base + d;
    return ((unsigned long long)drop_hash(s.seed, g, kMlmDrawHi) << 32) | drop_hash(s.seed, g, kMlmDrawLo);
}

MBPE_HD bool mlm_protected(const mbpe_mlm_spec &s, uint32_t id) {
    for (uint32_t i = 0; i < kMlmMaxProtect; ++i)
        if (i < s.n_protect && s.protect[i] == id) return true;
    return false;
}

// token k of a document with seed sg, whose word starts at token w <= k (w == k without whole_word), plain id `id`:
// the new id; *target = the old id where the token is selected, else MBPE_NO_TOKEN
MBPE_HD uint32_t mlm_token(const mbpe_mlm_spec &s, unsigned long long sg, unsigned long long k, unsigned long long w,
                           uint32_t id, uint32_t *target) {
    *target = MBPE_NO_TOKEN;
    if ((unsigned long long)drop_hash(sg, w, 0u) >= s.select) return id;
    if (mlm_protected(s, id)) return id;
    *target = id;
    const unsigned long long r = drop_hash(sg, k, 1u);
    if (r < s.mask) return s.mask_id;
    if (r < s.mask + s.random) return (uint32_t)(((unsigned long long)drop_hash(sg, k, 2u) * s.vocab_n) >> 32);
    return id;
}

// the rules of a spec for tokens of token_bits bits, without a word: MBPE_OK, MBPE_ERR_ARG or MBPE_ERR_VOCAB, *msg says why
inline int mlm_check_spec(const mbpe_mlm_spec *s, uint32_t token_bits, const char **msg) {
    *msg = "";
    if (!s) { *msg = "NULL mlm spec"; return MBPE_ERR_ARG; }
    if (s->select > kDropoutOne || s->mask > kDropoutOne || s->random > kDropoutOne) {
        *msg = "an mlm threshold above 2^32";
        return MBPE_ERR_ARG;
    }
    if (s->mask + s->random > kDropoutOne) { *msg = "mlm mask and random together exceed 2^32"; return MBPE_ERR_ARG; }
    if (s->random > 0 && s->vocab_n == 0) { *msg = "mlm random ids with vocab_n 0"; return MBPE_ERR_ARG; }
    if (s->n_protect > kMlmMaxProtect) { *msg = "more than 8 protected ids"; return MBPE_ERR_ARG; }
    if (s->whole_word > 1u) { *msg = "whole_word must be 0 or 1"; return MBPE_ERR_ARG; }
    if (s->mask_id >= kMlmMaxId || s->vocab_n >= kMlmMaxId) {
        *msg = "an mlm mask_id or vocab_n of 2^31 - 2 or more";
        return MBPE_ERR_ARG;
    }
    if (token_bits == 16 && s->whole_word) {
        *msg = "whole_word needs 32-bit tokens: 16-bit tokens carry no word ends";
        return MBPE_ERR_ARG;
    }
    if (token_bits == 16 && (s->mask_id >= 65536u || s->vocab_n > 65536u)) {
        *msg = "an mlm mask_id or vocab_n that does not fit 16-bit tokens";
        return MBPE_ERR_VOCAB;
    }
    return MBPE_OK;
}

// the host's rule over n_docs documents with token offsets off[0 .. n_docs] of tok (bits 16: plain ids; 32: bit 31 =
// last token of its word): tok_out (plain ids of the same width) and tgt_out (uint32), each off[n_docs] entries or NULL
inline void mlm_plan_host(const void *tok, uint32_t bits, const uint64_t *off, uint64_t n_docs, const mbpe_mlm_spec &s,
                          void *tok_out, uint32_t *tgt_out) {
    for (uint64_t d = 0; d < n_docs; ++d) {
        const unsigned long long sg = mlm_doc_seed(s, d);
        unsigned long long w = 0;
        for (uint64_t i = off[d]; i < off[d + 1]; ++i) {
            const unsigned long long k = i - off[d];
            const uint32_t raw = bits == 16 ? static_cast<const uint16_t *>(tok)[i] : static_cast<const uint32_t *>(tok)[i];
            const uint32_t id = bits == 16 ? raw : raw & kTokIdMask;
            if (!s.whole_word || k == 0 || (static_cast<const uint32_t *>(tok)[i - 1] & kTokEnd)) w = k;
            uint32_t tgt;
            const uint32_t v = mlm_token(s, sg, k, w, id, &tgt);
            if (tok_out) {
                if (bits == 16) static_cast<uint16_t *>(tok_out)[i] = (uint16_t)v;
                else static_cast<uint32_t *>(tok_out)[i] = v;
            }
            if (tgt_out) tgt_out[i] = tgt;
        }
    }
}

#ifdef __HIPCC__
// ---- the device stage (mlm.hip) ---------------------------------------------------------------------------------------
// What it needs beside the streams: with whole_word one word per span of 1,024 tokens
uint64_t mlm_scratch_bytes(uint64_t n_tokens);
struct MlmDst {
    void *tok;                               // n_tokens plain ids of `bits`
    uint32_t *tgt;                           // n_tokens, or NULL
    unsigned long long *scratch;             // mlm_scratch_bytes(n_tokens); read and written with whole_word only
};

// k_mlm_apply on `stream` over tok (n_tokens > 0 of `bits` bits) and doc_off (n_docs + 1, device; from 0 to n_tokens);
// with whole_word k_mlm_starts and k_mlm_scan before it.  Nothing is waited for
void mlm_launch(hipStream_t stream, const void *tok, uint64_t n_tokens, uint32_t bits, const unsigned long long *doc_off,
                uint64_t n_docs, const mbpe_mlm_spec &spec, const MlmDst &dst);
#endif

}  // namespace mbpe

#endif
