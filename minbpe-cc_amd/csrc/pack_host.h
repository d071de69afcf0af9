// The host arithmetic of the training-batch outputs of pack.hip (labels, positions, segments, cu_seqlens): the range
// of ignore_label, the limits of the 32-bit outputs, and the cu_seqlens merge over the host's document offsets.
// Plain C++ without a HIP include, so that a host compiler builds it alone (tests/pack_check.cpp).  Every function
// returns an mbpe_status and, on an error, a static text in *msg; nothing here touches a device.
#ifndef MBPE_PACK_HOST_H
#define MBPE_PACK_HOST_H

#include "mbpe.h"

#include <cstdint>

namespace mbpe {

// ignore_label is written truncated to out_bits: 16 bits hold 0 .. 65,535 (ids are unsigned there), 32 bits whatever
// an int32_t or a uint32_t holds, 64 bits every int64_t
inline int pack_check_ignore(uint32_t out_bits, int64_t ignore_label, const char **msg) {
    if (out_bits == 16 && (ignore_label < 0 || ignore_label > 65535)) {
        *msg = "out_bits 16 with an ignore_label outside 0 .. 65,535";
        return MBPE_ERR_VOCAB;
    }
    if (out_bits == 32 && (ignore_label < -2147483648ll || ignore_label > 4294967295ll)) {
        *msg = "out_bits 32 with an ignore_label outside -2^31 .. 2^32 - 1";
        return MBPE_ERR_ARG;
    }
    return MBPE_OK;
}

// seg holds d + 1 in 32 bits, 0 being the pad cell
inline int pack_check_seg_docs(uint64_t n_docs, const char **msg) {
    if (n_docs >= 0xFFFFFFFFull) {
        *msg = "seg with 2^32 - 1 documents or more";
        return MBPE_ERR_ARG;
    }
    return MBPE_OK;
}

// pos holds k < T_d in 32 bits; PACKED only (a PADDED row has at most seq_len elements).  nbe = nb + ne
inline int pack_check_pos_docs(const uint64_t *doc_tok_off, uint64_t n_docs, uint32_t nbe, const char **msg) {
    for (uint64_t d = 0; d < n_docs; ++d)
        if (doc_tok_off[d + 1] - doc_tok_off[d] + nbe > 0xFFFFFFFFull) {
            *msg = "pos with a document of 2^32 elements or more";
            return MBPE_ERR_ARG;
        }
    return MBPE_OK;
}

// cu_seqlens of the PACKED layout: the ascending, duplicate-free list of the row starts r * seq_len < n_stream, the
// document starts doc_tok_off[d] + d * nbe and n_stream itself -- the boundaries of the maximal runs of cells with
// equal (row, seg).  cu_out (or NULL: count only) has room for cap_seqs + 1 entries; a cap too small is MBPE_ERR_ARG
// with the counts filled and nothing written.  doc_tok_off: n_docs + 1 ascending offsets from 0.
inline int pack_cu_seqlens(const uint64_t *doc_tok_off, uint64_t n_docs, uint32_t seq_len, uint32_t nbe, int32_t *cu_out,
                           uint64_t cap_seqs, uint64_t *n_seqs_out, uint32_t *max_seqlen_out, const char **msg) {
    const uint64_t n_tokens = n_docs ? doc_tok_off[n_docs] : 0;
    if (n_tokens >= (1ull << 31) || n_docs >= (1ull << 31) || n_tokens + n_docs * nbe >= (1ull << 31)) {
        *msg = "cu_seqlens of a stream of 2^31 elements or more";
        return MBPE_ERR_ARG;
    }
    const uint64_t n_stream = n_tokens + n_docs * nbe;
    // two passes over the same merge: the count, then (when it fits) the entries
    for (int pass = 0; pass < 2; ++pass) {
        int32_t *out = pass ? cu_out : nullptr;
        uint64_t n = 0, last = 0, longest = 0, row = 0;     // entries so far, the latest one, the next row start
        auto emit = [&](uint64_t x) {
            if (n && x == last) return;
            if (n && x - last > longest) longest = x - last;
            if (out) out[n] = (int32_t)x;
            last = x;
            ++n;
        };
        for (uint64_t d = 0; d <= n_docs; ++d) {            // (d == n_docs: n_stream)
            const uint64_t b = d < n_docs ? doc_tok_off[d] + d * nbe : n_stream;
            for (; row < b; row += seq_len) emit(row);      // (row < b <= n_stream)
            emit(b);
        }
        if (pass == 0) {
            *n_seqs_out = n - 1;
            *max_seqlen_out = (uint32_t)longest;
            if (!cu_out) return MBPE_OK;
            if (cap_seqs < n - 1) {
                *msg = "cu_out too small";
                return MBPE_ERR_ARG;
            }
        }
    }
    return MBPE_OK;
}

}  // namespace mbpe

#endif
