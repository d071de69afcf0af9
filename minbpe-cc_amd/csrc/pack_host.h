// The host arithmetic of the training-batch outputs of pack.hip (labels, positions, segments, cu_seqlens): the range
// of ignore_label, the limits of the 32-bit outputs, and the cu_seqlens merge over the host's document offsets.
// Plain C++ without a HIP include, so that a host compiler builds it alone (tests/pack_check.cpp).  Every function
// returns an mbpe_status and, on an error, a static text in *msg; nothing here touches a device.  The arithmetic of
// the overlapping windows (mbpe_pack_windows) is here too: what the kernels of pack.hip and the host share is marked
// MBPE_HD (span.h), and tests/pack_window_check.cpp runs it.
#ifndef MBPE_PACK_HOST_H
#define MBPE_PACK_HOST_H

#include "mbpe.h"
#include "span.h"

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

// ---- overlapping windows (mbpe_pack_windows) -------------------------------------------------------------------------
// A document of L tokens that does not fit keep = seq_len - nb - ne body tokens becomes W rows of its own; window i
// holds tok[a .. b) with a = i * step, b = min(a + keep, L), step = keep - stride, and is the last one iff a + keep >= L
// (which for L > keep is i == ceil((L - keep) / step): the last window always brings a token no earlier one held).
MBPE_HD uint64_t pack_win_count(uint64_t L, uint32_t keep, uint32_t step) {
    return L <= keep ? 1ull : 1ull + (L - keep + step - 1) / step;
}

// window i of a document of L tokens: its body tok[a .. a + body), and whether it is the document's last
struct PackWinRow {
    uint64_t a;
    uint32_t body, last;
};
MBPE_HD PackWinRow pack_win_row(uint64_t L, uint64_t i, uint32_t keep, uint32_t step) {
    PackWinRow r;
    r.a = i * step;
    r.last = r.a + keep >= L;
    r.body = r.last ? (uint32_t)(L - r.a) : keep;
    return r;
}

constexpr uint64_t kPackWinMaxRows = 1ull << 40;

// the argument rules of the window calls that need no offsets: the spec is PADDED without pad_left / trunc_left and
// has room for one body token, stride < keep, score_once is 0 or 1, row_doc holds d in 32 bits
inline int pack_win_check(const mbpe_pack_spec &spec, const mbpe_pack_window *win, uint64_t n_docs, const char **msg) {
    if (!win) {
        *msg = "NULL pack window";
        return MBPE_ERR_ARG;
    }
    if (spec.layout != MBPE_PACK_PADDED || spec.pad_left || spec.trunc_left) {
        *msg = "windows go with MBPE_PACK_PADDED, pad_left 0 and trunc_left 0 only";
        return MBPE_ERR_ARG;
    }
    const uint32_t nbe = (spec.bos_id != MBPE_NO_TOKEN) + (spec.eos_id != MBPE_NO_TOKEN);
    if (spec.seq_len < nbe + 1) {
        *msg = "seq_len has no room for bos, eos and one token";
        return MBPE_ERR_ARG;
    }
    if (win->stride >= spec.seq_len - nbe) {
        *msg = "stride must be below seq_len - nb - ne";
        return MBPE_ERR_ARG;
    }
    if (win->score_once > 1) {
        *msg = "score_once must be 0 or 1";
        return MBPE_ERR_ARG;
    }
    if (win->row_doc && n_docs >= 0xFFFFFFFFull) {
        *msg = "row_doc with 2^32 - 1 documents or more";
        return MBPE_ERR_ARG;
    }
    return MBPE_OK;
}

// n_rows = the sum of W_d over the host's document offsets (the spec and the window have passed pack_win_check); more
// than 2^40 rows is MBPE_ERR_ARG with *n_rows_out left alone
inline int pack_win_rows(const uint64_t *doc_tok_off, uint64_t n_docs, uint32_t keep, uint32_t stride, uint64_t *n_rows_out,
                         const char **msg) {
    uint64_t n = 0;
    for (uint64_t d = 0; d < n_docs; ++d) {
        const uint64_t w = pack_win_count(doc_tok_off[d + 1] - doc_tok_off[d], keep, keep - stride);
        n = w > kPackWinMaxRows ? w : n + w;                     // (no wrap: n <= 2^40 here)
        if (n > kPackWinMaxRows) {
            *msg = "more than 2^40 rows";
            return MBPE_ERR_ARG;
        }
    }
    *n_rows_out = n;
    return MBPE_OK;
}

// the document and the window of a row < n_rows: the largest d with row_start[d] <= row (every document has a window,
// so row_start -- the exclusive prefix sum of W_d, n_docs + 1 entries, the last one n_rows -- ascends strictly), then
// i = row - row_start[d].  Every document has at least one row, before the row and behind it: d <= row, and
// n_docs - 1 - d <= n_rows - 1 - row.  The search starts from these bounds, so where every document is one row it
// probes nothing, and otherwise never more than log2 of the rows beyond one per document
MBPE_HD uint64_t pack_win_doc(const unsigned long long *row_start, uint64_t n_docs, uint64_t n_rows, uint64_t row) {
    const uint64_t behind = n_rows - row;                        // rows from this one on: at least as many documents
    uint64_t d = n_docs > behind ? n_docs - behind : 0;          // row_start[d] <= row < row_start[hi]
    uint64_t hi = row + 1 < n_docs ? row + 1 : n_docs;
    while (hi - d > 1) {
        const uint64_t mid = d + (hi - d) / 2;
        if (row_start[mid] <= row) d = mid;
        else hi = mid;
    }
    return d;
}

}  // namespace mbpe

#endif
