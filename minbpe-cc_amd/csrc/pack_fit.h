// The host planner of best-fit packing (mbpe_pack_fit, include/mbpe.h): whole documents, many per row, none cut unless
// it is longer than a row.  Plain C++ without a HIP include, like pack_host.h, so that a host compiler builds it alone
// (tests/pack_fit_check.cpp).  Nothing here touches a device.
//
// With S = seq_len and T_d = L_d + nb + ne, document d is cut into q_d = T_d / S full pieces of S elements and, where
// r_d = T_d % S > 0, one tail piece of r_d elements.  All pieces are taken by size descending, then d, then piece index
// ascending, and each goes to the open row with the smallest free >= its size (ties: the lowest row), at column
// S - free, or opens a new row.  The full pieces come first and each opens a row: rows 0 .. F - 1, F = sum q_d, are the
// full pieces in document order and are never looked at again.  Only the tails are sorted and placed: the open rows
// live in one min-heap of row numbers per value of `free`, the classes in an ordered map whose lower_bound is the
// smallest class that has room -- O(log S + log rows) per piece.
#ifndef MBPE_PACK_FIT_H
#define MBPE_PACK_FIT_H

#include "mbpe.h"

#include <algorithm>
#include <cstdint>
#include <functional>
#include <map>
#include <queue>
#include <vector>

namespace mbpe {

// elements [k0, k0 + size) of E_d in columns [col0, col0 + size) of the piece's row.  24 bytes: the kernel reads them
struct PackFitPiece {
    uint64_t d, k0;
    uint32_t col0, size;
};
static_assert(sizeof(PackFitPiece) == 24, "k_pack_fit reads 24-byte pieces");

constexpr uint64_t kPackFitMaxRows = 1ull << 40;
constexpr uint64_t kPackFitNoRow = ~0ull;

// the plan of one call; the vectors keep their capacity from call to call
struct PackFitPlan {
    uint64_t n_rows = 0;
    std::vector<PackFitPiece> pieces;        // sorted by (row, col0); every row has at least one
    std::vector<uint64_t> row_first;         // n_rows + 1: row r's pieces are [row_first[r], row_first[r + 1])
    std::vector<uint32_t> len;               // n_rows: cells used
    std::vector<uint64_t> doc_row;           // n_docs: the cell of the first element of the document's last piece
    std::vector<uint32_t> doc_col;           //         (kPackFitNoRow, 0 where T_d == 0)
    // scratch of pack_fit_plan
    std::vector<PackFitPiece> tails;
    std::vector<uint64_t> tail_row, cursor;
};

// F = the sum of q_d, or MBPE_ERR_ARG beyond 2^40 (the rows cannot be fewer).  doc_tok_off: n_docs + 1 ascending
// offsets; nbe = nb + ne; seq_len >= 1
inline int pack_fit_full_rows(const uint64_t *doc_tok_off, uint64_t n_docs, uint32_t seq_len, uint32_t nbe,
                              uint64_t *full_out, const char **msg) {
    uint64_t F = 0;
    for (uint64_t d = 0; d < n_docs; ++d) {
        const uint64_t L = doc_tok_off[d + 1] - doc_tok_off[d];
        // (L + nbe) / seq_len, where L + nbe may pass 2^64: in two parts, the second only below the limit
        uint64_t q = L / seq_len;
        if (q <= kPackFitMaxRows) q += (L % seq_len + nbe) / seq_len;
        F = q > kPackFitMaxRows ? q : F + q;                                 // (no wrap: F <= 2^40 here)
        if (F > kPackFitMaxRows) {
            *msg = "more than 2^40 rows";
            return MBPE_ERR_ARG;
        }
    }
    *full_out = F;
    return MBPE_OK;
}

// the whole plan.  MBPE_ERR_ARG beyond 2^40 rows, with the plan left in an unspecified state
inline int pack_fit_plan(const uint64_t *doc_tok_off, uint64_t n_docs, uint32_t seq_len, uint32_t nbe, PackFitPlan *p,
                         const char **msg) {
    const uint64_t S = seq_len;
    uint64_t F = 0;
    const int rc = pack_fit_full_rows(doc_tok_off, n_docs, seq_len, nbe, &F, msg);
    if (rc != MBPE_OK) return rc;
    p->n_rows = 0;
    p->pieces.clear();
    p->pieces.reserve(F + n_docs);
    p->doc_row.assign(n_docs, kPackFitNoRow);
    p->doc_col.assign(n_docs, 0);
    p->tails.clear();
    // the full pieces, and the tails in document order
    for (uint64_t d = 0; d < n_docs; ++d) {
        const uint64_t L = doc_tok_off[d + 1] - doc_tok_off[d];
        const uint64_t q = L / S + (L % S + nbe) / S;
        const uint32_t r = (uint32_t)((L % S + nbe) % S);
        for (uint64_t i = 0; i < q; ++i) p->pieces.push_back({d, i * S, 0u, seq_len});
        if (q) p->doc_row[d] = p->pieces.size() - 1;
        if (r) p->tails.push_back({d, q * S, 0u, r});
    }
    // size descending, then d ascending (a document has one tail: the piece index decides nothing)
    std::stable_sort(p->tails.begin(), p->tails.end(),
                     [](const PackFitPiece &a, const PackFitPiece &b) { return a.size > b.size; });
    typedef std::priority_queue<uint64_t, std::vector<uint64_t>, std::greater<uint64_t>> RowHeap;
    std::map<uint32_t, RowHeap> open;            // free -> the open rows that have it (0 is not kept)
    const uint64_t n_tails = p->tails.size();
    p->tail_row.resize(n_tails);
    uint64_t n_rows = F;
    for (uint64_t t = 0; t < n_tails; ++t) {
        PackFitPiece &pc = p->tails[t];
        uint64_t row;
        uint32_t free;
        auto it = open.lower_bound(pc.size);
        if (it == open.end()) {
            row = n_rows++;
            free = seq_len;
        } else {
            row = it->second.top();
            free = it->first;
            it->second.pop();
            if (it->second.empty()) open.erase(it);
        }
        pc.col0 = seq_len - free;
        p->tail_row[t] = row;
        if (free > pc.size) open[free - pc.size].push(row);
        p->doc_row[pc.d] = row;
        p->doc_col[pc.d] = pc.col0;
    }
    if (n_rows > kPackFitMaxRows) {
        *msg = "more than 2^40 rows";
        return MBPE_ERR_ARG;
    }
    p->n_rows = n_rows;
    // the table by (row, col0): a row's pieces were placed from left to right, so a counting sort by row keeps them so
    p->row_first.assign(n_rows + 1, 0);
    p->len.assign(n_rows, 0);
    for (uint64_t r = 0; r < F; ++r) p->len[r] = seq_len;
    for (uint64_t r = 0; r <= F; ++r) p->row_first[r] = r;
    for (uint64_t t = 0; t < n_tails; ++t) ++p->row_first[p->tail_row[t] + 1];
    for (uint64_t r = F; r < n_rows; ++r) p->row_first[r + 1] += p->row_first[r];
    p->pieces.resize(F + n_tails);
    p->cursor.assign(p->row_first.begin() + F, p->row_first.end() - 1);
    for (uint64_t t = 0; t < n_tails; ++t) {
        const uint64_t r = p->tail_row[t];
        const PackFitPiece &pc = p->tails[t];
        p->pieces[p->cursor[r - F]++] = pc;
        p->len[r] = pc.col0 + pc.size;
    }
    return MBPE_OK;
}

// cu_seqlens of a plan: the boundaries of the maximal runs of equal (row, seg) in the flattened matrix -- every piece
// start (no document has two pieces in one row), the start of every row's pad run, which counts as a sequence of its
// own, and n_rows * seq_len.  cu_out (or NULL: count only) has room for cap_seqs + 1 entries; a cap too small is
// MBPE_ERR_ARG with the counts filled and nothing written
inline int pack_fit_cu_seqlens(const PackFitPlan &p, uint32_t seq_len, int32_t *cu_out, uint64_t cap_seqs,
                               uint64_t *n_seqs_out, uint32_t *max_seqlen_out, const char **msg) {
    if (p.n_rows * (uint64_t)seq_len >= (1ull << 31)) {      // (n_rows <= 2^40, seq_len < 2^32: no wrap)
        *msg = "cu_seqlens of a matrix of 2^31 cells or more";
        return MBPE_ERR_ARG;
    }
    uint64_t n = p.pieces.size();
    uint32_t longest = 0;
    for (const PackFitPiece &pc : p.pieces) longest = std::max(longest, pc.size);
    for (uint64_t r = 0; r < p.n_rows; ++r)
        if (p.len[r] < seq_len) {
            ++n;
            longest = std::max(longest, seq_len - p.len[r]);
        }
    *n_seqs_out = n;
    *max_seqlen_out = longest;
    if (!cu_out) return MBPE_OK;
    if (cap_seqs < n) {
        *msg = "cu_out too small";
        return MBPE_ERR_ARG;
    }
    uint64_t at = 0;
    for (uint64_t r = 0; r < p.n_rows; ++r) {
        for (uint64_t i = p.row_first[r]; i < p.row_first[r + 1]; ++i)
            cu_out[at++] = (int32_t)(r * seq_len + p.pieces[i].col0);
        if (p.len[r] < seq_len) cu_out[at++] = (int32_t)(r * seq_len + p.len[r]);
    }
    cu_out[at] = (int32_t)(p.n_rows * seq_len);
    return MBPE_OK;
}

}  // namespace mbpe

#endif
