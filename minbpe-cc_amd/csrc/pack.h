// Packing a ragged token stream into fixed-length id matrices, and back (pack.hip): what the C-ABI entry points and
// the encoder's batch call (encode.hip) share.  The views name device memory; the checks touch no device.
#ifndef MBPE_PACK_H
#define MBPE_PACK_H

#include "mbpe.h"

#include <hip/hip_runtime.h>

namespace mbpe {

// the documents: n_tokens tokens of `bits` bits (16: plain ids; 32: bit 31 is ignored) and n_docs + 1 token offsets.
// label_tok: NULL for next-token labels, else n_tokens targets (mlm.h) that k_pack_aux, k_pack_windows and k_pack_fit
// write as labels: a body cell gets its token's entry, ignore_label where that is MBPE_NO_TOKEN and in every other cell
struct PackSrc {
    const void *tok;
    const unsigned long long *doc_off;
    uint64_t n_docs, n_tokens;
    uint32_t bits;
    const uint32_t *label_tok = nullptr;
};

// the matrix: n_rows x seq_len ids of the spec's out_bits, and (optional) one length per row
struct PackDst {
    void *ids;
    uint32_t *len;
    uint64_t n_rows;
};

// the rules of mbpe_pack_tokens for a spec and the width of the tokens it will read: MBPE_OK, or MBPE_ERR_ARG /
// MBPE_ERR_VOCAB with the last error set
int pack_check_spec(const mbpe_pack_spec *spec, uint32_t token_bits);

// rows of the matrix that n_tokens tokens in n_docs documents fill (the spec has passed pack_check_spec)
uint64_t pack_rows(const mbpe_pack_spec &spec, uint64_t n_tokens, uint64_t n_docs);

// one kernel on `stream`; dst.n_rows == pack_rows(...) > 0.  Nothing is waited for
void pack_launch(hipStream_t stream, const PackSrc &src, const mbpe_pack_spec &spec, const PackDst &dst);

// the rules of mbpe_pack_tokens_aux for its aux argument, before any device call: aux itself, the range of
// ignore_label for the spec's out_bits, the document count when seg is asked for and -- where doc_tok_off is given,
// PACKED -- the document lengths when pos is; with out_on_device the 16-byte alignment of ids_out and of every aux
// output.  MBPE_OK, or MBPE_ERR_ARG / MBPE_ERR_VOCAB with the last error set
int pack_check_aux(const mbpe_pack_spec &spec, const mbpe_pack_aux *aux, const uint64_t *doc_tok_off, uint64_t n_docs,
                   const void *ids_out, int out_on_device);

// the same matrix from k_pack_aux, which also writes whichever of aux's labels / pos / seg (device memory, 16-byte
// aligned like dst.ids) are not NULL
void pack_launch_aux(hipStream_t stream, const PackSrc &src, const mbpe_pack_spec &spec, const PackDst &dst,
                     const mbpe_pack_aux &aux);

// ---- overlapping windows (mbpe_pack_windows; the arithmetic is in pack_host.h) -----------------------------------------

// the rules of the window calls that need neither offsets nor a device: pack_check_spec, the window's own rules
// (pack_win_check), pack_check_aux, and with out_on_device the alignment of row_doc (4) and row_tok0 (8).  MBPE_OK, or
// MBPE_ERR_ARG / MBPE_ERR_VOCAB with the last error set
int pack_check_windows(const mbpe_pack_spec *spec, uint32_t token_bits, const mbpe_pack_aux *aux,
                       const mbpe_pack_window *win, uint64_t n_docs, const void *ids_out, int out_on_device);

// n_rows of the host's document offsets: MBPE_OK, or MBPE_ERR_ARG (more than 2^40 rows) with the last error set
int pack_window_rows(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec &spec, const mbpe_pack_window &win,
                     uint64_t *n_rows_out);

// k_win_rows, the scan and k_win_offsets on `stream`: row_start (device, pack_win_scratch_bytes(n_docs): n_docs + 1
// entries and, behind them, one per span of 1,024 documents) becomes the exclusive prefix sum of W_d over the device's
// document offsets, row_start[n_docs] the row count.  n_docs > 0.  Nothing is waited for
uint64_t pack_win_scratch_bytes(uint64_t n_docs);
void pack_launch_win_rows(hipStream_t stream, const unsigned long long *doc_off, uint64_t n_docs,
                          const mbpe_pack_spec &spec, const mbpe_pack_window &win, unsigned long long *row_start);

// k_pack_windows on `stream`: dst.n_rows == row_start[n_docs] > 0; aux's and win's pointers name device memory (ids,
// labels, pos and seg 16-byte aligned) or are NULL
void pack_launch_windows(hipStream_t stream, const PackSrc &src, const mbpe_pack_spec &spec, const PackDst &dst,
                         const mbpe_pack_aux &aux, const mbpe_pack_window &win, const unsigned long long *row_start);

// ---- best-fit packing (mbpe_pack_fit; the planner is in pack_fit.h) -------------------------------------------------------

struct PackFitPlan;

// the rules of the fit calls that need neither offsets nor a device: pack_check_spec, the layout (MBPE_PACK_PACKED),
// fit itself, pack_check_aux, and with out_on_device the alignment of doc_row (8) and doc_col (4).  MBPE_OK, or
// MBPE_ERR_ARG / MBPE_ERR_VOCAB with the last error set
int pack_check_fit(const mbpe_pack_spec *spec, uint32_t token_bits, const mbpe_pack_aux *aux, const struct mbpe_pack_fit *fit,
                   uint64_t n_docs, const void *ids_out, int out_on_device);

// the plan of the host's document offsets: MBPE_OK, or MBPE_ERR_ARG (more than 2^40 rows) with the last error set
int pack_fit_make(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec &spec, PackFitPlan *plan);

// what a plan puts on the device beside row_first ((n_rows + 1) * 8 bytes): its piece table
uint64_t pack_fit_piece_bytes(const PackFitPlan &plan);

// k_pack_fit on `stream`: dst.n_rows == plan.n_rows > 0; pieces and row_first are the plan's, in device memory; aux's
// pointers name device memory (ids, labels, pos and seg 16-byte aligned) or are NULL.  Nothing is waited for
void pack_launch_fit(hipStream_t stream, const PackSrc &src, const mbpe_pack_spec &spec, const PackDst &dst,
                     const mbpe_pack_aux &aux, const void *pieces, const unsigned long long *row_first);

// the plan's doc_row / doc_col to where fit asks for them: host memory, or device memory through `stream`, which is
// waited for
int pack_fit_doc_out(hipStream_t stream, const struct mbpe_pack_fit &fit, const PackFitPlan &plan, int out_on_device);

}  // namespace mbpe

#endif
