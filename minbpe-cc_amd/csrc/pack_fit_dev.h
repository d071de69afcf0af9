// The device planner of best-fit packing (option "fit_planner", mbpe_pack_fit_plan_device): what pack_fit_plan
// (pack_fit.h) computes -- n_rows, the piece table by (row, col0), row_first, len, doc_row, doc_col -- from document
// offsets that lie in device memory, into the buffers k_pack_fit reads.  pack_fit.h stays the rule's executable form;
// pack_fit_dev.hip evaluates the same rule one size class at a time (DESIGN.md 4p has the argument).
#ifndef MBPE_PACK_FIT_DEV_H
#define MBPE_PACK_FIT_DEV_H

#include "hip_host.h"
#include "pack_fit.h"

namespace mbpe {

// q_d and r_d of a document of L tokens (L < 2^40: no part can wrap), the two-part division of pack_fit_full_rows
struct FitQR { unsigned long long q; uint32_t r; };
#ifdef __HIPCC__
__host__ __device__
#endif
inline FitQR pack_fit_qr(unsigned long long L, uint32_t seq_len, uint32_t nbe) {
    const unsigned long long part = L % seq_len + nbe;
    return {L / seq_len + part / seq_len, (uint32_t)(part % seq_len)};
}

// what the planner keeps from call to call: one workspace sized by (n_docs, seq_len) alone, so that a repeat call of
// no larger size allocates nothing, and len (n_rows entries, only for a caller that asks)
struct PackFitDev {
    DevBuf<uint8_t> ws;
    DevBuf<uint32_t> d_len;
    unsigned long long *doc_row = nullptr;   // [n_docs], inside ws: valid after a plan
    uint32_t *doc_col = nullptr;             // [n_docs]
    uint64_t stats[4] = {0, 0, 0, 0};        // mbpe_encoder_fit_stats: planner, tails, non-empty classes, rows sorted
};

// the limits of the device planner (mbpe.h, MBPE_FIT_DEVICE_MAX_SEQ); beyond them the host planner runs
inline bool pack_fit_dev_serves(uint64_t n_docs, uint32_t seq_len) {
    return seq_len <= MBPE_FIT_DEVICE_MAX_SEQ && n_docs < 0xFFFFFFFFull;
}

// The plan of n_docs documents whose n_docs + 1 token offsets lie at d_doc_off, on `stream`.  Reserves and fills
// *d_pieces (24 B per piece) and *d_rows (row_first, n_rows + 1 entries), w->doc_row / doc_col and, with want_len,
// w->d_len.  One readback of 64 bytes (the full rows, the tails and the new rows) sizes those buffers.  *served false
// (nothing written, MBPE_OK): 2^32 rows or more, the caller runs the host planner.  Everything has run on return.
int pack_fit_dev_plan(hipStream_t stream, DevAlloc &mem, PackFitDev *w, const unsigned long long *d_doc_off,
                      uint64_t n_docs, uint32_t seq_len, uint32_t nbe, bool want_len, DevBuf<uint8_t> *d_pieces,
                      DevBuf<unsigned long long> *d_rows, uint64_t *n_rows_out, bool *served);

}  // namespace mbpe

#endif
