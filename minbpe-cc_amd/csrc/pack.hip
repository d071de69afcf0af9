// Ragged token streams <-> fixed-length id matrices on the device: what stands between mbpe_encoder_encode's flat
// tokens with per-document offsets and a model input of [rows, seq_len] ids plus one length per row.
//
//   MBPE_PACK_PADDED   one row per document: [bos] body [eos], pad_id up to seq_len (on the right, or on the left);
//                      body = the document's first (or last) seq_len - nb - ne tokens
//   MBPE_PACK_PACKED   the stream S = [bos] doc [eos] over all documents, cut row-major into rows of seq_len; pad_id
//                      behind its end
//   unpack             a right-padded PADDED matrix and its lengths -> the flat tokens mbpe_decode_batch reads
//   windows            PADDED rows, but a document that does not fit becomes several rows of its own that share `stride`
//                      tokens (mbpe_pack_windows; k_win_rows .. k_pack_windows below, after k_pack_aux)
//   fit                whole documents, many per row, placed by best fit on the host (mbpe_pack_fit; k_pack_fit below,
//                      after k_pack_windows)
//
// All three are OUTPUT-centric like decode.hip's copy: the output, whose rows follow each other without a gap, is cut
// at the 16-byte boundaries of its global address and a lane owns one such piece -- 8, 4 or 2 ids of 16, 32 or 64 bits.
// It finds where its first id comes from, walks on from there (the next column, row or document), gathers the source
// tokens with loads of the token's own width (a document starts at any offset) and stores the piece as one dwordx4.
// A piece may hold the end of one row and the start of the next: a seq_len that is no multiple of the piece costs no
// narrower store.  Only the first and the last piece of the whole output can be partial (an output address that is
// not 16-byte aligned, a tail shorter than a piece); those are stored id by id.
//   k_pack_padded   first id of a piece -> (row, column) by one division; a row's document offsets are read when the
//                   row is entered.  The lane that writes column 0 of a row also writes its length.
//   k_pack_stream   PACKED and unpack, which differ in where document d's token k lies (doc_off[d] + k, or
//                   d * seq_len + k in a matrix) and in what stands around it.  The first id of a piece finds its
//                   document by a binary search PER LANE over the shifted offsets doc_off[d] + d * (nb + ne), which
//                   are formed on the fly; the walk then steps over document ends (and empty documents).  The 64 lanes
//                   of a wave search neighbouring positions, so their probes fall into the same few cache lines.
// Every output index is 64-bit (row * seq_len passes 2^32).
//
// Bytes moved per output id: the id itself written once (2, 4 or 8 B), its token read once (2 or 4 B; pad ids read
// nothing), per row 16 B of offsets and 4 B of length.
#include "pack.h"

#include "hip_host.h"
#include "pack_fit.h"
#include "pack_host.h"
#include "span.h"

#include <algorithm>
#include <new>
#include <string>
#include <vector>

namespace {

using namespace mbpe;

constexpr int kPackThreads = 256;
constexpr uint32_t kPackMaxGrid = 0x7FFFFFFFu;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// what a kernel works on; nb / ne = 1 where bos / eos is set
struct PackJob {
    const void *tok;
    const unsigned long long *doc_off;       // n_docs + 1
    uint64_t n_docs;
    uint64_t n_stream;                       // k_pack_stream: ids of the stream (beyond it: pad)
    void *out;
    uint32_t *len;                           // or NULL
    uint64_t n_out;                          // ids of the output
    uint32_t seq_len, pad, bos, eos, nb, ne, keep, pad_left, trunc_left;
};

template <int IN>
__device__ __forceinline__ uint32_t pack_read(const void *__restrict__ tok, uint64_t i) {
    if (IN == 16) return static_cast<const uint16_t *>(tok)[i];
    if (IN == 32) return static_cast<const uint32_t *>(tok)[i] & kTokIdMask;
    return (uint32_t) static_cast<const unsigned long long *>(tok)[i];
}

template <int OUT> struct PackId;
template <> struct PackId<16> { typedef uint16_t type; };
template <> struct PackId<32> { typedef uint32_t type; };
template <> struct PackId<64> { typedef unsigned long long type; };

// the pieces of an output of n_out ids at address A: piece p is the bytes [B0 + 16 p, B0 + 16 p + 16) that lie in it
template <int OUT>
struct PackPieces {
    uint64_t A, E, B0, n;
    __device__ __forceinline__ PackPieces(const void *out, uint64_t n_out) {
        A = (uint64_t)(uintptr_t)out;
        E = A + n_out * (OUT / 8);
        B0 = A & ~15ull;
        n = (E - B0 + 15) >> 4;
    }
};

// cnt ids, id e in bits [OUT * e, OUT * e + OUT) of acc, to the bytes [lo, lo + cnt * OUT / 8) of piece B
template <int OUT>
__device__ __forceinline__ void pack_store(void *out, uint64_t A, uint64_t B, uint64_t lo, uint32_t cnt,
                                           unsigned __int128 acc) {
    uint8_t *base = static_cast<uint8_t *>(out);
    if (cnt == 128 / OUT) {                          // (then lo == B)
        u32x4 q;
        q.x = (uint32_t)acc;
        q.y = (uint32_t)(acc >> 32);
        q.z = (uint32_t)(acc >> 64);
        q.w = (uint32_t)(acc >> 96);
        *static_cast<u32x4 *>(__builtin_assume_aligned(base + (B - A), 16)) = q;
    } else {                                         // the first or the last piece of the output
        typename PackId<OUT>::type *dst = reinterpret_cast<typename PackId<OUT>::type *>(base + (lo - A));
        for (uint32_t e = 0; e < cnt; ++e) dst[e] = (typename PackId<OUT>::type)(acc >> (OUT * e));
    }
}

// a row of the PADDED layout: its ids are pad for columns below lead, then [bos] + body tokens from src0 + [eos]
struct PadRow {
    uint64_t src0;
    uint32_t len, lead;
};

__device__ __forceinline__ PadRow pad_row(const PackJob &j, uint64_t row) {
    const uint64_t d0 = j.doc_off[row], dl = j.doc_off[row + 1] - d0;
    const uint32_t body = dl < j.keep ? (uint32_t)dl : j.keep;
    PadRow r;
    r.src0 = d0 + (j.trunc_left ? dl - body : 0ull);
    r.len = j.nb + body + j.ne;
    r.lead = j.pad_left ? j.seq_len - r.len : 0u;
    return r;
}

template <int IN, int OUT>
__global__ __launch_bounds__(kPackThreads) void k_pack_padded(PackJob j) {
    constexpr uint32_t ob = OUT / 8;
    const PackPieces<OUT> pc(j.out, j.n_out);
    for (uint64_t p = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x; p < pc.n;
         p += (uint64_t)gridDim.x * kPackThreads) {
        const uint64_t B = pc.B0 + (p << 4);
        const uint64_t lo = B > pc.A ? B : pc.A;
        const uint64_t hi = B + 16 < pc.E ? B + 16 : pc.E;
        const uint32_t cnt = (uint32_t)(hi - lo) / ob;           // 1 .. 16 / ob
        const uint64_t f = (lo - pc.A) / ob;
        uint64_t row = f / j.seq_len;
        uint32_t col = (uint32_t)(f - row * j.seq_len);
        PadRow r = pad_row(j, row);
        unsigned __int128 acc = 0;
        for (uint32_t e = 0; e < cnt; ++e) {
            if (col == 0 && j.len) j.len[row] = r.len;
            const uint32_t k = col - r.lead;                     // wraps for a pad on the left: >= len
            uint32_t v = j.pad;
            if (col >= r.lead && k < r.len) {
                if (j.nb && k == 0) v = j.bos;
                else if (j.ne && k == r.len - 1) v = j.eos;
                else v = pack_read<IN>(j.tok, r.src0 + (k - j.nb));
            }
            acc |= (unsigned __int128)v << (OUT * e);
            if (++col == j.seq_len) {
                col = 0;
                ++row;
                if (e + 1 < cnt) r = pad_row(j, row);            // (another id of the piece: the row exists)
            }
        }
        pack_store<OUT>(j.out, pc.A, B, lo, cnt, acc);
    }
}

// where document d begins in the stream, and its ids there (bos and eos included)
__device__ __forceinline__ uint64_t stream_off(const PackJob &j, uint64_t d) {
    return j.doc_off[d] + d * (uint64_t)(j.nb + j.ne);
}

// ROWS: the source is a matrix, document d's token k is tok[d * seq_len + k], the output is the stream itself (unpack;
// nb == ne == 0, no lengths).  Otherwise PACKED: the source is flat, the output rows of seq_len with pad behind the
// stream, len[r] = ids of the stream in row r.
template <int IN, int OUT, bool ROWS>
__global__ __launch_bounds__(kPackThreads) void k_pack_stream(PackJob j) {
    constexpr uint32_t ob = OUT / 8;
    const PackPieces<OUT> pc(j.out, j.n_out);
    const uint32_t nbe = j.nb + j.ne;
    for (uint64_t p = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x; p < pc.n;
         p += (uint64_t)gridDim.x * kPackThreads) {
        const uint64_t B = pc.B0 + (p << 4);
        const uint64_t lo = B > pc.A ? B : pc.A;
        const uint64_t hi = B + 16 < pc.E ? B + 16 : pc.E;
        const uint32_t cnt = (uint32_t)(hi - lo) / ob;
        uint64_t f = (lo - pc.A) / ob;
        uint64_t row = 0;
        uint32_t col = 0;
        if (!ROWS) {
            row = f / j.seq_len;
            col = (uint32_t)(f - row * j.seq_len);
        }
        // the document that holds stream position f: the largest d with stream_off(d) <= f (empty documents without
        // bos / eos share their successor's offset and are passed over)
        uint64_t d = 0, k = 0, d0 = 0, dtot = 0;
        if (f < j.n_stream) {
            uint64_t hi_d = j.n_docs;                            // stream_off(d) <= f < stream_off(hi_d)
            while (hi_d - d > 1) {
                const uint64_t mid = d + (hi_d - d) / 2;
                if (stream_off(j, mid) <= f) d = mid;
                else hi_d = mid;
            }
            d0 = j.doc_off[d];
            dtot = j.doc_off[d + 1] - d0 + nbe;
            k = f - (d0 + d * (uint64_t)nbe);
        }
        unsigned __int128 acc = 0;
        for (uint32_t e = 0; e < cnt; ++e, ++f) {
            uint32_t v = j.pad;
            if (f < j.n_stream) {
                while (k >= dtot) {                              // ends: f < n_stream, a document with ids follows
                    ++d;
                    k = 0;
                    d0 = j.doc_off[d];
                    dtot = j.doc_off[d + 1] - d0 + nbe;
                }
                if (j.nb && k == 0) v = j.bos;
                else if (j.ne && k == dtot - 1) v = j.eos;
                else v = pack_read<IN>(j.tok, (ROWS ? d * j.seq_len : d0) + (k - j.nb));
                ++k;
            }
            if (!ROWS) {
                if (col == 0 && j.len) {
                    const uint64_t left = f < j.n_stream ? j.n_stream - f : 0ull;
                    j.len[row] = left < j.seq_len ? (uint32_t)left : j.seq_len;
                }
                if (++col == j.seq_len) { col = 0; ++row; }
            }
            acc |= (unsigned __int128)v << (OUT * e);
        }
        pack_store<OUT>(j.out, pc.A, B, lo, cnt, acc);
    }
}

// ---- the training-batch outputs ---------------------------------------------------------------------------------------
// k_pack_aux writes the ids of either layout and, from the SAME walk, whichever of three more matrices are asked for:
//   labels  the next element of the cell's document (ignore_label behind its last one and in pad cells)
//   pos     the element's index k in its document           seg   the document's number d + 1       (0 in pad cells)
// Unlike the two kernels above it cuts the matrix in CELL-index space: a lane owns the 8 consecutive cells
// [8 g, 8 g + 8) of the flattened matrix, whatever their width -- one dwordx4 of 16-bit ids, two of 32-bit ids, pos or
// seg, four of 64-bit ids -- so one (row, column) division or one binary search serves 8 cells of every output.  The
// outputs are 16-byte aligned (checked by the host), so a full group's stores are aligned and only the last group of
// the matrix can be partial; it is stored cell by cell.  For the labels the walk runs one element ahead: the element
// read as a label is kept and becomes the next cell's id, so a group reads 9 tokens at most and none across a
// document's end.  An output that is NULL is skipped by the whole wave.  Every cell index is 64-bit.
// With label_tok (the _labels calls; masked-LM targets; LT, an instantiation of its own so that the next-token kernels
// stay the code they were) nothing is read ahead: the cell of body token t gets label_tok[t], read with the id, and
// bos, eos and pad cells keep ignore_label.  k_pack_windows and k_pack_fit alike.
struct PackAuxJob {
    PackJob j;
    void *labels;                            // ids of OUT bits, or NULL
    uint32_t *pos, *seg;                     // or NULL
    unsigned long long ignore;               // ignore_label; its low OUT bits are written
    const uint32_t *label_tok;               // NULL: the labels are next elements.  Else a target per token of the flat
                                             // stream: a body cell's label is its token's entry (MBPE_NO_TOKEN: ignore)
};

constexpr uint32_t kAuxCells = 8;

// the lane's 8 values to cells [c0, c0 + cnt) of a 32-bit matrix
__device__ __forceinline__ void aux_store32(uint32_t *dst, uint64_t c0, uint32_t cnt, const uint32_t (&v)[kAuxCells]) {
    if (cnt == kAuxCells) {
        u32x4 *q = static_cast<u32x4 *>(__builtin_assume_aligned(dst + c0, 16));
        q[0] = u32x4{v[0], v[1], v[2], v[3]};
        q[1] = u32x4{v[4], v[5], v[6], v[7]};
    } else {
#pragma unroll
        for (uint32_t e = 0; e < kAuxCells; ++e)
            if (e < cnt) dst[c0 + e] = v[e];
    }
}

// the same for ids of OUT bits; a 64-bit id e has the high word `hi` where bit e of hi_mask is set, else 0
template <int OUT>
__device__ __forceinline__ void aux_store_ids(void *dst, uint64_t c0, uint32_t cnt, const uint32_t (&v)[kAuxCells],
                                              uint32_t hi_mask, uint32_t hi) {
    if (OUT == 32) {
        aux_store32(static_cast<uint32_t *>(dst), c0, cnt, v);
    } else if (OUT == 16) {
        uint16_t *d16 = static_cast<uint16_t *>(dst);
        if (cnt == kAuxCells) {
            *static_cast<u32x4 *>(__builtin_assume_aligned(d16 + c0, 16)) =
                u32x4{(v[0] & 0xFFFFu) | (v[1] << 16), (v[2] & 0xFFFFu) | (v[3] << 16), (v[4] & 0xFFFFu) | (v[5] << 16),
                      (v[6] & 0xFFFFu) | (v[7] << 16)};
        } else {
#pragma unroll
            for (uint32_t e = 0; e < kAuxCells; ++e)
                if (e < cnt) d16[c0 + e] = (uint16_t)v[e];
        }
    } else {
        unsigned long long *d64 = static_cast<unsigned long long *>(dst);
        uint32_t h[kAuxCells];
#pragma unroll
        for (uint32_t e = 0; e < kAuxCells; ++e) h[e] = (hi_mask >> e) & 1u ? hi : 0u;
        if (cnt == kAuxCells) {
            u32x4 *q = static_cast<u32x4 *>(__builtin_assume_aligned(d64 + c0, 16));
            q[0] = u32x4{v[0], h[0], v[1], h[1]};
            q[1] = u32x4{v[2], h[2], v[3], h[3]};
            q[2] = u32x4{v[4], h[4], v[5], h[5]};
            q[3] = u32x4{v[6], h[6], v[7], h[7]};
        } else {
#pragma unroll
            for (uint32_t e = 0; e < kAuxCells; ++e)
                if (e < cnt) d64[c0 + e] = ((unsigned long long)h[e] << 32) | v[e];
        }
    }
}

template <int IN, int OUT, bool PACKED, bool LT>
__global__ __launch_bounds__(kPackThreads) void k_pack_aux(PackAuxJob a) {
    const PackJob &j = a.j;
    const bool want_lab = a.labels != nullptr;
    const uint32_t nbe = j.nb + j.ne;
    const uint32_t ign_lo = (uint32_t)a.ignore, ign_hi = (uint32_t)(a.ignore >> 32);
    const uint64_t n_groups = (j.n_out + kAuxCells - 1) / kAuxCells;
    for (uint64_t g = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x; g < n_groups;
         g += (uint64_t)gridDim.x * kPackThreads) {
        const uint64_t c0 = g * kAuxCells;
        const uint32_t cnt = j.n_out - c0 < kAuxCells ? (uint32_t)(j.n_out - c0) : kAuxCells;
        uint64_t row = c0 / j.seq_len;
        uint32_t col = (uint32_t)(c0 - row * j.seq_len);
        // the document the walk stands in: number d, T elements (bos and eos included), its tokens from src0 on;
        // k = the element that the next cell inside it holds; lead = pad cells in front (PADDED with pad_left)
        uint64_t d = 0, k = 0, T = 0, src0 = 0;
        uint32_t lead = 0;
        if (PACKED) {
            if (c0 < j.n_stream) {                               // as in k_pack_stream
                uint64_t hi_d = j.n_docs;
                while (hi_d - d > 1) {
                    const uint64_t mid = d + (hi_d - d) / 2;
                    if (stream_off(j, mid) <= c0) d = mid;
                    else hi_d = mid;
                }
                src0 = j.doc_off[d];
                T = j.doc_off[d + 1] - src0 + nbe;
                k = c0 - (src0 + d * (uint64_t)nbe);
            }
        } else {
            const PadRow r = pad_row(j, row);
            d = row; T = r.len; src0 = r.src0; lead = r.lead;
        }
        auto element = [&](uint64_t i) -> uint32_t {             // element i < T of the document
            if (j.nb && i == 0) return j.bos;
            if (j.ne && i == T - 1) return j.eos;
            return pack_read<IN>(j.tok, src0 + (i - j.nb));
        };
        uint32_t id[kAuxCells], lab[kAuxCells], ps[kAuxCells], sg[kAuxCells];
        uint32_t ign_mask = 0, ahead = 0;                        // ahead: the element read as the cell before's label
        bool have_ahead = false;
#pragma unroll
        for (uint32_t e = 0; e < kAuxCells; ++e) {
            id[e] = j.pad; lab[e] = ign_lo; ps[e] = 0; sg[e] = 0;
            ign_mask |= 1u << e;
            if (e >= cnt) continue;
            bool in;
            if (PACKED) {
                const uint64_t f = c0 + e;
                in = f < j.n_stream;
                if (in) {
                    while (k >= T) {                             // ends: f < n_stream, a document with elements follows
                        ++d;
                        k = 0;
                        src0 = j.doc_off[d];
                        T = j.doc_off[d + 1] - src0 + nbe;
                    }
                }
                if (col == 0 && j.len) {
                    const uint64_t left = in ? j.n_stream - f : 0ull;
                    j.len[row] = left < j.seq_len ? (uint32_t)left : j.seq_len;
                }
            } else {
                if (col == 0 && j.len) j.len[row] = (uint32_t)T;
                k = col - lead;                                  // wraps for a pad on the left: >= T
                in = col >= lead && k < T;
            }
            if (in) {
                id[e] = have_ahead ? ahead : element(k);
                have_ahead = false;
                if (LT) {
                    if (want_lab && k >= j.nb && !(j.ne && k == T - 1)) {
                        const uint32_t v = a.label_tok[src0 + (k - j.nb)];
                        if (v != MBPE_NO_TOKEN) { lab[e] = v; ign_mask &= ~(1u << e); }
                    }
                } else if (want_lab && k + 1 < T) {
                    ahead = element(k + 1);
                    have_ahead = true;
                    lab[e] = ahead;
                    ign_mask &= ~(1u << e);
                }
                ps[e] = (uint32_t)k;
                sg[e] = (uint32_t)d + 1u;
                if (PACKED) ++k;
            }
            if (++col == j.seq_len) {
                col = 0;
                ++row;
                if (!PACKED && e + 1 < cnt) {                    // (another cell of the group: the row exists)
                    const PadRow r = pad_row(j, row);
                    d = row; T = r.len; src0 = r.src0; lead = r.lead;
                }
            }
        }
        aux_store_ids<OUT>(j.out, c0, cnt, id, 0u, 0u);
        if (want_lab) aux_store_ids<OUT>(a.labels, c0, cnt, lab, ign_mask, ign_hi);
        if (a.pos) aux_store32(a.pos, c0, cnt, ps);
        if (a.seg) aux_store32(a.seg, c0, cnt, sg);
    }
}

// ---- overlapping windows ------------------------------------------------------------------------------------------------
// A document that does not fit a row becomes several rows of its own, consecutive ones sharing `stride` body tokens
// (mbpe.h, mbpe_pack_window; the arithmetic is pack_host.h's).  Three kernels:
//   k_win_rows      one thread per document: W_d into row_start[d]; one wave per span of 1,024 documents, which also
//                   leaves the span's sum
//   k_win_scan      one workgroup: span.h's 64-bit scan over the spans' sums (per document it would walk 8 B at a
//                   stride of a slice, uncoalesced: measured at 2.8 us per 1,000 documents); the total -- the row
//                   count -- goes to row_start[n_docs]
//   k_win_offsets   the spans again: a wave prefix sum turns the counts into the exclusive prefix sum, in place
//   k_pack_windows  the matrices.  It cuts cell-index space like k_pack_aux (8 cells per lane, the same stores).  The
//                   first cell of a lane finds its row by one division and the row's document by one binary search
//                   PER LANE over row_start; the walk then steps to the next window and, behind a document's last
//                   one, to the next document.  Labels use the one-element look-ahead of k_pack_aux; the label that
//                   crosses a row end (tok[b] in the cell of tok[b - 1]) is one more read per row.
// Bytes moved per cell: what k_pack_aux moves (the id and each output written once, a token read once, twice where
// rows overlap), per row 16 B of offsets, 4 B of length and -- when asked for -- 4 B of row_doc and 8 B of row_tok0, per
// lane at most log2(n_docs) probes of 8 B that neighbouring lanes share (none where every document is one row), per
// document 16 B of offsets read and 8 B of row_start written twice and read once.
struct PackWinJob {
    PackAuxJob a;
    const unsigned long long *row_start;     // n_docs + 1
    uint32_t *row_doc;                       // or NULL
    unsigned long long *row_tok0;            // or NULL
    uint32_t stride, step, score_once;
};

__global__ __launch_bounds__(kSpanThreads) void k_win_rows(const unsigned long long *__restrict__ doc_off, uint64_t n_docs,
                                                            uint32_t keep, uint32_t step,
                                                            unsigned long long *__restrict__ row_start,
                                                            unsigned long long *__restrict__ span_cnt) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n_docs) return;
    const uint32_t lane = lane_id();
    unsigned long long s = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t d = base + (uint64_t)it * kWave + lane;
        if (d < n_docs) {
            const unsigned long long w = pack_win_count(doc_off[d + 1] - doc_off[d], keep, step);
            row_start[d] = w;
            s += w;
        }
    }
    for (int k = kWave / 2; k > 0; k >>= 1) s += __shfl_down(s, k, kWave);
    if (lane == 0) span_cnt[span] = s;
}

__global__ __launch_bounds__(kScanThreads) void k_win_scan(unsigned long long *__restrict__ span_cnt, uint64_t n_spans,
                                                            unsigned long long *__restrict__ total) {
    __shared__ unsigned long long sh[kScanThreads];
    const unsigned long long sum = span_scan_sum64(span_cnt, n_spans, sh);
    if (threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(kSpanThreads) void k_win_offsets(unsigned long long *__restrict__ row_start, uint64_t n_docs,
                                                               const unsigned long long *__restrict__ span_off) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n_docs) return;
    const uint32_t lane = lane_id();
    unsigned long long o = span_off[span];
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t d = base + (uint64_t)it * kWave + lane;
        const unsigned long long w = d < n_docs ? row_start[d] : 0ull;
        const unsigned long long incl = wave_prefix64(w, lane);
        if (d < n_docs) row_start[d] = o + incl - w;
        o += __shfl(incl, kWave - 1, kWave);
    }
}

// the row the walk stands in: window i of document d, whose L tokens begin at d0; r = its body and whether it is the
// last; T = its elements (bos and eos included)
struct WinAt {
    uint64_t d, i, d0, L;
    PackWinRow r;
    uint32_t T;
};

__device__ __forceinline__ void win_enter(const PackJob &j, uint32_t step, WinAt *w) {
    w->d0 = j.doc_off[w->d];
    w->L = j.doc_off[w->d + 1] - w->d0;
    w->r = pack_win_row(w->L, w->i, j.keep, step);
    w->T = j.nb + w->r.body + (j.ne & w->r.last);
}

template <int IN, int OUT, bool LT>
__global__ __launch_bounds__(kPackThreads) void k_pack_windows(PackWinJob wj) {
    const PackJob &j = wj.a.j;
    const bool want_lab = wj.a.labels != nullptr;
    const uint32_t ign_lo = (uint32_t)wj.a.ignore, ign_hi = (uint32_t)(wj.a.ignore >> 32);
    const uint64_t n_groups = (j.n_out + kAuxCells - 1) / kAuxCells;
    for (uint64_t g = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x; g < n_groups;
         g += (uint64_t)gridDim.x * kPackThreads) {
        const uint64_t c0 = g * kAuxCells;
        const uint32_t cnt = j.n_out - c0 < kAuxCells ? (uint32_t)(j.n_out - c0) : kAuxCells;
        uint64_t row = c0 / j.seq_len;
        uint32_t col = (uint32_t)(c0 - row * j.seq_len);
        WinAt w;
        w.d = pack_win_doc(wj.row_start, j.n_docs, j.n_out / j.seq_len, row);
        w.i = row - wj.row_start[w.d];
        win_enter(j, wj.step, &w);
        uint32_t id[kAuxCells], lab[kAuxCells], ps[kAuxCells], sg[kAuxCells];
        uint32_t ign_mask = 0, ahead = 0;                        // ahead: the token read as the cell before's label
        bool have_ahead = false;
#pragma unroll
        for (uint32_t e = 0; e < kAuxCells; ++e) {
            id[e] = j.pad; lab[e] = ign_lo; ps[e] = 0; sg[e] = 0;
            ign_mask |= 1u << e;
            if (e >= cnt) continue;
            if (col == 0) {
                if (j.len) j.len[row] = w.T;
                if (wj.row_doc) wj.row_doc[row] = (uint32_t)w.d;
                if (wj.row_tok0) wj.row_tok0[row] = w.r.a;
            }
            const uint32_t k = col, body_end = j.nb + w.r.body;  // elements [nb, body_end) are tokens
            if (k < w.T) {
                if (k >= body_end) id[e] = j.eos;
                else if (k < j.nb) id[e] = j.bos;
                else id[e] = have_ahead ? ahead : pack_read<IN>(j.tok, w.d0 + w.r.a + (k - j.nb));
                have_ahead = false;
                if (LT) {
                    if (want_lab && k >= j.nb && k < body_end && !(wj.score_once && w.i && k < j.nb + wj.stride)) {
                        const uint32_t v = wj.a.label_tok[w.d0 + w.r.a + (k - j.nb)];
                        if (v != MBPE_NO_TOKEN) { lab[e] = v; ign_mask &= ~(1u << e); }
                    }
                } else if (want_lab && k < body_end) {
                    // the target: the document's token behind this element (index nx), eos behind the last one
                    const uint64_t nx = w.r.a + (k + 1 - j.nb);
                    bool is = true;
                    uint32_t v = j.eos;
                    if (nx < w.L) {
                        v = pack_read<IN>(j.tok, w.d0 + nx);
                        if (k + 1 < body_end) { ahead = v; have_ahead = true; }
                    } else {
                        is = j.ne != 0;
                    }
                    if (wj.score_once && w.i && k < j.nb + wj.stride) is = false;
                    if (is) {
                        lab[e] = v;
                        ign_mask &= ~(1u << e);
                    }
                }
                ps[e] = k;
                sg[e] = (uint32_t)w.d + 1u;
            }
            if (++col == j.seq_len) {
                col = 0;
                ++row;
                if (e + 1 < cnt) {                               // (another cell of the group: the row exists)
                    if (w.r.last) { ++w.d; w.i = 0; }
                    else ++w.i;
                    win_enter(j, wj.step, &w);
                }
            }
        }
        aux_store_ids<OUT>(j.out, c0, cnt, id, 0u, 0u);
        if (want_lab) aux_store_ids<OUT>(wj.a.labels, c0, cnt, lab, ign_mask, ign_hi);
        if (wj.a.pos) aux_store32(wj.a.pos, c0, cnt, ps);
        if (wj.a.seg) aux_store32(wj.a.seg, c0, cnt, sg);
    }
}

// ---- best-fit packing ----------------------------------------------------------------------------------------------------
// Whole documents, many per row (mbpe.h, mbpe_pack_fit).  Where the pieces go is decided on the host (pack_fit.h); the
// kernel gets the plan: the piece table sorted by (row, column), 24 B per piece, and row_first, 8 B per row.
//   k_pack_fit      the matrices.  It cuts cell-index space like k_pack_aux (8 cells per lane, the same stores).  The
//                   first cell of a lane finds its row by one division and its piece by one binary search PER LANE
//                   over the row's slice of the table (the largest col0 <= column; the first piece of a row starts at
//                   column 0 and the pieces of a row touch, so whatever lies behind the last one is pad).  The walk
//                   then steps to the next piece, which is the next table entry also across a row end: every row has a
//                   piece.  Labels use the one-element look-ahead of k_pack_aux; it is dropped at a piece end, behind
//                   which another document begins, and the label there is read from the document itself (element
//                   k + 1 lies in the document's next piece, in another row).
// Bytes moved per cell: what k_pack_aux moves (the id and each output written once, a token read once, twice at the end
// of a piece that is not its document's last), per piece 24 B of the table and 16 B of offsets, per row 16 B of
// row_first, 24 B of its last piece and 4 B of length, per lane at most log2(pieces of its row) probes of 4 B in 24-byte
// entries that neighbouring lanes share.
struct PackFitJob {
    PackAuxJob a;
    const PackFitPiece *pieces;
    const unsigned long long *row_first;     // n_rows + 1
};

// the piece the walk stands in: table entry p, which ends before column `end`; its document has T elements, tokens from
// src0 on
struct FitAt {
    uint64_t p, d, k0, src0, T;
    uint32_t col0, end;
};

__device__ __forceinline__ void fit_enter(const PackJob &j, const PackFitPiece *__restrict__ pieces, FitAt *f) {
    const PackFitPiece pc = pieces[f->p];
    f->d = pc.d;
    f->k0 = pc.k0;
    f->col0 = pc.col0;
    f->end = pc.col0 + pc.size;                                  // (<= seq_len)
    f->src0 = j.doc_off[pc.d];
    f->T = j.doc_off[pc.d + 1] - f->src0 + j.nb + j.ne;
}

template <int IN, int OUT, bool LT>
__global__ __launch_bounds__(kPackThreads) void k_pack_fit(PackFitJob fj) {
    const PackJob &j = fj.a.j;
    const bool want_lab = fj.a.labels != nullptr;
    const uint32_t ign_lo = (uint32_t)fj.a.ignore, ign_hi = (uint32_t)(fj.a.ignore >> 32);
    const uint64_t n_groups = (j.n_out + kAuxCells - 1) / kAuxCells;
    for (uint64_t g = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x; g < n_groups;
         g += (uint64_t)gridDim.x * kPackThreads) {
        const uint64_t c0 = g * kAuxCells;
        const uint32_t cnt = j.n_out - c0 < kAuxCells ? (uint32_t)(j.n_out - c0) : kAuxCells;
        uint64_t row = c0 / j.seq_len;
        uint32_t col = (uint32_t)(c0 - row * j.seq_len);
        uint64_t row_end = fj.row_first[row + 1];                // the row's pieces are [.., row_end)
        FitAt f;
        f.p = fj.row_first[row];                                 // pieces[p].col0 <= col < pieces[hi].col0
        for (uint64_t hi = row_end; hi - f.p > 1;) {
            const uint64_t mid = f.p + (hi - f.p) / 2;
            if (fj.pieces[mid].col0 <= col) f.p = mid;
            else hi = mid;
        }
        fit_enter(j, fj.pieces, &f);
        auto element = [&](uint64_t i) -> uint32_t {             // element i < T of the document
            if (j.nb && i == 0) return j.bos;
            if (j.ne && i == f.T - 1) return j.eos;
            return pack_read<IN>(j.tok, f.src0 + (i - j.nb));
        };
        uint32_t id[kAuxCells], lab[kAuxCells], ps[kAuxCells], sg[kAuxCells];
        uint32_t ign_mask = 0, ahead = 0;                        // ahead: the element read as the cell before's label
        bool have_ahead = false;
#pragma unroll
        for (uint32_t e = 0; e < kAuxCells; ++e) {
            id[e] = j.pad; lab[e] = ign_lo; ps[e] = 0; sg[e] = 0;
            ign_mask |= 1u << e;
            if (e >= cnt) continue;
            if (col == 0 && j.len) {
                const PackFitPiece last = fj.pieces[row_end - 1];
                j.len[row] = last.col0 + last.size;
            }
            if (col < f.end) {                                   // (col >= col0: the walk entered the piece there)
                const uint64_t k = f.k0 + (col - f.col0);
                id[e] = have_ahead ? ahead : element(k);
                have_ahead = false;
                if (LT) {
                    if (want_lab && k >= j.nb && !(j.ne && k == f.T - 1)) {
                        const uint32_t v = fj.a.label_tok[f.src0 + (k - j.nb)];
                        if (v != MBPE_NO_TOKEN) { lab[e] = v; ign_mask &= ~(1u << e); }
                    }
                } else if (want_lab && k + 1 < f.T) {
                    ahead = element(k + 1);
                    have_ahead = col + 1 < f.end;
                    lab[e] = ahead;
                    ign_mask &= ~(1u << e);
                }
                ps[e] = (uint32_t)k;
                sg[e] = (uint32_t)f.d + 1u;
            }
            ++col;
            if (col == j.seq_len) {
                col = 0;
                ++row;
                if (e + 1 < cnt) {                               // (another cell of the group: the row exists)
                    f.p = row_end;
                    row_end = fj.row_first[row + 1];
                    fit_enter(j, fj.pieces, &f);
                }
            } else if (col == f.end && f.p + 1 < row_end) {
                ++f.p;
                fit_enter(j, fj.pieces, &f);
            }
        }
        aux_store_ids<OUT>(j.out, c0, cnt, id, 0u, 0u);
        if (want_lab) aux_store_ids<OUT>(fj.a.labels, c0, cnt, lab, ign_mask, ign_hi);
        if (fj.a.pos) aux_store32(fj.a.pos, c0, cnt, ps);
        if (fj.a.seg) aux_store32(fj.a.seg, c0, cnt, sg);
    }
}

#define PCHK(expr) MBPE_HIP_CHECK(expr, true)

uint32_t pack_grid(const void *out, uint64_t n_out, uint32_t out_bits) {
    const uint64_t A = (uint64_t)(uintptr_t)out, E = A + n_out * (out_bits / 8);
    const uint64_t n_pieces = (E - (A & ~15ull) + 15) >> 4;
    return (uint32_t)std::min<uint64_t>((n_pieces + kPackThreads - 1) / kPackThreads, kPackMaxGrid);
}

template <int IN, int OUT>
void launch_pack(hipStream_t stream, bool packed, const PackJob &j) {
    const dim3 grid(pack_grid(j.out, j.n_out, OUT)), block(kPackThreads);
    if (packed) hipLaunchKernelGGL((k_pack_stream<IN, OUT, false>), grid, block, 0, stream, j);
    else hipLaunchKernelGGL((k_pack_padded<IN, OUT>), grid, block, 0, stream, j);
}

template <int IN, int OUT>
void launch_unpack(hipStream_t stream, const PackJob &j) {
    hipLaunchKernelGGL((k_pack_stream<IN, OUT, true>), dim3(pack_grid(j.out, j.n_out, OUT)), dim3(kPackThreads), 0, stream,
                       j);
}

uint32_t aux_grid(uint64_t n_out) {
    const uint64_t n_groups = (n_out + kAuxCells - 1) / kAuxCells;
    return (uint32_t)std::min<uint64_t>((n_groups + kPackThreads - 1) / kPackThreads, kPackMaxGrid);
}

template <int IN, int OUT>
void launch_pack_aux(hipStream_t stream, bool packed, const PackAuxJob &a) {
    const dim3 grid(aux_grid(a.j.n_out)), block(kPackThreads);
    if (a.label_tok) {                                           // (kernels of their own: the others stay what they were)
        if (packed) hipLaunchKernelGGL((k_pack_aux<IN, OUT, true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((k_pack_aux<IN, OUT, false, true>), grid, block, 0, stream, a);
    } else if (packed) hipLaunchKernelGGL((k_pack_aux<IN, OUT, true, false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((k_pack_aux<IN, OUT, false, false>), grid, block, 0, stream, a);
}

template <int IN, int OUT>
void launch_pack_windows(hipStream_t stream, const PackWinJob &wj) {
    const dim3 grid(aux_grid(wj.a.j.n_out)), block(kPackThreads);
    if (wj.a.label_tok) hipLaunchKernelGGL((k_pack_windows<IN, OUT, true>), grid, block, 0, stream, wj);
    else hipLaunchKernelGGL((k_pack_windows<IN, OUT, false>), grid, block, 0, stream, wj);
}

template <int IN, int OUT>
void launch_pack_fit(hipStream_t stream, const PackFitJob &fj) {
    const dim3 grid(aux_grid(fj.a.j.n_out)), block(kPackThreads);
    if (fj.a.label_tok) hipLaunchKernelGGL((k_pack_fit<IN, OUT, true>), grid, block, 0, stream, fj);
    else hipLaunchKernelGGL((k_pack_fit<IN, OUT, false>), grid, block, 0, stream, fj);
}

// device time of the calling thread's latest one-shot pack or unpack kernel (mbpe_pack_kernel_ms)
thread_local float g_pack_ms = 0.f;

int pack_run(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
             const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec &spec, void *ids_out, uint64_t n_rows,
             int out_on_device, uint32_t *len_out, const mbpe_pack_aux *aux, const mbpe_pack_window *win = nullptr,
             const struct mbpe_pack_fit *fit = nullptr, const PackFitPlan *plan = nullptr,
             const uint32_t *label_tokens = nullptr) {
    int rc = find_device(device_id);
    if (rc != MBPE_OK) return rc;
    OneShot dev;
    rc = dev.open(device_id);
    if (rc != MBPE_OK) return rc;
    const uint64_t id_bytes = n_rows * spec.seq_len * (spec.out_bits / 8);
    void *d_tok = const_cast<void *>(tokens), *d_off = nullptr, *d_ids = ids_out, *d_len = len_out;
    if (!tokens_on_device) rc = dev.alloc(&d_tok, n_tokens * (token_bits / 8), tokens);
    void *d_lab_tok = const_cast<uint32_t *>(label_tokens);      // on the same side as the tokens
    if (rc == MBPE_OK && label_tokens && !tokens_on_device) rc = dev.alloc(&d_lab_tok, n_tokens * 4, label_tokens);
    if (rc == MBPE_OK) rc = dev.alloc(&d_off, (n_docs + 1) * 8, doc_tok_off);
    if (rc == MBPE_OK && !out_on_device) {
        rc = dev.alloc(&d_ids, id_bytes, nullptr);
        if (rc == MBPE_OK && len_out) rc = dev.alloc(&d_len, n_rows * 4, nullptr);
    }
    // the aux outputs of a host call go through device buffers of the call's own, like the ids
    const uint64_t cell_bytes = n_rows * spec.seq_len * 4;
    mbpe_pack_aux d_aux = aux ? *aux : mbpe_pack_aux{};
    if (rc == MBPE_OK && aux && !out_on_device) {
        void *p = nullptr;
        if (aux->labels) { rc = dev.alloc(&p, id_bytes, nullptr); d_aux.labels = p; }
        if (rc == MBPE_OK && aux->pos) { rc = dev.alloc(&p, cell_bytes, nullptr); d_aux.pos = static_cast<uint32_t *>(p); }
        if (rc == MBPE_OK && aux->seg) { rc = dev.alloc(&p, cell_bytes, nullptr); d_aux.seg = static_cast<uint32_t *>(p); }
    }
    // the windows: row_start, and row_doc / row_tok0 of a host call like the aux outputs
    mbpe_pack_window d_win = win ? *win : mbpe_pack_window{};
    void *d_row_start = nullptr;
    if (rc == MBPE_OK && win) {
        void *p = nullptr;
        rc = dev.alloc(&d_row_start, pack_win_scratch_bytes(n_docs), nullptr);
        if (rc == MBPE_OK && win->row_doc && !out_on_device) { rc = dev.alloc(&p, n_rows * 4, nullptr); d_win.row_doc = static_cast<uint32_t *>(p); }
        if (rc == MBPE_OK && win->row_tok0 && !out_on_device) { rc = dev.alloc(&p, n_rows * 8, nullptr); d_win.row_tok0 = static_cast<uint64_t *>(p); }
    }
    // the plan of a fit call: the piece table and row_first
    void *d_pieces = nullptr, *d_row_first = nullptr;
    if (rc == MBPE_OK && fit) {
        rc = dev.alloc(&d_pieces, pack_fit_piece_bytes(*plan), plan->pieces.data());
        if (rc == MBPE_OK) rc = dev.alloc(&d_row_first, (n_rows + 1) * 8, plan->row_first.data());
    }
    if (rc != MBPE_OK) return rc;
    const PackSrc src = {d_tok, static_cast<const unsigned long long *>(d_off), n_docs, n_tokens, token_bits,
                         static_cast<const uint32_t *>(d_lab_tok)};
    const PackDst dst = {d_ids, static_cast<uint32_t *>(d_len), n_rows};
    PCHK(hipEventRecord(dev.ev0, dev.stream));
    if (fit) {
        pack_launch_fit(dev.stream, src, spec, dst, d_aux, d_pieces, static_cast<const unsigned long long *>(d_row_first));
    } else if (win) {
        unsigned long long *row_start = static_cast<unsigned long long *>(d_row_start);
        pack_launch_win_rows(dev.stream, src.doc_off, n_docs, spec, d_win, row_start);
        pack_launch_windows(dev.stream, src, spec, dst, d_aux, d_win, row_start);
    } else if (aux) pack_launch_aux(dev.stream, src, spec, dst, d_aux);
    else pack_launch(dev.stream, src, spec, dst);
    rc = dev.finish(&g_pack_ms);
    if (rc != MBPE_OK) return rc;
    if (!out_on_device) {
        PCHK(hipMemcpyAsync(ids_out, d_ids, id_bytes, hipMemcpyDeviceToHost, dev.stream));
        if (len_out) PCHK(hipMemcpyAsync(len_out, d_len, n_rows * 4, hipMemcpyDeviceToHost, dev.stream));
        if (aux && aux->labels) PCHK(hipMemcpyAsync(aux->labels, d_aux.labels, id_bytes, hipMemcpyDeviceToHost, dev.stream));
        if (aux && aux->pos) PCHK(hipMemcpyAsync(aux->pos, d_aux.pos, cell_bytes, hipMemcpyDeviceToHost, dev.stream));
        if (aux && aux->seg) PCHK(hipMemcpyAsync(aux->seg, d_aux.seg, cell_bytes, hipMemcpyDeviceToHost, dev.stream));
        if (win && win->row_doc) PCHK(hipMemcpyAsync(win->row_doc, d_win.row_doc, n_rows * 4, hipMemcpyDeviceToHost, dev.stream));
        if (win && win->row_tok0) PCHK(hipMemcpyAsync(win->row_tok0, d_win.row_tok0, n_rows * 8, hipMemcpyDeviceToHost, dev.stream));
        PCHK(hipStreamSynchronize(dev.stream));
    }
    return fit ? pack_fit_doc_out(dev.stream, *fit, *plan, out_on_device) : MBPE_OK;
}

int unpack_run(int device_id, const void *ids, uint64_t n_rows, uint32_t seq_len, uint32_t id_bits, int ids_on_device,
               const uint32_t *len, void *tokens_out, uint64_t cap, uint32_t token_bits, int out_on_device,
               uint64_t *doc_tok_off_out, uint64_t *n_out) {
    // the lengths decide everything else: those of a device matrix come to the host first
    std::vector<uint32_t> len_host;
    std::vector<uint64_t> off(n_rows + 1, 0);
    if (ids_on_device && n_rows) {
        int rc = find_device(device_id);
        if (rc != MBPE_OK) return rc;
        len_host.resize(n_rows);
        PCHK(hipSetDevice(device_id));
        PCHK(hipMemcpy(len_host.data(), len, n_rows * 4, hipMemcpyDeviceToHost));
        len = len_host.data();
    }
    for (uint64_t r = 0; r < n_rows; ++r) {
        if (len[r] > seq_len)
            return fail(MBPE_ERR_ARG, "len[" + std::to_string(r) + "] = " + std::to_string(len[r]) + " exceeds seq_len");
        off[r + 1] = off[r] + len[r];
    }
    const uint64_t n = off[n_rows];
    *n_out = n;
    if (doc_tok_off_out) std::copy(off.begin(), off.end(), doc_tok_off_out);
    if (!tokens_out) return MBPE_OK;                             // the query
    if (cap < n) return fail(MBPE_ERR_ARG, "tokens_out too small");
    if (n == 0) return MBPE_OK;
    if (out_on_device && (uint64_t)(uintptr_t)tokens_out % (token_bits / 8))
        return fail(MBPE_ERR_ARG, "tokens_out is not aligned to its tokens");
    int rc = find_device(device_id);
    if (rc != MBPE_OK) return rc;
    OneShot dev;
    rc = dev.open(device_id);
    if (rc != MBPE_OK) return rc;
    void *d_ids = const_cast<void *>(ids), *d_off = nullptr, *d_tok = tokens_out;
    if (!ids_on_device) rc = dev.alloc(&d_ids, n_rows * seq_len * (id_bits / 8), ids);
    if (rc == MBPE_OK) rc = dev.alloc(&d_off, (n_rows + 1) * 8, off.data());
    if (rc == MBPE_OK && !out_on_device) rc = dev.alloc(&d_tok, n * (token_bits / 8), nullptr);
    if (rc != MBPE_OK) return rc;
    PackJob j = {};
    j.tok = d_ids;
    j.doc_off = static_cast<const unsigned long long *>(d_off);
    j.n_docs = n_rows;
    j.n_stream = n;
    j.out = d_tok;
    j.n_out = n;
    j.seq_len = seq_len;
    PCHK(hipEventRecord(dev.ev0, dev.stream));
    if (id_bits == 16 && token_bits == 16) launch_unpack<16, 16>(dev.stream, j);
    else if (id_bits == 16) launch_unpack<16, 32>(dev.stream, j);
    else if (id_bits == 32) launch_unpack<32, 32>(dev.stream, j);
    else launch_unpack<64, 32>(dev.stream, j);
    rc = dev.finish(&g_pack_ms);
    if (rc != MBPE_OK) return rc;
    if (!out_on_device) {
        PCHK(hipMemcpyAsync(tokens_out, d_tok, n * (token_bits / 8), hipMemcpyDeviceToHost, dev.stream));
        PCHK(hipStreamSynchronize(dev.stream));
    }
    return MBPE_OK;
}

}  // namespace

namespace mbpe {

int pack_check_spec(const mbpe_pack_spec *spec, uint32_t token_bits) {
    if (!spec) return fail(MBPE_ERR_ARG, "NULL pack spec");
    if (token_bits != 16 && token_bits != 32) return fail(MBPE_ERR_ARG, "token_bits must be 16 or 32");
    if (spec->layout != MBPE_PACK_PADDED && spec->layout != MBPE_PACK_PACKED)
        return fail(MBPE_ERR_ARG, "no such pack layout");
    if (spec->out_bits != 16 && spec->out_bits != 32 && spec->out_bits != 64)
        return fail(MBPE_ERR_ARG, "out_bits must be 16, 32 or 64");
    if (spec->seq_len == 0) return fail(MBPE_ERR_ARG, "seq_len must be at least 1");
    const uint32_t nbe = (spec->bos_id != MBPE_NO_TOKEN) + (spec->eos_id != MBPE_NO_TOKEN);
    if (spec->layout == MBPE_PACK_PADDED && spec->seq_len < nbe)
        return fail(MBPE_ERR_ARG, "seq_len has no room for bos and eos");
    if (spec->layout == MBPE_PACK_PACKED && (spec->pad_left || spec->trunc_left))
        return fail(MBPE_ERR_ARG, "pad_left and trunc_left go with MBPE_PACK_PADDED only");
    if (spec->out_bits == 16) {
        if (token_bits == 32) return fail(MBPE_ERR_VOCAB, "out_bits 16 with 32-bit tokens");
        if (spec->pad_id >= 65536u || (spec->bos_id != MBPE_NO_TOKEN && spec->bos_id >= 65536u) ||
            (spec->eos_id != MBPE_NO_TOKEN && spec->eos_id >= 65536u))
            return fail(MBPE_ERR_VOCAB, "out_bits 16 with a pad, bos or eos id that does not fit 16 bits");
    }
    return MBPE_OK;
}

uint64_t pack_rows(const mbpe_pack_spec &spec, uint64_t n_tokens, uint64_t n_docs) {
    if (spec.layout == MBPE_PACK_PADDED) return n_docs;
    const uint64_t nbe = (spec.bos_id != MBPE_NO_TOKEN) + (spec.eos_id != MBPE_NO_TOKEN);
    return (n_tokens + n_docs * nbe + spec.seq_len - 1) / spec.seq_len;
}

static PackJob pack_job(const PackSrc &src, const mbpe_pack_spec &spec, const PackDst &dst) {
    PackJob j = {};
    j.tok = src.tok;
    j.doc_off = src.doc_off;
    j.n_docs = src.n_docs;
    j.out = dst.ids;
    j.len = dst.len;
    j.n_out = dst.n_rows * spec.seq_len;
    j.seq_len = spec.seq_len;
    j.pad = spec.pad_id;
    j.nb = spec.bos_id != MBPE_NO_TOKEN;
    j.ne = spec.eos_id != MBPE_NO_TOKEN;
    j.bos = spec.bos_id;
    j.eos = spec.eos_id;
    j.n_stream = src.n_tokens + src.n_docs * (uint64_t)(j.nb + j.ne);
    j.keep = spec.seq_len - j.nb - j.ne;                         // (PADDED: checked; PACKED does not read it)
    j.pad_left = spec.pad_left != 0;
    j.trunc_left = spec.trunc_left != 0;
    return j;
}

void pack_launch(hipStream_t stream, const PackSrc &src, const mbpe_pack_spec &spec, const PackDst &dst) {
    const PackJob j = pack_job(src, spec, dst);
    const bool packed = spec.layout == MBPE_PACK_PACKED;
    if (src.bits == 16) {
        if (spec.out_bits == 16) launch_pack<16, 16>(stream, packed, j);
        else if (spec.out_bits == 32) launch_pack<16, 32>(stream, packed, j);
        else launch_pack<16, 64>(stream, packed, j);
    } else {
        if (spec.out_bits == 32) launch_pack<32, 32>(stream, packed, j);
        else launch_pack<32, 64>(stream, packed, j);
    }
}

void pack_launch_aux(hipStream_t stream, const PackSrc &src, const mbpe_pack_spec &spec, const PackDst &dst,
                     const mbpe_pack_aux &aux) {
    const PackAuxJob a = {pack_job(src, spec, dst), aux.labels, aux.pos, aux.seg, (unsigned long long)aux.ignore_label,
                          src.label_tok};
    const bool packed = spec.layout == MBPE_PACK_PACKED;
    if (src.bits == 16) {
        if (spec.out_bits == 16) launch_pack_aux<16, 16>(stream, packed, a);
        else if (spec.out_bits == 32) launch_pack_aux<16, 32>(stream, packed, a);
        else launch_pack_aux<16, 64>(stream, packed, a);
    } else {
        if (spec.out_bits == 32) launch_pack_aux<32, 32>(stream, packed, a);
        else launch_pack_aux<32, 64>(stream, packed, a);
    }
}

static PackWinJob pack_win_job(const PackSrc &src, const mbpe_pack_spec &spec, const PackDst &dst, const mbpe_pack_aux &aux,
                               const mbpe_pack_window &win, const unsigned long long *row_start) {
    PackWinJob wj = {};
    wj.a = {pack_job(src, spec, dst), aux.labels, aux.pos, aux.seg, (unsigned long long)aux.ignore_label, src.label_tok};
    wj.row_start = row_start;
    wj.row_doc = win.row_doc;
    wj.row_tok0 = reinterpret_cast<unsigned long long *>(win.row_tok0);
    wj.stride = win.stride;
    wj.step = wj.a.j.keep - win.stride;
    wj.score_once = win.score_once;
    return wj;
}

void pack_launch_win_rows(hipStream_t stream, const unsigned long long *doc_off, uint64_t n_docs,
                          const mbpe_pack_spec &spec, const mbpe_pack_window &win, unsigned long long *row_start) {
    const uint32_t keep = spec.seq_len - (spec.bos_id != MBPE_NO_TOKEN) - (spec.eos_id != MBPE_NO_TOKEN);
    unsigned long long *span_cnt = row_start + n_docs + 1;       // (pack_win_scratch_bytes)
    const dim3 grid(span_grid(n_docs)), block(kSpanThreads);
    hipLaunchKernelGGL(k_win_rows, grid, block, 0, stream, doc_off, n_docs, keep, keep - win.stride, row_start, span_cnt);
    hipLaunchKernelGGL(k_win_scan, dim3(1), dim3(kScanThreads), 0, stream, span_cnt, span_count(n_docs), row_start + n_docs);
    hipLaunchKernelGGL(k_win_offsets, grid, block, 0, stream, row_start, n_docs, span_cnt);
}

uint64_t pack_win_scratch_bytes(uint64_t n_docs) { return (n_docs + 1 + span_count(n_docs)) * 8; }

void pack_launch_windows(hipStream_t stream, const PackSrc &src, const mbpe_pack_spec &spec, const PackDst &dst,
                         const mbpe_pack_aux &aux, const mbpe_pack_window &win, const unsigned long long *row_start) {
    const PackWinJob wj = pack_win_job(src, spec, dst, aux, win, row_start);
    if (src.bits == 16) {
        if (spec.out_bits == 16) launch_pack_windows<16, 16>(stream, wj);
        else if (spec.out_bits == 32) launch_pack_windows<16, 32>(stream, wj);
        else launch_pack_windows<16, 64>(stream, wj);
    } else {
        if (spec.out_bits == 32) launch_pack_windows<32, 32>(stream, wj);
        else launch_pack_windows<32, 64>(stream, wj);
    }
}

int pack_check_windows(const mbpe_pack_spec *spec, uint32_t token_bits, const mbpe_pack_aux *aux,
                       const mbpe_pack_window *win, uint64_t n_docs, const void *ids_out, int out_on_device) {
    int rc = pack_check_spec(spec, token_bits);
    if (rc != MBPE_OK) return rc;
    const char *msg = "";
    if ((rc = pack_win_check(*spec, win, n_docs, &msg)) != MBPE_OK) return fail(rc, msg);
    if ((rc = pack_check_aux(*spec, aux, nullptr, n_docs, ids_out, out_on_device)) != MBPE_OK) return rc;
    if (ids_out && out_on_device && ((uint64_t)(uintptr_t)win->row_doc % 4 || (uint64_t)(uintptr_t)win->row_tok0 % 8))
        return fail(MBPE_ERR_ARG, "row_doc or row_tok0 in device memory is not aligned to its elements");
    return MBPE_OK;
}

int pack_window_rows(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec &spec, const mbpe_pack_window &win,
                     uint64_t *n_rows_out) {
    const char *msg = "";
    const uint32_t keep = spec.seq_len - (spec.bos_id != MBPE_NO_TOKEN) - (spec.eos_id != MBPE_NO_TOKEN);
    const int rc = pack_win_rows(doc_tok_off, n_docs, keep, win.stride, n_rows_out, &msg);
    return rc == MBPE_OK ? MBPE_OK : fail(rc, msg);
}

uint64_t pack_fit_piece_bytes(const PackFitPlan &plan) { return plan.pieces.size() * sizeof(PackFitPiece); }

void pack_launch_fit(hipStream_t stream, const PackSrc &src, const mbpe_pack_spec &spec, const PackDst &dst,
                     const mbpe_pack_aux &aux, const void *pieces, const unsigned long long *row_first) {
    PackFitJob fj = {};
    fj.a = {pack_job(src, spec, dst), aux.labels, aux.pos, aux.seg, (unsigned long long)aux.ignore_label, src.label_tok};
    fj.pieces = static_cast<const PackFitPiece *>(pieces);
    fj.row_first = row_first;
    if (src.bits == 16) {
        if (spec.out_bits == 16) launch_pack_fit<16, 16>(stream, fj);
        else if (spec.out_bits == 32) launch_pack_fit<16, 32>(stream, fj);
        else launch_pack_fit<16, 64>(stream, fj);
    } else {
        if (spec.out_bits == 32) launch_pack_fit<32, 32>(stream, fj);
        else launch_pack_fit<32, 64>(stream, fj);
    }
}

int pack_check_fit(const mbpe_pack_spec *spec, uint32_t token_bits, const mbpe_pack_aux *aux, const struct mbpe_pack_fit *fit,
                   uint64_t n_docs, const void *ids_out, int out_on_device) {
    int rc = pack_check_spec(spec, token_bits);
    if (rc != MBPE_OK) return rc;
    if (!fit) return fail(MBPE_ERR_ARG, "NULL pack fit");
    if (spec->layout != MBPE_PACK_PACKED)
        return fail(MBPE_ERR_ARG, "fit goes with MBPE_PACK_PACKED, pad_left 0 and trunc_left 0 only");
    if ((rc = pack_check_aux(*spec, aux, nullptr, n_docs, ids_out, out_on_device)) != MBPE_OK) return rc;
    if (ids_out && out_on_device && ((uint64_t)(uintptr_t)fit->doc_row % 8 || (uint64_t)(uintptr_t)fit->doc_col % 4))
        return fail(MBPE_ERR_ARG, "doc_row or doc_col in device memory is not aligned to its elements");
    return MBPE_OK;
}

int pack_fit_make(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec &spec, PackFitPlan *plan) {
    const char *msg = "";
    const int rc = pack_fit_plan(doc_tok_off, n_docs, spec.seq_len,
                                 (spec.bos_id != MBPE_NO_TOKEN) + (spec.eos_id != MBPE_NO_TOKEN), plan, &msg);
    return rc == MBPE_OK ? MBPE_OK : fail(rc, msg);
}

int pack_fit_doc_out(hipStream_t stream, const struct mbpe_pack_fit &fit, const PackFitPlan &plan, int out_on_device) {
    const uint64_t n_docs = plan.doc_row.size();
    if (!n_docs) return MBPE_OK;
    if (!out_on_device) {
        if (fit.doc_row) std::copy(plan.doc_row.begin(), plan.doc_row.end(), fit.doc_row);
        if (fit.doc_col) std::copy(plan.doc_col.begin(), plan.doc_col.end(), fit.doc_col);
        return MBPE_OK;
    }
    if (fit.doc_row) PCHK(hipMemcpyAsync(fit.doc_row, plan.doc_row.data(), n_docs * 8, hipMemcpyHostToDevice, stream));
    if (fit.doc_col) PCHK(hipMemcpyAsync(fit.doc_col, plan.doc_col.data(), n_docs * 4, hipMemcpyHostToDevice, stream));
    if (fit.doc_row || fit.doc_col) PCHK(hipStreamSynchronize(stream));
    return MBPE_OK;
}

int pack_check_aux(const mbpe_pack_spec &spec, const mbpe_pack_aux *aux, const uint64_t *doc_tok_off, uint64_t n_docs,
                   const void *ids_out, int out_on_device) {
    if (!aux) return fail(MBPE_ERR_ARG, "NULL pack aux");
    const char *msg = "";
    int rc = pack_check_ignore(spec.out_bits, aux->ignore_label, &msg);
    if (rc == MBPE_OK && aux->seg) rc = pack_check_seg_docs(n_docs, &msg);
    if (rc == MBPE_OK && aux->pos && doc_tok_off && spec.layout == MBPE_PACK_PACKED)
        rc = pack_check_pos_docs(doc_tok_off, n_docs,
                                 (spec.bos_id != MBPE_NO_TOKEN) + (spec.eos_id != MBPE_NO_TOKEN), &msg);
    if (rc != MBPE_OK) return fail(rc, msg);
    if (ids_out && out_on_device)
        for (const void *p : {ids_out, (const void *)aux->labels, (const void *)aux->pos, (const void *)aux->seg})
            if ((uint64_t)(uintptr_t)p % 16)
                return fail(MBPE_ERR_ARG, "ids_out, labels, pos and seg in device memory must be 16-byte aligned");
    return MBPE_OK;
}

}  // namespace mbpe

namespace mbpe_host {

int device_alloc(int device_id, uint64_t n_bytes, void **out) {
    *out = nullptr;
    const int rc = find_device(device_id);
    if (rc != MBPE_OK) return rc;
    PCHK(hipSetDevice(device_id));
    DevAlloc mem = {true};
    DevBuf<void> buf;
    const int rc_buf = buf.reserve(n_bytes ? n_bytes : 1, mem);
    *out = buf.release();                                        // the caller's from here on: device_free
    return rc_buf;
}

void device_free(void *p) { dev_free(p); }

}  // namespace mbpe_host

extern "C" {

int mbpe_pack_tokens(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                     const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec *spec, void *ids_out,
                     uint64_t cap_rows, int out_on_device, uint32_t *len_out, uint64_t *n_rows_out) {
    if (n_rows_out) *n_rows_out = 0;
    if (!n_rows_out || !doc_tok_off || !spec || (!tokens && n_tokens))
        return fail(MBPE_ERR_ARG, "mbpe_pack_tokens: NULL argument");
    int rc = pack_check_spec(spec, token_bits);
    if (rc == MBPE_OK) rc = mbpe_host::check_doc_tok_off(doc_tok_off, n_docs, n_tokens);
    if (rc != MBPE_OK) return rc;
    if (n_tokens >> 40 || n_docs >> 40) return fail(MBPE_ERR_ARG, "more than 2^40 tokens or documents");
    const uint64_t n_rows = pack_rows(*spec, n_tokens, n_docs);
    *n_rows_out = n_rows;
    if (!ids_out) return MBPE_OK;                                // the query
    if (cap_rows < n_rows) return fail(MBPE_ERR_ARG, "ids_out too small");
    if (n_rows == 0) return MBPE_OK;
    if (out_on_device && ((uint64_t)(uintptr_t)ids_out % (spec->out_bits / 8) || (uint64_t)(uintptr_t)len_out % 4))
        return fail(MBPE_ERR_ARG, "ids_out or len_out is not aligned to its elements");
    try {
        return pack_run(device_id, tokens, n_tokens, token_bits, tokens_on_device, doc_tok_off, n_docs, *spec, ids_out,
                        n_rows, out_on_device, len_out, nullptr);
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_pack_tokens: host allocation failed");
    }
}

// The three aux calls and their _labels forms share one implementation each.  with_labels: label_tokens is required
// (n_tokens entries on the side of the tokens, 4-byte aligned there); otherwise it is NULL
static int label_tokens_check(const std::string &who, bool with_labels, const uint32_t *label_tokens, uint64_t n_tokens,
                              int tokens_on_device) {
    if (!with_labels) return MBPE_OK;
    if (!label_tokens && n_tokens) return fail(MBPE_ERR_ARG, who + ": NULL argument");
    if (tokens_on_device && (uint64_t)(uintptr_t)label_tokens % 4)
        return fail(MBPE_ERR_ARG, who + ": label_tokens is not aligned to its elements");
    return MBPE_OK;
}

static int pack_aux_entry(const std::string &who, bool with_labels, int device_id, const void *tokens, uint64_t n_tokens,
                          uint32_t token_bits, int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                          const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows, int out_on_device,
                          uint32_t *len_out, uint64_t *n_rows_out, const mbpe_pack_aux *aux, const uint32_t *label_tokens) {
    if (n_rows_out) *n_rows_out = 0;
    if (!n_rows_out || !doc_tok_off || !spec || !aux || (!tokens && n_tokens))
        return fail(MBPE_ERR_ARG, who + ": NULL argument");
    if (const int rc0 = label_tokens_check(who, with_labels, label_tokens, n_tokens, tokens_on_device)) return rc0;
    int rc = pack_check_spec(spec, token_bits);
    if (rc == MBPE_OK) rc = mbpe_host::check_doc_tok_off(doc_tok_off, n_docs, n_tokens);
    if (rc != MBPE_OK) return rc;
    if (n_tokens >> 40 || n_docs >> 40) return fail(MBPE_ERR_ARG, "more than 2^40 tokens or documents");
    rc = pack_check_aux(*spec, aux, doc_tok_off, n_docs, ids_out, out_on_device);
    if (rc != MBPE_OK) return rc;
    const uint64_t n_rows = pack_rows(*spec, n_tokens, n_docs);
    *n_rows_out = n_rows;
    if (!ids_out) return MBPE_OK;                                // the query
    if (cap_rows < n_rows) return fail(MBPE_ERR_ARG, "ids_out too small");
    if (n_rows == 0) return MBPE_OK;
    if (out_on_device && (uint64_t)(uintptr_t)len_out % 4) return fail(MBPE_ERR_ARG, "len_out is not aligned to its elements");
    try {
        return pack_run(device_id, tokens, n_tokens, token_bits, tokens_on_device, doc_tok_off, n_docs, *spec, ids_out,
                        n_rows, out_on_device, len_out, aux, nullptr, nullptr, nullptr, label_tokens);
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, who + ": host allocation failed");
    }
}

int mbpe_pack_tokens_aux(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                         const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec *spec, void *ids_out,
                         uint64_t cap_rows, int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                         const mbpe_pack_aux *aux) {
    return pack_aux_entry("mbpe_pack_tokens_aux", false, device_id, tokens, n_tokens, token_bits, tokens_on_device,
                          doc_tok_off, n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, aux, nullptr);
}

int mbpe_pack_tokens_aux_labels(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits,
                                int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                                const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows, int out_on_device,
                                uint32_t *len_out, uint64_t *n_rows_out, const mbpe_pack_aux *aux,
                                const uint32_t *label_tokens) {
    return pack_aux_entry("mbpe_pack_tokens_aux_labels", true, device_id, tokens, n_tokens, token_bits, tokens_on_device,
                          doc_tok_off, n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, aux,
                          label_tokens);
}

static int pack_windows_entry(const std::string &who, bool with_labels, int device_id, const void *tokens, uint64_t n_tokens,
                              uint32_t token_bits, int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                              const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows, int out_on_device,
                              uint32_t *len_out, uint64_t *n_rows_out, const mbpe_pack_aux *aux,
                              const mbpe_pack_window *win, const uint32_t *label_tokens) {
    if (n_rows_out) *n_rows_out = 0;
    if (!n_rows_out || !doc_tok_off || !spec || !aux || !win || (!tokens && n_tokens))
        return fail(MBPE_ERR_ARG, who + ": NULL argument");
    if (const int rc0 = label_tokens_check(who, with_labels, label_tokens, n_tokens, tokens_on_device)) return rc0;
    int rc = pack_check_windows(spec, token_bits, aux, win, n_docs, ids_out, out_on_device);
    if (rc == MBPE_OK) rc = mbpe_host::check_doc_tok_off(doc_tok_off, n_docs, n_tokens);
    if (rc != MBPE_OK) return rc;
    if (n_tokens >> 40 || n_docs >> 40) return fail(MBPE_ERR_ARG, "more than 2^40 tokens or documents");
    uint64_t n_rows = 0;
    if ((rc = pack_window_rows(doc_tok_off, n_docs, *spec, *win, &n_rows)) != MBPE_OK) return rc;
    *n_rows_out = n_rows;
    if (!ids_out) return MBPE_OK;                                // the query
    if (cap_rows < n_rows) return fail(MBPE_ERR_ARG, "ids_out too small");
    if (n_rows == 0) return MBPE_OK;
    if (out_on_device && (uint64_t)(uintptr_t)len_out % 4) return fail(MBPE_ERR_ARG, "len_out is not aligned to its elements");
    try {
        return pack_run(device_id, tokens, n_tokens, token_bits, tokens_on_device, doc_tok_off, n_docs, *spec, ids_out,
                        n_rows, out_on_device, len_out, aux, win, nullptr, nullptr, label_tokens);
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, who + ": host allocation failed");
    }
}

int mbpe_pack_windows(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                      const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec *spec, void *ids_out,
                      uint64_t cap_rows, int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                      const mbpe_pack_aux *aux, const mbpe_pack_window *win) {
    return pack_windows_entry("mbpe_pack_windows", false, device_id, tokens, n_tokens, token_bits, tokens_on_device,
                              doc_tok_off, n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, aux, win,
                              nullptr);
}

int mbpe_pack_windows_labels(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                             const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec *spec, void *ids_out,
                             uint64_t cap_rows, int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                             const mbpe_pack_aux *aux, const mbpe_pack_window *win, const uint32_t *label_tokens) {
    return pack_windows_entry("mbpe_pack_windows_labels", true, device_id, tokens, n_tokens, token_bits, tokens_on_device,
                              doc_tok_off, n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, aux, win,
                              label_tokens);
}

int mbpe_pack_cu_seqlens(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec *spec, int32_t *cu_out,
                         uint64_t cap_seqs, uint64_t *n_seqs_out, uint32_t *max_seqlen_out) {
    if (n_seqs_out) *n_seqs_out = 0;
    if (max_seqlen_out) *max_seqlen_out = 0;
    if (!doc_tok_off || !spec || !n_seqs_out || !max_seqlen_out)
        return fail(MBPE_ERR_ARG, "mbpe_pack_cu_seqlens: NULL argument");
    int rc = pack_check_spec(spec, spec->out_bits == 16 ? 16 : 32);
    if (rc != MBPE_OK) return rc;
    if (spec->layout != MBPE_PACK_PACKED)
        return fail(MBPE_ERR_ARG, "cu_seqlens goes with MBPE_PACK_PACKED only (the sequences of PADDED are its rows)");
    rc = mbpe_host::check_doc_tok_off(doc_tok_off, n_docs, doc_tok_off[n_docs]);
    if (rc != MBPE_OK) return rc;
    const char *msg = "";
    uint64_t n_seqs = 0;
    uint32_t longest = 0;
    rc = pack_cu_seqlens(doc_tok_off, n_docs, spec->seq_len, (spec->bos_id != MBPE_NO_TOKEN) + (spec->eos_id != MBPE_NO_TOKEN),
                         cu_out, cap_seqs, &n_seqs, &longest, &msg);
    *n_seqs_out = n_seqs;                                        // (also when cap_seqs is too small)
    *max_seqlen_out = longest;
    return rc == MBPE_OK ? MBPE_OK : fail(rc, msg);
}

// what the two host-only fit calls check alike: the spec (for tokens as wide as its ids allow), the layout, the offsets
static int fit_host_check(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec *spec) {
    int rc = pack_check_spec(spec, spec->out_bits == 16 ? 16 : 32);
    if (rc != MBPE_OK) return rc;
    if (spec->layout != MBPE_PACK_PACKED)
        return fail(MBPE_ERR_ARG, "fit goes with MBPE_PACK_PACKED, pad_left 0 and trunc_left 0 only");
    if (n_docs >> 40) return fail(MBPE_ERR_ARG, "more than 2^40 tokens or documents");
    rc = mbpe_host::check_doc_tok_off(doc_tok_off, n_docs, doc_tok_off[n_docs]);
    if (rc == MBPE_OK && doc_tok_off[n_docs] >> 40) rc = fail(MBPE_ERR_ARG, "more than 2^40 tokens or documents");
    return rc;
}

int mbpe_pack_fit_plan(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec *spec, uint32_t *len_out,
                       uint64_t cap_rows, uint64_t *n_rows_out, uint64_t *doc_row_out, uint32_t *doc_col_out) {
    if (n_rows_out) *n_rows_out = 0;
    if (!doc_tok_off || !spec || !n_rows_out) return fail(MBPE_ERR_ARG, "mbpe_pack_fit_plan: NULL argument");
    int rc = fit_host_check(doc_tok_off, n_docs, spec);
    if (rc != MBPE_OK) return rc;
    try {
        PackFitPlan plan;
        if ((rc = pack_fit_make(doc_tok_off, n_docs, *spec, &plan)) != MBPE_OK) return rc;
        *n_rows_out = plan.n_rows;
        if (len_out && cap_rows < plan.n_rows) return fail(MBPE_ERR_ARG, "len_out too small");
        if (len_out) std::copy(plan.len.begin(), plan.len.end(), len_out);
        if (doc_row_out) std::copy(plan.doc_row.begin(), plan.doc_row.end(), doc_row_out);
        if (doc_col_out) std::copy(plan.doc_col.begin(), plan.doc_col.end(), doc_col_out);
        return MBPE_OK;
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_pack_fit_plan: host allocation failed");
    }
}

int mbpe_pack_fit_cu_seqlens(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec *spec, int32_t *cu_out,
                             uint64_t cap_seqs, uint64_t *n_seqs_out, uint32_t *max_seqlen_out) {
    if (n_seqs_out) *n_seqs_out = 0;
    if (max_seqlen_out) *max_seqlen_out = 0;
    if (!doc_tok_off || !spec || !n_seqs_out || !max_seqlen_out)
        return fail(MBPE_ERR_ARG, "mbpe_pack_fit_cu_seqlens: NULL argument");
    int rc = fit_host_check(doc_tok_off, n_docs, spec);
    if (rc != MBPE_OK) return rc;
    try {
        PackFitPlan plan;
        if ((rc = pack_fit_make(doc_tok_off, n_docs, *spec, &plan)) != MBPE_OK) return rc;
        const char *msg = "";
        uint64_t n_seqs = 0;
        uint32_t longest = 0;
        rc = pack_fit_cu_seqlens(plan, spec->seq_len, cu_out, cap_seqs, &n_seqs, &longest, &msg);
        *n_seqs_out = n_seqs;                                    // (also when cap_seqs is too small)
        *max_seqlen_out = longest;
        return rc == MBPE_OK ? MBPE_OK : fail(rc, msg);
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_pack_fit_cu_seqlens: host allocation failed");
    }
}

static int pack_fit_entry(const std::string &who, bool with_labels, int device_id, const void *tokens, uint64_t n_tokens,
                          uint32_t token_bits, int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                          const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows, int out_on_device,
                          uint32_t *len_out, uint64_t *n_rows_out, const mbpe_pack_aux *aux,
                          const struct mbpe_pack_fit *fit, const uint32_t *label_tokens) {
    if (n_rows_out) *n_rows_out = 0;
    if (!n_rows_out || !doc_tok_off || !spec || !aux || !fit || (!tokens && n_tokens))
        return fail(MBPE_ERR_ARG, who + ": NULL argument");
    if (const int rc0 = label_tokens_check(who, with_labels, label_tokens, n_tokens, tokens_on_device)) return rc0;
    int rc = pack_check_fit(spec, token_bits, aux, fit, n_docs, ids_out, out_on_device);
    if (rc == MBPE_OK) rc = mbpe_host::check_doc_tok_off(doc_tok_off, n_docs, n_tokens);
    if (rc != MBPE_OK) return rc;
    if (n_tokens >> 40 || n_docs >> 40) return fail(MBPE_ERR_ARG, "more than 2^40 tokens or documents");
    if ((rc = pack_check_aux(*spec, aux, doc_tok_off, n_docs, nullptr, 0)) != MBPE_OK) return rc;   // (pos: every T_d)
    try {
        PackFitPlan plan;
        if ((rc = pack_fit_make(doc_tok_off, n_docs, *spec, &plan)) != MBPE_OK) return rc;
        const uint64_t n_rows = plan.n_rows;
        *n_rows_out = n_rows;
        if (!ids_out) return MBPE_OK;                            // the query
        if (cap_rows < n_rows) return fail(MBPE_ERR_ARG, "ids_out too small");
        if (out_on_device && (uint64_t)(uintptr_t)len_out % 4)
            return fail(MBPE_ERR_ARG, "len_out is not aligned to its elements");
        if (n_rows == 0) {                                       // no document has an element: doc_row says so
            if (!out_on_device || !n_docs || (!fit->doc_row && !fit->doc_col))
                return pack_fit_doc_out(nullptr, *fit, plan, 0);
            if ((rc = find_device(device_id)) != MBPE_OK) return rc;
            OneShot dev;
            if ((rc = dev.open(device_id)) != MBPE_OK) return rc;
            return pack_fit_doc_out(dev.stream, *fit, plan, 1);
        }
        return pack_run(device_id, tokens, n_tokens, token_bits, tokens_on_device, doc_tok_off, n_docs, *spec, ids_out,
                        n_rows, out_on_device, len_out, aux, nullptr, fit, &plan, label_tokens);
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, who + ": host allocation failed");
    }
}

int mbpe_pack_fit(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                  const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec *spec, void *ids_out,
                  uint64_t cap_rows, int out_on_device, uint32_t *len_out, uint64_t *n_rows_out, const mbpe_pack_aux *aux,
                  const struct mbpe_pack_fit *fit) {
    return pack_fit_entry("mbpe_pack_fit", false, device_id, tokens, n_tokens, token_bits, tokens_on_device, doc_tok_off,
                          n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, aux, fit, nullptr);
}

int mbpe_pack_fit_labels(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                         const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec *spec, void *ids_out,
                         uint64_t cap_rows, int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                         const mbpe_pack_aux *aux, const struct mbpe_pack_fit *fit, const uint32_t *label_tokens) {
    return pack_fit_entry("mbpe_pack_fit_labels", true, device_id, tokens, n_tokens, token_bits, tokens_on_device,
                          doc_tok_off, n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, aux, fit,
                          label_tokens);
}

int mbpe_unpack_tokens(int device_id, const void *ids, uint64_t n_rows, uint32_t seq_len, uint32_t id_bits,
                       int ids_on_device, const uint32_t *len, void *tokens_out, uint64_t cap, uint32_t token_bits,
                       int out_on_device, uint64_t *doc_tok_off_out, uint64_t *n_out) {
    if (n_out) *n_out = 0;
    if (!n_out || ((!ids || !len) && n_rows)) return fail(MBPE_ERR_ARG, "mbpe_unpack_tokens: NULL argument");
    if (id_bits != 16 && id_bits != 32 && id_bits != 64) return fail(MBPE_ERR_ARG, "id_bits must be 16, 32 or 64");
    if (token_bits != 16 && token_bits != 32) return fail(MBPE_ERR_ARG, "token_bits must be 16 or 32");
    if (seq_len == 0) return fail(MBPE_ERR_ARG, "seq_len must be at least 1");
    if (n_rows >> 40) return fail(MBPE_ERR_ARG, "more than 2^40 rows");
    if (token_bits == 16 && id_bits != 16) return fail(MBPE_ERR_VOCAB, "token_bits 16 with wider ids");
    try {
        return unpack_run(device_id, ids, n_rows, seq_len, id_bits, ids_on_device, len, tokens_out, cap, token_bits,
                          out_on_device, doc_tok_off_out, n_out);
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_unpack_tokens: host allocation failed");
    }
}

int mbpe_pack_kernel_ms(float *ms_out) {
    if (!ms_out) return fail(MBPE_ERR_ARG, "mbpe_pack_kernel_ms: NULL argument");
    *ms_out = g_pack_ms;
    return MBPE_OK;
}

}  // extern "C"
