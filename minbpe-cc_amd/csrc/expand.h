// Expansion (expand.hip): the tokens of every chunk of a text, copied from a table of token runs that holds each
// distinct chunk once.  The encoder's "dedup" route (encode.hip) encodes the unique chunks a deduper (dedup.h) found,
// and this step writes every chunk's tokens to their place in the output.
//
//   table     the token runs one after the other, in the caller's output format: elements of 4 bytes (ids, or ids with
//             bit 31 on a chunk's last token) or of 2 bytes
//   ends      ends[j] = the table position after run j's last token; run j starts at ends[j - 1] (0 for j = 0).  A run may
//             be empty
//   unique_of unique_of[c] = the run that chunk c copies (an index at or beyond n_entries counts as an empty run)
//
// A SPAN is kExpSpan = 1,024 consecutive chunks, the unit one wave walks: a 64-bit token count per span, one scan over
// the spans (span_scan_sum64), and then per span: the prefix sums of its chunks' run lengths (64 bits: a chunk that
// passed the deduper unhashed may hold millions of tokens) and where each run starts in the table, both in LDS; the
// wave's lanes walk the span's OUTPUT range in pieces of 16 aligned bytes, each lane finds the chunk that holds its
// piece's first element by binary search in the prefix sums and gathers from there on.  The first and the last piece
// of a span are shared with its neighbours and stored element by element.
//
// This header is shared by the device code and by host programs: the index arithmetic, and expand_host, a plain
// restatement of the whole expansion through that arithmetic that tests/expand_check.cpp runs against a per-chunk
// concatenation.
#ifndef MBPE_EXPAND_H
#define MBPE_EXPAND_H

#include "span.h"

#include <stdint.h>

#ifndef __HIP_DEVICE_COMPILE__
#include <vector>
#endif

namespace mbpe {

constexpr int kExpSpan = 1024;                  // chunks one wave walks
constexpr int kExpIters = kExpSpan / kWave;
constexpr uint32_t kExpPiece = 16;              // bytes of an aligned store

MBPE_HD uint64_t expand_span_count(uint64_t n_chunks) { return (n_chunks + kExpSpan - 1) / kExpSpan; }

// run j of the table: where it starts and how many tokens it holds
MBPE_HD uint64_t expand_run_start(const unsigned long long *ends, uint64_t n_entries, uint64_t j) {
    return j < n_entries && j ? ends[j - 1] : 0;
}
MBPE_HD uint64_t expand_run_len(const unsigned long long *ends, uint64_t n_entries, uint64_t j) {
    if (j >= n_entries) return 0;
    const uint64_t s = j ? ends[j - 1] : 0;
    return ends[j] >= s ? ends[j] - s : 0;      // (ends ascend; anything else counts as nothing)
}

// How `total` elements of elem_bytes bytes that start at byte address addr (a multiple of elem_bytes) are stored:
// `head` elements one by one up to the first 16-byte boundary, n_vec whole pieces, `tail` elements one by one.
struct ExpandPieces { uint64_t head, n_vec, tail; };
MBPE_HD ExpandPieces expand_pieces(uint64_t addr, uint64_t total, uint32_t elem_bytes) {
    uint64_t head = ((kExpPiece - (addr & (kExpPiece - 1))) & (kExpPiece - 1)) / elem_bytes;
    if (head > total) head = total;
    const uint64_t per = kExpPiece / elem_bytes, rest = total - head;
    return {head, rest / per, rest % per};
}

// pre[0 .. kExpSpan] ascending with pre[0] = 0: the largest r < kExpSpan with pre[r] <= pos
MBPE_HD uint32_t expand_find(const unsigned long long *pre, unsigned long long pos) {
    uint32_t r = 0;
    for (uint32_t step = kExpSpan / 2; step; step >>= 1)
        if (pre[r + step] <= pos) r += step;
    return r;
}

// The element at position pos (< pre[kExpSpan]) of the span's output; *r = a chunk at or before the one that holds it
// (expand_find's answer, or what an earlier call with a smaller pos left), moved on to the one that does.  Table
// positions at or beyond n_table read as 0: a table and ends that disagree give wrong tokens, never a wrong address.
template <typename T>
MBPE_HD T expand_elem(const T *table, uint64_t n_table, const unsigned long long *pre, const unsigned long long *start,
                      unsigned long long pos, uint32_t *r) {
    uint32_t k = *r;
    while (k + 1 < (uint32_t)kExpSpan && pre[k + 1] <= pos) ++k;     // (skips empty runs; pos < pre[kExpSpan] ends it)
    *r = k;
    const unsigned long long src = start[k] + (pos - pre[k]);
    return src < n_table ? table[src] : (T)0;
}

#ifndef __HIP_DEVICE_COMPILE__
// The whole expansion on the host, span by span as the device walks it: the counts, their sums, and every span's
// output range through expand_pieces / expand_find / expand_elem.  out_addr: the byte address the output is taken to
// start at (only its low 4 bits matter: they decide where the pieces fall).  chunk_ends (optional): the output
// position after every chunk's last token.
template <typename T>
inline std::vector<T> expand_host(const T *table, uint64_t n_table, const unsigned long long *ends, uint64_t n_entries,
                                  const uint32_t *unique_of, uint64_t n_chunks, uint64_t out_addr,
                                  std::vector<uint64_t> *chunk_ends) {
    const uint64_t n_spans = expand_span_count(n_chunks);
    std::vector<unsigned long long> span_off(n_spans + 1, 0);
    for (uint64_t s = 0; s < n_spans; ++s) {
        unsigned long long cnt = 0;
        for (uint64_t c = s * kExpSpan; c < n_chunks && c < (s + 1) * kExpSpan; ++c)
            cnt += expand_run_len(ends, n_entries, unique_of[c]);
        span_off[s] = cnt;
    }
    const unsigned long long total = span_offsets_slice64(span_off.data(), span_off.data(), 0, n_spans + 1, 0);
    std::vector<T> out(total);
    if (chunk_ends) chunk_ends->assign(n_chunks, 0);
    std::vector<unsigned long long> pre(kExpSpan + 1), start(kExpSpan);
    for (uint64_t s = 0; s < n_spans; ++s) {
        pre[0] = 0;
        for (uint64_t i = 0; i < (uint64_t)kExpSpan; ++i) {
            const uint64_t c = s * kExpSpan + i;
            const uint64_t j = c < n_chunks ? unique_of[c] : n_entries;
            start[i] = expand_run_start(ends, n_entries, j);
            pre[i + 1] = pre[i] + expand_run_len(ends, n_entries, j);
            if (chunk_ends && c < n_chunks) (*chunk_ends)[c] = span_off[s] + pre[i + 1];
        }
        const unsigned long long T_span = pre[kExpSpan], o = span_off[s];
        const ExpandPieces pc = expand_pieces(out_addr + o * sizeof(T), T_span, sizeof(T));
        const uint64_t per = kExpPiece / sizeof(T);
        for (uint64_t h = 0; h < pc.head; ++h) {
            uint32_t r = expand_find(pre.data(), h);
            out[o + h] = expand_elem(table, n_table, pre.data(), start.data(), h, &r);
        }
        for (uint64_t v = 0; v < pc.n_vec; ++v) {
            const unsigned long long p0 = pc.head + v * per;
            uint32_t r = expand_find(pre.data(), p0);
            for (uint64_t k = 0; k < per; ++k) out[o + p0 + k] = expand_elem(table, n_table, pre.data(), start.data(), p0 + k, &r);
        }
        for (uint64_t t = 0; t < pc.tail; ++t) {
            const unsigned long long p = pc.head + pc.n_vec * per + t;
            uint32_t r = expand_find(pre.data(), p);
            out[o + p] = expand_elem(table, n_table, pre.data(), start.data(), p, &r);
        }
    }
    return out;
}
#endif  // !__HIP_DEVICE_COMPILE__

#ifdef __HIPCC__
// ---- the launchers (expand.hip); everything named is device memory, nothing is waited for ----------------------------
struct ExpandSrc {
    const void *table;                     // n_table elements of elem_bits bits
    uint64_t n_table;
    const unsigned long long *ends;        // n_entries
    uint64_t n_entries;
    const uint32_t *unique_of;             // n_chunks
    uint64_t n_chunks;
    uint32_t elem_bits;                    // 16 or 32
};

// span_off[0 .. n_spans] (n_spans = expand_span_count(n_chunks)): the output tokens before every span, [n_spans] = all
// of them, which also go to *total
void expand_count_launch(hipStream_t stream, const ExpandSrc &src, unsigned long long *span_off, unsigned long long *total);

// the tokens to `out` (aligned to its elements; span_off[n_spans] elements are written, the caller has checked that
// they fit) and, where chunk_ends is not NULL, base + the output position after every chunk's last token
void expand_write_launch(hipStream_t stream, const ExpandSrc &src, const unsigned long long *span_off, void *out,
                         unsigned long long *chunk_ends, unsigned long long base);

// tok_before[i] = the output tokens of the chunks before chunk chunk_idx[i] (<= n_chunks), for i < n
void expand_before_launch(hipStream_t stream, const ExpandSrc &src, const unsigned long long *span_off,
                          const unsigned long long *chunk_idx, uint64_t n, unsigned long long *tok_before);

// The one-token chunks: run n_first + k of the table becomes the one token tok[k] (flags included, as the table's
// format has them), which chunk first[k] copies from then on; the chunks first[k] + 1 .. last[k] - 1 (what else the
// mask cuts the single's bytes into) copy the empty run n_first + n_single.  table has room for n_table_before +
// n_single elements, ends for n_first + n_single + 1 entries; chunk indices at or beyond n_chunks are ignored.
struct ExpandSingles {
    const uint32_t *tok;
    const unsigned long long *first, *last;
    uint64_t n_single;
};
void expand_patch_launch(hipStream_t stream, void *table, uint64_t n_table_before, uint32_t elem_bits,
                         unsigned long long *ends, uint64_t n_first, uint32_t *unique_of, uint64_t n_chunks,
                         const ExpandSingles &sg);
#endif  // __HIPCC__

}  // namespace mbpe

#endif
