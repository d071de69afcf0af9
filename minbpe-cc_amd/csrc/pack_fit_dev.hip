// Best-fit packing planned on the device: see pack_fit_dev.h.  gfx950, wave64.
//
// The rule (mbpe.h) takes the tails by size descending, then document ascending, and gives each to the open row with the
// smallest free >= its size, lowest row first.  Within the class of size s the sequential planner takes the rows with
// free >= s in (free, row) order, and a row with room f takes floor(f / s) consecutive tails before the next row is
// looked at; then new rows open and take floor(S / s) each.  Only the last row touched can keep free >= s.  So the
// dependency runs over the S - 1 classes, and inside a class everything is arithmetic on ranks:
//
//   k_fit_split    chip-wide, a lane per document: q_d and the sort key S - r_d; r_d into a workgroup's LDS histogram,
//                  flushed once (as hist.hip does); the span sums of q_d
//   k_fit_scan / k_fit_offsets   span.h's 64-bit scan: the first full row of every document, F = their number
//   k_fit_count    ONE workgroup, the class loop on counts: how many rows sit at each free value does not depend on
//                  which rows they are.  It leaves the rows ever appended to each bucket (a bucket = the rows of one free
//                  value) as an exclusive scan -- every bucket owns a fixed slice of one flat array -- and the new rows
//   k_fit_radix_*  the stable order of the documents by (S - r, d): LSD radix sort, 8-bit digits, a wave per span of 1,024
//                  keys with its own 256 counters, ranks inside a wave by ballot.  One pass for seq_len < 256, else two
//   k_fit_place    ONE workgroup of 1,024, the class loop with row numbers.  head / tail of every bucket and the class
//                  histogram live in LDS.  A bucket is appended to in any order (LDS atomics on tail) and sorted by row when
//                  it is first consumed: in LDS by counting smaller elements up to kFitLdsSort rows, above that by a
//                  workgroup-wide radix sort through global memory.  It emits one SEGMENT per row touched: (row, rank of
//                  its first tail, col0, pieces the row held before); its work follows the rows touched, not the tails
//   k_fit_full / k_fit_assign / k_fit_len   chip-wide: full pieces by binary search over the documents' first rows,
//                  every tail by binary search over the segments, len from a row's last piece
// Row numbers of tail rows are kept relative to F in 32 bits; the pieces a row holds are counted in the 64-bit cells of
// row_first itself, which the scan then turns into row_first in place.
#include "pack_fit_dev.h"

#include "span.h"

#include <algorithm>

namespace mbpe {
namespace {

constexpr int kFitThreads = 1024;                       // the one workgroup of k_fit_count and k_fit_place
constexpr int kFitWaves = kFitThreads / kWave;
constexpr uint32_t kFitMaxSeq = MBPE_FIT_DEVICE_MAX_SEQ;
constexpr uint32_t kFitLdsSort = 2048;                  // rows of a bucket that are sorted in LDS
constexpr uint32_t kFitSplitGrid = 512;

// ctl: what the kernels leave for each other and for the host (64-bit words)
enum { kCtlFull = 0, kCtlTails, kCtlNew, kCtlClasses, kCtlSegs, kCtlSorted, kCtlErr, kCtlWords = 8 };

struct FitSeg { uint32_t row, first, col0, idx; };      // row relative to F; idx: pieces the row held before

// ---- split ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSpanThreads) void k_fit_split(const unsigned long long *__restrict__ doc_off, uint64_t n_docs,
                                                             uint32_t S, uint32_t nbe, unsigned long long *__restrict__ q_out,
                                                             uint32_t *__restrict__ key_out, uint32_t *__restrict__ hist,
                                                             unsigned long long *__restrict__ span_cnt) {
    __shared__ uint32_t s_bin[kFitMaxSeq];
    for (uint32_t i = threadIdx.x; i < S; i += kSpanThreads) s_bin[i] = 0;
    __syncthreads();
    const uint32_t lane = lane_id();
    const uint64_t n_spans = span_count(n_docs);
    for (uint64_t span = span_index(); span < n_spans; span += (uint64_t)gridDim.x * kSpanWaves) {
        unsigned long long sum = 0;
        for (int it = 0; it < kSpanIters; ++it) {
            const uint64_t d = span * kSpan + (uint64_t)it * kWave + lane;
            if (d < n_docs) {
                const FitQR x = pack_fit_qr(doc_off[d + 1] - doc_off[d], S, nbe);
                q_out[d] = x.q;
                key_out[d] = S - x.r;                            // r == 0: behind every tail
                if (x.r) atomicAdd(&s_bin[x.r], 1u);
                sum += x.q;
            }
        }
        for (int k = kWave / 2; k > 0; k >>= 1) sum += __shfl_down(sum, k, kWave);
        if (lane == 0) span_cnt[span] = sum;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < S; i += kSpanThreads) {
        const uint32_t c = s_bin[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

// the sums of cnt over the spans (the rows' piece counts)
__global__ __launch_bounds__(kSpanThreads) void k_fit_span_sums(const unsigned long long *__restrict__ cnt, uint64_t n,
                                                                 unsigned long long *__restrict__ span_cnt) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    unsigned long long sum = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        if (i < n) sum += cnt[i];
    }
    for (int k = kWave / 2; k > 0; k >>= 1) sum += __shfl_down(sum, k, kWave);
    if (lane == 0) span_cnt[span] = sum;
}

__global__ __launch_bounds__(kScanThreads) void k_fit_scan(unsigned long long *__restrict__ span_cnt, uint64_t n_spans,
                                                            unsigned long long *__restrict__ total, unsigned long long add) {
    __shared__ unsigned long long sh[kScanThreads];
    const unsigned long long sum = span_scan_sum64(span_cnt, n_spans, sh);
    if (threadIdx.x == 0) *total = sum + add;
}

// cnt[i] becomes add + cnt[0] + .. + cnt[i - 1], in place
__global__ __launch_bounds__(kSpanThreads) void k_fit_offsets(unsigned long long *__restrict__ cnt, uint64_t n,
                                                               const unsigned long long *__restrict__ span_off,
                                                               unsigned long long add) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    unsigned long long o = span_off[span] + add;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        const unsigned long long w = i < n ? cnt[i] : 0ull;
        const unsigned long long incl = wave_prefix64(w, lane);
        if (i < n) cnt[i] = o + incl - w;
        o += __shfl(incl, kWave - 1, kWave);
    }
}

// ---- the order of the tails -------------------------------------------------------------------------------------------
// the lanes of the wave that are valid and hold this lane's digit
__device__ __forceinline__ unsigned long long wave_match8(uint32_t digit, bool valid) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long B = __ballot(bit);
        m &= bit ? B : ~B;
    }
    return m;
}

// counts[digit * n_spans + span]: a scan over them is the first place of every (digit, span)
__global__ __launch_bounds__(kSpanThreads) void k_fit_radix_hist(const uint32_t *__restrict__ key, uint64_t n, uint32_t shift,
                                                                  unsigned long long *__restrict__ counts, uint64_t n_spans) {
    __shared__ uint32_t s_cnt[kSpanWaves][256];
    const uint32_t lane = lane_id(), w = threadIdx.x / kWave;
    const uint64_t span = span_index(), base = span * kSpan;
    for (uint32_t i = lane; i < 256; i += kWave) s_cnt[w][i] = 0;
    __syncthreads();
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        if (i < n) atomicAdd(&s_cnt[w][(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (span < n_spans)
        for (uint32_t i = lane; i < 256; i += kWave) counts[(uint64_t)i * n_spans + span] = s_cnt[w][i];
}

// pay_in NULL: the payload of element i is i
__global__ __launch_bounds__(kSpanThreads) void k_fit_radix_scatter(const uint32_t *__restrict__ key, const uint32_t *__restrict__ pay_in,
                                                                     uint64_t n, uint32_t shift,
                                                                     const unsigned long long *__restrict__ offs, uint64_t n_spans,
                                                                     uint32_t *__restrict__ key_out, uint32_t *__restrict__ pay_out) {
    __shared__ unsigned long long s_off[kSpanWaves][256];
    const uint32_t lane = lane_id(), w = threadIdx.x / kWave;
    const uint64_t span = span_index(), base = span * kSpan;
    const unsigned long long lt = lanes_below(lane);
    if (span < n_spans)
        for (uint32_t i = lane; i < 256; i += kWave) s_off[w][i] = offs[(uint64_t)i * n_spans + span];
    __syncthreads();
    for (int it = 0; it < kSpanIters; ++it) {                    // (every wave of the workgroup: the barriers)
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        const bool valid = i < n;
        const uint32_t k = valid ? key[i] : 0u, digit = (k >> shift) & 255u;
        const unsigned long long M = wave_match8(digit, valid);
        const unsigned long long at = valid ? s_off[w][digit] + (unsigned long long)__popcll(M & lt) : 0ull;
        __syncthreads();
        if (valid && (M & lt) == 0ull) s_off[w][digit] += (unsigned long long)__popcll(M);   // the digit's first lane
        __syncthreads();
        if (valid) {                                             // (at < n: the offsets are a permutation's)
            key_out[at] = k;
            pay_out[at] = pay_in ? pay_in[i] : (uint32_t)i;
        }
    }
}

// ---- the class loop -------------------------------------------------------------------------------------------------
// inclusive prefix sum of v over the workgroup's threads, the sum of all in *total; sh: kFitWaves entries.  Every thread
// calls it (two barriers; the first frees sh from its use before)
__device__ __forceinline__ unsigned long long fit_block_scan(unsigned long long v, unsigned long long *sh,
                                                             unsigned long long *total) {
    const uint32_t lane = lane_id(), w = threadIdx.x / kWave;
    const unsigned long long incl = wave_prefix64(v, lane);
    __syncthreads();
    if (lane == kWave - 1) sh[w] = incl;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (uint32_t i = 0; i < (uint32_t)kFitWaves; ++i) {
        const unsigned long long x = sh[i];
        if (i < w) before += x;
        all += x;
    }
    *total = all;
    return before + incl;
}

// One chunk of a class: this thread's bucket holds c rows that can take k tails each; m tails in the class, `done` of
// them placed before the chunk (the same in every thread).  take: the rows of the bucket that take tails, in row order;
// first: the class's tails before them; *done_out: placed after the chunk
struct FitTake { uint32_t take, first; };
__device__ __forceinline__ FitTake fit_take(uint32_t c, uint32_t k, uint32_t m, unsigned long long done,
                                            unsigned long long *sh, unsigned long long *done_out) {
    const unsigned long long cap = (unsigned long long)c * k;
    unsigned long long all;
    const unsigned long long before = done + fit_block_scan(cap, sh, &all) - cap;
    *done_out = done + all < m ? done + all : m;
    if (!c || before >= m) return {0u, 0u};
    const unsigned long long rows = (m - before + k - 1) / k;
    return {rows < c ? (uint32_t)rows : c, (uint32_t)before};
}

// hist: tails per size; bstart[f] <- the rows appended to the buckets below f, ever; ctl <- F, tails, new rows, classes
__global__ __launch_bounds__(kFitThreads) void k_fit_count(const uint32_t *__restrict__ hist, uint32_t S,
                                                            uint32_t *__restrict__ bstart,
                                                            const unsigned long long *__restrict__ full,
                                                            unsigned long long *__restrict__ ctl) {
    __shared__ uint32_t s_hist[kFitMaxSeq], s_cnt[kFitMaxSeq], s_app[kFitMaxSeq];
    __shared__ unsigned long long sh[kFitWaves];
    __shared__ unsigned long long s_new;
    const uint32_t tid = threadIdx.x;
    unsigned long long tails = 0, all;
    for (uint32_t i = tid; i < S; i += kFitThreads) {
        const uint32_t h = i ? hist[i] : 0u;
        s_hist[i] = h;
        s_cnt[i] = 0;
        s_app[i] = 0;
        tails += h;
    }
    if (tid == 0) s_new = 0;
    (void)fit_block_scan(tails, sh, &all);
    tails = all;
    uint32_t classes = 0;
    for (uint32_t s = S - 1; s >= 1 && S > 1; --s) {
        const uint32_t m = s_hist[s];
        if (!m) continue;
        ++classes;
        unsigned long long done = 0;
        for (uint32_t f0 = s; f0 < S && done < m; f0 += kFitThreads) {
            const uint32_t f = f0 + tid, c = f < S ? s_cnt[f] : 0u, k = f < S ? f / s : 1u;
            unsigned long long next;
            const FitTake t = fit_take(c, k, m, done, sh, &next);
            if (t.take) {
                const unsigned long long cap = (unsigned long long)t.take * k;
                const uint32_t got = cap < m - t.first ? (uint32_t)cap : m - t.first;
                const uint32_t whole = got / k, part = got - whole * k;    // rows that took k; tails of the last one
                atomicSub(&s_cnt[f], t.take);
                if (whole && f > k * s) { atomicAdd(&s_cnt[f - k * s], whole); atomicAdd(&s_app[f - k * s], whole); }
                if (part) { atomicAdd(&s_cnt[f - part * s], 1u); atomicAdd(&s_app[f - part * s], 1u); }
            }
            done = next;
        }
        if (done < m && tid == 0) {                              // new rows
            const uint32_t rem = m - (uint32_t)done, k = S / s, whole = rem / k, part = rem - whole * k;
            // (atomics: other threads may still be adding the chunk's rows)
            if (whole && S > k * s) { atomicAdd(&s_cnt[S - k * s], whole); atomicAdd(&s_app[S - k * s], whole); }
            if (part) { atomicAdd(&s_cnt[S - part * s], 1u); atomicAdd(&s_app[S - part * s], 1u); }
            s_new += whole + (part ? 1u : 0u);
        }
        __syncthreads();
    }
    // every bucket's slice
    unsigned long long carry = 0;
    for (uint32_t f0 = 0; f0 < S; f0 += kFitThreads) {
        const uint32_t f = f0 + tid, a = f < S ? s_app[f] : 0u;
        const unsigned long long incl = fit_block_scan(a, sh, &all);
        if (f < S) bstart[f] = (uint32_t)(carry + incl - a);
        carry += all;
    }
    if (tid == 0) {
        ctl[kCtlFull] = *full;
        ctl[kCtlTails] = tails;
        ctl[kCtlNew] = s_new;
        ctl[kCtlClasses] = classes;
    }
}

// a[0 .. n) ascending, n <= kFitLdsSort: every element counts the smaller ones (row numbers differ)
__device__ __forceinline__ void fit_sort_lds(uint32_t *a, uint32_t n, uint32_t *buf) {
    for (uint32_t i = threadIdx.x; i < n; i += kFitThreads) buf[i] = a[i];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += kFitThreads) {
        const uint32_t v = buf[i];
        uint32_t r = 0;
        for (uint32_t j = 0; j < n; ++j) r += buf[j] < v;
        a[r] = v;
    }
    __syncthreads();
}

// a[0 .. n) ascending through tmp[0 .. n): LSD radix sort by the whole workgroup, `bits` key bits.  A pass: histogram
// (LDS atomics), the bins' first places, then the elements 1,024 at a time in order -- the rank inside a wave by ballot,
// the waves before by their counts
__device__ __forceinline__ void fit_sort_global(uint32_t *a, uint32_t *tmp, uint32_t n, uint32_t bits, uint32_t *s_base,
                                                uint32_t (*s_wcnt)[256]) {
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid / kWave;
    const unsigned long long lt = lanes_below(lane);
    uint32_t *src = a, *dst = tmp;
    for (uint32_t shift = 0; shift < bits; shift += 8) {
        if (tid < 256) s_base[tid] = 0;
        for (uint32_t i = tid; i < kFitWaves * 256; i += kFitThreads) s_wcnt[i / 256][i % 256] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += kFitThreads) atomicAdd(&s_base[(src[i] >> shift) & 255u], 1u);
        __syncthreads();
        if (tid == 0) {
            uint32_t at = 0;
            for (uint32_t b = 0; b < 256; ++b) { const uint32_t c = s_base[b]; s_base[b] = at; at += c; }
        }
        __syncthreads();
        for (uint32_t i0 = 0; i0 < n; i0 += kFitThreads) {
            const uint32_t i = i0 + tid;
            const bool valid = i < n;
            const uint32_t v = valid ? src[i] : 0u, digit = (v >> shift) & 255u;
            const unsigned long long M = wave_match8(digit, valid);
            if (valid && (M & lt) == 0ull) s_wcnt[w][digit] = (uint32_t)__popcll(M);
            __syncthreads();
            if (valid) {
                uint32_t at = s_base[digit] + (uint32_t)__popcll(M & lt);
                for (uint32_t x = 0; x < w; ++x) at += s_wcnt[x][digit];
                dst[at] = v;                                     // (at < n: a permutation)
            }
            __syncthreads();
            if (tid < 256) {
                uint32_t c = 0;
                for (uint32_t x = 0; x < (uint32_t)kFitWaves; ++x) { c += s_wcnt[x][tid]; s_wcnt[x][tid] = 0; }
                s_base[tid] += c;
            }
            __syncthreads();
        }
        uint32_t *t = src; src = dst; dst = t;
    }
    if (src != a) {
        for (uint32_t i = tid; i < n; i += kFitThreads) a[i] = src[i];
        __syncthreads();
    }
}

// brow: the buckets' slices (bstart); tmp: as large; row_np[rel row]: pieces the row holds (64-bit: the cells of row_first).
// cap: entries of brow, tmp and segs; n_new: rows of row_np.  k_fit_count has counted both, so nothing can pass them; an
// index that would is not written and raises ctl[kCtlErr] instead
__global__ __launch_bounds__(kFitThreads) void k_fit_place(const uint32_t *__restrict__ hist, const uint32_t *__restrict__ bstart,
                                                            uint32_t S, uint32_t row_bits, uint32_t *brow, uint32_t *tmp,
                                                            FitSeg *__restrict__ segs, unsigned long long *row_np,
                                                            uint32_t cap, uint32_t n_new_rows,
                                                            unsigned long long *__restrict__ ctl) {
    __shared__ uint32_t s_hist[kFitMaxSeq], s_head[kFitMaxSeq], s_tail[kFitMaxSeq];
    __shared__ uint32_t s_dirty[kFitMaxSeq / 32];
    __shared__ uint32_t s_buf[kFitLdsSort];
    __shared__ uint32_t s_rowpre[kFitThreads + 1], s_first[kFitThreads], s_list[kFitThreads];
    __shared__ uint32_t s_base[256], s_wcnt[kFitWaves][256];
    __shared__ unsigned long long sh[kFitWaves];
    __shared__ uint32_t s_nlist;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < S; i += kFitThreads) {
        s_hist[i] = i ? hist[i] : 0u;
        s_head[i] = s_tail[i] = bstart[i];
    }
    for (uint32_t i = tid; i < kFitMaxSeq / 32; i += kFitThreads) s_dirty[i] = 0;
    if (tid == 0) s_nlist = 0;
    __syncthreads();
    uint32_t cbase = 0, n_segs = 0, next_row = 0;                // (the same in every thread)
    unsigned long long sorted = 0;
    auto append = [&](uint32_t g, uint32_t row) {
        const uint32_t at = atomicAdd(&s_tail[g], 1u);
        if (at < cap) brow[at] = row; else ctl[kCtlErr] = 1;
        atomicOr(&s_dirty[g / 32], 1u << (g % 32));
    };
    for (uint32_t s = S - 1; s >= 1 && S > 1; --s) {
        const uint32_t m = s_hist[s];
        if (!m) continue;
        unsigned long long done = 0;
        for (uint32_t f0 = s; f0 < S && done < m; f0 += kFitThreads) {
            const uint32_t f = f0 + tid, c = f < S ? s_tail[f] - s_head[f] : 0u, k = f < S ? f / s : 1u;
            unsigned long long next, rows_all;
            const FitTake t = fit_take(c, k, m, done, sh, &next);
            const unsigned long long rows_incl = fit_block_scan(t.take, sh, &rows_all);
            s_rowpre[tid] = (uint32_t)(rows_incl - t.take);
            s_first[tid] = t.first;
            if (tid == 0) s_rowpre[kFitThreads] = (uint32_t)rows_all;
            if (t.take && c > 1 && (s_dirty[f / 32] >> (f % 32) & 1u)) s_list[atomicAdd(&s_nlist, 1u)] = f;
            __syncthreads();
            // the buckets that are consumed for the first time since rows came in: by row
            const uint32_t n_list = s_nlist;
            for (uint32_t x = 0; x < n_list; ++x) {
                const uint32_t g = s_list[x], lo = s_head[g], n = s_tail[g] - lo;
                if (n <= kFitLdsSort) fit_sort_lds(brow + lo, n, s_buf);
                else fit_sort_global(brow + lo, tmp + lo, n, row_bits, s_base, s_wcnt);
                sorted += n;
            }
            if (t.take) atomicAnd(&s_dirty[f / 32], ~(1u << (f % 32)));
            __syncthreads();
            if (tid == 0) s_nlist = 0;
            // the rows that take tails, bucket after bucket in row order: a segment each
            const uint32_t R = (uint32_t)rows_all;
            for (uint32_t j = tid; j < R; j += kFitThreads) {
                uint32_t lo = 0, hi = kFitThreads;                // s_rowpre[lo] <= j < s_rowpre[hi]
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) / 2;
                    if (s_rowpre[mid] <= j) lo = mid; else hi = mid;
                }
                const uint32_t fb = f0 + lo, kb = fb / s, i = j - s_rowpre[lo];
                const uint32_t at = s_head[fb] + i;             // (inside the bucket's slice: i < its rows)
                const uint32_t row = at < cap ? brow[at] : n_new_rows;
                if (row >= n_new_rows || n_segs + j >= cap) { ctl[kCtlErr] = 1; continue; }
                const uint32_t first = s_first[lo] + i * kb;     // (< m)
                const uint32_t got = m - first < kb ? m - first : kb;
                const unsigned long long np = row_np[row];
                segs[n_segs + j] = {row, cbase + first, S - fb, (uint32_t)np};
                row_np[row] = np + got;
                if (fb > got * s) append(fb - got * s, row);
            }
            __syncthreads();
            if (t.take) s_head[f] += t.take;
            n_segs += R;
            done = next;
            __syncthreads();
        }
        if (done < m) {                                          // new rows, ascending numbers
            const uint32_t rem = m - (uint32_t)done, k = S / s, n_new = (rem + k - 1) / k;
            for (uint32_t j = tid; j < n_new; j += kFitThreads) {
                const uint32_t row = next_row + j, first = (uint32_t)done + j * k;
                const uint32_t got = m - first < k ? m - first : k;
                if (row >= n_new_rows || n_segs + j >= cap) { ctl[kCtlErr] = 1; continue; }
                segs[n_segs + j] = {row, cbase + first, 0u, 0u};
                row_np[row] = got;
                if (S > got * s) append(S - got * s, row);
            }
            next_row += n_new;
            n_segs += n_new;
            __syncthreads();
        }
        cbase += m;
    }
    if (tid == 0) {
        ctl[kCtlSegs] = n_segs;
        ctl[kCtlSorted] = sorted;
    }
}

// ---- the table ----------------------------------------------------------------------------------------------------------
struct FitOut {
    PackFitPiece *pieces;
    unsigned long long *row_first;
    unsigned long long *doc_row;
    uint32_t *doc_col;
    uint32_t *len;                                               // NULL: not asked for
};

// full piece p = row p: its document by binary search over the documents' first full rows (n_docs + 1 entries)
__global__ __launch_bounds__(256) void k_fit_full(const unsigned long long *__restrict__ full, uint64_t n_docs, uint64_t F,
                                                   uint32_t S, FitOut o) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < F; p += stride) {
        uint64_t lo = 0, hi = n_docs;                            // full[lo] <= p < full[hi]
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (full[mid] <= p) lo = mid; else hi = mid;
        }
        o.pieces[p] = {lo, (p - full[lo]) * S, 0u, S};
        o.row_first[p] = p;
        if (o.len) o.len[p] = S;
    }
}

// the document at place t of the order: a tail (t < the tails) finds its segment, the others have none
__global__ __launch_bounds__(256) void k_fit_assign(const unsigned long long *__restrict__ doc_off,
                                                     const unsigned long long *__restrict__ full, const uint32_t *__restrict__ order,
                                                     uint64_t n_docs, uint32_t S, uint32_t nbe, const FitSeg *__restrict__ segs,
                                                     const unsigned long long *__restrict__ ctl, FitOut o) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t F = ctl[kCtlFull], n_tails = ctl[kCtlTails], n_segs = ctl[kCtlSegs];
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_docs; t += stride) {
        const uint64_t d = order ? order[t] : t;
        const unsigned long long q = full[d + 1] - full[d];
        if (t >= n_tails) {
            o.doc_row[d] = q ? full[d + 1] - 1 : kPackFitNoRow;
            o.doc_col[d] = 0;
            continue;
        }
        const FitQR x = pack_fit_qr(doc_off[d + 1] - doc_off[d], S, nbe);
        uint64_t lo = 0, hi = n_segs;                            // segs[lo].first <= t < segs[hi].first
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (segs[mid].first <= t) lo = mid; else hi = mid;
        }
        const FitSeg g = segs[lo];
        const uint32_t i = (uint32_t)t - g.first, col = g.col0 + i * x.r;
        const uint64_t row = F + g.row;
        const uint64_t at = g.row < ctl[kCtlNew] ? o.row_first[row] + g.idx + i : ~0ull;
        if (at >= F + n_tails) continue;                         // (never: the rows' piece counts sum to the tails)
        o.pieces[at] = {d, q * S, col, x.r};
        o.doc_row[d] = row;
        o.doc_col[d] = col;
    }
}

__global__ __launch_bounds__(256) void k_fit_len(uint64_t F, uint64_t n_rows, FitOut o) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = F + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += stride) {
        const PackFitPiece last = o.pieces[o.row_first[r + 1] - 1];
        o.len[r] = last.col0 + last.size;
    }
}

uint32_t flat_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), 1u << 16); }

// the workspace, cut into 16-byte aligned parts
struct Carve {
    uint8_t *base;
    uint64_t at = 0;
    template <typename T> T *take(uint64_t n) {
        T *p = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += (n * sizeof(T) + 15) & ~15ull;
        return p;
    }
};

struct FitWs {
    unsigned long long *ctl, *full, *span_cnt, *rcount, *doc_row;
    uint32_t *hist, *bstart, *key[2], *pay[2], *brow, *tmp, *doc_col;
    FitSeg *segs;
    uint64_t bytes;
};

FitWs fit_ws(uint8_t *base, uint64_t n, uint32_t S) {
    Carve c{base};
    FitWs w;
    const uint64_t n_spans = span_count(n);
    w.ctl = c.take<unsigned long long>(kCtlWords);               // (ctl and hist: cleared together)
    w.hist = c.take<uint32_t>(S);
    w.bstart = c.take<uint32_t>(S);
    w.full = c.take<unsigned long long>(n + 1);
    w.span_cnt = c.take<unsigned long long>(n_spans + 1);
    for (int i = 0; i < 2; ++i) { w.key[i] = c.take<uint32_t>(n); w.pay[i] = c.take<uint32_t>(n); }
    w.rcount = c.take<unsigned long long>(256 * n_spans);
    w.brow = c.take<uint32_t>(n);                                // (rows appended <= segments <= tails <= documents)
    w.tmp = c.take<uint32_t>(n);
    w.segs = c.take<FitSeg>(n);
    w.doc_row = c.take<unsigned long long>(n);
    w.doc_col = c.take<uint32_t>(n);
    w.bytes = c.at;
    return w;
}

}  // namespace

#define FCHK(expr) MBPE_HIP_CHECK(expr, mem.clear_last)

int pack_fit_dev_plan(hipStream_t stream, DevAlloc &mem, PackFitDev *w, const unsigned long long *d_doc_off,
                      uint64_t n_docs, uint32_t seq_len, uint32_t nbe, bool want_len, DevBuf<uint8_t> *d_pieces,
                      DevBuf<unsigned long long> *d_rows, uint64_t *n_rows_out, bool *served) {
    const uint32_t S = seq_len;
    const uint64_t n = n_docs, n_spans = span_count(n);
    *served = false;
    *n_rows_out = 0;
    if (!n) {                                                    // no document, no row
        const uint64_t none[4] = {1, 0, 0, 0};
        std::copy(none, none + 4, w->stats);
        *served = true;
        return MBPE_OK;
    }
    int rc = w->ws.reserve(fit_ws(nullptr, n, S).bytes, mem);
    if (rc != MBPE_OK) return rc;
    const FitWs b = fit_ws(w->ws.get(), n, S);
    w->doc_row = b.doc_row;
    w->doc_col = b.doc_col;
    FCHK(hipMemsetAsync(b.ctl, 0, (uint64_t)((uint8_t *)(b.hist + S) - (uint8_t *)b.ctl), stream));
    const dim3 spans(span_grid(n)), span_block(kSpanThreads), one(1), scan_block(kScanThreads), fit_block(kFitThreads);
    hipLaunchKernelGGL(k_fit_split, dim3(std::min<uint32_t>(span_grid(n), kFitSplitGrid)), span_block, 0, stream, d_doc_off,
                       n, S, nbe, b.full, b.key[0], b.hist, b.span_cnt);
    hipLaunchKernelGGL(k_fit_scan, one, scan_block, 0, stream, b.span_cnt, n_spans, b.full + n, 0ull);
    hipLaunchKernelGGL(k_fit_offsets, spans, span_block, 0, stream, b.full, n, b.span_cnt, 0ull);
    hipLaunchKernelGGL(k_fit_count, one, fit_block, 0, stream, b.hist, S, b.bstart, b.full + n, b.ctl);
    unsigned long long ctl[kCtlWords];
    FCHK(hipMemcpyAsync(ctl, b.ctl, sizeof(ctl), hipMemcpyDeviceToHost, stream));
    FCHK(hipStreamSynchronize(stream));
    FCHK(hipGetLastError());
    const uint64_t F = ctl[kCtlFull], n_tails = ctl[kCtlTails], n_new = ctl[kCtlNew], n_rows = F + n_new;
    if (n_rows >= (1ull << 32)) return MBPE_OK;                  // (the host planner has the 2^40 check)
    rc = d_pieces->reserve(std::max<uint64_t>(F + n_tails, 1) * sizeof(PackFitPiece), mem);
    if (rc == MBPE_OK) rc = d_rows->reserve((n_rows + 1) * 8, mem);
    if (rc == MBPE_OK && want_len) rc = w->d_len.reserve(std::max<uint64_t>(n_rows, 1) * 4, mem);
    if (rc != MBPE_OK) return rc;
    const uint32_t *order = nullptr;
    if (n_tails) {
        const int passes = S > 255 ? 2 : 1;                      // (keys 1 .. S)
        for (int p = 0; p < passes; ++p) {
            const uint32_t shift = 8 * p;
            hipLaunchKernelGGL(k_fit_radix_hist, spans, span_block, 0, stream, b.key[p & 1], n, shift, b.rcount, n_spans);
            hipLaunchKernelGGL(k_fit_scan, one, scan_block, 0, stream, b.rcount, 256 * n_spans, b.span_cnt + n_spans, 0ull);
            hipLaunchKernelGGL(k_fit_radix_scatter, spans, span_block, 0, stream, b.key[p & 1],
                               p ? b.pay[p & 1] : (const uint32_t *)nullptr, n, shift, b.rcount, n_spans, b.key[~p & 1],
                               b.pay[~p & 1]);
        }
        order = b.pay[passes & 1];
        uint32_t row_bits = 8;
        while (row_bits < 32 && (n_new >> row_bits)) row_bits += 8;
        hipLaunchKernelGGL(k_fit_place, one, fit_block, 0, stream, b.hist, b.bstart, S, row_bits, b.brow, b.tmp, b.segs,
                           d_rows->get() + F, (uint32_t)n, (uint32_t)n_new, b.ctl);
    }
    // the rows' piece counts -> row_first, in place; row_first[n_rows] = F + the tails
    if (n_new) hipLaunchKernelGGL(k_fit_span_sums, dim3(span_grid(n_new)), span_block, 0, stream, d_rows->get() + F, n_new, b.span_cnt);
    hipLaunchKernelGGL(k_fit_scan, one, scan_block, 0, stream, b.span_cnt, span_count(n_new), d_rows->get() + n_rows, F);
    if (n_new) hipLaunchKernelGGL(k_fit_offsets, dim3(span_grid(n_new)), span_block, 0, stream, d_rows->get() + F, n_new, b.span_cnt, F);
    const FitOut o = {reinterpret_cast<PackFitPiece *>(d_pieces->get()), d_rows->get(), b.doc_row, b.doc_col,
                      want_len ? w->d_len.get() : nullptr};
    if (F) hipLaunchKernelGGL(k_fit_full, dim3(flat_grid(F)), dim3(256), 0, stream, b.full, n, F, S, o);
    hipLaunchKernelGGL(k_fit_assign, dim3(flat_grid(n)), dim3(256), 0, stream, d_doc_off, b.full, order, n, S, nbe, b.segs,
                       b.ctl, o);
    if (want_len && n_new) hipLaunchKernelGGL(k_fit_len, dim3(flat_grid(n_new)), dim3(256), 0, stream, F, n_rows, o);
    FCHK(hipMemcpyAsync(ctl, b.ctl, sizeof(ctl), hipMemcpyDeviceToHost, stream));
    FCHK(hipStreamSynchronize(stream));
    FCHK(hipGetLastError());
    if (ctl[kCtlErr]) return fail(MBPE_ERR_STATE, "fit planner: the count and the placement disagree");
    w->stats[0] = 1;
    w->stats[1] = n_tails;
    w->stats[2] = ctl[kCtlClasses];
    w->stats[3] = ctl[kCtlSorted];
    *n_rows_out = n_rows;
    *served = true;
    return MBPE_OK;
}

}  // namespace mbpe
