// Expansion on the device: see expand.h.  gfx950, wave64.
//
//   k_exp_count    per span of 1,024 chunks (one wave): the tokens its chunks copy, 64 bits
//   k_exp_scan     one workgroup: the tokens before every span, and all of them (the host reads that before it
//                  launches the write kernel: an output that is too small is never written to)
//   k_exp_write    per span: prefix sums of the run lengths and the runs' table positions into LDS, then OUTPUT-centric
//                  copying as k_dec_write does it: a lane owns a piece of 16 aligned output bytes, finds the chunk that
//                  holds the piece's first element by binary search and gathers on from there.  No run is walked by
//                  one lane: a chunk of a million tokens is 250,000 pieces like any others.  With ENDS also the output
//                  position after every chunk
//   k_exp_before   the tokens before a few given chunks (document boundaries): the span's offset and a walk of part of
//                  one span, one wave each
//   k_exp_patch    the chunks that are one token by rule become runs of their own behind the unique chunks' runs
//
// The table of the workloads this is for (a few thousand distinct chunks) stays in the caches; unique_of is read once
// by k_exp_count and once by k_exp_write, the output is written once.
#include "expand.h"

#include <hip/hip_runtime.h>

#include <type_traits>

namespace mbpe {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// two spans per workgroup: a span's prefix sums and table positions are 16 KiB of LDS, and 64 KiB is a workgroup's most
constexpr int kExpWaves = 2;
constexpr int kExpThreads = kExpWaves * kWave;
__device__ __forceinline__ uint64_t exp_span_index() { return (uint64_t)blockIdx.x * kExpWaves + threadIdx.x / kWave; }
uint32_t exp_grid(uint64_t n_spans) { return (uint32_t)((n_spans + kExpWaves - 1) / kExpWaves); }

struct ExpTab {
    const unsigned long long *ends;
    uint64_t n_entries;
    const uint32_t *unique_of;
    uint64_t n_chunks;
};

__global__ __launch_bounds__(kExpThreads) void k_exp_count(ExpTab t, uint64_t n_spans,
                                                            unsigned long long *__restrict__ span_cnt) {
    const uint64_t span = exp_span_index(), c0 = span * kExpSpan;
    if (span > n_spans) return;                     // (span n_spans holds no chunk: its 0 is the scan's last entry)
    const uint32_t lane = lane_id();
    unsigned long long s = 0;
    for (int it = 0; it < kExpIters; ++it) {
        const uint64_t c = c0 + (uint64_t)it * kWave + lane;
        if (c < t.n_chunks) s += expand_run_len(t.ends, t.n_entries, t.unique_of[c]);
    }
    for (int d = kWave / 2; d > 0; d >>= 1) s += __shfl_down(s, d, kWave);
    if (lane == 0) span_cnt[span] = s;
}

__global__ __launch_bounds__(kScanThreads) void k_exp_scan(unsigned long long *__restrict__ span_cnt, uint64_t n,
                                                           unsigned long long *__restrict__ total) {
    __shared__ unsigned long long sh[kScanThreads];
    const unsigned long long sum = span_scan_sum64(span_cnt, n, sh);
    if (threadIdx.x == 0) *total = sum;
}

template <typename T, bool ENDS>
__global__ __launch_bounds__(kExpThreads) void k_exp_write(const T *__restrict__ table, uint64_t n_table, ExpTab t,
                                                            const unsigned long long *__restrict__ span_off,
                                                            T *__restrict__ out,
                                                            unsigned long long *__restrict__ chunk_ends,
                                                            unsigned long long base) {
    __shared__ unsigned long long s_pre[kExpWaves][kExpSpan + 1];
    __shared__ unsigned long long s_start[kExpWaves][kExpSpan];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint64_t span = exp_span_index(), c0 = span * kExpSpan;
    const bool active = c0 < t.n_chunks;
    const unsigned long long o = active ? span_off[span] : 0ull;
    if (active) {
        unsigned long long run = 0;
        for (int it = 0; it < kExpIters; ++it) {
            const uint32_t i = (uint32_t)it * kWave + lane;
            const uint64_t c = c0 + i;
            const uint64_t j = c < t.n_chunks ? t.unique_of[c] : t.n_entries;
            const unsigned long long l = expand_run_len(t.ends, t.n_entries, j);
            const unsigned long long incl = wave_prefix64(l, lane);
            s_pre[w][i + 1] = run + incl;
            s_start[w][i] = expand_run_start(t.ends, t.n_entries, j);
            if (ENDS && c < t.n_chunks) chunk_ends[c] = base + o + run + incl;
            run += __shfl(incl, kWave - 1, kWave);
        }
        if (lane == 0) s_pre[w][0] = 0;
    }
    __syncthreads();
    if (!active || out == nullptr) return;          // (no output: a query that only asks for the chunks' ends)
    const unsigned long long *pre = s_pre[w], *start = s_start[w];
    const unsigned long long total = pre[kExpSpan];
    if (total == 0) return;
    constexpr uint32_t kPer = kExpPiece / sizeof(T);
    T *dst = out + o;
    const ExpandPieces pc = expand_pieces((uint64_t)(uintptr_t)dst, total, sizeof(T));
    if (lane < pc.head) {                           // up to the first boundary: shared with the span before
        uint32_t r = expand_find(pre, lane);
        dst[lane] = expand_elem(table, n_table, pre, start, lane, &r);
    }
    for (uint64_t v = lane; v < pc.n_vec; v += kWave) {
        const unsigned long long p0 = pc.head + v * kPer;
        uint32_t r = expand_find(pre, p0);
        T piece[kPer];
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) piece[k] = expand_elem(table, n_table, pre, start, p0 + k, &r);
        u32x4 q;
        __builtin_memcpy(&q, piece, kExpPiece);
        *static_cast<u32x4 *>(__builtin_assume_aligned(dst + p0, kExpPiece)) = q;
    }
    if (lane < pc.tail) {                           // behind the last boundary: shared with the span after
        const unsigned long long p = pc.head + pc.n_vec * kPer + lane;
        uint32_t r = expand_find(pre, p);
        dst[p] = expand_elem(table, n_table, pre, start, p, &r);
    }
}

__global__ __launch_bounds__(256) void k_exp_before(ExpTab t, const unsigned long long *__restrict__ span_off,
                                                    const unsigned long long *__restrict__ chunk_idx, uint64_t n,
                                                    unsigned long long *__restrict__ tok_before) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
    if (i >= n) return;                             // (whole waves leave together)
    const uint32_t lane = lane_id();
    const uint64_t idx = chunk_idx[i] < t.n_chunks ? chunk_idx[i] : t.n_chunks;
    const uint64_t span = idx / kExpSpan;           // (<= n_spans: span_off has that entry)
    unsigned long long s = 0;
    for (uint64_t c = span * kExpSpan + lane; c < idx; c += kWave) s += expand_run_len(t.ends, t.n_entries, t.unique_of[c]);
    for (int d = kWave / 2; d > 0; d >>= 1) s += __shfl_down(s, d, kWave);
    if (lane == 0) tok_before[i] = span_off[span] + s;
}

template <typename T>
__global__ __launch_bounds__(256) void k_exp_patch(T *__restrict__ table, uint64_t n_table_before,
                                                   unsigned long long *__restrict__ ends, uint64_t n_first,
                                                   uint32_t *__restrict__ unique_of, uint64_t n_chunks, ExpandSingles sg) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) ends[n_first + sg.n_single] = n_table_before + sg.n_single;      // the empty run
    if (k >= sg.n_single) return;
    table[n_table_before + k] = (T)sg.tok[k];
    ends[n_first + k] = n_table_before + k + 1;
    const uint64_t f = sg.first[k], l = sg.last[k] < n_chunks ? sg.last[k] : n_chunks;
    if (f >= n_chunks) return;
    unique_of[f] = (uint32_t)(n_first + k);
    for (uint64_t c = f + 1; c < l; ++c) unique_of[c] = (uint32_t)(n_first + sg.n_single);
}

ExpTab tab_of(const ExpandSrc &s) { return {s.ends, s.n_entries, s.unique_of, s.n_chunks}; }

}  // namespace

void expand_count_launch(hipStream_t stream, const ExpandSrc &src, unsigned long long *span_off, unsigned long long *total) {
    const uint64_t n_spans = expand_span_count(src.n_chunks);
    hipLaunchKernelGGL(k_exp_count, dim3(exp_grid(n_spans + 1)), dim3(kExpThreads), 0, stream, tab_of(src), n_spans, span_off);
    hipLaunchKernelGGL(k_exp_scan, dim3(1), dim3(kScanThreads), 0, stream, span_off, n_spans + 1, total);
}

void expand_write_launch(hipStream_t stream, const ExpandSrc &src, const unsigned long long *span_off, void *out,
                         unsigned long long *chunk_ends, unsigned long long base) {
    const uint64_t n_spans = expand_span_count(src.n_chunks);
    if (n_spans == 0) return;
    const dim3 grid(exp_grid(n_spans)), block(kExpThreads);
    auto launch = [&](auto elem, auto with_ends) {
        using T = decltype(elem);
        hipLaunchKernelGGL((k_exp_write<T, decltype(with_ends)::value>), grid, block, 0, stream,
                           static_cast<const T *>(src.table), src.n_table, tab_of(src), span_off, static_cast<T *>(out),
                           chunk_ends, base);
    };
    if (src.elem_bits == 16) {
        if (chunk_ends) launch(uint16_t(), std::true_type()); else launch(uint16_t(), std::false_type());
    } else {
        if (chunk_ends) launch(uint32_t(), std::true_type()); else launch(uint32_t(), std::false_type());
    }
}

void expand_before_launch(hipStream_t stream, const ExpandSrc &src, const unsigned long long *span_off,
                          const unsigned long long *chunk_idx, uint64_t n, unsigned long long *tok_before) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_exp_before, dim3((uint32_t)((n * kWave + 255) / 256)), dim3(256), 0, stream, tab_of(src), span_off,
                       chunk_idx, n, tok_before);
}

void expand_patch_launch(hipStream_t stream, void *table, uint64_t n_table_before, uint32_t elem_bits,
                         unsigned long long *ends, uint64_t n_first, uint32_t *unique_of, uint64_t n_chunks,
                         const ExpandSingles &sg) {
    const dim3 grid((uint32_t)((sg.n_single + 256) / 256)), block(256);
    if (elem_bits == 16)
        hipLaunchKernelGGL(k_exp_patch<uint16_t>, grid, block, 0, stream, static_cast<uint16_t *>(table), n_table_before,
                           ends, n_first, unique_of, n_chunks, sg);
    else
        hipLaunchKernelGGL(k_exp_patch<uint32_t>, grid, block, 0, stream, static_cast<uint32_t *>(table), n_table_before,
                           ends, n_first, unique_of, n_chunks, sg);
}

}  // namespace mbpe
