// The span machinery of the 32-bit token streams (encode.hip, wide.hip, decode.hip).
//
// Layout: 32-bit tokens, bit 31 = "last token of its chunk", all-ones = nothing.  A span = 1,024 consecutive tokens =
// the unit one wave walks (16 groups of 64 lanes; ballots give the group masks), 4 spans per 256-thread workgroup.
// Spans are linked by two single-workgroup scans: the parity of the run of candidates that reaches a span, and the
// offsets of the tokens a span keeps.
//
// A left-to-right walk that takes a candidate and then skips its right neighbour takes candidate i  <=>  r[i], the
// number of consecutive candidates immediately before i, is even.  Everything that computes r's parity is here, as
// functions on integers and 64-bit masks that a host compiler builds too (tests/test_span_cpu.py runs them).
#ifndef MBPE_SPAN_H
#define MBPE_SPAN_H

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MBPE_HD __host__ __device__ inline
#else
#define MBPE_HD inline
#endif

namespace mbpe {

constexpr uint32_t kTokEnd = 0x80000000u;       // last token of its chunk
constexpr uint32_t kTokNone = 0xFFFFFFFFu;      // no token: hole, no candidate, nothing for the next stream
constexpr uint32_t kTokIdMask = 0x7FFFFFFFu;
constexpr int kWave = 64;
constexpr int kSpan = 1024;                     // tokens one wave walks
constexpr int kSpanIters = kSpan / kWave;
constexpr int kSpanThreads = 256;               // 4 waves = 4 spans per workgroup
constexpr int kSpanWaves = kSpanThreads / kWave;
constexpr int kScanThreads = 1024;              // the one workgroup of a scan over the spans

MBPE_HD uint64_t span_count(uint64_t n) { return (n + kSpan - 1) / kSpan; }
inline uint32_t span_grid(uint64_t n) { return (uint32_t)((span_count(n) + kSpanWaves - 1) / kSpanWaves); }

// the hash of a (first << 32 | second) pair key; tests/encode_cases.py mirrors it as enc_hash
MBPE_HD uint32_t pair_hash(unsigned long long key, uint32_t shift) {
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> shift);
}

// ---- run parity: pure arithmetic ------------------------------------------------------------------------------
// parity of the run of candidates at the top of the group with candidate mask M, which continues a run of parity
// `carry` when the whole group is candidates (a full group adds 64: parity unchanged; ~M != 0 where clzll is asked)
MBPE_HD uint32_t run_carry(unsigned long long M, uint32_t carry) {
    return M != ~0ull ? (uint32_t)__builtin_clzll(~M) & 1u : carry;
}

// the lanes below `lane` (< 64) as a mask; loop-invariant, so a kernel forms it once outside its loop
MBPE_HD unsigned long long lanes_below(uint32_t lane) { return (1ull << lane) - 1ull; }

// r = consecutive candidates immediately below `lane`, continuing into `carry` when all of them are; lt = lanes_below(lane)
MBPE_HD uint32_t run_below(unsigned long long M, unsigned long long lt, uint32_t lane, uint32_t carry) {
    const unsigned long long zeros_below = ~M & lt;
    if (zeros_below == 0ull) return lane + carry;
    return lane - 1u - (63u - (uint32_t)__builtin_clzll(zeros_below));
}

// what a stretch of positions is to the scan: are all of them candidates, and the parity of its trailing run
struct SpanSum { uint32_t all, par; };
MBPE_HD SpanSum span_empty() { return {1u, 0u}; }      // nothing: a (full, even) stretch
MBPE_HD uint32_t span_pack(SpanSum s) { return s.all | (s.par << 1); }
MBPE_HD SpanSum span_unpack(uint32_t v) { return {v & 1u, v >> 1}; }

// a span's summary after one more group
MBPE_HD SpanSum span_add_group(SpanSum s, unsigned long long M) {
    return {M != ~0ull ? 0u : s.all, run_carry(M, s.par)};
}

// L then R; associative, which is what lets a scan cut the spans into slices  [a full span has even length]
MBPE_HD SpanSum span_fold(SpanSum L, SpanSum R) { return R.all ? SpanSum{L.all, L.par ^ R.par} : R; }

// the fold of the packed summaries span_sum[lo .. hi): the first sweep of the parity scan
MBPE_HD SpanSum span_fold_slice(const uint32_t *span_sum, uint64_t lo, uint64_t hi) {
    SpanSum acc = span_empty();
    for (uint64_t s = lo; s < hi; ++s) acc = span_fold(acc, span_unpack(span_sum[s]));
    return acc;
}

// ---- 64-bit sums over the spans: pure arithmetic (token byte offsets: a span's bytes, not its tokens) ------------
// the sum of cnt[lo .. hi)
MBPE_HD unsigned long long span_sum_slice64(const unsigned long long *cnt, uint64_t lo, uint64_t hi) {
    unsigned long long s = 0;
    for (uint64_t i = lo; i < hi; ++i) s += cnt[i];
    return s;
}

// off[i] = start + cnt[lo] + .. + cnt[i - 1] for i in [lo, hi); returns start + the slice's sum.  off may be cnt
MBPE_HD unsigned long long span_offsets_slice64(const unsigned long long *cnt, unsigned long long *off, uint64_t lo,
                                                uint64_t hi, unsigned long long start) {
    for (uint64_t i = lo; i < hi; ++i) {
        const unsigned long long v = cnt[i];
        off[i] = start;
        start += v;
    }
    return start;
}

// the slice of spans scan thread t owns: [*lo, *hi)
MBPE_HD void span_scan_slice(uint64_t n_spans, uint32_t t, uint64_t *lo, uint64_t *hi) {
    const uint64_t per = (n_spans + kScanThreads - 1) / kScanThreads;
    *lo = per * t < n_spans ? per * t : n_spans;
    *hi = *lo + per < n_spans ? *lo + per : n_spans;
}

// the first index in idx[0 .. n) (ascending) whose value is not below v
MBPE_HD uint64_t lower_bound64(const unsigned long long *idx, uint64_t n, unsigned long long v) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (idx[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

#ifdef __HIPCC__
// ---- wave helpers ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & (kWave - 1); }
__device__ __forceinline__ uint64_t span_index() { return (uint64_t)blockIdx.x * kSpanWaves + threadIdx.x / kWave; }

// lanes of the wave for which `keep` holds: how many, and how many of them below this lane; lt = lanes_below(lane)
struct WaveKeep { uint32_t rank, count; };
__device__ __forceinline__ WaveKeep wave_keep(bool keep, unsigned long long lt) {
    const unsigned long long K = __ballot(keep);
    return {(uint32_t)__popcll(K & lt), (uint32_t)__popcll(K)};
}
__device__ __forceinline__ uint32_t wave_count(bool keep) { return (uint32_t)__popcll(__ballot(keep)); }

// tok[i] and, in *next, its right neighbour (lane 63 fetches its own: no holes between two groups or two spans);
// `oob` stands for every position at or beyond n
__device__ __forceinline__ uint32_t load_pair(const uint32_t *__restrict__ tok, uint64_t i, uint64_t n, uint32_t lane,
                                              uint32_t oob, uint32_t *next) {
    const uint32_t t = i < n ? tok[i] : oob;
    uint32_t nx = __shfl_down(t, 1, kWave);
    if (lane == kWave - 1) nx = i + 1 < n ? tok[i + 1] : oob;
    *next = nx;
    return t;
}

// ---- scans over the spans: one workgroup of kScanThreads, two sweeps; sh = kScanThreads elements of LDS ----------
// Thread t owns ceil(n_spans / kScanThreads) consecutive spans; the fold across the threads is serial.
// Every thread of the workgroup has to call them (two barriers each).

// in_par[s] = parity of the run of candidates right before span s
__device__ __forceinline__ void span_scan_parity(const uint32_t *__restrict__ span_sum, uint64_t n_spans,
                                                 uint32_t *__restrict__ in_par, uint32_t *sh) {
    const uint64_t per = (n_spans + kScanThreads - 1) / kScanThreads;
    const uint64_t lo = per * threadIdx.x, hi = lo + per < n_spans ? lo + per : n_spans;
    sh[threadIdx.x] = span_pack(span_fold_slice(span_sum, lo, hi));
    __syncthreads();
    if (threadIdx.x == 0) {
        SpanSum acc = span_empty();            // nothing before the text
        for (int t = 0; t < kScanThreads; ++t) {
            const SpanSum v = span_unpack(sh[t]);
            sh[t] = acc.par;                   // parity of the run of candidates right before slice t
            acc = span_fold(acc, v);
        }
    }
    __syncthreads();
    SpanSum acc = {0u, sh[threadIdx.x]};
    for (uint64_t s = lo; s < hi; ++s) {
        in_par[s] = acc.par;
        acc = span_fold(acc, span_unpack(span_sum[s]));
    }
}

// off[s] = cnt[0] + .. + cnt[s - 1]; returns the total in thread 0 (only there)
__device__ __forceinline__ unsigned long long span_scan_sum(const uint32_t *__restrict__ cnt, uint64_t n_spans,
                                                            unsigned long long *__restrict__ off,
                                                            unsigned long long *sh) {
    const uint64_t per = (n_spans + kScanThreads - 1) / kScanThreads;
    const uint64_t lo = per * threadIdx.x, hi = lo + per < n_spans ? lo + per : n_spans;
    unsigned long long s = 0, total = 0;
    for (uint64_t i = lo; i < hi; ++i) s += cnt[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int t = 0; t < kScanThreads; ++t) { const unsigned long long v = sh[t]; sh[t] = total; total += v; }
    __syncthreads();
    s = sh[threadIdx.x];
    for (uint64_t i = lo; i < hi; ++i) { off[i] = s; s += cnt[i]; }
    return total;
}

// the same for 64-bit counts, in place: cnt[s] becomes cnt[0] + .. + cnt[s - 1]; returns the total in thread 0
__device__ __forceinline__ unsigned long long span_scan_sum64(unsigned long long *cnt, uint64_t n_spans,
                                                              unsigned long long *sh) {
    uint64_t lo, hi;
    span_scan_slice(n_spans, threadIdx.x, &lo, &hi);
    unsigned long long total = 0;
    sh[threadIdx.x] = span_sum_slice64(cnt, lo, hi);
    __syncthreads();
    if (threadIdx.x == 0)
        for (int t = 0; t < kScanThreads; ++t) { const unsigned long long v = sh[t]; sh[t] = total; total += v; }
    __syncthreads();
    span_offsets_slice64(cnt, cnt, lo, hi, sh[threadIdx.x]);
    return total;
}

// inclusive prefix sum of v over the wave's lanes
__device__ __forceinline__ unsigned long long wave_prefix64(unsigned long long v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned long long u = __shfl_up(v, d, kWave);
        if (lane >= (uint32_t)d) v += u;
    }
    return v;
}

// ---- compaction: the values of val[0 .. n) that are not kTokNone, in order, to out; span_off from span_scan_sum --
// CARRY: a second array travels with them, carry_out gets carry[i] wherever out gets val[i]
template <bool CARRY>
__device__ __forceinline__ void span_scatter_carry(const uint32_t *__restrict__ val, uint64_t n,
                                                   const unsigned long long *__restrict__ span_off,
                                                   uint32_t *__restrict__ out, const uint32_t *__restrict__ carry,
                                                   uint32_t *__restrict__ carry_out) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    const unsigned long long lt = lanes_below(lane);
    unsigned long long o = span_off[span];
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        const uint32_t v = i < n ? val[i] : kTokNone;
        const WaveKeep k = wave_keep(v != kTokNone, lt);
        if (v != kTokNone) {
            out[o + k.rank] = v;
            if (CARRY) carry_out[o + k.rank] = carry[i];
        }
        o += k.count;
    }
}

__device__ __forceinline__ void span_scatter(const uint32_t *__restrict__ val, uint64_t n,
                                             const unsigned long long *__restrict__ span_off,
                                             uint32_t *__restrict__ out) {
    span_scatter_carry<false>(val, n, span_off, out, nullptr, nullptr);
}
#endif  // __HIPCC__

}  // namespace mbpe

#endif
