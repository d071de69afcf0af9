// Device helpers that dedup.hip and wordcount.hip share: the workgroup prefix, the end-mask reader, and the three
// kernels that turn an end mask into the end offset of every chunk.  Everything is in an unnamed namespace: each of the
// two translation units gets its own copy of the kernels.
#ifndef MBPE_DEDUP_DEV_H
#define MBPE_DEDUP_DEV_H

#include "dedup.h"

#include <hip/hip_runtime.h>

namespace mbpe {
namespace {

constexpr int kDdThreads = 256;
constexpr int kDdWaves = kDdThreads / kWave;

// the end bits of bytes 64 w .. 64 w + 63, those at and beyond n_bytes cleared (w < ceil(n_bytes / 64))
__device__ __forceinline__ unsigned long long mask_word(const uint32_t *__restrict__ m32, uint64_t w, uint64_t n_bytes) {
    unsigned long long v = (unsigned long long)m32[2 * w] | ((unsigned long long)m32[2 * w + 1] << 32);
    const uint64_t left = n_bytes - w * 64;
    if (left < 64) v &= (1ull << left) - 1ull;
    return v;
}

// exclusive prefix of v over the workgroup's kDdThreads threads, the workgroup's sum in *total; sh: kDdWaves words
__device__ __forceinline__ unsigned long long block_excl(unsigned long long v, unsigned long long *sh,
                                                         unsigned long long *total) {
    const uint32_t lane = lane_id(), wave = threadIdx.x / kWave;
    const unsigned long long incl = wave_prefix64(v, lane);
    __syncthreads();                              // (sh may still be read from an earlier call)
    if (lane == kWave - 1) sh[wave] = incl;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)kDdWaves; ++w) {
        const unsigned long long s = sh[w];
        if (w < wave) base += s;
        tot += s;
    }
    *total = tot;
    return base + incl - v;
}

__global__ __launch_bounds__(kDdThreads) void k_dd_tile_count(const uint32_t *__restrict__ m32, uint64_t n_bytes,
                                                              uint64_t n_words, unsigned long long *__restrict__ tile_cnt) {
    __shared__ unsigned long long sh[kDdWaves];
    const uint64_t w = (uint64_t)blockIdx.x * kDdThreads + threadIdx.x;
    const unsigned long long v = w < n_words ? (unsigned long long)__popcll(mask_word(m32, w, n_bytes)) : 0ull;
    unsigned long long total;
    block_excl(v, sh, &total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// arr[i] becomes arr[0] + .. + arr[i - 1]; the total goes to *total_out
__global__ __launch_bounds__(kScanThreads) void k_dd_scan(unsigned long long *arr, uint64_t n,
                                                          unsigned long long *total_out) {
    __shared__ unsigned long long sh[kScanThreads];
    const unsigned long long total = span_scan_sum64(arr, n, sh);
    if (threadIdx.x == 0) *total_out = total;
}

__global__ __launch_bounds__(kDdThreads) void k_dd_chunk_ends(const uint32_t *__restrict__ m32, uint64_t n_bytes,
                                                              uint64_t n_words, const unsigned long long *__restrict__ tile_off,
                                                              uint64_t n_chunks, unsigned long long *__restrict__ cend) {
    __shared__ unsigned long long sh[kDdWaves];
    const uint64_t w = (uint64_t)blockIdx.x * kDdThreads + threadIdx.x;
    unsigned long long m = w < n_words ? mask_word(m32, w, n_bytes) : 0ull;
    unsigned long long total;
    uint64_t rank = tile_off[blockIdx.x] + block_excl((unsigned long long)__popcll(m), sh, &total);
    for (; m; m &= m - 1, ++rank)
        if (rank < n_chunks) cend[rank] = w * 64 + (uint64_t)__builtin_ctzll(m) + 1;      // (the count's own mask: always)
}

__device__ __forceinline__ void chunk_range(const unsigned long long *__restrict__ cend, uint64_t c, uint64_t *start,
                                            uint64_t *len) {
    const uint64_t s = c ? cend[c - 1] : 0;
    *start = s;
    *len = cend[c] - s;
}

// n bytes from src to dst, in 16-byte pieces where the two are aligned alike: src_at and dst_at are the positions of
// src and dst in buffers that are 16-byte aligned
__device__ __forceinline__ void copy_chunk(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint64_t dst_at,
                                           uint64_t src_at, uint64_t len) {
    uint64_t i = 0;
    if (((src_at ^ dst_at) & 15) == 0) {
        for (; i < len && ((dst_at + i) & 15); ++i) dst[i] = src[i];
        for (; i + 16 <= len; i += 16) *reinterpret_cast<uint4 *>(dst + i) = *reinterpret_cast<const uint4 *>(src + i);
    }
    for (; i < len; ++i) dst[i] = src[i];
}

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kDdThreads - 1) / kDdThreads); }
inline uint64_t mask_bytes_for(uint64_t n_bytes) { return (n_bytes + 15) / 16 * 2 + 16; }

}  // namespace
}  // namespace mbpe

#endif
