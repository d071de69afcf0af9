// Token frequency tables on the device: see hist.h.  gfx950, wave64.
//
//   k_hist_tokens  the hot one.  A lane loads 16 aligned bytes (4 or 8 elements), a workgroup of 256 lanes takes a tile of
//                  4,096 positions per step and the tiles g, g + G, ...  Ids below kHistLocalIds go to a workgroup-private
//                  32-bit LDS table (ds_add, no return), which is flushed -- its non-zero entries only -- with 64-bit
//                  global atomics; ids from kHistLocalIds on and the ids beyond the table (per lane in a register, one
//                  atomic per wave at the end) go to global memory directly.  Token ids follow merge order, so on text
//                  nearly everything lands in LDS.  The cliff: when all tokens are EQUAL every lane of a wave adds to one
//                  LDS address and the adds of a wave-instruction run one after the other.
//   k_hist_runs    a lane per table element, its run by binary search in ends, a 64-bit global atomic of the run's
//                  weight (weights can be near 2^32 and more: nothing is privatised in 32 bits).  Not hot: the table
//                  holds every distinct chunk once.
//   k_hist_fold    kept[i] += repeat * call[i].
#include "hist.h"
#include "hip_host.h"

#include <algorithm>

namespace mbpe {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename T>
__global__ __launch_bounds__(kHistThreads) void k_hist_tokens(const u32x4 *__restrict__ pieces, uint64_t skip, uint64_t n,
                                                              uint64_t n_tiles, unsigned long long *__restrict__ counts,
                                                              uint64_t n_ids, unsigned long long *__restrict__ other) {
    __shared__ uint32_t s_bin[kHistLocalIds];
    constexpr uint32_t kPer = kHistPiece / sizeof(T);
    constexpr uint32_t kTilePieces = kHistTile / kPer, kRounds = kTilePieces / kHistThreads;
    const uint32_t n_local = n_ids < kHistLocalIds ? (uint32_t)n_ids : kHistLocalIds;
    const uint64_t g = blockIdx.x, G = gridDim.x, end = skip + n, n_pieces = (end + kPer - 1) / kPer;
    unsigned long long beyond = 0;
    for (uint64_t k0 = 0; g + k0 * G < n_tiles; k0 += kHistFlushTiles) {
        for (uint32_t i = threadIdx.x; i < n_local; i += kHistThreads) s_bin[i] = 0;
        __syncthreads();
        // at most kHistFlushTiles tiles of kHistTile positions: below 2^32 adds to any one counter (hist.h)
        for (uint64_t k = k0; k < k0 + kHistFlushTiles && g + k * G < n_tiles; ++k) {
            const uint64_t q0 = (g + k * G) * kTilePieces + threadIdx.x;
            u32x4 v[kRounds];
#pragma unroll
            for (uint32_t r = 0; r < kRounds; ++r) {
                const uint64_t q = q0 + (uint64_t)r * kHistThreads;
                v[r] = q < n_pieces ? pieces[q] : u32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (uint32_t r = 0; r < kRounds; ++r) {
                const uint64_t q = q0 + (uint64_t)r * kHistThreads, p0 = q * kPer;
                if (q >= n_pieces) continue;
                T e[kPer];
                __builtin_memcpy(e, &v[r], kHistPiece);
                const bool whole = p0 >= skip && p0 + kPer <= end;
#pragma unroll
                for (uint32_t x = 0; x < kPer; ++x) {
                    if (!whole && (p0 + x < skip || p0 + x >= end)) continue;
                    const uint32_t id = hist_id(e[x], sizeof(T));
                    if (id >= n_ids) ++beyond;                      // (never an address)
                    else if (id < kHistLocalIds) atomicAdd(&s_bin[id], 1u);
                    else atomicAdd(&counts[id], 1ull);
                }
            }
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_local; i += kHistThreads) {
            const uint32_t c = s_bin[i];
            if (c) atomicAdd(&counts[i], (unsigned long long)c);
        }
        __syncthreads();
    }
    for (int d = kWave / 2; d > 0; d >>= 1) beyond += __shfl_down(beyond, d, kWave);
    if (lane_id() == 0 && beyond) atomicAdd(other, beyond);
}

template <typename T>
__global__ __launch_bounds__(256) void k_hist_runs(const T *__restrict__ table, uint64_t n_table,
                                                   const unsigned long long *__restrict__ ends, uint64_t n_entries,
                                                   const unsigned long long *__restrict__ w,
                                                   unsigned long long *__restrict__ counts, uint64_t n_ids,
                                                   unsigned long long *__restrict__ other,
                                                   unsigned long long *__restrict__ total) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long beyond = 0, sum = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_table; p += stride) {
        const uint64_t j = hist_run_of(ends, n_entries, p);
        if (j >= n_entries) continue;
        const unsigned long long wt = w[j];
        if (wt == 0) continue;
        const uint32_t id = hist_id(table[p], sizeof(T));
        if (id < n_ids) atomicAdd(&counts[id], wt); else beyond += wt;
        sum += wt;
    }
    for (int d = kWave / 2; d > 0; d >>= 1) {
        beyond += __shfl_down(beyond, d, kWave);
        sum += __shfl_down(sum, d, kWave);
    }
    if (lane_id() == 0) {
        if (beyond) atomicAdd(other, beyond);
        if (sum) atomicAdd(total, sum);
    }
}

__global__ __launch_bounds__(256) void k_hist_fold(unsigned long long *__restrict__ kept,
                                                   const unsigned long long *__restrict__ call, uint64_t n,
                                                   unsigned long long repeat) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) kept[i] += repeat * call[i];
}

#define HCHK(expr) MBPE_HIP_CHECK(expr, true)

thread_local float g_hist_ms = 0.f;

// mbpe_token_counts after its checks: a stream and buffers of the call's own, released at its end
int token_counts_run(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                     uint64_t *counts_out, uint64_t n_ids, int out_on_device, uint64_t *n_other_out) {
    int rc = find_device(device_id);
    if (rc != MBPE_OK) return rc;
    DevQueue dev(true);
    if ((rc = dev.open(device_id)) != MBPE_OK) return rc;
    DevBuf<uint8_t> d_in;
    DevBuf<unsigned long long> d_cnt;
    const uint64_t in_bytes = n_tokens * (token_bits / 8);
    const void *d_tok = tokens;
    if (!tokens_on_device && n_tokens) {
        if ((rc = d_in.reserve(in_bytes, dev.mem)) != MBPE_OK) return rc;
        HCHK(hipMemcpyAsync(d_in, tokens, in_bytes, hipMemcpyHostToDevice, dev.stream));
        d_tok = d_in.get();
    }
    // a host table and `other` share one buffer; a device table is the caller's and `other` has 8 bytes of its own
    if ((rc = d_cnt.reserve(out_on_device ? 8 : (n_ids + 1) * 8, dev.mem)) != MBPE_OK) return rc;
    unsigned long long *counts = out_on_device ? reinterpret_cast<unsigned long long *>(counts_out) : d_cnt.get();
    unsigned long long *other = out_on_device ? d_cnt.get() : d_cnt.get() + n_ids;
    HCHK(hipMemsetAsync(counts, 0, n_ids * 8, dev.stream));
    HCHK(hipMemsetAsync(other, 0, 8, dev.stream));
    HCHK(hipEventRecord(dev.ev0, dev.stream));
    hist_tokens_launch(dev.stream, d_tok, n_tokens, token_bits, counts, n_ids, other);
    if ((rc = dev.finish(&g_hist_ms)) != MBPE_OK) return rc;
    if (!out_on_device) HCHK(hipMemcpyAsync(counts_out, counts, n_ids * 8, hipMemcpyDeviceToHost, dev.stream));
    unsigned long long n_other = 0;
    HCHK(hipMemcpyAsync(&n_other, other, 8, hipMemcpyDeviceToHost, dev.stream));
    HCHK(hipStreamSynchronize(dev.stream));
    *n_other_out = n_other;
    return MBPE_OK;
}

}  // namespace

void hist_tokens_launch(hipStream_t stream, const void *elems, uint64_t n, uint32_t elem_bits, unsigned long long *counts,
                        uint64_t n_ids, unsigned long long *other) {
    if (n == 0) return;
    const uint64_t addr = (uint64_t)(uintptr_t)elems, skip = hist_skip(addr, elem_bits / 8);
    const uint64_t n_tiles = hist_tile_count(skip, n);
    const u32x4 *pieces = reinterpret_cast<const u32x4 *>(addr & ~(uint64_t)(kHistPiece - 1));
    const dim3 grid(hist_group_count(n_tiles)), block(kHistThreads);
    if (elem_bits == 16)
        hipLaunchKernelGGL(k_hist_tokens<uint16_t>, grid, block, 0, stream, pieces, skip, n, n_tiles, counts, n_ids, other);
    else
        hipLaunchKernelGGL(k_hist_tokens<uint32_t>, grid, block, 0, stream, pieces, skip, n, n_tiles, counts, n_ids, other);
}

void hist_runs_launch(hipStream_t stream, const void *table, uint64_t n_table, uint32_t elem_bits,
                      const unsigned long long *ends, uint64_t n_entries, const unsigned long long *w,
                      unsigned long long *counts, uint64_t n_ids, unsigned long long *other, unsigned long long *total) {
    if (n_table == 0 || n_entries == 0) return;
    const dim3 grid((uint32_t)std::min<uint64_t>((n_table + 255) / 256, 4096)), block(256);
    if (elem_bits == 16)
        hipLaunchKernelGGL(k_hist_runs<uint16_t>, grid, block, 0, stream, static_cast<const uint16_t *>(table), n_table, ends,
                           n_entries, w, counts, n_ids, other, total);
    else
        hipLaunchKernelGGL(k_hist_runs<uint32_t>, grid, block, 0, stream, static_cast<const uint32_t *>(table), n_table, ends,
                           n_entries, w, counts, n_ids, other, total);
}

void hist_fold_launch(hipStream_t stream, unsigned long long *kept, const unsigned long long *call, uint64_t n,
                      unsigned long long repeat) {
    if (n == 0) return;
    const dim3 grid((uint32_t)std::min<uint64_t>((n + 255) / 256, 4096)), block(256);
    hipLaunchKernelGGL(k_hist_fold, grid, block, 0, stream, kept, call, n, repeat);
}

}  // namespace mbpe

extern "C" {

int mbpe_token_counts(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                      uint64_t *counts_out, uint64_t n_ids, int out_on_device, uint64_t *n_other_out) {
    using namespace mbpe;
    if (n_other_out) *n_other_out = 0;
    if (!counts_out || !n_other_out || (!tokens && n_tokens)) return fail(MBPE_ERR_ARG, "mbpe_token_counts: NULL argument");
    if (token_bits != 16 && token_bits != 32) return fail(MBPE_ERR_ARG, "token_bits must be 16 or 32");
    if (n_ids == 0 || n_ids > MBPE_MAX_COUNT_IDS) return fail(MBPE_ERR_ARG, "n_ids must lie in 1 .. MBPE_MAX_COUNT_IDS");
    if (n_tokens >> 40) return fail(MBPE_ERR_ARG, "more than 2^40 tokens");
    if (tokens_on_device && ((uint64_t)(uintptr_t)tokens % (token_bits / 8)))
        return fail(MBPE_ERR_ARG, "mbpe_token_counts: tokens in device memory must be aligned to their elements");
    if (out_on_device && ((uint64_t)(uintptr_t)counts_out % 8))
        return fail(MBPE_ERR_ARG, "mbpe_token_counts: counts_out in device memory must be 8-byte aligned");
    return token_counts_run(device_id, tokens, n_tokens, token_bits, tokens_on_device, counts_out, n_ids, out_on_device,
                            n_other_out);
}

int mbpe_token_counts_kernel_ms(float *ms_out) {
    if (!ms_out) return mbpe::fail(MBPE_ERR_ARG, "mbpe_token_counts_kernel_ms: NULL argument");
    *ms_out = mbpe::g_hist_ms;
    return MBPE_OK;
}

}  // extern "C"
