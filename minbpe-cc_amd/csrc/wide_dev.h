// Device helpers that the kernels of the 32-bit training loop share (wide.hip, wide_resident.hip, wide_regions.hip): the concurrent
// insert-or-add and the lookup of the 64-bit-key pair table, the (count, ~key) order of the argmax and its wave and
// workgroup reductions, the bitmap hash of the `first` tie-break and the match test of a merge.  See wide.h.
#ifndef MBPE_WIDE_DEV_H
#define MBPE_WIDE_DEV_H

#include "wide.h"

namespace mbpe {

// create_or_modify_pair, PairCount.h:249-260: find the pair and add `delta`, or insert it with `delta`.  Entries are
// never removed.  Concurrent inserts of one key meet at the same free slot and the CAS lets exactly one of them in.
// Returns the slot (the resident kernel keeps bounds per slice of slots), ~0 with kWideErrFull when the table is full.
__device__ inline uint32_t wide_add(const WideTable &t, WideCtl *ctl, unsigned long long key, int32_t delta,
                                    int32_t *old_out = nullptr) {
    uint32_t h = pair_hash(key, t.shift);
    for (uint32_t probe = 0; probe <= t.mask; ++probe) {
        unsigned long long k = t.keys[h];
        if (k == kWideEmpty) {
            k = atomicCAS(&t.keys[h], kWideEmpty, key);
            if (k == kWideEmpty) {
                atomicAdd(&ctl->n_entries, 1u);
                k = key;
            }
        }
        if (k == key) {
            const int32_t old = atomicAdd(&t.cnts[h], delta);
            if (old_out) *old_out = old;
            return h;
        }
        h = (h + 1) & t.mask;
    }
    atomicOr(&ctl->err, kWideErrFull);
    return ~0u;
}

// count of `key`, or -1 when the pair was never inserted
__device__ __forceinline__ int32_t wide_lookup(const WideTable &t, unsigned long long key) {
    uint32_t h = pair_hash(key, t.shift);
    for (uint32_t probe = 0; probe <= t.mask; ++probe) {
        const unsigned long long k = t.keys[h];
        if (k == key) return t.cnts[h];
        if (k == kWideEmpty) return -1;
        h = (h + 1) & t.mask;
    }
    return -1;
}

// ---- argmax: (count desc, first asc, second asc) = the larger of (count, ~key) -------------------------------
constexpr int kWideArgBlocks = 1024;      // workgroups of the scan = partials the final stage reduces (wide.hip, wide_regions.hip)
struct Cand128 { long long count; unsigned long long nkey; };      // count = -1: nothing
__device__ __forceinline__ bool better(const Cand128 &a, const Cand128 &b) {
    return a.count > b.count || (a.count == b.count && a.nkey > b.nkey);
}
__device__ __forceinline__ Cand128 wave_best(Cand128 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Cand128 o;
        o.count = ((long long)__shfl_xor((int)(v.count >> 32), d, kWave) << 32) | (uint32_t)__shfl_xor((int)v.count, d, kWave);
        o.nkey = ((unsigned long long)(uint32_t)__shfl_xor((int)(v.nkey >> 32), d, kWave) << 32) |
                 (uint32_t)__shfl_xor((int)v.nkey, d, kWave);
        if (better(o, v)) v = o;
    }
    return v;
}
__device__ __forceinline__ Cand128 block_best(Cand128 v, Cand128 *sh) {
    v = wave_best(v);
    __syncthreads();
    if (lane_id() == 0) sh[threadIdx.x / kWave] = v;
    __syncthreads();
    Cand128 r = sh[0];
    for (uint32_t w = 1; w < blockDim.x / kWave; ++w)
        if (better(sh[w], r)) r = sh[w];
    return r;
}

// ---- `first` tie-break: the bit of a pair in the 64-Kibit bitmap of the tied pairs --------------------------------
__device__ __forceinline__ uint32_t first_bit(unsigned long long key) { return pair_hash(key, 48); }   // 16 bits

// ---- one merge: does (t, nx) match (a, b)? ---------------------------------------------------------------------
__device__ __forceinline__ bool is_cand(uint32_t t, uint32_t nx, uint32_t a, uint32_t b) {
    return !(t & kTokEnd) && t == a && (nx & kTokIdMask) == b;      // (t carries no end flag here, so t == a compares ids)
}

}  // namespace mbpe

#endif
