// The 32-bit training loop on wave-owned regions, two launches per merge: see wide_regions.h.  gfx950, wave64.
#include "wide_regions.h"
#include "wide_walk.h"

#include <hip/hip_runtime.h>

namespace mbpe {
namespace {

constexpr int kRegThreads = 256;                       // 4 waves = 4 regions per workgroup
constexpr int kRegWaves = kRegThreads / kWave;
constexpr int kRegPosBlocks = 1024;                    // `first`: the waves stride over the regions, in stream order

__device__ __forceinline__ uint32_t reg_load(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long reg_load(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The ticket of a launch.  Every workgroup calls it once, all its threads, AFTER it has made its part of the launch's
// result: the part is fenced to the device, thread 0 draws, and the workgroup that drew the last ticket -- every other
// part was fenced before its own draw -- gets true, behind a fence of its own, and reads the parts with reg_load.
// It puts the ticket back to 0 for the next launch.  No workgroup waits for another.
__device__ __forceinline__ bool reg_last_workgroup(uint32_t *ticket, uint32_t *sh_last) {
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool last = atomicAdd(ticket, 1u) == gridDim.x - 1u;
        if (last) *ticket = 0u;
        *sh_last = last ? 1u : 0u;
    }
    __syncthreads();
    if (!*sh_last) return false;
    __threadfence();
    return true;
}

// ---- the group's regions: thread r finds region r (two boundaries: no thread waits for its neighbour's) ---------------
__global__ __launch_bounds__(kRegThreads) void k_wide_regions_cut(const uint32_t *__restrict__ tok, const WideCtl *ctl,
                                                                  RegionPlan p, RegionBufs rb) {
    const uint32_t r = blockIdx.x * kRegThreads + threadIdx.x;
    const unsigned long long n64 = ctl->n;
    const bool planned = n64 <= kRegMaxTokens && n64 <= (unsigned long long)p.per * p.count;
    const uint32_t n = planned ? (uint32_t)n64 : 0u;
    if (r < p.count) {
        const RegionCut c = region_cut(tok, n, p, r, kResRegionCap);
        rb.off[r] = c.off;
        rb.len[r] = c.len;
        if (!c.ok || !planned) atomicOr(&rb.hdr->bad, 1u);
    } else if (r == p.count) {
        rb.off[r] = n;
    }
}

// ---- argmax: k_wide_argmax_partial, and the last workgroup is k_wide_argmax_final<false> -----------------------------
__global__ __launch_bounds__(256) void k_wide_regions_argmax(WideTable t, WideCtl *ctl, WideBest *best,
                                                             unsigned long long *part, WideRegions *reg) {
    __shared__ Cand128 sh[4];
    __shared__ uint32_t sh_last;
    // (uniform over the grid: nothing this launch writes is read here)
    if (reg->bad || ctl->k >= ctl->k_limit) return;
    Cand128 v = {-1, 0};
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i <= t.mask; i += stride) {
        const unsigned long long k = t.keys[i];
        if (k == kWideEmpty) continue;
        const Cand128 c = {(long long)t.cnts[i], ~k};
        if (better(c, v)) v = c;
    }
    v = block_best(v, sh);
    if (threadIdx.x == 0) {                                 // (k_wide_first_gather reads them too, a launch later)
        __hip_atomic_store(&part[2 * blockIdx.x], (unsigned long long)v.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&part[2 * blockIdx.x + 1], v.nkey, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!reg_last_workgroup(&reg->t_argmax, &sh_last)) return;
    v = {-1, 0};
    for (uint32_t b = threadIdx.x; b < gridDim.x; b += blockDim.x) {
        const Cand128 c = {(long long)reg_load(&part[2 * b]), reg_load(&part[2 * b + 1])};
        if (better(c, v)) v = c;
    }
    v = block_best(v, sh);
    if (threadIdx.x == 0) {
        // (a count can never be negative; `first`: a rebuilt table holds no zero-count pair, so M = 0 ends the loop)
        const bool any = ctl->first ? v.count > 0 : v.count >= 0;
        const unsigned long long key = ~v.nkey;
        ctl->live = any ? 1u : 0u;
        ctl->a = (uint32_t)(key >> 32);
        ctl->b = (uint32_t)key;
        ctl->count = any ? (int32_t)v.count : 0;
        ctl->matches = 0;
        ctl->ran = 0;
        if (any) {
            const WideBest wb = {(int32_t)v.count, (uint32_t)(key >> 32), (uint32_t)key, 0u};
            best[ctl->k] = wb;
        }
    }
}

// ---- `first`: the earliest position at which a pair of count M starts, over the regions in stream order ---------------
// After k_wide_first_gather.  off[r] + j is the token's index in the buffer, and regions lie in stream order, so the
// smallest such index is the earliest position of the stream.  The last workgroup is k_wide_first_pick<false>.
__global__ __launch_bounds__(kRegThreads) void k_wide_regions_first_pos(const uint32_t *__restrict__ tok, WideTable t,
                                                                        WideCtl *ctl, WideBest *best, WideFirst *fs,
                                                                        RegionPlan p, RegionBufs rb) {
    __shared__ uint32_t bm[kWideFirstBitmapWords];
    __shared__ uint32_t sh_last;
    if (rb.hdr->bad || ctl->k >= ctl->k_limit || !ctl->live) return;      // (uniform over the grid)
    const uint32_t n_tie = reg_load(&fs->n_tie);
    const uint32_t lane = lane_id();
    if (n_tie > 1) {                                          // (a unique maximum: the lexical winner is it)
        for (uint32_t i = threadIdx.x; i < kWideFirstBitmapWords; i += kRegThreads) bm[i] = fs->bitmap[i];
        __syncthreads();
        const int32_t M = ctl->count;
        const uint32_t n_waves = gridDim.x * kRegWaves;
        bool done = false;
        for (uint32_t r = blockIdx.x * kRegWaves + threadIdx.x / kWave; r < p.count && !done; r += n_waves) {
            const uint32_t base = rb.off[r], n = rb.len[r];
            // regions are visited in ascending order: nothing at or after this one can win any more
            unsigned long long found = reg_load(&fs->pos);
            found = __shfl(found, 0, kWave);                    // (one decision for the whole wave)
            if (found < base) break;
            uint32_t cur = lane < n ? tok[base + lane] : kTokNone;
            for (uint32_t rpos = 0; rpos < n; rpos += kWave) {
                const uint32_t jn = rpos + lane + kWave;
                const uint32_t nxt = jn < n ? tok[base + jn] : kTokNone;
                uint32_t nx = __shfl_down(cur, 1, kWave);
                const uint32_t n0 = __shfl(nxt, 0, kWave);
                if (lane == kWave - 1) nx = n0;
                bool hit = false;
                if (!(cur & kTokEnd)) {                            // a pair starts here (beyond the region: kTokNone)
                    const unsigned long long key = ((unsigned long long)cur << 32) | (nx & kTokIdMask);
                    const uint32_t hb = first_bit(key);
                    if ((bm[hb >> 5] >> (hb & 31u)) & 1u) hit = wide_lookup(t, key) == M;
                }
                const unsigned long long H = __ballot(hit);
                if (H) {
                    // lowest lane = earliest position; every later position of this wave lies behind it
                    if (lane == 0) atomicMin(&fs->pos, (unsigned long long)base + rpos + (uint32_t)__builtin_ctzll(H));
                    done = true;
                    break;
                }
                cur = nxt;
            }
        }
    }
    if (!reg_last_workgroup(&rb.hdr->t_pos, &sh_last)) return;
    if (threadIdx.x == 0) {
        const unsigned long long pos = reg_load(&fs->pos);
        if (n_tie > 1 && pos != ~0ull) {
            // (a: no end flag, a pair starts there -- so pos + 1 lies in the same region)
            const uint32_t a = tok[pos], b = tok[pos + 1] & kTokIdMask;
            ctl->a = a;
            ctl->b = b;
            const WideBest wb = {ctl->count, a, b, 0u};
            best[ctl->k] = wb;
        }
        fs->pos = ~0ull;
        fs->n_tie = 0;
    }
    if (n_tie) for (uint32_t i = threadIdx.x; i < kWideFirstBitmapWords; i += kRegThreads) fs->bitmap[i] = 0;
}

// ---- the merge: every wave its region, in place ----------------------------------------------------------------------
// The table updates are the five of k_wide_match, as plain wide_add.  The last workgroup closes the merge: every match
// removed one token.
template <bool W>
__global__ __launch_bounds__(kRegThreads) void k_wide_regions_walk(uint32_t *tok, uint32_t *wt, WideTable t, WideCtl *ctl,
                                                                   uint32_t new_id_base, RegionPlan p, RegionBufs rb) {
    __shared__ uint32_t sh_last;
    // (uniform over the grid: ctl->k moves only once every workgroup has drawn its ticket)
    if (rb.hdr->bad || ctl->k >= ctl->k_limit || !ctl->live) return;
    const uint32_t a = ctl->a, b = ctl->b, X = new_id_base + ctl->k;
    const uint32_t lane = lane_id(), region = blockIdx.x * kRegWaves + threadIdx.x / kWave;
    if (region < p.count) {
        const auto add = [&](unsigned long long key, int32_t delta) { wide_add(t, ctl, key, delta); };
        const WalkOut o = wide_walk_region<W>(tok, wt, rb.off[region], rb.len[region], a, b, X, lane, add);
        if (lane == 0 && o.n_match) {
            rb.len[region] = o.len;
            add(((unsigned long long)a << 32) | b, -(int32_t)(W ? o.w_match : o.n_match));
            atomicAdd(&ctl->matches, o.n_match);
        }
    }
    if (!reg_last_workgroup(&rb.hdr->t_walk, &sh_last)) return;
    if (threadIdx.x == 0) {
        ctl->n -= reg_load(&ctl->matches);
        ctl->k += 1;
    }
}

// ---- the group's end: where every region goes, then the copy -----------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void k_wide_regions_scan(RegionPlan p, RegionBufs rb, WideCtl *ctl) {
    __shared__ unsigned long long sh[kScanThreads];
    if (rb.hdr->bad) return;                                  // (uniform: the barriers of the scan need that)
    const unsigned long long total = span_scan_sum(rb.len, p.count, rb.to, sh);
    if (threadIdx.x == 0) {
        ctl->n_prev = ctl->n;
        ctl->n = total;
        ctl->ran = 0;
    }
}

template <bool W>
__global__ __launch_bounds__(kRegThreads) void k_wide_regions_copy(const uint32_t *__restrict__ tok, uint32_t *__restrict__ dst,
                                                                   const uint32_t *__restrict__ wt, uint32_t *__restrict__ wdst,
                                                                   RegionPlan p, RegionBufs rb) {
    const uint32_t region = blockIdx.x * kRegWaves + threadIdx.x / kWave;
    if (rb.hdr->bad || region >= p.count) return;
    const uint32_t from = rb.off[region], n = rb.len[region];
    const unsigned long long to = rb.to[region];
    for (uint32_t i = lane_id(); i < n; i += kWave) {
        dst[to + i] = tok[from + i];
        if (W) wdst[to + i] = wt[from + i];
    }
}

uint32_t region_grid(RegionPlan p) { return (p.count + kRegWaves - 1) / kRegWaves; }

}  // namespace

void launch_wide_regions_cut(hipStream_t s, const uint32_t *src, const WideCtl *ctl, RegionPlan plan, RegionBufs rb) {
    hipLaunchKernelGGL(k_wide_regions_cut, dim3(plan.count / kRegThreads + 1), dim3(kRegThreads), 0, s, src, ctl, plan, rb);
}

void launch_wide_regions_merge(hipStream_t s, uint32_t *tok, uint32_t *wt, RegionPlan plan, RegionBufs rb, WideTable t,
                               WideCtl *ctl, WideBest *best, unsigned long long *scratch, WideFirst *fs,
                               uint32_t new_id_base) {
    hipLaunchKernelGGL(k_wide_regions_argmax, dim3(kWideArgBlocks), dim3(256), 0, s, t, ctl, best, scratch, rb.hdr);
    if (fs) {
        launch_wide_first_gather(s, t, ctl, scratch, fs);
        const uint32_t blocks = region_grid(plan) < (uint32_t)kRegPosBlocks ? region_grid(plan) : (uint32_t)kRegPosBlocks;
        hipLaunchKernelGGL(k_wide_regions_first_pos, dim3(blocks), dim3(kRegThreads), 0, s, tok, t, ctl, best, fs, plan, rb);
    }
    if (wt)
        hipLaunchKernelGGL(k_wide_regions_walk<true>, dim3(region_grid(plan)), dim3(kRegThreads), 0, s, tok, wt, t, ctl, new_id_base, plan, rb);
    else
        hipLaunchKernelGGL(k_wide_regions_walk<false>, dim3(region_grid(plan)), dim3(kRegThreads), 0, s, tok, wt, t, ctl, new_id_base, plan, rb);
}

void launch_wide_regions_close(hipStream_t s, const uint32_t *tok, uint32_t *dst, const uint32_t *wt, uint32_t *wdst,
                               RegionPlan plan, RegionBufs rb, WideCtl *ctl) {
    hipLaunchKernelGGL(k_wide_regions_scan, dim3(1), dim3(kScanThreads), 0, s, plan, rb, ctl);
    if (wt)
        hipLaunchKernelGGL(k_wide_regions_copy<true>, dim3(region_grid(plan)), dim3(kRegThreads), 0, s, tok, dst, wt, wdst, plan, rb);
    else
        hipLaunchKernelGGL(k_wide_regions_copy<false>, dim3(region_grid(plan)), dim3(kRegThreads), 0, s, tok, dst, wt, wdst, plan, rb);
}

}  // namespace mbpe
