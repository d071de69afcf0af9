// The 32-bit training loop of a short stream in one workgroup: see wide_resident.h.  gfx950, wave64.
#include "wide_resident.h"
#include "wide_walk.h"

#include <hip/hip_runtime.h>

#include <limits.h>

namespace mbpe {
namespace {

// ---- set-up: the regions of this launch ----------------------------------------------------------------------------
// lane r finds boundary r (resident_boundary scans at most one chunk forward); lane 0 then checks the lengths
__global__ __launch_bounds__(kWave) void k_wide_resident_cut(const uint32_t *__restrict__ tok, const WideCtl *ctl,
                                                             WideResident *res) {
    __shared__ uint32_t off[kResRegions + 1];
    const unsigned long long n64 = ctl->n;
    const uint32_t n = n64 <= kResMaxTokens ? (uint32_t)n64 : 0u;
    if (threadIdx.x <= kResRegions) off[threadIdx.x] = resident_boundary(tok, n, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) {
        bool ok = n64 <= kResMaxTokens;
        for (uint32_t r = 0; r < kResRegions; ++r) ok = ok && off[r + 1] - off[r] <= kResRegionCap;
        for (uint32_t r = 0; r <= kResRegions; ++r) res->off[r] = off[r];
        res->ok = ok ? 1u : 0u;
    }
}

// ---- what the workgroup keeps in LDS (some 33 KiB; DESIGN.md has the budget) -----------------------------------------
struct ResLds {
    int32_t bound[kResSlices];                 // >= every count of the slice's slots (INT_MAX: never scanned)
    unsigned long long nkey[kResSlices];       // exact slices: ~key of the slice's best pair under better()
    uint32_t exact[kResSlices / 32];           // bit s: bound[s] IS the slice's largest count and nkey[s] its pair
    uint32_t bm[kWideFirstBitmapWords];        // `first`: the tied pairs' hashed keys
    Cand128 red[kResRegions];
    uint32_t len[kResRegions], off[kResRegions + 1], hit[kResRegions];
    int32_t m0;                                // the best exact count before a merge's rescan
    uint32_t first_region, n_tie, matches, a, b, rescanned;
};

__device__ __forceinline__ bool res_exact(const ResLds &L, uint32_t s) { return (L.exact[s >> 5] >> (s & 31u)) & 1u; }
__device__ __forceinline__ void res_inexact(ResLds &L, uint32_t s) {
    if (res_exact(L, s)) atomicAnd(&L.exact[s >> 5], ~(1u << (s & 31u)));
}

// wide_add, and the slice of the slot it changed keeps its invariants.  The bound stays an UPPER bound because every
// increment reports the value it made: the final count of a slot is at most the largest of its value before the walk
// (below the bound already) and of the values its increments made.  The exact bit goes wherever the slice's best may
// have changed: an increment that reaches the bound (a new best, or a tie the key order decides), a decrement of an
// entry that stood at the bound.  A slice that was not exact needs nothing but the bound.
__device__ __forceinline__ void res_add(const WideTable &t, WideCtl *ctl, ResLds &L, uint32_t sl_shift,
                                        unsigned long long key, int32_t delta) {
    int32_t old = 0;
    const uint32_t h = wide_add(t, ctl, key, delta, &old);
    if (h == ~0u) return;
    const uint32_t s = h >> sl_shift;
    const int32_t bound = __hip_atomic_load(&L.bound[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (delta > 0) {
        const int32_t now = old + delta;
        if (now >= bound) {
            if (now > bound) atomicMax(&L.bound[s], now);
            res_inexact(L, s);
        }
    } else if (old >= bound) {
        res_inexact(L, s);
    }
}

// The table as the other waves' atomics of the walks before left it: those are performed in L2, so the scans that
// follow a barrier read keys and counts there too (device-scope loads), not from a line the CU may still hold.
__device__ __forceinline__ unsigned long long res_key(const WideTable &t, uint32_t h) {
    return __hip_atomic_load(&t.keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int32_t res_cnt(const WideTable &t, uint32_t h) {
    return __hip_atomic_load(&t.cnts[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// wide_lookup on those loads: count of `key`, or -1 when the pair was never inserted
__device__ __forceinline__ int32_t res_lookup(const WideTable &t, unsigned long long key) {
    uint32_t h = pair_hash(key, t.shift);
    for (uint32_t probe = 0; probe <= t.mask; ++probe) {
        const unsigned long long k = res_key(t, h);
        if (k == key) return res_cnt(t, h);
        if (k == kWideEmpty) return -1;
        h = (h + 1) & t.mask;
    }
    return -1;
}

// one wave: the best pair of slice s under better(), as the slice's exact bound
__device__ __forceinline__ void res_rescan(const WideTable &t, ResLds &L, uint32_t s, uint32_t sl_shift, uint32_t lane) {
    const uint32_t base = s << sl_shift, size = 1u << sl_shift;
    Cand128 v = {-1, 0};
    for (uint32_t i = lane; i < size; i += kWave) {
        const unsigned long long k = res_key(t, base + i);
        if (k == kWideEmpty) continue;
        const Cand128 c = {(long long)res_cnt(t, base + i), ~k};
        if (better(c, v)) v = c;
    }
    v = wave_best(v);
    if (lane == 0) {
        L.bound[s] = (int32_t)v.count;
        L.nkey[s] = v.nkey;
        atomicOr(&L.exact[s >> 5], 1u << (s & 31u));
    }
}

// ---- one merge over one region, in place: the walk of wide_walk.h, its updates through res_add, its length in LDS ------
template <bool W>
__device__ __forceinline__ void res_walk(uint32_t *tok, uint32_t *wt, const WideTable &t, WideCtl *ctl, ResLds &L,
                                         uint32_t sl_shift, uint32_t region, uint32_t a, uint32_t b, uint32_t X,
                                         uint32_t lane) {
    const auto add = [&](unsigned long long key, int32_t delta) { res_add(t, ctl, L, sl_shift, key, delta); };
    const WalkOut o = wide_walk_region<W>(tok, wt, L.off[region], L.len[region], a, b, X, lane, add);
    if (lane == 0 && o.n_match) {
        L.len[region] = o.len;
        add(((unsigned long long)a << 32) | b, -(int32_t)(W ? o.w_match : o.n_match));
        atomicAdd(&L.matches, o.n_match);
    }
}

// ---- `first`: the earliest position of the region at which a pair of count M starts ---------------------------------
__device__ __forceinline__ void res_first_pos(const uint32_t *tok, const WideTable &t, ResLds &L, uint32_t region,
                                              int32_t M, uint32_t lane) {
    const uint32_t base = L.off[region], n = L.len[region];
    uint32_t cur = lane < n ? tok[base + lane] : kTokNone;
    for (uint32_t rpos = 0; rpos < n; rpos += kWave) {
        // regions lie in stream order: once one before this has a position, nothing here can win
        if (__hip_atomic_load(&L.first_region, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < region) break;
        const uint32_t jn = rpos + lane + kWave;
        const uint32_t nxt = jn < n ? tok[base + jn] : kTokNone;
        uint32_t nx = __shfl_down(cur, 1, kWave);
        const uint32_t n0 = __shfl(nxt, 0, kWave);
        if (lane == kWave - 1) nx = n0;
        bool hit = false;
        if (!(cur & kTokEnd)) {                                // a pair starts here (the region ends on an end flag)
            const unsigned long long key = ((unsigned long long)cur << 32) | (nx & kTokIdMask);
            const uint32_t hb = first_bit(key);
            if ((L.bm[hb >> 5] >> (hb & 31u)) & 1u) hit = res_lookup(t, key) == M;
        }
        const unsigned long long H = __ballot(hit);
        if (H) {
            if (lane == 0) {
                L.hit[region] = base + rpos + (uint32_t)__builtin_ctzll(H);
                atomicMin(&L.first_region, region);
            }
            break;
        }
        cur = nxt;
    }
}

// ---- the workgroup ---------------------------------------------------------------------------------------------------
template <bool W, bool FIRST>
__global__ __launch_bounds__(kResThreads) void k_wide_resident(uint32_t *tok, uint32_t *dst, uint32_t *wt, uint32_t *wdst,
                                                               WideTable t, WideCtl *ctl, WideBest *best,
                                                               uint32_t new_id_base, WideResident *res) {
    __shared__ ResLds L;
    if (!res->ok) return;                                   // (uniform: a region too long, the host falls back)
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
    // slices of the table's slots: as few slots each as kResSlices bounds allow, a wave step at least
    const uint32_t slots = t.mask + 1u;                     // (2^31 at most)
    const uint32_t sl_size = slots / kResSlices > kResSliceMin ? slots / kResSlices : kResSliceMin;
    const uint32_t sl_shift = 31u - (uint32_t)__builtin_clz(sl_size), n_sl = slots >> sl_shift;
    for (uint32_t s = tid; s < n_sl; s += kResThreads) L.bound[s] = INT_MAX;
    for (uint32_t i = tid; i < kResSlices / 32; i += kResThreads) L.exact[i] = 0u;
    if (FIRST) for (uint32_t i = tid; i < kWideFirstBitmapWords; i += kResThreads) L.bm[i] = 0u;
    if (tid < kResRegions) { L.off[tid] = res->off[tid]; L.len[tid] = res->off[tid + 1] - res->off[tid]; }
    if (tid == 0) { L.m0 = INT_MIN; L.rescanned = 0; L.matches = 0; L.off[kResRegions] = res->off[kResRegions]; }
    const uint32_t k0 = ctl->k, k_limit = ctl->k_limit;
    uint32_t k = k0, n_rescanned = 0;
    Cand128 top = {-1, 0};
    bool live = false, chose = false;
    uint32_t a = 0, b = 0;
    unsigned long long t_argmax = 0, t_first = 0, t_walk = 0, t0 = 0;
    __syncthreads();
    while (k < k_limit) {
        // ---- argmax: the best exact count so far, the slices that might beat or tie it, the best of all exact ones
        if (tid == 0) { t0 = wall_clock64(); L.matches = 0; L.n_tie = 0; L.first_region = kResRegions; }
        int32_t m = INT_MIN;
        for (uint32_t s = tid; s < n_sl; s += kResThreads)
            if (res_exact(L, s) && L.bound[s] > m) m = L.bound[s];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const int32_t o = __shfl_xor(m, d, kWave); m = o > m ? o : m; }
        if (lane == 0 && m > INT_MIN) atomicMax(&L.m0, m);
        __syncthreads();
        const int32_t m0 = L.m0;
        for (uint32_t s = wave; s < n_sl; s += kResRegions)
            if (!res_exact(L, s) && L.bound[s] >= m0) { res_rescan(t, L, s, sl_shift, lane); ++n_rescanned; }
        __syncthreads();
        Cand128 v = {-1, 0};
        for (uint32_t s = tid; s < n_sl; s += kResThreads) {
            if (!res_exact(L, s)) continue;                  // (left alone: its bound lies below m0)
            const Cand128 c = {(long long)L.bound[s], L.nkey[s]};
            if (better(c, v)) v = c;
        }
        top = block_best(v, L.red);
        if (tid == 0) L.m0 = INT_MIN;
        // (a count can never be negative; `first`: a rebuilt table holds no zero-count pair, so M = 0 ends the loop)
        live = FIRST ? top.count > 0 : top.count >= 0;
        chose = true;
        a = (uint32_t)(~top.nkey >> 32);
        b = (uint32_t)~top.nkey;
        if (tid == 0) { const unsigned long long t1 = wall_clock64(); t_argmax += t1 - t0; t0 = t1; }
        if (!live) break;
        if (!FIRST && top.count == 0) {
            // the best pair occurs nowhere: a merge changes nothing and the loop chooses it again up to k_limit
            const WideBest wb = {0, a, b, 0u};
            for (uint32_t i = k + tid; i < k_limit; i += kResThreads) best[i] = wb;
            k = k_limit;
            break;
        }
        if (FIRST) {
            // ---- the pairs of count M: how many, and the bitmap of their hashed keys (all slices that reach M are exact)
            const int32_t M = (int32_t)top.count;
            uint32_t found = 0;
            for (uint32_t s = wave; s < n_sl; s += kResRegions) {
                if (!res_exact(L, s) || L.bound[s] != M) continue;
                const uint32_t sb = s << sl_shift;
                for (uint32_t i = lane; i < (1u << sl_shift); i += kWave) {
                    if (res_cnt(t, sb + i) != M) continue;
                    const unsigned long long key = res_key(t, sb + i);
                    if (key == kWideEmpty) continue;
                    const uint32_t hb = first_bit(key);
                    atomicOr(&L.bm[hb >> 5], 1u << (hb & 31u));
                    ++found;
                }
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) found += __shfl_xor(found, d, kWave);
            if (lane == 0 && found) atomicAdd(&L.n_tie, found);
            __syncthreads();
            const uint32_t n_tie = L.n_tie;
            if (n_tie > 1) res_first_pos(tok, t, L, wave, M, lane);      // a unique maximum: the lexical winner is it
            __syncthreads();
            if (tid == 0 && n_tie > 1 && L.first_region < kResRegions) {
                const uint32_t pos = L.hit[L.first_region];
                L.a = tok[pos];                                 // (no end flag: a pair starts there)
                L.b = tok[pos + 1] & kTokIdMask;
            } else if (tid == 0) {
                L.a = a; L.b = b;
            }
            for (uint32_t i = tid; i < kWideFirstBitmapWords; i += kResThreads) L.bm[i] = 0u;
            __syncthreads();
            a = L.a;
            b = L.b;
            if (tid == 0) { const unsigned long long t1 = wall_clock64(); t_first += t1 - t0; t0 = t1; }
        }
        if (tid == 0) { const WideBest wb = {(int32_t)top.count, a, b, 0u}; best[k] = wb; }
        // ---- the merge: every wave its region
        if (W) res_walk<true>(tok, wt, t, ctl, L, sl_shift, wave, a, b, new_id_base + k, lane);
        else res_walk<false>(tok, wt, t, ctl, L, sl_shift, wave, a, b, new_id_base + k, lane);
        ++k;
        __syncthreads();
        if (tid == 0) t_walk += wall_clock64() - t0;
    }
    // ---- the regions closed up into the other buffer: a scan of their lengths, one copy -----------------------------
    if (lane == 0 && n_rescanned) atomicAdd(&L.rescanned, n_rescanned);
    __syncthreads();
    if (tid == 0) {
        uint32_t o = 0;
        for (uint32_t r = 0; r < kResRegions; ++r) { L.hit[r] = o; o += L.len[r]; }
        L.first_region = o;                                  // (the new length)
    }
    __syncthreads();
    if (k > k0) {
        for (uint32_t r = 0; r < kResRegions; ++r) {
            const uint32_t from = L.off[r], to = L.hit[r], n = L.len[r];
            for (uint32_t i = tid; i < n; i += kResThreads) {
                dst[to + i] = tok[from + i];
                if (W) wdst[to + i] = wt[from + i];
            }
        }
    }
    if (tid == 0) {
        if (chose) {
            ctl->live = live ? 1u : 0u;
            ctl->a = a;
            ctl->b = b;
            ctl->count = live ? (int32_t)top.count : 0;
            ctl->matches = L.matches;
        }
        if (k > k0) { ctl->n_prev = ctl->n; ctl->n = L.first_region; }
        ctl->ran = 0;
        ctl->k = k;
        res->n_rescanned += L.rescanned;
        res->t_argmax += t_argmax;
        res->t_first += t_first;
        res->t_walk += t_walk;
    }
}

}  // namespace

void launch_wide_resident(hipStream_t s, uint32_t *src, uint32_t *dst, uint32_t *wsrc, uint32_t *wdst, WideTable t,
                          WideCtl *ctl, WideBest *best, uint32_t new_id_base, bool first, WideResident *res) {
    hipLaunchKernelGGL(k_wide_resident_cut, dim3(1), dim3(kWave), 0, s, src, ctl, res);
    const dim3 grid(1), block(kResThreads);
    if (wsrc && first)
        hipLaunchKernelGGL((k_wide_resident<true, true>), grid, block, 0, s, src, dst, wsrc, wdst, t, ctl, best, new_id_base, res);
    else if (wsrc)
        hipLaunchKernelGGL((k_wide_resident<true, false>), grid, block, 0, s, src, dst, wsrc, wdst, t, ctl, best, new_id_base, res);
    else if (first)
        hipLaunchKernelGGL((k_wide_resident<false, true>), grid, block, 0, s, src, dst, wsrc, wdst, t, ctl, best, new_id_base, res);
    else
        hipLaunchKernelGGL((k_wide_resident<false, false>), grid, block, 0, s, src, dst, wsrc, wdst, t, ctl, best, new_id_base, res);
}

}  // namespace mbpe
