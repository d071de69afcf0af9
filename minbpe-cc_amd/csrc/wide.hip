// Kernels of the 32-bit continuation of a training: see wide.h.  gfx950, wave64.
#include "wide.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace mbpe {
namespace {

// create_or_modify_pair, PairCount.h:249-260: find the pair and add `delta`, or insert it with `delta`.  Entries are
// never removed.  Concurrent inserts of one key meet at the same free slot and the CAS lets exactly one of them in.
__device__ void wide_add(const WideTable &t, WideCtl *ctl, unsigned long long key, int32_t delta) {
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
            atomicAdd(&t.cnts[h], delta);
            return;
        }
        h = (h + 1) & t.mask;
    }
    atomicOr(&ctl->err, 1u);
}

__global__ void k_wide_table_clear(WideTable t) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i <= t.mask; i += stride) { t.keys[i] = kWideEmpty; t.cnts[i] = 0; }
}

__global__ void k_wide_table_from16(const uint32_t *__restrict__ ekey, const int32_t *__restrict__ ecnt, uint32_t n,
                                    WideTable t, WideCtl *ctl) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const uint32_t k16 = ekey[i];
        wide_add(t, ctl, ((unsigned long long)(k16 >> 16) << 32) | (k16 & 0xFFFFu), ecnt[i]);
    }
}

__global__ void k_wide_rehash(WideTable from, WideTable to, WideCtl *ctl) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i <= from.mask; i += stride) {
        const unsigned long long k = from.keys[i];
        if (k != kWideEmpty) wide_add(to, ctl, k, from.cnts[i]);
    }
}

// ---- the pair count of a stream that starts as 32-bit tokens (a training continued from existing merges) ------------
// The 64-bit-key counterpart of k_pair_count_tokens (kernels.hip): every position i whose token is not the last of its
// chunk counts (tok[i], tok[i+1]), overlapping ones too.  A workgroup counts its contiguous share in an LDS cache --
// kWpSlots open-addressed entries, 64-bit keys beside 32-bit counts, up to kWpProbes probes; the key is claimed with
// one 8-byte LDS compare-and-swap (skipped when the key is there already) -- and flushes the cache once through
// wide_add; a position that finds no entry goes to wide_add directly.  A share is at most 2^20 positions (the
// launcher's grid), so an LDS count cannot wrap.  ids: the token ids that exist; a token beyond them sets
// kWideErrToken and is never hashed or used as an address.  4 B read per token.
constexpr int kWpThreads = 256;
constexpr uint32_t kWpSlots = 1024, kWpProbes = 4;      // 8 KiB of keys + 4 KiB of counts
// W: a position counts wt[i] times, its chunk's weight (a corpus of unique chunks, wide.h), and the tally's
// "positions" is the 64-bit sum of the weights counted.  An LDS count may then wrap 2^32 like the table's own count
// it is added to; the census catches either, since the true sum no longer equals the sum of the table's counts.
template <bool W>
__global__ __launch_bounds__(kWpThreads) void k_wide_pair_count_tokens(const uint32_t *__restrict__ tok,
                                                                       const uint32_t *__restrict__ wt, uint64_t n_tok,
                                                                       uint32_t ids, WideTable t, WideCtl *ctl,
                                                                       WideTally *tally) {
    __shared__ unsigned long long ckey[kWpSlots];
    __shared__ uint32_t ccnt[kWpSlots];
    for (uint32_t i = threadIdx.x; i < kWpSlots; i += kWpThreads) { ckey[i] = kWideEmpty; ccnt[i] = 0; }
    __syncthreads();
    const uint64_t per = (n_tok + gridDim.x - 1) / gridDim.x;
    const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < n_tok ? lo + per : n_tok;
    uint32_t counted = 0;
    unsigned long long wsum = 0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += kWpThreads) {
        const uint32_t a = tok[i];
        if ((a & kTokEnd) || i + 1 >= n_tok) continue;
        const uint32_t b = tok[i + 1] & kTokIdMask;
        if (a >= ids || b >= ids) { atomicOr(&ctl->err, kWideErrToken); continue; }
        const unsigned long long key = ((unsigned long long)a << 32) | b;
        const uint32_t w = W ? wt[i] : 1u;
        if (W) wsum += w; else ++counted;
        uint32_t h = pair_hash(key, 64 - 10);
        static_assert(kWpSlots == 1u << 10, "pair_hash's shift above");
        bool done = false;
#pragma unroll
        for (uint32_t p = 0; p < kWpProbes && !done; ++p) {
            unsigned long long k = ckey[h];
            if (k == kWideEmpty) k = atomicCAS(&ckey[h], kWideEmpty, key);
            if (k == kWideEmpty || k == key) { atomicAdd(&ccnt[h], w); done = true; }
            h = (h + 1) & (kWpSlots - 1);
        }
        if (!done) wide_add(t, ctl, key, (int32_t)w);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kWpSlots; i += kWpThreads)
        if (ckey[i] != kWideEmpty) wide_add(t, ctl, ckey[i], (int32_t)ccnt[i]);
    if (W) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            wsum += ((unsigned long long)(uint32_t)__shfl_xor((int)(wsum >> 32), d, kWave) << 32) |
                    (uint32_t)__shfl_xor((int)wsum, d, kWave);
        if (lane_id() == 0 && wsum) atomicAdd(&tally->positions, wsum);
    } else {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) counted += __shfl_xor(counted, d, kWave);
        if (lane_id() == 0 && counted) atomicAdd(&tally->positions, (unsigned long long)counted);
    }
}

// ---- chunk weights (wide.h): every token gets the weight of its chunk ------------------------------------------------
// the chunk of token i is the number of end flags before it: per span the flags it holds, a scan, a ranked fill
__global__ __launch_bounds__(kSpanThreads) void k_wide_end_count(const uint32_t *__restrict__ tok, uint64_t n,
                                                                 uint32_t *__restrict__ span_ends) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    uint32_t ends = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        ends += wave_count(i < n && (tok[i] & kTokEnd));
    }
    if (lane == 0) span_ends[span] = ends;
}

__global__ __launch_bounds__(kScanThreads) void k_wide_scan_ends(const uint32_t *__restrict__ cnt, uint64_t n,
                                                                 unsigned long long *__restrict__ off) {
    __shared__ unsigned long long sh[kScanThreads];
    span_scan_sum(cnt, span_count(n), off, sh);
}

// wt[i] = weights[chunk of i]; a chunk beyond n_weights, a weight of 0 or one of 2^31 or more sets kWideErrWeight
__global__ __launch_bounds__(kSpanThreads) void k_wide_fill_weights(const uint32_t *__restrict__ tok, uint64_t n,
                                                                    const unsigned long long *__restrict__ span_off,
                                                                    const uint32_t *__restrict__ weights, uint64_t n_weights,
                                                                    uint32_t *__restrict__ wt, WideCtl *ctl) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    const unsigned long long lt = lanes_below(lane);
    unsigned long long chunk = span_off[span];
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        const WaveKeep k = wave_keep(i < n && (tok[i] & kTokEnd), lt);
        if (i < n) {
            const unsigned long long c = chunk + k.rank;
            uint32_t w = 1u;
            if (c < n_weights) w = weights[c];
            if (c >= n_weights || w == 0u || w >= 0x80000000u) { atomicOr(&ctl->err, kWideErrWeight); w = 1u; }
            wt[i] = w;
        }
        chunk += k.count;
    }
}

// flag[0] = 1 when one of the n weights is 0, or 2^31 or more
__global__ __launch_bounds__(256) void k_wide_check_weights(const uint32_t *__restrict__ weights, uint64_t n, uint32_t *flag) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (; i < n; i += stride) { const uint32_t w = weights[i]; bad |= w == 0u || w >= 0x80000000u; }
    if (bad) atomicOr(flag, 1u);
}

// the census of the table behind that count: the sum of its counts, the largest of them (as unsigned: a count that
// passed 2^31 shows as one)
__global__ __launch_bounds__(256) void k_wide_table_tally(WideTable t, WideTally *tally) {
    unsigned long long sum = 0;
    uint32_t top = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= t.mask; i += (uint64_t)gridDim.x * blockDim.x) {
        if (t.keys[i] == kWideEmpty) continue;
        const uint32_t v = (uint32_t)t.cnts[i];
        sum += v;
        top = v > top ? v : top;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sum += ((unsigned long long)(uint32_t)__shfl_xor((int)(sum >> 32), d, kWave) << 32) | (uint32_t)__shfl_xor((int)sum, d, kWave);
        const uint32_t o = __shfl_xor(top, d, kWave);
        top = o > top ? o : top;
    }
    if (lane_id() == 0 && top) { atomicAdd(&tally->total, sum); atomicMax(&tally->top, top); }
}

// the counterpart of k_resume_check: the counts must add up to the positions counted (a count that wrapped past 2^32
// does not), and none may have reached 2^31
__global__ void k_wide_resume_check(const WideTally *tally, WideCtl *ctl) {
    if (tally->total != tally->positions || tally->top >= 0x80000000u) atomicOr(&ctl->err, kWideErrCount);
}

// ---- argmax: (count desc, first asc, second asc) = the larger of (count, ~key) -------------------------------
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
__device__ Cand128 block_best(Cand128 v, Cand128 *sh) {
    v = wave_best(v);
    __syncthreads();
    if (lane_id() == 0) sh[threadIdx.x / kWave] = v;
    __syncthreads();
    Cand128 r = sh[0];
    for (uint32_t w = 1; w < blockDim.x / kWave; ++w)
        if (better(sh[w], r)) r = sh[w];
    return r;
}

// ---- stopping rules (wide.h): which pairs the argmax may choose ------------------------------------------------------
// len[a] + len[b] <= max_len; the entries saturate at kWideLenMax, so the sum does not wrap.  Every id of a key in the
// table or of a token in the stream lies below the training's vocab_size, which is how many entries len[] has.
__device__ __forceinline__ bool wide_eligible(const uint32_t *__restrict__ len, uint32_t max_len, unsigned long long key) {
    return len[(uint32_t)(key >> 32)] + len[(uint32_t)key] <= max_len;
}
// the length of the token that the merge under way makes, once ctl->a, b are final
__device__ __forceinline__ void wide_new_len(const WideLimits &lim, const WideCtl *ctl) {
    const uint32_t l = lim.len[ctl->a] + lim.len[ctl->b];
    lim.len[lim.new_id_base + ctl->k] = l < kWideLenMax ? l : kWideLenMax;
}

constexpr int kArgBlocks = 1024;
// LIM: only eligible pairs.  A pair is tested once it beats the thread's best so far, so the two gathers of the test
// are paid a few times per thread, not per entry (unless ineligible pairs lead the table, where every leader is
// tested once).
template <bool LIM>
__global__ __launch_bounds__(256) void k_wide_argmax_partial(WideTable t, const WideCtl *ctl,
                                                             unsigned long long *__restrict__ part,
                                                             const uint32_t *__restrict__ len, uint32_t max_len) {
    __shared__ Cand128 sh[4];
    Cand128 v = {-1, 0};
    if (ctl->k < ctl->k_limit) {
        uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
        for (; i <= t.mask; i += stride) {
            const unsigned long long k = t.keys[i];
            if (k == kWideEmpty) continue;
            Cand128 c = {(long long)t.cnts[i], ~k};
            if (better(c, v) && (!LIM || wide_eligible(len, max_len, k))) v = c;
        }
    }
    v = block_best(v, sh);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = (unsigned long long)v.count; part[2 * blockIdx.x + 1] = v.nkey; }
}

// LIM: the loop also ends when the best eligible count lies below lim.min_count (no eligible pair: the partials hold
// count -1, as for an empty table), and in lexical mode the new token's length is noted (`first`: k_wide_first_pick)
template <bool LIM>
__global__ __launch_bounds__(kArgBlocks) void k_wide_argmax_final(const unsigned long long *__restrict__ part,
                                                                  WideCtl *ctl, WideBest *best, WideLimits lim) {
    __shared__ Cand128 sh[kArgBlocks / kWave];
    if (threadIdx.x == 0) ctl->ran = 0;        // (whatever follows: no scatter without a merge of its own)
    if (ctl->k >= ctl->k_limit) return;
    Cand128 v = {(long long)part[2 * threadIdx.x], part[2 * threadIdx.x + 1]};
    v = block_best(v, sh);
    if (threadIdx.x == 0) {
        // (a count can never be negative: every decrement undoes an increment.  `first`: a rebuilt table holds no
        //  zero-count pair, so M = 0 ends the loop, Tokenizer.h:586-588)
        bool any = ctl->first ? v.count > 0 : v.count >= 0;
        if (LIM) any = any && v.count >= (long long)lim.min_count;
        const unsigned long long key = ~v.nkey;
        ctl->live = any ? 1u : 0u;
        ctl->a = (uint32_t)(key >> 32);
        ctl->b = (uint32_t)key;
        ctl->count = any ? (int32_t)v.count : 0;
        ctl->matches = 0;
        if (any) {
            WideBest wb = {(int32_t)v.count, (uint32_t)(key >> 32), (uint32_t)key, 0u};
            best[ctl->k] = wb;
            if (LIM && lim.len && !ctl->first) wide_new_len(lim, ctl);
        }
    }
}

// ---- `first` tie-break (see wide.h) ----------------------------------------------------------------------------
__device__ __forceinline__ uint32_t first_bit(unsigned long long key) { return pair_hash(key, 48); }   // 16 bits

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

// the grid and stride of k_wide_argmax_partial: block b walks the slice whose maximum is part[2 b].
// LIM: n_tie and the bitmap hold eligible pairs only (part[] is the eligible maximum already)
template <bool LIM>
__global__ __launch_bounds__(256) void k_wide_first_gather(WideTable t, const WideCtl *ctl,
                                                           const unsigned long long *__restrict__ part, WideFirst *fs,
                                                           const uint32_t *__restrict__ len, uint32_t max_len) {
    if (ctl->k >= ctl->k_limit || !ctl->live) return;
    const int32_t M = ctl->count;
    if ((long long)part[2 * blockIdx.x] < (long long)M) return;
    uint32_t found = 0;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i <= t.mask; i += stride) {
        if (t.cnts[i] != M) continue;
        const unsigned long long k = t.keys[i];
        if (k == kWideEmpty) continue;
        if (LIM && !wide_eligible(len, max_len, k)) continue;
        const uint32_t hb = first_bit(k), bit = 1u << (hb & 31u);
        // (thousands of tied pairs share 2,048 words: most bits are set already, skip their atomics)
        if (!(__hip_atomic_load(&fs->bitmap[hb >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit))
            atomicOr(&fs->bitmap[hb >> 5], bit);
        ++found;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) found += __shfl_xor(found, d, kWave);
    if (lane_id() == 0 && found) atomicAdd(&fs->n_tie, found);
}

constexpr int kPosBlocks = 1024;
// LIM: a hit needs count == M and eligibility -- an ineligible pair of count M may share a bitmap bit with a tied one,
// or be one whose bit an eligible pair of the same hash set
template <bool LIM>
__global__ __launch_bounds__(kSpanThreads) void k_wide_first_pos(const uint32_t *__restrict__ tok, WideTable t,
                                                                 const WideCtl *ctl, WideFirst *fs,
                                                                 const uint32_t *__restrict__ len, uint32_t max_len) {
    __shared__ uint32_t bm[kWideFirstBitmapWords];
    if (ctl->k >= ctl->k_limit || !ctl->live) return;
    if (fs->n_tie <= 1) return;                               // a unique maximum: the lexical winner is it
    const uint64_t n = ctl->n;
    const uint64_t n_spans = span_count(n);
    const uint64_t n_waves = (uint64_t)gridDim.x * kSpanWaves;
    const uint64_t first_span = (uint64_t)blockIdx.x * kSpanWaves;
    if (first_span >= n_spans) return;
    const int32_t M = ctl->count;
    for (uint32_t i = threadIdx.x; i < kWideFirstBitmapWords; i += kSpanThreads) bm[i] = fs->bitmap[i];
    __syncthreads();
    const uint32_t lane = lane_id();
    for (uint64_t span = first_span + threadIdx.x / kWave; span < n_spans; span += n_waves) {
        const uint64_t base = span * kSpan;
        // spans are visited in ascending order: nothing at or after this one can win any more
        unsigned long long cur = __hip_atomic_load(&fs->pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cur = __shfl(cur, 0, kWave);                          // (one decision for the whole wave)
        if (cur < base) break;
        bool hit_span = false;
        for (int it = 0; it < kSpanIters; ++it) {
            const uint64_t i = base + (uint64_t)it * kWave + lane;
            uint32_t nx;
            const uint32_t tv = load_pair(tok, i, n, lane, kTokEnd, &nx);
            bool hit = false;
            if (i + 1 < n && !(tv & kTokEnd)) {                  // a pair starts here (Tokenizer.h:135-144)
                const unsigned long long key = ((unsigned long long)tv << 32) | (nx & kTokIdMask);
                const uint32_t hb = first_bit(key);
                if ((bm[hb >> 5] >> (hb & 31u)) & 1u)
                    hit = wide_lookup(t, key) == M && (!LIM || wide_eligible(len, max_len, key));
            }
            const unsigned long long H = __ballot(hit);
            if (H) {
                // lowest lane = earliest position; every later position of this wave lies behind it
                if (lane == 0) atomicMin(&fs->pos, (unsigned long long)(base + (uint64_t)it * kWave + __builtin_ctzll(H)));
                hit_span = true;
                break;
            }
        }
        if (hit_span) break;
    }
}

// LIM: ctl->a, b are final here, whichever kernel chose them: the new token's length is noted
template <bool LIM>
__global__ __launch_bounds__(256) void k_wide_first_pick(const uint32_t *__restrict__ tok, WideCtl *ctl, WideBest *best,
                                                         WideFirst *fs, WideLimits lim) {
    __shared__ uint32_t nt;
    if (threadIdx.x == 0) {
        nt = fs->n_tie;
        const unsigned long long pos = fs->pos;
        if (ctl->k < ctl->k_limit && ctl->live && nt > 1 && pos != ~0ull) {
            const uint32_t a = tok[pos], b = tok[pos + 1] & kTokIdMask;      // (a: no end flag, a pair starts there)
            ctl->a = a;
            ctl->b = b;
            WideBest wb = {ctl->count, a, b, 0u};
            best[ctl->k] = wb;
        }
        if (LIM && ctl->k < ctl->k_limit && ctl->live) wide_new_len(lim, ctl);
        fs->pos = ~0ull;
        fs->n_tie = 0;
    }
    __syncthreads();
    if (nt) for (uint32_t i = threadIdx.x; i < kWideFirstBitmapWords; i += blockDim.x) fs->bitmap[i] = 0;
}

// ---- the scans and the compaction of span.h, under the loop's control block ----------------------------------------
__global__ __launch_bounds__(kScanThreads) void k_wide_scan_parity(const uint32_t *__restrict__ span_sum,
                                                                   const WideCtl *ctl, uint32_t *__restrict__ in_par) {
    __shared__ uint32_t sh[kScanThreads];
    span_scan_parity(span_sum, span_count(ctl->n), in_par, sh);
}

// exclusive sums of the spans' kept-token counts over the spans of n_in tokens; the total becomes ctl->n (and, when
// `advance`, the merge counter moves on)
__global__ __launch_bounds__(kScanThreads) void k_wide_scan_sum(const uint32_t *__restrict__ cnt, uint64_t n_in_fixed,
                                                                unsigned long long *__restrict__ off, WideCtl *ctl,
                                                                int advance) {
    __shared__ unsigned long long sh[kScanThreads];
    // Order: every thread reads ctl->k, live and n here, before the first barrier of span_scan_sum; thread 0 writes
    // n, n_prev, ran and k only after it.  The early return is uniform over the workgroup (the barriers need that).
    if (advance && (ctl->k >= ctl->k_limit || !ctl->live)) return;
    const uint64_t n_in = advance ? ctl->n : n_in_fixed;
    const unsigned long long total = span_scan_sum(cnt, span_count(n_in), off, sh);
    if (threadIdx.x == 0) {
        ctl->n_prev = n_in;                    // (the scatter walks the stream that was read)
        ctl->n = total;
        ctl->ran = 1;
        if (advance) ctl->k += 1;
    }
}

// W: the tokens' weights travel with them (a merged token stands where its left half stood and keeps that entry)
template <bool W>
__global__ __launch_bounds__(kSpanThreads) void k_wide_scatter(const uint32_t *__restrict__ val,
                                                               const unsigned long long *__restrict__ span_off,
                                                               uint32_t *__restrict__ out, const WideCtl *ctl,
                                                               const uint32_t *__restrict__ wt, uint32_t *__restrict__ wt_out) {
    // (a merge that did not run -- limit reached, empty table -- must not scatter either)
    if (!ctl->ran) return;
    span_scatter_carry<W>(val, ctl->n_prev, span_off, out, wt, wt_out);
}

// ---- conversion of the 16-bit slot stream ---------------------------------------------------------------------
__global__ __launch_bounds__(kSpanThreads) void k_wide_from_slots(const uint16_t *__restrict__ slots, uint64_t n_live,
                                                                  uint32_t barrier, uint32_t endbit, uint32_t *__restrict__ val,
                                                                  uint32_t *__restrict__ span_keep) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n_live) return;
    const uint32_t lane = lane_id();
    uint32_t kept = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        uint32_t v = kTokNone;
        if (i < n_live) {
            const uint32_t s = slots[i];
            if (s != barrier) {
                const bool last = i + 1 >= n_live;
                const uint32_t nx = last ? barrier : slots[i + 1];
                // flag bit: the slot says so; barrier layout: a barrier follows; one chunk: only the very last token
                const bool end = endbit ? (s & endbit) != 0u : barrier == 0xFFFFFFFFu ? last : nx == barrier;
                v = (s & ~endbit) | (end ? kTokEnd : 0u);
            }
            val[i] = v;
        }
        kept += wave_count(v != kTokNone);
    }
    if (lane == 0) span_keep[span] = kept;
}

// ---- one merge ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_cand(uint32_t t, uint32_t nx, uint32_t a, uint32_t b) {
    return !(t & kTokEnd) && t == a && (nx & kTokIdMask) == b;      // (t carries no end flag here, so t == a compares ids)
}

__global__ __launch_bounds__(kSpanThreads) void k_wide_cand(const uint32_t *__restrict__ tok, const WideCtl *ctl,
                                                            uint32_t *__restrict__ span_sum) {
    if (ctl->k >= ctl->k_limit || !ctl->live) return;
    const uint64_t n = ctl->n;
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t a = ctl->a, b = ctl->b;
    const uint32_t lane = lane_id();
    SpanSum sum = span_empty();
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        uint32_t nx;
        const uint32_t t = load_pair(tok, i, n, lane, kTokEnd, &nx);
        sum = span_add_group(sum, __ballot(i + 1 < n && is_cand(t, nx, a, b)));
    }
    if (lane == 0) span_sum[span] = span_pack(sum);
}

// W: every update is worth the weight of the match's chunk (its neighbours lie in the same chunk), and (a, b) loses
// the sum of the weights matched, which is at most its count and so below 2^31; ctl->matches stays a position count.
template <bool W>
__global__ __launch_bounds__(kSpanThreads) void k_wide_match(const uint32_t *__restrict__ tok, const uint32_t *__restrict__ wt,
                                                             const uint32_t *__restrict__ in_par,
                                                             uint32_t *__restrict__ val, uint32_t *__restrict__ span_keep,
                                                             WideTable tab, WideCtl *ctl, uint32_t new_id_base) {
    if (ctl->k >= ctl->k_limit || !ctl->live) return;
    const uint64_t n = ctl->n;
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t a = ctl->a, b = ctl->b, X = new_id_base + ctl->k;
    const uint32_t lane = lane_id();
    const unsigned long long lt = lanes_below(lane);
    uint32_t carry = in_par[span];
    uint32_t kept = 0, n_match = 0, w_match = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        uint32_t nx;
        const uint32_t t = load_pair(tok, i, n, lane, kTokEnd, &nx);
        const bool c = i + 1 < n && is_cand(t, nx, a, b);
        const unsigned long long M = __ballot(c);
        const bool odd = run_below(M, lt, lane, carry) & 1u;
        uint32_t v = kTokNone;
        const bool match = c && !odd;
        if (i < n && !odd) v = match ? (X | (nx & kTokEnd)) : t;
        if (i < n) val[i] = v;
        kept += wave_count(v != kTokNone);
        n_match += wave_count(match);
        if (match) {
            const int32_t w = W ? (int32_t)wt[i] : 1;
            if (W) w_match += (uint32_t)w;
            // Tokenizer.h:248-260: the left neighbour as it stands AFTER the walk has passed it.  It was swallowed by a
            // match (and is X now) iff a match ends right before i: for a == b that is "(i-1, i) is a candidate too"
            // (then the run before i-1 is odd, r being even here), for a != b "(i-2, i-1) is a candidate" (such
            // candidates never touch, so every one of them is a match).
            if (i > 0) {
                const uint32_t p = tok[i - 1];
                if (!(p & kTokEnd)) {
                    bool swallowed;
                    if (a == b) swallowed = p == a;                   // (no end flag on p: (p, t) is a candidate)
                    else swallowed = i > 1 && (p & kTokIdMask) == b && tok[i - 2] == a;   // (tok[i-2] == a: no end flag, id a)
                    const uint32_t x = swallowed ? X : p;
                    wide_add(tab, ctl, ((unsigned long long)x << 32) | a, -w);
                    wide_add(tab, ctl, ((unsigned long long)x << 32) | X, w);
                }
            }
            // :263-279: the right neighbour as it still is
            if (!(nx & kTokEnd) && i + 2 < n) {
                const uint32_t y = tok[i + 2] & kTokIdMask;
                wide_add(tab, ctl, ((unsigned long long)b << 32) | y, -w);
                wide_add(tab, ctl, ((unsigned long long)X << 32) | y, w);
            }
        }
        carry = run_carry(M, carry);
    }
    if (W) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) w_match += __shfl_xor(w_match, d, kWave);
    }
    if (lane == 0) {
        span_keep[span] = kept;
        if (n_match) {
            wide_add(tab, ctl, ((unsigned long long)a << 32) | b, -(int32_t)(W ? w_match : n_match));      // :240-246
            atomicAdd(&ctl->matches, n_match);
        }
    }
}

}  // namespace

size_t wide_scratch_words(uint64_t n_tokens) {
    const uint64_t n_spans = span_count(n_tokens) + 2;
    return (size_t)(n_spans * 5 + 8);          // span_sum, in_par, span_keep (u32 each), span_off (u64)
}

namespace {
struct Scratch { uint32_t *span_sum, *in_par, *span_keep; unsigned long long *span_off; };
Scratch carve(uint32_t *scratch, uint64_t n_tokens) {
    const uint64_t n_spans = span_count(n_tokens) + 2;
    Scratch s;
    s.span_off = reinterpret_cast<unsigned long long *>(scratch);          // (8-byte aligned: first)
    s.span_sum = scratch + 2 * n_spans;
    s.in_par = s.span_sum + n_spans;
    s.span_keep = s.in_par + n_spans;
    return s;
}
}  // namespace

void launch_wide_from_slots(hipStream_t s, const uint16_t *slots, uint64_t n_live, uint32_t barrier, uint32_t endbit,
                            uint32_t *val, uint32_t *span_scratch, uint32_t *tok_out, WideCtl *ctl) {
    if (!n_live) return;
    const Scratch sc = carve(span_scratch, n_live);
    hipLaunchKernelGGL(k_wide_from_slots, dim3(span_grid(n_live)), dim3(kSpanThreads), 0, s, slots, n_live, barrier, endbit, val, sc.span_keep);
    hipLaunchKernelGGL(k_wide_scan_sum, dim3(1), dim3(kScanThreads), 0, s, sc.span_keep, n_live, sc.span_off, ctl, 0);
    hipLaunchKernelGGL(k_wide_scatter<false>, dim3(span_grid(n_live)), dim3(kSpanThreads), 0, s, val, sc.span_off, tok_out, ctl,
                       (const uint32_t *)nullptr, (uint32_t *)nullptr);
}

void launch_wide_table_clear(hipStream_t s, WideTable t) {
    hipLaunchKernelGGL(k_wide_table_clear, dim3(2048), dim3(256), 0, s, t);
}

void launch_wide_table_from16(hipStream_t s, const uint32_t *ekey, const int32_t *ecnt, uint32_t n_entries, WideTable t,
                              WideCtl *ctl) {
    if (!n_entries) return;
    const uint32_t blocks = n_entries / 256 + 1 > 4096 ? 4096 : n_entries / 256 + 1;
    hipLaunchKernelGGL(k_wide_table_from16, dim3(blocks), dim3(256), 0, s, ekey, ecnt, n_entries, t, ctl);
}

void launch_wide_rehash(hipStream_t s, WideTable from, WideTable to, WideCtl *ctl) {
    hipLaunchKernelGGL(k_wide_rehash, dim3(2048), dim3(256), 0, s, from, to, ctl);
}

void launch_wide_token_weights(hipStream_t s, const uint32_t *tok, uint64_t n_tok, const uint32_t *weights,
                               uint64_t n_weights, uint32_t *wt, uint32_t *span_scratch, WideCtl *ctl) {
    if (!n_tok) return;
    const Scratch sc = carve(span_scratch, n_tok);
    const dim3 grid(span_grid(n_tok)), block(kSpanThreads);
    hipLaunchKernelGGL(k_wide_end_count, grid, block, 0, s, tok, n_tok, sc.span_keep);
    hipLaunchKernelGGL(k_wide_scan_ends, dim3(1), dim3(kScanThreads), 0, s, sc.span_keep, n_tok, sc.span_off);
    hipLaunchKernelGGL(k_wide_fill_weights, grid, block, 0, s, tok, n_tok, sc.span_off, weights, n_weights, wt, ctl);
}

void launch_wide_check_weights(hipStream_t s, const uint32_t *weights, uint64_t n, uint32_t *flag) {
    if (!n) return;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_wide_check_weights, dim3(blocks), dim3(256), 0, s, weights, n, flag);
}

void launch_wide_pair_count_tokens(hipStream_t s, const uint32_t *tok, const uint32_t *wt, uint64_t n_tok, uint32_t ids,
                                   WideTable t, WideCtl *ctl, WideTally *tally, int n_cus) {
    if (n_tok >= 2) {
        // 8 workgroups of 12 KiB LDS per CU; a workgroup's share is at least 4,096 tokens (so that the flush of its
        // cache is paid for) and at most 2^20 (LDS counts cannot wrap)
        uint64_t blocks = (uint64_t)(n_cus > 0 ? n_cus : 256) * 8;
        blocks = std::min<uint64_t>(blocks, (n_tok + 4095) / 4096);
        blocks = std::max<uint64_t>(blocks, (n_tok + (1u << 20) - 1) >> 20);
        if (wt)
            hipLaunchKernelGGL(k_wide_pair_count_tokens<true>, dim3((uint32_t)blocks), dim3(kWpThreads), 0, s, tok, wt, n_tok,
                               ids, t, ctl, tally);
        else
            hipLaunchKernelGGL(k_wide_pair_count_tokens<false>, dim3((uint32_t)blocks), dim3(kWpThreads), 0, s, tok, wt, n_tok,
                               ids, t, ctl, tally);
    }
    const uint64_t slots = (uint64_t)t.mask + 1;
    const uint32_t tb = (uint32_t)std::min<uint64_t>((slots + 1023) / 1024, 4096);
    hipLaunchKernelGGL(k_wide_table_tally, dim3(tb), dim3(256), 0, s, t, tally);
    hipLaunchKernelGGL(k_wide_resume_check, dim3(1), dim3(1), 0, s, tally, ctl);
}

// (the scans are limited by a length array, the final stage also by a minimal count alone)
void launch_wide_argmax(hipStream_t s, WideTable t, WideCtl *ctl, WideBest *best, unsigned long long *scratch, WideLimits lim) {
    const uint32_t *len = lim.len;
    if (len)
        hipLaunchKernelGGL(k_wide_argmax_partial<true>, dim3(kArgBlocks), dim3(256), 0, s, t, ctl, scratch, len, lim.max_len);
    else
        hipLaunchKernelGGL(k_wide_argmax_partial<false>, dim3(kArgBlocks), dim3(256), 0, s, t, ctl, scratch, len, 0u);
    if (len || lim.min_count)
        hipLaunchKernelGGL(k_wide_argmax_final<true>, dim3(1), dim3(kArgBlocks), 0, s, scratch, ctl, best, lim);
    else
        hipLaunchKernelGGL(k_wide_argmax_final<false>, dim3(1), dim3(kArgBlocks), 0, s, scratch, ctl, best, lim);
}

void launch_wide_first(hipStream_t s, const uint32_t *src, uint64_t n_upper, WideTable t, WideCtl *ctl, WideBest *best,
                       const unsigned long long *scratch, WideFirst *fs, WideLimits lim) {
    const uint32_t *len = lim.len;
    if (len)
        hipLaunchKernelGGL(k_wide_first_gather<true>, dim3(kArgBlocks), dim3(256), 0, s, t, ctl, scratch, fs, len, lim.max_len);
    else
        hipLaunchKernelGGL(k_wide_first_gather<false>, dim3(kArgBlocks), dim3(256), 0, s, t, ctl, scratch, fs, len, 0u);
    if (n_upper) {
        const uint32_t blocks = std::min<uint32_t>(span_grid(n_upper), kPosBlocks);
        if (len)
            hipLaunchKernelGGL(k_wide_first_pos<true>, dim3(blocks), dim3(kSpanThreads), 0, s, src, t, ctl, fs, len, lim.max_len);
        else
            hipLaunchKernelGGL(k_wide_first_pos<false>, dim3(blocks), dim3(kSpanThreads), 0, s, src, t, ctl, fs, len, 0u);
    }
    if (len)
        hipLaunchKernelGGL(k_wide_first_pick<true>, dim3(1), dim3(256), 0, s, src, ctl, best, fs, lim);
    else
        hipLaunchKernelGGL(k_wide_first_pick<false>, dim3(1), dim3(256), 0, s, src, ctl, best, fs, lim);
}

void launch_wide_merge(hipStream_t s, const uint32_t *src, uint32_t *dst, uint64_t n_upper, uint32_t *val,
                       uint32_t *span_scratch, WideTable t, WideCtl *ctl, uint32_t new_id_base, const uint32_t *wsrc,
                       uint32_t *wdst) {
    if (!n_upper) return;
    const Scratch sc = carve(span_scratch, n_upper);
    const dim3 grid(span_grid(n_upper)), block(kSpanThreads);
    hipLaunchKernelGGL(k_wide_cand, grid, block, 0, s, src, ctl, sc.span_sum);
    hipLaunchKernelGGL(k_wide_scan_parity, dim3(1), dim3(kScanThreads), 0, s, sc.span_sum, ctl, sc.in_par);
    if (wsrc)
        hipLaunchKernelGGL(k_wide_match<true>, grid, block, 0, s, src, wsrc, sc.in_par, val, sc.span_keep, t, ctl, new_id_base);
    else
        hipLaunchKernelGGL(k_wide_match<false>, grid, block, 0, s, src, wsrc, sc.in_par, val, sc.span_keep, t, ctl, new_id_base);
    hipLaunchKernelGGL(k_wide_scan_sum, dim3(1), dim3(kScanThreads), 0, s, sc.span_keep, (uint64_t)0, sc.span_off, ctl, 1);
    if (wsrc)
        hipLaunchKernelGGL(k_wide_scatter<true>, grid, block, 0, s, val, sc.span_off, dst, ctl, wsrc, wdst);
    else
        hipLaunchKernelGGL(k_wide_scatter<false>, grid, block, 0, s, val, sc.span_off, dst, ctl, wsrc, wdst);
}

}  // namespace mbpe
