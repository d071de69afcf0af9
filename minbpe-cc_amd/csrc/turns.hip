// Conversations on the device: (tokens, doc_off of n_docs turns, turn_off, flags) -> (joined tokens, targets, doc_off'
// of n_convs documents), between encode and pack.  The rule is turns.h's; this file runs it.
//
//   k_turns_len      one lane per turn, one wave per span of 1,024 turns: len + has_end, the span's sum
//   k_turns_scan     one workgroup: span.h's 64-bit scan over the spans' sums; the total goes behind the array
//   k_turns_offsets  the spans again: a wave prefix sum turns the widths into pos, the turns' starts in G, in place
//   k_turns_plan     one lane per conversation: turns_keep over pos -- for DROP_OLDEST a binary search of pos and the
//                    TRAIN skip over flags -- leaves the kept ranges (g0, a, g1, b), (dropped, cut) and the kept length;
//                    the scan and the offsets kernel once more turn the lengths into the n_convs + 1 output offsets
//   k_turns_place    one lane per RECORD.  A conversation of m turns has m + 1 records, one per turn and one for its end
//                    id, so record turn_off[c] + c + i is turn i of conversation c; a lane finds c by a binary search of
//                    turn_off.  A record is 16 bytes: where its ids begin in OUTPUT coordinates (the conversation's
//                    offset + turns_below of the turn's start), four bits -- the turn-end id is kept, trained, an end-id
//                    record, begins its conversation -- and the token offset of its first kept token.  Records that keep
//                    nothing (dropped turns, a cut turn, no end id) have no width: they share their successor's start.
//                    The record behind the last holds the joined token count, so "where the next begins" always exists.
//   k_turns_gather   ids and targets in one pass.  OUTPUT-centric like k_textpair_gather: the joined stream is cut at the
//                    16-byte boundaries of its global address, a lane owns one such piece and a wave 16 rounds of 64
//                    neighbouring pieces.  What differs is finding the turn.  At the start of its span lane 0 searches the
//                    records for the one that holds the span's first id and broadcasts it; the wave loads that record
//                    and the kTnTable - 1 behind it into LDS, 16 bytes a lane, coalesced; from then on a lane finds the
//                    record of its piece by a binary search of LDS (8 steps), and only a piece behind the table's last
//                    record -- a span with more than kTnTable - 1 record boundaries: runs of empty and one-token turns --
//                    searches the records in global memory from there on.
//                    A piece that lies inside one record's tokens is a copy: a dwordx4 load where source and destination
//                    are mutually aligned, else loads of the token's width.  Any other piece goes id by id, walking the
//                    records forward.  Beside every id the lane keeps one bit: may this position be a label, i.e. it does
//                    not begin a conversation and -- LABEL_TRAINED -- is trained.  A target is the id one position on
//                    where that position's bit is set: from the lane's registers, at a piece end from the next lane by
//                    two shuffles, and only lane 63 looks the position up.  Stores are dwordx4; only the first and last
//                    piece of the stream can be partial, and a target address off 16 bytes goes word by word.
// LDS: kTnTable (256) records of 16 bytes per wave, 16 KiB per workgroup of 4 waves.
// Every index is 64-bit.  No atomics; nothing is waited for in turns_launch.
//
// Bytes moved per joined id: read once (2 or 4 B), written once (2 or 4 B), target written once (4 B).  Per turn: 17 B
// read and 8 B written by k_turns_len, 8 B rewritten by the offsets, 41 B read and 16 B written by k_turns_place (beside
// its search of turn_off and its conversation's 48 B, which neighbouring lanes share), 16 B read by every wave whose
// table holds it.  Per conversation: 16 B of turn_off and two words of pos read and 56 B written by the plan, 8 B
// rewritten by the offsets, one more record.
#include "turns.h"

#include "hip_host.h"

#include <algorithm>
#include <new>
#include <string>
#include <vector>

namespace {

using namespace mbpe;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int kTnTable = 256;                                    // records a wave keeps in LDS
constexpr u64 kRecEndKept = 1ull << 63, kRecTrained = 1ull << 62, kRecIsEnd = 1ull << 61, kRecOpens = 1ull << 60;
constexpr u64 kRecPos = kRecOpens - 1;

__global__ __launch_bounds__(kSpanThreads) void k_turns_len(const u64 *__restrict__ doc_off, const uint8_t *__restrict__ flags,
                                                             uint64_t n_docs, mbpe_turns_spec spec, u64 *__restrict__ pos,
                                                             u64 *__restrict__ span_cnt) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n_docs) return;
    const uint32_t lane = lane_id();
    u64 s = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t t = base + (uint64_t)it * kWave + lane;
        if (t < n_docs) {
            const u64 w = turns_width(spec, doc_off[t + 1] - doc_off[t], flags[t]);
            pos[t] = w;
            s += w;
        }
    }
    for (int k = kWave / 2; k > 0; k >>= 1) s += __shfl_down(s, k, kWave);
    if (lane == 0) span_cnt[span] = s;
}

__global__ __launch_bounds__(kScanThreads) void k_turns_scan(u64 *__restrict__ span_cnt, uint64_t n_spans, u64 *__restrict__ total) {
    __shared__ u64 sh[kScanThreads];
    const u64 sum = span_scan_sum64(span_cnt, n_spans, sh);
    if (threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(kSpanThreads) void k_turns_offsets(u64 *__restrict__ off, uint64_t n, const u64 *__restrict__ span_off) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    u64 o = span_off[span];
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        const u64 w = i < n ? off[i] : 0ull;
        const u64 incl = wave_prefix64(w, lane);
        if (i < n) off[i] = o + incl - w;
        o += __shfl(incl, kWave - 1, kWave);
    }
}

__global__ __launch_bounds__(kSpanThreads) void k_turns_plan(const u64 *__restrict__ pos, const u64 *__restrict__ turn_off,
                                                              const uint8_t *__restrict__ flags, uint64_t n_convs,
                                                              mbpe_turns_spec spec, u64 *__restrict__ off, u64 *__restrict__ plan,
                                                              u64 *__restrict__ info, u64 *__restrict__ span_cnt) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n_convs) return;
    const uint32_t lane = lane_id();
    u64 s = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t c = base + (uint64_t)it * kWave + lane;
        if (c < n_convs) {
            const u64 t0 = turn_off[c], t1 = turn_off[c + 1];
            const TnKeep k = turns_keep(spec, pos + t0, flags + t0, t1 - t0);
            const u64 n = turns_len(k);
            plan[4 * c] = k.g0;
            plan[4 * c + 1] = k.a;
            plan[4 * c + 2] = k.g1;
            plan[4 * c + 3] = k.b;
            info[2 * c] = k.dropped;
            info[2 * c + 1] = k.cut;
            off[c] = n;
            s += n;
        }
    }
    for (int k = kWave / 2; k > 0; k >>= 1) s += __shfl_down(s, k, kWave);
    if (lane == 0) span_cnt[span] = s;
}

struct TnJob {
    const void *tok;
    const u64 *doc_off;                      // n_docs + 1
    const u64 *turn_off;                     // n_convs + 1
    const uint8_t *flags;
    const u64 *pos;                          // n_docs + 1
    const u64 *off;                          // n_convs + 1; off[n_convs] = ids of the output
    const u64 *plan;
    u64 *rec;                                // 2 * (n_rec + 1)
    uint64_t n_docs, n_convs, n_rec;         // n_rec = n_docs + n_convs
    void *out;
    uint32_t *tgt;                           // NULL: no targets
    uint64_t cap;                            // ids the outputs hold
    mbpe_turns_spec spec;
};

__global__ __launch_bounds__(kSpanThreads) void k_turns_place(TnJob j) {
    const uint64_t r = (uint64_t)blockIdx.x * kSpanThreads + threadIdx.x;
    if (r > j.n_rec) return;
    if (r == j.n_rec) {                                          // behind the last record: where the stream ends
        j.rec[2 * r] = j.off[j.n_convs];
        j.rec[2 * r + 1] = 0;
        return;
    }
    uint64_t c = 0, hi = j.n_convs;                              // turn_off[c] + c <= r < turn_off[hi] + hi
    while (hi - c > 1) {
        const uint64_t m = c + (hi - c) / 2;
        if (j.turn_off[m] + m <= r) c = m;
        else hi = m;
    }
    const u64 t0 = j.turn_off[c], t1 = j.turn_off[c + 1], i = r - (t0 + c);
    const TnKeep k = {j.plan[4 * c], j.plan[4 * c + 1], j.plan[4 * c + 2], j.plan[4 * c + 3], 0, 0, 0};
    const u64 o = j.off[c];
    u64 word, src = 0;
    if (i < t1 - t0) {
        const u64 t = t0 + i, p0 = j.pos[t], p1 = j.pos[t + 1], d0 = j.doc_off[t], len = j.doc_off[t + 1] - d0;
        const u64 b0 = turns_below(k, p0), bt = turns_below(k, p0 + len), b1 = turns_below(k, p1);
        word = o + b0;
        if (b1 > bt) word |= kRecEndKept;
        if (j.flags[t] & kTnTrain) word |= kRecTrained;
        if (b0 == 0) word |= kRecOpens;
        if (bt > b0) {                                           // the first token kept: in the first range or the second
            const bool first = k.a && p0 + len > k.g0 && p0 < k.g0 + k.a;
            const u64 g = first ? (p0 > k.g0 ? p0 : k.g0) : (p0 > k.g1 ? p0 : k.g1);
            src = d0 + (g - p0);
        }
    } else {
        word = (o + k.a + k.b) | kRecIsEnd;
        if (t1 > t0 && (j.flags[t1 - 1] & kTnTrain)) word |= kRecTrained;
        if (k.a + k.b == 0) word |= kRecOpens;
    }
    j.rec[2 * r] = word;
    j.rec[2 * r + 1] = src;
}

template <int BITS>
__device__ __forceinline__ uint32_t tn_tok(const void *__restrict__ tok, u64 i) {
    return BITS == 16 ? (uint32_t) static_cast<const uint16_t *>(tok)[i] : static_cast<const uint32_t *>(tok)[i] & kTokIdMask;
}

// the records as a lane sees them: those of the wave's table from LDS, any other (r <= n_rec) from global memory
struct TnTab {
    const u64 *rec;
    const u64 *lds;                          // word, src per entry
    uint64_t r0;
    uint32_t n;                              // entries: records r0 .. r0 + n - 1
    __device__ __forceinline__ u64 word(uint64_t r) const { return r - r0 < n ? lds[2 * (r - r0)] : rec[2 * r]; }
    __device__ __forceinline__ u64 src(uint64_t r) const { return r - r0 < n ? lds[2 * (r - r0) + 1] : rec[2 * r + 1]; }
};

// the largest record in [lo, hi) that begins at or before f, over global memory: word(lo) <= f < word(hi), hi <= n_rec
__device__ __forceinline__ uint64_t tn_search(const u64 *__restrict__ rec, uint64_t lo, uint64_t hi, u64 f) {
    while (hi - lo > 1) {
        const uint64_t m = lo + (hi - lo) / 2;
        if ((rec[2 * m] & kRecPos) <= f) lo = m;
        else hi = m;
    }
    return lo;
}

// the record that holds output position f (at or behind the first position of the wave's span, below the stream's end)
__device__ __forceinline__ uint64_t tn_find(const TnTab &tb, uint64_t n_rec, u64 f) {
    if (f >= (tb.lds[2 * (tb.n - 1)] & kRecPos)) return tn_search(tb.rec, tb.r0 + tb.n - 1, n_rec, f);
    uint32_t lo = 0, hi = tb.n - 1;                              // lds word(lo) <= f < lds word(hi)
    while (hi - lo > 1) {
        const uint32_t m = (lo + hi) / 2;
        if ((tb.lds[2 * m] & kRecPos) <= f) lo = m;
        else hi = m;
    }
    return tb.r0 + lo;
}

// where a lane stands: record r of `wdt` ids, at its id `at`
struct TnAt {
    uint64_t r;
    u64 word, wdt, at;
};

__device__ __forceinline__ void tn_enter(const TnTab &tb, uint64_t r, TnAt *w) {
    w->r = r;
    w->word = tb.word(r);
    w->wdt = (tb.word(r + 1) & kRecPos) - (w->word & kRecPos);
}

// the id where the lane stands, after stepping over the records that have ended (a record with ids follows: the
// position lies below the stream's end); *lab: may it be a label
template <int BITS>
__device__ __forceinline__ uint32_t tn_id(const TnJob &j, const TnTab &tb, TnAt *w, bool *lab) {
    while (w->at >= w->wdt) {
        tn_enter(tb, w->r + 1, w);
        w->at = 0;
    }
    *lab = (j.spec.label_mode == kTnLabelAll || (w->word & kRecTrained)) && !((w->word & kRecOpens) && w->at == 0);
    if (w->word & kRecIsEnd) return j.spec.end_id;
    if ((w->word & kRecEndKept) && w->at + 1 == w->wdt) return j.spec.turn_end_id;
    return tn_tok<BITS>(j.tok, tb.src(w->r) + w->at);
}

template <int BITS>
__global__ __launch_bounds__(kSpanThreads) void k_turns_gather(TnJob j) {
    constexpr uint32_t ob = BITS / 8, PER = 128 / BITS;
    __shared__ u64 table[kSpanWaves][2 * kTnTable];
    const u64 total = j.off[j.n_convs];
    const uint64_t n_out = total < j.cap ? total : j.cap;        // (they are equal or the buffers are larger)
    const uint64_t A = (uint64_t)(uintptr_t)j.out, E = A + n_out * ob, B0 = A & ~15ull;
    const uint64_t n_pieces = (E - B0 + 15) >> 4;
    const uint64_t p0 = span_index() * kSpan;                    // a wave's span: 1,024 pieces in 16 rounds
    const bool live = p0 < n_pieces && n_out;
    const uint32_t lane = lane_id();
    u64 *lds = table[threadIdx.x / kWave];
    TnTab tb = {j.rec, lds, 0, 0};
    if (live) {
        const uint64_t B = B0 + (p0 << 4);
        const u64 f0 = B > A ? (B - A) / ob : 0;                 // the span's first position (below n_out: p0 < n_pieces)
        uint64_t r0 = 0;
        if (lane == 0) r0 = tn_search(j.rec, 0, j.n_rec, f0);
        r0 = __shfl(r0, 0, kWave);
        const uint64_t left = j.n_rec + 1 - r0;                  // records from r0 on, the one behind the last included: >= 2
        tb.r0 = r0;
        tb.n = left < (uint64_t)kTnTable ? (uint32_t)left : (uint32_t)kTnTable;
        for (uint32_t i = lane; i < tb.n; i += kWave) {
            lds[2 * i] = j.rec[2 * (r0 + i)];
            lds[2 * i + 1] = j.rec[2 * (r0 + i) + 1];
        }
    }
    __syncthreads();
    if (!live) return;
    uint8_t *base = static_cast<uint8_t *>(j.out);
    for (int it = 0; it < kSpanIters; ++it) {                    // (every lane runs every round: the shuffles below)
        const uint64_t p = p0 + (uint64_t)it * kWave + lane;
        const uint64_t B = B0 + (p << 4);
        const uint64_t lo = B > A ? B : A;
        const uint64_t hi = B + 16 < E ? B + 16 : E;
        const uint32_t cnt = p < n_pieces && hi > lo ? (uint32_t)(hi - lo) / ob : 0u;
        const uint64_t f = (lo - A) / ob;
        uint32_t id[PER];
        uint32_t lab = 0;                                        // bit e: position f + e may be a label
        TnAt w = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t e = 0; e < PER; ++e) id[e] = 0u;
        if (cnt) {
            tn_enter(tb, tn_find(tb, j.n_rec, f), &w);
            w.at = f - (w.word & kRecPos);
            const u64 ntok = w.word & kRecIsEnd ? 0 : w.wdt - (w.word >> 63);
            if (w.at + cnt <= ntok) {                            // a copy out of one turn
                const u64 s = tb.src(w.r) + w.at;
                const uint8_t *src = static_cast<const uint8_t *>(j.tok) + s * ob;
                if (cnt == PER && ((uint64_t)(uintptr_t)src & 15ull) == 0) {
                    const u32x4 q = *static_cast<const u32x4 *>(__builtin_assume_aligned(src, 16));
                    const uint32_t v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                    for (uint32_t e = 0; e < PER; ++e)
                        id[e] = BITS == 16 ? (v[e / 2] >> (16 * (e & 1))) & 0xFFFFu : v[e] & kTokIdMask;
                } else {
#pragma unroll
                    for (uint32_t e = 0; e < PER; ++e)
                        if (e < cnt) id[e] = tn_tok<BITS>(j.tok, s + e);
                }
                if (j.spec.label_mode == kTnLabelAll || (w.word & kRecTrained)) lab = (1u << cnt) - 1u;
                if ((w.word & kRecOpens) && w.at == 0) lab &= ~1u;
                w.at += cnt;
            } else {                                             // a turn-end id, an end id or a record boundary inside
#pragma unroll
                for (uint32_t e = 0; e < PER; ++e) {
                    if (e < cnt) {
                        bool l;
                        id[e] = tn_id<BITS>(j, tb, &w, &l);
                        lab |= (l ? 1u : 0u) << e;
                        ++w.at;
                    }
                }
            }
        }
        // ---- the ids ----
        if (cnt == PER) {                                        // (then lo == B)
            u32x4 q;
            if (BITS == 16) {
                q.x = id[0] | id[1 % PER] << 16;
                q.y = id[2 % PER] | id[3 % PER] << 16;
                q.z = id[4 % PER] | id[5 % PER] << 16;
                q.w = id[6 % PER] | id[7 % PER] << 16;
            } else {
                q.x = id[0]; q.y = id[1]; q.z = id[2]; q.w = id[3];
            }
            *static_cast<u32x4 *>(__builtin_assume_aligned(base + (B - A), 16)) = q;
        } else if (BITS == 16) {                                 // the first or the last piece of the output
            uint16_t *dst = reinterpret_cast<uint16_t *>(base + (lo - A));
            for (uint32_t e = 0; e < cnt; ++e) dst[e] = (uint16_t)id[e];
        } else {
            uint32_t *dst = reinterpret_cast<uint32_t *>(base + (lo - A));
            for (uint32_t e = 0; e < cnt; ++e) dst[e] = id[e];
        }
        // ---- the targets ----
        if (j.tgt == nullptr) continue;                          // (uniform)
        uint32_t behind = __shfl_down(id[0], 1, kWave);          // the next piece's first id, and may it be a label
        uint32_t behind_lab = __shfl_down(lab & 1u, 1, kWave);
        if (lane == kWave - 1) {
            behind_lab = 0;
            if (cnt && f + cnt < total) {
                bool l;
                behind = tn_id<BITS>(j, tb, &w, &l);
                behind_lab = l ? 1u : 0u;
            }
        }
        uint32_t t[PER];
#pragma unroll
        for (uint32_t e = 0; e < PER; ++e) {
            const bool in = e + 1 < PER && e + 1 < cnt;
            const uint32_t nx = in ? id[(e + 1) % PER] : behind;
            const uint32_t nl = in ? lab >> ((e + 1) % PER) & 1u : behind_lab;
            t[e] = nl ? nx : kTokNone;
        }
        uint32_t *dst = j.tgt + f;
        if (cnt == PER && ((uint64_t)(uintptr_t)dst & 15ull) == 0) {
            u32x4 *q = static_cast<u32x4 *>(__builtin_assume_aligned(dst, 16));
#pragma unroll
            for (uint32_t v = 0; v < PER / 4; ++v) {
                u32x4 x;
                x.x = t[4 * v]; x.y = t[4 * v + 1]; x.z = t[4 * v + 2]; x.w = t[4 * v + 3];
                q[v] = x;
            }
        } else {
#pragma unroll
            for (uint32_t e = 0; e < PER; ++e)
                if (e < cnt) dst[e] = t[e];
        }
    }
}

#define TCHK(expr) MBPE_HIP_CHECK(expr, true)

// device time of the calling thread's latest mbpe_turns_tokens (mbpe_turns_kernel_ms)
thread_local float g_turns_ms = 0.f;

struct TurnsCall {
    const void *tokens;
    uint64_t n_tokens;
    uint32_t token_bits;
    int tokens_on_device;
    const uint64_t *doc_tok_off;
    uint64_t n_docs;
    const uint64_t *turn_off;
    uint64_t n_convs;
    const uint8_t *flags;
    const mbpe_turns_spec *spec;
};

int turns_run(int device_id, const TurnsCall &a, void *tokens_out, uint32_t *targets_out, uint64_t n_new, int out_on_device) {
    int rc = find_device(device_id);
    if (rc != MBPE_OK) return rc;
    OneShot dev;
    rc = dev.open(device_id);
    if (rc != MBPE_OK) return rc;
    const uint64_t tb = a.token_bits / 8;
    void *d_tok = const_cast<void *>(a.tokens), *d_off = nullptr, *d_turn = nullptr, *d_flags = nullptr, *d_out = tokens_out,
         *d_tgt = targets_out, *d_pos = nullptr, *d_new = nullptr, *d_plan = nullptr, *d_info = nullptr, *d_rec = nullptr;
    if (!a.tokens_on_device) rc = dev.alloc(&d_tok, a.n_tokens * tb, a.tokens);
    if (rc == MBPE_OK) rc = dev.alloc(&d_off, (a.n_docs + 1) * 8, a.doc_tok_off);
    if (rc == MBPE_OK) rc = dev.alloc(&d_turn, (a.n_convs + 1) * 8, a.turn_off);
    if (rc == MBPE_OK) rc = dev.alloc(&d_flags, a.n_docs, a.flags);
    if (rc == MBPE_OK && !out_on_device) rc = dev.alloc(&d_out, n_new * tb, nullptr);
    if (rc == MBPE_OK && !out_on_device && targets_out) rc = dev.alloc(&d_tgt, n_new * 4, nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_pos, turns_pos_bytes(a.n_docs), nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_new, turns_off_bytes(a.n_convs), nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_plan, a.n_convs * 32, nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_info, a.n_convs * 16, nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_rec, turns_rec_bytes(a.n_docs, a.n_convs), nullptr);
    if (rc != MBPE_OK) return rc;
    const TurnsSrc src = {d_tok, a.token_bits, static_cast<const u64 *>(d_off), a.n_docs, static_cast<const u64 *>(d_turn),
                          a.n_convs, static_cast<const uint8_t *>(d_flags)};
    const TurnsDst dst = {d_out, static_cast<uint32_t *>(d_tgt), n_new, static_cast<u64 *>(d_pos), static_cast<u64 *>(d_new),
                          static_cast<u64 *>(d_plan), static_cast<u64 *>(d_info), static_cast<u64 *>(d_rec)};
    TCHK(hipEventRecord(dev.ev0, dev.stream));
    turns_launch(dev.stream, src, *a.spec, dst);
    rc = dev.finish(&g_turns_ms);
    if (rc != MBPE_OK) return rc;
    if (!out_on_device) {
        TCHK(hipMemcpyAsync(tokens_out, d_out, n_new * tb, hipMemcpyDeviceToHost, dev.stream));
        if (targets_out) TCHK(hipMemcpyAsync(targets_out, d_tgt, n_new * 4, hipMemcpyDeviceToHost, dev.stream));
        TCHK(hipStreamSynchronize(dev.stream));
    }
    return MBPE_OK;
}

// what mbpe_turns_plan and mbpe_turns_tokens check alike, then the host's plan into off_out (n_convs + 1) and info_out
int turns_host_plan(const std::string &who, const TurnsCall &a, uint64_t *off_out, uint64_t *info_out) {
    const char *msg = "";
    int rc = turns_check_spec(a.spec, a.token_bits, &msg);
    if (rc == MBPE_OK) rc = turns_check_arrays(a.turn_off, a.n_convs, a.flags, a.n_docs, &msg);
    if (rc != MBPE_OK) return fail(rc, who + ": " + msg);
    rc = mbpe_host::check_doc_tok_off(a.doc_tok_off, a.n_docs, a.n_tokens);
    if (rc != MBPE_OK) return rc;
    if (a.n_tokens >> 40 || a.n_docs >> 40 || a.n_convs >> 40)
        return fail(MBPE_ERR_ARG, who + ": more than 2^40 tokens, turns or conversations");
    std::vector<unsigned long long> pos(a.n_docs + 1, 0);
    std::vector<uint64_t> off(a.n_convs + 1, 0), info(2 * a.n_convs, 0);     // (nothing is written where a check fails)
    turns_plan_host(a.doc_tok_off, a.n_docs, a.turn_off, a.n_convs, a.flags, *a.spec, pos.data(), off.data(), info.data());
    std::copy(off.begin(), off.end(), off_out);
    if (info_out) std::copy(info.begin(), info.end(), info_out);
    return MBPE_OK;
}

}  // namespace

namespace mbpe {

uint64_t turns_pos_bytes(uint64_t n_docs) { return (n_docs + 1 + span_count(n_docs)) * 8; }
uint64_t turns_off_bytes(uint64_t n_convs) { return (n_convs + 1 + span_count(n_convs)) * 8; }
uint64_t turns_rec_bytes(uint64_t n_docs, uint64_t n_convs) { return (n_docs + n_convs + 1) * 16; }

void turns_launch(hipStream_t stream, const TurnsSrc &src, const mbpe_turns_spec &spec, const TurnsDst &dst) {
    const uint64_t n_docs = src.n_docs, n_convs = src.n_convs;
    u64 *pos_cnt = dst.pos + n_docs + 1, *off_cnt = dst.off + n_convs + 1;   // (turns_pos_bytes, turns_off_bytes)
    const dim3 block(kSpanThreads), one(1), scan(kScanThreads);
    if (n_docs)
        hipLaunchKernelGGL(k_turns_len, dim3(span_grid(n_docs)), block, 0, stream, src.doc_off, src.flags, n_docs, spec,
                           dst.pos, pos_cnt);
    hipLaunchKernelGGL(k_turns_scan, one, scan, 0, stream, pos_cnt, span_count(n_docs), dst.pos + n_docs);
    if (n_docs) hipLaunchKernelGGL(k_turns_offsets, dim3(span_grid(n_docs)), block, 0, stream, dst.pos, n_docs, pos_cnt);
    const dim3 cgrid(span_grid(n_convs));
    hipLaunchKernelGGL(k_turns_plan, cgrid, block, 0, stream, dst.pos, src.turn_off, src.flags, n_convs, spec, dst.off,
                       dst.plan, dst.info, off_cnt);
    hipLaunchKernelGGL(k_turns_scan, one, scan, 0, stream, off_cnt, span_count(n_convs), dst.off + n_convs);
    hipLaunchKernelGGL(k_turns_offsets, cgrid, block, 0, stream, dst.off, n_convs, off_cnt);
    if (dst.cap == 0) return;
    const TnJob j = {src.tok, src.doc_off, src.turn_off, src.flags, dst.pos, dst.off, dst.plan, dst.rec, n_docs, n_convs,
                     n_docs + n_convs, dst.tok, dst.tgt, dst.cap, spec};
    const uint64_t n_place = j.n_rec + 1;
    hipLaunchKernelGGL(k_turns_place, dim3((uint32_t)((n_place + kSpanThreads - 1) / kSpanThreads)), block, 0, stream, j);
    const uint64_t A = (uint64_t)(uintptr_t)dst.tok, E = A + dst.cap * (src.bits / 8);
    const uint64_t n_pieces = (E - (A & ~15ull) + 15) >> 4;      // (no fewer than the kernel finds: it stops at off[n])
    const dim3 ggrid(span_grid(n_pieces));
    if (src.bits == 16) hipLaunchKernelGGL((k_turns_gather<16>), ggrid, block, 0, stream, j);
    else hipLaunchKernelGGL((k_turns_gather<32>), ggrid, block, 0, stream, j);
}

}  // namespace mbpe

extern "C" {

int mbpe_turns_plan(const uint64_t *doc_tok_off, uint64_t n_docs, const uint64_t *turn_off, uint64_t n_convs,
                    const uint8_t *flags, const mbpe_turns_spec *spec, uint64_t *doc_tok_off_out, uint64_t *kept_out) {
    if (!doc_tok_off || !spec || !doc_tok_off_out) return fail(MBPE_ERR_ARG, "mbpe_turns_plan: NULL argument");
    try {
        const TurnsCall a = {nullptr, doc_tok_off[n_docs], 32, 0, doc_tok_off, n_docs, turn_off, n_convs, flags, spec};
        return turns_host_plan("mbpe_turns_plan", a, doc_tok_off_out, kept_out);
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_turns_plan: host allocation failed");
    }
}

int mbpe_turns_tokens(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                      const uint64_t *doc_tok_off, uint64_t n_docs, const uint64_t *turn_off, uint64_t n_convs,
                      const uint8_t *flags, const mbpe_turns_spec *spec, void *tokens_out, uint32_t *targets_out,
                      uint64_t cap, int out_on_device, uint64_t *doc_tok_off_out, uint64_t *kept_out, uint64_t *n_out) {
    if (n_out) *n_out = 0;
    if (!n_out || !doc_tok_off || !spec || (!tokens && n_tokens)) return fail(MBPE_ERR_ARG, "mbpe_turns_tokens: NULL argument");
    if (token_bits != 16 && token_bits != 32) return fail(MBPE_ERR_ARG, "mbpe_turns_tokens: token_bits must be 16 or 32");
    try {
        const TurnsCall a = {tokens, n_tokens, token_bits, tokens_on_device, doc_tok_off, n_docs, turn_off, n_convs, flags, spec};
        std::vector<uint64_t> off(n_convs + 1, 0), info(2 * n_convs, 0);
        int rc = turns_host_plan("mbpe_turns_tokens", a, off.data(), info.data());
        if (rc != MBPE_OK) return rc;
        const uint64_t n_new = off[n_convs];
        *n_out = n_new;
        if (tokens_out && cap < n_new) return fail(MBPE_ERR_ARG, "mbpe_turns_tokens: tokens_out too small");
        if (tokens_out && out_on_device &&
            ((uint64_t)(uintptr_t)tokens_out % (token_bits / 8) || (uint64_t)(uintptr_t)targets_out % 4))
            return fail(MBPE_ERR_ARG, "mbpe_turns_tokens: tokens_out or targets_out is not aligned to its elements");
        if (tokens_out && n_new) {
            rc = turns_run(device_id, a, tokens_out, targets_out, n_new, out_on_device);
            if (rc != MBPE_OK) return rc;
        }
        if (doc_tok_off_out) std::copy(off.begin(), off.end(), doc_tok_off_out);
        if (kept_out) std::copy(info.begin(), info.end(), kept_out);
        return MBPE_OK;
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_turns_tokens: host allocation failed");
    }
}

int mbpe_turns_kernel_ms(float *ms_out) {
    if (!ms_out) return fail(MBPE_ERR_ARG, "mbpe_turns_kernel_ms: NULL argument");
    *ms_out = g_turns_ms;
    return MBPE_OK;
}

}  // extern "C"
