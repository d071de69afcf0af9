// Encode on the device: internal_encode / internal_internal_encode (reference Tokenizer.h:325-377)
// for all chunks of a text at once.
//
// The reference encodes a chunk with repeated left-to-right passes; a pass replaces ANY pair found in
// merges_lookup (first match wins, not rank order: `i += 2` after a hit) and the passes stop when one
// makes no replacement (:325-367).  A pass looks sequential but is not: call position i a CANDIDATE when
// (t[i], t[i+1]) is in merges_lookup and both tokens belong to the same chunk, and let r[i] be the number
// of consecutive candidates immediately before i.  The walk replaces at i  <=>  i is a candidate and r[i]
// is even, and it drops t[i]  <=>  r[i] is odd (then i-1 was replaced and swallowed it).  r[i] is a
// segmented count, so a pass is: look up every pair -> parity of r by a scan -> compact.  Chunks never
// interact (a candidate never starts at the last token of a chunk), a chunk that no longer changes stays
// as it is, so passes over the whole text until nothing changes give every chunk its reference result.
//
// Layout: 32-bit tokens (the reference's Token, Tokenizer.h:37), bit 31 = "last token of its chunk".
// A span = 1,024 consecutive tokens = the unit one wave walks; spans are linked by two small scans (run parity,
// output offsets).  span.h holds the layout, the run arithmetic, the scans and the compaction.
//
// An mbpe_encoder keeps what does not change between calls: the pair -> id table on the device, a stream, and the
// work buffers (text, end mask, two token arrays, cand, span arrays), which grow when a call needs more.  A call
// cuts a text that does not fit into pieces at chunk boundaries and runs each through: widen -> passes -> one
// finishing kernel that writes the ids in the caller's format (32-bit with or without the flags, 16-bit) and, when
// the caller wants to know which tokens belong to which chunk, the position after every flagged token (per-span
// count of flags -> k_enc_scan_sum -> ranked write).  A text that lives on the device is read in place; the chunk
// starts whose byte is NUL are listed by a small kernel so that the host can parse those chunks.
//
// The _byteoff calls also say which text bytes every token stands for: after the passes, from the final stream, a
// length per id -> a 64-bit byte count per span -> one scan workgroup -> a ranked write with a wave prefix sum; the
// chunks that are one token by rule are patched with their chunk's length (see "token byte offsets" below).
//
// Option "rank_order": a pass replaces, in every chunk, only the candidates whose id is the smallest candidate id of
// that chunk -- k_enc_cand, then a segmented minimum of cand over the chunks (rank.h) and a filter, then the same
// parity scan, match, sum scan and scatter.  Passes repeat until one changes nothing, as above; for a trained table
// the result is the merges replayed in order, chunk by chunk.
//
// BPE-dropout (mbpe_encoder_set_dropout, rank order only; dropout.h): a candidate whose instance (byte start of its
// left token, merged id) is dropped becomes kTokNone in k_enc_cand, before span_sum is formed and before the rank
// kernels see it; everything after k_enc_cand is unchanged.  Tokens move when a pass compacts, so every token's byte
// start travels with it: org[i] (32 bits, relative to the piece), written by the widen kernel, carried by the scatter
// kernel beside the tokens and ping-ponged like them; a merged token keeps its left token's org.  With threshold 0
// none of this exists: the plain kernels are launched and no org buffer is reserved.
//
// Option "dedup" (no dropout, no byte offsets): a chunk's tokens depend on its bytes alone, so the call's chunks go
// through the encoder's own deduper (dedup.h, with the inverse map), the passes above run over the unique text as one
// piece, the finishing kernel writes a table of token runs in the caller's format, and the expansion (expand.h) copies
// every chunk's run to its place -- see enc_dedup_body.  With the option off none of this exists either.
//
// The count calls (mbpe_encoder_count, _count_endmask; hist.h): the encode calls as a query, plus a histogram of every
// piece's final stream into a scratch table of the call's own, which is folded into the kept table once nothing can
// fail any more.  On the "dedup" route the expansion is left out: the runs' weights are the histogram of the patched
// unique_of map, and the table of token runs is counted with them -- see dedup_count.  An encoder that is never asked
// to count has none of these buffers.
#include "dedup.h"
#include "denoise.h"
#include "dropout.h"
#include "expand.h"
#include "fim.h"
#include "mlm.h"
#include "hip_host.h"
#include "hist.h"
#include "pack.h"
#include "pack_fit.h"
#include "rank.h"
#include "span.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

namespace {

using namespace mbpe;

constexpr uint32_t kDrop = 0x7FFFFFFEu;    // byte of a chunk that collapses to one token (Tokenizer.h:86-93)
constexpr unsigned long long kEmptyKey = ~0ull;

struct EncLut {
    const unsigned long long *keys;        // (first << 32) | second, kEmptyKey when free
    const uint32_t *vals;                  // id of the merged token
    uint32_t shift;                        // 64 - log2(capacity)
    uint32_t mask;
};

__device__ __forceinline__ uint32_t enc_lookup(const EncLut &lut, uint32_t a, uint32_t b) {
    const unsigned long long key = ((unsigned long long)a << 32) | b;
    uint32_t h = pair_hash(key, lut.shift);
    for (;;) {
        const unsigned long long k = lut.keys[h];
        if (k == key) return lut.vals[h];
        if (k == kEmptyKey) return kTokNone;
        h = (h + 1) & lut.mask;
    }
}

// text_to_vector, Tokenizer.h:94-99 (char_to_token :80-82) + chunk ends; ORG: also every token's byte start in the
// piece (n <= 2^32 then: piece_limit)
template <bool ORG>
__global__ void k_enc_widen(const uint8_t *__restrict__ text, uint64_t n, const uint8_t *__restrict__ endmask,
                            uint32_t *__restrict__ tok, uint32_t *__restrict__ org) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const uint32_t e = (endmask[i >> 3] >> (i & 7)) & 1u;
        tok[i] = text[i] | (e ? kTokEnd : 0u);
        if (ORG) org[i] = (uint32_t)i;
    }
}

// chunks that are ONE token (NUL + a number: how encode passes special tokens, Tokenizer.h:635-637, :667-670)
struct SingleChunk { unsigned long long start, len; uint32_t id, pad; };
__global__ void k_enc_single(const SingleChunk *__restrict__ sc, uint32_t n_sc, uint32_t *__restrict__ tok) {
    const uint32_t c = blockIdx.x;
    if (c >= n_sc) return;
    const SingleChunk s = sc[c];
    for (unsigned long long i = threadIdx.x; i < s.len; i += blockDim.x)
        tok[s.start + i] = i == 0 ? (s.id | kTokEnd) : kDrop;
}

// pass, step 1: cand[i] = id of the token that (t[i], t[i+1]) merges to, or kTokNone; per span: are all its
// positions candidates, and the parity of its trailing run of candidates.  DROP: a candidate whose instance
// (piece_base + org[i], id) is dropped is none (org is read where the lookup hit only)
struct EncDrop { const uint32_t *org; unsigned long long piece_base, seed, threshold; };

template <bool DROP>
__global__ __launch_bounds__(kSpanThreads) void k_enc_cand(const uint32_t *__restrict__ tok, uint64_t n, EncLut lut,
                                                           uint32_t *__restrict__ cand,
                                                           uint32_t *__restrict__ span_sum, EncDrop drop) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    SpanSum sum = span_empty();
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        uint32_t nx;
        const uint32_t t = load_pair(tok, i, n, lane, kDrop, &nx);
        uint32_t c = kTokNone;
        if (i < n && !(t & kTokEnd) && t != kDrop && nx != kDrop) c = enc_lookup(lut, t, nx & kTokIdMask);
        if (DROP && c != kTokNone && dropout_dropped(drop.seed, drop.piece_base + drop.org[i], c, drop.threshold))
            c = kTokNone;
        if (i < n) cand[i] = c;
        sum = span_add_group(sum, __ballot(c != kTokNone));
    }
    if (lane == 0) span_sum[span] = span_pack(sum);
}

// ---- rank order (option "rank_order"): between k_enc_cand and the parity scan, every candidate above the smallest
// candidate id of its chunk becomes kTokNone (rank.h).  Two candidates of one chunk with the same id are the same
// pair, so what is left of a chunk are runs of one pair (a,a) and lone candidates: the run parity decides as before.

// per span: does it hold a chunk end, the minimum of cand up to and including its first end, and after its last one
__global__ __launch_bounds__(kSpanThreads) void k_enc_rank_sum(const uint32_t *__restrict__ tok, uint64_t n,
                                                               const uint32_t *__restrict__ cand,
                                                               RankSum *__restrict__ rank_sum) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    uint32_t h = kTokNone, t = kTokNone;
    bool seen = false;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        const uint32_t c = i < n ? cand[i] : kTokNone;
        const unsigned long long E = __ballot(i < n && (tok[i] & kTokEnd));
        h = rank_head_part(h, seen, E, lane, c);
        t = rank_tail_part(t, E, lane, c);
        seen = seen || E != 0ull;
    }
    h = wave_min(h);
    t = wave_min(t);
    if (lane == 0) rank_sum[span] = {seen ? 1u : 0u, h, t};
}

// what reaches every span of its chunk from the left and from the right
__global__ __launch_bounds__(kScanThreads) void k_enc_scan_min(const RankSum *__restrict__ rank_sum, uint64_t n_spans,
                                                               uint32_t *__restrict__ in_left,
                                                               uint32_t *__restrict__ in_right) {
    __shared__ RankSum sh_sum[kScanThreads];
    __shared__ uint32_t sh_l[kScanThreads], sh_r[kScanThreads];
    span_scan_min(rank_sum, n_spans, in_left, in_right, sh_sum, sh_l, sh_r);
}

// the filter: cand keeps the candidates that equal their chunk's minimum; span_sum as k_enc_cand writes it, of those
__global__ __launch_bounds__(kSpanThreads) void k_enc_rank_filter(const uint32_t *__restrict__ tok, uint64_t n,
                                                                  uint32_t *__restrict__ cand,
                                                                  const uint32_t *__restrict__ in_left,
                                                                  const uint32_t *__restrict__ in_right,
                                                                  uint32_t *__restrict__ span_sum) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    const unsigned long long lt = lanes_below(lane);
    uint32_t c[kSpanIters], m[kSpanIters], head[kSpanIters], tail[kSpanIters];
    unsigned long long E[kSpanIters];
#pragma unroll
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        c[it] = i < n ? cand[i] : kTokNone;
        E[it] = __ballot(i < n && (tok[i] & kTokEnd));
        m[it] = group_seg_min(c[it], E[it], lt, lane);
        // (lane 0's segment is the group's head; lane 63's its tail, unless lane 63 ends a chunk)
        head[it] = (uint32_t)__shfl((int)m[it], 0, kWave);
        tail[it] = E[it] >> 63 ? kTokNone : (uint32_t)__shfl((int)m[it], kWave - 1, kWave);
    }
    uint32_t left[kSpanIters], right[kSpanIters];
    uint32_t run = in_left[span];
#pragma unroll
    for (int it = 0; it < kSpanIters; ++it) {
        left[it] = run;
        run = rank_carry(run, E[it] != 0ull, tail[it]);
    }
    run = in_right[span];
#pragma unroll
    for (int it = kSpanIters - 1; it >= 0; --it) {
        right[it] = run;
        run = rank_carry(run, E[it] != 0ull, head[it]);
    }
    SpanSum sum = span_empty();
#pragma unroll
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        uint32_t v = m[it];
        if (rank_open_left(E[it], lt)) v = rank_min(v, left[it]);
        if (rank_open_right(E[it], lt)) v = rank_min(v, right[it]);
        const uint32_t f = c[it] == v ? c[it] : kTokNone;       // (v == kTokNone: a chunk without candidates)
        if (i < n) cand[i] = f;
        sum = span_add_group(sum, __ballot(f != kTokNone));
    }
    if (lane == 0) span_sum[span] = span_pack(sum);
}

// the two scans that link the spans (span.h): the parity of the run of candidates that reaches each span ...
__global__ __launch_bounds__(kScanThreads) void k_enc_scan_parity(const uint32_t *__restrict__ span_sum,
                                                                  uint64_t n_spans, uint32_t *__restrict__ in_par) {
    __shared__ uint32_t sh[kScanThreads];
    span_scan_parity(span_sum, n_spans, in_par, sh);
}

// ... and the exclusive prefix sums of the spans' kept-token counts; total to *total
__global__ __launch_bounds__(kScanThreads) void k_enc_scan_sum(const uint32_t *__restrict__ cnt, uint64_t n_spans,
                                                               unsigned long long *__restrict__ off,
                                                               unsigned long long *__restrict__ total) {
    __shared__ unsigned long long sh[kScanThreads];
    const unsigned long long sum = span_scan_sum(cnt, n_spans, off, sh);
    if (threadIdx.x == 0) *total = sum;
}

// pass, step 2: with the parity of the candidate run before every position, decide.  cand[i] becomes the
// value position i contributes to the next stream (kTokNone: nothing).
__global__ __launch_bounds__(kSpanThreads) void k_enc_match(const uint32_t *__restrict__ tok, uint64_t n,
                                                            uint32_t *__restrict__ cand,
                                                            const uint32_t *__restrict__ in_par,
                                                            uint32_t *__restrict__ span_keep) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    const unsigned long long lt = lanes_below(lane);
    uint32_t carry = in_par[span];             // parity of the run of candidates right before this group
    uint32_t kept = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        const uint32_t c = i < n ? cand[i] : kTokNone;
        uint32_t nx;                           // (only its end flag is used, and only where i + 1 < n)
        const uint32_t t = load_pair(tok, i, n, lane, kDrop, &nx);
        const unsigned long long M = __ballot(c != kTokNone);
        const bool odd = run_below(M, lt, lane, carry) & 1u;
        uint32_t v = kTokNone;
        if (i < n && !odd && t != kDrop) v = c != kTokNone ? (c | (nx & kTokEnd)) : t;   // replaced, or kept as it is
        if (i < n) cand[i] = v;
        kept += wave_count(v != kTokNone);
        carry = run_carry(M, carry);
    }
    if (lane == 0) span_keep[span] = kept;
}

// pass, step 3: compact
__global__ __launch_bounds__(kSpanThreads) void k_enc_scatter(const uint32_t *__restrict__ val, uint64_t n,
                                                              const unsigned long long *__restrict__ span_off,
                                                              uint32_t *__restrict__ out) {
    span_scatter(val, n, span_off, out);
}

// the same with the byte starts: org_out gets org[i] wherever out gets val[i] (a replaced pair contributes at its left
// position: the merged token keeps the left token's start)
__global__ __launch_bounds__(kSpanThreads) void k_enc_scatter_org(const uint32_t *__restrict__ val, uint64_t n,
                                                                  const unsigned long long *__restrict__ span_off,
                                                                  uint32_t *__restrict__ out,
                                                                  const uint32_t *__restrict__ org,
                                                                  uint32_t *__restrict__ org_out) {
    span_scatter_carry<true>(val, n, span_off, out, org, org_out);
}

// ---- the finishing kernels: what leaves the passes becomes what the caller asked for ----------------------------

// chunk starts whose byte is NUL, for a text that lives on the device (the host runs stoi_value on those chunks):
// position i starts a chunk when it is the first byte or the byte before it ends one
__global__ void k_enc_nul_starts(const uint8_t *__restrict__ text, uint64_t n, const uint8_t *__restrict__ endmask,
                                 unsigned long long *__restrict__ list, unsigned long long cap,
                                 unsigned long long *__restrict__ count) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        if (text[i] != 0) continue;
        if (i != 0 && !((endmask[(i - 1) >> 3] >> ((i - 1) & 7)) & 1u)) continue;
        const unsigned long long at = atomicAdd(count, 1ull);
        if (at < cap) list[at] = i;                 // (the host grows the list and asks again when count > cap)
    }
}

// per span: how many of its tokens are the last of their chunk
__global__ __launch_bounds__(kSpanThreads) void k_enc_end_count(const uint32_t *__restrict__ tok, uint64_t n,
                                                                uint32_t *__restrict__ span_ends) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    uint32_t cnt = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        cnt += wave_count(i < n && (tok[i] & kTokEnd));
    }
    if (lane == 0) span_ends[span] = cnt;
}

// ---- document offsets from an end mask that is on the device (mbpe_encoder_encode_endmask) ----------------------
// rank(p) = end bits of the mask below text byte p = chunks that end before p.  A mask BLOCK is 64 words of 32 bits
// (2,048 text bytes): one wave counts a block, k_enc_scan_sum links the blocks, and a position adds the words of its
// block below its own and the low bits of that one.
constexpr uint32_t kMaskBlockWords = 64;

__global__ __launch_bounds__(256) void k_enc_mask_count(const uint32_t *__restrict__ mask, uint64_t n_words,
                                                        uint64_t n_blocks, uint32_t *__restrict__ cnt) {
    const uint64_t block = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
    if (block >= n_blocks) return;                                   // (whole waves leave together)
    const uint32_t lane = lane_id();
    const uint64_t w = block * kMaskBlockWords + lane;
    uint32_t c = w < n_words ? (uint32_t)__popc(mask[w]) : 0u;
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
    if (lane == 0) cnt[block] = c;
}

// a mask with its blocks counted (mask_count_launch): block_off = the end bits before every block, *total = all of them
struct MaskView {                          // (words: 4 * ceil(n_bytes / 32) bytes and 4 more are readable)
    const uint32_t *words; uint64_t n_bytes, n_blocks; const unsigned long long *block_off, *total;
};

// end bits of the mask below text byte p (<= n_bytes)
__device__ __forceinline__ unsigned long long mask_rank(uint64_t p, const MaskView &m) {
    const uint64_t w = p >> 5, block = w / kMaskBlockWords;
    if (block >= m.n_blocks) return *m.total;
    unsigned long long r = m.block_off[block];
    for (uint64_t j = block * kMaskBlockWords; j < w; ++j) r += (unsigned long long)__popc(m.words[j]);
    if (p & 31u) r += (unsigned long long)__popc(m.words[w] & ((1u << (p & 31u)) - 1u));
    return r;
}

// position i = pos[i * stride] (stride in 8-byte words: 1 for a list, 3 for the starts of SingleChunks), r = its rank =
// the index of the chunk that starts there.  ends NULL: out[i] = r.  Else out[i] = the piece's tokens that come from the
// bytes before the position: the end of chunk r - 1 in the finishing kernel's list, less tok_base; 0 before the first
__global__ __launch_bounds__(256) void k_enc_mask_query(const unsigned long long *__restrict__ pos, uint32_t stride,
                                                        uint64_t n_pos, MaskView m,
                                                        const unsigned long long *__restrict__ ends, uint64_t n_ends,
                                                        unsigned long long tok_base, unsigned long long *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pos) return;
    const unsigned long long at = pos[i * stride];
    unsigned long long r = mask_rank(at < m.n_bytes ? at : m.n_bytes, m);
    if (!ends) { out[i] = r; return; }
    if (r > n_ends) r = n_ends;
    out[i] = r ? ends[r - 1] - tok_base : 0ull;
}

enum FinMode {
    kFinFlags = 0,      // uint32_t, bit 31 = last token of its chunk (as the passes leave them)
    kFinU32 = 1,        // uint32_t ids
    kFinU16 = 2,        // uint16_t ids
    kFinNone = 3        // no tokens: only the chunk ends
};

// the final stream -> ids in the caller's format; with ENDS also, in order, the position after every token that ends
// a chunk (span_off = exclusive sums of k_enc_end_count's counts; tok_base = tokens of the pieces before this one)
template <int MODE, bool ENDS>
__global__ __launch_bounds__(kSpanThreads) void k_enc_finish(const uint32_t *__restrict__ tok, uint64_t n,
                                                             void *__restrict__ out,
                                                             const unsigned long long *__restrict__ span_off,
                                                             unsigned long long tok_base,
                                                             unsigned long long *__restrict__ ends,
                                                             unsigned long long ends_cap) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    const unsigned long long lt = lanes_below(lane);
    unsigned long long o = ENDS ? span_off[span] : 0ull;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        const uint32_t t = i < n ? tok[i] : 0u;
        if (i < n) {
            if (MODE == kFinFlags) static_cast<uint32_t *>(out)[i] = t;
            if (MODE == kFinU32) static_cast<uint32_t *>(out)[i] = t & kTokIdMask;
            if (MODE == kFinU16) static_cast<uint16_t *>(out)[i] = (uint16_t)t;
        }
        if (ENDS) {
            const bool end = i < n && (t & kTokEnd);
            const WaveKeep e = wave_keep(end, lt);
            if (end && o + e.rank < ends_cap) ends[o + e.rank] = tok_base + i + 1;
            o += e.count;
        }
    }
}

// ---- token byte offsets (mbpe_encoder_encode_byteoff, mbpe_encoder_encode_endmask_byteoff) ------------------------
// After the passes, from the final stream: a token stands for len[id] text bytes (a function of the id alone for a
// table mbpe_merges_check accepts), a chunk that is one token by rule for its whole chunk.  Per span a 64-bit byte
// count, one scan workgroup, then a ranked write with a wave prefix sum.  The one-token chunks are PATCHES: the index
// of single k in the final stream is the number of tokens before its first byte -- the rank of its start among the
// mask's end bits, looked up in the finishing kernel's list of chunk ends, as for the documents (k_enc_mask_query).
struct LenTab { const uint32_t *len; uint32_t n; };       // ids at or beyond n (they occur as singles only): 0
struct LenPatch {                                         // token idx[k] of the piece covers sc[k].len bytes; ascending
    const unsigned long long *idx;
    const SingleChunk *sc;
    uint64_t n;
};

// the bytes of this lane's token in the group that starts at i0; *k = the first patch at or after i0 (the same in every
// lane), moved past the group
__device__ __forceinline__ unsigned long long group_len(uint32_t t, bool live, uint64_t i0, uint32_t lane,
                                                        const LenTab &tab, const LenPatch &pt, uint64_t *k) {
    const uint32_t id = t & kTokIdMask;
    unsigned long long l = live && id < tab.n ? tab.len[id] : 0ull;
    while (*k < pt.n && pt.idx[*k] < i0 + kWave) {
        if (pt.idx[*k] == i0 + lane) l = pt.sc[*k].len;
        ++*k;
    }
    return l;
}

// per span: the text bytes its tokens stand for
__global__ __launch_bounds__(kSpanThreads) void k_enc_len_sum(const uint32_t *__restrict__ tok, uint64_t n, LenTab tab,
                                                              LenPatch pt, unsigned long long *__restrict__ span_bytes) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    uint64_t k = pt.n ? lower_bound64(pt.idx, pt.n, base) : 0;
    unsigned long long s = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i0 = base + (uint64_t)it * kWave, i = i0 + lane;
        s += group_len(i < n ? tok[i] : 0u, i < n, i0, lane, tab, pt, &k);
    }
    for (int d = kWave / 2; d > 0; d >>= 1) s += __shfl_down(s, d, kWave);
    if (lane == 0) span_bytes[span] = s;
}

// span_bytes -> the bytes before every span
__global__ __launch_bounds__(kScanThreads) void k_enc_scan_sum64(unsigned long long *__restrict__ span_bytes,
                                                                 uint64_t n_spans) {
    __shared__ unsigned long long sh[kScanThreads];
    (void)span_scan_sum64(span_bytes, n_spans, sh);
}

// out[i] = byte_base + the bytes before token i, for i in [0, n); out[n] = byte_base + all of them
__global__ __launch_bounds__(kSpanThreads) void k_enc_len_write(const uint32_t *__restrict__ tok, uint64_t n, LenTab tab,
                                                                LenPatch pt,
                                                                const unsigned long long *__restrict__ span_off,
                                                                unsigned long long byte_base,
                                                                unsigned long long *__restrict__ out) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    uint64_t k = pt.n ? lower_bound64(pt.idx, pt.n, base) : 0;
    unsigned long long o = byte_base + span_off[span];
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i0 = base + (uint64_t)it * kWave, i = i0 + lane;
        const unsigned long long l = group_len(i < n ? tok[i] : 0u, i < n, i0, lane, tab, pt, &k);
        const unsigned long long incl = wave_prefix64(l, lane);
        if (i < n) out[i] = o + incl - l;
        if (i + 1 == n) out[n] = o + incl;
        o += __shfl(incl, kWave - 1, kWave);
    }
}

#define ECHK(expr) MBPE_HIP_CHECK(expr, true)

// device bytes per text byte of a piece, rounded up (mbpe.h, "piece_bytes"): 13.2, and 20 / 1,024 more in rank order
constexpr uint64_t kPieceCost = 14;
constexpr uint64_t kPieceCostDropout = 8;  // more while dropout is on: the two org arrays, one uint32_t per token each
constexpr uint64_t kPieceMaxDropout = 1ull << 32;   // ... and the most bytes of a piece then: org is 32 bits
constexpr uint64_t kPieceCostByteOff = 8;  // more with byte offsets for the host: one uint64_t per token, at most per byte
constexpr uint64_t kNulListMin = 4096;     // entries the list of NUL-led chunk starts begins with
constexpr uint64_t kNulCopyEach = 256;     // up to this many NUL-led chunks are copied back one by one

}  // namespace

struct mbpe_encoder : DevQueue {
    mbpe_encoder() : DevQueue(true) {}
    float last_ms = 0.f;
    uint64_t piece_bytes = 0;                 // option "piece_bytes"; 0 = from the free device memory
    bool rank_order = false;                  // option "rank_order": a pass applies every chunk's lowest merge only
    unsigned long long drop_threshold = 0;    // mbpe_encoder_set_dropout: 0 = off, 2^32 = every instance is dropped
    unsigned long long drop_seed = 0;
    uint32_t n_merges = 0;
    // the lookup table
    DevBuf<unsigned long long> d_keys;
    DevBuf<uint32_t> d_vals;
    EncLut lut = {};
    // work buffers, grown on demand and kept
    DevBuf<uint8_t> d_text, d_mask;
    DevBuf<uint32_t> tok[2], cand, span_a, span_b;
    DevBuf<unsigned long long> span_off;
    DevBuf<RankSum> rank_sum;                 // rank order only: the spans' summaries, and what reaches every span
    DevBuf<uint32_t> rank_in;                 // from the left [0 .. n_spans) and from the right [n_spans .. 2 n_spans)
    DevBuf<uint32_t> org[2];                  // dropout only: the tokens' byte starts in the piece, beside tok[0 / 1]
    DevBuf<unsigned long long> d_res;         // [0] total of a sum scan, [1] NUL-led chunk starts found, [2] end bits of the mask
    DevBuf<SingleChunk> d_singles;
    DevBuf<unsigned long long> d_nul;         // starts of NUL-led chunks of a device text
    DevBuf<unsigned long long> d_ends;        // chunk ends, only when chunks are shorter than two bytes on average
    // mbpe_encoder_encode_batch: the flat tokens of the batch, its document offsets, and a matrix that goes to the host
    DevBuf<void> d_flat, d_ids;
    DevBuf<unsigned long long> d_doc_off;
    DevBuf<uint32_t> d_len;
    DevBuf<unsigned long long> d_doc_pos;     // mbpe_encoder_encode_endmask: the documents' byte offsets
    // mbpe_encoder_encode_batch_aux: labels, positions and segments that go to the host
    DevBuf<void> d_labels;
    DevBuf<uint32_t> d_pos, d_seg;
    // the _windows calls: the rows' prefix sum over the documents; row_doc and row_tok0 that go to the host
    DevBuf<unsigned long long> d_row_start, d_row_tok0;
    DevBuf<uint32_t> d_row_doc;
    // the _fit calls: the plan (host, made from the documents' token offsets) and its copy for k_pack_fit
    PackFitPlan fit_plan;
    DevBuf<uint8_t> d_fit_pieces;
    DevBuf<unsigned long long> d_fit_rows;
    float pack_ms = 0.f;                      // the pack kernel of the latest such call
    // mbpe_encoder_set_fim (nothing of this exists while it is off or its rate 0): the spec; the second flat buffer and
    // offset array the stage writes, the plan beside them; the latest batch call's documents and whether the stage ran
    bool fim_on = false;
    mbpe_fim_spec fim = {};
    DevBuf<void> d_fim_flat;
    DevBuf<unsigned long long> d_fim_off, d_fim_cut;
    DevBuf<uint8_t> d_fim_mode;
    uint64_t fim_docs = 0;
    bool fim_ran = false;
    // mbpe_encoder_set_mlm (nothing of this exists while it is off or its select 0): the spec; the second flat buffer,
    // the target stream and, for whole_word, the spans' word starts
    bool mlm_on = false;
    mbpe_mlm_spec mlm = {};
    DevBuf<void> d_mlm_flat;
    DevBuf<uint32_t> d_mlm_tgt;
    DevBuf<unsigned long long> d_mlm_scr;
    // the _denoise calls (nothing of this exists before the first one): the two flat streams the stage writes; its index
    // arrays in one buffer (dn_index); the rows' documents; the decoder side's matrix and lengths that go to the host
    DevBuf<void> d_dn_in, d_dn_tg, d_dn_dec_ids;
    DevBuf<unsigned long long> d_dn_idx;
    DevBuf<uint32_t> d_dn_row_doc, d_dn_dec_len;
    // token byte offsets: len[id] (host; empty with len_error set for a table mbpe_merges_check refuses), on the
    // device from the first such call on; the spans' byte counts, the singles' token indices, offsets bound for the host
    std::vector<uint32_t> len;
    std::string len_error;
    DevBuf<uint32_t> d_tok_len;
    DevBuf<unsigned long long> span_bytes, d_single_tok, d_boff;
    // host scratch
    std::vector<uint8_t> mask, bytes;
    std::vector<SingleChunk> singles, piece_singles;
    std::vector<unsigned long long> list;
    std::vector<uint64_t> pass_tokens;        // latest call: tokens that entered pass k, summed over the pieces
    std::vector<uint64_t> chunk_tok, doc_tok; // mbpe_encoder_encode_batch: token offsets of the chunks, of the documents
    // option "dedup" (nothing of this exists while it is 0): the deduper; the unique chunks' tokens in the caller's
    // format and their ends, the one-token chunks behind them; the expansion's span offsets and chunk ends; the
    // positions whose chunk is asked for and those chunks; the mask's block counts; host output on its way
    bool dedup = false;
    int64_t dedup_max_chunk = -1;             // option "dedup_max_chunk_bytes"; -1: the deduper's default
    mbpe_dedup *dd = nullptr;
    DevBuf<uint8_t> d_utab, d_stage;
    DevBuf<unsigned long long> d_uends, d_exp_off, d_exp_ends, d_q_pos, d_q_chunk, d_mblk_off;
    DevBuf<uint32_t> d_sg_tok, d_mblk_cnt;
    std::vector<uint32_t> sg_tok;
    std::vector<unsigned long long> q_pos;
    std::vector<SingleChunk> dd_singles;
    bool dd_ran = false;                      // the latest call went through the deduper (mbpe_encoder_dedup_stats)
    uint64_t dd_chunks = 0, dd_unique = 0, dd_unique_bytes = 0, dd_unique_tokens = 0;
    float dd_expand_ms = 0.f;
    // the count calls (nothing of this exists before the first one): the kept table, cnt_ids bins and `other` behind
    // them; the call's scratch table, with the call's token total behind `other` ("dedup" route); the runs' weights
    uint64_t count_ids = 0;                   // option "count_ids"
    uint64_t cnt_ids = 0;                     // bins of the table as it is allocated; 0: not yet
    uint64_t cnt_tokens = 0;                  // the weighted token total the table has reached
    bool cnt_used = false;                    // something has been counted and not reset
    DevBuf<unsigned long long> d_cnt, d_cnt_call, d_cnt_w;
};

namespace {

uint64_t enc_held(const mbpe_encoder *e) {
    return e->d_text.bytes() + e->d_mask.bytes() + e->tok[0].bytes() + e->tok[1].bytes() + e->cand.bytes() +
           e->span_a.bytes() + e->span_b.bytes() + e->span_off.bytes() + e->rank_sum.bytes() + e->rank_in.bytes() +
           e->org[0].bytes() + e->org[1].bytes();
}

struct Piece { uint64_t c0, c1; };            // chunks [c0, c1)

// chunk-end bits of the chunks [c0, c1), relative to the first one's start
void build_mask(mbpe_encoder *e, const uint64_t *chunk_off, Piece p) {
    const uint64_t base = chunk_off[p.c0], pn = chunk_off[p.c1] - base;
    e->mask.assign((pn + 7) / 8 + 8, 0);
    for (uint64_t c = p.c0; c < p.c1; ++c) {
        const uint64_t s = chunk_off[c], t = chunk_off[c + 1];
        if (t == s) continue;
        e->mask[(t - 1 - base) >> 3] |= (uint8_t)(1u << ((t - 1 - base) & 7));
    }
}

int add_single(mbpe_encoder *e, uint64_t start, uint64_t len, long long id, uint32_t token_bits) {
    if ((uint32_t)(int)id >= kDrop) return fail(MBPE_ERR_ARG, "token id of a NUL-led chunk does not fit 31 bits");
    if (token_bits == 16 && (uint32_t)(int)id >= 65536u)
        return fail(MBPE_ERR_VOCAB, "token id " + std::to_string(id) + " of a NUL-led chunk does not fit 16 bits");
    e->singles.push_back({start, len, (uint32_t)(int)id, 0});
    return MBPE_OK;
}

// the NUL-led chunks of one piece of a device text -> e->singles; leaves the piece's mask on the device
int device_singles(mbpe_encoder *e, const uint8_t *d_text, const uint64_t *chunk_off, Piece p, uint32_t token_bits) {
    const uint64_t base = chunk_off[p.c0], pn = chunk_off[p.c1] - base;
    if (pn == 0) return MBPE_OK;
    build_mask(e, chunk_off, p);
    int rc = e->d_mask.reserve(e->mask.size(), e->mem);
    if (rc == MBPE_OK && !e->d_nul) rc = e->d_nul.reserve(kNulListMin * 8, e->mem);
    if (rc != MBPE_OK) return rc;
    ECHK(hipMemcpyAsync(e->d_mask, e->mask.data(), e->mask.size(), hipMemcpyHostToDevice, e->stream));
    unsigned long long found = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        ECHK(hipMemsetAsync(e->d_res + 1, 0, 8, e->stream));
        const int blocks = (int)std::min<uint64_t>((pn + 255) / 256, 8192);
        hipLaunchKernelGGL(k_enc_nul_starts, dim3(blocks), dim3(256), 0, e->stream, d_text + base, pn, e->d_mask,
                           e->d_nul, e->d_nul.bytes() / 8, e->d_res + 1);
        ECHK(hipMemcpyAsync(&found, e->d_res + 1, 8, hipMemcpyDeviceToHost, e->stream));
        ECHK(hipStreamSynchronize(e->stream));
        ECHK(hipGetLastError());
        if (found <= e->d_nul.bytes() / 8) break;
        rc = e->d_nul.reserve(found * 8, e->mem);
        if (rc != MBPE_OK) return rc;
    }
    if (found == 0) return MBPE_OK;
    e->list.resize(found);
    ECHK(hipMemcpyAsync(e->list.data(), e->d_nul, found * 8, hipMemcpyDeviceToHost, e->stream));
    ECHK(hipStreamSynchronize(e->stream));
    std::sort(e->list.begin(), e->list.end());
    const bool whole = found > kNulCopyEach;      // many: one copy of the piece instead of one per chunk
    if (whole) {
        e->bytes.resize(pn);
        ECHK(hipMemcpyAsync(e->bytes.data(), d_text + base, pn, hipMemcpyDeviceToHost, e->stream));
        ECHK(hipStreamSynchronize(e->stream));
    }
    for (unsigned long long pos : e->list) {
        // the chunk that holds byte base + pos; it starts there (k_enc_nul_starts lists chunk starts only)
        const uint64_t c = (uint64_t)(std::upper_bound(chunk_off + p.c0, chunk_off + p.c1 + 1, base + pos) - chunk_off) - 1;
        const uint64_t s = chunk_off[c], len = chunk_off[c + 1] - s;
        if (s != base + pos || len == 0) return fail(MBPE_ERR_HIP, "mbpe_encoder_encode: chunk start list is inconsistent");
        const uint8_t *b;
        if (whole) {
            b = e->bytes.data() + pos;
        } else {
            e->bytes.resize(len);
            ECHK(hipMemcpyAsync(e->bytes.data(), d_text + s, len, hipMemcpyDeviceToHost, e->stream));
            ECHK(hipStreamSynchronize(e->stream));
            b = e->bytes.data();
        }
        long long id;
        if (stoi_value(b + 1, len - 1, &id)) {
            rc = add_single(e, s, len, id, token_bits);
            if (rc != MBPE_OK) return rc;
        }
    }
    return MBPE_OK;
}

// one encode request, as the C-ABI states it: text and chunks in braces, the other fields by name (left out: 0 / NULL)
struct EncCall {
    const uint8_t *text;
    uint64_t n_bytes;
    int text_on_device;
    const uint64_t *chunk_off;
    uint64_t n_chunks;
    void *tokens_out;            // NULL: count only (and chunk offsets, when asked for)
    uint64_t cap;
    uint32_t token_bits;
    int out_on_device;
    uint64_t *chunk_tok_off_out, *n_out;
    uint32_t *n_passes_out;
    // the only piece's mask where it is on the device already (the caller's, or e->d_mask: gather_singles); NULL: every
    // piece's is built from chunk_off and uploaded.  endmask (mbpe_encoder_encode_endmask): the chunks are that mask's,
    // not chunk_off's; the documents' token offsets are left in e->d_doc_off (and copied to doc_tok_off_out when given)
    const uint8_t *mask_dev;
    bool endmask;
    const mbpe_single *singles;
    uint64_t n_singles;
    const uint64_t *doc_off;
    uint64_t n_docs;
    uint64_t *doc_tok_off_out;
    // the _byteoff calls: cap + 1 byte offsets, where tokens_out lives (NULL: none are computed)
    uint64_t *tok_byte_off_out;
    // the count calls: every piece's final stream is counted into e->d_cnt_call (tokens_out is NULL)
    bool count;
};

// where a call's ids go and in what width, and where it reports how many they are
void enc_out(EncCall *a, void *tokens_out, uint64_t cap, uint32_t token_bits, int out_on_device, uint64_t *n_out,
             uint32_t *n_passes_out) {
    a->tokens_out = tokens_out;
    a->cap = cap;
    a->token_bits = token_bits;
    a->out_on_device = out_on_device;
    a->n_out = n_out;
    a->n_passes_out = n_passes_out;
}

// what the _denoise calls add to a batch call: the rule, the decoder side's spec, and where both matrices go
struct EncDenoise {
    const mbpe_denoise_spec *spec;
    const mbpe_pack_spec *dec_spec;
    const mbpe_denoise_batch *out;
};

// what the batch calls add: the documents as chunk ranges (the endmask call has them in EncCall) and the pack step
struct EncPack {
    const uint64_t *doc_chunk_off;
    uint64_t n_docs;
    const mbpe_pack_spec *spec;
    void *ids_out;
    uint64_t cap_rows;
    int out_on_device;
    uint32_t *len_out;
    uint64_t *n_rows_out, *n_tokens_out;
    const mbpe_pack_aux *aux;
    uint64_t *doc_tok_off_out;
    const mbpe_pack_window *win;    // the _windows calls; NULL: the spec's own layout
    const struct mbpe_pack_fit *fit;   // the _fit calls (win NULL); NULL: the spec's own layout
    const struct EncDenoise *dn;    // the _denoise calls (aux, win and fit NULL): spec, ids_out and len_out are the encoder side's
    uint32_t token_bits() const { return spec->out_bits == 16 ? 16 : 32; }
};

// a piece on its way: pn bytes at d_text with their end mask at d_mask, then n tokens in tok[cur] after `passes` passes;
// too_small: the caller's cap does not hold them and nothing was written
struct PieceRun {
    uint64_t pn = 0, n = 0;
    const uint8_t *d_text = nullptr, *d_mask = nullptr;
    int cur = 0;
    uint32_t passes = 0;
    bool too_small = false;
};

// the count and the passes of a call that has run, and what a cap that did not hold the tokens gets
int enc_report(const EncCall &a, const PieceRun &sum, bool too_small) {
    *a.n_out = sum.n;
    if (a.n_passes_out) *a.n_passes_out = sum.passes;
    return too_small ? fail(MBPE_ERR_ARG, "tokens_out too small") : MBPE_OK;
}

// buffers for the piece [base, base + pn) and what the host has of it: text, mask, singles, document offsets
int piece_upload(mbpe_encoder *e, const EncCall &a, Piece p, PieceRun *r) {
    const uint64_t base = a.chunk_off[p.c0], pn = r->pn;
    const uint64_t n_spans0 = span_count(pn);
    int rc = MBPE_OK;
    if (!a.text_on_device) rc = e->d_text.reserve(pn, e->mem);
    if (rc == MBPE_OK && !a.mask_dev) {
        build_mask(e, a.chunk_off, p);
        rc = e->d_mask.reserve(e->mask.size(), e->mem);
    }
    if (rc == MBPE_OK) rc = e->tok[0].reserve(pn * 4, e->mem);
    if (rc == MBPE_OK) rc = e->tok[1].reserve(pn * 4, e->mem);
    if (rc == MBPE_OK) rc = e->cand.reserve(pn * 4, e->mem);
    if (rc == MBPE_OK) rc = e->span_a.reserve(n_spans0 * 4, e->mem);
    if (rc == MBPE_OK) rc = e->span_b.reserve(n_spans0 * 4, e->mem);
    if (rc == MBPE_OK) rc = e->span_off.reserve(n_spans0 * 8, e->mem);
    if (rc == MBPE_OK && e->rank_order) {
        rc = e->rank_sum.reserve(n_spans0 * sizeof(RankSum), e->mem);
        if (rc == MBPE_OK) rc = e->rank_in.reserve(n_spans0 * 8, e->mem);
    }
    if (rc == MBPE_OK && e->drop_threshold) {
        rc = e->org[0].reserve(pn * 4, e->mem);
        if (rc == MBPE_OK) rc = e->org[1].reserve(pn * 4, e->mem);
    }
    if (rc != MBPE_OK) return rc;
    // the piece's NUL-led chunks (e->singles is sorted by start), relative to the piece
    e->piece_singles.clear();
    {
        auto lo = std::lower_bound(e->singles.begin(), e->singles.end(), base,
                                   [](const SingleChunk &s, uint64_t v) { return s.start < v; });
        for (; lo != e->singles.end() && lo->start < base + pn; ++lo)
            e->piece_singles.push_back({lo->start - base, lo->len, lo->id, 0});
    }
    if (!e->piece_singles.empty()) {
        rc = e->d_singles.reserve(e->piece_singles.size() * sizeof(SingleChunk), e->mem);
        if (rc == MBPE_OK && a.tok_byte_off_out) rc = e->d_single_tok.reserve(e->piece_singles.size() * 8, e->mem);
        if (rc != MBPE_OK) return rc;
    }
    if (a.tok_byte_off_out) {
        rc = e->span_bytes.reserve(n_spans0 * 8, e->mem);
        if (rc != MBPE_OK) return rc;
    }
    r->d_text = a.text + base;
    if (!a.text_on_device) {
        ECHK(hipMemcpyAsync(e->d_text, a.text + base, pn, hipMemcpyHostToDevice, e->stream));
        r->d_text = e->d_text;
    }
    r->d_mask = a.mask_dev ? a.mask_dev : e->d_mask.get();
    if (!a.mask_dev)
        ECHK(hipMemcpyAsync(e->d_mask, e->mask.data(), e->mask.size(), hipMemcpyHostToDevice, e->stream));
    if (!e->piece_singles.empty())
        ECHK(hipMemcpyAsync(e->d_singles, e->piece_singles.data(), e->piece_singles.size() * sizeof(SingleChunk),
                            hipMemcpyHostToDevice, e->stream));

    if (a.doc_off) {
        rc = e->d_doc_pos.reserve((a.n_docs + 1) * 8, e->mem);
        if (rc == MBPE_OK) rc = e->d_doc_off.reserve((a.n_docs + 1) * 8, e->mem);
        if (rc != MBPE_OK) return rc;
        ECHK(hipMemcpyAsync(e->d_doc_pos, a.doc_off, (a.n_docs + 1) * 8, hipMemcpyHostToDevice, e->stream));
    }
    return MBPE_OK;
}

// ev0, bytes -> tokens, then passes until one changes nothing.  piece_base = the piece's first byte in the call's text
int piece_passes(mbpe_encoder *e, uint64_t piece_base, PieceRun *r) {
    const uint64_t pn = r->pn;
    const bool drop = e->drop_threshold != 0;
    ECHK(hipEventRecord(e->ev0, e->stream));
    const int wblocks = (int)std::min<uint64_t>((pn + 255) / 256, 8192);
    if (drop)
        hipLaunchKernelGGL(k_enc_widen<true>, dim3(wblocks), dim3(256), 0, e->stream, r->d_text, pn,
                           r->d_mask, e->tok[0], e->org[0]);
    else
        hipLaunchKernelGGL(k_enc_widen<false>, dim3(wblocks), dim3(256), 0, e->stream, r->d_text, pn,
                           r->d_mask, e->tok[0], nullptr);
    if (!e->piece_singles.empty())
        hipLaunchKernelGGL(k_enc_single, dim3((uint32_t)e->piece_singles.size()), dim3(64), 0, e->stream, e->d_singles,
                           (uint32_t)e->piece_singles.size(), e->tok[0]);
    uint64_t n = pn;
    int cur = 0;
    uint32_t passes = 0;
    for (;;) {
        const uint64_t n_spans = span_count(n);
        const dim3 grid(span_grid(n)), block(kSpanThreads);
        if (drop)
            hipLaunchKernelGGL(k_enc_cand<true>, grid, block, 0, e->stream, e->tok[cur], n, e->lut, e->cand, e->span_a,
                               EncDrop{e->org[cur], piece_base, e->drop_seed, e->drop_threshold});
        else
            hipLaunchKernelGGL(k_enc_cand<false>, grid, block, 0, e->stream, e->tok[cur], n, e->lut, e->cand, e->span_a,
                               EncDrop{});
        if (e->rank_order) {
            uint32_t *in_left = e->rank_in, *in_right = e->rank_in + n_spans;
            hipLaunchKernelGGL(k_enc_rank_sum, grid, block, 0, e->stream, e->tok[cur], n, e->cand, e->rank_sum);
            hipLaunchKernelGGL(k_enc_scan_min, dim3(1), dim3(kScanThreads), 0, e->stream, e->rank_sum, n_spans, in_left,
                               in_right);
            hipLaunchKernelGGL(k_enc_rank_filter, grid, block, 0, e->stream, e->tok[cur], n, e->cand, in_left, in_right,
                               e->span_a);
        }
        hipLaunchKernelGGL(k_enc_scan_parity, dim3(1), dim3(kScanThreads), 0, e->stream, e->span_a, n_spans, e->span_b);
        hipLaunchKernelGGL(k_enc_match, grid, block, 0, e->stream, e->tok[cur], n, e->cand, e->span_b, e->span_a);
        hipLaunchKernelGGL(k_enc_scan_sum, dim3(1), dim3(kScanThreads), 0, e->stream, e->span_a, n_spans, e->span_off,
                           e->d_res);
        if (drop)
            hipLaunchKernelGGL(k_enc_scatter_org, grid, block, 0, e->stream, e->cand, n, e->span_off, e->tok[1 - cur],
                               e->org[cur], e->org[1 - cur]);
        else
            hipLaunchKernelGGL(k_enc_scatter, grid, block, 0, e->stream, e->cand, n, e->span_off, e->tok[1 - cur]);
        unsigned long long total = 0;
        ECHK(hipMemcpyAsync(&total, e->d_res, 8, hipMemcpyDeviceToHost, e->stream));
        ECHK(hipStreamSynchronize(e->stream));
        ECHK(hipGetLastError());
        if (e->pass_tokens.size() <= passes) e->pass_tokens.resize(passes + 1, 0);
        e->pass_tokens[passes] += n;
        ++passes;
        if (total == n) break;                 // the pass changed nothing: tok[cur] is the result (so is tok[1 - cur])
        n = total;
        cur = 1 - cur;
        if (n == 0) break;
    }
    r->n = n;
    r->cur = cur;
    r->passes = passes;
    return MBPE_OK;
}

// ---- the launch sequences that the plain pieces and the "dedup" route share ---------------------------------------
// the chunk ends of tok[0 .. n): the spans' counts in span_a, the ends before every span in span_off, all in d_res[0]
void end_count_launch(mbpe_encoder *e, const uint32_t *tok, uint64_t n) {
    hipLaunchKernelGGL(k_enc_end_count, dim3(span_grid(n)), dim3(kSpanThreads), 0, e->stream, tok, n, e->span_a);
    hipLaunchKernelGGL(k_enc_scan_sum, dim3(1), dim3(kScanThreads), 0, e->stream, e->span_a, span_count(n), e->span_off,
                       e->d_res);
}

// the finishing kernel in the form asked for (no tokens and no ends: nothing to launch).  with_ends: end_count_launch
// has run on the same tokens; ends[0 .. ends_cap) gets tok_base + the position after every token that ends a chunk
void finish_launch(mbpe_encoder *e, int mode, bool with_ends, const uint32_t *tok, uint64_t n, void *out,
                   unsigned long long tok_base, unsigned long long *ends, uint64_t ends_cap) {
    const dim3 grid(span_grid(n));
    auto finish = [&](auto m) {
        if (with_ends)
            hipLaunchKernelGGL((k_enc_finish<m(), true>), grid, dim3(kSpanThreads), 0, e->stream, tok, n, out, e->span_off,
                               tok_base, ends, ends_cap);
        else if constexpr (m() != kFinNone)
            hipLaunchKernelGGL((k_enc_finish<m(), false>), grid, dim3(kSpanThreads), 0, e->stream, tok, n, out, e->span_off,
                               tok_base, ends, ends_cap);
    };
    switch (mode) {
        case kFinFlags: finish(std::integral_constant<int, kFinFlags>()); break;
        case kFinU32: finish(std::integral_constant<int, kFinU32>()); break;
        case kFinU16: finish(std::integral_constant<int, kFinU16>()); break;
        default: finish(std::integral_constant<int, kFinNone>()); break;
    }
}

// the blocks of the mask of n_bytes text bytes, counted into cnt and linked into off (an entry per block each), for the
// queries of mask_query_launch; the total goes to d_res[2]: d_res[0] may hold a count of chunk ends that is read later
MaskView mask_count_launch(mbpe_encoder *e, const uint8_t *mask, uint64_t n_bytes, uint32_t *cnt,
                           unsigned long long *off) {
    const uint64_t n_words = (n_bytes + 31) / 32, n_blocks = (n_words + kMaskBlockWords - 1) / kMaskBlockWords;
    const uint32_t *words = reinterpret_cast<const uint32_t *>(mask);
    hipLaunchKernelGGL(k_enc_mask_count, dim3((uint32_t)((n_blocks * kWave + 255) / 256)), dim3(256), 0, e->stream, words,
                       n_words, n_blocks, cnt);
    hipLaunchKernelGGL(k_enc_scan_sum, dim3(1), dim3(kScanThreads), 0, e->stream, cnt, n_blocks, off, e->d_res + 2);
    return {words, n_bytes, n_blocks, off, e->d_res + 2};
}

void mask_query_launch(mbpe_encoder *e, const MaskView &m, const unsigned long long *pos, uint32_t stride, uint64_t n_pos,
                       const unsigned long long *ends, uint64_t n_ends, uint64_t tok_base, unsigned long long *out) {
    hipLaunchKernelGGL(k_enc_mask_query, dim3((uint32_t)((n_pos + 255) / 256)), dim3(256), 0, e->stream, pos, stride, n_pos,
                       m, ends, n_ends, tok_base, out);
}

// chunk_tok_off_out[c + 1] for the chunks [p.c0, p.c1): a chunk that is not empty takes the next of ends[0 .. n_ends),
// an empty one repeats its predecessor's offset (`before`: the offset the first chunk starts at)
void fill_chunk_tok_off(const EncCall &a, Piece p, uint64_t before, const unsigned long long *ends, uint64_t n_ends) {
    uint64_t k = 0, last = before;
    for (uint64_t c = p.c0; c < p.c1; ++c) {
        if (a.chunk_off[c + 1] > a.chunk_off[c] && k < n_ends) last = ends[k++];
        a.chunk_tok_off_out[c + 1] = last;
    }
}

// the finishing stage: chunk ends (their list in tok[1 - cur] when it fits), ids in the caller's format (into cand when
// they go to the host), document and byte offsets; ev1 and the kernel time; then what goes to the host
int piece_finish(mbpe_encoder *e, const EncCall &a, Piece p, uint64_t done, PieceRun *r) {
    const uint64_t n = r->n, pn = r->pn, tok_bytes = a.token_bits / 8;
    const uint32_t *tok = e->tok[r->cur];
    DevBuf<uint32_t> &idle = e->tok[1 - r->cur];          // the other token array: room for the list of chunk ends
    r->too_small = a.tokens_out && a.cap < done + n;
    const bool with_docs = a.doc_off && !r->too_small;
    const bool with_boff = a.tok_byte_off_out && a.tokens_out && !r->too_small && n;
    // (the one-token chunks of the piece: each needs its index in the final stream, which the chunk ends give)
    const uint64_t n_patch = with_boff ? e->piece_singles.size() : 0;
    const bool with_ends = (a.chunk_tok_off_out || a.doc_off || n_patch) && !r->too_small;
    const bool with_tokens = a.tokens_out && !r->too_small;
    int rc = MBPE_OK;
    if (with_boff && !a.out_on_device && (rc = e->d_boff.reserve((n + 1) * 8, e->mem)) != MBPE_OK) return rc;
    uint64_t n_ends = 0;
    unsigned long long *d_ends = nullptr;
    if (n && with_ends) {
        end_count_launch(e, tok, n);
        if (a.endmask) {                                  // the chunks are the mask's: their number comes from the device
            unsigned long long found = 0;
            ECHK(hipMemcpyAsync(&found, e->d_res, 8, hipMemcpyDeviceToHost, e->stream));
            ECHK(hipStreamSynchronize(e->stream));
            n_ends = found;
        } else {
            for (uint64_t c = p.c0; c < p.c1; ++c) n_ends += a.chunk_off[c + 1] > a.chunk_off[c];
        }
        d_ends = reinterpret_cast<unsigned long long *>(idle.get());
        if (n_ends * 8 > idle.bytes()) {                  // (chunks shorter than two bytes on average)
            if ((rc = e->d_ends.reserve(n_ends * 8, e->mem)) != MBPE_OK) return rc;
            d_ends = e->d_ends;
        }
    }
    if (n && (with_ends || with_tokens)) {
        void *out = !with_tokens ? nullptr
                    : a.out_on_device ? static_cast<uint8_t *>(a.tokens_out) + done * tok_bytes
                                      : reinterpret_cast<uint8_t *>(e->cand.get());
        const int mode = !with_tokens ? kFinNone : a.token_bits == 16 ? kFinU16 : a.out_on_device ? kFinFlags : kFinU32;
        finish_launch(e, mode, with_ends, tok, n, out, done, d_ends, n_ends);
    }
    if (n && (with_docs || n_patch)) {
        // the rank of every document offset and of every single's start in the mask, then the look-up in the chunk
        // ends (span_a and span_off are free again: the finishing kernel is ahead on the stream)
        const MaskView m = mask_count_launch(e, r->d_mask, pn, e->span_a, e->span_off);
        if (with_docs)
            mask_query_launch(e, m, e->d_doc_pos, 1, a.n_docs + 1, d_ends, n_ends, done, e->d_doc_off);
        if (n_patch)                                      // (a SingleChunk begins with its start)
            mask_query_launch(e, m, &e->d_singles.get()->start, sizeof(SingleChunk) / 8, n_patch, d_ends, n_ends, done,
                              e->d_single_tok);
    }
    if (with_boff) {
        const LenTab tab = {e->d_tok_len, (uint32_t)e->len.size()};
        const LenPatch pt = {e->d_single_tok, e->d_singles, n_patch};
        unsigned long long *boff = a.out_on_device ? reinterpret_cast<unsigned long long *>(a.tok_byte_off_out) + done
                                                   : e->d_boff.get();
        const dim3 grid(span_grid(n));
        hipLaunchKernelGGL(k_enc_len_sum, grid, dim3(kSpanThreads), 0, e->stream, tok, n, tab, pt, e->span_bytes);
        hipLaunchKernelGGL(k_enc_scan_sum64, dim3(1), dim3(kScanThreads), 0, e->stream, e->span_bytes, span_count(n));
        hipLaunchKernelGGL(k_enc_len_write, grid, dim3(kSpanThreads), 0, e->stream, tok, n, tab, pt, e->span_bytes,
                           a.chunk_off[p.c0], boff);
    }
    if (a.count && n)
        hist_tokens_launch(e->stream, tok, n, 32, e->d_cnt_call, e->cnt_ids, e->d_cnt_call + e->cnt_ids);
    ECHK(hipEventRecord(e->ev1, e->stream));
    unsigned long long ends_found = 0;
    if (with_ends && !a.endmask && n) ECHK(hipMemcpyAsync(&ends_found, e->d_res, 8, hipMemcpyDeviceToHost, e->stream));
    float ms = 0.f;
    if ((rc = e->wait(&ms)) != MBPE_OK) return rc;
    e->last_ms += ms;
    if (with_tokens && !a.out_on_device && n) {
        ECHK(hipMemcpyAsync(static_cast<uint8_t *>(a.tokens_out) + done * tok_bytes, e->cand, n * tok_bytes,
                            hipMemcpyDeviceToHost, e->stream));
        ECHK(hipStreamSynchronize(e->stream));
    }
    if (with_boff && !a.out_on_device) {
        ECHK(hipMemcpyAsync(a.tok_byte_off_out + done, e->d_boff, (n + 1) * 8, hipMemcpyDeviceToHost, e->stream));
        ECHK(hipStreamSynchronize(e->stream));
    }
    if (with_docs) {
        if (a.doc_tok_off_out) {
            ECHK(hipMemcpyAsync(a.doc_tok_off_out, e->d_doc_off, (a.n_docs + 1) * 8, hipMemcpyDeviceToHost, e->stream));
            ECHK(hipStreamSynchronize(e->stream));
        }
    } else if (with_ends && !a.endmask) {
        if (ends_found != n_ends) return fail(MBPE_ERR_HIP, "mbpe_encoder_encode: chunk ends and chunks differ in number");
        if (!a.chunk_tok_off_out) return MBPE_OK;          // (the ends served the byte offsets of one-token chunks only)
        e->list.resize(n_ends);
        if (n_ends) {
            ECHK(hipMemcpyAsync(e->list.data(), d_ends, n_ends * 8, hipMemcpyDeviceToHost, e->stream));
            ECHK(hipStreamSynchronize(e->stream));
        }
        fill_chunk_tok_off(a, p, done, e->list.data(), n_ends);
    }
    return MBPE_OK;
}

// one piece through the passes and the finishing stage.  done = tokens of the pieces before it.
int run_piece(mbpe_encoder *e, const EncCall &a, Piece p, uint64_t done, PieceRun *r) {
    *r = PieceRun{};
    r->pn = a.chunk_off[p.c1] - a.chunk_off[p.c0];
    if (r->pn == 0) {
        if (a.chunk_tok_off_out) fill_chunk_tok_off(a, p, done, nullptr, 0);
        return MBPE_OK;
    }
    int rc = piece_upload(e, a, p, r);
    if (rc == MBPE_OK) rc = piece_passes(e, a.chunk_off[p.c0], r);
    if (rc == MBPE_OK) rc = piece_finish(e, a, p, done, r);
    return rc;
}

// the pieces in order -> sum: n = tokens of all, passes = the deepest.  After a piece that does not fit, the rest
// is counted only.
int run_pieces(mbpe_encoder *e, EncCall a, const std::vector<Piece> &pieces, PieceRun *sum) {
    *sum = PieceRun{};
    for (const Piece &p : pieces) {
        PieceRun r;
        const int rc = run_piece(e, a, p, sum->n, &r);
        if (rc != MBPE_OK) return rc;
        sum->n += r.n;
        sum->passes = std::max(sum->passes, r.passes);
        if (r.too_small) { sum->too_small = true; a.tokens_out = nullptr; a.chunk_tok_off_out = nullptr; a.tok_byte_off_out = nullptr; }
    }
    return MBPE_OK;
}

// the bytes one piece may hold: the option, else what the buffers hold already, else from the free device memory
// (boff_host: byte offsets that go to the host are staged on the device, 8 bytes per token)
int piece_limit(mbpe_encoder *e, uint64_t n_bytes, bool boff_host, uint64_t *limit) {
    const bool drop = e->drop_threshold != 0;
    *limit = e->piece_bytes;
    if (*limit == 0) {
        // what the buffers hold already needs no question (with dropout: the org arrays are among them)
        *limit = drop ? std::min(e->cand.bytes(), e->org[1].bytes()) / 4 : e->cand.bytes() / 4;
        if (n_bytes > *limit) {
            size_t free_b = 0, total_b = 0;
            ECHK(hipMemGetInfo(&free_b, &total_b));
            const uint64_t avail = (uint64_t)free_b + enc_held(e) + (boff_host ? e->d_boff.bytes() : 0);
            const uint64_t cost = kPieceCost + (drop ? kPieceCostDropout : 0) + (boff_host ? kPieceCostByteOff : 0);
            *limit = std::max<uint64_t>((avail - avail / 16) / cost, *limit);
        }
    }
    if (drop) *limit = std::min(*limit, kPieceMaxDropout);
    return MBPE_OK;
}

// what a _byteoff call settles before its pieces run: len[] on the device from the first such call on, and the [0] = 0
// of an empty text (a query computes no offsets: the entry points have dropped the pointer)
int boff_begin(mbpe_encoder *e, const EncCall &a) {
    if (!a.tok_byte_off_out) return MBPE_OK;
    ECHK(hipSetDevice(e->device));
    if (!e->d_tok_len) {
        const int rc = e->d_tok_len.reserve(e->len.size() * 4, e->mem);
        if (rc != MBPE_OK) return rc;
        ECHK(hipMemcpyAsync(e->d_tok_len, e->len.data(), e->len.size() * 4, hipMemcpyHostToDevice, e->stream));
        ECHK(hipStreamSynchronize(e->stream));
    }
    if (a.n_bytes == 0) {
        if (!a.out_on_device) { a.tok_byte_off_out[0] = 0; return MBPE_OK; }
        ECHK(hipMemsetAsync(a.tok_byte_off_out, 0, 8, e->stream));
        ECHK(hipStreamSynchronize(e->stream));
    }
    return MBPE_OK;
}

// dropout is defined on the rank order alone: an encode call of an encoder with a threshold above 0 and the greedy
// order is refused before the device is touched (there is no silent switch of the order)
int drop_check(const mbpe_encoder *e, const std::string &who) {
    if (e->drop_threshold && !e->rank_order)
        return fail(MBPE_ERR_ARG, who + ": dropout needs the option \"rank_order\" (mbpe_encoder_set_dropout)");
    return MBPE_OK;
}

// the checks of a _byteoff call that need no device; drops the pointer of a query
int boff_check(const mbpe_encoder *e, const std::string &who, EncCall *a) {
    if (!a->tokens_out) a->tok_byte_off_out = nullptr;
    if (!a->tok_byte_off_out) return MBPE_OK;
    if (!e->len_error.empty())
        return fail(MBPE_ERR_ARG, who + ": token byte offsets need a table mbpe_merges_check accepts (" + e->len_error + ")");
    if (a->out_on_device && ((uintptr_t)a->tok_byte_off_out & 7))
        return fail(MBPE_ERR_ARG, who + ": tok_byte_off_out must be 8-byte aligned");
    return MBPE_OK;
}

// ---- option "dedup": dedup -> the passes over the unique chunks -> expansion (expand.h) ---------------------------
// Without dropout a chunk's tokens depend on its bytes alone, in both orders: the deduper (dedup.h, with "map") names
// the unique chunk of every chunk, the passes run over the unique text as one piece without any single -- a NUL-led
// chunk's bytes there are ordinary bytes that nothing points at --, the finishing kernel writes the table in the
// caller's format with the runs' ends, the chunks that are one token by rule become runs of their own, and the
// expansion writes every chunk's run to its place.

// what dropout and byte offsets get on this route, before the device is touched
int dedup_check(const mbpe_encoder *e, const std::string &who, const uint64_t *tok_byte_off_out) {
    if (!e->dedup) return MBPE_OK;
    if (e->drop_threshold)
        return fail(MBPE_ERR_ARG, who + ": dropout and the option \"dedup\" exclude each other (a dropped instance depends "
                                        "on its position, so equal chunks do not share their tokens)");
    if (tok_byte_off_out)
        return fail(MBPE_ERR_ARG, who + ": token byte offsets are not computed while the option \"dedup\" is on");
    return MBPE_OK;
}

// a call that met nothing to dedup (an empty text) still went this way
void dedup_nothing(mbpe_encoder *e) {
    e->dd_ran = true;
    e->dd_chunks = e->dd_unique = e->dd_unique_bytes = e->dd_unique_tokens = 0;
    e->dd_expand_ms = 0.f;
}

// checks of more than one entry point: chunk_off (absent: one chunk, in `one`, which lives as long as the request) ...
int chunk_off_check(EncCall *a, uint64_t one[2]) {
    if (!a->chunk_off) { one[0] = 0; one[1] = a->n_bytes; a->chunk_off = one; a->n_chunks = 1; }
    if (a->chunk_off[0] != 0 || a->chunk_off[a->n_chunks] != a->n_bytes)
        return fail(MBPE_ERR_ARG, "chunk_off must start at 0 and end at n_bytes");
    // (every offset is checked before one is used: one beyond n_bytes would index the mask and the text)
    for (uint64_t c = 0; c < a->n_chunks; ++c)
        if (a->chunk_off[c + 1] < a->chunk_off[c]) return fail(MBPE_ERR_ARG, "chunk_off must be ascending");
    return MBPE_OK;
}

// ... and 16-bit ids for a table that has more (word: what the call names the width, "token_bits" or "out_bits")
int vocab16_check(const mbpe_encoder *e, uint32_t bits, const char *word) {
    if (bits != 16 || 256ull + e->n_merges <= 65536ull) return MBPE_OK;
    return fail(MBPE_ERR_VOCAB, std::string(word) + " 16 with more than 65,536 token ids");
}

// the one-token chunks of the whole text, before any pass runs -> e->singles, sorted by start: the caller's list, a
// host text's NUL-led chunks, or a device text's piece by piece (one piece: its mask is then on the device, a->mask_dev)
int gather_singles(mbpe_encoder *e, EncCall *a, const Piece *pieces, size_t n_pieces) {
    int rc = MBPE_OK;
    e->singles.clear();
    if (a->endmask) {
        for (uint64_t k = 0; k < a->n_singles; ++k)
            e->singles.push_back({a->singles[k].start, a->singles[k].len, a->singles[k].id, 0});
    } else if (!a->text_on_device) {
        for (uint64_t c = 0; c < a->n_chunks; ++c) {
            const uint64_t s = a->chunk_off[c], t = a->chunk_off[c + 1];
            long long id;
            if (t > s && a->text[s] == 0 && stoi_value(a->text + s + 1, t - s - 1, &id))
                if ((rc = add_single(e, s, t - s, id, a->token_bits)) != MBPE_OK) return rc;
        }
    } else {
        for (size_t i = 0; i < n_pieces; ++i)
            if ((rc = device_singles(e, a->text, a->chunk_off, pieces[i], a->token_bits)) != MBPE_OK) return rc;
        if (n_pieces == 1) a->mask_dev = e->d_mask;
    }
    return MBPE_OK;
}

// the "dedup" route on its way: nu unique chunks of nub bytes, n_kept chunks (uof: the unique chunk of each), n_sg
// singles, the unique text's piece, and on the device the chunks of the positions asked for (q_chunk: dedup_queries)
struct DedupRun {
    std::string who;
    uint64_t nu = 0, nub = 0, n_kept = 0, n_sg = 0, n_docq = 0;
    const uint8_t *u_text = nullptr, *u_mask = nullptr;
    uint32_t *uof = nullptr;
    int mode = kFinU32;                           // the table's format: the caller's
    PieceRun r;
    unsigned long long *q_chunk = nullptr;
    uint64_t n_entries() const { return nu + n_sg + 1; }      // the unique chunks, the singles, the empty run
};

// stage 1, the deduper: created by the first call that needs it; its stream starts where the encoder's has finished
int dedup_unique(mbpe_encoder *e, const EncCall &a, DedupRun *d) {
    int rc = MBPE_OK;
    if (!e->dd) {
        if ((rc = mbpe_dedup_create(e->device, &e->dd)) != MBPE_OK) return rc;
        if ((rc = mbpe_dedup_set_option(e->dd, "map", 1)) != MBPE_OK) return rc;
    }
    if ((rc = mbpe_dedup_set_option(e->dd, "max_chunk_bytes",
                                    e->dedup_max_chunk >= 0 ? e->dedup_max_chunk : (int64_t)kDedupMaxChunkBytes)) != MBPE_OK)
        return rc;
    const uint8_t *text = a.text;
    const uint64_t n_bytes = a.n_bytes;
    if (a.text_on_device && ((uintptr_t)a.text & 15)) {        // the deduper reads 16 aligned bytes at a time
        if ((rc = e->d_text.reserve(n_bytes, e->mem)) != MBPE_OK) return rc;
        ECHK(hipMemcpyAsync(e->d_text, a.text, n_bytes, hipMemcpyDeviceToDevice, e->stream));
        text = e->d_text;
    }
    ECHK(hipStreamSynchronize(e->stream));
    rc = a.endmask ? mbpe_dedup_chunks_endmask(e->dd, text, n_bytes, a.mask_dev, &d->nu, &d->nub)
                   : mbpe_dedup_chunks(e->dd, text, n_bytes, a.text_on_device, a.chunk_off, a.n_chunks, &d->nu, &d->nub);
    if (rc != MBPE_OK) return rc;
    const uint32_t *uof_view = nullptr;
    float dd_ms = 0.f;
    if ((rc = mbpe_dedup_result(e->dd, &d->u_text, &d->u_mask, nullptr, nullptr)) != MBPE_OK) return rc;
    if ((rc = mbpe_dedup_map(e->dd, &uof_view, &d->n_kept)) != MBPE_OK) return rc;
    if ((rc = mbpe_dedup_kernel_ms(e->dd, &dd_ms)) != MBPE_OK) return rc;
    d->uof = const_cast<uint32_t *>(uof_view);                  // (the singles' chunks are patched in place)
    e->last_ms += dd_ms;
    if (d->n_entries() >= 0xFFFFFFFFull)
        return fail(MBPE_ERR_ARG, d->who + ": 2^32 - 1 table runs or more (option \"dedup\")");
    return MBPE_OK;
}

// stage 2: the unique text through the passes as one piece without any single (e->singles is empty), then the finishing
// kernel writes the table, d_utab, in the caller's format and the runs' ends, d_uends
int dedup_table(mbpe_encoder *e, const EncCall &a, DedupRun *d) {
    const uint64_t nub = d->nub, esz = a.token_bits / 8;
    int rc = MBPE_OK;
    d->r.pn = nub;
    uint64_t limit = 0;
    if ((rc = piece_limit(e, nub, false, &limit)) != MBPE_OK) return rc;
    if (nub > limit)
        return fail(MBPE_ERR_OOM, d->who + ": the unique chunks hold " + std::to_string(nub) +
                                      " bytes, more than one piece may hold (" + std::to_string(limit) +
                                      "; option \"piece_bytes\"), and the \"dedup\" route runs them as one piece");
    const uint64_t one[2] = {0, nub};
    EncCall u = {d->u_text, nub, 1, one, 1};
    u.token_bits = a.token_bits;
    u.mask_dev = d->u_mask;
    if (nub) {
        if ((rc = piece_upload(e, u, Piece{0, 1}, &d->r)) != MBPE_OK) return rc;
        if ((rc = piece_passes(e, 0, &d->r)) != MBPE_OK) return rc;
    }
    const uint64_t n = d->r.n;
    if ((rc = e->d_utab.reserve((n + d->n_sg + 8) * esz, e->mem)) != MBPE_OK) return rc;
    if ((rc = e->d_uends.reserve(d->n_entries() * 8, e->mem)) != MBPE_OK) return rc;
    if (n == 0) return d->nu ? fail(MBPE_ERR_HIP, d->who + ": the unique chunks left no token") : MBPE_OK;
    end_count_launch(e, e->tok[d->r.cur], n);
    finish_launch(e, d->mode, true, e->tok[d->r.cur], n, e->d_utab.get(), 0, e->d_uends, d->nu);
    ECHK(hipEventRecord(e->ev1, e->stream));
    unsigned long long found = 0;
    ECHK(hipMemcpyAsync(&found, e->d_res, 8, hipMemcpyDeviceToHost, e->stream));
    float ms = 0.f;
    if ((rc = e->wait(&ms)) != MBPE_OK) return rc;
    e->last_ms += ms;
    if (found != d->nu) return fail(MBPE_ERR_HIP, d->who + ": the unique chunks and their token runs differ in number");
    return MBPE_OK;
}

// stage 3, whose chunk is asked for: the singles' first and last bytes' (2 n_sg) and, from the endmask calls, the
// documents'.  chunk_off says it on the host; a mask is asked on the device.  Records ev0: the expansion follows
int dedup_queries(mbpe_encoder *e, const EncCall &a, DedupRun *d) {
    d->n_docq = a.endmask && a.doc_off ? a.n_docs + 1 : 0;
    const uint64_t n_sg = d->n_sg, n_docq = d->n_docq, n_q = 2 * n_sg + n_docq;
    int rc = MBPE_OK;
    e->sg_tok.resize(n_sg);
    e->q_pos.assign(n_q, 0);
    for (uint64_t k = 0; k < n_sg; ++k) e->sg_tok[k] = e->dd_singles[k].id | (d->mode == kFinFlags ? kTokEnd : 0u);
    if (a.endmask) {
        for (uint64_t k = 0; k < n_sg; ++k) {
            e->q_pos[k] = e->dd_singles[k].start;
            e->q_pos[n_sg + k] = e->dd_singles[k].start + e->dd_singles[k].len;
        }
        for (uint64_t i = 0; i < n_docq; ++i) e->q_pos[2 * n_sg + i] = a.doc_off[i];
    } else {
        // a single is one chunk, and its index counts the chunks that are not empty
        uint64_t kept = 0, k = 0;
        for (uint64_t c = 0; c < a.n_chunks && k < n_sg; ++c) {
            if (a.chunk_off[c + 1] == a.chunk_off[c]) continue;
            if (a.chunk_off[c] == e->dd_singles[k].start) { e->q_pos[k] = kept; e->q_pos[n_sg + k] = kept + 1; ++k; }
            ++kept;
        }
        if (k != n_sg) return fail(MBPE_ERR_HIP, d->who + ": a one-token chunk is not among the chunks");
    }
    if (!a.count && (rc = e->d_exp_off.reserve((expand_span_count(d->n_kept) + 1) * 8, e->mem)) != MBPE_OK) return rc;
    if (n_q) {
        if ((rc = e->d_q_pos.reserve(n_q * 8, e->mem)) != MBPE_OK) return rc;
        if ((rc = e->d_q_chunk.reserve(n_q * 8, e->mem)) != MBPE_OK) return rc;
        if (n_sg && (rc = e->d_sg_tok.reserve(n_sg * 4, e->mem)) != MBPE_OK) return rc;
    }
    if (n_docq && (rc = e->d_doc_off.reserve(n_docq * 8, e->mem)) != MBPE_OK) return rc;
    // (the mask spans the whole text while span_a and span_off are sized for the unique text: buffers of its own)
    const uint64_t n_blocks = ((a.n_bytes + 31) / 32 + kMaskBlockWords - 1) / kMaskBlockWords;
    if (a.endmask && n_q) {
        if ((rc = e->d_mblk_cnt.reserve(n_blocks * 4, e->mem)) != MBPE_OK) return rc;
        if ((rc = e->d_mblk_off.reserve(n_blocks * 8, e->mem)) != MBPE_OK) return rc;
    }
    ECHK(hipEventRecord(e->ev0, e->stream));
    d->q_chunk = a.endmask ? e->d_q_chunk.get() : e->d_q_pos.get();
    if (n_q == 0) return MBPE_OK;
    ECHK(hipMemcpyAsync(e->d_q_pos, e->q_pos.data(), n_q * 8, hipMemcpyHostToDevice, e->stream));
    if (n_sg) ECHK(hipMemcpyAsync(e->d_sg_tok, e->sg_tok.data(), n_sg * 4, hipMemcpyHostToDevice, e->stream));
    if (a.endmask) {
        const MaskView m = mask_count_launch(e, a.mask_dev, a.n_bytes, e->d_mblk_cnt, e->d_mblk_off);
        mask_query_launch(e, m, e->d_q_pos, 1, n_q, nullptr, 0, 0, e->d_q_chunk);
    }
    return MBPE_OK;
}

// stage 4: the singles become runs of the table, the expansion is counted (nothing is written before the cap is known
// to hold it), written, and what the host asked for is copied to it
int dedup_expand(mbpe_encoder *e, const EncCall &a, const DedupRun &d) {
    const uint64_t n = d.r.n, n_sg = d.n_sg, n_kept = d.n_kept, n_docq = d.n_docq, esz = a.token_bits / 8;
    int rc = MBPE_OK;
    expand_patch_launch(e->stream, e->d_utab.get(), n, a.token_bits, e->d_uends, d.nu, d.uof, n_kept,
                        ExpandSingles{e->d_sg_tok, d.q_chunk, d.q_chunk + n_sg, n_sg});
    const ExpandSrc src = {e->d_utab.get(), n + n_sg, e->d_uends, d.n_entries(), d.uof, n_kept, a.token_bits};
    expand_count_launch(e->stream, src, e->d_exp_off, e->d_res);
    ECHK(hipEventRecord(e->ev1, e->stream));
    unsigned long long total = 0;
    ECHK(hipMemcpyAsync(&total, e->d_res, 8, hipMemcpyDeviceToHost, e->stream));
    float ms_count = 0.f, ms_write = 0.f;
    if ((rc = e->wait(&ms_count)) != MBPE_OK) return rc;

    e->dd_ran = true;
    e->dd_chunks = n_kept;
    e->dd_unique = d.nu;
    e->dd_unique_bytes = d.nub;
    e->dd_unique_tokens = n;
    e->dd_expand_ms = ms_count;
    e->last_ms += ms_count;
    *a.n_out = total;
    if (a.n_passes_out) *a.n_passes_out = d.r.passes;
    // nothing has been written yet: an output that is too small stays as it was
    if (a.tokens_out && a.cap < total) return fail(MBPE_ERR_ARG, "tokens_out too small");

    const bool want_ends = a.chunk_tok_off_out != nullptr;
    const bool to_host = a.tokens_out && !a.out_on_device;
    if (to_host && (rc = e->d_stage.reserve(std::max<uint64_t>(total, 1) * esz, e->mem)) != MBPE_OK) return rc;
    if (want_ends && (rc = e->d_exp_ends.reserve(std::max<uint64_t>(n_kept, 1) * 8, e->mem)) != MBPE_OK) return rc;
    void *out = !a.tokens_out ? nullptr : to_host ? static_cast<void *>(e->d_stage.get()) : a.tokens_out;
    ECHK(hipEventRecord(e->ev0, e->stream));
    if ((out && total) || want_ends)
        expand_write_launch(e->stream, src, e->d_exp_off, out, want_ends ? e->d_exp_ends.get() : nullptr, 0);
    if (n_docq)
        expand_before_launch(e->stream, src, e->d_exp_off, d.q_chunk + 2 * n_sg, n_docq, e->d_doc_off);
    if ((rc = e->finish(&ms_write)) != MBPE_OK) return rc;
    e->dd_expand_ms += ms_write;
    e->last_ms += ms_write;

    if (to_host && total) ECHK(hipMemcpyAsync(a.tokens_out, e->d_stage, total * esz, hipMemcpyDeviceToHost, e->stream));
    if (n_docq && a.doc_tok_off_out)
        ECHK(hipMemcpyAsync(a.doc_tok_off_out, e->d_doc_off, n_docq * 8, hipMemcpyDeviceToHost, e->stream));
    if (want_ends) {
        e->list.resize(n_kept);
        if (n_kept) ECHK(hipMemcpyAsync(e->list.data(), e->d_exp_ends, n_kept * 8, hipMemcpyDeviceToHost, e->stream));
    }
    ECHK(hipStreamSynchronize(e->stream));
    if (want_ends) fill_chunk_tok_off(a, Piece{0, a.n_chunks}, 0, e->list.data(), n_kept);
    return MBPE_OK;
}

// stage 4 of a count call, in place of the expansion: the singles become runs of the table as there, the runs' weights
// are the histogram of the patched map (w[j] = the chunks that copy run j; the one-token chunks and the empty run
// included, by construction), and the table is counted with them into the call's scratch
int dedup_count(mbpe_encoder *e, const EncCall &a, const DedupRun &d) {
    const uint64_t n = d.r.n, n_sg = d.n_sg, n_ent = d.n_entries(), n_ids = e->cnt_ids;
    int rc = MBPE_OK;
    if (n_ent >> 31) return fail(MBPE_ERR_ARG, d.who + ": 2^31 table runs or more (option \"dedup\")");
    if ((rc = e->d_cnt_w.reserve((n_ent + 1) * 8, e->mem)) != MBPE_OK) return rc;
    ECHK(hipMemsetAsync(e->d_cnt_w, 0, (n_ent + 1) * 8, e->stream));
    expand_patch_launch(e->stream, e->d_utab.get(), n, a.token_bits, e->d_uends, d.nu, d.uof, d.n_kept,
                        ExpandSingles{e->d_sg_tok, d.q_chunk, d.q_chunk + n_sg, n_sg});
    hist_tokens_launch(e->stream, d.uof, d.n_kept, 32, e->d_cnt_w, n_ent, e->d_cnt_w + n_ent);
    unsigned long long *call = e->d_cnt_call;
    hist_runs_launch(e->stream, e->d_utab.get(), n + n_sg, a.token_bits, e->d_uends, n_ent, e->d_cnt_w, call, n_ids,
                     call + n_ids, call + n_ids + 1);
    ECHK(hipEventRecord(e->ev1, e->stream));
    unsigned long long total = 0;
    ECHK(hipMemcpyAsync(&total, call + n_ids + 1, 8, hipMemcpyDeviceToHost, e->stream));
    float ms = 0.f;
    if ((rc = e->wait(&ms)) != MBPE_OK) return rc;
    e->dd_ran = true;
    e->dd_chunks = d.n_kept;
    e->dd_unique = d.nu;
    e->dd_unique_bytes = d.nub;
    e->dd_unique_tokens = n;
    e->dd_expand_ms = 0.f;
    e->last_ms += ms;
    *a.n_out = total;
    if (a.n_passes_out) *a.n_passes_out = d.r.passes;
    return MBPE_OK;
}

// a.endmask: the endmask calls (text, mask, singles, doc_off as they state them); else chunk_off, checked, n_bytes > 0
int enc_dedup_body(mbpe_encoder *e, EncCall a) {
    DedupRun d;
    d.who = a.endmask ? "mbpe_encoder_encode_endmask" : "mbpe_encoder_encode";
    d.mode = a.token_bits == 16 ? kFinU16 : a.out_on_device ? kFinFlags : kFinU32;
    if (a.tokens_out && a.out_on_device && ((uintptr_t)a.tokens_out & (a.token_bits / 8 - 1)))
        return fail(MBPE_ERR_ARG, d.who + ": tokens_out must be aligned to its elements (option \"dedup\")");
    ECHK(hipSetDevice(e->device));
    e->dd_ran = false;
    // the chunks that are one token, before anything else (a host text: before the device is touched)
    const Piece all = {0, a.n_chunks};
    int rc = gather_singles(e, &a, &all, 1);
    if (rc != MBPE_OK) return rc;
    e->dd_singles.swap(e->singles);               // (the unique text is encoded without any: piece_upload reads e->singles)
    e->singles.clear();
    d.n_sg = e->dd_singles.size();
    if ((rc = dedup_unique(e, a, &d)) != MBPE_OK) return rc;
    if ((rc = dedup_table(e, a, &d)) != MBPE_OK) return rc;
    if ((rc = dedup_queries(e, a, &d)) != MBPE_OK) return rc;
    return a.count ? dedup_count(e, a, d) : dedup_expand(e, a, d);
}

// what a count call settles before its pieces run: the kept table (allocated and zeroed by the first count call, and
// again when "count_ids" has changed, which only an empty table allows) and the call's zeroed scratch
int count_begin(mbpe_encoder *e, const EncCall &a) {
    if (!a.count) return MBPE_OK;
    const uint64_t want = std::max<uint64_t>(256ull + e->n_merges, e->count_ids);
    if (want != e->cnt_ids) {
        e->cnt_ids = 0;
        int rc = e->d_cnt.reserve((want + 1) * 8, e->mem);
        if (rc == MBPE_OK) rc = e->d_cnt_call.reserve((want + 2) * 8, e->mem);
        if (rc != MBPE_OK) return rc;
        ECHK(hipMemsetAsync(e->d_cnt, 0, (want + 1) * 8, e->stream));
        e->cnt_ids = want;
    }
    ECHK(hipMemsetAsync(e->d_cnt_call, 0, (e->cnt_ids + 2) * 8, e->stream));
    return MBPE_OK;
}

int enc_run_body(mbpe_encoder *e, EncCall a) {
    uint64_t one[2];
    int rc = chunk_off_check(&a, one);
    if (rc == MBPE_OK) rc = vocab16_check(e, a.token_bits, "token_bits");
    if (rc != MBPE_OK) return rc;
    const uint64_t *chunk_off = a.chunk_off;
    const uint64_t n_bytes = a.n_bytes, n_chunks = a.n_chunks;
    if (a.chunk_tok_off_out) a.chunk_tok_off_out[0] = 0;
    e->dd_ran = false;
    if (n_bytes == 0) {
        if (a.chunk_tok_off_out) fill_chunk_tok_off(a, Piece{0, n_chunks}, 0, nullptr, 0);
        if (e->dedup) dedup_nothing(e);
        return boff_begin(e, a);
    }
    ECHK(hipSetDevice(e->device));
    if (int rc0 = boff_begin(e, a)) return rc0;
    if (int rc0 = count_begin(e, a)) return rc0;
    e->last_ms = 0.f;
    e->pass_tokens.clear();
    if (e->dedup) return enc_dedup_body(e, a);

    // pieces: whole chunks, at most `limit` bytes each
    uint64_t limit = 0;
    rc = piece_limit(e, n_bytes, a.tok_byte_off_out && !a.out_on_device, &limit);
    if (rc != MBPE_OK) return rc;
    std::vector<Piece> pieces;
    if (n_bytes <= limit) {
        pieces.push_back({0, n_chunks});
    } else {
        uint64_t c0 = 0;
        while (c0 < n_chunks) {
            uint64_t c1 = c0;
            while (c1 < n_chunks && chunk_off[c1 + 1] - chunk_off[c0] <= limit) ++c1;
            if (c1 == c0)
                return fail(MBPE_ERR_OOM, "chunk " + std::to_string(c0) + " has " +
                                              std::to_string(chunk_off[c0 + 1] - chunk_off[c0]) +
                                              " bytes, more than one piece may hold (" + std::to_string(limit) +
                                              "; option \"piece_bytes\")");
            pieces.push_back({c0, c1});
            c0 = c1;
        }
    }
    if ((rc = gather_singles(e, &a, pieces.data(), pieces.size())) != MBPE_OK) return rc;

    PieceRun sum;
    // "a cap too small writes no token": where the pieces before the one that overflows would already have written
    // theirs, the count comes first (cap >= n_bytes always suffices and never takes this path)
    if (pieces.size() > 1 && a.tokens_out && a.cap < n_bytes) {
        EncCall q = a;
        q.tokens_out = nullptr;
        q.chunk_tok_off_out = nullptr;
        q.tok_byte_off_out = nullptr;
        rc = run_pieces(e, q, pieces, &sum);
        if (rc != MBPE_OK) return rc;
        if (a.cap < sum.n) return enc_report(a, sum, true);
        e->pass_tokens.clear();                    // (the kernel time keeps both runs, the pass counts one)
    }
    rc = run_pieces(e, a, pieces, &sum);
    return rc != MBPE_OK ? rc : enc_report(a, sum, sum.too_small);
}

// (the host vectors -- mask, lists, the bytes of NUL-led chunks -- grow with the text: no exception leaves the C-ABI)
template <typename F>
int enc_guard(const std::string &who, F body) {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, who + ": host allocation failed");
    }
}

// the fill-in-the-middle stage of a batch call (mbpe_encoder_set_fim with rate > 0; n_tokens > 0): e->d_flat and the
// documents' offsets -> e->d_fim_flat and e->d_fim_off, which the pack step then reads.  One wait; the new token count
// and the flag come back with it, and, to_host, the new offsets into e->doc_tok
int enc_fim_stage(mbpe_encoder *e, const EncPack &k, uint64_t n_tokens, bool docs_on_device, bool to_host, uint64_t *n_new,
                  float *ms) {
    const uint64_t n_docs = k.n_docs, cap = n_tokens + 3 * n_docs;   // (every document transformed: no more ids than these)
    int rc = e->d_doc_off.reserve((n_docs + 1) * 8, e->mem);
    if (rc == MBPE_OK) rc = e->d_fim_flat.reserve(cap * (k.token_bits() / 8), e->mem);
    if (rc == MBPE_OK) rc = e->d_fim_off.reserve(fim_off_bytes(n_docs), e->mem);
    if (rc == MBPE_OK) rc = e->d_fim_cut.reserve(n_docs * 16, e->mem);
    if (rc == MBPE_OK) rc = e->d_fim_mode.reserve(n_docs, e->mem);
    if (rc != MBPE_OK) return rc;
    if (!docs_on_device)
        ECHK(hipMemcpyAsync(e->d_doc_off, e->doc_tok.data(), (n_docs + 1) * 8, hipMemcpyHostToDevice, e->stream));
    const FimDst dst = {e->d_fim_flat, cap, e->d_fim_off, e->d_fim_cut, e->d_fim_mode};
    ECHK(hipEventRecord(e->ev0, e->stream));
    fim_launch(e->stream, e->d_flat, n_tokens, k.token_bits(), e->d_doc_off, n_docs, e->fim, dst);
    if ((rc = e->finish(ms)) != MBPE_OK) return rc;
    e->last_ms += *ms;
    unsigned long long res[2] = {0, 0};                          // the new token count, the first document too long
    ECHK(hipMemcpyAsync(res, e->d_fim_off + n_docs, 16, hipMemcpyDeviceToHost, e->stream));
    if (to_host) {
        e->doc_tok.resize(n_docs + 1);
        ECHK(hipMemcpyAsync(e->doc_tok.data(), e->d_fim_off, (n_docs + 1) * 8, hipMemcpyDeviceToHost, e->stream));
    }
    ECHK(hipStreamSynchronize(e->stream));
    if (res[1] != ~0ull)
        return fail(MBPE_ERR_ARG, "fim: document " + std::to_string(res[1]) + " has 2^32 - 1 tokens or more");
    if (res[0] >> 40) return fail(MBPE_ERR_ARG, "fim: more than 2^40 tokens");
    *n_new = res[0];
    e->fim_ran = true;
    return MBPE_OK;
}

// the masked-LM stage of a batch call (mbpe_encoder_set_mlm with select > 0; n_tokens > 0): e->d_flat, which holds the
// passes' 32-bit tokens with their word-end flags (or plain 16-bit ids), and the documents' offsets in e->d_doc_off ->
// e->d_mlm_flat and e->d_mlm_tgt, which the pack step then reads as tokens and label tokens.  One wait, for the time
int enc_mlm_stage(mbpe_encoder *e, const EncPack &k, uint64_t n_tokens, bool docs_on_device, float *ms) {
    const uint64_t n_docs = k.n_docs;
    int rc = e->d_doc_off.reserve((n_docs + 1) * 8, e->mem);
    if (rc == MBPE_OK) rc = e->d_mlm_flat.reserve(n_tokens * (k.token_bits() / 8), e->mem);
    if (rc == MBPE_OK) rc = e->d_mlm_tgt.reserve(n_tokens * 4, e->mem);
    if (rc == MBPE_OK && e->mlm.whole_word) rc = e->d_mlm_scr.reserve(mlm_scratch_bytes(n_tokens), e->mem);
    if (rc != MBPE_OK) return rc;
    if (!docs_on_device)
        ECHK(hipMemcpyAsync(e->d_doc_off, e->doc_tok.data(), (n_docs + 1) * 8, hipMemcpyHostToDevice, e->stream));
    const MlmDst dst = {e->d_mlm_flat, e->d_mlm_tgt, e->d_mlm_scr};
    ECHK(hipEventRecord(e->ev0, e->stream));
    mlm_launch(e->stream, e->d_flat, n_tokens, k.token_bits(), e->d_doc_off, n_docs, e->mlm, dst);
    if ((rc = e->finish(ms)) != MBPE_OK) return rc;
    e->last_ms += *ms;
    return MBPE_OK;
}

// where the index arrays of the denoise stage lie in e->d_dn_idx, for n_docs documents and room for cap units
struct DnIndex {
    uint64_t uoff, unit_doc, in_off, tg_off, res, scratch, words;
    DnIndex(uint64_t n_docs, uint64_t cap) {
        uoff = 0;
        unit_doc = uoff + n_docs + 1;
        in_off = unit_doc + cap;
        tg_off = in_off + cap + 1;
        res = tg_off + cap + 1;
        scratch = res + 4;
        words = scratch + dn_scratch_bytes(n_docs, cap) / 8;
    }
};

// what a _denoise call checks beyond the batch calls' own arguments, before the device is touched
int enc_denoise_check(const mbpe_encoder *e, const EncPack &k) {
    const EncDenoise &dn = *k.dn;
    const mbpe_denoise_batch &o = *dn.out;
    const char *msg = "";
    if (const int rc = denoise_check_spec(dn.spec, k.token_bits(), &msg)) return fail(rc, msg);
    if (e->fim_on || e->mlm_on)
        return fail(MBPE_ERR_ARG, "fill-in-the-middle or masked-LM is on: they do not apply to the denoise calls, turn them off");
    if (const int rc = pack_check_spec(dn.dec_spec, k.token_bits())) return rc;
    if (k.spec->layout != MBPE_PACK_PADDED || dn.dec_spec->layout != MBPE_PACK_PADDED)
        return fail(MBPE_ERR_ARG, "the denoise calls take MBPE_PACK_PADDED specs");
    if (k.spec->out_bits != dn.dec_spec->out_bits)
        return fail(MBPE_ERR_ARG, "the denoise calls take two specs of equal out_bits");
    if (o.enc_ids && !o.dec_ids) return fail(MBPE_ERR_ARG, "enc_ids without dec_ids");
    if (o.row_doc && k.n_docs >= 0xFFFFFFFFull) return fail(MBPE_ERR_ARG, "row_doc needs fewer than 2^32 - 1 documents");
    if (o.enc_ids && k.out_on_device && ((uint64_t)(uintptr_t)o.dec_len % 4 || (uint64_t)(uintptr_t)o.row_doc % 4))
        return fail(MBPE_ERR_ARG, "dec_len or row_doc is not aligned to its elements");
    const mbpe_pack_aux aux = {o.dec_labels, nullptr, nullptr, o.ignore_label};
    return pack_check_aux(*dn.dec_spec, &aux, nullptr, 0, o.dec_ids, o.enc_ids ? k.out_on_device : 0);
}

// the tail of the _denoise calls: the flat tokens in e->d_flat and the documents' token offsets (as for enc_pack_tail)
// -> the stage's two streams, one unit per row -> k_pack_stream's matrix of the inputs and k_pack_aux's of the targets.
// One wait for the stage -- the unit count, both totals and the flag come back with it -- and one for the two packs
int enc_denoise_tail(mbpe_encoder *e, const EncPack &k, uint64_t n_enc, bool docs_on_device) {
    const EncDenoise &dn = *k.dn;
    const mbpe_denoise_batch &o = *dn.out;
    const mbpe_pack_spec &es = *k.spec, &ds = *dn.dec_spec;
    const uint64_t n_docs = k.n_docs, tb = k.token_bits() / 8;
    const bool query = !o.enc_ids;
    *k.n_rows_out = 0;
    if (k.n_tokens_out) *k.n_tokens_out = n_enc;
    if (n_docs == 0) return MBPE_OK;
    // (a document of L tokens has at most 1 + L / segment_tokens units, and neither stream more ids than the tokens)
    const uint64_t cap_units = n_docs + (dn.spec->segment_tokens ? n_enc / dn.spec->segment_tokens : 0);
    const DnIndex ix(n_docs, cap_units);
    int rc = e->d_doc_off.reserve((n_docs + 1) * 8, e->mem);
    if (rc == MBPE_OK) rc = e->d_dn_idx.reserve(ix.words * 8, e->mem);
    if (rc == MBPE_OK && o.row_doc) rc = e->d_dn_row_doc.reserve(cap_units * 4, e->mem);
    if (rc == MBPE_OK && !query) rc = e->d_dn_in.reserve(std::max<uint64_t>(n_enc, 1) * tb, e->mem);
    if (rc == MBPE_OK && !query) rc = e->d_dn_tg.reserve(std::max<uint64_t>(n_enc, 1) * tb, e->mem);
    if (rc != MBPE_OK) return rc;
    if (!docs_on_device)
        ECHK(hipMemcpyAsync(e->d_doc_off, e->doc_tok.data(), (n_docs + 1) * 8, hipMemcpyHostToDevice, e->stream));
    unsigned long long *idx = e->d_dn_idx;
    const DnDst dst = {query ? nullptr : e->d_dn_in.get(), query ? nullptr : e->d_dn_tg.get(), query ? 0 : n_enc,
                       query ? 0 : n_enc, idx + ix.uoff, idx + ix.unit_doc, idx + ix.in_off, idx + ix.tg_off, idx + ix.res,
                       idx + ix.scratch, o.row_doc ? e->d_dn_row_doc.get() : nullptr, cap_units};
    float stage_ms = 0.f;
    ECHK(hipEventRecord(e->ev0, e->stream));
    dn_launch(e->stream, e->d_flat, k.token_bits(), e->d_doc_off, n_docs, *dn.spec, dst);
    if ((rc = e->finish(&stage_ms)) != MBPE_OK) return rc;
    e->last_ms += stage_ms;
    e->pack_ms = stage_ms;
    unsigned long long res[4] = {0, 0, 0, 0};                    // units, input ids, target ids, the first document too long
    ECHK(hipMemcpyAsync(res, idx + ix.res, 32, hipMemcpyDeviceToHost, e->stream));
    ECHK(hipStreamSynchronize(e->stream));
    if (res[3] != ~0ull)
        return fail(MBPE_ERR_ARG, "denoise: document " + std::to_string(res[3]) + " has a unit of 2^32 - 1 tokens or more");
    if (res[0] >> 40) return fail(MBPE_ERR_ARG, "denoise: more than 2^40 units");
    const uint64_t n_rows = res[0];
    *k.n_rows_out = n_rows;
    if (query) return MBPE_OK;
    if (k.cap_rows < n_rows) return fail(MBPE_ERR_ARG, "ids_out too small");
    const uint64_t eb = es.out_bits / 8, enc_bytes = n_rows * es.seq_len * eb, dec_bytes = n_rows * ds.seq_len * eb;
    mbpe_denoise_batch d = o;                                    // where the kernels write
    if (!k.out_on_device) {
        rc = e->d_ids.reserve(enc_bytes, e->mem);
        d.enc_ids = e->d_ids;
        if (rc == MBPE_OK && o.enc_len) { rc = e->d_len.reserve(n_rows * 4, e->mem); d.enc_len = e->d_len; }
        if (rc == MBPE_OK) { rc = e->d_dn_dec_ids.reserve(dec_bytes, e->mem); d.dec_ids = e->d_dn_dec_ids; }
        if (rc == MBPE_OK && o.dec_len) { rc = e->d_dn_dec_len.reserve(n_rows * 4, e->mem); d.dec_len = e->d_dn_dec_len; }
        if (rc == MBPE_OK && o.dec_labels) { rc = e->d_labels.reserve(dec_bytes, e->mem); d.dec_labels = e->d_labels; }
        if (rc != MBPE_OK) return rc;
    }
    const PackSrc src_in = {e->d_dn_in.get(), idx + ix.in_off, n_rows, res[1], k.token_bits()};
    const PackSrc src_tg = {e->d_dn_tg.get(), idx + ix.tg_off, n_rows, res[2], k.token_bits()};
    const mbpe_pack_aux aux = {d.dec_labels, nullptr, nullptr, o.ignore_label};
    float packs_ms = 0.f;
    ECHK(hipEventRecord(e->ev0, e->stream));
    pack_launch(e->stream, src_in, es, {d.enc_ids, d.enc_len, n_rows});
    pack_launch_aux(e->stream, src_tg, ds, {d.dec_ids, d.dec_len, n_rows}, aux);
    if ((rc = e->finish(&packs_ms)) != MBPE_OK) return rc;
    e->last_ms += packs_ms;
    e->pack_ms += packs_ms;
    const hipMemcpyKind kind = k.out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (o.row_doc) ECHK(hipMemcpyAsync(o.row_doc, e->d_dn_row_doc, n_rows * 4, kind, e->stream));
    if (!k.out_on_device) {
        ECHK(hipMemcpyAsync(o.enc_ids, d.enc_ids, enc_bytes, kind, e->stream));
        if (o.enc_len) ECHK(hipMemcpyAsync(o.enc_len, d.enc_len, n_rows * 4, kind, e->stream));
        ECHK(hipMemcpyAsync(o.dec_ids, d.dec_ids, dec_bytes, kind, e->stream));
        if (o.dec_len) ECHK(hipMemcpyAsync(o.dec_len, d.dec_len, n_rows * 4, kind, e->stream));
        if (o.dec_labels) ECHK(hipMemcpyAsync(o.dec_labels, d.dec_labels, dec_bytes, kind, e->stream));
    }
    ECHK(hipStreamSynchronize(e->stream));
    return MBPE_OK;
}

// the pack step of the batch calls: the flat tokens in e->d_flat, the documents' token offsets in e->doc_tok (host;
// docs_on_device: in e->d_doc_off already, and on the host only where doc_tok_off_out asks for them).  With
// fill-in-the-middle on, the stage comes first and everything below reads what it wrote
int enc_pack_tail(mbpe_encoder *e, const EncPack &k, uint64_t n_enc, bool docs_on_device) {
    const mbpe_pack_spec &spec = *k.spec;
    const mbpe_pack_aux *aux = k.aux;
    const uint64_t n_docs = k.n_docs;
    const mbpe_pack_window *win = k.win;
    const struct mbpe_pack_fit *fit = k.fit;
    int rc = MBPE_OK;
    uint64_t n_tokens = n_enc;                                   // tokens the packers read
    float rows_ms = 0.f;                                         // the kernels before the pack kernel
    e->fim_docs = n_docs;
    e->fim_ran = false;
    if (k.dn) return enc_denoise_tail(e, k, n_enc, docs_on_device);
    const bool fim = e->fim_on && e->fim.rate && n_enc;
    if (fim) {
        const bool to_host = k.doc_tok_off_out || fit || (aux && n_enc + 3 * n_docs + 2 >= (1ull << 32));
        if ((rc = enc_fim_stage(e, k, n_enc, docs_on_device, to_host, &n_tokens, &rows_ms)) != MBPE_OK) return rc;
        e->pack_ms = rows_ms;
        if (aux && to_host && (rc = pack_check_aux(spec, aux, e->doc_tok.data(), n_docs, nullptr, 0)) != MBPE_OK) return rc;
    }
    const bool mlm = e->mlm_on && e->mlm.select && n_enc;        // (never with fim: enc_batch_check)
    if (mlm) {
        if ((rc = enc_mlm_stage(e, k, n_enc, docs_on_device, &rows_ms)) != MBPE_OK) return rc;
        e->pack_ms = rows_ms;
    }
    uint64_t n_rows = win ? 0 : pack_rows(spec, n_tokens, n_docs);
    if (fit) {
        // the rows depend on the plan, and the plan is host work: from e->doc_tok, which both callers have filled
        if ((rc = pack_fit_make(e->doc_tok.data(), n_docs, spec, &e->fit_plan)) != MBPE_OK) return rc;
        n_rows = e->fit_plan.n_rows;
    }
    if (win && n_docs) {
        // the row count depends on the tokens: k_win_rows, the scan and k_win_offsets over the device's offsets, then the total
        rc = e->d_doc_off.reserve((n_docs + 1) * 8, e->mem);
        if (rc == MBPE_OK) rc = e->d_row_start.reserve(pack_win_scratch_bytes(n_docs), e->mem);
        if (rc != MBPE_OK) return rc;
        if (!docs_on_device && !fim && !mlm)
            ECHK(hipMemcpyAsync(e->d_doc_off, e->doc_tok.data(), (n_docs + 1) * 8, hipMemcpyHostToDevice, e->stream));
        float win_ms = 0.f;
        ECHK(hipEventRecord(e->ev0, e->stream));
        pack_launch_win_rows(e->stream, fim ? e->d_fim_off : e->d_doc_off, n_docs, spec, *win, e->d_row_start);
        if ((rc = e->finish(&win_ms)) != MBPE_OK) return rc;
        unsigned long long total = 0;
        ECHK(hipMemcpyAsync(&total, e->d_row_start + n_docs, 8, hipMemcpyDeviceToHost, e->stream));
        ECHK(hipStreamSynchronize(e->stream));
        if (total > (1ull << 40)) return fail(MBPE_ERR_ARG, "more than 2^40 rows");
        n_rows = total;
        rows_ms += win_ms;
        e->pack_ms = rows_ms;
        e->last_ms += win_ms;
    }
    *k.n_rows_out = n_rows;
    if (k.n_tokens_out) *k.n_tokens_out = n_enc;
    if (k.ids_out && k.cap_rows < n_rows) return fail(MBPE_ERR_ARG, "ids_out too small");
    if (k.doc_tok_off_out) std::copy(e->doc_tok.begin(), e->doc_tok.end(), k.doc_tok_off_out);   // (filled in both cases)
    if (!k.ids_out) return MBPE_OK;                              // the query
    if (n_rows == 0) return fit ? pack_fit_doc_out(e->stream, *fit, e->fit_plan, k.out_on_device) : MBPE_OK;
    const uint64_t id_bytes = n_rows * spec.seq_len * (spec.out_bits / 8), cell_bytes = n_rows * spec.seq_len * 4;
    rc = e->d_doc_off.reserve((n_docs + 1) * 8, e->mem);
    if (rc == MBPE_OK && fit) {
        rc = e->d_fit_pieces.reserve(pack_fit_piece_bytes(e->fit_plan), e->mem);
        if (rc == MBPE_OK) rc = e->d_fit_rows.reserve((n_rows + 1) * 8, e->mem);
    }
    if (rc == MBPE_OK && !k.out_on_device) {
        rc = e->d_ids.reserve(id_bytes, e->mem);
        if (rc == MBPE_OK && k.len_out) rc = e->d_len.reserve(n_rows * 4, e->mem);
    }
    mbpe_pack_aux d_aux = aux ? *aux : mbpe_pack_aux{};
    if (rc == MBPE_OK && aux && !k.out_on_device) {
        if (aux->labels) { rc = e->d_labels.reserve(id_bytes, e->mem); d_aux.labels = e->d_labels; }
        if (rc == MBPE_OK && aux->pos) { rc = e->d_pos.reserve(cell_bytes, e->mem); d_aux.pos = e->d_pos; }
        if (rc == MBPE_OK && aux->seg) { rc = e->d_seg.reserve(cell_bytes, e->mem); d_aux.seg = e->d_seg; }
    }
    mbpe_pack_window d_win = win ? *win : mbpe_pack_window{};
    if (rc == MBPE_OK && win && !k.out_on_device) {
        if (win->row_doc) { rc = e->d_row_doc.reserve(n_rows * 4, e->mem); d_win.row_doc = e->d_row_doc; }
        if (rc == MBPE_OK && win->row_tok0) {
            rc = e->d_row_tok0.reserve(n_rows * 8, e->mem);
            d_win.row_tok0 = reinterpret_cast<uint64_t *>(e->d_row_tok0.get());
        }
    }
    if (rc != MBPE_OK) return rc;
    if (!docs_on_device && !win && !fim && !mlm)
        ECHK(hipMemcpyAsync(e->d_doc_off, e->doc_tok.data(), (n_docs + 1) * 8, hipMemcpyHostToDevice, e->stream));
    const PackSrc src = {fim ? e->d_fim_flat.get() : mlm ? e->d_mlm_flat.get() : e->d_flat.get(),
                         fim ? e->d_fim_off : e->d_doc_off, n_docs, n_tokens, k.token_bits(),
                         mlm ? e->d_mlm_tgt.get() : nullptr};
    const PackDst dst = {k.out_on_device ? k.ids_out : e->d_ids.get(),
                         k.out_on_device || !k.len_out ? k.len_out : e->d_len.get(), n_rows};
    if (fit) {
        ECHK(hipMemcpyAsync(e->d_fit_pieces, e->fit_plan.pieces.data(), pack_fit_piece_bytes(e->fit_plan),
                            hipMemcpyHostToDevice, e->stream));
        ECHK(hipMemcpyAsync(e->d_fit_rows, e->fit_plan.row_first.data(), (n_rows + 1) * 8, hipMemcpyHostToDevice, e->stream));
    }
    ECHK(hipEventRecord(e->ev0, e->stream));
    if (fit) pack_launch_fit(e->stream, src, spec, dst, d_aux, e->d_fit_pieces, e->d_fit_rows);
    else if (win) pack_launch_windows(e->stream, src, spec, dst, d_aux, d_win, e->d_row_start);
    else if (aux) pack_launch_aux(e->stream, src, spec, dst, d_aux);
    else pack_launch(e->stream, src, spec, dst);
    if ((rc = e->finish(&e->pack_ms)) != MBPE_OK) return rc;
    e->last_ms += e->pack_ms;
    e->pack_ms += rows_ms;
    if (!k.out_on_device) {
        ECHK(hipMemcpyAsync(k.ids_out, e->d_ids, id_bytes, hipMemcpyDeviceToHost, e->stream));
        if (k.len_out) ECHK(hipMemcpyAsync(k.len_out, e->d_len, n_rows * 4, hipMemcpyDeviceToHost, e->stream));
        if (aux && aux->labels) ECHK(hipMemcpyAsync(aux->labels, e->d_labels, id_bytes, hipMemcpyDeviceToHost, e->stream));
        if (aux && aux->pos) ECHK(hipMemcpyAsync(aux->pos, e->d_pos, cell_bytes, hipMemcpyDeviceToHost, e->stream));
        if (aux && aux->seg) ECHK(hipMemcpyAsync(aux->seg, e->d_seg, cell_bytes, hipMemcpyDeviceToHost, e->stream));
        if (win && win->row_doc) ECHK(hipMemcpyAsync(win->row_doc, e->d_row_doc, n_rows * 4, hipMemcpyDeviceToHost, e->stream));
        if (win && win->row_tok0) ECHK(hipMemcpyAsync(win->row_tok0, e->d_row_tok0, n_rows * 8, hipMemcpyDeviceToHost, e->stream));
        ECHK(hipStreamSynchronize(e->stream));
    }
    return fit ? pack_fit_doc_out(e->stream, *fit, e->fit_plan, k.out_on_device) : MBPE_OK;
}

// what the batch calls check alike once their own arguments are in order (the document lengths: after the encode)
int enc_batch_check(const mbpe_encoder *e, const EncPack &k) {
    if (const int rc = vocab16_check(e, k.spec->out_bits, "out_bits")) return rc;
    if (k.ids_out && k.out_on_device &&
        ((uint64_t)(uintptr_t)k.ids_out % (k.spec->out_bits / 8) || (uint64_t)(uintptr_t)k.len_out % 4))
        return fail(MBPE_ERR_ARG, "ids_out or len_out is not aligned to its elements");
    if (k.dn) return enc_denoise_check(e, k);
    if (e->fim_on) {
        const char *msg = "";
        if (const int rc = fim_check_spec(&e->fim, k.token_bits(), &msg)) return fail(rc, msg);
    }
    if (e->mlm_on) {
        const char *msg = "";
        if (e->fim_on) return fail(MBPE_ERR_ARG, "fill-in-the-middle and masked-LM are both on: turn one of them off");
        if (const int rc = mlm_check_spec(&e->mlm, k.token_bits(), &msg)) return fail(rc, msg);
    }
    if (k.win) return pack_check_windows(k.spec, k.token_bits(), k.aux, k.win, k.n_docs, k.ids_out, k.out_on_device);
    if (k.fit) return pack_check_fit(k.spec, k.token_bits(), k.aux, k.fit, k.n_docs, k.ids_out, k.out_on_device);
    return k.aux ? pack_check_aux(*k.spec, k.aux, nullptr, k.n_docs, k.ids_out, k.out_on_device) : MBPE_OK;
}

// the flat buffer both batch calls encode into, as the request's output
int enc_batch_flat(mbpe_encoder *e, EncCall *a, const EncPack &k, uint64_t *n_tokens) {
    ECHK(hipSetDevice(e->device));
    const int rc = e->d_flat.reserve(std::max<uint64_t>(a->n_bytes, 1) * (k.token_bits() / 8), e->mem);
    if (rc != MBPE_OK) return rc;
    e->pack_ms = 0.f;
    enc_out(a, e->d_flat, a->n_bytes, k.token_bits(), 1, n_tokens, nullptr);
    return MBPE_OK;
}

// encode into the kept flat buffer, then pack from it on the encoder's stream (arguments checked by the caller)
int enc_batch_body(mbpe_encoder *e, EncCall a, const EncPack &k) {
    uint64_t n_tokens = 0;
    int rc = enc_batch_flat(e, &a, k, &n_tokens);
    if (rc != MBPE_OK) return rc;
    e->last_ms = 0.f;
    e->chunk_tok.assign(a.n_chunks + 1, 0);
    a.chunk_tok_off_out = e->chunk_tok.data();
    rc = enc_run_body(e, a);
    if (rc != MBPE_OK) return rc;
    e->doc_tok.resize(k.n_docs + 1);
    for (uint64_t i = 0; i <= k.n_docs; ++i) e->doc_tok[i] = e->chunk_tok[k.doc_chunk_off[i]];
    // (the document lengths exist only now: the limit of pos comes here, still before the pack kernel)
    if (k.aux) rc = pack_check_aux(*k.spec, k.aux, e->doc_tok.data(), k.n_docs, nullptr, 0);
    if (rc != MBPE_OK) return rc;
    return enc_pack_tail(e, k, n_tokens, false);
}

// mbpe_encoder_encode_endmask after its checks: one piece, text and mask where they are
int enc_endmask_body(mbpe_encoder *e, EncCall a) {
    const uint64_t n_bytes = a.n_bytes, n_docs = a.n_docs;
    if (a.doc_off && a.doc_tok_off_out) a.doc_tok_off_out[0] = 0;
    ECHK(hipSetDevice(e->device));
    e->last_ms = 0.f;
    e->pass_tokens.clear();
    e->dd_ran = false;
    if (int rc0 = boff_begin(e, a)) return rc0;
    if (n_bytes == 0) {
        if (e->dedup) dedup_nothing(e);
        if (a.doc_off) {
            int rc = e->d_doc_off.reserve((n_docs + 1) * 8, e->mem);
            if (rc != MBPE_OK) return rc;
            ECHK(hipMemsetAsync(e->d_doc_off, 0, (n_docs + 1) * 8, e->stream));
            ECHK(hipStreamSynchronize(e->stream));
            if (a.doc_tok_off_out) std::fill(a.doc_tok_off_out, a.doc_tok_off_out + n_docs + 1, 0);
        }
        return MBPE_OK;
    }
    if (int rc0 = count_begin(e, a)) return rc0;
    if (e->dedup) return enc_dedup_body(e, a);
    uint64_t limit = 0;                                           // the rule of mbpe_encoder_encode
    int rc = piece_limit(e, n_bytes, a.tok_byte_off_out && !a.out_on_device, &limit);
    if (rc != MBPE_OK) return rc;
    if (n_bytes > limit)
        return fail(MBPE_ERR_OOM, "mbpe_encoder_encode_endmask: the text has " + std::to_string(n_bytes) +
                                      " bytes, more than one piece may hold (" + std::to_string(limit) +
                                      "; option \"piece_bytes\"), and a mask on the device is not cut into pieces");
    const uint64_t one[2] = {0, n_bytes};
    const Piece all = {0, 1};
    a.chunk_off = one;
    a.n_chunks = 1;
    if ((rc = gather_singles(e, &a, &all, 1)) != MBPE_OK) return rc;
    PieceRun r;
    rc = run_piece(e, a, all, 0, &r);
    return rc != MBPE_OK ? rc : enc_report(a, r, r.too_small);
}

// the checks of the two endmask calls that need neither encoder nor device
int enc_endmask_check(const char *who, uint64_t n_bytes, const mbpe_single *singles, uint64_t n_singles,
                      const uint64_t *doc_off, uint64_t n_docs, uint32_t token_bits) {
    const std::string w(who);
    if (token_bits != 16 && token_bits != 32) return fail(MBPE_ERR_ARG, w + ": token_bits must be 16 or 32");
    if ((!singles && n_singles) || (!doc_off && n_docs)) return fail(MBPE_ERR_ARG, w + ": NULL argument");
    uint64_t end = 0;
    for (uint64_t k = 0; k < n_singles; ++k) {
        const mbpe_single &g = singles[k];
        if (g.len == 0 || g.start > n_bytes || g.len > n_bytes - g.start)
            return fail(MBPE_ERR_ARG, w + ": single " + std::to_string(k) + " is empty or out of range");
        if (g.start < end) return fail(MBPE_ERR_ARG, w + ": singles must be ascending and disjoint");
        end = g.start + g.len;
        if (g.id >= kDrop) return fail(MBPE_ERR_ARG, w + ": token id of a single does not fit 31 bits");
        if (token_bits == 16 && g.id >= 65536u)
            return fail(MBPE_ERR_VOCAB, w + ": token id " + std::to_string(g.id) + " of a single does not fit 16 bits");
    }
    for (uint64_t i = 0; i < n_docs; ++i)
        if (doc_off[i + 1] < doc_off[i]) return fail(MBPE_ERR_ARG, w + ": doc_off must be ascending");
    if (n_docs && doc_off[n_docs] > n_bytes) return fail(MBPE_ERR_ARG, w + ": doc_off must not exceed n_bytes");
    return MBPE_OK;
}

// what the endmask calls say of their input: a device text whose chunks are its mask's
EncCall endmask_call(const uint8_t *text_dev, uint64_t n_bytes, const uint8_t *endmask_dev, const mbpe_single *singles,
                     uint64_t n_singles, const uint64_t *doc_off, uint64_t n_docs) {
    EncCall a = {text_dev, n_bytes, 1, nullptr, 0};
    a.mask_dev = endmask_dev;
    a.endmask = true;
    a.singles = singles;
    a.n_singles = n_singles;
    a.doc_off = doc_off;
    a.n_docs = n_docs;
    return a;
}

// the one-shot calls: a temporary encoder and one call
int encode_chunks(int device_id, const uint8_t *text, uint64_t n_bytes, const uint64_t *chunk_off, uint64_t n_chunks,
                  const uint32_t *merges, uint32_t n_merges, uint32_t *tokens_out, uint64_t cap, uint64_t *n_out,
                  uint32_t *n_passes_out, bool out_on_device) {
    if (n_out) *n_out = 0;
    if (n_passes_out) *n_passes_out = 0;
    if (!n_out || (!text && n_bytes) || (!merges && n_merges)) return fail(MBPE_ERR_ARG, "mbpe_encode_chunks: NULL argument");
    mbpe_encoder *e = nullptr;
    int rc = mbpe_encoder_create(device_id, merges, n_merges, &e);
    if (rc != MBPE_OK) return rc;
    EncCall a = {text, n_bytes, 0, chunk_off, n_chunks};
    enc_out(&a, tokens_out, cap, 32, out_on_device ? 1 : 0, n_out, n_passes_out);
    rc = enc_guard("mbpe_encoder_encode", [&] { return enc_run_body(e, a); });
    const std::string keep = rc == MBPE_OK ? std::string() : std::string(mbpe_host::last_error());
    mbpe_encoder_destroy(e);
    if (rc != MBPE_OK) mbpe_host::set_last_error(keep);
    return rc;
}

}  // namespace

extern "C" {

int mbpe_encoder_create(int device_id, const uint32_t *merges, uint32_t n_merges, mbpe_encoder **out) {
    if (!out || (!merges && n_merges)) return fail(MBPE_ERR_ARG, "mbpe_encoder_create: NULL argument");
    *out = nullptr;
    // host side: the pair -> id table
    uint32_t bits = 4;
    while ((1ull << bits) < 2ull * n_merges + 2) ++bits;
    const uint32_t capacity = 1u << bits;
    std::vector<unsigned long long> keys;
    std::vector<uint32_t> vals;
    try {
        keys.assign(capacity, kEmptyKey);
        vals.assign(capacity, 0);
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_encoder_create: host allocation failed");
    }
    for (uint32_t k = 0; k < n_merges; ++k) {       // merges_lookup[pair] = 256 + k: a repeated pair keeps the last id
        const unsigned long long key = ((unsigned long long)merges[2 * k] << 32) | merges[2 * k + 1];
        uint32_t h = pair_hash(key, 64 - bits);
        while (keys[h] != kEmptyKey && keys[h] != key) h = (h + 1) & (capacity - 1);
        keys[h] = key;
        vals[h] = 256 + k;
    }
    if (find_device(device_id) != MBPE_OK) return MBPE_ERR_NO_DEVICE;
    mbpe_encoder *e = new (std::nothrow) mbpe_encoder;
    if (!e) return fail(MBPE_ERR_OOM, "mbpe_encoder_create: host allocation failed");
    e->n_merges = n_merges;
    // len[id], for the byte offsets: only a trained table makes the bytes a token covers a function of its id
    if (mbpe_merges_check(merges, n_merges) != MBPE_OK) {
        e->len_error = mbpe_host::last_error();
    } else {
        try {
            e->len.assign(256 + (size_t)n_merges, 1u);
        } catch (const std::bad_alloc &) {
            delete e;
            return fail(MBPE_ERR_OOM, "mbpe_encoder_create: host allocation failed");
        }
        for (uint32_t k = 0; k < n_merges && e->len_error.empty(); ++k) {
            const uint64_t l = (uint64_t)e->len[merges[2 * k]] + e->len[merges[2 * k + 1]];
            if (l > 0xFFFFFFFFull) e->len_error = "token " + std::to_string(256 + k) + " is longer than 2^32 - 1 bytes";
            e->len[256 + k] = (uint32_t)l;
        }
    }
    auto build = [&]() -> int {
        int rc = e->open(device_id);
        if (rc == MBPE_OK) rc = e->d_keys.reserve((uint64_t)capacity * 8, e->mem);
        if (rc == MBPE_OK) rc = e->d_vals.reserve((uint64_t)capacity * 4, e->mem);
        if (rc == MBPE_OK) rc = e->d_res.reserve(24, e->mem);
        if (rc != MBPE_OK) return rc;
        ECHK(hipMemcpyAsync(e->d_keys, keys.data(), (size_t)capacity * 8, hipMemcpyHostToDevice, e->stream));
        ECHK(hipMemcpyAsync(e->d_vals, vals.data(), (size_t)capacity * 4, hipMemcpyHostToDevice, e->stream));
        ECHK(hipStreamSynchronize(e->stream));
        return MBPE_OK;
    };
    const int rc = build();
    if (rc != MBPE_OK) {
        const std::string keep = mbpe_host::last_error();
        mbpe_encoder_destroy(e);
        mbpe_host::set_last_error(keep);
        return rc;
    }
    e->lut = {e->d_keys, e->d_vals, 64 - bits, capacity - 1};
    *out = e;
    return MBPE_OK;
}

void mbpe_encoder_destroy(mbpe_encoder *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->dd) mbpe_dedup_destroy(e->dd);
    delete e;                                 // the buffers, then the events, then the stream
}

int mbpe_encoder_set_option(mbpe_encoder *e, const char *name, int64_t value) {
    if (!e || !name) return fail(MBPE_ERR_ARG, "mbpe_encoder_set_option: NULL argument");
    if (strcmp(name, "piece_bytes") == 0) {
        if (value < 0) return fail(MBPE_ERR_ARG, "piece_bytes must not be negative");
        e->piece_bytes = (uint64_t)value;
        return MBPE_OK;
    }
    if (strcmp(name, "rank_order") == 0) {
        if (value != 0 && value != 1) return fail(MBPE_ERR_ARG, "rank_order must be 0 or 1");
        e->rank_order = value == 1;
        return MBPE_OK;
    }
    if (strcmp(name, "dedup") == 0) {
        if (value != 0 && value != 1) return fail(MBPE_ERR_ARG, "dedup must be 0 or 1");
        e->dedup = value == 1;
        return MBPE_OK;
    }
    if (strcmp(name, "dedup_max_chunk_bytes") == 0) {
        if (value < 0 || value > 0x7FFFFFFF) return fail(MBPE_ERR_ARG, "dedup_max_chunk_bytes must lie in [0, 2^31)");
        e->dedup_max_chunk = value;
        return MBPE_OK;
    }
    if (strcmp(name, "count_ids") == 0) {
        if (value < 0 || value > (int64_t)MBPE_MAX_COUNT_IDS)
            return fail(MBPE_ERR_ARG, "count_ids must lie in 0 .. MBPE_MAX_COUNT_IDS");
        if (e->cnt_used)
            return fail(MBPE_ERR_STATE, "count_ids: tokens have been counted (mbpe_encoder_counts_reset comes first)");
        e->count_ids = (uint64_t)value;
        return MBPE_OK;
    }
    return fail(MBPE_ERR_ARG, std::string("mbpe_encoder_set_option: no option \"") + name + "\"");
}

int mbpe_dropout_threshold(double p, uint64_t *threshold_out) {
    if (!threshold_out) return fail(MBPE_ERR_ARG, "mbpe_dropout_threshold: NULL argument");
    unsigned long long t = 0;
    if (!dropout_threshold(p, &t)) return fail(MBPE_ERR_ARG, "mbpe_dropout_threshold: p must lie in [0, 1]");
    *threshold_out = t;
    return MBPE_OK;
}

int mbpe_encoder_set_dropout(mbpe_encoder *e, uint64_t threshold, uint64_t seed) {
    if (!e) return fail(MBPE_ERR_ARG, "mbpe_encoder_set_dropout: NULL argument");
    if (threshold > kDropoutOne) return fail(MBPE_ERR_ARG, "mbpe_encoder_set_dropout: threshold must not exceed 2^32");
    e->drop_threshold = threshold;
    e->drop_seed = seed;
    return MBPE_OK;
}

int mbpe_encoder_set_fim(mbpe_encoder *e, const mbpe_fim_spec *spec) {
    if (!e) return fail(MBPE_ERR_ARG, "mbpe_encoder_set_fim: NULL argument");
    if (spec) {
        const char *msg = "";
        if (const int rc = fim_check_spec(spec, 32, &msg)) return fail(rc, std::string("mbpe_encoder_set_fim: ") + msg);
        e->fim = *spec;
    }
    e->fim_on = spec != nullptr;
    return MBPE_OK;
}

int mbpe_encoder_set_mlm(mbpe_encoder *e, const mbpe_mlm_spec *spec) {
    if (!e) return fail(MBPE_ERR_ARG, "mbpe_encoder_set_mlm: NULL argument");
    if (spec) {
        const char *msg = "";
        if (const int rc = mlm_check_spec(spec, 32, &msg)) return fail(rc, std::string("mbpe_encoder_set_mlm: ") + msg);
        e->mlm = *spec;
    }
    e->mlm_on = spec != nullptr;
    return MBPE_OK;
}

int mbpe_encoder_fim_info(mbpe_encoder *e, uint8_t *mode_out, uint64_t *cut_out, uint64_t cap_docs, uint64_t *n_docs_out) {
    if (!e || !n_docs_out) return fail(MBPE_ERR_ARG, "mbpe_encoder_fim_info: NULL argument");
    const uint64_t n = e->fim_docs;
    *n_docs_out = n;
    if (!mode_out && !cut_out) return MBPE_OK;
    if (cap_docs < n) return fail(MBPE_ERR_ARG, "mbpe_encoder_fim_info: room for fewer documents than the call had");
    if (n == 0) return MBPE_OK;
    if (!e->fim_ran) {                                           // the stage was off: every document is as it was
        if (mode_out) std::fill(mode_out, mode_out + n, 0);
        if (cut_out) std::fill(cut_out, cut_out + 2 * n, 0);
        return MBPE_OK;
    }
    ECHK(hipSetDevice(e->device));
    if (mode_out) ECHK(hipMemcpyAsync(mode_out, e->d_fim_mode, n, hipMemcpyDeviceToHost, e->stream));
    if (cut_out) ECHK(hipMemcpyAsync(cut_out, e->d_fim_cut, n * 16, hipMemcpyDeviceToHost, e->stream));
    ECHK(hipStreamSynchronize(e->stream));
    return MBPE_OK;
}

int mbpe_encoder_encode_byteoff(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                const uint64_t *chunk_off, uint64_t n_chunks, void *tokens_out, uint64_t cap,
                                uint32_t token_bits, int out_on_device, uint64_t *tok_byte_off_out,
                                uint64_t *chunk_tok_off_out, uint64_t *n_out, uint32_t *n_passes_out) {
    if (n_out) *n_out = 0;
    if (n_passes_out) *n_passes_out = 0;
    if (!e || !n_out || (!text && n_bytes)) return fail(MBPE_ERR_ARG, "mbpe_encoder_encode: NULL argument");
    if (token_bits != 16 && token_bits != 32) return fail(MBPE_ERR_ARG, "token_bits must be 16 or 32");
    EncCall a = {text, n_bytes, text_on_device, chunk_off, n_chunks};
    enc_out(&a, tokens_out, cap, token_bits, out_on_device, n_out, n_passes_out);
    a.chunk_tok_off_out = chunk_tok_off_out;
    a.tok_byte_off_out = tok_byte_off_out;
    int rc = drop_check(e, "mbpe_encoder_encode");
    if (rc == MBPE_OK) rc = dedup_check(e, "mbpe_encoder_encode", tok_byte_off_out);
    if (rc == MBPE_OK) rc = boff_check(e, "mbpe_encoder_encode_byteoff", &a);
    if (rc != MBPE_OK) return rc;
    return enc_guard("mbpe_encoder_encode", [&] { return enc_run_body(e, a); });
}

int mbpe_encoder_encode(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                        const uint64_t *chunk_off, uint64_t n_chunks, void *tokens_out, uint64_t cap,
                        uint32_t token_bits, int out_on_device, uint64_t *chunk_tok_off_out, uint64_t *n_out,
                        uint32_t *n_passes_out) {
    return mbpe_encoder_encode_byteoff(e, text, n_bytes, text_on_device, chunk_off, n_chunks, tokens_out, cap, token_bits,
                                       out_on_device, nullptr, chunk_tok_off_out, n_out, n_passes_out);
}

// mbpe_encoder_encode_batch (aux NULL) and mbpe_encoder_encode_batch_aux: the checks that need no device, then the call
static int enc_batch(mbpe_encoder *e, EncCall a, const EncPack &k) {
    if (k.n_rows_out) *k.n_rows_out = 0;
    if (k.n_tokens_out) *k.n_tokens_out = 0;
    if (!e || !k.n_rows_out || !k.doc_chunk_off || !k.spec || (!a.text && a.n_bytes))
        return fail(MBPE_ERR_ARG, "mbpe_encoder_encode_batch: NULL argument");
    int rc = drop_check(e, "mbpe_encoder_encode_batch");
    if (rc == MBPE_OK) rc = dedup_check(e, "mbpe_encoder_encode_batch", nullptr);
    if (rc == MBPE_OK) rc = pack_check_spec(k.spec, k.token_bits());
    if (rc != MBPE_OK) return rc;
    uint64_t one[2];
    if ((rc = chunk_off_check(&a, one)) != MBPE_OK) return rc;
    if (k.doc_chunk_off[0] != 0 || k.doc_chunk_off[k.n_docs] != a.n_chunks)
        return fail(MBPE_ERR_ARG, "doc_chunk_off must start at 0 and end at n_chunks");
    for (uint64_t i = 0; i < k.n_docs; ++i)
        if (k.doc_chunk_off[i + 1] < k.doc_chunk_off[i]) return fail(MBPE_ERR_ARG, "doc_chunk_off must be ascending");
    rc = enc_batch_check(e, k);
    if (rc != MBPE_OK) return rc;
    return enc_guard("mbpe_encoder_encode_batch", [&] { return enc_batch_body(e, a, k); });
}

int mbpe_encoder_encode_batch_windows(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                      const uint64_t *chunk_off, uint64_t n_chunks, const uint64_t *doc_chunk_off,
                                      uint64_t n_docs, const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows,
                                      int out_on_device, uint32_t *len_out, uint64_t *n_rows_out, uint64_t *n_tokens_out,
                                      const mbpe_pack_aux *aux, uint64_t *doc_tok_off_out, const mbpe_pack_window *win) {
    if (n_rows_out) *n_rows_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!aux || !win) return fail(MBPE_ERR_ARG, "mbpe_encoder_encode_batch_windows: NULL argument");
    return enc_batch(e, {text, n_bytes, text_on_device, chunk_off, n_chunks},
                     {doc_chunk_off, n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, n_tokens_out, aux,
                      doc_tok_off_out, win});
}

int mbpe_encoder_encode_batch_fit(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                  const uint64_t *chunk_off, uint64_t n_chunks, const uint64_t *doc_chunk_off,
                                  uint64_t n_docs, const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows,
                                  int out_on_device, uint32_t *len_out, uint64_t *n_rows_out, uint64_t *n_tokens_out,
                                  const mbpe_pack_aux *aux, uint64_t *doc_tok_off_out, const struct mbpe_pack_fit *fit) {
    if (n_rows_out) *n_rows_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!aux || !fit) return fail(MBPE_ERR_ARG, "mbpe_encoder_encode_batch_fit: NULL argument");
    return enc_batch(e, {text, n_bytes, text_on_device, chunk_off, n_chunks},
                     {doc_chunk_off, n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, n_tokens_out, aux,
                      doc_tok_off_out, nullptr, fit});
}

int mbpe_encoder_encode_batch_aux(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                  const uint64_t *chunk_off, uint64_t n_chunks, const uint64_t *doc_chunk_off,
                                  uint64_t n_docs, const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows,
                                  int out_on_device, uint32_t *len_out, uint64_t *n_rows_out, uint64_t *n_tokens_out,
                                  const mbpe_pack_aux *aux, uint64_t *doc_tok_off_out) {
    if (n_rows_out) *n_rows_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!aux) return fail(MBPE_ERR_ARG, "mbpe_encoder_encode_batch_aux: NULL argument");
    return enc_batch(e, {text, n_bytes, text_on_device, chunk_off, n_chunks},
                     {doc_chunk_off, n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, n_tokens_out, aux,
                      doc_tok_off_out});
}

int mbpe_encoder_encode_batch(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                              const uint64_t *chunk_off, uint64_t n_chunks, const uint64_t *doc_chunk_off,
                              uint64_t n_docs, const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows,
                              int out_on_device, uint32_t *len_out, uint64_t *n_rows_out, uint64_t *n_tokens_out) {
    return enc_batch(e, {text, n_bytes, text_on_device, chunk_off, n_chunks},
                     {doc_chunk_off, n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, n_tokens_out,
                      nullptr, nullptr});
}

int mbpe_encoder_encode_batch_denoise(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                      const uint64_t *chunk_off, uint64_t n_chunks, const uint64_t *doc_chunk_off,
                                      uint64_t n_docs, const mbpe_denoise_spec *dn, const mbpe_pack_spec *enc_spec,
                                      const mbpe_pack_spec *dec_spec, const mbpe_denoise_batch *out, uint64_t cap_rows,
                                      int out_on_device, uint64_t *n_rows_out, uint64_t *n_tokens_out) {
    if (n_rows_out) *n_rows_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!dn || !dec_spec || !out) return fail(MBPE_ERR_ARG, "mbpe_encoder_encode_batch_denoise: NULL argument");
    const EncDenoise d = {dn, dec_spec, out};
    return enc_batch(e, {text, n_bytes, text_on_device, chunk_off, n_chunks},
                     {doc_chunk_off, n_docs, enc_spec, out->enc_ids, cap_rows, out_on_device, out->enc_len, n_rows_out,
                      n_tokens_out, nullptr, nullptr, nullptr, nullptr, &d});
}

int mbpe_encoder_encode_endmask(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes, const uint8_t *endmask_dev,
                                const mbpe_single *singles, uint64_t n_singles, const uint64_t *doc_off, uint64_t n_docs,
                                void *tokens_out, uint64_t cap, uint32_t token_bits, int out_on_device,
                                uint64_t *doc_tok_off_out, uint64_t *n_out, uint32_t *n_passes_out) {
    return mbpe_encoder_encode_endmask_byteoff(e, text_dev, n_bytes, endmask_dev, singles, n_singles, doc_off, n_docs,
                                               tokens_out, cap, token_bits, out_on_device, nullptr, doc_tok_off_out, n_out,
                                               n_passes_out);
}

int mbpe_encoder_encode_endmask_byteoff(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes,
                                        const uint8_t *endmask_dev, const mbpe_single *singles, uint64_t n_singles,
                                        const uint64_t *doc_off, uint64_t n_docs, void *tokens_out, uint64_t cap,
                                        uint32_t token_bits, int out_on_device, uint64_t *tok_byte_off_out,
                                        uint64_t *doc_tok_off_out, uint64_t *n_out, uint32_t *n_passes_out) {
    static_assert(sizeof(mbpe_single) == sizeof(SingleChunk), "mbpe.h and k_enc_single");
    if (n_out) *n_out = 0;
    if (n_passes_out) *n_passes_out = 0;
    int rc = enc_endmask_check("mbpe_encoder_encode_endmask", n_bytes, singles, n_singles, doc_off, n_docs, token_bits);
    if (rc != MBPE_OK) return rc;
    if (!e || !n_out || ((!text_dev || !endmask_dev) && n_bytes))
        return fail(MBPE_ERR_ARG, "mbpe_encoder_encode_endmask: NULL argument");
    if ((rc = drop_check(e, "mbpe_encoder_encode_endmask")) != MBPE_OK) return rc;
    if ((rc = dedup_check(e, "mbpe_encoder_encode_endmask", tok_byte_off_out)) != MBPE_OK) return rc;
    if ((uintptr_t)endmask_dev & 3) return fail(MBPE_ERR_ARG, "mbpe_encoder_encode_endmask: the mask must be 4-byte aligned");
    if ((rc = vocab16_check(e, token_bits, "token_bits")) != MBPE_OK) return rc;
    EncCall a = endmask_call(text_dev, n_bytes, endmask_dev, singles, n_singles, n_docs ? doc_off : nullptr, n_docs);
    enc_out(&a, tokens_out, cap, token_bits, out_on_device, n_out, n_passes_out);
    a.doc_tok_off_out = doc_tok_off_out;
    a.tok_byte_off_out = tok_byte_off_out;
    if ((rc = boff_check(e, "mbpe_encoder_encode_endmask_byteoff", &a)) != MBPE_OK) return rc;
    return enc_guard("mbpe_encoder_encode_endmask", [&] { return enc_endmask_body(e, a); });
}

// mbpe_encoder_encode_batch_endmask (win and fit NULL), mbpe_encoder_encode_batch_endmask_windows and _fit
static int enc_batch_endmask(const std::string &who, mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes,
                             const uint8_t *endmask_dev, const mbpe_single *singles, uint64_t n_singles,
                             const uint64_t *doc_off, uint64_t n_docs, const mbpe_pack_spec *spec, void *ids_out,
                             uint64_t cap_rows, int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                             uint64_t *n_tokens_out, const mbpe_pack_aux *aux, uint64_t *doc_tok_off_out,
                             const mbpe_pack_window *win, const struct mbpe_pack_fit *fit = nullptr,
                             const EncDenoise *dn = nullptr) {
    if (n_rows_out) *n_rows_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!spec || !doc_off || !n_rows_out) return fail(MBPE_ERR_ARG, who + ": NULL argument");
    const EncPack k = {nullptr, n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, n_tokens_out, aux,
                       doc_tok_off_out, win, fit, dn};
    int rc = pack_check_spec(spec, k.token_bits());
    if (rc != MBPE_OK) return rc;
    rc = enc_endmask_check(who.c_str(), n_bytes, singles, n_singles, doc_off, n_docs, k.token_bits());
    if (rc != MBPE_OK) return rc;
    if (doc_off[0] != 0 || doc_off[n_docs] != n_bytes)
        return fail(MBPE_ERR_ARG, who + ": doc_off must start at 0 and end at n_bytes");
    if (!e || ((!text_dev || !endmask_dev) && n_bytes)) return fail(MBPE_ERR_ARG, who + ": NULL argument");
    if ((rc = drop_check(e, who)) != MBPE_OK) return rc;
    if ((rc = dedup_check(e, who, nullptr)) != MBPE_OK) return rc;
    if ((uintptr_t)endmask_dev & 3) return fail(MBPE_ERR_ARG, who + ": the mask must be 4-byte aligned");
    rc = enc_batch_check(e, k);
    if (rc != MBPE_OK) return rc;
    return enc_guard(who, [&]() -> int {
        EncCall a = endmask_call(text_dev, n_bytes, endmask_dev, singles, n_singles, doc_off, n_docs);
        // (enc_batch_flat: where the tokens go)
        uint64_t n_tokens = 0;
        int rc = enc_batch_flat(e, &a, k, &n_tokens);
        if (rc != MBPE_OK) return rc;
        // the offsets stay on the device; the host sees them where it asks for them, or where a document could be too
        // long for pos (only a text of 2^32 bytes or more), or where the fit plan is made of them
        const bool to_host = doc_tok_off_out || fit || (aux && n_bytes + 2 >= (1ull << 32));
        e->doc_tok.assign(n_docs + 1, 0);
        a.doc_tok_off_out = to_host ? e->doc_tok.data() : nullptr;
        rc = enc_endmask_body(e, a);
        if (rc != MBPE_OK) return rc;
        if (aux && to_host) rc = pack_check_aux(*spec, aux, e->doc_tok.data(), n_docs, nullptr, 0);
        if (rc != MBPE_OK) return rc;
        return enc_pack_tail(e, k, n_tokens, true);
    });
}

int mbpe_encoder_encode_batch_endmask(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes,
                                      const uint8_t *endmask_dev, const mbpe_single *singles, uint64_t n_singles,
                                      const uint64_t *doc_off, uint64_t n_docs, const mbpe_pack_spec *spec, void *ids_out,
                                      uint64_t cap_rows, int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                                      uint64_t *n_tokens_out, const mbpe_pack_aux *aux, uint64_t *doc_tok_off_out) {
    return enc_batch_endmask("mbpe_encoder_encode_batch_endmask", e, text_dev, n_bytes, endmask_dev, singles, n_singles,
                             doc_off, n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, n_tokens_out, aux,
                             doc_tok_off_out, nullptr);
}

int mbpe_encoder_encode_batch_endmask_denoise(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes,
                                              const uint8_t *endmask_dev, const mbpe_single *singles, uint64_t n_singles,
                                              const uint64_t *doc_off, uint64_t n_docs, const mbpe_denoise_spec *dn,
                                              const mbpe_pack_spec *enc_spec, const mbpe_pack_spec *dec_spec,
                                              const mbpe_denoise_batch *out, uint64_t cap_rows, int out_on_device,
                                              uint64_t *n_rows_out, uint64_t *n_tokens_out) {
    if (n_rows_out) *n_rows_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!dn || !dec_spec || !out) return fail(MBPE_ERR_ARG, "mbpe_encoder_encode_batch_endmask_denoise: NULL argument");
    const EncDenoise d = {dn, dec_spec, out};
    return enc_batch_endmask("mbpe_encoder_encode_batch_endmask_denoise", e, text_dev, n_bytes, endmask_dev, singles,
                             n_singles, doc_off, n_docs, enc_spec, out->enc_ids, cap_rows, out_on_device, out->enc_len,
                             n_rows_out, n_tokens_out, nullptr, nullptr, nullptr, nullptr, &d);
}

int mbpe_encoder_encode_batch_endmask_windows(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes,
                                              const uint8_t *endmask_dev, const mbpe_single *singles, uint64_t n_singles,
                                              const uint64_t *doc_off, uint64_t n_docs, const mbpe_pack_spec *spec,
                                              void *ids_out, uint64_t cap_rows, int out_on_device, uint32_t *len_out,
                                              uint64_t *n_rows_out, uint64_t *n_tokens_out, const mbpe_pack_aux *aux,
                                              uint64_t *doc_tok_off_out, const mbpe_pack_window *win) {
    if (n_rows_out) *n_rows_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!aux || !win) return fail(MBPE_ERR_ARG, "mbpe_encoder_encode_batch_endmask_windows: NULL argument");
    return enc_batch_endmask("mbpe_encoder_encode_batch_endmask_windows", e, text_dev, n_bytes, endmask_dev, singles,
                             n_singles, doc_off, n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out,
                             n_tokens_out, aux, doc_tok_off_out, win);
}

int mbpe_encoder_encode_batch_endmask_fit(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes,
                                          const uint8_t *endmask_dev, const mbpe_single *singles, uint64_t n_singles,
                                          const uint64_t *doc_off, uint64_t n_docs, const mbpe_pack_spec *spec,
                                          void *ids_out, uint64_t cap_rows, int out_on_device, uint32_t *len_out,
                                          uint64_t *n_rows_out, uint64_t *n_tokens_out, const mbpe_pack_aux *aux,
                                          uint64_t *doc_tok_off_out, const struct mbpe_pack_fit *fit) {
    if (n_rows_out) *n_rows_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!aux || !fit) return fail(MBPE_ERR_ARG, "mbpe_encoder_encode_batch_endmask_fit: NULL argument");
    return enc_batch_endmask("mbpe_encoder_encode_batch_endmask_fit", e, text_dev, n_bytes, endmask_dev, singles, n_singles,
                             doc_off, n_docs, spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, n_tokens_out,
                             aux, doc_tok_off_out, nullptr, fit);
}

// ---- the count calls (hist.h) -----------------------------------------------------------------------------------------
// what they check on the host beyond their encode counterparts: repeat, the table's size, and the total, without wrapping
static int count_check(const mbpe_encoder *e, const std::string &who, uint64_t n_bytes, uint64_t repeat) {
    if (repeat == 0) return fail(MBPE_ERR_ARG, who + ": repeat must be at least 1");
    if (256ull + e->n_merges > MBPE_MAX_COUNT_IDS)
        return fail(MBPE_ERR_VOCAB, who + ": more than MBPE_MAX_COUNT_IDS token ids");
    // S + n_bytes * repeat < 2^64  <=>  n_bytes <= (2^64 - 1 - S) / repeat
    if (n_bytes > (~0ull - e->cnt_tokens) / repeat)
        return fail(MBPE_ERR_OVERFLOW, who + ": the weighted token total could reach 2^64");
    return MBPE_OK;
}

// the call's scratch into the kept table, `other` included; nothing can fail before it that has not failed already
static int count_fold(mbpe_encoder *e, uint64_t repeat, uint64_t n_tokens) {
    ECHK(hipEventRecord(e->ev0, e->stream));
    hist_fold_launch(e->stream, e->d_cnt, e->d_cnt_call, e->cnt_ids + 1, repeat);
    float ms = 0.f;
    const int rc = e->finish(&ms);
    if (rc != MBPE_OK) return rc;
    e->last_ms += ms;
    e->cnt_tokens += repeat * n_tokens;
    e->cnt_used = true;
    return MBPE_OK;
}

int mbpe_encoder_count(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                       const uint64_t *chunk_off, uint64_t n_chunks, uint64_t repeat, uint64_t *n_tokens_out,
                       uint32_t *n_passes_out) {
    if (n_tokens_out) *n_tokens_out = 0;
    if (n_passes_out) *n_passes_out = 0;
    if (!e || !n_tokens_out || (!text && n_bytes)) return fail(MBPE_ERR_ARG, "mbpe_encoder_count: NULL argument");
    EncCall a = {text, n_bytes, text_on_device, chunk_off, n_chunks};
    enc_out(&a, nullptr, 0, 32, 0, n_tokens_out, n_passes_out);
    a.count = true;
    int rc = drop_check(e, "mbpe_encoder_count");
    if (rc == MBPE_OK) rc = dedup_check(e, "mbpe_encoder_count", nullptr);
    if (rc == MBPE_OK) rc = count_check(e, "mbpe_encoder_count", n_bytes, repeat);
    if (rc != MBPE_OK) return rc;
    return enc_guard("mbpe_encoder_count", [&] {
        const int rc = enc_run_body(e, a);
        return rc != MBPE_OK || n_bytes == 0 ? rc : count_fold(e, repeat, *n_tokens_out);
    });
}

int mbpe_encoder_count_endmask(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes, const uint8_t *endmask_dev,
                               const mbpe_single *singles, uint64_t n_singles, uint64_t repeat, uint64_t *n_tokens_out,
                               uint32_t *n_passes_out) {
    if (n_tokens_out) *n_tokens_out = 0;
    if (n_passes_out) *n_passes_out = 0;
    int rc = enc_endmask_check("mbpe_encoder_count_endmask", n_bytes, singles, n_singles, nullptr, 0, 32);
    if (rc != MBPE_OK) return rc;
    if (!e || !n_tokens_out || ((!text_dev || !endmask_dev) && n_bytes))
        return fail(MBPE_ERR_ARG, "mbpe_encoder_count_endmask: NULL argument");
    if ((rc = drop_check(e, "mbpe_encoder_count_endmask")) != MBPE_OK) return rc;
    if ((rc = dedup_check(e, "mbpe_encoder_count_endmask", nullptr)) != MBPE_OK) return rc;
    if ((uintptr_t)endmask_dev & 3) return fail(MBPE_ERR_ARG, "mbpe_encoder_count_endmask: the mask must be 4-byte aligned");
    if ((rc = count_check(e, "mbpe_encoder_count_endmask", n_bytes, repeat)) != MBPE_OK) return rc;
    EncCall a = endmask_call(text_dev, n_bytes, endmask_dev, singles, n_singles, nullptr, 0);
    enc_out(&a, nullptr, 0, 32, 0, n_tokens_out, n_passes_out);
    a.count = true;
    return enc_guard("mbpe_encoder_count_endmask", [&] {
        const int rc = enc_endmask_body(e, a);
        return rc != MBPE_OK || n_bytes == 0 ? rc : count_fold(e, repeat, *n_tokens_out);
    });
}

int mbpe_encoder_counts(mbpe_encoder *e, uint64_t *counts_out, uint64_t cap_ids, int out_on_device, uint64_t *n_ids_out,
                        uint64_t *n_other_out, uint64_t *n_tokens_out) {
    if (!e) return fail(MBPE_ERR_ARG, "mbpe_encoder_counts: NULL argument");
    // (before the first count call, and after "count_ids" has changed, the table is what the next count call will
    // allocate: all zeros)
    const uint64_t n_ids = std::max<uint64_t>(256ull + e->n_merges, e->count_ids);
    const bool live = e->cnt_ids == n_ids;
    if (n_ids_out) *n_ids_out = n_ids;
    if (n_tokens_out) *n_tokens_out = e->cnt_tokens;
    if (n_other_out) *n_other_out = 0;
    if (counts_out && cap_ids < n_ids) return fail(MBPE_ERR_ARG, "counts_out too small");
    if (counts_out && out_on_device && ((uintptr_t)counts_out & 7))
        return fail(MBPE_ERR_ARG, "mbpe_encoder_counts: counts_out in device memory must be 8-byte aligned");
    if (!live && !(counts_out && out_on_device)) {
        if (counts_out) std::fill(counts_out, counts_out + n_ids, 0);
        return MBPE_OK;
    }
    ECHK(hipSetDevice(e->device));
    if (!live) {
        ECHK(hipMemsetAsync(counts_out, 0, n_ids * 8, e->stream));
        ECHK(hipStreamSynchronize(e->stream));
        return MBPE_OK;
    }
    unsigned long long other = 0;
    if (counts_out)
        ECHK(hipMemcpyAsync(counts_out, e->d_cnt, n_ids * 8, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                            e->stream));
    if (n_other_out) ECHK(hipMemcpyAsync(&other, e->d_cnt + n_ids, 8, hipMemcpyDeviceToHost, e->stream));
    ECHK(hipStreamSynchronize(e->stream));
    if (n_other_out) *n_other_out = other;
    return MBPE_OK;
}

int mbpe_encoder_counts_reset(mbpe_encoder *e) {
    if (!e) return fail(MBPE_ERR_ARG, "mbpe_encoder_counts_reset: NULL argument");
    if (e->cnt_ids) {
        ECHK(hipSetDevice(e->device));
        ECHK(hipMemsetAsync(e->d_cnt, 0, (e->cnt_ids + 1) * 8, e->stream));
        ECHK(hipStreamSynchronize(e->stream));
    }
    e->cnt_tokens = 0;
    e->cnt_used = false;
    return MBPE_OK;
}

int mbpe_encoder_pack_ms(const mbpe_encoder *e, float *ms_out) {
    if (!e || !ms_out) return fail(MBPE_ERR_ARG, "mbpe_encoder_pack_ms: NULL argument");
    *ms_out = e->pack_ms;
    return MBPE_OK;
}

int mbpe_encoder_kernel_ms(const mbpe_encoder *e, float *ms_out) {
    if (!e || !ms_out) return fail(MBPE_ERR_ARG, "mbpe_encoder_kernel_ms: NULL argument");
    *ms_out = e->last_ms;
    return MBPE_OK;
}

int mbpe_encoder_pass_tokens(const mbpe_encoder *e, uint64_t *tokens_out, uint32_t cap, uint32_t *n_out) {
    if (!e || !n_out) return fail(MBPE_ERR_ARG, "mbpe_encoder_pass_tokens: NULL argument");
    *n_out = (uint32_t)e->pass_tokens.size();
    if (!tokens_out) return MBPE_OK;
    if (cap < e->pass_tokens.size()) return fail(MBPE_ERR_ARG, "tokens_out too small");
    for (size_t k = 0; k < e->pass_tokens.size(); ++k) tokens_out[k] = e->pass_tokens[k];
    return MBPE_OK;
}

int mbpe_encoder_dedup_stats(const mbpe_encoder *e, uint64_t *n_chunks_out, uint64_t *n_unique_out,
                             uint64_t *n_unique_bytes_out, uint64_t *n_unique_tokens_out, float *expand_ms_out) {
    if (!e) return fail(MBPE_ERR_ARG, "mbpe_encoder_dedup_stats: NULL argument");
    if (!e->dd_ran) return fail(MBPE_ERR_STATE, "mbpe_encoder_dedup_stats: the latest call did not dedup");
    if (n_chunks_out) *n_chunks_out = e->dd_chunks;
    if (n_unique_out) *n_unique_out = e->dd_unique;
    if (n_unique_bytes_out) *n_unique_bytes_out = e->dd_unique_bytes;
    if (n_unique_tokens_out) *n_unique_tokens_out = e->dd_unique_tokens;
    if (expand_ms_out) *expand_ms_out = e->dd_expand_ms;
    return MBPE_OK;
}

int mbpe_encoder_alloc_count(const mbpe_encoder *e, uint64_t *n_out) {
    if (!e || !n_out) return fail(MBPE_ERR_ARG, "mbpe_encoder_alloc_count: NULL argument");
    *n_out = e->mem.n_allocs;
    return MBPE_OK;
}

int mbpe_encode_chunks(int device_id, const uint8_t *text, uint64_t n_bytes, const uint64_t *chunk_off,
                       uint64_t n_chunks, const uint32_t *merges, uint32_t n_merges, uint32_t *tokens_out,
                       uint64_t cap, uint64_t *n_out, uint32_t *n_passes_out) {
    return encode_chunks(device_id, text, n_bytes, chunk_off, n_chunks, merges, n_merges, tokens_out, cap, n_out,
                         n_passes_out, false);
}

int mbpe_encode_chunks_device(int device_id, const uint8_t *text, uint64_t n_bytes, const uint64_t *chunk_off,
                              uint64_t n_chunks, const uint32_t *merges, uint32_t n_merges, uint32_t *tokens_dev_out,
                              uint64_t cap, uint64_t *n_out, uint32_t *n_passes_out) {
    return encode_chunks(device_id, text, n_bytes, chunk_off, n_chunks, merges, n_merges, tokens_dev_out, cap, n_out,
                         n_passes_out, true);
}

}  // extern "C"
