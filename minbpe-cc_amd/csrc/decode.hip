// Decode on the device: Tokenizer::decode (reference Tokenizer.h:725-751) for a whole token stream at once.
//
// The reference appends, token by token, the special's string (the reverse lookup is asked FIRST, :729-733), nothing
// for an id beyond the vocabulary (a warning, :734-737) or vocab[id] (:738-741), where vocab[256 + k] =
// vocab[a_k] ++ vocab[b_k] (:562-564).  That is: per token a byte length, an exclusive prefix sum of the lengths, and
// a copy of every token's bytes to its offset.
//
// Device data of a decoder (built once on the host): len[E] (u32), off[E] (u64) and one flat byte blob.  Entries
// 0 .. V-1 (V = 256 + n_merges) are the vocabulary, with the entries of ids that a special overrides patched; the
// specials with ids >= V follow as entries V .. E-1 and are found through a small open-addressed table that is
// probed only for ids >= V.
//
// A span = 1,024 consecutive tokens = the unit one wave walks (span.h), as in encode.hip and wide.hip.
//   k_dec_len<F>     token -> length; per span the byte total (u64); ids that decode to nothing are counted
//   k_dec_scan64     exclusive 64-bit scan of the span totals (one workgroup, 4,096 spans per step)
//   k_dec_write<F>   per span: prefix sums of the lengths into LDS, then OUTPUT-centric copying: the span's output
//                    range is cut at the 16-byte boundaries of the global output address, a lane owns one piece per
//                    iteration, finds the token that holds the piece's first byte by binary search in the LDS offsets,
//                    gathers from the blob and stores one dwordx4.  Only the first and the last piece of a span, which
//                    it shares with its neighbours, are written byte by byte.  A token of any length costs what its
//                    bytes cost.
//   k_dec_bounds<F>  batches only (mbpe_decode_batch): the byte offset of every document boundary.  Span-centric like
//                    the rest: the wave of span s owns the boundaries t with t / 1,024 == s (two binary searches in
//                    the sorted token offsets find them), builds the span's prefix sums as k_dec_write does and
//                    stores span_off[s] + prefix[t - base] for each, lanes striding over the boundaries.  A span
//                    without a boundary reads no token.
// F is how a token is read (DecFmt): all of them yield "id or nothing".
//
// Bytes moved per decode: the tokens twice (4 B or 2 B each), the output once; len / off / blob are gathered from
// cache (a few hundred KB to a few MB for text vocabularies).  A batch adds the tokens of the spans that hold a
// boundary once more, and 16 B per boundary (its token offset in, its byte offset out).
#include "hip_host.h"
#include "span.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

namespace {

using namespace mbpe;

constexpr int kScanPer = 4;                // spans per thread and step of the scan
constexpr uint32_t kNone = 0xFFFFFFFFu;   // free slot of the specials' table
constexpr uint32_t kBlobPad = 16;          // a 16-byte gather may read this far beyond an entry

// how a token is read; the 16-bit layouts are those of mbpe_stream_device (mbpe.h)
enum DecFmt {
    kFmtU32 = 0,        // plain uint32_t ids
    kFmtU32End = 1,     // the layout of span.h: bit 31 = last token of its chunk, all-ones = hole
    kFmtU16 = 2,        // 16-bit slots, all-ones = hole
    kFmtU16End = 3,     // ... bit 15 = last token of its chunk
    kFmtU16Barrier = 4, // ... one slot value is the barrier after a chunk, no token
    kFmtU16Plain = 5    // plain uint16_t ids as mbpe_encoder_encode writes them: no flag, no hole, 0xFFFF is an id
};

struct DecTab {
    const uint32_t *len;                   // [n_entries]
    const unsigned long long *off;         // [n_entries] into blob
    const uint8_t *blob;
    const uint32_t *sp_key;                // ids >= V that are specials (open addressing, linear probing)
    const uint32_t *sp_ent;                // their entries; kNone = free slot
    uint32_t V;                            // 256 + n_merges
    uint32_t sp_mask;                      // capacity - 1
    uint32_t sp_shift;                     // 32 - log2(capacity)
    uint32_t sp_n;                         // 0: no such special, the table is not probed
};

__host__ __device__ inline uint32_t dec_hash(uint32_t id, uint32_t shift) { return (id * 0x9E3779B1u) >> shift; }

// slot i -> id; false: the slot holds no token (hole, barrier)
template <int F>
__device__ __forceinline__ bool dec_read(const void *__restrict__ tok, uint64_t i, uint32_t barrier, uint32_t *id) {
    if (F == kFmtU32 || F == kFmtU32End) {
        const uint32_t t = static_cast<const uint32_t *>(tok)[i];
        if (F == kFmtU32End && t == kTokNone) return false;
        *id = F == kFmtU32End ? (t & kTokIdMask) : t;
        return true;
    }
    const uint32_t s = static_cast<const uint16_t *>(tok)[i];
    if (F == kFmtU16Plain) { *id = s; return true; }
    if (s == 0xFFFFu) return false;
    if (F == kFmtU16Barrier && s == barrier) return false;
    *id = F == kFmtU16End ? (s & 0x7FFFu) : s;
    return true;
}

// id -> entry of len / off; false: the id decodes to nothing (Tokenizer.h:734-737)
__device__ __forceinline__ bool dec_entry(const DecTab &tab, uint32_t id, uint32_t *ent) {
    if (id < tab.V) { *ent = id; return true; }
    if (!tab.sp_n) return false;
    uint32_t h = dec_hash(id, tab.sp_shift);
    for (;;) {
        const uint32_t e = tab.sp_ent[h];
        if (e == kNone) return false;
        if (tab.sp_key[h] == id) { *ent = e; return true; }
        h = (h + 1) & tab.sp_mask;
    }
}

template <int F>
__global__ __launch_bounds__(kSpanThreads) void k_dec_len(const void *__restrict__ tok, uint64_t n, uint32_t barrier,
                                                          DecTab tab, unsigned long long *__restrict__ span_total,
                                                          unsigned long long *__restrict__ n_invalid) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    unsigned long long sum = 0;
    uint32_t bad = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        uint32_t id, ent;
        if (i < n && dec_read<F>(tok, i, barrier, &id)) {
            if (dec_entry(tab, id, &ent)) sum += tab.len[ent];
            else ++bad;
        }
    }
    for (int d = kWave / 2; d; d >>= 1) {
        sum += __shfl_xor(sum, d, kWave);
        bad += __shfl_xor(bad, d, kWave);
    }
    if (lane == 0) {
        span_total[span] = sum;
        if (bad) atomicAdd(n_invalid, (unsigned long long)bad);
    }
}

// v[s] <- sum of v[0 .. s-1], in place; *total <- the sum of all.  One workgroup walks the spans in steps of
// kScanThreads * kScanPer with a running carry (span.h's scans are 32-bit and one slice per thread).
__global__ __launch_bounds__(kScanThreads) void k_dec_scan64(unsigned long long *__restrict__ v, uint64_t n,
                                                             unsigned long long *__restrict__ total) {
    __shared__ unsigned long long wsum[kScanThreads / kWave];
    const uint32_t lane = lane_id(), wave = threadIdx.x / kWave;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n; base += (uint64_t)kScanThreads * kScanPer) {
        const uint64_t i0 = base + (uint64_t)threadIdx.x * kScanPer;
        unsigned long long x[kScanPer], t = 0;
        for (int j = 0; j < kScanPer; ++j) {
            x[j] = i0 + j < n ? v[i0 + j] : 0ull;
            t += x[j];
        }
        unsigned long long incl = t;
        for (int d = 1; d < kWave; d <<= 1) {
            const unsigned long long up = __shfl_up(incl, d, kWave);
            if (lane >= (uint32_t)d) incl += up;
        }
        if (lane == kWave - 1) wsum[wave] = incl;
        __syncthreads();
        unsigned long long before = 0, tile = 0;
        for (uint32_t w = 0; w < kScanThreads / kWave; ++w) {
            const unsigned long long s = wsum[w];
            if (w < wave) before += s;
            tile += s;
        }
        unsigned long long o = carry + before + incl - t;
        for (int j = 0; j < kScanPer; ++j) {
            if (i0 + j < n) v[i0 + j] = o;
            o += x[j];
        }
        carry += tile;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// 16 bytes from any address (the blob is padded so that this never leaves it)
__device__ __forceinline__ unsigned __int128 load16(const uint8_t *p) {
    unsigned __int128 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

// One wave, the span that starts at token `base`: s_off[j] = bytes of the span before its token j (s_off[kSpan] = the
// span's total, below 2^32: MBPE_DECODER_MAX_ENTRY) and, with kSrc, s_src[j] = where token j's bytes start in the
// blob (below 2^32: MBPE_DECODER_MAX_BLOB).  Tokens at or beyond n count as nothing.
template <int F, bool kSrc>
__device__ __forceinline__ void dec_span_prefix(const void *__restrict__ tok, uint64_t n, uint32_t barrier,
                                                const DecTab &tab, uint64_t base, uint32_t lane, uint32_t *s_off,
                                                uint32_t *s_src) {
    uint32_t run = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        uint32_t id, ent, l = 0, src = 0;
        if (i < n && dec_read<F>(tok, i, barrier, &id) && dec_entry(tab, id, &ent)) {
            l = tab.len[ent];
            if (kSrc) src = (uint32_t)tab.off[ent];
        }
        uint32_t incl = l;
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, kWave);
            if (lane >= (uint32_t)d) incl += up;
        }
        s_off[it * kWave + lane] = run + incl - l;
        if (kSrc) s_src[it * kWave + lane] = src;
        run += __shfl(incl, kWave - 1, kWave);
    }
    if (lane == 0) s_off[kSpan] = run;
}

template <int F>
__global__ __launch_bounds__(kSpanThreads) void k_dec_write(const void *__restrict__ tok, uint64_t n, uint32_t barrier,
                                                            DecTab tab, const unsigned long long *__restrict__ span_off,
                                                            uint8_t *__restrict__ out) {
    __shared__ uint32_t s_off[kSpanWaves][kSpan + 1];
    __shared__ uint32_t s_src[kSpanWaves][kSpan];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint64_t span = span_index();
    const uint64_t base = span * kSpan;
    const bool active = base < n;
    if (active) dec_span_prefix<F, true>(tok, n, barrier, tab, base, lane, s_off[w], s_src[w]);
    __syncthreads();
    if (!active) return;
    const uint32_t T = s_off[w][kSpan];
    if (T == 0) return;                              // a span that decodes to nothing
    const uint64_t out_addr = (uint64_t)(uintptr_t)out;
    const uint64_t A = out_addr + span_off[span];    // address of the span's first output byte
    const uint64_t B0 = A & ~15ull;
    const uint64_t n_pieces = (A + T - B0 + 15) >> 4;
    for (uint64_t p = lane; p < n_pieces; p += kWave) {
        const uint64_t B = B0 + (p << 4);
        const uint64_t lo = B > A ? B : A;
        const uint64_t hi = B + 16 < A + T ? B + 16 : A + T;
        const uint32_t cnt = (uint32_t)(hi - lo);    // 1 .. 16
        uint32_t pos = (uint32_t)(lo - A);
        uint32_t j = 0;                              // the largest j with s_off[j] <= pos: the token that holds byte pos
        for (uint32_t step = kSpan / 2; step; step >>= 1)
            if (s_off[w][j + step] <= pos) j += step;
        unsigned __int128 acc = 0;
        uint32_t filled = 0;
        while (filled < cnt) {                       // ends: bytes pos .. hi-A-1 lie in tokens j .. kSpan-1
            const uint32_t avail = s_off[w][j + 1] - pos;
            if (avail) {
                const uint32_t take = avail < cnt - filled ? avail : cnt - filled;
                unsigned __int128 v = load16(tab.blob + s_src[w][j] + (pos - s_off[w][j]));
                if (take < 16) v &= ((unsigned __int128)1 << (8 * take)) - 1;
                acc |= v << (8 * filled);
                filled += take;
                pos += take;
            }
            ++j;
        }
        if (cnt == 16) {
            u32x4 q;
            q.x = (uint32_t)acc;
            q.y = (uint32_t)(acc >> 32);
            q.z = (uint32_t)(acc >> 64);
            q.w = (uint32_t)(acc >> 96);
            *static_cast<u32x4 *>(__builtin_assume_aligned(out + (B - out_addr), 16)) = q;
        } else {                                     // the span's first or last piece: shared with a neighbour
            uint8_t *dst = out + (lo - out_addr);
            for (uint32_t b = 0; b < cnt; ++b) dst[b] = (uint8_t)(acc >> (8 * b));
        }
    }
}

// the first index b of the ascending v[0 .. n_v) with v[b] >= x (n_v when there is none)
__device__ __forceinline__ uint64_t dec_lower_bound(const unsigned long long *__restrict__ v, uint64_t n_v, uint64_t x) {
    uint64_t lo = 0, hi = n_v;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// doc_byte_off[b] <- the bytes that tokens [0, doc_tok_off[b]) decode to, for the n_b ascending boundaries
// doc_tok_off[b] <= n.  The wave of span s owns the boundaries in [s * kSpan, (s + 1) * kSpan); the last span's also
// owns those at n itself, which lie in a span that no wave walks when n is a multiple of kSpan (n - base <= kSpan:
// they read s_off[kSpan], the span's total).  span_off as for k_dec_write.
template <int F>
__global__ __launch_bounds__(kSpanThreads) void k_dec_bounds(const void *__restrict__ tok, uint64_t n, uint32_t barrier,
                                                             DecTab tab, const unsigned long long *__restrict__ span_off,
                                                             const unsigned long long *__restrict__ doc_tok_off,
                                                             uint64_t n_b, unsigned long long *__restrict__ doc_byte_off) {
    __shared__ uint32_t s_off[kSpanWaves][kSpan + 1];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint64_t span = span_index();
    const uint64_t base = span * kSpan;
    uint64_t lo = 0, hi = 0;
    if (base < n) {
        const uint64_t end = base + kSpan >= n ? n + 1 : base + kSpan;
        lo = dec_lower_bound(doc_tok_off, n_b, base);
        hi = lo + dec_lower_bound(doc_tok_off + lo, n_b - lo, end);
    }
    const bool active = lo < hi;                     // a span without a boundary reads no token
    if (active) dec_span_prefix<F, false>(tok, n, barrier, tab, base, lane, s_off[w], nullptr);
    __syncthreads();
    if (!active) return;
    const unsigned long long o = span_off[span];
    for (uint64_t b = lo + lane; b < hi; b += kWave) doc_byte_off[b] = o + s_off[w][doc_tok_off[b] - base];
}

#define DCHK(expr) MBPE_HIP_CHECK(expr, false)

}  // namespace

struct mbpe_decoder : DevQueue {
    mbpe_decoder() : DevQueue(false) {}
    float last_ms = 0.f;
    // the tables
    DevBuf<uint32_t> d_len, d_spk, d_spe;
    DevBuf<unsigned long long> d_off;
    DevBuf<uint8_t> d_blob;
    DecTab tab = {};
    // scratch, grown on demand and kept
    DevBuf<unsigned long long> d_span;        // span totals, then offsets
    DevBuf<unsigned long long> d_res;         // [0] decoded length, [1] ids that decoded to nothing
    DevBuf<void> d_tok;                       // staging for tokens that come from the host
    DevBuf<uint8_t> d_out;                    // staging for output that goes to the host
    DevBuf<unsigned long long> d_doc_tok;     // a batch's document boundaries: token offsets in,
    DevBuf<unsigned long long> d_doc_byte;    // byte offsets out
};

namespace {

// the runtime format -> the kernels' template argument: f(std::integral_constant<int, F>())
template <typename Fn>
void with_format(int fmt, Fn f) {
    switch (fmt) {
        case kFmtU32: f(std::integral_constant<int, kFmtU32>()); break;
        case kFmtU32End: f(std::integral_constant<int, kFmtU32End>()); break;
        case kFmtU16: f(std::integral_constant<int, kFmtU16>()); break;
        case kFmtU16End: f(std::integral_constant<int, kFmtU16End>()); break;
        case kFmtU16Barrier: f(std::integral_constant<int, kFmtU16Barrier>()); break;
        default: f(std::integral_constant<int, kFmtU16Plain>()); break;
    }
}

template <int F>
void launch_bounds(mbpe_decoder *d, const void *tok, uint64_t n, uint32_t barrier, uint32_t grid, uint64_t n_b) {
    hipLaunchKernelGGL(k_dec_bounds<F>, dim3(grid), dim3(kSpanThreads), 0, d->stream, tok, n, barrier, d->tab, d->d_span,
                       d->d_doc_tok, n_b, d->d_doc_byte);
}

// the documents of a batch: n_b = n_docs + 1 boundaries, checked by mbpe_decode_batch; both arrays are host memory
struct DecDocs {
    const uint64_t *tok_off;
    uint64_t n_b;
    uint64_t *byte_off_out;
};

// lengths + scan of n device-resident tokens and, for a batch, its boundaries' byte offsets (left on the device:
// dec_write fetches them); ev0 is recorded in front
int dec_measure(mbpe_decoder *d, int fmt, const void *tok, uint64_t n, uint32_t barrier, const DecDocs *docs,
                uint64_t *total, uint64_t *invalid) {
    const uint64_t n_spans = span_count(n);
    const uint32_t grid = span_grid(n);
    int rc = d->d_span.reserve((n_spans + 1) * 8, d->mem);
    if (rc != MBPE_OK) return rc;
    if (docs && n) {
        rc = d->d_doc_tok.reserve(docs->n_b * 8, d->mem);
        if (rc == MBPE_OK) rc = d->d_doc_byte.reserve(docs->n_b * 8, d->mem);
        if (rc != MBPE_OK) return rc;
        DCHK(hipMemcpyAsync(d->d_doc_tok, docs->tok_off, docs->n_b * 8, hipMemcpyHostToDevice, d->stream));
    }
    DCHK(hipMemsetAsync(d->d_res, 0, 16, d->stream));
    DCHK(hipEventRecord(d->ev0, d->stream));
    if (n) {
        with_format(fmt, [&](auto f) {
            hipLaunchKernelGGL(k_dec_len<f()>, dim3(grid), dim3(kSpanThreads), 0, d->stream, tok, n, barrier, d->tab,
                               d->d_span, d->d_res + 1);
        });
        hipLaunchKernelGGL(k_dec_scan64, dim3(1), dim3(kScanThreads), 0, d->stream, d->d_span, n_spans, d->d_res);
        if (docs) {
            // (a batch arrives as plain ids only: mbpe_decode_batch)
            if (fmt == kFmtU32) launch_bounds<kFmtU32>(d, tok, n, barrier, grid, docs->n_b);
            else launch_bounds<kFmtU16Plain>(d, tok, n, barrier, grid, docs->n_b);
        }
    }
    unsigned long long res[2] = {0, 0};
    DCHK(hipMemcpyAsync(res, d->d_res, 16, hipMemcpyDeviceToHost, d->stream));
    DCHK(hipStreamSynchronize(d->stream));
    DCHK(hipGetLastError());
    *total = res[0];
    *invalid = res[1];
    return MBPE_OK;
}

// the copy, after dec_measure of the same tokens; records ev1, fetches a batch's byte offsets and waits
int dec_write(mbpe_decoder *d, int fmt, const void *tok, uint64_t n, uint32_t barrier, const DecDocs *docs,
              uint8_t *out_dev, bool wrote) {
    if (wrote && n) {
        const uint32_t grid = span_grid(n);
        with_format(fmt, [&](auto f) {
            hipLaunchKernelGGL(k_dec_write<f()>, dim3(grid), dim3(kSpanThreads), 0, d->stream, tok, n, barrier, d->tab,
                               d->d_span, out_dev);
        });
    }
    DCHK(hipEventRecord(d->ev1, d->stream));
    if (docs) {
        if (n) DCHK(hipMemcpyAsync(docs->byte_off_out, d->d_doc_byte, docs->n_b * 8, hipMemcpyDeviceToHost, d->stream));
        else memset(docs->byte_off_out, 0, docs->n_b * 8);      // no tokens: no kernel ran, every document is empty
    }
    return d->wait(&d->last_ms);
}

// tokens / slots in any layout -> bytes; the common body of the entry points (docs: a batch, or NULL)
int dec_run(mbpe_decoder *d, int fmt, const void *tokens, uint64_t n, int tokens_on_device, uint32_t barrier,
            const DecDocs *docs, uint8_t *bytes_out, uint64_t cap, int out_on_device, uint64_t *n_out,
            uint64_t *n_invalid_out) {
    *n_out = 0;
    if (n_invalid_out) *n_invalid_out = 0;
    if (n >> 40) return fail(MBPE_ERR_ARG, "more than 2^40 tokens");
    DCHK(hipSetDevice(d->device));
    const uint64_t tok_bytes = n * (fmt <= kFmtU32End ? 4 : 2);
    const void *tok = tokens;
    if (!tokens_on_device && n) {
        int rc = d->d_tok.reserve(tok_bytes, d->mem);
        if (rc != MBPE_OK) return rc;
        DCHK(hipMemcpyAsync(d->d_tok, tokens, tok_bytes, hipMemcpyHostToDevice, d->stream));
        tok = d->d_tok;
    }
    uint64_t total = 0, invalid = 0;
    int rc = dec_measure(d, fmt, tok, n, barrier, docs, &total, &invalid);
    if (rc != MBPE_OK) return rc;
    *n_out = total;
    if (n_invalid_out) *n_invalid_out = invalid;
    if (!bytes_out) return dec_write(d, fmt, tok, n, barrier, docs, nullptr, false);       // the size query
    if (cap < total) {
        rc = dec_write(d, fmt, tok, n, barrier, docs, nullptr, false);
        return rc != MBPE_OK ? rc : fail(MBPE_ERR_ARG, "bytes_out too small");
    }
    if (out_on_device) return dec_write(d, fmt, tok, n, barrier, docs, bytes_out, true);
    if (total) {
        rc = d->d_out.reserve(total, d->mem);
        if (rc != MBPE_OK) return rc;
    }
    rc = dec_write(d, fmt, tok, n, barrier, docs, d->d_out, total != 0);
    if (rc != MBPE_OK) return rc;
    if (total) {
        DCHK(hipMemcpyAsync(bytes_out, d->d_out, total, hipMemcpyDeviceToHost, d->stream));
        DCHK(hipStreamSynchronize(d->stream));
    }
    return MBPE_OK;
}

int slot_format(uint32_t slot_bits, uint32_t end_bit, uint32_t barrier, int *fmt) {
    if (slot_bits == 32 && barrier == MBPE_NO_BARRIER && (end_bit == 0 || end_bit == kTokEnd)) {
        *fmt = end_bit ? kFmtU32End : kFmtU32;
        return MBPE_OK;
    }
    if (slot_bits == 16 && barrier == MBPE_NO_BARRIER && (end_bit == 0 || end_bit == 0x8000u)) {
        *fmt = end_bit ? kFmtU16End : kFmtU16;
        return MBPE_OK;
    }
    if (slot_bits == 16 && barrier < 0xFFFFu && end_bit == 0) {
        *fmt = kFmtU16Barrier;
        return MBPE_OK;
    }
    return fail(MBPE_ERR_ARG, "no such slot layout (see mbpe_stream_device)");
}

}  // namespace

namespace mbpe_host {

int check_doc_tok_off(const uint64_t *doc_tok_off, uint64_t n_docs, uint64_t n_tokens) {
    if (doc_tok_off[0] != 0) return fail(MBPE_ERR_ARG, "doc_tok_off must begin at 0");
    for (uint64_t i = 0; i < n_docs; ++i)
        if (doc_tok_off[i + 1] < doc_tok_off[i]) return fail(MBPE_ERR_ARG, "doc_tok_off must be ascending");
    if (doc_tok_off[n_docs] != n_tokens) return fail(MBPE_ERR_ARG, "doc_tok_off must end at n_tokens");
    return MBPE_OK;
}

int decode_to_string(mbpe_decoder *d, const uint32_t *tokens, uint64_t n, std::string *out, uint64_t *n_invalid) {
    out->clear();
    *n_invalid = 0;
    if (!d || (!tokens && n)) return fail(MBPE_ERR_ARG, "decode_to_string: NULL argument");
    DCHK(hipSetDevice(d->device));
    if (n) {
        int rc = d->d_tok.reserve(n * 4, d->mem);
        if (rc != MBPE_OK) return rc;
        DCHK(hipMemcpyAsync(d->d_tok, tokens, n * 4, hipMemcpyHostToDevice, d->stream));
    }
    uint64_t total = 0;
    int rc = dec_measure(d, kFmtU32, d->d_tok, n, MBPE_NO_BARRIER, nullptr, &total, n_invalid);
    if (rc != MBPE_OK) return rc;
    if (total) {
        rc = d->d_out.reserve(total, d->mem);
        if (rc != MBPE_OK) return rc;
    }
    rc = dec_write(d, kFmtU32, d->d_tok, n, MBPE_NO_BARRIER, nullptr, d->d_out, total != 0);
    if (rc != MBPE_OK) return rc;
    if (total) {
        out->resize(total);
        DCHK(hipMemcpyAsync(&(*out)[0], d->d_out, total, hipMemcpyDeviceToHost, d->stream));
        DCHK(hipStreamSynchronize(d->stream));
    }
    return MBPE_OK;
}

}  // namespace mbpe_host

extern "C" {

int mbpe_decoder_create(int device_id, const uint32_t *merges, uint32_t n_merges, const uint32_t *special_ids,
                        const uint8_t *special_bytes, const uint64_t *special_off, uint32_t n_special,
                        mbpe_decoder **out) {
    if (!out || (!merges && n_merges) || (n_special && (!special_ids || !special_off)))
        return fail(MBPE_ERR_ARG, "mbpe_decoder_create: NULL argument");
    *out = nullptr;
    if (n_merges > MBPE_MAX_VOCAB_WIDE - 256) return fail(MBPE_ERR_ARG, "n_merges beyond MBPE_MAX_VOCAB_WIDE - 256");
    for (uint32_t k = 0; k < n_special; ++k)
        if (special_off[k + 1] < special_off[k]) return fail(MBPE_ERR_ARG, "special_off must be ascending");
    if (n_special && special_off[n_special] > special_off[0] && !special_bytes)
        return fail(MBPE_ERR_ARG, "mbpe_decoder_create: NULL argument");

    // host side: lengths first (they can double with every merge), then the blob
    const uint32_t V = 256 + n_merges;
    std::vector<uint32_t> len(V);
    std::vector<unsigned long long> off(V);
    unsigned long long blob_size = 0;
    for (uint32_t id = 0; id < V; ++id) {
        unsigned long long l = 1;
        if (id >= 256) {
            // a side that names an id not yet defined contributes nothing (Tokenizer::rebuild_vocab)
            const uint32_t a = merges[2 * (id - 256)], b = merges[2 * (id - 256) + 1];
            l = (a < id ? len[a] : 0ull) + (b < id ? len[b] : 0ull);
        }
        if (l > MBPE_DECODER_MAX_ENTRY) return fail(MBPE_ERR_OOM, "a vocabulary entry exceeds MBPE_DECODER_MAX_ENTRY");
        len[id] = (uint32_t)l;
        off[id] = blob_size;
        blob_size += l;
        if (blob_size > MBPE_DECODER_MAX_BLOB) return fail(MBPE_ERR_OOM, "the vocabulary's bytes exceed MBPE_DECODER_MAX_BLOB");
    }
    // specials: the last one given for an id holds (special_tokens_reverse_lookup[id] = name)
    std::vector<uint32_t> sp_of(n_special, 0);      // 1: special k is the one that holds for its id
    uint32_t n_ext = 0;
    {
        std::vector<std::pair<uint32_t, uint32_t>> byid(n_special);
        for (uint32_t k = 0; k < n_special; ++k) byid[k] = {special_ids[k], k};
        std::sort(byid.begin(), byid.end());
        for (uint32_t k = 0; k < n_special; ++k)
            if (k + 1 == n_special || byid[k + 1].first != byid[k].first) sp_of[byid[k].second] = 1;
    }
    for (uint32_t k = 0; k < n_special; ++k) {
        if (!sp_of[k]) continue;
        const unsigned long long l = special_off[k + 1] - special_off[k];
        if (l > MBPE_DECODER_MAX_ENTRY) return fail(MBPE_ERR_OOM, "a special token exceeds MBPE_DECODER_MAX_ENTRY");
        blob_size += l;
        if (blob_size > MBPE_DECODER_MAX_BLOB) return fail(MBPE_ERR_OOM, "the vocabulary's bytes exceed MBPE_DECODER_MAX_BLOB");
        if (special_ids[k] >= V) ++n_ext;
    }
    std::vector<uint8_t> blob;
    try {
        blob.resize(blob_size + kBlobPad);
        len.reserve((size_t)V + n_ext);
        off.reserve((size_t)V + n_ext);
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_decoder_create: host allocation failed");
    }
    for (uint32_t id = 0; id < 256; ++id) blob[off[id]] = (uint8_t)id;
    for (uint32_t id = 256; id < V; ++id) {
        const uint32_t a = merges[2 * (id - 256)], b = merges[2 * (id - 256) + 1];
        uint8_t *dst = blob.data() + off[id];
        if (a < id) { memcpy(dst, blob.data() + off[a], len[a]); dst += len[a]; }
        if (b < id) memcpy(dst, blob.data() + off[b], len[b]);
    }
    uint32_t sp_bits = 2;
    while ((1u << sp_bits) < 2 * n_ext + 2) ++sp_bits;
    const uint32_t sp_cap = 1u << sp_bits;
    std::vector<uint32_t> spk(sp_cap, 0), spe(sp_cap, kNone);
    unsigned long long at = off[V - 1] + len[V - 1];      // the specials' bytes follow the vocabulary's
    for (uint32_t k = 0; k < n_special; ++k) {
        if (!sp_of[k]) continue;
        const uint32_t l = (uint32_t)(special_off[k + 1] - special_off[k]), id = special_ids[k];
        if (l) memcpy(blob.data() + at, special_bytes + special_off[k], l);
        if (id < V) {                               // overrides the vocabulary entry: the reverse lookup is asked first
            len[id] = l;
            off[id] = at;
        } else {
            uint32_t h = dec_hash(id, 32 - sp_bits);
            while (spe[h] != kNone) h = (h + 1) & (sp_cap - 1);
            spk[h] = id;
            spe[h] = (uint32_t)len.size();
            len.push_back(l);
            off.push_back(at);
        }
        at += l;
    }

    if (find_device(device_id) != MBPE_OK) return MBPE_ERR_NO_DEVICE;
    mbpe_decoder *d = new mbpe_decoder;
    auto build = [&]() -> int {
        int rc = d->open(device_id);
        if (rc == MBPE_OK) rc = d->d_len.reserve(len.size() * 4, d->mem);
        if (rc == MBPE_OK) rc = d->d_off.reserve(off.size() * 8, d->mem);
        if (rc == MBPE_OK) rc = d->d_blob.reserve(blob.size(), d->mem);
        if (rc == MBPE_OK) rc = d->d_spk.reserve((size_t)sp_cap * 4, d->mem);
        if (rc == MBPE_OK) rc = d->d_spe.reserve((size_t)sp_cap * 4, d->mem);
        if (rc == MBPE_OK) rc = d->d_res.reserve(16, d->mem);
        if (rc != MBPE_OK) return rc;
        DCHK(hipMemcpyAsync(d->d_len, len.data(), len.size() * 4, hipMemcpyHostToDevice, d->stream));
        DCHK(hipMemcpyAsync(d->d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, d->stream));
        DCHK(hipMemcpyAsync(d->d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice, d->stream));
        DCHK(hipMemcpyAsync(d->d_spk, spk.data(), (size_t)sp_cap * 4, hipMemcpyHostToDevice, d->stream));
        DCHK(hipMemcpyAsync(d->d_spe, spe.data(), (size_t)sp_cap * 4, hipMemcpyHostToDevice, d->stream));
        DCHK(hipStreamSynchronize(d->stream));
        return MBPE_OK;
    };
    const int rc = build();
    if (rc != MBPE_OK) {
        const std::string keep = mbpe_host::last_error();
        mbpe_decoder_destroy(d);
        mbpe_host::set_last_error(keep);
        return rc;
    }
    d->tab = {d->d_len, d->d_off, d->d_blob, d->d_spk, d->d_spe, V, sp_cap - 1, 32 - sp_bits, n_ext};
    *out = d;
    return MBPE_OK;
}

void mbpe_decoder_destroy(mbpe_decoder *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    delete d;                                 // the buffers, then the events, then the stream
}

int mbpe_decode_tokens(mbpe_decoder *d, const uint32_t *tokens, uint64_t n_tokens, int tokens_on_device,
                       uint8_t *bytes_out, uint64_t cap, int out_on_device, uint64_t *n_out, uint64_t *n_invalid_out) {
    if (!d || !n_out || (!tokens && n_tokens)) return fail(MBPE_ERR_ARG, "mbpe_decode_tokens: NULL argument");
    return dec_run(d, kFmtU32, tokens, n_tokens, tokens_on_device, MBPE_NO_BARRIER, nullptr, bytes_out, cap,
                   out_on_device, n_out, n_invalid_out);
}

int mbpe_decode_batch(mbpe_decoder *d, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                      const uint64_t *doc_tok_off, uint64_t n_docs, uint8_t *bytes_out, uint64_t cap, int out_on_device,
                      uint64_t *doc_byte_off_out, uint64_t *n_out, uint64_t *n_invalid_out) {
    if (n_out) *n_out = 0;
    if (!d || !n_out || !doc_tok_off || !doc_byte_off_out || (!tokens && n_tokens))
        return fail(MBPE_ERR_ARG, "mbpe_decode_batch: NULL argument");
    if (token_bits != 32 && token_bits != 16) return fail(MBPE_ERR_ARG, "token_bits must be 32 or 16");
    const int rc = mbpe_host::check_doc_tok_off(doc_tok_off, n_docs, n_tokens);
    if (rc != MBPE_OK) return rc;
    const DecDocs docs = {doc_tok_off, n_docs + 1, doc_byte_off_out};
    return dec_run(d, token_bits == 32 ? kFmtU32 : kFmtU16Plain, tokens, n_tokens, tokens_on_device, MBPE_NO_BARRIER,
                   &docs, bytes_out, cap, out_on_device, n_out, n_invalid_out);
}

int mbpe_decode_slots(mbpe_decoder *d, const void *slots, uint64_t n_slots, uint32_t slot_bits, uint32_t end_bit,
                      uint32_t barrier, uint8_t *bytes_out, uint64_t cap, int out_on_device, uint64_t *n_out,
                      uint64_t *n_invalid_out) {
    if (!d || !n_out || (!slots && n_slots)) return fail(MBPE_ERR_ARG, "mbpe_decode_slots: NULL argument");
    int fmt = 0;
    const int rc = slot_format(slot_bits, end_bit, barrier, &fmt);
    if (rc != MBPE_OK) return rc;
    return dec_run(d, fmt, slots, n_slots, 1, barrier, nullptr, bytes_out, cap, out_on_device, n_out, n_invalid_out);
}

int mbpe_decoder_kernel_ms(const mbpe_decoder *d, float *ms_out) {
    if (!d || !ms_out) return fail(MBPE_ERR_ARG, "mbpe_decoder_kernel_ms: NULL argument");
    *ms_out = d->last_ms;
    return MBPE_OK;
}

int mbpe_decoder_alloc_count(const mbpe_decoder *d, uint64_t *n_out) {
    if (!d || !n_out) return fail(MBPE_ERR_ARG, "mbpe_decoder_alloc_count: NULL argument");
    *n_out = d->mem.n_allocs;
    return MBPE_OK;
}

int mbpe_decode_stream(mbpe_ctx *ctx, uint8_t *bytes_out, uint64_t cap, int out_on_device, uint64_t *n_out) {
    if (!ctx || !n_out) return fail(MBPE_ERR_ARG, "mbpe_decode_stream: NULL argument");
    *n_out = 0;
    const void *slots = nullptr;
    uint64_t n_slots = 0;
    uint32_t bits = 0, end_bit = 0, barrier = MBPE_NO_BARRIER, n_merges = 0;
    int rc = mbpe_stream_device(ctx, &slots, &n_slots, &bits, &end_bit, &barrier);
    if (rc != MBPE_OK) return rc;
    rc = mbpe_train_result(ctx, nullptr, nullptr, 0, &n_merges);
    if (rc != MBPE_OK) return rc;
    std::vector<uint32_t> merges(2 * (size_t)n_merges + 2);
    rc = mbpe_train_result(ctx, merges.data(), nullptr, n_merges, &n_merges);
    if (rc != MBPE_OK) return rc;
    mbpe_decoder *d = nullptr;
    rc = mbpe_decoder_create(mbpe_host::ctx_device(ctx), merges.data(), n_merges, nullptr, nullptr, nullptr, 0, &d);
    if (rc != MBPE_OK) return rc;
    rc = mbpe_decode_slots(d, slots, n_slots, bits, end_bit, barrier, bytes_out, cap, out_on_device, n_out, nullptr);
    const std::string keep = rc == MBPE_OK ? std::string() : std::string(mbpe_host::last_error());
    mbpe_decoder_destroy(d);
    if (rc != MBPE_OK) mbpe_host::set_last_error(keep);
    return rc;
}

}  // extern "C"
