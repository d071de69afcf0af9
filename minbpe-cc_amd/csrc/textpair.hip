// Text pairs on the device: (tokens, doc_off of 2 n documents) -> (joined tokens, targets, doc_off' of n documents),
// between encode and pack.  The rule is textpair.h's; this file runs it.
//
//   k_textpair_plan     one lane per pair, one wave per span of 1,024 pairs: three offsets in, (a, b) and the joined
//                       length out, the span's sum of lengths
//   k_textpair_scan     one workgroup: span.h's 64-bit scan over the spans' sums; the total -- the joined token count --
//                       goes to off[n]
//   k_textpair_offsets  the spans again: a wave prefix sum turns the lengths into the exclusive prefix sum, in place
//   k_textpair_gather   ids and targets in one pass.  OUTPUT-centric: the joined stream is cut at the 16-byte boundaries
//                       of its global address, a lane owns one such piece (8 ids of 16 bits or 4 of 32) and a wave 16
//                       rounds of 64 neighbouring pieces, so its loads and stores are contiguous.  A lane keeps the pair
//                       it stands in from round to round: its next piece lies 1,024 bytes further, and tp_seek walks up
//                       to four pairs forward from there before it falls back to a binary search over the pairs ahead.
//                       In its first round a lane stands at pair 0, so that round is the one full search per lane and
//                       wave-span; with pairs of some 64 ids (32-bit tokens) or 128 (16-bit) and more the later
//                       rounds are walks, with shorter pairs every round ends in the (shortened) binary search.
//                       A joined pair is two source runs and up to three constants.  Per piece the lane decides whether
//                       all of it lies inside ONE run: then it is a plain copy, one dwordx4 load where source and
//                       destination are mutually aligned, else loads of the token's width.  Any other piece -- it holds
//                       a separator, an end id or a pair boundary -- goes id by id through tp_id_at.
//                       A target is the id one position on.  Inside a piece that id is in the lane's registers already;
//                       the id behind the piece's last comes from the next lane's registers by a shuffle, and only lane
//                       63, whose neighbour is another wave, fetches it.  So every source token is read once.
//                       The piece of ids and the piece (two with 16-bit tokens) of targets are stored as dwordx4; only
//                       the first and last piece of the stream can be partial, and a target address off 16 bytes (an
//                       output pointer that is) goes word by word.
// Every index is 64-bit.  No atomics; nothing is waited for in textpair_launch.
//
// Bytes moved per joined id: read once (2 or 4 B), written once (2 or 4 B), target written once (4 B); per pair 24 B of
// offsets read and 24 B of plan written by the plan, 8 B rewritten by the offsets; per pair entered by a lane 48 B.
#include "textpair.h"

#include "hip_host.h"

#include <algorithm>
#include <new>
#include <string>
#include <vector>

namespace {

using namespace mbpe;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kSpanThreads) void k_textpair_plan(const unsigned long long *__restrict__ doc_off, uint64_t n_pairs,
                                                                 mbpe_textpair_spec spec, unsigned long long *__restrict__ off,
                                                                 unsigned long long *__restrict__ kept,
                                                                 unsigned long long *__restrict__ span_cnt) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n_pairs) return;
    const uint32_t lane = lane_id();
    unsigned long long s = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        if (i < n_pairs) {
            const unsigned long long o0 = doc_off[2 * i], o1 = doc_off[2 * i + 1], o2 = doc_off[2 * i + 2];
            const TpKeep k = textpair_keep(spec, o1 - o0, o2 - o1);
            const unsigned long long n = textpair_len(spec, k);
            kept[2 * i] = k.a;
            kept[2 * i + 1] = k.b;
            off[i] = n;
            s += n;
        }
    }
    for (int k = kWave / 2; k > 0; k >>= 1) s += __shfl_down(s, k, kWave);
    if (lane == 0) span_cnt[span] = s;
}

__global__ __launch_bounds__(kScanThreads) void k_textpair_scan(unsigned long long *__restrict__ span_cnt, uint64_t n_spans,
                                                                 unsigned long long *__restrict__ total) {
    __shared__ unsigned long long sh[kScanThreads];
    const unsigned long long sum = span_scan_sum64(span_cnt, n_spans, sh);
    if (threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(kSpanThreads) void k_textpair_offsets(unsigned long long *__restrict__ off, uint64_t n_pairs,
                                                                    const unsigned long long *__restrict__ span_off) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n_pairs) return;
    const uint32_t lane = lane_id();
    unsigned long long o = span_off[span];
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        const unsigned long long w = i < n_pairs ? off[i] : 0ull;
        const unsigned long long incl = wave_prefix64(w, lane);
        if (i < n_pairs) off[i] = o + incl - w;
        o += __shfl(incl, kWave - 1, kWave);
    }
}

struct TpJob {
    const void *tok;
    const unsigned long long *doc_off;       // the 2 n + 1 offsets of A and B
    const unsigned long long *off;           // the n + 1 joined ones; off[n] = ids of the output
    const unsigned long long *kept;
    uint64_t n_pairs;
    void *out;
    uint32_t *tgt;                           // NULL: no targets
    uint64_t cap;                            // ids the outputs hold
    mbpe_textpair_spec spec;
};

// the pair the walk stands in: n joined ids, a of A' from token sa on, b of B' from sb on
struct TpAt {
    unsigned long long n, a, b, sa, sb;
};

__device__ __forceinline__ void tp_enter(const TpJob &j, uint64_t d, TpAt *w) {
    w->n = j.off[d + 1] - j.off[d];
    w->a = j.kept[2 * d];
    w->b = j.kept[2 * d + 1];
    // (a side that keeps its tail ends where the document ends)
    w->sa = j.spec.keep_tail_a ? j.doc_off[2 * d + 1] - w->a : j.doc_off[2 * d];
    w->sb = j.spec.keep_tail_b ? j.doc_off[2 * d + 2] - w->b : j.doc_off[2 * d + 1];
}

template <int BITS>
__device__ __forceinline__ uint32_t tp_tok(const void *__restrict__ tok, unsigned long long i) {
    return BITS == 16 ? (uint32_t) static_cast<const uint16_t *>(tok)[i] : static_cast<const uint32_t *>(tok)[i] & kTokIdMask;
}

// the id at position k < w.n of the joined pair
template <int BITS>
__device__ __forceinline__ uint32_t tp_id_at(const TpJob &j, const TpAt &w, unsigned long long k) {
    if (k < w.a) return tp_tok<BITS>(j.tok, w.sa + k);
    k -= w.a;
    if (k < j.spec.n_sep) return k == 0 ? j.spec.sep_id[0] : j.spec.sep_id[1];
    k -= j.spec.n_sep;
    return k < w.b ? tp_tok<BITS>(j.tok, w.sb + k) : j.spec.end_id;
}

// the pair that holds joined position f < off[n_pairs], from pair d <= it on: the largest pair with off <= f that has
// ids (empty pairs share their successor's offset and are passed over)
__device__ __forceinline__ uint64_t tp_seek(const TpJob &j, uint64_t d, unsigned long long f) {
    for (int step = 0; step < 4; ++step) {
        if (j.off[d + 1] > f) return d;
        ++d;
    }
    uint64_t hi = j.n_pairs;                                     // off[d] <= f < off[hi]
    while (hi - d > 1) {
        const uint64_t m = d + (hi - d) / 2;
        if (j.off[m] <= f) d = m;
        else hi = m;
    }
    return d;
}

template <int BITS>
__global__ __launch_bounds__(kSpanThreads) void k_textpair_gather(TpJob j) {
    constexpr uint32_t ob = BITS / 8, PER = 128 / BITS;
    const unsigned long long total = j.off[j.n_pairs];
    const uint64_t n_out = total < j.cap ? total : j.cap;        // (they are equal or the buffers are larger)
    const uint64_t A = (uint64_t)(uintptr_t)j.out, E = A + n_out * ob, B0 = A & ~15ull;
    const uint64_t n_pieces = (E - B0 + 15) >> 4;
    const uint64_t p0 = span_index() * kSpan;                    // a wave's span: 1,024 pieces in 16 rounds
    if (p0 >= n_pieces) return;
    uint8_t *base = static_cast<uint8_t *>(j.out);
    const uint32_t lane = lane_id();
    uint64_t d = 0;
    for (int it = 0; it < kSpanIters; ++it) {                    // (every lane runs every round: the shuffle below)
        const uint64_t p = p0 + (uint64_t)it * kWave + lane;
        const uint64_t B = B0 + (p << 4);
        const uint64_t lo = B > A ? B : A;
        const uint64_t hi = B + 16 < E ? B + 16 : E;
        const uint32_t cnt = p < n_pieces && hi > lo ? (uint32_t)(hi - lo) / ob : 0u;
        const uint64_t f = (lo - A) / ob;
        uint32_t id[PER];
        uint32_t want = 0;                                       // bit e: position f + e predicts the id behind it
        TpAt w = {0, 0, 0, 0, 0};
        unsigned long long k = 0;                                // where the walk stands behind the piece, in pair d
#pragma unroll
        for (uint32_t e = 0; e < PER; ++e) id[e] = 0u;
        if (cnt) {
            d = tp_seek(j, d, f);
            tp_enter(j, d, &w);
            k = f - j.off[d];
            const unsigned long long b0 = w.a + j.spec.n_sep;    // where B' begins
            const bool in_a = k + cnt <= w.a, in_b = k >= b0 && k + cnt <= b0 + w.b;
            if (in_a || in_b) {                                  // a copy out of one run
                const unsigned long long s = in_a ? w.sa + k : w.sb + (k - b0);
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
                        if (e < cnt) id[e] = tp_tok<BITS>(j.tok, s + e);
                }
#pragma unroll
                for (uint32_t e = 0; e < PER; ++e)
                    if (e < cnt && textpair_predicts(j.spec, w.a, w.n, k + e)) want |= 1u << e;
                k += cnt;
            } else {                                             // constants or a pair boundary inside: id by id
#pragma unroll
                for (uint32_t e = 0; e < PER; ++e) {
                    if (e < cnt) {
                        while (k >= w.n) {                       // ends: f + e < n_out, a pair with ids follows
                            ++d;
                            k = 0;
                            tp_enter(j, d, &w);
                        }
                        id[e] = tp_id_at<BITS>(j, w, k);
                        if (textpair_predicts(j.spec, w.a, w.n, k)) want |= 1u << e;
                        ++k;
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
        uint32_t behind = __shfl_down(id[0], 1, kWave);          // the next piece's first id
        const bool last_wants = cnt && (want >> (cnt - 1) & 1u);
        if (last_wants && lane == kWave - 1) behind = tp_id_at<BITS>(j, w, k);   // (k < w.n: the position predicts)
        uint32_t t[PER];
#pragma unroll
        for (uint32_t e = 0; e < PER; ++e) {
            const uint32_t nx = e + 1 < PER && e + 1 < cnt ? id[(e + 1) % PER] : behind;
            t[e] = want >> e & 1u ? nx : kTokNone;
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

// device time of the calling thread's latest mbpe_textpair_tokens (mbpe_textpair_kernel_ms)
thread_local float g_textpair_ms = 0.f;

int textpair_run(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                 const uint64_t *doc_tok_off, uint64_t n_pairs, const mbpe_textpair_spec &spec, void *tokens_out,
                 uint32_t *targets_out, uint64_t n_new, int out_on_device) {
    int rc = find_device(device_id);
    if (rc != MBPE_OK) return rc;
    OneShot dev;
    rc = dev.open(device_id);
    if (rc != MBPE_OK) return rc;
    const uint64_t tb = token_bits / 8;
    void *d_tok = const_cast<void *>(tokens), *d_off = nullptr, *d_out = tokens_out, *d_tgt = targets_out, *d_new = nullptr,
         *d_kept = nullptr;
    if (!tokens_on_device) rc = dev.alloc(&d_tok, n_tokens * tb, tokens);
    if (rc == MBPE_OK) rc = dev.alloc(&d_off, (2 * n_pairs + 1) * 8, doc_tok_off);
    if (rc == MBPE_OK && !out_on_device) rc = dev.alloc(&d_out, n_new * tb, nullptr);
    if (rc == MBPE_OK && !out_on_device && targets_out) rc = dev.alloc(&d_tgt, n_new * 4, nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_new, textpair_off_bytes(n_pairs), nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_kept, n_pairs * 16, nullptr);
    if (rc != MBPE_OK) return rc;
    const TextpairDst dst = {d_out, static_cast<uint32_t *>(d_tgt), n_new, static_cast<unsigned long long *>(d_new),
                             static_cast<unsigned long long *>(d_kept)};
    TCHK(hipEventRecord(dev.ev0, dev.stream));
    textpair_launch(dev.stream, d_tok, token_bits, static_cast<const unsigned long long *>(d_off), n_pairs, spec, dst);
    rc = dev.finish(&g_textpair_ms);
    if (rc != MBPE_OK) return rc;
    if (!out_on_device) {
        TCHK(hipMemcpyAsync(tokens_out, d_out, n_new * tb, hipMemcpyDeviceToHost, dev.stream));
        if (targets_out) TCHK(hipMemcpyAsync(targets_out, d_tgt, n_new * 4, hipMemcpyDeviceToHost, dev.stream));
        TCHK(hipStreamSynchronize(dev.stream));
    }
    return MBPE_OK;
}

// what mbpe_textpair_plan and mbpe_textpair_tokens check alike, then the host's plan into off_out (n_docs / 2 + 1)
int textpair_host_plan(const std::string &who, const uint64_t *doc_tok_off, uint64_t n_docs, uint64_t n_tokens,
                       const mbpe_textpair_spec *spec, uint32_t token_bits, uint64_t *off_out, uint64_t *kept_out) {
    const char *msg = "";
    int rc = textpair_check_spec(spec, token_bits, &msg);
    if (rc != MBPE_OK) return fail(rc, who + ": " + msg);
    if (n_docs & 1) return fail(MBPE_ERR_ARG, who + ": an odd document count: documents 2i and 2i + 1 are a pair");
    rc = mbpe_host::check_doc_tok_off(doc_tok_off, n_docs, n_tokens);
    if (rc != MBPE_OK) return rc;
    if (n_tokens >> 40 || n_docs >> 40) return fail(MBPE_ERR_ARG, who + ": more than 2^40 tokens or documents");
    textpair_plan_host(doc_tok_off, n_docs, *spec, off_out, kept_out);
    return MBPE_OK;
}

}  // namespace

namespace mbpe {

uint64_t textpair_off_bytes(uint64_t n_pairs) { return (n_pairs + 1 + span_count(n_pairs)) * 8; }

void textpair_launch(hipStream_t stream, const void *tok, uint32_t bits, const unsigned long long *doc_off, uint64_t n_pairs,
                     const mbpe_textpair_spec &spec, const TextpairDst &dst) {
    unsigned long long *span_cnt = dst.off + n_pairs + 1;        // (textpair_off_bytes)
    const dim3 grid(span_grid(n_pairs)), block(kSpanThreads);
    hipLaunchKernelGGL(k_textpair_plan, grid, block, 0, stream, doc_off, n_pairs, spec, dst.off, dst.kept, span_cnt);
    hipLaunchKernelGGL(k_textpair_scan, dim3(1), dim3(kScanThreads), 0, stream, span_cnt, span_count(n_pairs),
                       dst.off + n_pairs);
    hipLaunchKernelGGL(k_textpair_offsets, grid, block, 0, stream, dst.off, n_pairs, span_cnt);
    if (dst.cap == 0) return;
    const TpJob j = {tok, doc_off, dst.off, dst.kept, n_pairs, dst.tok, dst.tgt, dst.cap, spec};
    const uint64_t A = (uint64_t)(uintptr_t)dst.tok, E = A + dst.cap * (bits / 8);
    const uint64_t n_pieces = (E - (A & ~15ull) + 15) >> 4;      // (no fewer than the kernel finds: it stops at off[n])
    const dim3 ggrid(span_grid(n_pieces));
    if (bits == 16) hipLaunchKernelGGL((k_textpair_gather<16>), ggrid, block, 0, stream, j);
    else hipLaunchKernelGGL((k_textpair_gather<32>), ggrid, block, 0, stream, j);
}

}  // namespace mbpe

extern "C" {

int mbpe_textpair_plan(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_textpair_spec *spec,
                       uint64_t *doc_tok_off_out, uint64_t *kept_out) {
    if (!doc_tok_off || !spec || !doc_tok_off_out) return fail(MBPE_ERR_ARG, "mbpe_textpair_plan: NULL argument");
    return textpair_host_plan("mbpe_textpair_plan", doc_tok_off, n_docs, doc_tok_off[n_docs], spec, 32, doc_tok_off_out,
                              kept_out);
}

int mbpe_textpair_tokens(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                         const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_textpair_spec *spec, void *tokens_out,
                         uint32_t *targets_out, uint64_t cap, int out_on_device, uint64_t *doc_tok_off_out,
                         uint64_t *kept_out, uint64_t *n_out) {
    if (n_out) *n_out = 0;
    if (!n_out || !doc_tok_off || !spec || (!tokens && n_tokens))
        return fail(MBPE_ERR_ARG, "mbpe_textpair_tokens: NULL argument");
    if (token_bits != 16 && token_bits != 32)
        return fail(MBPE_ERR_ARG, "mbpe_textpair_tokens: token_bits must be 16 or 32");
    try {
        const uint64_t n_pairs = n_docs / 2;
        std::vector<uint64_t> off(n_pairs + 1, 0), kept(2 * n_pairs, 0);
        int rc = textpair_host_plan("mbpe_textpair_tokens", doc_tok_off, n_docs, n_tokens, spec, token_bits, off.data(),
                                    kept.data());
        if (rc != MBPE_OK) return rc;
        const uint64_t n_new = off[n_pairs];
        *n_out = n_new;
        if (tokens_out && cap < n_new) return fail(MBPE_ERR_ARG, "mbpe_textpair_tokens: tokens_out too small");
        if (tokens_out && out_on_device &&
            ((uint64_t)(uintptr_t)tokens_out % (token_bits / 8) || (uint64_t)(uintptr_t)targets_out % 4))
            return fail(MBPE_ERR_ARG, "mbpe_textpair_tokens: tokens_out or targets_out is not aligned to its elements");
        if (tokens_out && n_new) {
            rc = textpair_run(device_id, tokens, n_tokens, token_bits, tokens_on_device, doc_tok_off, n_pairs, *spec,
                              tokens_out, targets_out, n_new, out_on_device);
            if (rc != MBPE_OK) return rc;
        }
        if (doc_tok_off_out) std::copy(off.begin(), off.end(), doc_tok_off_out);
        if (kept_out) std::copy(kept.begin(), kept.end(), kept_out);
        return MBPE_OK;
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_textpair_tokens: host allocation failed");
    }
}

int mbpe_textpair_kernel_ms(float *ms_out) {
    if (!ms_out) return fail(MBPE_ERR_ARG, "mbpe_textpair_kernel_ms: NULL argument");
    *ms_out = g_textpair_ms;
    return MBPE_OK;
}

}  // extern "C"
