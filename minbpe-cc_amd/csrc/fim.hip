// Fill-in-the-middle on the device: (tokens, doc_off) -> (tokens', doc_off'), between encode and pack.  The rule is
// fim.h's; this file runs it.
//
//   k_fim_plan      one lane per document, one wave per span of 1,024 documents: the document's plan (mode, a, b) from
//                   its length and number, its new length L' into off[d], the span's sum; a document too long for the
//                   cuts leaves its number in the flag word (the smallest such number)
//   k_fim_scan      one workgroup: span.h's 64-bit scan over the spans' sums; the total -- the new token count -- goes
//                   to off[n_docs]
//   k_fim_offsets   the spans again: a wave prefix sum turns the lengths into the exclusive prefix sum, in place
//   k_fim_gather    the new stream.  OUTPUT-centric like pack.hip's k_pack_stream: the output is cut at the 16-byte
//                   boundaries of its global address and a lane owns one such piece, 8 ids of 16 bits or 4 of 32.  The
//                   first id of a piece finds its document by a binary search PER LANE over off (the 64 lanes of a
//                   wave search neighbouring positions, so their probes fall into the same few cache lines); the walk
//                   then steps over part and document ends (empty documents are passed over), reads the source tokens
//                   with loads of the token's own width -- a document's three runs start at any offset -- and stores
//                   the piece as one dwordx4.  Only the first and the last piece of the output can be partial; those
//                   are stored id by id.  The new token count is read from off[n_docs] on the device, so the host
//                   launches the four kernels back to back and waits once.
// Every index is 64-bit.
//
// Bytes moved per token: read once (2 or 4 B) and written once (2 or 4 B), as k_pack_stream moves them; per transformed
// document three ids more written; per document 16 B of old offsets read, 8 B of new offset written twice and read
// once, 17 B of plan written, and all of it (41 B) read again by the lanes that enter the document; per lane at most
// log2(n_docs) probes of 8 B that neighbouring lanes share.
#include "fim.h"

#include "hip_host.h"

#include <algorithm>
#include <new>
#include <string>
#include <vector>

namespace {

using namespace mbpe;

constexpr int kFimThreads = 256;
constexpr uint32_t kFimMaxGrid = 0x7FFFFFFFu;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kSpanThreads) void k_fim_plan(const unsigned long long *__restrict__ doc_off, uint64_t n_docs,
                                                            mbpe_fim_spec spec, unsigned long long *__restrict__ off,
                                                            unsigned long long *__restrict__ cut, uint8_t *__restrict__ mode,
                                                            unsigned long long *__restrict__ span_cnt,
                                                            unsigned long long *__restrict__ flag) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n_docs) return;
    const uint32_t lane = lane_id();
    unsigned long long s = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t d = base + (uint64_t)it * kWave + lane;
        if (d < n_docs) {
            const unsigned long long L = doc_off[d + 1] - doc_off[d];
            if (fim_too_long(spec, L)) atomicMin(flag, (unsigned long long)d);
            const FimPlan p = fim_plan_doc(spec, d, L);
            const unsigned long long n = fim_len(p.mode, L);
            mode[d] = (uint8_t)p.mode;
            cut[2 * d] = p.a;
            cut[2 * d + 1] = p.b;
            off[d] = n;
            s += n;
        }
    }
    for (int k = kWave / 2; k > 0; k >>= 1) s += __shfl_down(s, k, kWave);
    if (lane == 0) span_cnt[span] = s;
}

__global__ __launch_bounds__(kScanThreads) void k_fim_scan(unsigned long long *__restrict__ span_cnt, uint64_t n_spans,
                                                            unsigned long long *__restrict__ total) {
    __shared__ unsigned long long sh[kScanThreads];
    const unsigned long long sum = span_scan_sum64(span_cnt, n_spans, sh);
    if (threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(kSpanThreads) void k_fim_offsets(unsigned long long *__restrict__ off, uint64_t n_docs,
                                                               const unsigned long long *__restrict__ span_off) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n_docs) return;
    const uint32_t lane = lane_id();
    unsigned long long o = span_off[span];
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t d = base + (uint64_t)it * kWave + lane;
        const unsigned long long w = d < n_docs ? off[d] : 0ull;
        const unsigned long long incl = wave_prefix64(w, lane);
        if (d < n_docs) off[d] = o + incl - w;
        o += __shfl(incl, kWave - 1, kWave);
    }
}

struct FimJob {
    const void *tok;
    const unsigned long long *doc_off;       // the old offsets, n_docs + 1
    const unsigned long long *off;           // the new ones; off[n_docs] = ids of the output
    const unsigned long long *cut;
    const uint8_t *mode;
    uint64_t n_docs;
    void *out;
    uint64_t cap;                            // ids the output holds
    uint32_t pre, suf, mid;
};

// the document the walk stands in: its old tokens begin at s0 and are L, its new ids n
struct FimAt {
    FimPlan p;
    unsigned long long s0, L, n;
};

__device__ __forceinline__ void fim_enter(const FimJob &j, uint64_t d, FimAt *w) {
    w->s0 = j.doc_off[d];
    w->L = j.doc_off[d + 1] - w->s0;
    w->n = j.off[d + 1] - j.off[d];
    w->p.mode = j.mode[d];
    w->p.a = j.cut[2 * d];
    w->p.b = j.cut[2 * d + 1];
}

template <int BITS>
__global__ __launch_bounds__(kFimThreads) void k_fim_gather(FimJob j) {
    constexpr uint32_t ob = BITS / 8;
    const unsigned long long total = j.off[j.n_docs];
    const uint64_t n_out = total < j.cap ? total : j.cap;        // (they are equal or the buffer is larger)
    const uint64_t A = (uint64_t)(uintptr_t)j.out, E = A + n_out * ob, B0 = A & ~15ull;
    const uint64_t n_pieces = (E - B0 + 15) >> 4;
    uint8_t *base = static_cast<uint8_t *>(j.out);
    for (uint64_t p = (uint64_t)blockIdx.x * kFimThreads + threadIdx.x; p < n_pieces;
         p += (uint64_t)gridDim.x * kFimThreads) {
        const uint64_t B = B0 + (p << 4);
        const uint64_t lo = B > A ? B : A;
        const uint64_t hi = B + 16 < E ? B + 16 : E;
        if (hi <= lo) continue;                                  // (n_out == 0)
        const uint32_t cnt = (uint32_t)(hi - lo) / ob;
        const uint64_t f = (lo - A) / ob;
        // the document that holds position f < n_out: the largest d with off[d] <= f (empty documents share their
        // successor's offset and are passed over)
        uint64_t d = 0, hi_d = j.n_docs;
        while (hi_d - d > 1) {
            const uint64_t m = d + (hi_d - d) / 2;
            if (j.off[m] <= f) d = m;
            else hi_d = m;
        }
        FimAt w;
        fim_enter(j, d, &w);
        unsigned long long k = f - j.off[d];
        unsigned __int128 acc = 0;
        for (uint32_t e = 0; e < cnt; ++e) {
            while (k >= w.n) {                                   // ends: f + e < n_out, a document with ids follows
                ++d;
                k = 0;
                fim_enter(j, d, &w);
            }
            const unsigned long long src = fim_source(w.p, w.L, k);
            uint32_t v;
            if (src == kFimSrcPre) v = j.pre;
            else if (src == kFimSrcSuf) v = j.suf;
            else if (src == kFimSrcMid) v = j.mid;
            else if (BITS == 16) v = static_cast<const uint16_t *>(j.tok)[w.s0 + src];
            else v = static_cast<const uint32_t *>(j.tok)[w.s0 + src] & kTokIdMask;
            acc |= (unsigned __int128)v << (BITS * e);
            ++k;
        }
        if (cnt == 128 / BITS) {                                 // (then lo == B)
            u32x4 q;
            q.x = (uint32_t)acc;
            q.y = (uint32_t)(acc >> 32);
            q.z = (uint32_t)(acc >> 64);
            q.w = (uint32_t)(acc >> 96);
            *static_cast<u32x4 *>(__builtin_assume_aligned(base + (B - A), 16)) = q;
        } else {                                                 // the first or the last piece of the output
            if (BITS == 16) {
                uint16_t *dst = reinterpret_cast<uint16_t *>(base + (lo - A));
                for (uint32_t e = 0; e < cnt; ++e) dst[e] = (uint16_t)(acc >> (16 * e));
            } else {
                uint32_t *dst = reinterpret_cast<uint32_t *>(base + (lo - A));
                for (uint32_t e = 0; e < cnt; ++e) dst[e] = (uint32_t)(acc >> (32 * e));
            }
        }
    }
}

#define FCHK(expr) MBPE_HIP_CHECK(expr, true)

// device time of the calling thread's latest mbpe_fim_tokens (mbpe_fim_kernel_ms)
thread_local float g_fim_ms = 0.f;

int fim_run(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
            const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_fim_spec &spec, void *tokens_out, uint64_t n_new,
            int out_on_device) {
    int rc = find_device(device_id);
    if (rc != MBPE_OK) return rc;
    OneShot dev;
    rc = dev.open(device_id);
    if (rc != MBPE_OK) return rc;
    const uint64_t tb = token_bits / 8;
    void *d_tok = const_cast<void *>(tokens), *d_off = nullptr, *d_out = tokens_out, *d_new = nullptr, *d_cut = nullptr,
         *d_mode = nullptr;
    if (!tokens_on_device) rc = dev.alloc(&d_tok, n_tokens * tb, tokens);
    if (rc == MBPE_OK) rc = dev.alloc(&d_off, (n_docs + 1) * 8, doc_tok_off);
    if (rc == MBPE_OK && !out_on_device) rc = dev.alloc(&d_out, n_new * tb, nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_new, fim_off_bytes(n_docs), nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_cut, n_docs * 16, nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_mode, n_docs, nullptr);
    if (rc != MBPE_OK) return rc;
    const FimDst dst = {d_out, n_new, static_cast<unsigned long long *>(d_new), static_cast<unsigned long long *>(d_cut),
                        static_cast<uint8_t *>(d_mode)};
    FCHK(hipEventRecord(dev.ev0, dev.stream));
    fim_launch(dev.stream, d_tok, n_tokens, token_bits, static_cast<const unsigned long long *>(d_off), n_docs, spec, dst);
    rc = dev.finish(&g_fim_ms);
    if (rc != MBPE_OK) return rc;
    if (!out_on_device) {
        FCHK(hipMemcpyAsync(tokens_out, d_out, n_new * tb, hipMemcpyDeviceToHost, dev.stream));
        FCHK(hipStreamSynchronize(dev.stream));
    }
    return MBPE_OK;
}

// what mbpe_fim_plan and mbpe_fim_tokens check alike, then the host's plan into off_out (n_docs + 1)
int fim_host_plan(const std::string &who, const uint64_t *doc_tok_off, uint64_t n_docs, uint64_t n_tokens,
                  const mbpe_fim_spec *spec, uint32_t token_bits, uint64_t *off_out, uint8_t *mode_out, uint64_t *cut_out) {
    const char *msg = "";
    int rc = fim_check_spec(spec, token_bits, &msg);
    if (rc != MBPE_OK) return fail(rc, who + ": " + msg);
    rc = mbpe_host::check_doc_tok_off(doc_tok_off, n_docs, n_tokens);
    if (rc != MBPE_OK) return rc;
    if (n_tokens >> 40 || n_docs >> 40) return fail(MBPE_ERR_ARG, who + ": more than 2^40 tokens or documents");
    uint64_t bad = 0;
    for (uint64_t d = 0; d < n_docs; ++d)                        // (first, so that an error writes nothing)
        if (fim_too_long(*spec, doc_tok_off[d + 1] - doc_tok_off[d]))
            return fail(MBPE_ERR_ARG, who + ": document " + std::to_string(d) + " has 2^32 - 1 tokens or more");
    return fim_plan_host(doc_tok_off, n_docs, *spec, off_out, mode_out, cut_out, &bad);
}

}  // namespace

namespace mbpe {

uint64_t fim_off_bytes(uint64_t n_docs) { return (n_docs + 2 + span_count(n_docs)) * 8; }

void fim_launch(hipStream_t stream, const void *tok, uint64_t n_tokens, uint32_t bits, const unsigned long long *doc_off,
                uint64_t n_docs, const mbpe_fim_spec &spec, const FimDst &dst) {
    (void)n_tokens;
    unsigned long long *flag = dst.off + n_docs + 1, *span_cnt = flag + 1;   // (fim_off_bytes)
    (void)hipMemsetAsync(flag, 0xFF, 8, stream);
    const dim3 grid(span_grid(n_docs)), block(kSpanThreads);
    hipLaunchKernelGGL(k_fim_plan, grid, block, 0, stream, doc_off, n_docs, spec, dst.off, dst.cut, dst.mode, span_cnt, flag);
    hipLaunchKernelGGL(k_fim_scan, dim3(1), dim3(kScanThreads), 0, stream, span_cnt, span_count(n_docs), dst.off + n_docs);
    hipLaunchKernelGGL(k_fim_offsets, grid, block, 0, stream, dst.off, n_docs, span_cnt);
    if (dst.cap == 0) return;
    const FimJob j = {tok, doc_off, dst.off, dst.cut, dst.mode, n_docs, dst.tok, dst.cap, spec.pre_id, spec.suf_id, spec.mid_id};
    const uint64_t A = (uint64_t)(uintptr_t)dst.tok, E = A + dst.cap * (bits / 8);
    const uint64_t n_pieces = (E - (A & ~15ull) + 15) >> 4;
    const dim3 ggrid((uint32_t)std::min<uint64_t>((n_pieces + kFimThreads - 1) / kFimThreads, kFimMaxGrid));
    if (bits == 16) hipLaunchKernelGGL((k_fim_gather<16>), ggrid, dim3(kFimThreads), 0, stream, j);
    else hipLaunchKernelGGL((k_fim_gather<32>), ggrid, dim3(kFimThreads), 0, stream, j);
}

}  // namespace mbpe

extern "C" {

int mbpe_fim_plan(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_fim_spec *spec, uint64_t *doc_tok_off_out,
                  uint8_t *mode_out, uint64_t *cut_out) {
    if (!doc_tok_off || !spec || !doc_tok_off_out) return fail(MBPE_ERR_ARG, "mbpe_fim_plan: NULL argument");
    return fim_host_plan("mbpe_fim_plan", doc_tok_off, n_docs, doc_tok_off[n_docs], spec, 32, doc_tok_off_out, mode_out,
                         cut_out);
}

int mbpe_fim_tokens(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                    const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_fim_spec *spec, void *tokens_out, uint64_t cap,
                    int out_on_device, uint64_t *doc_tok_off_out, uint64_t *n_out) {
    if (n_out) *n_out = 0;
    if (!n_out || !doc_tok_off || !spec || (!tokens && n_tokens))
        return fail(MBPE_ERR_ARG, "mbpe_fim_tokens: NULL argument");
    if (token_bits != 16 && token_bits != 32) return fail(MBPE_ERR_ARG, "mbpe_fim_tokens: token_bits must be 16 or 32");
    try {
        std::vector<uint64_t> off(n_docs + 1, 0);
        int rc = fim_host_plan("mbpe_fim_tokens", doc_tok_off, n_docs, n_tokens, spec, token_bits, off.data(), nullptr,
                               nullptr);
        if (rc != MBPE_OK) return rc;
        const uint64_t n_new = off[n_docs];
        *n_out = n_new;
        if (tokens_out && cap < n_new) return fail(MBPE_ERR_ARG, "mbpe_fim_tokens: tokens_out too small");
        if (tokens_out && out_on_device && (uint64_t)(uintptr_t)tokens_out % (token_bits / 8))
            return fail(MBPE_ERR_ARG, "mbpe_fim_tokens: tokens_out is not aligned to its tokens");
        if (tokens_out && n_new) {
            rc = fim_run(device_id, tokens, n_tokens, token_bits, tokens_on_device, doc_tok_off, n_docs, *spec, tokens_out,
                         n_new, out_on_device);
            if (rc != MBPE_OK) return rc;
        }
        if (doc_tok_off_out) std::copy(off.begin(), off.end(), doc_tok_off_out);
        return MBPE_OK;
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_fim_tokens: host allocation failed");
    }
}

int mbpe_fim_kernel_ms(float *ms_out) {
    if (!ms_out) return fail(MBPE_ERR_ARG, "mbpe_fim_kernel_ms: NULL argument");
    *ms_out = g_fim_ms;
    return MBPE_OK;
}

}  // extern "C"
