// Masked-LM corruption on the device: (tokens, doc_off) -> (tokens', targets), between encode and pack.  The rule is
// mlm.h's; this file runs it.
//
//   k_mlm_apply     one wave per span of 1,024 tokens, a lane per 16 bytes of tokens (4 ids of 32 bits, 8 of 16) and
//                   iteration, so a wave's loads and stores are contiguous.  A lane finds the document of its first
//                   token by ONE binary search over doc_off per span and walks on from there: its next piece lies 1,024
//                   bytes further, usually in the same document or the next; a walk that has not arrived after four
//                   steps (runs of empty documents) searches again, from where it stands.  The document's seed s_g is
//                   drawn when the walk enters it.  Per token one draw decides the selection; a selected token costs
//                   one more and a random id a third.  The piece of new ids and the piece (two with 16-bit tokens) of
//                   targets are stored as dwordx4.
//   whole_word      every token needs the index of the latest word start at or before it.  Word starts are the
//                   positions behind a flagged token and the document starts; the latter the walk knows, so only the
//                   former cross lanes, spans and workgroups, as a running maximum of positions:
//   k_mlm_starts      per span the position behind its last flagged token (0: none; position 0 is a start anyway)
//   k_mlm_scan        one workgroup: the exclusive running maximum over the spans, in place
//                   and k_mlm_apply carries it on: per iteration a wave scan (maximum) of the lanes' own last starts,
//                   then max(carry, lanes below, own tokens so far, document start).
// With whole_word == 0 the first two kernels are not launched.  Vector loads and stores need the three addresses 16-byte
// aligned, which device allocations are; otherwise, and in the last piece of the stream, a lane goes id by id.
// Every index is 64-bit.
//
// Bytes moved per token: read once (2 or 4 B), the new id written once (2 or 4 B), the target written once (4 B); with
// whole_word 4 B more read by k_mlm_starts and 8 B per span written, scanned and read; per lane and span one search of
// at most log2(n_docs) probes of 8 B that neighbouring lanes share, per document entered 16 B of offsets.
#include "mlm.h"

#include "hip_host.h"

#include <new>
#include <string>

namespace {

using namespace mbpe;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the lane's piece of PER tokens from i0 on (cnt of them exist) as raw 32-bit values
template <int BITS>
__device__ __forceinline__ void mlm_load(const void *__restrict__ tok, uint64_t i0, uint32_t cnt, bool vec,
                                         uint32_t (&raw)[128 / BITS]) {
    constexpr uint32_t PER = 128 / BITS;
    if (vec && cnt == PER) {
        const u32x4 q = *static_cast<const u32x4 *>(
            __builtin_assume_aligned(static_cast<const uint8_t *>(tok) + i0 * (BITS / 8), 16));
        if (BITS == 32) {
            raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
        } else {
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (uint32_t e = 0; e < PER; ++e) raw[e] = (w[e / 2] >> (16 * (e & 1))) & 0xFFFFu;
        }
    } else {
#pragma unroll
        for (uint32_t e = 0; e < PER; ++e) {
            raw[e] = 0u;
            if (e < cnt) raw[e] = BITS == 16 ? static_cast<const uint16_t *>(tok)[i0 + e] : static_cast<const uint32_t *>(tok)[i0 + e];
        }
    }
}

__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v) {
#pragma unroll
    for (int k = kWave / 2; k > 0; k >>= 1) {
        const unsigned long long u = __shfl_xor(v, k, kWave);
        v = u > v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(kSpanThreads) void k_mlm_starts(const uint32_t *__restrict__ tok, uint64_t n, uint32_t vec,
                                                              unsigned long long *__restrict__ span_last) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    unsigned long long last = 0;
#pragma unroll
    for (int it = 0; it < kSpan / (kWave * 4); ++it) {
        const uint64_t i0 = base + (uint64_t)it * (kWave * 4) + 4u * lane;
        const uint32_t cnt = i0 >= n ? 0u : n - i0 < 4u ? (uint32_t)(n - i0) : 4u;
        uint32_t raw[4];
        mlm_load<32>(tok, i0, cnt, vec != 0, raw);
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e)
            if (e < cnt && (raw[e] & kTokEnd)) last = i0 + e + 1;
    }
    last = wave_max64(last);
    if (lane == 0) span_last[span] = last;
}

// a[s] becomes max(a[0 .. s)), 0 for s == 0: span.h's two sweeps with the maximum in place of the sum
__global__ __launch_bounds__(kScanThreads) void k_mlm_scan(unsigned long long *__restrict__ a, uint64_t n_spans) {
    __shared__ unsigned long long sh[kScanThreads];
    uint64_t lo, hi;
    span_scan_slice(n_spans, threadIdx.x, &lo, &hi);
    unsigned long long m = 0;
    for (uint64_t i = lo; i < hi; ++i) m = a[i] > m ? a[i] : m;
    sh[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long acc = 0;
        for (int t = 0; t < kScanThreads; ++t) {
            const unsigned long long v = sh[t];
            sh[t] = acc;
            acc = v > acc ? v : acc;
        }
    }
    __syncthreads();
    m = sh[threadIdx.x];
    for (uint64_t i = lo; i < hi; ++i) {
        const unsigned long long v = a[i];
        a[i] = m;
        m = v > m ? v : m;
    }
}

struct MlmJob {
    const void *tok;
    const unsigned long long *doc_off;       // n_docs + 1, from 0 to n
    uint64_t n_docs, n;
    void *out;
    uint32_t *tgt;                           // or NULL
    const unsigned long long *span_in;       // whole_word: k_mlm_scan's result
    uint32_t vec;                            // tok, out and tgt are 16-byte aligned
    mbpe_mlm_spec spec;
};

// the largest d in [lo, n_docs) with doc_off[d] <= i, given doc_off[lo] <= i (empty documents share their
// successor's offset and are passed over)
__device__ __forceinline__ uint64_t mlm_find(const unsigned long long *__restrict__ doc_off, uint64_t n_docs, uint64_t lo,
                                             uint64_t i) {
    uint64_t hi = n_docs;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (doc_off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <int BITS, bool WW>
__global__ __launch_bounds__(kSpanThreads) void k_mlm_apply(MlmJob j) {
    constexpr uint32_t PER = 128 / BITS;
    constexpr int kIters = kSpan / (kWave * (int)PER);
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= j.n) return;
    const uint32_t lane = lane_id();
    unsigned long long carry = WW ? j.span_in[span] : 0ull;   // the latest position behind a flagged token before the piece
    uint64_t d = 0;
    unsigned long long ds = 0, de = 0, sg = 0;
    bool found = false;
    for (int it = 0; it < kIters; ++it) {
        const uint64_t i0 = base + (uint64_t)it * (kWave * PER) + PER * lane;
        const uint32_t cnt = i0 >= j.n ? 0u : j.n - i0 < PER ? (uint32_t)(j.n - i0) : PER;
        uint32_t raw[PER];
        mlm_load<BITS>(j.tok, i0, cnt, j.vec != 0, raw);
        unsigned long long cur = 0;
        if (WW) {                                                // (every lane of the wave: shuffles)
            unsigned long long own = 0;
#pragma unroll
            for (uint32_t e = 0; e < PER; ++e)
                if (e < cnt && (raw[e] & kTokEnd)) own = i0 + e + 1;
            unsigned long long incl = own;
#pragma unroll
            for (int k = 1; k < kWave; k <<= 1) {
                const unsigned long long u = __shfl_up(incl, k, kWave);
                if (lane >= (uint32_t)k && u > incl) incl = u;
            }
            const unsigned long long below = __shfl_up(incl, 1, kWave);
            cur = lane && below > carry ? below : carry;
            const unsigned long long all = __shfl(incl, kWave - 1, kWave);
            carry = all > carry ? all : carry;
        }
        if (cnt == 0) continue;
        uint32_t v[PER], t[PER];
#pragma unroll
        for (uint32_t e = 0; e < PER; ++e) {
            v[e] = 0u;
            t[e] = MBPE_NO_TOKEN;
            if (e >= cnt) continue;
            const uint64_t i = i0 + e;
            if (!found || i >= de) {
                if (!found) {
                    d = mlm_find(j.doc_off, j.n_docs, 0, i);
                    found = true;
                } else {
                    uint32_t steps = 0;
                    unsigned long long e1 = de;
                    while (i >= e1 && d + 1 < j.n_docs && steps < 4u) { ++d; e1 = j.doc_off[d + 1]; ++steps; }
                    if (i >= e1 && d + 1 < j.n_docs) d = mlm_find(j.doc_off, j.n_docs, d, i);
                }
                ds = j.doc_off[d];
                de = d + 1 < j.n_docs ? j.doc_off[d + 1] : ~0ull;   // (the last document takes whatever is left)
                sg = mlm_doc_seed(j.spec, d);
            }
            const unsigned long long k = i - ds;
            unsigned long long w = k;
            if (WW) w = (cur > ds ? cur : ds) - ds;
            v[e] = mlm_token(j.spec, sg, k, w, BITS == 16 ? raw[e] : raw[e] & kTokIdMask, &t[e]);
            if (WW && (raw[e] & kTokEnd)) cur = i + 1;
        }
        if (j.vec && cnt == PER) {
            u32x4 q;
            if constexpr (BITS == 32) q = u32x4{v[0], v[1], v[2], v[3]};
            else q = u32x4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)};
            *static_cast<u32x4 *>(__builtin_assume_aligned(static_cast<uint8_t *>(j.out) + i0 * (BITS / 8), 16)) = q;
            if (j.tgt) {
                u32x4 *tq = static_cast<u32x4 *>(__builtin_assume_aligned(j.tgt + i0, 16));
                tq[0] = u32x4{t[0], t[1], t[2], t[3]};
                if constexpr (BITS == 16) tq[1] = u32x4{t[4], t[5], t[6], t[7]};
            }
        } else {
#pragma unroll
            for (uint32_t e = 0; e < PER; ++e) {
                if (e >= cnt) continue;
                if (BITS == 16) static_cast<uint16_t *>(j.out)[i0 + e] = (uint16_t)v[e];
                else static_cast<uint32_t *>(j.out)[i0 + e] = v[e];
                if (j.tgt) j.tgt[i0 + e] = t[e];
            }
        }
    }
}

#define MCHK(expr) MBPE_HIP_CHECK(expr, true)

// device time of the calling thread's latest mbpe_mlm_tokens (mbpe_mlm_kernel_ms)
thread_local float g_mlm_ms = 0.f;

int mlm_run(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
            const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_mlm_spec &spec, void *tokens_out, uint32_t *targets_out,
            int out_on_device) {
    int rc = find_device(device_id);
    if (rc != MBPE_OK) return rc;
    OneShot dev;
    rc = dev.open(device_id);
    if (rc != MBPE_OK) return rc;
    const uint64_t tb = token_bits / 8;
    void *d_tok = const_cast<void *>(tokens), *d_off = nullptr, *d_out = tokens_out, *d_tgt = targets_out, *d_scr = nullptr;
    if (!tokens_on_device) rc = dev.alloc(&d_tok, n_tokens * tb, tokens);
    if (rc == MBPE_OK) rc = dev.alloc(&d_off, (n_docs + 1) * 8, doc_tok_off);
    if (rc == MBPE_OK && !out_on_device) {
        rc = dev.alloc(&d_out, n_tokens * tb, nullptr);
        if (rc == MBPE_OK && targets_out) rc = dev.alloc(&d_tgt, n_tokens * 4, nullptr);
    }
    if (rc == MBPE_OK && spec.whole_word) rc = dev.alloc(&d_scr, mlm_scratch_bytes(n_tokens), nullptr);
    if (rc != MBPE_OK) return rc;
    const MlmDst dst = {d_out, static_cast<uint32_t *>(d_tgt), static_cast<unsigned long long *>(d_scr)};
    MCHK(hipEventRecord(dev.ev0, dev.stream));
    mlm_launch(dev.stream, d_tok, n_tokens, token_bits, static_cast<const unsigned long long *>(d_off), n_docs, spec, dst);
    rc = dev.finish(&g_mlm_ms);
    if (rc != MBPE_OK) return rc;
    if (!out_on_device) {
        MCHK(hipMemcpyAsync(tokens_out, d_out, n_tokens * tb, hipMemcpyDeviceToHost, dev.stream));
        if (targets_out) MCHK(hipMemcpyAsync(targets_out, d_tgt, n_tokens * 4, hipMemcpyDeviceToHost, dev.stream));
        MCHK(hipStreamSynchronize(dev.stream));
    }
    return MBPE_OK;
}

// what mbpe_mlm_plan and mbpe_mlm_tokens check alike
int mlm_host_check(const std::string &who, const uint64_t *doc_tok_off, uint64_t n_docs, uint64_t n_tokens,
                   const mbpe_mlm_spec *spec, uint32_t token_bits) {
    if (token_bits != 16 && token_bits != 32) return fail(MBPE_ERR_ARG, who + ": token_bits must be 16 or 32");
    const char *msg = "";
    int rc = mlm_check_spec(spec, token_bits, &msg);
    if (rc != MBPE_OK) return fail(rc, who + ": " + msg);
    rc = mbpe_host::check_doc_tok_off(doc_tok_off, n_docs, n_tokens);
    if (rc != MBPE_OK) return rc;
    if (n_tokens >> 40 || n_docs >> 40) return fail(MBPE_ERR_ARG, who + ": more than 2^40 tokens or documents");
    return MBPE_OK;
}

}  // namespace

namespace mbpe {

uint64_t mlm_scratch_bytes(uint64_t n_tokens) { return (span_count(n_tokens) + 1) * 8; }

void mlm_launch(hipStream_t stream, const void *tok, uint64_t n_tokens, uint32_t bits, const unsigned long long *doc_off,
                uint64_t n_docs, const mbpe_mlm_spec &spec, const MlmDst &dst) {
    const bool ww = spec.whole_word && bits == 32;               // (16-bit tokens carry no flag: mlm_check_spec)
    const uint32_t vec =
        (((uint64_t)(uintptr_t)tok | (uint64_t)(uintptr_t)dst.tok | (uint64_t)(uintptr_t)dst.tgt) & 15ull) == 0;
    const dim3 grid(span_grid(n_tokens)), block(kSpanThreads);
    if (ww) {
        hipLaunchKernelGGL(k_mlm_starts, grid, block, 0, stream, static_cast<const uint32_t *>(tok), n_tokens, vec,
                           dst.scratch);
        hipLaunchKernelGGL(k_mlm_scan, dim3(1), dim3(kScanThreads), 0, stream, dst.scratch, span_count(n_tokens));
    }
    const MlmJob j = {tok, doc_off, n_docs, n_tokens, dst.tok, dst.tgt, dst.scratch, vec, spec};
    if (bits == 16) hipLaunchKernelGGL((k_mlm_apply<16, false>), grid, block, 0, stream, j);
    else if (ww) hipLaunchKernelGGL((k_mlm_apply<32, true>), grid, block, 0, stream, j);
    else hipLaunchKernelGGL((k_mlm_apply<32, false>), grid, block, 0, stream, j);
}

}  // namespace mbpe

extern "C" {

int mbpe_mlm_plan(const void *tokens, uint64_t n_tokens, uint32_t token_bits, const uint64_t *doc_tok_off, uint64_t n_docs,
                  const mbpe_mlm_spec *spec, void *tokens_out, uint32_t *targets_out) {
    if (!doc_tok_off || !spec || (!tokens && n_tokens)) return fail(MBPE_ERR_ARG, "mbpe_mlm_plan: NULL argument");
    const int rc = mlm_host_check("mbpe_mlm_plan", doc_tok_off, n_docs, n_tokens, spec, token_bits);
    if (rc != MBPE_OK) return rc;
    mlm_plan_host(tokens, token_bits, doc_tok_off, n_docs, *spec, tokens_out, targets_out);
    return MBPE_OK;
}

int mbpe_mlm_tokens(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                    const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_mlm_spec *spec, void *tokens_out,
                    uint32_t *targets_out, int out_on_device) {
    if (!doc_tok_off || !spec || (!tokens && n_tokens) || (!tokens_out && n_tokens))
        return fail(MBPE_ERR_ARG, "mbpe_mlm_tokens: NULL argument");
    int rc = mlm_host_check("mbpe_mlm_tokens", doc_tok_off, n_docs, n_tokens, spec, token_bits);
    if (rc != MBPE_OK) return rc;
    if (out_on_device && ((uint64_t)(uintptr_t)tokens_out % (token_bits / 8) || (uint64_t)(uintptr_t)targets_out % 4))
        return fail(MBPE_ERR_ARG, "mbpe_mlm_tokens: tokens_out or targets_out is not aligned to its elements");
    if (tokens_on_device && (uint64_t)(uintptr_t)tokens % (token_bits / 8))
        return fail(MBPE_ERR_ARG, "mbpe_mlm_tokens: tokens in device memory are not aligned to their elements");
    if (n_tokens == 0) return MBPE_OK;
    try {
        return mlm_run(device_id, tokens, n_tokens, token_bits, tokens_on_device, doc_tok_off, n_docs, *spec, tokens_out,
                       targets_out, out_on_device);
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_mlm_tokens: host allocation failed");
    }
}

int mbpe_mlm_kernel_ms(float *ms_out) {
    if (!ms_out) return fail(MBPE_ERR_ARG, "mbpe_mlm_kernel_ms: NULL argument");
    *ms_out = g_mlm_ms;
    return MBPE_OK;
}

}  // extern "C"
