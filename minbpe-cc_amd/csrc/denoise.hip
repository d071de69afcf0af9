// Span corruption on the device: (tokens, doc_off) -> (inputs, unit_in_off) and (targets, unit_tg_off), between encode
// and two packs.  The rule is denoise.h's; this file runs it.
//
//   k_dn_units        one lane per document, one wave per span of 1,024 documents: the document's unit count U_d into
//                     uoff[d], the span's sum; a unit too long for the counts leaves its document's number in the flag
//                     word (the smallest such number)
//   k_dn_scan         one workgroup: span.h's 64-bit scan over the spans' sums; the total -- the unit count -- goes to
//                     uoff[n_docs] and stays on the device: every kernel below reads it there, and its grid is made for
//                     the bound the host knows
//   k_dn_offsets      the spans again: a wave prefix sum turns the counts into the exclusive prefix sum, in place
//   k_dn_lengths      one lane per unit: its document by binary search over uoff, its length, N and S in closed form;
//                     unit_doc, the input length into in_off, the target length into tg_off, the spans' two sums
//   k_dn_scan2        two workgroups, one per side: the scan again, over n_units read from the device; the totals go
//                     to in_off[n_units] / tg_off[n_units] and, next to the unit count and the flag, into res
//   k_dn_offsets2     k_dn_offsets for both sides (blockIdx.y)
//   k_dn_gather       once per side.  OUTPUT-centric like k_fim_gather: the output is cut at the 16-byte boundaries of
//                     its global address and a lane owns one such piece, 8 ids of 16 bits or 4 of 32.  The first id of a
//                     piece finds its unit by a binary search PER LANE over that side's offsets (empty units are passed
//                     over) and its part by a binary search over j with denoise.h's closed forms, ONE HASH PER PROBE;
//                     the walk then steps over part and unit ends, reads the source tokens with loads of the token's own
//                     width and stores the piece as one dwordx4.  Only the first and the last piece of an output can be
//                     partial; those are stored id by id.  No table of part boundaries exists in memory: a boundary is
//                     recomputed where it is needed (a table would cost 16 B per part written and read again, two fifths
//                     of the tokens' own traffic at T5's defaults with 16-bit ids, to save a hash that hides behind a load).
// Every index is 64-bit.
//
// Bytes moved per token: read once (2 or 4 B) and written once (2 or 4 B), to one side or the other; per unit S
// sentinels written on each side; per document 16 B of offsets read and 8 B of unit offset written twice and read once;
// per unit about 40 B: unit_doc (8 B) and two lengths (16 B) written, the lengths read and written again as offsets
// (16 B); all of it read again by the lanes that enter the unit; per lane at most log2(n_units) probes of 8 B that
// neighbouring lanes share, and log2(S) hashes.
#include "denoise.h"

#include "hip_host.h"

#include <algorithm>
#include <new>
#include <string>
#include <vector>

namespace {

using namespace mbpe;

constexpr int kDnThreads = 256;
constexpr uint32_t kDnMaxGrid = 0x7FFFFFFFu;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kSpanThreads) void k_dn_units(const unsigned long long *__restrict__ doc_off, uint64_t n_docs,
                                                            mbpe_denoise_spec spec, unsigned long long *__restrict__ uoff,
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
            if (dn_too_long(spec, L)) atomicMin(flag, (unsigned long long)d);
            const unsigned long long n = dn_units(spec, L);
            uoff[d] = n;
            s += n;
        }
    }
    for (int k = kWave / 2; k > 0; k >>= 1) s += __shfl_down(s, k, kWave);
    if (lane == 0) span_cnt[span] = s;
}

__global__ __launch_bounds__(kScanThreads) void k_dn_scan(unsigned long long *__restrict__ span_cnt, uint64_t n_spans,
                                                           unsigned long long *__restrict__ total,
                                                           unsigned long long *__restrict__ res) {
    __shared__ unsigned long long sh[kScanThreads];
    const unsigned long long sum = span_scan_sum64(span_cnt, n_spans, sh);
    if (threadIdx.x == 0) {
        *total = sum;
        *res = sum;
    }
}

// off[i] for i < n: lengths -> exclusive prefix sum, in place; span_off from the scan
__device__ __forceinline__ void dn_offsets(unsigned long long *__restrict__ off, uint64_t n,
                                           const unsigned long long *__restrict__ span_off) {
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n) return;
    const uint32_t lane = lane_id();
    unsigned long long o = span_off[span];
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t i = base + (uint64_t)it * kWave + lane;
        const unsigned long long w = i < n ? off[i] : 0ull;
        const unsigned long long incl = wave_prefix64(w, lane);
        if (i < n) off[i] = o + incl - w;
        o += __shfl(incl, kWave - 1, kWave);
    }
}

__global__ __launch_bounds__(kSpanThreads) void k_dn_offsets(unsigned long long *__restrict__ uoff, uint64_t n_docs,
                                                              const unsigned long long *__restrict__ span_off) {
    dn_offsets(uoff, n_docs, span_off);
}

__global__ __launch_bounds__(kSpanThreads) void k_dn_lengths(const unsigned long long *__restrict__ doc_off,
                                                              const unsigned long long *__restrict__ uoff, uint64_t n_docs,
                                                              mbpe_denoise_spec spec, uint64_t cap_units,
                                                              unsigned long long *__restrict__ unit_doc,
                                                              unsigned long long *__restrict__ in_off,
                                                              unsigned long long *__restrict__ tg_off,
                                                              uint32_t *__restrict__ row_doc,
                                                              unsigned long long *__restrict__ span_in,
                                                              unsigned long long *__restrict__ span_tg) {
    const unsigned long long units = uoff[n_docs];
    const uint64_t n_units = units < cap_units ? units : cap_units;      // (they are equal or there is more room)
    const uint64_t span = span_index(), base = span * kSpan;
    if (base >= n_units) return;
    const uint32_t lane = lane_id();
    unsigned long long si = 0, st = 0;
    for (int it = 0; it < kSpanIters; ++it) {
        const uint64_t k = base + (uint64_t)it * kWave + lane;
        if (k < n_units) {
            // the unit's document: the largest d with uoff[d] <= k (every document has a unit: uoff ascends strictly)
            uint64_t d = 0, hi = n_docs;
            while (hi - d > 1) {
                const uint64_t m = d + (hi - d) / 2;
                if (uoff[m] <= k) d = m;
                else hi = m;
            }
            const unsigned long long L = dn_unit_len(spec, doc_off[d + 1] - doc_off[d], k - uoff[d]);
            const DnCounts c = dn_counts(spec, L);
            const unsigned long long ni = dn_in_len(c, L), nt = c.S ? dn_tg_len(c) : 0ull;
            unit_doc[k] = d;
            if (row_doc) row_doc[k] = (uint32_t)d;
            in_off[k] = ni;
            tg_off[k] = nt;
            si += ni;
            st += nt;
        }
    }
    for (int k = kWave / 2; k > 0; k >>= 1) {
        si += __shfl_down(si, k, kWave);
        st += __shfl_down(st, k, kWave);
    }
    if (lane == 0) {
        span_in[span] = si;
        span_tg[span] = st;
    }
}

// the two sides of the stage, as the kernels behind k_dn_lengths see them
struct DnSides {
    unsigned long long *off[2];              // in_off, tg_off
    unsigned long long *span[2];             // their spans' sums
};

__global__ __launch_bounds__(kScanThreads) void k_dn_scan2(DnSides s, const unsigned long long *__restrict__ units,
                                                            uint64_t cap_units, unsigned long long *__restrict__ res) {
    __shared__ unsigned long long sh[kScanThreads];
    const uint64_t n_units = *units < cap_units ? *units : cap_units;
    const uint32_t side = blockIdx.x;
    const unsigned long long sum = span_scan_sum64(s.span[side], span_count(n_units), sh);
    if (threadIdx.x == 0) {
        s.off[side][n_units] = sum;
        res[1 + side] = sum;
    }
}

__global__ __launch_bounds__(kSpanThreads) void k_dn_offsets2(DnSides s, const unsigned long long *__restrict__ units,
                                                               uint64_t cap_units) {
    const uint64_t n_units = *units < cap_units ? *units : cap_units;
    dn_offsets(s.off[blockIdx.y], n_units, s.span[blockIdx.y]);
}

struct DnJob {
    const void *tok;
    const unsigned long long *doc_off;       // the documents' token offsets, n_docs + 1
    const unsigned long long *uoff;          // their unit offsets; uoff[n_docs] = the units
    const unsigned long long *unit_doc;
    const unsigned long long *off;           // this side's offsets; off[n_units] = ids of the output
    uint64_t n_docs, cap_units;
    void *out;
    uint64_t cap;                            // ids the output holds
    mbpe_denoise_spec spec;
};

// SIDE 0: the inputs, 1: the targets
template <int SIDE>
struct DnSideCur;
template <>
struct DnSideCur<0> {
    DnCur c;
    __device__ __forceinline__ void seek(const DnUnit &u, unsigned long long p) { dn_in_seek(u, p, &c); }
    __device__ __forceinline__ void start(const DnUnit &u) { dn_in_enter(u, 0, &c); }
    __device__ __forceinline__ unsigned long long step(const DnUnit &u, unsigned long long p) { return dn_in_step(u, p, &c); }
};
template <>
struct DnSideCur<1> {
    DnTgCur c;
    __device__ __forceinline__ void seek(const DnUnit &u, unsigned long long p) { dn_tg_seek(u, p, &c); }
    __device__ __forceinline__ void start(const DnUnit &u) { dn_tg_enter(u, 0, 0, &c); }
    __device__ __forceinline__ unsigned long long step(const DnUnit &u, unsigned long long p) { return dn_tg_step(u, p, &c); }
};

// unit k as the walk needs it: the rule's view of it, where its tokens begin, and its ids on this side
__device__ __forceinline__ void dn_enter(const DnJob &j, uint64_t k, DnUnit *un, unsigned long long *t0,
                                         unsigned long long *n) {
    const unsigned long long d = j.unit_doc[k], u = k - j.uoff[d], s0 = j.doc_off[d];
    *un = dn_unit(j.spec, d, j.doc_off[d + 1] - s0, u);
    *t0 = s0 + u * j.spec.segment_tokens;
    *n = j.off[k + 1] - j.off[k];
}

template <int BITS, int SIDE>
__global__ __launch_bounds__(kDnThreads) void k_dn_gather(DnJob j) {
    constexpr uint32_t ob = BITS / 8;
    const unsigned long long units = j.uoff[j.n_docs];
    const uint64_t n_units = units < j.cap_units ? units : j.cap_units;
    const unsigned long long total = j.off[n_units];
    const uint64_t n_out = total < j.cap ? total : j.cap;        // (they are equal or the buffer is larger)
    const uint64_t A = (uint64_t)(uintptr_t)j.out, E = A + n_out * ob, B0 = A & ~15ull;
    const uint64_t n_pieces = (E - B0 + 15) >> 4;
    uint8_t *base = static_cast<uint8_t *>(j.out);
    for (uint64_t p = (uint64_t)blockIdx.x * kDnThreads + threadIdx.x; p < n_pieces;
         p += (uint64_t)gridDim.x * kDnThreads) {
        const uint64_t B = B0 + (p << 4);
        const uint64_t lo = B > A ? B : A;
        const uint64_t hi = B + 16 < E ? B + 16 : E;
        if (hi <= lo) continue;                                  // (n_out == 0)
        const uint32_t cnt = (uint32_t)(hi - lo) / ob;
        const uint64_t f = (lo - A) / ob;
        // the unit that holds position f < n_out: the largest k with off[k] <= f (empty units share their successor's
        // offset and are passed over)
        uint64_t k = 0, hi_k = n_units;
        while (hi_k - k > 1) {
            const uint64_t m = k + (hi_k - k) / 2;
            if (j.off[m] <= f) k = m;
            else hi_k = m;
        }
        DnUnit un;
        unsigned long long t0, n, q = f - j.off[k];
        dn_enter(j, k, &un, &t0, &n);
        DnSideCur<SIDE> cur;
        cur.seek(un, q);
        unsigned __int128 acc = 0;
        for (uint32_t e = 0; e < cnt; ++e) {
            if (q >= n) {                                        // the unit's end: f + e < n_out, a unit with ids follows
                do ++k; while (j.off[k + 1] == j.off[k]);
                q = 0;
                dn_enter(j, k, &un, &t0, &n);
                cur.start(un);
            }
            const unsigned long long src = cur.step(un, q);
            uint32_t v;
            if (src & kDnSent) v = dn_sentinel(j.spec, src & ~kDnSent);
            else if (BITS == 16) v = static_cast<const uint16_t *>(j.tok)[t0 + src];
            else v = static_cast<const uint32_t *>(j.tok)[t0 + src] & kTokIdMask;
            acc |= (unsigned __int128)v << (BITS * e);
            ++q;
        }
        if (cnt == 128 / BITS) {                                 // (then lo == B)
            u32x4 w;
            w.x = (uint32_t)acc;
            w.y = (uint32_t)(acc >> 32);
            w.z = (uint32_t)(acc >> 64);
            w.w = (uint32_t)(acc >> 96);
            *static_cast<u32x4 *>(__builtin_assume_aligned(base + (B - A), 16)) = w;
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

template <int SIDE>
void dn_gather_launch(hipStream_t stream, uint32_t bits, const DnJob &j) {
    const uint64_t A = (uint64_t)(uintptr_t)j.out, E = A + j.cap * (bits / 8);
    const uint64_t n_pieces = (E - (A & ~15ull) + 15) >> 4;
    const dim3 grid((uint32_t)std::min<uint64_t>((n_pieces + kDnThreads - 1) / kDnThreads, kDnMaxGrid));
    if (bits == 16) hipLaunchKernelGGL((k_dn_gather<16, SIDE>), grid, dim3(kDnThreads), 0, stream, j);
    else hipLaunchKernelGGL((k_dn_gather<32, SIDE>), grid, dim3(kDnThreads), 0, stream, j);
}

#define DCHK(expr) MBPE_HIP_CHECK(expr, true)

// device time of the calling thread's latest mbpe_denoise_tokens (mbpe_denoise_kernel_ms)
thread_local float g_dn_ms = 0.f;

// the host's plan of a call
struct DnHostPlan {
    std::vector<uint64_t> in_off, tg_off, unit_doc;
    uint64_t n_units = 0;
};

int dn_run(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
           const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_denoise_spec &spec, void *inputs_out, void *targets_out,
           int out_on_device, DnHostPlan *plan) {
    int rc = find_device(device_id);
    if (rc != MBPE_OK) return rc;
    OneShot dev;
    rc = dev.open(device_id);
    if (rc != MBPE_OK) return rc;
    const uint64_t tb = token_bits / 8, n_units = plan->n_units, n_in = plan->in_off[n_units], n_tg = plan->tg_off[n_units];
    void *d_tok = const_cast<void *>(tokens), *d_off = nullptr, *d_in = inputs_out, *d_tg = targets_out, *d_uoff = nullptr,
         *d_udoc = nullptr, *d_ioff = nullptr, *d_toff = nullptr, *d_res = nullptr, *d_scr = nullptr;
    if (!tokens_on_device) rc = dev.alloc(&d_tok, n_tokens * tb, tokens);
    if (rc == MBPE_OK) rc = dev.alloc(&d_off, (n_docs + 1) * 8, doc_tok_off);
    if (rc == MBPE_OK && !out_on_device) rc = dev.alloc(&d_in, n_in * tb, nullptr);
    if (rc == MBPE_OK && !out_on_device) rc = dev.alloc(&d_tg, n_tg * tb, nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_uoff, (n_docs + 1) * 8, nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_udoc, n_units * 8, nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_ioff, (n_units + 1) * 8, nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_toff, (n_units + 1) * 8, nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_res, 32, nullptr);
    if (rc == MBPE_OK) rc = dev.alloc(&d_scr, dn_scratch_bytes(n_docs, n_units), nullptr);
    if (rc != MBPE_OK) return rc;
    typedef unsigned long long ull;
    const DnDst dst = {d_in, d_tg, n_in, n_tg, static_cast<ull *>(d_uoff), static_cast<ull *>(d_udoc),
                       static_cast<ull *>(d_ioff), static_cast<ull *>(d_toff), static_cast<ull *>(d_res),
                       static_cast<ull *>(d_scr), nullptr, n_units};
    DCHK(hipEventRecord(dev.ev0, dev.stream));
    dn_launch(dev.stream, d_tok, token_bits, static_cast<const ull *>(d_off), n_docs, spec, dst);
    rc = dev.finish(&g_dn_ms);
    if (rc != MBPE_OK) return rc;
    // what the device made of it: the totals, which the host's plan has sized the buffers by, and the unit arrays
    ull res[4] = {0, 0, 0, 0};
    DCHK(hipMemcpyAsync(res, d_res, 32, hipMemcpyDeviceToHost, dev.stream));
    DCHK(hipStreamSynchronize(dev.stream));
    if (res[0] != n_units || res[1] != n_in || res[2] != n_tg || res[3] != ~0ull)
        return fail(MBPE_ERR_HIP, "mbpe_denoise_tokens: the device's plan differs from the host's");
    DCHK(hipMemcpyAsync(plan->in_off.data(), d_ioff, (n_units + 1) * 8, hipMemcpyDeviceToHost, dev.stream));
    DCHK(hipMemcpyAsync(plan->tg_off.data(), d_toff, (n_units + 1) * 8, hipMemcpyDeviceToHost, dev.stream));
    DCHK(hipMemcpyAsync(plan->unit_doc.data(), d_udoc, n_units * 8, hipMemcpyDeviceToHost, dev.stream));
    if (!out_on_device) {
        DCHK(hipMemcpyAsync(inputs_out, d_in, n_in * tb, hipMemcpyDeviceToHost, dev.stream));
        if (n_tg) DCHK(hipMemcpyAsync(targets_out, d_tg, n_tg * tb, hipMemcpyDeviceToHost, dev.stream));
    }
    DCHK(hipStreamSynchronize(dev.stream));
    return MBPE_OK;
}

// what mbpe_denoise_plan and mbpe_denoise_tokens check alike, then the host's plan
int dn_host_plan(const std::string &who, const uint64_t *doc_tok_off, uint64_t n_docs, uint64_t n_tokens,
                 const mbpe_denoise_spec *spec, uint32_t token_bits, DnHostPlan *plan) {
    const char *msg = "";
    int rc = denoise_check_spec(spec, token_bits, &msg);
    if (rc != MBPE_OK) return fail(rc, who + ": " + msg);
    rc = mbpe_host::check_doc_tok_off(doc_tok_off, n_docs, n_tokens);
    if (rc != MBPE_OK) return rc;
    if (n_tokens >> 40 || n_docs >> 40) return fail(MBPE_ERR_ARG, who + ": more than 2^40 tokens or documents");
    uint64_t bad = 0;
    rc = denoise_plan_host(doc_tok_off, n_docs, *spec, &plan->n_units, nullptr, nullptr, nullptr, 0, &bad);
    if (rc == MBPE_OK) {
        plan->in_off.assign(plan->n_units + 1, 0);
        plan->tg_off.assign(plan->n_units + 1, 0);
        plan->unit_doc.assign(plan->n_units, 0);
        rc = denoise_plan_host(doc_tok_off, n_docs, *spec, &plan->n_units, plan->in_off.data(), plan->tg_off.data(),
                               plan->unit_doc.data(), plan->n_units, &bad);
    }
    if (rc != MBPE_OK)
        return fail(rc, bad != ~0ull ? who + ": document " + std::to_string(bad) + " has a unit of 2^32 - 1 tokens or more"
                                     : who + ": more than 2^40 units");
    return MBPE_OK;
}

// the plan into the caller's arrays, each NULL or with room for the units (checked by the caller)
void dn_plan_out(const DnHostPlan &p, uint64_t *unit_in_off, uint64_t *unit_tg_off, uint64_t *unit_doc) {
    if (unit_in_off) std::copy(p.in_off.begin(), p.in_off.end(), unit_in_off);
    if (unit_tg_off) std::copy(p.tg_off.begin(), p.tg_off.end(), unit_tg_off);
    if (unit_doc) std::copy(p.unit_doc.begin(), p.unit_doc.end(), unit_doc);
}

}  // namespace

namespace mbpe {

uint64_t dn_scratch_bytes(uint64_t n_docs, uint64_t cap_units) {
    return (span_count(n_docs) + 2 * span_count(cap_units)) * 8;
}

void dn_launch(hipStream_t stream, const void *tok, uint32_t bits, const unsigned long long *doc_off, uint64_t n_docs,
               const mbpe_denoise_spec &spec, const DnDst &dst) {
    unsigned long long *flag = dst.res + 3, *span_u = dst.scratch, *span_in = span_u + span_count(n_docs),
                       *span_tg = span_in + span_count(dst.cap_units);
    (void)hipMemsetAsync(flag, 0xFF, 8, stream);
    const dim3 grid(span_grid(n_docs)), block(kSpanThreads);
    hipLaunchKernelGGL(k_dn_units, grid, block, 0, stream, doc_off, n_docs, spec, dst.uoff, span_u, flag);
    hipLaunchKernelGGL(k_dn_scan, dim3(1), dim3(kScanThreads), 0, stream, span_u, span_count(n_docs), dst.uoff + n_docs,
                       dst.res);
    hipLaunchKernelGGL(k_dn_offsets, grid, block, 0, stream, dst.uoff, n_docs, span_u);
    const uint32_t ugrid = span_grid(dst.cap_units);
    hipLaunchKernelGGL(k_dn_lengths, dim3(ugrid), block, 0, stream, doc_off, dst.uoff, n_docs, spec, dst.cap_units,
                       dst.unit_doc, dst.in_off, dst.tg_off, dst.row_doc, span_in, span_tg);
    const DnSides sides = {{dst.in_off, dst.tg_off}, {span_in, span_tg}};
    hipLaunchKernelGGL(k_dn_scan2, dim3(2), dim3(kScanThreads), 0, stream, sides, dst.uoff + n_docs, dst.cap_units, dst.res);
    hipLaunchKernelGGL(k_dn_offsets2, dim3(ugrid, 2), block, 0, stream, sides, dst.uoff + n_docs, dst.cap_units);
    DnJob j = {tok, doc_off, dst.uoff, dst.unit_doc, dst.in_off, n_docs, dst.cap_units, dst.in, dst.cap_in, spec};
    if (dst.cap_in) dn_gather_launch<0>(stream, bits, j);
    j.off = dst.tg_off;
    j.out = dst.tg;
    j.cap = dst.cap_tg;
    if (dst.cap_tg) dn_gather_launch<1>(stream, bits, j);
}

}  // namespace mbpe

extern "C" {

int mbpe_denoise_plan(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_denoise_spec *spec, uint64_t *n_units_out,
                      uint64_t *unit_in_off, uint64_t *unit_tg_off, uint64_t *unit_doc, uint64_t cap_units) {
    if (n_units_out) *n_units_out = 0;
    if (!doc_tok_off || !spec || !n_units_out) return fail(MBPE_ERR_ARG, "mbpe_denoise_plan: NULL argument");
    try {
        DnHostPlan plan;
        const int rc = dn_host_plan("mbpe_denoise_plan", doc_tok_off, n_docs, doc_tok_off[n_docs], spec, 32, &plan);
        if (rc != MBPE_OK) return rc;
        *n_units_out = plan.n_units;
        if ((unit_in_off || unit_tg_off || unit_doc) && cap_units < plan.n_units)
            return fail(MBPE_ERR_ARG, "mbpe_denoise_plan: room for fewer units than the call has");
        dn_plan_out(plan, unit_in_off, unit_tg_off, unit_doc);
        return MBPE_OK;
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_denoise_plan: host allocation failed");
    }
}

int mbpe_denoise_tokens(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits, int tokens_on_device,
                        const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_denoise_spec *spec, void *inputs_out,
                        uint64_t cap_in, void *targets_out, uint64_t cap_tg, int out_on_device, uint64_t *unit_in_off,
                        uint64_t *unit_tg_off, uint64_t *unit_doc, uint64_t cap_units, uint64_t *n_units_out,
                        uint64_t *n_in_out, uint64_t *n_tg_out) {
    if (n_units_out) *n_units_out = 0;
    if (n_in_out) *n_in_out = 0;
    if (n_tg_out) *n_tg_out = 0;
    if (!n_units_out || !n_in_out || !n_tg_out || !doc_tok_off || !spec || (!tokens && n_tokens))
        return fail(MBPE_ERR_ARG, "mbpe_denoise_tokens: NULL argument");
    if (token_bits != 16 && token_bits != 32) return fail(MBPE_ERR_ARG, "mbpe_denoise_tokens: token_bits must be 16 or 32");
    try {
        DnHostPlan plan;
        int rc = dn_host_plan("mbpe_denoise_tokens", doc_tok_off, n_docs, n_tokens, spec, token_bits, &plan);
        if (rc != MBPE_OK) return rc;
        const uint64_t n_in = plan.in_off[plan.n_units], n_tg = plan.tg_off[plan.n_units];
        *n_units_out = plan.n_units;
        *n_in_out = n_in;
        *n_tg_out = n_tg;
        if ((unit_in_off || unit_tg_off || unit_doc) && cap_units < plan.n_units)
            return fail(MBPE_ERR_ARG, "mbpe_denoise_tokens: room for fewer units than the call has");
        if (inputs_out) {
            if (!targets_out && n_tg) return fail(MBPE_ERR_ARG, "mbpe_denoise_tokens: inputs_out without targets_out");
            if (cap_in < n_in) return fail(MBPE_ERR_ARG, "mbpe_denoise_tokens: inputs_out too small");
            if (cap_tg < n_tg) return fail(MBPE_ERR_ARG, "mbpe_denoise_tokens: targets_out too small");
            if (out_on_device &&
                ((uint64_t)(uintptr_t)inputs_out % (token_bits / 8) || (uint64_t)(uintptr_t)targets_out % (token_bits / 8)))
                return fail(MBPE_ERR_ARG, "mbpe_denoise_tokens: an output is not aligned to its tokens");
            if (n_in) {
                rc = dn_run(device_id, tokens, n_tokens, token_bits, tokens_on_device, doc_tok_off, n_docs, *spec, inputs_out,
                            targets_out, out_on_device, &plan);
                if (rc != MBPE_OK) return rc;
            }
        }
        dn_plan_out(plan, unit_in_off, unit_tg_off, unit_doc);
        return MBPE_OK;
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_denoise_tokens: host allocation failed");
    }
}

int mbpe_denoise_kernel_ms(float *ms_out) {
    if (!ms_out) return fail(MBPE_ERR_ARG, "mbpe_denoise_kernel_ms: NULL argument");
    *ms_out = g_dn_ms;
    return MBPE_OK;
}

}  // extern "C"
