// The gpt2 / gpt4 pre-split on the device: the chunk-end mask of a text, in the trainer's format,
// without a regex engine or a Unicode table on the device.  split_rule.h holds the rule and the exactness argument;
// here are the passes around it:
//   k_split_find     (split_docs with names) 16 text bytes per lane -> the list of (position, name) occurrences
//   k_split_gather   (split_docs of a device text) the first byte of every part
//   k_split_patch    (split_docs) the cut list -> the cut bitmap;  k_split_raw: the ranges -> the bitmap of their bytes
//   k_split_sync     16 text bytes per lane -> the boundary bitmap (sync points | cuts) and the non-ASCII bitmap
//   k_split_walk     one thread per 64-byte block: every span that starts in it is walked with the step rule (its chunk
//                    ends are OR-ed into the zeroed mask) or, when it is too long or holds a non-ASCII byte, marked
//   k_split_compact  the marked spans as a list of (a, b), whose capacity is the walk's own count of its marks
//   (host)           the listed spans through PCRE2 (presplit.cpp), their chunk ends uploaded
//   k_split_patch    those chunk ends OR-ed into the mask
//   k_mask_popcount  the number of chunks
// With the option "unicode" the sync pass and the walk are k_split_sync_u and k_split_walk_u: the rule on scalar values,
// classes from the table PCRE2 filled (split_rule.h), the second bitmap = the ill-formed bytes.  The default mode's two
// kernels are untouched by it.
// All positions are 64-bit.
#include "hip_host.h"
#include "split.h"
#include "split_rule.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace mbpe {
namespace {

constexpr int kSplitThreads = 256;
static_assert(kSplitBlock == MBPE_SPLIT_BLOCK, "mbpe.h publishes the walk's block size");
static_assert(kSplitBlock * kSplitThreads == MBPE_SPLIT_TILE, "... and the bytes of one of its workgroups");

// control words of one call
enum { kCtlHost = 0, kCtlCursor = 1, kCtlChunks = 2, kCtlFound = 3, kCtlWords = 4 };

// bitmaps as 16-bit pieces, one per vector: n_pieces = 4 * n_words of them, those at and beyond the text are 0
__global__ __launch_bounds__(kSplitThreads) void k_split_sync(const uint8_t *__restrict__ t, uint64_t n,
                                                              uint64_t n_pieces, const uint16_t *__restrict__ cut,
                                                              uint16_t *__restrict__ sync,
                                                              uint16_t *__restrict__ hi) {
    const uint64_t v = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (v >= n_pieces) return;
    const uint64_t at = v * kSplitVec;
    uint32_t w[4] = {0u, 0u, 0u, 0u}, s = 0u, h = 0u;
    if (at < n) {
        if (n - at >= (uint64_t)kSplitVec) {
            const uint4 q = *reinterpret_cast<const uint4 *>(t + at);      // (the text is 16-byte aligned)
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
            for (uint32_t k = 0; k < (uint32_t)(n - at); ++k) w[k >> 2] |= (uint32_t)t[at + k] << (8u * (k & 3u));
        }
        split_vec_bits(w, at ? t[at - 1] : (uint32_t)' ', &s, &h);
    }
    sync[v] = (uint16_t)(cut ? s | cut[v] : s);
    hi[v] = (uint16_t)h;
}

// unicode mode: the same lane, the same 16 bytes; a lane that sees a byte >= 0x80 reads its neighbourhood as plain bytes.
// hi = the ill-formed bitmap
__global__ __launch_bounds__(kSplitThreads) void k_split_sync_u(const uint8_t *__restrict__ t, uint64_t n,
                                                                uint64_t n_pieces, const uint16_t *__restrict__ cut,
                                                                int pattern, const uint32_t *__restrict__ tab,
                                                                uint16_t *__restrict__ sync,
                                                                uint16_t *__restrict__ hi) {
    const uint64_t v = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (v >= n_pieces) return;
    const uint64_t at = v * kSplitVec;
    uint32_t w[4] = {0u, 0u, 0u, 0u}, s = 0u, h = 0u;
    if (at < n) {
        if (n - at >= (uint64_t)kSplitVec) {
            const uint4 q = *reinterpret_cast<const uint4 *>(t + at);
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
            for (uint32_t k = 0; k < (uint32_t)(n - at); ++k) w[k >> 2] |= (uint32_t)t[at + k] << (8u * (k & 3u));
        }
        split_vec_bits_u(t, n, at, w, pattern, tab, &s, &h);
    }
    sync[v] = (uint16_t)(cut ? s | cut[v] : s);
    hi[v] = (uint16_t)h;
}

// the occurrences of the names; blob = first-byte set (8 words), n_names + 1 offsets, the names' bytes
struct FindHit {
    unsigned long long *list;
    unsigned long long cap;
    unsigned long long *count;
    __device__ void operator()(uint64_t p, uint32_t name) {
        const unsigned long long at = atomicAdd(count, 1ull);
        if (at < cap) list[at] = ((unsigned long long)p << kSplitNameBits) | name;   // (the host grows the list and asks again)
    }
};

__global__ __launch_bounds__(kSplitThreads) void k_split_find(const uint8_t *__restrict__ t, uint64_t n, uint64_t n_vec,
                                                              const uint32_t *__restrict__ blob, uint32_t n_names,
                                                              uint32_t name_bytes, unsigned long long *__restrict__ list,
                                                              unsigned long long cap,
                                                              unsigned long long *__restrict__ count) {
    __shared__ uint32_t sh_first[8];
    __shared__ uint32_t sh_off[kSplitMaxNames + 1];
    __shared__ uint32_t sh_bytes[kSplitMaxNameBytes / 4];
    if (threadIdx.x < 8) sh_first[threadIdx.x] = blob[threadIdx.x];
    for (uint32_t i = threadIdx.x; i <= n_names; i += kSplitThreads) sh_off[i] = blob[8 + i];
    for (uint32_t i = threadIdx.x; i < (name_bytes + 3) / 4; i += kSplitThreads) sh_bytes[i] = blob[8 + n_names + 1 + i];
    __syncthreads();
    const uint64_t v = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (v >= n_vec) return;
    const uint64_t at = v * kSplitVec;
    uint64_t lo = 0, up = 0;
    if (n - at >= (uint64_t)kSplitVec) {
        const uint4 q = *reinterpret_cast<const uint4 *>(t + at);
        lo = q.x | ((uint64_t)q.y << 32);
        up = q.z | ((uint64_t)q.w << 32);
    } else {
        for (uint32_t k = 0; k < (uint32_t)(n - at); ++k) {
            if (k < 8u) lo |= (uint64_t)t[at + k] << (8u * k);
            else up |= (uint64_t)t[at + k] << (8u * (k - 8u));
        }
    }
    const SplitNames nm = {reinterpret_cast<const uint8_t *>(sh_bytes), sh_off, sh_first, n_names};
    FindHit hit = {list, cap, count};
    split_find_vec(t, n, at, lo, up, nm, hit);
}

__global__ __launch_bounds__(kSplitThreads) void k_split_gather(const uint8_t *__restrict__ t, uint64_t n,
                                                                const unsigned long long *__restrict__ pos,
                                                                uint64_t n_pos, uint8_t *__restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (j >= n_pos) return;
    const uint64_t p = pos[j];
    out[j] = p < n ? t[p] : (uint8_t)0xFF;
}

// rng[2 j], rng[2 j + 1] = start and length of range j: its bytes' bits, OR-ed into the zeroed bitmap
__global__ __launch_bounds__(kSplitThreads) void k_split_raw(const unsigned long long *__restrict__ rng, uint64_t n_rng,
                                                             uint64_t n, unsigned long long *__restrict__ raw) {
    const uint64_t j = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (j >= n_rng) return;
    const uint64_t a = rng[2 * j], len = rng[2 * j + 1];
    if (a >= n || len == 0 || len > n - a) return;
    const uint64_t last = a + len - 1;
    for (uint64_t w = a >> 6; w <= last >> 6; ++w) {
        unsigned long long m = ~0ull;
        if (w == a >> 6) m &= ~0ull << (a & 63);
        if (w == last >> 6) m &= ~0ull >> (63 - (last & 63));
        atomicOr(raw + w, m);
    }
}

// the chunk ends of one thread, gathered per 32-bit word of the mask: a span may reach into the blocks of other
// threads, so every word goes out with one atomic OR
struct EndBits {
    uint32_t *mask;
    uint64_t word;
    uint32_t bits;
    __device__ void operator()(uint64_t p) {
        const uint64_t w = p >> 5;
        if (w != word) { flush(); word = w; }
        bits |= 1u << (p & 31u);
    }
    __device__ void flush() {
        if (bits) atomicOr(mask + word, bits);
        bits = 0u;
    }
};

__global__ __launch_bounds__(kSplitThreads) void k_split_walk(const uint8_t *__restrict__ t, uint64_t n,
                                                              const unsigned long long *__restrict__ sync,
                                                              const unsigned long long *__restrict__ hi,
                                                              const unsigned long long *__restrict__ cut,
                                                              const unsigned long long *__restrict__ raw, uint64_t n_words,
                                                              uint64_t max_span, int pattern, uint32_t *__restrict__ mask,
                                                              unsigned long long *__restrict__ hostmark,
                                                              unsigned long long *__restrict__ ctl) {
    const uint64_t T = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (T >= n_words) return;
    EndBits end = {mask, ~0ull, 0u};
    const unsigned long long host = split_walk_block(t, n, sync, hi, cut, raw, T, max_span, pattern, end);
    end.flush();
    hostmark[T] = host;
    if (host) atomicAdd(ctl + kCtlHost, (unsigned long long)__popcll(host));
}

__global__ __launch_bounds__(kSplitThreads) void k_split_walk_u(const uint8_t *__restrict__ t, uint64_t n,
                                                                const unsigned long long *__restrict__ sync,
                                                                const unsigned long long *__restrict__ bad,
                                                                const unsigned long long *__restrict__ cut,
                                                                const unsigned long long *__restrict__ raw, uint64_t n_words,
                                                                uint64_t max_span, int pattern,
                                                                const uint32_t *__restrict__ tab, SplitFold fold,
                                                                uint32_t *__restrict__ mask,
                                                                unsigned long long *__restrict__ hostmark,
                                                                unsigned long long *__restrict__ ctl) {
    const uint64_t T = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (T >= n_words) return;
    EndBits end = {mask, ~0ull, 0u};
    const SplitCharStep step = {pattern, tab, fold};
    const unsigned long long host = split_walk_block_with(t, n, sync, bad, cut, raw, T, max_span, step, end);
    end.flush();
    hostmark[T] = host;
    if (host) atomicAdd(ctl + kCtlHost, (unsigned long long)__popcll(host));
}

// list[2 j], list[2 j + 1] = a host span and its end, in no particular order; cap = the spans the walk counted
__global__ __launch_bounds__(kSplitThreads) void k_split_compact(const unsigned long long *__restrict__ sync,
                                                                 const unsigned long long *__restrict__ hostmark,
                                                                 uint64_t n, uint64_t n_words,
                                                                 unsigned long long *__restrict__ list, uint64_t cap,
                                                                 unsigned long long *__restrict__ ctl) {
    const uint64_t T = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (T >= n_words) return;
    unsigned long long hm = hostmark[T];
    while (hm) {
        const uint64_t a = (T << 6) + (uint64_t)__builtin_ctzll(hm);
        hm &= hm - 1;
        const uint64_t b = split_next_bit(sync, a + 1, n);
        const unsigned long long j = atomicAdd(ctl + kCtlCursor, 1ull);
        if (j < cap) { list[2 * j] = a; list[2 * j + 1] = b; }
    }
}

__global__ __launch_bounds__(kSplitThreads) void k_split_patch(const unsigned long long *__restrict__ pos, uint64_t n_pos,
                                                               uint64_t n, uint32_t *__restrict__ mask) {
    const uint64_t j = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (j >= n_pos) return;
    const uint64_t p = pos[j];
    if (p < n) atomicOr(mask + (p >> 5), 1u << (p & 31u));
}

// the set bits of the first n_words32 words of a mask, added to *out
__global__ __launch_bounds__(kSplitThreads) void k_mask_popcount(const uint32_t *__restrict__ mask, uint64_t n_words32,
                                                                 unsigned long long *__restrict__ out) {
    unsigned long long s = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x; i < n_words32;
         i += (uint64_t)gridDim.x * kSplitThreads)
        s += (unsigned long long)__popc(mask[i]);
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}

uint32_t grid_for(uint64_t n_items) { return (uint32_t)((n_items + kSplitThreads - 1) / kSplitThreads); }

#define SCHK(expr) MBPE_HIP_CHECK(expr, false)

}  // namespace

void launch_mask_popcount(hipStream_t stream, const uint8_t *mask, uint64_t n_bytes, unsigned long long *count_out) {
    const uint64_t n_words32 = (n_bytes + 31) / 32;
    if (!n_words32) return;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(grid_for(n_words32), 2048);
    hipLaunchKernelGGL(k_mask_popcount, dim3(grid), dim3(kSplitThreads), 0, stream,
                       reinterpret_cast<const uint32_t *>(mask), n_words32, count_out);
}

}  // namespace mbpe

using namespace mbpe;

struct mbpe_splitter : DevQueue {
    mbpe_splitter() : DevQueue(false) {}
    int pattern = kSplitGpt2;
    mbpe_host::Splitter host;                 // the same pattern through PCRE2, for the host spans
    uint64_t max_span = MBPE_SPLIT_MAX_SPAN;
    bool unicode = false;                     // the option; the table is uploaded by the first call that needs it
    DevBuf<uint32_t> d_tab;
    SplitFold fold = {};
    // buffers, grown on demand and kept
    DevBuf<uint8_t> d_text;                   // a host text's copy
    DevBuf<unsigned long long> d_sync, d_hi, d_hostmark;
    DevBuf<uint8_t> d_mask;
    DevBuf<unsigned long long> d_ctl;
    DevBuf<unsigned long long> d_list;        // cuts, ranges; host spans, then their chunk ends
    DevBuf<unsigned long long> d_cut, d_raw;  // split_docs: the cut bitmap, the bytes inside ranges
    DevBuf<unsigned long long> d_find;        // ... the occurrences of the names; the positions of the parts
    DevBuf<uint32_t> d_names;                 // ... the names as k_split_find takes them
    DevBuf<uint8_t> d_first;                  // ... the first byte of every part of a device text
    std::vector<SplitRange> ranges;           // the latest split_docs call's
    float find_ms = 0.f;
    std::vector<uint8_t> h_mask;              // the mask on the host, when offsets are asked for
    // the latest call
    float last_ms = 0.f;
    uint64_t last_n = 0, last_chunks = 0, last_host_spans = 0, last_host_bytes = 0;
    const uint8_t *last_text = nullptr;       // the text on the device
    bool have_mask = false;
};

namespace {

// adds the device time between the two events (both recorded, the stream idle) to the call's total
int add_ms(mbpe_splitter *s) {
    float ms = 0.f;
    SCHK(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    s->last_ms += ms;
    return MBPE_OK;
}

// what split_docs adds to a call: the documents and the names (checked by the caller)
struct DocArgs {
    const uint64_t *doc_off;
    uint64_t n_docs;
    const uint8_t *names;
    const uint32_t *name_off;
    uint32_t n_names;
};

constexpr uint64_t kFindListMin = 4096;       // entries the list of occurrences begins with

// the occurrences of the names in the text, ordered by (position, name)
int split_find(mbpe_splitter *s, const uint8_t *d_text, uint64_t n, const DocArgs &d, std::vector<uint64_t> *hits) {
    hits->clear();
    const uint32_t name_bytes = d.name_off[d.n_names];
    std::vector<uint32_t> blob(8 + d.n_names + 1 + (name_bytes + 3) / 4, 0u);
    split_first_set(d.names, d.name_off, d.n_names, blob.data());
    bool any = false;
    for (int i = 0; i < 8; ++i) any = any || blob[i];
    if (!any) return MBPE_OK;                  // no name, or empty ones only
    memcpy(blob.data() + 8, d.name_off, (d.n_names + 1) * 4);
    if (name_bytes) memcpy(blob.data() + 8 + d.n_names + 1, d.names, name_bytes);
    int rc = s->d_names.reserve((8 + kSplitMaxNames + 1) * 4 + kSplitMaxNameBytes, s->mem);
    if (rc == MBPE_OK && !s->d_find) rc = s->d_find.reserve(kFindListMin * 8, s->mem);
    if (rc != MBPE_OK) return rc;
    SCHK(hipMemcpyAsync(s->d_names, blob.data(), blob.size() * 4, hipMemcpyHostToDevice, s->stream));
    const uint64_t n_vec = (n + kSplitVec - 1) / kSplitVec;
    unsigned long long found = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        SCHK(hipEventRecord(s->ev0, s->stream));
        SCHK(hipMemsetAsync(s->d_ctl + kCtlFound, 0, 8, s->stream));
        hipLaunchKernelGGL(k_split_find, dim3(grid_for(n_vec)), dim3(kSplitThreads), 0, s->stream, d_text, n, n_vec,
                           s->d_names, d.n_names, name_bytes, s->d_find, s->d_find.bytes() / 8, s->d_ctl + kCtlFound);
        SCHK(hipGetLastError());
        SCHK(hipEventRecord(s->ev1, s->stream));
        SCHK(hipMemcpyAsync(&found, s->d_ctl + kCtlFound, 8, hipMemcpyDeviceToHost, s->stream));
        SCHK(hipStreamSynchronize(s->stream));
        float ms = 0.f;
        SCHK(hipEventElapsedTime(&ms, s->ev0, s->ev1));
        s->find_ms += ms;
        s->last_ms += ms;
        if (found <= s->d_find.bytes() / 8) break;
        if (attempt == 1) return fail(MBPE_ERR_HIP, "mbpe_splitter_split_docs: the list of occurrences changed size");
        rc = s->d_find.reserve(found * 8, s->mem);
        if (rc != MBPE_OK) return rc;
    }
    hits->resize(found);
    if (found) {
        SCHK(hipMemcpyAsync(hits->data(), s->d_find, found * 8, hipMemcpyDeviceToHost, s->stream));
        SCHK(hipStreamSynchronize(s->stream));
        std::sort(hits->begin(), hits->end());
    }
    return MBPE_OK;
}

// the passes; writes nothing the caller sees.  docs NULL: one text (mbpe_splitter_split)
int split_run_passes(mbpe_splitter *s, const uint8_t *text, uint64_t n, int text_on_device, const DocArgs *docs,
                     std::vector<SplitRange> *ranges, uint64_t *n_chunks) {
    const uint64_t n_words = (n + kSplitBlock - 1) / kSplitBlock, n_vec = (n + kSplitVec - 1) / kSplitVec;
    const uint64_t mask_bytes = (n_vec * 2 + 16 + 7) & ~7ull;
    int rc;
    if (!text_on_device) {
        if ((rc = s->d_text.reserve(n_vec * 16, s->mem)) != MBPE_OK) return rc;
        SCHK(hipMemcpyAsync(s->d_text, text, n, hipMemcpyHostToDevice, s->stream));
    }
    const uint8_t *d_text = text_on_device ? text : s->d_text;
    if ((rc = s->d_sync.reserve(n_words * 8, s->mem)) != MBPE_OK) return rc;
    if ((rc = s->d_hi.reserve(n_words * 8, s->mem)) != MBPE_OK) return rc;
    if ((rc = s->d_hostmark.reserve(n_words * 8, s->mem)) != MBPE_OK) return rc;
    if ((rc = s->d_mask.reserve(mask_bytes, s->mem)) != MBPE_OK) return rc;
    if (s->unicode && !s->d_tab) {
        std::string err;
        const mbpe_host::SplitUnicodeTable *tb = mbpe_host::split_unicode_table(&err);
        if (!tb) return fail(MBPE_ERR_REGEX, err);
        if ((rc = s->d_tab.reserve(kSplitTableWords * 4, s->mem)) != MBPE_OK) return rc;
        SCHK(hipMemcpy(s->d_tab, tb->cls.data(), kSplitTableWords * 4, hipMemcpyHostToDevice));
        s->fold.n = tb->n_fold;
        for (uint32_t k = 0; k < tb->n_fold; ++k) { s->fold.cp[k] = tb->fold_cp[k]; s->fold.to[k] = tb->fold_to[k]; }
    }
    s->have_mask = false;
    s->last_text = d_text;

    // split_docs: the occurrences taken, the parts between them, and from both the ranges and the cuts
    std::vector<uint64_t> hits, cuts, part_pos;
    std::vector<SplitRange> taken, parts;
    std::vector<uint8_t> first;
    ranges->clear();
    if (docs) {
        if (docs->n_names && (rc = split_find(s, d_text, n, *docs, &hits)) != MBPE_OK) return rc;
        split_plan_parts(hits.data(), hits.size(), docs->doc_off, docs->n_docs, docs->name_off, &taken, &parts);
        first.resize(parts.size());
        if (!text_on_device) {
            for (size_t k = 0; k < parts.size(); ++k) first[k] = text[parts[k].start];
        } else if (!parts.empty()) {
            part_pos.resize(parts.size());
            for (size_t k = 0; k < parts.size(); ++k) part_pos[k] = parts[k].start;
            if ((rc = s->d_find.reserve(parts.size() * 8, s->mem)) != MBPE_OK) return rc;
            if ((rc = s->d_first.reserve(parts.size(), s->mem)) != MBPE_OK) return rc;
            SCHK(hipMemcpyAsync(s->d_find, part_pos.data(), parts.size() * 8, hipMemcpyHostToDevice, s->stream));
            hipLaunchKernelGGL(k_split_gather, dim3(grid_for(parts.size())), dim3(kSplitThreads), 0, s->stream, d_text, n,
                               s->d_find, (uint64_t)parts.size(), s->d_first);
            SCHK(hipGetLastError());
            SCHK(hipMemcpyAsync(first.data(), s->d_first, parts.size(), hipMemcpyDeviceToHost, s->stream));
            SCHK(hipStreamSynchronize(s->stream));
        }
        split_plan_finish(taken, parts, first.data(), ranges, &cuts);
    }
    const bool have_cuts = !cuts.empty(), have_raw = !ranges->empty();
    std::vector<uint64_t> rng(2 * ranges->size());
    if (have_cuts || have_raw) {
        for (size_t k = 0; k < ranges->size(); ++k) { rng[2 * k] = (*ranges)[k].start; rng[2 * k + 1] = (*ranges)[k].len; }
        if ((rc = s->d_list.reserve((cuts.size() + rng.size()) * 8, s->mem)) != MBPE_OK) return rc;
        if (have_cuts && (rc = s->d_cut.reserve(n_words * 8, s->mem)) != MBPE_OK) return rc;
        if (have_raw && (rc = s->d_raw.reserve(n_words * 8, s->mem)) != MBPE_OK) return rc;
        if (have_cuts) SCHK(hipMemcpyAsync(s->d_list, cuts.data(), cuts.size() * 8, hipMemcpyHostToDevice, s->stream));
        if (have_raw)
            SCHK(hipMemcpyAsync(s->d_list + cuts.size(), rng.data(), rng.size() * 8, hipMemcpyHostToDevice, s->stream));
    }

    SCHK(hipEventRecord(s->ev0, s->stream));
    SCHK(hipMemsetAsync(s->d_mask, 0, mask_bytes, s->stream));
    SCHK(hipMemsetAsync(s->d_ctl, 0, kCtlWords * 8, s->stream));
    if (have_cuts) {
        SCHK(hipMemsetAsync(s->d_cut, 0, n_words * 8, s->stream));
        hipLaunchKernelGGL(k_split_patch, dim3(grid_for(cuts.size())), dim3(kSplitThreads), 0, s->stream, s->d_list,
                           (uint64_t)cuts.size(), n, reinterpret_cast<uint32_t *>(s->d_cut.get()));
    }
    if (have_raw) {
        SCHK(hipMemsetAsync(s->d_raw, 0, n_words * 8, s->stream));
        hipLaunchKernelGGL(k_split_raw, dim3(grid_for(ranges->size())), dim3(kSplitThreads), 0, s->stream,
                           s->d_list + cuts.size(), (uint64_t)ranges->size(), n, s->d_raw);
    }
    const unsigned long long *d_cut = have_cuts ? s->d_cut : nullptr, *d_raw = have_raw ? s->d_raw : nullptr;
    if (s->unicode) {
        hipLaunchKernelGGL(k_split_sync_u, dim3(grid_for(n_words * 4)), dim3(kSplitThreads), 0, s->stream, d_text, n,
                           n_words * 4, reinterpret_cast<const uint16_t *>(d_cut), s->pattern, s->d_tab,
                           reinterpret_cast<uint16_t *>(s->d_sync.get()), reinterpret_cast<uint16_t *>(s->d_hi.get()));
        hipLaunchKernelGGL(k_split_walk_u, dim3(grid_for(n_words)), dim3(kSplitThreads), 0, s->stream, d_text, n,
                           s->d_sync, s->d_hi, d_cut, d_raw, n_words, s->max_span, s->pattern, s->d_tab, s->fold,
                           reinterpret_cast<uint32_t *>(s->d_mask.get()), s->d_hostmark, s->d_ctl);
    } else {
        hipLaunchKernelGGL(k_split_sync, dim3(grid_for(n_words * 4)), dim3(kSplitThreads), 0, s->stream, d_text, n,
                           n_words * 4, reinterpret_cast<const uint16_t *>(d_cut), reinterpret_cast<uint16_t *>(s->d_sync.get()),
                           reinterpret_cast<uint16_t *>(s->d_hi.get()));
        hipLaunchKernelGGL(k_split_walk, dim3(grid_for(n_words)), dim3(kSplitThreads), 0, s->stream, d_text, n, s->d_sync,
                           s->d_hi, d_cut, d_raw, n_words, s->max_span, s->pattern,
                           reinterpret_cast<uint32_t *>(s->d_mask.get()), s->d_hostmark, s->d_ctl);
    }
    SCHK(hipGetLastError());
    SCHK(hipEventRecord(s->ev1, s->stream));
    unsigned long long ctl[kCtlWords] = {0, 0, 0, 0};
    SCHK(hipMemcpyAsync(ctl, s->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, s->stream));
    SCHK(hipStreamSynchronize(s->stream));
    if ((rc = add_ms(s)) != MBPE_OK) return rc;

    const uint64_t n_host = ctl[kCtlHost];
    uint64_t n_patch = 0;
    std::vector<uint64_t> ends;
    if (n_host) {
        if ((rc = s->d_list.reserve(n_host * 16, s->mem)) != MBPE_OK) return rc;
        SCHK(hipEventRecord(s->ev0, s->stream));
        hipLaunchKernelGGL(k_split_compact, dim3(grid_for(n_words)), dim3(kSplitThreads), 0, s->stream, s->d_sync,
                           s->d_hostmark, n, n_words, s->d_list, n_host, s->d_ctl);
        SCHK(hipGetLastError());
        SCHK(hipEventRecord(s->ev1, s->stream));
        std::vector<uint64_t> spans(2 * n_host);
        SCHK(hipMemcpyAsync(spans.data(), s->d_list, n_host * 16, hipMemcpyDeviceToHost, s->stream));
        SCHK(hipStreamSynchronize(s->stream));
        if ((rc = add_ms(s)) != MBPE_OK) return rc;

        // ascending, and neighbours joined into runs: [a, b) [b, c) is the run [a, c), unless b is a cut
        auto is_cut = [&](uint64_t p) { return std::binary_search(cuts.begin(), cuts.end(), p); };
        struct Span { uint64_t a, b; };
        Span *sp = reinterpret_cast<Span *>(spans.data());
        std::sort(sp, sp + n_host, [](const Span &x, const Span &y) { return x.a < y.a; });
        uint64_t n_runs = 0, host_bytes = 0;
        for (uint64_t i = 0; i < n_host; ++i) {
            if (sp[i].a >= sp[i].b || sp[i].b > n || (n_runs && sp[i].a < sp[n_runs - 1].b))
                return fail(MBPE_ERR_HIP, "mbpe_splitter_split: the device listed an impossible host span");
            host_bytes += sp[i].b - sp[i].a;
            if (n_runs && sp[n_runs - 1].b == sp[i].a && !is_cut(sp[i].a)) sp[n_runs - 1].b = sp[i].b;
            else sp[n_runs++] = sp[i];
        }
        s->last_host_spans = n_host;
        s->last_host_bytes = host_bytes;

        // the bytes PCRE2 reads: [a, min(b + 1, n)) of every run.  A device text comes back once, from the first
        // run to the last
        std::vector<uint8_t> back;
        const uint8_t *sub = text;
        uint64_t origin = 0;
        if (text_on_device) {
            origin = sp[0].a;
            const uint64_t to = std::min(sp[n_runs - 1].b + 1, n);
            back.resize(to - origin);
            SCHK(hipMemcpy(back.data(), text + origin, to - origin, hipMemcpyDeviceToHost));
            sub = back.data();
        }
        std::vector<uint8_t> end_is_cut;
        if (have_cuts) {
            end_is_cut.resize(n_runs);
            for (uint64_t i = 0; i < n_runs; ++i) end_is_cut[i] = is_cut(sp[i].b);
        }
        std::string err;
        rc = s->host.split_spans(sub, origin, n, spans.data(), n_runs, mbpe_host::split_thread_count(host_bytes), &ends, &err,
                                 have_cuts ? end_is_cut.data() : nullptr);
        if (rc != MBPE_OK) return fail(rc, err);
    }
    for (const SplitRange &r : *ranges) ends.push_back(r.start + r.len - 1);      // a range is one chunk
    n_patch = ends.size();
    if (n_patch) {
        if ((rc = s->d_list.reserve(n_patch * 8, s->mem)) != MBPE_OK) return rc;
        SCHK(hipMemcpyAsync(s->d_list, ends.data(), n_patch * 8, hipMemcpyHostToDevice, s->stream));
        SCHK(hipStreamSynchronize(s->stream));           // (ends is about to go)
    }

    SCHK(hipEventRecord(s->ev0, s->stream));
    if (n_patch)
        hipLaunchKernelGGL(k_split_patch, dim3(grid_for(n_patch)), dim3(kSplitThreads), 0, s->stream, s->d_list, n_patch,
                           n, reinterpret_cast<uint32_t *>(s->d_mask.get()));
    launch_mask_popcount(s->stream, s->d_mask, n, s->d_ctl + kCtlChunks);
    SCHK(hipGetLastError());
    SCHK(hipEventRecord(s->ev1, s->stream));
    SCHK(hipMemcpyAsync(ctl, s->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, s->stream));
    SCHK(hipStreamSynchronize(s->stream));
    if ((rc = add_ms(s)) != MBPE_OK) return rc;
    *n_chunks = ctl[kCtlChunks];
    s->have_mask = true;
    return MBPE_OK;
}

}  // namespace

extern "C" {

int mbpe_splitter_create(int device_id, const char *pattern, mbpe_splitter **out) {
    if (!pattern || !out) return fail(MBPE_ERR_ARG, "mbpe_splitter_create: NULL argument");
    int which = -1;
    if (!strcmp(pattern, mbpe_host::split_pattern_for("gpt2"))) which = kSplitGpt2;
    else if (!strcmp(pattern, mbpe_host::split_pattern_for("gpt4"))) which = kSplitGpt4;
    if (which < 0)
        return fail(MBPE_ERR_ARG, "the device split knows the built-in gpt2 and gpt4 patterns only (use mbpe_presplit)");
    if (find_device(device_id) != MBPE_OK) return MBPE_ERR_NO_DEVICE;
    mbpe_splitter *s = new mbpe_splitter;
    s->device = device_id;                    // (destroy selects it, also where the pattern fails before open)
    s->pattern = which;
    auto build = [&]() -> int {
        std::string err;
        int rc = s->host.compile(pattern, &err);
        if (rc != MBPE_OK) return fail(rc, err);
        if ((rc = s->open(device_id)) != MBPE_OK) return rc;
        return s->d_ctl.reserve(kCtlWords * 8, s->mem);
    };
    const int rc = build();
    if (rc != MBPE_OK) {
        const std::string keep = mbpe_host::last_error();
        mbpe_splitter_destroy(s);
        mbpe_host::set_last_error(keep);
        return rc;
    }
    *out = s;
    return MBPE_OK;
}

void mbpe_splitter_destroy(mbpe_splitter *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;                                 // the buffers, then the events, then the stream
}

int mbpe_splitter_set_option(mbpe_splitter *s, const char *name, int64_t value) {
    if (!s || !name) return fail(MBPE_ERR_ARG, "mbpe_splitter_set_option: NULL argument");
    if (!strcmp(name, "max_span") && value >= 1) { s->max_span = (uint64_t)value; return MBPE_OK; }
    if (!strcmp(name, "unicode") && (value == 0 || value == 1)) { s->unicode = value == 1; return MBPE_OK; }
    return fail(MBPE_ERR_ARG, std::string("mbpe_splitter_set_option: unknown option or bad value: ") + name);
}

// the part both split calls share: the state of a new call, then the passes (or the empty mask of an empty text)
static int split_call(mbpe_splitter *s, const uint8_t *text, uint64_t n_bytes, int text_on_device, const DocArgs *docs,
                      uint64_t *n_chunks) {
    SCHK(hipSetDevice(s->device));
    s->last_ms = s->find_ms = 0.f;
    s->last_n = n_bytes;
    s->last_chunks = s->last_host_spans = s->last_host_bytes = 0;
    s->last_text = nullptr;
    s->have_mask = false;
    s->ranges.clear();
    *n_chunks = 0;
    if (n_bytes) {
        std::vector<SplitRange> ranges;
        const int rc = split_run_passes(s, text, n_bytes, text_on_device, docs, &ranges, n_chunks);
        if (rc != MBPE_OK) return rc;
        s->ranges.swap(ranges);
    } else {
        const int rc = s->d_mask.reserve(16, s->mem);
        if (rc != MBPE_OK) return rc;
        SCHK(hipMemsetAsync(s->d_mask, 0, 16, s->stream));
        SCHK(hipStreamSynchronize(s->stream));
        s->have_mask = true;
    }
    s->last_chunks = *n_chunks;
    return MBPE_OK;
}

int mbpe_splitter_split(mbpe_splitter *s, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                        uint8_t *endmask_dev_out, uint64_t *chunk_off_out, uint64_t cap_chunks, uint64_t *n_chunks_out) {
    if (n_chunks_out) *n_chunks_out = 0;
    if (!s || !n_chunks_out || (!text && n_bytes)) return fail(MBPE_ERR_ARG, "mbpe_splitter_split: NULL argument");
    if ((text_on_device && ((uintptr_t)text & 15)) || ((uintptr_t)endmask_dev_out & 15))
        return fail(MBPE_ERR_ARG, "mbpe_splitter_split: device text and device mask must be 16-byte aligned");
    const uint64_t mask_bytes = (n_bytes + 15) / 16 * 2 + 16;
    uint64_t n_chunks = 0;
    try {
        const int rc = split_call(s, text, n_bytes, text_on_device, nullptr, &n_chunks);
        if (rc != MBPE_OK) return rc;
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_splitter_split: host allocation failed");
    }
    *n_chunks_out = n_chunks;
    if (chunk_off_out) {
        if (cap_chunks < n_chunks) return fail(MBPE_ERR_ARG, "mbpe_splitter_split: chunk_off_out is too small");
        // 1 bit per text byte comes back instead of 8 bytes per chunk; the offsets are read off the mask here
        s->h_mask.resize((n_bytes + 63) / 64 * 8);
        if (n_bytes) SCHK(hipMemcpy(s->h_mask.data(), s->d_mask, s->h_mask.size(), hipMemcpyDeviceToHost));
        uint64_t k = 0;
        chunk_off_out[k++] = 0;
        for (uint64_t w = 0; w < s->h_mask.size() / 8 && k <= n_chunks; ++w) {
            unsigned long long m;
            memcpy(&m, s->h_mask.data() + 8 * w, 8);
            for (; m && k <= n_chunks; m &= m - 1) chunk_off_out[k++] = (w << 6) + (uint64_t)__builtin_ctzll(m) + 1;
        }
        if (k != n_chunks + 1) return fail(MBPE_ERR_HIP, "mbpe_splitter_split: the mask and its count disagree");
    }
    if (endmask_dev_out) {
        SCHK(hipMemcpyAsync(endmask_dev_out, s->d_mask, mask_bytes, hipMemcpyDeviceToDevice, s->stream));
        SCHK(hipStreamSynchronize(s->stream));
    }
    return MBPE_OK;
}

int mbpe_splitter_split_docs(mbpe_splitter *s, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                             const uint64_t *doc_off, uint64_t n_docs, const uint8_t *names, const uint64_t *name_off,
                             uint32_t n_names, uint8_t *endmask_dev_out, mbpe_split_range *ranges_out,
                             uint64_t cap_ranges, uint64_t *n_ranges_out, uint64_t *n_chunks_out) {
    static_assert(sizeof(mbpe_split_range) == sizeof(SplitRange) && MBPE_SPLIT_RAW == kSplitRaw, "mbpe.h and split_rule.h");
    static_assert(MBPE_SPLIT_MAX_NAMES == kSplitMaxNames && MBPE_SPLIT_MAX_NAME_BYTES == kSplitMaxNameBytes, "... agree");
    if (n_chunks_out) *n_chunks_out = 0;
    if (n_ranges_out) *n_ranges_out = 0;
    if (!s || !n_chunks_out || (!text && n_bytes) || (!doc_off && n_docs) || (n_names && (!name_off || !names)))
        return fail(MBPE_ERR_ARG, "mbpe_splitter_split_docs: NULL argument");
    if ((text_on_device && ((uintptr_t)text & 15)) || ((uintptr_t)endmask_dev_out & 15))
        return fail(MBPE_ERR_ARG, "mbpe_splitter_split_docs: device text and device mask must be 16-byte aligned");
    if (n_docs == 0) n_bytes = 0;                                // no document: an empty result
    if (n_docs && (doc_off[0] != 0 || doc_off[n_docs] != n_bytes))
        return fail(MBPE_ERR_ARG, "mbpe_splitter_split_docs: doc_off must start at 0 and end at n_bytes");
    for (uint64_t i = 0; i < n_docs; ++i)
        if (doc_off[i + 1] < doc_off[i]) return fail(MBPE_ERR_ARG, "mbpe_splitter_split_docs: doc_off must be ascending");
    if (n_bytes >> (64 - kSplitNameBits)) return fail(MBPE_ERR_ARG, "mbpe_splitter_split_docs: the text is too long");
    if (n_names > kSplitMaxNames)
        return fail(MBPE_ERR_ARG, "mbpe_splitter_split_docs: more than " + std::to_string(kSplitMaxNames) + " names");
    if (n_names && name_off[0] != 0) return fail(MBPE_ERR_ARG, "mbpe_splitter_split_docs: name_off must start at 0");
    for (uint32_t j = 0; j < n_names; ++j)
        if (name_off[j + 1] < name_off[j] || name_off[j + 1] > kSplitMaxNameBytes)
            return fail(MBPE_ERR_ARG, "mbpe_splitter_split_docs: name_off must be ascending and end at no more than " +
                                          std::to_string(kSplitMaxNameBytes) + " bytes");
    const uint64_t mask_bytes = (n_bytes + 15) / 16 * 2 + 16;
    uint64_t n_chunks = 0;
    try {
        std::vector<uint32_t> off32(n_names + 1, 0u);
        for (uint32_t j = 0; j <= n_names && n_names; ++j) off32[j] = (uint32_t)name_off[j];
        const DocArgs docs = {doc_off, n_docs, names, off32.data(), n_names};
        const int rc = split_call(s, text, n_bytes, text_on_device, &docs, &n_chunks);
        if (rc != MBPE_OK) return rc;
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_splitter_split_docs: host allocation failed");
    }
    *n_chunks_out = n_chunks;
    if (n_ranges_out) *n_ranges_out = s->ranges.size();
    if (ranges_out) {
        if (cap_ranges < s->ranges.size()) return fail(MBPE_ERR_ARG, "mbpe_splitter_split_docs: ranges_out is too small");
        if (!s->ranges.empty()) memcpy(ranges_out, s->ranges.data(), s->ranges.size() * sizeof(SplitRange));
    }
    if (endmask_dev_out) {
        SCHK(hipMemcpyAsync(endmask_dev_out, s->d_mask, mask_bytes, hipMemcpyDeviceToDevice, s->stream));
        SCHK(hipStreamSynchronize(s->stream));
    }
    return MBPE_OK;
}

int mbpe_splitter_ranges(const mbpe_splitter *s, const mbpe_split_range **ranges_out, uint64_t *n_ranges_out) {
    if (!s || !ranges_out || !n_ranges_out) return fail(MBPE_ERR_ARG, "mbpe_splitter_ranges: NULL argument");
    if (!s->have_mask) return fail(MBPE_ERR_STATE, "mbpe_splitter_ranges: no split has succeeded yet");
    *ranges_out = reinterpret_cast<const mbpe_split_range *>(s->ranges.data());
    *n_ranges_out = s->ranges.size();
    return MBPE_OK;
}

int mbpe_splitter_find_ms(const mbpe_splitter *s, float *ms_out) {
    if (!s || !ms_out) return fail(MBPE_ERR_ARG, "mbpe_splitter_find_ms: NULL argument");
    *ms_out = s->find_ms;
    return MBPE_OK;
}

int mbpe_splitter_endmask(const mbpe_splitter *s, const uint8_t **endmask_dev_out, uint64_t *mask_bytes_out,
                          const uint8_t **text_dev_out) {
    if (!s || !endmask_dev_out) return fail(MBPE_ERR_ARG, "mbpe_splitter_endmask: NULL argument");
    if (!s->have_mask) return fail(MBPE_ERR_STATE, "mbpe_splitter_endmask: no split has succeeded yet");
    *endmask_dev_out = s->d_mask;
    if (mask_bytes_out) *mask_bytes_out = (s->last_n + 15) / 16 * 2 + 16;
    if (text_dev_out) *text_dev_out = s->last_text;
    return MBPE_OK;
}

int mbpe_splitter_kernel_ms(const mbpe_splitter *s, float *ms_out) {
    if (!s || !ms_out) return fail(MBPE_ERR_ARG, "mbpe_splitter_kernel_ms: NULL argument");
    *ms_out = s->last_ms;
    return MBPE_OK;
}

int mbpe_splitter_alloc_count(const mbpe_splitter *s, uint64_t *n_out) {
    if (!s || !n_out) return fail(MBPE_ERR_ARG, "mbpe_splitter_alloc_count: NULL argument");
    *n_out = s->mem.n_allocs;
    return MBPE_OK;
}

int mbpe_splitter_host_spans(const mbpe_splitter *s, uint64_t *n_spans_out, uint64_t *n_bytes_out) {
    if (!s || !n_spans_out) return fail(MBPE_ERR_ARG, "mbpe_splitter_host_spans: NULL argument");
    *n_spans_out = s->last_host_spans;
    if (n_bytes_out) *n_bytes_out = s->last_host_bytes;
    return MBPE_OK;
}

}  // extern "C"
