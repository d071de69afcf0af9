// Chunk deduplication on the device: see dedup.h.  gfx950, wave64.
//
// Passes over a text of n bytes whose chunk ends are a mask (bit i: byte i is the last of its chunk; 64 bytes = one
// mask word = one lane, 256 words = one tile):
//
//   k_dd_tile_count   end bits per tile                                      -> scan -> the chunks before each tile
//   k_dd_chunk_ends   ranked write of every chunk's end offset               (8 B per chunk)
//   k_dd_insert       one lane per chunk: hash, probe, claim or join; class counts through an LDS cache per workgroup
//                     (the table of dedup.h; 8 B home per chunk)
//   k_dd_first_count  per 256 chunks: first occurrences and their bytes      -> two scans -> n_unique, n_unique_bytes
//   k_dd_emit         the first occurrences' bytes (16-byte pieces where source and target are aligned alike), end
//                     mask, weights and first_chunk
//   k_dd_map          option "map" only: unique_of[c] of every chunk that is not a first occurrence, read from its
//                     representative's (k_dd_emit has written those)
//
// Bytes at and beyond n never count: mask bits there are cleared as the words are read.  Bytes behind the last end bit
// belong to no chunk and vanish.
#include "dedup.h"
#include "dedup_dev.h"
#include "hip_host.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <string.h>
#include <vector>

namespace mbpe {
namespace {

#define DCHK(expr) MBPE_HIP_CHECK(expr, false)

// what the host reads back
struct DdCtl { unsigned long long n_chunks, n_unique, n_unique_bytes, pad; };

struct DdTable {
    unsigned long long *slots;     // dedup_slot(tag, representative), kDedupEmpty when free
    uint32_t *cnts;                // members of the slot's class
    uint64_t mask;                 // capacity - 1
    uint32_t bits;
};

// where chunk c belongs in the table: the slot it claimed or joined (kDedupNoHome: unreachable, see below)
__device__ __forceinline__ unsigned long long dd_place(const uint8_t *__restrict__ text,
                                                       const unsigned long long *__restrict__ cend, const DdTable &t,
                                                       uint64_t c, uint64_t start, uint64_t len, uint32_t hash_bits) {
    const unsigned long long h = dedup_hash(text + start, len, hash_bits);
    const uint32_t tag = dedup_tag(h);
    const unsigned long long mine = dedup_slot(tag, c);
    uint64_t pos = dedup_home(h, t.bits);
    // (the table has at least 2 x n_chunks slots and a chunk occupies at most one: a free or a matching slot comes)
    for (uint64_t probe = 0; probe <= t.mask; ++probe, pos = (pos + 1) & t.mask) {
        // A load that may be served by this CU's cache: a slot word only ever goes from free to a class and then to
        // smaller representatives of that class, so a stale value is a free slot (the compare-and-swap below then
        // returns the truth) or an older representative with the same bytes.  The frequent chunks' slots stay cached.
        unsigned long long v = __hip_atomic_load(&t.slots[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (v == kDedupEmpty) {
            v = atomicCAS(&t.slots[pos], kDedupEmpty, mine);
            if (v == kDedupEmpty) v = mine;
        }
        bool same = v == mine;
        if (!same && dedup_tag(v) == tag) {
            uint64_t rs, rl;
            chunk_range(cend, v & 0xFFFFFFFFull, &rs, &rl);
            same = rl == len && dedup_equal(text + start, text + rs, len);
            // (the representative only falls: nothing to lower when the value seen is below this chunk already)
            if (same && mine < v) atomicMin(&t.slots[pos], mine);
        }
        if (same) return pos;
    }
    return kDedupNoHome;           // (unreachable; such a chunk would pass through, which is still exact)
}

// One lane per chunk, a workgroup over `per` consecutive chunks.  The class counts are what millions of chunks would
// otherwise add to a few thousand addresses one by one (the frequent words): a workgroup counts its share in an LDS
// cache keyed by the slot position -- kDdCacheSlots open-addressed entries, up to kDdCacheProbes probes, the key claimed
// with one 8-byte LDS compare-and-swap, as k_wide_pair_count_tokens does -- and adds every entry once at the end; a
// chunk that finds no entry adds to the table directly.
constexpr uint32_t kDdCacheSlots = 2048, kDdCacheProbes = 4;      // 16 KiB of keys + 8 KiB of counts
constexpr uint64_t kDdMaxPerBlock = 16384;
__global__ __launch_bounds__(kDdThreads) void k_dd_insert(const uint8_t *__restrict__ text,
                                                          const unsigned long long *__restrict__ cend, uint64_t n_chunks,
                                                          uint64_t per, DdTable t, uint32_t max_chunk, uint32_t hash_bits,
                                                          unsigned long long *__restrict__ home) {
    __shared__ unsigned long long ckey[kDdCacheSlots];
    __shared__ uint32_t ccnt[kDdCacheSlots];
    for (uint32_t i = threadIdx.x; i < kDdCacheSlots; i += kDdThreads) { ckey[i] = kDedupEmpty; ccnt[i] = 0; }
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < n_chunks ? lo + per : n_chunks;
    for (uint64_t c = lo + threadIdx.x; c < hi; c += kDdThreads) {
        uint64_t start, len;
        chunk_range(cend, c, &start, &len);
        const unsigned long long pos = len > max_chunk ? kDedupNoHome : dd_place(text, cend, t, c, start, len, hash_bits);
        home[c] = pos;
        if (pos == kDedupNoHome) continue;
        uint32_t h = (uint32_t)((pos * 0x9E3779B97F4A7C15ull) >> (64 - 11));
        static_assert(kDdCacheSlots == 1u << 11, "the shift above");
        bool done = false;
#pragma unroll
        for (uint32_t p = 0; p < kDdCacheProbes && !done; ++p) {
            unsigned long long k = ckey[h];
            if (k == kDedupEmpty) k = atomicCAS(&ckey[h], kDedupEmpty, pos);
            if (k == kDedupEmpty || k == pos) { atomicAdd(&ccnt[h], 1u); done = true; }
            h = (h + 1) & (kDdCacheSlots - 1);
        }
        if (!done) atomicAdd(&t.cnts[pos], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kDdCacheSlots; i += kDdThreads)
        if (ckey[i] != kDedupEmpty) atomicAdd(&t.cnts[ckey[i]], ccnt[i]);
}

// is chunk c the first occurrence of its bytes?  (after k_dd_insert has finished)
__device__ __forceinline__ bool is_first(const unsigned long long *__restrict__ home, const DdTable &t, uint64_t c) {
    const unsigned long long p = home[c];
    return p == kDedupNoHome || (t.slots[p] & 0xFFFFFFFFull) == c;
}

__global__ __launch_bounds__(kDdThreads) void k_dd_first_count(const unsigned long long *__restrict__ cend,
                                                               const unsigned long long *__restrict__ home, DdTable t,
                                                               uint64_t n_chunks, unsigned long long *__restrict__ blk_cnt,
                                                               unsigned long long *__restrict__ blk_bytes) {
    __shared__ unsigned long long sh[kDdWaves];
    const uint64_t c = (uint64_t)blockIdx.x * kDdThreads + threadIdx.x;
    uint64_t start = 0, len = 0;
    bool first = false;
    if (c < n_chunks) {
        chunk_range(cend, c, &start, &len);
        first = is_first(home, t, c);
    }
    unsigned long long n, b;
    block_excl(first ? 1ull : 0ull, sh, &n);
    block_excl(first ? len : 0ull, sh, &b);
    if (threadIdx.x == 0) { blk_cnt[blockIdx.x] = n; blk_bytes[blockIdx.x] = b; }
}

__global__ __launch_bounds__(kDdThreads) void k_dd_emit(const uint8_t *__restrict__ text,
                                                        const unsigned long long *__restrict__ cend,
                                                        const unsigned long long *__restrict__ home, DdTable t,
                                                        uint64_t n_chunks, const unsigned long long *__restrict__ blk_cnt,
                                                        const unsigned long long *__restrict__ blk_bytes,
                                                        const unsigned long long *__restrict__ remap, uint64_t n_unique,
                                                        uint64_t n_unique_bytes, uint8_t *__restrict__ out_text,
                                                        uint32_t *__restrict__ out_mask, uint32_t *__restrict__ weights,
                                                        unsigned long long *__restrict__ first_chunk,
                                                        uint32_t *__restrict__ unique_of) {
    __shared__ unsigned long long sh[kDdWaves];
    const uint64_t c = (uint64_t)blockIdx.x * kDdThreads + threadIdx.x;
    uint64_t start = 0, len = 0;
    bool first = false;
    if (c < n_chunks) {
        chunk_range(cend, c, &start, &len);
        first = is_first(home, t, c);
    }
    unsigned long long tot;
    const uint64_t j = blk_cnt[blockIdx.x] + block_excl(first ? 1ull : 0ull, sh, &tot);
    const uint64_t o = blk_bytes[blockIdx.x] + block_excl(first ? len : 0ull, sh, &tot);
    if (!first || j >= n_unique || o + len > n_unique_bytes) return;      // (the counts' own flags: never beyond)
    const unsigned long long p = home[c];
    weights[j] = p == kDedupNoHome ? 1u : t.cnts[p];
    first_chunk[j] = remap ? remap[c] : c;
    if (unique_of) unique_of[c] = (uint32_t)j;
    copy_chunk(out_text + o, text + start, o, start, len);      // (text and out_text are 16-byte aligned)
    const uint64_t e = o + len - 1;
    atomicOr(&out_mask[e >> 5], 1u << (e & 31));
}

// option "map": the chunks that are not a first occurrence take their representative's index among the unique chunks
// (k_dd_emit wrote it; a representative's entry is not written here, so reads and writes never meet)
__global__ __launch_bounds__(kDdThreads) void k_dd_map(const unsigned long long *__restrict__ home, DdTable t,
                                                       uint64_t n_chunks, uint32_t *__restrict__ unique_of) {
    const uint64_t c = (uint64_t)blockIdx.x * kDdThreads + threadIdx.x;
    if (c >= n_chunks) return;
    const unsigned long long p = home[c];
    if (p == kDedupNoHome) return;                 // passes through: its own representative
    const uint64_t rep = t.slots[p] & 0xFFFFFFFFull;
    if (rep != c && rep < n_chunks) unique_of[c] = unique_of[rep];
}

}  // namespace
}  // namespace mbpe

using namespace mbpe;

struct mbpe_dedup : DevQueue {
    mbpe_dedup() : DevQueue(false) {}
    uint32_t max_chunk = kDedupMaxChunkBytes, hash_bits = 64;
    DevBuf<uint8_t> d_text_in, d_mask_in;                 // mbpe_dedup_chunks: the uploaded text, the mask built for it
    DevBuf<unsigned long long> d_remap;                   //   and, with empty chunks, the input index of each kept chunk
    DevBuf<unsigned long long> d_tile, d_cend, d_home, d_slots, d_blk, d_ctl;
    DevBuf<uint32_t> d_cnts;
    DevBuf<uint8_t> d_out_text, d_out_mask;
    DevBuf<uint32_t> d_weights;
    DevBuf<unsigned long long> d_first;
    DevBuf<uint32_t> d_unique_of;                         // option "map": the unique chunk of every kept chunk
    bool want_map = false, have_map = false;
    uint64_t n_chunks = 0, n_unique = 0, n_unique_bytes = 0;
    bool have = false;
    float last_ms = 0.f;
};

namespace {

int dd_add_ms(mbpe_dedup *d) {
    float ms = 0.f;
    DCHK(hipEventElapsedTime(&ms, d->ev0, d->ev1));
    d->last_ms += ms;
    return MBPE_OK;
}

// text and mask on the device; remap: NULL, or n_chunks input indices on the device
int dd_run(mbpe_dedup *d, const uint8_t *text, uint64_t n_bytes, const uint8_t *mask, const unsigned long long *remap) {
    int rc;
    d->have = d->have_map = false;
    d->last_ms = 0.f;
    d->n_chunks = d->n_unique = d->n_unique_bytes = 0;
    const uint32_t *m32 = reinterpret_cast<const uint32_t *>(mask);
    const uint64_t n_words = (n_bytes + 63) / 64, n_tiles = blocks_for(n_words);
    if ((rc = d->d_ctl.reserve(sizeof(DdCtl), d->mem)) != MBPE_OK) return rc;
    DdCtl ctl = {};
    DCHK(hipMemsetAsync(d->d_ctl, 0, sizeof(DdCtl), d->stream));
    DdCtl *dctl = reinterpret_cast<DdCtl *>(d->d_ctl.get());
    if (n_words) {
        if ((rc = d->d_tile.reserve(n_tiles * 8, d->mem)) != MBPE_OK) return rc;
        DCHK(hipEventRecord(d->ev0, d->stream));
        hipLaunchKernelGGL(k_dd_tile_count, dim3((uint32_t)n_tiles), dim3(kDdThreads), 0, d->stream, m32, n_bytes, n_words,
                           d->d_tile.get());
        hipLaunchKernelGGL(k_dd_scan, dim3(1), dim3(kScanThreads), 0, d->stream, d->d_tile.get(), n_tiles, &dctl->n_chunks);
        DCHK(hipGetLastError());
        DCHK(hipEventRecord(d->ev1, d->stream));
        DCHK(hipMemcpyAsync(&ctl, d->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, d->stream));
        DCHK(hipStreamSynchronize(d->stream));
        if ((rc = dd_add_ms(d)) != MBPE_OK) return rc;
    }
    const uint64_t n_chunks = ctl.n_chunks;
    if (n_chunks >= 0xFFFFFFFFull) return fail(MBPE_ERR_ARG, "dedup: 2^32 - 1 chunks or more");
    d->n_chunks = n_chunks;
    if (n_chunks) {
        const uint32_t n_blk = blocks_for(n_chunks);
        DdTable t = {};
        t.bits = dedup_table_bits(n_chunks);
        t.mask = (1ull << t.bits) - 1;
        if ((rc = d->d_cend.reserve(n_chunks * 8, d->mem)) != MBPE_OK) return rc;
        if ((rc = d->d_home.reserve(n_chunks * 8, d->mem)) != MBPE_OK) return rc;
        if ((rc = d->d_slots.reserve((t.mask + 1) * 8, d->mem)) != MBPE_OK) return rc;
        if ((rc = d->d_cnts.reserve((t.mask + 1) * 4, d->mem)) != MBPE_OK) return rc;
        if ((rc = d->d_blk.reserve((uint64_t)n_blk * 16, d->mem)) != MBPE_OK) return rc;
        t.slots = d->d_slots;
        t.cnts = d->d_cnts;
        unsigned long long *blk_cnt = d->d_blk, *blk_bytes = d->d_blk.get() + n_blk;
        DCHK(hipEventRecord(d->ev0, d->stream));
        DCHK(hipMemsetAsync(t.slots, 0xFF, (t.mask + 1) * 8, d->stream));
        DCHK(hipMemsetAsync(t.cnts, 0, (t.mask + 1) * 4, d->stream));
        hipLaunchKernelGGL(k_dd_chunk_ends, dim3((uint32_t)n_tiles), dim3(kDdThreads), 0, d->stream, m32, n_bytes, n_words,
                           d->d_tile.get(), n_chunks, d->d_cend.get());
        // a workgroup's share: about 2,048 workgroups, 256 .. kDdMaxPerBlock chunks each (a multiple of 256)
        const uint64_t per = std::max<uint64_t>(kDdThreads, std::min<uint64_t>(kDdMaxPerBlock, (n_chunks / 2048 + kDdThreads - 1) / kDdThreads * kDdThreads));
        hipLaunchKernelGGL(k_dd_insert, dim3((uint32_t)((n_chunks + per - 1) / per)), dim3(kDdThreads), 0, d->stream, text,
                           d->d_cend.get(), n_chunks, per, t, d->max_chunk, d->hash_bits, d->d_home.get());
        hipLaunchKernelGGL(k_dd_first_count, dim3(n_blk), dim3(kDdThreads), 0, d->stream, d->d_cend.get(), d->d_home.get(), t,
                           n_chunks, blk_cnt, blk_bytes);
        hipLaunchKernelGGL(k_dd_scan, dim3(1), dim3(kScanThreads), 0, d->stream, blk_cnt, (uint64_t)n_blk, &dctl->n_unique);
        hipLaunchKernelGGL(k_dd_scan, dim3(1), dim3(kScanThreads), 0, d->stream, blk_bytes, (uint64_t)n_blk,
                           &dctl->n_unique_bytes);
        DCHK(hipGetLastError());
        DCHK(hipEventRecord(d->ev1, d->stream));
        DCHK(hipMemcpyAsync(&ctl, d->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, d->stream));
        DCHK(hipStreamSynchronize(d->stream));
        if ((rc = dd_add_ms(d)) != MBPE_OK) return rc;
        if (!ctl.n_unique || ctl.n_unique > n_chunks || ctl.n_unique_bytes > n_bytes || ctl.n_unique_bytes < ctl.n_unique)
            return fail(MBPE_ERR_HIP, "dedup: the device counted impossible unique chunks");
        const uint64_t out_mask_bytes = mask_bytes_for(ctl.n_unique_bytes);
        if ((rc = d->d_out_text.reserve((ctl.n_unique_bytes + 15) / 16 * 16, d->mem)) != MBPE_OK) return rc;
        if ((rc = d->d_out_mask.reserve(out_mask_bytes, d->mem)) != MBPE_OK) return rc;
        if ((rc = d->d_weights.reserve(ctl.n_unique * 4, d->mem)) != MBPE_OK) return rc;
        if ((rc = d->d_first.reserve(ctl.n_unique * 8, d->mem)) != MBPE_OK) return rc;
        if (d->want_map && (rc = d->d_unique_of.reserve(n_chunks * 4, d->mem)) != MBPE_OK) return rc;
        uint32_t *unique_of = d->want_map ? d->d_unique_of.get() : nullptr;
        DCHK(hipEventRecord(d->ev0, d->stream));
        DCHK(hipMemsetAsync(d->d_out_mask, 0, out_mask_bytes, d->stream));
        hipLaunchKernelGGL(k_dd_emit, dim3(n_blk), dim3(kDdThreads), 0, d->stream, text, d->d_cend.get(), d->d_home.get(), t,
                           n_chunks, blk_cnt, blk_bytes, remap, (uint64_t)ctl.n_unique, (uint64_t)ctl.n_unique_bytes,
                           d->d_out_text.get(), reinterpret_cast<uint32_t *>(d->d_out_mask.get()), d->d_weights.get(),
                           d->d_first.get(), unique_of);
        if (unique_of)
            hipLaunchKernelGGL(k_dd_map, dim3(n_blk), dim3(kDdThreads), 0, d->stream, d->d_home.get(), t, n_chunks, unique_of);
        DCHK(hipGetLastError());
        DCHK(hipEventRecord(d->ev1, d->stream));
        DCHK(hipStreamSynchronize(d->stream));
        if ((rc = dd_add_ms(d)) != MBPE_OK) return rc;
        d->n_unique = ctl.n_unique;
        d->n_unique_bytes = ctl.n_unique_bytes;
    } else {
        // nothing: an empty text with an all-zero mask, so that the views stay valid device pointers
        if ((rc = d->d_out_text.reserve(16, d->mem)) != MBPE_OK) return rc;
        if ((rc = d->d_out_mask.reserve(16, d->mem)) != MBPE_OK) return rc;
        if ((rc = d->d_weights.reserve(16, d->mem)) != MBPE_OK) return rc;
        if ((rc = d->d_first.reserve(16, d->mem)) != MBPE_OK) return rc;
        if (d->want_map && (rc = d->d_unique_of.reserve(16, d->mem)) != MBPE_OK) return rc;
        DCHK(hipMemsetAsync(d->d_out_mask, 0, 16, d->stream));
        DCHK(hipStreamSynchronize(d->stream));
    }
    d->have = true;
    d->have_map = d->want_map;
    return MBPE_OK;
}

}  // namespace

extern "C" {

int mbpe_dedup_create(int device_id, mbpe_dedup **out) {
    if (!out) return fail(MBPE_ERR_ARG, "mbpe_dedup_create: NULL argument");
    if (find_device(device_id) != MBPE_OK) return MBPE_ERR_NO_DEVICE;
    mbpe_dedup *d = new (std::nothrow) mbpe_dedup;
    if (!d) return fail(MBPE_ERR_OOM, "mbpe_dedup_create: host allocation failed");
    d->device = device_id;
    const int rc = d->open(device_id);
    if (rc != MBPE_OK) {
        const std::string keep = mbpe_host::last_error();
        mbpe_dedup_destroy(d);
        mbpe_host::set_last_error(keep);
        return rc;
    }
    *out = d;
    return MBPE_OK;
}

void mbpe_dedup_destroy(mbpe_dedup *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    delete d;                                     // the buffers, then the events, then the stream
}

int mbpe_dedup_set_option(mbpe_dedup *d, const char *name, int64_t value) {
    if (!d || !name) return fail(MBPE_ERR_ARG, "mbpe_dedup_set_option: NULL argument");
    if (!strcmp(name, "max_chunk_bytes") && value >= 0 && value <= 0x7FFFFFFF) { d->max_chunk = (uint32_t)value; return MBPE_OK; }
    if (!strcmp(name, "hash_bits") && value >= 0 && value <= 64) { d->hash_bits = (uint32_t)value; return MBPE_OK; }
    if (!strcmp(name, "map") && (value == 0 || value == 1)) { d->want_map = value == 1; return MBPE_OK; }
    return fail(MBPE_ERR_ARG, std::string("mbpe_dedup_set_option: unknown option or bad value: ") + name);
}

int mbpe_dedup_chunks_endmask(mbpe_dedup *d, const uint8_t *text_dev, uint64_t n_bytes, const uint8_t *endmask_dev,
                              uint64_t *n_unique_out, uint64_t *n_unique_bytes_out) {
    if (n_unique_out) *n_unique_out = 0;
    if (n_unique_bytes_out) *n_unique_bytes_out = 0;
    if (!d || !n_unique_out || (n_bytes && (!text_dev || !endmask_dev)))
        return fail(MBPE_ERR_ARG, "mbpe_dedup_chunks_endmask: NULL argument");
    if (((uintptr_t)text_dev & 15) || ((uintptr_t)endmask_dev & 3))
        return fail(MBPE_ERR_ARG, "mbpe_dedup_chunks_endmask: device text must be 16-byte aligned, the end mask 4-byte aligned");
    DCHK(hipSetDevice(d->device));
    const int rc = dd_run(d, text_dev, n_bytes, endmask_dev, nullptr);
    if (rc != MBPE_OK) return rc;
    *n_unique_out = d->n_unique;
    if (n_unique_bytes_out) *n_unique_bytes_out = d->n_unique_bytes;
    return MBPE_OK;
}

int mbpe_dedup_chunks(mbpe_dedup *d, const uint8_t *text, uint64_t n_bytes, int text_on_device, const uint64_t *chunk_off,
                      uint64_t n_chunks, uint64_t *n_unique_out, uint64_t *n_unique_bytes_out) {
    if (n_unique_out) *n_unique_out = 0;
    if (n_unique_bytes_out) *n_unique_bytes_out = 0;
    if (!d || !n_unique_out || (!text && n_bytes) || !chunk_off)
        return fail(MBPE_ERR_ARG, "mbpe_dedup_chunks: NULL argument");
    if (n_chunks >= 0xFFFFFFFFull) return fail(MBPE_ERR_ARG, "mbpe_dedup_chunks: 2^32 - 1 chunks or more");
    if (chunk_off[0] != 0 || chunk_off[n_chunks] != n_bytes)
        return fail(MBPE_ERR_ARG, "mbpe_dedup_chunks: chunk_off must start at 0 and end at n_bytes");
    for (uint64_t i = 0; i < n_chunks; ++i)
        if (chunk_off[i] > chunk_off[i + 1]) return fail(MBPE_ERR_ARG, "mbpe_dedup_chunks: chunk_off must be ascending");
    if (text_on_device && ((uintptr_t)text & 15))
        return fail(MBPE_ERR_ARG, "mbpe_dedup_chunks: device text must be 16-byte aligned");
    try {
        const uint64_t mask_bytes = mask_bytes_for(n_bytes);
        std::vector<uint8_t> mask(mask_bytes, 0);
        uint64_t n_kept = 0;
        for (uint64_t ci = 0; ci < n_chunks; ++ci) {
            const uint64_t s = chunk_off[ci], e = chunk_off[ci + 1];
            if (e == s) continue;                 // an empty chunk vanishes
            mask[(e - 1) >> 3] |= (uint8_t)(1u << ((e - 1) & 7));
            ++n_kept;
        }
        // with empty chunks among them, the kept chunks' indices in the input: first_chunk speaks of those
        const bool need_map = n_kept != n_chunks && n_kept;
        std::vector<unsigned long long> kept;
        if (need_map) {
            kept.reserve(n_kept);
            for (uint64_t ci = 0; ci < n_chunks; ++ci)
                if (chunk_off[ci + 1] != chunk_off[ci]) kept.push_back(ci);
        }
        DCHK(hipSetDevice(d->device));
        int rc;
        const uint8_t *d_text = text;
        if (!text_on_device) {
            if ((rc = d->d_text_in.reserve(std::max<uint64_t>((n_bytes + 15) / 16 * 16, 16), d->mem)) != MBPE_OK) return rc;
            if (n_bytes) DCHK(hipMemcpyAsync(d->d_text_in, text, n_bytes, hipMemcpyHostToDevice, d->stream));
            d_text = d->d_text_in;
        }
        if ((rc = d->d_mask_in.reserve(mask_bytes, d->mem)) != MBPE_OK) return rc;
        DCHK(hipMemcpyAsync(d->d_mask_in, mask.data(), mask_bytes, hipMemcpyHostToDevice, d->stream));
        if (need_map) {
            if ((rc = d->d_remap.reserve(n_kept * 8, d->mem)) != MBPE_OK) return rc;
            DCHK(hipMemcpyAsync(d->d_remap, kept.data(), n_kept * 8, hipMemcpyHostToDevice, d->stream));
        }
        DCHK(hipStreamSynchronize(d->stream));    // (mask and kept are about to go)
        rc = dd_run(d, d_text, n_bytes, d->d_mask_in, need_map ? d->d_remap.get() : nullptr);
        if (rc != MBPE_OK) return rc;
        if (d->n_chunks != n_kept) {
            d->have = false;
            return fail(MBPE_ERR_HIP, "mbpe_dedup_chunks: the mask and the chunk count disagree");
        }
    } catch (const std::bad_alloc &) {
        return fail(MBPE_ERR_OOM, "mbpe_dedup_chunks: host allocation failed");
    }
    *n_unique_out = d->n_unique;
    if (n_unique_bytes_out) *n_unique_bytes_out = d->n_unique_bytes;
    return MBPE_OK;
}

int mbpe_dedup_result(const mbpe_dedup *d, const uint8_t **text_dev_out, const uint8_t **endmask_dev_out,
                      const uint32_t **weights_dev_out, const uint64_t **first_chunk_dev_out) {
    if (!d) return fail(MBPE_ERR_ARG, "mbpe_dedup_result: NULL argument");
    if (!d->have) return fail(MBPE_ERR_STATE, "mbpe_dedup_result: no dedup has succeeded yet");
    if (text_dev_out) *text_dev_out = d->d_out_text;
    if (endmask_dev_out) *endmask_dev_out = d->d_out_mask;
    if (weights_dev_out) *weights_dev_out = d->d_weights;
    if (first_chunk_dev_out) *first_chunk_dev_out = reinterpret_cast<const uint64_t *>(d->d_first.get());
    return MBPE_OK;
}

int mbpe_dedup_get(mbpe_dedup *d, uint8_t *text_out, uint64_t *chunk_off_out, uint32_t *weights_out,
                   uint64_t *first_chunk_out, uint64_t cap_bytes, uint64_t cap_chunks) {
    if (!d) return fail(MBPE_ERR_ARG, "mbpe_dedup_get: NULL argument");
    if (!d->have) return fail(MBPE_ERR_STATE, "mbpe_dedup_get: no dedup has succeeded yet");
    if (text_out && cap_bytes < d->n_unique_bytes) return fail(MBPE_ERR_ARG, "mbpe_dedup_get: text_out is too small");
    if ((chunk_off_out || weights_out || first_chunk_out) && cap_chunks < d->n_unique)
        return fail(MBPE_ERR_ARG, "mbpe_dedup_get: the chunk arrays are too small");
    DCHK(hipSetDevice(d->device));
    const uint64_t nu = d->n_unique, nb = d->n_unique_bytes;
    if (text_out && nb) DCHK(hipMemcpy(text_out, d->d_out_text, nb, hipMemcpyDeviceToHost));
    if (weights_out && nu) DCHK(hipMemcpy(weights_out, d->d_weights, nu * 4, hipMemcpyDeviceToHost));
    if (first_chunk_out && nu) DCHK(hipMemcpy(first_chunk_out, d->d_first, nu * 8, hipMemcpyDeviceToHost));
    if (chunk_off_out) {
        try {
            std::vector<uint8_t> m((nb + 63) / 64 * 8);
            if (nb) DCHK(hipMemcpy(m.data(), d->d_out_mask, m.size(), hipMemcpyDeviceToHost));
            uint64_t k = 0;
            chunk_off_out[k++] = 0;
            for (uint64_t w = 0; w < m.size() / 8 && k <= nu; ++w) {
                unsigned long long v;
                memcpy(&v, m.data() + 8 * w, 8);
                for (; v && k <= nu; v &= v - 1) chunk_off_out[k++] = (w << 6) + (uint64_t)__builtin_ctzll(v) + 1;
            }
            if (k != nu + 1) return fail(MBPE_ERR_HIP, "mbpe_dedup_get: the mask and its count disagree");
        } catch (const std::bad_alloc &) {
            return fail(MBPE_ERR_OOM, "mbpe_dedup_get: host allocation failed");
        }
    }
    return MBPE_OK;
}

int mbpe_dedup_map(const mbpe_dedup *d, const uint32_t **unique_of_dev_out, uint64_t *n_chunks_out) {
    if (!d) return fail(MBPE_ERR_ARG, "mbpe_dedup_map: NULL argument");
    if (!d->have) return fail(MBPE_ERR_STATE, "mbpe_dedup_map: no dedup has succeeded yet");
    if (!d->have_map) return fail(MBPE_ERR_STATE, "mbpe_dedup_map: the latest dedup ran without the option \"map\"");
    if (unique_of_dev_out) *unique_of_dev_out = d->d_unique_of;
    if (n_chunks_out) *n_chunks_out = d->n_chunks;
    return MBPE_OK;
}

int mbpe_dedup_get_map(mbpe_dedup *d, uint32_t *unique_of_out, uint64_t cap_chunks, uint64_t *n_chunks_out) {
    const uint32_t *src = nullptr;
    uint64_t n = 0;
    const int rc = mbpe_dedup_map(d, &src, &n);
    if (rc != MBPE_OK) return rc;
    if (n_chunks_out) *n_chunks_out = n;
    if (!unique_of_out) return MBPE_OK;
    if (cap_chunks < n) return fail(MBPE_ERR_ARG, "mbpe_dedup_get_map: unique_of_out is too small");
    DCHK(hipSetDevice(d->device));
    if (n) DCHK(hipMemcpy(unique_of_out, src, n * 4, hipMemcpyDeviceToHost));
    return MBPE_OK;
}

int mbpe_dedup_kernel_ms(const mbpe_dedup *d, float *ms_out) {
    if (!d || !ms_out) return fail(MBPE_ERR_ARG, "mbpe_dedup_kernel_ms: NULL argument");
    *ms_out = d->last_ms;
    return MBPE_OK;
}

int mbpe_dedup_alloc_count(const mbpe_dedup *d, uint64_t *n_out) {
    if (!d || !n_out) return fail(MBPE_ERR_ARG, "mbpe_dedup_alloc_count: NULL argument");
    *n_out = d->mem.n_allocs;
    return MBPE_OK;
}

}  // extern "C"
