// Word counts across calls on the device: see wordcount.h.  gfx950, wave64.
//
// A piece runs through the owned deduper (dedup.hip); nu unique chunks come out as a text with an end mask, u32 weights
// and first_chunk.  The fold into the accumulated table, on this object's own stream:
//
//   k_dd_tile_count, k_dd_scan, k_dd_chunk_ends   the piece's end mask -> the end offset of each of its unique chunks
//   k_wc_rehash     only when the table has to grow: every hashed entry claims a slot of the new, empty table
//   k_wc_lookup     one lane per unique chunk of the piece, read-only on the table: found -> its entry's weight grows;
//                   not found, or above "max_chunk_bytes" -> flagged new; per 256 chunks the new ones and their bytes
//   k_dd_scan x 2   -> the new chunks and bytes before each workgroup, the totals (the call's one readback)
//   k_wc_append     the new chunks' bytes (16-byte pieces where source and target are aligned alike), ends, weights,
//                   first_chunk, and one compare-and-swap each for a free slot
//
// The order between them is the order of the kernels on the stream; nothing else is needed.
//
// A merge folds another table instead of a piece: the same steps from k_wc_rehash on, with the table's own u64 ends and
// weights (k_wc_lookup and k_wc_append are templates over the weight type).  A table that arrives as a blob is checked
// first -- wordcount_blob_check on the host, then k_wc_distinct on the device: the incoming hashed chunks claim slots of
// a scratch table, and a chunk that meets its own bytes there raises a flag -- and only then does a weight change.
#include "wordcount.h"
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

#define WCHK(expr) MBPE_HIP_CHECK(expr, false)

// what the host reads back after the lookup
struct WcCtl { unsigned long long n_ends, n_new, n_new_bytes, piece_chunks, overflow, dup; };

struct WcTable {
    unsigned long long *slots;     // dedup_slot(tag, entry), kDedupEmpty when free
    uint64_t mask;                 // capacity - 1
    uint32_t bits;
};

// the accumulated entries
struct WcAcc {
    uint8_t *text;
    unsigned long long *ends, *weights, *first;
    uint64_t n, n_bytes;
};

// a free slot on h's probe sequence for `entry`.  The table has at least twice as many slots as entries: one comes
__device__ __forceinline__ void wc_claim(const WcTable &t, unsigned long long h, uint64_t entry) {
    const unsigned long long mine = dedup_slot(dedup_tag(h), entry);
    uint64_t pos = dedup_home(h, t.bits);
    for (uint64_t probe = 0; probe <= t.mask; ++probe, pos = (pos + 1) & t.mask)
        if (atomicCAS(&t.slots[pos], kDedupEmpty, mine) == kDedupEmpty) return;
}

__global__ __launch_bounds__(kDdThreads) void k_wc_rehash(WcAcc a, WcTable t, uint32_t max_chunk, uint32_t hash_bits) {
    const uint64_t e = (uint64_t)blockIdx.x * kDdThreads + threadIdx.x;
    if (e >= a.n) return;
    uint64_t start, len;
    chunk_range(a.ends, e, &start, &len);
    if (len <= max_chunk) wc_claim(t, dedup_hash(a.text + start, len, hash_bits), e);
}

// The piece's unique chunks that were hashed are pairwise distinct -- the owned deduper runs with this object's
// "max_chunk_bytes", so every chunk at or below it occurs once in the piece's result -- hence no two lanes find the same
// entry and the weight is updated with a plain load and store.
// (W: uint32_t for a piece out of the deduper, unsigned long long for a table that is merged)
template <typename W>
__global__ __launch_bounds__(kDdThreads) void k_wc_lookup(const uint8_t *__restrict__ ptext,
                                                          const unsigned long long *__restrict__ pend,
                                                          const W *__restrict__ pweights, uint64_t nu, uint32_t repeat,
                                                          WcAcc a, WcTable t, uint32_t max_chunk, uint32_t hash_bits,
                                                          unsigned long long *__restrict__ hash_out,
                                                          uint8_t *__restrict__ new_out,
                                                          unsigned long long *__restrict__ blk_cnt,
                                                          unsigned long long *__restrict__ blk_bytes, WcCtl *ctl) {
    __shared__ unsigned long long sh[kDdWaves];
    const uint64_t j = (uint64_t)blockIdx.x * kDdThreads + threadIdx.x;
    uint64_t start = 0, len = 0;
    unsigned long long w = 0;
    bool is_new = false, over = false;
    if (j < nu) {
        chunk_range(pend, j, &start, &len);
        w = pweights[j];
        const unsigned long long add_w = wordcount_sat_mul(w, repeat);
        over = add_w >= kWordcountWeightLimit;
        is_new = true;
        if (len <= max_chunk) {
            const unsigned long long h = dedup_hash(ptext + start, len, hash_bits);
            const uint32_t tag = dedup_tag(h);
            hash_out[j] = h;
            uint64_t pos = dedup_home(h, t.bits);
            for (uint64_t probe = 0; probe <= t.mask; ++probe, pos = (pos + 1) & t.mask) {
                const unsigned long long v = t.slots[pos];
                if (v == kDedupEmpty) break;
                if (dedup_tag(v) != tag) continue;
                const uint64_t e = v & 0xFFFFFFFFull;
                if (e >= a.n) continue;           // (never: the table speaks of entries only)
                uint64_t es, el;
                chunk_range(a.ends, e, &es, &el);
                if (el != len || !dedup_equal(ptext + start, a.text + es, len)) continue;
                const unsigned long long sum = wordcount_sat_add(a.weights[e], add_w);
                a.weights[e] = sum;
                over = over || sum >= kWordcountWeightLimit;
                is_new = false;
                break;
            }
        }
        new_out[j] = is_new ? 1 : 0;
    }
    unsigned long long n, b, c;
    block_excl(is_new ? 1ull : 0ull, sh, &n);
    block_excl(is_new ? len : 0ull, sh, &b);
    block_excl(w, sh, &c);
    if (threadIdx.x == 0) {
        blk_cnt[blockIdx.x] = n;
        blk_bytes[blockIdx.x] = b;
        atomicAdd(&ctl->piece_chunks, c);
    }
    if (over) ctl->overflow = 1;
}

template <typename W>
__global__ __launch_bounds__(kDdThreads) void k_wc_append(const uint8_t *__restrict__ ptext,
                                                          const unsigned long long *__restrict__ pend,
                                                          const W *__restrict__ pweights,
                                                          const unsigned long long *__restrict__ pfirst, uint64_t nu,
                                                          uint32_t repeat, uint64_t chunk_base, WcAcc a, WcTable t,
                                                          uint32_t max_chunk, const unsigned long long *__restrict__ hash,
                                                          const uint8_t *__restrict__ is_new_in,
                                                          const unsigned long long *__restrict__ blk_cnt,
                                                          const unsigned long long *__restrict__ blk_bytes, uint64_t n_new,
                                                          uint64_t n_new_bytes) {
    __shared__ unsigned long long sh[kDdWaves];
    const uint64_t j = (uint64_t)blockIdx.x * kDdThreads + threadIdx.x;
    uint64_t start = 0, len = 0;
    bool is_new = false;
    if (j < nu) {
        chunk_range(pend, j, &start, &len);
        is_new = is_new_in[j] != 0;
    }
    unsigned long long tot;
    const uint64_t k = blk_cnt[blockIdx.x] + block_excl(is_new ? 1ull : 0ull, sh, &tot);
    const uint64_t o = blk_bytes[blockIdx.x] + block_excl(is_new ? len : 0ull, sh, &tot);
    if (!is_new || k >= n_new || o + len > n_new_bytes) return;          // (the counts' own flags: never beyond)
    const uint64_t e = a.n + k, at = a.n_bytes + o;                       // the buffers hold a.n + n_new entries
    copy_chunk(a.text + at, ptext + start, at, start, len);              // (both texts are 16-byte aligned)
    a.ends[e] = at + len;
    a.weights[e] = wordcount_sat_mul(pweights[j], repeat);
    a.first[e] = chunk_base + pfirst[j];
    if (len <= max_chunk) wc_claim(t, hash[j], e);
}

// The check of a table nobody vouches for: are its hashed chunks pairwise distinct?  Every one claims a slot of the empty
// scratch table t with the insert of dedup.hip -- a free slot by compare-and-swap, whose answer is looked at when it
// fails -- and one that meets a slot with its own bytes sets *dup.  Chunks with the same bytes walk the same probe
// sequence and slots never become free, so the later of two always meets the earlier.  Nothing else is written.
__global__ __launch_bounds__(kDdThreads) void k_wc_distinct(const uint8_t *__restrict__ ptext,
                                                            const unsigned long long *__restrict__ pend, uint64_t nu,
                                                            WcTable t, uint32_t max_chunk, uint32_t hash_bits,
                                                            unsigned long long *dup) {
    const uint64_t j = (uint64_t)blockIdx.x * kDdThreads + threadIdx.x;
    if (j >= nu) return;
    uint64_t start, len;
    chunk_range(pend, j, &start, &len);
    if (len > max_chunk) return;
    const unsigned long long h = dedup_hash(ptext + start, len, hash_bits);
    const uint32_t tag = dedup_tag(h);
    const unsigned long long mine = dedup_slot(tag, j);
    uint64_t pos = dedup_home(h, t.bits);
    for (uint64_t probe = 0; probe <= t.mask; ++probe, pos = (pos + 1) & t.mask) {
        unsigned long long v = t.slots[pos];
        if (v == kDedupEmpty) {
            v = atomicCAS(&t.slots[pos], kDedupEmpty, mine);
            if (v == kDedupEmpty) return;
        }
        if (dedup_tag(v) != tag) continue;
        const uint64_t r = v & 0xFFFFFFFFull;
        if (r >= nu) continue;                    // (never: the scratch table speaks of these chunks only)
        uint64_t rs, rl;
        chunk_range(pend, r, &rs, &rl);
        if (rl == len && dedup_equal(ptext + start, ptext + rs, len)) {
            *dup = 1;
            return;
        }
    }
}

// the views of mbpe_wordcount_result: the end mask of the packed text and the weights as u32
__global__ __launch_bounds__(kDdThreads) void k_wc_views(WcAcc a, uint32_t *__restrict__ out_mask,
                                                         uint32_t *__restrict__ out_weights) {
    const uint64_t e = (uint64_t)blockIdx.x * kDdThreads + threadIdx.x;
    if (e >= a.n) return;
    const uint64_t last = a.ends[e] - 1;
    atomicOr(&out_mask[last >> 5], 1u << (last & 31));
    const unsigned long long w = a.weights[e];
    out_weights[e] = w < kWordcountWeightLimit ? (uint32_t)w : 0xFFFFFFFFu;      // (never: overflow is refused before)
}

}  // namespace
}  // namespace mbpe

using namespace mbpe;

struct mbpe_wordcount : DevQueue {
    mbpe_wordcount() : DevQueue(false) {}
    ~mbpe_wordcount() { mbpe_dedup_destroy(dd); }
    mbpe_dedup *dd = nullptr;                              // on its own stream; every call of it ends synchronised
    uint32_t max_chunk = kDedupMaxChunkBytes, hash_bits = 64;
    // the accumulated table
    DevBuf<uint8_t> d_text;
    DevBuf<unsigned long long> d_ends, d_weights, d_first, d_slots;
    uint32_t table_bits = 0;                               // 0: no table yet
    uint64_t n_unique = 0, n_bytes = 0;
    uint64_t n_pieces = 0, n_chunks_total = 0;             // chunks counted (repeats included)
    uint64_t chunk_base = 0;                               // chunks of the concatenated list before the next piece
    bool overflow = false;
    // one piece
    DevBuf<unsigned long long> d_tile, d_pend, d_hash, d_blk, d_ctl;
    DevBuf<uint8_t> d_new;
    // one table out of a blob: ends, weights, first_chunk and text as uploaded, the scratch table of its check
    DevBuf<unsigned long long> d_in, d_scratch;
    DevBuf<uint8_t> d_in_text;
    bool last_was_add = true;                              // does the deduper's time belong to the latest call?
    // mbpe_wordcount_result
    DevBuf<uint8_t> d_mask;
    DevBuf<uint32_t> d_w32;
    bool views_valid = false;
    float last_ms = 0.f;

    WcAcc acc() const { return {d_text.get(), d_ends.get(), d_weights.get(), d_first.get(), n_unique, n_bytes}; }
    WcTable table() const { return {d_slots.get(), (1ull << table_bits) - 1, table_bits}; }
};

namespace {

int wc_add_ms(mbpe_wordcount *w) {
    float ms = 0.f;
    WCHK(hipEventElapsedTime(&ms, w->ev0, w->ev1));
    w->last_ms += ms;
    return MBPE_OK;
}

// What steps 1 - 4 fold into the accumulated table: nu chunks that are pairwise distinct wherever they are hashed, in a
// packed text of nb bytes (in a 16-byte aligned buffer), with weights and first_chunk on the device.  The deduper's
// result is one (u32 weights; its ends come out of the end mask m32), another table the other (u64 weights, ends given,
// m32 NULL).
template <typename W>
struct WcSource {
    const uint8_t *text;
    const uint32_t *m32;
    const unsigned long long *ends;
    const W *weights;
    const unsigned long long *first;
    uint64_t nu, nb;
};

// steps 1 - 4 for a source with nu > 0; *kept_out: the sum of its weights.  first_chunk moves on by w->chunk_base
template <typename W>
int wc_fold_source(mbpe_wordcount *w, const WcSource<W> &s, uint32_t repeat, uint64_t *kept_out) {
    int rc;
    const uint64_t nu = s.nu, nb = s.nb;
    if (w->n_unique + nu >= 0xFFFFFFFFull) return fail(MBPE_ERR_ARG, "wordcount: 2^32 - 1 unique chunks or more");
    const uint64_t n_words = (nb + 63) / 64, n_tiles = blocks_for(n_words);
    const uint32_t n_blk = blocks_for(nu);
    if ((rc = w->d_ctl.reserve(sizeof(WcCtl), w->mem)) != MBPE_OK) return rc;
    if (s.m32) {
        if ((rc = w->d_tile.reserve(n_tiles * 8, w->mem)) != MBPE_OK) return rc;
        if ((rc = w->d_pend.reserve(nu * 8, w->mem)) != MBPE_OK) return rc;
    }
    if ((rc = w->d_hash.reserve(nu * 8, w->mem)) != MBPE_OK) return rc;
    if ((rc = w->d_new.reserve(nu, w->mem)) != MBPE_OK) return rc;
    if ((rc = w->d_blk.reserve((uint64_t)n_blk * 16, w->mem)) != MBPE_OK) return rc;
    // 1. capacity, before anything else: the lookup and the append below can never fill the table
    const bool rebuild = wordcount_needs_rebuild(w->n_unique + nu, w->table_bits ? 1ull << w->table_bits : 0);
    if (rebuild) {
        const uint32_t bits = dedup_table_bits(w->n_unique + nu);
        if ((rc = w->d_slots.reserve((1ull << bits) * 8, w->mem)) != MBPE_OK) { w->table_bits = 0; return rc; }
        w->table_bits = bits;
    }
    WcCtl *dctl = reinterpret_cast<WcCtl *>(w->d_ctl.get());
    unsigned long long *blk_cnt = w->d_blk, *blk_bytes = w->d_blk.get() + n_blk;
    const unsigned long long *pend = s.m32 ? w->d_pend.get() : s.ends;
    const WcTable t = w->table();
    WCHK(hipEventRecord(w->ev0, w->stream));
    WCHK(hipMemsetAsync(w->d_ctl, 0, sizeof(WcCtl), w->stream));
    if (s.m32) {
        hipLaunchKernelGGL(k_dd_tile_count, dim3((uint32_t)n_tiles), dim3(kDdThreads), 0, w->stream, s.m32, nb, n_words,
                           w->d_tile.get());
        hipLaunchKernelGGL(k_dd_scan, dim3(1), dim3(kScanThreads), 0, w->stream, w->d_tile.get(), n_tiles, &dctl->n_ends);
        hipLaunchKernelGGL(k_dd_chunk_ends, dim3((uint32_t)n_tiles), dim3(kDdThreads), 0, w->stream, s.m32, nb, n_words,
                           w->d_tile.get(), nu, w->d_pend.get());
    }
    if (rebuild) {
        WCHK(hipMemsetAsync(t.slots, 0xFF, (t.mask + 1) * 8, w->stream));
        if (w->n_unique)
            hipLaunchKernelGGL(k_wc_rehash, dim3(blocks_for(w->n_unique)), dim3(kDdThreads), 0, w->stream, w->acc(), t,
                               w->max_chunk, w->hash_bits);
    }
    // 2. lookup, 3. scan
    hipLaunchKernelGGL(k_wc_lookup<W>, dim3(n_blk), dim3(kDdThreads), 0, w->stream, s.text, pend, s.weights, nu, repeat,
                       w->acc(), t, w->max_chunk, w->hash_bits, w->d_hash.get(), w->d_new.get(), blk_cnt, blk_bytes, dctl);
    hipLaunchKernelGGL(k_dd_scan, dim3(1), dim3(kScanThreads), 0, w->stream, blk_cnt, (uint64_t)n_blk, &dctl->n_new);
    hipLaunchKernelGGL(k_dd_scan, dim3(1), dim3(kScanThreads), 0, w->stream, blk_bytes, (uint64_t)n_blk,
                       &dctl->n_new_bytes);
    WCHK(hipGetLastError());
    WCHK(hipEventRecord(w->ev1, w->stream));
    WcCtl ctl = {};
    WCHK(hipMemcpyAsync(&ctl, w->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, w->stream));
    WCHK(hipStreamSynchronize(w->stream));
    if ((rc = wc_add_ms(w)) != MBPE_OK) return rc;
    // (weights of entries that were found have grown already: from here on the source counts)
    w->overflow = w->overflow || ctl.overflow != 0;
    if ((s.m32 && ctl.n_ends != nu) || ctl.n_new > nu || ctl.n_new_bytes > nb || ctl.n_new_bytes < ctl.n_new)
        return fail(MBPE_ERR_HIP, "wordcount: the device counted impossible new chunks");
    // 4. append
    if (ctl.n_new) {
        const uint64_t n_after = w->n_unique + ctl.n_new, b_after = w->n_bytes + ctl.n_new_bytes;
        if ((rc = w->d_text.grow(w->n_bytes, (b_after + 15) / 16 * 16, w->mem, w->stream)) != MBPE_OK) return rc;
        if ((rc = w->d_ends.grow(w->n_unique * 8, n_after * 8, w->mem, w->stream)) != MBPE_OK) return rc;
        if ((rc = w->d_weights.grow(w->n_unique * 8, n_after * 8, w->mem, w->stream)) != MBPE_OK) return rc;
        if ((rc = w->d_first.grow(w->n_unique * 8, n_after * 8, w->mem, w->stream)) != MBPE_OK) return rc;
        WCHK(hipEventRecord(w->ev0, w->stream));
        hipLaunchKernelGGL(k_wc_append<W>, dim3(n_blk), dim3(kDdThreads), 0, w->stream, s.text, pend, s.weights, s.first, nu,
                           repeat, w->chunk_base, w->acc(), t, w->max_chunk, w->d_hash.get(), w->d_new.get(), blk_cnt,
                           blk_bytes, (uint64_t)ctl.n_new, (uint64_t)ctl.n_new_bytes);
        WCHK(hipGetLastError());
        WCHK(hipEventRecord(w->ev1, w->stream));
        WCHK(hipStreamSynchronize(w->stream));
        if ((rc = wc_add_ms(w)) != MBPE_OK) return rc;
        w->n_unique = n_after;
        w->n_bytes = b_after;
    }
    *kept_out = ctl.piece_chunks;
    return MBPE_OK;
}

// the piece the deduper holds -> the accumulated table.  piece_input_chunks: what first_chunk of the piece counts in
// (mbpe_wordcount_add: its chunk_off entries, the empty chunks included); kWcKeptChunks: the chunks of the piece's mask,
// which are its weights' sum, taken by the lookup
constexpr uint64_t kWcKeptChunks = ~0ull;
int wc_fold(mbpe_wordcount *w, uint64_t nu, uint64_t nb, uint64_t piece_input_chunks, uint32_t repeat) {
    int rc;
    w->views_valid = false;
    const uint8_t *ptext = nullptr, *pmask = nullptr;
    const uint32_t *pweights = nullptr;
    const uint64_t *pfirst = nullptr;
    if ((rc = mbpe_dedup_result(w->dd, &ptext, &pmask, &pweights, &pfirst)) != MBPE_OK) return rc;
    uint64_t kept = 0;
    if (nu) {
        const WcSource<uint32_t> s = {ptext, reinterpret_cast<const uint32_t *>(pmask), nullptr, pweights,
                                      reinterpret_cast<const unsigned long long *>(pfirst), nu, nb};
        if ((rc = wc_fold_source(w, s, repeat, &kept)) != MBPE_OK) return rc;
    }
    w->n_chunks_total += kept * repeat;
    w->chunk_base += (piece_input_chunks == kWcKeptChunks ? kept : piece_input_chunks) * repeat;
    w->n_pieces += 1;
    return MBPE_OK;
}

// Another table -> the accumulated table: its entries on this object's device, vouched for (another object's, or a blob's
// after wordcount_blob_check and wc_distinct), and its totals
struct WcIncoming {
    WcSource<unsigned long long> s;
    uint64_t n_pieces, n_chunks_total, chunk_base;
};
int wc_fold_table(mbpe_wordcount *w, const WcIncoming &in) {
    w->views_valid = false;
    uint64_t sum = 0;
    if (in.s.nu) {
        const int rc = wc_fold_source(w, in.s, 1, &sum);
        if (rc != MBPE_OK) return rc;
    }
    w->n_chunks_total += in.n_chunks_total;
    w->chunk_base += in.chunk_base;
    w->n_pieces += in.n_pieces;
    return MBPE_OK;
}

// are the hashed chunks of s pairwise distinct?  Touches the scratch table only
int wc_distinct(mbpe_wordcount *w, const WcSource<unsigned long long> &s, bool *distinct_out) {
    int rc;
    const uint32_t bits = dedup_table_bits(s.nu);
    if ((rc = w->d_ctl.reserve(sizeof(WcCtl), w->mem)) != MBPE_OK) return rc;
    if ((rc = w->d_scratch.reserve((1ull << bits) * 8, w->mem)) != MBPE_OK) return rc;
    const WcTable t = {w->d_scratch.get(), (1ull << bits) - 1, bits};
    WcCtl *dctl = reinterpret_cast<WcCtl *>(w->d_ctl.get());
    WCHK(hipEventRecord(w->ev0, w->stream));
    WCHK(hipMemsetAsync(w->d_ctl, 0, sizeof(WcCtl), w->stream));
    WCHK(hipMemsetAsync(t.slots, 0xFF, (t.mask + 1) * 8, w->stream));
    hipLaunchKernelGGL(k_wc_distinct, dim3(blocks_for(s.nu)), dim3(kDdThreads), 0, w->stream, s.text, s.ends, s.nu, t,
                       w->max_chunk, w->hash_bits, &dctl->dup);
    WCHK(hipGetLastError());
    WCHK(hipEventRecord(w->ev1, w->stream));
    WcCtl ctl = {};
    WCHK(hipMemcpyAsync(&ctl, w->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, w->stream));
    WCHK(hipStreamSynchronize(w->stream));
    if ((rc = wc_add_ms(w)) != MBPE_OK) return rc;
    *distinct_out = ctl.dup == 0;
    return MBPE_OK;
}

void wc_report(const mbpe_wordcount *w, uint64_t *n_unique_out, uint64_t *n_unique_bytes_out) {
    if (n_unique_out) *n_unique_out = w->n_unique;
    if (n_unique_bytes_out) *n_unique_bytes_out = w->n_bytes;
}

int wc_usable(const mbpe_wordcount *w, const char *who) {
    if (w->overflow) return fail(MBPE_ERR_OVERFLOW, std::string(who) + ": a chunk's count has reached 2^31");
    return MBPE_OK;
}

}  // namespace

extern "C" {

int mbpe_wordcount_create(int device_id, mbpe_wordcount **out) {
    if (!out) return fail(MBPE_ERR_ARG, "mbpe_wordcount_create: NULL argument");
    if (find_device(device_id) != MBPE_OK) return MBPE_ERR_NO_DEVICE;
    mbpe_wordcount *w = new (std::nothrow) mbpe_wordcount;
    if (!w) return fail(MBPE_ERR_OOM, "mbpe_wordcount_create: host allocation failed");
    w->device = device_id;
    int rc = w->open(device_id);
    if (rc == MBPE_OK) rc = mbpe_dedup_create(device_id, &w->dd);
    if (rc != MBPE_OK) {
        const std::string keep = mbpe_host::last_error();
        mbpe_wordcount_destroy(w);
        mbpe_host::set_last_error(keep);
        return rc;
    }
    *out = w;
    return MBPE_OK;
}

void mbpe_wordcount_destroy(mbpe_wordcount *w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    delete w;                                     // the deduper, the buffers, then the events, then the stream
}

int mbpe_wordcount_set_option(mbpe_wordcount *w, const char *name, int64_t value) {
    if (!name) return fail(MBPE_ERR_ARG, "mbpe_wordcount_set_option: NULL argument");
    const bool is_max = !strcmp(name, "max_chunk_bytes"), is_bits = !strcmp(name, "hash_bits");
    if (!(is_max && value >= 0 && value <= 0x7FFFFFFF) && !(is_bits && value >= 0 && value <= 64))
        return fail(MBPE_ERR_ARG, std::string("mbpe_wordcount_set_option: unknown option or bad value: ") + name);
    if (!w) return fail(MBPE_ERR_ARG, "mbpe_wordcount_set_option: NULL argument");
    if (w->n_pieces || w->n_unique || w->chunk_base)
        return fail(MBPE_ERR_STATE, "mbpe_wordcount_set_option: a piece has been added already");
    const int rc = mbpe_dedup_set_option(w->dd, name, value);
    if (rc != MBPE_OK) return rc;
    (is_max ? w->max_chunk : w->hash_bits) = (uint32_t)value;
    return MBPE_OK;
}

int mbpe_wordcount_add_endmask(mbpe_wordcount *w, const uint8_t *text_dev, uint64_t n_bytes, const uint8_t *endmask_dev,
                               uint32_t repeat, uint64_t *n_unique_total_out, uint64_t *n_unique_bytes_total_out) {
    if (repeat == 0) return fail(MBPE_ERR_ARG, "mbpe_wordcount_add_endmask: repeat must be at least 1");
    if (!w || !n_unique_total_out || (n_bytes && (!text_dev || !endmask_dev)))
        return fail(MBPE_ERR_ARG, "mbpe_wordcount_add_endmask: NULL argument");
    wc_report(w, n_unique_total_out, n_unique_bytes_total_out);
    uint64_t nu = 0, nb = 0;
    w->last_ms = 0.f;
    w->last_was_add = true;
    int rc = mbpe_dedup_chunks_endmask(w->dd, text_dev, n_bytes, endmask_dev, &nu, &nb);      // (checks the alignment)
    if (rc != MBPE_OK) return rc;
    WCHK(hipSetDevice(w->device));
    if ((rc = wc_fold(w, nu, nb, kWcKeptChunks, repeat)) != MBPE_OK) return rc;
    wc_report(w, n_unique_total_out, n_unique_bytes_total_out);
    return MBPE_OK;
}

int mbpe_wordcount_add(mbpe_wordcount *w, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                       const uint64_t *chunk_off, uint64_t n_chunks, uint32_t repeat, uint64_t *n_unique_total_out,
                       uint64_t *n_unique_bytes_total_out) {
    if (repeat == 0) return fail(MBPE_ERR_ARG, "mbpe_wordcount_add: repeat must be at least 1");
    if (!w || !n_unique_total_out || (!text && n_bytes) || !chunk_off)
        return fail(MBPE_ERR_ARG, "mbpe_wordcount_add: NULL argument");
    wc_report(w, n_unique_total_out, n_unique_bytes_total_out);
    uint64_t nu = 0, nb = 0;
    w->last_ms = 0.f;
    w->last_was_add = true;
    int rc = mbpe_dedup_chunks(w->dd, text, n_bytes, text_on_device, chunk_off, n_chunks, &nu, &nb);   // (checks the rest)
    if (rc != MBPE_OK) return rc;
    WCHK(hipSetDevice(w->device));
    if ((rc = wc_fold(w, nu, nb, n_chunks, repeat)) != MBPE_OK) return rc;      // (first_chunk counts the empty chunks)
    wc_report(w, n_unique_total_out, n_unique_bytes_total_out);
    return MBPE_OK;
}

int mbpe_wordcount_result(mbpe_wordcount *w, const uint8_t **text_dev_out, const uint8_t **endmask_dev_out,
                          const uint32_t **weights_dev_out, const uint64_t **first_chunk_dev_out) {
    if (!w) return fail(MBPE_ERR_ARG, "mbpe_wordcount_result: NULL argument");
    int rc = wc_usable(w, "mbpe_wordcount_result");
    if (rc != MBPE_OK) return rc;
    WCHK(hipSetDevice(w->device));
    if (!w->views_valid) {
        const uint64_t mask_bytes = mask_bytes_for(w->n_bytes);
        if ((rc = w->d_mask.reserve(mask_bytes, w->mem)) != MBPE_OK) return rc;
        if ((rc = w->d_w32.reserve(std::max<uint64_t>(w->n_unique * 4, 16), w->mem)) != MBPE_OK) return rc;
        // (nothing accumulated yet: the views are still valid device pointers)
        if ((rc = w->d_text.grow(0, 16, w->mem, w->stream)) != MBPE_OK) return rc;
        if ((rc = w->d_first.grow(0, 16, w->mem, w->stream)) != MBPE_OK) return rc;
        WCHK(hipMemsetAsync(w->d_mask, 0, mask_bytes, w->stream));
        if (w->n_unique)
            hipLaunchKernelGGL(k_wc_views, dim3(blocks_for(w->n_unique)), dim3(kDdThreads), 0, w->stream, w->acc(),
                               reinterpret_cast<uint32_t *>(w->d_mask.get()), w->d_w32.get());
        WCHK(hipGetLastError());
        WCHK(hipStreamSynchronize(w->stream));
        w->views_valid = true;
    }
    if (text_dev_out) *text_dev_out = w->d_text;
    if (endmask_dev_out) *endmask_dev_out = w->d_mask;
    if (weights_dev_out) *weights_dev_out = w->d_w32;
    if (first_chunk_dev_out) *first_chunk_dev_out = reinterpret_cast<const uint64_t *>(w->d_first.get());
    return MBPE_OK;
}

int mbpe_wordcount_get(mbpe_wordcount *w, uint8_t *text_out, uint64_t *chunk_off_out, uint32_t *weights_out,
                       uint64_t *first_chunk_out, uint64_t cap_bytes, uint64_t cap_chunks) {
    if (!w) return fail(MBPE_ERR_ARG, "mbpe_wordcount_get: NULL argument");
    const int rc = wc_usable(w, "mbpe_wordcount_get");
    if (rc != MBPE_OK) return rc;
    if (text_out && cap_bytes < w->n_bytes) return fail(MBPE_ERR_ARG, "mbpe_wordcount_get: text_out is too small");
    if ((chunk_off_out || weights_out || first_chunk_out) && cap_chunks < w->n_unique)
        return fail(MBPE_ERR_ARG, "mbpe_wordcount_get: the chunk arrays are too small");
    WCHK(hipSetDevice(w->device));
    const uint64_t nu = w->n_unique, nb = w->n_bytes;
    if (text_out && nb) WCHK(hipMemcpy(text_out, w->d_text, nb, hipMemcpyDeviceToHost));
    if (first_chunk_out && nu) WCHK(hipMemcpy(first_chunk_out, w->d_first, nu * 8, hipMemcpyDeviceToHost));
    if (chunk_off_out) {
        chunk_off_out[0] = 0;
        if (nu) WCHK(hipMemcpy(chunk_off_out + 1, w->d_ends, nu * 8, hipMemcpyDeviceToHost));
    }
    if (weights_out && nu) {
        try {
            std::vector<unsigned long long> wide(nu);
            WCHK(hipMemcpy(wide.data(), w->d_weights, nu * 8, hipMemcpyDeviceToHost));
            for (uint64_t e = 0; e < nu; ++e) weights_out[e] = (uint32_t)wide[e];      // (all below 2^31: see above)
        } catch (const std::bad_alloc &) {
            return fail(MBPE_ERR_OOM, "mbpe_wordcount_get: host allocation failed");
        }
    }
    return MBPE_OK;
}

int mbpe_wordcount_export_size(const mbpe_wordcount *w, uint64_t *n_bytes_out) {
    if (!w || !n_bytes_out) return fail(MBPE_ERR_ARG, "mbpe_wordcount_export_size: NULL argument");
    const int rc = wc_usable(w, "mbpe_wordcount_export_size");
    if (rc != MBPE_OK) return rc;
    *n_bytes_out = wordcount_blob_size(w->n_unique, w->n_bytes);
    return MBPE_OK;
}

int mbpe_wordcount_export(mbpe_wordcount *w, uint8_t *blob_out, uint64_t cap_bytes, uint64_t *n_bytes_out) {
    if (!w || !blob_out) return fail(MBPE_ERR_ARG, "mbpe_wordcount_export: NULL argument");
    const int rc = wc_usable(w, "mbpe_wordcount_export");
    if (rc != MBPE_OK) return rc;
    const uint64_t nu = w->n_unique, nb = w->n_bytes, size = wordcount_blob_size(nu, nb);
    if (cap_bytes < size) return fail(MBPE_ERR_ARG, "mbpe_wordcount_export: blob_out is too small");
    WCHK(hipSetDevice(w->device));
    const uint32_t head[2] = {kWordcountBlobMagic, kWordcountBlobVersion};
    const uint64_t fields[7] = {w->max_chunk, nu, nb, w->n_pieces, w->n_chunks_total, w->chunk_base, 0};
    memcpy(blob_out, head, 8);
    memcpy(blob_out + 8, fields, 56);
    uint8_t *at = blob_out + kWordcountBlobHeader;
    for (const unsigned long long *src : {w->d_ends.get(), w->d_weights.get(), w->d_first.get()}) {
        if (nu) WCHK(hipMemcpy(at, src, nu * 8, hipMemcpyDeviceToHost));
        at += nu * 8;
    }
    if (nb) WCHK(hipMemcpy(at, w->d_text, nb, hipMemcpyDeviceToHost));
    memset(at + nb, 0, size - (uint64_t)(at - blob_out) - nb);
    if (n_bytes_out) *n_bytes_out = size;
    return MBPE_OK;
}

int mbpe_wordcount_merge_blob(mbpe_wordcount *w, const uint8_t *blob, uint64_t n_bytes, uint64_t *n_unique_total_out,
                              uint64_t *n_unique_bytes_total_out) {
    if (!w || !blob) return fail(MBPE_ERR_ARG, "mbpe_wordcount_merge_blob: NULL argument");
    wc_report(w, n_unique_total_out, n_unique_bytes_total_out);
    WordcountBlob b;
    const char *why = wordcount_blob_check(blob, n_bytes, &b);
    if (why) return fail(MBPE_ERR_ARG, std::string("mbpe_wordcount_merge_blob: ") + why);
    if (b.max_chunk_bytes != w->max_chunk)
        return fail(MBPE_ERR_ARG, "mbpe_wordcount_merge_blob: counted with another max_chunk_bytes");
    WCHK(hipSetDevice(w->device));
    w->last_ms = 0.f;
    w->last_was_add = false;
    int rc;
    WcIncoming in = {{nullptr, nullptr, nullptr, nullptr, nullptr, b.n_unique, b.n_bytes},
                     b.n_pieces, b.n_chunks_total, b.chunk_base};
    if (b.n_unique) {
        // ends, weights and first_chunk lie back to back in the blob: one upload, and one for the text
        const uint64_t nu = b.n_unique;
        if ((rc = w->d_in.reserve(nu * 24, w->mem)) != MBPE_OK) return rc;
        if ((rc = w->d_in_text.reserve((b.n_bytes + 15) / 16 * 16, w->mem)) != MBPE_OK) return rc;
        WCHK(hipMemcpyAsync(w->d_in, b.ends, nu * 24, hipMemcpyHostToDevice, w->stream));
        WCHK(hipMemcpyAsync(w->d_in_text, b.text, b.n_bytes, hipMemcpyHostToDevice, w->stream));
        in.s.text = w->d_in_text;
        in.s.ends = w->d_in;
        in.s.weights = w->d_in.get() + nu;
        in.s.first = w->d_in.get() + 2 * nu;
        // nothing of the table changes before the incoming chunks are known to be distinct
        bool distinct = false;
        if ((rc = wc_distinct(w, in.s, &distinct)) != MBPE_OK) return rc;
        if (!distinct) return fail(MBPE_ERR_ARG, "mbpe_wordcount_merge_blob: a hashed chunk is present twice");
    }
    if ((rc = wc_fold_table(w, in)) != MBPE_OK) return rc;
    wc_report(w, n_unique_total_out, n_unique_bytes_total_out);
    return MBPE_OK;
}

int mbpe_wordcount_merge(mbpe_wordcount *w, const mbpe_wordcount *other) {
    if (!w || !other) return fail(MBPE_ERR_ARG, "mbpe_wordcount_merge: NULL argument");
    if (w == other) return fail(MBPE_ERR_ARG, "mbpe_wordcount_merge: an object cannot be merged into itself");
    if (w->device != other->device)
        return fail(MBPE_ERR_ARG, "mbpe_wordcount_merge: the objects are on different devices (mbpe_wordcount_merge_blob)");
    if (w->max_chunk != other->max_chunk || w->hash_bits != other->hash_bits)
        return fail(MBPE_ERR_ARG, "mbpe_wordcount_merge: the objects' options differ");
    const int rc = wc_usable(other, "mbpe_wordcount_merge");
    if (rc != MBPE_OK) return rc;
    WCHK(hipSetDevice(w->device));
    w->last_ms = 0.f;
    w->last_was_add = false;
    // (every call of `other` ended synchronised: its buffers are at rest, and its own entries are distinct as they are)
    const WcIncoming in = {{other->d_text.get(), nullptr, other->d_ends.get(), other->d_weights.get(), other->d_first.get(),
                            other->n_unique, other->n_bytes},
                           other->n_pieces, other->n_chunks_total, other->chunk_base};
    return wc_fold_table(w, in);
}

int mbpe_wordcount_stats(const mbpe_wordcount *w, uint64_t *n_pieces_out, uint64_t *n_chunks_total_out,
                         uint64_t *n_unique_out, uint64_t *n_unique_bytes_out) {
    if (!w) return fail(MBPE_ERR_ARG, "mbpe_wordcount_stats: NULL argument");
    if (n_pieces_out) *n_pieces_out = w->n_pieces;
    if (n_chunks_total_out) *n_chunks_total_out = w->n_chunks_total;
    wc_report(w, n_unique_out, n_unique_bytes_out);
    return MBPE_OK;
}

int mbpe_wordcount_reset(mbpe_wordcount *w) {
    if (!w) return fail(MBPE_ERR_ARG, "mbpe_wordcount_reset: NULL argument");
    WCHK(hipSetDevice(w->device));
    if (w->table_bits) {
        WCHK(hipMemsetAsync(w->d_slots, 0xFF, (1ull << w->table_bits) * 8, w->stream));
        WCHK(hipStreamSynchronize(w->stream));
    }
    w->n_unique = w->n_bytes = w->n_pieces = w->n_chunks_total = w->chunk_base = 0;
    w->overflow = w->views_valid = false;
    return MBPE_OK;
}

int mbpe_wordcount_kernel_ms(const mbpe_wordcount *w, float *ms_out) {
    if (!w || !ms_out) return fail(MBPE_ERR_ARG, "mbpe_wordcount_kernel_ms: NULL argument");
    float dd_ms = 0.f;
    const int rc = mbpe_dedup_kernel_ms(w->dd, &dd_ms);
    if (rc != MBPE_OK) return rc;
    *ms_out = (w->last_was_add ? dd_ms : 0.f) + w->last_ms;      // (a merge does not run the deduper)
    return MBPE_OK;
}

int mbpe_wordcount_alloc_count(const mbpe_wordcount *w, uint64_t *n_out) {
    if (!w || !n_out) return fail(MBPE_ERR_ARG, "mbpe_wordcount_alloc_count: NULL argument");
    uint64_t dd_n = 0;
    const int rc = mbpe_dedup_alloc_count(w->dd, &dd_n);
    if (rc != MBPE_OK) return rc;
    *n_out = dd_n + w->mem.n_allocs;
    return MBPE_OK;
}

}  // extern "C"
