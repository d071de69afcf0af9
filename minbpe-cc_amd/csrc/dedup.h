// Chunk deduplication (dedup.hip): the distinct chunks of a chunked text in the order of their first occurrence, with
// the number of occurrences of each.  A training that counts pairs with those numbers as weights (wide.h) sees the
// counts of the full corpus on a stream of the distinct chunks only.
//
// Equality is decided by the bytes.  The hash only places a chunk in an open-addressing table:
//
//   slot = (tag << 32) | representative chunk index, kDedupEmpty when free; tag = dedup_tag(hash)
//   a chunk probes from dedup_home(hash) on: a free slot is claimed with one compare-and-swap; a slot with the same
//   tag whose representative has the same bytes is joined (64-bit atomicMin lowers the representative: every member
//   of a class has the same bytes and the same tag, so a changing representative is harmless); any other slot is passed
//
// Slots never become free again and every member of a class walks the same probe sequence, so a class sits in exactly
// one slot, whoever claimed it; after the pass its representative is the class's smallest chunk index = its first
// occurrence, and the slot's count the class's size.  Nothing in the result depends on the hash function, on the
// thread that claimed a slot, or on collisions ("hash_bits" lowers the hash so that tests make them common).
//
// A chunk longer than "max_chunk_bytes" is never hashed: it passes through as a unique chunk of weight 1 at its place
// in the order (a duplicate of it appears twice, which is as exact), and no lane walks a megabyte of whitespace.
//
// This header is shared by the device code and by host programs: the hash, the slot arithmetic, and dedup_host, a
// plain restatement of the whole operation that tests/dedup_check.cpp runs against a std::map.
#ifndef MBPE_DEDUP_H
#define MBPE_DEDUP_H

#include "span.h"

#include <stdint.h>

#ifndef __HIP_DEVICE_COMPILE__
#include <vector>
#endif

namespace mbpe {

constexpr uint32_t kDedupMaxChunkBytes = 256;           // default of "max_chunk_bytes"
constexpr unsigned long long kDedupEmpty = ~0ull;       // a free slot (chunk indices stay below 2^32 - 1)
constexpr unsigned long long kDedupNoHome = ~0ull;      // home[] of a chunk that passes through unhashed

// FNV-1a over the bytes, a 64-bit finalizer, then the lowest hash_bits bits (64: all, 0: every chunk hashes to 0)
MBPE_HD unsigned long long dedup_hash(const uint8_t *p, uint64_t len, uint32_t hash_bits) {
    unsigned long long h = 0xCBF29CE484222325ull;
    for (uint64_t i = 0; i < len; ++i) { h ^= p[i]; h *= 0x100000001B3ull; }
    h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return hash_bits >= 64 ? h : hash_bits == 0 ? 0ull : h & ((1ull << hash_bits) - 1ull);
}

MBPE_HD uint32_t dedup_tag(unsigned long long h) { return (uint32_t)(h >> 32); }
MBPE_HD unsigned long long dedup_slot(uint32_t tag, uint64_t chunk) { return ((unsigned long long)tag << 32) | chunk; }
// log2 of the table size for n_chunks chunks: at least 2 x n_chunks slots, at least 16
MBPE_HD uint32_t dedup_table_bits(uint64_t n_chunks) {
    uint32_t bits = 4;
    while ((1ull << bits) < 2 * n_chunks) ++bits;
    return bits;
}
MBPE_HD uint64_t dedup_home(unsigned long long h, uint32_t table_bits) {
    return (uint64_t)((h * 0x9E3779B97F4A7C15ull) >> (64 - table_bits));
}
MBPE_HD bool dedup_equal(const uint8_t *a, const uint8_t *b, uint64_t len) {
    for (uint64_t i = 0; i < len; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

#ifndef __HIP_DEVICE_COMPILE__
// The whole operation on the host, through the same table.  Chunk c is text[c ? ends[c - 1] : 0 .. ends[c]), none
// empty.  Result: the unique chunks' bytes packed in order of first occurrence, their ends in that text, their
// weights and the input index of each one's first occurrence; unique_of[c] = the unique chunk that has chunk c's bytes.
struct DedupHost {
    std::vector<uint8_t> text;
    std::vector<uint64_t> ends;
    std::vector<uint32_t> weights;
    std::vector<uint64_t> first_chunk;
    std::vector<uint32_t> unique_of;
};
inline DedupHost dedup_host(const uint8_t *text, const uint64_t *ends, uint64_t n_chunks, uint32_t max_chunk_bytes,
                            uint32_t hash_bits) {
    DedupHost r;
    const uint32_t bits = dedup_table_bits(n_chunks);
    const uint64_t mask = (1ull << bits) - 1;
    std::vector<unsigned long long> slots(mask + 1, kDedupEmpty);
    std::vector<uint64_t> slot_unique(mask + 1, 0);    // slot -> index among the unique chunks
    for (uint64_t c = 0; c < n_chunks; ++c) {
        const uint64_t start = c ? ends[c - 1] : 0, len = ends[c] - start;
        bool is_new = true;
        if (len <= max_chunk_bytes) {
            const unsigned long long h = dedup_hash(text + start, len, hash_bits);
            const uint32_t tag = dedup_tag(h);
            uint64_t pos = dedup_home(h, bits);
            for (;; pos = (pos + 1) & mask) {
                const unsigned long long v = slots[pos];
                if (v == kDedupEmpty) {
                    slots[pos] = dedup_slot(tag, c);
                    slot_unique[pos] = r.weights.size();
                    break;
                }
                const uint64_t rep = v & 0xFFFFFFFFull, rs = rep ? ends[rep - 1] : 0;
                if (dedup_tag(v) == tag && ends[rep] - rs == len && dedup_equal(text + start, text + rs, len)) {
                    r.weights[slot_unique[pos]] += 1;
                    r.unique_of.push_back((uint32_t)slot_unique[pos]);
                    is_new = false;
                    break;
                }
            }
        }
        if (is_new) {
            r.unique_of.push_back((uint32_t)r.weights.size());
            r.text.insert(r.text.end(), text + start, text + start + len);
            r.ends.push_back(r.text.size());
            r.weights.push_back(1);
            r.first_chunk.push_back(c);
        }
    }
    return r;
}
#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace mbpe

#endif
