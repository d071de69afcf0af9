// Word counts across calls (wordcount.hip): the distinct chunks of a corpus that arrives in pieces, in the order of
// their first occurrence over all pieces, with the number of occurrences of each -- what one dedup (dedup.h) of the
// pieces' chunk lists laid end to end gives, without that list ever existing.
//
// A piece goes through the owned deduper first; its result -- unique chunks that are pairwise distinct wherever they
// were hashed, with weights and first occurrences -- is then folded into the accumulated table:
//
//   entries   packed text, and per unique chunk a u64 end offset, a u64 weight and a u64 first_chunk (the index in the
//             concatenated chunk list: the chunks before the piece + the piece's own first_chunk)
//   table     open addressing as in dedup.h: slot = (tag << 32) | entry index, kDedupEmpty when free; dedup_hash,
//             dedup_tag and dedup_home place a chunk, the bytes decide equality.  Slots never become free, an entry
//             sits behind occupied slots only, so a lookup that meets a free slot has seen every candidate.
//
//   1. capacity  2 x (entries + the piece's unique chunks) above the capacity: the table is rebuilt at the power of two
//                that holds them, every hashed entry claiming a slot again from its bytes.  Nothing below can fill it.
//   2. lookup    read-only on the table: a chunk that is found adds weight x repeat to its entry (no atomic: no two
//                chunks of a piece find the same entry), one that is not found is new; a chunk above "max_chunk_bytes"
//                is new without a look, every time it occurs, as in one dedup of the whole.
//   3. scan      the new chunks and their bytes before each one
//   4. append    the new chunks' bytes, ends, weights and first_chunk behind the entries, in the piece's order, and one
//                compare-and-swap per hashed new chunk for a free slot on its probe sequence (they are pairwise
//                distinct and none is in the table: no byte compare)
//
// Weights are u64 sums that saturate; the weighted load takes u32 below 2^31, so an entry that reaches 2^31 makes the
// table unusable for a training until it is reset (sticky).
//
// This header is shared by the device code and by host programs: the arithmetic, and wordcount_host, a plain
// restatement over dedup_host results through the same table, rehash included, that tests/wordcount_check.cpp runs
// against a std::map.
#ifndef MBPE_WORDCOUNT_H
#define MBPE_WORDCOUNT_H

#include "dedup.h"

namespace mbpe {

constexpr unsigned long long kWordcountWeightLimit = 1ull << 31;       // a weight has to stay below

MBPE_HD unsigned long long wordcount_sat_add(unsigned long long a, unsigned long long b) {
    return a + b < a ? ~0ull : a + b;
}
MBPE_HD unsigned long long wordcount_sat_mul(unsigned long long w, uint32_t repeat) {
    return w > ~0ull / repeat ? ~0ull : w * repeat;
}
// does a table of `capacity` slots (0: none yet) have to be rebuilt before it holds n_entries?
MBPE_HD bool wordcount_needs_rebuild(uint64_t n_entries, uint64_t capacity) { return 2 * n_entries > capacity; }

#ifndef __HIP_DEVICE_COMPILE__
struct WordcountHost {
    uint32_t max_chunk_bytes = kDedupMaxChunkBytes, hash_bits = 64;
    std::vector<uint8_t> text;
    std::vector<uint64_t> ends, weights, first_chunk;
    std::vector<unsigned long long> slots;
    uint32_t bits = 0;
    uint64_t n_pieces = 0, n_chunks_total = 0, n_rebuilds = 0;
    bool overflow = false;

    void claim(unsigned long long h, uint64_t entry) {
        const uint64_t mask = slots.size() - 1;
        uint64_t pos = dedup_home(h, bits);
        while (slots[pos] != kDedupEmpty) pos = (pos + 1) & mask;
        slots[pos] = dedup_slot(dedup_tag(h), entry);
    }
    uint64_t start_of(uint64_t entry) const { return entry ? ends[entry - 1] : 0; }

    // one piece: chunk c is piece_text[c ? piece_ends[c - 1] : 0 .. piece_ends[c]), none empty; counted `repeat` times
    void add(const uint8_t *piece_text, const uint64_t *piece_ends, uint64_t n_chunks, uint32_t repeat) {
        const DedupHost p = dedup_host(piece_text, piece_ends, n_chunks, max_chunk_bytes, hash_bits);
        const uint64_t nu = p.weights.size(), base = n_chunks_total;
        if (wordcount_needs_rebuild(ends.size() + nu, slots.size())) {
            bits = dedup_table_bits(ends.size() + nu);
            slots.assign(1ull << bits, kDedupEmpty);
            for (uint64_t e = 0; e < ends.size(); ++e) {
                const uint64_t s = start_of(e), len = ends[e] - s;
                if (len <= max_chunk_bytes) claim(dedup_hash(text.data() + s, len, hash_bits), e);
            }
            ++n_rebuilds;
        }
        const uint64_t mask = slots.size() - 1;
        // lookup, against the table as it was before the piece
        std::vector<uint8_t> is_new(nu, 1);
        std::vector<unsigned long long> hash(nu, 0);
        for (uint64_t j = 0; j < nu; ++j) {
            const uint64_t s = j ? p.ends[j - 1] : 0, len = p.ends[j] - s;
            const unsigned long long add_w = wordcount_sat_mul(p.weights[j], repeat);
            if (add_w >= kWordcountWeightLimit) overflow = true;
            if (len > max_chunk_bytes) continue;
            const unsigned long long h = hash[j] = dedup_hash(p.text.data() + s, len, hash_bits);
            for (uint64_t pos = dedup_home(h, bits); slots[pos] != kDedupEmpty; pos = (pos + 1) & mask) {
                const uint64_t e = slots[pos] & 0xFFFFFFFFull, es = start_of(e);
                if (dedup_tag(slots[pos]) == dedup_tag(h) && ends[e] - es == len &&
                    dedup_equal(p.text.data() + s, text.data() + es, len)) {
                    weights[e] = wordcount_sat_add(weights[e], add_w);
                    if (weights[e] >= kWordcountWeightLimit) overflow = true;
                    is_new[j] = 0;
                    break;
                }
            }
        }
        // append
        for (uint64_t j = 0; j < nu; ++j) {
            if (!is_new[j]) continue;
            const uint64_t s = j ? p.ends[j - 1] : 0, len = p.ends[j] - s;
            text.insert(text.end(), p.text.begin() + s, p.text.begin() + s + len);
            ends.push_back(text.size());
            weights.push_back(wordcount_sat_mul(p.weights[j], repeat));
            first_chunk.push_back(base + p.first_chunk[j]);
            if (len <= max_chunk_bytes) claim(hash[j], ends.size() - 1);
        }
        n_chunks_total += n_chunks * repeat;
        ++n_pieces;
    }
};
#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace mbpe

#endif
