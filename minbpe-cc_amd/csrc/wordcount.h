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
// A table is itself a source of the fold: distinct chunks with u64 weights and first occurrences.  merge(A, B) runs
// steps 1 - 4 over B's entries -- found: the weight is added; not found: appended in B's order with first_chunk =
// A.chunk_base + B.first_chunk; above "max_chunk_bytes": appended without a look -- and then chunk_base, n_chunks_total
// and n_pieces grow by B's.  With A the count of pieces P_0 .. P_{i-1} and B that of P_i .. P_{k-1}, A is afterwards, bit
// for bit, the count of P_0 .. P_{k-1}.
//
// The serialised table (little-endian, as the hosts this runs on):
//   64-byte header  u32 magic "MBWC", u32 version, then u64 max_chunk_bytes, n_unique, n_bytes, n_pieces, n_chunks_total,
//                   chunk_base, and one u64 that is 0
//   ends, weights, first_chunk   n_unique u64 each
//   text            n_bytes, padded with zeros to a multiple of 16
// wordcount_blob_check states what a blob has to fulfil before anything reads it; that hashed chunks are pairwise
// distinct is checked by whoever folds it (wordcount.hip on the device, WordcountHost::from_blob here).
//
// This header is shared by the device code and by host programs: the arithmetic, the blob's rules, and wordcount_host, a
// plain restatement over dedup_host results through the same table, rehash included, that tests/wordcount_check.cpp and
// tests/wordcount_merge_check.cpp run against a std::map.
#ifndef MBPE_WORDCOUNT_H
#define MBPE_WORDCOUNT_H

#include "dedup.h"

#include <string.h>

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

// ---- the serialised table ----------------------------------------------------------------------------------------------
constexpr uint32_t kWordcountBlobMagic = 0x4357424Du;                   // "MBWC"
constexpr uint32_t kWordcountBlobVersion = 1;
constexpr uint64_t kWordcountBlobHeader = 64;

struct WordcountBlob {              // a blob that wordcount_blob_check has passed; the arrays may be unaligned
    uint64_t max_chunk_bytes, n_unique, n_bytes, n_pieces, n_chunks_total, chunk_base;
    const uint8_t *ends, *weights, *first_chunk, *text;
};

MBPE_HD uint64_t wordcount_blob_u64(const uint8_t *p, uint64_t i) {
    uint64_t v;
    memcpy(&v, p + 8 * i, 8);
    return v;
}
MBPE_HD uint64_t wordcount_blob_size(uint64_t n_unique, uint64_t n_bytes) {
    return kWordcountBlobHeader + 24 * n_unique + (n_bytes + 15) / 16 * 16;
}

// The rules of a blob, in the order they are checked; nullptr when it passes, else the rule that is broken.  Nothing
// beyond n is read, and nothing is read through an offset before the sizes have been checked against n.
MBPE_HD const char *wordcount_blob_check(const uint8_t *blob, uint64_t n, WordcountBlob *out) {
    if (n < kWordcountBlobHeader) return "truncated: shorter than the header";
    uint32_t magic, version;
    memcpy(&magic, blob, 4);
    memcpy(&version, blob + 4, 4);
    if (magic != kWordcountBlobMagic) return "bad magic";
    if (version != kWordcountBlobVersion) return "unknown version";
    WordcountBlob b;
    b.max_chunk_bytes = wordcount_blob_u64(blob, 1);
    b.n_unique = wordcount_blob_u64(blob, 2);
    b.n_bytes = wordcount_blob_u64(blob, 3);
    b.n_pieces = wordcount_blob_u64(blob, 4);
    b.n_chunks_total = wordcount_blob_u64(blob, 5);
    b.chunk_base = wordcount_blob_u64(blob, 6);
    if (b.max_chunk_bytes > 0x7FFFFFFFull) return "max_chunk_bytes out of range";
    const uint64_t body = n - kWordcountBlobHeader;
    if (b.n_unique >= 0xFFFFFFFFull || b.n_unique > body / 24 || b.n_bytes > body - 24 * b.n_unique ||
        wordcount_blob_size(b.n_unique, b.n_bytes) != n)
        return "sizes do not match the blob's length (truncated?)";
    b.ends = blob + kWordcountBlobHeader;
    b.weights = b.ends + 8 * b.n_unique;
    b.first_chunk = b.weights + 8 * b.n_unique;
    b.text = b.first_chunk + 8 * b.n_unique;
    uint64_t end = 0, first = 0, sum = 0;
    for (uint64_t e = 0; e < b.n_unique; ++e) {
        const uint64_t this_end = wordcount_blob_u64(b.ends, e), w = wordcount_blob_u64(b.weights, e),
                       f = wordcount_blob_u64(b.first_chunk, e);
        if (this_end <= end) return "ends are not strictly ascending";
        if (w == 0) return "a weight is 0";
        if ((e && f <= first) || f >= b.chunk_base) return "first_chunk is not strictly ascending below chunk_base";
        if (sum + w < sum) return "the weights' sum is not n_chunks_total";
        end = this_end;
        first = f;
        sum += w;
    }
    if (end != b.n_bytes) return "ends do not end at n_bytes";
    if (sum != b.n_chunks_total) return "the weights' sum is not n_chunks_total";
    *out = b;
    return nullptr;
}

#ifndef __HIP_DEVICE_COMPILE__
struct WordcountHost {
    uint32_t max_chunk_bytes = kDedupMaxChunkBytes, hash_bits = 64;
    std::vector<uint8_t> text;
    std::vector<uint64_t> ends, weights, first_chunk;
    std::vector<unsigned long long> slots;
    uint32_t bits = 0;
    uint64_t n_pieces = 0, n_chunks_total = 0, n_rebuilds = 0;
    uint64_t chunk_base = 0;               // chunks of the concatenated list before the next piece
    bool overflow = false;

    void claim(unsigned long long h, uint64_t entry) {
        const uint64_t mask = slots.size() - 1;
        uint64_t pos = dedup_home(h, bits);
        while (slots[pos] != kDedupEmpty) pos = (pos + 1) & mask;
        slots[pos] = dedup_slot(dedup_tag(h), entry);
    }
    uint64_t start_of(uint64_t entry) const { return entry ? ends[entry - 1] : 0; }

    // steps 1 - 4 over a source: nu chunks in ptext with ends, weights (u32 of a piece, u64 of a table) and first_chunk,
    // pairwise distinct wherever they are hashed; the weights count `repeat` times and first_chunk is moved on by `base`
    template <typename W>
    void fold(const uint8_t *ptext, const uint64_t *pends, const W *pweights, const uint64_t *pfirst, uint64_t nu,
              uint32_t repeat, uint64_t base) {
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
        // lookup, against the table as it was before the source
        std::vector<uint8_t> is_new(nu, 1);
        std::vector<unsigned long long> hash(nu, 0);
        for (uint64_t j = 0; j < nu; ++j) {
            const uint64_t s = j ? pends[j - 1] : 0, len = pends[j] - s;
            const unsigned long long add_w = wordcount_sat_mul(pweights[j], repeat);
            if (add_w >= kWordcountWeightLimit) overflow = true;
            if (len > max_chunk_bytes) continue;
            const unsigned long long h = hash[j] = dedup_hash(ptext + s, len, hash_bits);
            for (uint64_t pos = dedup_home(h, bits); slots[pos] != kDedupEmpty; pos = (pos + 1) & mask) {
                const uint64_t e = slots[pos] & 0xFFFFFFFFull, es = start_of(e);
                if (dedup_tag(slots[pos]) == dedup_tag(h) && ends[e] - es == len &&
                    dedup_equal(ptext + s, text.data() + es, len)) {
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
            const uint64_t s = j ? pends[j - 1] : 0, len = pends[j] - s;
            text.insert(text.end(), ptext + s, ptext + s + len);
            ends.push_back(text.size());
            weights.push_back(wordcount_sat_mul(pweights[j], repeat));
            first_chunk.push_back(base + pfirst[j]);
            if (len <= max_chunk_bytes) claim(hash[j], ends.size() - 1);
        }
    }

    // one piece: chunk c is piece_text[c ? piece_ends[c - 1] : 0 .. piece_ends[c]), none empty; counted `repeat` times
    void add(const uint8_t *piece_text, const uint64_t *piece_ends, uint64_t n_chunks, uint32_t repeat) {
        const DedupHost p = dedup_host(piece_text, piece_ends, n_chunks, max_chunk_bytes, hash_bits);
        fold(p.text.data(), p.ends.data(), p.weights.data(), p.first_chunk.data(), p.weights.size(), repeat, chunk_base);
        n_chunks_total += n_chunks * repeat;
        chunk_base += n_chunks * repeat;
        ++n_pieces;
    }

    // another table, counted with the same max_chunk_bytes (else, or for itself: false and nothing changes): this one
    // becomes the count of its own pieces followed by o's
    bool merge(const WordcountHost &o) {
        if (&o == this || o.max_chunk_bytes != max_chunk_bytes) return false;
        fold(o.text.data(), o.ends.data(), o.weights.data(), o.first_chunk.data(), o.ends.size(), 1, chunk_base);
        if (o.overflow) overflow = true;
        n_chunks_total += o.n_chunks_total;
        chunk_base += o.chunk_base;
        n_pieces += o.n_pieces;
        return true;
    }

    std::vector<uint8_t> to_blob() const {
        std::vector<uint8_t> blob(wordcount_blob_size(ends.size(), text.size()), 0);
        const uint32_t head[2] = {kWordcountBlobMagic, kWordcountBlobVersion};
        const uint64_t fields[6] = {max_chunk_bytes, ends.size(), text.size(), n_pieces, n_chunks_total, chunk_base};
        memcpy(blob.data(), head, 8);
        memcpy(blob.data() + 8, fields, 48);
        uint8_t *at = blob.data() + kWordcountBlobHeader;
        for (const std::vector<uint64_t> *v : {&ends, &weights, &first_chunk}) {
            if (!v->empty()) memcpy(at, v->data(), 8 * v->size());
            at += 8 * v->size();
        }
        if (!text.empty()) memcpy(at, text.data(), text.size());
        return blob;
    }

    // merge of a serialised table that nobody vouches for.  Refused -- false, the rule in *why, nothing changed -- when
    // wordcount_blob_check refuses it, when it was counted with another max_chunk_bytes, or when two of its hashed
    // chunks have the same bytes (the property the fold relies on: checked through a scratch table, as on the device)
    bool from_blob(const uint8_t *blob, uint64_t n, const char **why) {
        WordcountBlob b;
        if ((*why = wordcount_blob_check(blob, n, &b)) != nullptr) return false;
        if (b.max_chunk_bytes != max_chunk_bytes) { *why = "counted with another max_chunk_bytes"; return false; }
        WordcountHost o;
        o.max_chunk_bytes = max_chunk_bytes;
        o.hash_bits = hash_bits;
        o.text.assign(b.text, b.text + b.n_bytes);
        for (uint64_t e = 0; e < b.n_unique; ++e) {
            o.ends.push_back(wordcount_blob_u64(b.ends, e));
            o.weights.push_back(wordcount_blob_u64(b.weights, e));
            o.first_chunk.push_back(wordcount_blob_u64(b.first_chunk, e));
        }
        o.n_pieces = b.n_pieces;
        o.n_chunks_total = b.n_chunks_total;
        o.chunk_base = b.chunk_base;
        o.bits = dedup_table_bits(b.n_unique);
        o.slots.assign(1ull << o.bits, kDedupEmpty);
        const uint64_t mask = o.slots.size() - 1;
        for (uint64_t e = 0; e < b.n_unique; ++e) {
            const uint64_t s = o.start_of(e), len = o.ends[e] - s;
            if (len > max_chunk_bytes) continue;
            const unsigned long long h = dedup_hash(o.text.data() + s, len, hash_bits);
            uint64_t pos = dedup_home(h, o.bits);
            for (; o.slots[pos] != kDedupEmpty; pos = (pos + 1) & mask) {
                const uint64_t r = o.slots[pos] & 0xFFFFFFFFull, rs = o.start_of(r);
                if (dedup_tag(o.slots[pos]) == dedup_tag(h) && o.ends[r] - rs == len &&
                    dedup_equal(o.text.data() + s, o.text.data() + rs, len)) {
                    *why = "a hashed chunk is present twice";
                    return false;
                }
            }
            o.slots[pos] = dedup_slot(dedup_tag(h), e);
        }
        return merge(o);
    }
};
#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace mbpe

#endif
