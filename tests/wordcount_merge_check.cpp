// WordcountHost::merge, to_blob and from_blob (csrc/wordcount.h) against a std::map recount of the whole chunk list, on
// cases this program generates: random pieces counted into 2, 3 and 7 tables that are merged as a chain, as a tree and
// through blobs, hash_bits 64, 4 and 0, a 2,000-entry table merged into a 16-entry one (the target's table is rebuilt),
// chunks above max_chunk_bytes on both sides, the 2^31 limit, and one corrupt blob per rule of the check, each of which
// must be refused with the target unchanged.  Built plain and with -fsanitize=address,undefined by
// tests/test_wordcount_merge_cpu.py.
#include "wordcount.h"

#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <vector>

namespace {

using mbpe::WordcountHost;

unsigned long long rng_state = 0x2545F4914F6CDD1Dull;
uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}

int failures = 0, cases = 0;
void expect(bool ok, const char *what, uint32_t hash_bits) {
    ++cases;
    if (ok) return;
    ++failures;
    std::printf("FAIL %s (hash_bits %u)\n", what, hash_bits);
}

using Piece = std::vector<std::string>;

WordcountHost fresh(uint32_t max_chunk, uint32_t hash_bits) {
    WordcountHost w;
    w.max_chunk_bytes = max_chunk;
    w.hash_bits = hash_bits;
    return w;
}

void add(WordcountHost *w, const Piece &p) {
    std::vector<uint8_t> text;
    std::vector<uint64_t> ends;
    for (const std::string &c : p) {
        text.insert(text.end(), c.begin(), c.end());
        ends.push_back(text.size());
    }
    w->add(text.data(), ends.data(), p.size(), 1);
}

WordcountHost count(const std::vector<Piece> &pieces, size_t from, size_t to, uint32_t max_chunk, uint32_t hash_bits) {
    WordcountHost w = fresh(max_chunk, hash_bits);
    for (size_t k = from; k < to; ++k) add(&w, pieces[k]);
    return w;
}

// everything the statement covers (the slots may differ: they place, they decide nothing)
bool same(const WordcountHost &a, const WordcountHost &b) {
    return a.text == b.text && a.ends == b.ends && a.weights == b.weights && a.first_chunk == b.first_chunk &&
           a.n_pieces == b.n_pieces && a.n_chunks_total == b.n_chunks_total && a.chunk_base == b.chunk_base &&
           a.overflow == b.overflow && a.max_chunk_bytes == b.max_chunk_bytes;
}

// the recount: one walk over the whole list with a std::map
bool recount(const WordcountHost &got, const std::vector<Piece> &pieces, uint32_t max_chunk) {
    std::map<std::string, size_t> index;
    std::vector<std::string> uniq;
    std::vector<uint64_t> weights, first;
    uint64_t at = 0;
    for (const Piece &p : pieces)
        for (const std::string &c : p) {
            const bool hashed = c.size() <= max_chunk;
            const auto it = hashed ? index.find(c) : index.end();
            if (it != index.end()) { weights[it->second] += 1; ++at; continue; }
            if (hashed) index[c] = uniq.size();
            uniq.push_back(c);
            weights.push_back(1);
            first.push_back(at++);
        }
    std::vector<uint8_t> text;
    std::vector<uint64_t> ends;
    for (const std::string &c : uniq) {
        text.insert(text.end(), c.begin(), c.end());
        ends.push_back(text.size());
    }
    return got.text == text && got.ends == ends && got.weights == weights && got.first_chunk == first &&
           got.n_chunks_total == at && got.chunk_base == at && got.n_pieces == pieces.size() && !got.overflow;
}

bool import(WordcountHost *into, const WordcountHost &from) {
    const std::vector<uint8_t> blob = from.to_blob();
    const char *why = nullptr;
    return into->from_blob(blob.data(), blob.size(), &why) && why == nullptr;
}

// the pieces counted into n_tables tables (cut at `cuts`), merged as a chain, as a tree, and through blobs
void check(const std::vector<Piece> &pieces, uint32_t n_tables, uint32_t max_chunk, uint32_t hash_bits, const char *what,
           uint64_t min_rebuilds = 0) {
    std::vector<size_t> at{0};
    for (uint32_t t = 1; t < n_tables; ++t) at.push_back(pieces.size() * t / n_tables);
    at.push_back(pieces.size());
    std::vector<WordcountHost> tables;
    for (uint32_t t = 0; t < n_tables; ++t) tables.push_back(count(pieces, at[t], at[t + 1], max_chunk, hash_bits));
    const WordcountHost whole = count(pieces, 0, pieces.size(), max_chunk, hash_bits);
    expect(recount(whole, pieces, max_chunk), "one object against the recount", hash_bits);
    // a chain ((T0 + T1) + T2) + ...
    WordcountHost chain = tables[0];
    bool merged = true;
    for (uint32_t t = 1; t < n_tables; ++t) merged = chain.merge(tables[t]) && merged;
    expect(merged && same(chain, whole) && recount(chain, pieces, max_chunk) && chain.n_rebuilds >= min_rebuilds, what,
           hash_bits);
    // a tree: T0 + (T1 + (T2 + ...)), built from the right
    WordcountHost right = tables[n_tables - 1];
    for (uint32_t t = n_tables - 1; t-- > 1;) {
        WordcountHost left = tables[t];
        merged = left.merge(right) && merged;
        right = left;
    }
    WordcountHost tree = tables[0];
    if (n_tables > 1) merged = tree.merge(right) && merged;
    expect(merged && same(tree, whole), "a tree against the chain", hash_bits);
    // through blobs, into an empty object first: an import, whose export is the blob again
    WordcountHost by_blob = fresh(max_chunk, hash_bits);
    bool ok = true;
    for (uint32_t t = 0; t < n_tables; ++t) ok = import(&by_blob, tables[t]) && ok;
    expect(ok && same(by_blob, whole), "merged through blobs", hash_bits);
    WordcountHost again = fresh(max_chunk, hash_bits);
    expect(import(&again, whole) && again.to_blob() == whole.to_blob() && same(again, whole), "the blob round trip",
           hash_bits);
    // the tables themselves were left alone
    for (uint32_t t = 0; t < n_tables; ++t)
        expect(same(tables[t], count(pieces, at[t], at[t + 1], max_chunk, hash_bits)), "the merged table is unchanged",
               hash_bits);
}

std::string random_chunk(uint32_t max_len, uint32_t n_sym) {
    std::string s(1 + rnd(max_len), 'a');
    for (char &c : s) c = (char)('a' + rnd(n_sym));
    return s;
}

void put64(std::vector<uint8_t> *blob, uint64_t at, uint64_t v) { memcpy(blob->data() + at, &v, 8); }
uint64_t get64(const std::vector<uint8_t> &blob, uint64_t at) { return mbpe::wordcount_blob_u64(blob.data() + at, 0); }

// one corrupt blob per rule: refused, and the target as it was
void refusals(uint32_t hash_bits) {
    std::vector<Piece> pieces(2);
    for (int i = 0; i < 40; ++i) pieces[0].push_back("t" + std::to_string(i % 25));
    for (int i = 0; i < 40; ++i) pieces[1].push_back("s" + std::to_string(i % 30));
    pieces[1].push_back(std::string(300, 'L'));
    pieces[1].push_back(std::string(300, 'L'));
    const WordcountHost source = count(pieces, 1, 2, 256, hash_bits);
    const std::vector<uint8_t> good = source.to_blob();
    const uint64_t nu = source.ends.size(), ends_at = mbpe::kWordcountBlobHeader, weights_at = ends_at + 8 * nu,
                   first_at = weights_at + 8 * nu, text_at = first_at + 8 * nu;
    struct Case { const char *rule; std::function<void(std::vector<uint8_t> *)> edit; };
    const std::vector<Case> all = {
        {"truncated", [&](std::vector<uint8_t> *b) { b->resize(b->size() - 16); }},
        {"shorter than the header", [&](std::vector<uint8_t> *b) { b->resize(40); }},
        {"magic", [&](std::vector<uint8_t> *b) { (*b)[0] ^= 1; }},
        {"version", [&](std::vector<uint8_t> *b) { (*b)[4] += 1; }},
        {"n_unique beyond the blob", [&](std::vector<uint8_t> *b) { put64(b, 16, nu + 2); }},
        {"n_unique enormous", [&](std::vector<uint8_t> *b) { put64(b, 16, ~0ull / 8); }},
        {"n_bytes beyond the blob", [&](std::vector<uint8_t> *b) { put64(b, 24, get64(*b, 24) + 16); }},
        {"n_bytes enormous", [&](std::vector<uint8_t> *b) { put64(b, 24, ~0ull - 7); }},
        {"another max_chunk_bytes", [&](std::vector<uint8_t> *b) { put64(b, 8, 255); }},
        {"an end out of order", [&](std::vector<uint8_t> *b) { put64(b, ends_at + 8, get64(*b, ends_at)); }},
        {"the last end is not n_bytes", [&](std::vector<uint8_t> *b) { put64(b, weights_at - 8, get64(*b, weights_at - 8) - 1); }},
        {"an end beyond n_bytes", [&](std::vector<uint8_t> *b) { put64(b, weights_at - 8, ~0ull); }},
        {"weight 0", [&](std::vector<uint8_t> *b) { put64(b, weights_at + 8, 0); }},
        {"first_chunk out of order", [&](std::vector<uint8_t> *b) { put64(b, first_at + 16, get64(*b, first_at + 8)); }},
        {"first_chunk at chunk_base", [&](std::vector<uint8_t> *b) { put64(b, text_at - 8, get64(*b, 48)); }},
        {"the weights' sum", [&](std::vector<uint8_t> *b) { put64(b, 40, get64(*b, 40) + 1); }},
        {"a weight that wraps the sum", [&](std::vector<uint8_t> *b) { put64(b, weights_at, ~0ull); }},
        {"a hashed chunk twice", [&](std::vector<uint8_t> *b) { memcpy(b->data() + text_at + 2, b->data() + text_at, 2); }},
    };
    for (const Case &c : all) {
        std::vector<uint8_t> blob = good;
        c.edit(&blob);
        // an exact-size heap copy, so that a read beyond the blob is seen by the sanitizer
        std::vector<uint8_t> exact(blob.begin(), blob.end());
        exact.shrink_to_fit();
        WordcountHost target = count(pieces, 0, 1, 256, hash_bits);
        const WordcountHost before = target;
        const char *why = nullptr;
        const bool taken = target.from_blob(exact.data(), exact.size(), &why);
        expect(!taken && why != nullptr && same(target, before) && target.slots == before.slots, c.rule, hash_bits);
    }
    // the unedited blob is taken, and the two long chunks stay two entries
    WordcountHost target = count(pieces, 0, 1, 256, hash_bits);
    expect(import(&target, source) && recount(target, pieces, 256), "the good blob", hash_bits);
    // merge refuses itself and another max_chunk_bytes
    WordcountHost other = count(pieces, 1, 2, 255, hash_bits);
    const WordcountHost before = target;
    expect(!target.merge(target) && !target.merge(other) && same(target, before), "merge(w, w) and other options", hash_bits);
}

}  // namespace

int main() {
    const uint32_t bits[] = {64, 4, 0};
    for (uint32_t hb : bits) {
        check({{}, {}}, 2, 256, hb, "empty tables");
        check({{"a", "b", "a"}, {}, {"b", "c"}}, 3, 256, hb, "tiny");
        for (int round = 0; round < 8; ++round) {
            std::vector<Piece> pieces;
            const uint32_t n_pieces = 7 + rnd(8), max_len = 1 + rnd(12), n_sym = 1 + rnd(4);
            for (uint32_t p = 0; p < n_pieces; ++p) {
                Piece piece;
                const uint32_t n = rnd(4) ? rnd(400) : 0;
                for (uint32_t i = 0; i < n; ++i) piece.push_back(random_chunk(max_len, n_sym));
                pieces.push_back(piece);
            }
            for (uint32_t n_tables : {2u, 3u, 7u}) check(pieces, n_tables, 256, hb, "random");
        }
        // a 2,000-entry table into a 16-entry one: the target's table is rebuilt, and its entries are found afterwards
        {
            std::vector<Piece> pieces(3);
            for (uint32_t i = 0; i < 16; ++i) pieces[0].push_back("w" + std::to_string(i));
            for (uint32_t i = 16; i < 2016; ++i) pieces[1].push_back("w" + std::to_string(i));
            for (uint32_t i = 0; i < 40; ++i) pieces[2].push_back("w" + std::to_string(i * 50));
            check(pieces, 3, 256, hb, "2,000 entries into 16", 2);
        }
        // lengths around max_chunk_bytes on both sides: the longer ones are appended every time
        for (uint32_t mc : {1u, 7u, 256u}) {
            std::vector<Piece> pieces(4);
            for (Piece &p : pieces)
                for (uint32_t len : {mc - 1 ? mc - 1 : 1u, mc, mc + 1, mc + 2}) {
                    p.push_back(std::string(len, 'q'));
                    p.push_back("ab");
                }
            check(pieces, 2, mc, hb, "around max_chunk_bytes");
            check(pieces, 3, mc, hb, "around max_chunk_bytes, three tables");
        }
        refusals(hb);
    }
    // the limit of the weighted load: 2^31 - 1 in one table, the chunk once more in the other
    {
        const uint8_t text[2] = {'h', 'i'};
        const uint64_t ends[1] = {2};
        WordcountHost a, b;
        a.add(text, ends, 1, 0x7FFFFFFFu);
        b.add(text, ends, 1, 1);
        bool ok = !a.overflow && a.merge(b) && a.overflow && a.weights[0] == 0x80000000ull && a.n_chunks_total == 0x80000000ull;
        WordcountHost c;
        c.add(text, ends, 1, 0x7FFFFFFFu);
        ok = ok && import(&c, b) && c.overflow && same(c, a);
        expect(ok, "the 2^31 limit", 64);
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
