// The host restatement of csrc/wordcount.h against a std::map, on cases this program generates: random chunk lists cut
// into 1, 2 and 7 pieces with empty pieces between them, hash_bits 64, 4 and 0, growing pieces that rebuild the table
// several times, repeat > 1, chunk lengths around max_chunk_bytes spread over two pieces, and the 2^31 limit.  Built
// plain and with -fsanitize=address,undefined by tests/test_wordcount_cpu.py.
#include "wordcount.h"

#include <algorithm>
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace {

unsigned long long rng_state = 88172645463325252ull;
uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}

int failures = 0, cases = 0;

using Piece = std::pair<std::vector<std::string>, uint32_t>;      // chunks, repeat

// accumulating the pieces must give one dedup of the written-out list: every piece `repeat` times, back to back
mbpe::WordcountHost check(const std::vector<Piece> &pieces, uint32_t max_chunk, uint32_t hash_bits, const char *what,
                          uint64_t min_rebuilds = 0) {
    ++cases;
    mbpe::WordcountHost got;
    got.max_chunk_bytes = max_chunk;
    got.hash_bits = hash_bits;
    std::map<std::string, size_t> index;
    std::vector<std::string> uniq;
    std::vector<uint64_t> weights, first;
    uint64_t at = 0;
    for (const Piece &p : pieces) {
        std::vector<uint8_t> text;
        std::vector<uint64_t> ends;
        for (const std::string &c : p.first) {
            text.insert(text.end(), c.begin(), c.end());
            ends.push_back(text.size());
        }
        got.add(text.data(), ends.data(), p.first.size(), p.second);
        for (uint32_t r = 0; r < p.second; ++r)
            for (const std::string &c : p.first) {
                const bool hashed = c.size() <= max_chunk;
                const auto it = hashed ? index.find(c) : index.end();
                // (a long chunk passes through once per occurrence of one copy; the copies add to its weight, as the
                // repeat of a piece is defined: weights times repeat, order and first_chunk of one copy)
                if (it != index.end()) { weights[it->second] += 1; ++at; continue; }
                if (!hashed && r > 0) { ++at; continue; }
                if (hashed) index[c] = uniq.size();
                uniq.push_back(c);
                weights.push_back(hashed ? 1 : p.second);
                first.push_back(at++);
            }
    }
    std::vector<uint8_t> want_text;
    std::vector<uint64_t> want_ends;
    for (const std::string &c : uniq) {
        want_text.insert(want_text.end(), c.begin(), c.end());
        want_ends.push_back(want_text.size());
    }
    const bool ok = got.text == want_text && got.ends == want_ends && got.weights == weights && got.first_chunk == first &&
                    got.n_chunks_total == at && got.n_pieces == pieces.size() && got.n_rebuilds >= min_rebuilds &&
                    !got.overflow;
    if (!ok) {
        ++failures;
        std::printf("FAIL %s: max_chunk %u hash_bits %u, %zu pieces, %zu unique (want %zu), %llu rebuilds\n", what, max_chunk,
                    hash_bits, pieces.size(), got.weights.size(), uniq.size(), (unsigned long long)got.n_rebuilds);
    }
    return got;
}

std::string random_chunk(uint32_t max_len, uint32_t n_sym) {
    std::string s(1 + rnd(max_len), 'a');
    for (char &c : s) c = (char)('a' + rnd(n_sym));
    return s;
}

// chunks cut into n_pieces pieces at random places, an empty piece after each, the repeats as given (cycled)
std::vector<Piece> cut(const std::vector<std::string> &chunks, uint32_t n_pieces, const std::vector<uint32_t> &repeats) {
    std::vector<size_t> at{0, chunks.size()};
    for (uint32_t i = 1; i < n_pieces; ++i) at.push_back(rnd((uint32_t)chunks.size() + 1));
    std::sort(at.begin(), at.end());
    std::vector<Piece> out;
    for (size_t i = 0; i + 1 < at.size(); ++i) {
        out.push_back({std::vector<std::string>(chunks.begin() + at[i], chunks.begin() + at[i + 1]),
                       repeats[i % repeats.size()]});
        out.push_back({{}, 1});
    }
    return out;
}

}  // namespace

int main() {
    const uint32_t bits[] = {64, 4, 0};
    for (uint32_t hb : bits) {
        check({}, 256, hb, "no piece");
        check({{{}, 1}, {{}, 3}}, 256, hb, "empty pieces");
        check({{{"a"}, 1}, {{"a"}, 1}, {{"b", "a"}, 1}}, 256, hb, "tiny");
        for (int round = 0; round < 12; ++round) {
            std::vector<std::string> chunks;
            const uint32_t n = 1 + rnd(2500), max_len = 1 + rnd(12), n_sym = 1 + rnd(4);
            for (uint32_t i = 0; i < n; ++i) chunks.push_back(random_chunk(max_len, n_sym));
            for (uint32_t n_pieces : {1u, 2u, 7u}) {
                check(cut(chunks, n_pieces, {1}), 256, hb, "random");
                check(cut(chunks, n_pieces, {3, 1, 2}), 256, hb, "random with repeats");
            }
        }
        // pieces of distinct chunks that grow: the table is rebuilt several times, and the first piece is found again
        std::vector<Piece> growing;
        uint32_t next = 0;
        for (uint32_t n : {16u, 64u, 256u, 2000u}) {
            std::vector<std::string> p;
            for (uint32_t i = 0; i < n; ++i) p.push_back("w" + std::to_string(next++));
            growing.push_back({p, 1});
        }
        growing.push_back(growing[0]);
        const mbpe::WordcountHost g = check(growing, 256, hb, "growing", 3);
        ++cases;
        if (g.weights.size() != 2336 || g.weights[0] != 2 || g.weights[15] != 2 || g.weights[16] != 1) {
            ++failures;
            std::printf("FAIL growing: the first piece was not found again\n");
        }
        // lengths around max_chunk_bytes, each in both pieces: the longer ones pass through every time
        for (uint32_t mc : {0u, 1u, 7u, 256u}) {
            std::vector<Piece> two;
            for (int rep = 0; rep < 2; ++rep) {
                std::vector<std::string> p;
                for (uint32_t len : {mc ? mc - 1 : 1u, mc ? mc : 1u, mc + 1, mc + 2}) {
                    p.push_back(std::string(len ? len : 1, 'q'));
                    p.push_back("ab");
                }
                two.push_back({p, 1});
            }
            check(two, mc, hb, "around max_chunk_bytes");
            two[1].second = 3;
            check(two, mc, hb, "around max_chunk_bytes, repeated");
        }
    }
    // the limit of the weighted load: 2^31 - 1 is a weight, one more occurrence is overflow, and the sum saturates
    {
        ++cases;
        mbpe::WordcountHost w;
        const uint8_t text[2] = {'h', 'i'};
        const uint64_t ends[1] = {2};
        w.add(text, ends, 1, 0x7FFFFFFFu);
        bool ok = !w.overflow && w.weights.size() == 1 && w.weights[0] == 0x7FFFFFFFull && w.n_chunks_total == 0x7FFFFFFFull;
        w.add(text, ends, 1, 1);
        ok = ok && w.overflow && w.weights[0] == 0x80000000ull;
        for (int i = 0; i < 5; ++i) w.add(text, ends, 1, 0xFFFFFFFFu);
        ok = ok && w.overflow && w.weights[0] == 0x80000000ull + 5ull * 0xFFFFFFFFull;
        ok = ok && mbpe::wordcount_sat_add(~0ull - 1, 5) == ~0ull && mbpe::wordcount_sat_mul(1ull << 40, 1u << 30) == ~0ull &&
             mbpe::wordcount_sat_mul(7, 3) == 21 && mbpe::wordcount_sat_add(7, 3) == 10;
        if (!ok) {
            ++failures;
            std::printf("FAIL the 2^31 limit\n");
        }
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
