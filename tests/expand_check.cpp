// The host restatement of csrc/expand.h against a per-chunk concatenation, and dedup_host's unique_of (csrc/dedup.h)
// against a std::map, on cases this program generates: the chunk counts at the span and workgroup edges (0, 1, 700
// equal, 600 distinct, 1,023 .. 1,025, 4,095 .. 4,097), run lengths that start a span's output at every residue mod 16
// bytes for 4- and 2-byte elements, a 5,000-token run three times between one-token runs, empty runs, indices beyond
// the table, and hash_bits 64, 4 and 0.  Built plain and with -fsanitize=address,undefined by tests/test_expand_cpu.py.
#include "dedup.h"
#include "expand.h"

#include <cstdio>
#include <map>
#include <string>
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

// run j has lens[j] tokens; chunk c copies run of[c]
template <typename T>
void check_expand(const std::vector<uint32_t> &lens, const std::vector<uint32_t> &of, const char *what) {
    std::vector<T> table;
    std::vector<unsigned long long> ends;
    for (size_t j = 0; j < lens.size(); ++j) {
        for (uint32_t k = 0; k < lens[j]; ++k) table.push_back((T)(j * 131u + k * 7u + 1u));
        ends.push_back(table.size());
    }
    std::vector<T> want;
    std::vector<uint64_t> want_ends;
    for (uint32_t j : of) {
        if (j < lens.size()) {
            const size_t s = j ? ends[j - 1] : 0;
            want.insert(want.end(), table.begin() + s, table.begin() + ends[j]);
        }
        want_ends.push_back(want.size());
    }
    for (uint64_t addr = 0; addr < 16; addr += sizeof(T)) {
        ++cases;
        std::vector<uint64_t> got_ends;
        const std::vector<T> got = mbpe::expand_host<T>(table.data(), table.size(), ends.data(), ends.size(), of.data(),
                                                        of.size(), 4096 + addr, &got_ends);
        if (got != want || got_ends != want_ends) {
            ++failures;
            std::printf("FAIL expand %s: %zu-byte elements, address %llu, %zu runs, %zu chunks, %zu tokens (want %zu)\n", what,
                        sizeof(T), (unsigned long long)addr, lens.size(), of.size(), got.size(), want.size());
        }
    }
}

void check_both(const std::vector<uint32_t> &lens, const std::vector<uint32_t> &of, const char *what) {
    check_expand<uint32_t>(lens, of, what);
    check_expand<uint16_t>(lens, of, what);
}

void check_map(const std::vector<std::string> &chunks, uint32_t max_chunk, uint32_t hash_bits, const char *what) {
    ++cases;
    std::vector<uint8_t> text;
    std::vector<uint64_t> ends;
    for (const std::string &c : chunks) {
        text.insert(text.end(), c.begin(), c.end());
        ends.push_back(text.size());
    }
    const mbpe::DedupHost got = mbpe::dedup_host(text.data(), ends.data(), chunks.size(), max_chunk, hash_bits);
    std::map<std::string, uint32_t> index;
    std::vector<uint32_t> want;
    uint32_t n_unique = 0;
    for (const std::string &c : chunks) {
        const bool hashed = c.size() <= max_chunk;
        const auto it = hashed ? index.find(c) : index.end();
        if (it != index.end()) { want.push_back(it->second); continue; }
        if (hashed) index[c] = n_unique;
        want.push_back(n_unique++);
    }
    bool ok = got.unique_of == want && got.weights.size() == n_unique;
    // and the map names a chunk with the same bytes
    for (size_t c = 0; ok && c < chunks.size(); ++c) {
        const uint32_t j = got.unique_of[c];
        const uint64_t s = j ? got.ends[j - 1] : 0;
        ok = std::string(got.text.begin() + s, got.text.begin() + got.ends[j]) == chunks[c];
    }
    if (!ok) {
        ++failures;
        std::printf("FAIL unique_of %s: max_chunk %u hash_bits %u, %zu chunks\n", what, max_chunk, hash_bits, chunks.size());
    }
}

}  // namespace

int main() {
    // ---- the expansion ----
    check_both({}, {}, "nothing");
    check_both({3}, {0}, "one chunk");
    check_both({2}, std::vector<uint32_t>(700, 0), "700 equal chunks");
    {
        std::vector<uint32_t> lens, of;
        for (uint32_t j = 0; j < 600; ++j) { lens.push_back(1 + j % 5); of.push_back(j); }
        check_both(lens, of, "600 distinct chunks");
    }
    for (uint32_t n : {1023u, 1024u, 1025u, 4095u, 4096u, 4097u}) {
        std::vector<uint32_t> lens = {1, 2, 3, 0, 5, 1, 1, 9}, of;
        for (uint32_t c = 0; c < n; ++c) of.push_back(rnd((uint32_t)lens.size()));
        check_both(lens, of, "span and workgroup edges");
    }
    // the first span holds r tokens more than a multiple of 8: the second span's output starts at every residue
    for (uint32_t r = 0; r < 8; ++r) {
        std::vector<uint32_t> lens = {1, 2, 1 + r}, of(1024, 0);
        of[17] = 2;
        for (uint32_t c = 0; c < 300; ++c) of.push_back(c % 2);
        check_both(lens, of, "residues");
    }
    {
        std::vector<uint32_t> lens = {1, 5000, 1}, of = {0, 1, 2, 1, 0, 0, 1, 2};
        check_both(lens, of, "a long run three times");
        lens = {5000, 5001, 4999, 1};
        of = {3, 0, 3, 1, 3, 2, 3};
        check_both(lens, of, "long runs that pass through");
    }
    {
        std::vector<uint32_t> lens = {0, 3, 0, 0, 2, 0}, of;
        for (uint32_t c = 0; c < 2500; ++c) of.push_back(rnd(8));       // (6 and 7: beyond the table, nothing)
        check_both(lens, of, "empty runs and indices beyond the table");
        check_both({0, 0}, std::vector<uint32_t>(1500, 1), "only empty runs");
    }
    for (int round = 0; round < 12; ++round) {
        std::vector<uint32_t> lens, of;
        const uint32_t n_runs = 1 + rnd(40), n = rnd(5000);
        for (uint32_t j = 0; j < n_runs; ++j) lens.push_back(rnd(7) ? rnd(6) : rnd(300));
        for (uint32_t c = 0; c < n; ++c) of.push_back(rnd(n_runs));
        check_both(lens, of, "random");
    }
    // the pieces themselves
    {
        ++cases;
        const mbpe::ExpandPieces a = mbpe::expand_pieces(4096 + 4, 2, 4), b = mbpe::expand_pieces(4096 + 6, 20, 2),
                                 c = mbpe::expand_pieces(4096, 9, 4), d = mbpe::expand_pieces(4096 + 12, 0, 4);
        if (a.head != 2 || a.n_vec != 0 || a.tail != 0 || b.head != 5 || b.n_vec != 1 || b.tail != 7 || c.head != 0 ||
            c.n_vec != 2 || c.tail != 1 || d.head != 0 || d.n_vec != 0 || d.tail != 0) {
            ++failures;
            std::printf("FAIL expand_pieces\n");
        }
    }
    // ---- unique_of ----
    for (uint32_t hb : {64u, 4u, 0u}) {
        check_map({}, 256, hb, "empty");
        check_map({"a"}, 256, hb, "one chunk");
        check_map(std::vector<std::string>(700, "same"), 256, hb, "700 equal chunks");
        std::vector<std::string> distinct;
        for (int i = 0; i < 600; ++i) distinct.push_back("w" + std::to_string(i));
        check_map(distinct, 256, hb, "600 distinct chunks");
        for (uint32_t n : {1023u, 1024u, 1025u, 4095u, 4096u, 4097u}) {
            std::vector<std::string> chunks;
            for (uint32_t i = 0; i < n; ++i) {
                std::string s(1 + rnd(4), 'a');
                for (char &ch : s) ch = (char)('a' + rnd(3));
                chunks.push_back(s);
            }
            check_map(chunks, 256, hb, "span and workgroup edges");
        }
        const std::string big(5000, 'z');
        check_map({"a", big, "b", big, "a", "a", big, "b"}, 8192, hb, "a long chunk three times, hashed");
        check_map({"a", big, "b", big, "a", "a", big, "b"}, 256, hb, "a long chunk three times, passing through");
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
