// The host restatement of csrc/dedup.h against a std::map, on cases this program generates: random chunk lists over
// small alphabets, hash_bits 64, 4 and 0 (every chunk in one probe sequence), chunk lengths around max_chunk_bytes,
// the empty input and a single chunk.  Built plain and with -fsanitize=address,undefined by tests/test_dedup_cpu.py.
#include "dedup.h"

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

void check(const std::vector<std::string> &chunks, uint32_t max_chunk, uint32_t hash_bits, const char *what) {
    ++cases;
    std::vector<uint8_t> text;
    std::vector<uint64_t> ends;
    for (const std::string &c : chunks) {
        text.insert(text.end(), c.begin(), c.end());
        ends.push_back(text.size());
    }
    const mbpe::DedupHost got = mbpe::dedup_host(text.data(), ends.data(), chunks.size(), max_chunk, hash_bits);

    // the reference: a map from bytes to the index among the unique chunks
    std::map<std::string, size_t> index;
    std::vector<std::string> uniq;
    std::vector<uint32_t> weights;
    std::vector<uint64_t> first;
    for (size_t i = 0; i < chunks.size(); ++i) {
        const std::string &c = chunks[i];
        const bool hashed = c.size() <= max_chunk;
        const auto it = hashed ? index.find(c) : index.end();
        if (it != index.end()) { weights[it->second] += 1; continue; }
        if (hashed) index[c] = uniq.size();
        uniq.push_back(c);
        weights.push_back(1);
        first.push_back(i);
    }
    std::vector<uint8_t> want_text;
    std::vector<uint64_t> want_ends;
    for (const std::string &c : uniq) {
        want_text.insert(want_text.end(), c.begin(), c.end());
        want_ends.push_back(want_text.size());
    }
    uint64_t sum = 0;
    for (uint32_t w : got.weights) sum += w;
    const bool ok = got.text == want_text && got.ends == want_ends && got.weights == weights && got.first_chunk == first &&
                    sum == chunks.size();
    if (!ok) {
        ++failures;
        std::printf("FAIL %s: max_chunk %u hash_bits %u, %zu chunks, %zu unique (want %zu)\n", what, max_chunk, hash_bits,
                    chunks.size(), got.weights.size(), uniq.size());
    }
}

std::string random_chunk(uint32_t max_len, uint32_t n_sym) {
    std::string s(1 + rnd(max_len), 'a');
    for (char &c : s) c = (char)('a' + rnd(n_sym));
    return s;
}

}  // namespace

int main() {
    const uint32_t bits[] = {64, 4, 0};
    for (uint32_t hb : bits) {
        check({}, 256, hb, "empty");
        check({"a"}, 256, hb, "one chunk");
        check({std::string(300, 'x')}, 256, hb, "one long chunk");
        check(std::vector<std::string>(100, "same"), 256, hb, "all equal");
        std::vector<std::string> distinct;
        for (int i = 0; i < 500; ++i) distinct.push_back("w" + std::to_string(i));
        check(distinct, 256, hb, "all distinct");
        for (int round = 0; round < 20; ++round) {
            std::vector<std::string> chunks;
            const uint32_t n = 1 + rnd(3000), max_len = 1 + rnd(12), n_sym = 1 + rnd(4);
            for (uint32_t i = 0; i < n; ++i) chunks.push_back(random_chunk(max_len, n_sym));
            check(chunks, 256, hb, "random");
        }
        // lengths around max_chunk_bytes, each twice: the longer ones pass through both times
        for (uint32_t mc : {0u, 1u, 7u, 256u}) {
            std::vector<std::string> chunks;
            for (int rep = 0; rep < 2; ++rep)
                for (uint32_t len : {mc ? mc - 1 : 1u, mc ? mc : 1u, mc + 1, mc + 2}) {
                    chunks.push_back(std::string(len ? len : 1, 'q'));
                    chunks.push_back("ab");
                }
            check(chunks, mc, hb, "around max_chunk_bytes");
        }
    }
    // the hash itself: the cut keeps the lowest bits, 0 bits is the constant 0
    const uint8_t probe[3] = {1, 2, 3};
    const unsigned long long h64 = mbpe::dedup_hash(probe, 3, 64);
    ++cases;
    if (mbpe::dedup_hash(probe, 3, 0) != 0 || mbpe::dedup_hash(probe, 3, 4) != (h64 & 15) ||
        mbpe::dedup_hash(probe, 3, 70) != h64 || mbpe::dedup_hash(probe, 2, 64) == h64) {
        ++failures;
        std::printf("FAIL hash_bits\n");
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
