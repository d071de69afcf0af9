// Stand-alone check of csrc/dropout.h on the host (tests/test_dropout_cpu.py builds it plain and under ASan + UBSan):
// the known answers of drop_hash, the threshold helper, and the per-chunk loop of the definition in two restatements
// on generated strings.
//   loop_walk   the sequential loop as the host tokenizer writes it: minimum over the surviving candidates, then one
//               left-to-right walk that steps over a replaced pair
//   loop_list   a brute-force restatement: the chunk as a linked list over byte starts; per round all surviving
//               instances are listed and sorted by (id, pos), and those of the smallest id are replaced in ascending
//               position unless the round already consumed their left token
#include "dropout.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <map>
#include <string>
#include <utility>
#include <vector>

using namespace mbpe;

namespace {

int failures = 0;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++failures;                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);           \
        }                                                                   \
    } while (0)

using Lookup = std::map<std::pair<uint32_t, uint32_t>, uint32_t>;
struct Result {
    std::vector<uint32_t> tok;
    std::vector<unsigned long long> pos;
    bool operator==(const Result &o) const { return tok == o.tok && pos == o.pos; }
};

Result loop_walk(const std::string &s, const Lookup &lut, unsigned long long base, unsigned long long seed,
                 unsigned long long threshold) {
    Result r;
    for (size_t i = 0; i < s.size(); ++i) {
        r.tok.push_back((uint8_t)s[i]);
        r.pos.push_back(base + i);
    }
    const uint32_t none = kTokNone;
    auto candidate = [&](size_t i) -> uint32_t {
        auto it = lut.find({r.tok[i], r.tok[i + 1]});
        if (it == lut.end() || dropout_dropped(seed, r.pos[i], it->second, threshold)) return none;
        return it->second;
    };
    for (;;) {
        uint32_t best = none;
        for (size_t i = 0; i + 1 < r.tok.size(); ++i) best = std::min(best, candidate(i));
        if (best == none) return r;
        Result out;
        for (size_t i = 0; i < r.tok.size();) {
            const bool hit = i + 1 < r.tok.size() && candidate(i) == best;
            out.tok.push_back(hit ? best : r.tok[i]);
            out.pos.push_back(r.pos[i]);
            i += hit ? 2 : 1;
        }
        r = out;
    }
}

Result loop_list(const std::string &s, const Lookup &lut, unsigned long long base, unsigned long long seed,
                 unsigned long long threshold) {
    const size_t n = s.size();
    std::vector<uint32_t> tok(n);
    std::vector<size_t> next(n);              // the byte index of the token after the one that starts here; n = none
    std::vector<char> alive(n, 1);
    for (size_t i = 0; i < n; ++i) {
        tok[i] = (uint8_t)s[i];
        next[i] = i + 1;
    }
    for (;;) {
        struct Inst { uint32_t id; size_t at; };
        std::vector<Inst> inst;
        for (size_t i = 0; i < n; ++i) {
            if (!alive[i] || next[i] >= n) continue;
            auto it = lut.find({tok[i], tok[next[i]]});
            if (it == lut.end()) continue;
            if ((unsigned long long)drop_hash(seed, base + i, it->second) < threshold) continue;
            inst.push_back({it->second, i});
        }
        if (inst.empty()) break;
        std::sort(inst.begin(), inst.end(), [](const Inst &a, const Inst &b) { return a.id != b.id ? a.id < b.id : a.at < b.at; });
        std::vector<char> consumed(n, 0);
        for (const Inst &k : inst) {
            if (k.id != inst[0].id) break;
            if (consumed[k.at]) continue;     // the instance to its left took this token
            const size_t right = next[k.at];
            consumed[right] = 1;
            alive[right] = 0;
            tok[k.at] = k.id;
            next[k.at] = next[right];
        }
    }
    Result r;
    for (size_t i = 0; i < n; ++i)
        if (alive[i]) {
            r.tok.push_back(tok[i]);
            r.pos.push_back(base + i);
        }
    return r;
}

void known_answers() {
    CHECK(drop_hash(0, 0, 256) == 0xa4a47e7eu);
    CHECK(drop_hash(0, 1, 256) == 0x57cb3d0cu);
    CHECK(drop_hash(1, 0, 256) == 0x926993adu);
    CHECK(drop_hash(42, 1023, 511) == 0xcac74bc6u);
    CHECK(drop_hash(~0ull, (1ull << 40) + 5, 65535) == 0x59525672u);
    CHECK(drop_hash(7, 1ull << 32, 16777215) == 0xf3b38aaau);
    CHECK(!dropout_dropped(0, 0, 256, 0));
    CHECK(dropout_dropped(0, 0, 256, kDropoutOne));
    CHECK(dropout_dropped(0, 0, 256, 0xa4a47e7full) && !dropout_dropped(0, 0, 256, 0xa4a47e7eull));
    CHECK(!dropout_dropped(~0ull, ~0ull, kTokIdMask, 0) && dropout_dropped(~0ull, ~0ull, kTokIdMask, kDropoutOne));
}

void thresholds() {
    unsigned long long t = 99;
    CHECK(dropout_threshold(0.0, &t) && t == 0);
    CHECK(dropout_threshold(-0.0, &t) && t == 0);
    CHECK(dropout_threshold(1.0, &t) && t == kDropoutOne);
    CHECK(dropout_threshold(0.5, &t) && t == (1ull << 31));
    CHECK(dropout_threshold(std::ldexp(1.0, -32), &t) && t == 1);
    CHECK(dropout_threshold(std::ldexp(1.0, -33), &t) && t == 0);                 // floor
    CHECK(dropout_threshold(0.1, &t) && t == 429496729ull);                       // floor(0.1 * 2^32) = 429,496,729.6
    CHECK(dropout_threshold(std::nextafter(1.0, 0.0), &t) && t == kDropoutOne - 1);
    t = 77;
    CHECK(!dropout_threshold(-0.1, &t) && t == 77);
    CHECK(!dropout_threshold(std::nextafter(1.0, 2.0), &t));
    CHECK(!dropout_threshold(2.0, &t));
    CHECK(!dropout_threshold(std::numeric_limits<double>::quiet_NaN(), &t));
    CHECK(!dropout_threshold(std::numeric_limits<double>::infinity(), &t));
    CHECK(!dropout_threshold(-std::numeric_limits<double>::infinity(), &t) && t == 77);
}

}  // namespace

int main() {
    known_answers();
    thresholds();

    const uint32_t A = 'a', B = 'b', C = 'c';
    const Lookup lut = {{{A, A}, 256}, {{A, B}, 257}, {{256, 256}, 258}, {{257, C}, 259},
                        {{256, A}, 260}, {{B, B}, 261}, {{261, 261}, 262}};
    // a a a with (a,a): the instance at 0 dropped and the one at 1 not -> a m (the walk runs over the survivors)
    int witnesses = 0;
    for (unsigned long long seed = 0; seed < 64; ++seed) {
        const unsigned long long half = 1ull << 31;
        if (!dropout_dropped(seed, 0, 256, half) || dropout_dropped(seed, 1, 256, half)) continue;
        ++witnesses;
        const Result r = loop_walk("aaa", lut, 0, seed, half);
        CHECK((r.tok == std::vector<uint32_t>{A, 256}) && (r.pos == std::vector<unsigned long long>{0, 1}));
        CHECK(loop_list("aaa", lut, 0, seed, half) == r);
    }
    CHECK(witnesses > 0);

    unsigned long long state = 0x2545F4914F6CDD1Dull;
    auto rnd = [&](uint32_t m) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)((state >> 33) % m);
    };
    const unsigned long long thresholds_[] = {0, 1ull << 30, 1ull << 31, 3ull << 30, kDropoutOne};
    const unsigned long long seeds[] = {0, 1, 12345};
    const unsigned long long bases[] = {0, 1000, 1ull << 40};
    long strings = 0, differing = 0;
    for (int k = 0; k < 400; ++k) {
        std::string s;
        const uint32_t len = rnd(41);
        for (uint32_t i = 0; i < len; ++i) s.push_back("aaabc"[rnd(5)]);
        ++strings;
        const Result plain = loop_walk(s, lut, 0, 0, 0);
        for (unsigned long long th : thresholds_)
            for (unsigned long long seed : seeds) {
                const unsigned long long base = bases[rnd(3)];
                const Result a = loop_walk(s, lut, base, seed, th), b = loop_list(s, lut, base, seed, th);
                CHECK(a == b);
                // the tokens tile the chunk: their starts ascend from the base
                CHECK(a.pos.empty() == s.empty() && (s.empty() || a.pos[0] == base));
                for (size_t i = 0; i + 1 < a.pos.size(); ++i) CHECK(a.pos[i] < a.pos[i + 1]);
                if (th == 0) CHECK(a.tok == plain.tok);
                if (th == kDropoutOne) CHECK(a.tok.size() == s.size());
                if (a.tok != plain.tok) ++differing;
            }
    }
    CHECK(differing > 1000);                  // (dropout does change segmentations: the loops are not compared on nothing)
    if (failures == 0) std::printf("ok: %ld strings, 0 failures\n", strings);
    else std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
