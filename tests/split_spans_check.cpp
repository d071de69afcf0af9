// Stand-alone check of Splitter::split_spans (host/presplit.cpp), the PCRE2 side of the device split, built by the host
// compiler together with presplit.cpp and errors.cpp (tests/test_split_spans_cpu.py):
//   - a stretch whose matches do not tile it returns MBPE_ERR_SPLIT_GAP and leaves the output empty,
//   - stretches that cover a text, matched each on its own subject [a, min(b + 1, n)) from a copy that starts at
//     `origin`, give the chunk ends of the whole-text split, with one thread and with several.
#include "mbpe.h"
#include "mbpe_host.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using mbpe_host::Splitter;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    std::string err;
    {   // a pattern that leaves the space in no match
        Splitter sp;
        CHECK(sp.compile("[a-z]+", &err) == MBPE_OK);
        const std::string t = "ab cd";
        const uint64_t whole[2] = {0, t.size()};
        std::vector<uint64_t> last = {7, 7, 7};
        CHECK(sp.split_spans((const uint8_t *)t.data(), 0, t.size(), whole, 1, 1, &last, &err) == MBPE_ERR_SPLIT_GAP);
        CHECK(last.empty());
        CHECK(err.find("unmatched") != std::string::npos);
        // ... and a stretch it does tile
        const uint64_t word[2] = {3, 5};
        CHECK(sp.split_spans((const uint8_t *)t.data(), 0, t.size(), word, 1, 1, &last, &err) == MBPE_OK);
        CHECK(last == std::vector<uint64_t>{4});
    }
    for (const char *enc : {"gpt2", "gpt4"}) {
        Splitter sp;
        CHECK(sp.compile(mbpe_host::split_pattern_for(enc), &err) == MBPE_OK);
        const std::string t = "It's caf\xc3\xa9 time  \n\n12345 na\xc3\xafve words\t here, d\xc3\xa9j\xc3\xa0 vu 'll  ";
        const uint8_t *p = (const uint8_t *)t.data();
        std::vector<uint64_t> starts, ends, want, last;
        CHECK(sp.split(p, t.size(), &starts, &ends, &err) == MBPE_OK);
        for (uint64_t e : ends) want.push_back(e - 1);
        // the stretches between the places where a letter or digit is followed by whitespace, from the fourth byte on
        auto ln = [](uint8_t c) { return (c | 0x20) - 'a' < 26u || c - '0' < 10u; };
        auto ws = [](uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); };
        std::vector<uint64_t> spans;
        uint64_t a = 4;                                  // "It's" ends there, before " caf"
        for (uint64_t i = a + 1; i <= t.size(); ++i)
            if (i == t.size() || (ln(p[i - 1]) && ws(p[i]))) { spans.push_back(a); spans.push_back(i); a = i; }
        std::vector<uint64_t> tail;
        for (uint64_t e : want) if (e >= 4) tail.push_back(e);
        for (unsigned threads : {1u, 3u}) {
            CHECK(sp.split_spans(p + 4, 4, t.size(), spans.data(), spans.size() / 2, threads, &last, &err) == MBPE_OK);
            CHECK(last == tail);
        }
    }
    printf("%s: %d failures\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
