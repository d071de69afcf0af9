// Stand-alone emulation of the device split (csrc/split_rule.h, csrc/split.hip), built by the host compiler
// (tests/test_split_cpu.py): the sync pass one 16-byte vector per iteration, the walk one 64-byte block per iteration,
// as the device threads take them.  Every text lives in a buffer of exactly its size, and so do its bitmaps, so that
// a sanitized build sees any read beyond them.
//
//   split_check <gpt2|gpt4> <max_span> <in> <out>
//   in:  u64 n_texts, n_texts + 1 u64 offsets, the texts' bytes one after the other
//   out: u64 n_ends, u64 n_host, n_ends u64 positions (in the concatenation) of the last byte of every chunk of a
//        clean span, n_host pairs (a, b) of u64: the host spans
#include "split_rule.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace mbpe;

struct Collect {
    std::vector<uint64_t> *ends;
    uint64_t base, n, last;
    int bad;
    void operator()(uint64_t p) {
        if (p >= n || (last != ~0ull && p <= last)) ++bad;      // inside the text and ascending within a thread
        last = p;
        ends->push_back(base + p);
    }
};

static int split_text(const uint8_t *src, uint64_t n, uint64_t base, uint64_t max_span, int pattern,
                      std::vector<uint64_t> *ends, std::vector<uint64_t> *host) {
    if (n == 0) return 0;
    const std::vector<uint8_t> text(src, src + n);
    const uint8_t *t = text.data();
    const uint64_t n_vec = (n + kSplitVec - 1) / kSplitVec, n_words = (n + kSplitBlock - 1) / kSplitBlock;
    std::vector<unsigned long long> sync(n_words, 0), hi(n_words, 0);
    for (uint64_t v = 0; v < n_vec; ++v) {                      // k_split_sync: one lane
        const uint64_t at = v * kSplitVec;
        const uint64_t valid = n - at < (uint64_t)kSplitVec ? n - at : (uint64_t)kSplitVec;
        uint32_t w[4] = {0, 0, 0, 0}, s = 0, h = 0;
        memcpy(w, t + at, valid);                               // (little-endian host, as the device)
        split_vec_bits(w, at ? t[at - 1] : ' ', &s, &h);
        sync[at >> 6] |= (unsigned long long)s << (at & 63);
        hi[at >> 6] |= (unsigned long long)h << (at & 63);
    }
    int bad = 0;
    for (uint64_t T = 0; T < n_words; ++T) {                    // k_split_walk: one thread
        Collect c{ends, base, n, ~0ull, 0};
        unsigned long long hm = split_walk_block(t, n, sync.data(), hi.data(), T, max_span, pattern, c);
        bad += c.bad;
        while (hm) {                                            // k_split_compact: one thread
            const uint64_t a = (T << 6) + (uint64_t)__builtin_ctzll(hm);
            hm &= hm - 1;
            host->push_back(base + a);
            host->push_back(base + split_next_bit(sync.data(), a + 1, n));
        }
    }
    return bad;
}

int main(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "usage: split_check <gpt2|gpt4> <max_span> <in> <out>\n"); return 2; }
    const int pattern = std::string(argv[1]) == "gpt4" ? kSplitGpt4 : kSplitGpt2;
    const uint64_t max_span = strtoull(argv[2], nullptr, 10);
    FILE *f = fopen(argv[3], "rb");
    if (!f) { perror(argv[3]); return 2; }
    uint64_t n_texts = 0;
    if (fread(&n_texts, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> off(n_texts + 1);
    if (fread(off.data(), 8, off.size(), f) != off.size()) return 2;
    std::vector<uint8_t> blob(off[n_texts]);
    if (!blob.empty() && fread(blob.data(), 1, blob.size(), f) != blob.size()) return 2;
    fclose(f);

    std::vector<uint64_t> ends, host;
    int bad = 0;
    for (uint64_t k = 0; k < n_texts; ++k)
        bad += split_text(blob.data() + off[k], off[k + 1] - off[k], off[k], max_span, pattern, &ends, &host);

    f = fopen(argv[4], "wb");
    if (!f) { perror(argv[4]); return 2; }
    const uint64_t head[2] = {ends.size(), host.size() / 2};
    fwrite(head, 8, 2, f);
    if (!ends.empty()) fwrite(ends.data(), 8, ends.size(), f);
    if (!host.empty()) fwrite(host.data(), 8, host.size(), f);
    fclose(f);
    printf("%s: %llu texts, %llu ends, %llu host spans, %d ends out of order or out of the text\n", bad ? "FAILED" : "ok",
           (unsigned long long)n_texts, (unsigned long long)head[0], (unsigned long long)head[1], bad);
    return bad ? 1 : 0;
}
