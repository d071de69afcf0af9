// Stand-alone emulation of the device split in "unicode" mode (csrc/split_rule.h, csrc/split.hip), built by the host
// compiler (tests/test_split_unicode_cpu.py): the sync pass one 16-byte vector per iteration, the walk one 64-byte
// block per iteration, as the device threads take them.  Every text lives in a buffer of exactly its size, and so do
// its bitmaps, so that a sanitized build sees any read beyond them.
//
//   split_unicode_check <gpt2|gpt4> <max_span> <table> <in> <out>
//   table: 0x110000 / 16 u32 (2 bits per code point), u32 n_fold, 8 u32 code points, 8 u8 letters
//          (mbpe_split_unicode_table, written by the test)
//   in:    u64 n_texts, n_texts + 1 u64 offsets, u64 n_cuts, n_cuts u64 cut positions (in the concatenation, ascending,
//          each inside a text and not at its start), the texts' bytes one after the other
//   out:   u64 n_ends, u64 n_host, n_ends u64 positions (in the concatenation) of the last byte of every chunk of a
//          walked span, n_host pairs (a, b) of u64: the host spans
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

static int split_text(const uint8_t *src, uint64_t n, uint64_t base, const std::vector<uint64_t> &cuts, uint64_t max_span,
                      const SplitCharStep &step, std::vector<uint64_t> *ends, std::vector<uint64_t> *host) {
    if (n == 0) return 0;
    const std::vector<uint8_t> text(src, src + n);
    const uint8_t *t = text.data();
    const uint64_t n_vec = (n + kSplitVec - 1) / kSplitVec, n_words = (n + kSplitBlock - 1) / kSplitBlock;
    std::vector<unsigned long long> cut(n_words, 0), bnd(n_words, 0), bad(n_words, 0);
    for (uint64_t c : cuts) cut[c >> 6] |= 1ull << (c & 63);    // k_split_patch
    for (uint64_t v = 0; v < n_vec; ++v) {                      // k_split_sync_u: one lane
        const uint64_t at = v * kSplitVec;
        const uint64_t valid = n - at < (uint64_t)kSplitVec ? n - at : (uint64_t)kSplitVec;
        uint32_t w[4] = {0, 0, 0, 0}, s = 0, h = 0;
        memcpy(w, t + at, valid);                               // (little-endian host, as the device)
        split_vec_bits_u(t, n, at, w, step.pattern, step.tab, &s, &h);
        if ((s | h) >> valid) return 1;                         // bits at or beyond the end of the text
        bnd[at >> 6] |= (unsigned long long)s << (at & 63);
        bad[at >> 6] |= (unsigned long long)h << (at & 63);
    }
    for (uint64_t w = 0; w < n_words; ++w) bnd[w] |= cut[w];
    int wrong = 0;
    for (uint64_t T = 0; T < n_words; ++T) {                    // k_split_walk_u: one thread
        Collect c{ends, base, n, ~0ull, 0};
        unsigned long long hm = split_walk_block_with(t, n, bnd.data(), bad.data(), cuts.empty() ? nullptr : cut.data(),
                                                      nullptr, T, max_span, step, c);
        wrong += c.bad;
        while (hm) {                                            // k_split_compact: one thread
            const uint64_t a = (T << 6) + (uint64_t)__builtin_ctzll(hm);
            hm &= hm - 1;
            host->push_back(base + a);
            host->push_back(base + split_next_bit(bnd.data(), a + 1, n));
        }
    }
    return wrong;
}

static bool read_all(FILE *f, void *p, size_t size, size_t count) { return count == 0 || fread(p, size, count, f) == count; }

int main(int argc, char **argv) {
    if (argc != 6) { fprintf(stderr, "usage: split_unicode_check <gpt2|gpt4> <max_span> <table> <in> <out>\n"); return 2; }
    const int pattern = std::string(argv[1]) == "gpt4" ? kSplitGpt4 : kSplitGpt2;
    const uint64_t max_span = strtoull(argv[2], nullptr, 10);

    FILE *f = fopen(argv[3], "rb");
    if (!f) { perror(argv[3]); return 2; }
    std::vector<uint32_t> tab(kSplitTableWords);
    SplitFold fold = {};
    if (!read_all(f, tab.data(), 4, tab.size()) || !read_all(f, &fold.n, 4, 1) || !read_all(f, fold.cp, 4, kSplitMaxFold) ||
        !read_all(f, fold.to, 1, kSplitMaxFold) || fold.n > kSplitMaxFold)
        return 2;
    fclose(f);
    for (uint32_t c = 0; c < 0x80u; ++c)                        // the table and the byte rule agree below 0x80
        if (((tab[c >> 4] >> (2u * (c & 15u))) & 3u) != split_class(c)) { printf("FAILED: the table's class of %u\n", c); return 1; }

    f = fopen(argv[4], "rb");
    if (!f) { perror(argv[4]); return 2; }
    uint64_t n_texts = 0, n_cuts = 0;
    if (!read_all(f, &n_texts, 8, 1)) return 2;
    std::vector<uint64_t> off(n_texts + 1);
    if (!read_all(f, off.data(), 8, off.size()) || !read_all(f, &n_cuts, 8, 1)) return 2;
    std::vector<uint64_t> cuts(n_cuts);
    if (!read_all(f, cuts.data(), 8, n_cuts)) return 2;
    std::vector<uint8_t> blob(off[n_texts]);
    if (!read_all(f, blob.data(), 1, blob.size())) return 2;
    fclose(f);

    const SplitCharStep step = {pattern, tab.data(), fold};
    std::vector<uint64_t> ends, host, own;
    int bad = 0;
    size_t c = 0;
    for (uint64_t k = 0; k < n_texts; ++k) {
        own.clear();
        for (; c < cuts.size() && cuts[c] < off[k + 1]; ++c)
            if (cuts[c] > off[k]) own.push_back(cuts[c] - off[k]);
        bad += split_text(blob.data() + off[k], off[k + 1] - off[k], off[k], own, max_span, step, &ends, &host);
    }

    f = fopen(argv[5], "wb");
    if (!f) { perror(argv[5]); return 2; }
    const uint64_t head[2] = {ends.size(), host.size() / 2};
    fwrite(head, 8, 2, f);
    if (!ends.empty()) fwrite(ends.data(), 8, ends.size(), f);
    if (!host.empty()) fwrite(host.data(), 8, host.size(), f);
    fclose(f);
    printf("%s: %llu texts, %llu ends, %llu host spans, %d ends out of order or out of the text\n", bad ? "FAILED" : "ok",
           (unsigned long long)n_texts, (unsigned long long)head[0], (unsigned long long)head[1], bad);
    return bad ? 1 : 0;
}
