// Stand-alone emulation of the device split of many documents around names (csrc/split_rule.h, csrc/split.hip:
// mbpe_splitter_split_docs), built by the host compiler (tests/test_split_docs_cpu.py): the find pass and the sync
// pass one 16-byte vector per iteration, the walk one 64-byte block per iteration, as the device threads take them,
// and between them the host's plan (split_plan_parts, split_plan_finish) -- the very functions split.hip calls.  The
// text lives in a buffer of exactly its size, and so do its bitmaps, so that a sanitized build sees any read beyond
// them.
//
//   split_docs_check <gpt2|gpt4> <max_span> <in> <out>
//   in:  u64 n_docs, n_docs + 1 u64 document offsets, u64 n_names, n_names + 1 u64 name offsets, the names' bytes,
//        the text's bytes
//   out: u64 n_ends, u64 n_host, u64 n_ranges, n_ends u64 positions of the last byte of every chunk of a clean span
//        and of every range, n_host triples (a, b, b is a cut) of u64: the host spans, n_ranges triples (start, len,
//        name) of u64
#include "split_rule.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace mbpe;

struct Collect {
    std::vector<uint64_t> *ends;
    uint64_t n, last;
    int bad;
    void operator()(uint64_t p) {
        if (p >= n || (last != ~0ull && p <= last)) ++bad;      // inside the text and ascending within a thread
        last = p;
        ends->push_back(p);
    }
};

struct Hits {
    std::vector<uint64_t> *list;
    void operator()(uint64_t p, uint32_t name) { list->push_back((p << kSplitNameBits) | name); }
};

static void read_words(const uint8_t *t, uint64_t n, uint64_t at, uint32_t w[4]) {
    const uint64_t valid = n - at < (uint64_t)kSplitVec ? n - at : (uint64_t)kSplitVec;
    w[0] = w[1] = w[2] = w[3] = 0;
    memcpy(w, t + at, valid);                                   // (little-endian host, as the device)
}

static bool get_bit(const std::vector<unsigned long long> &bm, uint64_t p) { return (bm[p >> 6] >> (p & 63)) & 1ull; }

int main(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "usage: split_docs_check <gpt2|gpt4> <max_span> <in> <out>\n"); return 2; }
    const int pattern = std::string(argv[1]) == "gpt4" ? kSplitGpt4 : kSplitGpt2;
    const uint64_t max_span = strtoull(argv[2], nullptr, 10);
    FILE *f = fopen(argv[3], "rb");
    if (!f) { perror(argv[3]); return 2; }
    uint64_t n_docs = 0, n_names = 0;
    if (fread(&n_docs, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> doc_off(n_docs + 1);
    if (fread(doc_off.data(), 8, doc_off.size(), f) != doc_off.size()) return 2;
    if (fread(&n_names, 8, 1, f) != 1 || n_names > kSplitMaxNames) return 2;
    std::vector<uint64_t> name_off64(n_names + 1);
    if (fread(name_off64.data(), 8, name_off64.size(), f) != name_off64.size()) return 2;
    std::vector<uint32_t> name_off(name_off64.begin(), name_off64.end());
    const std::vector<uint8_t> name_bytes_in = [&] {
        std::vector<uint8_t> b(name_off[n_names]);
        if (!b.empty() && fread(b.data(), 1, b.size(), f) != b.size()) exit(2);
        return b;
    }();
    const uint64_t n = doc_off[n_docs];
    std::vector<uint8_t> text_in(n);
    if (n && fread(text_in.data(), 1, n, f) != n) return 2;
    fclose(f);
    const std::vector<uint8_t> text(text_in);                   // exactly n bytes
    const uint8_t *t = text.data();

    std::vector<uint64_t> ends, host;
    std::vector<SplitRange> ranges;
    int bad = 0;
    if (n) {
        const uint64_t n_vec = (n + kSplitVec - 1) / kSplitVec, n_words = (n + kSplitBlock - 1) / kSplitBlock;
        // k_split_find: one lane per iteration
        std::vector<uint64_t> hits;
        uint32_t first_set[8];
        split_first_set(name_bytes_in.data(), name_off.data(), (uint32_t)n_names, first_set);
        const SplitNames nm = {name_bytes_in.data(), name_off.data(), first_set, (uint32_t)n_names};
        Hits hit{&hits};
        for (uint64_t v = 0; v < n_vec && n_names; ++v) {
            uint32_t w[4];
            read_words(t, n, v * kSplitVec, w);
            split_find_vec(t, n, v * kSplitVec, w[0] | ((uint64_t)w[1] << 32), w[2] | ((uint64_t)w[3] << 32), nm, hit);
        }
        std::sort(hits.begin(), hits.end());
        // the host's plan
        std::vector<SplitRange> taken, parts;
        std::vector<uint64_t> cuts;
        split_plan_parts(hits.data(), hits.size(), doc_off.data(), n_docs, name_off.data(), &taken, &parts);
        std::vector<uint8_t> first(parts.size());
        for (size_t k = 0; k < parts.size(); ++k) first[k] = t[parts[k].start];
        split_plan_finish(taken, parts, first.data(), &ranges, &cuts);
        // the cut bitmap and the bitmap of the bytes inside ranges
        std::vector<unsigned long long> cut(n_words, 0), raw(n_words, 0), bnd(n_words, 0), hi(n_words, 0);
        for (uint64_t p : cuts) {
            if (p == 0 || p >= n) ++bad;
            else cut[p >> 6] |= 1ull << (p & 63);
        }
        for (const SplitRange &r : ranges) {
            if (r.len == 0 || r.start >= n || r.len > n - r.start) { ++bad; continue; }
            for (uint64_t p = r.start; p < r.start + r.len; ++p) raw[p >> 6] |= 1ull << (p & 63);
            ends.push_back(r.start + r.len - 1);                // (the host adds a range's one end bit)
        }
        for (uint64_t v = 0; v < n_vec; ++v) {                  // k_split_sync: one lane
            const uint64_t at = v * kSplitVec;
            uint32_t w[4], s = 0, h = 0;
            read_words(t, n, at, w);
            split_vec_bits(w, at ? t[at - 1] : ' ', &s, &h);
            bnd[at >> 6] |= ((unsigned long long)s << (at & 63)) | (cut[at >> 6] & (0xFFFFull << (at & 63)));
            hi[at >> 6] |= (unsigned long long)h << (at & 63);
        }
        const bool have_cuts = !cuts.empty(), have_raw = !ranges.empty();
        for (uint64_t T = 0; T < n_words; ++T) {                // k_split_walk: one thread
            Collect c{&ends, n, ~0ull, 0};
            unsigned long long hm = split_walk_block(t, n, bnd.data(), hi.data(), have_cuts ? cut.data() : nullptr,
                                                     have_raw ? raw.data() : nullptr, T, max_span, pattern, c);
            bad += c.bad;
            while (hm) {                                        // k_split_compact: one thread
                const uint64_t a = (T << 6) + (uint64_t)__builtin_ctzll(hm);
                hm &= hm - 1;
                const uint64_t b = split_next_bit(bnd.data(), a + 1, n);
                host.push_back(a);
                host.push_back(b);
                host.push_back(b < n && get_bit(cut, b) ? 1 : 0);
            }
        }
    }

    f = fopen(argv[4], "wb");
    if (!f) { perror(argv[4]); return 2; }
    const uint64_t head[3] = {ends.size(), host.size() / 3, ranges.size()};
    fwrite(head, 8, 3, f);
    if (!ends.empty()) fwrite(ends.data(), 8, ends.size(), f);
    if (!host.empty()) fwrite(host.data(), 8, host.size(), f);
    for (const SplitRange &r : ranges) {
        const uint64_t row[3] = {r.start, r.len, r.name};
        fwrite(row, 8, 3, f);
    }
    fclose(f);
    printf("%s: %llu documents, %llu ends, %llu host spans, %llu ranges, %d ends or cuts out of order or out of the text\n",
           bad ? "FAILED" : "ok", (unsigned long long)n_docs, (unsigned long long)head[0], (unsigned long long)head[1],
           (unsigned long long)head[2], bad);
    return bad ? 1 : 0;
}
