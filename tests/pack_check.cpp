// Stand-alone check of the host arithmetic of csrc/pack_host.h, built by the host compiler (tests/test_pack_aux_cpu.py).
//   part 1: pack_cu_seqlens against a brute-force scan over the cells of the PACKED matrix: every cell gets its
//           (row, seg) by walking the documents, and a boundary is where that pair changes.  Cases: seq_len 1 .. 9
//           and 16, document lengths 0 .. 3 * seq_len + 1, all four bos / eos settings; the query, a cap too small
//           and an exact cap
//   part 2: the limits -- ignore_label for 16 and 32 bits, n_docs for seg with a synthetic count (no array), T_d for
//           pos and n_stream for cu_seqlens with two-entry offset arrays
#include "pack_host.h"

#include <cstdio>
#include <vector>

using namespace mbpe;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {                          // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the boundaries of the runs of equal (row, seg) over the n_stream cells, cell by cell, and the longest run
static std::vector<int32_t> brute(const std::vector<uint64_t> &off, uint32_t seq_len, uint32_t nbe, uint32_t *longest) {
    std::vector<uint64_t> seg;                   // per stream cell: d + 1
    for (uint64_t d = 0; d + 1 < off.size(); ++d)
        for (uint64_t k = 0; k < off[d + 1] - off[d] + nbe; ++k) seg.push_back(d + 1);
    std::vector<int32_t> cu;
    for (uint64_t f = 0; f < seg.size(); ++f)
        if (f == 0 || seg[f] != seg[f - 1] || f / seq_len != (f - 1) / seq_len) cu.push_back((int32_t)f);
    cu.push_back((int32_t)seg.size());
    if (seg.empty()) cu.assign(1, 0);
    *longest = 0;
    for (size_t i = 1; i < cu.size(); ++i)
        if ((uint32_t)(cu[i] - cu[i - 1]) > *longest) *longest = (uint32_t)(cu[i] - cu[i - 1]);
    return cu;
}

static int check_case(const std::vector<uint64_t> &off, uint32_t seq_len, uint32_t nbe, const char *what) {
    const uint64_t n_docs = off.size() - 1;
    uint32_t want_longest = 0, longest = 77;
    const std::vector<int32_t> want = brute(off, seq_len, nbe, &want_longest);
    const char *msg = "";
    uint64_t n_seqs = 77;
    int bad = 0;
    if (pack_cu_seqlens(off.data(), n_docs, seq_len, nbe, nullptr, 0, &n_seqs, &longest, &msg) != MBPE_OK ||
        n_seqs != want.size() - 1 || longest != want_longest) {
        printf("%s seq_len %u nbe %u: query gives %llu sequences, longest %u; want %zu, %u\n", what, seq_len, nbe,
               (unsigned long long)n_seqs, longest, want.size() - 1, want_longest);
        ++bad;
    }
    std::vector<int32_t> got(want.size() + 1, -7);                  // one guard entry behind
    if (pack_cu_seqlens(off.data(), n_docs, seq_len, nbe, got.data(), want.size() - 1, &n_seqs, &longest, &msg) != MBPE_OK ||
        n_seqs != want.size() - 1 || longest != want_longest || got.back() != -7) {
        printf("%s seq_len %u nbe %u: the exact cap fails\n", what, seq_len, nbe);
        ++bad;
    }
    got.pop_back();
    if (got != want) {
        printf("%s seq_len %u nbe %u: the list differs\n", what, seq_len, nbe);
        ++bad;
    }
    if (longest > seq_len) { printf("%s: max_seqlen %u above seq_len %u\n", what, longest, seq_len); ++bad; }
    if (want.size() > 1) {                                          // a cap too small: the counts, nothing written
        std::vector<int32_t> none(want.size(), -7);
        n_seqs = 77;
        if (pack_cu_seqlens(off.data(), n_docs, seq_len, nbe, none.data(), want.size() - 2, &n_seqs, &longest, &msg) !=
                MBPE_ERR_ARG || n_seqs != want.size() - 1 || none != std::vector<int32_t>(want.size(), -7)) {
            printf("%s seq_len %u nbe %u: a cap too small is not refused cleanly\n", what, seq_len, nbe);
            ++bad;
        }
    }
    return bad;
}

static int check_lists(int *n_cases) {
    int bad = 0;
    const uint32_t seq_lens[] = {1, 2, 3, 4, 5, 7, 8, 9, 16};
    for (uint32_t seq_len : seq_lens)
        for (uint32_t nbe = 0; nbe < 3; ++nbe) {
            // by hand: no document, empty ones only, one token, an end exactly at a row end, three rows spanned
            const std::vector<std::vector<uint64_t>> fixed = {
                {0}, {0, 0, 0, 0}, {0, 1}, {0, seq_len, 2ull * seq_len}, {0, 0, 3ull * seq_len + 1, 3ull * seq_len + 1},
                {0, seq_len - (seq_len > nbe ? nbe : 0), seq_len + 1ull}};
            for (const auto &off : fixed) { bad += check_case(off, seq_len, nbe, "fixed"); ++*n_cases; }
            for (int i = 0; i < 8; ++i) {
                std::vector<uint64_t> off(1, 0);
                const uint64_t n_docs = rnd() % 12;
                for (uint64_t d = 0; d < n_docs; ++d) {
                    const uint64_t pick = rnd() % 4;
                    const uint64_t len = pick == 0 ? 0 : pick == 1 ? (rnd() % 3) * seq_len : rnd() % (3ull * seq_len + 2);
                    off.push_back(off.back() + len);
                }
                bad += check_case(off, seq_len, nbe, "random");
                ++*n_cases;
            }
        }
    return bad;
}

static int check_limits() {
    int bad = 0;
    const char *msg = "";
    auto expect = [&](int got, int want, const char *what) {
        if (got != want) { printf("%s: %d, want %d\n", what, got, want); ++bad; }
    };
    expect(pack_check_ignore(16, 0, &msg), MBPE_OK, "ignore 0 at 16 bits");
    expect(pack_check_ignore(16, 65535, &msg), MBPE_OK, "ignore 65535 at 16 bits");
    expect(pack_check_ignore(16, 65536, &msg), MBPE_ERR_VOCAB, "ignore 65536 at 16 bits");
    expect(pack_check_ignore(16, -100, &msg), MBPE_ERR_VOCAB, "ignore -100 at 16 bits");
    expect(pack_check_ignore(32, -100, &msg), MBPE_OK, "ignore -100 at 32 bits");
    expect(pack_check_ignore(32, -2147483648ll, &msg), MBPE_OK, "ignore -2^31 at 32 bits");
    expect(pack_check_ignore(32, -2147483649ll, &msg), MBPE_ERR_ARG, "ignore -2^31 - 1 at 32 bits");
    expect(pack_check_ignore(32, 4294967295ll, &msg), MBPE_OK, "ignore 2^32 - 1 at 32 bits");
    expect(pack_check_ignore(32, 4294967296ll, &msg), MBPE_ERR_ARG, "ignore 2^32 at 32 bits");
    expect(pack_check_ignore(64, INT64_MIN, &msg), MBPE_OK, "ignore INT64_MIN at 64 bits");
    expect(pack_check_ignore(64, INT64_MAX, &msg), MBPE_OK, "ignore INT64_MAX at 64 bits");
    // seg: a synthetic document count, no array
    expect(pack_check_seg_docs(0, &msg), MBPE_OK, "seg with no document");
    expect(pack_check_seg_docs(0xFFFFFFFEull, &msg), MBPE_OK, "seg with 2^32 - 2 documents");
    expect(pack_check_seg_docs(0xFFFFFFFFull, &msg), MBPE_ERR_ARG, "seg with 2^32 - 1 documents");
    expect(pack_check_seg_docs(1ull << 40, &msg), MBPE_ERR_ARG, "seg with 2^40 documents");
    // pos: T_d = tokens + nbe must stay below 2^32
    const uint64_t big[3] = {0, 5, 5 + 0xFFFFFFFEull};
    expect(pack_check_pos_docs(big, 2, 0, &msg), MBPE_OK, "pos with 2^32 - 2 elements");
    expect(pack_check_pos_docs(big, 2, 1, &msg), MBPE_OK, "pos with 2^32 - 1 elements");
    expect(pack_check_pos_docs(big, 2, 2, &msg), MBPE_ERR_ARG, "pos with 2^32 elements");
    // cu_seqlens: n_stream must stay below 2^31
    uint64_t n_seqs = 0;
    uint32_t longest = 0;
    const uint64_t edge[2] = {0, (1ull << 31) - 2};
    expect(pack_cu_seqlens(edge, 1, 1u << 30, 1, nullptr, 0, &n_seqs, &longest, &msg), MBPE_OK, "n_stream 2^31 - 1");
    if (n_seqs != 2 || longest != (1u << 30)) { printf("n_stream 2^31 - 1: %llu sequences, longest %u\n", (unsigned long long)n_seqs, longest); ++bad; }
    expect(pack_cu_seqlens(edge, 1, 1u << 30, 2, nullptr, 0, &n_seqs, &longest, &msg), MBPE_ERR_ARG, "n_stream 2^31");
    const uint64_t huge[2] = {0, ~0ull - 1};
    expect(pack_cu_seqlens(huge, 1, 8, 2, nullptr, 0, &n_seqs, &longest, &msg), MBPE_ERR_ARG, "n_stream that wraps");
    return bad;
}

int main() {
    int n_cases = 0;
    const int bad = check_lists(&n_cases) + check_limits();
    printf("ok: %d lists, %d failures\n", n_cases, bad);
    return bad ? 1 : 0;
}
