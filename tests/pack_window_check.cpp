// Stand-alone check of the window arithmetic of csrc/pack_host.h, built by the host compiler
// (tests/test_pack_windows_cpu.py).
//   part 1: pack_win_count, pack_win_row, pack_win_rows and pack_win_doc against a brute-force walk that lays the
//           windows of every document out token by token: seq_len 1 .. 9 and 16, every stride below keep, nb + ne 0 .. 2,
//           document lengths 0 .. 4 * keep + 3.  Checked per document: the windows cover tok[0 .. L) without a gap,
//           consecutive ones share exactly `stride` tokens, every window but the last is full, the last one brings a
//           token no earlier one held; per row: the binary search over the prefix sums finds its document
//   part 2: the argument rules of pack_win_check and the 2^40-row limit of pack_win_rows with two-entry offset arrays
#include "pack_host.h"

#include <cstdio>
#include <vector>

using namespace mbpe;

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() {                          // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the windows of one document by walking: start at 0, advance by step until a window reaches the end
static std::vector<std::pair<uint64_t, uint64_t>> brute(uint64_t L, uint32_t keep, uint32_t step) {
    std::vector<std::pair<uint64_t, uint64_t>> w;
    for (uint64_t a = 0;; a += step) {
        const uint64_t b = a + keep < L ? a + keep : L;
        w.push_back({a, b});
        if (b == L) break;
    }
    return w;
}

static int check_doc(uint64_t L, uint32_t keep, uint32_t stride) {
    const uint32_t step = keep - stride;
    const auto want = brute(L, keep, step);
    int bad = 0;
    if (pack_win_count(L, keep, step) != want.size()) {
        printf("L %llu keep %u stride %u: %llu windows, want %zu\n", (unsigned long long)L, keep, stride,
               (unsigned long long)pack_win_count(L, keep, step), want.size());
        return 1;
    }
    uint64_t covered = 0;                        // tokens [0, covered) were held by the windows so far
    for (size_t i = 0; i < want.size(); ++i) {
        const PackWinRow r = pack_win_row(L, i, keep, step);
        const bool last = i + 1 == want.size();
        if (r.a != want[i].first || r.a + r.body != want[i].second || (r.last != 0) != last) ++bad;
        if (!last && r.body != keep) ++bad;
        if (i && r.a + stride != covered) ++bad;             // shares exactly `stride` tokens with the one before
        if (i && r.a + r.body <= covered) ++bad;             // brings a new token
        covered = r.a + r.body;
    }
    if (covered != L) ++bad;
    if (bad) printf("L %llu keep %u stride %u: %d window errors\n", (unsigned long long)L, keep, stride, bad);
    return bad;
}

static int check_lists(int *n_cases) {
    int bad = 0;
    const uint32_t seq_lens[] = {1, 2, 3, 4, 5, 7, 8, 9, 16};
    for (uint32_t seq_len : seq_lens)
        for (uint32_t nbe = 0; nbe < 3 && nbe < seq_len; ++nbe) {
            const uint32_t keep = seq_len - nbe;
            for (uint32_t stride = 0; stride < keep; ++stride) {
                for (uint64_t L = 0; L <= 4ull * keep + 3; ++L) bad += check_doc(L, keep, stride);
                // a list of documents: the prefix sums, the row count and the search per row
                std::vector<uint64_t> off(1, 0);
                const uint64_t n_docs = 1 + rnd() % 40;
                for (uint64_t d = 0; d < n_docs; ++d) off.push_back(off.back() + (rnd() % 3 ? rnd() % (3ull * keep + 2) : 0));
                std::vector<unsigned long long> row_start(1, 0);
                for (uint64_t d = 0; d < n_docs; ++d)
                    row_start.push_back(row_start.back() + brute(off[d + 1] - off[d], keep, keep - stride).size());
                uint64_t n_rows = 77;
                const char *msg = "";
                if (pack_win_rows(off.data(), n_docs, keep, stride, &n_rows, &msg) != MBPE_OK || n_rows != row_start.back()) {
                    printf("seq_len %u nbe %u stride %u: %llu rows, want %llu\n", seq_len, nbe, stride,
                           (unsigned long long)n_rows, row_start.back());
                    ++bad;
                }
                for (uint64_t row = 0; row < row_start.back(); ++row) {
                    const uint64_t d = pack_win_doc(row_start.data(), n_docs, row_start.back(), row);
                    if (d >= n_docs || row_start[d] > row || row >= row_start[d + 1]) {
                        printf("seq_len %u nbe %u stride %u: row %llu found in document %llu\n", seq_len, nbe, stride,
                               (unsigned long long)row, (unsigned long long)d);
                        ++bad;
                        break;
                    }
                }
                ++*n_cases;
            }
        }
    return bad;
}

static int check_rules() {
    int bad = 0;
    const char *msg = "";
    auto expect = [&](int got, int want, const char *what) {
        if (got != want) { printf("%s: %d, want %d\n", what, got, want); ++bad; }
    };
    uint32_t row_doc = 0;
    const mbpe_pack_spec none = {MBPE_PACK_PADDED, 8, 32, 0, MBPE_NO_TOKEN, MBPE_NO_TOKEN, 0, 0};
    const mbpe_pack_spec both = {MBPE_PACK_PADDED, 8, 32, 0, 1, 2, 0, 0};
    mbpe_pack_window w = {0, 0, nullptr, nullptr};
    expect(pack_win_check(none, nullptr, 1, &msg), MBPE_ERR_ARG, "NULL window");
    expect(pack_win_check(none, &w, 1, &msg), MBPE_OK, "stride 0");
    w.stride = 7;
    expect(pack_win_check(none, &w, 1, &msg), MBPE_OK, "stride keep - 1");
    expect(pack_win_check(both, &w, 1, &msg), MBPE_ERR_ARG, "stride above keep with bos and eos");
    w.stride = 8;
    expect(pack_win_check(none, &w, 1, &msg), MBPE_ERR_ARG, "stride keep");
    w.stride = 6;
    expect(pack_win_check(both, &w, 1, &msg), MBPE_ERR_ARG, "stride keep with bos and eos");
    w.stride = 5;
    expect(pack_win_check(both, &w, 1, &msg), MBPE_OK, "stride keep - 1 with bos and eos");
    w.stride = 0xFFFFFFFFu;
    expect(pack_win_check(none, &w, 1, &msg), MBPE_ERR_ARG, "stride 2^32 - 1");
    w.stride = 0;
    w.score_once = 1;
    expect(pack_win_check(none, &w, 1, &msg), MBPE_OK, "score_once 1");
    w.score_once = 2;
    expect(pack_win_check(none, &w, 1, &msg), MBPE_ERR_ARG, "score_once 2");
    w.score_once = 0;
    mbpe_pack_spec s = none;
    s.layout = MBPE_PACK_PACKED;
    expect(pack_win_check(s, &w, 1, &msg), MBPE_ERR_ARG, "PACKED");
    s = none; s.pad_left = 1;
    expect(pack_win_check(s, &w, 1, &msg), MBPE_ERR_ARG, "pad_left");
    s = none; s.trunc_left = 1;
    expect(pack_win_check(s, &w, 1, &msg), MBPE_ERR_ARG, "trunc_left");
    s = both; s.seq_len = 2;
    expect(pack_win_check(s, &w, 1, &msg), MBPE_ERR_ARG, "seq_len nb + ne");
    s.seq_len = 3;
    expect(pack_win_check(s, &w, 1, &msg), MBPE_OK, "seq_len nb + ne + 1");
    s = none; s.seq_len = 0;
    expect(pack_win_check(s, &w, 1, &msg), MBPE_ERR_ARG, "seq_len 0");
    // row_doc holds d in 32 bits: a synthetic document count, no array
    expect(pack_win_check(none, &w, 1ull << 40, &msg), MBPE_OK, "2^40 documents without row_doc");
    w.row_doc = &row_doc;
    expect(pack_win_check(none, &w, 0xFFFFFFFEull, &msg), MBPE_OK, "row_doc with 2^32 - 2 documents");
    expect(pack_win_check(none, &w, 0xFFFFFFFFull, &msg), MBPE_ERR_ARG, "row_doc with 2^32 - 1 documents");
    // the row limit: one document of L tokens at keep 1, step 1 has L rows
    uint64_t n_rows = 77;
    const uint64_t edge[2] = {0, 1ull << 40}, over[2] = {0, (1ull << 40) + 1}, huge[2] = {0, ~0ull};
    expect(pack_win_rows(edge, 1, 1, 0, &n_rows, &msg), MBPE_OK, "2^40 rows");
    if (n_rows != (1ull << 40)) { printf("2^40 rows: %llu\n", (unsigned long long)n_rows); ++bad; }
    n_rows = 77;
    expect(pack_win_rows(over, 1, 1, 0, &n_rows, &msg), MBPE_ERR_ARG, "2^40 + 1 rows");
    expect(pack_win_rows(huge, 1, 1, 0, &n_rows, &msg), MBPE_ERR_ARG, "2^64 - 1 rows");
    if (n_rows != 77) { printf("a refused count was written\n"); ++bad; }
    // wide rows: the sums stay in 64 bits
    const uint64_t wide[2] = {0, ~0ull};
    expect(pack_win_rows(wide, 1, 0xFFFFFFFFu, 0, &n_rows, &msg), MBPE_OK, "2^64 - 1 tokens in rows of 2^32 - 1");
    if (n_rows != 0x100000001ull) { printf("wide rows: %llu\n", (unsigned long long)n_rows); ++bad; }
    return bad;
}

int main() {
    int n_cases = 0;
    const int bad = check_lists(&n_cases) + check_rules();
    printf("ok: %d lists, %d failures\n", n_cases, bad);
    return bad ? 1 : 0;
}
