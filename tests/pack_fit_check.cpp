// Stand-alone check of the best-fit planner of csrc/pack_fit.h, built by the host compiler (tests/test_pack_fit_cpu.py).
//   part 1: pack_fit_plan against a brute-force placement that scans every open row per piece: seq_len 1 .. 9, 16 and
//           64, nb + ne 0 .. 2, lists of up to 60 documents with lengths on the edges of the rule.  Checked per list:
//           the row count, every piece's row and column, the table's order, row_first, len, doc_row and doc_col, and
//           the consequences the rule promises (full pieces first in document order, sizes not increasing within a row,
//           no gap, at most one row filled to half or less); pack_fit_cu_seqlens against the runs of the table
//   part 2: the 2^40-row limit and the arithmetic near 2^64 with two-entry offset arrays
#include "pack_fit.h"

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

struct Placed {
    uint64_t row, d, k0;
    uint32_t col0, size;
};

// the rule, piece by piece: sizes from seq_len down, documents ascending within a size; every open row is looked at
static std::vector<Placed> brute(const std::vector<uint64_t> &off, uint32_t S, uint32_t nbe, std::vector<uint32_t> *free) {
    std::vector<Placed> out;
    const uint64_t n_docs = off.size() - 1;
    for (uint32_t size = S; size >= 1; --size)
        for (uint64_t d = 0; d < n_docs; ++d) {
            const uint64_t T = off[d + 1] - off[d] + nbe;
            const uint64_t q = T / S, r = T % S;
            const uint64_t n_of_size = size == S ? q : (r == size ? 1 : 0);
            for (uint64_t i = 0; i < n_of_size; ++i) {
                const uint64_t k0 = size == S ? i * S : q * S;
                uint64_t best = free->size();
                for (uint64_t row = 0; row < free->size(); ++row)
                    if ((*free)[row] >= size && (best == free->size() || (*free)[row] < (*free)[best])) best = row;
                if (best == free->size()) free->push_back(S);
                out.push_back({best, d, k0, S - (*free)[best], size});
                (*free)[best] -= size;
            }
        }
    return out;
}

static int check_list(const std::vector<uint64_t> &off, uint32_t S, uint32_t nbe, PackFitPlan *plan) {
    const uint64_t n_docs = off.size() - 1;
    const char *msg = "";
    if (pack_fit_plan(off.data(), n_docs, S, nbe, plan, &msg) != MBPE_OK) {
        printf("seq_len %u nbe %u: plan refused: %s\n", S, nbe, msg);
        return 1;
    }
    std::vector<uint32_t> free;
    const std::vector<Placed> want = brute(off, S, nbe, &free);
    int bad = 0;
    if (plan->n_rows != free.size() || plan->pieces.size() != want.size() || plan->row_first.size() != free.size() + 1 ||
        plan->len.size() != free.size() || plan->doc_row.size() != n_docs || plan->doc_col.size() != n_docs) {
        printf("seq_len %u nbe %u: %llu rows and %zu pieces, want %zu and %zu\n", S, nbe, (unsigned long long)plan->n_rows,
               plan->pieces.size(), free.size(), want.size());
        return 1;
    }
    // every piece of the brute-force placement stands in the table, in its row's slice
    std::vector<uint64_t> want_doc_row(n_docs, kPackFitNoRow), last_k0(n_docs, 0);
    std::vector<uint32_t> want_doc_col(n_docs, 0);
    for (const Placed &w : want) {
        bool found = false;
        for (uint64_t i = plan->row_first[w.row]; i < plan->row_first[w.row + 1]; ++i) {
            const PackFitPiece &pc = plan->pieces[i];
            if (pc.d == w.d && pc.k0 == w.k0 && pc.col0 == w.col0 && pc.size == w.size) found = true;
        }
        if (!found) ++bad;
        if (want_doc_row[w.d] == kPackFitNoRow || w.k0 >= last_k0[w.d]) {
            want_doc_row[w.d] = w.row;
            want_doc_col[w.d] = w.col0;
            last_k0[w.d] = w.k0;
        }
    }
    for (uint64_t d = 0; d < n_docs; ++d)
        if (plan->doc_row[d] != want_doc_row[d] || plan->doc_col[d] != want_doc_col[d]) ++bad;
    // the table: sorted by (row, column), no gap, sizes not increasing, len = cells used; the full pieces first
    uint64_t F = 0, half = 0;
    for (uint64_t d = 0; d < n_docs; ++d) F += (off[d + 1] - off[d] + nbe) / S;
    if (plan->row_first[0] != 0 || plan->row_first[plan->n_rows] != plan->pieces.size()) ++bad;
    uint64_t full_d = 0, full_k = 0;
    for (uint64_t r = 0; r < plan->n_rows; ++r) {
        const uint64_t a = plan->row_first[r], b = plan->row_first[r + 1];
        if (a >= b) { ++bad; continue; }
        uint32_t col = 0, prev = S;
        for (uint64_t i = a; i < b; ++i) {
            const PackFitPiece &pc = plan->pieces[i];
            if (pc.col0 != col || pc.size == 0 || pc.size > prev) ++bad;
            col += pc.size;
            prev = pc.size;
        }
        if (col > S || plan->len[r] != col || plan->len[r] != S - free[r]) ++bad;
        if (2ull * col <= S) ++half;
        if (r < F) {
            const PackFitPiece &pc = plan->pieces[a];
            if (b - a != 1 || pc.size != S || pc.d < full_d || (pc.d == full_d && r && pc.k0 != full_k + S) ||
                (pc.d > full_d && pc.k0 != 0))
                ++bad;
            full_d = pc.d;
            full_k = pc.k0;
        }
    }
    if (half > 1) ++bad;
    // cu_seqlens: the piece starts, the pad starts and the end
    std::vector<int32_t> want_cu;
    uint32_t want_longest = 0;
    for (uint64_t r = 0; r < plan->n_rows; ++r) {
        for (uint64_t i = plan->row_first[r]; i < plan->row_first[r + 1]; ++i) {
            want_cu.push_back((int32_t)(r * S + plan->pieces[i].col0));
            if (plan->pieces[i].size > want_longest) want_longest = plan->pieces[i].size;
        }
        if (plan->len[r] < S) {
            want_cu.push_back((int32_t)(r * S + plan->len[r]));
            if (S - plan->len[r] > want_longest) want_longest = S - plan->len[r];
        }
    }
    want_cu.push_back((int32_t)(plan->n_rows * S));
    uint64_t n_seqs = 77;
    uint32_t longest = 77;
    if (pack_fit_cu_seqlens(*plan, S, nullptr, 0, &n_seqs, &longest, &msg) != MBPE_OK || n_seqs + 1 != want_cu.size() ||
        longest != want_longest)
        ++bad;
    std::vector<int32_t> cu(want_cu.size() + 1, -7);
    if (n_seqs && pack_fit_cu_seqlens(*plan, S, cu.data(), n_seqs - 1, &n_seqs, &longest, &msg) != MBPE_ERR_ARG) ++bad;
    if (cu[0] != -7) ++bad;                                  // a cap too small writes nothing
    if (pack_fit_cu_seqlens(*plan, S, cu.data(), n_seqs, &n_seqs, &longest, &msg) != MBPE_OK) ++bad;
    for (size_t i = 0; i < want_cu.size(); ++i)
        if (cu[i] != want_cu[i]) { ++bad; break; }
    if (cu[want_cu.size()] != -7) ++bad;
    if (bad) printf("seq_len %u nbe %u, %llu documents: %d errors\n", S, nbe, (unsigned long long)n_docs, bad);
    return bad;
}

static int check_lists(int *n_cases) {
    int bad = 0;
    PackFitPlan plan;                                            // kept: its vectors are reused from list to list
    const uint32_t seq_lens[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 64};
    for (uint32_t S : seq_lens)
        for (uint32_t nbe = 0; nbe < 3; ++nbe)
            for (int rep = 0; rep < 12; ++rep) {
                std::vector<uint64_t> off(1, 0);
                const uint64_t n_docs = rep ? rnd() % 61 : 0;
                for (uint64_t d = 0; d < n_docs; ++d) {
                    const uint64_t fits = S > nbe ? S - nbe : 0;
                    const uint64_t edge[] = {0, 1, fits ? fits - 1 : 0, fits, fits + 1, 2ull * S, 3ull * S + 1, rnd() % (2ull * S + 2)};
                    off.push_back(off.back() + (rep == 1 ? 0 : edge[rnd() % 8]));
                }
                bad += check_list(off, S, nbe, &plan);
                ++*n_cases;
            }
    return bad;
}

static int check_limits() {
    int bad = 0;
    const char *msg = "";
    auto expect = [&](int got, int want, const char *what) {
        if (got != want) { printf("%s: %d, want %d\n", what, got, want); ++bad; }
    };
    uint64_t F = 77;
    const uint64_t edge[2] = {0, 1ull << 40}, over[2] = {0, (1ull << 40) + 1}, huge[2] = {0, ~0ull};
    expect(pack_fit_full_rows(edge, 1, 1, 0, &F, &msg), MBPE_OK, "2^40 full rows");
    if (F != (1ull << 40)) { printf("2^40 full rows: %llu\n", (unsigned long long)F); ++bad; }
    F = 77;
    expect(pack_fit_full_rows(over, 1, 1, 0, &F, &msg), MBPE_ERR_ARG, "2^40 + 1 full rows");
    expect(pack_fit_full_rows(edge, 1, 1, 1, &F, &msg), MBPE_ERR_ARG, "2^40 tokens and bos in rows of 1");
    expect(pack_fit_full_rows(huge, 1, 1, 2, &F, &msg), MBPE_ERR_ARG, "2^64 - 1 tokens, bos and eos in rows of 1");
    if (F != 77) { printf("a refused count was written\n"); ++bad; }
    PackFitPlan plan;
    expect(pack_fit_plan(over, 1, 1, 0, &plan, &msg), MBPE_ERR_ARG, "a plan of 2^40 + 1 rows");
    // wide rows: T = 2^64 - 1 + 2 wraps, the quotient must not.  (2^64 + 1) / (2^32 - 1) = 2^32 + 1, remainder 2
    expect(pack_fit_full_rows(huge, 1, 0xFFFFFFFFu, 2, &F, &msg), MBPE_OK, "2^64 + 1 elements in rows of 2^32 - 1");
    if (F != 0x100000001ull) { printf("wide rows: %llu\n", (unsigned long long)F); ++bad; }
    // one long document in wide rows: three full pieces and a tail of 7, behind the second document's 9 elements
    const uint64_t wide[3] = {0, 3ull * 0xFFFFFFFFu + 5, 3ull * 0xFFFFFFFFu + 12};
    expect(pack_fit_plan(wide, 2, 0xFFFFFFFFu, 2, &plan, &msg), MBPE_OK, "wide plan");
    if (plan.n_rows != 4 || plan.pieces.size() != 5 || plan.doc_row[0] != 3 || plan.doc_col[0] != 9 || plan.len[3] != 9 + 7 ||
        plan.doc_row[1] != 3 || plan.doc_col[1] != 0 || plan.pieces[3].size != 9 || plan.pieces[4].size != 7 ||
        plan.pieces[4].k0 != 3ull * 0xFFFFFFFFu) {
        printf("wide plan: %llu rows, %zu pieces\n", (unsigned long long)plan.n_rows, plan.pieces.size());
        ++bad;
    }
    // cu_seqlens at 2^31 cells: 2^20 rows of 2^11 (the plan is built from full rows alone)
    std::vector<uint64_t> off(2, 0);
    off[1] = 1ull << 31;
    expect(pack_fit_plan(off.data(), 1, 1u << 11, 0, &plan, &msg), MBPE_OK, "2^31 cells");
    uint64_t n_seqs = 77;
    uint32_t longest = 77;
    expect(pack_fit_cu_seqlens(plan, 1u << 11, nullptr, 0, &n_seqs, &longest, &msg), MBPE_ERR_ARG, "cu_seqlens of 2^31 cells");
    off[1] = (1ull << 31) - 1;
    expect(pack_fit_plan(off.data(), 1, 1u << 11, 0, &plan, &msg), MBPE_OK, "2^31 - 1 elements");
    expect(pack_fit_cu_seqlens(plan, 1u << 11, nullptr, 0, &n_seqs, &longest, &msg), MBPE_ERR_ARG, "2^31 cells with a pad");
    off[1] = (1ull << 31) - (1u << 11);
    expect(pack_fit_plan(off.data(), 1, 1u << 11, 0, &plan, &msg), MBPE_OK, "2^31 - 2^11 cells");
    expect(pack_fit_cu_seqlens(plan, 1u << 11, nullptr, 0, &n_seqs, &longest, &msg), MBPE_OK, "cu_seqlens below 2^31 cells");
    if (n_seqs != (1u << 20) - 1 || longest != (1u << 11)) { printf("cu_seqlens below 2^31: %llu\n", (unsigned long long)n_seqs); ++bad; }
    return bad;
}

int main() {
    int n_cases = 0;
    const int bad = check_lists(&n_cases) + check_limits();
    printf("ok: %d lists, %d failures\n", n_cases, bad);
    return bad ? 1 : 0;
}
