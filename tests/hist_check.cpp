// The host restatements of csrc/hist.h against a std::map count, on cases this program generates: the lengths of
// tests/hist_cases.py (0, 1, 63 .. 65, 1,023 .. 1,025, 4,095 .. 4,097, 2^20 + 3) at every element offset within 16 bytes,
// ids at 2^k - 1, 2^k, 2^k + 1 for k = 8 .. 24, table sizes 1 .. 2^25, all tokens equal, 16-bit elements with 65,535,
// 32-bit elements with bit 31 set; hist_runs with empty runs, run weights of 2^32 - 1 and elements behind the last run;
// the fold with repeat = 2^61.  Built plain and with -fsanitize=address,undefined by tests/test_hist_cpu.py.
#include "hist.h"

#include <cstdio>
#include <map>
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

void fail(const char *what, uint64_t a, uint64_t b, uint64_t c) {
    ++failures;
    std::printf("FAIL %s: %llu %llu %llu\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
}

// counts against the map: every entry of the map, and the table's sum (so nothing else is non-zero)
bool same(const std::vector<unsigned long long> &counts, unsigned long long other,
          const std::map<uint32_t, unsigned long long> &want, uint64_t n_ids) {
    unsigned long long in = 0, out = 0, sum = 0;
    for (const auto &kv : want) {
        if (kv.first < n_ids) {
            if (counts[kv.first] != kv.second) return false;
            in += kv.second;
        } else {
            out += kv.second;
        }
    }
    for (unsigned long long c : counts) sum += c;
    return sum == in && other == out;
}

template <typename T>
void check_tokens(const std::vector<T> &elems, uint64_t n_ids, const char *what) {
    std::map<uint32_t, unsigned long long> want;
    for (T e : elems) ++want[mbpe::hist_id(e, sizeof(T))];
    for (uint64_t addr = 0; addr < 16; addr += sizeof(T)) {
        ++cases;
        std::vector<unsigned long long> counts(n_ids, 0);
        unsigned long long other = 0;
        uint64_t max_local = 0;
        mbpe::hist_host<T>(elems.data(), elems.size(), 4096 + addr, counts.data(), n_ids, &other, &max_local);
        if (!same(counts, other, want, n_ids) || max_local > elems.size()) fail(what, sizeof(T), elems.size(), n_ids);
        if (n_ids > 65537) break;                    // (the large tables once: they are the same walk)
    }
}

std::vector<uint32_t> edge_tokens(uint64_t n) {
    std::vector<uint32_t> ids;
    for (int k = 8; k <= 24; ++k)
        for (int d = -1; d <= 1; ++d) ids.push_back((uint32_t)((1u << k) + d));
    std::vector<uint32_t> t(n);
    for (uint64_t i = 0; i < n; ++i) t[i] = i % 3 == 0 ? ids[(i / 3) % ids.size()] : rnd((1u << 25) + 2);
    return t;
}

void check_runs(const std::vector<uint32_t> &lens, const std::vector<unsigned long long> &w, uint64_t extra, uint64_t n_ids,
                const char *what) {
    ++cases;
    std::vector<uint32_t> table;
    std::vector<unsigned long long> ends;
    std::map<uint32_t, unsigned long long> want;
    unsigned long long want_total = 0;
    for (size_t j = 0; j < lens.size(); ++j) {
        for (uint32_t k = 0; k < lens[j]; ++k) {
            const uint32_t id = rnd(3) ? rnd(300) : rnd(70000);
            table.push_back(id | (k + 1 == lens[j] ? mbpe::kTokEnd : 0u));
            want[id] += w[j];
            want_total += w[j];
        }
        ends.push_back(table.size());
    }
    for (uint64_t k = 0; k < extra; ++k) table.push_back(7);      // behind the last run: nobody copies them
    std::vector<unsigned long long> counts(n_ids, 0);
    unsigned long long other = 0, total = 0;
    mbpe::hist_runs_host<uint32_t>(table.data(), table.size(), ends.data(), ends.size(), w.data(), counts.data(), n_ids,
                                   &other, &total);
    if (!same(counts, other, want, n_ids) || total != want_total) fail(what, lens.size(), table.size(), n_ids);
}

}  // namespace

int main() {
    const uint64_t lengths[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, (1u << 20) + 3};
    const uint64_t n_ids_small[] = {1, 256, 257, 65536, 65537};
    for (uint64_t n : lengths) {
        const std::vector<uint32_t> t = edge_tokens(n);
        for (uint64_t n_ids : n_ids_small) {
            if (n > 4097 && n_ids != 65537) continue;             // (the long one once per element width)
            check_tokens<uint32_t>(t, n_ids, "edge ids, 32 bits");
        }
        std::vector<uint32_t> flagged(t);
        for (uint64_t i = 0; i < n; i += 3) flagged[i] |= mbpe::kTokEnd;
        check_tokens<uint32_t>(flagged, 65537, "bit 31 on a third");
        std::vector<uint16_t> t16(n);
        for (uint64_t i = 0; i < n; ++i) t16[i] = i % 5 == 0 ? 65535 : (uint16_t)t[i];
        check_tokens<uint16_t>(t16, 65536, "16 bits with 65,535");
        check_tokens<uint16_t>(t16, 257, "16 bits, small table");
    }
    {
        const std::vector<uint32_t> t = edge_tokens(5000);
        check_tokens<uint32_t>(t, 1u << 24, "2^24 ids");
        check_tokens<uint32_t>(t, 1u << 25, "2^25 ids");
        for (uint32_t id : {0u, 256u, 257u}) {                     // all tokens equal: id 0, n_ids - 1, beyond the table
            const std::vector<uint32_t> eq(9000, id);
            check_tokens<uint32_t>(eq, 257, "all equal");
        }
    }
    // runs: empty ones, one long one, weights of 0, 1 and 2^32 - 1, elements behind the last run
    {
        const unsigned long long big = 0xFFFFFFFFull;
        check_runs({}, {}, 0, 300, "no run");
        check_runs({0}, {5}, 3, 300, "one empty run");
        check_runs({3, 0, 0, 5000, 1, 0, 2}, {1, 9, big, big, 0, 4, big}, 5, 300, "runs");
        check_runs({1, 1, 1, 1}, {big, big, big, big}, 0, 70000, "one-token runs");
        std::vector<uint32_t> lens;
        std::vector<unsigned long long> w;
        for (int j = 0; j < 1500; ++j) { lens.push_back(rnd(6)); w.push_back(rnd(2) ? rnd(1000) : big - rnd(3)); }
        check_runs(lens, w, 0, 65536, "1,500 runs");
    }
    // the fold: any 32-bit step would show in repeat = 2^61 and in counts of 2^32 - 1
    {
        ++cases;
        std::vector<unsigned long long> kept = {1, 0, 5, 7}, call = {4, 1, 0, 3};
        mbpe::hist_fold_host(kept.data(), call.data(), kept.size(), 1ull << 61);
        if (kept[0] != (1ull << 63) + 1 || kept[1] != (1ull << 61) || kept[2] != 5 || kept[3] != 3 * (1ull << 61) + 7)
            fail("fold 2^61", kept[0], kept[1], kept[3]);
        ++cases;
        std::vector<unsigned long long> k2 = {10}, c2 = {0xFFFFFFFFull};
        mbpe::hist_fold_host(k2.data(), c2.data(), 1, 0xFFFFFFFFull);
        if (k2[0] != 0xFFFFFFFE00000001ull + 10) fail("fold (2^32 - 1)^2", k2[0], 0, 0);
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
