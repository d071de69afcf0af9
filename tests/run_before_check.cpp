// run_before_tile (csrc/run_before.h), the host form, against a restatement of the scan it replaces: the segment join
// of k_run_partial / k_run_final (kernels.hip), folded from tile 0 up to every tile in turn.  Hand-built summary arrays
// for the cases the walk distinguishes, then random ones.  Prints "<n> failures"; exit status 0 only with none.
#include "run_before.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

struct Sum {            // the fields of TileSum (mbpe_dev.h) that the walk reads, in its layout
    uint16_t head0, head1, tail1, tail0, n_live, tail_run, pad0, pad1;
};
struct Edge {           // RankEdge
    uint32_t head0, head1, tail1, tail0, n_live_lo, n_live_hi, tail_run_lo, tail_run_hi;
};
constexpr uint32_t kHole = 0xFFFFu, kEnd = 0x8000u;

// ---- the scan, restated: element (len, token, full, empty); L then R ----
struct Seg { unsigned long long len; uint32_t token; bool full, empty; };
Seg seg_none() { return Seg{0, 0, true, true}; }
Seg seg_join(Seg l, Seg r) {
    if (r.empty) return l;
    if (l.empty) return r;
    Seg o = r;
    if (r.full && l.token == r.token) { o.len = l.len + r.len; o.full = l.full; }
    else o.full = false;
    return o;
}
Seg seg_of(const Sum &s) {
    if (s.n_live == 0) return seg_none();
    return Seg{s.tail_run, s.tail0, s.tail_run == s.n_live, false};
}
std::vector<uint32_t> scan_all(const std::vector<Sum> &sums, const Edge *le) {
    std::vector<uint32_t> out(sums.size());
    const unsigned long long edge = le ? ((unsigned long long)le->tail_run_hi << 32) | le->tail_run_lo : 0ull;
    const uint32_t edge_tok = le ? le->tail0 : kHole;
    Seg run = seg_none();
    for (size_t i = 0; i < sums.size(); ++i) {
        const bool reach = le && edge_tok != kHole && (run.empty || (run.full && run.token == edge_tok));
        const unsigned long long rb = run.len + (reach ? edge : 0ull);
        out[i] = (uint32_t)(rb & 1ull) | (rb >= 2 ? 2u : 0u);
        run = seg_join(run, seg_of(sums[i]));
    }
    return out;
}

// ---- summaries ----
Sum tile_of(uint32_t tail0, uint32_t tail_run, uint32_t n_live) {
    Sum s = {};
    s.head0 = s.head1 = s.tail1 = (uint16_t)kHole;
    s.tail0 = (uint16_t)(n_live ? tail0 : kHole);
    s.n_live = (uint16_t)n_live;
    s.tail_run = (uint16_t)(n_live ? tail_run : 0);
    return s;
}
Sum full(uint32_t t, uint32_t n = 512) { return tile_of(t, n, n); }
Sum part(uint32_t t, uint32_t run, uint32_t n = 512) { return tile_of(t, run, n); }
Sum empty() { return tile_of(kHole, 0, 0); }
Edge edge_of(uint32_t tail0, unsigned long long run) {
    Edge e = {};
    e.head0 = e.head1 = e.tail1 = kHole;
    e.tail0 = tail0;
    e.tail_run_lo = (uint32_t)run, e.tail_run_hi = (uint32_t)(run >> 32);
    return e;
}

int failures = 0;
long checked = 0;

void check(const char *name, const std::vector<Sum> &sums, const Edge *le) {
    const std::vector<uint32_t> want = scan_all(sums, le);
    const uint32_t n = (uint32_t)sums.size();
    for (uint32_t t = 0; t < n; ++t) {
        const uint32_t got = mbpe::run_before_tile(sums.data(), n, t, le);
        ++checked;
        if (got != want[t]) {
            if (failures < 20) std::printf("%s: tile %u of %u: walk %u, scan %u\n", name, t, n, got, want[t]);
            ++failures;
        }
    }
}

// every case with no edge, an edge of the same token (runs 1, 2, 3 and one past 2^32), another token, a chunk-end
// token and an edge without a token
void check_edges(const char *name, const std::vector<Sum> &sums, uint32_t t) {
    check(name, sums, nullptr);
    const unsigned long long runs[] = {1ull, 2ull, 3ull, (1ull << 32) + 1ull, (1ull << 33)};
    for (unsigned long long r : runs) {
        const Edge same = edge_of(t, r), other = edge_of(t + 1u, r), ended = edge_of(t | kEnd, 1), none = edge_of(kHole, 0);
        check(name, sums, &same);
        check(name, sums, &other);
        check(name, sums, &ended);
        check(name, sums, &none);
    }
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 33) % n);
}

}  // namespace

int main() {
    const uint32_t A = 65, B = 66;
    // the predecessor ends on a partial run: lengths 1 (odd), 2 (even, >= 2), 3, 4, 511
    for (uint32_t run : {1u, 2u, 3u, 4u, 511u})
        check_edges("partial predecessor", {part(B, 7), part(A, run), part(B, 1), full(A), part(A, 5)}, A);
    // one, two and many full tiles of one token, behind a partial run of it / of another token / nothing
    for (uint32_t n_full : {1u, 2u, 3u, 70u, 130u}) {
        for (int before = 0; before < 4; ++before) {
            std::vector<Sum> v;
            if (before == 1) v.push_back(part(A, 3));
            if (before == 2) v.push_back(part(B, 3));
            if (before == 3) v.push_back(full(B));
            for (uint32_t i = 0; i < n_full; ++i) v.push_back(full(A, i % 3 == 1 ? 511 : 512));    // (odd and even)
            v.push_back(part(B, 2));
            v.push_back(full(A, 1));
            v.push_back(part(A, 1, 9));
            check_edges("full tiles", v, A);
        }
    }
    // full tiles of a different token directly behind full tiles
    check_edges("full, other token", {full(A), full(A), full(B), full(B), full(A), part(A, 2), full(B, 3), full(B, 2)}, A);
    // empty tiles: in between, at the start, everywhere; short tiles that are one whole run
    check_edges("empties between", {part(A, 3), empty(), empty(), full(A), empty(), full(A, 7), empty(), part(B, 1)}, A);
    check_edges("empties at the start", {empty(), empty(), full(A), empty(), full(A), part(A, 1), empty()}, A);
    check_edges("all empty", {empty(), empty(), empty(), empty()}, A);
    {
        std::vector<Sum> v(200, empty());
        v[3] = part(A, 2);
        v[150] = full(A, 5);
        v[199] = full(A, 2);
        check_edges("long empty stretches", v, A);
    }
    // tile 0 alone; a single full tile
    check_edges("one tile", {part(A, 2)}, A);
    check_edges("one full tile", {full(A)}, A);
    // a chunk-end token: its raw value differs, so it continues no run and nothing continues it
    check_edges("chunk end", {full(A), full(A | kEnd, 1), full(A), part(A | kEnd, 1), full(A), full(A), full(A | kEnd, 1)}, A);
    check_edges("chunk end, edge", {full(A | kEnd, 1), full(A)}, A | kEnd);

    // random arrays: few tokens, many full and empty tiles, sizes around the 64-summary step of the device walk
    for (int round = 0; round < 4000; ++round) {
        const uint32_t n = 1u + rnd(round % 4 == 0 ? 300u : 12u);
        std::vector<Sum> v;
        const uint32_t p_full = rnd(100), p_empty = rnd(60);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t t = A + rnd(2) + (rnd(16) == 0 ? kEnd : 0u);
            const uint32_t live = 1u + rnd(512);
            if (rnd(100) < p_empty) v.push_back(empty());
            else if (rnd(100) < p_full) v.push_back(full(t, (t & kEnd) ? 1u : live));
            else v.push_back(part(t, (t & kEnd) ? 1u : 1u + rnd(live), live + 1u > 512u ? 512u : live + 1u));
        }
        check("random", v, nullptr);
        const Edge e = edge_of(rnd(8) == 0 ? kHole : A + rnd(2) + (rnd(8) == 0 ? kEnd : 0u), 1ull + rnd(5));
        check("random, edge", v, &e);
    }
    std::printf("%ld tiles checked\n%d failures\n", checked, failures);
    return failures ? 1 : 0;
}
