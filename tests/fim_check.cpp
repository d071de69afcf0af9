// A stand-alone check of csrc/fim.h, the one statement of the fill-in-the-middle rule that the host's plan, the plan
// kernel and the gather kernel share (tests/test_fim_cpu.py builds it plain and with -fsanitize=address,undefined):
//   - for every document length 0 .. 70 and many document numbers: a <= b <= L, and the positions of the new document
//     name each old token exactly once and the three sentinels in the order of the mode;
//   - the longest document the cuts are drawn for, L = 2^32 - 2: the 64-bit products do not wrap, the cuts stay in
//     [0, L], and the positions around the parts' ends name what the rule says;
//   - L = 2^32 - 1 is an error of the call while rate > 0 (fim_plan_host names the document) and none with rate 0;
//   - the spec's own rules.
#include "fim.h"

#include <cstdio>
#include <vector>

using namespace mbpe;

static unsigned long long g_checks = 0, g_failures = 0;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond)) {                                                               \
            ++g_failures;                                                            \
            if (g_failures <= 20) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
        }                                                                            \
    } while (0)

static mbpe_fim_spec make_spec(uint64_t rate, uint64_t spm, uint64_t seed, uint64_t base) {
    mbpe_fim_spec s = {};
    s.rate = rate;
    s.spm = spm;
    s.seed = seed;
    s.doc_base = base;
    s.pre_id = 1000;
    s.suf_id = 1001;
    s.mid_id = 1002;
    return s;
}

// the new document of plan p over the tokens 0 .. L - 1, sentinels as L, L + 1, L + 2
static std::vector<unsigned long long> apply(const FimPlan &p, unsigned long long L) {
    std::vector<unsigned long long> out;
    for (unsigned long long k = 0; k < fim_len(p.mode, L); ++k) {
        const unsigned long long src = fim_source(p, L, k);
        out.push_back(src == kFimSrcPre ? L : src == kFimSrcSuf ? L + 1 : src == kFimSrcMid ? L + 2 : src);
    }
    return out;
}

static std::vector<unsigned long long> expect(const FimPlan &p, unsigned long long L) {
    std::vector<unsigned long long> out;
    auto run = [&](unsigned long long lo, unsigned long long hi) { for (unsigned long long i = lo; i < hi; ++i) out.push_back(i); };
    if (p.mode == kFimNone) { run(0, L); return out; }
    out.push_back(L);
    if (p.mode == kFimPsm) { run(0, p.a); out.push_back(L + 1); run(p.b, L); out.push_back(L + 2); run(p.a, p.b); }
    else { out.push_back(L + 1); run(p.b, L); out.push_back(L + 2); run(0, p.a); run(p.a, p.b); }
    return out;
}

int main() {
    // small documents, every mode
    unsigned long long seen[3] = {0, 0, 0};
    for (uint64_t spm : {0ull, 1ull << 31, 1ull << 32})
        for (uint64_t base : {0ull, 1ull << 40, ~0ull - 5})
            for (unsigned long long L = 0; L <= 70; ++L)
                for (unsigned long long d = 0; d < 40; ++d) {
                    const mbpe_fim_spec s = make_spec(3ull << 30, spm, 7 + L, base);
                    const FimPlan p = fim_plan_doc(s, d, L);
                    CHECK(p.mode <= kFimSpm && p.a <= p.b && p.b <= L);
                    CHECK(L > 0 || p.mode == kFimNone);
                    CHECK(p.mode != kFimNone || (p.a == 0 && p.b == 0));
                    CHECK(spm != 0 || p.mode != kFimSpm);
                    CHECK(spm != (1ull << 32) || p.mode != kFimPsm);
                    CHECK(apply(p, L) == expect(p, L));
                    ++seen[p.mode];
                }
    CHECK(seen[0] && seen[1] && seen[2]);
    // rate 0 and rate 1, the length limits
    for (unsigned long long L = 0; L <= 70; ++L) {
        mbpe_fim_spec s = make_spec(0, 1ull << 31, 1, 0);
        CHECK(fim_plan_doc(s, L, L).mode == kFimNone);
        s.rate = 1ull << 32;
        CHECK((fim_plan_doc(s, L, L).mode != kFimNone) == (L >= 1));
        s.min_tokens = 5;
        s.max_tokens = 30;
        CHECK((fim_plan_doc(s, L, L).mode != kFimNone) == (L >= 5 && L <= 30));
    }
    // the longest document: the products stay below 2^64
    {
        const unsigned long long L = kFimMaxLen;
        CHECK(L == 0xFFFFFFFEull);
        CHECK(fim_cut(0xFFFFFFFFu, L) == L);                     // (2^32 - 1)^2 >> 32 == 2^32 - 2
        CHECK(fim_cut(0u, L) == 0 && fim_cut(0x80000000u, L) == 0x7FFFFFFFull);
        mbpe_fim_spec s = make_spec(1ull << 32, 1ull << 31, 99, 0);
        for (unsigned long long d = 0; d < 200; ++d) {
            const FimPlan p = fim_plan_doc(s, d, L);
            CHECK(p.mode != kFimNone && p.a <= p.b && p.b <= L);
            CHECK(!fim_too_long(s, L) && fim_len(p.mode, L) == L + 3);
            const unsigned long long ns = L - p.b;
            CHECK(fim_source(p, L, 0) == kFimSrcPre);
            if (p.mode == kFimPsm) {
                CHECK(fim_source(p, L, p.a + 1) == kFimSrcSuf && fim_source(p, L, p.a + 2 + ns) == kFimSrcMid);
                if (p.a) CHECK(fim_source(p, L, p.a) == p.a - 1);
                if (ns) CHECK(fim_source(p, L, p.a + 2) == p.b && fim_source(p, L, p.a + 1 + ns) == L - 1);
                if (p.b > p.a) CHECK(fim_source(p, L, p.a + 3 + ns) == p.a && fim_source(p, L, L + 2) == p.b - 1);
            } else {
                CHECK(fim_source(p, L, 1) == kFimSrcSuf && fim_source(p, L, 2 + ns) == kFimSrcMid);
                if (ns) CHECK(fim_source(p, L, 2) == p.b && fim_source(p, L, 1 + ns) == L - 1);
                if (p.b) CHECK(fim_source(p, L, 3 + ns) == 0 && fim_source(p, L, L + 2) == p.b - 1);
            }
        }
    }
    // one token more is an error of the call while rate > 0
    {
        const unsigned long long L = kFimMaxLen + 1;
        mbpe_fim_spec s = make_spec(1, 0, 0, 0);
        CHECK(fim_too_long(s, L) && fim_too_long(s, ~0ull) && !fim_too_long(s, L - 1));
        CHECK(fim_plan_doc(s, 0, L).mode == kFimNone);
        const uint64_t off[4] = {0, 5, 5 + L, 5 + L + 2};
        uint64_t out[4] = {1, 1, 1, 1}, bad = 77;
        CHECK(fim_plan_host(off, 3, s, out, nullptr, nullptr, &bad) == MBPE_ERR_ARG && bad == 1);
        s.rate = 0;
        CHECK(!fim_too_long(s, L));
        uint8_t mode[3] = {9, 9, 9};
        uint64_t cut[6] = {9, 9, 9, 9, 9, 9};
        CHECK(fim_plan_host(off, 3, s, out, mode, cut, &bad) == MBPE_OK);
        CHECK(out[0] == 0 && out[1] == 5 && out[2] == 5 + L && out[3] == 5 + L + 2);
        for (int i = 0; i < 3; ++i) CHECK(mode[i] == 0 && cut[2 * i] == 0 && cut[2 * i + 1] == 0);
    }
    // the spec's rules
    {
        const char *msg = nullptr;
        mbpe_fim_spec s = make_spec(1ull << 32, 1ull << 32, 0, 0);
        CHECK(fim_check_spec(&s, 32, &msg) == MBPE_OK && fim_check_spec(&s, 16, &msg) == MBPE_OK);
        CHECK(fim_check_spec(nullptr, 32, &msg) == MBPE_ERR_ARG);
        s.rate = (1ull << 32) + 1;
        CHECK(fim_check_spec(&s, 32, &msg) == MBPE_ERR_ARG);
        s.rate = 0;
        s.spm = ~0ull;
        CHECK(fim_check_spec(&s, 32, &msg) == MBPE_ERR_ARG);
        s.spm = 0;
        s.min_tokens = 4;
        s.max_tokens = 3;
        CHECK(fim_check_spec(&s, 32, &msg) == MBPE_ERR_ARG);
        s.max_tokens = 0;
        CHECK(fim_check_spec(&s, 32, &msg) == MBPE_OK);
        s.mid_id = 0x7FFFFFFDu;
        CHECK(fim_check_spec(&s, 32, &msg) == MBPE_OK && fim_check_spec(&s, 16, &msg) == MBPE_ERR_VOCAB);
        s.mid_id = 0x7FFFFFFEu;
        CHECK(fim_check_spec(&s, 32, &msg) == MBPE_ERR_ARG && fim_check_spec(&s, 16, &msg) == MBPE_ERR_ARG);
        s.mid_id = 65536;
        CHECK(fim_check_spec(&s, 16, &msg) == MBPE_ERR_VOCAB);
        s.mid_id = 65535;
        CHECK(fim_check_spec(&s, 16, &msg) == MBPE_OK);
    }
    std::printf("ok: %llu checks, %llu failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
