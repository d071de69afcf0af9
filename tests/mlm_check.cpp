// A stand-alone check of csrc/mlm.h, the one statement of the masked-LM rule that the host's plan and the apply kernel
// share (tests/test_mlm_cpu.py builds it plain and with -fsanitize=address,undefined).
//   mlm_check          the header's own invariants: the spec's rules, the thresholds' extremes, protected ids, words
//                      selected as wholes, targets, the largest vocab_n the product is formed for
//   mlm_check apply    reads cases from standard input and writes what mlm_plan_host makes of them, which the test
//                      compares with the rule restated in Python (tests/mlm_cases.py).  A case is, in decimal numbers
//                      separated by blanks: select mask random seed doc_base mask_id vocab_n whole_word n_protect, the 8
//                      protect ids, bits n_docs n_tokens, the n_docs + 1 offsets, the tokens; the answer is one line of
//                      new ids and one of targets.  The input begins with the number of cases.
#include "mlm.h"

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

static mbpe_mlm_spec make_spec(uint64_t select, uint64_t mask, uint64_t random, uint32_t ww) {
    mbpe_mlm_spec s = {};
    s.select = select;
    s.mask = mask;
    s.random = random;
    s.seed = 5;
    s.mask_id = 70000;
    s.vocab_n = 1000;
    s.whole_word = ww;
    return s;
}

static int apply_cases() {
    unsigned long long n_cases = 0;
    if (std::scanf("%llu", &n_cases) != 1) return 2;
    for (unsigned long long c = 0; c < n_cases; ++c) {
        mbpe_mlm_spec s = {};
        unsigned long long v[5];
        unsigned w[4], bits = 0;
        unsigned long long n_docs = 0, n_tokens = 0;
        if (std::scanf("%llu %llu %llu %llu %llu %u %u %u %u", &v[0], &v[1], &v[2], &v[3], &v[4], &w[0], &w[1], &w[2], &w[3]) != 9)
            return 2;
        s.select = v[0]; s.mask = v[1]; s.random = v[2]; s.seed = v[3]; s.doc_base = v[4];
        s.mask_id = w[0]; s.vocab_n = w[1]; s.whole_word = w[2]; s.n_protect = w[3];
        for (int i = 0; i < 8; ++i)
            if (std::scanf("%u", &s.protect[i]) != 1) return 2;
        if (std::scanf("%u %llu %llu", &bits, &n_docs, &n_tokens) != 3) return 2;
        const char *msg = "";
        if (mlm_check_spec(&s, bits, &msg) != MBPE_OK) { std::printf("bad spec: %s\n", msg); return 2; }
        std::vector<uint64_t> off(n_docs + 1);
        for (auto &o : off) {
            unsigned long long x;
            if (std::scanf("%llu", &x) != 1) return 2;
            o = x;
        }
        std::vector<uint32_t> t32(n_tokens), o32(n_tokens), tgt(n_tokens);
        std::vector<uint16_t> t16(n_tokens), o16(n_tokens);
        for (unsigned long long i = 0; i < n_tokens; ++i) {
            unsigned x;
            if (std::scanf("%u", &x) != 1) return 2;
            t32[i] = x;
            t16[i] = (uint16_t)x;
        }
        if (bits == 16) mlm_plan_host(t16.data(), 16, off.data(), n_docs, s, o16.data(), tgt.data());
        else mlm_plan_host(t32.data(), 32, off.data(), n_docs, s, o32.data(), tgt.data());
        for (unsigned long long i = 0; i < n_tokens; ++i) std::printf("%u ", bits == 16 ? (unsigned)o16[i] : o32[i]);
        std::printf("\n");
        for (unsigned long long i = 0; i < n_tokens; ++i) std::printf("%u ", tgt[i]);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char **) {
    if (argc > 1) return apply_cases();
    const uint64_t one = kDropoutOne;
    // a stream of 3 documents; words of 1 .. 4 tokens; the last token of document 1 is not flagged
    const uint64_t off[4] = {0, 7, 40, 64};
    std::vector<uint32_t> tok(64);
    for (uint32_t i = 0; i < 64; ++i) tok[i] = (i * 37u) % 1000u | ((i % 4u == 3u || i % 7u == 0u) ? kTokEnd : 0u);
    tok[39] &= kTokIdMask;
    std::vector<uint32_t> out(64), tgt(64);
    // select 0: the identity, no target -- with and without whole words
    for (uint32_t ww = 0; ww < 2; ++ww) {
        mbpe_mlm_spec s = make_spec(0, one, 0, ww);
        mlm_plan_host(tok.data(), 32, off, 3, s, out.data(), tgt.data());
        for (uint32_t i = 0; i < 64; ++i) CHECK(out[i] == (tok[i] & kTokIdMask) && tgt[i] == MBPE_NO_TOKEN);
    }
    // select 2^32: every token a target; mask 2^32: all mask_id; random 2^32: all below vocab_n; both 0: ids stay
    {
        mbpe_mlm_spec s = make_spec(one, one, 0, 0);
        mlm_plan_host(tok.data(), 32, off, 3, s, out.data(), tgt.data());
        for (uint32_t i = 0; i < 64; ++i) CHECK(out[i] == 70000u && tgt[i] == (tok[i] & kTokIdMask));
        s = make_spec(one, 0, one, 1);
        s.vocab_n = 10;
        mlm_plan_host(tok.data(), 32, off, 3, s, out.data(), tgt.data());
        for (uint32_t i = 0; i < 64; ++i) CHECK(out[i] < 10u && tgt[i] == (tok[i] & kTokIdMask));
        s = make_spec(one, 0, 0, 1);
        mlm_plan_host(tok.data(), 32, off, 3, s, out.data(), tgt.data());
        for (uint32_t i = 0; i < 64; ++i) CHECK(out[i] == (tok[i] & kTokIdMask) && tgt[i] == out[i]);
        // protected ids stay and are no targets
        s = make_spec(one, one, 0, 1);
        s.n_protect = 2;
        s.protect[0] = tok[5] & kTokIdMask;
        s.protect[1] = tok[41] & kTokIdMask;
        s.protect[2] = tok[6] & kTokIdMask;                      // beyond n_protect: not protected
        mlm_plan_host(tok.data(), 32, off, 3, s, out.data(), tgt.data());
        for (uint32_t i = 0; i < 64; ++i) {
            const uint32_t id = tok[i] & kTokIdMask;
            const bool prot = id == s.protect[0] || id == s.protect[1];
            CHECK(prot ? (out[i] == id && tgt[i] == MBPE_NO_TOKEN) : (out[i] == 70000u && tgt[i] == id));
        }
    }
    // whole words: all tokens of a word are targets or none is; the outputs may be NULL
    {
        unsigned long long words = 0, hit = 0;
        for (uint64_t seed = 0; seed < 50; ++seed) {
            mbpe_mlm_spec s = make_spec(one / 2, one, 0, 1);
            s.seed = seed;
            s.doc_base = ~0ull - 1;                              // (wraps inside the call)
            mlm_plan_host(tok.data(), 32, off, 3, s, nullptr, tgt.data());
            mlm_plan_host(tok.data(), 32, off, 3, s, out.data(), nullptr);
            for (uint64_t d = 0; d < 3; ++d) {
                uint64_t w0 = off[d];
                for (uint64_t i = off[d]; i < off[d + 1]; ++i) {
                    CHECK((tgt[i] != MBPE_NO_TOKEN) == (tgt[w0] != MBPE_NO_TOKEN));
                    CHECK((out[i] == 70000u) == (tgt[i] != MBPE_NO_TOKEN));
                    if ((tok[i] & kTokEnd) || i + 1 == off[d + 1]) {
                        ++words;
                        hit += tgt[w0] != MBPE_NO_TOKEN;
                        w0 = i + 1;
                    }
                }
            }
        }
        CHECK(hit > words / 3 && hit < 2 * words / 3);
    }
    // the product of the largest vocab_n stays below 2^64 and the id below vocab_n
    {
        mbpe_mlm_spec s = make_spec(one, 0, one, 0);
        s.vocab_n = kMlmMaxId - 1;
        uint32_t t = 0, top = 0;
        for (unsigned long long k = 0; k < 2000; ++k) {
            const uint32_t v = mlm_token(s, mlm_doc_seed(s, k), k, k, 7u, &t);
            CHECK(v < s.vocab_n && t == 7u);
            top = v > top ? v : top;
        }
        CHECK(top > s.vocab_n / 2);
    }
    // the spec's rules
    {
        const char *msg = nullptr;
        mbpe_mlm_spec s = make_spec(one, one / 2, one / 2, 0);
        s.mask_id = 65535;
        s.vocab_n = 65536;
        CHECK(mlm_check_spec(&s, 32, &msg) == MBPE_OK && mlm_check_spec(&s, 16, &msg) == MBPE_OK);
        CHECK(mlm_check_spec(nullptr, 32, &msg) == MBPE_ERR_ARG);
        mbpe_mlm_spec b = s;
        b.select = one + 1;
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_ERR_ARG);
        b = s; b.mask = one + 1; b.random = 0;
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_ERR_ARG);
        b = s; b.random = ~0ull; b.mask = 1;                     // (their sum wraps: each is checked first)
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_ERR_ARG);
        b = s; b.random = one / 2 + 1;
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_ERR_ARG);
        b = s; b.vocab_n = 0;
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_ERR_ARG);
        b.random = 0;
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_OK);
        b = s; b.n_protect = 9;
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_ERR_ARG);
        b.n_protect = 8;
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_OK);
        b = s; b.whole_word = 2;
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_ERR_ARG);
        b.whole_word = 1;
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_OK && mlm_check_spec(&b, 16, &msg) == MBPE_ERR_ARG);
        b = s; b.mask_id = kMlmMaxId;
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_ERR_ARG && mlm_check_spec(&b, 16, &msg) == MBPE_ERR_ARG);
        b.mask_id = kMlmMaxId - 1;
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_OK && mlm_check_spec(&b, 16, &msg) == MBPE_ERR_VOCAB);
        b = s; b.vocab_n = kMlmMaxId;
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_ERR_ARG);
        b.vocab_n = 65537;
        CHECK(mlm_check_spec(&b, 32, &msg) == MBPE_OK && mlm_check_spec(&b, 16, &msg) == MBPE_ERR_VOCAB);
        b = s; b.mask_id = 65536;
        CHECK(mlm_check_spec(&b, 16, &msg) == MBPE_ERR_VOCAB);
    }
    std::printf("ok: %llu checks, %llu failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
