// Multi-turn conversations joined into one document each (turns.hip; mbpe_turns_plan, mbpe_turns_tokens,
// mbpe_encoder_set_turns): a system prompt and any number of user and assistant turns, the loss on the trained turns.
//
// A call has n_docs documents, the turns; conversation c owns turns turn_off[c] .. turn_off[c + 1], and flags[t] says
// whether turn t is trained (MBPE_TURN_TRAIN) and whether it goes without the turn-end id (MBPE_TURN_NO_END).  A turn of
// len tokens has len + has_end ids.  G, "the concatenation", is every turn's ids one after the other: pos[t] is where
// turn t begins in it, so a conversation of m turns from turn t0 on is G[pos[t0] .. pos[t0 + m]) and, where end_id is
// set, one more id.  What is kept of it is at most two ranges of G -- the head and the rest -- and that end id:
// turns_keep.  Everything here is integer arithmetic that a host compiler builds too; the host's plan and the plan
// kernel share this one statement of the rule.
#ifndef MBPE_TURNS_H
#define MBPE_TURNS_H

#include "mbpe.h"

#include "span.h"

namespace mbpe {

constexpr uint32_t kTnRight = 0, kTnLeft = 1, kTnDropOldest = 2;                 // spec.truncation
constexpr uint32_t kTnLabelAll = 0, kTnLabelTrained = 1;                         // spec.label_mode
constexpr uint32_t kTnMaxId = 0x7FFFFFFEu;                                       // turn_end_id and end_id lie below it
constexpr uint8_t kTnTrain = MBPE_TURN_TRAIN, kTnNoEnd = MBPE_TURN_NO_END;

// what is kept of one conversation: G[g0 .. g0 + a), then G[g1 .. g1 + b) with g1 >= g0 + a, then e (0 or 1) end ids
struct TnKeep {
    unsigned long long g0, a, g1, b, e;
    unsigned long long dropped, cut;         // whole turns dropped by DROP_OLDEST; ids removed by the RIGHT or LEFT cut
};

MBPE_HD unsigned long long tn_min(unsigned long long x, unsigned long long y) { return x < y ? x : y; }

// the ids of a turn of len tokens with these flags
MBPE_HD unsigned long long turns_width(const mbpe_turns_spec &s, unsigned long long len, uint8_t flags) {
    return len + (s.turn_end_id != MBPE_NO_TOKEN && !(flags & kTnNoEnd) ? 1u : 0u);
}

// what is kept of the conversation of m turns whose turns begin at P[0 .. m] in G (P[m]: where its last turn ends) and
// have the flags fl[0 .. m)
MBPE_HD TnKeep turns_keep(const mbpe_turns_spec &s, const unsigned long long *P, const uint8_t *fl, uint64_t m) {
    const unsigned long long E = s.end_id != MBPE_NO_TOKEN ? 1u : 0u, T = P[m] - P[0], N = T + E, K = s.max_tokens;
    TnKeep k = {P[0], T, P[m], 0, E, 0, 0};
    if (K == 0) return k;
    if (s.truncation == kTnRight || s.truncation == kTnLeft) {
        const unsigned long long kept = tn_min(N, K), skip = s.truncation == kTnLeft ? tn_min(N - kept, T) : 0;
        k.g0 = P[0] + skip;
        k.a = tn_min(T - skip, kept);
        k.g1 = k.g0 + k.a;
        k.e = kept - k.a;
        k.cut = N - kept;
        return k;
    }
    // DROP_OLDEST: F(j) = H + (P[m] - P[j]) + E <= K  <=>  P[j] >= P[m] + H + E - K, and P ascends
    const uint64_t h = s.head_turns < m ? s.head_turns : m;
    const unsigned long long H = P[h] - P[0], lim = P[m] + H + E;
    uint64_t j = lim <= K ? h : h + lower_bound64(P + h, m - h + 1, lim - K);
    if (j > m) j = m;                                            // (no j fits: the head and the end id alone)
    while (j < m && (fl[j] & kTnTrain)) ++j;                     // never open on an answer without its question
    const unsigned long long R = P[m] - P[j], L = H + R + E, kept = tn_min(L, K);
    k.a = tn_min(H, kept);
    k.g1 = P[j];
    k.b = tn_min(R, kept - k.a);
    k.e = kept - k.a - k.b;
    k.dropped = j - h;
    k.cut = L - kept;
    return k;
}

MBPE_HD unsigned long long turns_len(const TnKeep &k) { return k.a + k.b + k.e; }

// how many kept ids of G lie below position g
MBPE_HD unsigned long long turns_below(const TnKeep &k, unsigned long long g) {
    const unsigned long long x = g > k.g0 ? tn_min(g - k.g0, k.a) : 0, y = g > k.g1 ? tn_min(g - k.g1, k.b) : 0;
    return x + y;
}

// the rules of a spec for tokens of token_bits bits, without a word: MBPE_OK, MBPE_ERR_ARG or MBPE_ERR_VOCAB, *msg says why
inline int turns_check_spec(const mbpe_turns_spec *s, uint32_t token_bits, const char **msg) {
    *msg = "";
    if (!s) { *msg = "NULL turns spec"; return MBPE_ERR_ARG; }
    if (s->truncation > kTnDropOldest || s->label_mode > kTnLabelTrained) { *msg = "a turns enum out of range"; return MBPE_ERR_ARG; }
    uint32_t top = s->end_id != MBPE_NO_TOKEN ? s->end_id : 0u;
    if (s->turn_end_id != MBPE_NO_TOKEN && s->turn_end_id > top) top = s->turn_end_id;
    if (top >= kTnMaxId) { *msg = "a turn_end_id or end_id of 2^31 - 2 or more"; return MBPE_ERR_ARG; }
    if (token_bits == 16 && top >= 65536u) { *msg = "a turn_end_id or end_id that does not fit 16-bit tokens"; return MBPE_ERR_VOCAB; }
    return MBPE_OK;
}

// the rules of turn_off (n_convs + 1) and flags (n_docs): MBPE_OK or MBPE_ERR_ARG, *msg says why
inline int turns_check_arrays(const uint64_t *turn_off, uint64_t n_convs, const uint8_t *flags, uint64_t n_docs,
                              const char **msg) {
    *msg = "";
    if (!turn_off || (!flags && n_docs)) { *msg = "NULL turn_off or flags"; return MBPE_ERR_ARG; }
    if (turn_off[0] != 0) { *msg = "turn_off must begin at 0"; return MBPE_ERR_ARG; }
    for (uint64_t c = 0; c < n_convs; ++c)
        if (turn_off[c + 1] < turn_off[c]) { *msg = "turn_off must be ascending"; return MBPE_ERR_ARG; }
    if (turn_off[n_convs] != n_docs) { *msg = "turn_off must end at the document count"; return MBPE_ERR_ARG; }
    for (uint64_t t = 0; t < n_docs; ++t)
        if (flags[t] & ~(kTnTrain | kTnNoEnd)) { *msg = "a turn flag beyond MBPE_TURN_TRAIN | MBPE_TURN_NO_END"; return MBPE_ERR_ARG; }
    return MBPE_OK;
}

// the host's plan of n_docs turns with token offsets off[0 .. n_docs]: pos (n_docs + 1, scratch of the caller), off_out
// (n_convs + 1) and, where given, info_out (dropped, cut per conversation)
inline void turns_plan_host(const uint64_t *off, uint64_t n_docs, const uint64_t *turn_off, uint64_t n_convs,
                            const uint8_t *flags, const mbpe_turns_spec &s, unsigned long long *pos, uint64_t *off_out,
                            uint64_t *info_out) {
    pos[0] = 0;
    for (uint64_t t = 0; t < n_docs; ++t) pos[t + 1] = pos[t] + turns_width(s, off[t + 1] - off[t], flags[t]);
    uint64_t o = 0;
    for (uint64_t c = 0; c < n_convs; ++c) {
        const uint64_t t0 = turn_off[c];
        const TnKeep k = turns_keep(s, pos + t0, flags + t0, turn_off[c + 1] - t0);
        off_out[c] = o;
        o += turns_len(k);
        if (info_out) { info_out[2 * c] = k.dropped; info_out[2 * c + 1] = k.cut; }
    }
    off_out[n_convs] = o;
}

#ifdef __HIPCC__
// ---- the device stage (turns.hip) --------------------------------------------------------------------------------------
// What it leaves on the device for n_convs > 0 conversations: pos = the turns' starts in G (n_docs + 1) and off = the
// joined documents' token offsets (n_convs + 1; off[n_convs] the joined token count), each with its scan's scratch
// behind it; plan = g0, a, g1, b per conversation; info = dropped, cut per conversation; rec = the records the gather
// searches (turns.hip); tok = the joined stream, plain ids of `bits`; tgt = its targets (NULL: none are written).
uint64_t turns_pos_bytes(uint64_t n_docs);
uint64_t turns_off_bytes(uint64_t n_convs);
uint64_t turns_rec_bytes(uint64_t n_docs, uint64_t n_convs);
struct TurnsSrc {
    const void *tok;                         // `bits` bits: 16 plain ids, 32 with bit 31 ignored
    uint32_t bits;
    const unsigned long long *doc_off;       // n_docs + 1
    uint64_t n_docs;
    const unsigned long long *turn_off;      // n_convs + 1
    uint64_t n_convs;
    const uint8_t *flags;                    // n_docs
};
struct TurnsDst {
    void *tok;
    uint32_t *tgt;
    uint64_t cap;                            // ids tok (and tgt) holds; the kernel writes no more than these
    unsigned long long *pos;                 // turns_pos_bytes(n_docs)
    unsigned long long *off;                 // turns_off_bytes(n_convs)
    unsigned long long *plan;                // 4 * n_convs
    unsigned long long *info;                // 2 * n_convs
    unsigned long long *rec;                 // turns_rec_bytes(n_docs, n_convs)
};

// the kernels of turns.hip on `stream`, everything in device memory.  n_convs > 0.  Nothing is waited for and nothing
// comes back: the joined token count is the word at dst.off + n_convs
void turns_launch(hipStream_t stream, const TurnsSrc &src, const mbpe_turns_spec &spec, const TurnsDst &dst);
#endif

}  // namespace mbpe

#endif
