// Which route a training's begin takes, decided from the corpus' kind, the options and the request alone -- no device,
// no HIP: the rules of mbpe_train_begin, mbpe_train_begin_from and the options "chunk_barrier", "wide_from",
// "first_wide", "resume_wide", "min_frequency", "max_token_length" (mbpe.h), with their refusals in the order the
// entry points always gave them.  Beside it, the sizing arithmetic of the 32-bit loop's pair table (wide_run.h).
#ifndef MBPE_TRAIN_PLAN_H
#define MBPE_TRAIN_PLAN_H

#include "mbpe.h"

#include <algorithm>
#include <string>

namespace mbpe {

// Slot: the 16-bit slot stream, all the way.  SlotThenWide: the slot stream up to slot_vocab, then the conversion to
// 32-bit tokens.  WideDirect: 32-bit tokens from the first new merge, the replay's stream, no slot stream.
enum class Route { Slot, SlotThenWide, WideDirect };

struct BeginIn {
    bool chunked;
    int64_t opt_barrier, opt_first, opt_first_wide, opt_resume_wide, opt_wide_from;
    bool weighted, limited, multi;     // chunk weights; a stopping rule is set; several ranks (or "force_exchange")
    uint32_t vocab_size, n_prior;      // as the entry point checked them: vocab_size >= 256 + n_prior
};

struct BeginPlan {
    int rc;                  // MBPE_OK, or the refusal and its message
    std::string message;
    Route route;
    uint32_t slot_vocab;     // the slot stream's vocab_size (Slot: the caller's)
    bool barrier;            // chunk ends as barrier slots: by the caller's vocab_size, whatever slot_vocab is
};

inline BeginPlan plan_begin(const BeginIn &in) {
    const uint32_t V = in.vocab_size, T = V - 256;
    const uint32_t vmax = !in.chunked ? MBPE_MAX_VOCAB_BASIC : in.opt_barrier == 0 ? MBPE_MAX_VOCAB_ENDBIT : MBPE_MAX_VOCAB_CHUNKED;
    BeginPlan p = {MBPE_OK, std::string(), Route::Slot, V,
                   in.chunked && (in.opt_barrier == 1 || (in.opt_barrier != 0 && V > MBPE_MAX_VOCAB_ENDBIT))};
    auto refuse = [&](int rc, const std::string &msg) { p.rc = rc; p.message = msg; return p; };
    const std::string from = in.n_prior ? "mbpe_train_begin_from: " : "";
    const std::string too_wide = "vocab_size exceeds " + std::to_string(MBPE_MAX_VOCAB_WIDE);
    const bool first_only = in.opt_first && !in.opt_first_wide;
    // Chunk weights or a stopping rule (the rules live in the 32-bit loop's argmax): 32-bit tokens from merge n_prior on,
    // 0 included, whatever the vocabulary and either tie-break; "wide_from", "first_wide", "resume_wide" play no part.
    if (in.weighted || in.limited) {
        if (in.multi)
            return refuse(MBPE_ERR_STATE, in.weighted ? "a corpus with chunk weights trains on one rank only"
                                                      : "a training with min_frequency or max_token_length runs on one rank only");
        if (V > MBPE_MAX_VOCAB_WIDE) return refuse(MBPE_ERR_VOCAB, too_wide);
        p.route = Route::WideDirect;
        return p;
    }
    if (in.n_prior == 0) {
        // Beyond the 16-bit slot format (Token is a uint32_t in the reference, Tokenizer.h:37-38): the first vmax - 256
        // merges on the slot stream, the rest on 32-bit tokens (wide.h); one GPU, `first` only with "first_wide".
        if (V <= vmax && !(in.opt_wide_from >= 0 && (int64_t)T > in.opt_wide_from)) return p;
        if (V > MBPE_MAX_VOCAB_WIDE) return refuse(MBPE_ERR_VOCAB, too_wide);
        if (first_only || in.multi)
            return refuse(MBPE_ERR_VOCAB, "vocab_size exceeds the 16-bit slot format (" + std::to_string(vmax) +
                                              "): the 32-bit continuation runs on one GPU only, and with the `first` "
                                              "tie-break only with the option first_wide = 1");
        p.route = Route::SlotThenWide;
        p.slot_vocab = in.opt_wide_from >= 0 ? (uint32_t)std::min<int64_t>(256 + in.opt_wide_from, vmax) : vmax;
        return p;
    }
    if (in.multi) return refuse(MBPE_ERR_STATE, from + "continuing from existing merges runs on one rank only");
    // "resume_wide": T merges in all, of which the slot stream can make the first h.  T <= h: the slot case, as ever;
    // n_prior < h < T: the mixed case, the slot stream up to 256 + h, then the handover; n_prior >= h: the direct case.
    const uint32_t h = in.opt_wide_from >= 0 ? (uint32_t)std::min<int64_t>(in.opt_wide_from, vmax - 256) : vmax - 256;
    const bool beyond = in.opt_resume_wide && T > h;
    if (beyond) {
        if (V > MBPE_MAX_VOCAB_WIDE) return refuse(MBPE_ERR_VOCAB, too_wide);
        if (first_only)
            return refuse(MBPE_ERR_VOCAB, from + "vocab_size exceeds the 16-bit slot format (" + std::to_string(vmax) +
                                              "): with the `first` tie-break the 32-bit continuation runs only with the "
                                              "option first_wide = 1");
    } else if (!in.opt_resume_wide && (V > vmax || in.opt_wide_from >= 0)) {
        return refuse(MBPE_ERR_VOCAB, from + "vocab_size " + std::to_string(V) + " (with " + std::to_string(in.n_prior) +
                                          " prior merges) lies beyond the 16-bit slot format of this corpus (" +
                                          std::to_string(vmax) + "), or \"wide_from\" is set: the 32-bit continuation "
                                          "does not start from existing merges");
    }
    if (beyond) {
        p.route = in.n_prior >= h ? Route::WideDirect : Route::SlotThenWide;
        p.slot_vocab = 256 + h;
    }
    return p;
}

// Entries `merges` merges of the 32-bit loop can add at most when no count exceeds `top`: per match one (x,X) and one
// (X,y), per merge possibly the transient (X,a) of touching matches; a merge has at most `top` matches -- and at most
// one per position of the stream, which bounds it where counts are weighted (a count of 10^9 on a stream of ten tokens)
inline uint64_t wide_headroom(unsigned long long top, uint64_t positions, uint32_t merges) {
    return (uint64_t)merges * (2ull * std::min<unsigned long long>(top, positions) + 2);
}

// The 32-bit loop's pair table for `entries` pairs at load factor 1/2: 2^*bits slots, 2^12 at least.  False beyond
// 2^30 entries (*bits is 31 then).
inline bool table_bits(uint64_t entries, uint32_t *bits) {
    *bits = 12;
    while ((1ull << *bits) < 2 * entries && *bits < 31) ++*bits;
    return (1ull << *bits) >= 2 * entries;
}

}  // namespace mbpe

#endif
