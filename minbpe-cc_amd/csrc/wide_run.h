// Host side of the 32-bit training loop (wide.h): its device buffers, its begin from a slot stream (the conversion) or
// from replayed tokens (the direct begin), the groups of merges with the growth of the pair table between them, and
// what the C-ABI's readers report once a training runs here.  Knows nothing of the training context: the caller
// (train.cpp) decides the route (train_plan.h) and passes what each call needs.
#ifndef MBPE_WIDE_RUN_H
#define MBPE_WIDE_RUN_H

#include "dev_pool.h"
#include "mbpe.h"
#include "wide.h"

#include <vector>

namespace mbpe {

// the context's side of every call: its stream, its two timing events, its pool, and the stats the loop adds to
struct WideDev { hipStream_t stream; hipEvent_t ev0, ev1; DevPool &pool; int n_cus; mbpe_stats &stats; };

// what a begin says of the loop ahead: the merges it may make, the id of its first one, the tie-break
struct WideGoal { uint32_t n_wide, new_id_base; bool first; };

// The conversion's source: a compacted slot stream (no holes among the first n_slots slots, n_barriers of them barrier
// slots; barrier / endbit as launch_wide_from_slots takes them), the hashed pair table's n_entries entries, and a
// bound of every count from here on (~0: none known).
struct WideSlots {
    const uint16_t *slots; uint64_t n_slots, n_barriers; uint32_t barrier, endbit;
    const uint32_t *ekey; const int32_t *ecnt; uint32_t n_entries; unsigned long long top;
};

// The direct begin's source: the replay's n_tok flagged tokens (*tok: an array of the caller's, freed here once they are
// copied) and its device time, the prior merges, the corpus' chunk weights (NULL: none), the stopping rules (0: none).
struct WideTokens {
    uint32_t **tok; uint64_t n_tok; float ms_replay;
    const uint32_t *prior; uint32_t n_prior, vocab_total;
    const uint32_t *weights; uint64_t n_weights;
    int64_t min_frequency, max_token_length;
};

struct WideRun {
    uint32_t *tok[2] = {nullptr, nullptr};
    int cur = 0;
    uint32_t *val = nullptr, *scratch = nullptr;
    uint32_t *wt[2] = {nullptr, nullptr};   // weighted corpus: the weight of every token's chunk, beside tok[]
    WideTable tab = {};
    WideCtl *ctl = nullptr;
    WideBest *best = nullptr;
    unsigned long long *arg = nullptr;
    WideFirst *fs = nullptr;         // `first` tie-break scratch
    WideTally *tally = nullptr;      // the census of a direct begin's pair count
    WideLimits lim = {};             // the stopping rules the training was begun with (lim.len: vocab_total u32 of the pool)
    WideGoal goal = {};
    unsigned long long top0 = 0;     // what the begin knew of the first merge's count: no count exceeds it
    uint64_t n_upper = 0;            // host-side upper bound of the stream length
    uint32_t k = 0;                  // merges known to the host
    WideCtl h_ctl = {};
    std::vector<WideBest> h_best;    // ... and what they were
    bool active = false;             // the training's stream, table and merge counter live here

    void release(DevPool &pool);     // every buffer back to the pool, every member as it is declared above
    int convert(const WideDev &d, const WideSlots &src, const WideGoal &goal);
    int begin_from(const WideDev &d, const WideTokens &src, const WideGoal &goal);
    int steps(const WideDev &d, uint32_t n_steps, uint32_t *done_out);

    // what mbpe_get_stream, mbpe_stream_device, mbpe_get_pairs, mbpe_train_result and mbpe_get_stats report of it
    int get_stream(bool chunked, uint32_t *tokens_out, uint8_t *chunk_end_out, uint64_t cap, uint64_t *n_out) const;
    int stream_device(const WideDev &d, const void **slots_out, uint64_t *n_slots_out, uint32_t *slot_bits_out,
                      uint32_t *end_bit_out, uint32_t *barrier_out) const;
    int get_pairs(const WideDev &d, uint32_t *first_out, uint32_t *second_out, int32_t *count_out, uint64_t cap, uint64_t *n_out) const;
    uint32_t n_merges() const { return active ? (uint32_t)h_best.size() : 0u; }
    void merges(uint32_t *merges_out, int32_t *counts_out) const;     // n_merges() pairs (counts_out may be NULL)
    void add_stats(mbpe_stats *s) const;

private:
    int alloc_table(const WideDev &d, uint64_t want_entries);
    int regrow(const WideDev &d, uint64_t need_entries);
    int sync(const WideDev &d);
    int alloc_loop(const WideDev &d, uint64_t n_tok, uint64_t n_val, uint64_t n_init);
    int begin_limits(const WideDev &d, const WideTokens &src);
};

}  // namespace mbpe

#endif
