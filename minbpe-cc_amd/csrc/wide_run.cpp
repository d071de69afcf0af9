// The 32-bit training loop's host code (wide_run.h) over the kernels of wide.hip.
#include "wide_run.h"
#include "hip_host.h"
#include "train_plan.h"

#include <algorithm>

namespace mbpe {

#define HIPCHK(expr) MBPE_HIP_CHECK(expr, false)

void WideRun::release(DevPool &pool) {
    pool.free(tok[0]); pool.free(tok[1]); pool.free(val); pool.free(scratch); pool.free(wt[0]); pool.free(wt[1]);
    pool.free(tab.keys); pool.free(tab.cnts); pool.free(ctl); pool.free(best); pool.free(arg);
    pool.free(fs); pool.free(tally); pool.free(lim.len);
    *this = WideRun{};
}

int WideRun::alloc_table(const WideDev &d, uint64_t want_entries) {
    uint32_t bits;
    if (!table_bits(want_entries, &bits)) return fail(MBPE_ERR_OVERFLOW, "pair table beyond 2^30 entries");
    tab = {};
    tab.mask = (uint32_t)((1ull << bits) - 1);
    tab.shift = 64 - bits;
    HIPCHK(d.pool.alloc(&tab.keys, (size_t)8 << bits));
    HIPCHK(d.pool.alloc(&tab.cnts, (size_t)4 << bits));
    launch_wide_table_clear(d.stream, tab);
    return MBPE_OK;
}

// The table replaced by one for need_entries pairs: every entry rehashed, the old arrays gone for good.  Waits for the
// rehash, so a table it fills is reported here.
int WideRun::regrow(const WideDev &d, uint64_t need_entries) {
    const WideTable old = tab;
    int rc = alloc_table(d, need_entries);
    if (rc != MBPE_OK) return rc;
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&ctl->n_entries), 0, 1, d.stream));
    launch_wide_rehash(d.stream, old, tab, ctl);
    rc = sync(d);
    d.pool.release(old.keys); d.pool.release(old.cnts);
    return rc;
}

int WideRun::sync(const WideDev &d) {
    HIPCHK(hipMemcpyAsync(&h_ctl, ctl, sizeof(WideCtl), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(hipStreamSynchronize(d.stream));
    HIPCHK(hipGetLastError());
    if (h_ctl.err & kWideErrFull) return fail(MBPE_ERR_OVERFLOW, "device error: the 32-bit pair table is full");
    if (h_ctl.err & kWideErrWeight)
        return fail(MBPE_ERR_ARG, "device error: a chunk weight is 0, or 2^31 or more, or the stream has more chunks than weights");
    if (h_ctl.err)
        return fail(MBPE_ERR_OVERFLOW, h_ctl.err & kWideErrToken
                                           ? "device error: the replayed stream holds a token id that no prior merge made"
                                           : "device error: a pair occurs 2^31 times or more, or the pair counts do not add up "
                                             "to the pairs scanned");
    return MBPE_OK;
}

// The buffers of the loop for a stream of at most n_tok tokens (n_val: positions the value array holds, the slot
// stream's barriers included at a conversion) and its control block, with n_init tokens in the stream already.  Every
// begin starts from a released WideRun: no merge made, buffer 0 live.
int WideRun::alloc_loop(const WideDev &d, uint64_t n_tok, uint64_t n_val, uint64_t n_init) {
    if (!tok[0]) HIPCHK(d.pool.alloc(&tok[0], std::max<uint64_t>(n_tok, 1) * 4));      // (begin_from: there already)
    HIPCHK(d.pool.alloc(&tok[1], std::max<uint64_t>(n_tok, 1) * 4));
    HIPCHK(d.pool.alloc(&val, std::max<uint64_t>(n_val, 1) * 4));
    HIPCHK(d.pool.alloc(&scratch, wide_scratch_words(n_val) * 4));
    HIPCHK(d.pool.alloc(&ctl, sizeof(WideCtl)));
    HIPCHK(d.pool.alloc(&best, ((size_t)goal.n_wide + 2) * sizeof(WideBest)));
    HIPCHK(d.pool.alloc(&arg, 2 * 1024 * 8));
    h_ctl = WideCtl{};
    h_ctl.n = n_init;
    h_ctl.first = goal.first ? 1u : 0u;
    HIPCHK(hipMemcpyAsync(ctl, &h_ctl, sizeof(WideCtl), hipMemcpyHostToDevice, d.stream));
    if (goal.first) {
        HIPCHK(d.pool.alloc(&fs, sizeof(WideFirst)));
        HIPCHK(hipMemsetAsync(fs, 0, sizeof(WideFirst), d.stream));
        HIPCHK(hipMemsetAsync(&fs->pos, 0xFF, sizeof(fs->pos), d.stream));
    }
    return MBPE_OK;
}

// slot stream + hashed pair table of the 16-bit part -> 32-bit tokens + 64-bit-key table.  From here on the training's
// stream, table and merge counter live here; the caller gives the 16-bit buffers back to the pool.
int WideRun::convert(const WideDev &d, const WideSlots &src, const WideGoal &g) {
    goal = g;
    const uint64_t n_tok = src.n_slots - src.n_barriers;
    int rc = alloc_loop(d, n_tok, src.n_slots, 0);
    if (rc != MBPE_OK) return rc;
    launch_wide_from_slots(d.stream, src.slots, src.n_slots, src.barrier, src.endbit, val, scratch, tok[0], ctl);
    top0 = src.top == ~0ull ? n_tok : src.top;
    rc = alloc_table(d, (uint64_t)src.n_entries + wide_headroom(top0, n_tok, 16));
    if (rc != MBPE_OK) return rc;
    launch_wide_table_from16(d.stream, src.ekey, src.ecnt, src.n_entries, tab, ctl);
    rc = sync(d);
    if (rc != MBPE_OK) return rc;
    if (h_ctl.n != n_tok || h_ctl.n_entries != src.n_entries)
        return fail(MBPE_ERR_OVERFLOW, "conversion to 32-bit tokens lost tokens or pairs");
    n_upper = n_tok;
    active = true;
    return MBPE_OK;
}

// The stopping rules of the training that begins (wide.h): the options as they stand, and for a length limit the
// lengths of the bytes and of the prior merges -- which count, whatever their length; the limits apply to the new
// merges only.  The entries of the new tokens are written by the loop.
int WideRun::begin_limits(const WideDev &d, const WideTokens &src) {
    lim.min_count = (int32_t)src.min_frequency;
    lim.new_id_base = goal.new_id_base;
    if (!src.max_token_length) return MBPE_OK;
    std::vector<uint32_t> len((size_t)src.vocab_total, 0u);
    for (uint32_t i = 0; i < 256 && i < src.vocab_total; ++i) len[i] = 1;
    for (uint32_t m = 0; m < src.n_prior; ++m)      // (mbpe_merges_check: both halves exist before merge m)
        len[256 + m] = (uint32_t)std::min<uint64_t>((uint64_t)len[src.prior[2 * m]] + len[src.prior[2 * m + 1]], kWideLenMax);
    HIPCHK(d.pool.alloc(&lim.len, len.size() * 4));
    HIPCHK(hipMemcpyAsync(lim.len, len.data(), len.size() * 4, hipMemcpyHostToDevice, d.stream));
    HIPCHK(hipStreamSynchronize(d.stream));
    lim.max_len = (uint32_t)src.max_token_length;
    return MBPE_OK;
}

// A training that begins on 32-bit tokens: the replay's tokens ARE the stream, the 64-bit-key table is counted from
// them, and the loop runs from merge n_prior.  The table is allocated before the count for the most distinct pairs the
// stream can hold (wide_add inserts concurrently: no bins, no census) and replaced by one of the right size once the
// count is known.  stats.ms_begin: the device time from here on plus the replay's.
int WideRun::begin_from(const WideDev &d, const WideTokens &src, const WideGoal &g) {
    goal = g;
    const uint64_t n_tok = src.n_tok;
    HIPCHK(hipEventRecord(d.ev0, d.stream));
    // the stream first, so that the replay's n_bytes x 4 array is gone before anything else is allocated
    HIPCHK(d.pool.alloc(&tok[0], std::max<uint64_t>(n_tok, 1) * 4));
    if (n_tok) HIPCHK(hipMemcpyAsync(tok[0], *src.tok, n_tok * 4, hipMemcpyDeviceToDevice, d.stream));
    HIPCHK(hipStreamSynchronize(d.stream));
    (void)hipFree(*src.tok);
    *src.tok = nullptr;
    int rc = alloc_loop(d, n_tok, n_tok, n_tok);
    if (rc != MBPE_OK) return rc;
    HIPCHK(d.pool.alloc(&tally, sizeof(WideTally)));
    HIPCHK(hipMemsetAsync(tally, 0, sizeof(WideTally), d.stream));
    if (src.weights) {
        HIPCHK(d.pool.alloc(&wt[0], std::max<uint64_t>(n_tok, 1) * 4));
        HIPCHK(d.pool.alloc(&wt[1], std::max<uint64_t>(n_tok, 1) * 4));
        launch_wide_token_weights(d.stream, tok[0], n_tok, src.weights, src.n_weights, wt[0], scratch, ctl);
    }
    if (src.min_frequency || src.max_token_length) {
        rc = begin_limits(d, src);
        if (rc != MBPE_OK) return rc;
    }
    const uint64_t ids = goal.new_id_base;
    const uint64_t most = std::min<uint64_t>({n_tok ? n_tok - 1 : 0, ids * ids, 1ull << 30});
    rc = alloc_table(d, std::max<uint64_t>(most, 1));
    if (rc != MBPE_OK) return rc;
    launch_wide_pair_count_tokens(d.stream, tok[0], wt[0], n_tok, (uint32_t)ids, tab, ctl, tally, d.n_cus);
    WideTally h = {};
    HIPCHK(hipMemcpyAsync(&h, tally, sizeof(h), hipMemcpyDeviceToHost, d.stream));
    rc = sync(d);
    if (rc != MBPE_OK) return rc;
    // the right size: the pairs there are plus what the first group of merges can add, at load factor 1/2
    const uint64_t need = (uint64_t)h_ctl.n_entries + wide_headroom(h.top, n_tok, 16);
    uint32_t bits;
    (void)table_bits(need, &bits);       // (beyond 2^30 entries: regrow refuses, unless the table has 2^31 slots already)
    if ((uint64_t)tab.mask + 1 != (1ull << bits)) {
        rc = regrow(d, need);
        if (rc != MBPE_OK) return rc;
    }
    HIPCHK(hipEventRecord(d.ev1, d.stream));
    HIPCHK(hipEventSynchronize(d.ev1));
    HIPCHK(hipEventElapsedTime(&d.stats.ms_begin, d.ev0, d.ev1));
    d.stats.ms_begin += src.ms_replay;
    d.stats.ms_steps = 0;
    n_upper = n_tok;
    top0 = h.top;
    active = true;
    return MBPE_OK;
}

int WideRun::steps(const WideDev &d, uint32_t n_steps, uint32_t *done_out) {
    *done_out = 0;
    const uint32_t n_wide = goal.n_wide;
    uint32_t done = 0;
    unsigned long long top = h_best.empty() ? top0 : (unsigned long long)h_best.back().count;
    while (done < n_steps && k < n_wide) {
        const uint32_t group = std::min<uint32_t>({16u, n_steps - done, n_wide - k});
        // room for what this group can insert (load factor 1/2 at most)
        const uint64_t need = (uint64_t)h_ctl.n_entries + wide_headroom(top, n_upper, group);
        if (2 * need > (uint64_t)tab.mask + 1) {
            const int rc = regrow(d, 2 * need);
            if (rc != MBPE_OK) return rc;
            d.stats.n_table_grows++;
        }
        HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&ctl->k_limit), (int)(k + group), 1, d.stream));
        HIPCHK(hipEventRecord(d.ev0, d.stream));
        for (uint32_t g = 0; g < group; ++g) {
            const int src = cur ^ (int)(g & 1), dst = src ^ 1;
            launch_wide_argmax(d.stream, tab, ctl, best, arg, lim);
            if (goal.first) launch_wide_first(d.stream, tok[src], n_upper, tab, ctl, best, arg, fs, lim);
            launch_wide_merge(d.stream, tok[src], tok[dst], n_upper, val, scratch, tab, ctl, goal.new_id_base, wt[src], wt[dst]);
        }
        HIPCHK(hipEventRecord(d.ev1, d.stream));
        const int rc = sync(d);
        if (rc != MBPE_OK) return rc;
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, d.ev0, d.ev1));
        d.stats.ms_steps += ms;
        const uint32_t ran = h_ctl.k - k;
        // empty table (Tokenizer.h:586-588): cannot happen after a 16-bit part that merged -- except in `first` mode, where
        // it means no pair is left: the loop ends there, with fewer merges than the vocabulary asks for
        if (ran == 0) break;
        h_best.resize((size_t)k + ran);
        HIPCHK(hipMemcpy(h_best.data() + k, best + k, (size_t)ran * sizeof(WideBest), hipMemcpyDeviceToHost));
        cur ^= (int)(ran & 1u);
        n_upper = h_ctl.n;
        k += ran;
        done += ran;
        top = (unsigned long long)std::max(0, h_best.back().count);
        if (!goal.first && h_best.back().count == 0 && done < n_steps && k < n_wide) {
            // The best pair no longer occurs anywhere: merging it changes nothing, the reference chooses it again and
            // again (never-erased table, PairCount.h:249-260; the loop only ends on an empty table, Tokenizer.h:586-588)
            const uint32_t fill = std::min<uint32_t>(n_steps - done, n_wide - k);
            h_best.resize((size_t)k + fill, h_best.back());
            k += fill;
            done += fill;
            HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&ctl->k), (int)k, 1, d.stream));
            HIPCHK(hipStreamSynchronize(d.stream));
            h_ctl.k = k;
        }
        if (ran < group) break;
    }
    *done_out = done;
    return MBPE_OK;
}

int WideRun::get_stream(bool chunked, uint32_t *tokens_out, uint8_t *chunk_end_out, uint64_t cap, uint64_t *n_out) const {
    const uint64_t n = h_ctl.n;
    *n_out = n;
    if (!tokens_out) return MBPE_OK;
    if (cap < n) return fail(MBPE_ERR_ARG, "tokens_out too small");
    if (n) HIPCHK(hipMemcpy(tokens_out, tok[cur], n * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; ++i) {
        // (a one-chunk corpus reports no chunk ends, like the slot stream)
        if (chunk_end_out) chunk_end_out[i] = chunked ? (uint8_t)(tokens_out[i] >> 31) : 0;
        tokens_out[i] &= kTokIdMask;
    }
    return MBPE_OK;
}

int WideRun::stream_device(const WideDev &d, const void **slots_out, uint64_t *n_slots_out, uint32_t *slot_bits_out,
                           uint32_t *end_bit_out, uint32_t *barrier_out) const {
    HIPCHK(hipStreamSynchronize(d.stream));
    *slots_out = tok[cur];
    *n_slots_out = h_ctl.n;
    if (slot_bits_out) *slot_bits_out = 32;
    if (end_bit_out) *end_bit_out = kTokEnd;
    if (barrier_out) *barrier_out = MBPE_NO_BARRIER;
    return MBPE_OK;
}

int WideRun::get_pairs(const WideDev &d, uint32_t *first_out, uint32_t *second_out, int32_t *count_out, uint64_t cap,
                       uint64_t *n_out) const {
    HIPCHK(hipStreamSynchronize(d.stream));
    const uint64_t n = h_ctl.n_entries, slots = (uint64_t)tab.mask + 1;
    *n_out = n;
    if (!first_out) return MBPE_OK;
    if (cap < n) return fail(MBPE_ERR_ARG, "pair arrays too small");
    std::vector<unsigned long long> keys(slots);
    std::vector<int32_t> cnts(slots);
    HIPCHK(hipMemcpy(keys.data(), tab.keys, slots * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cnts.data(), tab.cnts, slots * 4, hipMemcpyDeviceToHost));
    uint64_t o = 0;
    for (uint64_t i = 0; i < slots; ++i) {
        if (keys[i] == kWideEmpty) continue;
        if (o >= n) return fail(MBPE_ERR_OVERFLOW, "pair table holds more pairs than counted");
        first_out[o] = (uint32_t)(keys[i] >> 32);
        second_out[o] = (uint32_t)keys[i];
        if (count_out) count_out[o] = cnts[i];
        ++o;
    }
    if (o != n) return fail(MBPE_ERR_OVERFLOW, "pair table holds fewer pairs than counted");
    return MBPE_OK;
}

void WideRun::merges(uint32_t *merges_out, int32_t *counts_out) const {
    for (uint32_t i = 0; i < n_merges(); ++i) {
        merges_out[2 * i] = h_best[i].first;
        merges_out[2 * i + 1] = h_best[i].second;
        if (counts_out) counts_out[i] = h_best[i].count;
    }
}

// the stream and the table are the 32-bit ones now
void WideRun::add_stats(mbpe_stats *s) const {
    s->n_slots = h_ctl.n;
    s->n_live = h_ctl.n;
    s->n_merges += (uint32_t)h_best.size();
    s->n_pairs = h_ctl.n_entries;
    s->n_batches += k;            // (one stream pass per merge)
}

}  // namespace mbpe
