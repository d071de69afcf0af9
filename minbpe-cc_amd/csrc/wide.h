// The 32-bit continuation of a training (reference Token = uint32_t, Tokenizer.h:37-38): what runs once the token ids
// no longer fit the 16-bit slot stream of kernels.hip.  A training whose vocabulary lies beyond the 16-bit format runs
// its first merges on the slot stream (batch sequences, fused passes) and is then CONVERTED: the stream becomes 32-bit
// tokens with bit 31 = "last token of its chunk" (the layout of span.h), the pair table an open-addressing table
// with 64-bit keys, and the loop of Tokenizer.h:557-589 continues one merge per pass:
//
//   k_wide_argmax_*  get_top_pair_count, PairCount.h:262-269: full scan of the table under CompareLexicalOrder
//                    (:194-207: count descending, first ascending, second ascending), zero-count pairs included
//                    (create_or_modify_pair :249-260 never erases)
//   k_wide_cand      merge_incremental's match test, Tokenizer.h:231, for every position; per 1,024-token span the
//                    parity of its trailing run of candidates (a == b: `a a a` -> `X a`, the walk is greedy)
//   k_wide_match     which candidates the left-to-right walk really takes (run parity from a scan over the spans), the
//                    count updates of :239-280 as atomics on the table -- (a,b)-1, (x,a)-1, (x,X)+1, (b,y)-1, (X,y)+1
//                    with x the ALREADY-REWRITTEN left neighbour and y the not-yet-rewritten right one -- and the
//                    value every position contributes to the next stream
//   k_wide_scatter   the list erase of :237 as a compaction into the other buffer
//
// The `first` tie-break (PairCountInsertOrder, PairCount.h:55-181; the table rebuilt before every merge,
// Tokenizer.h:581-585) adds three kernels between the argmax and the merge, as kernels.hip does on the slot stream:
//
//   k_wide_first_gather  how many pairs have the maximal count M; a bitmap of their hashed keys (the slices of the
//                        table whose argmax partial is below M are skipped)
//   k_wide_first_pos     only when several do: the smallest 64-bit stream position at which one of them starts -- waves
//                        walk the 1,024-token spans in ascending order and stop at the first span beyond the best
//                        position found so far
//   k_wide_first_pick    the pair at that position replaces the lexical winner
//
// and the loop ends at M = 0 (Tokenizer.h:586-588: a rebuilt table holds no zero-count pair).
//
// A training that continues from existing merges (mbpe_train_begin_from, "resume_wide") can also START here, without
// a slot stream: the rank-ordered replay leaves this very token layout, and
//
//   k_wide_pair_count_tokens  counts its adjacent pairs into the table (LDS cache of 64-bit keys per workgroup,
//                             flushed through the concurrent insert of the merge kernels), followed by a census of
//                             the table that must add up to the positions counted
//
// CHUNK WEIGHTS (mbpe_load_corpus_weighted, mbpe_load_corpus_endmask_weighted).  A chunk's token sequence after any
// number of merges is a function of its bytes alone, so a corpus may be given as its distinct chunks with the number of
// occurrences of each (dedup.h): every pair count of the full corpus is the weight-sum over the unique chunks.  Such a
// training runs here from its first merge.  A u32 array beside the tokens holds every token's chunk weight -- filled
// at the begin from the token's rank among the end flags, carried through the compaction, a merged token keeping its
// left half's entry -- and the pair count adds w where it added 1, k_wide_match +-w on the neighbours and the sum of
// the matched weights on (a, b).  The kernels are templates on "weighted": the unweighted instantiations are the code
// they were.  ctl->matches and ctl->n stay position counts; table headroom is therefore bounded by the stream's
// positions, not by a count (a count can be 10^9 on a stream of ten tokens).
// The `first` position search needs no change: it compares table counts with the maximum M, both weighted alike, and
// looks for the earliest position in the stream it is given.  With the unique chunks in order of first occurrence that
// position decides as the full corpus would: the earliest occurrence of any pair in the full corpus lies in the first
// occurrence of its chunk (an earlier copy of the chunk would hold the pair too), so the tied pairs' first positions
// keep their order.
//
// STOPPING RULES (the options "min_frequency" and "max_token_length" of mbpe.h).  A training that began here may carry
// a WideLimits: the pairs the argmax may choose are the ELIGIBLE ones, len[a] + len[b] <= max_len with len[] the tokens'
// lengths in bytes, and the loop ends (ctl->live = 0, as on an empty table) when no pair is eligible or the largest
// eligible count lies below min_count.  Ineligible pairs stay in the stream and the table and are counted as ever.
//   len[]  one u32 per token id below the training's vocab_size, SATURATING at kWideLenMax = 2^31 - 1 (a prior merge
//          may be longer than any text; max_len is below 2^31, so a saturated token is in no eligible pair, and the
//          sum of two entries never wraps).  The host fills bytes and prior merges; the entry of id 256 + k is written
//          on the device where ctl->a, b of merge k are final: k_wide_argmax_final (lexical), k_wide_first_pick (`first`)
//   where  eligibility is decided in the scans, not at insert time.  It is a property of the key alone, but the table
//          has no room for it (64-bit keys that every probe compares, 32-bit counts whose every bit counts), and the
//          four inserts of a match would each pay two gathers.  The argmax tests a pair only once it beats the
//          thread's best so far, the gather and the position search only pairs whose count is M: a handful of 4-byte
//          gathers per thread from an array of 4 B per token id, which stays in L2 beside the 12 B per entry streamed
//   kernels are templates on "limited": the unlimited instantiations are the code they were, and a training without
//          limits launches exactly those
//
// One GPU, either tie-break.  Slower per merge than the 16-bit path (one merge per pass, ~20 B of traffic per token),
// but it turns MBPE_ERR_VOCAB into a training for GPT-4-size vocabularies.  The host side of the loop is wide_run.h.
#ifndef MBPE_WIDE_H
#define MBPE_WIDE_H

#include "span.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mbpe {

constexpr unsigned long long kWideEmpty = ~0ull;

struct WideTable {
    unsigned long long *keys;      // (first << 32) | second, kWideEmpty when free
    int32_t *cnts;
    uint32_t mask;                 // capacity - 1 (a power of two)
    uint32_t shift;                // 64 - log2(capacity)
};

// WideCtl::err
constexpr uint32_t kWideErrFull = 1u;       // the table is full
constexpr uint32_t kWideErrToken = 2u;      // the pair count met a token id that does not exist
constexpr uint32_t kWideErrCount = 4u;      // the pair count's table does not add up to the positions counted, or a
                                            //   pair occurs 2^31 times or more
constexpr uint32_t kWideErrWeight = 8u;     // a chunk weight of 0, or of 2^31 or more, or fewer weights than chunks

// census of the pair count of a resumed stream (launch_wide_pair_count_tokens)
struct WideTally { unsigned long long positions, total; uint32_t top, pad; };

struct WideCtl {
    unsigned long long n;          // tokens in the stream
    uint32_t n_entries;            // pairs ever inserted
    uint32_t err;                  // kWideErr* flags
    uint32_t k;                    // merges done by the wide loop
    uint32_t k_limit;
    uint32_t a, b;                 // the pair chosen for the merge under way
    int32_t count;
    uint32_t live;                 // 0: the table is empty (Tokenizer.h:586-588)
    uint32_t matches;              // matches of the merge under way
    uint32_t ran;                  // the merge under way got as far as its scan: its scatter has to run
    unsigned long long n_prev;     // length of the stream the merge under way read
    uint32_t first;                // 1: `first` tie-break (the argmax ends the loop at count 0)
    uint32_t pad;
};

// scratch of the `first` tie-break; pos = ~0, n_tie = 0 and the bitmap all zero between two merges
constexpr uint32_t kWideFirstBitmapWords = 2048;      // 64 Ki bits
struct WideFirst {
    unsigned long long pos;        // stream position of the earliest tied pair found so far, ~0: none
    uint32_t n_tie;                // pairs whose count is the maximum
    uint32_t pad;
    uint32_t bitmap[kWideFirstBitmapWords];
};

// stopping rules of a training (see above); all zero: none
constexpr uint32_t kWideLenMax = 0x7FFFFFFFu;
struct WideLimits {
    uint32_t *len;                 // NULL: no length limit; else the byte length of every token id, saturating
    uint32_t max_len;              // a pair is eligible iff len[a] + len[b] <= max_len
    int32_t min_count;             // the loop ends when the largest eligible count is below this
    uint32_t new_id_base;          // len[new_id_base + ctl->k] receives the length of the merge under way
};

// best[k] of the wide loop: count, first, second
struct WideBest { int32_t count; uint32_t first, second, pad; };

size_t wide_scratch_words(uint64_t n_tokens);   // u32 words of span scratch for a stream of n_tokens

// 16-bit slot stream (no holes among the first n_live slots: compact first) -> 32-bit tokens.  barrier: the slot
// value that follows the last token of a chunk (mbpe_dev.h kBarrier), or 0xFFFFFFFF when there is none; endbit: the
// slot bit that marks the last token of a chunk (kEndBit), or 0.  With neither the corpus is one chunk.
// val: n_live words of scratch.  The new length goes to ctl->n.
void launch_wide_from_slots(hipStream_t s, const uint16_t *slots, uint64_t n_live, uint32_t barrier, uint32_t endbit,
                            uint32_t *val, uint32_t *span_scratch, uint32_t *tok_out, WideCtl *ctl);
// hashed 16-bit-key pair table (ekey = first << 16 | second) -> wide table
void launch_wide_table_from16(hipStream_t s, const uint32_t *ekey, const int32_t *ecnt, uint32_t n_entries, WideTable t,
                              WideCtl *ctl);
void launch_wide_table_clear(hipStream_t s, WideTable t);
void launch_wide_rehash(hipStream_t s, WideTable from, WideTable to, WideCtl *ctl);
// A stream that starts as 32-bit tokens (a training continued from existing merges, no slot stream): the count of its
// adjacent pairs into the cleared table t -- k_wide_pair_count_tokens, the 64-bit-key counterpart of
// k_pair_count_tokens -- then the table's census and its check against the positions counted.  tok: n_tok flagged
// tokens; ids: the token ids that exist (kWideErrToken for one beyond them).  tally: zeroed by the caller.
// wt: NULL, or the tokens' weights (launch_wide_token_weights): a position counts that often, and the census compares
// the table with the 64-bit sum of the weights counted.
void launch_wide_pair_count_tokens(hipStream_t s, const uint32_t *tok, const uint32_t *wt, uint64_t n_tok, uint32_t ids,
                                   WideTable t, WideCtl *ctl, WideTally *tally, int n_cus);
// wt[i] = weights[number of end flags before token i], for the n_tok flagged tokens of tok; weights: n_weights u32 on
// the device.  kWideErrWeight for a chunk without a weight and for a weight outside 1 .. 2^31 - 1.
void launch_wide_token_weights(hipStream_t s, const uint32_t *tok, uint64_t n_tok, const uint32_t *weights,
                               uint64_t n_weights, uint32_t *wt, uint32_t *span_scratch, WideCtl *ctl);
// flag[0] |= 1 when one of the n device weights lies outside 1 .. 2^31 - 1
void launch_wide_check_weights(hipStream_t s, const uint32_t *weights, uint64_t n, uint32_t *flag);
// argmax -> ctl->a, b, count, live and best[ctl->k]; clears ctl->ran.  lim: the stopping rules (all zero: none)
void launch_wide_argmax(hipStream_t s, WideTable t, WideCtl *ctl, WideBest *best, unsigned long long *scratch /* 3 * 1024 */,
                        WideLimits lim = WideLimits{});
// `first` mode, after launch_wide_argmax (same scratch): among the pairs of the maximal count the one whose first
// occurrence in the stream src (ctl->n tokens, at most n_upper) comes first replaces ctl->a, b and best[ctl->k].
// lim: what launch_wide_argmax was given
void launch_wide_first(hipStream_t s, const uint32_t *src, uint64_t n_upper, WideTable t, WideCtl *ctl, WideBest *best,
                       const unsigned long long *scratch, WideFirst *fs, WideLimits lim = WideLimits{});
// one merge (ctl->a, ctl->b) -> new_id_base + ctl->k over the stream src (ctl->n tokens, at most n_upper) into dst;
// advances ctl->k, sets ctl->n.  Does nothing when ctl->k >= ctl->k_limit or the table is empty.
// wsrc / wdst: NULL, or the weights of the tokens of src and the array that receives those of dst.
void launch_wide_merge(hipStream_t s, const uint32_t *src, uint32_t *dst, uint64_t n_upper, uint32_t *val,
                       uint32_t *span_scratch, WideTable t, WideCtl *ctl, uint32_t new_id_base, const uint32_t *wsrc = nullptr,
                       uint32_t *wdst = nullptr);

}  // namespace mbpe

#endif
